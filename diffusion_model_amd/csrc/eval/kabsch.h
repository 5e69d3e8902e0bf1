// Launch constants and the partial-result record of the RMSD evaluation kernels (kabsch.hip).
#pragma once
#include <stdint.h>

#include "../../../include/egnn_amd.h"
#include "kabsch_math.h"

namespace egnn {

static_assert(kKabschCentroid == EGNN_KABSCH_CENTROID && kKabschFirst == EGNN_KABSCH_FIRST, "center codes");
static_assert(kKabschFlipRow == EGNN_KABSCH_FLIP_ROW && kKabschFlipColumn == EGNN_KABSCH_FLIP_COLUMN, "flip codes");

constexpr int kKabschOutStride = 16;   // floats per graph of egnn_kabsch's output: R [9], t [3], rmsd, two counts, 0
constexpr int kPermMaxAtoms = 12;      // 11! = 39,916,800 orderings fit 32-bit ranks; the table is 12 * 12 * 72 B = 10.4 KB of LDS
constexpr int kPermThreads = 256;

// what one workgroup of the search leaves for the final reduction
struct PermPartial {
  double score;     // trace of the optimal proper rotation of the best ordering of the workgroup's ranks (-1: none)
  uint32_t rank;    // its lexicographic rank among the (n-1)! orderings
  uint32_t pad;
};
static_assert(sizeof(PermPartial) == 16, "partial layout");

}  // namespace egnn

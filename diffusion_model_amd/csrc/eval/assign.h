// Launch constants of the batched linear-assignment solver and of its pre-alignment (assign.hip).
//
// TIE RULE.  The solver augments the rows in index order 0, 1, ..., n-1.  Inside one augmentation the column that leaves the
// frontier is the one with the smallest path cost; EQUAL path costs go to the LOWEST column index.  Nothing else is left to
// chance (no atomics, fixed reduction trees), so the assignment, its cost and the duals are bitwise reproducible and do not
// depend on where in the batch a graph sits or on what else the launch holds.  Where the optimum is unique this is
// scipy.optimize.linear_sum_assignment's answer; where several assignments share the optimal cost it is one of them, not
// necessarily scipy's (which prefers an unassigned column among equal path costs and scans the columns in its own order).
#pragma once
#include <stdint.h>

#include "../../../include/egnn_amd.h"
#include "assign_host.h"

namespace egnn {

constexpr int kAssignMaxAtoms = 1024;   // C3 of BASELINE is 512 atoms
constexpr int kAssignWaveAtoms = 64;    // up to here one wavefront solves a graph, one lane per column
constexpr int kAssignThreads = 256;     // workgroup of the larger graphs: each thread owns kAssignCols columns, in registers
constexpr int kAssignCols = kAssignMaxAtoms / kAssignThreads;
static_assert(kAssignMaxAtoms == EGNN_ASSIGN_MAX_ATOMS, "limit in the public header");
static_assert(kAssignCols * kAssignThreads == kAssignMaxAtoms && kAssignThreads % 64 == 0, "column ownership");

// LDS of one workgroup for graphs of up to cap atoms: row coordinates (3 floats), row duals (double), row4col, col4row and the
// predecessor of every column (3 ints), plus two buffers of per-wave (value, index) partials: 32 B per atom -> 32 KB + 128 B at
// 1,024 atoms of the 160 KB a CU has.  The column side (coordinates, duals, path costs) lives in registers.
constexpr int kAssignWaves = kAssignThreads / 64;
inline size_t assign_lds_bytes(int cap) { return (size_t)cap * 32u + 2u * kAssignWaves * 16u; }

}  // namespace egnn

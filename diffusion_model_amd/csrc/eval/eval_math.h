// What the definition headers of the evaluation families (eval/*_math.h, cells/cell_math.h) share: the host/device macro their
// functions stand behind, and the two definitions more than one family uses.  Plain C++, so that kernels and host statements read
// the same text.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define EGNN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define EGNN_HD inline
#endif

namespace egnn {

// number of unordered pairs of A types (or classes) and the index of (b, c), in either order
EGNN_HD int type_pairs(int A) { return A * (A + 1) / 2; }
EGNN_HD int type_pair_index(int b, int c, int A) {
  const int lo = b < c ? b : c, hi = b < c ? c : b;
  return lo * A - lo * (lo - 1) / 2 + (hi - lo);
}

// fp64 distance from float32 positions, in exactly this order: dx = (double)q.x - (double)p.x, d = sqrt((dx*dx + dy*dy) + dz*dz).
// The difference of two float32 values is exact in fp64, so d(p, q) == d(q, p) bitwise.
EGNN_HD double distance64(float px, float py, float pz, float qx, float qy, float qz) {
  const double dx = (double)qx - (double)px, dy = (double)qy - (double)py, dz = (double)qz - (double)pz;
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

}  // namespace egnn

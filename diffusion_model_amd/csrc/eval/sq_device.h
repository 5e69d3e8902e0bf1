// The reader of one (h, k) row of a cell's index box, shared by the kernels that walk the reciprocal vectors of periodic cells
// (sq.hip, cells/cell_ewald.hip).  Device only, on top of eval_device.h; the arithmetic is sq_math.h.
#pragma once
#include "eval_device.h"
#include "sq_math.h"

namespace egnn {

// plan [C, 4] = {H, K, L, first row}: the index box of a cell and where its (h, k) rows start in the row arrays
struct SqRow {
  int h, k, Lb, row;
  double Bm[9];
};

__device__ __forceinline__ bool sq_row_read(const int* __restrict__ plan, const double* __restrict__ lattice, int c, int local, int n_rows,
                                            SqRow* R) {
  const int H = plan[4 * c], K = plan[4 * c + 1];
  R->Lb = plan[4 * c + 2];
  if (H < 0 || H > kSqMaxIndex || K < 0 || K > kSqMaxIndex || R->Lb < 0 || R->Lb > kSqMaxIndex) return false;
  if (local >= sq_box_rows(H, K)) return false;
  R->row = plan[4 * c + 3] + local;
  if (plan[4 * c + 3] < 0 || R->row < 0 || R->row >= n_rows) return false;
  R->h = local / (2 * K + 1);
  R->k = local % (2 * K + 1) - K;
  double L[9];
  for (int t = 0; t < 9; ++t) L[t] = lattice[9 * (size_t)c + t];
  return sq_reciprocal(L, R->Bm);
}

}  // namespace egnn

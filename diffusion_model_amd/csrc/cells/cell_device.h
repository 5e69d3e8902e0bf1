// What the kernels of the periodic-cell families (cell_env.hip, cell_stats.hip, cell_grid.hip, cell_soap.hip, cell_boo.hip) share:
// the readers that guard every index of a batch of cells before it is used -- the cell of an atom, the atoms of a cell, a
// {cell, first centre} tile, a CSR row, the row of a listed centre -- and the staging of a chunk's wrapped coordinates in LDS.
// Device only, on top of eval/eval_device.h.  The arithmetic is cell_math.h: the wrap (cell_wrapped_read), the test of a list entry
// (cell_site_listed) and the vector of a listed site (cell_listed_site_vector) live there, behind the host/device macro, because
// the host statements and cell_boo_math.h compile them too.
//
// A reader trusts nothing: it returns false, and its caller writes nothing, where an index or a range does not fit the extents.
#pragma once
#include "../eval/eval_device.h"
#include "cell_math.h"

namespace egnn {

// the atoms [lo, lo + n) of cell c; false unless c lies in [0, C) and cell_ptr gives a range inside [0, N]
__device__ __forceinline__ bool cell_read(int c, const int* __restrict__ cell_ptr, int C, int N, int* lo, int* n) {
  if (c < 0 || c >= C) return false;
  const int a = cell_ptr[c], b = cell_ptr[c + 1];
  if (a < 0 || b < a || b > N) return false;
  *lo = a;
  *n = b - a;
  return true;
}

// the cell of batch atom i: the last c with cell_ptr[c] <= i; false unless the cell's range is sane and holds i
__device__ __forceinline__ bool cell_of_atom(const int* __restrict__ cell_ptr, int C, int N, int i, int* cell, int* lo, int* hi) {
  if (i < 0 || i >= N) return false;
  int a = 0, b = C;   // cell_ptr[a] <= i < cell_ptr[b] is the aim
  while (b - a > 1) {
    const int mid = (a + b) / 2;
    if (cell_ptr[mid] <= i) a = mid; else b = mid;
  }
  *cell = a;
  *lo = cell_ptr[a];
  *hi = cell_ptr[a + 1];
  return *lo >= 0 && *hi <= N && i >= *lo && i < *hi && *hi - *lo <= kCellMaxAtoms;
}

// tile {cell, first centre} (the first two entries of a work-list row) of a block of kCentres centres: the cell's atoms
// [lo, lo + n) and the nc centres lo + c0 .. lo + c0 + nc - 1 that are left of it; false unless the block starts inside the cell
struct CellTile {
  int c, c0, lo, n, nc;
};

// the nc centres of the block of kCentres that starts at centre c0 of a cell of n atoms; false unless it starts inside the cell
template <int kCentres>
__device__ __forceinline__ bool cell_block_read(int c0, int n, int* nc) {
  if (c0 < 0 || c0 >= n) return false;
  *nc = min(kCentres, n - c0);
  return true;
}

template <int kCentres>
__device__ __forceinline__ bool cell_tile_read(const int* __restrict__ tile, const int* __restrict__ cell_ptr, int C, int N, CellTile* T) {
  T->c = tile[0];
  T->c0 = tile[1];
  return cell_read(T->c, cell_ptr, C, N, &T->lo, &T->n) && cell_block_read<kCentres>(T->c0, T->n, &T->nc);
}

__device__ __forceinline__ void cell_lattice_read(const double* __restrict__ lattice, int c, double* L) {
  for (int k = 0; k < 9; ++k) L[k] = lattice[9 * (size_t)c + k];
}

// stages atoms first .. first + nj - 1 in LDS by the 256 threads of a workgroup: wrapped coordinates, one array per axis (64
// consecutive lanes read 64 consecutive doubles), and, where s_type is given, the types.  The caller places the barriers.
template <int kChunk>
__device__ __forceinline__ void cell_chunk_stage(const double* __restrict__ frac, const int* __restrict__ type, int first, int nj, int tid,
                                                 double (*s_w)[kChunk], int* s_type) {
  for (int t = tid; t < 3 * nj; t += 256) {
    const int a = t / 3, k = t - 3 * a;
    s_w[k][a] = cell_wrap(frac[3 * (size_t)first + t]);
  }
  if (s_type)
    for (int t = tid; t < nj; t += 256) s_type[t] = type[first + t];
}

// the entries [e0, e1) of row r of a CSR of n_rows rows over `extent` entries; false where r is no row or row_ptr is not what a
// prefix sum inside the extent gives
__device__ __forceinline__ bool cell_row_read(const int* __restrict__ row_ptr, int n_rows, int extent, int r, int* e0, int* e1) {
  if (r < 0 || r >= n_rows) return false;
  *e0 = row_ptr[r];
  *e1 = row_ptr[r + 1];
  return *e0 >= 0 && *e1 >= *e0 && *e1 <= extent;
}

// what a kernel over listed centres reads of centre m: the atom, its cell c and the cell's atoms [lo, hi), and the entries
// [e0, e1) of row centre_row[m] of the site CSR; false: no such atom or no such row
struct CellCentreRow {
  int i, c, lo, hi, e0, e1;
};

__device__ __forceinline__ bool cell_centre_row_read(const int* __restrict__ cell_ptr, int C, int N, const int* __restrict__ row_ptr, int n_rows,
                                                     int T, const int* __restrict__ centre_atom, const int* __restrict__ centre_row, int m,
                                                     CellCentreRow* R) {
  R->i = centre_atom[m];
  if (!cell_of_atom(cell_ptr, C, N, R->i, &R->c, &R->lo, &R->hi)) return false;
  return cell_row_read(row_ptr, n_rows, T, centre_row[m], &R->e0, &R->e1);
}

}  // namespace egnn

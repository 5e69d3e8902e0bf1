// Host-only argument validation that the periodic-cell families share (cell_env.hip, cell_stats.hip, cell_grid.hip, cell_soap.hip,
// cell_boo.hip and their *_host.cpp), and the host statement egnn_cell_env_host.  Plain C++ beside host_logic: it is also compiled
// into the CPU-only sanitizer library (make asan).
#pragma once
#include <math.h>

#include "../eval/eval_host.h"
#include "cell_math.h"

namespace egnn {

// every check returns EGNN_OK or EGNN_EINVAL with the message set; nothing is launched before they pass.

// what a family asks of the perpendicular widths w of cell c (lattice L, regular) at its radius `reach`
typedef int (*CellWidthRule)(const char* who, int c, const double* L, const double* w, double reach);

// The one check of a batch behind every entry.  cell_ptr and lattice are HOST arrays: cell_ptr runs from 0 to N, does not decrease
// and no cell holds more than kCellMaxAtoms atoms; every lattice is regular (a singular one is refused, naming the cell) and
// passes `rule` where one is given.  lattice may be null where an entry reads no lattice.
int cell_batch_core_check(const char* who, int C, int N, const int32_t* cell_ptr, const double* lattice, CellWidthRule rule, double reach);

// the batch of an entry that walks 27 images: cutoff positive and finite, every perpendicular width >= cutoff
int cell_batch_check(const char* who, int C, int N, const int32_t* cell_ptr, const double* lattice, double cutoff);
int cell_env_params_check(const char* who, int M, int shells, int max_atoms, const void* centre_cell, const void* centre);

// The small ones are inline, as the checks of eval_host.h are.

// what the host statements ask of their inputs beyond the batch: frac finite; type (where given) in [0, A); centre_atom (M > 0)
// inside [0, N) -- in this order
inline int cell_frac_finite_check(const char* who, const double* frac, int begin, int end) {   // atoms [begin, end), as type_range_check
  for (size_t t = 3 * (size_t)begin; t < 3 * (size_t)end; ++t)
    if (!(fabs(frac[t]) < 1e15)) { set_error("%s: atom %d has a fractional coordinate that is not finite", who, (int)(t / 3)); return EGNN_EINVAL; }
  return EGNN_OK;
}

inline int cell_inputs_check(const char* who, int N, const double* frac, const int32_t* type, int A, int M, const int32_t* centre_atom) {
  if (int rc = cell_frac_finite_check(who, frac, 0, N)) return rc;
  if (type)
    if (int rc = type_range_check(who, type, 0, N, A)) return rc;
  for (int m = 0; m < M; ++m)
    if (centre_atom[m] < 0 || centre_atom[m] >= N) {
      set_error("%s: centre %d is atom %d outside [0, %d)", who, m, centre_atom[m], N);
      return EGNN_EINVAL;
    }
  return EGNN_OK;
}

// w[3 N] = the wrapped coordinates of the batch; EGNN_ENOMEM where w could not be allocated
inline int cell_wrap_batch(const char* who, int N, const double* frac, Scratch<double>& w) {
  if (!w.p) { set_error("%s: out of memory", who); return EGNN_ENOMEM; }
  for (size_t t = 0; t < 3 * (size_t)N; ++t) w[t] = cell_wrap(frac[t]);
  return EGNN_OK;
}

// the cell of batch atom i of a checked batch: the last c with cell_ptr[c] <= i (empty cells skipped)
inline int cell_of_atom_host(const int32_t* cell_ptr, int C, int i) {
  int a = 0, b = C;   // cell_ptr[a] <= i < cell_ptr[b]
  while (b - a > 1) {
    const int mid = (a + b) / 2;
    if (cell_ptr[mid] <= i) a = mid; else b = mid;
  }
  return a;
}

// the device arrays of an entry over the rows of a site CSR (egnn_cell_soap_descriptor, egnn_cell_boo_*): all given, n_rows >= 0
// rows of T >= 0 sites, M >= 1 centres.  false: the entry names them in its own message
inline bool cell_rows_given(const void* d_cell_ptr, const void* d_lattice, const void* d_frac, const void* d_type, int n_rows, const void* d_row_ptr,
                            int T, const void* d_site_atom, const void* d_site_shift, int M, const void* d_centre_atom, const void* d_centre_row) {
  return d_cell_ptr && d_lattice && d_frac && d_type && n_rows >= 0 && d_row_ptr && T >= 0 && (T == 0 || (d_site_atom && d_site_shift)) && M >= 1 &&
         d_centre_atom && d_centre_row;
}

// the bonds of atom i of the cell [lo, hi) among 27 images, ascending by (atom, shift code), on wrapped coordinates w; reach_k =
// cutoff (1 + 1e-6) / w_k is the axis cull of the bond kernel, c2 = cutoff^2.  -> the number of bonds; atom / code hold up to
// 27 (hi - lo) entries.
// Inline: it is the inner loop of two host statements.
inline int cell_row_bonds(const double* w, const double* L, const double* reach, int lo, int hi, int i, double c2, int32_t* atom, int32_t* code) {
  int n = 0;
  const double* wi = w + 3 * (size_t)i;
  for (int j = lo; j < hi; ++j) {
    const double* wj = w + 3 * (size_t)j;
    for (int sx = -1; sx <= 1; ++sx) {
      if (!(fabs(cell_delta(wj[0], wi[0], sx)) < reach[0])) continue;
      for (int sy = -1; sy <= 1; ++sy) {
        if (!(fabs(cell_delta(wj[1], wi[1], sy)) < reach[1])) continue;
        for (int sz = -1; sz <= 1; ++sz) {
          if (j == i && sx == 0 && sy == 0 && sz == 0) continue;
          const int s[3] = {sx, sy, sz};
          double r[3];
          cell_site_vector(wj, wi, s, L, r);
          if (!(cell_norm2(r) < c2)) continue;
          atom[n] = j;
          code[n++] = cell_shift_code(sx, sy, sz);
        }
      }
    }
  }
  return n;
}

}  // namespace egnn

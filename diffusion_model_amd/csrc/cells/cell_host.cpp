// Host side of the periodic-cell environments: the argument checks of the device entries (cell_env.hip) and the host statement
// egnn_cell_env_host -- the bond list and the shell clusters of a batch of cells computed on the CPU through cell_math.h, the text
// the kernels compile.  No HIP call, no device code: checked (and run under the sanitizers, make asan) on a machine without a GPU.
#include <math.h>
#include <string.h>

#include "cell_host.h"
#include "cell_math.h"

namespace egnn {

int cell_batch_core_check(const char* who, int C, int N, const int32_t* cell_ptr, const double* lattice, CellWidthRule rule, double reach) {
  if (cell_ptr[0] != 0 || cell_ptr[C] != N) { set_error("%s: cell_ptr must run from 0 to N = %d", who, N); return EGNN_EINVAL; }
  for (int c = 0; c < C; ++c)
    if (int rc = ptr_step_check(who, "cell_ptr", "cell", cell_ptr, c, kCellMaxAtoms)) return rc;
  if (!lattice) return EGNN_OK;
  for (int c = 0; c < C; ++c) {
    const double* L = lattice + 9 * (size_t)c;
    double w[3];
    if (!cell_widths(L, w)) { set_error("%s: cell %d has a singular lattice", who, c); return EGNN_EINVAL; }
    if (rule)
      if (int rc = rule(who, c, L, w, reach)) return rc;
  }
  return EGNN_OK;
}

// 27 images hold every bond of a cell whose widths reach the cutoff (cell_math.h)
static int cell_widths_cover_rule(const char* who, int c, const double*, const double* w, double cutoff) {
  for (int k = 0; k < 3; ++k)
    if (!(w[k] >= cutoff)) {
      set_error("%s: cell %d has a perpendicular width %.6g below the cutoff %.6g (27 images are not complete)", who, c, w[k], cutoff);
      return EGNN_EINVAL;
    }
  return EGNN_OK;
}

int cell_batch_check(const char* who, int C, int N, const int32_t* cell_ptr, const double* lattice, double cutoff) {
  if (C < 1 || N < 0 || !cell_ptr) { set_error("bad %s arguments (C >= 1, N >= 0, the host copy of cell_ptr given)", who); return EGNN_EINVAL; }
  if (!(cutoff > 0.0) || !(cutoff < 1e30)) { set_error("%s: cutoff must be positive and finite", who); return EGNN_EINVAL; }
  return cell_batch_core_check(who, C, N, cell_ptr, lattice, cell_widths_cover_rule, cutoff);
}

int cell_env_params_check(const char* who, int M, int shells, int max_atoms, const void* centre_cell, const void* centre) {
  if (M < 0 || (M > 0 && (!centre_cell || !centre))) { set_error("bad %s arguments (M >= 0 centres given)", who); return EGNN_EINVAL; }
  if (shells < 1 || shells > kCellMaxShells) { set_error("%s: shells %d (1 <= shells <= %d)", who, shells, kCellMaxShells); return EGNN_EINVAL; }
  if (max_atoms < 1 || max_atoms > kCellMaxEnvAtoms) {
    set_error("%s: max_atoms %d (1 <= max_atoms <= %d)", who, max_atoms, kCellMaxEnvAtoms);
    return EGNN_EINVAL;
  }
  return EGNN_OK;
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_cell_env_host(int C, int A, const int32_t* cell_ptr, const double* lattice, const double* frac, const int32_t* type,
                       double cutoff, int M, const int32_t* centre_cell, const int32_t* centre, int shells, int max_atoms,
                       int32_t* bond_ptr, int64_t bond_cap, int32_t* bond_atom, int32_t* bond_shift, int32_t* env_size,
                       int64_t env_cap, int32_t* env_atom, int32_t* env_shift, int32_t* env_type, float* env_pos) {
  const char* who = "egnn_cell_env_host";
  if (C < 1 || !cell_ptr || !lattice || (cell_ptr[C] > 0 && (!frac || !type)) || !bond_ptr || (M > 0 && !env_size)) {
    set_error("bad %s arguments (C >= 1; cell_ptr, lattice, frac, type, bond_ptr and env_size given)", who);
    return EGNN_EINVAL;
  }
  if (int rc = atom_types_check(who, A, kCellMaxTypes)) return rc;
  if (int rc = cell_env_params_check(who, M, shells, max_atoms, centre_cell, centre)) return rc;
  const int N = cell_ptr[C];
  if (int rc = cell_batch_check(who, C, N, cell_ptr, lattice, cutoff)) return rc;
  for (int i = 0; i < N; ++i) {   // atom by atom: the first bad atom is named, its type before its coordinates
    if (int rc = type_range_check(who, type, i, i + 1, A)) return rc;
    if (int rc = cell_frac_finite_check(who, frac, i, i + 1)) return rc;
  }
  for (int m = 0; m < M; ++m) {
    const int c = centre_cell[m];
    if (c < 0 || c >= C) { set_error("%s: centre %d names cell %d outside [0, %d)", who, m, c, C); return EGNN_EINVAL; }
    if (centre[m] < cell_ptr[c] || centre[m] >= cell_ptr[c + 1]) {
      set_error("%s: centre %d is atom %d outside its cell %d, atoms [%d, %d)", who, m, centre[m], c, cell_ptr[c], cell_ptr[c + 1]);
      return EGNN_EINVAL;
    }
  }

  int n_max = 0;
  for (int c = 0; c < C; ++c) n_max = cell_ptr[c + 1] - cell_ptr[c] > n_max ? cell_ptr[c + 1] - cell_ptr[c] : n_max;
  Scratch<double> w(3 * (size_t)N);
  Scratch<int32_t> keys((size_t)max_atoms + 2), seen((size_t)max_atoms + 2), r_atom(27 * (size_t)n_max), r_code(27 * (size_t)n_max);
  if (int rc = cell_wrap_batch(who, N, frac, w)) return rc;
  if (!keys.p || !seen.p || !r_atom.p || !r_code.p) { set_error("%s: out of memory", who); return EGNN_ENOMEM; }
  const double c2 = cutoff * cutoff;

  // ---- bond list: rows ascending by (atom, shift code); counted, then written ----
  Scratch<int32_t> b_atom(0), b_shift(0);
  bond_ptr[0] = 0;
  for (int pass = 0; pass < 2; ++pass) {
    int64_t n_bonds = 0;
    for (int c = 0; c < C; ++c) {
      const double* L = lattice + 9 * (size_t)c;
      const int lo = cell_ptr[c], hi = cell_ptr[c + 1];
      double width[3], reach[3];
      cell_widths(L, width);   // regular: the batch check has passed
      for (int k = 0; k < 3; ++k) reach[k] = cutoff * (1.0 + 1e-6) / width[k];
      for (int i = lo; i < hi; ++i) {
        const int deg = cell_row_bonds(w.p, L, reach, lo, hi, i, c2, r_atom.p, r_code.p);
        if (pass == 1 && deg > 0) {
          memcpy(b_atom.p + n_bonds, r_atom.p, sizeof(int32_t) * (size_t)deg);
          memcpy(b_shift.p + n_bonds, r_code.p, sizeof(int32_t) * (size_t)deg);
        }
        n_bonds += deg;
        if (n_bonds > 2147483647LL) { set_error("%s: more than 2^31 - 1 bonds", who); return EGNN_EINVAL; }
        bond_ptr[i + 1] = (int32_t)n_bonds;
      }
    }
    if (pass == 0 && (!b_atom.reset((size_t)n_bonds) || !b_shift.reset((size_t)n_bonds))) {
      set_error("%s: out of memory", who);
      return EGNN_ENOMEM;
    }
  }
  const int64_t E = bond_ptr[N];
  if (bond_atom && bond_shift && bond_cap >= E && E > 0) {
    memcpy(bond_atom, b_atom.p, sizeof(int32_t) * (size_t)E);
    memcpy(bond_shift, b_shift.p, sizeof(int32_t) * (size_t)E);
  }

  // ---- environments: breadth-first over the bond list.  `keys` holds the sites in discovery order, `seen` the same keys kept
  // sorted: the output is the centre, then `seen` without it ----
  const bool lists = env_atom && env_shift && env_type && env_pos;
  for (int pass = 0; pass < 2; ++pass) {
    int64_t total = 0;
    for (int m = 0; m < M; ++m) {
      const int cell = centre_cell[m], lo = cell_ptr[cell];
      const int32_t key0 = (centre[m] - lo) * kCellShiftCodes + kCellCentreCode;
      int count = 1, begin = 0;
      keys[0] = seen[0] = key0;
      for (int hop = 0; hop < shells && count <= max_atoms; ++hop) {
        const int end = count;
        for (int f = begin; f < end && count <= max_atoms; ++f) {
          const int atom = lo + keys[f] / kCellShiftCodes, code = keys[f] % kCellShiftCodes;
          for (int e = bond_ptr[atom]; e < bond_ptr[atom + 1] && count <= max_atoms; ++e) {
            const int nc = cell_shift_add(code, b_shift[e]);
            if (nc < 0) continue;   // unreachable in four hops of |s_k| <= 1
            const int32_t key = (b_atom[e] - lo) * kCellShiftCodes + nc;
            int a = 0, b = count;   // first entry of seen not below key
            while (a < b) {
              const int mid = (a + b) / 2;
              if (seen[mid] < key) a = mid + 1; else b = mid;
            }
            if (a < count && seen[a] == key) continue;
            for (int t = count; t > a; --t) seen[t] = seen[t - 1];
            seen[a] = key;
            keys[count++] = key;
          }
        }
        begin = end;
      }
      if (count > max_atoms) {   // the sentinel: nothing is listed for this centre
        env_size[m] = max_atoms + 1;
        continue;
      }
      env_size[m] = count;
      if (pass == 1) {
        const double* L = lattice + 9 * (size_t)cell;
        size_t at = (size_t)total;
        for (int t = -1; t < count; ++t) {
          const int32_t key = t < 0 ? key0 : seen[t];
          if (t >= 0 && key == key0) continue;
          const int atom = lo + key / kCellShiftCodes, code = key % kCellShiftCodes;
          double r[3];
          cell_listed_vector(w.p, L, &w[3 * (size_t)centre[m]], atom, code, r);
          env_atom[at] = atom;
          env_shift[at] = code;
          env_type[at] = type[atom];
          for (int x = 0; x < 3; ++x) env_pos[3 * at + x] = (float)r[x];
          ++at;
        }
      }
      total += count;
    }
    if (!lists || env_cap < total) break;   // sizes only
  }
  return EGNN_OK;
}

}  // extern "C"

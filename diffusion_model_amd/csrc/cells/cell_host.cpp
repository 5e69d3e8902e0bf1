// Host side of the periodic-cell environments: the argument checks of the device entries (cell_env.hip) and the host statement
// egnn_cell_env_host -- the bond list and the shell clusters of a batch of cells computed on the CPU through cell_math.h, the text
// the kernels compile.  No HIP call, no device code: checked (and run under the sanitizers, make asan) on a machine without a GPU.
#include <math.h>
#include <string.h>

#include "cell_host.h"
#include "cell_math.h"

namespace egnn {

int cell_batch_check(const char* who, int C, int N, const int32_t* cell_ptr, const double* lattice, double cutoff) {
  if (C < 1 || N < 0 || !cell_ptr) { set_error("bad %s arguments (C >= 1, N >= 0, the host copy of cell_ptr given)", who); return EGNN_EINVAL; }
  if (!(cutoff > 0.0) || !(cutoff < 1e30)) { set_error("%s: cutoff must be positive and finite", who); return EGNN_EINVAL; }
  if (cell_ptr[0] != 0 || cell_ptr[C] != N) { set_error("%s: cell_ptr must run from 0 to N = %d", who, N); return EGNN_EINVAL; }
  for (int c = 0; c < C; ++c)
    if (int rc = ptr_step_check(who, "cell_ptr", "cell", cell_ptr, c, kCellMaxAtoms)) return rc;
  if (!lattice) return EGNN_OK;
  for (int c = 0; c < C; ++c) {
    double w[3];
    if (!cell_widths(lattice + 9 * (size_t)c, w)) { set_error("%s: cell %d has a singular lattice", who, c); return EGNN_EINVAL; }
    for (int k = 0; k < 3; ++k)
      if (!(w[k] >= cutoff)) {
        set_error("%s: cell %d has a perpendicular width %.6g below the cutoff %.6g (27 images are not complete)", who, c, w[k], cutoff);
        return EGNN_EINVAL;
      }
  }
  return EGNN_OK;
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
  for (int i = 0; i < N; ++i) {
    if (type[i] < 0 || type[i] >= A) { set_error("%s: atom %d has type %d outside [0, %d)", who, i, type[i], A); return EGNN_EINVAL; }
    for (int k = 0; k < 3; ++k)
      if (!(fabs(frac[3 * (size_t)i + k]) < 1e15)) { set_error("%s: atom %d has a fractional coordinate that is not finite", who, i); return EGNN_EINVAL; }
  }
  for (int m = 0; m < M; ++m) {
    const int c = centre_cell[m];
    if (c < 0 || c >= C) { set_error("%s: centre %d names cell %d outside [0, %d)", who, m, c, C); return EGNN_EINVAL; }
    if (centre[m] < cell_ptr[c] || centre[m] >= cell_ptr[c + 1]) {
      set_error("%s: centre %d is atom %d outside its cell %d, atoms [%d, %d)", who, m, centre[m], c, cell_ptr[c], cell_ptr[c + 1]);
      return EGNN_EINVAL;
    }
  }

  Scratch<double> w(3 * (size_t)N);
  Scratch<int32_t> keys((size_t)max_atoms + 2), seen((size_t)max_atoms + 2);
  if (!w.p || !keys.p || !seen.p) { set_error("%s: out of memory", who); return EGNN_ENOMEM; }
  for (size_t t = 0; t < 3 * (size_t)N; ++t) w[t] = cell_wrap(frac[t]);
  const double c2 = cutoff * cutoff;

  // ---- bond list: rows ascending by (atom, shift code); counted, then written ----
  Scratch<int32_t> b_atom(0), b_shift(0);
  bond_ptr[0] = 0;
  for (int pass = 0; pass < 2; ++pass) {
    int64_t n_bonds = 0;
    for (int c = 0; c < C; ++c) {
      const double* L = lattice + 9 * (size_t)c;
      for (int i = cell_ptr[c]; i < cell_ptr[c + 1]; ++i) {
        for (int j = cell_ptr[c]; j < cell_ptr[c + 1]; ++j)
          for (int sx = -1; sx <= 1; ++sx)
            for (int sy = -1; sy <= 1; ++sy)
              for (int sz = -1; sz <= 1; ++sz) {
                if (j == i && sx == 0 && sy == 0 && sz == 0) continue;
                const int s[3] = {sx, sy, sz};
                double r[3];
                cell_site_vector(&w[3 * (size_t)j], &w[3 * (size_t)i], s, L, r);
                if (!(cell_norm2(r) < c2)) continue;
                if (pass == 1) {
                  b_atom[(size_t)n_bonds] = j;
                  b_shift[(size_t)n_bonds] = cell_shift_code(sx, sy, sz);
                }
                ++n_bonds;
              }
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
          int s[3];
          double r[3];
          cell_shift_decode(code, s);
          cell_site_vector(&w[3 * (size_t)atom], &w[3 * (size_t)centre[m]], s, L, r);
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

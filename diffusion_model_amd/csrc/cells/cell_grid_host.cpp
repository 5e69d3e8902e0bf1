// Host side of the linked-cell search of periodic cells: the argument checks of the device entries (cell_grid.hip), the grid rule
// egnn_cell_grid_dims and the host statement egnn_cell_grid_host -- bins, bin starts and sorted order of a batch of cells, and the
// bond list and the pair counts found THROUGH THE GRID WALK, computed on the CPU through cell_grid_math.h, the text the kernels
// compile.  No HIP call, no device code: checked (and run under the sanitizers) on a machine without a GPU.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "cell_grid_host.h"
#include "cell_grid_math.h"

namespace egnn {

int cell_grid_params_check(const char* who, double radius, int reach, double min_width) {
  if (!(radius > 0.0) || !(radius < 1e30)) { set_error("%s: radius must be positive and finite", who); return EGNN_EINVAL; }
  if (reach < 1 || reach > kCellGridMaxReach) { set_error("%s: reach %d (1 <= reach <= %d)", who, reach, kCellGridMaxReach); return EGNN_EINVAL; }
  if (!(min_width >= 0.0) || !(min_width < 1e30)) { set_error("%s: min_width must be finite and not negative", who); return EGNN_EINVAL; }
  return EGNN_OK;
}

int cell_grid_dims_check(const char* who, int C, const double* lattice, const int32_t* nb, double radius, int reach, int64_t* n_bins) {
  int64_t total = 0;
  for (int c = 0; c < C; ++c) {
    const int32_t* g = nb + 3 * (size_t)c;
    if (g[0] == 0 && g[1] == 0 && g[2] == 0) continue;
    const int d[3] = {g[0], g[1], g[2]};
    double w[3];
    if (!cell_widths(lattice + 9 * (size_t)c, w)) { set_error("%s: cell %d has a singular lattice", who, c); return EGNN_EINVAL; }
    if (!cell_grid_valid(lattice + 9 * (size_t)c, radius, reach, d)) {
      set_error("%s: cell %d (widths %.6g, %.6g, %.6g) has the grid %d x %d x %d, which the walk of radius %.6g and reach %d is not "
                "complete on (2 reach + 1 <= nb_k <= floor(reach w_k / radius), at most %d)", who, c, w[0], w[1], w[2], d[0], d[1], d[2],
                radius, reach, kCellGridMaxBins);
      return EGNN_EINVAL;
    }
    total += (int64_t)d[0] * d[1] * d[2];
    if (total > 2147483646LL) { set_error("%s: more than 2^31 - 2 bins in the batch (fewer cells per call, or a larger min_width)", who); return EGNN_EINVAL; }
  }
  *n_bins = total;
  return EGNN_OK;
}

int cell_grid_tiles_check(const char* who, int C, const int32_t* nb, const int32_t* tiles, int n_tiles) {
  if (n_tiles < 0 || (n_tiles > 0 && !tiles)) { set_error("bad %s arguments (n_tiles >= 0 tiles given, with their HOST copy)", who); return EGNN_EINVAL; }
  for (int t = 0; t < n_tiles; ++t) {
    const int c = tiles[2 * (size_t)t];
    if (c < 0 || c >= C) { set_error("%s: tile %d names cell %d outside [0, %d)", who, t, c, C); return EGNN_EINVAL; }
    if (nb[3 * (size_t)c] == 0) { set_error("%s: tile %d names cell %d, which is not gridded (nb = 0)", who, t, c); return EGNN_EINVAL; }
  }
  return EGNN_OK;
}

namespace {

int compare_keys(const void* a, const void* b) {
  const int32_t x = *static_cast<const int32_t*>(a), y = *static_cast<const int32_t*>(b);
  return x < y ? -1 : (x > y ? 1 : 0);
}

}  // namespace

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_cell_grid_dims(int C, const double* lattice, double radius, int reach, double min_width, int32_t* nb) {
  const char* who = "egnn_cell_grid_dims";
  if (C < 1 || !lattice || !nb) { set_error("bad %s arguments (C >= 1; lattice and nb given)", who); return EGNN_EINVAL; }
  if (int rc = cell_grid_params_check(who, radius, reach, min_width)) return rc;
  for (int c = 0; c < C; ++c) {
    int d[3];
    if (!cell_grid_dims(lattice + 9 * (size_t)c, radius, reach, min_width, d)) { set_error("%s: cell %d has a singular lattice", who, c); return EGNN_EINVAL; }
    for (int k = 0; k < 3; ++k) nb[3 * (size_t)c + k] = d[k];
  }
  return EGNN_OK;
}

int egnn_cell_grid_host(int C, int A, const int32_t* cell_ptr, const double* lattice, const double* frac, const int32_t* type,
                        double radius, int reach, double min_width, int32_t* nb, int64_t* n_bins, int32_t* atom_bin, int64_t bin_cap,
                        int32_t* bin_start, int32_t* sorted_atom, double* sorted_frac, int32_t* bond_ptr, int64_t bond_cap,
                        int32_t* bond_atom, int32_t* bond_shift, double dR, int nbins, int64_t* counts) {
  const char* who = "egnn_cell_grid_host";
  if (C < 1 || !cell_ptr || !lattice || (cell_ptr[C] > 0 && (!frac || !type)) || !nb || !n_bins) {
    set_error("bad %s arguments (C >= 1; cell_ptr, lattice, frac, type, nb and n_bins given)", who);
    return EGNN_EINVAL;
  }
  if (int rc = atom_types_check(who, A, kCellMaxTypes)) return rc;
  if (int rc = cell_grid_params_check(who, radius, reach, min_width)) return rc;
  const int N = cell_ptr[C];
  if (int rc = cell_batch_check(who, C, N, cell_ptr, lattice, bond_ptr ? radius : 1e-300)) return rc;
  if (counts) {
    if (int rc = cell_stat_pair_check(who, C, A, lattice, dR, nbins)) return rc;
    if (!((double)nbins * dR <= radius)) {
      set_error("%s: the pair counts reach nbins dR = %.6g, beyond the radius %.6g of the grid", who, (double)nbins * dR, radius);
      return EGNN_EINVAL;
    }
  }
  if (int rc = type_range_check(who, type, 0, N, A)) return rc;
  if (int rc = cell_frac_finite_check(who, frac, 0, N)) return rc;

  // ---- the grids ----
  Scratch<int32_t> dims(3 * (size_t)C);
  Scratch<int64_t> first(C + (size_t)1);   // the first bin of every cell
  if (!dims.p || !first.p) { set_error("%s: out of memory", who); return EGNN_ENOMEM; }
  int n_max = 0;
  for (int c = 0; c < C; ++c) {
    int d[3];
    const double* L = lattice + 9 * (size_t)c;
    if (!cell_grid_dims(L, radius, reach, min_width, d)) { set_error("%s: cell %d has a singular lattice", who, c); return EGNN_EINVAL; }
    if (d[0] == 0 && (bond_ptr || counts)) {
      double w[3];
      cell_widths(L, w);
      set_error("%s: cell %d (widths %.6g, %.6g, %.6g) is not griddable at radius %.6g and reach %d: fewer than %d bins on an axis",
                who, c, w[0], w[1], w[2], radius, reach, 2 * reach + 1);
      return EGNN_EINVAL;
    }
    for (int k = 0; k < 3; ++k) dims[3 * (size_t)c + k] = d[k];
    first[c + (size_t)1] = first[c] + (int64_t)d[0] * d[1] * d[2];
    if (first[c + (size_t)1] > 2147483646LL) { set_error("%s: more than 2^31 - 2 bins in the batch", who); return EGNN_EINVAL; }
    n_max = cell_ptr[c + 1] - cell_ptr[c] > n_max ? cell_ptr[c + 1] - cell_ptr[c] : n_max;
  }
  const int64_t B = first[C];
  memcpy(nb, dims.p, sizeof(int32_t) * 3 * (size_t)C);
  *n_bins = B;

  // ---- bins, bin starts (a counting sort: stable, so a bin holds its atoms ascending by index) ----
  Scratch<double> w(3 * (size_t)N);
  Scratch<int32_t> bin(N), start((size_t)B + 1), order(N), cursor((size_t)B + 1);
  if (int rc = cell_wrap_batch(who, N, frac, w)) return rc;
  if (!bin.p || !start.p || !order.p || !cursor.p) { set_error("%s: out of memory", who); return EGNN_ENOMEM; }
  for (int c = 0; c < C; ++c) {
    const int d[3] = {dims[3 * (size_t)c], dims[3 * (size_t)c + 1], dims[3 * (size_t)c + 2]};
    for (int i = cell_ptr[c]; i < cell_ptr[c + 1]; ++i) {
      bin[i] = d[0] ? cell_grid_bin(frac + 3 * (size_t)i, d) : -1;
      if (d[0]) ++start[(size_t)first[c] + bin[i] + 1];
    }
  }
  for (int64_t b = 0; b < B; ++b) start[(size_t)b + 1] += start[(size_t)b];
  memcpy(cursor.p, start.p, sizeof(int32_t) * ((size_t)B + 1));
  for (int i = 0; i < N; ++i) order[i] = -1;
  for (int c = 0; c < C; ++c) {
    if (!dims[3 * (size_t)c]) continue;
    const int lo = cell_ptr[c], base = start[(size_t)first[c]];
    for (int i = lo; i < cell_ptr[c + 1]; ++i) order[lo + (cursor[(size_t)first[c] + bin[i]]++ - base)] = i;
  }
  if (atom_bin && N > 0) memcpy(atom_bin, bin.p, sizeof(int32_t) * (size_t)N);
  if (bin_start && bin_cap >= B + 1) memcpy(bin_start, start.p, sizeof(int32_t) * ((size_t)B + 1));
  if (sorted_atom && N > 0) memcpy(sorted_atom, order.p, sizeof(int32_t) * (size_t)N);
  if (sorted_frac)
    for (int p = 0; p < N; ++p)
      for (int x = 0; x < 3; ++x) sorted_frac[3 * (size_t)p + x] = order[p] >= 0 ? w[3 * (size_t)order[p] + x] : 0.0;
  if (!bond_ptr && !counts) return EGNN_OK;

  // the atoms of bin cb of cell c are order[lo + start[first + cb] - base .. lo + start[first + cb + 1] - base)
  // ---- bond list through the walk: the candidates arrive in bin order, a row is sorted by key (atom 729 + code) ----
  if (bond_ptr) {
    Scratch<int32_t> keys(n_max);
    if (!keys.p) { set_error("%s: out of memory", who); return EGNN_ENOMEM; }
    const double c2 = radius * radius;
    const int T = (2 * reach + 1) * (2 * reach + 1) * (2 * reach + 1);
    bond_ptr[0] = 0;
    for (int pass = 0; pass < 2; ++pass) {
      int64_t n_bonds = 0;
      for (int c = 0; c < C; ++c) {
        const double* L = lattice + 9 * (size_t)c;
        const int d[3] = {dims[3 * (size_t)c], dims[3 * (size_t)c + 1], dims[3 * (size_t)c + 2]};
        const int lo = cell_ptr[c], base = start[(size_t)first[c]];
        for (int i = lo; i < cell_ptr[c + 1]; ++i) {
          int b[3], deg = 0;
          cell_grid_unflat(bin[i], d, b);
          for (int t = 0; t < T; ++t) {
            int s[3];
            const int cb = cell_grid_candidate(b, d, reach, t, s);
            const int code = cell_shift_code(s[0], s[1], s[2]);
            for (int p = start[(size_t)first[c] + cb] - base; p < start[(size_t)first[c] + cb + 1] - base; ++p) {
              const int j = order[lo + p];
              if (j == i && code == kCellCentreCode) continue;
              double r[3];
              cell_site_vector(&w[3 * (size_t)j], &w[3 * (size_t)i], s, L, r);
              if (cell_norm2(r) < c2) keys[deg++] = (j - lo) * kCellShiftCodes + code;
            }
          }
          if (pass == 1) {
            qsort(keys.p, (size_t)deg, sizeof(int32_t), compare_keys);
            for (int e = 0; e < deg; ++e) {
              bond_atom[n_bonds + e] = lo + keys[e] / kCellShiftCodes;
              bond_shift[n_bonds + e] = keys[e] % kCellShiftCodes;
            }
          }
          n_bonds += deg;
          if (n_bonds > 2147483647LL) { set_error("%s: more than 2^31 - 1 bonds", who); return EGNN_EINVAL; }
          bond_ptr[i + 1] = (int32_t)n_bonds;
        }
      }
      if (!bond_atom || !bond_shift || bond_cap < n_bonds) break;   // sizes only
    }
  }

  // ---- pair counts through the walk: with nb_k >= 2 reach + 1 the image box of the direct walk is S_k = 1 ----
  if (counts) {
    memset(counts, 0, sizeof(int64_t) * (size_t)C * A * A * nbins);
    const double limit = cell_stat_r2_limit(dR, nbins);
    const int T = (2 * reach + 1) * (2 * reach + 1) * (2 * reach + 1);
    for (int c = 0; c < C; ++c) {
      const double* L = lattice + 9 * (size_t)c;
      const int d[3] = {dims[3 * (size_t)c], dims[3 * (size_t)c + 1], dims[3 * (size_t)c + 2]};
      const int lo = cell_ptr[c], base = start[(size_t)first[c]];
      int64_t* out = counts + (size_t)c * A * A * nbins;
      for (int i = lo; i < cell_ptr[c + 1]; ++i) {
        int b[3];
        cell_grid_unflat(bin[i], d, b);
        for (int t = 0; t < T; ++t) {
          int s[3];
          const int cb = cell_grid_candidate(b, d, reach, t, s);
          const bool centre = s[0] == 0 && s[1] == 0 && s[2] == 0;
          for (int p = start[(size_t)first[c] + cb] - base; p < start[(size_t)first[c] + cb + 1] - base; ++p) {
            const int j = order[lo + p];
            if (j == i && centre) continue;
            double r[3];
            cell_site_vector(&w[3 * (size_t)j], &w[3 * (size_t)i], s, L, r);
            const double r2 = cell_norm2(r);
            if (!(r2 < limit)) continue;
            const int k = cell_stat_bin(sqrt(r2), dR, nbins);
            if (k >= 0) ++out[((size_t)type[i] * A + type[j]) * nbins + k];
          }
        }
      }
    }
  }
  return EGNN_OK;
}

}  // extern "C"

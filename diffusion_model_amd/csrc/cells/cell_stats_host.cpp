// Host side of the real-space statistics of periodic cells: the argument checks of the device entries (cell_stats.hip) and the host
// statement egnn_cell_stats_host -- pair counts, coordination numbers, bond angles and Q^n of a batch of cells computed on the CPU
// through cell_stats_math.h, the text the kernels compile.  No HIP call, no device code: checked (and run under the sanitizers) on a
// machine without a GPU.
#include <math.h>
#include <string.h>

#include "cell_stats_host.h"
#include "cell_stats_math.h"

namespace egnn {

int cell_stat_pair_check(const char* who, int C, int A, const double* lattice, double dR, int nbins) {
  if (!(dR > 0.0) || !(dR < 1e30)) { set_error("%s: dR must be positive and finite", who); return EGNN_EINVAL; }
  if (nbins < 1) { set_error("%s: nbins %d (nbins >= 1)", who, nbins); return EGNN_EINVAL; }
  if ((long long)A * A * nbins > kCellStatMaxHist) {
    set_error("%s: %d x %d x %d histogram bins (at most %d: 64 KiB of LDS)", who, A, A, nbins, kCellStatMaxHist);
    return EGNN_EINVAL;
  }
  for (int c = 0; c < C; ++c) {
    int S[3];
    if (!cell_stat_image_box(lattice + 9 * (size_t)c, dR, nbins, S)) { set_error("%s: cell %d has a singular lattice", who, c); return EGNN_EINVAL; }
    for (int k = 0; k < 3; ++k)
      if (S[k] > kCellStatMaxImages) {
        set_error("%s: cell %d needs more than %d images along axis %d to reach %.6g (an image box too wide; lower R)", who, c,
                  kCellStatMaxImages, k, (double)nbins * dR);
        return EGNN_EINVAL;
      }
  }
  return EGNN_OK;
}

int cell_stat_bond_check(const char* who, int A, double dtheta, int max_cn, int former, int bridge) {
  if (!(dtheta >= 0.5) || !(dtheta <= 180.0) || struct_angle_bins(dtheta) > kStructMaxAngleBins) {
    set_error("%s: dtheta must lie in [0.5, 180] degrees (at most %d angle bins)", who, kStructMaxAngleBins);
    return EGNN_EINVAL;
  }
  if (max_cn < 1 || max_cn > kStructMaxCn) { set_error("%s: max_cn %d (1 <= max_cn <= %d)", who, max_cn, kStructMaxCn); return EGNN_EINVAL; }
  if (former < 0 || former >= A || bridge < 0 || bridge >= A || former == bridge) {
    set_error("%s: former %d and bridge %d must be two different types in [0, %d)", who, former, bridge, A);
    return EGNN_EINVAL;
  }
  return EGNN_OK;
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_cell_stats_host(int C, int A, const int32_t* cell_ptr, const double* lattice, const double* frac, const int32_t* type,
                         double dR, int nbins, int64_t* counts, double cutoff, double dtheta, int max_cn, int former, int bridge,
                         int32_t* coordination, int64_t* cn, int64_t* angles, int32_t* qn, int64_t* qn_hist, int32_t* overflow) {
  const char* who = "egnn_cell_stats_host";
  const bool pairs = counts != nullptr, bonds = coordination != nullptr;
  if (C < 1 || !cell_ptr || !lattice || (cell_ptr[C] > 0 && (!frac || !type)) || (!pairs && !bonds) ||
      (bonds && (!cn || !angles || !qn || !qn_hist || !overflow))) {
    set_error("bad %s arguments (C >= 1; cell_ptr, lattice, frac and type given; counts, or coordination with cn, angles, qn, qn_hist "
              "and overflow)", who);
    return EGNN_EINVAL;
  }
  if (int rc = atom_types_check(who, A, kCellMaxTypes)) return rc;
  const int N = cell_ptr[C];
  if (int rc = cell_batch_check(who, C, N, cell_ptr, lattice, bonds ? cutoff : 1e-300)) return rc;
  if (pairs)
    if (int rc = cell_stat_pair_check(who, C, A, lattice, dR, nbins)) return rc;
  if (bonds)
    if (int rc = cell_stat_bond_check(who, A, dtheta, max_cn, former, bridge)) return rc;
  if (int rc = type_range_check(who, type, 0, N, A)) return rc;
  if (int rc = cell_frac_finite_check(who, frac, 0, N)) return rc;

  int n_max = 0;
  for (int c = 0; c < C; ++c) n_max = cell_ptr[c + 1] - cell_ptr[c] > n_max ? cell_ptr[c + 1] - cell_ptr[c] : n_max;
  Scratch<double> w(3 * (size_t)N);
  if (int rc = cell_wrap_batch(who, N, frac, w)) return rc;

  // ---- ordered pairs over the image box ----
  if (pairs) {
    memset(counts, 0, sizeof(int64_t) * (size_t)C * A * A * nbins);
    const double limit = cell_stat_r2_limit(dR, nbins);
    for (int c = 0; c < C; ++c) {
      const double* L = lattice + 9 * (size_t)c;
      int S[3];
      double width[3], reach[3];
      cell_stat_image_box(L, dR, nbins, S);
      cell_widths(L, width);
      for (int k = 0; k < 3; ++k) reach[k] = cell_stat_axis_reach(dR, nbins, width[k]);
      int64_t* out = counts + (size_t)c * A * A * nbins;
      for (int i = cell_ptr[c]; i < cell_ptr[c + 1]; ++i)
        for (int j = cell_ptr[c]; j < cell_ptr[c + 1]; ++j) {
          int64_t* row = out + ((size_t)type[i] * A + type[j]) * nbins;
          for (int sx = -S[0]; sx <= S[0]; ++sx) {
            if (!(fabs(cell_delta(w[3 * (size_t)j], w[3 * (size_t)i], sx)) < reach[0])) continue;
            for (int sy = -S[1]; sy <= S[1]; ++sy) {
              if (!(fabs(cell_delta(w[3 * (size_t)j + 1], w[3 * (size_t)i + 1], sy)) < reach[1])) continue;
              for (int sz = -S[2]; sz <= S[2]; ++sz) {
                if (j == i && sx == 0 && sy == 0 && sz == 0) continue;
                const int s[3] = {sx, sy, sz};
                double r[3];
                cell_site_vector(&w[3 * (size_t)j], &w[3 * (size_t)i], s, L, r);
                const double r2 = cell_norm2(r);
                if (!(r2 < limit)) continue;
                const int k = cell_stat_bin(sqrt(r2), dR, nbins);
                if (k >= 0) ++row[k];
              }
            }
          }
        }
    }
  }
  if (!bonds) return EGNN_OK;

  // ---- bonds: coordination, CN histogram and angles; then Q^n from the finished coordination ----
  const int nth = struct_angle_bins(dtheta), P = type_pairs(A), ncn = max_cn + 1;
  const size_t n_cn = (size_t)A * A * ncn, n_ang = (size_t)A * P * nth;
  memset(cn, 0, sizeof(int64_t) * C * n_cn);
  memset(angles, 0, sizeof(int64_t) * C * n_ang);
  memset(qn_hist, 0, sizeof(int64_t) * (size_t)C * ncn);
  memset(overflow, 0, sizeof(int32_t) * (size_t)C);
  if (N > 0) memset(coordination, 0, sizeof(int32_t) * (size_t)N * A);
  Scratch<int32_t> b_atom(27 * (size_t)n_max), b_code(27 * (size_t)n_max);
  Scratch<double> vec(3 * (size_t)kMaxNeighbours);
  if (!b_atom.p || !b_code.p || !vec.p) { set_error("%s: out of memory", who); return EGNN_ENOMEM; }
  const double c2 = cutoff * cutoff;
  for (int pass = 0; pass < 2; ++pass)
    for (int c = 0; c < C; ++c) {
      const double* L = lattice + 9 * (size_t)c;
      const int lo = cell_ptr[c], hi = cell_ptr[c + 1];
      double width[3], reach[3];
      cell_widths(L, width);
      for (int k = 0; k < 3; ++k) reach[k] = cutoff * (1.0 + 1e-6) / width[k];
      for (int i = lo; i < hi; ++i) {
        const int deg = cell_row_bonds(w.p, L, reach, lo, hi, i, c2, b_atom.p, b_code.p);
        const int ti = type[i];
        if (pass == 1) {   // Q^n
          if (ti != former) { qn[i] = -1; continue; }
          int q = 0;
          for (int e = 0; e < deg; ++e) q += type[b_atom[e]] == bridge && coordination[(size_t)b_atom[e] * A + former] >= 2;
          qn[i] = q;
          ++qn_hist[(size_t)c * ncn + (q < max_cn ? q : max_cn)];
          continue;
        }
        int32_t* nb = coordination + (size_t)i * A;
        for (int e = 0; e < deg; ++e) ++nb[type[b_atom[e]]];
        for (int b = 0; b < A; ++b) ++cn[c * n_cn + ((size_t)ti * A + b) * ncn + (nb[b] < max_cn ? nb[b] : max_cn)];
        if (deg > kMaxNeighbours) { ++overflow[c]; continue; }
        for (int e = 0; e < deg; ++e) cell_listed_vector(w.p, L, &w[3 * (size_t)i], b_atom[e], b_code[e], &vec[3 * (size_t)e]);
        for (int p = 0; p < deg; ++p)
          for (int q = p + 1; q < deg; ++q) {
            const int k = struct_angle_bin(&vec[3 * (size_t)p], &vec[3 * (size_t)q], dtheta, nth);
            if (k >= 0) ++angles[c * n_ang + ((size_t)ti * P + type_pair_index(type[b_atom[p]], type[b_atom[q]], A)) * nth + k];
          }
      }
    }
  return EGNN_OK;
}

}  // extern "C"

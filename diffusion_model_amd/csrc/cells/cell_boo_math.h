// Definitions of the bond-orientational order of periodic cells (cell_boo.hip, cell_boo_host.cpp): Steinhardt's q_l, w_l and w^_l
// per atom, the Lechner-Dellago neighbour averages and the ten Wolde-Frenkel solid-bond count.  Plain C++ behind the host/device
// macro, so that the kernels and the host statement compile the same text.  An extension: no file of the reference computes it.
//
//  * neighbours of atom i: the sites (j, s) of egnn_cell_sites_* at cut = cutoff (cell_soap_math.h: every image, fp64,
//    cell_norm2(r) < cutoff^2, (i, 0) left out, the atom's own images ordinary sites), in ascending (atom, shift code), KEPT where
//    bit type_i * A + type_j of `select` is set and cell_norm2(r) != 0 (a site on top of its centre has no direction).  n_i is the
//    number of kept sites.
//  * unit vector: d = sqrt(cell_norm2(r)), u_x = r_x / d; Y_lm(u) = soap_solid_column(u_x, u_y, u_z, cell_norm2(u), m, l_max, N),
//    the real orthonormal harmonics at index l*l + l + m of soap_math.h, N its N_lm table (mpmath, rounded once).
//  * q_lm(i) = (sum over kept sites, ascending, ONE running sum from 0.0) / (double)n_i; 0 where n_i = 0.
//  * s2_l = sum_m q_lm^2, ascending in m (index l*l .. l*l + 2l), one running sum (boo_norm2);
//    q_l = sqrt((kBooFourPi / (double)(2l + 1)) * s2_l).
//  * w_l = sum over the entries e of G^l, ascending, one running sum, of ((G_e * q_a) * q_b) * q_c: G^l is the Wigner 3j tensor
//    (l l l; m1 m2 m3) carried into the real basis, stored for a <= b <= c (a, b, c = l + m in [0, 2l]) with the permutation
//    multiplicities folded in, non-zero entries only, ascending in (a, b, c).  Real for even l; for odd l the table is empty and
//    w_l is exactly 0.  Built by the caller (Racah's formula in exact arithmetic, root and basis change in mpmath, rounded once).
//  * w^_l = w_l / (s2_l * sqrt(s2_l)); 0 where s2_l is exactly 0.
//  * averaged (Lechner-Dellago): qbar_lm(i) = (q_lm(i) + sum over kept sites k, ascending, of q_lm(atom_k)) / (double)(1 + n_i),
//    one running sum that STARTS at q_lm(i); qbar_l, wbar_l and the normalised wbar_l by the formulas above.
//  * solid bonds (ten Wolde-Frenkel) at one l: s_ik = dot / (sqrt(s2(i)) * sqrt(s2(k))), dot = sum_m q_lm(i) q_lm(k) ascending in
//    m; 0 where either s2 is 0.  n_solid(i) counts the kept sites with s_ik > threshold, strictly.  The unaveraged q_lm is used.
//  * tables: g_off int32 [l_max + 2] (entries of l are g_off[l] .. g_off[l + 1]), g_idx int32 [E, 3], g_val double [E].
// No sum is reduced across threads and no floating-point atomic is used: host and device execute the same operations in the same
// order (+, -, *, /, sqrt under -ffp-contract=off).
#pragma once
#include "cell_soap_math.h"

namespace egnn {

constexpr int kBooMaxL = kSoapMaxL;     // l_max, l_solid
constexpr int kBooWaves = 4;            // rows of a workgroup, one wavefront each
constexpr int kBooChunk = 16;           // kept sites whose harmonics are staged in LDS at a time
constexpr int kBooParts = 4;            // lanes that share the harmonic columns of one staged site (64 / kBooChunk)
constexpr double kBooFourPi = 12.566370614359172;   // 4 pi rounded to fp64

EGNN_HD bool boo_config_ok(int A, int l_max) { return A >= 1 && A <= kCellMaxTypes && l_max >= 0 && l_max <= kBooMaxL; }
EGNN_HD bool boo_selected(unsigned select, int A, int ti, int tj) { return (select >> (ti * A + tj)) & 1u; }

// the stride of one staged site's harmonics: odd, so that consecutive sites start in different LDS banks
EGNN_HD int boo_stride(int l_max) { return soap_lm_count(l_max) | 1; }

// whether site (atom j, shift code) of a row of centre i is kept; u is its unit vector where it is.  lo .. hi: the centre's cell.
EGNN_HD bool boo_site(const double* frac, const int* type, const double* L, int lo, int hi, int A, unsigned select, int i, int j, int code,
                      double* u) {
  if (!cell_site_listed(lo, hi, j, code)) return false;
  const int ti = type[i], tj = type[j];
  if (ti < 0 || ti >= A || tj < 0 || tj >= A || !boo_selected(select, A, ti, tj)) return false;
  double wi[3], r[3];
  cell_wrapped_read(frac, i, wi);
  cell_listed_vector(frac, L, wi, j, code, r);
  const double d2 = cell_norm2(r);
  if (!(d2 > 0.0)) return false;
  const double d = sqrt(d2);
  u[0] = r[0] / d; u[1] = r[1] / d; u[2] = r[2] / d;
  return true;
}

// s2_l of one row of q_lm
EGNN_HD double boo_norm2(const double* qlm, int l) {
  double sum = 0.0;
  for (int m = 0; m <= 2 * l; ++m) sum += qlm[l * l + m] * qlm[l * l + m];
  return sum;
}

EGNN_HD double boo_q(double s2, int l) { return sqrt((kBooFourPi / (double)(2 * l + 1)) * s2); }

// w_l of one row; E entries in all: a table the row cannot be read through (offsets or an index out of range) contributes nothing
EGNN_HD double boo_w(const double* qlm, int l, int E, const int* g_off, const int* g_idx, const double* g_val) {
  const int e0 = g_off[l], e1 = g_off[l + 1];
  if (e0 < 0 || e1 < e0 || e1 > E) return 0.0;
  const double* q = qlm + l * l;
  double sum = 0.0;
  for (int e = e0; e < e1; ++e) {
    const int a = g_idx[3 * e], b = g_idx[3 * e + 1], c = g_idx[3 * e + 2];
    if (a < 0 || b < 0 || c < 0 || a > 2 * l || b > 2 * l || c > 2 * l) continue;
    sum += ((g_val[e] * q[a]) * q[b]) * q[c];
  }
  return sum;
}

EGNN_HD double boo_w_hat(double w, double s2) { return s2 == 0.0 ? 0.0 : w / (s2 * sqrt(s2)); }

// s_ik at l from the rows of the two atoms
EGNN_HD double boo_solid(const double* qi, const double* qk, int l) {
  const double si = boo_norm2(qi, l), sk = boo_norm2(qk, l);
  if (si == 0.0 || sk == 0.0) return 0.0;
  double dot = 0.0;
  for (int m = 0; m <= 2 * l; ++m) dot += qi[l * l + m] * qk[l * l + m];
  return dot / (sqrt(si) * sqrt(sk));
}

// the three invariants of degree l of one row, written at out[l], out[L1 + l], out[2 L1 + l]
EGNN_HD void boo_invariants(const double* qlm, int l, int l_max, int E, const int* g_off, const int* g_idx, const double* g_val, double* out) {
  const double s2 = boo_norm2(qlm, l), w = boo_w(qlm, l, E, g_off, g_idx, g_val);
  out[l] = boo_q(s2, l);
  out[(l_max + 1) + l] = w;
  out[2 * (l_max + 1) + l] = boo_w_hat(w, s2);
}

}  // namespace egnn

// Definitions of the SOAP power spectrum, its cosine similarity and the nearest-spectrum search (soap.hip, soap_host.cpp).  Plain
// C++ behind a host/device macro (the pattern of topo_math.h), so that the kernels and the host statement read the same text.
// They restate template_matching.py:41-68 (dscribe's SOAP(species=["O","Si"], r_cut=8, n_max=15, l_max=10, sigma=0.1), row [0],
// cosine, MSE of spectrum[0]) without ASE or dscribe, from the descriptor's DEFINITION, not from a library's numbers.
//
// Inputs: the ragged batch of egnn_topo_*: pos float32 [N,3], type int32 [N] in [0, A), A <= 4, graph_ptr int32 [B+1].  Species
// order is type index order (O = 0, Si = 1: ascending atomic number).  A centre is any atom of the batch.
//
// Parameters: r_cut, n_max <= 16, l_max <= 10, sigma, neighbour_cut (default r_cut + sigma sqrt(2 ln 1000)); a = 1 / (2 sigma^2).
//
//  * neighbours of centre i: the atoms j of the same graph with d2 < neighbour_cut^2, j = i INCLUDED (it contributes at d = 0,
//    which touches l = 0 only); d2 = (dx*dx + dy*dy) + dz*dz in fp64 from exact fp64 differences of the float32 positions.  No
//    weighting.  A type outside [0, A) contributes nothing.
//  * radial basis: r_n = linspace(1, r_cut, n_max), alpha_nl = -ln(1e-3 / r_n^l) / r_n^2, primitive phi_nl(r) = r^l exp(-alpha_nl
//    r^2), overlap S^l_nn' = 1/2 Gamma(l + 3/2) (alpha_nl + alpha_n'l)^-(l + 3/2), beta^l = (S^l)^(-1/2) (the symmetric root),
//    g_nl = sum_n' beta^l_nn' phi_n'l.
//  * primitive coefficient, p = alpha_nl + a (closed form of  int 4 pi r^2 phi_nl(r) exp(-a (r^2 + d^2)) i_l(2 a d r) dr  times
//    Y_lm(direction)):
//        c'[Z][n][l][m] = sum_{j of species Z}  (K_nl * exp(-(gamma_nl * d_j2))) * R_lm(x_j, y_j, z_j),   ascending in j,
//        K_nl = pi^(3/2) p^(-3/2) (a / p)^l,        gamma_nl = a alpha_nl / p.
//  * R_lm = d^l Y_lm are the real solid harmonics, orthonormal on the sphere: polynomials in x, y, z by recurrence
//    (soap_solid_column), no square root and no division by d.  Index lm = l*l + l + m, m = -l .. l; m > 0 carries cos(m phi),
//    m < 0 sin(|m| phi).
//  * orthonormalised coefficient: c[Z][n][l][m] = sum_n' beta^l_nn' c'[Z][n'][l][m], ascending in n'.
//  * power spectrum: p[Z1,Z2,n,n',l] = w_l * sum_m c[Z1][n][l][m] * c[Z2][n'][l][m], ascending in m, w_l = pi sqrt(8 / (2l + 1));
//    kept for Z1 <= Z2, all n, and n' >= n where Z1 = Z2 (all n' otherwise); order: (Z1, Z2) outermost ((0,0), (0,1), ..,
//    (1,1), ..), then n, then n', l innermost.  F = A n(n+1)/2 (l_max+1) + A(A-1)/2 n^2 (l_max+1): 5,115 at A = 2 and the defaults.
//  * tables: one buffer of doubles, built by the caller (SoapBasis: mpmath at >= 60 digits, rounded once to fp64):
//        K [n_max][l_max+1] | gamma [n_max][l_max+1] | beta [l_max+1][n_max][n_max] | N [(l_max+1)^2] | w [l_max+1]
//    with N_lm = sqrt((2l+1)/(4 pi) (l-|m|)!/(l+|m|)!) * (m != 0 ? sqrt 2 : 1).
//  * every sum over a row (dot product, squared norm, squared spectrum difference) has ONE order (soap_row_sum): element f goes
//    to partial f % 64, each partial adds its elements ascending; then six butterfly steps off = 32, 16, .., 1 replace
//    every partial q by partial[q] + partial[q ^ off].  That is what a wavefront does with one element per lane and __shfl_xor.
//  * cosine = dot / (sqrt(sum a^2) * sqrt(sum b^2)).  A descriptor is never zero: the centre contributes itself.
//  * spectrum distance: mse(t, r) = (sum_s ((double)t_s - (double)r_s)^2) / S, the row sum above; host and device are bitwise
//    equal.  The k smallest over the references whose group differs from the target's (a group < 0 matches nothing) ascending,
//    ties to the lower reference index, missing entries index -1 and mse +inf.
#pragma once
#include "eval_math.h"

namespace egnn {

constexpr int kSoapMaxTypes = 4;    // A
constexpr int kSoapMaxN = 16;       // n_max
constexpr int kSoapMaxL = 10;       // l_max
constexpr int kSoapMaxK = 8;        // nearest spectra kept
constexpr int kSoapChunk = 32;      // neighbours staged at a time by the descriptor kernel

EGNN_HD int soap_lm_count(int l_max) { return (l_max + 1) * (l_max + 1); }
EGNN_HD int soap_feature_count(int A, int n_max, int l_max) {
  return (A * (n_max * (n_max + 1) / 2) + A * (A - 1) / 2 * n_max * n_max) * (l_max + 1);
}
EGNN_HD bool soap_config_ok(int A, int n_max, int l_max) {
  return A >= 1 && A <= kSoapMaxTypes && n_max >= 1 && n_max <= kSoapMaxN && l_max >= 0 && l_max <= kSoapMaxL;
}
EGNN_HD bool soap_cut_ok(double cut) { return cut > 0.0 && cut < 1e150; }   // positive, finite, not NaN, and its square finite

// offsets into the table buffer
EGNN_HD int soap_table_gamma(int n_max, int l_max) { return n_max * (l_max + 1); }
EGNN_HD int soap_table_beta(int n_max, int l_max) { return 2 * n_max * (l_max + 1); }
EGNN_HD int soap_table_norm(int n_max, int l_max) { return soap_table_beta(n_max, l_max) + (l_max + 1) * n_max * n_max; }
EGNN_HD int soap_table_weight(int n_max, int l_max) { return soap_table_norm(n_max, l_max) + soap_lm_count(l_max); }
EGNN_HD int soap_table_count(int n_max, int l_max) { return soap_table_weight(n_max, l_max) + (l_max + 1); }

EGNN_HD int soap_l_of(int lm) {
  int l = 0;
  while ((l + 1) * (l + 1) <= lm) ++l;
  return l;
}

// d2 and the differences neighbour - centre
EGNN_HD double soap_dist2(const float* centre, const float* q, double* dx, double* dy, double* dz) {
  *dx = (double)q[0] - (double)centre[0];
  *dy = (double)q[1] - (double)centre[1];
  *dz = (double)q[2] - (double)centre[2];
  return ((*dx) * (*dx) + (*dy) * (*dy)) + (*dz) * (*dz);
}

// radial value of neighbour at d2 for entry q = n (l_max+1) + l of the K and gamma tables
EGNN_HD double soap_radial(const double* tables, int n_max, int l_max, int q, double d2) {
  const double g = tables[soap_table_gamma(n_max, l_max) + q] * d2;
  return tables[q] * exp(-g);
}

// R_lm for one m >= 0 and l = m .. l_max, written to out[l*l + l + m] and (m > 0) out[l*l + l - m].
//   (x + i y)^m = ca + i sa by m complex products;  P_m^m = (2m-1)!!,  P_l^m = ((2l-1) z P_(l-1)^m - (l+m-1) r2 P_(l-2)^m) / (l-m)
// (the associated Legendre function times d^(l-m) / sin^m, without the Condon-Shortley sign), R_lm = (N_lm P_l^m) * ca or sa.
EGNN_HD void soap_solid_column(double x, double y, double z, double r2, int m, int l_max, const double* norm, double* out) {
  double ca = 1.0, sa = 0.0, pmm = 1.0;
  for (int k = 1; k <= m; ++k) {
    const double na = ca * x - sa * y, nb = ca * y + sa * x;
    ca = na;
    sa = nb;
    pmm = pmm * (double)(2 * k - 1);
  }
  double p2 = 0.0, p1 = pmm;
  for (int l = m; l <= l_max; ++l) {
    double p = p1;
    if (l > m) {
      const double u = ((double)(2 * l - 1) * z) * p1, v = ((double)(l + m - 1) * r2) * p2;
      p = (u - v) / (double)(l - m);
      p2 = p1;
      p1 = p;
    }
    const int at = l * l + l;
    const double np = norm[at + m] * p;
    out[at + m] = np * ca;
    if (m > 0) out[at - m] = (norm[at - m] * p) * sa;
  }
}

// feature f -> (Z1, Z2, n, n', l)
EGNN_HD void soap_feature_decode(int f, int A, int n_max, int l_max, int* z1, int* z2, int* n, int* np, int* l) {
  const int L1 = l_max + 1, same = n_max * (n_max + 1) / 2 * L1, diff = n_max * n_max * L1;
  int a = 0, b = 0;
  for (;;) {
    const int size = a == b ? same : diff;
    if (f < size) break;
    f -= size;
    if (++b == A) { ++a; b = a; }
  }
  *z1 = a; *z2 = b;
  *l = f % L1;
  int q = f / L1;
  if (a == b) {
    int row = 0;
    while (q >= n_max - row) { q -= n_max - row; ++row; }
    *n = row; *np = row + q;
  } else {
    *n = q / n_max; *np = q % n_max;
  }
}

// one power-spectrum entry from the coefficients c [A][n_max][(l_max+1)^2] of one centre
EGNN_HD double soap_power_entry(const double* c, const double* tables, int f, int A, int n_max, int l_max) {
  int z1, z2, n, np, l;
  soap_feature_decode(f, A, n_max, l_max, &z1, &z2, &n, &np, &l);
  const int LM = soap_lm_count(l_max);
  const double* u = c + (z1 * n_max + n) * LM + l * l;
  const double* v = c + (z2 * n_max + np) * LM + l * l;
  double sum = 0.0;
  for (int m = 0; m <= 2 * l; ++m) sum += u[m] * v[m];
  return tables[soap_table_weight(n_max, l_max) + l] * sum;
}

// the butterfly of soap_row_sum on 64 partials held in an array (the host side of a wavefront's __shfl_xor steps)
EGNN_HD double soap_butterfly(double* partial) {
  double next[64];
  for (int off = 32; off >= 1; off >>= 1) {
    for (int q = 0; q < 64; ++q) next[q] = partial[q] + partial[q ^ off];
    for (int q = 0; q < 64; ++q) partial[q] = next[q];
  }
  return partial[0];
}

EGNN_HD double soap_row_dot(const double* a, const double* b, long F) {
  double partial[64];
  for (int q = 0; q < 64; ++q) partial[q] = 0.0;
  for (long f = 0; f < F; ++f) partial[f & 63] += a[f] * b[f];
  return soap_butterfly(partial);
}

EGNN_HD double soap_cosine(double dot, double na, double nb) { return dot / (sqrt(na) * sqrt(nb)); }

EGNN_HD double soap_sq_diff(float t, float r) {
  const double d = (double)t - (double)r;
  return d * d;
}

EGNN_HD double soap_row_mse(const float* t, const float* r, int S) {
  double partial[64];
  for (int q = 0; q < 64; ++q) partial[q] = 0.0;
  for (int s = 0; s < S; ++s) partial[s & 63] += soap_sq_diff(t[s], r[s]);
  return soap_butterfly(partial) / (double)S;
}

// the kSoapMaxK best (mse, index) ascending; candidates arrive in ascending index, so a tie stays behind the earlier entry
struct SoapBest {
  double mse[kSoapMaxK];
  int idx[kSoapMaxK];
};

EGNN_HD void soap_best_clear(SoapBest* b) {
  for (int q = 0; q < kSoapMaxK; ++q) { b->mse[q] = INFINITY; b->idx[q] = -1; }
}

EGNN_HD void soap_best_insert(SoapBest* b, double mse, int r) {
  bool moving = false;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int q = 0; q < kSoapMaxK; ++q) {
    if (moving || mse < b->mse[q]) {
      const double m = b->mse[q];
      const int i = b->idx[q];
      b->mse[q] = mse;
      b->idx[q] = r;
      mse = m;
      r = i;
      moving = true;
    }
  }
}

EGNN_HD bool soap_excluded(int target_group, int reference_group) { return target_group >= 0 && target_group == reference_group; }

}  // namespace egnn

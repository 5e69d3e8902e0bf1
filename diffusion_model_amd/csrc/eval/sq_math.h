// Definitions of the reciprocal-space statistics (sq.hip, sq_host.cpp): Debye sums of clusters and reciprocal-lattice sums of
// periodic cells.  Plain C++ behind a host/device macro (the pattern of structure_math.h and cells/cell_math.h), so that the
// kernels and the host statement read the same text.  No file of the reference computes a structure factor: this is an extension.
//
// Clusters.  D_ab(q) = sum_{i in a} sum_{j in b, j != i, r_ij < r_max} w(r_ij) sinc(q r_ij)
//  * distance: fp64 from the float32 positions, the differences taken in fp64: dx = (double)q.x - (double)p.x,
//    r = sqrt((dx*dx + dy*dy) + dz*dz), in exactly this order (the library is built with -ffp-contract=off).
//  * sinc(x) = 1 where x == 0, else sin(x) / x: coincident atoms and q = 0 contribute w(r).
//  * cut: a pair counts iff r < r_max; r_max = +inf is no cut.  Window: none (w = 1) or Lorch, w(r) = sinc((pi r) / r_max).
//  * every unordered pair i < j is visited once and added to the unordered type pair {t_i, t_j}; D_ab is that sum, doubled on the
//    diagonal a = b.  With no cut and q = 0 every term is exactly 1.0, so D_ab(0) = N_a N_b - delta_ab N_a exactly.
//
// Cells.  Lattice rows (a_1, a_2, a_3), integer m = (h, k, l) != 0:
//  * reciprocal rows b_i = 2 pi (a_j x a_k) / det, b_i . a_j = 2 pi delta_ij; k_m = (h b_1 + k b_2) + l b_3 per component,
//    k2 = (kx*kx + ky*ky) + kz*kz, |k_m| = sqrt(k2).  m is a vector of the sum iff it lies in the half space (h > 0, or h = 0 and
//    k > 0, or h = k = 0 and l > 0) and k2 < q_max * q_max.  Shell bin floor(|k_m| / dq), nbins = ceil(q_max / dq).  All of this is
//    +, *, /, sqrt and floor of fp64 in one fixed order: host and device agree bitwise on membership, |k| and bin.
//  * phase: t = (h w_1 + k w_2) + l w_3 on the wrapped fractional coordinates w (cell_wrap), taken mod 1 (t - floor(t)) before
//    the sine and cosine of 2 pi t; rho_a(m) = sum_{j in a} exp(-i k_m . r_j) = sum (cos, -sin).
//  * index box: |h| <= floor(q_max |a_1| / 2 pi) (|k_m . a_1| = 2 pi |h| <= |k_m| |a_1|), likewise k and l; the box the kernels
//    walk is one wider (a rounding of the bound cannot lose a vector; the membership test rejects the extra ones), capped at 1023.
#pragma once
#include "eval_math.h"

#include "../cells/cell_math.h"

namespace egnn {

constexpr int kSqMaxTypes = 4;              // A
constexpr int kSqMaxTypePairs = 10;         // A (A + 1) / 2
constexpr int kSqMaxQ = 4096;               // Q of one call
constexpr int kSqMaxBins = 4096;            // nbins
constexpr int kSqMaxAtoms = 32768;          // atoms of one graph, the limit of egnn_struct_*
constexpr int kSqMaxIndex = 1023;           // |h|, |k|, |l|
constexpr int kSqMaxVectors = 1 << 24;      // half-space vectors of one cell
constexpr int kSqRowBlock = 64;             // Debye tile: atoms i
constexpr int kSqChunk = 256;               // Debye tile: atoms j, one per thread
constexpr int kSqQBlock = 512;              // q values one pass of a Debye tile holds in registers (2 per thread)
constexpr int kSqVectorBlock = 256;         // vectors of one workgroup of the rho kernel, one per thread
constexpr int kSqAtomChunk = 1024;          // atoms of a cell staged in LDS at a time
constexpr int kSqShellBlock = 1024;         // vectors one step of the shell kernel looks at
constexpr int kSqWindowNone = 0, kSqWindowLorch = 1;
constexpr double kSqTwoPi = 6.283185307179586476925286766559;

EGNN_HD double sq_sinc(double x) { return x == 0.0 ? 1.0 : sin(x) / x; }

EGNN_HD double sq_window(double r, double r_max, int window) {
  return window == kSqWindowLorch ? sq_sinc((M_PI * r) / r_max) : 1.0;
}

// ---- cells ----
// reciprocal rows; false for a singular or non-finite lattice (the rule of cell_widths)
EGNN_HD bool sq_reciprocal(const double* L, double* Bm) {
  double w[3];
  if (!cell_widths(L, w)) return false;
  const double* a = L;
  const double* b = L + 3;
  const double* c = L + 6;
  const double bc[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
  const double ca[3] = {c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]};
  const double ab[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const double det = (a[0] * bc[0] + a[1] * bc[1]) + a[2] * bc[2];
  for (int x = 0; x < 3; ++x) {
    Bm[x] = (kSqTwoPi * bc[x]) / det;
    Bm[3 + x] = (kSqTwoPi * ca[x]) / det;
    Bm[6 + x] = (kSqTwoPi * ab[x]) / det;
  }
  return true;
}

// largest index each axis needs: floor(q_max |a_i| / 2 pi); false where one exceeds kSqMaxIndex (or is not finite)
EGNN_HD bool sq_index_need(const double* L, double q_max, int* need) {
  for (int i = 0; i < 3; ++i) {
    const double v = floor((q_max * sqrt(cell_norm2(L + 3 * i))) / kSqTwoPi);
    if (!(v <= (double)kSqMaxIndex)) return false;
    need[i] = (int)v;
  }
  return true;
}
EGNN_HD int sq_index_box(int need) { return need + 1 < kSqMaxIndex ? need + 1 : kSqMaxIndex; }

EGNN_HD bool sq_half_space(int h, int k, int l) { return h > 0 || (h == 0 && (k > 0 || (k == 0 && l > 0))); }

EGNN_HD double sq_k2(int h, int k, int l, const double* Bm) {
  double kv[3];
  for (int x = 0; x < 3; ++x) kv[x] = ((double)h * Bm[x] + (double)k * Bm[3 + x]) + (double)l * Bm[6 + x];
  return (kv[0] * kv[0] + kv[1] * kv[1]) + kv[2] * kv[2];
}

EGNN_HD bool sq_is_vector(int h, int k, int l, const double* Bm, double q_max, double* k2) {
  *k2 = sq_k2(h, k, l, Bm);
  return sq_half_space(h, k, l) && *k2 < q_max * q_max;
}

EGNN_HD int sq_nbins(double q_max, double dq) {
  const double n = ceil(q_max / dq);
  return n >= 1.0 && n <= 1e9 ? (int)n : -1;
}

EGNN_HD int sq_bin(double kabs, double dq, int nbins) {
  const int n = (int)floor(kabs / dq);
  return n < nbins ? n : nbins - 1;
}

// sine and cosine of 2 pi t, t = the phase mod 1
EGNN_HD double sq_phase(int h, int k, int l, const double* w) {
  const double t = ((double)h * w[0] + (double)k * w[1]) + (double)l * w[2];
  return t - floor(t);
}
EGNN_HD void sq_phase_sincos(double t, double* s, double* c) {
#if defined(__HIP_DEVICE_COMPILE__)
  sincospi(2.0 * t, s, c);   // 2 t is exact and the argument reduction of sincospi is exact
#else
  const double x = kSqTwoPi * t;
  *s = sin(x);
  *c = cos(x);
#endif
}

// rows of the index box of one cell: (h, k) with 0 <= h <= H, |k| <= K; row = h (2K + 1) + (k + K)
EGNN_HD int sq_box_rows(int H, int K) { return (H + 1) * (2 * K + 1); }

// vectors of row (h, k): the l in [-Lb, Lb] that pass sq_is_vector, ascending; `emit` is called for each
template <typename F>
EGNN_HD int sq_row_vectors(int h, int k, int Lb, const double* Bm, double q_max, F emit) {
  int n = 0;
  for (int l = -Lb; l <= Lb; ++l) {
    double k2;
    if (sq_is_vector(h, k, l, Bm, q_max, &k2)) {
      emit(n, l, k2);
      ++n;
    }
  }
  return n;
}

}  // namespace egnn

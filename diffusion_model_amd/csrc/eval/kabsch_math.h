// 3x3 numerics of the RMSD evaluation (kabsch.hip), in fp64.  Plain C++ behind a host/device macro so that the same text can be
// compiled and checked on a CPU.
//
//  * kabsch_fit: the rotation of the three Kabsch spellings of the reference from H = p^T q (H[r][c] = sum_i p_i[r] q_i[c]),
//    by a one-sided (Hestenes) Jacobi SVD H V = U S, which keeps the small singular direction at full relative accuracy
//    (no H^T H).  With V right-handed and U' = [u1, u2, u1 x u2]:
//      flip row    (Vt[-1, :] *= -1, the textbook fix):  R = V U'^T            -- the optimal proper rotation, whatever det H
//      flip column (Vt[:, -1] *= -1):                    R = diag(1,1,-1) V U^T -- the polar factor with its last ROW negated
//    where U = U' for det H >= 0 and [u1, u2, -u1 x u2] otherwise.  Rank-deficient H (|s3| <= 1e-12 s1: two atoms, three atoms
//    about their centroid, planar sets) has no defined reflection sign: both flips return the optimal proper rotation there, and
//    missing singular directions are completed by a fixed rule (the coordinate axis least aligned with u1).
//  * kabsch_trace: the trace s1 + s2 + sign(det H) s3 of the optimal proper rotation = the largest eigenvalue of Horn's 4x4
//    matrix, the largest root of  x^4 - 2 |H|_F^2 x^2 - 8 det(H) x + (2 tr((H^T H)^2) - |H|_F^4),  by Newton's iteration from
//    the upper bound sqrt(3) |H|_F.  All roots are real, so the iterates fall monotonically onto the largest root: every
//    iterate is itself an upper bound and the caller may stop as soon as one drops below the score it has to beat.
//  * kabsch_fit_backward: the derivative of kabsch_fit, dL/dH from dL/dR, from the same factors (for the RMSD loss).
#pragma once
#include "eval_math.h"

namespace egnn {

constexpr int kKabschCentroid = 0, kKabschFirst = 1;   // center
constexpr int kKabschFlipRow = 0, kKabschFlipColumn = 1;

EGNN_HD void kabsch_jacobi_pair(double* A, double* V, int p, int q, bool& rotated) {
  double alpha = 0.0, beta = 0.0, gamma = 0.0;
  for (int r = 0; r < 3; ++r) {
    alpha += A[3 * r + p] * A[3 * r + p];
    beta += A[3 * r + q] * A[3 * r + q];
    gamma += A[3 * r + p] * A[3 * r + q];
  }
  if (gamma == 0.0 || gamma * gamma <= 1e-32 * alpha * beta) return;
  rotated = true;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
  for (int r = 0; r < 3; ++r) {
    const double ap = A[3 * r + p], aq = A[3 * r + q];
    A[3 * r + p] = c * ap - s * aq;
    A[3 * r + q] = s * ap + c * aq;
    const double vp = V[3 * r + p], vq = V[3 * r + q];
    V[3 * r + p] = c * vp - s * vq;
    V[3 * r + q] = s * vp + c * vq;
  }
}

EGNN_HD void kabsch_swap_cols(double* A, double* V, double* s, int i, int j) {
  if (s[i] >= s[j]) return;
  double t = s[i]; s[i] = s[j]; s[j] = t;
  for (int r = 0; r < 3; ++r) {
    t = A[3 * r + i]; A[3 * r + i] = A[3 * r + j]; A[3 * r + j] = t;
    t = V[3 * r + i]; V[3 * r + i] = V[3 * r + j]; V[3 * r + j] = t;
  }
}

// The factors kabsch_fit forms on its way to R:  H = U diag(s) V^T  with V and U = [u1, u2, u1 x u2] both right-handed, s[0] >=
// s[1] >= 0 and s[2] SIGNED (sign(det H) sigma_3), and  R = J V J U^T  with J = diag(1, 1, w3): w3 = -1 in a column-flip
// reflection case, else 1.  H = 0 leaves s = 0, U = V = I, w3 = 1.
struct KabschFactors {
  double V[9], U[9];   // row-major; the singular vectors are the COLUMNS
  double s[3];
  double w3;
};

// R [9] row-major such that R p_i ~ q_i, and the factors it was formed from
EGNN_HD void kabsch_fit_factors(const double* H, int flip, double* R, KabschFactors& F) {
  double A[9], V[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  for (int k = 0; k < 9; ++k) A[k] = H[k];
  for (int sweep = 0; sweep < 16; ++sweep) {
    bool rotated = false;
    kabsch_jacobi_pair(A, V, 0, 1, rotated);
    kabsch_jacobi_pair(A, V, 0, 2, rotated);
    kabsch_jacobi_pair(A, V, 1, 2, rotated);
    if (!rotated) break;
  }
  double s[3];
  for (int j = 0; j < 3; ++j) s[j] = sqrt(A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j]);
  kabsch_swap_cols(A, V, s, 0, 1);
  kabsch_swap_cols(A, V, s, 1, 2);
  kabsch_swap_cols(A, V, s, 0, 1);
  const double detV = V[0] * (V[4] * V[8] - V[5] * V[7]) - V[1] * (V[3] * V[8] - V[5] * V[6]) + V[2] * (V[3] * V[7] - V[4] * V[6]);
  if (detV < 0.0)
    for (int r = 0; r < 3; ++r) { V[3 * r + 2] = -V[3 * r + 2]; A[3 * r + 2] = -A[3 * r + 2]; }
  if (!(s[0] > 0.0)) {   // H = 0: nothing to align
    for (int k = 0; k < 9; ++k) R[k] = F.V[k] = F.U[k] = (k % 4 == 0) ? 1.0 : 0.0;
    F.s[0] = F.s[1] = F.s[2] = 0.0;
    F.w3 = 1.0;
    return;
  }
  double u1[3], u2[3], u3[3];
  for (int r = 0; r < 3; ++r) u1[r] = A[3 * r] / s[0];
  double d = A[1] * u1[0] + A[4] * u1[1] + A[7] * u1[2];
  for (int r = 0; r < 3; ++r) u2[r] = A[3 * r + 1] - d * u1[r];
  double nw = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
  if (!(nw > 1e-14 * s[0])) {   // rank one: complete with the axis least aligned with u1
    const double a0 = fabs(u1[0]), a1 = fabs(u1[1]), a2 = fabs(u1[2]);
    const int k = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
    for (int r = 0; r < 3; ++r) u2[r] = (r == k ? 1.0 : 0.0) - u1[k] * u1[r];
    nw = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
  }
  for (int r = 0; r < 3; ++r) u2[r] /= nw;
  u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
  u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
  u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
  const double s3 = A[2] * u3[0] + A[5] * u3[1] + A[8] * u3[2];   // signed: sign(det H) * sigma_3
  const bool reflect_column = flip == kKabschFlipColumn && s3 < 0.0 && fabs(s3) > 1e-12 * s[0];
  const double w3 = reflect_column ? -1.0 : 1.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R[3 * r + c] = V[3 * r] * u1[c] + V[3 * r + 1] * u2[c] + w3 * (V[3 * r + 2] * u3[c]);
  if (reflect_column)
    for (int c = 0; c < 3; ++c) R[6 + c] = -R[6 + c];
  for (int k = 0; k < 9; ++k) F.V[k] = V[k];
  for (int r = 0; r < 3; ++r) { F.U[3 * r] = u1[r]; F.U[3 * r + 1] = u2[r]; F.U[3 * r + 2] = u3[r]; }
  F.s[0] = s[0]; F.s[1] = s[1]; F.s[2] = s3;
  F.w3 = w3;
}

// R [9] row-major such that R p_i ~ q_i
EGNN_HD void kabsch_fit(const double* H, int flip, double* R) {
  KabschFactors F;
  kabsch_fit_factors(H, flip, R, F);
}

// Hbar = dL/dH [9] of L(R(H)) from Rbar = dL/dR [9].  With dU = U Wu, dV = V Wv (Wu, Wv antisymmetric) and dA = U^T dH V,
//   dA_ij = Wu_ij s_j - s_i Wv_ij  (i != j),   dR = J V (Wv J - J Wu) U^T,
// which solved for (Wv J - J Wu)_ij = a_ij dA_ij + b_ij dA_ji gives, with K = V^T J Rbar U and j = diag(J),
//   Abar_ij = -K_ij / (j_j s_i + j_i s_j) + K_ji / (j_i s_i + j_j s_j),   Abar_ii = 0,   Hbar = U Abar V^T.
// No 1 / (s_i^2 - s_j^2): the denominators are s_i + s_j, which with the signed s[2] is sigma_i - sigma_3 in a row-flip reflection
// case.  A term whose denominator is at most 1e-12 s[0] in magnitude is dropped (kabsch_fit's rank threshold: the forward
// completes that direction by a fixed rule, which is locally constant), so the result is finite for every H.
EGNN_HD void kabsch_fit_backward_factors(const KabschFactors& F, const double* Rbar, double* Hbar) {
  const double j[3] = {1.0, 1.0, F.w3};
  double T[9], K[9], M[9];
  for (int i = 0; i < 3; ++i)     // T = V^T J Rbar
    for (int c = 0; c < 3; ++c) T[3 * i + c] = F.V[i] * Rbar[c] + F.V[3 + i] * Rbar[3 + c] + F.w3 * (F.V[6 + i] * Rbar[6 + c]);
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) K[3 * i + k] = T[3 * i] * F.U[k] + T[3 * i + 1] * F.U[3 + k] + T[3 * i + 2] * F.U[6 + k];
  const double tiny = 1e-12 * F.s[0];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) {
      double m = 0.0;
      if (i != k) {
        const double den1 = j[k] * F.s[i] + j[i] * F.s[k], den2 = j[i] * F.s[i] + j[k] * F.s[k];
        if (fabs(den1) > tiny) m -= K[3 * i + k] / den1;
        if (fabs(den2) > tiny) m += K[3 * k + i] / den2;
      }
      M[3 * i + k] = m;
    }
  for (int r = 0; r < 3; ++r)     // T = U Abar
    for (int k = 0; k < 3; ++k) T[3 * r + k] = F.U[3 * r] * M[k] + F.U[3 * r + 1] * M[3 + k] + F.U[3 * r + 2] * M[6 + k];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Hbar[3 * r + c] = T[3 * r] * F.V[3 * c] + T[3 * r + 1] * F.V[3 * c + 1] + T[3 * r + 2] * F.V[3 * c + 2];
}

EGNN_HD void kabsch_fit_backward(const double* H, int flip, const double* Rbar, double* Hbar) {
  double R[9];
  KabschFactors F;
  kabsch_fit_factors(H, flip, R, F);
  kabsch_fit_backward_factors(F, Rbar, Hbar);
}

// -> the largest eigenvalue of Horn's matrix of H, or -1 as soon as an iterate (an upper bound of it) is below `beat`
EGNN_HD double kabsch_trace(const double* H, double beat) {
  double a = 0.0;
  for (int k = 0; k < 9; ++k) a += H[k] * H[k];
  double x = sqrt(3.0 * a) * (1.0 + 1e-15);
  if (x < beat) return -1.0;
  const double det = H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6]) + H[2] * (H[3] * H[7] - H[4] * H[6]);
  const double g00 = H[0] * H[0] + H[3] * H[3] + H[6] * H[6], g11 = H[1] * H[1] + H[4] * H[4] + H[7] * H[7],
               g22 = H[2] * H[2] + H[5] * H[5] + H[8] * H[8], g01 = H[0] * H[1] + H[3] * H[4] + H[6] * H[7],
               g02 = H[0] * H[2] + H[3] * H[5] + H[6] * H[8], g12 = H[1] * H[2] + H[4] * H[5] + H[7] * H[8];
  const double trg2 = g00 * g00 + g11 * g11 + g22 * g22 + 2.0 * (g01 * g01 + g02 * g02 + g12 * g12);
  const double c2 = -2.0 * a, c1 = -8.0 * det, c0 = 2.0 * trg2 - a * a;
  for (int it = 0; it < 48; ++it) {
    const double x2 = x * x;
    const double P = ((x2 + c2) * x + c1) * x + c0;
    const double dP = (4.0 * x2 + 2.0 * c2) * x + c1;
    if (!(dP > 0.0)) break;
    const double xn = x - P / dP;
    if (!(xn < x)) break;
    const bool done = x - xn <= 4e-16 * x;
    x = xn;
    if (done) break;
    if (x < beat) return -1.0;
  }
  return x;
}

}  // namespace egnn

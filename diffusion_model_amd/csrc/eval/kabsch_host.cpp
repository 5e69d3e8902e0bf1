// Host statement of the gradient of the Kabsch fit (kabsch_backward_kernel of kabsch.hip), one pair, all in double.  Plain C++
// over the 3x3 numerics the kernel uses (kabsch_math.h): no HIP call, no device code, so the mathematics can be checked -- and
// run under the sanitizers (make asan) -- on a machine without a GPU.
#include <vector>

#include "../host_logic.h"
#include "kabsch_math.h"

using namespace egnn;

extern "C" {

int egnn_kabsch_grad_host(int n, const double* P, const double* Q, int center, int flip, const double* g_R, const double* g_t,
                          double g_rmsd, double* dP, double* dQ) {
  if (n < 1 || !P || !Q || !dP || (center != kKabschCentroid && center != kKabschFirst) ||
      (flip != kKabschFlipRow && flip != kKabschFlipColumn)) {
    set_error("bad egnn_kabsch_grad_host arguments (n >= 1, P, Q and dP given, center 0 / 1, flip 0 / 1)");
    return EGNN_EINVAL;
  }
  if (n == 1) {   // one atom: R = I and rmsd = 0 whatever the coordinates; no gradient is defined, zero is returned
    for (int d = 0; d < 3; ++d) {
      dP[d] = 0.0;
      if (dQ) dQ[d] = 0.0;
    }
    return EGNN_OK;
  }
  double cp[3] = {0.0, 0.0, 0.0}, cq[3] = {0.0, 0.0, 0.0};
  if (center == kKabschCentroid) {
    for (int i = 0; i < n; ++i)
      for (int d = 0; d < 3; ++d) { cp[d] += P[3 * i + d]; cq[d] += Q[3 * i + d]; }
    for (int d = 0; d < 3; ++d) { cp[d] /= (double)n; cq[d] /= (double)n; }
  } else {
    for (int d = 0; d < 3; ++d) { cp[d] = P[d]; cq[d] = Q[d]; }
  }
  std::vector<double> p(3 * (size_t)n), q(3 * (size_t)n);
  double H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < n; ++i) {
    for (int d = 0; d < 3; ++d) { p[3 * i + d] = P[3 * i + d] - cp[d]; q[3 * i + d] = Q[3 * i + d] - cq[d]; }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) H[3 * r + c] += p[3 * i + r] * q[3 * i + c];
  }
  double R[9];
  KabschFactors F;
  kabsch_fit_factors(H, flip, R, F);
  // residual, sum e p^T, sum p, sum q
  double res = 0.0, E[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, sp[3] = {0.0, 0.0, 0.0}, sq[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < n; ++i) {
    const double* pi = &p[3 * i];
    for (int r = 0; r < 3; ++r) {
      const double e = (R[3 * r] * pi[0] + R[3 * r + 1] * pi[1] + R[3 * r + 2] * pi[2]) - q[3 * i + r];
      res += e * e;
      for (int c = 0; c < 3; ++c) E[3 * r + c] += e * pi[c];
      sp[r] += pi[r];
      sq[r] += q[3 * i + r];
    }
  }
  const double rmsd = sqrt(res / (double)n);
  const double c = rmsd > 0.0 ? g_rmsd / ((double)n * rmsd) : 0.0;
  double Rbar[9], Hbar[9];
  for (int k = 0; k < 9; ++k) Rbar[k] = (g_R ? g_R[k] : 0.0) + c * E[k];
  kabsch_fit_backward_factors(F, Rbar, Hbar);
  double gt[3];
  for (int d = 0; d < 3; ++d) gt[d] = g_t ? g_t[d] : 0.0;
  // sum of pbar_i = c R^T e_i + Hbar q_i and of qbar_i = -c e_i + Hbar^T p_i, with sum e = R sum p - sum q
  double se[3], mp[3], mq[3];
  for (int r = 0; r < 3; ++r) se[r] = (R[3 * r] * sp[0] + R[3 * r + 1] * sp[1] + R[3 * r + 2] * sp[2]) - sq[r];
  for (int d = 0; d < 3; ++d) {
    mp[d] = c * (R[d] * se[0] + R[3 + d] * se[1] + R[6 + d] * se[2]) + (Hbar[3 * d] * sq[0] + Hbar[3 * d + 1] * sq[1] + Hbar[3 * d + 2] * sq[2]) + gt[d];
    mq[d] = -c * se[d] + (Hbar[d] * sp[0] + Hbar[3 + d] * sp[1] + Hbar[6 + d] * sp[2]) - gt[d];
    if (center == kKabschCentroid) { mp[d] /= (double)n; mq[d] /= (double)n; }
  }
  for (int i = 0; i < n; ++i) {
    const double *pi = &p[3 * i], *qi = &q[3 * i];
    double e[3];
    for (int r = 0; r < 3; ++r) e[r] = (R[3 * r] * pi[0] + R[3 * r + 1] * pi[1] + R[3 * r + 2] * pi[2]) - qi[r];
    const bool takes_mean = center == kKabschCentroid || i == 0;
    for (int d = 0; d < 3; ++d) {
      const double pb = c * (R[d] * e[0] + R[3 + d] * e[1] + R[6 + d] * e[2]) + (Hbar[3 * d] * qi[0] + Hbar[3 * d + 1] * qi[1] + Hbar[3 * d + 2] * qi[2]);
      const double qb = -c * e[d] + (Hbar[d] * pi[0] + Hbar[3 + d] * pi[1] + Hbar[6 + d] * pi[2]);
      dP[3 * i + d] = takes_mean ? pb - mp[d] : pb;
      if (dQ) dQ[3 * i + d] = takes_mean ? qb - mq[d] : qb;
    }
  }
  return EGNN_OK;
}

}  // extern "C"

// Host side of the SOAP entries: the argument checks of the device entries (soap.hip) and the host statement egnn_soap_host --
// descriptors, cosines, the cosine matrix and the nearest spectra computed on the CPU through soap_math.h, the text the kernels
// compile.  No HIP call, no device code: checked (and run under the sanitizers) on a machine without a GPU.
#include <string.h>

#include <memory>

#include "soap_host.h"
#include "soap_math.h"

namespace egnn {

int soap_descriptor_check(const char* who, int B, int N, int A, const void* pos, const void* type, const void* graph_ptr, int n_max,
                          int l_max, double neighbour_cut, const void* tables, int n_centres, const int32_t* centres, const void* desc) {
  if (B < 1 || N < 1 || n_centres < 1 || !pos || !type || !graph_ptr || !tables || !centres || !desc) {
    set_error("bad %s arguments (B, N, n_centres >= 1; pos, type, graph_ptr, tables, centres and desc given)", who);
    return EGNN_EINVAL;
  }
  if (int rc = atom_types_check(who, A, kSoapMaxTypes)) return rc;
  if (n_max < 1 || n_max > kSoapMaxN) { set_error("%s: n_max %d (1 <= n_max <= %d)", who, n_max, kSoapMaxN); return EGNN_EINVAL; }
  if (l_max < 0 || l_max > kSoapMaxL) { set_error("%s: l_max %d (0 <= l_max <= %d)", who, l_max, kSoapMaxL); return EGNN_EINVAL; }
  if (!soap_cut_ok(neighbour_cut)) { set_error("%s: neighbour_cut must be positive and finite", who); return EGNN_EINVAL; }
  if ((long long)n_centres * soap_feature_count(A, n_max, l_max) > 2147483647LL * 4) {
    set_error("%s: %d centres of %d features (at most 2^33 values a call)", who, n_centres, soap_feature_count(A, n_max, l_max));
    return EGNN_EINVAL;
  }
  for (int c = 0; c < n_centres; ++c)
    if (centres[c] < 0 || centres[c] >= N) {
      set_error("%s: centre %d is atom %d outside [0, %d)", who, c, centres[c], N);
      return EGNN_EINVAL;
    }
  return EGNN_OK;
}

int soap_rows_check(const char* who, int F, const void* a, int rows_a, const void* b, int rows_b) {
  if (F < 1 || rows_a < 1 || rows_b < 1 || !a || !b) {
    set_error("bad %s arguments (F, rows_a, rows_b >= 1; both matrices given)", who);
    return EGNN_EINVAL;
  }
  return EGNN_OK;
}

int soap_nearest_check(const char* who, int T, int R, int S, int k, const void* target, const void* reference, const void* idx,
                       const void* mse) {
  if (T < 1 || R < 1 || S < 1 || !target || !reference || !idx || !mse) {
    set_error("bad %s arguments (T, R, S >= 1; target, reference, idx and mse given)", who);
    return EGNN_EINVAL;
  }
  if (k < 1 || k > kSoapMaxK) { set_error("%s: k %d (1 <= k <= %d)", who, k, kSoapMaxK); return EGNN_EINVAL; }
  return EGNN_OK;
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_soap_features(int A, int n_max, int l_max) {
  if (!soap_config_ok(A, n_max, l_max)) {
    set_error("egnn_soap_features: A %d, n_max %d, l_max %d (A <= %d, 1 <= n_max <= %d, 0 <= l_max <= %d)", A, n_max, l_max, kSoapMaxTypes,
              kSoapMaxN, kSoapMaxL);
    return EGNN_EINVAL;
  }
  return soap_feature_count(A, n_max, l_max);
}

int egnn_soap_table_doubles(int n_max, int l_max) {
  if (!soap_config_ok(1, n_max, l_max)) {
    set_error("egnn_soap_table_doubles: n_max %d, l_max %d (1 <= n_max <= %d, 0 <= l_max <= %d)", n_max, l_max, kSoapMaxN, kSoapMaxL);
    return EGNN_EINVAL;
  }
  return soap_table_count(n_max, l_max);
}

int egnn_soap_host(int B, int N, int A, const float* pos, const int32_t* type, const int32_t* graph_ptr, int n_max, int l_max,
                   double neighbour_cut, const double* tables, int n_centres, const int32_t* centres, double* desc, double* coeff, int F,
                   const double* rows_a, int n_a, const double* rows_b, int n_b, int n_pairs, const int32_t* pairs, double* cosine,
                   double* gram, int T, int R, int S, int k, const float* target, const float* reference, const int32_t* target_group,
                   const int32_t* reference_group, int32_t* idx, double* mse) {
  const char* who = "egnn_soap_host";
  if (n_centres < 0 || n_pairs < 0 || T < 0) { set_error("bad %s arguments (n_centres, n_pairs, T >= 0)", who); return EGNN_EINVAL; }

  if (n_centres > 0) {   // ---- descriptors --------------------------------------------------------------------------------------
    if (int rc = soap_descriptor_check(who, B, N, A, pos, type, graph_ptr, n_max, l_max, neighbour_cut, tables, n_centres, centres, desc))
      return rc;
    for (int g = 0; g < B; ++g) {
      const int lo = graph_ptr[g], hi = graph_ptr[g + 1];
      if (lo < 0 || hi < lo || hi > N || (g == 0 && lo != 0) || (g == B - 1 && hi != N)) {
        set_error("%s: graph_ptr must start at 0, not decrease and end at N", who);
        return EGNN_EINVAL;
      }
    }
    if (int rc = type_range_check(who, type, 0, N, A)) return rc;
    const int L1 = l_max + 1, LM = soap_lm_count(l_max), nF = soap_feature_count(A, n_max, l_max);
    const double cut2 = neighbour_cut * neighbour_cut;
    const double* norm = tables + soap_table_norm(n_max, l_max);
    const double* beta = tables + soap_table_beta(n_max, l_max);
    // (plain arrays: a std::vector constructor that is not inlined would be exported from the library)
    const size_t nC = (size_t)A * n_max * LM;
    const std::unique_ptr<double[]> prim_(new double[nC]), c_(new double[nC]), solid_(new double[LM]), radial_(new double[(size_t)n_max * L1]);
    double *prim = prim_.get(), *c = c_.get(), *solid = solid_.get(), *radial = radial_.get();
    for (int ci = 0; ci < n_centres; ++ci) {
      const int i = centres[ci];
      int g = 0;
      while (graph_ptr[g + 1] <= i) ++g;   // the graph of atom i (empty graphs skipped)
      for (size_t o = 0; o < nC; ++o) prim[o] = 0.0;
      for (int j = graph_ptr[g]; j < graph_ptr[g + 1]; ++j) {
        double dx, dy, dz;
        const double d2 = soap_dist2(pos + 3 * (size_t)i, pos + 3 * (size_t)j, &dx, &dy, &dz);
        if (!(d2 < cut2)) continue;
        for (int m = 0; m <= l_max; ++m) soap_solid_column(dx, dy, dz, d2, m, l_max, norm, solid);
        for (int q = 0; q < n_max * L1; ++q) radial[q] = soap_radial(tables, n_max, l_max, q, d2);
        double* pz = prim + (size_t)type[j] * n_max * LM;
        for (int n = 0; n < n_max; ++n)
          for (int lm = 0; lm < LM; ++lm) pz[n * LM + lm] += radial[n * L1 + soap_l_of(lm)] * solid[lm];
      }
      for (int z = 0; z < A; ++z)
        for (int lm = 0; lm < LM; ++lm) {
          const double* bl = beta + (size_t)soap_l_of(lm) * n_max * n_max;
          for (int n = 0; n < n_max; ++n) {
            double sum = 0.0;
            for (int np = 0; np < n_max; ++np) sum += bl[n * n_max + np] * prim[((size_t)z * n_max + np) * LM + lm];
            c[((size_t)z * n_max + n) * LM + lm] = sum;
          }
        }
      if (coeff) memcpy(coeff + (size_t)ci * nC, c, sizeof(double) * nC);
      for (int f = 0; f < nF; ++f) desc[(size_t)ci * nF + f] = soap_power_entry(c, tables, f, A, n_max, l_max);
    }
  }

  if (n_pairs > 0 || gram) {   // ---- cosines of rows --------------------------------------------------------------------------
    if (int rc = soap_rows_check(who, F, rows_a, n_a, rows_b, n_b)) return rc;
    if (n_pairs > 0 && !cosine) { set_error("bad %s arguments (cosine given with n_pairs)", who); return EGNN_EINVAL; }
    for (int p = 0; p < n_pairs; ++p) {
      const int ra = pairs ? pairs[2 * p] : p, rb = pairs ? pairs[2 * p + 1] : p;
      if (ra < 0 || ra >= n_a || rb < 0 || rb >= n_b) { set_error("%s: pair %d names a row outside the matrices", who, p); return EGNN_EINVAL; }
    }
    const std::unique_ptr<double[]> na(new double[n_a]), nb(new double[n_b]);
    for (int r = 0; r < n_a; ++r) na[r] = soap_row_dot(rows_a + (size_t)r * F, rows_a + (size_t)r * F, F);
    for (int r = 0; r < n_b; ++r) nb[r] = soap_row_dot(rows_b + (size_t)r * F, rows_b + (size_t)r * F, F);
    for (int p = 0; p < n_pairs; ++p) {
      const int ra = pairs ? pairs[2 * p] : p, rb = pairs ? pairs[2 * p + 1] : p;
      cosine[p] = soap_cosine(soap_row_dot(rows_a + (size_t)ra * F, rows_b + (size_t)rb * F, F), na[ra], nb[rb]);
    }
    if (gram)
      for (int ra = 0; ra < n_a; ++ra)
        for (int rb = 0; rb < n_b; ++rb)
          gram[(size_t)ra * n_b + rb] = soap_cosine(soap_row_dot(rows_a + (size_t)ra * F, rows_b + (size_t)rb * F, F), na[ra], nb[rb]);
  }

  if (T > 0) {   // ---- nearest spectra --------------------------------------------------------------------------------------------
    if (int rc = soap_nearest_check(who, T, R, S, k, target, reference, idx, mse)) return rc;
    for (int t = 0; t < T; ++t) {
      SoapBest best;
      soap_best_clear(&best);
      for (int r = 0; r < R; ++r) {
        if (target_group && reference_group && soap_excluded(target_group[t], reference_group[r])) continue;
        soap_best_insert(&best, soap_row_mse(target + (size_t)t * S, reference + (size_t)r * S, S), r);
      }
      for (int q = 0; q < k; ++q) { idx[(size_t)t * k + q] = best.idx[q]; mse[(size_t)t * k + q] = best.mse[q]; }
    }
  }
  return EGNN_OK;
}

}  // extern "C"

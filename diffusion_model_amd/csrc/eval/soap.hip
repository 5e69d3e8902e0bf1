// SOAP power spectra of chosen centres, their cosine similarities and the nearest-spectrum search on the device.  Definitions:
// soap_math.h (shared with the host statement, soap_host.cpp).  Restates template_matching.py:41-68, which goes through ASE and
// dscribe one pair of records at a time and recomputes every descriptor inside its loop.
//
// No kernel has an atomic: every output is the sum of one thread (or of one wavefront's fixed butterfly), so a repeated call is
// bitwise reproducible.  A kernel trusts no entry it reads: a centre is checked against N, its graph against N, a type against
// A, a pair against the row counts.
#include "soap_device.h"
#include "soap_host.h"
#include "soap_math.h"

namespace egnn {

constexpr int kSoapGramA = 4;         // rows of a in one tile of the cosine matrix: one per wavefront
constexpr int kSoapGramB = 8;         // rows of b in one tile: eight running sums per lane

// ---- descriptor: one workgroup of 16 wavefronts per centre ---------------------------------------------------------------------
// The graph's atoms are staged 32 at a time: one thread per atom takes the difference, d2 and the cut decision; then the
// workgroup's threads share the 32 (l_max+1) harmonic columns (soap_solid_column: one m, all l) and the 32 n_max (l_max+1) radial
// values (the only exp calls); then every thread adds the chunk's atoms, ascending, to the (n, l, m) outputs it owns, one running
// sum per species in registers.  After the last chunk a thread per (species, l, m) column applies beta over n in place, and the
// power-spectrum phase writes the row with l innermost across threads: contiguous.
//
// LDS at the limits (A = 4, n_max = 16, l_max = 10): 62 KB of coefficients + 31 KB + 44 KB + 1 KB of staging = 136 KiB of a CU's
// 160 KiB, requested as dynamic LDS by the entry; at the defaults and A = 2 it is 100 KiB.
__global__ __launch_bounds__(kSoapThreads) void soap_descriptor_kernel(const float* __restrict__ pos, const int* __restrict__ type,
                                                                       const int* __restrict__ graph_ptr, int B, int N, int A, int n_max,
                                                                       int l_max, double cut2, const double* __restrict__ tables,
                                                                       const int* __restrict__ centres, int n_centres,
                                                                       double* __restrict__ desc, double* __restrict__ coeff) {
  extern __shared__ double s_soap[];
  __shared__ int s_range[2];
  const int tid = threadIdx.x, ci = blockIdx.x;
  if (ci >= n_centres) return;
  const int LM = soap_lm_count(l_max), nC = A * n_max * LM, F = soap_feature_count(A, n_max, l_max);
  const SoapLds s = soap_lds_carve(s_soap, A, n_max, l_max);
  const int i = centres[ci];
  if (tid == 0) {   // the graph of atom i: the last g with graph_ptr[g] <= i
    int lo = -1, hi = -1;
    if (i >= 0 && i < N) {
      int a = 0, b = B;   // graph_ptr[a] <= i < graph_ptr[b] is the aim
      while (b - a > 1) {
        const int mid = (a + b) / 2;
        if (graph_ptr[mid] <= i) a = mid; else b = mid;
      }
      lo = graph_ptr[a];
      hi = graph_ptr[a + 1];
      if (lo < 0 || hi > N || i < lo || i >= hi) lo = hi = -1;
    }
    s_range[0] = lo;
    s_range[1] = hi;
  }
  for (int o = tid; o < nC; o += kSoapThreads) s.c[o] = 0.0;
  __syncthreads();
  const int lo = s_range[0], hi = s_range[1];
  double* row = desc + (size_t)ci * F;
  double* coeff_row = coeff ? coeff + (size_t)ci * nC : nullptr;
  if (lo < 0) {   // no such atom or no such graph: a row of zeros, which no descriptor is
    soap_zero_row(A, n_max, l_max, row, coeff_row, tid);
    return;
  }
  for (int j0 = lo; j0 < hi; j0 += kSoapChunk) {   // uniform in the workgroup
    const int cnt = min(kSoapChunk, hi - j0);
    if (tid < cnt) {
      const int j = j0 + tid, tj = type[j];
      double dx, dy, dz;
      const double d2 = soap_dist2(pos + 3 * (size_t)i, pos + 3 * (size_t)j, &dx, &dy, &dz);
      s.xyz[4 * tid] = dx; s.xyz[4 * tid + 1] = dy; s.xyz[4 * tid + 2] = dz; s.xyz[4 * tid + 3] = d2;
      s.species[tid] = (d2 < cut2 && tj >= 0 && tj < A) ? tj : -1;
    }
    soap_chunk_accumulate(s, cnt, A, n_max, l_max, tables, tid);   // soap_device.h: shared with cells/cell_soap.hip
  }
  soap_finish(s, A, n_max, l_max, tables, row, coeff_row, tid);
}

// ---- cosine of listed pairs of rows: one wavefront per pair -------------------------------------------------------------------
__global__ __launch_bounds__(256) void soap_cosine_kernel(const double* __restrict__ a, int rows_a, const double* __restrict__ b,
                                                          int rows_b, const int* __restrict__ pairs, int n_pairs, int F,
                                                          double* __restrict__ out) {
  const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= n_pairs) return;
  const int ra = pairs ? pairs[2 * p] : p, rb = pairs ? pairs[2 * p + 1] : p;
  if (ra < 0 || ra >= rows_a || rb < 0 || rb >= rows_b) {   // no such row: no similarity
    if (lane == 0) out[p] = __builtin_nan("");
    return;
  }
  const double* x = a + (size_t)ra * F;
  const double* y = b + (size_t)rb * F;
  double dot = 0.0, na = 0.0, nb = 0.0;
  for (int f = lane; f < F; f += 64) {
    const double u = x[f], v = y[f];
    dot += u * v;
    na += u * u;
    nb += v * v;
  }
  dot = wave_sum(dot);
  na = wave_sum(na);
  nb = wave_sum(nb);
  if (lane == 0) out[p] = soap_cosine(dot, na, nb);
}

// ---- squared norms of the rows of a matrix: one wavefront per row ---------------------------------------------------------------
__global__ __launch_bounds__(256) void soap_norm_kernel(const double* __restrict__ a, int rows, int F, double* __restrict__ out) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const double* x = a + (size_t)r * F;
  double na = 0.0;
  for (int f = lane; f < F; f += 64) na += x[f] * x[f];
  na = wave_sum(na);
  if (lane == 0) out[r] = na;
}

// ---- the cosine matrix: tile (4 rows of a) x (8 rows of b); wavefront w holds one row of a, a lane its elements f = lane + 64 t
// in turn and eight running sums, one per row of b: each dot product is the row sum of soap_math.h, the one soap_cosine_kernel
// takes, so the two entries agree bitwise ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void soap_gram_kernel(const double* __restrict__ a, int rows_a, const double* __restrict__ b,
                                                        int rows_b, int F, const double* __restrict__ norm_a,
                                                        const double* __restrict__ norm_b, double* __restrict__ gram) {
  const int lane = threadIdx.x & 63, ra = blockIdx.x * kSoapGramA + (threadIdx.x >> 6), rb0 = blockIdx.y * kSoapGramB;
  if (ra >= rows_a) return;   // uniform in a wavefront; no barrier follows
  const double* x = a + (size_t)ra * F;
  double dot[kSoapGramB];
#pragma unroll
  for (int q = 0; q < kSoapGramB; ++q) dot[q] = 0.0;
  for (int f = lane; f < F; f += 64) {
    const double u = x[f];
#pragma unroll
    for (int q = 0; q < kSoapGramB; ++q)
      if (rb0 + q < rows_b) dot[q] += u * b[(size_t)(rb0 + q) * F + f];
  }
  const double na = norm_a[ra];
#pragma unroll
  for (int q = 0; q < kSoapGramB; ++q) {
    const double d = wave_sum(dot[q]);
    if (lane == 0 && rb0 + q < rows_b) gram[(size_t)ra * rows_b + rb0 + q] = soap_cosine(d, na, norm_b[rb0 + q]);
  }
}

// ---- nearest spectra: one wavefront per target streams the references and keeps the k best in registers ------------------------
__global__ __launch_bounds__(256) void soap_nearest_kernel(const float* __restrict__ target, const float* __restrict__ reference, int T,
                                                           int R, int S, int k, const int* __restrict__ target_group,
                                                           const int* __restrict__ reference_group, int* __restrict__ idx,
                                                           double* __restrict__ mse) {
  const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const float* x = target + (size_t)t * S;
  const bool grouped = target_group && reference_group;
  const int tg = grouped ? target_group[t] : -1;
  SoapBest best;
  soap_best_clear(&best);
  for (int r = 0; r < R; ++r) {   // uniform in a wavefront
    if (grouped && soap_excluded(tg, reference_group[r])) continue;
    const float* y = reference + (size_t)r * S;
    double sum = 0.0;
    for (int s = lane; s < S; s += 64) sum += soap_sq_diff(x[s], y[s]);
    soap_best_insert(&best, wave_sum(sum) / (double)S, r);
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < kSoapMaxK; ++q)
      if (q < k) { idx[(size_t)t * k + q] = best.idx[q]; mse[(size_t)t * k + q] = best.mse[q]; }
  }
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_soap_descriptor(void* stream, int B, int N, int A, const float* d_pos, const int32_t* d_type, const int32_t* d_graph_ptr,
                         int n_max, int l_max, double neighbour_cut, const double* d_tables, int n_centres, const int32_t* centres,
                         const int32_t* d_centres, double* d_desc, double* d_coeff) {
  const char* who = "egnn_soap_descriptor";
  if (int rc = soap_descriptor_check(who, B, N, A, d_pos, d_type, d_graph_ptr, n_max, l_max, neighbour_cut, d_tables, n_centres, centres,
                                     d_desc))
    return rc;
  if (!d_centres) { set_error("bad %s arguments (d_centres given)", who); return EGNN_EINVAL; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // up to 136 KiB of dynamic LDS; a CU has 160 KiB
  static LdsLimitRecord raised;
  if (int rc = raise_lds_limit(raised, &soap_descriptor_kernel, soap_lds_bytes(kSoapMaxTypes, kSoapMaxN, kSoapMaxL))) return rc;
  hipLaunchKernelGGL(soap_descriptor_kernel, dim3(n_centres), dim3(kSoapThreads), soap_lds_bytes(A, n_max, l_max), st, d_pos, d_type,
                     d_graph_ptr, B, N, A, n_max, l_max, neighbour_cut * neighbour_cut, d_tables, d_centres, n_centres, d_desc, d_coeff);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_soap_cosine(void* stream, int n_pairs, int F, const double* d_a, int rows_a, const double* d_b, int rows_b,
                     const int32_t* d_pairs, double* d_cos) {
  const char* who = "egnn_soap_cosine";
  if (int rc = soap_rows_check(who, F, d_a, rows_a, d_b, rows_b)) return rc;
  if (n_pairs < 1 || !d_cos) { set_error("bad %s arguments (n_pairs >= 1; cos given)", who); return EGNN_EINVAL; }
  hipLaunchKernelGGL(soap_cosine_kernel, dim3((n_pairs + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_a, rows_a, d_b,
                     rows_b, d_pairs, n_pairs, F, d_cos);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_soap_gram(void* stream, int F, const double* d_a, int rows_a, const double* d_b, int rows_b, double* d_norms, double* d_gram) {
  const char* who = "egnn_soap_gram";
  if (int rc = soap_rows_check(who, F, d_a, rows_a, d_b, rows_b)) return rc;
  if (!d_norms || !d_gram) { set_error("bad %s arguments (norms and gram given)", who); return EGNN_EINVAL; }
  if (rows_b > 65535 * kSoapGramB) { set_error("%s: %d rows of b (at most %d)", who, rows_b, 65535 * kSoapGramB); return EGNN_EINVAL; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(soap_norm_kernel, dim3((rows_a + 3) / 4), dim3(256), 0, st, d_a, rows_a, F, d_norms);
  hipLaunchKernelGGL(soap_norm_kernel, dim3((rows_b + 3) / 4), dim3(256), 0, st, d_b, rows_b, F, d_norms + rows_a);
  hipLaunchKernelGGL(soap_gram_kernel, dim3((rows_a + kSoapGramA - 1) / kSoapGramA, (rows_b + kSoapGramB - 1) / kSoapGramB), dim3(256), 0,
                     st, d_a, rows_a, d_b, rows_b, F, (const double*)d_norms, (const double*)(d_norms + rows_a), d_gram);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_spectrum_nearest(void* stream, int T, int R, int S, int k, const float* d_target, const float* d_reference,
                          const int32_t* d_target_group, const int32_t* d_reference_group, int32_t* d_idx, double* d_mse) {
  if (int rc = soap_nearest_check("egnn_spectrum_nearest", T, R, S, k, d_target, d_reference, d_idx, d_mse)) return rc;
  hipLaunchKernelGGL(soap_nearest_kernel, dim3((T + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_target, d_reference, T,
                     R, S, k, d_target_group, d_reference_group, d_idx, d_mse);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

}  // extern "C"

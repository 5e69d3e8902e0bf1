// Structural RMSD evaluation on the device: what the reference's driver does with the output of generate() before
// anything else (main.py:264-320 -> parts/def_for_main.py:73-117) and what its post-hoc script refines
// (evaluate_rmsd.py:79-115).
//
//  * kabsch_kernel: one wavefront per graph.  Centres, covariance H = p^T q and the residual are reduced across the lanes in
//    fp64 (the data are tiny, as in rdf_kernel); the 3x3 part is kabsch_math.h.  The RMSD is the RESIDUAL
//    sqrt(sum |R p - q|^2 / n), never E0 - 2 sum(sigma), which cancels for good fits.  The same launch counts the rows equal to
//    one-hot O = [1, 0, ...] of the original and the generated atom types (def_for_main.py:103-111).
//  * kabsch_backward_kernel: the gradient of (R, t, rmsd) with respect to P and Q, so that the RMSD can be a loss term
//    (train_2024_11.py:233-236).  One wavefront per graph again.  Nothing is kept from the forward (a 64-atom pair is 768 B):
//    centres, H, the factors of the fit and the residual are recomputed in fp64 by the forward's own routine, a second
//    lane-strided pass reduces sum e_i p_i^T, sum p and sum q, the 3x3 part is kabsch_fit_backward_factors (kabsch_math.h), and a
//    third pass writes every row of dP and dQ as fp32.  Butterfly sums only, no atomics: bitwise reproducible.
//  * kabsch_perm_search_kernel + kabsch_perm_final_kernel: minimum over all orderings [0] + perm(1..n-1) of the generated
//    structure of the atom-0-anchored, row-flip RMSD (evaluate_rmsd.py:93-107).  Atom 0 is the centre and stays put, so
//    sum |p|^2 + sum |q|^2 is the same for every ordering and arg min RMSD = arg max of the optimal proper rotation's trace
//    (kabsch_trace); no difference of large numbers is ever ranked.  H(order) = sum_i M[order(i)][i] with M[a][i] = p_a q_i^T
//    tabulated once per workgroup in LDS, fp64, position-major ([i][a][9]: the lanes of a wave read the same position i at
//    different atoms a, i.e. consecutive 72-byte entries, an odd stride in 8-byte units -> conflict-free ds_read_b64; equal
//    atoms broadcast).  Orderings are taken in lexicographic rank order (= itertools.permutations) in blocks of 3! = 6 that
//    share the first n-4 positions: one prefix sum + 9 table entries serve 6 orderings.  A thread owns a contiguous range of
//    blocks: it unranks once (factorial number system) and then counts its digits up.  Every score is an fp64 Newton iteration
//    that stops as soon as its iterate -- an upper bound -- is below the best score known to the thread or the workgroup; such
//    an ordering cannot win, so pruning never changes the result.  Each workgroup leaves one (score, rank) partial; the final
//    kernel (one wavefront per graph) reduces them, equal scores to the LOWEST rank (the reference keeps the first strict
//    minimum), unranks the winner and fits it with the routine kabsch_kernel uses.  Bitwise reproducible: no float atomics,
//    no dependence on arrival order.
#include "kabsch.h"

#include "eval_device.h"

namespace egnn {
namespace {

// Kabsch fit of n atom pairs by one wavefront: P row order[i] (order == nullptr: row i) against Q row i.
// All lanes return the same R [9], t [3] = c_Q - c_P and rmsd; the backward also takes the centres and the factors of the fit.
struct KabschWaveFit {
  double cp[3], cq[3];
  KabschFactors F;
};

template <bool kKeep>
__device__ __forceinline__ void kabsch_wave_fit(const float* __restrict__ P, const float* __restrict__ Q, const int* order, int n,
                                                int center, int flip, int lane, double* R, double* t, double& rmsd,
                                                KabschWaveFit* keep) {
  double cp[3] = {0.0, 0.0, 0.0}, cq[3] = {0.0, 0.0, 0.0};
  if (center == kKabschCentroid) {
    for (int i = lane; i < n; i += 64) {
      const int ip = order ? order[i] : i;
      for (int d = 0; d < 3; ++d) { cp[d] += (double)P[3 * ip + d]; cq[d] += (double)Q[3 * i + d]; }
    }
    for (int d = 0; d < 3; ++d) { cp[d] = wave_sum(cp[d]) / (double)n; cq[d] = wave_sum(cq[d]) / (double)n; }
  } else {
    const int ip = order ? order[0] : 0;
    for (int d = 0; d < 3; ++d) { cp[d] = (double)P[3 * ip + d]; cq[d] = (double)Q[d]; }
  }
  double H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = lane; i < n; i += 64) {
    const int ip = order ? order[i] : i;
    double p[3], q[3];
    for (int d = 0; d < 3; ++d) { p[d] = (double)P[3 * ip + d] - cp[d]; q[d] = (double)Q[3 * i + d] - cq[d]; }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) H[3 * r + c] += p[r] * q[c];
  }
  for (int k = 0; k < 9; ++k) H[k] = wave_sum(H[k]);
  if (kKeep) {
    kabsch_fit_factors(H, flip, R, keep->F);
    for (int d = 0; d < 3; ++d) { keep->cp[d] = cp[d]; keep->cq[d] = cq[d]; }
  } else {
    kabsch_fit(H, flip, R);
  }
  double res = 0.0;
  for (int i = lane; i < n; i += 64) {
    const int ip = order ? order[i] : i;
    double p[3];
    for (int d = 0; d < 3; ++d) p[d] = (double)P[3 * ip + d] - cp[d];
    for (int r = 0; r < 3; ++r) {
      const double e = (R[3 * r] * p[0] + R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2]) - ((double)Q[3 * i + r] - cq[r]);
      res += e * e;
    }
  }
  rmsd = sqrt(wave_sum(res) / (double)n);
  for (int d = 0; d < 3; ++d) t[d] = cq[d] - cp[d];
}

__device__ void kabsch_wave(const float* __restrict__ P, const float* __restrict__ Q, const int* order, int n, int center,
                            int flip, int lane, double* R, double* t, double& rmsd) {
  kabsch_wave_fit<false>(P, Q, order, n, center, flip, lane, R, t, rmsd, nullptr);
}

// The ordering of one graph as the kernels take it: `order` + lo (local indices: row i of the fit is row order[i] of P), or
// nullptr -- the identity -- without an order or where an entry lies outside [0, n).  This guards ADDRESSES only (no such index
// is ever used as one); it does not make an ordering valid: the caller passes a permutation of every graph's rows (an in-range
// ordering with repeated indices is fitted as it stands, and the lanes that share a dP row then write it in no defined order).
__device__ __forceinline__ const int* graph_order(const int* __restrict__ order, int lo, int n, int lane) {
  if (!order) return nullptr;
  int bad = 0;
  for (int i = lane; i < n; i += 64) bad |= (unsigned)order[lo + i] >= (unsigned)n;
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) bad |= __shfl_xor(bad, m, 64);
  return bad ? nullptr : order + lo;
}

__global__ __launch_bounds__(64) void kabsch_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                    const int* __restrict__ graph_ptr, const int* __restrict__ order,
                                                    int center, int flip, const int* __restrict__ x_p,
                                                    const int* __restrict__ x_q, int A, float* __restrict__ out) {
  const int g = blockIdx.x, lane = threadIdx.x, lo = graph_ptr[g], n = graph_ptr[g + 1] - lo;
  float* o = out + (size_t)g * kKabschOutStride;
  if (n < 1) {
    if (lane < kKabschOutStride) o[lane] = (lane == 0 || lane == 4 || lane == 8) ? 1.f : 0.f;
    return;
  }
  double R[9], t[3], rmsd;
  kabsch_wave(P + 3 * (size_t)lo, Q + 3 * (size_t)lo, graph_order(order, lo, n, lane), n, center, flip, lane, R, t, rmsd);
  int cnt_p = 0, cnt_q = 0;
  if (x_p && x_q) {
    for (int i = lane; i < n; i += 64) {
      bool is_p = true, is_q = true;
      for (int a = 0; a < A; ++a) {
        const int want = a == 0 ? 1 : 0;
        is_p = is_p && x_p[(size_t)(lo + i) * A + a] == want;
        is_q = is_q && x_q[(size_t)(lo + i) * A + a] == want;
      }
      cnt_p += is_p;
      cnt_q += is_q;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) { cnt_p += __shfl_xor(cnt_p, m, 64); cnt_q += __shfl_xor(cnt_q, m, 64); }
  }
  if (lane == 0) {
    for (int k = 0; k < 9; ++k) o[k] = (float)R[k];
    for (int d = 0; d < 3; ++d) o[9 + d] = (float)t[d];
    o[12] = (float)rmsd;
    o[13] = (float)cnt_p;
    o[14] = (float)cnt_q;
    o[15] = 0.f;
  }
}

// gout [B,16] in the forward's layout: dL/dR [9], dL/dt [3], dL/drmsd (the rest is not read).  With p, q the centred rows,
// e_i = R p_i - q_i and c = g_rmsd / (n rmsd) (0 where rmsd = 0):
//   Rbar = g_R + c sum e_i p_i^T,  Hbar = kabsch_fit_backward(Rbar),  pbar_i = c R^T e_i + Hbar q_i,  qbar_i = -c e_i + Hbar^T p_i,
//   centroid:  dP_i = pbar_i - (sum pbar + g_t) / n,  dQ_i = qbar_i - (sum qbar - g_t) / n
//   first:     dP_i = pbar_i, dQ_i = qbar_i, and row 0 takes -(sum pbar + g_t), -(sum qbar - g_t)
// Every row of the graph is written (dP row i at row order[i]); one-atom graphs get zeros.
__global__ __launch_bounds__(64) void kabsch_backward_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                             const int* __restrict__ graph_ptr, const int* __restrict__ order,
                                                             int center, int flip, const float* __restrict__ gout,
                                                             float* __restrict__ dP, float* __restrict__ dQ) {
  const int g = blockIdx.x, lane = threadIdx.x, lo = graph_ptr[g], n = graph_ptr[g + 1] - lo;
  if (n < 1) return;
  const float* Pg = P + 3 * (size_t)lo;
  const float* Qg = Q + 3 * (size_t)lo;
  float* dPg = dP + 3 * (size_t)lo;
  float* dQg = dQ ? dQ + 3 * (size_t)lo : nullptr;
  if (n == 1) {
    if (lane < 3) {
      dPg[lane] = 0.f;
      if (dQg) dQg[lane] = 0.f;
    }
    return;
  }
  const int* ord = graph_order(order, lo, n, lane);
  double R[9], t[3], rmsd;
  KabschWaveFit fit;
  kabsch_wave_fit<true>(Pg, Qg, ord, n, center, flip, lane, R, t, rmsd, &fit);
  double E[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, sp[3] = {0.0, 0.0, 0.0}, sq[3] = {0.0, 0.0, 0.0};
  for (int i = lane; i < n; i += 64) {
    const int ip = ord ? ord[i] : i;
    double p[3], q[3];
    for (int d = 0; d < 3; ++d) { p[d] = (double)Pg[3 * ip + d] - fit.cp[d]; q[d] = (double)Qg[3 * i + d] - fit.cq[d]; }
    for (int r = 0; r < 3; ++r) {
      const double e = (R[3 * r] * p[0] + R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2]) - q[r];
      for (int c = 0; c < 3; ++c) E[3 * r + c] += e * p[c];
      sp[r] += p[r];
      sq[r] += q[r];
    }
  }
  for (int k = 0; k < 9; ++k) E[k] = wave_sum(E[k]);
  for (int d = 0; d < 3; ++d) { sp[d] = wave_sum(sp[d]); sq[d] = wave_sum(sq[d]); }
  const float* go = gout + (size_t)g * kKabschOutStride;
  const double c = rmsd > 0.0 ? (double)go[12] / ((double)n * rmsd) : 0.0;
  double Rbar[9], Hbar[9];
  for (int k = 0; k < 9; ++k) Rbar[k] = (double)go[k] + c * E[k];
  kabsch_fit_backward_factors(fit.F, Rbar, Hbar);
  double se[3], mp[3], mq[3];
  for (int r = 0; r < 3; ++r) se[r] = (R[3 * r] * sp[0] + R[3 * r + 1] * sp[1] + R[3 * r + 2] * sp[2]) - sq[r];
  for (int d = 0; d < 3; ++d) {
    const double gt = (double)go[9 + d];
    mp[d] = c * (R[d] * se[0] + R[3 + d] * se[1] + R[6 + d] * se[2]) + (Hbar[3 * d] * sq[0] + Hbar[3 * d + 1] * sq[1] + Hbar[3 * d + 2] * sq[2]) + gt;
    mq[d] = -c * se[d] + (Hbar[d] * sp[0] + Hbar[3 + d] * sp[1] + Hbar[6 + d] * sp[2]) - gt;
    if (center == kKabschCentroid) { mp[d] /= (double)n; mq[d] /= (double)n; }
  }
  for (int i = lane; i < n; i += 64) {
    const int ip = ord ? ord[i] : i;
    double p[3], q[3], e[3];
    for (int d = 0; d < 3; ++d) { p[d] = (double)Pg[3 * ip + d] - fit.cp[d]; q[d] = (double)Qg[3 * i + d] - fit.cq[d]; }
    for (int r = 0; r < 3; ++r) e[r] = (R[3 * r] * p[0] + R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2]) - q[r];
    const bool takes_mean = center == kKabschCentroid || i == 0;
    for (int d = 0; d < 3; ++d) {
      const double pb = c * (R[d] * e[0] + R[3 + d] * e[1] + R[6 + d] * e[2]) + (Hbar[3 * d] * q[0] + Hbar[3 * d + 1] * q[1] + Hbar[3 * d + 2] * q[2]);
      const double qb = -c * e[d] + (Hbar[d] * p[0] + Hbar[3 + d] * p[1] + Hbar[6 + d] * p[2]);
      dPg[3 * ip + d] = (float)(takes_mean ? pb - mp[d] : pb);
      if (dQg) dQg[3 * i + d] = (float)(takes_mean ? qb - mq[d] : qb);
    }
  }
}

// ---- correspondence search ----------------------------------------------------------------------------------------
__constant__ unsigned kFact[12] = {1u, 1u, 2u, 6u, 24u, 120u, 720u, 5040u, 40320u, 362880u, 3628800u, 39916800u};

__device__ __forceinline__ int nth_set_bit(unsigned m, int d) {
  for (int j = 0; j < d; ++j) m &= m - 1;
  return __ffs(m) - 1;
}

// (score, rank) order of the search: the larger score, equal scores to the lower rank
__device__ __forceinline__ bool perm_better(double s, unsigned r, double s0, unsigned r0) { return s > s0 || (s == s0 && r < r0); }

__global__ __launch_bounds__(kPermThreads) void kabsch_perm_search_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                                           const int* __restrict__ graph_ptr, int max_atoms,
                                                                           PermPartial* __restrict__ partials) {
  __shared__ double tab[kPermMaxAtoms * kPermMaxAtoms * 9];   // [position i][atom a][3 x 3]
  __shared__ double red_s[kPermThreads];
  __shared__ unsigned red_r[kPermThreads];
  __shared__ unsigned long long wg_best;   // bits of the best score any thread of the workgroup has seen (>= 0: ordered as integers)
  const int g = blockIdx.y, chunk = blockIdx.x, C = gridDim.x, tid = threadIdx.x;
  const int lo = graph_ptr[g], n = graph_ptr[g + 1] - lo;
  if (n < 2 || n > max_atoms) return;   // not searched: no work, nothing written
  const float* p0 = P + 3 * (size_t)lo;
  const float* q0 = Q + 3 * (size_t)lo;
  for (int e = tid; e < n * n; e += kPermThreads) {
    const int i = e / n, a = e % n;
    double p[3], q[3];
    for (int d = 0; d < 3; ++d) { p[d] = (double)p0[3 * a + d] - (double)p0[d]; q[d] = (double)q0[3 * i + d] - (double)q0[d]; }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) tab[9 * e + 3 * r + c] = p[r] * q[c];
  }
  if (tid == 0) wg_best = 0ull;
  __syncthreads();

  double best = -1.0;
  unsigned best_rank = 0xffffffffu;
  if (n < 4) {   // one or two orderings: [0,1]; [0,1,2], [0,2,1]
    if (chunk == 0 && tid == 0) {
      for (unsigned rank = 0; rank < kFact[n - 1]; ++rank) {
        double H[9];
        for (int k = 0; k < 9; ++k) H[k] = 0.0;
        for (int i = 1; i < n; ++i) {
          const int a = (n == 3 && rank == 1) ? 3 - i : i;
          for (int k = 0; k < 9; ++k) H[k] += tab[9 * (i * n + a) + k];
        }
        const double s = kabsch_trace(H, -1.0);
        if (s > best) { best = s; best_rank = rank; }
      }
    }
  } else {
    const unsigned nblocks = kFact[n - 1] / 6u;
    const unsigned per_wg = (nblocks + C - 1) / C, per_thread = (per_wg + kPermThreads - 1) / kPermThreads;
    const unsigned wg_end = min(nblocks, (chunk + 1u) * per_wg);
    unsigned blk = chunk * per_wg + tid * per_thread;
    const unsigned blk_end = min(wg_end, blk + per_thread);
    const int npre = n - 4;   // positions 1 .. n-4 carry the digits; the last three positions are the block
    unsigned long long digits = 0ull;   // factorial-number-system digit of position i in bits [4i, 4i + 4)
    {
      unsigned r = blk < nblocks ? blk : 0u;
      for (int i = 1; i <= npre; ++i) {
        const unsigned w = kFact[n - 1 - i] / 6u;   // blocks per unit of digit i
        digits |= (unsigned long long)(r / w) << (4 * i);
        r %= w;
      }
    }
    for (; blk < blk_end; ++blk) {
      double H0[9];
      for (int k = 0; k < 9; ++k) H0[k] = 0.0;
      unsigned mask = (1u << n) - 2u;   // atoms 1 .. n-1 still free
#pragma unroll
      for (int i = 1; i <= kPermMaxAtoms - 4; ++i) {
        if (i <= npre) {
          const int a = nth_set_bit(mask, (int)((digits >> (4 * i)) & 15ull));
          mask &= ~(1u << a);
          const double* m = tab + 9 * (i * n + a);
          for (int k = 0; k < 9; ++k) H0[k] += m[k];
        }
      }
      int atom[3];
      atom[0] = __ffs(mask) - 1; mask &= mask - 1;
      atom[1] = __ffs(mask) - 1; mask &= mask - 1;
      atom[2] = __ffs(mask) - 1;
      double m[3][3][9];   // [which free atom][which of the last three positions]
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const double* src = tab + 9 * ((n - 3 + s) * n + atom[j]);
#pragma unroll
          for (int k = 0; k < 9; ++k) m[j][s][k] = src[k];
        }
      const double shared_best = __longlong_as_double((long long)*(volatile unsigned long long*)&wg_best);
      bool improved = false;
#pragma unroll
      for (int e = 0; e < 6; ++e) {   // lexicographic: 012 021 102 120 201 210
        constexpr int kOrd[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
        double H[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) H[k] = ((H0[k] + m[kOrd[e][0]][0][k]) + m[kOrd[e][1]][1][k]) + m[kOrd[e][2]][2][k];
        const double s = kabsch_trace(H, fmax(best, shared_best));
        if (s > best) { best = s; best_rank = blk * 6u + e; improved = true; }
      }
      if (improved) atomicMax(&wg_best, (unsigned long long)__double_as_longlong(best));
      for (int i = npre; i >= 1; --i) {   // count the prefix digits up, radix of position i = n - i
        const unsigned long long d = ((digits >> (4 * i)) & 15ull) + 1ull;
        digits &= ~(15ull << (4 * i));
        if ((int)d < n - i) { digits |= d << (4 * i); break; }
      }
    }
  }
  red_s[tid] = best;
  red_r[tid] = best_rank;
  __syncthreads();
  for (int w = kPermThreads / 2; w > 0; w >>= 1) {
    if (tid < w && perm_better(red_s[tid + w], red_r[tid + w], red_s[tid], red_r[tid])) {
      red_s[tid] = red_s[tid + w];
      red_r[tid] = red_r[tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    PermPartial out;
    out.score = red_s[0];
    out.rank = red_r[0];
    out.pad = 0u;
    partials[(size_t)g * C + chunk] = out;
  }
}

__global__ __launch_bounds__(64) void kabsch_perm_final_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                               const int* __restrict__ graph_ptr, int max_atoms, int C,
                                                               const PermPartial* __restrict__ partials, float* __restrict__ min_rmsd,
                                                               int* __restrict__ order_out, float* __restrict__ R_out,
                                                               int* __restrict__ searched) {
  __shared__ int order[kPermMaxAtoms];
  const int g = blockIdx.x, lane = threadIdx.x, lo = graph_ptr[g], n = graph_ptr[g + 1] - lo;
  if (n < 2 || n > max_atoms) {
    if (lane == 0) searched[g] = 0;
    return;
  }
  double s = -2.0;
  unsigned r = 0xffffffffu;
  for (int c = lane; c < C; c += 64) {
    const PermPartial p = partials[(size_t)g * C + c];
    if (perm_better(p.score, p.rank, s, r)) { s = p.score; r = p.rank; }
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const double s2 = __shfl_xor(s, m, 64);
    const unsigned r2 = (unsigned)__shfl_xor((int)r, m, 64);
    if (perm_better(s2, r2, s, r)) { s = s2; r = r2; }
  }
  if (lane == 0) {
    unsigned mask = (1u << n) - 2u, rest = r < kFact[n - 1] ? r : 0u;   // no finite score (NaN input): the identity ordering
    order[0] = 0;
    for (int i = 1; i < n; ++i) {
      const unsigned f = kFact[n - 1 - i];
      const int a = nth_set_bit(mask, (int)(rest / f));
      rest %= f;
      mask &= ~(1u << a);
      order[i] = a;
    }
  }
  __syncthreads();
  double R[9], t[3], rmsd;
  kabsch_wave(P + 3 * (size_t)lo, Q + 3 * (size_t)lo, order, n, kKabschFirst, kKabschFlipRow, lane, R, t, rmsd);
  if (lane < n) order_out[lo + lane] = order[lane];
  if (lane == 0) {
    min_rmsd[g] = (float)rmsd;
    for (int k = 0; k < 9; ++k) R_out[9 * (size_t)g + k] = (float)R[k];
    searched[g] = 1;
  }
}

// workgroups per graph: enough that a handful of graphs of max_atoms atoms fills the chip (about 1,024 workgroups in all), never
// fewer than one block of six orderings per thread, one workgroup per graph from 1,024 graphs on
int perm_chunks(int B, int max_atoms) {
  static const unsigned fact[12] = {1u, 1u, 2u, 6u, 24u, 120u, 720u, 5040u, 40320u, 362880u, 3628800u, 39916800u};
  const unsigned nblocks = max_atoms >= 4 ? fact[max_atoms - 1] / 6u : 1u;
  const unsigned cmax = (nblocks + kPermThreads - 1) / kPermThreads;
  unsigned c = (1024u + (unsigned)B - 1u) / (unsigned)B;
  if (c > cmax) c = cmax;
  if (c > 1024u) c = 1024u;
  return c < 1u ? 1 : (int)c;
}

}  // namespace
}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_kabsch(void* stream, int B, const float* P, const float* Q, const int32_t* graph_ptr, int center, int flip,
                const int32_t* x_p, const int32_t* x_q, int A, float* out) {
  if (B < 1 || !P || !Q || !graph_ptr || !out || (center != EGNN_KABSCH_CENTROID && center != EGNN_KABSCH_FIRST) ||
      (flip != EGNN_KABSCH_FLIP_ROW && flip != EGNN_KABSCH_FLIP_COLUMN) || ((x_p != nullptr) != (x_q != nullptr)) || (x_p && A < 1)) {
    set_error("bad egnn_kabsch arguments");
    return EGNN_EINVAL;
  }
  hipLaunchKernelGGL(kabsch_kernel, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), P, Q, graph_ptr,
                     (const int32_t*)nullptr, center, flip, x_p, x_q, A, out);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_kabsch_ordered(void* stream, int B, const float* P, const float* Q, const int32_t* graph_ptr, const int32_t* order,
                        int center, int flip, float* out) {
  if (B < 1 || !P || !Q || !graph_ptr || !out || (center != EGNN_KABSCH_CENTROID && center != EGNN_KABSCH_FIRST) ||
      (flip != EGNN_KABSCH_FLIP_ROW && flip != EGNN_KABSCH_FLIP_COLUMN)) {
    set_error("bad egnn_kabsch_ordered arguments");
    return EGNN_EINVAL;
  }
  hipLaunchKernelGGL(kabsch_kernel, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), P, Q, graph_ptr, order, center,
                     flip, (const int32_t*)nullptr, (const int32_t*)nullptr, 0, out);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_kabsch_backward(void* stream, int B, const float* P, const float* Q, const int32_t* graph_ptr, const int32_t* order,
                         int center, int flip, const float* gout, float* dP, float* dQ) {
  if (B < 1 || !P || !Q || !graph_ptr || !gout || !dP || (center != EGNN_KABSCH_CENTROID && center != EGNN_KABSCH_FIRST) ||
      (flip != EGNN_KABSCH_FLIP_ROW && flip != EGNN_KABSCH_FLIP_COLUMN)) {
    set_error("bad egnn_kabsch_backward arguments");
    return EGNN_EINVAL;
  }
  hipLaunchKernelGGL(kabsch_backward_kernel, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), P, Q, graph_ptr, order,
                     center, flip, gout, dP, dQ);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

size_t egnn_kabsch_perm_workspace_bytes(int B, int max_atoms) {
  if (B < 1 || max_atoms < 2 || max_atoms > kPermMaxAtoms) return 0;
  return (size_t)B * (size_t)perm_chunks(B, max_atoms) * sizeof(PermPartial);
}

int egnn_kabsch_perm(void* stream, int B, const float* P, const float* Q, const int32_t* graph_ptr, int max_atoms,
                     float* min_rmsd, int32_t* order, float* R, int32_t* searched, void* workspace, size_t workspace_bytes) {
  if (B < 1 || B > 65535 || !P || !Q || !graph_ptr || !min_rmsd || !order || !R || !searched || max_atoms < 2 ||
      max_atoms > kPermMaxAtoms) {
    set_error("bad egnn_kabsch_perm arguments (1 <= B <= 65535, 2 <= max_atoms <= %d)", kPermMaxAtoms);
    return EGNN_EINVAL;
  }
  if (!workspace || workspace_bytes < egnn_kabsch_perm_workspace_bytes(B, max_atoms)) {
    set_error("egnn_kabsch_perm: workspace smaller than egnn_kabsch_perm_workspace_bytes(B, max_atoms)");
    return EGNN_EINVAL;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int C = perm_chunks(B, max_atoms);
  PermPartial* partials = reinterpret_cast<PermPartial*>(workspace);
  hipLaunchKernelGGL(kabsch_perm_search_kernel, dim3(C, B), dim3(kPermThreads), 0, st, P, Q, graph_ptr, max_atoms, partials);
  hipLaunchKernelGGL(kabsch_perm_final_kernel, dim3(B), dim3(64), 0, st, P, Q, graph_ptr, max_atoms, C, partials, min_rmsd, order,
                     R, searched);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

}  // extern "C"

// Whole-structure statistics on the device: partial pair counts over EVERY centre (-> partial RDFs g_ab), coordination-number
// histograms and bond-angle histograms by type, of a ragged batch of graphs.  Definitions: structure_math.h (shared with the host
// statement, structure_host.cpp).  Generalises evaluate_RDF.py:39-60, evaluate_Si-O-Si.py:23-41 and CN2_evaluate.py:12-21, which
// look at atom 0 only.
//
// Every accumulator is an integer: LDS integer atomics inside a workgroup, one global integer atomicAdd per non-zero bin at the
// end of a tile.  Integer sums do not depend on arrival order, so the results are bitwise identical from run to run.
//
// Tiles come from the caller ({graph, first centre, first neighbour} int32 triples, built from the graph sizes on the host).  A
// kernel trusts no entry: graph, centre block and neighbour chunk are checked against graph_ptr, and every atom index a kernel
// forms lies in [graph_ptr[g], graph_ptr[g + 1]), also where the last centre block or neighbour chunk of a graph is partial.
#include "eval_device.h"
#include "structure_host.h"
#include "structure_math.h"

namespace egnn {

constexpr int kStructWeightTaps = 128;   // half width of the smoothing filter up to which its weights are tabled in LDS

// ---- ordered pairs -> c[g][a][b][k] --------------------------------------------------------------------------------------------
// One workgroup of 256 threads per tile (graph, <= 64 centres, <= 1024 neighbour atoms): 256 graphs of 64 atoms, 32 of 512 and one
// of 4096 atoms all give 256 tiles, one per CU.  The neighbour chunk (positions, types) is staged in LDS; a thread keeps one centre
// in registers and walks every fourth atom of the chunk (each wavefront its own quarter), all lanes of a wavefront reading the same
// neighbour (an LDS broadcast).  Dynamic LDS: the histogram, A * A * nbins int32.
__global__ __launch_bounds__(256) void struct_pair_kernel(const float* __restrict__ pos, const int* __restrict__ type,
                                                          const int* __restrict__ graph_ptr, int B, int A,
                                                          const int* __restrict__ tiles, double dR, int nbins,
                                                          int* __restrict__ counts) {
  extern __shared__ int pair_hist[];
  __shared__ float s_pos[3 * kStructChunk];
  __shared__ int s_type[kStructChunk];
  const int tid = threadIdx.x;
  PairTile T;
  if (!pair_tile_read<kStructCentreBlock, kStructChunk>(tiles, blockIdx.x, graph_ptr, B, &T)) return;
  const int g = T.g, lo = T.lo, c0 = T.c0, j0 = T.j0, nc = T.nc, nj = T.nj;
  const int nh = A * A * nbins;
  for (int k = tid; k < nh; k += 256) pair_hist[k] = 0;
  for (int t = tid; t < 3 * nj; t += 256) s_pos[t] = pos[3 * (size_t)(lo + j0) + t];
  for (int t = tid; t < nj; t += 256) s_type[t] = type[lo + j0 + t];
  __syncthreads();
  constexpr int slices = 256 / kStructCentreBlock, per = kStructCentreBlock;
  const int c = tid % per, s = tid / per;
  if (c < nc) {
    const int i = lo + c0 + c, ti = type[i];
    if (ti >= 0 && ti < A) {
      const float px = pos[3 * (size_t)i], py = pos[3 * (size_t)i + 1], pz = pos[3 * (size_t)i + 2];
      const float inv_dR = (float)(1.0 / dR);
      int* row = pair_hist + (size_t)ti * A * nbins;
      for (int j = s; j < nj; j += slices) {
        const int tj = s_type[j];
        if (j0 + j == c0 + c || tj < 0 || tj >= A) continue;
        const float d = struct_distance(px, py, pz, s_pos[3 * j], s_pos[3 * j + 1], s_pos[3 * j + 2]);
        const int k0 = struct_bin_guess(d, inv_dR, nbins);
        for (int k = k0 - 1; k <= k0 + 1; ++k)
          if (k >= 0 && k < nbins && struct_in_bin(d, k, dR)) atomicAdd(&row[tj * nbins + k], 1);
      }
    }
  }
  __syncthreads();
  int* out = counts + (size_t)g * nh;
  for (int k = tid; k < nh; k += 256) {
    const int v = pair_hist[k];
    if (v) atomicAdd(&out[k], v);
  }
}

// ---- bonds -> cn[g][a][b][m], ang[g][a][p][k], overflow[g] ---------------------------------------------------------------------
// One workgroup of four wavefronts per tile (graph, <= 8 centres); ONE WAVEFRONT PER CENTRE, four centres in flight.  The lanes
// stride over the graph's atoms, 64 at a time, staged through the wavefront's own LDS chunk (coalesced loads of 192 floats);
// bonded neighbours are appended in ascending j by ballot + popcount compaction to the wavefront's LDS list (type, double bond
// vector) of kMaxNeighbours entries.  The per-type bond counts come from the ballots, so CN is exact beyond the cap; a centre
// with more bonds than the list holds increments overflow[g] and contributes no angle.  The m (m - 1) / 2 neighbour pairs are
// spread over the 64 lanes.  Dynamic LDS: ang [A][P][nth], cn [A][A][max_cn + 1], overflow [1], all int32.
struct BondWave {
  float stage[3 * 64];
  double v[3 * kMaxNeighbours];
  int t[kMaxNeighbours];
};

__global__ __launch_bounds__(256) void struct_bond_kernel(const float* __restrict__ pos, const int* __restrict__ type,
                                                          const int* __restrict__ graph_ptr, int B, int A,
                                                          const int* __restrict__ tiles, float cutoff, double dtheta, int nth,
                                                          int max_cn, int* __restrict__ cn, int* __restrict__ angles,
                                                          int* __restrict__ overflow) {
  extern __shared__ int bond_hist[];
  __shared__ BondWave s_wave[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = tiles[3 * blockIdx.x], c0 = tiles[3 * blockIdx.x + 1];
  if (g < 0 || g >= B) return;
  const int lo = graph_ptr[g], n = graph_ptr[g + 1] - lo;
  if (c0 < 0 || c0 >= n) return;
  const int nc = min(kStructBondCentres, n - c0);
  const int P = type_pairs(A), ncn = max_cn + 1;
  const int n_ang = A * P * nth, n_cn = A * A * ncn, nh = n_ang + n_cn + 1;
  int* h_ang = bond_hist;
  int* h_cn = bond_hist + n_ang;
  int* h_over = bond_hist + n_ang + n_cn;
  for (int k = tid; k < nh; k += 256) bond_hist[k] = 0;
  __syncthreads();
  BondWave& W = s_wave[wave];
  for (int c = c0 + wave; c < c0 + nc; c += 4) {   // uniform in a wavefront
    const int i = lo + c, ti = type[i];
    if (ti < 0 || ti >= A) continue;
    const float px = pos[3 * (size_t)i], py = pos[3 * (size_t)i + 1], pz = pos[3 * (size_t)i + 2];
    int nb[kStructMaxTypes] = {0, 0, 0, 0}, nlist = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {
      const int m = min(64, n - j0);
      const int j = j0 + lane;
      const int tj = lane < m ? type[lo + j] : -1;   // in flight together with the positions
      for (int t = lane; t < 3 * m; t += 64) W.stage[t] = pos[3 * (size_t)(lo + j0) + t];
      wave_sync();
      bool bonded = false;
      float qx = 0.f, qy = 0.f, qz = 0.f;
      if (lane < m && j != c) {
        qx = W.stage[3 * lane]; qy = W.stage[3 * lane + 1]; qz = W.stage[3 * lane + 2];
        bonded = tj >= 0 && tj < A && struct_distance(px, py, pz, qx, qy, qz) < cutoff;
      }
      const unsigned long long mask = __ballot(bonded);
#pragma unroll
      for (int b = 0; b < kStructMaxTypes; ++b) nb[b] += __popcll(__ballot(bonded && tj == b));
      const int slot = nlist + lane_prefix(mask, lane);
      if (bonded && slot < kMaxNeighbours) {
        W.v[3 * slot] = (double)qx - (double)px;
        W.v[3 * slot + 1] = (double)qy - (double)py;
        W.v[3 * slot + 2] = (double)qz - (double)pz;
        W.t[slot] = tj;
      }
      nlist += __popcll(mask);
      wave_sync();
    }
    if (lane < A) atomicAdd(&h_cn[(ti * A + lane) * ncn + min(nb[lane], max_cn)], 1);
    if (nlist > kMaxNeighbours) {
      if (lane == 0) atomicAdd(h_over, 1);
    } else {
      for (int p = lane; p < nlist * nlist; p += 64) {
        const int a = p / nlist, b = p - a * nlist;
        if (a >= b) continue;
        const int k = struct_angle_bin(&W.v[3 * a], &W.v[3 * b], dtheta, nth);
        if (k >= 0) atomicAdd(&h_ang[(ti * P + type_pair_index(W.t[a], W.t[b], A)) * nth + k], 1);
      }
    }
    wave_sync();   // the list is rewritten for the next centre
  }
  __syncthreads();
  int* o_ang = angles + (size_t)g * n_ang;
  int* o_cn = cn + (size_t)g * n_cn;
  for (int k = tid; k < n_ang; k += 256) {
    const int v = h_ang[k];
    if (v) atomicAdd(&o_ang[k], v);
  }
  for (int k = tid; k < n_cn; k += 256) {
    const int v = h_cn[k];
    if (v) atomicAdd(&o_cn[k], v);
  }
  if (tid == 0 && overflow && *h_over) atomicAdd(&overflow[g], *h_over);
}

// ---- counts -> g_ab --------------------------------------------------------------------------------------------------------------
// One workgroup per (g, a, b) row: c / max(n_a, 1) / (4 pi rho r_k^2 dR) with rho = n / (4/3 pi R^3) over ALL atoms of the graph
// (the reference's normaliser, evaluate_RDF.py:50-56), then the Gaussian filter; fp64 inside, float32 out.  An absent type has
// zero counts: rows of zeros, never NaN.
__global__ __launch_bounds__(256) void struct_rdf_finish_kernel(const int* __restrict__ counts, const int* __restrict__ type,
                                                                const int* __restrict__ graph_ptr, int A, double R, double dR,
                                                                double sigma, int nbins, float* __restrict__ out) {
  __shared__ double raw[kStructMaxBins];
  __shared__ double s_w[2 * kStructWeightTaps + 1];   // the filter's weights, where 4 sigma fits (the same values, the same order)
  __shared__ int s_na;
  const int row = blockIdx.x, g = row / (A * A), a = (row / A) % A;
  const int lo = graph_ptr[g], hi = graph_ptr[g + 1], n = hi - lo;
  if (threadIdx.x == 0) s_na = 0;
  __syncthreads();
  int mine = 0;
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) mine += type[i] == a;
  if (mine) atomicAdd(&s_na, mine);
  __syncthreads();
  const double na = (double)max(s_na, 1);
  const double rho = (double)n / (4.0 / 3.0 * M_PI * R * R * R);
  for (int k = threadIdx.x; k < nbins; k += blockDim.x) {
    const double rk = dR + (double)k * dR;
    const int c = counts[(size_t)row * nbins + k];
    raw[k] = c ? (double)c / na / (4.0 * M_PI * rho * rk * rk * dR) : 0.0;
  }
  __syncthreads();
  const int lw = struct_smooth_half_width(sigma);
  const bool tabled = lw <= kStructWeightTaps;
  if (tabled)
    for (int t = threadIdx.x; t <= 2 * lw; t += blockDim.x) s_w[t] = struct_smooth_weight(t - lw, sigma);
  __syncthreads();
  double wsum = 0.0;
  for (int t = -lw; t <= lw; ++t) wsum += tabled ? s_w[t + lw] : struct_smooth_weight(t, sigma);
  for (int k = threadIdx.x; k < nbins; k += blockDim.x) {
    double acc;
    if (tabled) {
      acc = 0.0;
      for (int t = -lw; t <= lw; ++t) acc += raw[struct_reflect(k + t, nbins)] * s_w[t + lw];
      acc /= wsum;
    } else {
      acc = struct_smooth_at(raw, nbins, k, sigma, lw, wsum);
    }
    out[(size_t)row * nbins + k] = (float)acc;
  }
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_struct_pair_counts(void* stream, int B, int A, const float* pos, const int32_t* type, const int32_t* graph_ptr,
                            int max_atoms, const int32_t* tiles, int n_tiles, double dR, int nbins, int32_t* counts) {
  const char* who = "egnn_struct_pair_counts";
  if (int rc = struct_pair_args_check(who, B, A, pos, type, graph_ptr, max_atoms, dR, nbins, counts)) return rc;
  if (int rc = tiles_check(who, tiles, n_tiles)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t lds = sizeof(int) * (size_t)A * A * nbins;
  // 64 KiB of histogram at A = 4, nbins = 1024, beside 16 KiB of staged neighbours; a CU has 160 KiB
  static LdsLimitRecord raised;
  if (int rc = raise_lds_limit(raised, &struct_pair_kernel, sizeof(int) * kStructMaxTypes * kStructMaxTypes * kStructMaxBins)) return rc;
  EGNN_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)B * A * A * nbins, st));
  if (n_tiles > 0)
    hipLaunchKernelGGL(struct_pair_kernel, dim3(n_tiles), dim3(256), lds, st, pos, type, graph_ptr, B, A, tiles, dR, nbins, counts);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_struct_bonds(void* stream, int B, int A, const float* pos, const int32_t* type, const int32_t* graph_ptr, int max_atoms,
                      const int32_t* tiles, int n_tiles, float cutoff, double dtheta, int max_cn, int32_t* cn, int32_t* angles,
                      int32_t* overflow) {
  const char* who = "egnn_struct_bonds";
  if (int rc = struct_bond_args_check(who, B, A, pos, type, graph_ptr, max_atoms, cutoff, dtheta, max_cn, cn, angles)) return rc;
  if (int rc = tiles_check(who, tiles, n_tiles)) return rc;
  if (!overflow) { set_error("bad %s arguments (overflow given)", who); return EGNN_EINVAL; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nth = struct_angle_bins(dtheta), P = type_pairs(A), ncn = max_cn + 1;
  const size_t n_ang = (size_t)A * P * nth, n_cn = (size_t)A * A * ncn;
  const size_t most = (size_t)kStructMaxTypes * type_pairs(kStructMaxTypes) * kStructMaxAngleBins +
                      (size_t)kStructMaxTypes * kStructMaxTypes * (kStructMaxCn + 1) + 1;
  static LdsLimitRecord raised;
  if (int rc = raise_lds_limit(raised, &struct_bond_kernel, sizeof(int) * most)) return rc;
  EGNN_HIP(hipMemsetAsync(cn, 0, sizeof(int32_t) * B * n_cn, st));
  EGNN_HIP(hipMemsetAsync(angles, 0, sizeof(int32_t) * B * n_ang, st));
  EGNN_HIP(hipMemsetAsync(overflow, 0, sizeof(int32_t) * (size_t)B, st));
  if (n_tiles > 0)
    hipLaunchKernelGGL(struct_bond_kernel, dim3(n_tiles), dim3(256), sizeof(int) * (n_ang + n_cn + 1), st, pos, type, graph_ptr, B, A,
                       tiles, cutoff, dtheta, nth, max_cn, cn, angles, overflow);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_struct_rdf_finish(void* stream, int B, int A, const int32_t* counts, const int32_t* type, const int32_t* graph_ptr, double R,
                           double dR, double sigma, int nbins, float* out) {
  if (int rc = struct_finish_args_check(B, A, counts, type, graph_ptr, R, dR, sigma, nbins, out)) return rc;
  hipLaunchKernelGGL(struct_rdf_finish_kernel, dim3(B * A * A), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), counts, type,
                     graph_ptr, A, R, dR, sigma, nbins, out);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

}  // extern "C"

// The topological (bond-graph) fingerprint on the device: bonds guessed from distances with a threshold per type pair, kept as a
// CSR list; hop distances, connected fragments and the atom-pair count vector from one breadth-first search per atom; Tanimoto
// similarity of count vectors.  Definitions: topo_math.h (shared with the host statement, topo_host.cpp).  Restates
// evaluate_fingerprint.py:49-114, which goes through xyz files, ASE and RDKit one graph at a time.
//
// Every accumulator is an integer and every list is written in ascending order by ballot + popcount compaction, so the results
// are bitwise identical from run to run and equal to the host statement's.  There is no float atomic.
//
// A kernel trusts no entry it reads: graphs are checked against N, a bond list against the 32 N entries the caller allocates,
// a neighbour against its graph, a degree against the list width.
#include "eval_device.h"
#include "topo_host.h"
#include "topo_math.h"

namespace egnn {

constexpr int kTopoBondCentres = 16;   // centres of one workgroup of the bond kernels (four wavefronts, one centre each at a time)
constexpr int kTopoPathWaves = 16;     // wavefronts of the path kernel: sources in flight per graph

struct TopoThresholds { double v[kTopoMaxTypes * kTopoMaxTypes]; };

__device__ __forceinline__ int topo_list_width(int degree) { return degree < 0 ? 0 : (degree < kTopoMaxDegree ? degree : kTopoMaxDegree); }

// ---- bonds -> degree[i], overflow[g] (kFill = false), then neighbours (kFill = true) ------------------------------------------
// Workgroup (g, b) takes centres 16 b .. 16 b + 15 of graph g, ONE WAVEFRONT PER CENTRE; the lanes stride over the graph's atoms
// 64 at a time, and a ballot of the bonded lanes gives the count and, by the popcount of the lower lanes, every neighbour's slot:
// rows come out ascending.  The count pass and the fill pass make the same decisions from the same text (topo_bonded).
template <bool kFill>
__global__ __launch_bounds__(256) void topo_bonds_kernel(const float* __restrict__ pos, const int* __restrict__ type,
                                                         const int* __restrict__ graph_ptr, int B, int N, int A, TopoThresholds thr,
                                                         const int* __restrict__ row_ptr, int* __restrict__ neighbours,
                                                         int* __restrict__ degree, int* __restrict__ overflow) {
  __shared__ double s_thr[kTopoMaxTypes * kTopoMaxTypes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x, c0 = blockIdx.y * kTopoBondCentres;
  if (tid < kTopoMaxTypes * kTopoMaxTypes) s_thr[tid] = thr.v[tid];
  __syncthreads();
  if (g >= B) return;
  const int lo = graph_ptr[g], n = graph_ptr[g + 1] - lo;
  if (lo < 0 || n <= 0 || lo > N - n || c0 >= n) return;
  const int c1 = min(c0 + kTopoBondCentres, n);
  for (int c = c0 + wave; c < c1; c += 4) {   // uniform in a wavefront
    const int i = lo + c, ti = type[i];
    const float p[3] = {pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2]};
    const int base = kFill ? row_ptr[i] : 0;
    int count = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {
      const int j = j0 + lane;
      bool bonded = false;
      if (j < n && j != c) {
        const size_t at = 3 * (size_t)(lo + j);
        const float q[3] = {pos[at], pos[at + 1], pos[at + 2]};
        bonded = topo_bonded(p, ti, q, type[lo + j], s_thr, A);
      }
      const unsigned long long mask = __ballot(bonded);
      if (kFill) {
        const int slot = count + lane_prefix(mask, lane);
        if (bonded && slot < kTopoMaxDegree && base >= 0 && base <= kTopoMaxDegree * N - kTopoMaxDegree) neighbours[base + slot] = lo + j;
      }
      count += __popcll(mask);
    }
    if (!kFill && lane == 0) {
      degree[i] = count;
      if (count > kTopoMaxDegree) atomicAdd(&overflow[g], 1);
    }
  }
}

// ---- degree -> row_ptr [N + 1]: the exclusive prefix sum of min(degree, 32), one workgroup ------------------------------------
__global__ __launch_bounds__(1024) void topo_row_ptr_kernel(const int* __restrict__ degree, int N, int* __restrict__ row_ptr) {
  __shared__ int s_sum[1024];
  const int tid = threadIdx.x;
  const int per = (N + 1023) / 1024, b = min(tid * per, N), e = min(b + per, N);
  int sum = 0;
  for (int i = b; i < e; ++i) sum += topo_list_width(degree[i]);
  s_sum[tid] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = tid >= off ? s_sum[tid - off] : 0;
    __syncthreads();
    s_sum[tid] += v;
    __syncthreads();
  }
  int run = s_sum[tid] - sum;
  for (int i = b; i < e; ++i) {
    row_ptr[i] = run;
    run += topo_list_width(degree[i]);
  }
  if (tid == 1023) row_ptr[N] = s_sum[1023];
}

// ---- bond lists -> distances, components, fragments, fingerprint --------------------------------------------------------------
// One workgroup of 16 wavefronts per graph.  The graph's bond lists are staged in LDS, TRANSPOSED: neighbour k of atom j (local
// index, uint16) at s_adj[k * npad + j], so that the 64 lanes of a wavefront -- which own atoms c 64 + lane -- read consecutive
// halfwords (no bank conflict; [atom][32] rows of 64 B would put 8 lanes of a half-wave on one bank).  Wavefront w takes the
// sources s = w, w + 16, ... and runs a level-synchronous breadth-first search from each: an unvisited atom joins level l iff one
// of its neighbours is in the frontier bit set of level l - 1 (a pull, so no atomic builds the frontier); the ballot of the
// joining lanes IS the next frontier word of that chunk.  It is kept in the register of lane c until the level is complete, then
// lanes 0 .. 15 store the 16 words and OR them into the visited set.  The search ends at the first level nobody joins.
//
// LDS: dynamic 32 * npad * 2 B (64 KiB at 1024 atoms); static 2 KiB of degrees and classes, 4 KiB of frontier and visited sets
// (2 * 128 B per wavefront) and 2 KiB of class counters: 72 KiB of a CU's 160 KiB.  The fingerprint itself stays in GLOBAL
// memory: at A = 4, L = 64 it has 25,984 keys = 101.5 KiB, which does not fit beside the lists.  All atoms that join one level
// share the source's class and the distance, so their keys differ by the joiner's class only: the lanes count joiners by class in
// 28 LDS counters of their wavefront (integer atomics), and after the level one lane per non-zero class adds it to the global row.
__global__ __launch_bounds__(1024) void topo_paths_kernel(const int* __restrict__ type, const int* __restrict__ graph_ptr, int B, int N,
                                                          int A, const int* __restrict__ row_ptr, const int* __restrict__ neighbours,
                                                          const int* __restrict__ degree, const int* __restrict__ overflow, int L,
                                                          int npad, uint16_t* __restrict__ dist, const long long* __restrict__ dist_ptr,
                                                          int* __restrict__ component, int* __restrict__ fragments, int* __restrict__ fp) {
  extern __shared__ uint16_t s_adj[];
  __shared__ uint8_t s_deg[kTopoMaxAtoms], s_cls[kTopoMaxAtoms];
  __shared__ unsigned long long s_frontier[kTopoPathWaves][kTopoMaxAtoms / 64], s_visited[kTopoPathWaves][kTopoMaxAtoms / 64];
  __shared__ int s_count[kTopoPathWaves][32];
  __shared__ int s_roots;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x;
  if (g >= B) return;
  const int lo = graph_ptr[g], n = graph_ptr[g + 1] - lo;
  if (n == 0 && lo >= 0 && lo <= N) {   // an empty graph has no fragment (and nothing else to write), as the host statement says
    if (fragments && tid == 0) fragments[g] = 0;
    return;
  }
  if (lo < 0 || n <= 0 || n > npad || npad > kTopoMaxAtoms || lo > N - n) return;   // uniform in the workgroup
  uint16_t* dist_g = dist ? dist + dist_ptr[g] : nullptr;
  if (overflow[g] != 0) {   // a bond list is cut short: no distances, no components, no fingerprint
    if (dist_g) for (int k = tid; k < n * n; k += 1024) dist_g[k] = kTopoUnreachable;
    if (component) for (int i = tid; i < n; i += 1024) component[lo + i] = -1;
    if (fragments && tid == 0) fragments[g] = -1;
    return;
  }
  if (tid == 0) s_roots = 0;
  for (int i = tid; i < n; i += 1024) {
    int d = topo_list_width(degree[lo + i]);
    const int rp = row_ptr[lo + i], ti = type[lo + i];
    if (rp < 0 || rp > kTopoMaxDegree * N - d) d = 0;
    s_deg[i] = (uint8_t)d;
    s_cls[i] = (uint8_t)(ti >= 0 && ti < A ? topo_class(ti, d) : 0);   // an atom of no type has no bond and is in no pair
    for (int k = 0; k < d; ++k) {
      const int v = neighbours[rp + k] - lo;
      s_adj[k * npad + i] = (uint16_t)(v >= 0 && v < n ? v : i);       // an atom is never in the frontier it may join
    }
  }
  __syncthreads();
  const int C = topo_classes(A), nchunks = (n + 63) >> 6;
  unsigned long long* F = s_frontier[wave];
  unsigned long long* V = s_visited[wave];
  int* cnt = s_count[wave];
  int* fp_g = fp ? fp + (size_t)g * topo_keys(A, L) : nullptr;
  for (int s = wave; s < n; s += kTopoPathWaves) {   // uniform in a wavefront
    if (lane < kTopoMaxAtoms / 64) {
      const unsigned long long w = lane == (s >> 6) ? 1ull << (s & 63) : 0ull;
      F[lane] = w;
      V[lane] = w;
    }
    if (lane < 32) cnt[lane] = 0;
    wave_sync();
    uint16_t* row = dist_g ? dist_g + (size_t)s * n : nullptr;
    if (row && lane == 0) row[s] = 0;
    const int cs = s_cls[s];
    int lowest = s;
    for (int level = 1;; ++level) {
      unsigned long long mine = 0ull;
      bool any = false;
      for (int c = 0; c < nchunks; ++c) {
        const unsigned long long seen = V[c];
        const int left = n - c * 64;
        const unsigned long long valid = left >= 64 ? ~0ull : (1ull << left) - 1ull;
        if ((seen & valid) == valid) continue;
        const int j = c * 64 + lane;
        bool join = false;
        if (j < n && !((seen >> lane) & 1ull)) {
          const int d = s_deg[j];
          for (int k = 0; k < d && !join; ++k) {
            const int v = s_adj[k * npad + j];
            join = (F[v >> 6] >> (v & 63)) & 1ull;
          }
        }
        const unsigned long long m = __ballot(join);
        if (!m) continue;
        any = true;
        if (lane == c) mine = m;
        lowest = min(lowest, c * 64 + __ffsll((long long)m) - 1);
        if (join) {
          if (row) row[j] = (uint16_t)level;
          if (fp_g && j > s && level <= L) atomicAdd(&cnt[s_cls[j]], 1);
        }
      }
      if (!any) break;
      wave_sync();   // every read of this level's frontier and every count is done
      if (lane < kTopoMaxAtoms / 64) {
        F[lane] = mine;
        V[lane] |= mine;
      }
      if (fp_g && level <= L && lane < C) {
        const int v = cnt[lane];
        if (v) {
          atomicAdd(&fp_g[topo_key(cs, lane, level, C, L)], v);
          cnt[lane] = 0;
        }
      }
      wave_sync();
    }
    if (row)
      for (int c = 0; c < nchunks; ++c) {
        const int j = c * 64 + lane;
        if (j < n && !((V[c] >> lane) & 1ull)) row[j] = kTopoUnreachable;
      }
    if (lane == 0) {
      if (component) component[lo + s] = lo + lowest;
      if (lowest == s) atomicAdd(&s_roots, 1);
    }
    wave_sync();   // the sets are rewritten for the next source
  }
  __syncthreads();
  if (fragments && tid == 0) fragments[g] = s_roots;
}

// ---- Tanimoto similarity of listed pairs of rows: one wavefront per pair ------------------------------------------------------
__global__ __launch_bounds__(256) void topo_tanimoto_kernel(const int* __restrict__ fp_a, int rows_a, const int* __restrict__ fp_b,
                                                            int rows_b, const int* __restrict__ pairs, int n_pairs, int K,
                                                            double* __restrict__ sim, long long* __restrict__ sa,
                                                            long long* __restrict__ sb) {
  const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= n_pairs) return;
  const int ra = pairs ? pairs[2 * p] : p, rb = pairs ? pairs[2 * p + 1] : p;
  if (ra < 0 || ra >= rows_a || rb < 0 || rb >= rows_b) {   // no such row: no similarity
    if (lane == 0) { sim[p] = 0.0; sa[p] = -1; sb[p] = -1; }
    return;
  }
  const int* a = fp_a + (size_t)ra * K;
  const int* b = fp_b + (size_t)rb * K;
  long long both = 0, ta = 0, tb = 0;
  for (int k = lane; k < K; k += 64) {
    const int x = a[k], y = b[k];
    both += min(x, y);
    ta += x;
    tb += y;
  }
  both = wave_sum(both);
  ta = wave_sum(ta);
  tb = wave_sum(tb);
  if (lane == 0) {
    sim[p] = topo_tanimoto(both, ta, tb);
    sa[p] = ta;
    sb[p] = tb;
  }
}

}  // namespace egnn

using namespace egnn;

static int topo_atoms_check(const char* who, int N) {
  if (N < 1 || N > 2147483647 / kTopoMaxDegree) { set_error("%s: %d atoms (1 <= N, and 32 N list entries inside int32)", who, N); return EGNN_EINVAL; }
  return EGNN_OK;
}

extern "C" {

int egnn_topo_bonds(void* stream, int B, int N, int A, const float* pos, const int32_t* type, const int32_t* graph_ptr, int max_atoms,
                    const double* thr, int32_t* row_ptr, int32_t* neighbours, int32_t* degree, int32_t* overflow) {
  const char* who = "egnn_topo_bonds";
  if (int rc = topo_common_check(who, B, A, type, graph_ptr, max_atoms)) return rc;
  if (int rc = topo_atoms_check(who, N)) return rc;
  if (!pos || !row_ptr || !neighbours || !degree || !overflow) {
    set_error("bad %s arguments (pos, row_ptr, neighbours, degree and overflow given)", who);
    return EGNN_EINVAL;
  }
  if (int rc = topo_threshold_check(who, A, thr)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  TopoThresholds t;
  for (int k = 0; k < kTopoMaxTypes * kTopoMaxTypes; ++k) t.v[k] = k < A * A ? thr[k] : 0.0;
  EGNN_HIP(hipMemsetAsync(overflow, 0, sizeof(int32_t) * (size_t)B, st));
  EGNN_HIP(hipMemsetAsync(degree, 0, sizeof(int32_t) * (size_t)N, st));
  const dim3 grid(B, (max_atoms + kTopoBondCentres - 1) / kTopoBondCentres);
  if (max_atoms > 0)
    hipLaunchKernelGGL(topo_bonds_kernel<false>, grid, dim3(256), 0, st, pos, type, graph_ptr, B, N, A, t, (const int*)nullptr,
                       (int*)nullptr, degree, overflow);
  hipLaunchKernelGGL(topo_row_ptr_kernel, dim3(1), dim3(1024), 0, st, degree, N, row_ptr);
  if (max_atoms > 0)
    hipLaunchKernelGGL(topo_bonds_kernel<true>, grid, dim3(256), 0, st, pos, type, graph_ptr, B, N, A, t, (const int*)row_ptr, neighbours,
                       (int*)nullptr, (int*)nullptr);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_topo_paths(void* stream, int B, int N, int A, const int32_t* type, const int32_t* graph_ptr, int max_atoms,
                    const int32_t* row_ptr, const int32_t* neighbours, const int32_t* degree, const int32_t* overflow, int L,
                    uint16_t* dist, const int64_t* dist_ptr, int32_t* component, int32_t* fragments, int32_t* fp) {
  const char* who = "egnn_topo_paths";
  if (int rc = topo_common_check(who, B, A, type, graph_ptr, max_atoms)) return rc;
  if (int rc = topo_atoms_check(who, N)) return rc;
  if (!row_ptr || !neighbours || !degree || !overflow) {
    set_error("bad %s arguments (row_ptr, neighbours, degree and overflow given)", who);
    return EGNN_EINVAL;
  }
  if (dist && !dist_ptr) { set_error("bad %s arguments (dist_ptr given with dist)", who); return EGNN_EINVAL; }
  if (int rc = topo_length_check(who, L)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // 64 KiB of bond lists at 1024 atoms beside 8 KiB of static LDS; a CU has 160 KiB
  static LdsLimitRecord raised;
  if (int rc = raise_lds_limit(raised, &topo_paths_kernel, sizeof(uint16_t) * kTopoMaxDegree * kTopoMaxAtoms)) return rc;
  if (fp) EGNN_HIP(hipMemsetAsync(fp, 0, sizeof(int32_t) * (size_t)B * topo_keys(A, L), st));
  const int npad = max_atoms > 0 ? (max_atoms + 63) / 64 * 64 : 64;
  hipLaunchKernelGGL(topo_paths_kernel, dim3(B), dim3(64 * kTopoPathWaves), sizeof(uint16_t) * kTopoMaxDegree * (size_t)npad, st, type,
                     graph_ptr, B, N, A, row_ptr, neighbours, degree, overflow, L, npad, dist, (const long long*)dist_ptr, component,
                     fragments, fp);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_topo_tanimoto(void* stream, int n_pairs, int K, const int32_t* fp_a, int rows_a, const int32_t* fp_b, int rows_b,
                       const int32_t* pairs, double* sim, int64_t* sa, int64_t* sb) {
  if (n_pairs < 1 || K < 1 || rows_a < 1 || rows_b < 1 || !fp_a || !fp_b || !sim || !sa || !sb) {
    set_error("bad egnn_topo_tanimoto arguments (n_pairs, K, rows >= 1; fp_a, fp_b, sim, sa and sb given)");
    return EGNN_EINVAL;
  }
  hipLaunchKernelGGL(topo_tanimoto_kernel, dim3((n_pairs + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), fp_a, rows_a,
                     fp_b, rows_b, pairs, n_pairs, K, sim, (long long*)sa, (long long*)sb);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

}  // extern "C"

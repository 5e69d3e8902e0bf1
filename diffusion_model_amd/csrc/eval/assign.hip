// Atom matching of large graphs on the device: what the reference's export script computes for graphs of six atoms or more
// before it writes files (create_xyz.py:157-192).
//
//  * assign_prealign_kernel (steps :158-176): one wavefront per graph.  The four atoms nearest to atom 0 of either structure
//    (return_near_from_exO, :87-96: a stable sort, so equal distances go to the lower index) are found by four rounds of a
//    cross-lane arg min.  Lanes 0..23 then fit one pairing each -- lane = rank of the permutation in itertools.permutations(
//    range(4)) order, generated_near[i+1] = gen[idx_gen[perm[i]]] against original_near[i+1] = orig[idx_orig[i]], atom 0 the
//    anchor -- with kabsch_fit (FIRST + FLIP_ROW, five points, fp64), and the smallest residual wins, equal residuals to the
//    lowest rank (the reference keeps the first strict minimum).
//  * assign_kernel (hungarian_algorithm, :82-85,182): exact shortest-augmenting-path solver of
//    min over permutations of sum_i |P_i - Q_col[i]|, one graph per workgroup.  The column side of the state -- coordinates,
//    dual v, path cost, predecessor, "scanned" bit -- lives in registers: one column per lane for n <= 64 (one wavefront),
//    kAssignCols columns per thread of a 256-thread workgroup above.  The row side (coordinates, dual u, the two matchings) is
//    in LDS.  The cost matrix exists nowhere: an entry is recomputed where it is used as the fp32 norm of the fp32 difference,
//    sqrtf((dx*dx + dy*dy) + dz*dz) uncontracted -- numpy.linalg.norm on float32 arrays -- widened to fp64; duals and path
//    costs are fp64 and are updated by the formulas of scipy's rectangular_lsap, in its operation order.  One step of an
//    augmentation = one relaxation of the owned columns, one butterfly arg min across the lanes (no LDS round trip) and, for
//    more than one wave, one exchange of per-wave partials through a double-buffered LDS slot (one barrier per step).
//    Tie rule and reproducibility: assign.h.
#include "assign.h"

#include <limits.h>

#include "eval_device.h"
#include "kabsch_math.h"

namespace egnn {
namespace {

__device__ __forceinline__ float dist32(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return sqrtf((dx * dx + dy * dy) + dz * dz);
}

// (value, index) order of every arg min here: the smaller value, equal values to the lower index
template <typename T>
__device__ __forceinline__ bool lower(T v, int j, T v0, int j0) { return v < v0 || (v == v0 && j < j0); }

template <typename T>
__device__ __forceinline__ void wave_argmin(T& v, int& j) {   // butterfly: every lane ends with the same pair
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const T v2 = __shfl_xor(v, m, 64);
    const int j2 = __shfl_xor(j, m, 64);
    if (lower(v2, j2, v, j)) { v = v2; j = j2; }
  }
}

struct AssignPartial {
  double v;
  int j;
  int pad;
};

// all threads of the solver meet here; one wavefront runs in lock step and its LDS operations complete in order, so it only
// has to keep the compiler from moving LDS accesses across this point (waves 1.. of its workgroup have left the kernel)
template <int WAVES>
__device__ __forceinline__ void solver_sync() {
  if constexpr (WAVES == 1) {
    wave_sync();
  } else {
    __syncthreads();
  }
}

// Thread tid of WAVES * 64 owns columns tid, tid + T, ..., tid + (K - 1) T.  n <= K T and n <= cap (the LDS arrays' length).
template <int WAVES, int K>
__device__ void assign_solve(const float* __restrict__ P, const float* __restrict__ Q, int n, int cap, int tid, double* lds,
                             int* __restrict__ col_out, double* __restrict__ cost_out, int* __restrict__ solved_out) {
  constexpr int T = WAVES * 64;
  double* u = lds;                                                         // [cap] row duals
  AssignPartial* red = reinterpret_cast<AssignPartial*>(u + cap);          // [2][kAssignWaves]
  float* prow = reinterpret_cast<float*>(red + 2 * kAssignWaves);          // [cap][3]
  int* row4col = reinterpret_cast<int*>(prow + 3 * cap);                   // [cap]
  int* col4row = row4col + cap;                                            // [cap]
  int* path = col4row + cap;                                               // [cap] predecessor row of a scanned column
  const int lane = tid & 63, wave = tid >> 6;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);

  for (int i = tid; i < n; i += T) {
    u[i] = 0.0;
    row4col[i] = -1;
    col4row[i] = -1;
    for (int d = 0; d < 3; ++d) prow[3 * i + d] = P[3 * i + d];
  }
  float qx[K], qy[K], qz[K];
  double v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int j = tid + k * T;
    qx[k] = j < n ? Q[3 * j] : 0.f;
    qy[k] = j < n ? Q[3 * j + 1] : 0.f;
    qz[k] = j < n ? Q[3 * j + 2] : 0.f;
    v[k] = 0.0;
  }
  solver_sync<WAVES>();

  bool failed = false;
  unsigned step = 0;   // parity picks the partials' buffer; runs on over the rows
  for (int cur = 0; cur < n && !failed; ++cur) {
    double sp[K];
    int pred[K];
    unsigned scanned = 0u;
#pragma unroll
    for (int k = 0; k < K; ++k) { sp[k] = inf; pred[k] = -1; }
    double min_val = 0.0;
    int i = cur, sink = -1;
    while (sink < 0) {
      const float pix = prow[3 * i], piy = prow[3 * i + 1], piz = prow[3 * i + 2];
      const double ui = u[i];
      double bv = inf;
      int bj = INT_MAX;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int j = tid + k * T;
        if (j < n && !((scanned >> k) & 1u)) {
          const double r = ((min_val + (double)dist32(pix, piy, piz, qx[k], qy[k], qz[k])) - ui) - v[k];
          if (r < sp[k]) { sp[k] = r; pred[k] = i; }
          if (lower(sp[k], j, bv, bj)) { bv = sp[k]; bj = j; }
        }
      }
      wave_argmin(bv, bj);
      if constexpr (WAVES > 1) {
        AssignPartial* buf = red + (step & 1u) * kAssignWaves;
        if (lane == 0) { buf[wave].v = bv; buf[wave].j = bj; }
        __syncthreads();
        bv = buf[0].v;
        bj = buf[0].j;
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
          const double v2 = buf[w].v;
          const int j2 = buf[w].j;
          if (lower(v2, j2, bv, bj)) { bv = v2; bj = j2; }
        }
        ++step;
      }
      if (bj >= n) { failed = true; break; }   // no column left: cannot happen while row cur is unmatched; never index with it
      min_val = bv;
      if ((bj % T) == tid) scanned |= 1u << (bj / T);
      const int r4 = row4col[bj];
      if (r4 < 0) sink = bj; else i = r4;
    }
    // an infinite path cost (NaN or infinite coordinates) leaves columns without a predecessor: stop, uniformly
    if (failed || !(min_val < inf)) { failed = true; break; }
    // duals (u of the scanned rows through the columns they are matched to, v of the scanned columns) and predecessors
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if ((scanned >> k) & 1u) {
        const int j = tid + k * T;
        const double delta = min_val - sp[k];
        const int r = row4col[j];
        if (r >= 0) u[r] += delta;
        v[k] -= delta;
        path[j] = pred[k];
      }
    }
    if (tid == 0) u[cur] += min_val;
    solver_sync<WAVES>();
    if (tid == 0) {   // augment along the predecessors; at most n columns
      int j = sink;
      for (int guard = 0; guard < n; ++guard) {
        const int r = path[j];
        if (r < 0 || r >= n) break;   // cannot happen with finite path costs; never index with it
        row4col[j] = r;
        const int next = col4row[r];
        col4row[r] = j;
        j = next;
        if (r == cur) break;
      }
    }
    solver_sync<WAVES>();
  }

  // cost of the assignment, summed in a fixed order
  double c = 0.0;
  bool ok = !failed;
  for (int i = tid; i < n && ok; i += T) {
    const int j = col4row[i];
    if (j < 0 || j >= n) { ok = false; break; }
    c += (double)dist32(prow[3 * i], prow[3 * i + 1], prow[3 * i + 2], Q[3 * j], Q[3 * j + 1], Q[3 * j + 2]);
  }
  c = wave_sum(ok ? c : inf);
  if constexpr (WAVES > 1) {
    AssignPartial* buf = red + (step & 1u) * kAssignWaves;
    if (lane == 0) buf[wave].v = c;
    __syncthreads();
    c = buf[0].v;
#pragma unroll
    for (int w = 1; w < WAVES; ++w) c += buf[w].v;
  }
  if (!(c < inf)) {   // NaN or infinite coordinates: not solved, nothing else written
    if (tid == 0) *solved_out = 0;
    return;
  }
  for (int i = tid; i < n; i += T) col_out[i] = col4row[i];
  if (tid == 0) {
    *cost_out = c;
    *solved_out = 1;
  }
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void assign_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                         const int* __restrict__ graph_ptr, int max_atoms, int cap,
                                                         int* __restrict__ col, double* __restrict__ cost, int* __restrict__ solved) {
  extern __shared__ double assign_lds[];
  const int g = blockIdx.x, tid = threadIdx.x, lo = graph_ptr[g], n = graph_ptr[g + 1] - lo;
  if (n < 1 || n > max_atoms || n > cap) {   // skipped: no work, nothing else written
    if (tid == 0) solved[g] = 0;
    return;
  }
  const float* p = P + 3 * (size_t)lo;
  const float* q = Q + 3 * (size_t)lo;
  if (n <= kAssignWaveAtoms) {
    if (tid >= 64) return;
    assign_solve<1, 1>(p, q, n, cap, tid, assign_lds, col + lo, cost + g, solved + g);
  } else if constexpr (THREADS > 64) {
    assign_solve<THREADS / 64, kAssignMaxAtoms / THREADS>(p, q, n, cap, tid, assign_lds, col + lo, cost + g, solved + g);
  }
}

// ---- pre-alignment -------------------------------------------------------------------------------------------------
// the four atoms nearest to atom 0 in ascending (distance, index) order; false when fewer than four have a distance (NaN)
__device__ bool nearest4(const float* __restrict__ x, int n, int lane, int* out) {
  float dprev = -1.f;
  int iprev = 0;
  for (int r = 0; r < 4; ++r) {
    float bd = __int_as_float(0x7f800000);
    int bi = INT_MAX;
    for (int i = 1 + lane; i < n; i += 64) {
      const float d = dist32(x[3 * i], x[3 * i + 1], x[3 * i + 2], x[0], x[1], x[2]);
      if ((d > dprev || (d == dprev && i > iprev)) && lower(d, i, bd, bi)) { bd = d; bi = i; }
    }
    wave_argmin(bd, bi);
    if (bi >= n) return false;
    out[r] = bi;
    dprev = bd;
    iprev = bi;
  }
  return true;
}

__global__ __launch_bounds__(64) void assign_prealign_kernel(const float* __restrict__ orig, const float* __restrict__ gen,
                                                             const int* __restrict__ graph_ptr, int min_atoms,
                                                             float* __restrict__ R_out, int* __restrict__ prealigned) {
  const int g = blockIdx.x, lane = threadIdx.x, lo = graph_ptr[g], n = graph_ptr[g + 1] - lo;
  const float* o = orig + 3 * (size_t)lo;
  const float* x = gen + 3 * (size_t)lo;
  int near_o[4], near_g[4];
  if (n < min_atoms || !nearest4(o, n, lane, near_o) || !nearest4(x, n, lane, near_g)) {   // wave-uniform
    if (lane == 0) prealigned[g] = 0;
    return;
  }
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, rmsd = inf;
  if (lane < 24) {
    int perm[4];
    unsigned mask = 15u;
    int rest = lane;
    const int fact[4] = {6, 2, 1, 1};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      unsigned m = mask;
      for (int s = rest / fact[k]; s > 0; --s) m &= m - 1;
      perm[k] = __ffs(m) - 1;
      mask &= ~(1u << perm[k]);
      rest %= fact[k];
    }
    double p[4][3], q[4][3], H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int src = near_g[0];
#pragma unroll
      for (int s = 1; s < 4; ++s) src = perm[k] == s ? near_g[s] : src;
      for (int d = 0; d < 3; ++d) {
        p[k][d] = (double)x[3 * src + d] - (double)x[d];
        q[k][d] = (double)o[3 * near_o[k] + d] - (double)o[d];
      }
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) H[3 * r + c] += p[k][r] * q[k][c];
    }
    kabsch_fit(H, kKabschFlipRow, R);
    double res = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      for (int r = 0; r < 3; ++r) {
        const double e = (R[3 * r] * p[k][0] + R[3 * r + 1] * p[k][1] + R[3 * r + 2] * p[k][2]) - q[k][r];
        res += e * e;
      }
    rmsd = sqrt(res / 5.0);   // five points: the anchor pair contributes 0
    if (!(rmsd == rmsd)) rmsd = inf;
  }
  int winner = lane;
  wave_argmin(rmsd, winner);
  if (!(rmsd < inf)) {   // no pairing has a finite residual (non-finite neighbour coordinates): no rotation; wave-uniform
    if (lane == 0) prealigned[g] = 0;
    return;
  }
  float out = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const double rk = __shfl(R[k], winner, 64);
    if (lane == k) out = (float)rk;
  }
  if (lane < 9) R_out[9 * (size_t)g + lane] = out;
  if (lane == 0) prealigned[g] = 1;
}

}  // namespace
}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_assign(void* stream, int B, const float* P, const float* Q, const int32_t* graph_ptr, int max_atoms, int32_t* col,
                double* cost, int32_t* solved) {
  const int rc = assign_args_check(B, P, Q, graph_ptr, max_atoms, col, cost, solved);
  if (rc != EGNN_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (max_atoms <= kAssignWaveAtoms) {
    const int cap = kAssignWaveAtoms;
    hipLaunchKernelGGL(assign_kernel<64>, dim3(B), dim3(64), assign_lds_bytes(cap), st, P, Q, graph_ptr, max_atoms, cap, col, cost,
                       solved);
  } else {
    const int cap = (max_atoms + 63) / 64 * 64;
    hipLaunchKernelGGL(assign_kernel<kAssignThreads>, dim3(B), dim3(kAssignThreads), assign_lds_bytes(cap), st, P, Q, graph_ptr,
                       max_atoms, cap, col, cost, solved);
  }
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_assign_prealign(void* stream, int B, const float* orig, const float* gen, const int32_t* graph_ptr, int min_atoms,
                         float* R, int32_t* prealigned) {
  const int rc = assign_prealign_args_check(B, orig, gen, graph_ptr, min_atoms, R, prealigned);
  if (rc != EGNN_OK) return rc;
  hipLaunchKernelGGL(assign_prealign_kernel, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), orig, gen, graph_ptr,
                     min_atoms, R, prealigned);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

}  // extern "C"

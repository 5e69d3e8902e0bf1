// Reciprocal-space statistics on the device: Debye sums D_ab(q) of a ragged batch of clusters, and for periodic cells the
// half-space reciprocal vectors below q_max, rho_a per vector and the shell averages of Re(rho_a rho_b*).  Definitions: sq_math.h
// (shared with the host statement, sq_host.cpp).  No file of the reference computes these: an extension, like rings.hip.
//
// Every floating-point sum is taken in fp64 in one fixed order and there is no floating-point atomic: a thread owns its
// accumulators, per-tile partial sums are added by a finishing pass in ascending tile index, and a shell adds its vectors in
// ascending vector index.  Two runs on the same input give the same bits, and a graph gives the same bits in any batch.
//
// Work lists come from the caller (built from the sizes on the host).  A kernel trusts no entry: graph / cell, blocks and offsets
// are checked against graph_ptr / vec_ptr / the plan, and every index a kernel forms lies inside the arrays the entry was given.
#include "sq_device.h"
#include "sq_host.h"

namespace egnn {

// ---- Debye sums ----------------------------------------------------------------------------------------------------------------
// tile {graph, first atom i, first atom j} (local indices): the pairs i < j of a 64 x 256 block, read and checked by
// pair_tile_read<kSqRowBlock, kSqChunk> (eval_device.h)
//
// One workgroup of 256 threads per tile.  The 64 atoms i and the 256 atoms j (positions, types) are staged in LDS.  For each atom
// i in turn, thread t takes the pair (i, j0 + t): r, the window and the unordered type pair go to LDS, ONCE per pair; then every
// thread walks the row's pairs for ITS q values (two per thread, 512 per pass), all lanes reading the same pair (LDS broadcasts).
// The type pair of a pair is therefore uniform in a wavefront: it is read into a scalar register and selects the accumulator by
// scalar branches, so the <= 10 accumulators per q stay in registers with no indexed access and no waterfall loop.
// partial [n_tiles, P, Q]: every entry of a valid tile is written.
__global__ __launch_bounds__(256) void sq_debye_kernel(const float* __restrict__ pos, const int* __restrict__ type,
                                                       const int* __restrict__ graph_ptr, int B, int A, const int* __restrict__ tiles,
                                                       const double* __restrict__ q, int Q, double r_max, int window,
                                                       double* __restrict__ partial) {
  __shared__ float s_pj[3 * kSqChunk], s_pi[3 * kSqRowBlock];
  __shared__ int s_tj[kSqChunk], s_ti[kSqRowBlock];
  __shared__ double s_r[kSqChunk], s_w[kSqChunk];
  __shared__ int s_p[kSqChunk];
  const int tid = threadIdx.x;
  PairTile T;
  if (!pair_tile_read<kSqRowBlock, kSqChunk>(tiles, blockIdx.x, graph_ptr, B, &T)) return;
  const int P = type_pairs(A);
  for (int t = tid; t < 3 * T.nj; t += 256) s_pj[t] = pos[3 * (size_t)(T.lo + T.j0) + t];
  for (int t = tid; t < T.nj; t += 256) s_tj[t] = type[T.lo + T.j0 + t];
  for (int t = tid; t < 3 * T.nc; t += 256) s_pi[t] = pos[3 * (size_t)(T.lo + T.c0) + t];
  for (int t = tid; t < T.nc; t += 256) s_ti[t] = type[T.lo + T.c0 + t];
  __syncthreads();
  double* out = partial + (size_t)blockIdx.x * P * Q;
  for (int qb = 0; qb < Q; qb += kSqQBlock) {
    const int k0 = qb + tid, k1 = qb + 256 + tid;
    const bool second = qb + 256 < Q;   // uniform
    const double q0 = k0 < Q ? q[k0] : 0.0, q1 = k1 < Q ? q[k1] : 0.0;
    double acc0[kSqMaxTypePairs], acc1[kSqMaxTypePairs];
#pragma unroll
    for (int p = 0; p < kSqMaxTypePairs; ++p) acc0[p] = acc1[p] = 0.0;
    for (int ii = 0; ii < T.nc; ++ii) {
      const int first = T.c0 + ii + 1 - T.j0;   // the first j of the chunk above i
      if (first >= T.nj) continue;              // uniform
      __syncthreads();                          // the previous row has been read
      {
        int p = -1;
        double r = 0.0, w = 0.0;
        const int ti = s_ti[ii];
        if (tid < T.nj && tid >= first && ti >= 0 && ti < A) {
          const int tj = s_tj[tid];
          r = distance64(s_pi[3 * ii], s_pi[3 * ii + 1], s_pi[3 * ii + 2], s_pj[3 * tid], s_pj[3 * tid + 1], s_pj[3 * tid + 2]);
          if (tj >= 0 && tj < A && r < r_max) {
            p = type_pair_index(ti, tj, A);
            w = sq_window(r, r_max, window);
          }
        }
        s_r[tid] = r;
        s_w[tid] = w;
        s_p[tid] = p;
      }
      __syncthreads();
      for (int e = max(first, 0); e < T.nj; ++e) {
        const int pp = __builtin_amdgcn_readfirstlane(s_p[e]);
        if (pp < 0) continue;
        const double r = s_r[e], w = s_w[e];
        const double t0 = w * sq_sinc(q0 * r);
        double t1 = 0.0;
        if (second) t1 = w * sq_sinc(q1 * r);
#pragma unroll
        for (int p = 0; p < kSqMaxTypePairs; ++p)
          if (pp == p) {
            asm volatile("");   // keeps the scalar branch: without it the compiler turns the ten cases into ten selects and adds
            acc0[p] += t0;
            acc1[p] += t1;
          }
      }
    }
#pragma unroll
    for (int p = 0; p < kSqMaxTypePairs; ++p)
      if (p < P) {
        if (k0 < Q) out[(size_t)p * Q + k0] = acc0[p];
        if (k1 < Q) out[(size_t)p * Q + k1] = acc1[p];
      }
  }
}

// D[g][a][b][q] = the partial sums of the graph's tiles, added in ascending tile index (tile_ptr [B+1]: the tiles of graph g),
// doubled on the diagonal.  One thread per output; an entry of tile_ptr outside [0, n_tiles], or a tile of another graph, adds nothing.
__global__ __launch_bounds__(256) void sq_debye_finish_kernel(const int* __restrict__ graph_ptr, int B, int A, const int* __restrict__ tiles,
                                                              int n_tiles, const int* __restrict__ tile_ptr,
                                                              const double* __restrict__ partial, int Q, double* __restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)B * A * A * Q) return;
  const int k = (int)(idx % Q), ab = (int)(idx / Q % (A * A)), g = (int)(idx / Q / (A * A));
  const int a = ab / A, b = ab % A, P = type_pairs(A), p = type_pair_index(a, b, A);
  const int t_lo = min(max(tile_ptr[g], 0), n_tiles), t_hi = min(max(tile_ptr[g + 1], t_lo), n_tiles);
  double sum = 0.0;
  for (int t = t_lo; t < t_hi; ++t) {
    PairTile T;
    if (!pair_tile_read<kSqRowBlock, kSqChunk>(tiles, t, graph_ptr, B, &T) || T.g != g) continue;
    sum += partial[((size_t)t * P + p) * Q + k];
  }
  out[idx] = a == b ? 2.0 * sum : sum;
}

// ---- cells: the vectors ----------------------------------------------------------------------------------------------------------
// the (h, k) rows of a cell's index box are read by sq_row_read (sq_device.h)

// one thread per (h, k) row of the index box of cell blockIdx.y: the number of its l that are vectors
__global__ __launch_bounds__(256) void sq_cell_count_kernel(const int* __restrict__ plan, const double* __restrict__ lattice, double q_max,
                                                            int n_rows, int* __restrict__ row_count) {
  SqRow R;
  if (!sq_row_read(plan, lattice, blockIdx.y, blockIdx.x * 256 + threadIdx.x, n_rows, &R)) return;
  row_count[R.row] = sq_row_vectors(R.h, R.k, R.Lb, R.Bm, q_max, [](int, int, double) {});
}

// the same walk, writing (h, k, l), |k| and the shell bin of the row's vectors from row_ptr[row] on: ascending (h, k, l) in a cell
__global__ __launch_bounds__(256) void sq_cell_fill_kernel(const int* __restrict__ plan, const double* __restrict__ lattice, double q_max,
                                                           double dq, int nbins, int n_rows, const int* __restrict__ row_ptr, int K,
                                                           int* __restrict__ hkl, double* __restrict__ kabs, int* __restrict__ bin) {
  SqRow R;
  if (!sq_row_read(plan, lattice, blockIdx.y, blockIdx.x * 256 + threadIdx.x, n_rows, &R)) return;
  const int v0 = row_ptr[R.row], v1 = row_ptr[R.row + 1];
  if (v0 < 0 || v1 < v0 || v1 > K) return;
  sq_row_vectors(R.h, R.k, R.Lb, R.Bm, q_max, [&](int n, int l, double k2) {
    const int v = v0 + n;
    if (v >= v1) return;
    const double ka = sqrt(k2);
    hkl[3 * (size_t)v] = R.h;
    hkl[3 * (size_t)v + 1] = R.k;
    hkl[3 * (size_t)v + 2] = l;
    kabs[v] = ka;
    bin[v] = sq_bin(ka, dq, nbins);
  });
}

// ---- cells: rho_a per vector -----------------------------------------------------------------------------------------------------
// One workgroup of 256 threads per tile {cell, first vector (local)}: a thread owns one vector.  The cell's atoms (wrapped
// fractional coordinates in fp64, types) are staged in LDS 1024 at a time and shared by the block's vectors; all lanes read the
// same atom (LDS broadcasts), so the atom's type is uniform in a wavefront and selects the accumulator by scalar branches.
// Atoms are added in ascending index.  rho [K, A, 2] = (re, im).
__global__ __launch_bounds__(256) void sq_cell_rho_kernel(const int* __restrict__ cell_ptr, const int* __restrict__ vec_ptr, int C, int N,
                                                          int A, const double* __restrict__ frac, const int* __restrict__ type,
                                                          const int* __restrict__ tiles, const int* __restrict__ hkl, int K,
                                                          double* __restrict__ rho) {
  __shared__ double s_w[3 * kSqAtomChunk];
  __shared__ int s_t[kSqAtomChunk];
  const int tid = threadIdx.x;
  const int c = tiles[2 * blockIdx.x], v_first = tiles[2 * blockIdx.x + 1];
  if (c < 0 || c >= C || v_first < 0) return;
  const int lo = cell_ptr[c], hi = cell_ptr[c + 1];
  const int v_lo = vec_ptr[c], v_hi = vec_ptr[c + 1];
  if (lo < 0 || hi < lo || hi > N || v_lo < 0 || v_hi < v_lo || v_hi > K || v_first >= v_hi - v_lo) return;
  const int v = v_lo + v_first + tid;
  const bool live = v < v_hi;
  const int h = live ? hkl[3 * (size_t)v] : 0, k = live ? hkl[3 * (size_t)v + 1] : 0, l = live ? hkl[3 * (size_t)v + 2] : 0;
  double re[kSqMaxTypes] = {0.0, 0.0, 0.0, 0.0}, im[kSqMaxTypes] = {0.0, 0.0, 0.0, 0.0};
  for (int j0 = lo; j0 < hi; j0 += kSqAtomChunk) {
    const int m = min(kSqAtomChunk, hi - j0);
    __syncthreads();
    for (int t = tid; t < 3 * m; t += 256) s_w[t] = cell_wrap(frac[3 * (size_t)j0 + t]);
    for (int t = tid; t < m; t += 256) s_t[t] = type[j0 + t];
    __syncthreads();
    for (int j = 0; j < m; ++j) {
      const int tj = __builtin_amdgcn_readfirstlane(s_t[j]);
      if (tj < 0 || tj >= A) continue;
      double sn, cs;
      sq_phase_sincos(sq_phase(h, k, l, &s_w[3 * j]), &sn, &cs);
#pragma unroll
      for (int a = 0; a < kSqMaxTypes; ++a)
        if (tj == a) {
          asm volatile("");   // keeps the scalar branch (sq_debye_kernel)
          re[a] += cs;
          im[a] -= sn;
        }
    }
  }
  if (live) {
#pragma unroll
    for (int a = 0; a < kSqMaxTypes; ++a)
      if (a < A) {
        rho[((size_t)v * A + a) * 2] = re[a];
        rho[((size_t)v * A + a) * 2 + 1] = im[a];
      }
  }
}

// ---- cells: shell averages -------------------------------------------------------------------------------------------------------
// One workgroup of 256 threads per (cell, bin).  It walks the cell's vectors 1024 at a time (coalesced reads of the bin array),
// compacts the indices of those in its bin into an LDS list IN ASCENDING ORDER (ballot + popcount, as the neighbour lists of
// structure.hip), and threads 0 .. A*A add the listed vectors one after the other: thread ab < A*A the product Re(rho_a rho_b*),
// thread A*A the |k|.  So every sum runs over the bin's vectors in ascending vector index.
__global__ __launch_bounds__(256) void sq_cell_shell_kernel(const int* __restrict__ vec_ptr, int A, int nbins, int K,
                                                            const double* __restrict__ kabs, const int* __restrict__ bin,
                                                            const double* __restrict__ rho, long long* __restrict__ count,
                                                            double* __restrict__ mean_k, double* __restrict__ s) {
  constexpr int kSlices = kSqShellBlock / 256;
  __shared__ int s_cnt[kSlices * 4];
  __shared__ int s_list[kSqShellBlock];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.y, b = blockIdx.x;
  const int v_lo = vec_ptr[c], v_hi = vec_ptr[c + 1];
  double acc = 0.0;
  long long n_half = 0;
  const bool valid = v_lo >= 0 && v_hi >= v_lo && v_hi <= K;   // uniform
  const int a_of = tid / A, b_of = tid % A;
  for (int base = valid ? v_lo : 0; valid && base < v_hi; base += kSqShellBlock) {
    bool match[kSlices];
    unsigned long long mask[kSlices];
#pragma unroll
    for (int sl = 0; sl < kSlices; ++sl) {
      const int v = base + sl * 256 + tid;
      match[sl] = v < v_hi && bin[v] == b;
    }
#pragma unroll
    for (int sl = 0; sl < kSlices; ++sl) {
      mask[sl] = __ballot(match[sl]);
      if (lane == 0) s_cnt[sl * 4 + wave] = __popcll(mask[sl]);
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int sl = 0; sl < kSlices; ++sl)
#pragma unroll
      for (int wv = 0; wv < 4; ++wv) {
        if (match[sl] && wv == wave) s_list[total + lane_prefix(mask[sl], lane)] = base + sl * 256 + tid;
        total += s_cnt[sl * 4 + wv];
      }
    __syncthreads();
    if (tid < A * A) {
      for (int e = 0; e < total; ++e) {
        const double* r = rho + (size_t)s_list[e] * A * 2;
        acc += r[2 * a_of] * r[2 * b_of] + r[2 * a_of + 1] * r[2 * b_of + 1];
      }
    } else if (tid == A * A) {
      for (int e = 0; e < total; ++e) acc += kabs[s_list[e]];
      n_half += total;
    }
    __syncthreads();   // the list and the counts are rewritten by the next step
  }
  if (tid == A * A) {
    count[(size_t)c * nbins + b] = 2 * n_half;
    mean_k[(size_t)c * nbins + b] = n_half > 0 ? acc / (double)n_half : NAN;
    s_cnt[0] = (int)min(n_half, (long long)kSqMaxVectors);
  }
  __syncthreads();
  if (tid < A * A) {
    const int m = s_cnt[0];
    s[((size_t)c * A * A + tid) * nbins + b] = m > 0 ? acc / (double)m : NAN;
  }
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_sq_debye(void* stream, int B, int A, const float* d_pos, const int32_t* d_type, const int32_t* d_graph_ptr, int max_atoms, int Q,
                  const double* q, const double* d_q, double r_max, int window, const int32_t* d_tiles, int n_tiles,
                  const int32_t* d_tile_ptr, double* d_partial, double* d_out) {
  const char* who = "egnn_sq_debye";
  if (int rc = sq_debye_args_check(who, B, A, d_pos, d_type, d_graph_ptr, max_atoms, Q, q, r_max, window, d_out)) return rc;
  if (!d_q) { set_error("bad %s arguments (the device copy of q given)", who); return EGNN_EINVAL; }
  if (int rc = sq_tiles_args_check(who, d_tiles, n_tiles, d_tile_ptr, d_partial)) return rc;
  const size_t n_out = (size_t)B * A * A * Q;
  if ((n_out + 255) / 256 > 2147483647ull) { set_error("%s: B * A * A * Q exceeds the grid", who); return EGNN_EINVAL; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (n_tiles > 0)
    hipLaunchKernelGGL(sq_debye_kernel, dim3(n_tiles), dim3(256), 0, st, d_pos, d_type, d_graph_ptr, B, A, d_tiles, d_q, Q, r_max, window,
                       d_partial);
  hipLaunchKernelGGL(sq_debye_finish_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, d_graph_ptr, B, A, d_tiles, n_tiles,
                     d_tile_ptr, d_partial, Q, d_out);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_sq_cell_count(void* stream, int C, const double* lattice, const int32_t* plan, const double* d_lattice, const int32_t* d_plan,
                       double q_max, int n_rows, int32_t* d_row_count) {
  const char* who = "egnn_sq_cell_count";
  if (int rc = sq_cells_check(who, C, 1, nullptr, lattice, q_max, nullptr)) return rc;
  int max_rows = 0;
  if (int rc = sq_plan_check(who, C, lattice, q_max, plan, n_rows, &max_rows)) return rc;
  if (!d_lattice || !d_plan || !d_row_count) { set_error("bad %s arguments (the device copies and row_count given)", who); return EGNN_EINVAL; }
  hipLaunchKernelGGL(sq_cell_count_kernel, dim3((max_rows + 255) / 256, C), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_plan,
                     d_lattice, q_max, n_rows, d_row_count);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_sq_cell_rho(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* plan,
                     const int32_t* vec_ptr, const int32_t* d_cell_ptr, const double* d_lattice, const int32_t* d_plan,
                     const int32_t* d_vec_ptr, const double* d_frac, const int32_t* d_type, double q_max, double dq, int nbins, int n_rows,
                     const int32_t* d_row_ptr, int K, const int32_t* d_tiles, int n_tiles, int32_t* d_hkl, double* d_k, int32_t* d_bin,
                     double* d_rho) {
  const char* who = "egnn_sq_cell_rho";
  if (N < 0 || !cell_ptr || cell_ptr[0] != 0 || (C >= 1 && C <= 65535 && cell_ptr[C] != N)) {
    set_error("%s: the host copy of cell_ptr must run from 0 to N = %d", who, N);
    return EGNN_EINVAL;
  }
  if (int rc = sq_cells_check(who, C, A, cell_ptr, lattice, q_max, nullptr)) return rc;
  if (int rc = sq_bins_check(who, q_max, dq, nbins)) return rc;
  int max_rows = 0;
  if (int rc = sq_plan_check(who, C, lattice, q_max, plan, n_rows, &max_rows)) return rc;
  if (int rc = sq_vec_ptr_check(who, C, vec_ptr, K)) return rc;
  if (!d_cell_ptr || !d_lattice || !d_plan || !d_vec_ptr || !d_row_ptr || (N > 0 && (!d_frac || !d_type))) {
    set_error("bad %s arguments (the device copies of the cells, the plan, vec_ptr and row_ptr given)", who);
    return EGNN_EINVAL;
  }
  if (n_tiles < 0 || (n_tiles > 0 && !d_tiles) || (K > 0 && (!d_hkl || !d_k || !d_bin || !d_rho))) {
    set_error("bad %s arguments (n_tiles >= 0 tiles and the four outputs given)", who);
    return EGNN_EINVAL;
  }
  if (K == 0) return EGNN_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sq_cell_fill_kernel, dim3((max_rows + 255) / 256, C), dim3(256), 0, st, d_plan, d_lattice, q_max, dq, nbins, n_rows,
                     d_row_ptr, K, d_hkl, d_k, d_bin);
  EGNN_HIP(hipMemsetAsync(d_rho, 0, sizeof(double) * (size_t)K * A * 2, st));
  if (n_tiles > 0)
    hipLaunchKernelGGL(sq_cell_rho_kernel, dim3(n_tiles), dim3(256), 0, st, d_cell_ptr, d_vec_ptr, C, N, A, d_frac, d_type, d_tiles, d_hkl,
                       K, d_rho);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_sq_cell_shells(void* stream, int C, int A, int nbins, const int32_t* vec_ptr, const int32_t* d_vec_ptr, int K, const double* d_k,
                        const int32_t* d_bin, const double* d_rho, int64_t* d_count, double* d_mean_k, double* d_s) {
  const char* who = "egnn_sq_cell_shells";
  if (C < 1 || C > 65535 || A < 1 || A > kSqMaxTypes || nbins < 1 || nbins > kSqMaxBins) {
    set_error("%s: C %d, A %d, nbins %d (1 <= C <= 65535, 1 <= A <= %d, 1 <= nbins <= %d)", who, C, A, nbins, kSqMaxTypes, kSqMaxBins);
    return EGNN_EINVAL;
  }
  if (int rc = sq_vec_ptr_check(who, C, vec_ptr, K)) return rc;
  if (!d_vec_ptr || !d_count || !d_mean_k || !d_s || (K > 0 && (!d_k || !d_bin || !d_rho))) {
    set_error("bad %s arguments (vec_ptr, the per-vector arrays and the three outputs given)", who);
    return EGNN_EINVAL;
  }
  hipLaunchKernelGGL(sq_cell_shell_kernel, dim3(nbins, C), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_vec_ptr, A, nbins, K, d_k,
                     d_bin, d_rho, reinterpret_cast<long long*>(d_count), d_mean_k, d_s);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

}  // extern "C"

// Linked-cell search of periodic cells on the device: the atoms of a cell are binned on a grid whose bins are at least
// radius / reach thick and sorted by (bin, atom index); the periodic bond list and the partial pair counts are then found among the
// (2 reach + 1)^3 bins about a centre instead of among every atom of the cell.  Definitions: cell_grid_math.h (shared with the host
// statement, cell_grid_host.cpp).  An extension: no file of the reference bins a cell.  The grid only chooses which sites (j, s) are
// tested; the test is the text of cell_math.h / cell_stats_math.h that cell_bond_kernel and cell_pair_kernel compile, one site
// vector with exactly that s, so the outputs hold the bits of the direct kernels.
//
// Nothing here depends on arrival order: the place of an atom inside its bin is its rank by atom index (an atomic hands out a slot in
// a work array only), a bond row is written at the rank of its keys, and every accumulator is an integer.  Results are bitwise
// identical from run to run and a cell gives the same bits alone and in any batch.
//
// A kernel trusts no index: tile, cell, grid, bin, bin range, sorted atom, bond row and shift code are checked against the extents
// of the arrays before they are used, and every write is checked against the extent of its output.
#include "cell_device.h"
#include "cell_grid_host.h"
#include "cell_grid_math.h"

namespace egnn {

// a gridded cell as a kernel reads it: atoms [lo, lo + n), grid nb, its bins [first, first + bins) of the batch's bin arrays and
// `base`, the sorted position bin_start[first] its first bin starts at (bin_start counts over the gridded atoms of the whole batch)
struct GridCell {
  int lo, n, nb[3], first, bins, base;
};

__device__ __forceinline__ bool grid_cell_read(int c, const int* __restrict__ cell_ptr, int C, int N, const int* __restrict__ nbv,
                                               const int* __restrict__ bin_ptr, int n_bins, const int* __restrict__ bin_start,
                                               GridCell* G) {
  if (!cell_read(c, cell_ptr, C, N, &G->lo, &G->n)) return false;
  for (int k = 0; k < 3; ++k) {
    G->nb[k] = nbv[3 * (size_t)c + k];
    if (G->nb[k] < 1 || G->nb[k] > kCellGridMaxBins) return false;
  }
  G->first = bin_ptr[c];
  G->bins = G->nb[0] * G->nb[1] * G->nb[2];
  if (G->first < 0 || G->first > n_bins - G->bins) return false;
  G->base = bin_start ? bin_start[G->first] : 0;
  return true;
}

// the atoms of bin cb as sorted positions [p0, p0 + cnt) inside the cell; cnt = 0 where bin_start is not what the prefix sum gave
__device__ __forceinline__ void grid_bin_range(const GridCell& G, const int* __restrict__ bin_start, int cb, int* p0, int* cnt) {
  *p0 = 0;
  *cnt = 0;
  if (cb < 0 || cb >= G.bins) return;
  const int a = bin_start[G.first + cb] - G.base, b = bin_start[G.first + cb + 1] - G.base;
  if (a < 0 || b < a || b > G.n) return;
  *p0 = a;
  *cnt = b - a;
}

// the cell of atom i, -1 where cell_ptr does not hold i
__device__ __forceinline__ int grid_cell_of(const int* __restrict__ cell_ptr, int C, int N, int i) {
  int c, lo, hi;
  return cell_of_atom(cell_ptr, C, N, i, &c, &lo, &hi) ? c : -1;
}

// ---- binning -------------------------------------------------------------------------------------------------------------------
// One thread per atom: its flat bin (-1 in a cell that is not gridded) and one integer atomic on the bin's count.
__global__ __launch_bounds__(256) void cell_grid_bin_kernel(const double* __restrict__ frac, const int* __restrict__ cell_ptr, int C, int N,
                                                            const int* __restrict__ nbv, const int* __restrict__ bin_ptr, int n_bins,
                                                            int* __restrict__ atom_bin, int* __restrict__ bin_count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int bin = -1;
  const int c = grid_cell_of(cell_ptr, C, N, i);
  GridCell G;
  if (c >= 0 && nbv[3 * (size_t)c] != 0 && grid_cell_read(c, cell_ptr, C, N, nbv, bin_ptr, n_bins, nullptr, &G)) {
    bin = cell_grid_bin(frac + 3 * (size_t)i, G.nb);
    atomicAdd(&bin_count[G.first + bin], 1);   // bin < G.bins by the clamp of cell_grid_axis_bin; first + bins <= n_bins
  }
  atom_bin[i] = bin;
}

// Fill, first step: an atomic hands every atom a slot of its bin in the work array `arrival` (arrival order: not an output).
__global__ __launch_bounds__(256) void cell_grid_scatter_kernel(const int* __restrict__ cell_ptr, int C, int N, const int* __restrict__ nbv,
                                                                const int* __restrict__ bin_ptr, int n_bins,
                                                                const int* __restrict__ bin_start, const int* __restrict__ atom_bin,
                                                                int* __restrict__ cursor, int* __restrict__ arrival) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int bin = atom_bin[i];
  if (bin < 0) return;
  const int c = grid_cell_of(cell_ptr, C, N, i);
  GridCell G;
  if (c < 0 || !grid_cell_read(c, cell_ptr, C, N, nbv, bin_ptr, n_bins, bin_start, &G)) return;
  int p0, cnt;
  grid_bin_range(G, bin_start, bin, &p0, &cnt);
  if (cnt == 0) return;
  const int slot = atomicAdd(&cursor[G.first + bin], 1);
  if (slot >= 0 && slot < cnt) arrival[G.lo + p0 + slot] = i;
}

// Fill, second step: the place of an atom inside its bin is the number of atoms of the bin with a smaller index (bins are small);
// the sorted atom, its wrapped coordinates and its type are written there.
__global__ __launch_bounds__(256) void cell_grid_rank_kernel(const double* __restrict__ frac, const int* __restrict__ type,
                                                             const int* __restrict__ cell_ptr, int C, int N, const int* __restrict__ nbv,
                                                             const int* __restrict__ bin_ptr, int n_bins, const int* __restrict__ bin_start,
                                                             const int* __restrict__ atom_bin, const int* __restrict__ arrival,
                                                             int* __restrict__ sorted_atom, double* __restrict__ sorted_frac,
                                                             int* __restrict__ sorted_type) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int bin = atom_bin[i];
  if (bin < 0) return;
  const int c = grid_cell_of(cell_ptr, C, N, i);
  GridCell G;
  if (c < 0 || !grid_cell_read(c, cell_ptr, C, N, nbv, bin_ptr, n_bins, bin_start, &G)) return;
  int p0, cnt;
  grid_bin_range(G, bin_start, bin, &p0, &cnt);
  int rank = 0;
  bool seen = false;
  for (int p = 0; p < cnt; ++p) {
    const int j = arrival[G.lo + p0 + p];
    rank += j >= 0 && j < i;
    seen = seen || j == i;
  }
  if (!seen || rank >= cnt) return;   // the bin does not hold this atom: bin_start is not the prefix sum of the count pass
  const size_t at = (size_t)G.lo + p0 + rank;
  sorted_atom[at] = i;
  cell_wrapped_read(frac, i, sorted_frac + 3 * at);
  sorted_type[at] = type[i];
}

// ---- periodic bond list over the grid ---------------------------------------------------------------------------------------------
// The candidates of one centre, walked by one wavefront: the (2 reach + 1)^3 offsets are dealt to the lanes 64 at a time, a lane
// reads the range of its bin, an inclusive scan over the wavefront lays the ranges end to end, and the lanes then take the
// candidates 64 at a time, each finding its (bin, atom) by a binary search over the scanned ranges (shuffles, no LDS).  A lane tests
// ONE site (j, s).  `f(hit, key, found)` is called once per step by the whole wavefront; found = bonds before this step.
template <typename F>
__device__ __forceinline__ int grid_walk_bonds(const GridCell& G, const int* __restrict__ bin_start, const int* __restrict__ sorted_atom,
                                               const double* __restrict__ sorted_frac, const double* L, const double* wi, const int* b,
                                               int i, double c2, int reach, int lane, F&& f) {
  const int span = 2 * reach + 1, T = span * span * span, hi = G.lo + G.n;
  int found = 0;
  for (int tb = 0; tb < T; tb += 64) {
    const int t = tb + lane;
    int p0 = 0, cnt = 0, code = kCellCentreCode;
    if (t < T) {
      int s[3];
      const int cb = cell_grid_candidate(b, G.nb, reach, t, s);
      code = cell_shift_code(s[0], s[1], s[2]);
      grid_bin_range(G, bin_start, cb, &p0, &cnt);
    }
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    const int total = __shfl(incl, 63), excl = incl - cnt;
    for (int q0 = 0; q0 < total; q0 += 64) {
      const int q = q0 + lane;
      int tl = 0;   // the last lane whose range starts at or before q: excl is ascending, and that lane's range holds q
#pragma unroll
      for (int step = 32; step > 0; step >>= 1) {
        const int cand = tl + step;
        const int e = __shfl(excl, cand & 63);
        if (cand < 64 && e <= q) tl = cand;
      }
      const int e_t = __shfl(excl, tl), p_t = __shfl(p0, tl), n_t = __shfl(cnt, tl), code_t = __shfl(code, tl);
      bool hit = false;
      int key = 0;
      if (q < total && q - e_t < n_t) {
        const size_t at = (size_t)G.lo + p_t + (q - e_t);   // p_t + n_t <= n by grid_bin_range
        const int j = sorted_atom[at];
        if (j >= G.lo && j < hi && !(j == i && code_t == kCellCentreCode)) {
          int s[3];
          double r[3];
          cell_shift_decode(code_t, s);
          cell_site_vector(sorted_frac + 3 * at, wi, s, L, r);
          hit = cell_norm2(r) < c2;
          key = (j - G.lo) * kCellShiftCodes + code_t;
        }
      }
      const unsigned long long hits = __ballot(hit);
      f(hit, key, found + lane_prefix(hits, lane));
      found += __popcll(hits);
    }
  }
  return found;
}

// One workgroup of 256 threads per tile {cell, first centre}: 64 centres IN SORTED ORDER (neighbouring centres share bins and
// cache lines), 16 per wavefront, one at a time, so the centre's bin and coordinates are uniform in a wavefront.  Count: the degree
// is a sum of ballot popcounts and is written at the centre's ORIGINAL index.  Fill: a row must come out ascending by key
// (atom 729 + shift code) while the candidates arrive in bin order, so the wavefront stages the keys of the row in LDS
// (kCellGridRowKeys = 128 keys, two per lane) and writes each at row_lo + #{smaller keys}.  A row above the capacity is ranked in
// pieces: piece P is staged, then every other piece Q is staged in turn beside it (the walk is repeated) and the smaller keys are
// counted across all of them.  LDS: 2 x 128 keys per wavefront, 4 KiB per workgroup.
template <bool FILL>
__global__ __launch_bounds__(256) void cell_bond_grid_kernel(const double* __restrict__ lattice, const int* __restrict__ cell_ptr, int C, int N,
                                                             const int* __restrict__ nbv, const int* __restrict__ bin_ptr, int n_bins,
                                                             const int* __restrict__ bin_start, const int* __restrict__ sorted_atom,
                                                             const double* __restrict__ sorted_frac, const int* __restrict__ tiles,
                                                             double cutoff, int reach, const int* __restrict__ row_ptr, int n_bonds,
                                                             int* __restrict__ degree, int* __restrict__ bond_atom,
                                                             int* __restrict__ bond_shift) {
  static_assert(kCellGridRowKeys == 128, "two keys per lane");
  __shared__ int s_keys[kWaves][2][kCellGridRowKeys];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = tiles[2 * (size_t)blockIdx.x], c0 = tiles[2 * (size_t)blockIdx.x + 1];
  GridCell G;
  if (reach < 1 || reach > kCellGridMaxReach || !grid_cell_read(c, cell_ptr, C, N, nbv, bin_ptr, n_bins, bin_start, &G)) return;
  for (int k = 0; k < 3; ++k)
    if (G.nb[k] < 2 * reach + 1) return;
  int nc;
  if (!cell_block_read<kCellCentreBlock>(c0, G.n, &nc)) return;
  const int hi = G.lo + G.n;
  double L[9];
  cell_lattice_read(lattice, c, L);
  const double c2 = cutoff * cutoff;
  constexpr int per_wave = kCellCentreBlock / kWaves;
  const int ci_end = min(nc, (wave + 1) * per_wave);
  int* buf_a = s_keys[wave][0];
  int* buf_b = s_keys[wave][1];
  for (int ci = wave * per_wave; ci < ci_end; ++ci) {   // uniform in a wavefront
    const size_t pos = (size_t)G.lo + c0 + ci;
    const int i = sorted_atom[pos];
    if (i < G.lo || i >= hi) continue;
    const double wi[3] = {sorted_frac[3 * pos], sorted_frac[3 * pos + 1], sorted_frac[3 * pos + 2]};
    int b[3];
    cell_grid_unflat(cell_grid_bin(wi, G.nb), G.nb, b);
    if (!FILL) {
      const int deg = grid_walk_bonds(G, bin_start, sorted_atom, sorted_frac, L, wi, b, i, c2, reach, lane, [](bool, int, int) {});
      if (lane == 0) degree[i] = deg;
      continue;
    }
    int row_lo, row_hi;
    if (!cell_row_read(row_ptr, N, n_bonds, i, &row_lo, &row_hi)) continue;
    const int deg = row_hi - row_lo, pieces = (deg + kCellGridRowKeys - 1) / kCellGridRowKeys;
    for (int P = 0; P < pieces; ++P) {
      auto stage = [&](int* buf, int piece) {
        wave_sync();   // the readers of this buffer are done
        grid_walk_bonds(G, bin_start, sorted_atom, sorted_frac, L, wi, b, i, c2, reach, lane, [&](bool hit, int key, int at) {
          const int e = at - piece * kCellGridRowKeys;
          if (hit && e >= 0 && e < kCellGridRowKeys) buf[e] = key;
        });
        wave_sync();
      };
      stage(buf_a, P);
      const int n_a = min(kCellGridRowKeys, deg - P * kCellGridRowKeys);
      const int k0 = lane < n_a ? buf_a[lane] : 0, k1 = lane + 64 < n_a ? buf_a[lane + 64] : 0;
      int r0 = 0, r1 = 0;
      for (int Q = 0; Q < pieces; ++Q) {
        const int* src = buf_a;
        if (Q != P) {
          stage(buf_b, Q);
          src = buf_b;
        }
        const int n_q = min(kCellGridRowKeys, deg - Q * kCellGridRowKeys);
        for (int e = 0; e < n_q; ++e) {
          const int v = src[e];   // one address for the wavefront: a broadcast
          r0 += v < k0;
          r1 += v < k1;
        }
      }
      if (lane < n_a) {
        const int at = row_lo + r0;
        if (at >= row_lo && at < row_hi && at < n_bonds && k0 >= 0) {
          bond_atom[at] = G.lo + k0 / kCellShiftCodes;
          bond_shift[at] = k0 % kCellShiftCodes;
        }
      }
      if (lane + 64 < n_a) {
        const int at = row_lo + r1;
        if (at >= row_lo && at < row_hi && at < n_bonds && k1 >= 0) {
          bond_atom[at] = G.lo + k1 / kCellShiftCodes;
          bond_shift[at] = k1 % kCellShiftCodes;
        }
      }
    }
  }
}

// ---- ordered pairs over the grid -> c[cell][a][b][k] ---------------------------------------------------------------------------------
// One workgroup of 256 threads per tile {cell, first centre}: 64 consecutive SORTED centres of a cell.  Sorted centres fall into
// runs of one bin; the workgroup takes the runs one after the other.  For a run it lists the (2 reach + 1)^3 candidate bins with
// their shifts -- the shift depends on the centre's bin and the offset alone, so it is STAGED PER BIN OFFSET, with the atom, and not
// recomputed in the walk -- lays their ranges end to end by a workgroup scan, and stages the candidates in chunks of <= 1024: wrapped
// coordinates (fp64, one array per axis), type and shift code packed in one int, and the sorted position (the self test).  The
// threads are dealt as (centre of the run, slice): a run of ns centres has 256 / ns slices, so a run of two centres still uses
// every lane.  There is no image loop: a thread tests one site per staged atom, the r2 cull of cell_stat_r2_limit before the
// square root, and what counts is decided by cell_stat_bin alone.
//
// Dynamic LDS: the histogram of cell_pair_kernel, A A nbins unsigned 32-bit bins (<= 64 KiB), flushed by one 64-bit global add per
// non-zero bin.  A tile holds fewer than 64 x 2^20 terms (a site is a candidate of a centre once): a bin cannot wrap.  Static LDS:
// 32 KiB of staged candidates and 4 KiB of offset tables.
__global__ __launch_bounds__(256) void cell_pair_grid_kernel(const double* __restrict__ lattice, const int* __restrict__ cell_ptr, int C, int N,
                                                             int A, const int* __restrict__ nbv, const int* __restrict__ bin_ptr, int n_bins,
                                                             const int* __restrict__ bin_start, const double* __restrict__ sorted_frac,
                                                             const int* __restrict__ sorted_type, const int* __restrict__ tiles, double dR,
                                                             int nbins, int reach, unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned cell_pair_grid_hist[];
  __shared__ double s_w[3][kCellStatChunk];
  __shared__ int s_tc[kCellStatChunk];    // type (255: none) | shift code << 8
  __shared__ int s_pos[kCellStatChunk];   // sorted position in the batch
  __shared__ int s_pref[kCellGridMaxOffsets + 1], s_p0[kCellGridMaxOffsets], s_code[kCellGridMaxOffsets];
  __shared__ int s_cbin[kCellStatCentreBlock];
  __shared__ int s_part[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = tiles[2 * (size_t)blockIdx.x], c0 = tiles[2 * (size_t)blockIdx.x + 1];
  GridCell G;
  if (reach < 1 || reach > kCellGridMaxReach || !grid_cell_read(c, cell_ptr, C, N, nbv, bin_ptr, n_bins, bin_start, &G)) return;
  for (int k = 0; k < 3; ++k)
    if (G.nb[k] < 2 * reach + 1) return;
  int nc;
  if (!cell_block_read<kCellStatCentreBlock>(c0, G.n, &nc)) return;
  double L[9];
  cell_lattice_read(lattice, c, L);
  const double limit = cell_stat_r2_limit(dR, nbins);
  const int nh = A * A * nbins;
  const int span = 2 * reach + 1, T = span * span * span;
  for (int k = tid; k < nh; k += 256) cell_pair_grid_hist[k] = 0u;
  if (tid < kCellStatCentreBlock) s_cbin[tid] = tid < nc ? cell_grid_bin(sorted_frac + 3 * ((size_t)G.lo + c0 + tid), G.nb) : -1;
  __syncthreads();
  for (int sa = 0; sa < nc;) {   // uniform in the workgroup: the run [sa, sb) of centres of one bin
    const int run_bin = s_cbin[sa];
    int sb = sa + 1;
    while (sb < nc && s_cbin[sb] == run_bin) ++sb;
    int b[3];
    cell_grid_unflat(run_bin, G.nb, b);
    // the candidate bins of the run, two consecutive offsets per thread, and the exclusive scan of their sizes
    int p0[2] = {0, 0}, cnt[2] = {0, 0}, code[2] = {kCellCentreCode, kCellCentreCode};
    for (int u = 0; u < 2; ++u) {
      const int t = 2 * tid + u;
      if (t < T) {
        int s[3];
        const int cb = cell_grid_candidate(b, G.nb, reach, t, s);
        code[u] = cell_shift_code(s[0], s[1], s[2]);
        grid_bin_range(G, bin_start, cb, &p0[u], &cnt[u]);
      }
    }
    int incl = cnt[0] + cnt[1];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_part[wave] = incl;
    __syncthreads();   // also: the readers of the previous run's tables and chunk are done
    int before = 0;
    for (int v = 0; v < wave; ++v) before += s_part[v];
    const int total = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    int at = before + incl - cnt[0] - cnt[1];
    for (int u = 0; u < 2; ++u) {
      const int t = 2 * tid + u;
      if (t < T) {
        s_pref[t] = at;
        s_p0[t] = p0[u];
        s_code[t] = code[u];
      }
      at += cnt[u];
    }
    if (tid == 0) s_pref[T] = total;
    // the threads of the run: (centre, slice)
    const int ns = sb - sa, slices = 256 / ns;
    const int ci = sa + tid % ns, slice = tid / ns;
    const size_t pos_i = (size_t)G.lo + c0 + ci;
    const int ti = sorted_type[pos_i];
    const bool active = slice < slices && ti >= 0 && ti < A;
    const double wi[3] = {sorted_frac[3 * pos_i], sorted_frac[3 * pos_i + 1], sorted_frac[3 * pos_i + 2]};
    unsigned* row = cell_pair_grid_hist + (size_t)(active ? ti : 0) * A * nbins;
    for (int q0 = 0; q0 < total; q0 += kCellStatChunk) {
      const int nq = min(kCellStatChunk, total - q0);
      __syncthreads();   // the tables are written; the readers of the previous chunk are done
      for (int e = tid; e < nq; e += 256) {
        const int q = q0 + e;
        int lo_t = 0, hi_t = T;   // s_pref[lo_t] <= q < s_pref[hi_t]
        while (hi_t - lo_t > 1) {
          const int mid = (lo_t + hi_t) / 2;
          if (s_pref[mid] <= q) lo_t = mid; else hi_t = mid;
        }
        const size_t p = (size_t)G.lo + s_p0[lo_t] + (q - s_pref[lo_t]);   // inside the bin's range: q < s_pref[lo_t + 1]
        const int ty = sorted_type[p];
        s_w[0][e] = sorted_frac[3 * p];
        s_w[1][e] = sorted_frac[3 * p + 1];
        s_w[2][e] = sorted_frac[3 * p + 2];
        s_tc[e] = (ty >= 0 && ty < A ? ty : 255) | (s_code[lo_t] << 8);
        s_pos[e] = (int)p;
      }
      __syncthreads();
      if (active) {
        for (int j = slice; j < nq; j += slices) {
          const int tc = s_tc[j], tj = tc & 255, cj = tc >> 8;
          if (tj == 255) continue;
          if (s_pos[j] == (int)pos_i && cj == kCellCentreCode) continue;
          const double wj[3] = {s_w[0][j], s_w[1][j], s_w[2][j]};
          int s[3];
          double r[3];
          cell_shift_decode(cj, s);
          cell_site_vector(wj, wi, s, L, r);
          const double r2 = cell_norm2(r);
          if (!(r2 < limit)) continue;
          const int k = cell_stat_bin(sqrt(r2), dR, nbins);
          if (k >= 0) atomicAdd(&row[tj * nbins + k], 1u);
        }
      }
    }
    sa = sb;
    __syncthreads();   // every thread has read this run's totals before the next run writes its own
  }
  unsigned long long* out = counts + (size_t)c * nh;
  for (int k = tid; k < nh; k += 256) {
    const unsigned v = cell_pair_grid_hist[k];
    if (v) atomicAdd(&out[k], (unsigned long long)v);
  }
}

// what the entries share: the batch, the grids (HOST copy) and that n_bins is their total
static int grid_entry_check(const char* who, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* nb, double radius,
                            int reach, double cutoff, int n_bins) {
  if (int rc = cell_grid_params_check(who, radius, reach, 0.0)) return rc;
  if (int rc = cell_batch_check(who, C, N, cell_ptr, lattice, cutoff)) return rc;
  int64_t total = 0;
  if (int rc = cell_grid_dims_check(who, C, lattice, nb, radius, reach, &total)) return rc;
  if (total != (int64_t)n_bins) { set_error("%s: n_bins %d, but the grids of the batch hold %lld bins", who, n_bins, (long long)total); return EGNN_EINVAL; }
  return EGNN_OK;
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_cell_grid_count(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* nb, double radius,
                         int reach, const int32_t* d_cell_ptr, const int32_t* d_nb, const int32_t* d_bin_ptr, const double* d_frac,
                         int n_bins, int32_t* d_atom_bin, int32_t* d_bin_count) {
  const char* who = "egnn_cell_grid_count";
  if (!lattice || !nb || !d_cell_ptr || !d_nb || !d_bin_ptr || (N > 0 && (!d_frac || !d_atom_bin)) || n_bins < 0 || (n_bins > 0 && !d_bin_count)) {
    set_error("bad %s arguments (lattice, nb, d_cell_ptr, d_nb, d_bin_ptr, d_frac and d_atom_bin given; n_bins >= 0 entries of d_bin_count)", who);
    return EGNN_EINVAL;
  }
  if (int rc = grid_entry_check(who, C, N, cell_ptr, lattice, nb, radius, reach, 1e-300, n_bins)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (n_bins > 0) EGNN_HIP(hipMemsetAsync(d_bin_count, 0, sizeof(int32_t) * (size_t)n_bins, st));
  if (N > 0)
    hipLaunchKernelGGL(cell_grid_bin_kernel, dim3((N + 255) / 256), dim3(256), 0, st, d_frac, d_cell_ptr, C, N, d_nb, d_bin_ptr, n_bins,
                       d_atom_bin, d_bin_count);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_grid_fill(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* nb, double radius,
                        int reach, const int32_t* d_cell_ptr, const int32_t* d_nb, const int32_t* d_bin_ptr, const double* d_frac,
                        const int32_t* d_type, int n_bins, const int32_t* d_bin_start, const int32_t* d_atom_bin, int32_t* d_work,
                        int32_t* d_sorted_atom, double* d_sorted_frac, int32_t* d_sorted_type) {
  const char* who = "egnn_cell_grid_fill";
  if (!lattice || !nb || !d_cell_ptr || !d_nb || !d_bin_ptr || !d_bin_start || n_bins < 0 ||
      (N > 0 && (!d_frac || !d_type || !d_atom_bin || !d_sorted_atom || !d_sorted_frac || !d_sorted_type)) || (N + n_bins > 0 && !d_work)) {
    set_error("bad %s arguments (lattice, nb, d_cell_ptr, d_nb, d_bin_ptr, d_bin_start, d_frac, d_type, d_atom_bin, d_work and the three "
              "outputs given; n_bins >= 0)", who);
    return EGNN_EINVAL;
  }
  if (int rc = grid_entry_check(who, C, N, cell_ptr, lattice, nb, radius, reach, 1e-300, n_bins)) return rc;
  if (N == 0) return EGNN_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int32_t* cursor = d_work;
  int32_t* arrival = d_work + n_bins;
  if (n_bins > 0) EGNN_HIP(hipMemsetAsync(cursor, 0, sizeof(int32_t) * (size_t)n_bins, st));
  EGNN_HIP(hipMemsetAsync(arrival, 0xFF, sizeof(int32_t) * (size_t)N, st));
  EGNN_HIP(hipMemsetAsync(d_sorted_atom, 0xFF, sizeof(int32_t) * (size_t)N, st));   // -1: an atom of a cell that is not gridded
  EGNN_HIP(hipMemsetAsync(d_sorted_type, 0xFF, sizeof(int32_t) * (size_t)N, st));
  EGNN_HIP(hipMemsetAsync(d_sorted_frac, 0, sizeof(double) * 3 * (size_t)N, st));
  hipLaunchKernelGGL(cell_grid_scatter_kernel, dim3((N + 255) / 256), dim3(256), 0, st, d_cell_ptr, C, N, d_nb, d_bin_ptr, n_bins, d_bin_start,
                     d_atom_bin, cursor, arrival);
  hipLaunchKernelGGL(cell_grid_rank_kernel, dim3((N + 255) / 256), dim3(256), 0, st, d_frac, d_type, d_cell_ptr, C, N, d_nb, d_bin_ptr, n_bins,
                     d_bin_start, d_atom_bin, arrival, d_sorted_atom, d_sorted_frac, d_sorted_type);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_bonds_grid_count(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* nb,
                               const int32_t* tiles, const int32_t* d_cell_ptr, const double* d_lattice, const int32_t* d_nb,
                               const int32_t* d_bin_ptr, int n_bins, const int32_t* d_bin_start, const int32_t* d_sorted_atom,
                               const double* d_sorted_frac, double cutoff, int reach, const int32_t* d_tiles, int n_tiles,
                               int32_t* d_degree) {
  const char* who = "egnn_cell_bonds_grid_count";
  if (!lattice || !nb || !d_cell_ptr || !d_lattice || !d_nb || !d_bin_ptr || !d_bin_start || n_bins < 0 ||
      (N > 0 && (!d_sorted_atom || !d_sorted_frac || !d_degree))) {
    set_error("bad %s arguments (lattice, nb, d_cell_ptr, d_lattice, d_nb, d_bin_ptr, d_bin_start, d_sorted_atom, d_sorted_frac and "
              "d_degree given; n_bins >= 0)", who);
    return EGNN_EINVAL;
  }
  if (int rc = tiles_check(who, d_tiles, n_tiles)) return rc;
  if (int rc = grid_entry_check(who, C, N, cell_ptr, lattice, nb, cutoff, reach, cutoff, n_bins)) return rc;
  if (int rc = cell_grid_tiles_check(who, C, nb, tiles, n_tiles)) return rc;
  if (n_tiles > 0)
    hipLaunchKernelGGL(cell_bond_grid_kernel<false>, dim3(n_tiles), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_lattice, d_cell_ptr,
                       C, N, d_nb, d_bin_ptr, n_bins, d_bin_start, d_sorted_atom, d_sorted_frac, d_tiles, cutoff, reach, (const int*)nullptr, 0,
                       d_degree, (int*)nullptr, (int*)nullptr);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_bonds_grid_fill(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* nb,
                              const int32_t* tiles, const int32_t* d_cell_ptr, const double* d_lattice, const int32_t* d_nb,
                              const int32_t* d_bin_ptr, int n_bins, const int32_t* d_bin_start, const int32_t* d_sorted_atom,
                              const double* d_sorted_frac, double cutoff, int reach, const int32_t* d_tiles, int n_tiles,
                              const int32_t* d_row_ptr, int n_bonds, int32_t* d_bond_atom, int32_t* d_bond_shift) {
  const char* who = "egnn_cell_bonds_grid_fill";
  if (!lattice || !nb || !d_cell_ptr || !d_lattice || !d_nb || !d_bin_ptr || !d_bin_start || n_bins < 0 || !d_row_ptr ||
      (N > 0 && (!d_sorted_atom || !d_sorted_frac)) || n_bonds < 0 || (n_bonds > 0 && (!d_bond_atom || !d_bond_shift))) {
    set_error("bad %s arguments (lattice, nb, d_cell_ptr, d_lattice, d_nb, d_bin_ptr, d_bin_start, d_sorted_atom, d_sorted_frac and "
              "d_row_ptr given; n_bins >= 0; n_bonds >= 0 entries of d_bond_atom and d_bond_shift)", who);
    return EGNN_EINVAL;
  }
  if (int rc = tiles_check(who, d_tiles, n_tiles)) return rc;
  if (int rc = grid_entry_check(who, C, N, cell_ptr, lattice, nb, cutoff, reach, cutoff, n_bins)) return rc;
  if (int rc = cell_grid_tiles_check(who, C, nb, tiles, n_tiles)) return rc;
  if (n_tiles > 0 && n_bonds > 0)
    hipLaunchKernelGGL(cell_bond_grid_kernel<true>, dim3(n_tiles), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_lattice, d_cell_ptr,
                       C, N, d_nb, d_bin_ptr, n_bins, d_bin_start, d_sorted_atom, d_sorted_frac, d_tiles, cutoff, reach, d_row_ptr, n_bonds,
                       (int*)nullptr, d_bond_atom, d_bond_shift);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_pair_counts_grid(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* nb,
                               const int32_t* tiles, const int32_t* d_cell_ptr, const double* d_lattice, const int32_t* d_nb,
                               const int32_t* d_bin_ptr, int n_bins, const int32_t* d_bin_start, const double* d_sorted_frac,
                               const int32_t* d_sorted_type, double dR, int nbins, int reach, const int32_t* d_tiles, int n_tiles,
                               int64_t* d_counts) {
  const char* who = "egnn_cell_pair_counts_grid";
  if (!lattice || !nb || !d_cell_ptr || !d_lattice || !d_nb || !d_bin_ptr || !d_bin_start || n_bins < 0 ||
      (N > 0 && (!d_sorted_frac || !d_sorted_type)) || !d_counts) {
    set_error("bad %s arguments (lattice, nb, d_cell_ptr, d_lattice, d_nb, d_bin_ptr, d_bin_start, d_sorted_frac, d_sorted_type and "
              "d_counts given; n_bins >= 0)", who);
    return EGNN_EINVAL;
  }
  if (int rc = atom_types_check(who, A, kCellMaxTypes)) return rc;
  if (int rc = tiles_check(who, d_tiles, n_tiles)) return rc;
  if (!(dR > 0.0) || !(dR < 1e30)) { set_error("%s: dR must be positive and finite", who); return EGNN_EINVAL; }
  if (nbins < 1) { set_error("%s: nbins %d (nbins >= 1)", who, nbins); return EGNN_EINVAL; }
  if ((long long)A * A * nbins > kCellStatMaxHist) {
    set_error("%s: %d x %d x %d histogram bins (at most %d: 64 KiB of LDS)", who, A, A, nbins, kCellStatMaxHist);
    return EGNN_EINVAL;
  }
  if (int rc = grid_entry_check(who, C, N, cell_ptr, lattice, nb, (double)nbins * dR, reach, 1e-300, n_bins)) return rc;
  if (int rc = cell_grid_tiles_check(who, C, nb, tiles, n_tiles)) return rc;
  // 64 KiB of histogram at A = 4, nbins = 1024, beside 36 KiB of staged candidates and tables; a CU has 160 KiB
  static LdsLimitRecord raised;
  if (int rc = raise_lds_limit(raised, &cell_pair_grid_kernel, sizeof(unsigned) * kCellStatMaxHist)) return rc;
  if (n_tiles > 0)
    hipLaunchKernelGGL(cell_pair_grid_kernel, dim3(n_tiles), dim3(256), sizeof(unsigned) * (size_t)A * A * nbins,
                       reinterpret_cast<hipStream_t>(stream), d_lattice, d_cell_ptr, C, N, A, d_nb, d_bin_ptr, n_bins, d_bin_start, d_sorted_frac,
                       d_sorted_type, d_tiles, dR, nbins, reach, reinterpret_cast<unsigned long long*>(d_counts));
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

}  // extern "C"

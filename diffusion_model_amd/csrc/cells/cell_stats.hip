// Real-space statistics of periodic cells on the device: partial pair counts over every centre and every image (-> g_ab(r) and the
// running coordination numbers), coordination numbers, bond angles and the Q^n speciation from the periodic bond list.
// Definitions: cell_stats_math.h (shared with the host statement, cell_stats_host.cpp).  Extends evaluate_RDF.py:39-60,
// evaluate_Si-O-Si.py:23-41 and CN2_evaluate.py:12-16, which look at atom 0 of one cluster, to the infinite lattice of a cell.
//
// Every accumulator is an integer: LDS integer atomics inside a workgroup, one global 64-bit integer atomicAdd per non-zero bin at
// the end of a tile.  No floating-point atomic anywhere.  Integer sums do not depend on arrival order, so the results are bitwise
// identical from run to run and a cell gives the same bits alone and in any batch.
//
// A kernel trusts no index: tile, cell, centre block, neighbour chunk, shift piece, bond row, neighbour and shift code are checked
// against the extents of the arrays before they are used, and every write is checked against the extent of its output.
#include "cell_device.h"
#include "cell_stats_host.h"
#include "cell_stats_math.h"

namespace egnn {

// ---- ordered pairs -> c[cell][a][b][k] -----------------------------------------------------------------------------------------
// One workgroup of 256 threads per tile {cell, first centre, first neighbour, piece, pieces}: <= 64 centres against <= 1024
// neighbour atoms and one piece of the first shift component's values -S_0 .. S_0 (cell_stat_piece; the caller chooses `pieces`, so
// that one large cell still fills the device: 3,000 atoms give 47 centre blocks x 3 chunks x 3 pieces = 423 workgroups).  The
// chunk's wrapped fractional coordinates (fp64, one array per axis) and types are staged in LDS; a thread keeps one centre in
// registers and walks every fourth atom of the chunk (each wavefront its own quarter), all lanes of a wavefront reading the same
// neighbour (an LDS broadcast), over the image box.  An axis whose |d_k| reaches cell_stat_axis_reach cannot count and is skipped,
// as is a pair whose r2 reaches cell_stat_r2_limit, before its square root and division: for a cell wider than the radius most
// images are.  What counts is decided by cell_stat_bin alone.
//
// Dynamic LDS: the histogram, A A nbins UNSIGNED 32-bit bins.  A tile holds at most 64 x 1024 x 33^3 = 2,355,167,232 (pair, image)
// terms (33 = 2 x 16 + 1 values per shift component), fewer than 2^32 = 4,294,967,296: a bin cannot wrap inside a tile, whatever
// the geometry.  The flush widens to 64 bits.
__global__ __launch_bounds__(256) void cell_pair_kernel(const double* __restrict__ frac, const double* __restrict__ lattice,
                                                        const int* __restrict__ type, const int* __restrict__ cell_ptr, int C, int N,
                                                        int A, const int* __restrict__ tiles, double dR, int nbins,
                                                        unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned cell_pair_hist[];
  __shared__ double s_w[3][kCellStatChunk];
  __shared__ int s_type[kCellStatChunk];
  const int tid = threadIdx.x;
  const int* tile = tiles + 5 * (size_t)blockIdx.x;
  const int j0 = tile[2], piece = tile[3], pieces = tile[4];
  CellTile T;
  if (!cell_tile_read<kCellStatCentreBlock>(tile, cell_ptr, C, N, &T) || j0 < 0 || j0 >= T.n) return;
  if (pieces < 1 || pieces > 2 * kCellStatMaxImages + 1 || piece < 0 || piece >= pieces) return;
  const int c = T.c, c0 = T.c0, lo = T.lo, nc = T.nc, nj = min(kCellStatChunk, T.n - j0);
  double L[9], width[3], reach[3];
  int S[3];
  cell_lattice_read(lattice, c, L);
  if (!cell_stat_image_box(L, dR, nbins, S) || !cell_widths(L, width)) return;   // refused by the host check of every entry
  if (S[0] > kCellStatMaxImages || S[1] > kCellStatMaxImages || S[2] > kCellStatMaxImages) return;
  for (int k = 0; k < 3; ++k) reach[k] = cell_stat_axis_reach(dR, nbins, width[k]);
  int p_lo, p_hi;
  cell_stat_piece(S[0], piece, pieces, &p_lo, &p_hi);
  const int sx_lo = p_lo - S[0], sx_hi = p_hi - S[0];   // [sx_lo, sx_hi)
  const double limit = cell_stat_r2_limit(dR, nbins);
  const int nh = A * A * nbins;
  for (int k = tid; k < nh; k += 256) cell_pair_hist[k] = 0u;
  cell_chunk_stage<kCellStatChunk>(frac, type, lo + j0, nj, tid, s_w, s_type);
  __syncthreads();
  constexpr int slices = 256 / kCellStatCentreBlock;
  const int ci = tid % kCellStatCentreBlock, slice = tid / kCellStatCentreBlock;
  if (ci < nc && sx_lo < sx_hi) {
    const int i = lo + c0 + ci, ti = type[i];
    if (ti >= 0 && ti < A) {
      double wi[3];
      cell_wrapped_read(frac, i, wi);
      unsigned* row = cell_pair_hist + (size_t)ti * A * nbins;
      for (int j = slice; j < nj; j += slices) {
        const int tj = s_type[j];
        if (tj < 0 || tj >= A) continue;
        const bool self = j0 + j == c0 + ci;
        const double wj0 = s_w[0][j], wj1 = s_w[1][j], wj2 = s_w[2][j];
        unsigned* bins = row + tj * nbins;
        for (int sx = sx_lo; sx < sx_hi; ++sx) {
          const double d0 = cell_delta(wj0, wi[0], sx);
          if (!(fabs(d0) < reach[0])) continue;
          for (int sy = -S[1]; sy <= S[1]; ++sy) {
            const double d1 = cell_delta(wj1, wi[1], sy);
            if (!(fabs(d1) < reach[1])) continue;
            for (int sz = -S[2]; sz <= S[2]; ++sz) {
              const double d2 = cell_delta(wj2, wi[2], sz);
              if (!(fabs(d2) < reach[2])) continue;
              if (self && sx == 0 && sy == 0 && sz == 0) continue;
              double r[3];
              cell_cartesian(d0, d1, d2, L, r);
              const double r2 = cell_norm2(r);
              if (!(r2 < limit)) continue;
              const int k = cell_stat_bin(sqrt(r2), dR, nbins);
              if (k >= 0) atomicAdd(&bins[k], 1u);
            }
          }
        }
      }
    }
  }
  __syncthreads();
  unsigned long long* out = counts + (size_t)c * nh;
  for (int k = tid; k < nh; k += 256) {
    const unsigned v = cell_pair_hist[k];
    if (v) atomicAdd(&out[k], (unsigned long long)v);
  }
}

// ---- bonds -> coordination[i][b], cn[cell][a][b][m], ang[cell][a][p][k], overflow[cell] ----------------------------------------
// One workgroup of four wavefronts per tile {cell, first centre} of <= 8 centres; ONE WAVEFRONT PER CENTRE.  The lanes walk the
// centre's row of the bond list, 64 entries at a time; the per-type counts come from ballots, so coordination and CN are exact
// for any degree.  The bond vectors of the first 64 entries (cell_site_vector, fp64) and their types are staged in the wavefront's
// LDS in row order, and the m (m - 1) / 2 pairs p < q are spread over the 64 lanes in a loop.  A centre with more than 64 bonds
// increments overflow[cell] and gives no angle.  Dynamic LDS: ang [A][P][nth], cn [A][A][max_cn + 1], overflow [1], all int32 (a
// tile holds 8 centres: at most 8 x 2016 angles).
struct CellBondWave {
  double v[3 * kMaxNeighbours];
  int t[kMaxNeighbours];
};

__global__ __launch_bounds__(256) void cell_bond_stats_kernel(const double* __restrict__ frac, const double* __restrict__ lattice,
                                                              const int* __restrict__ type, const int* __restrict__ cell_ptr, int C,
                                                              int N, int A, const int* __restrict__ row_ptr, int n_bonds,
                                                              const int* __restrict__ bond_atom, const int* __restrict__ bond_shift,
                                                              const int* __restrict__ tiles, double dtheta, int nth, int max_cn,
                                                              int* __restrict__ coordination, unsigned long long* __restrict__ cn,
                                                              unsigned long long* __restrict__ angles, int* __restrict__ overflow) {
  extern __shared__ int cell_bond_hist[];
  __shared__ CellBondWave s_wave[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  CellTile T;
  if (!cell_tile_read<kCellStatBondCentres>(tiles + 2 * (size_t)blockIdx.x, cell_ptr, C, N, &T)) return;
  const int c = T.c, c0 = T.c0, lo = T.lo, hi = T.lo + T.n, nc = T.nc;
  const int P = type_pairs(A), ncn = max_cn + 1;
  const int n_ang = A * P * nth, n_cn = A * A * ncn, nh = n_ang + n_cn + 1;
  int* h_ang = cell_bond_hist;
  int* h_cn = cell_bond_hist + n_ang;
  int* h_over = cell_bond_hist + n_ang + n_cn;
  for (int k = tid; k < nh; k += 256) cell_bond_hist[k] = 0;
  __syncthreads();
  double L[9];
  cell_lattice_read(lattice, c, L);
  CellBondWave& W = s_wave[wave];
  for (int ci = c0 + wave; ci < c0 + nc; ci += kWaves) {   // uniform in a wavefront
    const int i = lo + ci, ti = type[i];
    if (ti < 0 || ti >= A) continue;
    int e0, e1;
    if (!cell_row_read(row_ptr, N, n_bonds, i, &e0, &e1)) continue;   // row_ptr is not what the fill pass wrote
    const int deg = e1 - e0;
    double wi[3];
    cell_wrapped_read(frac, i, wi);
    int nb0 = 0, nb1 = 0, nb2 = 0, nb3 = 0;
    for (int eb = 0; eb < deg; eb += 64) {
      const int e = eb + lane;
      int ja = -1, tj = -1, sc = 0;
      if (e < deg) {
        ja = bond_atom[e0 + e];
        sc = bond_shift[e0 + e];
        if (cell_site_listed(lo, hi, ja, sc)) {
          tj = type[ja];
          if (tj < 0 || tj >= A) tj = -1;
        }
      }
      nb0 += __popcll(__ballot(tj == 0));
      nb1 += __popcll(__ballot(tj == 1));
      nb2 += __popcll(__ballot(tj == 2));
      nb3 += __popcll(__ballot(tj == 3));
      if (eb == 0) {   // the first 64 entries of the row, in row order
        if (tj >= 0) {   // cell_site_listed has passed the entry
          double r[3];
          cell_listed_vector(frac, L, wi, ja, sc, r);
          W.v[3 * lane] = r[0];
          W.v[3 * lane + 1] = r[1];
          W.v[3 * lane + 2] = r[2];
        }
        W.t[lane] = tj;
      }
    }
    if (lane < A) {
      const int mine = lane == 0 ? nb0 : (lane == 1 ? nb1 : (lane == 2 ? nb2 : nb3));
      coordination[(size_t)i * A + lane] = mine;
      atomicAdd(&h_cn[(ti * A + lane) * ncn + min(mine, max_cn)], 1);
    }
    wave_sync();   // the list is written
    if (deg > kMaxNeighbours) {
      if (lane == 0) atomicAdd(h_over, 1);
    } else {
      for (int p = lane; p < deg * deg; p += 64) {
        const int a = p / deg, b = p - a * deg;
        if (a >= b) continue;
        const int ta = W.t[a], tb = W.t[b];
        if (ta < 0 || tb < 0) continue;
        const int k = struct_angle_bin(&W.v[3 * a], &W.v[3 * b], dtheta, nth);
        if (k >= 0) atomicAdd(&h_ang[(ti * P + type_pair_index(ta, tb, A)) * nth + k], 1);
      }
    }
    wave_sync();   // the list is rewritten for the next centre
  }
  __syncthreads();
  unsigned long long* o_ang = angles + (size_t)c * n_ang;
  unsigned long long* o_cn = cn + (size_t)c * n_cn;
  for (int k = tid; k < n_ang; k += 256) {
    const int v = h_ang[k];
    if (v) atomicAdd(&o_ang[k], (unsigned long long)v);
  }
  for (int k = tid; k < n_cn; k += 256) {
    const int v = h_cn[k];
    if (v) atomicAdd(&o_cn[k], (unsigned long long)v);
  }
  if (tid == 0 && *h_over) atomicAdd(&overflow[c], *h_over);
}

// ---- finished coordination -> qn[i], qn_hist[cell][m] ---------------------------------------------------------------------------
// The same tiles, one wavefront per centre: a former atom counts its bonds to bridge atoms that have two or more former neighbours.
__global__ __launch_bounds__(256) void cell_qn_kernel(const int* __restrict__ type, const int* __restrict__ cell_ptr, int C, int N, int A,
                                                      const int* __restrict__ row_ptr, int n_bonds, const int* __restrict__ bond_atom,
                                                      const int* __restrict__ tiles, int max_cn, int former, int bridge,
                                                      const int* __restrict__ coordination, int* __restrict__ qn,
                                                      unsigned long long* __restrict__ qn_hist) {
  __shared__ int h_qn[kStructMaxCn + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  CellTile T;
  if (!cell_tile_read<kCellStatBondCentres>(tiles + 2 * (size_t)blockIdx.x, cell_ptr, C, N, &T) || max_cn < 0 || max_cn > kStructMaxCn) return;
  const int c = T.c, c0 = T.c0, lo = T.lo, hi = T.lo + T.n, nc = T.nc;
  if (tid <= kStructMaxCn) h_qn[tid] = 0;
  __syncthreads();
  for (int ci = c0 + wave; ci < c0 + nc; ci += kWaves) {   // uniform in a wavefront
    const int i = lo + ci;
    int e0, e1;
    if (type[i] != former || !cell_row_read(row_ptr, N, n_bonds, i, &e0, &e1)) {
      if (lane == 0) qn[i] = -1;
      continue;
    }
    const int deg = e1 - e0;
    int q = 0;
    for (int e = lane; e < deg; e += 64) {
      const int ja = bond_atom[e0 + e];
      if (ja >= lo && ja < hi && type[ja] == bridge && coordination[(size_t)ja * A + former] >= 2) ++q;
    }
    q = wave_sum(q);
    if (lane == 0) {
      qn[i] = q;
      atomicAdd(&h_qn[min(q, max_cn)], 1);
    }
  }
  __syncthreads();
  if (tid <= max_cn) {
    const int v = h_qn[tid];
    if (v) atomicAdd(&qn_hist[(size_t)c * (max_cn + 1) + tid], (unsigned long long)v);
  }
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_cell_pair_counts(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                          const double* d_lattice, const double* d_frac, const int32_t* d_type, double dR, int nbins,
                          const int32_t* d_tiles, int n_tiles, int64_t* d_counts) {
  const char* who = "egnn_cell_pair_counts";
  if (!lattice || !d_cell_ptr || !d_lattice || (N > 0 && (!d_frac || !d_type)) || !d_counts) {
    set_error("bad %s arguments (lattice, d_cell_ptr, d_lattice, d_frac, d_type and d_counts given)", who);
    return EGNN_EINVAL;
  }
  if (int rc = atom_types_check(who, A, kCellMaxTypes)) return rc;
  if (int rc = cell_batch_check(who, C, N, cell_ptr, lattice, 1e-300)) return rc;   // no cutoff here: a singular lattice is refused
  if (int rc = cell_stat_pair_check(who, C, A, lattice, dR, nbins)) return rc;
  if (int rc = tiles_check(who, d_tiles, n_tiles)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // 64 KiB of histogram at A = 4, nbins = 1024, beside 28 KiB of staged neighbours; a CU has 160 KiB
  static LdsLimitRecord raised;
  if (int rc = raise_lds_limit(raised, &cell_pair_kernel, sizeof(unsigned) * kCellStatMaxHist)) return rc;
  const size_t nh = (size_t)A * A * nbins;
  EGNN_HIP(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * (size_t)C * nh, st));
  if (n_tiles > 0)
    hipLaunchKernelGGL(cell_pair_kernel, dim3(n_tiles), dim3(256), sizeof(unsigned) * nh, st, d_frac, d_lattice, d_type, d_cell_ptr, C, N, A,
                       d_tiles, dR, nbins, reinterpret_cast<unsigned long long*>(d_counts));
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_bond_stats(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                         const double* d_lattice, const double* d_frac, const int32_t* d_type, const int32_t* d_row_ptr, int n_bonds,
                         const int32_t* d_bond_atom, const int32_t* d_bond_shift, double dtheta, int max_cn, int former, int bridge,
                         const int32_t* d_tiles, int n_tiles, int32_t* d_coordination, int64_t* d_cn, int64_t* d_angles, int32_t* d_qn,
                         int64_t* d_qn_hist, int32_t* d_overflow) {
  const char* who = "egnn_cell_bond_stats";
  if (!lattice || !d_cell_ptr || !d_lattice || !d_row_ptr || n_bonds < 0 || (n_bonds > 0 && (!d_bond_atom || !d_bond_shift)) ||
      (N > 0 && (!d_frac || !d_type || !d_coordination || !d_qn)) || !d_cn || !d_angles || !d_qn_hist || !d_overflow) {
    set_error("bad %s arguments (lattice, d_cell_ptr, d_lattice, d_frac, d_type, d_row_ptr and the six outputs given; n_bonds >= 0 "
              "entries of d_bond_atom and d_bond_shift)", who);
    return EGNN_EINVAL;
  }
  if (int rc = atom_types_check(who, A, kCellMaxTypes)) return rc;
  if (int rc = cell_stat_bond_check(who, A, dtheta, max_cn, former, bridge)) return rc;
  if (int rc = cell_batch_check(who, C, N, cell_ptr, lattice, 1e-300)) return rc;   // the bond list carries the cutoff
  if (int rc = tiles_check(who, d_tiles, n_tiles)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nth = struct_angle_bins(dtheta), P = type_pairs(A), ncn = max_cn + 1;
  const size_t n_ang = (size_t)A * P * nth, n_cn = (size_t)A * A * ncn;
  const size_t most = (size_t)kCellMaxTypes * type_pairs(kCellMaxTypes) * kStructMaxAngleBins +
                      (size_t)kCellMaxTypes * kCellMaxTypes * (kStructMaxCn + 1) + 1;
  static LdsLimitRecord raised;
  if (int rc = raise_lds_limit(raised, &cell_bond_stats_kernel, sizeof(int) * most)) return rc;
  EGNN_HIP(hipMemsetAsync(d_cn, 0, sizeof(int64_t) * C * n_cn, st));
  EGNN_HIP(hipMemsetAsync(d_angles, 0, sizeof(int64_t) * C * n_ang, st));
  EGNN_HIP(hipMemsetAsync(d_qn_hist, 0, sizeof(int64_t) * (size_t)C * ncn, st));
  EGNN_HIP(hipMemsetAsync(d_overflow, 0, sizeof(int32_t) * (size_t)C, st));
  if (N > 0) {
    EGNN_HIP(hipMemsetAsync(d_coordination, 0, sizeof(int32_t) * (size_t)N * A, st));
    EGNN_HIP(hipMemsetAsync(d_qn, 0xFF, sizeof(int32_t) * (size_t)N, st));   // -1: an atom no tile names is no former
  }
  if (n_tiles > 0) {
    hipLaunchKernelGGL(cell_bond_stats_kernel, dim3(n_tiles), dim3(256), sizeof(int) * (n_ang + n_cn + 1), st, d_frac, d_lattice, d_type,
                       d_cell_ptr, C, N, A, d_row_ptr, n_bonds, d_bond_atom, d_bond_shift, d_tiles, dtheta, nth, max_cn, d_coordination,
                       reinterpret_cast<unsigned long long*>(d_cn), reinterpret_cast<unsigned long long*>(d_angles), d_overflow);
    hipLaunchKernelGGL(cell_qn_kernel, dim3(n_tiles), dim3(256), 0, st, d_type, d_cell_ptr, C, N, A, d_row_ptr, n_bonds, d_bond_atom, d_tiles,
                       max_cn, former, bridge, d_coordination, d_qn, reinterpret_cast<unsigned long long*>(d_qn_hist));
  }
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

}  // extern "C"

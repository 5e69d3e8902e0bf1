// Local environments of periodic cells on the device: the periodic bond list of a batch of cells (count / fill, the caller takes
// the prefix sum in between, as egnn_radius_graph_count / _fill) and the shell cluster about every requested centre (count / fill).
// Definitions: cell_math.h (shared with the host statement, cell_host.cpp).  Restates make_dataset.py:79-142 on the infinite
// lattice: that script builds the 27 n sites of a 3x3x3 supercell, their full distance matrix, and walks it in Python for ONE centre.
//
// Nothing here depends on arrival order: a bond row is compacted by a wavefront scan in ascending (atom, image); the set of sites a
// breadth-first search finds does not depend on which lane wins an LDS compare-and-swap, and its order comes from a rank sort of
// the keys.  Positions are formed from the site key.  Results are bitwise identical from run to run.
//
// A kernel trusts no index: tile, cell, centre, bond row, neighbour and shift code are checked against the extents of the arrays
// before they are used, and every write is checked against the extent of its output.
#include "cell_device.h"
#include "cell_host.h"

namespace egnn {

// ---- periodic bond list ------------------------------------------------------------------------------------------------------
// One workgroup of 256 threads per tile {cell, first centre}: 64 centres, 16 per wavefront, against the whole cell in chunks of
// 1024 atoms whose wrapped fractional coordinates are staged in LDS (fp64, one array per axis: 64 consecutive lanes read 64
// consecutive doubles).  A wavefront takes one centre at a time (its coordinates are uniform) and 64 neighbour atoms per step, a
// lane looping the 27 images of its atom in registers.  An axis whose |d_k + s_k| reaches cutoff (1 + 1e-6) / w_k cannot bond (the
// inequality of cell_math.h, with a margin a million times the rounding of d_k) and is skipped: for a cell much wider than the
// cutoff most of the 27 are.  The images that bond are a 27-bit mask per lane; an inclusive scan of the popcounts over the
// wavefront gives every lane the place of its first entry in the row, so rows come out ascending by atom, then by shift code.
template <bool FILL>
__global__ __launch_bounds__(256) void cell_bond_kernel(const double* __restrict__ frac, const double* __restrict__ lattice,
                                                        const int* __restrict__ cell_ptr, int C, int N,
                                                        const int* __restrict__ tiles, double cutoff,
                                                        const int* __restrict__ row_ptr, int n_bonds, int* __restrict__ degree,
                                                        int* __restrict__ bond_atom, int* __restrict__ bond_shift) {
  __shared__ double s_w[3][kCellChunk];
  __shared__ int s_cnt[kCellCentreBlock];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  CellTile T;
  if (!cell_tile_read<kCellCentreBlock>(tiles + 2 * (size_t)blockIdx.x, cell_ptr, C, N, &T)) return;
  const int c0 = T.c0, lo = T.lo, n = T.n, nc = T.nc;
  double L[9], width[3], reach[3];
  cell_lattice_read(lattice, T.c, L);
  const bool regular = cell_widths(L, width);
  for (int k = 0; k < 3; ++k) reach[k] = regular ? cutoff * (1.0 + 1e-6) / width[k] : 4.0;   // 4.0: no image is skipped
  const double c2 = cutoff * cutoff;
  if (tid < kCellCentreBlock) s_cnt[tid] = 0;
  constexpr int per_wave = kCellCentreBlock / kWaves;
  const int ci_end = min(nc, (wave + 1) * per_wave);
  for (int j0 = 0; j0 < n; j0 += kCellChunk) {
    const int nj = min(kCellChunk, n - j0);
    __syncthreads();   // the readers of the previous chunk are done
    cell_chunk_stage<kCellChunk>(frac, nullptr, lo + j0, nj, tid, s_w, nullptr);
    __syncthreads();
    for (int ci = wave * per_wave; ci < ci_end; ++ci) {   // uniform in a wavefront
      const int i = lo + c0 + ci;
      double wi[3];
      cell_wrapped_read(frac, i, wi);
      int cnt = s_cnt[ci];
      int row_lo = 0, row_hi = 0;
      if (FILL) { row_lo = row_ptr[i]; row_hi = row_ptr[i + 1]; }   // not cell_row_read: every write below is tested against the row
      for (int jb = 0; jb < nj; jb += 64) {
        const int jj = jb + lane;
        unsigned mask = 0;
        if (jj < nj) {
          const bool self = j0 + jj == c0 + ci;
          const double wj0 = s_w[0][jj], wj1 = s_w[1][jj], wj2 = s_w[2][jj];
          for (int sx = -1; sx <= 1; ++sx) {
            const double d0 = cell_delta(wj0, wi[0], sx);
            if (!(fabs(d0) < reach[0])) continue;
            for (int sy = -1; sy <= 1; ++sy) {
              const double d1 = cell_delta(wj1, wi[1], sy);
              if (!(fabs(d1) < reach[1])) continue;
              for (int sz = -1; sz <= 1; ++sz) {
                const double d2 = cell_delta(wj2, wi[2], sz);
                if (!(fabs(d2) < reach[2])) continue;
                if (self && sx == 0 && sy == 0 && sz == 0) continue;
                double r[3];
                cell_cartesian(d0, d1, d2, L, r);
                if (cell_norm2(r) < c2) mask |= 1u << ((sx + 1) * 9 + (sy + 1) * 3 + (sz + 1));
              }
            }
          }
        }
        const int mine = __popc(mask);
        int incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const int up = __shfl_up(incl, d);
          if (lane >= d) incl += up;
        }
        const int total = __shfl(incl, 63);
        if (FILL) {
          int at = row_lo + cnt + (incl - mine);
          unsigned todo = mask;
          while (todo) {
            const int b = __ffs(todo) - 1;
            todo &= todo - 1;
            if (at >= 0 && at >= row_lo && at < row_hi && at < n_bonds) {
              bond_atom[at] = lo + j0 + jj;
              bond_shift[at] = cell_shift_code(b / 9 - 1, b / 3 % 3 - 1, b % 3 - 1);
            }
            ++at;
          }
        }
        cnt += total;
      }
      if (lane == 0) s_cnt[ci] = cnt;
    }
  }
  if (!FILL) {
    wave_sync();   // the wavefront reads what its lane 0 wrote
    for (int ci = wave * per_wave + lane; ci < ci_end; ci += 64) degree[lo + c0 + ci] = s_cnt[ci];
  }
}

// ---- environment expansion -----------------------------------------------------------------------------------------------------
// One wavefront per centre, four centres per workgroup, no workgroup barrier.  Dynamic LDS per wavefront: the site list in discovery
// order, int32 [max_atoms + 64], and an open-addressing table of the keys seen, int32 [2^log_table] with 2^log_table >=
// 2 (max_atoms + 64), empty = -1.  Breadth-first: the lanes take 64 sites of the frontier, step k visits the k-th bond of each
// lane's site; a new key enters the table by atomicCAS (one lane wins a key two lanes found), the winners append to the list by
// ballot + popcount.  The search stops once the list exceeds max_atoms, at most 64 entries later: the table never fills.
// The order of the output comes from a rank sort: the centre is row 0, a site's row is 1 + the number of smaller keys.
template <bool FILL>
__global__ __launch_bounds__(256) void cell_env_kernel(const double* __restrict__ frac, const double* __restrict__ lattice,
                                                       const int* __restrict__ type, const int* __restrict__ cell_ptr, int C, int N,
                                                       int A, const int* __restrict__ row_ptr, int n_bonds,
                                                       const int* __restrict__ bond_atom, const int* __restrict__ bond_shift, int M,
                                                       const int* __restrict__ centre_cell, const int* __restrict__ centre,
                                                       int shells, int max_atoms, int log_table, int* __restrict__ size_out,
                                                       const int* __restrict__ env_ptr, int n_sites, int* __restrict__ env_atom,
                                                       int* __restrict__ env_shift, int* __restrict__ env_type,
                                                       float* __restrict__ env_pos) {
  extern __shared__ int env_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = blockIdx.x * kCellEnvWaves + wave;
  if (m >= M) return;
  const int cap = max_atoms + kCellEnvSlack, H = 1 << log_table;
  int* list = env_lds + (size_t)wave * (cap + H);
  int* table = list + cap;
  const int c = centre_cell[m], ctr = centre[m];
  int lo = 0, n = 0;
  const bool valid = cell_read(c, cell_ptr, C, N, &lo, &n) && n <= kCellMaxAtoms && ctr >= lo && ctr < lo + n;
  const int hi = lo + n;
  if (!valid) {   // refused by the host check of every caller that has one; size 0 says so, nothing is listed
    if (!FILL && lane == 0) size_out[m] = 0;
    return;
  }
  for (int t = lane; t < H; t += 64) table[t] = -1;
  const int key0 = (ctr - lo) * kCellShiftCodes + kCellCentreCode;
  wave_sync();
  if (lane == 0) {
    list[0] = key0;
    table[((unsigned)key0 * 2654435761u) >> (32 - log_table)] = key0;
  }
  wave_sync();
  int count = 1, begin = 0;
  for (int hop = 0; hop < shells && count <= max_atoms; ++hop) {
    const int end = count;
    for (int fb = begin; fb < end && count <= max_atoms; fb += 64) {
      const int f = fb + lane;
      int code = 0, e0 = 0, e1 = 0, deg = 0;
      if (f < end) {
        const int key = list[f];
        code = key % kCellShiftCodes;
        if (cell_row_read(row_ptr, N, n_bonds, lo + key / kCellShiftCodes, &e0, &e1)) deg = e1 - e0;
      }
      for (int k = 0; count <= max_atoms && __ballot(k < deg) != 0ull; ++k) {
        int fresh = -1;
        if (k < deg) {
          const int ja = bond_atom[e0 + k], sc = bond_shift[e0 + k];
          if (cell_site_listed(lo, hi, ja, sc)) {
            const int nc = cell_shift_add(code, sc);
            if (nc >= 0) fresh = (ja - lo) * kCellShiftCodes + nc;
          }
        }
        bool won = false;
        if (fresh >= 0) {
          int slot = (int)(((unsigned)fresh * 2654435761u) >> (32 - log_table));
          for (int probe = 0; probe < H; ++probe) {
            const int prev = atomicCAS(&table[slot], -1, fresh);
            if (prev == -1) { won = true; break; }
            if (prev == fresh) break;
            slot = (slot + 1) & (H - 1);
          }
        }
        const unsigned long long winners = __ballot(won);
        if (won) list[count + lane_prefix(winners, lane)] = fresh;   // count <= max_atoms here: below max_atoms + 64
        count += __popcll(winners);
        wave_sync();
      }
    }
    begin = end;
  }
  if (!FILL) {
    if (lane == 0) size_out[m] = count <= max_atoms ? count : max_atoms + 1;
    return;
  }
  if (count > max_atoms) return;
  const int base = env_ptr[m];
  if (base < 0 || env_ptr[m + 1] - base != count || base > n_sites - count) return;   // not the sizes the count pass gave
  double L[9], wi[3];
  cell_lattice_read(lattice, c, L);
  cell_wrapped_read(frac, ctr, wi);
  for (int e = lane; e < count; e += 64) {
    const int key = list[e];
    int rank = 0;
    if (e > 0) {
      rank = 1;
      for (int t = 1; t < count; ++t) rank += list[t] < key;
    }
    const int atom = lo + key / kCellShiftCodes, code = key % kCellShiftCodes;
    double r[3];
    cell_listed_vector(frac, L, wi, atom, code, r);   // the search lists entries cell_site_listed has passed
    const size_t at = (size_t)base + rank;
    const int ty = type[atom];
    env_atom[at] = atom;
    env_shift[at] = code;
    env_type[at] = ty >= 0 && ty < A ? ty : -1;
    env_pos[3 * at] = (float)r[0];
    env_pos[3 * at + 1] = (float)r[1];
    env_pos[3 * at + 2] = (float)r[2];
  }
}

static int cell_log_table(int max_atoms) {
  int lg = 7;
  while ((1 << lg) < 2 * (max_atoms + kCellEnvSlack)) ++lg;
  return lg;
}

static size_t cell_env_lds_bytes(int max_atoms) {
  return sizeof(int) * (size_t)kCellEnvWaves * ((size_t)max_atoms + kCellEnvSlack + ((size_t)1 << cell_log_table(max_atoms)));
}

// A launch that needs more dynamic LDS than a function is given by default (64 KiB; 81 KiB at max_atoms = 1024, a CU has 160 KiB)
// raises the function's limit first, once per device (eval/lds_limit.h).  The default max_atoms = 256 needs 21 KiB and makes no
// call.
template <bool FILL>
static int cell_env_configure(size_t lds_bytes) {
  static LdsLimitRecord raised;   // one per instantiation: one per kernel
  if (lds_bytes > 64u * 1024u) return raise_lds_limit(raised, &cell_env_kernel<FILL>, cell_env_lds_bytes(kCellMaxEnvAtoms));
  return EGNN_OK;
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_cell_bonds_count(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                          const double* d_lattice, const double* d_frac, double cutoff, const int32_t* d_tiles, int n_tiles,
                          int32_t* d_degree) {
  const char* who = "egnn_cell_bonds_count";
  if (!lattice || !d_cell_ptr || !d_lattice || (N > 0 && (!d_frac || !d_degree))) {
    set_error("bad %s arguments (lattice, d_cell_ptr, d_lattice, d_frac and d_degree given)", who);
    return EGNN_EINVAL;
  }
  if (int rc = cell_batch_check(who, C, N, cell_ptr, lattice, cutoff)) return rc;
  if (int rc = tiles_check(who, d_tiles, n_tiles)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (N > 0) EGNN_HIP(hipMemsetAsync(d_degree, 0, sizeof(int32_t) * (size_t)N, st));
  if (n_tiles > 0)
    hipLaunchKernelGGL(cell_bond_kernel<false>, dim3(n_tiles), dim3(256), 0, st, d_frac, d_lattice, d_cell_ptr, C, N, d_tiles, cutoff,
                       (const int*)nullptr, 0, d_degree, (int*)nullptr, (int*)nullptr);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_bonds_fill(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                         const double* d_lattice, const double* d_frac, double cutoff, const int32_t* d_tiles, int n_tiles,
                         const int32_t* d_row_ptr, int n_bonds, int32_t* d_bond_atom, int32_t* d_bond_shift) {
  const char* who = "egnn_cell_bonds_fill";
  if (!lattice || !d_cell_ptr || !d_lattice || !d_row_ptr || (N > 0 && !d_frac) || n_bonds < 0 ||
      (n_bonds > 0 && (!d_bond_atom || !d_bond_shift))) {
    set_error("bad %s arguments (lattice, d_cell_ptr, d_lattice, d_frac, d_row_ptr given; n_bonds >= 0 entries of d_bond_atom and "
              "d_bond_shift)", who);
    return EGNN_EINVAL;
  }
  if (int rc = cell_batch_check(who, C, N, cell_ptr, lattice, cutoff)) return rc;
  if (int rc = tiles_check(who, d_tiles, n_tiles)) return rc;
  if (n_tiles > 0 && n_bonds > 0)
    hipLaunchKernelGGL(cell_bond_kernel<true>, dim3(n_tiles), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_frac, d_lattice,
                       d_cell_ptr, C, N, d_tiles, cutoff, d_row_ptr, n_bonds, (int*)nullptr, d_bond_atom, d_bond_shift);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_env_count(void* stream, int C, int N, const int32_t* cell_ptr, const int32_t* d_cell_ptr, const int32_t* d_row_ptr,
                        int n_bonds, const int32_t* d_bond_atom, const int32_t* d_bond_shift, int M, const int32_t* d_centre_cell,
                        const int32_t* d_centre, int shells, int max_atoms, int32_t* d_size) {
  const char* who = "egnn_cell_env_count";
  if (!d_cell_ptr || !d_row_ptr || n_bonds < 0 || (n_bonds > 0 && (!d_bond_atom || !d_bond_shift)) || (M > 0 && !d_size)) {
    set_error("bad %s arguments (d_cell_ptr, d_row_ptr and d_size given; n_bonds >= 0 entries of d_bond_atom and d_bond_shift)", who);
    return EGNN_EINVAL;
  }
  if (int rc = cell_env_params_check(who, M, shells, max_atoms, d_centre_cell, d_centre)) return rc;
  if (int rc = cell_batch_check(who, C, N, cell_ptr, nullptr, 1.0)) return rc;
  if (M == 0) return EGNN_OK;
  if (int rc = cell_env_configure<false>(cell_env_lds_bytes(max_atoms))) return rc;
  hipLaunchKernelGGL(cell_env_kernel<false>, dim3((M + kCellEnvWaves - 1) / kCellEnvWaves), dim3(256), cell_env_lds_bytes(max_atoms),
                     reinterpret_cast<hipStream_t>(stream), (const double*)nullptr, (const double*)nullptr, (const int*)nullptr,
                     d_cell_ptr, C, N, 0, d_row_ptr, n_bonds, d_bond_atom, d_bond_shift, M, d_centre_cell, d_centre, shells, max_atoms,
                     cell_log_table(max_atoms), d_size, (const int*)nullptr, 0, (int*)nullptr, (int*)nullptr, (int*)nullptr,
                     (float*)nullptr);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_env_fill(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                       const double* d_lattice, const double* d_frac, const int32_t* d_type, const int32_t* d_row_ptr, int n_bonds,
                       const int32_t* d_bond_atom, const int32_t* d_bond_shift, int M, const int32_t* d_centre_cell,
                       const int32_t* d_centre, int shells, int max_atoms, const int32_t* d_env_ptr, int n_sites, int32_t* d_env_atom,
                       int32_t* d_env_shift, int32_t* d_env_type, float* d_env_pos) {
  const char* who = "egnn_cell_env_fill";
  if (!lattice || !d_cell_ptr || !d_lattice || (N > 0 && (!d_frac || !d_type)) || !d_row_ptr || n_bonds < 0 ||
      (n_bonds > 0 && (!d_bond_atom || !d_bond_shift)) || n_sites < 0 || (M > 0 && !d_env_ptr) ||
      (n_sites > 0 && (!d_env_atom || !d_env_shift || !d_env_type || !d_env_pos))) {
    set_error("bad %s arguments (lattice, d_cell_ptr, d_lattice, d_frac, d_type, d_row_ptr and d_env_ptr given; n_bonds >= 0 bonds; "
              "n_sites >= 0 entries of the four outputs)", who);
    return EGNN_EINVAL;
  }
  if (int rc = atom_types_check(who, A, kCellMaxTypes)) return rc;
  if (int rc = cell_env_params_check(who, M, shells, max_atoms, d_centre_cell, d_centre)) return rc;
  if (int rc = cell_batch_check(who, C, N, cell_ptr, lattice, 1e-300)) return rc;   // no cutoff here: a singular lattice is refused
  if (M == 0 || n_sites == 0) return EGNN_OK;
  if (int rc = cell_env_configure<true>(cell_env_lds_bytes(max_atoms))) return rc;
  hipLaunchKernelGGL(cell_env_kernel<true>, dim3((M + kCellEnvWaves - 1) / kCellEnvWaves), dim3(256), cell_env_lds_bytes(max_atoms),
                     reinterpret_cast<hipStream_t>(stream), d_frac, d_lattice, d_type, d_cell_ptr, C, N, A, d_row_ptr, n_bonds,
                     d_bond_atom, d_bond_shift, M, d_centre_cell, d_centre, shells, max_atoms, cell_log_table(max_atoms), (int*)nullptr,
                     d_env_ptr, n_sites, d_env_atom, d_env_shift, d_env_type, d_env_pos);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

}  // extern "C"

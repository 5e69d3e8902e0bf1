// Bond-orientational order of periodic cells on the device: q_lm of the atoms of a CSR of site rows (pass 1) and, from those rows,
// q_l, w_l, w^_l, their Lechner-Dellago averages and the solid-bond count of every listed centre (pass 2: it gathers the q_lm rows
// of OTHER atoms, so it is a second kernel).  Definitions and summation orders: cell_boo_math.h (shared with the host statement,
// cell_boo_host.cpp).  An extension: no file of the reference computes it.
//
// All fp64, no matrix work: the kernels are bound by the VALU (the harmonic recurrences) and by the gathers of site atoms and q_lm
// rows.  One wavefront per row, four per workgroup; nothing is shared between wavefronts, so there is no workgroup barrier.
//
// No kernel has an atomic and no sum is reduced across lanes: every q_lm and every invariant is one thread's running sum in the
// order of cell_boo_math.h, so the device executes the host statement's operations.  Results are bitwise identical from run to run.
//
// A kernel trusts no index: centre, cell, row, site atom, shift code, type and G entry are checked against the extents of the
// arrays before they are used.
#include "cell_device.h"
#include "cell_boo_host.h"
#include "cell_boo_math.h"

namespace egnn {

static_assert(kBooChunk * kBooParts == 64, "a wavefront stages kBooChunk sites with kBooParts lanes each");
constexpr int kBooMaxLM = (kBooMaxL + 1) * (kBooMaxL + 1);
static_assert(kBooMaxLM <= 128, "a lane holds two running sums: lm = lane and lane + 64");

// ---- pass 1: q_lm ----------------------------------------------------------------------------------------------------------------
// The wavefront walks its row kBooChunk entries at a time.  Lane (part, slot) = (lane / 16, lane % 16) tests entry k0 + slot
// (boo_site: the four lanes of a slot agree); the kept entries take consecutive LDS slots by ballot and popcount, and the lanes of a
// slot write the harmonic columns m = part, part + 4, .. of its unit vector (soap_solid_column), so no lane ever holds a site's 121
// harmonics.  Then lane lm (and lm + 64) adds the staged slots in order to its running sum, which lives across the chunks: one
// ascending sum whatever the chunking.  LDS: kBooWaves * kBooChunk * boo_stride(l_max) doubles (25 KiB at l_max = 6, 61 KiB at 10),
// within the default dynamic limit; a row without a centre or a CSR row is a row of zeros with n = 0.
__global__ __launch_bounds__(64 * kBooWaves) void cell_boo_qlm_kernel(const double* __restrict__ frac, const double* __restrict__ lattice,
                                                                     const int* __restrict__ type, const int* __restrict__ cell_ptr, int C, int N,
                                                                     int A, unsigned select, int l_max, const double* __restrict__ norm,
                                                                     const int* __restrict__ row_ptr, int n_rows, int T,
                                                                     const int* __restrict__ site_atom, const int* __restrict__ site_shift, int M,
                                                                     const int* __restrict__ centre_atom, const int* __restrict__ centre_row,
                                                                     double* __restrict__ qlm, int* __restrict__ n_out) {
  extern __shared__ double s_boo[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = blockIdx.x * kBooWaves + wave;
  if (m >= M) return;   // uniform in a wavefront; no workgroup barrier follows
  const int LM = soap_lm_count(l_max), stride = boo_stride(l_max);
  double* stage = s_boo + (size_t)wave * kBooChunk * stride;
  CellCentreRow R;
  const bool valid = cell_centre_row_read(cell_ptr, C, N, row_ptr, n_rows, T, centre_atom, centre_row, m, &R);
  const int slot_of = lane & (kBooChunk - 1), part = lane / kBooChunk;
  double acc0 = 0.0, acc1 = 0.0;
  int kept = 0;
  if (valid) {
    double L[9];
    cell_lattice_read(lattice, R.c, L);
    for (int k0 = R.e0; k0 < R.e1; k0 += kBooChunk) {   // uniform in the wavefront
      const int e = k0 + slot_of;
      bool keep = false;
      double u[3] = {0.0, 0.0, 0.0};
      if (e < R.e1) keep = boo_site(frac, type, L, R.lo, R.hi, A, select, R.i, site_atom[e], site_shift[e], u);
      const unsigned long long hits = __ballot(keep) & ((1ull << kBooChunk) - 1ull);   // the lanes of part 0: one bit a slot
      const int cnt = __popcll(hits);
      if (keep) {
        double* col = stage + lane_prefix(hits, slot_of) * stride;
        const double uu = cell_norm2(u);
        for (int mm = part; mm <= l_max; mm += kBooParts) soap_solid_column(u[0], u[1], u[2], uu, mm, l_max, norm, col);
      }
      wave_sync();
      for (int s = 0; s < cnt; ++s) {
        if (lane < LM) acc0 += stage[s * stride + lane];
        if (lane + 64 < LM) acc1 += stage[s * stride + lane + 64];
      }
      wave_sync();
      kept += cnt;
    }
  }
  double* row = qlm + (size_t)m * LM;
  if (lane < LM) row[lane] = kept > 0 ? acc0 / (double)kept : 0.0;
  if (lane + 64 < LM) row[lane + 64] = kept > 0 ? acc1 / (double)kept : 0.0;
  if (lane == 0) n_out[m] = kept;
}

// ---- pass 2: invariants ----------------------------------------------------------------------------------------------------------
// The wavefront stages its centre's q_lm row in LDS, then walks the CSR row 64 entries at a time: a lane tests its entry and, where
// it is kept, computes s_ik from the two rows (boo_solid: one thread, ascending m); ballots count n and n_solid.  For the averages
// the kept entries of the step are visited in ascending order (uniform: the bits of the ballot), the atom broadcast by shuffle, and
// lane lm (and lm + 64) adds q_lm of that atom to a running sum that started at the centre's own value: coalesced reads of a row.
// Finally lane which * (l_max + 1) + l computes the three invariants of degree l of the own (which = 0) or the averaged row.
// out is [M, blocks, l_max + 1], blocks = 3 (q, w, w^) or 6 (then qbar, wbar, wbar^) with `averaged`.
__global__ __launch_bounds__(64 * kBooWaves) void cell_boo_invariants_kernel(
    const double* __restrict__ frac, const double* __restrict__ lattice, const int* __restrict__ type, const int* __restrict__ cell_ptr, int C,
    int N, int A, unsigned select, int l_max, const double* __restrict__ qlm, int E, const int* __restrict__ g_off,
    const int* __restrict__ g_idx, const double* __restrict__ g_val, int l_solid, double threshold, int averaged,
    const int* __restrict__ row_ptr, int n_rows, int T, const int* __restrict__ site_atom, const int* __restrict__ site_shift, int M,
    const int* __restrict__ centre_atom, const int* __restrict__ centre_row, double* __restrict__ out, int* __restrict__ n_out,
    int* __restrict__ n_solid_out) {
  __shared__ double s_rows[kBooWaves][2][kBooMaxLM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = blockIdx.x * kBooWaves + wave;
  if (m >= M) return;   // uniform in a wavefront; no workgroup barrier follows
  const int L1 = l_max + 1, LM = soap_lm_count(l_max), sets = averaged ? 2 : 1;
  double* o = out + (size_t)m * (3 * sets) * L1;
  CellCentreRow R;
  if (!cell_centre_row_read(cell_ptr, C, N, row_ptr, n_rows, T, centre_atom, centre_row, m, &R)) {
    for (int k = lane; k < 3 * sets * L1; k += 64) o[k] = 0.0;
    if (lane == 0) { n_out[m] = 0; n_solid_out[m] = 0; }
    return;
  }
  double L[9];
  cell_lattice_read(lattice, R.c, L);
  double* own = s_rows[wave][0];
  double* avg = s_rows[wave][1];
  double acc0 = lane < LM ? qlm[(size_t)R.i * LM + lane] : 0.0, acc1 = lane + 64 < LM ? qlm[(size_t)R.i * LM + lane + 64] : 0.0;
  if (lane < LM) own[lane] = acc0;
  if (lane + 64 < LM) own[lane + 64] = acc1;
  wave_sync();
  int kept = 0, solid = 0;
  for (int k0 = R.e0; k0 < R.e1; k0 += 64) {   // uniform in the wavefront
    const int e = k0 + lane;
    bool keep = false;
    int j = 0;
    if (e < R.e1) {
      double u[3];
      j = site_atom[e];
      keep = boo_site(frac, type, L, R.lo, R.hi, A, select, R.i, j, site_shift[e], u);
    }
    const bool is_solid = keep && boo_solid(own, qlm + (size_t)j * LM, l_solid) > threshold;
    unsigned long long hits = __ballot(keep);
    kept += __popcll(hits);
    solid += __popcll(__ballot(is_solid));
    if (averaged) {
      while (hits) {   // uniform: ascending entries
        const int b = __ffsll((long long)hits) - 1;
        hits &= hits - 1ull;
        const size_t at = (size_t)__shfl(j, b, 64) * LM;
        if (lane < LM) acc0 += qlm[at + lane];
        if (lane + 64 < LM) acc1 += qlm[at + lane + 64];
      }
    }
  }
  if (averaged) {
    if (lane < LM) avg[lane] = acc0 / (double)(1 + kept);
    if (lane + 64 < LM) avg[lane + 64] = acc1 / (double)(1 + kept);
    wave_sync();
  }
  for (int k = lane; k < sets * L1; k += 64) {
    const int which = k / L1, l = k - which * L1;
    boo_invariants(which ? avg : own, l, l_max, E, g_off, g_idx, g_val, o + 3 * which * L1);
  }
  if (lane == 0) { n_out[m] = kept; n_solid_out[m] = solid; }
}

static int cell_boo_rows_check(const char* who, const void* d_cell_ptr, const void* d_lattice, const void* d_frac, const void* d_type,
                               int n_rows, const void* d_row_ptr, int T, const void* d_site_atom, const void* d_site_shift, int M,
                               const void* d_centre_atom, const void* d_centre_row) {
  if (!cell_rows_given(d_cell_ptr, d_lattice, d_frac, d_type, n_rows, d_row_ptr, T, d_site_atom, d_site_shift, M, d_centre_atom, d_centre_row)) {
    set_error("bad %s arguments (d_cell_ptr, d_lattice, d_frac, d_type, d_row_ptr and the centres given; n_rows >= 0 rows of T >= 0 sites; "
              "M >= 1)", who);
    return EGNN_EINVAL;
  }
  return EGNN_OK;
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_cell_boo_qlm(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                      const double* d_lattice, const double* d_frac, const int32_t* d_type, double cutoff, unsigned select, int l_max,
                      const double* d_norm, int n_rows, const int32_t* d_row_ptr, int T, const int32_t* d_site_atom,
                      const int32_t* d_site_shift, int M, const int32_t* d_centre_atom, const int32_t* d_centre_row, double* d_qlm,
                      int32_t* d_n) {
  const char* who = "egnn_cell_boo_qlm";
  if (int rc = cell_boo_rows_check(who, d_cell_ptr, d_lattice, d_frac, d_type, n_rows, d_row_ptr, T, d_site_atom, d_site_shift, M, d_centre_atom,
                                   d_centre_row)) return rc;
  if (!d_norm || !d_qlm || !d_n) { set_error("bad %s arguments (d_norm, d_qlm and d_n given)", who); return EGNN_EINVAL; }
  if (int rc = cell_boo_config_check(who, A, l_max, -1, select)) return rc;
  if (cutoff == 0.0) { set_error("%s: cutoff must be positive and finite", who); return EGNN_EINVAL; }
  if (int rc = cell_soap_batch_check(who, C, N, cell_ptr, lattice, cutoff)) return rc;
  const size_t lds = sizeof(double) * kBooWaves * kBooChunk * (size_t)boo_stride(l_max);   // at most 61 KiB: within the default limit
  hipLaunchKernelGGL(cell_boo_qlm_kernel, dim3((M + kBooWaves - 1) / kBooWaves), dim3(64 * kBooWaves), lds, reinterpret_cast<hipStream_t>(stream),
                     d_frac, d_lattice, d_type, d_cell_ptr, C, N, A, select, l_max, d_norm, d_row_ptr, n_rows, T, d_site_atom, d_site_shift, M,
                     d_centre_atom, d_centre_row, d_qlm, d_n);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_boo_invariants(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                             const double* d_lattice, const double* d_frac, const int32_t* d_type, unsigned select, int l_max,
                             const double* d_qlm, int E, const int32_t* g_off, const int32_t* d_g_off, const int32_t* d_g_idx,
                             const double* d_g_val, int l_solid, double threshold, int averaged, int n_rows, const int32_t* d_row_ptr, int T,
                             const int32_t* d_site_atom, const int32_t* d_site_shift, int M, const int32_t* d_centre_atom,
                             const int32_t* d_centre_row, double* d_out, int32_t* d_n, int32_t* d_n_solid) {
  const char* who = "egnn_cell_boo_invariants";
  if (int rc = cell_boo_rows_check(who, d_cell_ptr, d_lattice, d_frac, d_type, n_rows, d_row_ptr, T, d_site_atom, d_site_shift, M, d_centre_atom,
                                   d_centre_row)) return rc;
  if (!d_qlm || !d_g_off || (E > 0 && (!d_g_idx || !d_g_val)) || !d_out || !d_n || !d_n_solid) {
    set_error("bad %s arguments (d_qlm, the G tables, d_out, d_n and d_n_solid given)", who);
    return EGNN_EINVAL;
  }
  if (l_solid < 0) { set_error("%s: l_solid %d (0 <= l_solid <= l_max)", who, l_solid); return EGNN_EINVAL; }
  if (int rc = cell_boo_config_check(who, A, l_max, l_solid, select)) return rc;
  if (int rc = cell_boo_table_check(who, l_max, E, g_off)) return rc;
  if (int rc = cell_soap_batch_check(who, C, N, cell_ptr, lattice, 0.0)) return rc;   // no cut here: a singular lattice is refused
  hipLaunchKernelGGL(cell_boo_invariants_kernel, dim3((M + kBooWaves - 1) / kBooWaves), dim3(64 * kBooWaves), 0,
                     reinterpret_cast<hipStream_t>(stream), d_frac, d_lattice, d_type, d_cell_ptr, C, N, A, select, l_max, d_qlm, E, d_g_off, d_g_idx,
                     d_g_val, l_solid, threshold, averaged ? 1 : 0, d_row_ptr, n_rows, T, d_site_atom, d_site_shift, M, d_centre_atom, d_centre_row,
                     d_out, d_n, d_n_solid);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

}  // extern "C"

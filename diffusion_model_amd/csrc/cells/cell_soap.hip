// SOAP descriptors of periodic cells on the device: the site list of every listed centre over an image box of up to 9^3 shifts
// (count / fill, the caller takes the prefix sum in between, as egnn_cell_bonds_count / _fill), the descriptor over a site list in
// fp64 fractional coordinates, and the mean descriptor of every cell.  Definitions: cell_soap_math.h (shared with the host
// statements, cell_soap_host.cpp); everything after the staging of a chunk is eval/soap_device.h, the text the cluster kernel
// (eval/soap.hip) runs.  An extension: dscribe's periodic=True restated from its description.
//
// No kernel has an atomic: a site row is compacted by ballot and popcount in ascending candidate order, a descriptor is the sum of
// one thread per output, a mean the running sum of one thread.  Results are bitwise identical from run to run.
//
// A kernel trusts no index: centre, cell, row, site atom and shift code are checked against the extents of the arrays before they
// are used, and every write is checked against the extent of its output.
#include "../eval/soap_device.h"
#include "cell_soap_host.h"
#include "cell_device.h"
#include "cell_soap_math.h"

namespace egnn {

// ---- site lists ----------------------------------------------------------------------------------------------------------------
// One wavefront per listed centre, four per workgroup, no LDS and no barrier.  The wavefront walks the candidates q = j nbox + t of
// its centre's cell in ascending order, 64 per step: a lane forms the vector of its candidate (cell_soap_site, the test of the
// host statement) and a ballot with a popcount prefix gives each hit its place, so a row comes out ascending by (atom, shift code).
// There is no cull: every candidate of the box is tested.  A centre outside the batch, or a cell the host check would refuse,
// gives an empty row.
template <bool FILL>
__global__ __launch_bounds__(64 * kCellSiteWaves) void cell_sites_kernel(const double* __restrict__ frac, const double* __restrict__ lattice,
                                                                        const int* __restrict__ cell_ptr, int C, int N, double cut,
                                                                        int M, const int* __restrict__ centre_atom,
                                                                        int* __restrict__ degree, const int* __restrict__ row_ptr, int T,
                                                                        int* __restrict__ site_atom, int* __restrict__ site_shift) {
  const int lane = threadIdx.x & 63, m = blockIdx.x * kCellSiteWaves + (threadIdx.x >> 6);
  if (m >= M) return;   // uniform in a wavefront; no barrier follows
  const int i = centre_atom[m];
  int c = 0, lo = 0, hi = 0, b[3] = {0, 0, 0};
  double L[9], width[3];
  bool valid = cell_of_atom(cell_ptr, C, N, i, &c, &lo, &hi);
  if (valid) {
    cell_lattice_read(lattice, c, L);
    valid = cell_soap_box(L, cut, b, width);
  }
  int row_lo = 0, row_hi = 0;
  if (FILL && !cell_row_read(row_ptr, M, T, m, &row_lo, &row_hi)) valid = false;
  if (!valid) {
    if (!FILL && lane == 0) degree[m] = 0;
    return;
  }
  const int n = hi - lo, nbox = cell_soap_box_count(b), total = n * nbox;   // at most 2^20 * 729 < 2^31
  const int self = (i - lo) * nbox + ((b[0] * (2 * b[1] + 1) + b[1]) * (2 * b[2] + 1) + b[2]);   // the candidate (i, 0)
  double wi[3];
  cell_wrapped_read(frac, i, wi);
  const double cut2 = cut * cut;
  int cnt = 0;
  for (int q0 = 0; q0 < total; q0 += 64) {   // uniform in the wavefront
    const int q = q0 + lane;
    bool hit = false;
    int j = 0, s[3] = {0, 0, 0};
    if (q < total && q != self) {
      j = q / nbox;
      cell_soap_box_shift(q - j * nbox, b, s);
      double wj[3], r[3];
      cell_wrapped_read(frac, lo + j, wj);
      hit = cell_soap_site(wj, wi, s, L, cut2, r);
    }
    const unsigned long long hits = __ballot(hit);
    if (FILL && hit) {
      const int at = row_lo + cnt + lane_prefix(hits, lane);
      if (at >= row_lo && at < row_hi) {
        site_atom[at] = lo + j;
        site_shift[at] = cell_shift_code(s[0], s[1], s[2]);
      }
    }
    cnt += __popcll(hits);
  }
  if (!FILL && lane == 0) degree[m] = cnt;
}

// ---- descriptor: one workgroup of 16 wavefronts per centre, the LDS plan of soap_descriptor_kernel ------------------------------
// The centre and the sites of its row make one sequence, the centre first (d = 0: it touches l = 0 only), staged 32 at a time: one
// thread per site reads (atom, shift code), wraps the two atoms' coordinates and calls cell_site_vector; the chunk then goes through
// soap_chunk_accumulate, the text the cluster kernel runs.  The row is `centre_row[m]` of any CSR in the format of a bond list: the
// site kernels' (row m) or a BondList of cutoff = cut (row = atom).  A site whose atom lies outside the centre's cell, whose code
// lies outside [0, 729) or whose type lies outside [0, A) contributes nothing.
//
// LDS as soap_descriptor_kernel: 136 KiB of a CU's 160 KiB at the limits, 100 KiB at the defaults and A = 2, requested as dynamic
// LDS by the entry.
__global__ __launch_bounds__(kSoapThreads) void cell_soap_kernel(const double* __restrict__ frac, const double* __restrict__ lattice,
                                                                 const int* __restrict__ type, const int* __restrict__ cell_ptr, int C, int N,
                                                                 int A, int n_max, int l_max, const double* __restrict__ tables,
                                                                 const int* __restrict__ row_ptr, int n_rows, int T,
                                                                 const int* __restrict__ site_atom, const int* __restrict__ site_shift, int M,
                                                                 const int* __restrict__ centre_atom, const int* __restrict__ centre_row,
                                                                 double* __restrict__ desc, double* __restrict__ coeff) {
  extern __shared__ double s_soap[];
  __shared__ int s_range[5];   // cell, its first and last atom, the row's first and last entry; cell -1: no such centre
  const int tid = threadIdx.x, m = blockIdx.x;
  if (m >= M) return;
  const int LM = soap_lm_count(l_max), nC = A * n_max * LM, F = soap_feature_count(A, n_max, l_max);
  const SoapLds s = soap_lds_carve(s_soap, A, n_max, l_max);
  const int i = centre_atom[m];
  if (tid == 0) {
    CellCentreRow R = {};
    const bool found = cell_centre_row_read(cell_ptr, C, N, row_ptr, n_rows, T, centre_atom, centre_row, m, &R);
    s_range[0] = found ? R.c : -1; s_range[1] = R.lo; s_range[2] = R.hi; s_range[3] = R.e0; s_range[4] = R.e1;
  }
  for (int o = tid; o < nC; o += kSoapThreads) s.c[o] = 0.0;
  __syncthreads();
  const int c = s_range[0], lo = s_range[1], hi = s_range[2], e0 = s_range[3], e1 = s_range[4];
  double* row = desc + (size_t)m * F;
  double* coeff_row = coeff ? coeff + (size_t)m * nC : nullptr;
  if (c < 0) {   // no such atom or no such row: a row of zeros, which no descriptor is
    soap_zero_row(A, n_max, l_max, row, coeff_row, tid);
    return;
  }
  const int len = 1 + (e1 - e0);   // the centre, then its sites
  for (int k0 = 0; k0 < len; k0 += kSoapChunk) {   // uniform in the workgroup
    const int cnt = min(kSoapChunk, len - k0);
    if (tid < cnt) {
      const int k = k0 + tid;
      double r[3] = {0.0, 0.0, 0.0};
      int species = -1;
      if (k == 0) {
        const int ti = type[i];
        species = (ti >= 0 && ti < A) ? ti : -1;
      } else {
        const int j = site_atom[e0 + k - 1], code = site_shift[e0 + k - 1];
        double wi[3], L[9];
        cell_wrapped_read(frac, i, wi);
        cell_lattice_read(lattice, c, L);
        if (cell_listed_site_vector(frac, L, lo, hi, wi, j, code, r)) {
          const int tj = type[j];
          species = (tj >= 0 && tj < A) ? tj : -1;
        }
      }
      s.xyz[4 * tid] = r[0]; s.xyz[4 * tid + 1] = r[1]; s.xyz[4 * tid + 2] = r[2]; s.xyz[4 * tid + 3] = cell_norm2(r);
      s.species[tid] = species;
    }
    soap_chunk_accumulate(s, cnt, A, n_max, l_max, tables, tid);
  }
  soap_finish(s, A, n_max, l_max, tables, row, coeff_row, tid);
}

// ---- mean descriptor of every cell: one thread per (cell, feature) ---------------------------------------------------------------
// Rows cell_rows[c] .. cell_rows[c + 1] of desc are the centres of cell c in this call, ascending; the thread adds them in that
// order to the running sum (zero where `first`), and where `final` divides once by count[c], the cell's centres over all calls
// (a cell without one keeps zeros).  Consecutive threads take consecutive features of one row.
__global__ __launch_bounds__(256) void cell_soap_mean_kernel(const double* __restrict__ desc, int M, const int* __restrict__ cell_rows, int C,
                                                             int F, const long long* __restrict__ count, int first, int final,
                                                             double* __restrict__ sum) {
  const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= (size_t)C * F) return;
  const int c = (int)(o / F), f = (int)(o - (size_t)c * F);
  int m0 = cell_rows[c], m1 = cell_rows[c + 1];
  if (m0 < 0 || m1 < m0 || m1 > M) m0 = m1 = 0;
  double acc = first ? 0.0 : sum[o];
  for (int m = m0; m < m1; ++m) acc += desc[(size_t)m * F + f];
  if (final) {
    const long long n = count[c];
    acc = n > 0 ? acc / (double)n : 0.0;
  }
  sum[o] = acc;
}

static int cell_sites_check(const char* who, int C, int N, const int32_t* cell_ptr, const double* lattice, const void* d_cell_ptr,
                            const void* d_lattice, const void* d_frac, double cut, int M, const void* d_centre_atom) {
  if (!d_cell_ptr || !d_lattice || (N > 0 && !d_frac) || M < 0 || (M > 0 && !d_centre_atom)) {
    set_error("bad %s arguments (d_cell_ptr, d_lattice and d_frac given; M >= 0 centres given)", who);
    return EGNN_EINVAL;
  }
  if (cut == 0.0) { set_error("%s: cut must be positive and finite", who); return EGNN_EINVAL; }
  return cell_soap_batch_check(who, C, N, cell_ptr, lattice, cut);
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_cell_sites_count(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                          const double* d_lattice, const double* d_frac, double cut, int M, const int32_t* d_centre_atom,
                          int32_t* d_degree) {
  const char* who = "egnn_cell_sites_count";
  if (int rc = cell_sites_check(who, C, N, cell_ptr, lattice, d_cell_ptr, d_lattice, d_frac, cut, M, d_centre_atom)) return rc;
  if (M > 0 && !d_degree) { set_error("bad %s arguments (d_degree given)", who); return EGNN_EINVAL; }
  if (M == 0) return EGNN_OK;
  hipLaunchKernelGGL(cell_sites_kernel<false>, dim3((M + kCellSiteWaves - 1) / kCellSiteWaves), dim3(64 * kCellSiteWaves), 0,
                     reinterpret_cast<hipStream_t>(stream), d_frac, d_lattice, d_cell_ptr, C, N, cut, M, d_centre_atom, d_degree,
                     (const int*)nullptr, 0, (int*)nullptr, (int*)nullptr);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_sites_fill(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                         const double* d_lattice, const double* d_frac, double cut, int M, const int32_t* d_centre_atom,
                         const int32_t* d_row_ptr, int T, int32_t* d_site_atom, int32_t* d_site_shift) {
  const char* who = "egnn_cell_sites_fill";
  if (int rc = cell_sites_check(who, C, N, cell_ptr, lattice, d_cell_ptr, d_lattice, d_frac, cut, M, d_centre_atom)) return rc;
  if (!d_row_ptr || T < 0 || (T > 0 && (!d_site_atom || !d_site_shift))) {
    set_error("bad %s arguments (d_row_ptr given; T >= 0 entries of d_site_atom and d_site_shift)", who);
    return EGNN_EINVAL;
  }
  if (M == 0 || T == 0) return EGNN_OK;
  hipLaunchKernelGGL(cell_sites_kernel<true>, dim3((M + kCellSiteWaves - 1) / kCellSiteWaves), dim3(64 * kCellSiteWaves), 0,
                     reinterpret_cast<hipStream_t>(stream), d_frac, d_lattice, d_cell_ptr, C, N, cut, M, d_centre_atom, (int*)nullptr,
                     d_row_ptr, T, d_site_atom, d_site_shift);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_soap_descriptor(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                              const double* d_lattice, const double* d_frac, const int32_t* d_type, int n_max, int l_max,
                              const double* d_tables, int n_rows, const int32_t* d_row_ptr, int T, const int32_t* d_site_atom,
                              const int32_t* d_site_shift, int M, const int32_t* d_centre_atom, const int32_t* d_centre_row, double* d_desc,
                              double* d_coeff) {
  const char* who = "egnn_cell_soap_descriptor";
  if (!cell_rows_given(d_cell_ptr, d_lattice, d_frac, d_type, n_rows, d_row_ptr, T, d_site_atom, d_site_shift, M, d_centre_atom, d_centre_row) ||
      !d_desc) {
    set_error("bad %s arguments (d_cell_ptr, d_lattice, d_frac, d_type, d_row_ptr, the centres and d_desc given; n_rows >= 0 rows of T >= 0 "
              "sites; M >= 1)", who);
    return EGNN_EINVAL;
  }
  if (int rc = cell_soap_basis_check(who, A, n_max, l_max, d_tables)) return rc;
  if (int rc = cell_soap_batch_check(who, C, N, cell_ptr, lattice, 0.0)) return rc;   // no cut here: a singular lattice is refused
  if ((long long)M * soap_feature_count(A, n_max, l_max) > 2147483647LL * 4) {
    set_error("%s: %d centres of %d features (at most 2^33 values a call)", who, M, soap_feature_count(A, n_max, l_max));
    return EGNN_EINVAL;
  }
  // up to 136 KiB of dynamic LDS; a CU has 160 KiB
  static LdsLimitRecord raised;
  if (int rc = raise_lds_limit(raised, &cell_soap_kernel, soap_lds_bytes(kSoapMaxTypes, kSoapMaxN, kSoapMaxL))) return rc;
  hipLaunchKernelGGL(cell_soap_kernel, dim3(M), dim3(kSoapThreads), soap_lds_bytes(A, n_max, l_max), reinterpret_cast<hipStream_t>(stream),
                     d_frac, d_lattice, d_type, d_cell_ptr, C, N, A, n_max, l_max, d_tables, d_row_ptr, n_rows, T, d_site_atom, d_site_shift, M,
                     d_centre_atom, d_centre_row, d_desc, d_coeff);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_soap_mean(void* stream, int C, int F, int M, const double* d_desc, const int32_t* d_cell_rows, const int64_t* d_count,
                        int first, int final, double* d_sum) {
  const char* who = "egnn_cell_soap_mean";
  if (C < 1 || F < 1 || M < 0 || (M > 0 && !d_desc) || !d_cell_rows || !d_sum || (final && !d_count)) {
    set_error("bad %s arguments (C, F >= 1; M >= 0 rows of d_desc; d_cell_rows and d_sum given; d_count given with final)", who);
    return EGNN_EINVAL;
  }
  const size_t total = (size_t)C * F;
  if (total > 2147483647u * (size_t)256) { set_error("%s: %d cells of %d features", who, C, F); return EGNN_EINVAL; }
  hipLaunchKernelGGL(cell_soap_mean_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_desc,
                     M, d_cell_rows, C, F, reinterpret_cast<const long long*>(d_count), first, final, d_sum);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

}  // extern "C"

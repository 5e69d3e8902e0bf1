// Relaxation of periodic cells on the device: the FIRE minimiser over the lattice energy of cell_ewald.hip, real-space sites from
// lists held over many evaluations.  Definitions, the freeze rule and the order of every sum: cell_relax_math.h (shared with the
// host statement, cell_relax_host.cpp).  An extension: no file of the reference relaxes a structure.
//
//  1. real + short over a held row: cell_ewald_real_kernel with two changes -- the coordinates are read UNWRAPPED and every entry
//     of the row (a site inside r_cut + skin when the list was built) is tested again, cell_norm2(d) < r_cut^2, before ewald_site.
//     One wavefront per row, four per workgroup, no workgroup barrier; a lane takes the entries e0 + lane, + 64, ..; the butterfly
//     wave_sum.  Bound by the VALU (erfc and exp in fp64); the entries beyond r_cut cost a distance each.
//  2. step: one workgroup of 256 threads per cell.  Thread t walks the atoms t, t + 256, .. of the cell four times: the sums (P, FF,
//     vv, max |F|^2), the largest tentative move, the largest reach since the list was built, the commit; between the walks ONE
//     tree pass over the 256 partials of every quantity of that walk in LDS (offsets 128 .. 1).  A cell that is done, or waits for
//     its list, returns at once.  Bound by latency: a few dozen bytes per atom and three dependent reductions.
//
// The reciprocal part, self term, background and finish of an evaluation are egnn_cell_ewald_amplitudes, _recip and _finish on the
// current coordinates (they wrap on read).  All fp64 and no floating-point atomic; two runs give the same bits, and a cell gives the
// same bits alone and in any batch.  A kernel trusts no index: cell, row, site atom, shift code, type and step are checked against
// the extents of the arrays before they are used.  The LDS of kernel 2 is static, 8 KiB.
#include "cell_device.h"
#include "cell_relax_host.h"
#include "cell_relax_math.h"

namespace egnn {

// out [M, 5] = (e_real, e_short, F_x, F_y, F_z) of centre m; a row without a centre or a CSR row, or a centre of no type, is zeros.
// flag [C]: set to 1 (a plain store; every writer stores the same value) where a site of the cell lies on its centre.
__global__ __launch_bounds__(64 * kEwaldWaves) void cell_relax_real_kernel(const double* __restrict__ frac, const double* __restrict__ lattice,
                                                                          const int* __restrict__ type, const int* __restrict__ cell_ptr, int C,
                                                                          int N, EwaldModel P, const int* __restrict__ row_ptr, int n_rows, int T,
                                                                          const int* __restrict__ site_atom, const int* __restrict__ site_shift,
                                                                          int M, const int* __restrict__ centre_atom,
                                                                          const int* __restrict__ centre_row, double* __restrict__ out,
                                                                          int* __restrict__ flag) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = blockIdx.x * kEwaldWaves + wave;
  if (m >= M) return;   // uniform in a wavefront; no workgroup barrier follows
  CellCentreRow R;
  double er = 0.0, es = 0.0, F[3] = {0.0, 0.0, 0.0};
  bool on_centre = false;
  int ti = -1;
  const bool valid = cell_centre_row_read(cell_ptr, C, N, row_ptr, n_rows, T, centre_atom, centre_row, m, &R);
  if (valid) ti = type[R.i];
  if (valid && ti >= 0 && ti < P.A) {
    double L[9], ui[3];
    cell_lattice_read(lattice, R.c, L);
    for (int k = 0; k < 3; ++k) ui[k] = frac[3 * (size_t)R.i + k];
    const double cut2 = P.r_cut * P.r_cut;
    for (int e = R.e0 + lane; e < R.e1; e += 64) {
      const int j = site_atom[e];
      double d[3];
      if (!relax_held_site(frac, L, R.lo, R.hi, ui, j, site_shift[e], cut2, d)) continue;
      const int tj = type[j];
      if (tj < 0 || tj >= P.A) continue;
      const double r2 = cell_norm2(d);
      if (r2 == 0.0) { on_centre = true; continue; }
      double a, b, f;
      ewald_site(P, ti, tj, r2, &a, &b, &f);
      er += a;
      es += b;
      F[0] += f * d[0];
      F[1] += f * d[1];
      F[2] += f * d[2];
    }
    er = wave_sum(er);
    es = wave_sum(es);
    F[0] = wave_sum(F[0]);
    F[1] = wave_sum(F[1]);
    F[2] = wave_sum(F[2]);
    if (__ballot(on_centre) && lane == 0) flag[R.c] = 1;
    er = ewald_real_energy(P, ti, er);
    es = ewald_short_energy(es);
  }
  if (lane == 0) {
    double* o = out + (size_t)m * 5;
    o[0] = er; o[1] = es; o[2] = F[0]; o[3] = F[1]; o[4] = F[2];
  }
}

// the tree of cell_relax_math.h over the 256 partials of kArrays quantities at once: s[k][t] (+ or max)= s[k][t + off], off = 128 ..
// 1; bit k of kMaxMask makes array k a maximum.  Every thread of the workgroup calls it; out[k] = s[k][0] after the last barrier.
template <int kArrays, unsigned kMaxMask>
__device__ __forceinline__ void relax_tree(double (*s)[kRelaxThreads], int t, double* out) {
  for (int off = kRelaxThreads / 2; off > 0; off >>= 1) {
    __syncthreads();
    if (t < off) {
#pragma unroll
      for (int k = 0; k < kArrays; ++k) s[k][t] = ((kMaxMask >> k) & 1u) ? relax_max(s[k][t], s[k][t + off]) : s[k][t] + s[k][t + off];
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kArrays; ++k) out[k] = s[k][0];
  __syncthreads();   // the arrays may be written again
}

// One workgroup per cell: the step of cell_relax_math.h.  Every branch below is uniform in the workgroup (it depends on the cell's
// state and on reduced values that every thread reads from LDS), so every thread meets the same barriers.
__global__ __launch_bounds__(kRelaxThreads) void cell_relax_step_kernel(const int* __restrict__ cell_ptr, int C, int N, FireModel M,
                                                                       const double* __restrict__ lattice, const double* __restrict__ force,
                                                                       const double* __restrict__ energy, const int* __restrict__ coincident,
                                                                       double* __restrict__ frac, double* __restrict__ velocity,
                                                                       double* __restrict__ since, double* __restrict__ moved,
                                                                       double* __restrict__ scalars, int* __restrict__ counters,
                                                                       int* __restrict__ done, int* __restrict__ rebuild,
                                                                       double* __restrict__ energy_trace, double* __restrict__ force_trace) {
  __shared__ double s_part[4][kRelaxThreads];
  const int c = blockIdx.x, t = threadIdx.x;
  int lo = 0, n = 0;
  if (!cell_read(c, cell_ptr, C, N, &lo, &n) || n > kCellMaxAtoms) return;   // uniform
  // Uniform but for one harmless case: thread 0 of the coincident branch below may store done[c] = 1 before a later wavefront has
  // read it here; that wavefront then leaves by this line and not by that branch, and neither touches the state.
  if (done[c] || rebuild[c]) return;
  double* sc = scalars + (size_t)c * kRelaxScalars;
  int* ct = counters + (size_t)c * kRelaxCounters;
  if (coincident[c]) {
    if (t == 0) { ct[kRelaxStatus] = kRelaxCoincident; done[c] = 1; }
    return;
  }
  const double* F = force + 3 * (size_t)lo;
  double* u = frac + 3 * (size_t)lo;
  double* v = velocity + 3 * (size_t)lo;
  double* s = since + 3 * (size_t)lo;
  double* mv = moved + 3 * (size_t)lo;
  double four[4], sums[4];
  relax_thread_sums(t, n, F, v, four);
  for (int k = 0; k < 4; ++k) s_part[k][t] = four[k];
  relax_tree<4, 8u>(s_part, t, sums);   // P, FF, vv summed; fm2 a maximum
  // the state is read by every thread before thread 0 writes any of it: the barriers of the trees below lie between
  const int steps = ct[kRelaxSteps];
  const RelaxPlan R = relax_plan(M, sc[kRelaxDt], sc[kRelaxA], ct[kRelaxNPos], steps, sums);
  if (R.status == kRelaxNotFinite) {
    if (t == 0) { ct[kRelaxStatus] = R.status; done[c] = 1; }
    return;
  }
  const double fm = sqrt(sums[3]), E = energy[c];
  const bool in_trace = relax_in_trace(M, steps);
  if (R.status != kRelaxRunning) {
    if (t == 0) {
      sc[kRelaxEnergy] = E;
      sc[kRelaxMaxForce] = fm;
      if (steps == 0) sc[kRelaxInitial] = E;
      if (energy_trace && in_trace) energy_trace[(size_t)steps * C + c] = E;
      if (force_trace && in_trace) force_trace[(size_t)steps * C + c] = fm;
      ct[kRelaxStatus] = R.status;
      done[c] = 1;
    }
    return;
  }
  double m2, two[2];
  s_part[0][t] = relax_thread_move(t, n, R, F, v);
  relax_tree<1, 1u>(s_part, t, &m2);
  const double scale = relax_cap(M, m2);
  relax_thread_reach(t, n, R, scale, F, v, s, two);
  s_part[0][t] = two[0];
  s_part[1][t] = two[1];
  relax_tree<2, 3u>(s_part, t, two);
  const bool frozen = relax_frozen(M, two[0], two[1]);
  const int frozen_at = ct[kRelaxFrozen];   // only thread 0 uses it, and only thread 0 writes it
  if (t == 0) {
    sc[kRelaxEnergy] = E;
    sc[kRelaxMaxForce] = fm;
    if (steps == 0) sc[kRelaxInitial] = E;
    if (energy_trace && in_trace) energy_trace[(size_t)steps * C + c] = E;
    if (force_trace && in_trace) force_trace[(size_t)steps * C + c] = fm;
  }
  if (frozen) {
    if (t == 0) {
      if (relax_stuck(frozen_at, steps)) { ct[kRelaxStatus] = kRelaxStuck; done[c] = 1; }
      else { ct[kRelaxFrozen] = steps + 1; rebuild[c] = 1; }
    }
    return;
  }
  double L[9], K[9];
  cell_lattice_read(lattice, c, L);
  relax_inverse(L, K);
  relax_thread_commit(t, n, R, scale, K, F, u, v, s, mv);
  if (t == 0) {
    sc[kRelaxDt] = R.dt;
    sc[kRelaxA] = R.a;
    ct[kRelaxNPos] = R.n_pos;
    ct[kRelaxSteps] = steps + 1;
  }
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_cell_relax_real(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                         const double* d_lattice, const double* d_frac, const int32_t* d_type, const double* charges, const double* pot, int n,
                         int shift, double kappa, double alpha, double r_cut, double short_cut, double k_max, double skin, int n_rows,
                         const int32_t* d_row_ptr, int T, const int32_t* d_site_atom, const int32_t* d_site_shift, int M,
                         const int32_t* d_centre_atom, const int32_t* d_centre_row, double* d_real, int32_t* d_coincident) {
  const char* who = "egnn_cell_relax_real";
  if (!cell_rows_given(d_cell_ptr, d_lattice, d_frac, d_type, n_rows, d_row_ptr, T, d_site_atom, d_site_shift, M, d_centre_atom, d_centre_row) ||
      !d_real || !d_coincident) {
    set_error("bad %s arguments (d_cell_ptr, d_lattice, d_frac, d_type, d_row_ptr and the centres given; n_rows >= 0 rows of T >= 0 sites; "
              "M >= 1; d_real and d_coincident given)", who);
    return EGNN_EINVAL;
  }
  if (!(skin > 0.0 && skin < 1e300)) { set_error("%s: skin = %g must be positive and finite", who, skin); return EGNN_EINVAL; }
  EwaldModel P;
  if (int rc = cell_ewald_model_check(who, A, charges, pot, n, shift, kappa, alpha, r_cut, short_cut, k_max, 1, &P)) return rc;
  if (int rc = cell_ewald_batch_check(who, C, N, A, cell_ptr, lattice, r_cut, k_max)) return rc;
  if (int rc = cell_soap_batch_check(who, C, N, cell_ptr, lattice, r_cut + skin)) return rc;
  hipLaunchKernelGGL(cell_relax_real_kernel, dim3((M + kEwaldWaves - 1) / kEwaldWaves), dim3(64 * kEwaldWaves), 0,
                     reinterpret_cast<hipStream_t>(stream), d_frac, d_lattice, d_type, d_cell_ptr, C, N, P, d_row_ptr, n_rows, T, d_site_atom,
                     d_site_shift, M, d_centre_atom, d_centre_row, d_real, d_coincident);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_relax_step(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                         const double* d_lattice, const double* d_force, const double* d_energy, const int32_t* d_coincident, double dt_max,
                         int n_min, double f_inc, double f_dec, double a_start, double f_a, double max_step, double f_max, int max_steps,
                         double skin, double* d_frac, double* d_velocity, double* d_since, double* d_moved, double* d_scalars,
                         int32_t* d_counters, int32_t* d_done, int32_t* d_rebuild, double* d_energy_trace, double* d_force_trace) {
  const char* who = "egnn_cell_relax_step";
  FireModel M;
  if (int rc = cell_relax_fire_check(who, dt_max, n_min, f_inc, f_dec, a_start, f_a, max_step, f_max, max_steps, skin, &M)) return rc;
  if (int rc = cell_relax_batch_check(who, C, N, cell_ptr, lattice)) return rc;
  if (!d_cell_ptr || !d_lattice || !d_energy || !d_coincident || !d_scalars || !d_counters || !d_done || !d_rebuild ||
      (N > 0 && (!d_force || !d_frac || !d_velocity || !d_since || !d_moved))) {
    set_error("bad %s arguments (the device copies of the cells, d_force, d_energy, d_coincident, the state arrays, the counters and the two "
              "flag arrays given)", who);
    return EGNN_EINVAL;
  }
  hipLaunchKernelGGL(cell_relax_step_kernel, dim3(C), dim3(kRelaxThreads), 0, reinterpret_cast<hipStream_t>(stream), d_cell_ptr, C, N, M,
                     d_lattice, d_force, d_energy, d_coincident, d_frac, d_velocity, d_since, d_moved, d_scalars, d_counters, d_done, d_rebuild,
                     d_energy_trace, d_force_trace);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

}  // extern "C"

// Lattice energy of periodic cells on the device: the Ewald sum of point charges and a short-range pair potential (BKS), per-atom
// energies and forces.  Definitions, prefactors and the order of every sum: cell_ewald_math.h (shared with the host statement,
// cell_ewald_host.cpp).  An extension: no file of the reference computes an energy.
//
//  1. real + short: one wavefront per row of the site CSR (egnn_cell_sites_* at cut = r_cut), four per workgroup and no workgroup
//     barrier.  A lane takes the entries e0 + lane, + 64, ..: the site vector from the fractional coordinates, erfc, exp and the
//     pair potential (ewald_site), five running sums; then the butterfly wave_sum.  Bound by the VALU (erfc and exp in fp64).
//  2. amplitudes: the vector table of a cell, filled as sq.hip fills it, and one thread per vector that adds the cell's atoms in
//     ascending order from LDS tiles (all lanes read the same atom: a broadcast), one sincospi a term.  Bound by the VALU.
//  3. reciprocal, per atom: one wavefront per atom; the lanes walk the cell's vector table 64 at a time (coalesced), one sincospi a
//     term, four running sums, the same butterfly.  Bound by the VALU.
//  4. finish: per atom the five components, the energy and the force; per cell the sums over its atoms in ascending order.
//  5. the strain derivative of that energy (cell_stress_math.h: the Ewald virial, stress, pressure), asked for separately and by
//     kernels of its own, so that 1 - 4 produce the same bits with or without it: a second walk of the rows of 1 with twelve
//     running sums (real and short virial), a second walk of the vector table of 3 with six (B_m from the stored k), and a finish
//     in the pattern of 4.  The orders and the guards are those of 1, 3 and 4.
//
// All fp64 and no floating-point atomic: every sum is a lane's running sum, a fixed butterfly or an ascending running sum, so two
// runs give the same bits and a cell gives the same bits alone, in any batch and through any slab of centres.  The integer atomics
// of the finish count the atoms per type of a cell.
//
// A kernel trusts no index: centre, cell, row, site atom, shift code, type, vector range and plan are checked against the extents
// of the arrays before they are used.  The LDS of kernel 2 is static, 32 KiB: below the default limit, nothing to raise.
#include "../eval/sq_device.h"
#include "cell_device.h"
#include "cell_ewald_host.h"
#include "cell_ewald_math.h"
#include "cell_stress_math.h"

namespace egnn {

// ---- 1: real space ---------------------------------------------------------------------------------------------------------------
// out [M, 5] = (e_real, e_short, F_x, F_y, F_z) of centre m; a row without a centre or a CSR row, or a centre of no type, is zeros.
// flag [C]: set to 1 (a plain store; every writer stores the same value) where a site of the cell lies on its centre.
__global__ __launch_bounds__(64 * kEwaldWaves) void cell_ewald_real_kernel(const double* __restrict__ frac, const double* __restrict__ lattice,
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
    double L[9], wi[3];
    cell_lattice_read(lattice, R.c, L);
    cell_wrapped_read(frac, R.i, wi);
    for (int e = R.e0 + lane; e < R.e1; e += 64) {
      const int j = site_atom[e];
      double d[3];
      if (!cell_listed_site_vector(frac, L, R.lo, R.hi, wi, j, site_shift[e], d)) continue;
      const int tj = type[j];
      if (tj < 0 || tj >= P.A) continue;
      const double r2 = cell_norm2(d);
      if (r2 == 0.0) { on_centre = true; continue; }
      double a, b, f;
      ewald_site(P, ti, tj, r2, &a, &b, &f);
      er += a;
      es += b;
      if (P.forces) {
        F[0] += f * d[0];
        F[1] += f * d[1];
        F[2] += f * d[2];
      }
    }
    er = wave_sum(er);
    es = wave_sum(es);
    if (P.forces) {
      F[0] = wave_sum(F[0]);
      F[1] = wave_sum(F[1]);
      F[2] = wave_sum(F[2]);
    }
    if (__ballot(on_centre) && lane == 0) flag[R.c] = 1;
    er = ewald_real_energy(P, ti, er);
    es = ewald_short_energy(es);
  }
  if (lane == 0) {
    double* o = out + (size_t)m * 5;
    o[0] = er; o[1] = es; o[2] = F[0]; o[3] = F[1]; o[4] = F[2];
  }
}

// ---- 2: the vectors and their amplitudes -----------------------------------------------------------------------------------------
// the walk of sq_cell_fill_kernel, writing (h, k, l) of the row's vectors from row_ptr[row] on: ascending (h, k, l) in a cell
__global__ __launch_bounds__(256) void cell_ewald_fill_kernel(const int* __restrict__ plan, const double* __restrict__ lattice, double k_max,
                                                              int n_rows, const int* __restrict__ row_ptr, int K, int* __restrict__ hkl) {
  SqRow R;
  if (!sq_row_read(plan, lattice, blockIdx.y, blockIdx.x * 256 + threadIdx.x, n_rows, &R)) return;
  const int v0 = row_ptr[R.row], v1 = row_ptr[R.row + 1];
  if (v0 < 0 || v1 < v0 || v1 > K) return;
  sq_row_vectors(R.h, R.k, R.Lb, R.Bm, k_max, [&](int n, int l, double) {
    const int v = v0 + n;
    if (v >= v1) return;
    hkl[3 * (size_t)v] = R.h;
    hkl[3 * (size_t)v + 1] = R.k;
    hkl[3 * (size_t)v + 2] = l;
  });
}

// One workgroup of 256 threads per tile {cell, first vector (local)}: a thread owns one vector.  The cell's wrapped coordinates and
// charges are staged in LDS kEwaldAtomChunk atoms at a time (an atom of no type has charge 0) and added in ascending order.
// vec [K, 5] = (k_x, k_y, k_z, g S^c, g S^s).
__global__ __launch_bounds__(256) void cell_ewald_amplitude_kernel(const int* __restrict__ cell_ptr, const int* __restrict__ vec_ptr, int C, int N,
                                                                   EwaldModel P, const double* __restrict__ lattice,
                                                                   const double* __restrict__ frac, const int* __restrict__ type,
                                                                   const int* __restrict__ tiles, const int* __restrict__ hkl, int K,
                                                                   double* __restrict__ vec) {
  __shared__ double s_w[3 * kEwaldAtomChunk];
  __shared__ double s_q[kEwaldAtomChunk];
  const int tid = threadIdx.x;
  const int c = tiles[2 * blockIdx.x], v_first = tiles[2 * blockIdx.x + 1];
  int lo, n;
  if (v_first < 0 || !cell_read(c, cell_ptr, C, N, &lo, &n)) return;   // uniform
  const int hi = lo + n, v_lo = vec_ptr[c], v_hi = vec_ptr[c + 1];
  if (v_lo < 0 || v_hi < v_lo || v_hi > K || v_first >= v_hi - v_lo) return;
  const int v = v_lo + v_first + tid;
  const bool live = v < v_hi;
  const int h = live ? hkl[3 * (size_t)v] : 0, k = live ? hkl[3 * (size_t)v + 1] : 0, l = live ? hkl[3 * (size_t)v + 2] : 0;
  double sc = 0.0, ss = 0.0;
  for (int j0 = lo; j0 < hi; j0 += kEwaldAtomChunk) {
    const int m = min(kEwaldAtomChunk, hi - j0);
    __syncthreads();
    for (int t = tid; t < 3 * m; t += 256) s_w[t] = cell_wrap(frac[3 * (size_t)j0 + t]);
    for (int t = tid; t < m; t += 256) {
      const int tj = type[j0 + t];
      s_q[t] = tj >= 0 && tj < P.A ? P.charge[tj] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < m; ++j) {
      double sn, cs;
      sq_phase_sincos(sq_phase(h, k, l, &s_w[3 * j]), &sn, &cs);
      const double qj = s_q[j];
      sc += qj * cs;
      ss += qj * sn;
    }
  }
  if (!live) return;
  double L[9], Bm[9], kv[3];
  cell_lattice_read(lattice, c, L);
  double* o = vec + 5 * (size_t)v;
  if (!sq_reciprocal(L, Bm)) {
    for (int x = 0; x < 5; ++x) o[x] = 0.0;
    return;
  }
  ewald_kvec(h, k, l, Bm, kv);
  const double g = ewald_g(cell_norm2(kv), P.alpha);
  o[0] = kv[0]; o[1] = kv[1]; o[2] = kv[2];
  o[3] = g * sc;
  o[4] = g * ss;
}

// ---- 3: reciprocal space, per atom -----------------------------------------------------------------------------------------------
// rec [N, 4] = (e_rec, F_x, F_y, F_z) of batch atom i; an atom of no cell or type, or of a cell without a sane vector range, is zeros
__global__ __launch_bounds__(64 * kEwaldWaves) void cell_ewald_recip_kernel(const int* __restrict__ cell_ptr, const int* __restrict__ vec_ptr, int C,
                                                                           int N, EwaldModel P, const double* __restrict__ lattice,
                                                                           const double* __restrict__ frac, const int* __restrict__ type,
                                                                           const int* __restrict__ hkl, const double* __restrict__ vec, int K,
                                                                           double* __restrict__ rec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = blockIdx.x * kEwaldWaves + wave;
  if (i >= N) return;   // uniform in a wavefront; no workgroup barrier follows
  int c, lo, hi;
  double e = 0.0, F[3] = {0.0, 0.0, 0.0};
  if (cell_of_atom(cell_ptr, C, N, i, &c, &lo, &hi)) {
    const int ti = type[i], v_lo = vec_ptr[c], v_hi = vec_ptr[c + 1];
    if (ti >= 0 && ti < P.A && v_lo >= 0 && v_hi >= v_lo && v_hi <= K) {
      double L[9], wi[3];
      cell_lattice_read(lattice, c, L);
      cell_wrapped_read(frac, i, wi);
      for (int v = v_lo + lane; v < v_hi; v += 64) {
        const double* tv = vec + 5 * (size_t)v;
        double sn, cs;
        sq_phase_sincos(sq_phase(hkl[3 * (size_t)v], hkl[3 * (size_t)v + 1], hkl[3 * (size_t)v + 2], wi), &sn, &cs);
        const double gc = tv[3], gs = tv[4];
        e += ewald_recip_energy_term(sn, cs, gc, gs);
        if (P.forces) {
          const double ft = ewald_recip_force_term(sn, cs, gc, gs);
          F[0] += tv[0] * ft;
          F[1] += tv[1] * ft;
          F[2] += tv[2] * ft;
        }
      }
      const double V = ewald_volume(L), qi = P.charge[ti];
      e = ewald_recip_energy(P, V, qi, wave_sum(e));
      if (P.forces)
        for (int x = 0; x < 3; ++x) F[x] = ewald_recip_force(P, V, qi, wave_sum(F[x]));
    }
  }
  if (lane == 0) {
    double* o = rec + (size_t)i * 4;
    o[0] = e; o[1] = F[0]; o[2] = F[1]; o[3] = F[2];
  }
}

// ---- 4: finish -------------------------------------------------------------------------------------------------------------------
// n_type [C, A] (zeroed before): the atoms of every type of every cell.  Integer atomics: the counts do not depend on their order.
__global__ __launch_bounds__(256) void cell_ewald_count_kernel(const int* __restrict__ cell_ptr, int C, int N, int A, const int* __restrict__ type,
                                                               int* __restrict__ n_type) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  int c, lo, hi;
  if (i >= N || !cell_of_atom(cell_ptr, C, N, i, &c, &lo, &hi)) return;
  const int t = type[i];
  if (t >= 0 && t < A) atomicAdd(&n_type[c * A + t], 1);
}

// one thread per atom: comp [N, 5], energy_per_atom [N], force [N, 3] = real [i, 2..4] + rec [i, 1..3] (where forces are asked for)
__global__ __launch_bounds__(256) void cell_ewald_atom_kernel(const int* __restrict__ cell_ptr, int C, int N, EwaldModel P,
                                                              const double* __restrict__ lattice, const int* __restrict__ type,
                                                              const int* __restrict__ n_type, const double* __restrict__ real,
                                                              const double* __restrict__ rec, double* __restrict__ comp,
                                                              double* __restrict__ energy_per_atom, double* __restrict__ force) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int c, lo, hi;
  double cp[kEwaldComponents] = {0.0, 0.0, 0.0, 0.0, 0.0}, F[3] = {0.0, 0.0, 0.0};
  if (cell_of_atom(cell_ptr, C, N, i, &c, &lo, &hi)) {
    const int ti = type[i];
    if (ti >= 0 && ti < P.A) {
      double L[9];
      cell_lattice_read(lattice, c, L);
      const double V = ewald_volume(L), qi = P.charge[ti];
      cp[kEwaldReal] = real[5 * (size_t)i];
      cp[kEwaldShort] = real[5 * (size_t)i + 1];
      cp[kEwaldSelf] = ewald_self(P, qi);
      cp[kEwaldBackground] = ewald_background(P, V, qi, ewald_cell_charge(P, n_type + (size_t)c * P.A));
      if (rec) cp[kEwaldRecip] = rec[4 * (size_t)i];
      for (int x = 0; x < 3; ++x) F[x] = rec ? real[5 * (size_t)i + 2 + x] + rec[4 * (size_t)i + 1 + x] : real[5 * (size_t)i + 2 + x];
    }
  }
  for (int k = 0; k < kEwaldComponents; ++k) comp[kEwaldComponents * (size_t)i + k] = cp[k];
  energy_per_atom[i] = ewald_atom_energy(cp);
  if (force)
    for (int x = 0; x < 3; ++x) force[3 * (size_t)i + x] = F[x];
}

// one wavefront per cell: lane k < 5 adds component k of the cell's atoms, lane 5 their energies, in ascending atom order
__global__ __launch_bounds__(64) void cell_ewald_cell_kernel(const int* __restrict__ cell_ptr, int C, int N, const double* __restrict__ comp,
                                                             const double* __restrict__ energy_per_atom, double* __restrict__ components,
                                                             double* __restrict__ energy) {
  const int c = blockIdx.x, lane = threadIdx.x;
  int lo = 0, n = 0;
  if (lane > kEwaldComponents) return;
  const bool valid = cell_read(c, cell_ptr, C, N, &lo, &n);
  double sum = 0.0;
  if (valid) {
    const double* src = lane < kEwaldComponents ? comp + kEwaldComponents * (size_t)lo + lane : energy_per_atom + lo;
    const int step = lane < kEwaldComponents ? kEwaldComponents : 1;
#pragma unroll 8
    for (int i = 0; i < n; ++i) sum += src[(size_t)i * step];
  }
  if (lane < kEwaldComponents) components[kEwaldComponents * (size_t)c + lane] = sum;
  else energy[c] = sum;
}

// ---- 5: the strain derivative (cell_stress_math.h) ---------------------------------------------------------------------------------
// A second walk of the rows of kernel 1, which stays as it is: out [M, 12] = D_real (six, Voigt order) and D_short (six) of centre
// m; a row without a centre or a CSR row, or a centre of no type, is zeros.  Twelve running sums a lane, the butterfly of kernel 1.
// Bound by the VALU (erfc and exp in fp64, as kernel 1).
__global__ __launch_bounds__(64 * kEwaldWaves) void cell_ewald_virial_real_kernel(const double* __restrict__ frac, const double* __restrict__ lattice,
                                                                                 const int* __restrict__ type, const int* __restrict__ cell_ptr,
                                                                                 int C, int N, EwaldModel P, const int* __restrict__ row_ptr,
                                                                                 int n_rows, int T, const int* __restrict__ site_atom,
                                                                                 const int* __restrict__ site_shift, int M,
                                                                                 const int* __restrict__ centre_atom,
                                                                                 const int* __restrict__ centre_row, double* __restrict__ out,
                                                                                 int* __restrict__ flag) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = blockIdx.x * kEwaldWaves + wave;
  if (m >= M) return;   // uniform in a wavefront; no workgroup barrier follows
  CellCentreRow R;
  double sum[2 * kVoigt];
  for (int v = 0; v < 2 * kVoigt; ++v) sum[v] = 0.0;
  bool on_centre = false;
  int ti = -1;
  const bool valid = cell_centre_row_read(cell_ptr, C, N, row_ptr, n_rows, T, centre_atom, centre_row, m, &R);
  if (valid) ti = type[R.i];
  if (valid && ti >= 0 && ti < P.A) {
    double L[9], wi[3];
    cell_lattice_read(lattice, R.c, L);
    cell_wrapped_read(frac, R.i, wi);
    for (int e = R.e0 + lane; e < R.e1; e += 64) {
      const int j = site_atom[e];
      double d[3];
      if (!cell_listed_site_vector(frac, L, R.lo, R.hi, wi, j, site_shift[e], d)) continue;
      const int tj = type[j];
      if (tj < 0 || tj >= P.A) continue;
      const double r2 = cell_norm2(d);
      if (r2 == 0.0) { on_centre = true; continue; }
      double fr, fs;
      ewald_site_factors(P, ti, tj, r2, &fr, &fs);
      ewald_virial_add(fr, fs, d, sum);
    }
    for (int v = 0; v < 2 * kVoigt; ++v) sum[v] = ewald_virial_site_sum(wave_sum(sum[v]));
    if (__ballot(on_centre) && lane == 0) flag[R.c] = 1;
  }
  if (lane == 0) {
    double* o = out + (size_t)m * (2 * kVoigt);
    for (int v = 0; v < 2 * kVoigt; ++v) o[v] = sum[v];
  }
}

// One wavefront per atom over its cell's vector table, as kernel 3: rec [N, 6] = D_rec of batch atom i; an atom of no cell or type,
// or of a cell without a sane vector range, is zeros.  B_m from the stored k, six running sums.  Bound by the VALU (one sincospi a
// term; the six B are a reciprocal and a dozen multiplications beside it).
__global__ __launch_bounds__(64 * kEwaldWaves) void cell_ewald_virial_recip_kernel(const int* __restrict__ cell_ptr, const int* __restrict__ vec_ptr,
                                                                                  int C, int N, EwaldModel P, const double* __restrict__ lattice,
                                                                                  const double* __restrict__ frac, const int* __restrict__ type,
                                                                                  const int* __restrict__ hkl, const double* __restrict__ vec, int K,
                                                                                  double* __restrict__ rec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = blockIdx.x * kEwaldWaves + wave;
  if (i >= N) return;   // uniform in a wavefront; no workgroup barrier follows
  int c, lo, hi;
  double sum[kVoigt] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (cell_of_atom(cell_ptr, C, N, i, &c, &lo, &hi)) {
    const int ti = type[i], v_lo = vec_ptr[c], v_hi = vec_ptr[c + 1];
    if (ti >= 0 && ti < P.A && v_lo >= 0 && v_hi >= v_lo && v_hi <= K) {
      double L[9], wi[3];
      cell_lattice_read(lattice, c, L);
      cell_wrapped_read(frac, i, wi);
      for (int v = v_lo + lane; v < v_hi; v += 64) {
        const double* tv = vec + 5 * (size_t)v;
        double sn, cs, B[kVoigt];
        sq_phase_sincos(sq_phase(hkl[3 * (size_t)v], hkl[3 * (size_t)v + 1], hkl[3 * (size_t)v + 2], wi), &sn, &cs);
        const double kv[3] = {tv[0], tv[1], tv[2]};
        const double term = ewald_recip_energy_term(sn, cs, tv[3], tv[4]);
        ewald_recip_B(kv, P.alpha, B);
        for (int x = 0; x < kVoigt; ++x) sum[x] += term * B[x];
      }
      const double V = ewald_volume(L), qi = P.charge[ti];
      for (int x = 0; x < kVoigt; ++x) sum[x] = ewald_recip_energy(P, V, qi, wave_sum(sum[x]));
    }
  }
  if (lane == 0)
    for (int x = 0; x < kVoigt; ++x) rec[(size_t)i * kVoigt + x] = sum[x];
}

// one thread per atom: comp [N, 5, 6] (component, Voigt) and per_atom [N, 6]
__global__ __launch_bounds__(256) void cell_ewald_virial_atom_kernel(const int* __restrict__ cell_ptr, int C, int N, EwaldModel P,
                                                                     const double* __restrict__ lattice, const int* __restrict__ type,
                                                                     const int* __restrict__ n_type, const double* __restrict__ real,
                                                                     const double* __restrict__ rec, double* __restrict__ comp,
                                                                     double* __restrict__ per_atom) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int c, lo, hi, ti = -1;
  double e_bg = 0.0;
  bool live = cell_of_atom(cell_ptr, C, N, i, &c, &lo, &hi);
  if (live) ti = type[i];
  live = live && ti >= 0 && ti < P.A;
  if (live) {
    double L[9];
    cell_lattice_read(lattice, c, L);
    e_bg = ewald_background(P, ewald_volume(L), P.charge[ti], ewald_cell_charge(P, n_type + (size_t)c * P.A));
  }
  for (int v = 0; v < kVoigt; ++v) {
    double cp[kEwaldComponents] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (live) {
      cp[kEwaldReal] = real[2 * kVoigt * (size_t)i + v];
      cp[kEwaldShort] = real[2 * kVoigt * (size_t)i + kVoigt + v];
      cp[kEwaldBackground] = ewald_virial_background(e_bg, v);
      if (rec) cp[kEwaldRecip] = rec[kVoigt * (size_t)i + v];
    }
    for (int k = 0; k < kEwaldComponents; ++k) comp[(kEwaldComponents * (size_t)i + k) * kVoigt + v] = cp[k];
    per_atom[kVoigt * (size_t)i + v] = ewald_atom_energy(cp);
  }
}

// one wavefront per cell, the pattern of cell_ewald_cell_kernel: lane t < 30 adds entry t of comp [., 5, 6] over the cell's atoms,
// lane 30 + v entry v of per_atom, in ascending atom order; the lanes 30 + v then divide by V and lane 30 forms the pressure
__global__ __launch_bounds__(64) void cell_ewald_virial_cell_kernel(const int* __restrict__ cell_ptr, int C, int N, const double* __restrict__ lattice,
                                                                    const double* __restrict__ comp, const double* __restrict__ per_atom,
                                                                    double* __restrict__ components, double* __restrict__ strain,
                                                                    double* __restrict__ stress, double* __restrict__ pressure) {
  constexpr int kParts = kEwaldComponents * kVoigt;
  const int c = blockIdx.x, lane = threadIdx.x;
  int lo = 0, n = 0;
  const bool valid = cell_read(c, cell_ptr, C, N, &lo, &n);   // c < C: the grid is C workgroups
  double sum = 0.0;
  if (valid && lane < kParts + kVoigt) {
    const double* src = lane < kParts ? comp + kParts * (size_t)lo + lane : per_atom + kVoigt * (size_t)lo + (lane - kParts);
    const int step = lane < kParts ? kParts : kVoigt;
#pragma unroll 8
    for (int i = 0; i < n; ++i) sum += src[(size_t)i * step];
  }
  double L[9];
  cell_lattice_read(lattice, c, L);
  const double s = sum / ewald_volume(L);
  const double three[3] = {__shfl(s, kParts), __shfl(s, kParts + 1), __shfl(s, kParts + 2)};   // every lane of the wavefront takes part
  if (lane < kParts) components[kParts * (size_t)c + lane] = sum;
  else if (lane < kParts + kVoigt) {
    strain[kVoigt * (size_t)c + (lane - kParts)] = sum;
    stress[kVoigt * (size_t)c + (lane - kParts)] = s;
    if (lane == kParts) pressure[c] = ewald_pressure(three);
  }
}

static int cell_ewald_cells_given(const char* who, const void* d_cell_ptr, const void* d_lattice, const void* d_frac, const void* d_type, int N) {
  if (!d_cell_ptr || !d_lattice || (N > 0 && (!d_frac || !d_type))) {
    set_error("bad %s arguments (the device copies of cell_ptr, the lattices, frac and type given)", who);
    return EGNN_EINVAL;
  }
  return EGNN_OK;
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_cell_ewald_real(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                         const double* d_lattice, const double* d_frac, const int32_t* d_type, const double* charges, const double* pot, int n,
                         int shift, double kappa, double alpha, double r_cut, double short_cut, double k_max, int forces, int n_rows,
                         const int32_t* d_row_ptr, int T, const int32_t* d_site_atom, const int32_t* d_site_shift, int M,
                         const int32_t* d_centre_atom, const int32_t* d_centre_row, double* d_real, int32_t* d_coincident) {
  const char* who = "egnn_cell_ewald_real";
  if (!cell_rows_given(d_cell_ptr, d_lattice, d_frac, d_type, n_rows, d_row_ptr, T, d_site_atom, d_site_shift, M, d_centre_atom, d_centre_row) ||
      !d_real || !d_coincident) {
    set_error("bad %s arguments (d_cell_ptr, d_lattice, d_frac, d_type, d_row_ptr and the centres given; n_rows >= 0 rows of T >= 0 sites; "
              "M >= 1; d_real and d_coincident given)", who);
    return EGNN_EINVAL;
  }
  EwaldModel P;
  if (int rc = cell_ewald_model_check(who, A, charges, pot, n, shift, kappa, alpha, r_cut, short_cut, k_max, forces, &P)) return rc;
  if (int rc = cell_ewald_batch_check(who, C, N, A, cell_ptr, lattice, r_cut, k_max)) return rc;
  hipLaunchKernelGGL(cell_ewald_real_kernel, dim3((M + kEwaldWaves - 1) / kEwaldWaves), dim3(64 * kEwaldWaves), 0,
                     reinterpret_cast<hipStream_t>(stream), d_frac, d_lattice, d_type, d_cell_ptr, C, N, P, d_row_ptr, n_rows, T, d_site_atom,
                     d_site_shift, M, d_centre_atom, d_centre_row, d_real, d_coincident);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_ewald_amplitudes(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* plan,
                               const int32_t* vec_ptr, const int32_t* d_cell_ptr, const double* d_lattice, const int32_t* d_plan,
                               const int32_t* d_vec_ptr, const double* d_frac, const int32_t* d_type, const double* charges, double kappa,
                               double alpha, double r_cut, double k_max, int n_rows, const int32_t* d_row_ptr, int K, const int32_t* d_tiles,
                               int n_tiles, int32_t* d_hkl, double* d_vec) {
  const char* who = "egnn_cell_ewald_amplitudes";
  if (N < 0 || !cell_ptr || cell_ptr[0] != 0 || (C >= 1 && C <= 65535 && cell_ptr[C] != N)) {
    set_error("%s: the host copy of cell_ptr must run from 0 to N = %d", who, N);
    return EGNN_EINVAL;
  }
  EwaldModel P;
  if (int rc = cell_ewald_model_check(who, A, charges, nullptr, 1, 0, kappa, alpha, r_cut, r_cut, k_max, 0, &P)) return rc;
  if (int rc = cell_ewald_batch_check(who, C, N, A, cell_ptr, lattice, r_cut, k_max)) return rc;
  int max_rows = 0;
  if (int rc = sq_plan_check(who, C, lattice, k_max, plan, n_rows, &max_rows)) return rc;
  if (int rc = sq_vec_ptr_check(who, C, vec_ptr, K)) return rc;
  if (int rc = cell_ewald_cells_given(who, d_cell_ptr, d_lattice, d_frac, d_type, N)) return rc;
  if (!d_plan || !d_vec_ptr || !d_row_ptr || n_tiles < 0 || (n_tiles > 0 && !d_tiles) || (K > 0 && (!d_hkl || !d_vec))) {
    set_error("bad %s arguments (the device copies of the plan, vec_ptr and row_ptr, n_tiles >= 0 tiles and the two outputs given)", who);
    return EGNN_EINVAL;
  }
  if (K == 0) return EGNN_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(cell_ewald_fill_kernel, dim3((max_rows + 255) / 256, C), dim3(256), 0, st, d_plan, d_lattice, k_max, n_rows, d_row_ptr, K,
                     d_hkl);
  EGNN_HIP(hipMemsetAsync(d_vec, 0, sizeof(double) * 5 * (size_t)K, st));
  if (n_tiles > 0)
    hipLaunchKernelGGL(cell_ewald_amplitude_kernel, dim3(n_tiles), dim3(256), 0, st, d_cell_ptr, d_vec_ptr, C, N, P, d_lattice, d_frac, d_type,
                       d_tiles, d_hkl, K, d_vec);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_ewald_recip(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* vec_ptr,
                          const int32_t* d_cell_ptr, const double* d_lattice, const int32_t* d_vec_ptr, const double* d_frac,
                          const int32_t* d_type, const double* charges, double kappa, double alpha, double r_cut, double k_max, int forces, int K,
                          const int32_t* d_hkl, const double* d_vec, double* d_rec) {
  const char* who = "egnn_cell_ewald_recip";
  EwaldModel P;
  if (int rc = cell_ewald_model_check(who, A, charges, nullptr, 1, 0, kappa, alpha, r_cut, r_cut, k_max, forces, &P)) return rc;
  if (int rc = cell_ewald_batch_check(who, C, N, A, cell_ptr, lattice, r_cut, k_max)) return rc;
  if (int rc = sq_vec_ptr_check(who, C, vec_ptr, K)) return rc;
  if (int rc = cell_ewald_cells_given(who, d_cell_ptr, d_lattice, d_frac, d_type, N)) return rc;
  if (!d_vec_ptr || (K > 0 && (!d_hkl || !d_vec)) || (N > 0 && !d_rec)) {
    set_error("bad %s arguments (the device copy of vec_ptr, the vector table and d_rec given)", who);
    return EGNN_EINVAL;
  }
  if (N == 0) return EGNN_OK;
  hipLaunchKernelGGL(cell_ewald_recip_kernel, dim3((N + kEwaldWaves - 1) / kEwaldWaves), dim3(64 * kEwaldWaves), 0,
                     reinterpret_cast<hipStream_t>(stream), d_cell_ptr, d_vec_ptr, C, N, P, d_lattice, d_frac, d_type, d_hkl, d_vec, K, d_rec);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_ewald_finish(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                           const double* d_lattice, const int32_t* d_type, const double* charges, double kappa, double alpha, double r_cut,
                           double k_max, const double* d_real, const double* d_rec, int32_t* d_n_type, double* d_atom_components,
                           double* d_energy_per_atom, double* d_force, double* d_components, double* d_energy) {
  const char* who = "egnn_cell_ewald_finish";
  EwaldModel P;
  if (int rc = cell_ewald_model_check(who, A, charges, nullptr, 1, 0, kappa, alpha, r_cut, r_cut, k_max, d_force != nullptr, &P)) return rc;
  if (int rc = cell_ewald_batch_check(who, C, N, A, cell_ptr, lattice, r_cut, k_max)) return rc;
  if (!d_cell_ptr || !d_lattice || !d_n_type || !d_components || !d_energy ||
      (N > 0 && (!d_type || !d_real || !d_atom_components || !d_energy_per_atom))) {
    set_error("bad %s arguments (the device copies of the cells, d_real, d_n_type and the outputs given)", who);
    return EGNN_EINVAL;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  EGNN_HIP(hipMemsetAsync(d_n_type, 0, sizeof(int32_t) * (size_t)C * A, st));
  if (N > 0) {
    hipLaunchKernelGGL(cell_ewald_count_kernel, dim3((N + 255) / 256), dim3(256), 0, st, d_cell_ptr, C, N, A, d_type, d_n_type);
    hipLaunchKernelGGL(cell_ewald_atom_kernel, dim3((N + 255) / 256), dim3(256), 0, st, d_cell_ptr, C, N, P, d_lattice, d_type, d_n_type, d_real,
                       d_rec, d_atom_components, d_energy_per_atom, d_force);
  }
  hipLaunchKernelGGL(cell_ewald_cell_kernel, dim3(C), dim3(64), 0, st, d_cell_ptr, C, N, d_atom_components, d_energy_per_atom, d_components,
                     d_energy);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_ewald_virial_real(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                                const double* d_lattice, const double* d_frac, const int32_t* d_type, const double* charges, const double* pot,
                                int n, int shift, double kappa, double alpha, double r_cut, double short_cut, double k_max, int n_rows,
                                const int32_t* d_row_ptr, int T, const int32_t* d_site_atom, const int32_t* d_site_shift, int M,
                                const int32_t* d_centre_atom, const int32_t* d_centre_row, double* d_virial, int32_t* d_coincident) {
  const char* who = "egnn_cell_ewald_virial_real";
  if (!cell_rows_given(d_cell_ptr, d_lattice, d_frac, d_type, n_rows, d_row_ptr, T, d_site_atom, d_site_shift, M, d_centre_atom, d_centre_row) ||
      !d_virial || !d_coincident) {
    set_error("bad %s arguments (d_cell_ptr, d_lattice, d_frac, d_type, d_row_ptr and the centres given; n_rows >= 0 rows of T >= 0 sites; "
              "M >= 1; d_virial and d_coincident given)", who);
    return EGNN_EINVAL;
  }
  EwaldModel P;
  if (int rc = cell_ewald_model_check(who, A, charges, pot, n, shift, kappa, alpha, r_cut, short_cut, k_max, 0, &P)) return rc;
  if (int rc = cell_ewald_batch_check(who, C, N, A, cell_ptr, lattice, r_cut, k_max)) return rc;
  hipLaunchKernelGGL(cell_ewald_virial_real_kernel, dim3((M + kEwaldWaves - 1) / kEwaldWaves), dim3(64 * kEwaldWaves), 0,
                     reinterpret_cast<hipStream_t>(stream), d_frac, d_lattice, d_type, d_cell_ptr, C, N, P, d_row_ptr, n_rows, T, d_site_atom,
                     d_site_shift, M, d_centre_atom, d_centre_row, d_virial, d_coincident);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_ewald_virial_recip(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* vec_ptr,
                                 const int32_t* d_cell_ptr, const double* d_lattice, const int32_t* d_vec_ptr, const double* d_frac,
                                 const int32_t* d_type, const double* charges, double kappa, double alpha, double r_cut, double k_max, int K,
                                 const int32_t* d_hkl, const double* d_vec, double* d_virial) {
  const char* who = "egnn_cell_ewald_virial_recip";
  EwaldModel P;
  if (int rc = cell_ewald_model_check(who, A, charges, nullptr, 1, 0, kappa, alpha, r_cut, r_cut, k_max, 0, &P)) return rc;
  if (int rc = cell_ewald_batch_check(who, C, N, A, cell_ptr, lattice, r_cut, k_max)) return rc;
  if (int rc = sq_vec_ptr_check(who, C, vec_ptr, K)) return rc;
  if (int rc = cell_ewald_cells_given(who, d_cell_ptr, d_lattice, d_frac, d_type, N)) return rc;
  if (!d_vec_ptr || (K > 0 && (!d_hkl || !d_vec)) || (N > 0 && !d_virial)) {
    set_error("bad %s arguments (the device copy of vec_ptr, the vector table and d_virial given)", who);
    return EGNN_EINVAL;
  }
  if (N == 0) return EGNN_OK;
  hipLaunchKernelGGL(cell_ewald_virial_recip_kernel, dim3((N + kEwaldWaves - 1) / kEwaldWaves), dim3(64 * kEwaldWaves), 0,
                     reinterpret_cast<hipStream_t>(stream), d_cell_ptr, d_vec_ptr, C, N, P, d_lattice, d_frac, d_type, d_hkl, d_vec, K, d_virial);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int egnn_cell_ewald_virial_finish(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                                  const double* d_lattice, const int32_t* d_type, const double* charges, double kappa, double alpha, double r_cut,
                                  double k_max, const double* d_virial_real, const double* d_virial_recip, int32_t* d_n_type,
                                  double* d_atom_components, double* d_per_atom, double* d_components, double* d_strain, double* d_stress,
                                  double* d_pressure) {
  const char* who = "egnn_cell_ewald_virial_finish";
  EwaldModel P;
  if (int rc = cell_ewald_model_check(who, A, charges, nullptr, 1, 0, kappa, alpha, r_cut, r_cut, k_max, 0, &P)) return rc;
  if (int rc = cell_ewald_batch_check(who, C, N, A, cell_ptr, lattice, r_cut, k_max)) return rc;
  if (!d_cell_ptr || !d_lattice || !d_n_type || !d_components || !d_strain || !d_stress || !d_pressure ||
      (N > 0 && (!d_type || !d_virial_real || !d_atom_components || !d_per_atom))) {
    set_error("bad %s arguments (the device copies of the cells, d_virial_real, d_n_type and the outputs given)", who);
    return EGNN_EINVAL;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  EGNN_HIP(hipMemsetAsync(d_n_type, 0, sizeof(int32_t) * (size_t)C * A, st));
  if (N > 0) {
    hipLaunchKernelGGL(cell_ewald_count_kernel, dim3((N + 255) / 256), dim3(256), 0, st, d_cell_ptr, C, N, A, d_type, d_n_type);
    hipLaunchKernelGGL(cell_ewald_virial_atom_kernel, dim3((N + 255) / 256), dim3(256), 0, st, d_cell_ptr, C, N, P, d_lattice, d_type, d_n_type,
                       d_virial_real, d_virial_recip, d_atom_components, d_per_atom);
  }
  hipLaunchKernelGGL(cell_ewald_virial_cell_kernel, dim3(C), dim3(64), 0, st, d_cell_ptr, C, N, d_lattice, d_atom_components, d_per_atom,
                     d_components, d_strain, d_stress, d_pressure);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

}  // extern "C"

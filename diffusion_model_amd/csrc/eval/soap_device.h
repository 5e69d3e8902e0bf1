// What the two SOAP descriptor kernels share (eval/soap.hip: clusters in float32 positions; cells/cell_soap.hip: the sites of every
// image of a periodic cell in fp64): the LDS plan of one workgroup of 1,024 threads per centre and everything after the staging of
// a chunk of neighbours.  A kernel stages the vectors, d2 and the species of up to kSoapChunk neighbours its own way and then runs
// this text, so the two agree bitwise on equal vectors.
#pragma once
#include "eval_device.h"
#include "soap_math.h"

namespace egnn {

constexpr int kSoapThreads = 1024;    // threads of a descriptor workgroup (16 wavefronts share the staging of a chunk)

// LDS of a descriptor kernel, in doubles: coefficients [A][n_max][LM] | solid harmonics [chunk][LM] | radial values
// [chunk][n_max (l_max+1)] | dx, dy, dz, d2 [chunk][4]; then the species of the chunk's atoms, int [chunk]
__host__ __device__ inline size_t soap_lds_doubles(int A, int n_max, int l_max) {
  return (size_t)A * n_max * soap_lm_count(l_max) + (size_t)kSoapChunk * (soap_lm_count(l_max) + n_max * (l_max + 1) + 4);
}
__host__ __device__ inline size_t soap_lds_bytes(int A, int n_max, int l_max) {
  return sizeof(double) * soap_lds_doubles(A, n_max, l_max) + sizeof(int) * kSoapChunk;
}

// the carving of the dynamic LDS of one workgroup
struct SoapLds {
  double* c;        // coefficients [A][n_max][LM]: primitives while the chunks run, then orthonormalised in place
  double* solid;    // [chunk][LM]
  double* rad;      // [chunk][n_max (l_max+1)]
  double* xyz;      // [chunk][4]: dx, dy, dz, d2
  int* species;     // [chunk]: the species of a staged neighbour, -1 where it contributes nothing
};

__device__ __forceinline__ SoapLds soap_lds_carve(double* lds, int A, int n_max, int l_max) {
  const int LM = soap_lm_count(l_max);
  SoapLds s;
  s.c = lds;
  s.solid = s.c + A * n_max * LM;
  s.rad = s.solid + kSoapChunk * LM;
  s.xyz = s.rad + kSoapChunk * n_max * (l_max + 1);
  s.species = reinterpret_cast<int*>(s.xyz + 4 * kSoapChunk);
  return s;
}

// One chunk of cnt <= kSoapChunk staged neighbours (xyz and species written by threads of this workgroup, no barrier yet): the
// workgroup's threads share the cnt (l_max+1) harmonic columns (soap_solid_column: one m, all l) and the cnt n_max (l_max+1) radial
// values (the only exp calls); then every thread adds the chunk's neighbours, ascending, to the (n, l, m) outputs it owns, one
// running sum per species in registers.  Uniform in the workgroup; ends behind a barrier, so the staging may be rewritten.
__device__ __forceinline__ void soap_chunk_accumulate(const SoapLds& s, int cnt, int A, int n_max, int l_max, const double* __restrict__ tables,
                                                      int tid) {
  const int L1 = l_max + 1, LM = soap_lm_count(l_max), nL = n_max * L1;
  const double* norm = tables + soap_table_norm(n_max, l_max);
  __syncthreads();
  for (int task = tid; task < cnt * L1; task += kSoapThreads) {
    const int jj = task / L1, m = task - jj * L1;
    if (s.species[jj] < 0) continue;
    soap_solid_column(s.xyz[4 * jj], s.xyz[4 * jj + 1], s.xyz[4 * jj + 2], s.xyz[4 * jj + 3], m, l_max, norm, s.solid + jj * LM);
  }
  for (int task = tid; task < cnt * nL; task += kSoapThreads) {
    const int jj = task / nL, q = task - jj * nL;
    if (s.species[jj] < 0) continue;
    s.rad[jj * nL + q] = soap_radial(tables, n_max, l_max, q, s.xyz[4 * jj + 3]);
  }
  __syncthreads();
  for (int o = tid; o < n_max * LM; o += kSoapThreads) {
    const int n = o / LM, lm = o - n * LM, q = n * L1 + soap_l_of(lm);
    double acc[kSoapMaxTypes];
#pragma unroll
    for (int z = 0; z < kSoapMaxTypes; ++z) acc[z] = z < A ? s.c[(z * n_max + n) * LM + lm] : 0.0;
    for (int jj = 0; jj < cnt; ++jj) {
      const int z = s.species[jj];
      if (z < 0) continue;
      const double term = s.rad[jj * nL + q] * s.solid[jj * LM + lm];
#pragma unroll
      for (int t = 0; t < kSoapMaxTypes; ++t)
        if (t == z) acc[t] += term;
    }
#pragma unroll
    for (int z = 0; z < kSoapMaxTypes; ++z)
      if (z < A) s.c[(z * n_max + n) * LM + lm] = acc[z];
  }
  __syncthreads();   // the staging is rewritten by the next chunk
}

// After the last chunk: beta over n, in place (the thread of column (z, lm) reads its n_max primitives, then writes its n_max
// coefficients); then the coefficients where asked, and the power-spectrum row with l innermost across threads: contiguous.
__device__ __forceinline__ void soap_finish(const SoapLds& s, int A, int n_max, int l_max, const double* __restrict__ tables,
                                            double* __restrict__ row, double* __restrict__ coeff_row, int tid) {
  const int LM = soap_lm_count(l_max), nC = A * n_max * LM, F = soap_feature_count(A, n_max, l_max);
  const double* beta = tables + soap_table_beta(n_max, l_max);
  for (int col = tid; col < A * LM; col += kSoapThreads) {
    const int z = col / LM, lm = col - z * LM;
    const double* bl = beta + (size_t)soap_l_of(lm) * n_max * n_max;
    double v[kSoapMaxN];
#pragma unroll
    for (int n = 0; n < kSoapMaxN; ++n) v[n] = n < n_max ? s.c[(z * n_max + n) * LM + lm] : 0.0;
    for (int n = 0; n < n_max; ++n) {
      double sum = 0.0;
#pragma unroll
      for (int np = 0; np < kSoapMaxN; ++np)
        if (np < n_max) sum += bl[n * n_max + np] * v[np];
      s.c[(z * n_max + n) * LM + lm] = sum;
    }
  }
  __syncthreads();
  if (coeff_row) for (int o = tid; o < nC; o += kSoapThreads) coeff_row[o] = s.c[o];
  for (int f = tid; f < F; f += kSoapThreads) row[f] = soap_power_entry(s.c, tables, f, A, n_max, l_max);
}

// a row of zeros, which no descriptor is: what a centre that names no atom gets
__device__ __forceinline__ void soap_zero_row(int A, int n_max, int l_max, double* __restrict__ row, double* __restrict__ coeff_row, int tid) {
  const int nC = A * n_max * soap_lm_count(l_max), F = soap_feature_count(A, n_max, l_max);
  for (int f = tid; f < F; f += kSoapThreads) row[f] = 0.0;
  if (coeff_row) for (int o = tid; o < nC; o += kSoapThreads) coeff_row[o] = 0.0;
}

}  // namespace egnn

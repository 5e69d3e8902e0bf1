// What the kernels of the evaluation families (eval/*.hip, and through cells/cell_device.h every cells/cell_*.hip) share: the steps
// of one wavefront, the reader of a {graph, first centre, first neighbour} tile, and the one policy for raising a kernel's
// dynamic-LDS limit (lds_limit.h).  What only the periodic-cell kernels share is in cells/cell_device.h.
#pragma once
#include "../common.h"
#include "lds_limit.h"

namespace egnn {

// one wavefront runs in lock step and its LDS operations complete in order, so it only has to keep the compiler from moving LDS
// accesses across this point
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// butterfly over the 64 lanes, offsets 32 .. 1: every lane ends with the same bits, the same from run to run
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// the number of set bits of a ballot below `lane`: the slot of a lane in an ascending compaction
__device__ __forceinline__ int lane_prefix(unsigned long long mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

// tile {graph, first centre, first neighbour} (local indices) of a kCentres x kChunk block of one graph's pairs.  The reader
// trusts no entry: false unless the graph lies in [0, B) and both blocks start inside it; nc and nj are what is left of the graph,
// so every atom lo + c0 + c (c < nc) and lo + j0 + j (j < nj) lies in [graph_ptr[g], graph_ptr[g + 1]).
struct PairTile {
  int g, lo, c0, j0, nc, nj;
};

template <int kCentres, int kChunk>
__device__ __forceinline__ bool pair_tile_read(const int* __restrict__ tiles, int t, const int* __restrict__ graph_ptr, int B, PairTile* T) {
  T->g = tiles[3 * t];
  T->c0 = tiles[3 * t + 1];
  T->j0 = tiles[3 * t + 2];
  if (T->g < 0 || T->g >= B) return false;
  T->lo = graph_ptr[T->g];
  const int n = graph_ptr[T->g + 1] - T->lo;
  if (T->c0 < 0 || T->j0 < 0 || T->c0 >= n || T->j0 >= n) return false;
  T->nc = min(kCentres, n - T->c0);
  T->nj = min(kChunk, n - T->j0);
  return true;
}

// Raises the dynamic-LDS limit of `kernel` to `bytes` on the current device unless `record` says it has been raised there.
template <typename Kernel>
inline int raise_lds_limit(LdsLimitRecord& record, Kernel* kernel, size_t bytes) {
  int device = 0;
  EGNN_HIP(hipGetDevice(&device));
  if (record.is_raised(device)) return EGNN_OK;
  EGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  record.mark(device);
  return EGNN_OK;
}

}  // namespace egnn

// Kernel-argument layout of the multi-tensor optimizer step (optim_step.hip).  HIP-free: plain C++ so that the size
// arithmetic below is checked by any compiler that sees it.
#pragma once
#include <stdint.h>

#include "../../../include/egnn_amd.h"

namespace egnn {

// A launch carries its tensor list BY VALUE in the kernel arguments (no device-side table to allocate, fill or keep alive,
// nothing a graph capture would have to own).  The dispatch packet's kernarg segment is 4 KiB, of which the compiler's hidden
// arguments take up to 256 B: 112 descriptors of 32 B + the header below = 3,656 B.
constexpr int kOptimCapacity = 112;    // tensors per launch (production lists: 72 / 88 tensors + the learned schedule's 8)
constexpr int kOptimThreads = 256;
constexpr int kOptimQuads = 2;         // 16-byte accesses per thread and stream, all issued before the first use
constexpr uint32_t kOptimChunk = kOptimThreads * kOptimQuads * 4;   // elements of ONE tensor per workgroup (2,048)

// internal kind of egnn_optim_interp (after the public EGNN_OPTIM_* values): p += ckp1 (g - p), the g slot carrying z
constexpr int kOptimInterp = 3;

struct OptimTensor {
  float* p;
  const float* g;
  float* s0;         // s1 / s2 sit at the launch's common byte spacing from s0
  uint32_t numel;
  uint32_t chunk0;   // first workgroup of this tensor (prefix sum of ceil(numel / kOptimChunk))
};
struct OptimLaunch {
  egnn_optim_consts c;
  int32_t n;
  int64_t d1, d2;    // byte spacing s1 - s0, s2 - s0
  OptimTensor t[kOptimCapacity];
};
static_assert(sizeof(OptimTensor) == 32, "descriptor layout");
static_assert(sizeof(OptimLaunch) + 256 <= 4096, "tensor list + hidden arguments must fit the 4 KiB kernarg segment");

}  // namespace egnn

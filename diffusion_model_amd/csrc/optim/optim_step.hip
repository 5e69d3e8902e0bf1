// The optimizer step as ONE launch over the whole parameter list: torch.optim.Adam, torch.optim.AdamW(amsgrad=True) and
// RAdamScheduleFree (parts/def_for_main.py:119-139; diffusion_model_amd/optim.py), and the y <-> x interpolation of
// RAdamScheduleFree.train() / .eval().
//
// A stream: per element 16 B read (p, g, two states) and 12 B written (20 / 16 with amsgrad), ~30 fp32 operations with one
// correctly rounded sqrt and one division.  Each workgroup takes one 2,048-element chunk of one tensor; it finds its
// (tensor, chunk) by a binary search of the prefix table in the kernel arguments (scalar loads, wave-uniform).  Every access is
// 16 bytes wide but typed with 4-BYTE alignment: gfx950 requires dword alignment only for multi-dword global accesses, so p, g
// and every state may sit at any element offset, each on its own (gradients that are views into a flat all-reduce bucket do).
// The last 1-3 elements of a tensor whose numel is not a multiple of 4 go through scalar accesses.
//
// Arithmetic: one IEEE fp32 operation per statement, in the order tests/_optim_mirror.py restates (the build has
// -ffp-contract=off; sqrtf and / are hipcc's correctly rounded ones; fp32 denormals are kept).  Do not reorder.
#include "optim_step.h"

#include "../common.h"

namespace egnn {
namespace {

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // a 16-byte access that promises dword alignment only

template <int KIND>
__device__ __forceinline__ void optim_elem(const egnn_optim_consts& k, float& p, float g, float& a, float& b, float& c) {
  if constexpr (KIND == kOptimInterp) {
    float d = g - p;
    d = k.ckp1 * d;
    p = p + d;
  } else if constexpr (KIND == EGNN_OPTIM_RADAM_SF) {   // a = z, b = exp_avg_sq (optim.py: RAdamScheduleFree.step)
    float t = g * g;
    t = t * k.one_minus_beta2;
    b = b * k.beta2;
    b = b + t;
    float gn = g;
    if (k.rectified) {
      float d = b / k.bias_correction2;
      d = sqrtf(d);
      d = d + k.eps;
      gn = g / d;
    }
    if (k.weight_decay != 0.f) {
      const float w = k.weight_decay * p;   // decay at y
      gn = gn + w;
    }
    float d = a - p;
    d = k.ckp1 * d;
    p = p + d;                              // y <- y + c (z - y)
    float u = k.adaptive_y_lr * gn;
    p = p + u;
    u = k.lr * gn;
    a = a - u;                              // z <- z - lr gn
  } else {                                  // a = exp_avg, b = exp_avg_sq, c = max_exp_avg_sq (torch's _single_tensor_adam)
    if constexpr (KIND == EGNN_OPTIM_ADAMW_AMSGRAD) {
      p = p * k.decay_mul;
    } else {
      if (k.weight_decay != 0.f) {
        const float w = k.weight_decay * p;
        g = g + w;
      }
    }
    float d = g - a;
    d = k.one_minus_beta1 * d;
    a = a + d;
    float t = g * g;
    t = t * k.one_minus_beta2;
    b = b * k.beta2;
    b = b + t;
    if constexpr (KIND == EGNN_OPTIM_ADAMW_AMSGRAD) {
      c = c >= b ? c : b;                   // a NaN in b passes through, as torch.maximum's does
      d = sqrtf(c);
    } else {
      d = sqrtf(b);
    }
    d = d / k.bias_correction2_sqrt;
    d = d + k.eps;
    float q = a / d;
    q = k.step_size * q;
    p = p - q;
  }
}

// which streams a kind reads / writes
template <int KIND> struct Streams {
  static constexpr bool kS0 = KIND != kOptimInterp, kS1 = KIND != kOptimInterp, kS2 = KIND == EGNN_OPTIM_ADAMW_AMSGRAD;
};

// FULL: every quad of the chunk lies inside the tensor (the workgroup-uniform common case: no bounds logic at all)
template <int KIND, bool FULL>
__device__ __forceinline__ void optim_chunk(const egnn_optim_consts& k, float* p, const float* g, float* s0, float* s1,
                                            float* s2, uint32_t base, uint32_t numel) {
  using S = Streams<KIND>;
  float4 vp[kOptimQuads], vg[kOptimQuads], va[kOptimQuads], vb[kOptimQuads], vc[kOptimQuads];
  int cnt[kOptimQuads];
  // all loads of the chunk first (the compiler places the wait at the first use below)
#pragma unroll
  for (int u = 0; u < kOptimQuads; ++u) {
    const uint32_t e = base + (uint32_t)(u * kOptimThreads + threadIdx.x) * 4u;
    cnt[u] = FULL ? 4 : (e >= numel ? 0 : (numel - e >= 4u ? 4 : (int)(numel - e)));
    va[u] = vb[u] = vc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cnt[u] == 4) {
      const f32x4u tp = *reinterpret_cast<const f32x4u*>(p + e), tg = *reinterpret_cast<const f32x4u*>(g + e);
      vp[u] = make_float4(tp.x, tp.y, tp.z, tp.w);
      vg[u] = make_float4(tg.x, tg.y, tg.z, tg.w);
      if constexpr (S::kS0) { const f32x4u t = *reinterpret_cast<const f32x4u*>(s0 + e); va[u] = make_float4(t.x, t.y, t.z, t.w); }
      if constexpr (S::kS1) { const f32x4u t = *reinterpret_cast<const f32x4u*>(s1 + e); vb[u] = make_float4(t.x, t.y, t.z, t.w); }
      if constexpr (S::kS2) { const f32x4u t = *reinterpret_cast<const f32x4u*>(s2 + e); vc[u] = make_float4(t.x, t.y, t.z, t.w); }
    } else if (!FULL) {
      // the tensor's last 1-3 elements (components beyond them compute on zeros and are never stored)
      float* fp = &vp[u].x; float* fg = &vg[u].x; float* fa = &va[u].x; float* fb = &vb[u].x; float* fc = &vc[u].x;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const bool in = j < cnt[u];
        fp[j] = in ? p[e + j] : 0.f;
        fg[j] = in ? g[e + j] : 0.f;
        if constexpr (S::kS0) fa[j] = in ? s0[e + j] : 0.f;
        if constexpr (S::kS1) fb[j] = in ? s1[e + j] : 0.f;
        if constexpr (S::kS2) fc[j] = in ? s2[e + j] : 0.f;
      }
      vp[u].w = 0.f;
      vg[u].w = 0.f;
    }
  }
#pragma unroll
  for (int u = 0; u < kOptimQuads; ++u) {
    optim_elem<KIND>(k, vp[u].x, vg[u].x, va[u].x, vb[u].x, vc[u].x);
    optim_elem<KIND>(k, vp[u].y, vg[u].y, va[u].y, vb[u].y, vc[u].y);
    optim_elem<KIND>(k, vp[u].z, vg[u].z, va[u].z, vb[u].z, vc[u].z);
    optim_elem<KIND>(k, vp[u].w, vg[u].w, va[u].w, vb[u].w, vc[u].w);
  }
#pragma unroll
  for (int u = 0; u < kOptimQuads; ++u) {
    const uint32_t e = base + (uint32_t)(u * kOptimThreads + threadIdx.x) * 4u;
    if (cnt[u] == 4) {
      f32x4u t;
      t.x = vp[u].x; t.y = vp[u].y; t.z = vp[u].z; t.w = vp[u].w;
      *reinterpret_cast<f32x4u*>(p + e) = t;
      if constexpr (S::kS0) { t.x = va[u].x; t.y = va[u].y; t.z = va[u].z; t.w = va[u].w; *reinterpret_cast<f32x4u*>(s0 + e) = t; }
      if constexpr (S::kS1) { t.x = vb[u].x; t.y = vb[u].y; t.z = vb[u].z; t.w = vb[u].w; *reinterpret_cast<f32x4u*>(s1 + e) = t; }
      if constexpr (S::kS2) { t.x = vc[u].x; t.y = vc[u].y; t.z = vc[u].z; t.w = vc[u].w; *reinterpret_cast<f32x4u*>(s2 + e) = t; }
    } else if (!FULL) {
      const float* fp = &vp[u].x; const float* fa = &va[u].x; const float* fb = &vb[u].x; const float* fc = &vc[u].x;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        if (j < cnt[u]) {
          p[e + j] = fp[j];
          if constexpr (S::kS0) s0[e + j] = fa[j];
          if constexpr (S::kS1) s1[e + j] = fb[j];
          if constexpr (S::kS2) s2[e + j] = fc[j];
        }
      }
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(kOptimThreads) void optim_step_kernel(const OptimLaunch L) {
  // the last tensor whose first workgroup is <= this one (chunk0 is non-decreasing, t[0].chunk0 == 0)
  int lo = 0, hi = L.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (L.t[mid].chunk0 <= blockIdx.x) lo = mid; else hi = mid - 1;
  }
  float* p = L.t[lo].p;
  const float* g = L.t[lo].g;
  float* s0 = L.t[lo].s0;
  const uint32_t numel = L.t[lo].numel;
  const uint32_t base = (blockIdx.x - L.t[lo].chunk0) * kOptimChunk;
  float* s1 = reinterpret_cast<float*>(reinterpret_cast<char*>(s0) + L.d1);
  float* s2 = reinterpret_cast<float*>(reinterpret_cast<char*>(s0) + L.d2);
  if (base + kOptimChunk <= numel) optim_chunk<KIND, true>(L.c, p, g, s0, s1, s2, base, numel);
  else optim_chunk<KIND, false>(L.c, p, g, s0, s1, s2, base, numel);
}

template <int KIND>
int launch_optim(const OptimLaunch& L, uint32_t chunks, hipStream_t st) {
  hipLaunchKernelGGL(optim_step_kernel<KIND>, dim3(chunks), dim3(kOptimThreads), 0, st, L);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

int flush(int kind, OptimLaunch& L, uint32_t& chunks, hipStream_t st) {
  if (L.n == 0) return EGNN_OK;
  int rc = EGNN_EINVAL;
  switch (kind) {
    case EGNN_OPTIM_ADAM: rc = launch_optim<EGNN_OPTIM_ADAM>(L, chunks, st); break;
    case EGNN_OPTIM_ADAMW_AMSGRAD: rc = launch_optim<EGNN_OPTIM_ADAMW_AMSGRAD>(L, chunks, st); break;
    case EGNN_OPTIM_RADAM_SF: rc = launch_optim<EGNN_OPTIM_RADAM_SF>(L, chunks, st); break;
    case kOptimInterp: rc = launch_optim<kOptimInterp>(L, chunks, st); break;
  }
  L.n = 0;
  chunks = 0;
  return rc;
}

bool dword_aligned(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3u) == 0; }

// Cuts the list into launches: a launch ends at kOptimCapacity tensors or where the state spacing changes.
int optim_run(hipStream_t st, int kind, int n, float* const* p, const float* const* g, float* const* s0, float* const* s1,
              float* const* s2, const int64_t* numel, const egnn_optim_consts& consts) {
  const bool has_s0 = kind != kOptimInterp, has_s2 = kind == EGNN_OPTIM_ADAMW_AMSGRAD;
  if (n < 0 || (n > 0 && (!p || !g || !numel || (has_s0 && (!s0 || !s1)) || (has_s2 && !s2)))) {
    set_error("optimizer step: null tensor list");
    return EGNN_EINVAL;
  }
  for (int i = 0; i < n; ++i) {   // validate everything before the first launch: a bad list changes nothing
    if (numel[i] < 0 || numel[i] > INT32_MAX) { set_error("optimizer step: tensor %d has %lld elements", i, (long long)numel[i]); return EGNN_EINVAL; }
    if (!g[i] || numel[i] == 0) continue;
    if (!p[i] || (has_s0 && (!s0[i] || !s1[i])) || (has_s2 && !s2[i])) { set_error("optimizer step: tensor %d has a null parameter or state pointer", i); return EGNN_EINVAL; }
    if (!dword_aligned(p[i]) || !dword_aligned(g[i]) || (has_s0 && (!dword_aligned(s0[i]) || !dword_aligned(s1[i]))) ||
        (has_s2 && !dword_aligned(s2[i]))) {
      set_error("optimizer step: tensor %d is not 4-byte aligned", i);
      return EGNN_EINVAL;
    }
  }
  OptimLaunch L;
  L.c = consts;
  L.n = 0;
  L.d1 = L.d2 = 0;
  uint32_t chunks = 0;
  for (int i = 0; i < n; ++i) {
    if (!g[i] || numel[i] == 0) continue;   // p.grad is None
    const int64_t d1 = has_s0 ? reinterpret_cast<const char*>(s1[i]) - reinterpret_cast<const char*>(s0[i]) : 0;
    const int64_t d2 = has_s2 ? reinterpret_cast<const char*>(s2[i]) - reinterpret_cast<const char*>(s0[i]) : 0;
    if (L.n == kOptimCapacity || (L.n > 0 && (d1 != L.d1 || d2 != L.d2))) {
      const int rc = flush(kind, L, chunks, st);
      if (rc) return rc;
    }
    if (L.n == 0) { L.d1 = d1; L.d2 = d2; }
    OptimTensor& t = L.t[L.n++];
    t.p = p[i];
    t.g = g[i];
    t.s0 = has_s0 ? s0[i] : nullptr;
    t.numel = (uint32_t)numel[i];
    t.chunk0 = chunks;
    chunks += (t.numel + kOptimChunk - 1) / kOptimChunk;   // <= 112 * 2^20: no overflow
  }
  return flush(kind, L, chunks, st);
}

}  // namespace
}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_optim_step(void* stream, int kind, int n, float* const* d_p, const float* const* d_g, float* const* d_s0,
                    float* const* d_s1, float* const* d_s2, const int64_t* numel, const egnn_optim_consts* consts) {
  if (kind != EGNN_OPTIM_ADAM && kind != EGNN_OPTIM_ADAMW_AMSGRAD && kind != EGNN_OPTIM_RADAM_SF) {
    set_error("egnn_optim_step: unknown optimizer kind %d", kind);
    return EGNN_EINVAL;
  }
  if (!consts) { set_error("egnn_optim_step: null constants"); return EGNN_EINVAL; }
  return optim_run(reinterpret_cast<hipStream_t>(stream), kind, n, d_p, d_g, d_s0, d_s1, d_s2, numel, *consts);
}

int egnn_optim_interp(void* stream, int n, float* const* d_p, const float* const* d_z, const int64_t* numel, float weight) {
  egnn_optim_consts c;
  memset(&c, 0, sizeof(c));
  c.ckp1 = weight;
  return optim_run(reinterpret_cast<hipStream_t>(stream), kOptimInterp, n, d_p, d_z, nullptr, nullptr, nullptr, numel, c);
}

int egnn_optim_tensors_per_launch(void) { return kOptimCapacity; }

}  // extern "C"

// Packed parameters of libegnn_amd (gfx950): the pack kernels that turn a layer's nn.Linear weights into the streams of
// LayerPack (layer_pack.h), and the entry points that own those streams -- egnn_set_model, egnn_pack_layer, free_layer.
// A layer's streams live in ONE device allocation; which streams exist, their element sizes and counts are stated once, in
// carve_layer_pack (host_logic.cpp).  Every precision's streams are packed eagerly.
#include "common.h"
#include "kernels.h"

namespace egnn {

// ------------------------------------------------------------------------------------------------
// pack kernels
// ------------------------------------------------------------------------------------------------
// B fragments of D = A.B with B[k][n] = W[n][k] (nn.Linear weight [Nout, K], leading dim ldw,
// column offset koff) for v_mfma_f32_32x32x2_f32: lane l holds B[k = 2*ks + (l>>5)][n = 32*nb + (l&31)].
// Four consecutive k-steps are stored together so one 16-byte load per lane feeds 4 MFMAs:
// out[((nb*KS4 + ks4)*64 + lane)*4 + s] = W[32nb + (l&31)][8*ks4 + 2*s + (l>>5)].
__global__ void pack_frags_f32(const float* __restrict__ W, int Nout, int K, int ldw, int NP, int KP,
                               float* __restrict__ out) {
  const int KS4 = KP / 8;
  const size_t total = (size_t)(NP / 32) * KS4 * 64 * 4;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int s = i & 3, lane = (i >> 2) & 63;
    const size_t f = i >> 8;
    const int ks4 = f % KS4, nb = f / KS4;
    const int n = 32 * nb + (lane & 31), k = 8 * ks4 + 2 * s + (lane >> 5);
    out[i] = (n < Nout && k < K) ? W[(size_t)n * ldw + k] : 0.f;
  }
}
// v_mfma_f32_32x32x16_bf16: lane l holds B[k = 16*ks + 8*(l>>5) + j][n = 32*nb + (l&31)], j = 0..7.
// out[((nb*KS + ks)*64 + lane)*8 + j]
// OT = __bf16, or _Float16 for precision fp16 (scale then carries kF16WScale; clamped to the finite fp16 range)
// LO: the remainder v - OT(v) of the same element (split-operand products)
template <typename OT, bool LO = false>
__device__ __forceinline__ OT to_operand(float v) {
  if constexpr (sizeof(OT) == 2 && !__is_same(OT, __bf16)) v = fminf(fmaxf(v, -65504.f), 65504.f);
  if constexpr (LO) return (OT)(v - (float)(OT)v);
  return (OT)v;
}
template <typename OT, bool LO = false>
__global__ void pack_frags_bf16(const float* __restrict__ W, int Nout, int K, int ldw, int NP, int KP,
                                OT* __restrict__ out, float scale) {
  const int KS = KP / 16;
  const size_t total = (size_t)(NP / 32) * KS * 64 * 8;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int j = i & 7, lane = (i >> 3) & 63;
    const size_t f = i >> 9;
    const int ks = f % KS, nb = f / KS;
    const int n = 32 * nb + (lane & 31), k = 16 * ks + 8 * (lane >> 5) + j;
    out[i] = to_operand<OT, LO>((n < Nout && k < K) ? W[(size_t)n * ldw + k] * scale : 0.f);
  }
}
// v_mfma_f32_16x16x32_bf16: lane l holds B[k = 32*ks + 8*(l>>4) + j][n = 16*nb + (l&15)], j = 0..7.
// out[((nb*KS + ks)*64 + lane)*8 + j]
template <typename OT>
__global__ void pack_frags_bf16_n16(const float* __restrict__ W, int Nout, int K, int ldw, int NP, int KP,
                                    OT* __restrict__ out, float scale) {
  const int KS = KP / 32;
  const size_t total = (size_t)(NP / 16) * KS * 64 * 8;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int j = i & 7, lane = (i >> 3) & 63;
    const size_t f = i >> 9;
    const int ks = f % KS, nb = f / KS;
    const int n = 16 * nb + (lane & 15), k = 32 * ks + 8 * (lane >> 4) + j;
    out[i] = to_operand<OT>((n < Nout && k < K) ? W[(size_t)n * ldw + k] * scale : 0.f);
  }
}
// bf16 remainder of the same fragments: out = bf16(v - bf16(v)), v = W * scale (precision bf16x3)
__global__ void pack_frags_bf16_lo(const float* __restrict__ W, int Nout, int K, int ldw, int NP, int KP,
                                   __bf16* __restrict__ out, float scale) {
  const int KS = KP / 16;
  const size_t total = (size_t)(NP / 32) * KS * 64 * 8;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int j = i & 7, lane = (i >> 3) & 63;
    const size_t f = i >> 9;
    const int ks = f % KS, nb = f / KS;
    const int n = 32 * nb + (lane & 31), k = 16 * ks + 8 * (lane >> 5) + j;
    const float v = (n < Nout && k < K) ? W[(size_t)n * ldw + k] * scale : 0.f;
    out[i] = (__bf16)(v - (float)(__bf16)v);
  }
}
// mlp_h.2 as the A operand of out^T = W2h . hidden^T where hidden^T comes straight from an accumulator tile:
// element j of lane half hh in k-step ks is hidden unit 32*(ks/2) + 16*(ks%2) + 8*(j>>2) + 4*hh + (j&3).
template <typename OT, bool LO = false>
__global__ void pack_frags_bf16_accperm(const float* __restrict__ W, int Nout, int K, int ldw, int NP, int KP,
                                        OT* __restrict__ out, float scale) {
  const int KS = KP / 16;
  const size_t total = (size_t)(NP / 32) * KS * 64 * 8;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int j = i & 7, lane = (i >> 3) & 63;
    const size_t f = i >> 9;
    const int ks = f % KS, nb = f / KS;
    const int n = 32 * nb + (lane & 31);
    const int k = 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3);
    out[i] = to_operand<OT, LO>((n < Nout && k < K) ? W[(size_t)n * ldw + k] * scale : 0.f);
  }
}
// the same fragment layout for B[k][n] = W[k][n] (the transposed use of an nn.Linear weight: dgrad g . W)
__global__ void pack_frags_bf16_T(const float* __restrict__ W, int Krows, int Ncols, int ldw, int NP, int KP,
                                  __bf16* __restrict__ out) {
  const int KS = KP / 16;
  const size_t total = (size_t)(NP / 32) * KS * 64 * 8;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int j = i & 7, lane = (i >> 3) & 63;
    const size_t f = i >> 9;
    const int ks = f % KS, nb = f / KS;
    const int n = 32 * nb + (lane & 31), k = 16 * ks + 8 * (lane >> 5) + j;
    out[i] = (__bf16)((n < Ncols && k < Krows) ? W[(size_t)k * ldw + n] : 0.f);
  }
}
__global__ void scale_copy(const float* __restrict__ src, size_t n, float scale, float* __restrict__ dst) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i] * scale;
}
__global__ void pad_copy(const float* __restrict__ src, int n, int stride, float* __restrict__ dst, int nP) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nP; i += gridDim.x * blockDim.x)
    dst[i] = i < n ? src[(size_t)i * stride] : 0.f;
}
// first layers of mlp_x / mlp_m, split per input block and transposed: w1catT[h][col]
__global__ void pack_first(const float* __restrict__ x0_w, const float* __restrict__ x0_b,
                           const float* __restrict__ m0_w, const float* __restrict__ m0_b, int H, int Wx,
                           int Wm, int WxP, int WmP, float* __restrict__ w1catT, float* __restrict__ b1cat) {
  const int TC = 2 * WxP + 2 * WmP, ld = 2 * H + 1;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < TC * (H + 1); i += gridDim.x * blockDim.x) {
    const int col = i % TC, h = i / TC;  // h == H -> bias row
    int k, W, hoff;
    const float *w, *b;
    if (col < WxP) { k = col; W = Wx; hoff = 0; w = x0_w; b = x0_b; }
    else if (col < 2 * WxP) { k = col - WxP; W = Wx; hoff = H; w = x0_w; b = nullptr; }
    else if (col < 2 * WxP + WmP) { k = col - 2 * WxP; W = Wm; hoff = 0; w = m0_w; b = m0_b; }
    else { k = col - 2 * WxP - WmP; W = Wm; hoff = H; w = m0_w; b = nullptr; }
    if (h < H) w1catT[(size_t)h * TC + col] = k < W ? w[(size_t)k * ld + hoff + h] : 0.f;
    else b1cat[col] = (k < W && b) ? b[k] : 0.f;
  }
}
// B fragments of the (pre-scaled) first-layer weights for node_pre_hilo_kernel (egnn_forward.hip): w1catT = LayerPack::w1catT_s
// (rows k < H are read); out = [TC/32 column blocks][3 k-steps][hi|lo][64 lanes][8 bf16].
__global__ void pack_w1_hilo(const float* __restrict__ w1catT, int H, int TC, __bf16* __restrict__ out) {
  const size_t total = (size_t)(TC / 32) * 3 * 64 * 8;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int j = i & 7, lane = (i >> 3) & 63;
    const size_t f = i >> 9;
    const int ks = f % 3, nb = f / 3;
    const int n = 32 * nb + (lane & 31), k = 16 * ks + 8 * (lane >> 5) + j;
    const float v = k < H ? w1catT[(size_t)k * TC + n] : 0.f;
    const __bf16 hi = (__bf16)v;
    const __bf16 lo = (__bf16)(v - (float)hi);
    const size_t base = (f * 2) * 512 + (size_t)lane * 8 + j;
    out[base] = hi;
    out[base + 512] = lo;
  }
}

void free_layer(LayerPack& lp) {
  if (lp.arena) (void)hipFree(lp.arena);
  lp = LayerPack();
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_set_model(egnn_ctx* c, int L, int H, int M, int Wm, int Wx, int Wh) {
  if (!c) return EGNN_EINVAL;
  ModelDims md;
  {
    const int rc = model_dims(L, H, M, Wm, Wx, Wh, &md);   // validation + padded widths (host_logic.cpp)
    if (rc) return rc;
  }
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  for (auto& lp : c->layers) free_layer(lp);
  c->layers.assign(L, LayerPack());
  c->forget_support();
  c->L = L; c->H = H; c->M = M; c->Wm = Wm; c->Wx = Wx; c->Wh = Wh;
  c->WxP = md.WxP; c->WmP = md.WmP; c->MP = md.MP; c->cbx = md.cbx; c->cbm = md.cbm;
  c->WhP = md.WhP; c->HP = md.HP; c->K1P = md.K1P; c->K1Q = md.K1Q; c->TC = md.TC;
  c->cap_nodes = c->cap_tiles = c->cap_graphs = 0;  // MP / TC may have changed
  if (post_smem_bytes(c->K1P, c->WhP) > 160 * 1024 || edge_smem_bytes(64, c->MP) > 160 * 1024) {
    set_error("model does not fit the 160 KiB LDS budget");
    return EGNN_EINVAL;
  }
  return EGNN_OK;
}

int egnn_pack_layer(egnn_ctx* c, void* stream, int l, const float* m0_w, const float* m0_b, const float* m2_w,
                    const float* m2_b, const float* x0_w, const float* x0_b, const float* x2_w,
                    const float* x2_b, const float* x4_w, const float* x4_b, const float* h0_w,
                    const float* h0_b, const float* h2_w, const float* h2_b, const float* a_w,
                    const float* a_b) {
  if (!c || c->L == 0) { set_error("egnn_set_model first"); return EGNN_ESTATE; }
  if (l < 0 || l >= c->L) { set_error("layer %d out of range", l); return EGNN_EINVAL; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  EGNN_HIP(hipSetDevice(c->device));
  LayerPack& lp = c->layers[l];
  c->forget_support();
  const int H = c->H, M = c->M, Wm = c->Wm, Wx = c->Wx, Wh = c->Wh;
  const int WxP = c->WxP, WmP = c->WmP, MP = c->MP, WhP = c->WhP, HP = c->HP, K1P = c->K1P, TC = c->TC;
  int rc;
  if (!lp.arena) {   // one allocation per layer, carved by carve_layer_pack (host_logic.cpp); set only once it exists
    ModelDims md;
    md.WxP = WxP; md.WmP = WmP; md.MP = MP; md.WhP = WhP; md.HP = HP; md.K1P = K1P; md.K1Q = c->K1Q; md.TC = TC;
    md.cbx = c->cbx; md.cbm = c->cbm;
    const size_t bytes = carve_layer_pack(lp, md, H, node_post_split_k(), nullptr);
    char* arena = nullptr;
    if ((rc = dev_alloc(&arena, bytes))) return rc;
    carve_layer_pack(lp, md, H, node_post_split_k(), arena);
    lp.arena = arena; lp.arena_bytes = bytes;
  }
  const dim3 g(256), b(256);
  hipLaunchKernelGGL(pack_first, g, b, 0, st, x0_w, x0_b, m0_w, m0_b, H, Wx, Wm, WxP, WmP, lp.w1catT, lp.b1cat);
  hipLaunchKernelGGL(pad_copy, dim3(8), b, 0, st, x0_w + 2 * H, Wx, 2 * H + 1, lp.wdx, WxP);
  hipLaunchKernelGGL(pad_copy, dim3(8), b, 0, st, m0_w + 2 * H, Wm, 2 * H + 1, lp.wdm, WmP);
  hipLaunchKernelGGL(pack_frags_f32, g, b, 0, st, x2_w, Wx, Wx, Wx, WxP, WxP, lp.w2x_f32);
  hipLaunchKernelGGL(pack_frags_bf16<__bf16>, g, b, 0, st, x2_w, Wx, Wx, Wx, WxP, WxP, reinterpret_cast<__bf16*>(lp.w2x_bf16), 1.0f);
  hipLaunchKernelGGL(pad_copy, dim3(8), b, 0, st, x2_b, Wx, 1, lp.b2x, WxP);
  hipLaunchKernelGGL(pad_copy, dim3(8), b, 0, st, x4_w, Wx, 1, lp.w3x, WxP);
  hipLaunchKernelGGL(pack_frags_f32, g, b, 0, st, m2_w, M, Wm, Wm, MP, WmP, lp.w2m_f32);
  hipLaunchKernelGGL(pack_frags_bf16<__bf16>, g, b, 0, st, m2_w, M, Wm, Wm, MP, WmP, reinterpret_cast<__bf16*>(lp.w2m_bf16), 1.0f);
  hipLaunchKernelGGL(pad_copy, dim3(8), b, 0, st, m2_b, M, 1, lp.b2m, MP);
  hipLaunchKernelGGL(pad_copy, dim3(8), b, 0, st, a_w, M, 1, lp.wa, MP);
  hipLaunchKernelGGL(pad_copy, dim3(1), dim3(64), 0, st, x4_b, 1, 1, lp.scal, 1);
  hipLaunchKernelGGL(pad_copy, dim3(1), dim3(64), 0, st, a_b, 1, 1, lp.scal + 1, 1);
  // mlp_h.0 sees [h | sum_m]; the kernel's K index is [h (H) | sum_m (MP, zero-padded beyond M)]
  hipLaunchKernelGGL(pack_frags_f32, g, b, 0, st, h0_w, Wh, H + M, H + M, WhP, K1P, lp.w1h_f32);
  hipLaunchKernelGGL(pad_copy, dim3(8), b, 0, st, h0_b, Wh, 1, lp.b1h, WhP);
  hipLaunchKernelGGL(pack_frags_f32, g, b, 0, st, h2_w, H, Wh, Wh, HP, WhP, lp.w2h_f32);
  hipLaunchKernelGGL(pad_copy, dim3(8), b, 0, st, h2_b, H, 1, lp.b2h, HP);
  {  // scaled copies for the bf16 fast path (see LayerPack::w1catT_s)
    const float s1 = kNegLog2e, s2 = kNegInvLog2e;
    hipLaunchKernelGGL(scale_copy, g, b, 0, st, lp.w1catT, (size_t)H * TC, s1, lp.w1catT_s);
    hipLaunchKernelGGL(scale_copy, dim3(8), b, 0, st, lp.b1cat, (size_t)TC, s1, lp.b1cat_s);
    hipLaunchKernelGGL(scale_copy, dim3(8), b, 0, st, lp.wdx, (size_t)WxP, s1, lp.wdx_s);
    hipLaunchKernelGGL(scale_copy, dim3(8), b, 0, st, lp.wdm, (size_t)WmP, s1, lp.wdm_s);
    hipLaunchKernelGGL(scale_copy, dim3(8), b, 0, st, lp.b2x, (size_t)WxP, s1, lp.b2x_s);
    hipLaunchKernelGGL(scale_copy, dim3(8), b, 0, st, lp.w3x, (size_t)WxP, s2, lp.w3x_s);
    hipLaunchKernelGGL(scale_copy, dim3(8), b, 0, st, lp.b2m, (size_t)MP, s1, lp.b2m_s);
    hipLaunchKernelGGL(scale_copy, dim3(8), b, 0, st, lp.wa, (size_t)MP, s2, lp.wa_s);
    hipLaunchKernelGGL(pack_frags_bf16<__bf16>, g, b, 0, st, x2_w, Wx, Wx, Wx, WxP, WxP, reinterpret_cast<__bf16*>(lp.w2x_bf16s), s2);
    hipLaunchKernelGGL(pack_frags_bf16<__bf16>, g, b, 0, st, m2_w, M, Wm, Wm, MP, WmP, reinterpret_cast<__bf16*>(lp.w2m_bf16s), s2);
    hipLaunchKernelGGL(pack_frags_bf16_n16<__bf16>, g, b, 0, st, x2_w, Wx, Wx, Wx, WxP, WxP, reinterpret_cast<__bf16*>(lp.w2x_bf16s16), s2);
    hipLaunchKernelGGL(pack_frags_bf16_n16<__bf16>, g, b, 0, st, m2_w, M, Wm, Wm, MP, WmP, reinterpret_cast<__bf16*>(lp.w2m_bf16s16), s2);
    hipLaunchKernelGGL(pack_frags_bf16_n16<_Float16>, g, b, 0, st, m2_w, M, Wm, Wm, MP, WmP, reinterpret_cast<_Float16*>(lp.w2m_f16s16), s2 * kF16WScale);
    // precision fp16: the same streams as fp16 fragments, times 2^8 (kernels.h "MFMA operand type")
    hipLaunchKernelGGL(pack_frags_bf16_n16<_Float16>, g, b, 0, st, x2_w, Wx, Wx, Wx, WxP, WxP, reinterpret_cast<_Float16*>(lp.w2x_f16s16), s2 * kF16WScale);
    hipLaunchKernelGGL(pack_frags_bf16<_Float16>, g, b, 0, st, m2_w, M, Wm, Wm, MP, WmP, reinterpret_cast<_Float16*>(lp.w2m_f16s), s2 * kF16WScale);
    hipLaunchKernelGGL(pack_frags_bf16_accperm<_Float16>, g, b, 0, st, h2_w, H, Wh, Wh, HP, WhP, reinterpret_cast<_Float16*>(lp.w2h_f16p), kF16WScale);
    if (lp.w1h_f16k) {   // split-operand node MLP: heads + remainders, mlp_h.0 with K padded to the ring's two turns
      const int KS = node_post_split_k();
      hipLaunchKernelGGL(pack_frags_bf16<_Float16>, g, b, 0, st, h0_w, Wh, H + M, H + M, WhP, KS, reinterpret_cast<_Float16*>(lp.w1h_f16k), kF16WScale);
      hipLaunchKernelGGL((pack_frags_bf16<_Float16, true>), g, b, 0, st, h0_w, Wh, H + M, H + M, WhP, KS, reinterpret_cast<_Float16*>(lp.w1h_f16k_lo), kF16WScale);
      hipLaunchKernelGGL((pack_frags_bf16_accperm<_Float16, true>), g, b, 0, st, h2_w, H, Wh, Wh, HP, WhP, reinterpret_cast<_Float16*>(lp.w2h_f16p_lo), kF16WScale);
    }
    // precision f16c8 (edge_f16c8w.hip): the same scaled weights as 32-column fp16 fragments (mlp_m.2: w2m_f16s) and as e4m3
    // head / remainder fragments for the block-scaled correction product
    hipLaunchKernelGGL(pack_frags_bf16<_Float16>, g, b, 0, st, x2_w, Wx, Wx, Wx, WxP, WxP, reinterpret_cast<_Float16*>(lp.w2x_f16s), s2 * kF16WScale);
    if ((rc = pack_c8w_stream(x2_w, Wx, Wx, Wx, WxP, WxP, lp.w2x_c8w, s2 * kF16WScale, lp.c8_exp, reinterpret_cast<unsigned*>(lp.c8_exp + 4), st))) return rc;
    if ((rc = pack_c8w_stream(m2_w, M, Wm, Wm, MP, WmP, lp.w2m_c8w, s2 * kF16WScale, lp.c8_exp + 2, reinterpret_cast<unsigned*>(lp.c8_exp + 5), st))) return rc;
    hipLaunchKernelGGL(pack_frags_bf16_lo, g, b, 0, st, x2_w, Wx, Wx, Wx, WxP, WxP, reinterpret_cast<__bf16*>(lp.w2x_bf16s_lo), s2);
    hipLaunchKernelGGL(pack_frags_bf16_lo, g, b, 0, st, m2_w, M, Wm, Wm, MP, WmP, reinterpret_cast<__bf16*>(lp.w2m_bf16s_lo), s2);
    hipLaunchKernelGGL(pack_frags_bf16<__bf16>, g, b, 0, st, h0_w, Wh, H + M, H + M, WhP, c->K1Q, reinterpret_cast<__bf16*>(lp.w1h_bf16), 1.0f);
    hipLaunchKernelGGL(pack_frags_bf16_accperm<__bf16>, g, b, 0, st, h2_w, H, Wh, Wh, HP, WhP, reinterpret_cast<__bf16*>(lp.w2h_bf16p), 1.0f);
    if (H <= 48)   // hi/lo bf16 fragments of the scaled first-layer weights (node_pre_hilo_kernel)
      hipLaunchKernelGGL(pack_w1_hilo, g, b, 0, st, lp.w1catT_s, H, TC, reinterpret_cast<__bf16*>(lp.w1hl_bf16));
    // transposed packs for the backward dgrad: B[k = second-layer output][column = hidden unit]
    hipLaunchKernelGGL(pack_frags_bf16_T, g, b, 0, st, x2_w, Wx, Wx, Wx, WxP, WxP, reinterpret_cast<__bf16*>(lp.w2xT_bf16));
    hipLaunchKernelGGL(pack_frags_bf16_T, g, b, 0, st, m2_w, M, Wm, Wm, WmP, MP, reinterpret_cast<__bf16*>(lp.w2mT_bf16));
  }
  EGNN_HIP(hipGetLastError());
  lp.packed = true;
  return EGNN_OK;
}

}  // extern "C"

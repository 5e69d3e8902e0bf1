// Packed parameters of one EGCL layer: the streams every forward precision, the training forward and the fused backward read.
// HIP-free (pointers and plain ints only): host_logic.cpp carves them out of the layer's one device allocation, and the
// stand-alone layout test (tests/host/layer_pack_main.cpp) runs the same function on host memory.
#pragma once
#include <stddef.h>

namespace egnn {

struct ModelDims;

// All device memory, owned by the context: `arena` is the one allocation (pack.hip: egnn_pack_layer / free_layer), every other
// pointer is a stream inside it.  carve_layer_pack (host_logic.cpp) states each stream's element size and count, once.
struct LayerPack {
  bool packed = false;
  char* arena = nullptr;
  size_t arena_bytes = 0;
  float* w1catT = nullptr;   // [H][TC]  transposed first-layer weights, columns = {Px|Qx|Pm|Qm}
  float* b1cat = nullptr;    // [TC]     first-layer bias (P columns only)
  float* wdx = nullptr;      // [WxP]    d^2 column of mlp_x.0
  float* wdm = nullptr;      // [WmP]    d^2 column of mlp_m.0
  float* w2x_f32 = nullptr;  // mlp_x.2 as f32 MFMA B fragments  [NB][KS4][64][4]
  void* w2x_bf16 = nullptr;  // mlp_x.2 as bf16 MFMA B fragments [NB][KS][64][8]
  float* b2x = nullptr;      // [WxP]
  float* w3x = nullptr;      // [WxP]    mlp_x.4 weight
  float* w2m_f32 = nullptr;  // mlp_m.2 fragments, N = MP, K = WmP
  void* w2m_bf16 = nullptr;
  float* b2m = nullptr;      // [MP]
  float* wa = nullptr;       // [MP]     attention.0 weight
  float* scal = nullptr;     // [4]      {mlp_x.4 bias, attention.0 bias}
  float* w1h_f32 = nullptr;  // mlp_h.0 fragments, N = WhP, K = K1P (= pad8(H+MP))
  float* b1h = nullptr;      // [WhP]
  float* w2h_f32 = nullptr;  // mlp_h.2 fragments, N = HP, K = WhP
  float* b2h = nullptr;      // [HP]
  // bf16 fast path: SiLU is evaluated as t * rcp(1 + exp2(t)) on t = -log2(e) * z.  The first-layer table,
  // biases and d^2 columns are pre-multiplied by -log2(e) and the following weights by -1/log2(e), which
  // removes one multiply per SiLU.  The scaled copies of the vectors above (same shapes):
  float *w1catT_s = nullptr, *b1cat_s = nullptr, *wdx_s = nullptr, *wdm_s = nullptr, *b2x_s = nullptr, *w3x_s = nullptr,
        *b2m_s = nullptr, *wa_s = nullptr;
  void* w2x_bf16s = nullptr;
  void* w2m_bf16s = nullptr;
  void* w2x_bf16s_lo = nullptr;   // bf16 remainders of the scaled second-layer weights (precision bf16x3)
  void* w2m_bf16s_lo = nullptr;
  void* w2x_bf16s16 = nullptr;  // mlp_x.2 scaled, as v_mfma_f32_16x16x32_bf16 B fragments [N/16][K/32][64][8]
  void* w2m_bf16s16 = nullptr;  // mlp_m.2 scaled, same 16-column layout (edge_small.hip)
  void* w2xT_bf16 = nullptr;  // mlp_x.2 TRANSPOSED bf16 fragments for the backward dgrad (k = output n, column = hidden k)
  void* w2mT_bf16 = nullptr;  // mlp_m.2 transposed (K = MP, N = WmP)
  void* w1hl_bf16 = nullptr;  // scaled first layers as bf16 hi/lo B fragments [TC/32][3][hi|lo][64][8] (node_pre_hilo_kernel)
  void* w1h_bf16 = nullptr;   // mlp_h.0 bf16 fragments (N = WhP, K = K1Q)
  void* w2h_bf16p = nullptr;  // mlp_h.2 bf16 fragments, k in accumulator-row order
  // precision fp16: the streams of the bf16 path as fp16 fragments, every one multiplied by kF16WScale = 2^8 (kernels.h)
  void* w2x_f16s16 = nullptr;  // mlp_x.2 scaled, v_mfma_f32_16x16x32_f16 B fragments
  void* w2m_f16s = nullptr;    // mlp_m.2 scaled, v_mfma_f32_32x32x16_f16 B fragments
  void* w2m_f16s16 = nullptr;  // mlp_m.2 scaled, v_mfma_f32_16x16x32_f16 B fragments (edge_small.hip)
  void* w2h_f16p = nullptr;    // mlp_h.2, k in accumulator-row order
  // split-operand node MLP (node_post_bf16_kernel<., f16x8, true>): mlp_h.0 head / remainder with K padded to its ring's two
  // turns, mlp_h.2 remainder (its head is w2h_f16p); null when the shape is outside that kernel
  void *w1h_f16k = nullptr, *w1h_f16k_lo = nullptr, *w2h_f16p_lo = nullptr;
  // precision f16c8 (edge_f16c8w.hip): mlp_x.2 as v_mfma_f32_32x32x16_f16 B fragments (mlp_m.2: w2m_f16s above), e4m3 fragments
  // [N/32][K/32][2][64][16 B] of the heads and remainders of the fp16 streams, and the e8m0 bytes of their block scales
  // {x: hi, lo, m: hi, lo} (+ [4..5]: the packs' max |w| scratch words)
  void *w2x_f16s = nullptr, *w2x_c8w = nullptr, *w2m_c8w = nullptr;
  int* c8_exp = nullptr;
};

constexpr size_t kPackAlign = 4096;   // every stream starts on a multiple of this (hipMalloc's own granularity)

// Points every stream of `lp` into the arena at `base` and returns the arena's size in bytes.  base == nullptr: measures only
// and leaves every stream null.  split_k = K of the split-operand node MLP (node_bf16.hip: node_post_split_k()); its three
// streams exist only for HP <= 64 && split_k / 2 < H + MP <= split_k.  Touches neither lp.packed nor lp.arena / arena_bytes.
size_t carve_layer_pack(LayerPack& lp, const ModelDims& md, int H, int split_k, char* base);

}  // namespace egnn

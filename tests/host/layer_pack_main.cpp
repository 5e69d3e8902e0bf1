// Stand-alone layout test of carve_layer_pack (csrc/host_logic.cpp), built with -fsanitize=address,undefined by
// tests/test_layer_pack_host.py.  For each shape: the measuring call leaves every stream null, the carving call returns the
// same total, every stream is 4 KiB-aligned, inside the block and disjoint from every other, the split-operand node MLP's
// streams exist exactly under their shape rule -- and every byte of every stream is written, so that ASan reports a stream
// carved smaller than the extent its pack kernel writes.  The extents below are restated from the pack kernels (pack.hip,
// edge_f16c8w.hip: pack_frags_c8w), not taken from carve_layer_pack.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../diffusion_model_amd/csrc/host_logic.h"
#include "../../diffusion_model_amd/csrc/layer_pack.h"

using namespace egnn;

namespace {

constexpr int kSplitK = 320;   // node_bf16.hip: K of the split-operand node MLP

struct Stream { const char* name; void* p; size_t bytes; bool conditional; };

#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                              \
      fprintf(stderr, "\n");                                     \
      exit(1);                                                   \
    }                                                            \
  } while (0)

std::vector<Stream> streams(const LayerPack& lp, const ModelDims& d, int H) {
  const size_t TC = d.TC, WxP = d.WxP, WmP = d.WmP, MP = d.MP, WhP = d.WhP, HP = d.HP, K1P = d.K1P, K1Q = d.K1Q;
  const size_t f = 4, h = 2;   // bytes per fp32 / per bf16, fp16 element
  // fragment packs write NP x KP elements: pack_frags_f32 (NP/32)(KP/8) x 256, pack_frags_bf16* (NP/32)(KP/16) x 512,
  // pack_frags_bf16_n16 (NP/16)(KP/32) x 512; pack_frags_c8w NP x KP byte PAIRS; pack_w1_hilo (TC/32) x 3 x (512 hi + 512 lo)
  return {
      {"w1catT", lp.w1catT, H * TC * f, false},      {"b1cat", lp.b1cat, TC * f, false},
      {"wdx", lp.wdx, WxP * f, false},               {"wdm", lp.wdm, WmP * f, false},
      {"w2x_f32", lp.w2x_f32, WxP * WxP * f, false}, {"w2x_bf16", lp.w2x_bf16, WxP * WxP * h, false},
      {"b2x", lp.b2x, WxP * f, false},               {"w3x", lp.w3x, WxP * f, false},
      {"w2m_f32", lp.w2m_f32, MP * WmP * f, false},  {"w2m_bf16", lp.w2m_bf16, MP * WmP * h, false},
      {"b2m", lp.b2m, MP * f, false},                {"wa", lp.wa, MP * f, false},
      {"scal", lp.scal, 4 * f, false},
      {"w1h_f32", lp.w1h_f32, WhP * K1P * f, false}, {"b1h", lp.b1h, WhP * f, false},
      {"w2h_f32", lp.w2h_f32, HP * WhP * f, false},  {"b2h", lp.b2h, HP * f, false},
      {"w1catT_s", lp.w1catT_s, H * TC * f, false},  {"b1cat_s", lp.b1cat_s, TC * f, false},
      {"wdx_s", lp.wdx_s, WxP * f, false},           {"wdm_s", lp.wdm_s, WmP * f, false},
      {"b2x_s", lp.b2x_s, WxP * f, false},           {"w3x_s", lp.w3x_s, WxP * f, false},
      {"b2m_s", lp.b2m_s, MP * f, false},            {"wa_s", lp.wa_s, MP * f, false},
      {"w2x_bf16s", lp.w2x_bf16s, WxP * WxP * h, false},       {"w2m_bf16s", lp.w2m_bf16s, MP * WmP * h, false},
      {"w2x_bf16s_lo", lp.w2x_bf16s_lo, WxP * WxP * h, false}, {"w2m_bf16s_lo", lp.w2m_bf16s_lo, MP * WmP * h, false},
      {"w2x_bf16s16", lp.w2x_bf16s16, WxP * WxP * h, false},   {"w2m_bf16s16", lp.w2m_bf16s16, MP * WmP * h, false},
      {"w2xT_bf16", lp.w2xT_bf16, WxP * WxP * h, false},       {"w2mT_bf16", lp.w2mT_bf16, WmP * MP * h, false},
      {"w1hl_bf16", lp.w1hl_bf16, (TC / 32) * 3 * 1024 * h, false},
      {"w1h_bf16", lp.w1h_bf16, WhP * K1Q * h, false},         {"w2h_bf16p", lp.w2h_bf16p, HP * WhP * h, false},
      {"w2x_f16s16", lp.w2x_f16s16, WxP * WxP * h, false},     {"w2m_f16s", lp.w2m_f16s, MP * WmP * h, false},
      {"w2m_f16s16", lp.w2m_f16s16, MP * WmP * h, false},      {"w2h_f16p", lp.w2h_f16p, HP * WhP * h, false},
      {"w1h_f16k", lp.w1h_f16k, WhP * kSplitK * h, true},      {"w1h_f16k_lo", lp.w1h_f16k_lo, WhP * kSplitK * h, true},
      {"w2h_f16p_lo", lp.w2h_f16p_lo, HP * WhP * h, true},
      {"w2x_f16s", lp.w2x_f16s, WxP * WxP * h, false},
      {"w2x_c8w", lp.w2x_c8w, WxP * WxP * 2, false},           {"w2m_c8w", lp.w2m_c8w, MP * WmP * 2, false},
      {"c8_exp", lp.c8_exp, 8 * sizeof(int), false},
  };
}

void run_shape(int L, int H, int M, int Wm, int Wx, int Wh, bool expect_split) {
  ModelDims d;
  CHECK(model_dims(L, H, M, Wm, Wx, Wh, &d) == EGNN_OK, "model_dims");
  const bool split = d.HP <= 64 && H + d.MP > kSplitK / 2 && H + d.MP <= kSplitK;
  CHECK(split == expect_split, "shape (%d,%d,%d,%d,%d,%d): split rule %d", L, H, M, Wm, Wx, Wh, (int)split);

  LayerPack lp;
  const size_t total = carve_layer_pack(lp, d, H, kSplitK, nullptr);
  CHECK(total > 0 && total % kPackAlign == 0, "total %zu", total);
  for (const Stream& s : streams(lp, d, H)) CHECK(s.p == nullptr, "%s set by the measuring call", s.name);
  CHECK(lp.arena == nullptr && lp.arena_bytes == 0 && !lp.packed, "measuring call touched the owner fields");

  char* block = static_cast<char*>(aligned_alloc(kPackAlign, total));
  CHECK(block != nullptr, "aligned_alloc(%zu)", total);
  CHECK(carve_layer_pack(lp, d, H, kSplitK, block) == total, "carving call returned another total");
  const std::vector<Stream> ss = streams(lp, d, H);
  CHECK(ss.size() == 47, "stream table has %zu entries", ss.size());
  for (const Stream& s : ss) {
    if (s.conditional) CHECK((s.p != nullptr) == split, "%s: null exactly outside the split-operand rule", s.name);
    else CHECK(s.p != nullptr, "%s is null", s.name);
    if (!s.p) continue;
    const char* a = static_cast<const char*>(s.p);
    CHECK((uintptr_t)a % kPackAlign == 0, "%s not 4 KiB-aligned", s.name);
    CHECK(s.bytes > 0 && a >= block && a + s.bytes <= block + total, "%s outside the block", s.name);
    for (const Stream& t : ss) {
      if (&t == &s || !t.p) continue;
      const char* b = static_cast<const char*>(t.p);
      CHECK(a + s.bytes <= b || b + t.bytes <= a, "%s overlaps %s", s.name, t.name);
    }
  }
  for (const Stream& s : ss)
    if (s.p) memset(s.p, 0xA5, s.bytes);   // ASan: heap-buffer-overflow if a stream ends past the block
  free(block);
  printf("shape (%d,%d,%d,%d,%d,%d): %zu bytes, split streams %s\n", L, H, M, Wm, Wx, Wh, total, split ? "present" : "null");
}

}  // namespace

int main() {
  run_shape(4, 36, 256, 1024, 1024, 1024, true);   // the reference shape
  run_shape(2, 3, 5, 7, 300, 130, true);           // every width padded
  run_shape(1, 70, 16, 64, 64, 64, false);         // HP = 96 > 64: outside the split-operand node MLP
  printf("LAYER-PACK-OK\n");
  return 0;
}

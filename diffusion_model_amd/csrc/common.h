// Shared declarations of libegnn_amd (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../include/egnn_amd.h"
#include "layer_pack.h"   // LayerPack: the packed parameters of one EGCL layer and the function that carves them
#include "host_logic.h"   // set_error, padded model dimensions, argument checks, GEMM plan: the HIP-free part of the host side

namespace egnn {

constexpr int kThreads = 256;   // 4 wave64 per workgroup, one per SIMD
constexpr int kWaves = 4;

#define EGNN_HIP(call)                                                                      \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) {                                                                 \
      egnn::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      return EGNN_EHIP;                                                                     \
    }                                                                                       \
  } while (0)

// (Re)allocates *p as `count` elements of device memory; *p is null after a failure.
template <typename T>
inline int dev_alloc(T** p, size_t count) {
  if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (count == 0) return EGNN_OK;
  if (hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T)) != hipSuccess) {
    set_error("hipMalloc of %zu bytes failed", count * sizeof(T));
    *p = nullptr;
    return EGNN_ENOMEM;
  }
  // EGNN_DEBUG_POISON=1 (tests): every scratch / pack buffer starts as 0xFF bytes -- NaN as fp32, fp16 and bf16, -1 as an index --
  // so that an element a kernel reads before any kernel wrote it cannot pass for a plausible value (hipMalloc hands out zeros
  // in a fresh process and whatever the previous owner left afterwards: tests/test_gpu_parity.py::test_no_scratch_read_before_write)
  const char* poison = getenv("EGNN_DEBUG_POISON");
  if (poison && poison[0] == '1' && hipMemset(*p, 0xFF, count * sizeof(T)) != hipSuccess) {
    set_error("hipMemset (EGNN_DEBUG_POISON) failed");
    (void)hipFree(*p); *p = nullptr;
    return EGNN_EHIP;
  }
  return EGNN_OK;
}

// egcl_forward_save: where a layer's edge kernels leave what the backward needs
struct SaveBuffers {
  void *s1x, *s1m, *t2x, *t2m;
  float* s;   // [nsplit][E] column-split shares of s_e
};

struct CachedSupport { bool known = false; KernelSupport sup; };   // egnn_ctx::support

constexpr int kGraphSteps = 8;   // reverse steps captured per hipGraph
struct Sampler {
  bool ready = false;
  int T = 0, A = 0, t = 0;
  int x_only = 0;                  // 1: positions diffuse, atom types fixed (test.py:253-279)
  float onehot_scale = 1.f;
  uint64_t seed = 0;
  const float* d_table = nullptr;  // [(T+1)*4] caller-owned
  float* pos = nullptr;            // [N][3]
  float* h = nullptr;              // [N][H]
  float* h_out = nullptr;          // [N][H]
  float* x_out = nullptr;          // [N][3]
  float* cond = nullptr;           // [N][H-A-1] constant conditioning block
  int* t_dev = nullptr;            // current t on device (graph replay reads it)
  int* bad = nullptr;              // [B] sticky non-finite flags
  hipGraph_t graph[2] = {nullptr, nullptr};            // [0]: one reverse step, [1]: kGraphSteps steps
  hipGraphExec_t graph_exec[2] = {nullptr, nullptr};
  int graph_prec = -1, graph_norm = -1;
};

}  // namespace egnn

struct egnn_ctx {
  int device = 0;
  // model
  int L = 0, H = 0, M = 0, Wm = 0, Wx = 0, Wh = 0;
  int WxP = 0, WmP = 0, MP = 0, WhP = 0, HP = 0, K1P = 0, K1Q = 0, TC = 0;
  int cbx = 0, cbm = 0;  // 32-column blocks per wave for the x / m second-layer GEMMs
  std::vector<egnn::LayerPack> layers;
  // graph
  int N = 0, E = 0, B = 0;
  const int32_t *edge_dst = nullptr, *edge_src = nullptr, *row_ptr = nullptr, *graph_ptr = nullptr,
                *node_graph = nullptr;
  // scratch (grown on demand by reserve())
  size_t cap_nodes = 0, cap_tiles = 0, cap_graphs = 0;
  float* table = nullptr;    // [N][TC] first-layer partial pre-activations
  float* agg_m = nullptr;    // [N][MP]
  float* agg_x = nullptr;    // [N][4]
  float* part_m = nullptr;   // [tiles][2][MP]
  float* part_x = nullptr;   // [tiles][2][4]
  float* node_d2 = nullptr;  // [N]
  float* gscale = nullptr;   // [B] sum of d^2 per graph (G^2); node_post applies 1/(G+1)
  egnn::ForwardPlan plan;               // how the last launch_layer_begin ran (host_logic.h: plan_forward); launch_layer_end reads it
  int ncu = 256;                        // compute units of the device (egnn_create)
  // answers of the kernels' *_supported predicates per (layer, precision): they depend on the model, the packed streams and N
  // only, so they are asked once and forgotten by egnn_set_model / egnn_pack_layer / egnn_set_graph (forget_support)
  std::vector<egnn::CachedSupport> support;
  void forget_support() { support.clear(); }
  bool small_ok = false;                // the partial slots were sized for 32-edge tiles (E <= 65536): edge_small.hip may run
  // A layer's hidden-split node_post leaves its 8 partial h' in h_partial; inside a multi-layer call the NEXT layer's node_pre
  // adds them up (and writes h') instead of a launch of its own (small graphs: every launch is a serial link of the step)
  struct { bool active = false; int hs = 0; const float* b2h = nullptr; float* h_out = nullptr; } pend;
  float* h_partial = nullptr;  // [8][N][H] partial node-MLP outputs (hidden-split node_post at small N)
  float* bwd_s = nullptr;    // [nsplit][chunk edges] column-split shares of s_e (backward recompute)
  size_t cap_bwd_s = 0;
  unsigned long long* stamps = nullptr;  // [2 kernels][8 waves][32 chunks][4] diagnostic time stamps
  float* h_tmp[2] = {nullptr, nullptr};  // [N][H] ping-pong between layers
  float* x_tmp[2] = {nullptr, nullptr};  // [N][3]
  egnn::Sampler smp;
  hipStream_t side = nullptr;                       // small graphs: the message edge kernel runs beside the coordinate kernel
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // profiling
  bool prof = false;
  std::vector<hipEvent_t> ev;  // pairs
  std::vector<int> ev_kind;    // 0 = edge kernel, 1 = node kernels
  size_t ev_used = 0;
};

namespace egnn {
int reserve(egnn_ctx* c);
// save: a training forward's buffers, null = plain forward
int launch_layer(egnn_ctx* c, hipStream_t st, int layer, int prec, int norm_scope, const float* h, const float* x, float* h_out,
                 float* x_out, bool need_gscale = false, bool defer_finish = false, const SaveBuffers* save = nullptr);
// all L layers from (h, x) to (h_out, x_out), ping-ponging through c->h_tmp / c->x_tmp
int launch_stack(egnn_ctx* c, hipStream_t st, int prec, int norm_scope, const float* h, const float* x, float* h_out, float* x_out);
void free_layer(LayerPack& lp);   // pack.hip
// backward recompute on the forward's bf16 edge kernels (egcl_backward_edge_recompute)
int backward_recompute_supported(egnn_ctx* c);
int backward_table(egnn_ctx* c, hipStream_t st, int layer, const float* h);
int backward_recompute(egnn_ctx* c, hipStream_t st, int layer, const float* x, const float* g_sum_x, const float* g_sum_m,
                       int e_first, int n_edges, void* s1x, void* s1m, void* g_a2x, void* g_a2m, float* s_halves,
                       float* g_b2x, float* g_w3, float* g_b3, float* g_b2m, float* g_wa, float* g_ba);
int backward_dgrad(egnn_ctx* c, hipStream_t st, int layer, const float* x, int e_first, int n_edges, const void* g_a2x,
                   const void* g_a2m, void* g_a1x, void* g_a1m);
int backward_heads_saved(egnn_ctx* c, hipStream_t st, int layer, const float* x, const float* g_sum_x, const float* g_sum_m,
                         int e_first, int n_edges, void* t2x, void* t2m, float* g_b2x, float* g_w3, float* g_b3, float* g_b2m,
                         float* g_wa, float* g_ba);
bool heads_saved_supported(int WxP, int MP);
int launch_heads_saved(int n_edges, const int* dst, const int* src, const float* x, const float* g_sum_x, const float* g_sum_m,
                       int WxP, int MP, const float* w3s, const float* was, const float* scal, void* t2x, void* t2m,
                       float* g_b2x, float* g_w3, float* g_b3, float* g_b2m, float* g_wa, float* g_ba, hipStream_t st);
int init_edge_dgrad_attributes();
int fork_streams(egnn_ctx* c);
int launch_edge_dgrad(int N, int E, const int* dst, const int* src, const float* x, const void* table, int TC, int offP, int offQ,
                      const float* wd, const void* g_a2, int Kd, const void* w2t, int KP, void* g_a1_out, hipStream_t st);
}  // namespace egnn

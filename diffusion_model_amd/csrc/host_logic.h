// Host-only logic of libegnn_amd: everything that decides, validates or tabulates WITHOUT touching the HIP runtime.
// Kept in one plain C++ translation unit (host_logic.cpp) so that it also builds with g++ -fsanitize=address,undefined into
// a CPU-only library the build container's tests run (make asan -> build/libegnn_host_asan.so; tests/test_host_asan.py):
// the schedule builder, argument / shape validation of every entry point that has any, the padded model dimensions,
// the split-K plan of the weight-gradient GEMM and the forward dispatch (plan_forward).  No hip header is included here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/egnn_amd.h"

namespace egnn {

void set_error(const char* fmt, ...);

// Padded dimensions of one model (egnn_set_model): zero-padded widths contribute SiLU(0) * 0 = 0.
struct ModelDims {
  int WxP, WmP, MP, WhP, HP, K1P, K1Q, TC, cbx, cbm;
};
constexpr int kMaxCB = 8;       // 32-column blocks per wave in the fused edge GEMMs (N <= 1024)
constexpr int kPostMaxOB = 8;   // output column blocks of node_post (H <= 256)
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
// EGNN_OK and *out filled, or EGNN_EINVAL with the error text set
int model_dims(int L, int H, int M, int Wm, int Wx, int Wh, ModelDims* out);

int graph_args_check(bool have_model, int N, int E, int B, const void* edge_dst, const void* edge_src, const void* row_ptr,
                     const void* graph_ptr, const void* node_graph);
int precision_scope_check(bool ready, int prec, int norm_scope);

// split-K plan of egnn_gemm_tn_bf16 (gemm_tn.hip): column tile BN, tiles along N, number of slices S, k-steps per slice
constexpr int kGemmBM = 256, kGemmBK = 32;
void plan_gemm_tn(int E, int M, int N, int& BN, int& tiles_n, int& S, int& steps_per_slice);
int gemm_tn_args_check(int E, int M, int N, const void* A, int lda, const void* B, int ldb, const void* C, int ldc, int rows,
                       int cols, const void* workspace, size_t workspace_bytes);
int gemm_rows_args_check(int E, const void* A0, int lda0, int K0, const void* W0, const void* A1, int lda1, int K1, const void* W1,
                         const void* out, int ldo);
// the output side of egnn_gemm_rows_bf16: n_chunks column chunks inside ldo; a bf16 output is stored in 16-byte pieces, so its
// base must be 16-byte aligned and its row stride a multiple of 8 (an fp32 output is stored element by element: ldo % 4)
int gemm_rows_out_check(const void* out, int ldo, int out_f32, int n_chunks);
int dense_rows_args_check(int N, int K, int J, const void* in, const void* W, const void* b, const void* out);

// the message edge kernel goes to the caller's side stream when the coordinate kernel's last round of workgroups leaves
// enough CUs idle for all message workgroups (two per CU); a detail of plan_forward
bool fork_candidate(int E, int WxP);

// ---- forward dispatch ------------------------------------------------------------------------------------------------
// plan_forward is the ONE place that decides how a layer's forward runs; launch_layer_begin / launch_layer_end
// (egnn_forward.hip) launch what the plan says and decide nothing.  Everything it reads is a value: the shape, what the call
// asks for, the CU count, the environment switches and the answers of the kernels' *_supported predicates (which stay in
// their translation units, next to the LDS constants they depend on).  tests/host/forward_plan_main.cpp pins it on the CPU.
//
// Edge path of a precision, taken when its kernels take the shape (else the generic kernel: bf16 keeps bf16 fragments, every
// other precision becomes the exact fp32 path; EGNN_EDGE=1 forces the generic kernel):
//   bf16    edge_x_m16.hip (hidden width 512 / 1024) or edge_bf16_v3.hip (256) + edge_bf16_v4.hip, fp16 table
//   bf16x3  edge_bf16x3.hip (head / remainder operands, fp32 table)
//   fp16    the bf16 path's kernels on fp16 operands (hidden width 512 / 1024), fp16 table
//   f16c8   edge_f16c8w.hip (fp16 heads + e4m3 corrections, fp32 table)
// Small graphs on a half-precision table run 32- / 64-edge tiles (edge_small.hip; limits: EGNN_SMALL_EDGES /
// EGNN_SMALL64_EDGES), everything else 128-edge tiles; the generic kernel has 64-edge tiles.
enum class EdgePath { kGeneric, kBf16, kBf16x3, kF16, kF16c8 };
enum class NodePre { kHilo8, kHilo2, kMfma, kValu };   // node_pre_hilo_kernel<8> / <2>, node_pre_mfma_kernel, node_pre_kernel
enum class EdgeForm { kNone, kGeneric64, kSmall, kBf16x3, kF16c8, kTile128 };   // kNone: E == 0, no edge launch
enum class CoordKernel { kOwn, kV3, kXm16, kXm16Persistent };   // kTile128's coordinate kernel; kOwn: the form has one kernel of its own
// per-graph (per-call) sums of d^2 in gscale: node_d2 + graph_sum before the edge pass (generic kernel), a memset (tiled, E == 0),
// a graph_sq_sums launch after the edge pass, or none because node_post adds them up itself
enum class SqSource { kNodeD2, kMemset, kLaunch, kNodePost };
enum class NodePost { kSplit, kBf16, kF32 };   // split-operand fp16 (node_bf16.hip), bf16 (node_bf16.hip), exact fp32
constexpr int kGenericRows = 64, kTileRows = 128;   // edges per tile (static_asserts tie them to the kernels' own constants)
constexpr int kHiloNodes = 32;                      // nodes per workgroup of node_pre_hilo_kernel

struct ForwardSwitches {   // environment switches of the forward dispatch (read in one place: forward_switches(), egnn_forward.hip)
  int edge = 4;                                  // EGNN_EDGE: < 4 forces the generic kernel
  long small_edges = 2048, small64_edges = 6144; // EGNN_SMALL_EDGES / EGNN_SMALL64_EDGES: edge-count limits of the 32- / 64-row tiles
  bool x_persist = true;                         // EGNN_X_PERSIST=0: never the persistent coordinate kernel
};
struct KernelSupport {   // answers of the *_supported predicates on the params the layer would be launched with
  bool v3 = false, v4 = false, x_m16 = false, small = false, bf16x3 = false, f16c8w = false, post_split = false, post_bf16 = false;
};
struct ForwardAsk {
  int N = 0, E = 0, B = 0, H = 0;
  ModelDims md = {};
  bool small_ok = false;       // the partial slots were sized for 32-edge tiles
  int prec = EGNN_PREC_F32, norm_scope = EGNN_NORM_CALL;
  bool save = false;           // training forward (egcl_forward_save)
  bool need_gscale = false;    // the caller reads the d^2 sums (single-layer entry points)
  bool side_ok = false;        // a side stream with fork / join events is there
  bool prof = false;           // event profiling on: one stream
  int ncu = 256;
  ForwardSwitches sw;
  KernelSupport sup;
};
struct ForwardPlan {
  EdgePath path = EdgePath::kGeneric;
  bool frag_bf16 = false;      // generic kernel: bf16 fragments (else fp32)
  bool half_table = false;     // fp16 first-layer table (else fp32)
  NodePre node_pre = NodePre::kValu;
  bool absorbs_finish = false; // this node_pre can add up a pending hidden-split finish of the previous layer
  EdgeForm form = EdgeForm::kNone;
  bool f16 = false;            // operand type of kSmall / kTile128: fp16 (else bf16)
  CoordKernel coord = CoordKernel::kOwn;
  int persist_grid = 0;        // workgroups of kXm16Persistent
  bool save = false;
  int R = kGenericRows, nsplit_x = 1;   // edges per tile and column-split copies of the coordinate sums, as node_post reads them
  bool fork = false;           // message kernel on the side stream
  SqSource sq = SqSource::kNodeD2;
  NodePost node_post = NodePost::kF32;
};
// whether a shape can reach the persistent coordinate kernel at all: more than two 512-column units per CU.  The launcher reads
// EGNN_X_PERSIST only then (measured: one getenv per layer is 0.7 us of the eager reverse step of a single 64-atom graph)
inline bool persistent_possible(int E, int WxP, int ncu) { return ((long)E + kTileRows - 1) / kTileRows * (WxP / 512) > 2L * ncu; }
EdgePath path_of_precision(int prec);
NodePre node_pre_form(bool half_table, int N, int H, int TC);
// EGNN_OK and *out filled, or EGNN_EINVAL with the error text set (a training forward off the 128-edge-tile bf16 kernels)
int plan_forward(const ForwardAsk& a, ForwardPlan* out);

}  // namespace egnn

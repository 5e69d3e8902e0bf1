// Host-only logic of libegnn_amd (see host_logic.h).  Plain C++: no HIP call, no device code.
#include "host_logic.h"
#include "layer_pack.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

namespace egnn {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static int pow2_ceil(int v) { int p = 1; while (p < v) p <<= 1; return p; }

int model_dims(int L, int H, int M, int Wm, int Wx, int Wh, ModelDims* out) {
  if (!out || L < 1 || H < 1 || M < 1 || Wm < 1 || Wx < 1 || Wh < 1) { set_error("bad model dims"); return EGNN_EINVAL; }
  if (Wx > 128 * kMaxCB || Wm > 128 * kMaxCB || M > 128 * kMaxCB || H > 32 * kPostMaxOB) {
    set_error("unsupported width: hidden/message widths must be <= %d and H <= %d", 128 * kMaxCB, 32 * kPostMaxOB);
    return EGNN_EINVAL;
  }
  // widths are padded to 256 * 2^k: 8 waves x 32-column blocks in the bf16 kernel, 4 waves x 64 in the fp32 one
  out->WxP = 256 * pow2_ceil((Wx + 255) / 256);   // K and N of mlp_x.2
  out->WmP = 256 * pow2_ceil((Wm + 255) / 256);   // K of mlp_m.2
  out->MP = 256 * pow2_ceil((M + 255) / 256);     // N of mlp_m.2
  out->cbx = out->WxP / 128;
  out->cbm = out->MP / 128;
  out->WhP = round_up(Wh, 128);
  out->HP = round_up(H, 32);
  out->K1P = round_up(H + out->MP, 8);
  out->K1Q = round_up(H + out->MP, 16);
  out->TC = 2 * out->WxP + 2 * out->WmP;
  return EGNN_OK;
}

int graph_args_check(bool have_model, int N, int E, int B, const void* edge_dst, const void* edge_src, const void* row_ptr,
                     const void* graph_ptr, const void* node_graph) {
  if (N < 1 || E < 0 || B < 1 || !row_ptr || !graph_ptr || !node_graph || (E > 0 && (!edge_dst || !edge_src))) {
    set_error("bad graph arguments");
    return EGNN_EINVAL;
  }
  if (!have_model) { set_error("egnn_set_model first"); return EGNN_ESTATE; }
  return EGNN_OK;
}

int precision_scope_check(bool ready, int prec, int norm_scope) {
  if (!ready) { set_error("model/graph not set"); return EGNN_ESTATE; }
  if (prec != EGNN_PREC_F32 && prec != EGNN_PREC_BF16 && prec != EGNN_PREC_BF16X3 && prec != EGNN_PREC_F16 && prec != EGNN_PREC_F16C8) {
    set_error("bad precision %d", prec);
    return EGNN_EINVAL;
  }
  if (norm_scope != EGNN_NORM_CALL && norm_scope != EGNN_NORM_GRAPH) { set_error("bad norm scope"); return EGNN_EINVAL; }
  return EGNN_OK;
}

void plan_gemm_tn(int E, int M, int N, int& BN, int& tiles_n, int& S, int& steps_per_slice) {
  BN = (N % 256 == 0) ? 256 : 128;
  tiles_n = N / BN;
  const int ntiles = (M / kGemmBM) * tiles_n;
  const int total_steps = (E + kGemmBK - 1) / kGemmBK;
  int want = (768 + ntiles - 1) / ntiles;                    // ~3 workgroups per CU in all
  const int max_s = total_steps / 16 > 0 ? total_steps / 16 : 1;   // at least 16 steps per slice
  S = want < 1 ? 1 : (want > max_s ? max_s : want);
  steps_per_slice = (total_steps + S - 1) / S;
  S = (total_steps + steps_per_slice - 1) / steps_per_slice;
}

static bool gemm_tn_shape_ok(int E, int M, int N) { return !(E < 1 || M < 256 || M % 256 != 0 || N < 128 || N % 128 != 0); }
// the LDS-DMA loads fetch 16-byte pieces at base + row * ld * 2 + 16 * piece (ld % 8 == 0): the base must be aligned too
static bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

int gemm_tn_args_check(int E, int M, int N, const void* A, int lda, const void* B, int ldb, const void* C, int ldc, int rows,
                       int cols, const void* workspace, size_t workspace_bytes) {
  if (!gemm_tn_shape_ok(E, M, N) || lda < M || ldb < N || lda % 8 != 0 || ldb % 8 != 0 || !A || !B || !C || rows < 1 || rows > M ||
      cols < 1 || cols > N || ldc < cols) {
    set_error("egnn_gemm_tn_bf16: unsupported shape E=%d M=%d N=%d lda=%d ldb=%d", E, M, N, lda, ldb);
    return EGNN_EINVAL;
  }
  if (misaligned16(A) || misaligned16(B)) {
    set_error("egnn_gemm_tn_bf16: the operands must be 16-byte aligned");
    return EGNN_EINVAL;
  }
  // The kernel forms 32-bit byte offsets for the rows of its LAST k-step too (up to kGemmBK - 1 rows past E, answered with
  // zeros by the buffer range check): those offsets must not wrap either.
  const size_t lim = (size_t)1 << 32;
  if ((size_t)(E + kGemmBK - 1) * lda * 2 >= lim || (size_t)(E + kGemmBK - 1) * ldb * 2 >= lim) {
    set_error("egnn_gemm_tn_bf16: operand larger than 4 GiB (cut the reduction into chunks)");
    return EGNN_EINVAL;
  }
  int BN, tiles_n, S, sps;
  plan_gemm_tn(E, M, N, BN, tiles_n, S, sps);
  if (!workspace || workspace_bytes < (size_t)S * M * N * sizeof(float)) {
    set_error("egnn_gemm_tn_bf16: workspace too small (%zu bytes, see egnn_gemm_tn_workspace_bytes)", workspace_bytes);
    return EGNN_EINVAL;
  }
  return EGNN_OK;
}

int gemm_rows_args_check(int E, const void* A0, int lda0, int K0, const void* W0, const void* A1, int lda1, int K1, const void* W1,
                         const void* out, int ldo) {
  if (E < 1 || !A0 || !W0 || !out || K0 < 64 || K0 % 64 != 0 || lda0 < K0 || lda0 % 8 != 0 || ldo < 128 || ldo % 4 != 0 ||
      (A1 && (!W1 || K1 < 64 || K1 % 64 != 0 || lda1 < K1 || lda1 % 8 != 0))) {
    set_error("egnn_gemm_rows_bf16: unsupported shape E=%d K0=%d K1=%d", E, K0, K1);
    return EGNN_EINVAL;
  }
  if (misaligned16(A0) || misaligned16(W0) || (A1 && (misaligned16(A1) || misaligned16(W1)))) {
    set_error("egnn_gemm_rows_bf16: the operands and the fragment packs must be 16-byte aligned");
    return EGNN_EINVAL;
  }
  // a workgroup covers 256 rows: the offsets of the rows past E in the last workgroup must not wrap (see gemm_tn_args_check)
  const size_t lim = (size_t)1 << 32;
  if ((size_t)(E + 255) * lda0 * 2 >= lim || (A1 && (size_t)(E + 255) * lda1 * 2 >= lim)) {
    set_error("egnn_gemm_rows_bf16: operand larger than 4 GiB (cut the rows into chunks)");
    return EGNN_EINVAL;
  }
  return EGNN_OK;
}

int gemm_rows_out_check(const void* out, int ldo, int out_f32, int n_chunks) {
  if (n_chunks < 1 || n_chunks > 65535 || ldo < 128 * n_chunks) {
    set_error("egnn_gemm_rows_bf16: %d column chunks need ldo >= %d", n_chunks, 128 * n_chunks);
    return EGNN_EINVAL;
  }
  if (!out_f32 && (ldo % 8 != 0 || misaligned16(out))) {
    set_error("egnn_gemm_rows_bf16: a bf16 output is stored in 16-byte pieces: ldo %% 8 == 0 and a 16-byte aligned base (ldo=%d)", ldo);
    return EGNN_EINVAL;
  }
  return EGNN_OK;
}

int dense_rows_args_check(int N, int K, int J, const void* in, const void* W, const void* b, const void* out) {
  if (N < 1 || K < 1 || J < 1 || K > 2048 || !in || !W || !b || !out) {
    set_error("bad egnn_dense_rows arguments (K <= 2048)");
    return EGNN_EINVAL;
  }
  return EGNN_OK;
}

// The one statement of a layer's packed streams: field, element size in bytes, element count.  Offsets are integers, so the
// measuring call (base == nullptr) does no pointer arithmetic.
size_t carve_layer_pack(LayerPack& lp, const ModelDims& md, int H, int split_k, char* base) {
  size_t off = 0;
  auto put = [&](auto*& field, size_t elem, size_t count) {
    field = base ? reinterpret_cast<decltype(+field)>(base + off) : nullptr;
    off += (elem * count + kPackAlign - 1) / kPackAlign * kPackAlign;
  };
  const size_t TC = md.TC, WxP = md.WxP, WmP = md.WmP, MP = md.MP, WhP = md.WhP, HP = md.HP;
  const size_t w2x = WxP * WxP, w2m = MP * WmP, w2h = HP * WhP;   // elements of the three second-layer weight matrices
  put(lp.w1catT, 4, H * TC);
  put(lp.b1cat, 4, TC);
  put(lp.wdx, 4, WxP);
  put(lp.wdm, 4, WmP);
  put(lp.w2x_f32, 4, w2x);
  put(lp.w2x_bf16, 2, w2x);
  put(lp.b2x, 4, WxP);
  put(lp.w3x, 4, WxP);
  put(lp.w2m_f32, 4, w2m);
  put(lp.w2m_bf16, 2, w2m);
  put(lp.b2m, 4, MP);
  put(lp.wa, 4, MP);
  put(lp.scal, 4, 4);
  put(lp.w1h_f32, 4, WhP * md.K1P);
  put(lp.b1h, 4, WhP);
  put(lp.w2h_f32, 4, w2h);
  put(lp.b2h, 4, HP);
  put(lp.w1catT_s, 4, H * TC);
  put(lp.b1cat_s, 4, TC);
  put(lp.wdx_s, 4, WxP);
  put(lp.wdm_s, 4, WmP);
  put(lp.b2x_s, 4, WxP);
  put(lp.w3x_s, 4, WxP);
  put(lp.b2m_s, 4, MP);
  put(lp.wa_s, 4, MP);
  put(lp.w1h_bf16, 2, WhP * md.K1Q);
  put(lp.w2h_bf16p, 2, w2h);
  put(lp.w2x_bf16s, 2, w2x);
  put(lp.w2m_bf16s, 2, w2m);
  put(lp.w2x_bf16s16, 2, w2x);
  put(lp.w2x_bf16s_lo, 2, w2x);
  put(lp.w2m_bf16s_lo, 2, w2m);
  put(lp.w2xT_bf16, 2, w2x);
  put(lp.w2mT_bf16, 2, w2m);
  put(lp.w1hl_bf16, 2, (TC / 32) * 3 * 2 * 512);
  put(lp.w2m_bf16s16, 2, w2m);
  put(lp.w2m_f16s16, 2, w2m);
  put(lp.w2x_f16s16, 2, w2x);
  put(lp.w2m_f16s, 2, w2m);
  put(lp.w2h_f16p, 2, w2h);
  lp.w1h_f16k = lp.w1h_f16k_lo = lp.w2h_f16p_lo = nullptr;
  if (md.HP <= 64 && H + md.MP > split_k / 2 && H + md.MP <= split_k) {   // shapes of the split-operand node MLP
    put(lp.w1h_f16k, 2, WhP * split_k);
    put(lp.w1h_f16k_lo, 2, WhP * split_k);
    put(lp.w2h_f16p_lo, 2, w2h);
  }
  put(lp.w2x_f16s, 2, w2x);
  put(lp.w2x_c8w, 1, 2 * w2x);   // e4m3 heads + remainders: 2 bytes per weight
  put(lp.w2m_c8w, 1, 2 * w2m);
  put(lp.c8_exp, 4, 8);          // [0..3] scale exponents {x: hi, lo, m: hi, lo}, [4..5] max |w| scratch
  return off;
}

bool fork_candidate(int E, int WxP) {
  const long tiles = ((long)E + 127) / 128, xw = tiles * (WxP >= 512 ? WxP / 512 : 1);
  const long idle = (xw + 255) / 256 * 256 - xw;
  return E > 0 && idle >= (tiles + 1) / 2;
}

EdgePath path_of_precision(int prec) {
  return prec == EGNN_PREC_BF16 ? EdgePath::kBf16 : prec == EGNN_PREC_BF16X3 ? EdgePath::kBf16x3
       : prec == EGNN_PREC_F16 ? EdgePath::kF16 : prec == EGNN_PREC_F16C8 ? EdgePath::kF16c8 : EdgePath::kGeneric;
}

// half-precision table: bf16 hi/lo MFMA for H <= 48 (1024-column workgroups once they fill the chip, else 256-column ones),
// else exact f32 MFMA for H <= 64, else the VALU kernel; the fp32 table has the last two only
NodePre node_pre_form(bool half_table, int N, int H, int TC) {
  if (half_table && H <= 48) return (long)((N + kHiloNodes - 1) / kHiloNodes) * (TC / 1024) >= 256 ? NodePre::kHilo8 : NodePre::kHilo2;
  return H <= 64 ? NodePre::kMfma : NodePre::kValu;
}

int plan_forward(const ForwardAsk& a, ForwardPlan* out) {
  ForwardPlan pl;
  const KernelSupport& sup = a.sup;
  const int WxP = a.md.WxP;
  const EdgePath want = path_of_precision(a.prec);
  const bool takes = want == EdgePath::kBf16 ? sup.v4 && sup.v3 : want == EdgePath::kBf16x3 ? sup.bf16x3
                   : want == EdgePath::kF16 ? sup.v4 && sup.x_m16 : want == EdgePath::kF16c8 ? sup.f16c8w : false;
  pl.path = a.sw.edge >= 4 && takes ? want : EdgePath::kGeneric;
  if (a.save && pl.path != EdgePath::kBf16) { set_error("egcl_forward_save needs the 128-edge-tile bf16 kernels"); return EGNN_EINVAL; }
  const bool tiled = pl.path != EdgePath::kGeneric;   // the tiled kernels sum d^2 per receiving node themselves
  pl.frag_bf16 = !tiled && a.prec == EGNN_PREC_BF16;
  pl.half_table = pl.path == EdgePath::kBf16 || pl.path == EdgePath::kF16;
  pl.node_pre = node_pre_form(pl.half_table, a.N, a.H, a.md.TC);
  pl.absorbs_finish = pl.half_table && a.H <= 48;
  pl.save = a.save;

  if (a.E > 0) {
    // fork_candidate(): whether the message kernel fits the shadow of the coordinate kernel's last round; the small-tile
    // kernels fork whenever there is a side stream; a training forward and the one-launch bf16x3 pair never do
    const bool can_fork = a.side_ok && !a.prof, fork = can_fork && fork_candidate(a.E, WxP);
    // 32- / 64-edge tiles (edge_small.hip) up to 2,048 / 6,144 edges (profiles/r04e_latency_small_tiles.log, ms per replayed
    // reverse step: 20-atom cell 0.289 -> 0.277, but one 64-atom cell on 32 rows 0.313 -> 0.343 and five 0.41 -> 0.70): a layer's
    // weight traffic through L2 is (E / tile rows) x 2.5 MB whatever the column split, and L2 delivers ~7 TB/s to 256 streaming CUs
    const bool small_ok = pl.half_table && !a.save && a.small_ok && sup.small;
    const int small = !small_ok ? 0 : a.E <= a.sw.small_edges ? 32 : a.E <= a.sw.small64_edges ? 64 : 0;
    switch (pl.path) {
      case EdgePath::kGeneric: pl.form = EdgeForm::kGeneric64; break;
      case EdgePath::kBf16x3: pl.form = EdgeForm::kBf16x3; pl.R = kTileRows; pl.nsplit_x = WxP / 256; break;
      case EdgePath::kF16c8: pl.form = EdgeForm::kF16c8; pl.R = kTileRows; pl.nsplit_x = WxP / 512; pl.fork = fork; break;
      case EdgePath::kBf16:
      case EdgePath::kF16:
        pl.f16 = pl.path == EdgePath::kF16;
        if (small) { pl.form = EdgeForm::kSmall; pl.R = small; pl.nsplit_x = WxP / 512; pl.fork = can_fork; break; }
        pl.form = EdgeForm::kTile128; pl.R = kTileRows; pl.fork = fork && !a.save;
        if (!sup.x_m16) { pl.coord = CoordKernel::kV3; break; }   // hidden width 256
        pl.nsplit_x = WxP / 512;
        // one persistent workgroup per CU once there are more than two 512-column units per CU
        if (!a.save && a.sw.x_persist && persistent_possible(a.E, WxP, a.ncu)) {
          pl.coord = CoordKernel::kXm16Persistent; pl.persist_grid = a.ncu;
        } else pl.coord = CoordKernel::kXm16;
        break;
    }
  }

  // node MLP of fp16, bf16x3 and f16c8 on their tiled paths: split-operand fp16 products where the shape allows; bf16: the bf16
  // kernel; else the exact fp32 kernel
  const bool split_path = pl.path == EdgePath::kF16 || pl.path == EdgePath::kBf16x3 || pl.path == EdgePath::kF16c8;
  pl.node_post = split_path && sup.post_split ? NodePost::kSplit
               : a.prec == EGNN_PREC_BF16 && sup.post_bf16 ? NodePost::kBf16 : NodePost::kF32;

  // the per-graph sums need no launch when only node_post reads them and it can add them up itself (not the fp32 kernel)
  const bool per_graph = a.norm_scope == EGNN_NORM_GRAPH;
  pl.sq = !tiled ? SqSource::kNodeD2 : a.E == 0 ? SqSource::kMemset
        : !per_graph || a.need_gscale || pl.node_post == NodePost::kF32 ? SqSource::kLaunch : SqSource::kNodePost;
  *out = pl;
  return EGNN_OK;
}

}  // namespace egnn

using namespace egnn;

extern "C" {

const char* egnn_last_error(void) { return g_err; }
int egnn_version(void) { return 1; }

size_t egnn_gemm_tn_workspace_bytes(int E, int M, int N) {   // 0 = unsupported shape
  if (!gemm_tn_shape_ok(E, M, N)) return 0;
  int BN, tiles_n, S, sps;
  plan_gemm_tn(E, M, N, BN, tiles_n, S, sps);
  return (size_t)S * M * N * sizeof(float);
}

// ---- schedule (host, fp32, same operation order as torch on CPU) ----------------------------------
int schedule_table_from_alpha(int T, const float* alpha, const float* sigma, float* table) {
  if (T < 1 || !alpha || !table) { set_error("bad schedule arguments"); return EGNN_EINVAL; }
  for (int t = 1; t <= T; ++t) {
    // calculate_mu / reverse_diffuse_one_step, diffusion_x_h.py:61-90 (fp32 scalar arithmetic)
    const float at = alpha[t], as = alpha[t - 1];
    const float sq_t = 1.0f - at * at, sq_s = 1.0f - as * as;
    const float ats = at / as;
    const float sq_ts = sq_t - (ats * ats) * sq_s;
    const float sig_t = sqrtf(sq_t);
    table[4 * t + 0] = 1.0f / ats;
    table[4 * t + 1] = sq_ts / ats / sig_t;
    table[4 * t + 2] = sqrtf(sq_ts * sq_s / sq_t);
    table[4 * t + 3] = (float)t / (float)T;
  }
  const float a0 = alpha[0], s0 = sigma ? sigma[0] : sqrtf(1.0f - a0 * a0);
  table[0] = 1.0f / a0; table[1] = s0 / a0; table[2] = s0 / a0; table[3] = 0.f;
  return EGNN_OK;
}

int schedule_table_build(int T, double s, double power, float* alpha, float* sigma, float* table) {
  if (T < 1) { set_error("T must be >= 1"); return EGNN_EINVAL; }
  std::vector<float> a(T + 1), sg(T + 1);
  // polynomial_schedule (:99-106): x = linspace(0,T,T+1); a2 = (1 - (x/T)^p)^2
  // clip_noise_schedule (:92-97): ratios to the previous entry (first vs 1), clamp [0.001, 1], cumprod.
  // Python scalars enter torch's fp32 tensor arithmetic rounded to fp32: (1 - 2*s) and s are formed in
  // double first; torch.pow with exponent 2 / 3 is evaluated as x*x / x*x*x.
  const float prec = (float)(1.0 - 2.0 * s), sf = (float)s, pw = (float)power;
  // torch.cumprod on CPU accumulates fp32 inputs in double and rounds each output to fp32
  float prev = 1.0f;
  double cum = 1.0;
  for (int i = 0; i <= T; ++i) {
    const float q = (float)i / (float)T;  // linspace(0, T, T+1) is exact for integer endpoints
    float qp;
    if (power == 2.0) qp = q * q;
    else if (power == 3.0) qp = q * q * q;
    else if (power == 1.0) qp = q;
    else qp = powf(q, pw);
    const float base = 1.0f - qp;
    const float a2 = base * base;
    float step = a2 / prev;
    step = fminf(fmaxf(step, 0.001f), 1.0f);
    cum = (i == 0) ? (double)step : cum * (double)step;
    prev = a2;
    a[i] = prec * (float)cum + sf;
    sg[i] = sqrtf(1.0f - a[i] * a[i]);
  }
  if (alpha) memcpy(alpha, a.data(), sizeof(float) * (T + 1));
  if (sigma) memcpy(sigma, sg.data(), sizeof(float) * (T + 1));
  if (table) return schedule_table_from_alpha(T, a.data(), sg.data(), table);
  return EGNN_OK;
}

// Entry points of the CPU-only sanitizer build (make asan): the validation layer of the device entry points, callable
// without a GPU.  Not exported by libegnn_amd.so (compiled only with -DEGNN_HOST_TEST_API).
#ifdef EGNN_HOST_TEST_API
int egnn_host_model_dims(int L, int H, int M, int Wm, int Wx, int Wh, int* out10) {
  ModelDims d;
  const int rc = model_dims(L, H, M, Wm, Wx, Wh, &d);
  if (rc == EGNN_OK && out10) {
    const int v[10] = {d.WxP, d.WmP, d.MP, d.WhP, d.HP, d.K1P, d.K1Q, d.TC, d.cbx, d.cbm};
    memcpy(out10, v, sizeof(v));
  }
  return rc;
}
int egnn_host_graph_args_check(int have_model, int N, int E, int B, const void* a, const void* b, const void* c, const void* d,
                               const void* e) {
  return graph_args_check(have_model != 0, N, E, B, a, b, c, d, e);
}
int egnn_host_precision_scope_check(int ready, int prec, int scope) { return precision_scope_check(ready != 0, prec, scope); }
int egnn_host_plan_gemm_tn(int E, int M, int N, int* out4) {
  int BN, tn, S, sps;
  plan_gemm_tn(E, M, N, BN, tn, S, sps);
  out4[0] = BN; out4[1] = tn; out4[2] = S; out4[3] = sps;
  return EGNN_OK;
}
int egnn_host_gemm_tn_args_check(int E, int M, int N, const void* A, int lda, const void* B, int ldb, const void* C, int ldc, int rows,
                                 int cols, const void* ws, size_t wsb) {
  return gemm_tn_args_check(E, M, N, A, lda, B, ldb, C, ldc, rows, cols, ws, wsb);
}
int egnn_host_gemm_rows_args_check(int E, const void* A0, int lda0, int K0, const void* W0, const void* A1, int lda1, int K1,
                                   const void* W1, const void* out, int ldo) {
  return gemm_rows_args_check(E, A0, lda0, K0, W0, A1, lda1, K1, W1, out, ldo);
}
int egnn_host_dense_rows_args_check(int N, int K, int J, const void* in, const void* W, const void* b, const void* out) {
  return dense_rows_args_check(N, K, J, in, W, b, out);
}
int egnn_host_fork_candidate(int E, int WxP) { return fork_candidate(E, WxP) ? 1 : 0; }
#endif

}  // extern "C"

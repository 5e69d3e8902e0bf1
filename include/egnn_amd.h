/*
 * egnn_amd.h -- C ABI of the MI355X (gfx950) EGNN denoiser library (libegnn_amd.so).
 *
 * The reference (Ren-Okubo/diffusion_model) is pure Python and has no FFI layer; its de-facto
 * operator interface for the eps_theta(x_t, h_t, t) path is two call signatures and a state-dict
 * layout.  Each entry point below names the reference interface it replaces.
 *
 * Conventions
 *   - every function returns 0 on success or a negative EGNN_E* code; nothing throws;
 *   - all pointers named d_* are DEVICE pointers owned by the caller; the library allocates
 *     device memory only inside the opaque egnn_ctx workspace (freed by egnn_destroy);
 *   - every launch goes to the hipStream_t passed in (as void*); no call synchronises the
 *     device except egnn_create/egnn_destroy/egnn_reserve_*, egnn_sampler_prepare (allocation),
 *     and the explicitly named *_sync helpers;
 *   - a context is re-entrant across streams only if calls are externally ordered; it is not
 *     thread-safe;
 *   - tensors are row-major fp32 unless noted; weights are torch.nn.Linear layout [out, in].
 */
#ifndef EGNN_AMD_H
#define EGNN_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libegnn_amd.so is built with -fvisibility=hidden: exactly the functions declared below are exported */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef struct egnn_ctx egnn_ctx;

enum {
  EGNN_OK = 0,
  EGNN_EINVAL = -22,   /* bad argument / unsupported dimension           */
  EGNN_ENOMEM = -12,   /* device allocation failed                       */
  EGNN_ESTATE = -1,    /* call order violated (model/graph/weights unset) */
  EGNN_EHIP = -5       /* a HIP runtime call failed (see egnn_last_error) */
};

/* arithmetic of the per-edge MLP contractions */
enum { EGNN_PREC_F32 = 0,   /* v_mfma_f32_32x32x2_f32: exact fp32 (parity mode)          */
       EGNN_PREC_BF16 = 1,  /* v_mfma_f32_32x32x16_bf16, fp32 accumulate (throughput)    */
       EGNN_PREC_BF16X3 = 2,/* fp32-grade accuracy on the bf16 matrix cores: both operands of the per-edge second-layer
                               * products split into bf16 head + bf16 remainder, three MFMAs per tile (2^-17 relative);
                               * fp32 table, heads and node MLP.  Shapes outside the 128-edge-tile kernels run as F32. */
       EGNN_PREC_F16 = 3,   /* the BF16 path's kernels on fp16 MFMA operands (v_mfma_f32_16x16x32_f16 / 32x32x16_f16: same
                               * rate, 11 significant bits instead of 8; overflow saturates at +-65504); inference only
                               * (egcl_forward_save stays bf16).  Hidden widths other than 512 / 1024 run as F32. */
       EGNN_PREC_F16C8 = 4 };/* fp32-grade accuracy for TWO bf16-equivalents of matrix work: fp16 heads on
                               * v_mfma_f32_32x32x16_f16 + both remainder products on ONE block-scaled e4m3 instruction
                               * (v_mfma_scale_f32_32x32x64_f8f6f4, twice the f16 rate) with fixed power-of-two block scales;
                               * fp32 table, heads and split-operand node MLP as BF16X3 (csrc/edge_f16c8w.hip); inference
                               * only.  Hidden widths other than 512 / 1024 run as F32. */

/* scope of the coordinate normaliser ||X_i - X_j||_F of EquivariantGraphNeuralNetwork.py:64 */
enum { EGNN_NORM_CALL = 0,  /* literal reference: one scalar over every edge of the call  */
       EGNN_NORM_GRAPH = 1 };/* one scalar per graph (== reference when called per graph) */

const char* egnn_last_error(void);
int egnn_version(void);

/* ---- workspace ------------------------------------------------------------------------ */
int egnn_create(egnn_ctx** out, int device);
int egnn_destroy(egnn_ctx* ctx);

/* Model dimensions.  Replaces the constructor arguments of
 * EquivariantGNN(L, m_input, m_hidden, m_output, x_input, x_hidden, x_output, h_input, h_hidden,
 * h_output) (EquivariantGraphNeuralNetwork.py:74-78) under the wiring of main.py:102-121:
 * m_input = x_input = 2*H+1, x_output = 1, h_input = H+M, h_output = H. */
int egnn_set_model(egnn_ctx* ctx, int L, int H, int M, int Wm, int Wx, int Wh);

/* Upload + repack the parameters of layer l (state-dict entries egcl_list.{l}.*; fp32 device
 * pointers in nn.Linear layout).  Must be called again whenever the parameters change. */
int egnn_pack_layer(egnn_ctx* ctx, void* stream, int l,
                    const float* d_m0_w, const float* d_m0_b,   /* mlp_m.0  [Wm, 2H+1], [Wm] */
                    const float* d_m2_w, const float* d_m2_b,   /* mlp_m.2  [M, Wm],    [M]  */
                    const float* d_x0_w, const float* d_x0_b,   /* mlp_x.0  [Wx, 2H+1], [Wx] */
                    const float* d_x2_w, const float* d_x2_b,   /* mlp_x.2  [Wx, Wx],   [Wx] */
                    const float* d_x4_w, const float* d_x4_b,   /* mlp_x.4  [1, Wx],    [1]  */
                    const float* d_h0_w, const float* d_h0_b,   /* mlp_h.0  [Wh, H+M],  [Wh] */
                    const float* d_h2_w, const float* d_h2_b,   /* mlp_h.2  [H, Wh],    [H]  */
                    const float* d_a_w, const float* d_a_b);    /* attention.0 [1, M],  [1]  */

/* Graph topology for subsequent forwards.  Replaces the edge_index argument of
 * EquivariantGNN.forward(edge_index, h, x) (:85) plus PyG's batch vector.
 *   d_edge_dst/d_edge_src : int32[E], edges sorted by destination (edge_index[0]) -- the node
 *                           that RECEIVES the message (flow='target_to_source', :10-11);
 *   d_row_ptr             : int32[N+1] CSR offsets of that ordering;
 *   d_graph_ptr           : int32[B+1] node ranges of the B graphs (graphs are contiguous);
 *   d_node_graph          : int32[N] graph id of every node.
 * The arrays are referenced, not copied: they must stay alive while the graph is set. */
int egnn_set_graph(egnn_ctx* ctx, int N, int E, int B,
                   const int32_t* d_edge_dst, const int32_t* d_edge_src, const int32_t* d_row_ptr,
                   const int32_t* d_graph_ptr, const int32_t* d_node_graph);

/* Optional second stream of the caller's for small graphs: when a layer's coordinate kernel leaves most CUs idle, the
 * message kernel of the same layer is launched on `stream` between a fork and a join event (graph edges under capture).
 * The library itself never creates a stream; NULL (default) = everything on the stream of the call. */
int egnn_set_side_stream(egnn_ctx* ctx, void* stream);

/* One EGCL layer: EGCL.forward(edge_index, h, coords) -> (h', x')
 * (EquivariantGraphNeuralNetwork.py:67-71).  h [N,H], x [N,3]; outputs must not alias inputs. */
int egcl_forward(egnn_ctx* ctx, void* stream, int layer, int prec, int norm_scope,
                 const float* d_h, const float* d_x, float* d_h_out, float* d_x_out);

/* The same layer in two stages, for one large graph whose receiving nodes are partitioned over ranks
 * (BASELINE configs[4]): each rank sets a graph that holds only the edges its nodes receive.
 * _begin runs node_pre + the fused edge pass and returns this rank's sums of d^2 (float[B], or [1] in 'call'
 * scope); the caller all-reduces them (the coordinate normaliser of :64 spans all edges) and passes the
 * totals to _end, which runs node_post; rows of nodes the rank does not own are meaningless and the caller
 * all-gathers the owned rows.  d_sq_sums may be NULL (single rank: use the local sums).  _end finishes the layer the last
 * _begin on this context started: its layer and prec must be that call's (the node kernel was chosen there). */
int egcl_forward_begin(egnn_ctx* ctx, void* stream, int layer, int prec, int norm_scope,
                       const float* d_h, const float* d_x, float* d_sq_sums);
int egcl_forward_end(egnn_ctx* ctx, void* stream, int layer, int prec, int norm_scope,
                     const float* d_h, const float* d_x, const float* d_sq_sums, float* d_h_out, float* d_x_out);

/* ---- backward of one EGCL layer (training: EquivariantGNN.forward must be differentiable w.r.t. h, x and all
 * parameters; the reference gets this from torch autograd over :55-71) -------------------------
 * The layer's backward is   l1_act -> GEMM -> heads -> GEMM,GEMM -> l1_grad -> GEMM,GEMM   where the GEMMs are
 * the plain dgrad / wgrad products of the Linear layers (run by the caller's BLAS on the buffers below) and the
 * three stage functions fuse everything in between, one pass over HBM each.  prec selects the storage type of
 * the [edges, width] buffers (EGNN_PREC_F32: float, EGNN_PREC_BF16: bf16); arithmetic is fp32.  dst/src are
 * the int32 edge arrays of egnn_set_graph (any contiguous slice of edges); all pointers are device memory.
 *
 * egcl_read_aggregates: the three segment sums of the layer that was just run on ctx by egcl_forward
 *   (sum_m [N,M] = sum of gated messages :68, sum_x [N,3] = sum of (x_i-x_j)*s before the 1/(G+1) factor :64/:70,
 *   sq_sums [B] or [1] = sum of d^2 per graph / per call), so that the backward need not recompute them. */
int egcl_read_aggregates(egnn_ctx* ctx, void* stream, int norm_scope, float* d_sum_m, float* d_sum_x,
                         float* d_sq_sums);
/* s1[e][c] = SiLU(P[dst e][c] + Q[src e][c] + wd[c]*d2[e]) for C table columns: the first Linear+SiLU of mlp_x
 * and mlp_m (:13-14, :19-20) on in = [h_i | h_j | d2] (:56), with P = h.W1[:, :H]^T + b1 and Q = h.W1[:, H:2H]^T
 * tabulated per node by the caller and wd = W1[:, 2H]. */
int egcl_backward_l1_act(void* stream, int prec, int n_edges, int C, const int32_t* d_dst, const int32_t* d_src,
                         const float* d_P, const float* d_Q, const float* d_wd, const float* d_d2, void* d_s1_out);
/* In place: a2x [n_edges,W] (= s1x.W2x^T) -> dL/da2x and a2m [n_edges,M] (= s1m.W2m^T) -> dL/da2m, through
 * SiLU, the scalar head mlp_x.4 and xm = (x_i-x_j)*s (:62-65), and SiLU, the attention gate and m*gate (:57-60),
 * given the gradients of the segment sums g_sum_x [N,3] (already multiplied by 1/(G+1)) and g_sum_m [N,M].
 * Also writes g_diff [n_edges,3] = dL/d(x_i-x_j) through s, and ADDS the column sums to g_b2x [W], g_w3 [W],
 * g_b3 [1], g_b2m [M], g_wa [M], g_ba [1] (gradients of mlp_x.2.bias, mlp_x.4.weight/.bias, mlp_m.2.bias,
 * attention.0.weight/.bias).  b3 and ba are device pointers to the two scalar biases. */
int egcl_backward_heads(void* stream, int prec, int n_edges, int W, int M, const int32_t* d_dst, const int32_t* d_src,
                        const float* d_x, const float* d_g_sum_x, const float* d_g_sum_m, void* d_a2x_inout,
                        void* d_a2m_inout, const float* d_b2x, const float* d_w3, const float* d_b3,
                        const float* d_b2m, const float* d_wa, const float* d_ba, float* d_g_diff, float* d_g_b2x,
                        float* d_g_w3, float* d_g_b3, float* d_g_b2m, float* d_g_wa, float* d_g_ba);
/* In place: g_s1[e][c] *= SiLU'(P[dst e][c] + Q[src e][c] + wd[c]*d2[e])  (dL/ds1 -> dL/da1). */
int egcl_backward_l1_grad(void* stream, int prec, int n_edges, int C, const int32_t* d_dst, const int32_t* d_src,
                          const float* d_P, const float* d_Q, const float* d_wd, const float* d_d2,
                          void* d_g_s1_inout);

/* in[e] = [h_i | h_j | d2 | 1 | 0 ...] (:56; K1P >= 2H+2 columns, the ones column carries the bias gradient through
 * the wgrad GEMM) in the storage type of prec, and d2[e] = |x_i - x_j|^2 as float. */
int egcl_backward_gather_in(void* stream, int prec, int n_edges, int H, int K1P, const int32_t* d_dst,
                            const int32_t* d_src, const float* d_h, const float* d_x, void* d_in_out, float* d_d2_out);
/* Adjoint of the gather: g_in [n_edges,K1P] = dL/d[h_i | h_j | d2 | ...] (storage type of prec).
 * g_h[i] += g_in[:H], g_h[j] += g_in[H:2H]; dL/d(x_i-x_j) = g_diff[e] + 2 (g_in[2H] + g_sq_sums[segment of i]) (x_i-x_j)
 * is added to g_x[i] and subtracted from g_x[j] (fp32 atomic adds).  node_segment [N] maps a node to its entry of
 * g_sq_sums (the gradient of egcl_read_aggregates' sq_sums); NULL = one sum for the whole call. */
int egcl_backward_scatter(void* stream, int prec, int n_edges, int H, int K1P, const int32_t* d_dst,
                          const int32_t* d_src, const float* d_x, const void* d_g_in, const float* d_g_diff,
                          const float* d_g_sq_sums, const int32_t* d_node_segment, float* d_g_h, float* d_g_x);

/* Node MLP backward, activation stage (mlp_h = Linear -> SiLU -> Linear, :26-30 under autograd): from the recomputed first-layer
 * product z [N, ldz] fp32 (WITHOUT its bias b1 [W]) and dL/ds [N, ldg] fp32, one pass writes s = SiLU(z + b1) and
 * dL/dz = dL/ds * SiLU'(z + b1) as bf16 [N, ldo] (the operands of the weight-gradient / dgrad products) and ADDS the bias
 * gradient (column sums of dL/dz) to d_g_b1 [W] (fp32 atomics: zero it first).  W and the row strides multiples of 4. */
int egcl_backward_node_act(void* stream, int N, int W, const float* d_z, int ldz, const float* d_b1, const float* d_g_s, int ldg,
                           void* d_g_z_out, void* d_s_out, int ldo, float* d_g_b1);

/* First Linear layers of both edge MLPs, factorised as the forward factorises them (csrc/edge_bwd_first.hip): ONE pass over
 * dL/da1 (d_g1x [n_edges, Wx], d_g1m [n_edges, Wm], bf16; the outputs of egcl_backward_dgrad for the edges
 * [e_first, e_first + n_edges) of the plan) produces, for batches of graphs of at most 64 nodes, the per-node sums
 * Gd[n] = sum of g1 over the edges n receives, Gs[n] = over the edges n sends ([N, W] fp32, ACCUMULATED: zero them per layer),
 * cd[graph] = sum_e g1[e] d2_e ([B, W], accumulated) and the (Wx + Wm) / 256 shares of dL/d(d2_e) = g1[e] . W1[:, 2H]
 * (d_gd2_part [(Wx + Wm) / 256, n_edges], assigned).  The first-layer weight gradients and dL/dh are then node-level products
 * (dL/dW1[:, :H] = Gd^T h, dL/dW1[:, H:2H] = Gs^T h, dL/dW1[:, 2H] = sum of cd, dL/db1 = sum of Gd, dL/dh += Gd W1[:, :H] +
 * Gs W1[:, H:2H]) -- replaces egcl_backward_gather_in, two weight-gradient GEMMs over all edges, the row-streaming dgrad GEMM and
 * the feature half of egcl_backward_scatter (torch autograd over EquivariantGraphNeuralNetwork.py:13-25, :56). */
int egcl_backward_first_reduce(void* stream, int B, int max_graph_nodes, int e_first, int n_edges, const int32_t* d_graph_ptr,
                               const int32_t* d_row_ptr, const int32_t* d_edge_src, const float* d_x, const void* d_g1x, int Wx,
                               const void* d_g1m, int Wm, const float* d_wdx, const float* d_wdm, float* d_Gd_x, float* d_Gs_x,
                               float* d_Gd_m, float* d_Gs_m, float* d_cd_x, float* d_cd_m, float* d_gd2_part);
/* The geometry half of egcl_backward_scatter for that path: dL/d(x_i - x_j) = g_diff[e] + 2 (sum of the nparts shares of
 * dL/d(d2_e) + g_sq_sums[segment of i]) (x_i - x_j), added to g_x[i] and subtracted from g_x[j] (fp32 atomic adds). */
int egcl_backward_scatter_geom(void* stream, int n_edges, int nparts, const int32_t* d_dst, const int32_t* d_src, const float* d_x,
                               const float* d_gd2_part, const float* d_g_diff, const float* d_g_sq_sums,
                               const int32_t* d_node_segment, float* d_g_x);

/* Fused first half of the chain above for the bf16 fast path (reference widths: hidden 256 / 512 / 1024, m = 256, unpadded):
 * one pass of the forward's own MFMA edge kernels in "backward" mode replaces gather/l1_act -> GEMM -> heads.  For the
 * edges [e_first, e_first + n_edges) of the graph set on ctx it recomputes SiLU(P[dst] + Q[src] + wd d2) (fp16 table built
 * by egcl_backward_table from the layer's input h) and the second-layer products exactly as the forward did, and writes
 *   s1x [n_edges, Wx], s1m [n_edges, Wm]  bf16, the activations AS THE MFMA CONSUMED THEM: scaled by -log2(e) (multiply the
 *                                         wgrad g_a2^T . s1 by -ln 2),
 *   g_a2x [n_edges, Wx], g_a2m [n_edges, M]  bf16 = dL/d(second-layer pre-activation) (what egcl_backward_heads leaves),
 *   g_diff [n_edges, 3] and the column sums ADDED to g_b2x, g_w3, g_b3, g_b2m, g_wa, g_ba, as egcl_backward_heads does.
 * g_sum_x [N,3] must already carry the 1/(G+1) factor; g_sum_m is [N, M].  egcl_backward_fused_supported = 1 if the
 * context's model takes this path; it is asked on the packed streams of layer 0, so it answers 0 (and the entry points of this
 * path report the path as unavailable) until egnn_pack_layer has packed that layer. */
int egcl_backward_fused_supported(egnn_ctx* ctx);
int egcl_backward_table(egnn_ctx* ctx, void* stream, int layer, const float* d_h);
int egcl_backward_edge_recompute(egnn_ctx* ctx, void* stream, int layer, const float* d_x, const float* d_g_sum_x,
                                 const float* d_g_sum_m, int e_first, int n_edges, void* d_s1x, void* d_s1m,
                                 void* d_g_a2x, void* d_g_a2m, float* d_g_diff, float* d_g_b2x, float* d_g_w3,
                                 float* d_g_b3, float* d_g_b2m, float* d_g_wa, float* d_g_ba);

/* The same first half WITHOUT the recompute pass, for a training process that can afford E x (2 Wx + Wm + M) bf16 per
 * layer (7 GB at 2^20 edges and the reference widths): egcl_forward_save is egcl_forward in bf16 mode whose edge kernels
 * also leave in HBM, for ALL E edges of the layer,
 *   s1x [E, Wx], s1m [E, Wm]  bf16 as above (scaled by -log2(e)),
 *   t2x [E, Wx], t2m [E, M]   bf16 = -log2(e) * (second-layer pre-activation incl. bias),
 *   s_shares [Wx / 512][E]    fp32 column-split shares of s_e = w3 . SiLU(a2) + b3 (their sum is s_e);
 * (h_out, x_out) are those of egcl_forward in bf16 -- bitwise where egcl_forward runs the same 128-edge-tile kernels (hidden
 * width 256, or more than 6,144 edges); for smaller batches at hidden width 512 / 1024 egcl_forward takes 32 / 64-edge tiles
 * (csrc/edge_small.hip), whose per-edge products and per-node sums are the same terms accumulated in another order: the three
 * aggregates then agree to fp32 accumulation error, not bitwise.  The per-graph sums of d^2 stay readable (egcl_read_aggregates).
 * egcl_backward_heads_saved then turns rows [e_first, e_first + n_edges) of t2x / t2m into dL/d(a2) IN PLACE (an
 * element-wise pass at HBM speed: loss.backward() of parts/train_per_iretation.py:172 for the two heads, :57-65) and adds
 * the column sums / writes g_diff exactly as egcl_backward_edge_recompute does.  d_t2x / d_t2m point at row e_first. */
int egcl_forward_save(egnn_ctx* ctx, void* stream, int layer, int norm_scope, const float* d_h, const float* d_x,
                      float* d_h_out, float* d_x_out, void* d_s1x, void* d_s1m, void* d_t2x, void* d_t2m,
                      float* d_s_shares);
int egcl_backward_heads_saved(egnn_ctx* ctx, void* stream, int layer, const float* d_x, const float* d_g_sum_x,
                              const float* d_g_sum_m, int e_first, int n_edges, void* d_t2x, void* d_t2m,
                              const float* d_s_shares, float* d_g_diff, float* d_g_b2x, float* d_g_w3, float* d_g_b3,
                              float* d_g_b2m, float* d_g_wa, float* d_g_ba);

/* Fused second half for the same path: g_a1 = (g_a2 . W2) * SiLU'(a1) for mlp_x ([n_edges, Wx] from [n_edges, Wx]) and
 * mlp_m ([n_edges, Wm] from [n_edges, M]) on MFMA, i.e. the dgrad GEMMs of mlp_x.2 / mlp_m.2 with egcl_backward_l1_grad
 * in their epilogue (the first-layer pre-activations come from the table egcl_backward_table left on ctx).  bf16 row-major
 * in and out. */
int egcl_backward_dgrad(egnn_ctx* ctx, void* stream, int layer, const float* d_x, int e_first, int n_edges,
                        const void* d_g_a2x, const void* d_g_a2m, void* d_g_a1x_out, void* d_g_a1m_out);

/* The same dgrad WITHOUT dL/da1 in memory (csrc/edge_bwd_dgrad_graph.hip; replaces egcl_backward_dgrad +
 * egcl_backward_first_reduce for batches of graphs of at most 64 nodes): one workgroup per (graph, 256 hidden units) multiplies
 * g_a2 . W2, applies SiLU'(a1) on the accumulator tile and reduces it there for the first Linear layers:
 *   d_G  bf16 [N, 2 Wx + 2 Wm] = [Gd_x | Gs_x | Gd_m | Gs_m], Gd[n] / Gs[n] = fp32 sums of g1 over the edges node n receives /
 *        sends, stored as the bf16 operands of the node-level products (dW1 = G^T [h | 1], dL/dh += G W1);
 *   d_cd_x / d_cd_m [B, W] fp32: cd[graph] = sum_e g1[e] d2_e;
 *   d_gd2_part [(Wx + Wm) / 256, n_edges]: the column-slice shares of dL/d(d2_e) for egcl_backward_scatter_geom.
 * All ASSIGNED for the graphs of the chunk (rows of graphs without edges are left as they are: zero them once).  The chunk
 * [e_first, e_first + n_edges) must consist of WHOLE graphs (egnn_set_graph's graph ranges); d_g_a2x / d_g_a2m are the chunk's
 * rows. */
int egcl_backward_dgrad_reduce(egnn_ctx* ctx, void* stream, int layer, const float* d_x, int e_first, int n_edges,
                               const void* d_g_a2x, const void* d_g_a2m, void* d_G, float* d_cd_x, float* d_cd_m,
                               float* d_gd2_part);

/* Weight gradients of the backward (loss.backward() of parts/train_per_iretation.py:172 through the Linear layers of
 * EquivariantGraphNeuralNetwork.py:13-30): a reduction over ALL edges (or nodes) on the matrix cores,
 *     C[m][n] (+)= scale * sum_e A[e][m] * B[e][n],   m < rows, n < cols,
 * A [E, lda] and B [E, ldb] row-major bf16 with the reduction index as ROWS (the operands as the other backward kernels
 * leave them: dL/da2 and the activations s1; dL/da1 and the gathered inputs), C fp32 with leading dimension ldc.  M and N are
 * the operand widths the kernel reads (M % 256 == 0, N % 128 == 0, M <= lda, N <= ldb; columns beyond rows / cols are
 * computed and dropped), split over slices of E whose fp32 partial tiles go through d_workspace
 * (egnn_gemm_tn_workspace_bytes) and are added in slice order: deterministic.  Replaces torch.mm / bmm (round 2).
 * Reads and writes: d_A and d_B are 16-byte aligned, lda and ldb multiples of 8.  Rows at and past E of a taller buffer are
 * never read, nor are columns at and past M / N.  Columns rows..M-1 of A and cols..N-1 of B (the padding inside the operand
 * width) are read and may hold anything, NaN included: column m of A only ever meets row m of C.  Of C exactly the elements
 * [0, rows) x [0, cols) are written (ldc >= cols; everything else in a wider or taller C is left alone), and of the
 * workspace only its first egnn_gemm_tn_workspace_bytes(E, M, N) bytes. */
size_t egnn_gemm_tn_workspace_bytes(int E, int M, int N);
int egnn_gemm_tn_bf16(void* stream, int E, int M, int N, const void* d_A, int lda, const void* d_B, int ldb, float scale,
                      float* d_C, int ldc, int rows, int cols, int accumulate, void* d_workspace, size_t workspace_bytes);

/* First-layer dgrad of the backward (autograd through the first Linear of mlp_x / mlp_m, :13, :19): a row-streaming product
 *     out[e][n] = sum_c A0[e][c] W0[c][n] + sum_c A1[e][c] W1[c][n],   n < 128,
 * A0 / A1 row-major bf16 [E, lda] (dL/da1 of the two MLPs; A1 may be NULL), out bf16 [E, ldo] (128 columns written);
 * W0 / W1 are fragment packs made by egnn_gemm_rows_pack from fp32 [K, ldw] matrices whose first ncols columns are used:
 * K * 128 bf16 per chunk of 128 columns, chunk after chunk (ceil(ncols / 128) chunks).  K % 64 == 0.  n_chunks column chunks
 * run in ONE launch (out columns 128 j .. 128 j + 127 from chunk j of both packs; ldo >= 128 n_chunks): the node MLP's
 * backward products are 8 chunks wide over only N / 256 row blocks.  Replaces torch.mm + addmm_ (round 2).
 * Reads and writes: A0, A1 and the packs are 16-byte aligned, lda0 and lda1 multiples of 8.  Rows at and past E and columns at
 * and past K0 / K1 of the operands are never read.  Of out, rows [0, E) x columns [0, 128 n_chunks) are written, ALL of them
 * (columns ncols..128 n_chunks-1 receive the zeros of the pack's padding), nothing else.  A bf16 out is stored in 16-byte
 * pieces: 16-byte aligned base and ldo % 8 == 0; an fp32 out element by element: ldo % 4 == 0.
 * egnn_gemm_rows_pack reads the first ncols columns of its K rows of d_W only (ldw >= ncols; the rest may hold anything) and
 * writes K * 128 * ceil(ncols / 128) bf16. */
int egnn_gemm_rows_pack(void* stream, int K, int ncols, const float* d_W, int ldw, void* d_frags_out);
int egnn_gemm_rows_bf16(void* stream, int E, const void* d_A0, int lda0, int K0, const void* d_W0, const void* d_A1, int lda1,
                        int K1, const void* d_W1, void* d_out, int ldo, int out_f32 /* fp32 [E, ldo] output */, int n_chunks);

/* EquivariantGNN.forward(edge_index, h, x) -> (h_L, x_L) (:85-88): all L layers. */
int egnn_forward(egnn_ctx* ctx, void* stream, int prec, int norm_scope,
                 const float* d_h, const float* d_x, float* d_h_out, float* d_x_out);

/* epsilon extraction of the callers (parts/train_per_iretation.py:161-163, :367-369):
 * eps_x = remove_mean(x_L - x_in), eps_h = h_L[:, :A].  d_graph_ptr int32[B+1] gives per-graph
 * means (remove_mean(x, batch_index), diffusion_x_h.py:9-13); NULL = one mean over all N nodes
 * (:6-8). */
int egnn_eps(void* stream, int N, int H, int A, const int32_t* d_graph_ptr, int B, const float* d_h_out,
             const float* d_x_out, const float* d_x_in, float* d_eps_x, float* d_eps_h);

/* remove_mean(x, batch_index) (diffusion_x_h.py:5-14) on [N,D], out of place. */
int egnn_remove_mean(void* stream, int N, int D, const int32_t* d_graph_ptr, int B, const float* d_in,
                     float* d_out);

/* ---- diffusion process ----------------------------------------------------------------- */
/* polynomial_schedule + clip_noise_schedule (diffusion_x_h.py:92-106) evaluated on the host in
 * fp32 in the same operation order.  alpha/sigma: float[T+1]; table: float[(T+1)*4] rows
 * {1/alpha_ts, sigma2_ts/(alpha_ts*sigma_t), std, t/T}; row 0 = final decode constants
 * {1/alpha_0, sigma_0/alpha_0, sigma_0/alpha_0, 0} (train_per_iretation.py:416-426).
 * Any of the three outputs may be NULL. */
int schedule_table_build(int T, double s, double power, float* alpha, float* sigma, float* table);
/* same table from explicit alpha/sigma arrays (learned gamma schedule, diffusion_x_h.py:36-46) */
int schedule_table_from_alpha(int T, const float* alpha, const float* sigma, float* table);

/* reverse_diffuse_one_step(z, eps, t, mode) (diffusion_x_h.py:75-90) with the step constants
 * c = {1/alpha_ts, sigma2_ts/(alpha_ts sigma_t), std}:  z_out = z*c0 - eps*c1 + c2*noise, noise
 * mean-removed (per graph if d_graph_ptr, else over all nodes) when mode_pos != 0.  d_noise supplies
 * the N(0,1) draw (the reference uses torch's global RNG).  z is [N, D] with row stride ldz.
 * With (c0, c1, c2) = (alpha_t, 0, sigma_t) the same kernel is diffuse_zero_to_t (:51-59). */
int ddpm_reverse_step(void* stream, int N, int D, int mode_pos, const int32_t* d_graph_ptr, int B,
                      float c0, float c1, float c2, const float* d_z, int ldz, const float* d_eps,
                      const float* d_noise, float* d_z_out, int ldo);

/* ---- device-resident sampler (generate(), parts/train_per_iretation.py:264-444) ---------- */
/* Allocates sampler state for the current graph: pos [N,3], h [N,H] = [s*x_types | cond | t/T].
 * d_cond [N, H-A-1] is the constant conditioning block ([compressed spectrum | exO]); d_table is
 * the DEVICE copy of schedule_table_build's table.  Noise comes from a counter-based Philox
 * generator keyed by (seed, step, node, component) unless d_noise_* are given to
 * egnn_sampler_step. */
int egnn_sampler_prepare(egnn_ctx* ctx, int T, int A, float onehot_scale, const float* d_table,
                         const float* d_cond, uint64_t seed);
/* x_only = 1 selects the x-only reverse loop of the reference's test.py:253-279 (process of E3diffusion_new.py:63-98):
 * the atom types given to egnn_sampler_init stay FIXED, only the positions take reverse steps (mu in the x_hat form is
 * algebraically the mu of diffusion_x_h.py:61-73, so the same step table serves both), and the loop ends with the reverse
 * step at t = 1: there is no t = 0 decode (egnn_sampler_final refuses; read egnn_sampler_state).  0 (default) = x and h. */
int egnn_sampler_set_mode(egnn_ctx* ctx, int x_only);
/* x_T ~ N(0,I) mean-removed per graph, h_T ~ N(0,I) (:301-305); or copy from the given arrays */
int egnn_sampler_init(egnn_ctx* ctx, void* stream, const float* d_pos_init, const float* d_x_init);
/* run `nsteps` reverse steps starting at the sampler's current t (initially T), optionally
 * replaying a captured hipGraph of one step; explicit noise arrays [nsteps][N][3] / [nsteps][N][A]
 * (step-major, first entry = highest t) may be NULL. */
int egnn_sampler_run(egnn_ctx* ctx, void* stream, int prec, int norm_scope, int nsteps,
                     int use_graph, const float* d_noise_pos, const float* d_noise_h);
/* final t=0 decode (:391-428): pos_0, continuous h_0, argmax one-hot (int32 [N,A]) */
int egnn_sampler_final(egnn_ctx* ctx, void* stream, int prec, int norm_scope,
                       const float* d_noise_pos, const float* d_noise_h,
                       float* d_pos_out, float* d_hc_out, int32_t* d_onehot_out);
/* current state + sticky per-graph non-finite flags (int32[B]; :376-389, :431-434) */
int egnn_sampler_state(egnn_ctx* ctx, void* stream, float* d_pos, float* d_x_types,
                       int32_t* d_bad_flags, int* t_host);

/* The same three fused kernels (x_T/h_T draw, one reverse step :366-373, t = 0 decode :412-428) on CALLER-owned state,
 * for the sampler of ONE LARGE GRAPH whose receiving nodes are partitioned over ranks (BASELINE configs[4]): between
 * two steps the EGNN forward runs stage-wise (egcl_forward_begin / _end) with collectives in between, so the loop is
 * driven by the caller and every rank applies the step to its replicated copy of the state (Philox noise is keyed by
 * (seed, step, GLOBAL node id): identical on every rank).  pos [N,3] and h [N,H] = [s*x_types | cond | t/T] are updated
 * in place; bad int32[B] is the sticky non-finite flag; d_noise_* (this step's draws, [N,3] / [N,A]) may be NULL. */
int ddpm_sampler_init(void* stream, int N, int H, int A, int B, int T, const int32_t* d_graph_ptr, const float* d_table,
                      float onehot_scale, uint64_t seed, const float* d_cond, const float* d_pos_init,
                      const float* d_x_init, float* d_pos, float* d_h, int32_t* d_bad);
int ddpm_sampler_step(void* stream, int N, int H, int A, int B, int T, int t, const int32_t* d_graph_ptr,
                      const float* d_table, float onehot_scale, uint64_t seed, const float* d_h_out, const float* d_x_out,
                      const float* d_noise_pos, const float* d_noise_h, float* d_pos, float* d_h, int32_t* d_bad);
int ddpm_sampler_final(void* stream, int N, int H, int A, int B, int T, const int32_t* d_graph_ptr, const float* d_table,
                       float onehot_scale, uint64_t seed, const float* d_h_out, const float* d_x_out,
                       const float* d_noise_pos, const float* d_noise_h, float* d_pos, float* d_h, int32_t* d_bad,
                       float* d_pos_out, float* d_hc_out, int32_t* d_onehot_out);

/* ---- graph construction ----------------------------------------------------------
 * Fully connected graphs in the edge kernels' CSR layout: node i receives from every j != i of its graph,
 * j ascending -- the edge set and order of parts/train_per_iretation.py:308-313 /
 * split_to_train_and_test.py:88-92 with PyG collate offsets.  d_edge_base int64[B] = number of edges of
 * the graphs before g (host prefix sum of n(n-1)); edge arrays may be NULL to fill row_ptr only. */
int egnn_fc_graph_build(void* stream, int N, int B, const int32_t* d_graph_ptr, const int32_t* d_node_graph,
                        const int64_t* d_edge_base, int32_t* d_row_ptr, int32_t* d_edge_dst, int32_t* d_edge_src);
/* Radius graph (not a reference feature; BASELINE configs[4]): pass 1 counts neighbours with |x_i-x_j| < r
 * inside each graph, the caller prefix-sums deg into row_ptr, pass 2 fills the CSR edge list. */
int egnn_radius_graph_count(void* stream, int N, const float* d_x, const int32_t* d_graph_ptr,
                            const int32_t* d_node_graph, float radius, int32_t* d_deg);
int egnn_radius_graph_fill(void* stream, int N, const float* d_x, const int32_t* d_graph_ptr,
                           const int32_t* d_node_graph, float radius, const int32_t* d_row_ptr,
                           int32_t* d_edge_dst, int32_t* d_edge_src);

/* ---- evaluation statistics -------------------------------------------------------
 * RDF(position, sigma, R, dR, Normalize) about atom 0 of every graph (evaluate_RDF.py:39-60), out
 * float[B, nbins], nbins = number of entries of np.arange(dR, R + dR, dR).  R and dR are doubles: the bin edges are
 * numpy's float64 values (rounded to float32 only inside the reference's `r < d < r + dR` comparison). */
int egnn_rdf(void* stream, int B, const float* d_pos, const int32_t* d_graph_ptr, double R, double dR, float sigma,
             int normalize, int nbins, float* d_out);
/* Si-O-Si selection + CN2 angle / bond lengths (evaluate_Si-O-Si.py:23-53, CN2_evaluate.py:12-21):
 * out float[B,4] = {valid, angle in degrees, |r1-r0|, |r2-r0|}; onehot int32 [N, A], Si = [0,1]. */
int egnn_si_o_si(void* stream, int B, int A, const float* d_pos, const int32_t* d_onehot,
                 const int32_t* d_graph_ptr, float cutoff, float* d_out);

/* ---- structural RMSD evaluation (csrc/eval/kabsch.hip) ---------------------------------------------------
 * Batched Kabsch fit of P onto Q (both [N,3], graphs through d_graph_ptr int32[B+1] as for egnn_rdf), one wavefront per graph,
 * fp64 inside.  The reference has three spellings that differ in the centre and in the reflection fix:
 *   kabsch_torch  (evaluate_rmsd_for_pos_generate.py:11-51; what def_for_main.py:82,101 call)  CENTROID + FLIP_COLUMN
 *   kabsch_numpy  (evaluate_rmsd_for_pos_generate.py:53-92)                                     CENTROID + FLIP_ROW
 *   kabsch_numpy  (evaluate_rmsd.py:10-42, create_xyz.py:48-80)                                 FIRST    + FLIP_ROW
 * FLIP_ROW (`Vt[-1, :] *= -1`) is the textbook fix: the optimal proper rotation.  FLIP_COLUMN (`Vt[:, -1] *= -1`) returns
 * diag(1,1,-1) V U^T in a reflection case: a proper rotation, not the optimal one.  Where H = p^T q is rank deficient (two
 * atoms; three atoms about their centroid; planar sets: sigma_3 <= 1e-12 sigma_1) the reference's answer in a reflection case
 * depends on LAPACK's choice of null vector; the device result there is the optimal proper rotation for BOTH flips, with missing
 * singular directions completed by a fixed rule (csrc/eval/kabsch_math.h).
 * d_out float[B,16] per graph: R [3,3] row-major (R p_i ~ q_i), t [3] = c_Q - c_P (the centroids, or Q[0] - P[0] for FIRST),
 * rmsd = sqrt(sum |R p - q|^2 / n) computed as that residual, then the number of rows of d_x_p / d_x_q (int32 [N,A], both or
 * neither NULL) equal to one-hot O = [1, 0, ...] (the atom-type counts of def_for_main.py:103-111), and 0. */
enum { EGNN_KABSCH_CENTROID = 0, EGNN_KABSCH_FIRST = 1 };
enum { EGNN_KABSCH_FLIP_ROW = 0, EGNN_KABSCH_FLIP_COLUMN = 1 };
int egnn_kabsch(void* stream, int B, const float* d_P, const float* d_Q, const int32_t* d_graph_ptr, int center, int flip,
                const int32_t* d_x_p, const int32_t* d_x_q, int A, float* d_out);
/* The same fit after a reordering of P: row i of a graph's fit is row d_order[lo + i] of its P (d_order int32 [N], indices local
 * to the graph: the form in which egnn_kabsch_perm returns an ordering and egnn_assign a matching); d_order NULL is the
 * identity.  The caller passes a permutation of every graph's rows; egnn_kabsch_perm and egnn_assign leave the rows of graphs
 * they did not search / solve unwritten, so the identity has to be filled in there.  As a guard of ADDRESSES only, a graph whose
 * ordering holds an index outside [0, n) is fitted in identity order (no such index is used as an address); an in-range ordering
 * that is no permutation is fitted as it stands.  No atom-type counts: d_out[13..15] = 0. */
int egnn_kabsch_ordered(void* stream, int B, const float* d_P, const float* d_Q, const int32_t* d_graph_ptr,
                        const int32_t* d_order, int center, int flip, float* d_out);
/* Gradient of egnn_kabsch / egnn_kabsch_ordered with respect to P and Q, so that the RMSD (train_2024_11.py:233-236) or any
 * function of (R, t, rmsd) can be a loss term: one launch, one wavefront per graph, fp64 inside, nothing kept from the forward
 * (centres, H, the fit and the residual are recomputed), no atomics, bitwise reproducible.  d_gout float[B,16] in the forward's
 * layout: dL/dR [9], dL/dt [3], dL/drmsd; the rest is not read.  d_dP float[N,3] and d_dQ float[N,3] (or NULL) are fully written
 * for every graph with n >= 1 (the d_dP row of fit row i is row d_order[lo + i]; a d_order with repeated indices leaves rows
 * unwritten and the repeated rows unspecified).  Defined where autograd through an SVD returns NaN or inf: rmsd = 0 contributes no rmsd gradient; a pair of
 * singular values whose sum (difference, in a FLIP_ROW reflection case) is at most 1e-12 sigma_1 contributes nothing (the
 * forward completes such directions by a fixed rule); one-atom graphs get zeros. */
int egnn_kabsch_backward(void* stream, int B, const float* d_P, const float* d_Q, const int32_t* d_graph_ptr,
                         const int32_t* d_order, int center, int flip, const float* d_gout, float* d_dP, float* d_dQ);
/* Host statement of egnn_kabsch_backward for ONE pair, everything in double, HOST pointers, no GPU: the same 3x3 numerics
 * (csrc/eval/kabsch_math.h) in plain C++.  P, Q [n,3]; g_R [9] and g_t [3] may be NULL (zero); dP [n,3]; dQ [n,3] or NULL. */
int egnn_kabsch_grad_host(int n, const double* P, const double* Q, int center, int flip, const double* g_R, const double* g_t,
                          double g_rmsd, double* dP, double* dQ);
/* Correspondence search of evaluate_rmsd.py:93-107: per graph with 2 <= n <= max_atoms (max_atoms <= 12) the minimum over all
 * orderings [0] + perm(1..n-1) of the rows of P (the generated structure) of the FIRST + FLIP_ROW RMSD against Q (the original).
 * Orderings are ranked in fp64 by the trace of their optimal proper rotation (atom 0 is the centre of every ordering, so this
 * is arg min RMSD without a difference of large numbers); equal scores go to the lexicographically first ordering
 * (itertools.permutations order: the reference keeps the first strict minimum); the result is bitwise reproducible.
 * Outputs per searched graph: d_min_rmsd [B] (residual of the winner), d_order int32 [N] (ragged through d_graph_ptr:
 * row i of the result is row order[i] of P), d_R [B,9] (rotation of the winner), d_searched int32 [B] = 1.  Graphs with
 * n < 2 or n > max_atoms cost no work: d_searched = 0 and their other outputs are not written.  1 <= B <= 65535 per call.
 * d_workspace: egnn_kabsch_perm_workspace_bytes(B, max_atoms) bytes of device memory (the workgroups' partial results). */
size_t egnn_kabsch_perm_workspace_bytes(int B, int max_atoms);
int egnn_kabsch_perm(void* stream, int B, const float* d_P, const float* d_Q, const int32_t* d_graph_ptr, int max_atoms,
                     float* d_min_rmsd, int32_t* d_order, float* d_R, int32_t* d_searched, void* d_workspace,
                     size_t workspace_bytes);

/* ---- atom matching of large graphs (csrc/eval/assign.hip) --------------------------------------------------
 * What create_xyz.py:157-192 computes for graphs of six atoms or more before it writes files: a pre-alignment on the four atoms
 * nearest to atom 0, a linear sum assignment on the distance matrix of all atoms, and (through egnn_kabsch, FIRST + FLIP_ROW, on
 * the reordered rows) the RMSD of the matched pair.  Both entries: caller-owned buffers, graphs through d_graph_ptr int32[B+1],
 * one workgroup per graph, 1 <= B <= 2147483647 (grid x), no workspace, no allocation, copy or synchronisation.
 *
 * egnn_assign replaces hungarian_algorithm (create_xyz.py:82-85, called at :182): per graph with 1 <= n <= max_atoms
 * (max_atoms <= EGNN_ASSIGN_MAX_ATOMS) the permutation col that minimises sum_i |P_i - Q_col[i]|, by an exact
 * shortest-augmenting-path solver with fp64 duals.  A cost entry is the fp32 norm of the fp32 coordinate difference,
 * sqrtf((dx*dx + dy*dy) + dz*dz), widened to fp64 -- what numpy.linalg.norm on float32 arrays hands to scipy; the matrix is
 * never stored.  Rows are augmented in index order and equal path costs go to the lowest column index: where the optimum is
 * unique the result is scipy.optimize.linear_sum_assignment's col_ind (its row_ind is 0..n-1), where it is not, one optimal
 * assignment, always the same one, bitwise, wherever the graph sits in the batch.
 * Outputs per solved graph: d_col int32 [N] (ragged through d_graph_ptr: row i of P is matched to row col[i] of Q, local
 * indices), d_cost double [B] (the sum above, fp64), d_solved int32 [B] = 1.  Graphs with n < 1 or n > max_atoms cost no work,
 * graphs with non-finite coordinates have no optimum: d_solved = 0 and their other outputs are not written.  Graphs of up to 64
 * atoms run on one wavefront; pass max_atoms <= 64 where no graph is larger (64-thread workgroups, 2 KB of LDS). */
#define EGNN_ASSIGN_MAX_ATOMS 1024
int egnn_assign(void* stream, int B, const float* d_P, const float* d_Q, const int32_t* d_graph_ptr, int max_atoms,
                int32_t* d_col, double* d_cost, int32_t* d_solved);
/* egnn_assign_prealign replaces create_xyz.py:158-176 (with return_near_from_exO, :87-96): per graph with n >= min_atoms
 * (min_atoms >= 5) the four atoms nearest to atom 0 of d_orig and of d_gen (ascending distance, equal distances to the lower
 * index, as the reference's stable sort), the 24 FIRST + FLIP_ROW fits of [gen[0], gen[idx_gen[perm[0..3]]]] onto
 * [orig[0], orig[idx_orig[0..3]]] in itertools.permutations(range(4)) order, fp64, and the rotation of the smallest five-point
 * RMSD, equal values to the first permutation.  d_R float [B,9] row-major: R (gen_i - gen_0) ~ orig_i - orig_0, i.e. the
 * reference's aligned_generated_pos (:177-181) is (gen - gen[0]) R^T.  d_prealigned int32 [B] = 1; graphs with n < min_atoms
 * (or without four finite neighbour distances, or with no pairing of finite residual) get 0 and their R is not written. */
int egnn_assign_prealign(void* stream, int B, const float* d_orig, const float* d_gen, const int32_t* d_graph_ptr, int min_atoms,
                         float* d_R, int32_t* d_prealigned);

/* ---- whole-structure statistics (csrc/eval/structure.hip; definitions in csrc/eval/structure_math.h) --------------------
 * The reference judges a structure by what surrounds atom 0: the RDF about it (evaluate_RDF.py:39-60), the atoms bonded to it
 * (evaluate_Si-O-Si.py:23-41) and the angle they make (CN2_evaluate.py:12-21).  These entries take the same three statistics
 * over EVERY centre of every graph, by atom type.  Atoms carry a type index d_type int32 [N] in [0, A), A <= 4; graphs through
 * d_graph_ptr int32 [B+1]; max_atoms is the size of the largest graph, at most 32768 (the ordered pairs of one graph are counted
 * in int32).  d_tiles int32 [n_tiles, 3] lists the work, one workgroup each, built from the graph sizes by the caller:
 *   pair tiles  {g, c0, j0}: centres c0 .. c0+63 against neighbour atoms j0 .. j0+1023 of graph g (local indices), every
 *               (multiple of 64, multiple of 1024) below the graph's size once;
 *   bond tiles  {g, c0, 0}:  centres c0 .. c0+7 of graph g, every multiple of 8 below its size once.
 * A kernel checks every entry against d_graph_ptr and reads no atom outside its graph; a tile listed twice is counted twice.
 * All accumulators are integers (LDS atomics, then one global atomicAdd per non-zero bin): bitwise reproducible.  The outputs
 * are zeroed by the call.  Bad arguments (nbins > 1024, A > 4, dtheta below 0.5 degrees = more than 361 angle bins, cutoff <= 0,
 * max_cn outside [1, 64], max_atoms > 32768) return EGNN_EINVAL before anything is launched.
 *
 * egnn_struct_pair_counts generalises length_from_exO + the counting loop of RDF (evaluate_RDF.py:39-56): d_counts int32
 * [B, A, A, nbins], c[g][a][b][k] = number of ordered pairs i != j of graph g with type(i) = a, type(j) = b and the float32
 * distance sqrtf((dx*dx + dy*dy) + dz*dz) in bin k by egnn_rdf's rule, (float)(dR + k dR) < d < (float)(dR + k dR + dR). */
int egnn_struct_pair_counts(void* stream, int B, int A, const float* d_pos, const int32_t* d_type, const int32_t* d_graph_ptr,
                            int max_atoms, const int32_t* d_tiles, int n_tiles, double dR, int nbins, int32_t* d_counts);
/* egnn_struct_bonds generalises the neighbour selection of evaluate_Si-O-Si.py:23-41 (j is bonded to i iff the float32 distance
 * is below cutoff) and calculate_angle_for_CN2 (CN2_evaluate.py:12-16), one wavefront per centre:
 *   d_cn int32 [B, A, A, max_cn+1]: cn[g][a][b][m] = centres of type a with m bonded neighbours of type b, m clamped to max_cn
 *     (the last bin means "max_cn or more");
 *   d_angles int32 [B, A, A(A+1)/2, nth], nth = floor(180/dtheta + 0.5) + 1: for centre i of type a and bonded neighbours j < k
 *     of types (b <= c, pair index b A - b(b-1)/2 + c - b) the angle between the bond vectors, fp64 from the float32 positions,
 *     in the bin floor(theta/dtheta + 0.5) CENTRED on a multiple of dtheta; a zero-length bond has no angle;
 *   d_overflow int32 [B]: centres with more than 64 bonds; they are counted in d_cn, their angles are not taken. */
int egnn_struct_bonds(void* stream, int B, int A, const float* d_pos, const int32_t* d_type, const int32_t* d_graph_ptr,
                      int max_atoms, const int32_t* d_tiles, int n_tiles, float cutoff, double dtheta, int max_cn, int32_t* d_cn,
                      int32_t* d_angles, int32_t* d_overflow);
/* egnn_struct_rdf_finish generalises the normalisation and smoothing of RDF (evaluate_RDF.py:50-57): d_out float [B, A, A, nbins],
 * g_ab(r_k) = gaussian_filter1d(c[g][a][b][.] / max(n_a, 1) / (4 pi rho r_k^2 dR), sigma) with rho = n / (4/3 pi R^3) over ALL
 * atoms of the graph, fp64 inside.  The sum over b is the mean over the centres i of type a of RDF(roll(position, i)); an absent
 * type gives rows of zeros. */
int egnn_struct_rdf_finish(void* stream, int B, int A, const int32_t* d_counts, const int32_t* d_type, const int32_t* d_graph_ptr,
                           double R, double dR, double sigma, int nbins, float* d_out);
/* Host statement of egnn_struct_pair_counts + egnn_struct_bonds (evaluate_RDF.py:39-60, CN2_evaluate.py:12-21,
 * evaluate_Si-O-Si.py:23-41 over every centre): HOST pointers, no GPU, no tiles, the same definitions in plain C++.  overflow may be
 * NULL.  Types outside [0, A) and graphs above 32768 atoms are EGNN_EINVAL. */
int egnn_struct_counts_host(int B, int A, const float* pos, const int32_t* type, const int32_t* graph_ptr, double dR, int nbins,
                            float cutoff, double dtheta, int max_cn, int32_t* counts, int32_t* cn, int32_t* angles,
                            int32_t* overflow);

/* ---- topological fingerprint (csrc/eval/topo.hip; definitions in csrc/eval/topo_math.h) ------------------------------------
 * evaluate_fingerprint.py:99-114 scores a sample by its bonding network: bonds guessed from distances (guess_bonds, :49-84),
 * RDKit's atom-pair fingerprint of the bond graph, Tanimoto similarity.  These entries restate it for a ragged batch without ASE
 * or RDKit.  Atoms carry a type index d_type int32 [N] in [0, A), A <= 4; graphs through d_graph_ptr int32 [B+1] over N atoms;
 * max_atoms is the size of the largest graph, at most 1024 (EGNN_ASSIGN_MAX_ATOMS).  Atom indices in every list count over the
 * whole batch (0 .. N-1).  All sums are integers: the outputs are bitwise reproducible and equal to egnn_topo_host's.  Bad
 * arguments (A > 4, max_atoms > 1024, L outside [1, 64], a threshold that is not positive and finite, a required pointer NULL)
 * return EGNN_EINVAL before anything is launched; a kernel ignores a type outside [0, A) (the atom bonds to nothing).
 *
 * egnn_topo_bonds: i != j of one graph are bonded iff d < thr[type i][type j], d = sqrt((dx*dx + dy*dy) + dz*dz) in fp64 from the
 * float32 positions; thr is a HOST table double [A][A] (scale * (radius_a + radius_b), computed once by the caller).
 *   d_degree int32 [N]:      bonds of each atom, all of them;
 *   d_row_ptr int32 [N+1]:   exclusive prefix sum of min(degree, 32);
 *   d_neighbours int32:      the caller allocates 32 N entries; row i holds the first min(degree, 32) neighbours, ascending;
 *   d_overflow int32 [B]:    atoms of the graph with more than 32 bonds.  Such a graph has no distances and no fingerprint.
 * d_row_ptr is one workgroup's prefix sum, ceil(N / 1024) degrees per thread: meant for evaluation batches (tens of thousands of
 * atoms); N up to 2^26 is accepted and correct, but that sum then runs on one CU. */
int egnn_topo_bonds(void* stream, int B, int N, int A, const float* d_pos, const int32_t* d_type, const int32_t* d_graph_ptr,
                    int max_atoms, const double* thr, int32_t* d_row_ptr, int32_t* d_neighbours, int32_t* d_degree,
                    int32_t* d_overflow);
/* egnn_topo_paths: one breadth-first search per atom over the lists of egnn_topo_bonds, one workgroup per graph.  Each output may
 * be NULL:
 *   d_dist uint16:           graph g's [n, n] hop distances (bonds on a shortest path, never capped) from element d_dist_ptr[g]
 *                            on (int64 [B], the caller's prefix sum of n^2); 0xFFFF = unreachable;
 *   d_component int32 [N]:   the lowest atom index reachable from i;   d_fragments int32 [B]: connected components;
 *   d_fp int32 [B, K]:       atom-pair counts, K = C (C+1)/2 * L with C = 7 A: for i < j with 1 <= d <= L,
 *                            ++fp[(c_lo C - c_lo (c_lo-1)/2 + c_hi - c_lo) L + d - 1], class = type * 7 + degree % 7.  Zeroed by the call.
 * A graph with d_overflow[g] != 0 gets distances 0xFFFF, components -1, fragments -1 and a zero fingerprint; a graph of no atoms
 * gets fragments 0 and a zero fingerprint. */
int egnn_topo_paths(void* stream, int B, int N, int A, const int32_t* d_type, const int32_t* d_graph_ptr, int max_atoms,
                    const int32_t* d_row_ptr, const int32_t* d_neighbours, const int32_t* d_degree, const int32_t* d_overflow, int L,
                    uint16_t* d_dist, const int64_t* d_dist_ptr, int32_t* d_component, int32_t* d_fragments, int32_t* d_fp);
/* egnn_topo_tanimoto: pair p compares row d_pairs[2p] of d_fp_a [rows_a, K] with row d_pairs[2p+1] of d_fp_b [rows_b, K]
 * (d_pairs int32 [n_pairs, 2]; NULL = row p with row p): both = sum min, sa = sum a, sb = sum b in int64,
 * d_sim double [n_pairs] = both / (sa + sb - both) as one fp64 division, 0.0 where the denominator is 0; d_sa, d_sb int64 [n_pairs].
 * A pair that names no row gets sim 0, sa = sb = -1. */
int egnn_topo_tanimoto(void* stream, int n_pairs, int K, const int32_t* d_fp_a, int rows_a, const int32_t* d_fp_b, int rows_b,
                       const int32_t* d_pairs, double* d_sim, int64_t* d_sa, int64_t* d_sb);
/* Host statement of the three entries above: HOST pointers, no GPU, the same definitions in plain C++.  dist is contiguous (graph
 * g's block follows graph g-1's); dist, component, fragments and fp may be NULL; the n_pairs pairs name rows of fp itself.
 * Types outside [0, A) and graphs above 1024 atoms are EGNN_EINVAL. */
int egnn_topo_host(int B, int A, const float* pos, const int32_t* type, const int32_t* graph_ptr, const double* thr, int L,
                   int32_t* row_ptr, int32_t* neighbours, int32_t* degree, int32_t* overflow, uint16_t* dist, int32_t* component,
                   int32_t* fragments, int32_t* fp, int n_pairs, const int32_t* pairs, double* sim, int64_t* sa, int64_t* sb);

/* ---- shortest-path ring statistics (csrc/eval/rings.hip; definitions in csrc/eval/rings_math.h) ----------------------------
 * The medium-range order of a network: for every angle (p, q), p < q, of positions in the bond-list row of a centre c, the size of
 * the smallest ring through it (King's shortest-path criterion, per angle as Rino et al. apply it) and the number of shortest
 * closing paths.  No reference file computes rings: an extension beyond the reference.  The input is a bond list in CSR form over
 * the N atoms: d_row_ptr int32 [N+1], d_atom int32 [E], and for periodic cells d_shift int32 [E, 3], the lattice shift of every
 * bond, each component in {-1, 0, 1} (NULL for clusters).  A site is (atom, shift) of the infinite lattice: following bond e of
 * atom a from (a, s) leads to (d_atom[e], s + d_shift[e]); images are never folded.  d_centre int32 [M] indexes the atoms, any
 * order, repeats allowed; d_angle_ptr int32 [M+1] is the exclusive prefix sum of d (d - 1) / 2 over the centres' degrees d, and
 * n_angles its last entry.  A centre's angles are in lexicographic order of (p, q).
 *   d_size int32 [n_angles]:         2 + the bonds on a shortest path from site row[p] to site row[q] with the site (c, 0) removed
 *                                    (it counts ATOMS on the ring: a "6-membered" silica ring has size 12); 0 where no such path
 *                                    has size <= max_size; -1 where the search overflowed;
 *   d_count int32 [n_angles]:        the number of distinct shortest such paths, saturating at 2^31 - 1; 0 where size <= 0;
 *   d_overflow int32 [M]:            1 where a search of the centre labelled more than max_sites sites or the centre has more than
 *                                    32 bonds (all its angles -1), else 0;
 *   d_hist int32 [A, max_size + 1]:  angles by centre type (d_type int32 [N]) and size, bin 0 = no ring, overflowed angles not
 *                                    counted; or NULL.
 * 3 <= max_size <= 32; 1 <= max_sites <= 4096 (RING_MAX_SITES).  One workgroup per (centre, p) labels sites in an LDS hash table
 * of max(512, 2 max_sites rounded up to a power of two) * 12 + 4 max_sites bytes (112 KiB at 4096).  All outputs are integers,
 * bitwise reproducible and equal to egnn_rings_host's.  row_ptr, atom, shift and centre are HOST copies of the lists, each may be
 * NULL; those given are checked before anything is launched (a centre outside the atoms, a non-monotone row_ptr, a neighbour
 * outside [0, N), a shift outside {-1, 0, 1}: EGNN_EINVAL, as max_size, max_sites and NULL pointers outside their limits).  The
 * kernel trusts none of the device lists either way: it ignores a bond it cannot follow and a centre it cannot read. */
int egnn_rings(void* stream, int N, const int32_t* d_row_ptr, int E, const int32_t* d_atom, const int32_t* d_shift, const int32_t* d_type,
               int A, int M, const int32_t* d_centre, const int32_t* d_angle_ptr, int n_angles, int max_size, int max_sites, int32_t* d_size,
               int32_t* d_count, int32_t* d_overflow, int32_t* d_hist, const int32_t* row_ptr, const int32_t* atom, const int32_t* shift,
               const int32_t* centre);
/* Host statement of egnn_rings: HOST pointers, no GPU, the same definitions in plain C++.  Also EGNN_EINVAL: a type outside
 * [0, A), an angle_ptr that is not the prefix sum of d (d - 1) / 2 ending at n_angles. */
int egnn_rings_host(int N, const int32_t* row_ptr, int E, const int32_t* atom, const int32_t* shift, const int32_t* type, int A, int M,
                    const int32_t* centre, const int32_t* angle_ptr, int n_angles, int max_size, int max_sites, int32_t* size,
                    int32_t* count, int32_t* overflow, int32_t* hist);

/* ---- SOAP descriptors and spectrum template matching (csrc/eval/soap.hip; definitions in csrc/eval/soap_math.h) -------------
 * template_matching.py:41-68 finds, for every target record, the three reference records with the nearest XANES spectrum (MSE of
 * spectrum[0]) and reports the cosine similarity of dscribe's SOAP power spectrum of atom 0.  These entries restate it for a ragged
 * batch without ASE or dscribe, from the descriptor's definition (soap_math.h states every formula and every summation order).
 * Atoms and graphs as in the topo block: d_type int32 [N] in [0, A), A <= 4, d_graph_ptr int32 [B+1] over N atoms; species order
 * is type order.  The tables (K, gamma, beta, the harmonic norms and the l weights: egnn_soap_table_doubles(n_max, l_max) doubles in
 * the layout of soap_math.h) are built by the caller ONCE per configuration, exactly (the package: SoapBasis, mpmath at 60 digits).
 * No kernel has an atomic: a repeated call is bitwise reproducible.  Bad arguments (A > 4, n_max outside [1, 16], l_max outside
 * [0, 10], k outside [1, 8], a cut that is not positive and finite, a centre outside [0, N), a required pointer NULL) return
 * EGNN_EINVAL before anything is launched; a kernel ignores a type outside [0, A) (the atom contributes nothing).
 *
 * egnn_soap_features: F = (A n(n+1)/2 + A(A-1)/2 n^2)(l_max+1), 5,115 at A = 2, n_max = 15, l_max = 10; EGNN_EINVAL outside the limits. */
int egnn_soap_features(int A, int n_max, int l_max);
int egnn_soap_table_doubles(int n_max, int l_max);
/* egnn_soap_descriptor: one workgroup per centre.  centres is a HOST list int32 [n_centres] of atom indices counted over the batch,
 * in any order, repeats allowed (it is checked against N here), d_centres the same list on the device.  Neighbours of a centre are
 * the atoms of its graph with d2 < neighbour_cut^2, the centre included.
 *   d_desc double [n_centres, F]:                         the power spectrum, (Z1 <= Z2) outermost, then n, n' (n' >= n where Z1 = Z2), l innermost;
 *   d_coeff double [n_centres, A, n_max, (l_max+1)^2]:    the orthonormalised coefficients c[Z][n][l*l + l + m], or NULL.
 * Dynamic LDS: (A n_max (l_max+1)^2 + 32 ((l_max+1)^2 + n_max (l_max+1) + 4)) * 8 + 128 bytes, 136 KiB at the limits. */
int egnn_soap_descriptor(void* stream, int B, int N, int A, const float* d_pos, const int32_t* d_type, const int32_t* d_graph_ptr,
                         int n_max, int l_max, double neighbour_cut, const double* d_tables, int n_centres, const int32_t* centres,
                         const int32_t* d_centres, double* d_desc, double* d_coeff);
/* egnn_soap_cosine: pair p compares row d_pairs[2p] of d_a [rows_a, F] with row d_pairs[2p+1] of d_b [rows_b, F] (d_pairs int32
 * [n_pairs, 2]; NULL = row p with row p): d_cos double [n_pairs] = dot / (sqrt(sum a^2) sqrt(sum b^2)), every sum in the one order
 * of soap_math.h.  A pair that names no row gets NaN. */
int egnn_soap_cosine(void* stream, int n_pairs, int F, const double* d_a, int rows_a, const double* d_b, int rows_b,
                     const int32_t* d_pairs, double* d_cos);
/* egnn_soap_gram: d_gram double [rows_a, rows_b], every entry the value egnn_soap_cosine gives for that pair (bitwise); d_norms is a
 * workspace double [rows_a + rows_b] that receives the squared norms, computed once per row. */
int egnn_soap_gram(void* stream, int F, const double* d_a, int rows_a, const double* d_b, int rows_b, double* d_norms, double* d_gram);
/* egnn_spectrum_nearest: d_target float [T, S], d_reference float [R, S] -> for every target the k <= 8 references of smallest
 * mse = (sum_s ((double)t_s - (double)r_s)^2) / S, ascending, ties to the lower index: d_idx int32 [T, k], d_mse double [T, k]
 * (bitwise the host statement's); missing entries are index -1, mse +inf.  A reference whose group (d_reference_group int32 [R])
 * equals the target's (d_target_group int32 [T]) is skipped; a group < 0 matches nothing; both NULL = no exclusion.  One wavefront
 * per target streams the references: the [T, R] matrix is never stored. */
int egnn_spectrum_nearest(void* stream, int T, int R, int S, int k, const float* d_target, const float* d_reference,
                          const int32_t* d_target_group, const int32_t* d_reference_group, int32_t* d_idx, double* d_mse);
/* Host statement of the four entries above: HOST pointers, no GPU, the same definitions in plain C++.  Three parts, each skipped
 * where its count is 0: descriptors (n_centres > 0); cosines of the pairs and / or the whole matrix gram [n_a, n_b] of rows_a
 * [n_a, F] and rows_b [n_b, F] (n_pairs > 0 or gram given); nearest spectra (T > 0).  Also EGNN_EINVAL: a type outside [0, A), a
 * graph_ptr that does not run from 0 to N, a pair that names no row. */
int egnn_soap_host(int B, int N, int A, const float* pos, const int32_t* type, const int32_t* graph_ptr, int n_max, int l_max,
                   double neighbour_cut, const double* tables, int n_centres, const int32_t* centres, double* desc, double* coeff, int F,
                   const double* rows_a, int n_a, const double* rows_b, int n_b, int n_pairs, const int32_t* pairs, double* cosine,
                   double* gram, int T, int R, int S, int k, const float* target, const float* reference, const int32_t* target_group,
                   const int32_t* reference_group, int32_t* idx, double* mse);

/* ---- local environments of periodic cells (csrc/cells/cell_env.hip; definitions in csrc/cells/cell_math.h) ---------------
 * Every record of the reference is a local environment cut out of a periodic cell: make_dataset.py:79-142 builds the 3x3x3
 * supercell (:79-92), its full distance matrix (:99), takes the sites closer than 2.0 A to the excited oxygen
 * (return_index_within_2ang, :50-57, :101) and theirs in nested loops to 2NN / 3NN / 4NN (:103-107), and stores positions
 * relative to the centre (:111), for ONE centre per cell.  These entries make the same cut about ANY set of centres of a batch of
 * cells, on the infinite lattice (where the reference's search wraps round its supercell it aliases an image onto a far site;
 * INTEGRATION.md, "Periodic cells").
 *   cells    cell_ptr int32 [C+1] over N atoms, lattice double [C, 9] (rows a, b, c), frac double [N, 3] (any real value; wrapped
 *            to [0, 1) as f - floor(f), all shifts refer to the wrapped atoms), type int32 [N] in [0, A), A <= 4.  cell_ptr and
 *            lattice are given twice: HOST copies for the checks (sizes, a singular lattice, a perpendicular width below the
 *            cutoff -- with every width >= cutoff the 27 images s in {-1,0,1}^3 hold every bond) and device copies for the kernels.
 *   bond     site (j, s) != (i, 0) is bonded to atom i iff |(frac_j - frac_i + s) L|^2 < cutoff^2 in fp64, one fixed order.
 *   shift    code ((s_x + 4) 9 + (s_y + 4)) 9 + (s_z + 4) in [0, 729); 364 is no shift.
 *   tiles    d_tiles int32 [n_tiles, 2] = {cell, first centre}: 64 centres of a cell (local index, every multiple of 64 below
 *            its size once), one workgroup each, built by the caller; a kernel checks every entry.
 * Atom indices in every list count over the whole batch (0 .. N-1).  Bad arguments return EGNN_EINVAL, naming the cell where
 * one is at fault, before anything is launched.  Results are bitwise reproducible.
 *
 * egnn_cell_bonds_count / _fill replace the distance matrix of make_dataset.py:99 and return_index_within_2ang (:50-57) for every
 * atom: d_degree int32 [N] = bonds of each atom; the caller takes the exclusive prefix sum d_row_ptr int32 [N+1]; the fill pass
 * writes d_bond_atom / d_bond_shift int32 [n_bonds], every row ascending by (atom, shift code). */
int egnn_cell_bonds_count(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                          const double* d_lattice, const double* d_frac, double cutoff, const int32_t* d_tiles, int n_tiles,
                          int32_t* d_degree);
int egnn_cell_bonds_fill(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                         const double* d_lattice, const double* d_frac, double cutoff, const int32_t* d_tiles, int n_tiles,
                         const int32_t* d_row_ptr, int n_bonds, int32_t* d_bond_atom, int32_t* d_bond_shift);
/* egnn_cell_env_count / _fill replace the nested neighbour loops of make_dataset.py:101-107 (2NN), :177-188 (3NN) and :258-272
 * (4NN), and the positions of :111: for centre m (atom d_centre[m] of cell d_centre_cell[m]; any order, duplicates allowed)
 * the sites reachable in at most `shells` (1..4) bonds, the centre first, the others ascending by (atom, shift code).  One
 * wavefront per centre; at most max_atoms (1..1024) sites each.  The count pass writes d_size int32 [M]; a centre whose
 * environment exceeds max_atoms gets the sentinel max_atoms + 1, and a centre outside its cell 0.  The caller takes the prefix sum
 * d_env_ptr int32 [M+1] (sentinels counted as 0) and the fill pass writes, for every centre whose size equals its share of
 * d_env_ptr, d_env_atom, d_env_shift, d_env_type int32 [n_sites] and d_env_pos float [n_sites, 3] =
 * float((frac_j - frac_i + s) L), rounded once from fp64; other centres write nothing. */
int egnn_cell_env_count(void* stream, int C, int N, const int32_t* cell_ptr, const int32_t* d_cell_ptr, const int32_t* d_row_ptr,
                        int n_bonds, const int32_t* d_bond_atom, const int32_t* d_bond_shift, int M, const int32_t* d_centre_cell,
                        const int32_t* d_centre, int shells, int max_atoms, int32_t* d_size);
int egnn_cell_env_fill(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                       const double* d_lattice, const double* d_frac, const int32_t* d_type, const int32_t* d_row_ptr, int n_bonds,
                       const int32_t* d_bond_atom, const int32_t* d_bond_shift, int M, const int32_t* d_centre_cell,
                       const int32_t* d_centre, int shells, int max_atoms, const int32_t* d_env_ptr, int n_sites, int32_t* d_env_atom,
                       int32_t* d_env_shift, int32_t* d_env_type, float* d_env_pos);
/* Host statement of the four entries above (make_dataset.py:79-111 about every requested centre): HOST pointers, no GPU, no
 * tiles, the same definitions in plain C++.  bond_ptr int32 [N+1] and env_size int32 [M] are always written; the lists are written
 * where their pointers are given and bond_cap / env_cap hold them (call once with capacities 0 to learn the sizes).  An
 * environment above max_atoms has size max_atoms + 1 and no rows.  Also EGNN_EINVAL: a type outside [0, A), a coordinate that is
 * not finite, a centre outside its cell. */
int egnn_cell_env_host(int C, int A, const int32_t* cell_ptr, const double* lattice, const double* frac, const int32_t* type,
                       double cutoff, int M, const int32_t* centre_cell, const int32_t* centre, int shells, int max_atoms,
                       int32_t* bond_ptr, int64_t bond_cap, int32_t* bond_atom, int32_t* bond_shift, int32_t* env_size,
                       int64_t env_cap, int32_t* env_atom, int32_t* env_shift, int32_t* env_type, float* env_pos);

/* ---- real-space statistics of periodic cells (csrc/cells/cell_stats.hip; definitions in csrc/cells/cell_stats_math.h) ----------
 * The real-space counterpart of egnn_sq_cell_*: partial pair counts (-> g_ab(r), running coordination numbers), coordination
 * numbers, bond angles and the Q^n speciation of whole cells, on the infinite lattice.  An extension: the reference has these
 * statistics for one cluster about atom 0 only, and all three entries extend evaluate_RDF.py:39-60, evaluate_Si-O-Si.py:23-41 and
 * CN2_evaluate.py:12-16 to periodic cells.  Cells as in egnn_cell_bonds_* (cell_ptr and lattice given twice, HOST copies for
 * the checks); every accumulator is an integer and the results are bitwise reproducible, a cell giving the same bits in any batch.
 * Bad arguments return EGNN_EINVAL with a message, naming the cell where one is at fault, before anything is launched: dR <= 0,
 * nbins < 1, A > 4, A A nbins > 16384 (the LDS histogram), dtheta outside [0.5, 180], max_cn outside [1, 64], former or bridge
 * outside [0, A) or equal, a singular lattice, a cell that needs more than 16 images along an axis.
 *
 * egnn_cell_pair_counts extends the counting loop of evaluate_RDF.py:39-60 to periodic cells, about every centre: d_counts int64
 * [C, A, A, nbins], c[cell, a, b, k] = ordered pairs (i, (j, s)), s in Z^3, (j, s) != (i, 0), type(i) = a, type(j) = b, with
 * floor(|(frac_j - frac_i + s) L| / dR) = k < nbins in fp64 (bin k is [k dR, (k + 1) dR): NOT the open bins (dR + k dR, dR +
 * (k + 1) dR) of egnn_rdf and egnn_struct_pair_counts).  An atom pairs with its own images; c[a][b] == c[b][a] bitwise.  The image
 * box |s_k| <= ceil(nbins dR / w_k) (w: the perpendicular widths) holds every such pair.  d_tiles int32 [n_tiles, 5] = {cell, first
 * centre, first neighbour, piece, pieces}: 64 centres against 1024 neighbour atoms of a cell (local indices, every pair of
 * multiples once) and piece `piece` of `pieces` (1 <= pieces <= 33, each piece once) of the values of s_0; one workgroup each. */
int egnn_cell_pair_counts(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                          const double* d_lattice, const double* d_frac, const int32_t* d_type, double dR, int nbins,
                          const int32_t* d_tiles, int n_tiles, int64_t* d_counts);
/* egnn_cell_bond_stats extends the bond rule of evaluate_Si-O-Si.py:23-41 and the angle of CN2_evaluate.py:12-16 to periodic
 * cells, about every centre, over the bond list of egnn_cell_bonds_fill: d_coordination int32 [N, A] = bonds of each atom by
 * neighbour type; d_cn int64 [C, A, A, max_cn + 1] (the last bin: max_cn or more); d_angles int64 [C, A, A(A+1)/2, ntheta], bonded
 * pairs p < q of a row about centres of type a with neighbour types (b <= c) at index b A - b(b-1)/2 + c - b, angle in fp64 from
 * the site vectors, bin floor(theta / dtheta + 0.5), ntheta = floor(180 / dtheta + 0.5) + 1; d_qn int32 [N] = for an atom of type
 * `former` its bonds to atoms of type `bridge` that have two or more bonds to formers, -1 for every other atom; d_qn_hist int64
 * [C, max_cn + 1] (the last bin saturates); d_overflow int32 [C] = centres with more than 64 bonds: they count in d_coordination
 * and d_cn and give no angle.  d_tiles int32 [n_tiles, 2] = {cell, first centre}: 8 centres (local index, every multiple of 8 below
 * the cell's size once), one wavefront per centre. */
int egnn_cell_bond_stats(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                         const double* d_lattice, const double* d_frac, const int32_t* d_type, const int32_t* d_row_ptr, int n_bonds,
                         const int32_t* d_bond_atom, const int32_t* d_bond_shift, double dtheta, int max_cn, int former, int bridge,
                         const int32_t* d_tiles, int n_tiles, int32_t* d_coordination, int64_t* d_cn, int64_t* d_angles, int32_t* d_qn,
                         int64_t* d_qn_hist, int32_t* d_overflow);
/* Host statement of the two entries above (evaluate_RDF.py:39-60, evaluate_Si-O-Si.py:23-41 and CN2_evaluate.py:12-16 extended
 * to periodic cells): HOST pointers, no GPU, no tiles, the same definitions in plain C++; it builds the bond list of `cutoff`
 * itself (egnn_cell_env_host's).  The pair part runs where counts is given, the bond part where coordination is given (then all six
 * of its outputs are).  Also EGNN_EINVAL: a type outside [0, A), a coordinate that is not finite, a perpendicular width below the
 * cutoff (bond part). */
int egnn_cell_stats_host(int C, int A, const int32_t* cell_ptr, const double* lattice, const double* frac, const int32_t* type,
                         double dR, int nbins, int64_t* counts, double cutoff, double dtheta, int max_cn, int former, int bridge,
                         int32_t* coordination, int64_t* cn, int64_t* angles, int32_t* qn, int64_t* qn_hist, int32_t* overflow);

/* ---- linked-cell search of periodic cells (csrc/cells/cell_grid.hip; definitions in csrc/cells/cell_grid_math.h) ---------------
 * A second way to the outputs of egnn_cell_bonds_count / _fill and egnn_cell_pair_counts, bit for bit, whose cost grows with the
 * number of atoms and not with its square: the atoms of a cell are binned on a grid, sorted by (bin, atom index), and a centre is
 * tested against the (2 reach + 1)^3 bins about its own instead of against the whole cell.  An extension: no file of the reference
 * bins a cell; the statistics are those of make_dataset.py:50-57,99 (bonds) and evaluate_RDF.py:39-60 (pairs) as the entries above
 * extend them.  Whether a site (j, s) counts is decided by the text the direct kernels compile, so the two ways agree exactly.
 *   grid     nb int32 [C, 3] per cell, from egnn_cell_grid_dims: nb_k = floor(reach w_k / max(radius (1 + 1e-6), reach min_width)),
 *            at most 256 (w: the perpendicular widths); a cell with an axis below 2 reach + 1 bins is not griddable and has
 *            nb = 0, 0, 0: it takes no part here and is left to the direct entries.  1 <= reach <= 3.  nb is given twice (HOST copy
 *            for the checks, as cell_ptr and lattice are): an entry refuses a grid finer than its radius and reach allow.
 *   bins     d_bin_ptr int32 [C+1]: the first bin of every cell among the n_bins = sum nb_0 nb_1 nb_2 bins of the batch; the bin of
 *            an atom is (b_0 nb_1 + b_1) nb_2 + b_2 with b_k = min(nb_k - 1, floor(wrap(frac_k) nb_k)).
 *   sorted   the atoms of a gridded cell ascending by (bin, atom index), in the cell's own range of the batch: d_bin_start int32
 *            [n_bins + 1] counts the gridded atoms before each bin, d_sorted_atom int32 [N] (index into the batch, -1 in a cell
 *            that is not gridded), d_sorted_frac double [N, 3] (wrapped), d_sorted_type int32 [N].
 *   tiles    tiles / d_tiles int32 [n_tiles, 2] = {cell, first centre}: 64 consecutive SORTED centres of a gridded cell, given
 *            twice (HOST copy for the checks); a tile that names a cell with nb = 0 is EGNN_EINVAL.
 * Bad arguments return EGNN_EINVAL, naming the cell, before anything is launched.  Results are bitwise reproducible.
 *
 * egnn_cell_grid_dims (host only, no GPU): writes nb; a singular lattice is EGNN_EINVAL. */
int egnn_cell_grid_dims(int C, const double* lattice, double radius, int reach, double min_width, int32_t* nb);
/* egnn_cell_grid_count / _fill bin and sort a batch (count / prefix-by-caller / fill).  The count pass WRITES d_atom_bin int32 [N]
 * (-1 in a cell that is not gridded) and d_bin_count int32 [n_bins]; the caller takes the exclusive prefix sum d_bin_start over all
 * bins of the batch; the fill pass WRITES the three sorted arrays in full.  The place of an atom inside its bin is its rank by atom
 * index, not the order in which an atomic handed out slots.  d_work int32 [n_bins + N] is workspace. */
int egnn_cell_grid_count(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* nb, double radius,
                         int reach, const int32_t* d_cell_ptr, const int32_t* d_nb, const int32_t* d_bin_ptr, const double* d_frac,
                         int n_bins, int32_t* d_atom_bin, int32_t* d_bin_count);
int egnn_cell_grid_fill(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* nb, double radius,
                        int reach, const int32_t* d_cell_ptr, const int32_t* d_nb, const int32_t* d_bin_ptr, const double* d_frac,
                        const int32_t* d_type, int n_bins, const int32_t* d_bin_start, const int32_t* d_atom_bin, int32_t* d_work,
                        int32_t* d_sorted_atom, double* d_sorted_frac, int32_t* d_sorted_type);
/* egnn_cell_bonds_grid_count / _fill: the outputs of egnn_cell_bonds_count / _fill for the cells the tiles name, bit for bit, over
 * a grid of radius = cutoff.  The count pass WRITES d_degree at the ORIGINAL index of every centre of its tiles and touches no other
 * entry (egnn_cell_bonds_count zeroes all of d_degree first: in a mixed batch call it first); d_row_ptr is the same prefix sum as
 * before, and the fill pass WRITES the rows of its centres, ascending by (atom, shift code). */
int egnn_cell_bonds_grid_count(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* nb,
                               const int32_t* tiles, const int32_t* d_cell_ptr, const double* d_lattice, const int32_t* d_nb,
                               const int32_t* d_bin_ptr, int n_bins, const int32_t* d_bin_start, const int32_t* d_sorted_atom,
                               const double* d_sorted_frac, double cutoff, int reach, const int32_t* d_tiles, int n_tiles,
                               int32_t* d_degree);
int egnn_cell_bonds_grid_fill(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* nb,
                              const int32_t* tiles, const int32_t* d_cell_ptr, const double* d_lattice, const int32_t* d_nb,
                              const int32_t* d_bin_ptr, int n_bins, const int32_t* d_bin_start, const int32_t* d_sorted_atom,
                              const double* d_sorted_frac, double cutoff, int reach, const int32_t* d_tiles, int n_tiles,
                              const int32_t* d_row_ptr, int n_bonds, int32_t* d_bond_atom, int32_t* d_bond_shift);
/* egnn_cell_pair_counts_grid: d_counts int64 [C, A, A, nbins] as egnn_cell_pair_counts defines it, over a grid of radius =
 * nbins dR.  It ADDS the counts of the cells its tiles name and zeroes nothing (egnn_cell_pair_counts zeroes all of d_counts and
 * then adds its own tiles: in a mixed batch call it first, or zero d_counts).  A A nbins <= 16384. */
int egnn_cell_pair_counts_grid(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* nb,
                               const int32_t* tiles, const int32_t* d_cell_ptr, const double* d_lattice, const int32_t* d_nb,
                               const int32_t* d_bin_ptr, int n_bins, const int32_t* d_bin_start, const double* d_sorted_frac,
                               const int32_t* d_sorted_type, double dR, int nbins, int reach, const int32_t* d_tiles, int n_tiles,
                               int64_t* d_counts);
/* Host statement of the entries above: HOST pointers, no GPU, no tiles, the same definitions in plain C++.  nb int32 [C, 3] and
 * *n_bins are always written; atom_bin int32 [N], sorted_atom int32 [N] and sorted_frac double [N, 3] where given; bin_start int32
 * [n_bins + 1] where given and bin_cap holds it.  Where bond_ptr int32 [N+1] is given, the bond list of cutoff = radius is found
 * THROUGH THE GRID WALK (rows sorted by key; the lists written where given and bond_cap holds them); where counts int64
 * [C, A, A, nbins] is given, the pair counts likewise (nbins dR <= radius).  Either walk refuses a batch with a cell that is not
 * griddable (EGNN_EINVAL naming the cell and its widths).  Also EGNN_EINVAL: a type outside [0, A), a coordinate that is not
 * finite. */
int egnn_cell_grid_host(int C, int A, const int32_t* cell_ptr, const double* lattice, const double* frac, const int32_t* type,
                        double radius, int reach, double min_width, int32_t* nb, int64_t* n_bins, int32_t* atom_bin, int64_t bin_cap,
                        int32_t* bin_start, int32_t* sorted_atom, double* sorted_frac, int32_t* bond_ptr, int64_t bond_cap,
                        int32_t* bond_atom, int32_t* bond_shift, double dR, int nbins, int64_t* counts);

/* ---- SOAP descriptors of periodic cells (csrc/cells/cell_soap.hip; definitions in csrc/cells/cell_soap_math.h) -----------------
 * The descriptor of egnn_soap_descriptor about atoms of periodic cells, over the sites of EVERY image inside the neighbour cut:
 * site (j, s), s in Z^3, belongs to centre i iff |(wrap(frac_j) - wrap(frac_i) + s) L|^2 < cut^2 in fp64 (the vector of
 * egnn_cell_bonds_*); the centre itself contributes at d = 0 and its own images are ordinary sites.  Vectors and d2 stay in fp64;
 * tables, summation orders and the feature order are those of egnn_soap_descriptor.  An extension: template_matching.py:41-47 builds
 * its descriptors on clusters; dscribe's periodic=True is the behaviour restated, from its description ("SOAP").
 * Cells as in egnn_cell_bonds_* (cell_ptr and lattice given twice, HOST copies for the checks).  The image box of a cell is
 * b_k = floor(cut / w_k) + 1 (w: the perpendicular widths) and must stay <= 4, the range of the shift code: a cell with a width
 * <= cut / 4, or a singular lattice, is EGNN_EINVAL naming the cell and its widths, before anything is launched.  No atomic:
 * results are bitwise reproducible and a cell gives the same bits in any batch.
 *
 * egnn_cell_sites_count / _fill (count / prefix-by-caller / fill): the sites of M listed centres, d_centre_atom int32 [M] (index
 * into the batch; any order, repeats allowed; a centre outside [0, N) gets an empty row).  The count pass WRITES d_degree int32 [M];
 * the caller takes the exclusive prefix sum d_row_ptr int32 [M+1]; the fill pass WRITES d_site_atom int32 [T] (index into the
 * batch) and d_site_shift int32 [T] (shift code): a row in the format of a bond-list row, ascending by (atom, shift code), the
 * centre (i, 0) left out.  One wavefront per centre walks every candidate (atom, shift of the box); work is done for the listed
 * centres only.  Where every width is >= cut the rows are those of egnn_cell_bonds_fill at cutoff = cut, bitwise. */
int egnn_cell_sites_count(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                          const double* d_lattice, const double* d_frac, double cut, int M, const int32_t* d_centre_atom,
                          int32_t* d_degree);
int egnn_cell_sites_fill(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                         const double* d_lattice, const double* d_frac, double cut, int M, const int32_t* d_centre_atom,
                         const int32_t* d_row_ptr, int T, int32_t* d_site_atom, int32_t* d_site_shift);
/* egnn_cell_soap_descriptor: d_desc double [M, F] (F = egnn_soap_features(A, n_max, l_max)) and, where given, d_coeff double
 * [M, A, n_max, (l_max+1)^2], of the M >= 1 centres d_centre_atom; centre m owns row d_centre_row[m] of the CSR (d_row_ptr int32
 * [n_rows + 1], d_site_atom, d_site_shift int32 [T]): the site kernels' (row m) or a bond list of cutoff = cut (row = atom).  The
 * sum runs over the centre first, then the row in its order.  A <= 4, n_max <= 16, l_max <= 10; d_tables as egnn_soap_descriptor.
 * A centre outside [0, N) or a row outside the CSR gives a row of zeros; a site outside the centre's cell contributes nothing. */
int egnn_cell_soap_descriptor(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                              const double* d_lattice, const double* d_frac, const int32_t* d_type, int n_max, int l_max,
                              const double* d_tables, int n_rows, const int32_t* d_row_ptr, int T, const int32_t* d_site_atom,
                              const int32_t* d_site_shift, int M, const int32_t* d_centre_atom, const int32_t* d_centre_row, double* d_desc,
                              double* d_coeff);
/* egnn_cell_soap_mean: the mean descriptor of every cell, d_sum double [C, F].  Rows d_cell_rows[c] .. d_cell_rows[c + 1] (int32
 * [C+1]) of d_desc [M, F] are the centres of cell c in this call, ascending; they are added in that order to the running sum
 * (started from zero where first != 0, else continued from d_sum: centres may come in slabs), and where final != 0 the sum is
 * divided once by d_count[c] (int64 [C], the cell's centres over all calls; a cell without one keeps a row of zeros). */
int egnn_cell_soap_mean(void* stream, int C, int F, int M, const double* d_desc, const int32_t* d_cell_rows, const int64_t* d_count,
                        int first, int final, double* d_sum);
/* Host statements of the entries above: HOST pointers, no GPU, the same definitions in plain C++ (the box walk without a cull).
 * egnn_cell_sites_host always writes row_ptr int32 [M+1]; the lists where given and site_cap holds them (call once with site_cap 0
 * to learn T).  Also EGNN_EINVAL: a centre outside [0, N), a type outside [0, A), a coordinate that is not finite. */
int egnn_cell_sites_host(int C, const int32_t* cell_ptr, const double* lattice, const double* frac, double cut, int M,
                         const int32_t* centre_atom, int32_t* row_ptr, int64_t site_cap, int32_t* site_atom, int32_t* site_shift);
int egnn_cell_soap_host(int C, int A, const int32_t* cell_ptr, const double* lattice, const double* frac, const int32_t* type, int n_max,
                        int l_max, double cut, const double* tables, int M, const int32_t* centre_atom, double* desc, double* coeff);
int egnn_cell_soap_mean_host(int C, int F, const int32_t* cell_rows, const double* desc, const int64_t* count, int first, int final,
                             double* sum);

/* ---- bond-orientational order of periodic cells (csrc/cells/cell_boo.hip; definitions in csrc/cells/cell_boo_math.h) ------------
 * Steinhardt's q_l, w_l and w^_l per atom, the Lechner-Dellago neighbour averages and the ten Wolde-Frenkel solid-bond count, over
 * the sites of egnn_cell_sites_* at cut = cutoff.  No file of the reference computes them (an extension, like the rings).  A site
 * (j, s) of centre i is KEPT where bit type_i * A + type_j of `select` is set (and it does not lie on the centre); n is the number
 * of kept sites.  Y_lm are the real orthonormal harmonics of egnn_soap_descriptor on the unit vector (d_norm double [(l_max+1)^2]:
 * its N_lm table), l_max <= 10, A <= 4.  All fp64; every sum is one thread's running sum in ascending order (no atomic, no
 * reduction across lanes): the device executes the host statement's operations, results are bitwise reproducible and a cell gives
 * the same bits in any batch.  Cells, the CSR (d_row_ptr int32 [n_rows + 1], d_site_atom, d_site_shift int32 [T]) and the centres
 * (d_centre_atom, d_centre_row int32 [M], M >= 1) as in egnn_cell_soap_descriptor.  Bad arguments are EGNN_EINVAL with a message
 * before anything is launched.
 *
 * egnn_cell_boo_qlm (pass 1): d_qlm double [M, (l_max+1)^2], row m = (sum of Y_lm over the kept sites of row d_centre_row[m],
 * ascending) / n, zeros where n = 0; d_n int32 [M].  A width <= cutoff / 4 is refused as by egnn_cell_sites_count.
 * egnn_cell_boo_invariants (pass 2): d_qlm double [N, (l_max+1)^2] holds the rows of EVERY atom of the batch (pass 1 with centre m =
 * atom m).  d_out double [M, blocks, l_max+1], blocks = q, w, w^ and, with averaged != 0, qbar, wbar, wbar^ (3 or 6);
 * q_l = sqrt(4 pi / (2l+1) sum_m q_lm^2); w_l = sum over the entries of G^l of G q_a q_b q_c, G the 3j tensor (l l l; m1 m2 m3) in
 * the real basis for a <= b <= c with multiplicities folded in: g_off int32 [l_max + 2] (HOST copy and d_g_off), d_g_idx int32
 * [E, 3] (a, b, c in [0, 2l]), d_g_val double [E], empty for odd l (w_l = 0); w^_l = w_l / (sum_m q_lm^2)^(3/2), 0 where the sum is
 * 0.  qbar_lm = (q_lm(i) + sum over kept sites of q_lm(atom)) / (1 + n).  d_n int32 [M]; d_n_solid int32 [M] counts the kept sites
 * with s_ik = q(i).q(k) / (|q(i)| |q(k)|) at l_solid strictly above threshold (0 where a norm is 0). */
int egnn_cell_boo_qlm(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                      const double* d_lattice, const double* d_frac, const int32_t* d_type, double cutoff, unsigned select, int l_max,
                      const double* d_norm, int n_rows, const int32_t* d_row_ptr, int T, const int32_t* d_site_atom,
                      const int32_t* d_site_shift, int M, const int32_t* d_centre_atom, const int32_t* d_centre_row, double* d_qlm,
                      int32_t* d_n);
int egnn_cell_boo_invariants(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                             const double* d_lattice, const double* d_frac, const int32_t* d_type, unsigned select, int l_max,
                             const double* d_qlm, int E, const int32_t* g_off, const int32_t* d_g_off, const int32_t* d_g_idx,
                             const double* d_g_val, int l_solid, double threshold, int averaged, int n_rows, const int32_t* d_row_ptr, int T,
                             const int32_t* d_site_atom, const int32_t* d_site_shift, int M, const int32_t* d_centre_atom,
                             const int32_t* d_centre_row, double* d_out, int32_t* d_n, int32_t* d_n_solid);
/* Host statement of the two entries above: HOST pointers, no GPU, the same definitions in plain C++.  It finds its own sites as
 * egnn_cell_sites_host does (the box walk without a cull), computes q_lm of every atom and the invariants of the M >= 0 listed
 * centres: out [M, blocks, l_max+1], n and n_solid int32 [M], and where given qlm double [M, (l_max+1)^2] (the centres' rows).  Also
 * EGNN_EINVAL: a centre outside [0, N), a type outside [0, A), a coordinate that is not finite, a width <= cutoff / 4. */
int egnn_cell_boo_host(int C, int A, const int32_t* cell_ptr, const double* lattice, const double* frac, const int32_t* type, double cutoff,
                       unsigned select, int l_max, const double* norm, int E, const int32_t* g_off, const int32_t* g_idx, const double* g_val,
                       int l_solid, double threshold, int averaged, int M, const int32_t* centre_atom, double* out, int32_t* n,
                       int32_t* n_solid, double* qlm);

/* ---- lattice energy of periodic cells (csrc/cells/cell_ewald.hip; definitions in csrc/cells/cell_ewald_math.h) -----------------
 * Ewald sum of point charges plus a short-range pair potential (Buckingham with an optional D / r^n term: BKS), per-atom energies
 * (eV) and forces (eV / A).  An extension: no file of the reference computes an energy.  The model of a call, HOST arguments: A <= 4,
 * charges double [A] (q_i = charges[type_i]); pot double [4, A, A] = the symmetric tables A, b, C, D of u_ab(r) = A exp(-b r) -
 * C / r^6 + D / r^n or NULL (Coulomb only), 1 <= n <= 64, shift != 0 subtracts u_ab(short_cut); kappa the Coulomb constant, alpha
 * the splitting parameter, 0 < short_cut <= r_cut, k_max: positive and finite.  Sites are those of egnn_cell_sites_* at cut = r_cut,
 * vectors those of egnn_sq_cell_* at q_max = k_max (plan, count, prefix sums and tiles as there).  All fp64, no floating-point
 * atomic: a sum is a lane's ascending running sum and one fixed butterfly over the wavefront, or an ascending running sum; results
 * are bitwise reproducible and a cell gives the same bits in any batch and slab.  Host and device agree bitwise on membership and
 * to rounding on values.  Bad arguments are EGNN_EINVAL with a message before anything is launched; a width <= r_cut / 4 and an
 * index need above 1023 are refused as by egnn_cell_sites_count and egnn_sq_cell_plan.
 *
 * egnn_cell_ewald_real (an extension): the CSR and the centres as in egnn_cell_boo_qlm; d_real double [M, 5] = (e_real, e_short, F_x,
 * F_y, F_z) of centre m (F zeros without forces); d_coincident int32 [C], zeroed by the caller, set to 1 for a cell with a site on
 * its centre (r = 0: the site is left out).
 * egnn_cell_ewald_amplitudes (an extension): d_hkl int32 [K, 3] and d_vec double [K, 5] = (k_x, k_y, k_z, g S^c, g S^s), g =
 * exp(-k^2 / 4 alpha^2) / k^2, S^c + i S^s = sum_j q_j exp(i k . r_j) over the atoms in ascending order; d_tiles int32 [n_tiles, 2] =
 * {cell, first vector (local, a multiple of 256)}.
 * egnn_cell_ewald_recip (an extension): d_rec double [N, 4] = (e_rec, F_x, F_y, F_z) of every atom of the batch from the table.
 * egnn_cell_ewald_finish (an extension): d_real double [N, 5] (centre m = atom m), d_rec double [N, 4] or NULL (no reciprocal part);
 * d_n_type int32 [C, A] workspace; d_atom_components double [N, 5] = (real, reciprocal, self, background, short),
 * d_energy_per_atom double [N], d_force double [N, 3] or NULL; d_components double [C, 5] and d_energy double [C], the sums over a
 * cell's atoms in ascending order. */
int egnn_cell_ewald_real(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                         const double* d_lattice, const double* d_frac, const int32_t* d_type, const double* charges, const double* pot, int n,
                         int shift, double kappa, double alpha, double r_cut, double short_cut, double k_max, int forces, int n_rows,
                         const int32_t* d_row_ptr, int T, const int32_t* d_site_atom, const int32_t* d_site_shift, int M,
                         const int32_t* d_centre_atom, const int32_t* d_centre_row, double* d_real, int32_t* d_coincident);
int egnn_cell_ewald_amplitudes(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* plan,
                               const int32_t* vec_ptr, const int32_t* d_cell_ptr, const double* d_lattice, const int32_t* d_plan,
                               const int32_t* d_vec_ptr, const double* d_frac, const int32_t* d_type, const double* charges, double kappa,
                               double alpha, double r_cut, double k_max, int n_rows, const int32_t* d_row_ptr, int K, const int32_t* d_tiles,
                               int n_tiles, int32_t* d_hkl, double* d_vec);
int egnn_cell_ewald_recip(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* vec_ptr,
                          const int32_t* d_cell_ptr, const double* d_lattice, const int32_t* d_vec_ptr, const double* d_frac,
                          const int32_t* d_type, const double* charges, double kappa, double alpha, double r_cut, double k_max, int forces, int K,
                          const int32_t* d_hkl, const double* d_vec, double* d_rec);
int egnn_cell_ewald_finish(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                           const double* d_lattice, const int32_t* d_type, const double* charges, double kappa, double alpha, double r_cut,
                           double k_max, const double* d_real, const double* d_rec, int32_t* d_n_type, double* d_atom_components,
                           double* d_energy_per_atom, double* d_force, double* d_components, double* d_energy);
/* Host statement of the four entries above (an extension): HOST pointers, no GPU, the same definitions in plain C++, walking the
 * image box and the index box itself, every sum one ascending running sum.  energy [C], components [C, 5], energy_per_atom [N],
 * n_vectors int64 [C] (0 where every charge is 0: no reciprocal part) and coincident int32 [C] are always written; atom_components
 * [N, 5], n_sites int32 [N] (the sites of every atom inside r_cut) where given, force [N, 3] with forces != 0.  Also EGNN_EINVAL: a
 * type outside [0, A), a coordinate that is not finite. */
int egnn_cell_ewald_host(int C, int A, const int32_t* cell_ptr, const double* lattice, const double* frac, const int32_t* type,
                         const double* charges, const double* pot, int n, int shift, double kappa, double alpha, double r_cut, double short_cut,
                         double k_max, int forces, double* energy, double* components, double* energy_per_atom, double* atom_components,
                         double* force, int32_t* n_sites, int64_t* n_vectors, int32_t* coincident);

/* ---- strain derivative of the lattice energy: Ewald virial, stress, pressure (csrc/cells/cell_ewald.hip, section 5; definitions
 * in csrc/cells/cell_stress_math.h) ------------------------------------------------------------------------------------------
 * D_xy = dE / d eps_xy (eV) under a homogeneous strain L -> L (1 + eps) with the fractional coordinates, alpha, the cutoffs and the
 * membership of sites and vectors held; six numbers in Voigt order xx, yy, zz, yz, xz, xy; split per atom and per component (real,
 * reciprocal, self = 0, background, short) as the energy is.  stress = D / V (eV / A^3, tension positive), pressure = -(s_xx +
 * s_yy + s_zz) / 3.  An extension: no file of the reference computes a stress.  The model, the sites, the vector table, the orders
 * of the sums, the checks and the refusals are those of the lattice-energy entries above; the entries of the energy are not
 * changed by these and produce the same bits with or without them.
 *
 * egnn_cell_ewald_virial_real (an extension): the arguments of egnn_cell_ewald_real without `forces`; d_virial double [M, 12] =
 * D_real (six) and D_short (six) of centre m; d_coincident as there.
 * egnn_cell_ewald_virial_recip (an extension): the arguments of egnn_cell_ewald_recip without `forces`, the table of
 * egnn_cell_ewald_amplitudes; d_virial double [N, 6] = D_reciprocal of every atom of the batch.
 * egnn_cell_ewald_virial_finish (an extension): d_virial_real double [N, 12] (centre m = atom m), d_virial_recip double [N, 6] or
 * NULL (no reciprocal part); d_n_type int32 [C, A] workspace; d_atom_components double [N, 5, 6], d_per_atom double [N, 6];
 * d_components double [C, 5, 6] and d_strain double [C, 6], the sums over a cell's atoms in ascending order; d_stress double [C, 6],
 * d_pressure double [C]. */
int egnn_cell_ewald_virial_real(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                                const double* d_lattice, const double* d_frac, const int32_t* d_type, const double* charges, const double* pot,
                                int n, int shift, double kappa, double alpha, double r_cut, double short_cut, double k_max, int n_rows,
                                const int32_t* d_row_ptr, int T, const int32_t* d_site_atom, const int32_t* d_site_shift, int M,
                                const int32_t* d_centre_atom, const int32_t* d_centre_row, double* d_virial, int32_t* d_coincident);
int egnn_cell_ewald_virial_recip(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* vec_ptr,
                                 const int32_t* d_cell_ptr, const double* d_lattice, const int32_t* d_vec_ptr, const double* d_frac,
                                 const int32_t* d_type, const double* charges, double kappa, double alpha, double r_cut, double k_max, int K,
                                 const int32_t* d_hkl, const double* d_vec, double* d_virial);
int egnn_cell_ewald_virial_finish(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                                  const double* d_lattice, const int32_t* d_type, const double* charges, double kappa, double alpha, double r_cut,
                                  double k_max, const double* d_virial_real, const double* d_virial_recip, int32_t* d_n_type,
                                  double* d_atom_components, double* d_per_atom, double* d_components, double* d_strain, double* d_stress,
                                  double* d_pressure);
/* Host statement of the three entries above (an extension): HOST pointers, no GPU, the same definitions in plain C++, every sum one
 * ascending running sum.  strain [C, 6], components [C, 5, 6], per_atom [N, 6], stress [C, 6], pressure [C], n_vectors int64 [C]
 * and coincident int32 [C] are always written; atom_components [N, 5, 6] where given.  The refusals of egnn_cell_ewald_host. */
int egnn_cell_ewald_virial_host(int C, int A, const int32_t* cell_ptr, const double* lattice, const double* frac, const int32_t* type,
                                const double* charges, const double* pot, int n, int shift, double kappa, double alpha, double r_cut,
                                double short_cut, double k_max, double* strain, double* components, double* per_atom, double* atom_components,
                                double* stress, double* pressure, int64_t* n_vectors, int32_t* coincident);

/* ---- relaxation of periodic cells: FIRE over held site lists (csrc/cells/cell_relax.hip; definitions in
 * csrc/cells/cell_relax_math.h) ---------------------------------------------------------------------------------------------
 * The atoms of a fixed cell move down the lattice energy above by FIRE (Bitzek et al., PRL 97, 170201; unit mass 1).  An extension:
 * no file of the reference relaxes a structure.  The sites of an evaluation come from rows of egnn_cell_sites_* at cut = r_cut +
 * skin that are held while no atom has moved more than skin / 2 since they were built.  State of a call, caller-owned device
 * arrays: d_frac double [N, 3] UNWRAPPED fractional coordinates, d_velocity, d_since (the Cartesian move since the cell's list was
 * built) and d_moved (the net move) double [N, 3]; d_scalars double [C, 5] = (dt, a, energy, initial energy, max force); d_counters
 * int32 [C, 4] = (n_pos, steps, status: 0 running, 1 converged, 2 step limit, 3 coincident atoms, 4 forces not finite, 5 stuck: froze
 * twice without a move in between; frozen: steps + 1 of the last freeze, 0 at the start); d_done and
 * d_rebuild int32 [C].  All fp64, no floating-point atomic, every sum in one fixed order that depends on the cell alone: results are
 * bitwise reproducible and a cell gives the same bits in any batch.  Bad arguments are EGNN_EINVAL with a message before anything
 * is launched.
 *
 * egnn_cell_relax_real (an extension): egnn_cell_ewald_real over HELD rows -- the arguments of that entry with `skin` in place of
 * `forces` (always computed); d_frac is read unwrapped, the vector of site (j, s) is ((u_j - u_i) + s) L in the operation order of
 * the search, and an entry counts iff cell_norm2(d) < r_cut^2 now.  The image box of r_cut + skin must stay within 4.
 * egnn_cell_relax_step (an extension): one step of every cell from d_force double [N, 3], d_energy double [C] and d_coincident int32
 * [C] of an evaluation: convergence (max |F| < f_max), the step limit, the FIRE update, the cap max_step on the largest move of an
 * atom, the freeze rule (a move that would bring an atom beyond skin / 2 since the build is not made: d_rebuild is set and nothing
 * else of the cell changes; a cell whose d_since is all zero, just built, always moves), the move, the counters.  A cell with d_done or d_rebuild set is left alone; the caller rebuilds
 * (d_frac <- wrapped, d_since <- 0, the rows searched again) and clears d_rebuild.  d_energy_trace, d_force_trace double
 * [max_steps + 1, C] or NULL: row k holds the energy and max |F| before move k.  max_step <= skin / 2. */
int egnn_cell_relax_real(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                         const double* d_lattice, const double* d_frac, const int32_t* d_type, const double* charges, const double* pot, int n,
                         int shift, double kappa, double alpha, double r_cut, double short_cut, double k_max, double skin, int n_rows,
                         const int32_t* d_row_ptr, int T, const int32_t* d_site_atom, const int32_t* d_site_shift, int M,
                         const int32_t* d_centre_atom, const int32_t* d_centre_row, double* d_real, int32_t* d_coincident);
int egnn_cell_relax_step(void* stream, int C, int N, const int32_t* cell_ptr, const double* lattice, const int32_t* d_cell_ptr,
                         const double* d_lattice, const double* d_force, const double* d_energy, const int32_t* d_coincident, double dt_max,
                         int n_min, double f_inc, double f_dec, double a_start, double f_a, double max_step, double f_max, int max_steps,
                         double skin, double* d_frac, double* d_velocity, double* d_since, double* d_moved, double* d_scalars,
                         int32_t* d_counters, int32_t* d_done, int32_t* d_rebuild, double* d_energy_trace, double* d_force_trace);
/* Host statement of egnn_cell_relax_step (an extension): HOST pointers, no GPU, the same text in plain C++; bitwise what the kernel
 * gives. */
int egnn_cell_relax_step_host(int C, int N, const int32_t* cell_ptr, const double* lattice, const double* force, const double* energy,
                              const int32_t* coincident, double dt_max, int n_min, double f_inc, double f_dec, double a_start, double f_a,
                              double max_step, double f_max, int max_steps, double skin, double* frac, double* velocity, double* since,
                              double* moved, double* scalars, int32_t* counters, int32_t* done, int32_t* rebuild, double* energy_trace,
                              double* force_trace);
/* Host statement of the whole relaxation (an extension): HOST pointers, no GPU.  Per cell: the held list at r_cut + skin by the box
 * walk of egnn_cell_ewald_host, the evaluation by the code behind that statement with the real part added over the held row in
 * ascending order, the step above, a rebuild as soon as the cell asks.  dt is the first time step.  Always written: frac_out [N, 3]
 * (unwrapped since the last build), energy, initial_energy, max_force double [C], force [N, 3] at the final coordinates, steps,
 * status and n_rebuilds int32 [C], moved [N, 3].  Where given: energy_trace, force_trace [max_steps + 1, C] and frac_trace
 * [max_steps + 1, N, 3] (the coordinates evaluated before move k), NaN beyond a cell's last evaluation.  The refusals of
 * egnn_cell_ewald_host and of the step; the image box of r_cut + skin within 4. */
int egnn_cell_relax_host(int C, int A, const int32_t* cell_ptr, const double* lattice, const double* frac, const int32_t* type,
                         const double* charges, const double* pot, int n, int shift, double kappa, double alpha, double r_cut, double short_cut,
                         double k_max, double dt, double dt_max, int n_min, double f_inc, double f_dec, double a_start, double f_a, double max_step,
                         double f_max, int max_steps, double skin, double* frac_out, double* energy, double* initial_energy, double* force,
                         double* max_force, int32_t* steps, int32_t* status, double* moved, int32_t* n_rebuilds, double* energy_trace,
                         double* force_trace, double* frac_trace);

/* ---- structure factors (csrc/eval/sq.hip; definitions in csrc/eval/sq_math.h) -----------------------------------------------
 * Reciprocal-space statistics: Debye sums of clusters and reciprocal-lattice sums of periodic cells.  No file of the reference
 * computes them (an extension, like the rings).  All sums are fp64 in one fixed order, no floating-point atomic: results are
 * bitwise reproducible and a graph gives the same bits in any batch.  Bad arguments return EGNN_EINVAL with a message before
 * anything is launched; every output is written by the call.
 *
 * egnn_sq_debye: d_out double [B, A, A, Q], D_ab(q_k) = sum_{i in a} sum_{j in b, j != i, r_ij < r_max} w(r_ij) sinc(q_k r_ij);
 * r in fp64 from the float32 positions, sinc(0) = 1, r_max = +inf no cut, window 0 (w = 1) or 1 (Lorch, sinc(pi r / r_max),
 * finite r_max).  q double [Q], finite and >= 0, any order, Q <= 4096, given twice (HOST copy for the checks, device copy for
 * the kernel); A <= 4; graphs of at most 32768 atoms.  d_tiles int32 [n_tiles, 3] = {graph, first atom i, first atom j} (local
 * indices; multiples of 64 and of 256): every 64 x 256 block of a graph that holds a pair i < j, the tiles of a graph contiguous,
 * d_tile_ptr int32 [B+1] the first tile of each graph; d_partial double [n_tiles, A(A+1)/2, Q] is workspace.  One workgroup per
 * tile visits each unordered pair once (r once per pair and 512 q values); a finishing pass adds the tiles of a graph in
 * ascending index.  D_ab(0) without a cut is exactly N_a N_b - delta_ab N_a. */
int egnn_sq_debye(void* stream, int B, int A, const float* d_pos, const int32_t* d_type, const int32_t* d_graph_ptr, int max_atoms, int Q,
                  const double* q, const double* d_q, double r_max, int window, const int32_t* d_tiles, int n_tiles,
                  const int32_t* d_tile_ptr, double* d_partial, double* d_out);
/* Cells: lattice double [C, 9] (rows a_1, a_2, a_3), frac double [N, 3] (wrapped to [0, 1) as in egnn_cell_*), k_m = 2 pi m L^-T
 * for integer m = (h, k, l); the vectors of a cell are the m of the half space (h > 0, or h = 0 and k > 0, or h = k = 0 and
 * l > 0) with |k_m| < q_max, each standing for +-m, ordered cell by cell and ascending (h, k, l).  q_max must keep
 * floor(q_max |a_i| / 2 pi) <= 1023 on every axis and at most 2^24 vectors per cell.
 *
 * egnn_sq_cell_plan (host only, no GPU): plan int32 [C, 4] = {H, K, L, first row}, the index box of each cell (one wider than
 * the bound, at most 1023) and where its (H + 1)(2K + 1) rows (h, k) start; *n_rows their total.
 * egnn_sq_cell_count: d_row_count int32 [n_rows], the vectors of every (h, k) row.  The caller takes the exclusive prefix sum
 * d_row_ptr int32 [n_rows + 1] and, at the first row of each cell, vec_ptr int32 [C+1].
 * egnn_sq_cell_rho (the fill pass): d_hkl int32 [K, 3], d_k double [K] = |k_m|, d_bin int32 [K] = floor(|k_m| / dq) (nbins =
 * ceil(q_max / dq) <= 4096) and d_rho double [K, A, 2] = (re, im) of rho_a(m) = sum_{j in a} exp(-i k_m . r_j), the phase
 * h f_1 + k f_2 + l f_3 taken mod 1 before the sine and cosine.  d_tiles int32 [n_tiles, 2] = {cell, first vector (local, a
 * multiple of 256)}: one workgroup per 256 vectors of a cell, the cell's atoms staged in LDS and shared by them.  cell_ptr,
 * lattice, plan and vec_ptr are given twice (HOST copies for the checks).
 * egnn_sq_cell_shells: per cell and shell bin, d_count int64 [C, nbins] = vectors over the full sphere (2 x the half space),
 * d_mean_k double [C, nbins] and d_s double [C, A, A, nbins] = the mean of Re(rho_a rho_b*), every sum over the bin's vectors in
 * ascending vector index; an empty bin has count 0 and NaN means. */
int egnn_sq_cell_plan(int C, const double* lattice, double q_max, int32_t* plan, int32_t* n_rows);
int egnn_sq_cell_count(void* stream, int C, const double* lattice, const int32_t* plan, const double* d_lattice, const int32_t* d_plan,
                       double q_max, int n_rows, int32_t* d_row_count);
int egnn_sq_cell_rho(void* stream, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const int32_t* plan,
                     const int32_t* vec_ptr, const int32_t* d_cell_ptr, const double* d_lattice, const int32_t* d_plan,
                     const int32_t* d_vec_ptr, const double* d_frac, const int32_t* d_type, double q_max, double dq, int nbins, int n_rows,
                     const int32_t* d_row_ptr, int K, const int32_t* d_tiles, int n_tiles, int32_t* d_hkl, double* d_k, int32_t* d_bin,
                     double* d_rho);
int egnn_sq_cell_shells(void* stream, int C, int A, int nbins, const int32_t* vec_ptr, const int32_t* d_vec_ptr, int K, const double* d_k,
                        const int32_t* d_bin, const double* d_rho, int64_t* d_count, double* d_mean_k, double* d_s);
/* Host statement of the entries above: HOST pointers, no GPU, no tiles, the same definitions in plain C++ with a summation order of
 * its own (pairs i < j ascending; atoms ascending; vectors ascending).  Two parts, each skipped where its count is 0: Debye sums
 * (B > 0) and cells (C > 0; cell_A types).  vec_ptr int64 [C+1] is always written; hkl, kabs, bin, rho are written where given and
 * vec_cap holds them (call once with vec_cap 0 to learn K); count, mean_k and s where all three are given.  Also EGNN_EINVAL: a
 * type outside [0, A), a graph_ptr that does not run from 0 to N (cell_ptr: to cell_N) or decreases, a coordinate that is not finite. */
int egnn_sq_host(int B, int N, int A, const float* pos, const int32_t* type, const int32_t* graph_ptr, int Q, const double* q, double r_max,
                 int window, double* debye, int C, int cell_N, int cell_A, const int32_t* cell_ptr, const double* lattice, const double* frac,
                 const int32_t* cell_type, double q_max, double dq, int nbins, int64_t vec_cap, int64_t* vec_ptr, int32_t* hkl, double* kabs,
                 int32_t* bin, double* rho, int64_t* count, double* mean_k, double* s);

/* ---- the two small networks at the edge of the path ---------------------------------------------------
 * gamma_tilde(t_i) = l1(t_i) + l3(sigmoid(l2(l1(t_i)))) of GammaNetwork (SNR.py:50-52) with PositiveLinear's softplus weights
 * (:5-22) for n time points; d_l1_w [1], d_l2_w [hidden], d_l3_w [hidden] are the RAW parameters (l1.weight, l2.weight,
 * l3.weight).  The caller normalises with gamma_tilde(0), gamma_tilde(1) and rescales to [gamma_0, gamma_1] (:54-64). */
int egnn_gamma_tilde(void* stream, int n, int hidden, const float* d_t, const float* d_l1_w, const float* d_l2_w,
                     const float* d_l3_w, float* d_out);
/* One Linear (+ ReLU) over node rows: out [N, J] = act(in [N, K] . W^T + b), W in nn.Linear layout [J, K]
 * (SpectrumCompressor, DataPreprocessor.py:10-19, layer by layer).  1 <= K <= 2048: a workgroup stages 16 rows of K floats in
 * LDS, 128 KiB at the limit; a larger K returns EGNN_EINVAL before anything is launched. */
int egnn_dense_rows(void* stream, int N, int K, int J, const float* d_in, const float* d_W, const float* d_b, int relu,
                    float* d_out);

/* ---- optimizer step (csrc/optim/optim_step.hip) ------------------------------------------------------
 * The three optimizers of define_optimizer (parts/def_for_main.py:119-139) as ONE multi-tensor launch per step: replaces the
 * per-tensor element-wise loops of torch.optim.Adam, torch.optim.AdamW(amsgrad=True) (torch's single-tensor form) and
 * schedulefree's RAdamScheduleFree (restated in diffusion_model_amd/optim.py).  All arithmetic is fp32, one IEEE operation at
 * a time (no contraction, correctly rounded sqrt / div, denormals kept), in the order tests/_optim_mirror.py restates.
 * The kernels hold no step-count logic: the CALLER computes the per-step scalars in double (bias corrections, rectified
 * learning rate, averaging weight c_{k+1}, ...) and passes them rounded to fp32. */
enum { EGNN_OPTIM_ADAM = 0,            /* torch.optim.Adam: L2 weight decay (g += wd p)                             */
       EGNN_OPTIM_ADAMW_AMSGRAD = 1,   /* torch.optim.AdamW(amsgrad=True): decoupled decay (p *= 1 - lr wd)         */
       EGNN_OPTIM_RADAM_SF = 2 };      /* RAdamScheduleFree.step (optim.py), parameters hold y                      */
typedef struct egnn_optim_consts {
  float beta2, one_minus_beta2;        /* all kinds: v = v beta2 + (g g) (1 - beta2)                                 */
  float eps;                           /* all kinds                                                                  */
  float weight_decay;                  /* ADAM: g += wd p; RADAM_SF: gn += wd y; 0 = skipped.  ADAMW: unused        */
  float one_minus_beta1;               /* ADAM / ADAMW: m += (1 - beta1) (g - m)                                     */
  float bias_correction2_sqrt;         /* ADAM / ADAMW: sqrt(1 - beta2^step)                                         */
  float step_size;                     /* ADAM / ADAMW: lr / (1 - beta1^step)                                        */
  float decay_mul;                     /* ADAMW: 1 - lr wd                                                           */
  float bias_correction2;              /* RADAM_SF: 1 - beta2^step                                                   */
  float ckp1;                          /* RADAM_SF: c_{k+1} = weight / weight_sum (0 while weight_sum is 0)          */
  float adaptive_y_lr;                 /* RADAM_SF: lr_t (beta1 (1 - c_{k+1}) - 1)                                   */
  float lr;                            /* RADAM_SF: the rectified (scheduled) learning rate lr_t                     */
  int32_t rectified;                   /* RADAM_SF: rho_t > 4 (gn = g / (sqrt(v / bc2) + eps)); 0: gn = g           */
} egnn_optim_consts;
/* One step over n tensors.  d_p / d_g / d_s0 / d_s1 / d_s2 are HOST arrays of n device pointers, numel the n element counts
 * (fp32, contiguous; each pointer needs 4-byte alignment only, each on its own).  d_g[i] == NULL skips tensor i (p.grad is
 * None).  States: ADAM s0 = exp_avg, s1 = exp_avg_sq (d_s2 may be NULL); ADAMW_AMSGRAD + s2 = max_exp_avg_sq; RADAM_SF s0 = z,
 * s1 = exp_avg_sq (d_s2 may be NULL).  Tensor descriptors travel in the kernel arguments: one launch takes up to
 * egnn_optim_tensors_per_launch() tensors whose state pointers share one spacing (s1[i] - s0[i] and s2[i] - s0[i] the same for
 * every i, as with states laid out alike in flat buffers); a list is cut where the capacity or the spacing ends, so ANY list
 * is valid and a flat-state list of n tensors takes ceil(n / capacity) launches.  No allocation, copy or synchronisation. */
int egnn_optim_step(void* stream, int kind, int n, float* const* d_p, const float* const* d_g, float* const* d_s0,
                    float* const* d_s1, float* const* d_s2, const int64_t* numel, const egnn_optim_consts* consts);
/* p <- p + weight (z - p) over the list: the y <-> x switch of RAdamScheduleFree.train() / .eval() (optim.py;
 * parts/train_per_iretation.py:103-104, :189-190), same launch rule. */
int egnn_optim_interp(void* stream, int n, float* const* d_p, const float* const* d_z, const int64_t* numel, float weight);
/* compile-time tensor capacity of one launch (pure host) */
int egnn_optim_tensors_per_launch(void);

/* timing helper for bench.py: average duration (ms) of the fused edge kernel over the launches
 * recorded since the last reset, measured with HIP events on the launch stream. */
/* diagnostic builds only (-DEGNN_EXP_STAMP): s_memtime stamps [2][8][32][4] of one edge workgroup */
int egnn_debug_stamps(egnn_ctx* ctx, unsigned long long* host_out);
int egnn_profile_enable(egnn_ctx* ctx, int enable);
int egnn_profile_read(egnn_ctx* ctx, float* edge_ms_avg, int* edge_launches, float* node_ms_avg);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* EGNN_AMD_H */

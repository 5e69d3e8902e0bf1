"""Differentiable EGNN forward for training.

Forward: the fused HIP kernels (same call as inference); per layer the inputs (h_l, x_l) and the three segment sums the edge
pass produced (egcl_read_aggregates) are kept.  decide_keep() settles once per shape whether the forward also keeps the edge
activations (egcl_forward_save: the first-layer activations and the second-layer pre-activations of every edge, 7 GB per
layer at 2^20 edges), so that the backward has no recompute pass.

Backward: plan_backward() turns the precision, the widths, the graph and the switches (_switches(), the only reader of the
environment; table in INTEGRATION.md) into ONE BackwardPlan at the top of the call; everything below follows that record and
decides nothing.  Per layer, in reverse order:

  node part  (N rows, small): x' = x + sum_x / (G + 1), G = sqrt(sum d^2), differentiated by torch (_coordinate_update), and
             h' = mlp_h([h | sum_m]) in the plan's node form: "hip" (the library's own GEMM kernels, bf16 operands: bf16 / fp16
             at the reference widths), "split" (head + remainder products on the same kernels: bf16x3 / f16c8, or EGNN_BWD_OWN=1)
             or "torch" (exact fp32 products of the BLAS library: fp32, and every shape the own kernels do not tile).
  edge part  (E rows, the cost): _edge_setup, then per chunk of edges four stages, each in the variant _stages() picks:
               dL/da2   second-layer pre-activations -> dL/da2 in place, g_diff and the bias / w3 / wa column sums
                        kept: egcl_backward_heads_saved on the kept buffers (default for bf16 when HBM allows) | fused:
                        egcl_backward_edge_recompute on the forward's MFMA edge kernels | chain: l1_act, product, heads
               w2       second-layer weight gradients: gemm_tn (own split-K kernel) | library products (_wgrad)
               dL/da1   first == "graph": egcl_backward_dgrad_reduce, the first layers' per-node sums taken in the dgrad kernel's
                        epilogue, dL/da1 never written (default for graphs of at most 64 nodes) | fused: egcl_backward_dgrad |
                        chain: products, l1_grad
               first    first-layer gradients and the scatter to dL/dh, dL/dx: factorised (first == "reduce": one extra pass,
                        egcl_backward_first_reduce, the reference form; then scatter_geom for both forms) | gather + gemm_tn x 2
                        + gemm_rows + scatter | gather + library products + scatter
             and _edge_finish: the node-level products of the factorised forms and the hand-over of the parameter gradients.
             bf16 storage keeps the [edges, W] buffers and runs the products in bf16 (fp32 accumulate, fp32 master gradients);
             fp32 storage is fp32 end to end.  fp16 forwards take the bf16 backward, bf16x3 / f16c8 the fp32 one.

Math (reference EquivariantGraphNeuralNetwork.py:55-71), per edge e = (i <- j):
  in = [h_i | h_j | d2],  d2 = |x_i - x_j|^2
  m branch : m = SiLU(W2m SiLU(W1m in + b1m) + b2m);  out = m * sigmoid(wa . m + ba)          -> sum_m[i]
  x branch : s = w3 . SiLU(W2x SiLU(W1x in + b1x) + b2x) + b3;  xm = (x_i - x_j) * s          -> sum_x[i]
"""
from __future__ import annotations

import bisect
import math
import os
from dataclasses import InitVar, dataclass
from functools import partial
from types import SimpleNamespace

import torch

from . import _lib


def _switches(env=None):
    """the switches of the training path as plain values (table: INTEGRATION.md); nothing else here reads the environment"""
    g = (os.environ if env is None else env).get
    return {"SAVE": g("EGNN_BWD_SAVE", "1") != "0", "FUSED": g("EGNN_BWD_FUSED", "1") != "0", "EDGE": int(g("EGNN_EDGE", "4")),
            "FIRST": g("EGNN_BWD_FIRST", "0") == "1", "GRAPH": g("EGNN_BWD_GRAPH", "1") != "0",
            "BLAS": g("EGNN_BWD_BLAS", "0") == "1", "OWN": g("EGNN_BWD_OWN", "0") == "1",
            "CHUNK": int(g("EGNN_BWD_CHUNK", 1 << 20)), "POISON_KEPT": g("EGNN_DEBUG_POISON_KEPT", "0") == "1"}


EDGE_CHUNK = _switches()["CHUNK"]   # edges per backward chunk (workspace = up to 6 bf16 [chunk, W] buffers); read at plan time

# training.GradAllReducer.arm() puts itself here: the backward below hands it every layer's parameter gradients as soon
# as they are final, so the bucket's all-reduce runs under the backward of the earlier layers
ACTIVE_REDUCER = None
LAST_PLAN = None               # the BackwardPlan of the last backward call (tests)
LAST_FIRST_LAYER_FORM = None   # its `first` field, once an edge backward has run: None (chain) / "graph" / "reduce" (tests)


def _round_up(v, m):
    return (v + m - 1) // m * m


@dataclass(frozen=True)
class BackwardPlan:
    """every decision of one backward call; combinations no stage routine exists for are rejected here"""
    prec: int              # storage precision of the edge buffers and stage kernels: PREC_BF16 (bf16, fp16) or PREC_F32 (the rest)
    split_products: bool   # fp32 products as head + remainder on the own kernels (gemm.mm_tn_split / mm_nn_split), not the BLAS library
    fused: bool            # the context-handle kernels run: the forward's MFMA edge kernels recompute, egcl_backward_dgrad*
    hip_gemms: bool        # the remaining products on gemm_tn.hip / gemm_rows.hip (widths that fit their tiles)
    kept: bool             # the forward kept the edge activations: no recompute pass
    first: str | None      # first Linear layers: None (chain over all edges) / "graph" / "reduce" (factorised, <= 64-node graphs)
    rows: int              # rows of the [chunk, W] workspace buffers
    chunks: tuple          # ((first edge, edges), ...); whole graphs in the "graph" form
    K1P: int               # padded width of in = [h_i | h_j | d2 | 1 | 0...]: the own GEMMs' 128, else a multiple of 8
    node: str              # node MLP form: "hip" / "split" / "torch"
    graph_edge_ptr: InitVar[object] = None   # (checked against `chunks`, not kept)

    def __post_init__(self, graph_edge_ptr):
        cuts = set(graph_edge_ptr or ())
        for bad, why in ((self.fused and self.prec != _lib.PREC_BF16, "the context-handle kernels are bf16 kernels"),
                         (self.hip_gemms and not self.fused, "hip_gemms without fused"),
                         (self.kept and not self.fused, "kept without fused"),
                         (self.first is not None and not self.hip_gemms, "first without hip_gemms"),
                         (self.first == "graph" and any(a not in cuts or a + n not in cuts for a, n in self.chunks),
                          "'graph' with chunks not cut at graph boundaries"),
                         (self.node == "hip" and not self.hip_gemms, "node form 'hip' without hip_gemms"),
                         (self.node == "split" and not self.split_products, "node form 'split' without split_products")):
            if bad:
                raise ValueError(f"BackwardPlan: {why}")

    @property
    def dtype(self):
        return torch.bfloat16 if self.prec == _lib.PREC_BF16 else torch.float32


def _keep_asked(prec, E, sw):
    return E > 0 and prec == _lib.PREC_BF16 and sw["SAVE"] and sw["FUSED"] and sw["EDGE"] >= 4


def decide_keep(prec, E, L, Wx, Wm, M, sw, fused_supported, free):
    """keep the edge activations instead of recomputing them in the backward?  When the bf16 fast path runs and the buffers --
    E x (2 Wx + Wm + M) bf16 per layer -- take less than half of the free HBM (`free`, bytes) and fit the keeping forward's
    32-bit buffer descriptor: E x Wx x 2 B < 4 GiB"""
    need = L * _round_up(E, 64) * (2 * Wx + Wm + M) * 2
    return bool(_keep_asked(prec, E, sw) and fused_supported and need < 0.5 * free and E * Wx * 2 < 2 ** 32)


def _storage_prec(prec):
    """bf16x3 / f16c8 forward on the split-operand kernels, their backward is the fp32 chain; fp16 forwards recompute on the bf16
    kernels"""
    return {_lib.PREC_BF16X3: _lib.PREC_F32, _lib.PREC_F16C8: _lib.PREC_F32, _lib.PREC_F16: _lib.PREC_BF16}.get(prec, prec)


def fused_asked(prec, E, kept, sw):
    """do the switches ask for the context-handle kernels?  (the caller then asks the library whether the widths have them)"""
    return bool(kept or (E > 0 and _storage_prec(prec) == _lib.PREC_BF16 and sw["FUSED"]))


def _hip_gemm_shapes(H, Wx, Wm, M):
    """the bf16 backward's GEMMs run on the library's own kernels (gemm_tn.hip, gemm_rows.hip) when the widths fit their
    tiles: reduction widths multiples of 64, output widths multiples of 256 / 128"""
    return Wx % 256 == 0 and Wm % 256 == 0 and M % 256 == 0 and 2 * H + 2 <= 128


def _graph_chunks(plan, rows):
    """[(first edge, edges)] chunks of WHOLE graphs with at most `rows` edges each (None: a graph alone has more)"""
    gep = getattr(plan, "graph_edge_ptr", None)
    if gep is None:
        return None
    out, a, E = [], 0, gep[-1]
    while a < E:
        b = gep[bisect.bisect_right(gep, a + rows) - 1]
        if b <= a:
            return None
        out.append((a, b - a))
        a = b
    return out


def plan_backward(prec, H, Wx, Wm, M, Wh, E, edge_chunk, graph_edge_ptr, max_graph_nodes, kept, fused_supported, sw):
    """the BackwardPlan of one call.  `kept`: the forward kept the activations and they are not spent yet; `fused_supported`: the
    library's answer (asked only when fused_asked()); `sw`: _switches()"""
    # tolerance-grade precisions multiply through the own kernels, fp32 (parity mode) through the BLAS library unless
    # EGNN_BWD_OWN=1; EGNN_BWD_BLAS=1 forces the BLAS library for every precision (A/B)
    split = not sw["BLAS"] and (prec in (_lib.PREC_BF16X3, _lib.PREC_F16C8) or sw["OWN"])
    fused = fused_asked(prec, E, kept, sw) and bool(fused_supported)
    hip = fused and _hip_gemm_shapes(H, Wx, Wm, M)
    rows = _round_up(min(edge_chunk, E), 64)
    first, chunks = None, [(a, min(rows, E - a)) for a in range(0, E, rows or 1)]
    if hip and max_graph_nodes <= 64:   # the factorised first layers: batches of graphs of at most 64 nodes
        if sw["FIRST"]:
            first = "reduce"
        elif sw["GRAPH"]:
            cut = _graph_chunks(SimpleNamespace(graph_edge_ptr=graph_edge_ptr), rows)
            if cut is not None:         # (None: a graph with more edges than the chunk -- the chain, which may cut anywhere)
                first, chunks = "graph", cut
    node = "hip" if hip and Wh % 256 == 0 else "split" if split else "torch"
    return BackwardPlan(prec=_storage_prec(prec), split_products=split, fused=fused, hip_gemms=hip, kept=bool(kept), first=first,
                        rows=rows, chunks=tuple(chunks), K1P=128 if hip else _round_up(2 * H + 2, 8), node=node,
                        graph_edge_ptr=graph_edge_ptr)


class _Workspace:
    """[chunk, width] buffers of the edge part, allocated once per backward call: the ones the plan's forms touch"""

    def __init__(self, bp, Wx, Wm, M, device):
        rows = bp.rows
        e = lambda *shape, dt=bp.dtype: torch.empty(*shape, dtype=dt, device=device)
        if not bp.kept:   # (the saved-activation backward reads s1 / a2 from what the forward kept)
            self.s1x, self.s1m = e(rows, Wx), e(rows, Wm)
            self.a2x, self.a2m = e(rows, Wx), e(rows, M)
        self.d2 = e(rows, dt=torch.float32)
        self.g_diff = e(rows, 3, dt=torch.float32)
        # dL/da1 and the gathered first-layer inputs / their gradients exist only in the forms that store them: the default
        # 'graph' form of the first Linear layers never touches them (2 x 2 GiB + 2 x 256 MiB at 2^20 rows, W = 1024)
        if bp.first != "graph":
            self.g1x, self.g1m = e(rows, Wx), e(rows, Wm)
        if bp.first is None:
            self.inp, self.g_in = e(rows, bp.K1P), e(rows, bp.K1P)


def _mm(split, a, b, out=None):
    """a @ b for fp32 operands of the fp32-grade chain; `split`: as head + remainder products (gemm.mm_nn_split, 2^-16 per
    operand -- what the tolerance-grade precisions' forward carries)"""
    if split and a.is_cuda and a.dtype == torch.float32:
        from .gemm import mm_nn_split
        return mm_nn_split(a, b.float(), out=out)
    return torch.mm(a, b, out=out) if out is not None else torch.mm(a, b)


def _wgrad(split, g, a, n_pad, splits):
    """g[:n_pad]^T . a[:n_pad] with the long edge dimension cut into `splits` batched products (the BLAS library's
    single-GEMM choice for K = 2^18 and a small output runs at a fraction of its batched rate); fp32 result"""
    if split and g.is_cuda and g.dtype == torch.float32:
        from .gemm import mm_tn_split
        return mm_tn_split(g[:n_pad], a[:n_pad])
    S = splits
    while S > 1 and (n_pad % S or n_pad // S < 1024):
        S //= 2
    if S == 1:
        return torch.mm(g[:n_pad].t(), a[:n_pad]).float()
    gv, av = g[:n_pad].view(S, n_pad // S, -1), a[:n_pad].view(S, n_pad // S, -1)
    return torch.bmm(gv.transpose(1, 2), av).float().sum(0)


def _acc(grads, p, g):
    grads[p] = g if p not in grads else grads[p] + g        # (no `0 + g` launch for the first contribution)


P = _lib.ptr


# ---- edge part -------------------------------------------------------------------------------------------------------------
def _first_layer_operands(s, lin):
    """per-node halves P, Q of the first Linear layer (:56's concatenation factorised), its d2 column and its dgrad operand"""
    w, H = lin.weight.detach(), s.H
    if s.bp.hip_gemms:   # the fused kernels take P / Q from the forward's table; the dgrad runs on packed fragments
        from .gemm import pack_rows_weights
        return None, None, None, (None if s.bp.first else pack_rows_weights(w.float().contiguous(), 2 * H + 1))
    Pn = (s.mm(s.h, w[:, :H].t().contiguous()) + lin.bias.detach()).contiguous()
    Qn = s.mm(s.h, w[:, H:2 * H].t().contiguous()).contiguous()
    wpad = torch.zeros(w.shape[0], s.bp.K1P, dtype=s.bp.dtype, device=s.h.device)
    wpad[:, :2 * H + 1] = w
    return Pn, Qn, w[:, 2 * H].contiguous(), wpad


def _edge_setup(bp, layer, ws, fused, kept, h, x, graph, node_seg, g_am, g_ax, g_S, g_h, g_x):
    """weights in the operand form the plan needs and the zero-filled fp32 accumulators of one layer"""
    s = SimpleNamespace(bp=bp, ws=ws, kept=kept, h=h, x=x, graph=graph, node_seg=node_seg,
                        g_S=g_S, g_h=g_h, g_x=g_x, L=_lib.lib(), st=_lib.stream_ptr(), H=h.shape[1], N=h.shape[0],
                        dst32=graph.edge_dst, src32=graph.edge_src, E=graph.edge_dst.numel(),
                        mm=partial(_mm, bp.split_products), wgrad=partial(_wgrad, bp.split_products))
    s.lin_x0, s.lin_x2, s.lin_x4 = layer.mlp_x[0], layer.mlp_x[2], layer.mlp_x[4]
    s.lin_m0, s.lin_m2, s.att = layer.mlp_m[0], layer.mlp_m[2], layer.attention[0]
    H, K1P, dt = s.H, bp.K1P, bp.dtype
    Wx, Wm, M = s.Wx, s.Wm, s.M = s.lin_x0.out_features, s.lin_m0.out_features, s.lin_m2.out_features
    f32 = dict(dtype=torch.float32, device=h.device)
    s.Px, s.Qx, s.wdx, s.w1x = _first_layer_operands(s, s.lin_x0)
    s.Pm, s.Qm, s.wdm, s.w1m = _first_layer_operands(s, s.lin_m0)
    s.w2x, s.w2m = s.lin_x2.weight.detach().to(dt), s.lin_m2.weight.detach().to(dt)
    s.b2x, s.b2m = s.lin_x2.bias.detach().contiguous(), s.lin_m2.bias.detach().contiguous()
    s.w3, s.b3 = s.lin_x4.weight.detach().reshape(-1).contiguous(), s.lin_x4.bias.detach().contiguous()
    s.wa, s.ba = s.att.weight.detach().reshape(-1).contiguous(), s.att.bias.detach().contiguous()
    # fp32 accumulators; the first Linear layers carry their bias gradient in column 2H+1 (ones column of `in`)
    # (one zero fill for all of them: a dozen 5-us launches per layer otherwise; every piece starts at a multiple of 4 floats)
    shapes = [(Wx, K1P), (Wm, K1P), (Wx, Wx), (M, Wm), (Wx,), (Wx,), (4,), (M,), (M,), (4,), (graph.B, Wx), (graph.B, Wm)]
    sizes = [_round_up(math.prod(sh), 4) for sh in shapes]
    flat = torch.zeros(sum(sizes), **f32)
    offs = [sum(sizes[:i]) for i in range(len(sizes))]
    (s.g_w1x, s.g_w1m, s.g_w2x, s.g_w2m, s.g_b2x, s.g_w3, g_b3, s.g_b2m, s.g_wa, g_ba, s.cd_x,
     s.cd_m) = (flat[o:o + math.prod(sh)].view(*sh) for o, sh in zip(offs, shapes))
    s.g_b3, s.g_ba = g_b3[:1], g_ba[:1]
    s.g_am, s.g_ax = g_am.contiguous(), g_ax.contiguous()
    s.sums = tuple(P(t) for t in (s.g_b2x, s.g_w3, s.g_b3, s.g_b2m, s.g_wa, s.g_ba))   # the bias / w3 / wa column sums
    s.handle_args = (fused[0], s.st, fused[1], P(x))                                   # head of every context-handle call
    if bp.first:   # per-node sums of dL/da1 over the edges a node receives (Gd) / sends (Gs), and the partial sums of dL/d(d2)
        s.nparts = (Wx + Wm) // 256
        s.gd2_part = torch.empty(s.nparts * min(bp.rows, s.E), **f32)
    if bp.first == "graph":     # the kernel leaves the sums as the bf16 operands of the node-level products: [Gd_x | Gs_x | Gd_m | Gs_m]
        s.G = torch.zeros(s.N, 2 * Wx + 2 * Wm, dtype=torch.bfloat16, device=h.device)
    elif bp.first == "reduce":
        s.Gd_x, s.Gs_x, s.Gd_m, s.Gs_m = (torch.zeros(s.N, w, **f32) for w in (Wx, Wx, Wm, Wm))
        s.wdx_f = s.lin_x0.weight.detach()[:, 2 * H].float().contiguous()
        s.wdm_f = s.lin_m0.weight.detach()[:, 2 * H].float().contiguous()
    return s


def _chunk(s, a, n):
    """views of edges [a, a + n) on the workspace (or on the layer-long kept buffers, whose rows beyond E are zero), and d2"""
    ws, n_pad = s.ws, _round_up(n, 64)
    c = SimpleNamespace(a=a, n=n, n_pad=n_pad, d32=s.dst32[a:a + n], s32=s.src32[a:a + n], d2=ws.d2[:n], g_diff=ws.g_diff[:n])
    if s.bp.kept:
        c.S1X, c.S1M, c.A2X, c.A2M = (t[a:a + n_pad] for t in s.kept[:4])
    else:
        c.S1X, c.S1M, c.A2X, c.A2M = ws.s1x, ws.s1m, ws.a2x, ws.a2m
    c.s1x, c.s1m, c.a2x, c.a2m = c.S1X[:n], c.S1M[:n], c.A2X[:n], c.A2M[:n]
    if s.bp.first != "graph":   # (the 'graph' form has no dL/da1 in memory)
        c.g1x, c.g1m = ws.g1x[:n], ws.g1m[:n]
    if s.bp.first is None:
        c.inp, c.g_in = ws.inp[:n], ws.g_in[:n]
    if n_pad > n and not s.bp.hip_gemms:   # rows the library products read beyond the chunk (the own GEMMs stop at row n)
        for t in ((ws.g1x, ws.g1m, ws.inp) if s.bp.kept else (ws.s1x, ws.s1m, ws.a2x, ws.a2m, ws.g1x, ws.g1m, ws.inp)):
            t[n:n_pad].zero_()
    if s.bp.first is None:   # the chain's gathered inputs [h_i | h_j | d2 | 1]
        _lib.check(s.L.egcl_backward_gather_in(s.st, s.bp.prec, n, s.H, s.bp.K1P, P(c.d32), P(c.s32), P(s.h), P(s.x), P(c.inp), P(c.d2)))
    return c


def _a2_saved(s, c):
    """dL/da2 in place over the kept pre-activations, g_diff and the bias / w3 / wa column sums: one element-wise pass"""
    _lib.check(s.L.egcl_backward_heads_saved(*s.handle_args, P(s.g_ax), P(s.g_am), c.a, c.n, P(c.a2x), P(c.a2m), P(s.kept[4]),
                                             P(c.g_diff), *s.sums))


def _a2_recompute(s, c):
    """s1 (scaled by -log2 e), dL/da2, g_diff and the bias / w3 / wa column sums in one pass of the MFMA edge kernels"""
    _lib.check(s.L.egcl_backward_edge_recompute(*s.handle_args, P(s.g_ax), P(s.g_am), c.a, c.n, P(c.s1x), P(c.s1m), P(c.a2x),
                                                P(c.a2m), P(c.g_diff), *s.sums))


def _a2_chain(s, c):
    L, st, prec, n = s.L, s.st, s.bp.prec, c.n
    _lib.check(L.egcl_backward_l1_act(st, prec, n, s.Wx, P(c.d32), P(c.s32), P(s.Px), P(s.Qx), P(s.wdx), P(c.d2), P(c.s1x)))
    _lib.check(L.egcl_backward_l1_act(st, prec, n, s.Wm, P(c.d32), P(c.s32), P(s.Pm), P(s.Qm), P(s.wdm), P(c.d2), P(c.s1m)))
    s.mm(c.s1x, s.w2x.t().contiguous(), out=c.a2x)
    s.mm(c.s1m, s.w2m.t().contiguous(), out=c.a2m)
    _lib.check(L.egcl_backward_heads(st, prec, n, s.Wx, s.M, P(c.d32), P(c.s32), P(s.x), P(s.g_ax), P(s.g_am), P(c.a2x), P(c.a2m),
                                     P(s.b2x), P(s.w3), P(s.b3), P(s.b2m), P(s.wa), P(s.ba), P(c.g_diff), *s.sums))


def _w2_own(s, c):
    """reductions over the chunk's edges on the library's own split-K kernel (gemm_tn.hip), fp32 accumulate
    (the recompute / keeping kernels store s1 as the MFMA consumed it, -log2(e) * SiLU(a1): undone by the scale.
    Measured and dropped: the message head on a second stream beside the coordinate MLP's product -- HBM-bound
    beside MFMA-bound -- made the step 1.0 ms LONGER, 51.8 vs 50.8 ms on one box)"""
    from .gemm import gemm_tn
    gemm_tn(c.a2x, c.s1x, out=s.g_w2x, accumulate=True, scale=-math.log(2.0))
    gemm_tn(c.a2m, c.s1m, out=s.g_w2m, accumulate=True, scale=-math.log(2.0))


def _w2_library(s, c):
    s.g_w2x += s.wgrad(c.A2X, c.S1X, c.n_pad, 16)
    s.g_w2m += s.wgrad(c.A2M, c.S1M, c.n_pad, 32)


def _da1_graph(s, c):
    """dgrad of the second layers, SiLU'(a1) and the first layers' per-node sums in one kernel: no dL/da1 in memory"""
    _lib.check(s.L.egcl_backward_dgrad_reduce(*s.handle_args, c.a, c.n, P(c.a2x), P(c.a2m), P(s.G), P(s.cd_x), P(s.cd_m),
                                              P(s.gd2_part)))


def _da1_fused(s, c):
    """dgrad of the second layers with SiLU'(a1) in the epilogue, on MFMA (no [n, W] round trip in between)"""
    _lib.check(s.L.egcl_backward_dgrad(*s.handle_args, c.a, c.n, P(c.a2x), P(c.a2m), P(c.g1x), P(c.g1m)))


def _da1_chain(s, c):
    L, st, prec, n = s.L, s.st, s.bp.prec, c.n
    s.mm(c.a2x, s.w2x, out=c.g1x)
    s.mm(c.a2m, s.w2m, out=c.g1m)
    _lib.check(L.egcl_backward_l1_grad(st, prec, n, s.Wx, P(c.d32), P(c.s32), P(s.Px), P(s.Qx), P(s.wdx), P(c.d2), P(c.g1x)))
    _lib.check(L.egcl_backward_l1_grad(st, prec, n, s.Wm, P(c.d32), P(c.s32), P(s.Pm), P(s.Qm), P(s.wdm), P(c.d2), P(c.g1m)))


def _first_factorised(s, c):
    """per-node sums of dL/da1 (already taken by the "graph" form's dgrad kernel) and the geometric half of the scatter"""
    g = s.graph
    if s.bp.first == "reduce":
        _lib.check(s.L.egcl_backward_first_reduce(s.st, g.B, g.max_graph_nodes, c.a, c.n, P(g.graph_ptr), P(g.row_ptr), P(s.src32),
                                                  P(s.x), P(c.g1x), s.Wx, P(c.g1m), s.Wm, P(s.wdx_f), P(s.wdm_f), P(s.Gd_x),
                                                  P(s.Gs_x), P(s.Gd_m), P(s.Gs_m), P(s.cd_x), P(s.cd_m), P(s.gd2_part)))
    _lib.check(s.L.egcl_backward_scatter_geom(s.st, c.n, s.nparts, P(c.d32), P(c.s32), P(s.x), P(s.gd2_part), P(c.g_diff), P(s.g_S),
                                              P(s.node_seg), P(s.g_x)))


def _scatter(s, c):
    _lib.check(s.L.egcl_backward_scatter(s.st, s.bp.prec, c.n, s.H, s.bp.K1P, P(c.d32), P(c.s32), P(s.x), P(c.g_in), P(c.g_diff),
                                         P(s.g_S), P(s.node_seg), P(s.g_h), P(s.g_x)))


def _first_own(s, c):
    """wgrad against in = [h_i | h_j | d2 | 1] and dgrad back to the gathered inputs on the own kernels"""
    from .gemm import gemm_rows, gemm_tn
    gemm_tn(c.g1x, c.inp, cols=2 * s.H + 2, out=s.g_w1x, accumulate=True)
    gemm_tn(c.g1m, c.inp, cols=2 * s.H + 2, out=s.g_w1m, accumulate=True)
    gemm_rows(c.g1x, s.w1x, c.g1m, s.w1m, out=c.g_in)      # row-streaming product (gemm_rows.hip): every dL/da1 row read once
    _scatter(s, c)


def _first_library(s, c):
    s.g_w1x += s.wgrad(s.ws.g1x, s.ws.inp, c.n_pad, 32)
    s.g_w1m += s.wgrad(s.ws.g1m, s.ws.inp, c.n_pad, 32)
    s.mm(c.g1x, s.w1x, out=c.g_in)
    c.g_in += s.mm(c.g1m, s.w1m)
    _scatter(s, c)


def _stages(bp):
    """the per-chunk routines of a plan: (dL/da2, second-layer wgrad, dL/da1, first layers + scatter)"""
    return (_a2_saved if bp.kept else _a2_recompute if bp.fused else _a2_chain,
            _w2_own if bp.hip_gemms else _w2_library,
            _da1_graph if bp.first == "graph" else _da1_fused if bp.fused else _da1_chain,
            _first_factorised if bp.first else _first_own if bp.hip_gemms else _first_library)


def _finish_graph(s):
    """node-level products of the factorised first layers on the library's own GEMMs (N rows, bf16 operands)"""
    from .gemm import gemm_rows, gemm_tn, pack_rows_weights
    H, N, Wx, Wm, G = s.H, s.N, s.Wx, s.Wm, s.G
    hb = torch.zeros(N, 128, dtype=torch.bfloat16, device=s.h.device)
    hb[:, :H] = s.h
    hb[:, H] = 1.0                                       # (ones column: the bias gradients = column sums of Gd)
    Wg = gemm_tn(G, hb, cols=H + 1)                      # [2 Wx + 2 Wm, H + 1] = G^T [h | 1]
    for g_w1, o, W, cd in ((s.g_w1x, 0, Wx, s.cd_x), (s.g_w1m, 2 * Wx, Wm, s.cd_m)):
        g_w1[:, :H] = Wg[o:o + W, :H]
        g_w1[:, H:2 * H] = Wg[o + W:o + 2 * W, :H]
        g_w1[:, 2 * H] = cd.sum(0)
        g_w1[:, 2 * H + 1] = Wg[o:o + W, H]
    # dL/dh += Gd W1[:, :H] + Gs W1[:, H:2H] for both MLPs: one row-streaming product over [Gd | Gs] (K = 2 W each)
    wcat = [pack_rows_weights(torch.cat([lin.weight.detach()[:, :H], lin.weight.detach()[:, H:2 * H]], 0).float().contiguous(), H)
            for lin in (s.lin_x0, s.lin_m0)]
    gh_add = torch.empty(N, 128, dtype=torch.float32, device=s.h.device)
    gemm_rows(G[:, :2 * Wx], wcat[0], G[:, 2 * Wx:], wcat[1], out=gh_add)
    s.g_h += gh_add[:, :H]


def _finish_reduce(s):
    """the same products for the reference form: fp32 library products"""
    H, hf = s.H, s.h.float()
    for g_w1, Gd, Gs, cd, lin in ((s.g_w1x, s.Gd_x, s.Gs_x, s.cd_x, s.lin_x0), (s.g_w1m, s.Gd_m, s.Gs_m, s.cd_m, s.lin_m0)):
        g_w1[:, :H] = Gd.t() @ hf
        g_w1[:, H:2 * H] = Gs.t() @ hf
        g_w1[:, 2 * H] = cd.sum(0)
        g_w1[:, 2 * H + 1] = Gd.sum(0)
        w1 = lin.weight.detach().float()
        s.g_h.addmm_(Gd, w1[:, :H])
        s.g_h.addmm_(Gs, w1[:, H:2 * H])


def _edge_finish(s, grads):
    H = s.H
    if s.bp.fused and not s.bp.hip_gemms:   # the recompute kernels store s1 as the MFMA consumed it: -log2(e) * SiLU(a1)
        s.g_w2x *= -math.log(2.0)
        s.g_w2m *= -math.log(2.0)
    if s.bp.first == "graph":
        _finish_graph(s)
    elif s.bp.first == "reduce":
        _finish_reduce(s)
    for p, g in ((s.lin_x0.weight, s.g_w1x[:, :2 * H + 1]), (s.lin_x0.bias, s.g_w1x[:, 2 * H + 1]),
                 (s.lin_m0.weight, s.g_w1m[:, :2 * H + 1]), (s.lin_m0.bias, s.g_w1m[:, 2 * H + 1]),
                 (s.lin_x2.weight, s.g_w2x), (s.lin_x2.bias, s.g_b2x), (s.lin_m2.weight, s.g_w2m), (s.lin_m2.bias, s.g_b2m),
                 (s.lin_x4.weight, s.g_w3), (s.lin_x4.bias, s.g_b3), (s.att.weight, s.g_wa), (s.att.bias, s.g_ba)):
        _acc(grads, p, g.reshape(p.shape).contiguous())


def _edge_backward(bp, layer, ws, fused, kept, h, x, graph, node_seg, g_am, g_ax, g_S, g_h, g_x, grads):
    """adds the edge part's contributions to g_h, g_x and to the parameter gradients in `grads`.  ``fused`` = (context handle or
    None, layer index); ``kept`` = (s1x, s1m, t2x, t2m, s_shares) of this layer when the forward ran as egcl_forward_save."""
    s = _edge_setup(bp, layer, ws, fused, kept, h, x, graph, node_seg, g_am, g_ax, g_S, g_h, g_x)
    if bp.fused:
        _lib.check(s.L.egcl_backward_table(*s.handle_args[:3], P(h)))
    a2, w2, da1, first_layers = _stages(bp)
    for a, n in bp.chunks:
        c = _chunk(s, a, n)
        a2(s, c)             # a2x / a2m now hold dL/da2
        w2(s, c)
        da1(s, c)
        first_layers(s, c)
    _edge_finish(s, grads)


# ---- node part -------------------------------------------------------------------------------------------------------------
def _zero(o, like):
    return o.clone() if o is not None else torch.zeros_like(like)


def _segment_scale(S, scope_graph, node_graph):
    G = torch.sqrt(S.clamp_min(1e-30))   # graphs without edges: S = 0, zero gradient
    c = 1.0 / (G + 1.0)
    return c.index_select(0, node_graph).unsqueeze(1) if scope_graph else c


def _coordinate_update(x_l, sum_x, S, scope_graph, node_graph):
    """x' = x + sum_x / (G + 1) (:64, :70) on torch's tape (element-wise): x' and its leaves (x, sum_x, S)"""
    leaves = [t.detach().requires_grad_(True) for t in (x_l, sum_x, S)]
    return leaves[0] + leaves[1] * _segment_scale(leaves[2], scope_graph, node_graph), leaves


def _coordinate_backward(x_l, sum_x, S, gx, scope_graph, node_graph):
    """dL/dx, dL/d sum_x, dL/dS of the coordinate update"""
    with torch.enable_grad():
        x_new, leaves = _coordinate_update(x_l, sum_x, S, scope_graph, node_graph)
        o = torch.autograd.grad([x_new], leaves, [gx], allow_unused=True)
    return _zero(o[0], x_l), _zero(o[1], sum_x), _zero(o[2], S)


def _node_backward_hip(layer, h_l, sum_m, gh, grads):
    """backward of h' = mlp_h([h | sum_m]) (EquivariantGraphNeuralNetwork.py:26-30, :69) on the library's own GEMM kernels
    (bf16 operands, fp32 accumulate and fp32 pre-activations): recompute z1 = W1 [h | sum_m] + b1, then
        dL/ds = gh W2,  dL/dz1 = dL/ds * SiLU'(z1),  dL/d[h | sum_m] = dL/dz1 W1,
        dL/dW2 = gh^T SiLU(z1),  dL/dW1 = dL/dz1^T [h | sum_m],  bias gradients = column sums.
    Returns (dL/dh [N, H], dL/d sum_m [N, M]); parameter gradients are added to `grads`."""
    from .gemm import gemm_tn, linear_rows
    lin1, lin2 = layer.mlp_h[0], layer.mlp_h[2]
    N, H = h_l.shape
    M = sum_m.shape[1]
    K1 = H + M
    K1k, K1n = _round_up(K1, 64), _round_up(K1, 128)              # reduction width (gemm_rows) / operand width (gemm_tn)
    bf = dict(dtype=torch.bfloat16, device=h_l.device)
    hcat = torch.zeros(N, max(K1k, K1n), **bf)
    hcat[:, :H] = h_l
    hcat[:, H:K1] = sum_m
    z1 = linear_rows(hcat, lin1.weight, k=K1k)                    # (without the bias: the activation stage adds it)
    ghb = torch.zeros(N, 128, **bf)                               # gh as a GEMM operand: H <= 64 real columns
    ghb[:, :H] = gh
    g_s = linear_rows(ghb, lin2.weight.detach().t(), k=64)        # [N, Wh] = gh @ W2
    Wh = lin1.weight.shape[0]
    # s = SiLU(z1 + b1), dL/dz1 = dL/ds * SiLU'(z1 + b1) as bf16 operands and the bias gradient, in one pass (backward.hip)
    g_z1b, s_b = torch.empty(N, Wh, **bf), torch.empty(N, Wh, **bf)
    g_b1 = torch.zeros(Wh, dtype=torch.float32, device=h_l.device)
    _lib.check(_lib.lib().egcl_backward_node_act(_lib.stream_ptr(), N, Wh, P(z1), z1.stride(0), P(lin1.bias.detach()),
                                                 P(g_s), g_s.stride(0), P(g_z1b), P(s_b), Wh, P(g_b1)))
    _acc(grads, lin2.bias, gh.sum(0))
    _acc(grads, lin1.bias, g_b1)
    _acc(grads, lin2.weight, gemm_tn(s_b, ghb, rows=Wh, cols=H).t())                     # [Wh, H]^T
    _acc(grads, lin1.weight, gemm_tn(g_z1b, hcat, rows=Wh, cols=K1))                     # [Wh, H + M]
    g_cat = linear_rows(g_z1b, lin1.weight.detach().t())                                 # [N, H + M] = dL/dz1 @ W1
    return g_cat[:, :H].contiguous(), g_cat[:, H:K1].contiguous()


def _node_backward_split(layer, h_l, sum_m, gh, grads):
    """the formulas of _node_backward_hip for the fp32-grade precisions on the library's own kernels: every product as head +
    remainder (gemm.mm_nn_split / mm_tn_split, no BLAS library) and the element-wise stages in fp32 by torch"""
    lin1, lin2, split = layer.mlp_h[0], layer.mlp_h[2], True   # (the plan picks this form only with split_products)
    H = h_l.shape[1]
    w1, w2 = lin1.weight.detach().float(), lin2.weight.detach().float()
    hcat = torch.cat((h_l, sum_m), dim=1).float()
    z1 = _mm(split, hcat, w1.t().contiguous()) + lin1.bias.detach()
    sg = torch.sigmoid(z1)
    s = z1 * sg
    g_s = _mm(split, gh.float().contiguous(), w2)               # [N, Wh] = gh @ W2
    g_z1 = g_s * (sg * (1.0 + z1 * (1.0 - sg)))                 # SiLU'(z1)
    _acc(grads, lin2.bias, gh.sum(0))
    _acc(grads, lin1.bias, g_z1.sum(0))
    _acc(grads, lin2.weight, _wgrad(split, gh.float().contiguous(), s, gh.shape[0], 1))     # [H, Wh]
    _acc(grads, lin1.weight, _wgrad(split, g_z1, hcat, hcat.shape[0], 1))                   # [Wh, H + M]
    g_cat = _mm(split, g_z1, w1)                                                            # [N, H + M]
    return g_cat[:, :H].contiguous(), g_cat[:, H:].contiguous()


def _node_backward_torch(layer, h_l, sum_m, gh, grads, x_l, sum_x, S, gx, scope_graph, node_graph):
    """the whole node part on ONE torch tape, the coordinate update included (its launch order is the one this form always had):
    exact fp32 products of the BLAS library -- parity mode, and shapes the own kernels do not tile.
    Returns dL/dh, dL/d sum_m, dL/dx, dL/d sum_x, dL/dS"""
    node_params = list(layer.mlp_h.parameters())
    with torch.enable_grad():
        h_leaf, am = h_l.detach().requires_grad_(True), sum_m.detach().requires_grad_(True)
        h_new = layer.mlp_h(torch.cat((h_leaf, am), dim=1))
        x_new, (x_leaf, ax, S_leaf) = _coordinate_update(x_l, sum_x, S, scope_graph, node_graph)
        outs = torch.autograd.grad([h_new, x_new], [h_leaf, x_leaf, am, ax, S_leaf] + node_params, [gh, gx], allow_unused=True)
    g_h, g_x = _zero(outs[0], h_l), _zero(outs[1], x_l)
    g_am, g_ax, g_S = _zero(outs[2], sum_m), _zero(outs[3], sum_x), _zero(outs[4], S)
    for p, g in zip(node_params, outs[5:]):
        if g is not None:
            _acc(grads, p, g)
    return g_h, g_am, g_x, g_ax, g_S


class _EGNNFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, layers, plan, prec, scope, h, x, *params):
        from .egnn import _context
        c = _context(owner, layers, h.device)
        c.set_graph(plan)
        c.pack(layers)
        L, sw = _lib.lib(), _switches()
        nseg = plan.B if scope == _lib.NORM_GRAPH else 1
        saved = []
        hc, xc = h.detach().float().contiguous(), x.detach().float().contiguous()
        kept, E = None, plan.E
        Wx, Wm, M = layers[0].mlp_x[0].out_features, layers[0].mlp_m[0].out_features, layers[0].dims["M"]
        Epad = _round_up(E, 64)
        if _keep_asked(prec, E, sw) and bool(L.egcl_backward_fused_supported(c.handle)):
            # decided ONCE per (edge count, widths) on the context: "free" = what the driver reports plus what the caching
            # allocator holds reserved but unallocated (after the first step the kept buffers sit there), so the path does
            # not flip between steps or between ranks that share a device
            key = (Epad, len(layers), Wx, Wm, M)
            cache = getattr(c, "_keep_decision", None)
            if cache is None or cache[0] != key:
                free = torch.cuda.mem_get_info(hc.device)[0] + (torch.cuda.memory_reserved(hc.device) -
                                                                torch.cuda.memory_allocated(hc.device))
                cache = c._keep_decision = (key, decide_keep(prec, E, len(layers), Wx, Wm, M, sw, True, free))
            if cache[1]:
                kept = []
        if E > 0 and prec == _lib.PREC_BF16:   # (bench.py reads it; EGNN_BWD_SAVE=0 / unsupported shapes: nothing is kept)
            c.last_backward_path = "kept activations" if kept is not None else "recompute"
        for l in range(len(layers)):
            ho, xo = torch.empty_like(hc), torch.empty_like(xc)
            if kept is not None:
                bf = dict(dtype=torch.bfloat16, device=hc.device)
                bufs = [torch.empty(Epad, Wx, **bf), torch.empty(Epad, Wm, **bf), torch.empty(Epad, Wx, **bf),
                        torch.empty(Epad, M, **bf), torch.empty(max(Wx // 512, 1), E, device=hc.device)]
                if sw["POISON_KEPT"]:   # (tests: an element the forward leaves unwritten and the backward reads shows up as NaN)
                    for t in bufs:
                        t.fill_(float("nan"))
                if Epad > E:
                    for t in bufs[:4]:
                        t[E:].zero_()
                _lib.check(L.egcl_forward_save(c.handle, _lib.stream_ptr(), l, scope, P(hc), P(xc), P(ho), P(xo), *[P(t) for t in bufs]))
                kept.append(bufs)
            else:
                _lib.check(L.egcl_forward(c.handle, _lib.stream_ptr(), l, prec, scope, P(hc), P(xc), P(ho), P(xo)))
            sum_m = torch.empty(hc.shape[0], layers[l].dims["M"], device=hc.device)
            sum_x = torch.empty(hc.shape[0], 3, device=hc.device)
            S = torch.empty(nseg, device=hc.device)
            _lib.check(L.egcl_read_aggregates(c.handle, _lib.stream_ptr(), scope, P(sum_m), P(sum_x), P(S)))
            saved += [hc, xc, sum_m, sum_x, S]
            hc, xc = ho, xo
        ctx.layers, ctx.plan, ctx.scope, ctx.prec, ctx.egnn_ctx, ctx.kept = layers, plan, scope, prec, c, kept
        ctx.save_for_backward(*saved)
        return hc, xc

    @staticmethod
    def backward(ctx, gh, gx):
        global LAST_PLAN, LAST_FIRST_LAYER_FORM
        layers, graph, c, sw = ctx.layers, ctx.plan, ctx.egnn_ctx, _switches()
        scope_graph = ctx.scope == _lib.NORM_GRAPH
        saved = ctx.saved_tensors
        node_graph = graph.node_graph.long()
        node_seg = graph.node_graph if scope_graph else None   # int32 segment of the d^2 sum each node belongs to
        gh = torch.zeros_like(saved[0]) if gh is None else gh.contiguous().float()
        gx = torch.zeros_like(saved[1]) if gx is None else gx.contiguous().float()
        grads = {}
        d0, E = layers[0].dims, graph.edge_dst.numel()
        Wx, Wm = layers[0].mlp_x[0].out_features, layers[0].mlp_m[0].out_features
        # the kept activations are spent by the first backward (dL/da2 is written over them): a second backward through
        # the same graph (retain_graph=True) is planned as recompute
        kept = ctx.kept if ctx.kept is not None and all(k is not None for k in ctx.kept) else None
        supported = False
        if fused_asked(ctx.prec, E, kept is not None, sw):
            c.set_graph(graph)
            c.pack(layers)
            supported = bool(_lib.lib().egcl_backward_fused_supported(c.handle))
        bp = LAST_PLAN = plan_backward(ctx.prec, d0["H"], Wx, Wm, d0["M"], layers[0].mlp_h[0].weight.shape[0], E, EDGE_CHUNK,
                                       getattr(graph, "graph_edge_ptr", None), getattr(graph, "max_graph_nodes", 1 << 30),
                                       kept is not None, supported, sw)
        if E > 0:
            LAST_FIRST_LAYER_FORM = bp.first
            ws = _Workspace(bp, Wx, Wm, d0["M"], gh.device)
        for l in reversed(range(len(layers))):
            layer = layers[l]
            h_l, x_l, sum_m, sum_x, S = saved[5 * l:5 * l + 5]
            if bp.node == "torch":
                g_h, g_am, g_x, g_ax, g_S = _node_backward_torch(layer, h_l, sum_m, gh, grads, x_l, sum_x, S, gx, scope_graph, node_graph)
            else:
                g_x, g_ax, g_S = _coordinate_backward(x_l, sum_x, S, gx, scope_graph, node_graph)
                g_h, g_am = (_node_backward_hip if bp.node == "hip" else _node_backward_split)(layer, h_l, sum_m, gh, grads)
            if E > 0:
                _edge_backward(bp, layer, ws, (c.handle if bp.fused else None, l), kept[l] if kept is not None else None, h_l, x_l,
                               graph, node_seg, g_am, g_ax, g_S.contiguous(), g_h, g_x, grads)
                if kept is not None:
                    ctx.kept[l] = None   # this layer's buffers are spent
            gh, gx = g_h, g_x
            red = ACTIVE_REDUCER
            if red is not None and id(layer) in red.bucket_of:
                ps = red.buckets[red.bucket_of[id(layer)]]
                for p_, g_ in zip(ps, red.layer_ready(layer, [grads.get(p_) for p_ in ps])):
                    grads[p_] = g_
        if ACTIVE_REDUCER is not None:
            ACTIVE_REDUCER.sync()
        flat = []
        for layer in layers:
            for p in layer._ordered_params():
                g = grads.get(p, None)
                flat.append(g if torch.is_tensor(g) else None)
        return (None, None, None, None, None, gh, gx, *flat)


def egnn_forward_autograd(owner, layers, edge_index, h, x, batch):
    from .egnn import _plan_for
    if not (h.is_cuda and x.is_cuda):
        raise RuntimeError("training needs CUDA(ROCm) tensors; there is no CPU fallback")
    plan = _plan_for(owner, edge_index, h.shape[0], batch)
    prec = _lib.PRECISIONS[owner.precision]
    scope = _lib.NORM_SCOPES[owner.norm_scope]
    params = [p for layer in layers for p in layer._ordered_params()]
    return _EGNNFunction.apply(owner, layers, plan, prec, scope, h, x, *params)

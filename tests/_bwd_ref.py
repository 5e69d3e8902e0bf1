"""float64 restatement of ONE EGCL layer's edge backward, stage by stage (test infrastructure, no HIP).

One function per stage of the C ABI (include/egnn_amd.h, "backward of one EGCL layer"), taking and returning what the entry
point takes and returns.  Math: diffusion_model_amd/autograd.py (module docstring), csrc/edge_bwd_heads.hip:9-12,
csrc/edge_bwd_dgrad_graph.hip:5-8.  Per edge e = (i <- j), in = [h_i | h_j | d2]:

    a1 = P[i] + Q[j] + wd d2          s1 = SiLU(a1)         a2 = W2 s1 + b2
    x branch: s_e = w3 . SiLU(a2x) + b3,  xm = (x_i - x_j) s_e       m branch: m = SiLU(a2m), out = m sigmoid(wa . m + ba)

Every function has two modes:
  model=False  the mathematical operation in float64 on the operands as handed in;
  model=True   the same with ONLY the roundings the kernels document (cited at each function); values that the bf16 fast path
               keeps scaled by -log2(e) (kernels.h:15-18: SiLU is evaluated as t / (1 + 2^t) on t = -log2(e) z) are kept in
               that scale ("scaled") exactly where the kernels keep them.
Every sum comes with `abs_*`: per output element the sum of |terms| it was formed from, for the element-wise bound
K 2^-24 sum|terms| of an fp32 accumulation of K terms (acc_bound()).
"""
from types import SimpleNamespace as NS

import torch

D = torch.float64
LOG2E = 1.4426950408889634
# the two constants as the kernels hold them (kernels.h:17-18, constexpr float)
K_NEG_LOG2E = float(torch.tensor(-1.4426950408889634, dtype=torch.float32))
K_NEG_LN2 = float(torch.tensor(-0.6931471805599453, dtype=torch.float32))
EPS32 = 2.0 ** -24


def d(t):
    return t.detach().to(D)


def f32(t):
    return t.to(torch.float32).to(D)


def bf16(t):
    """round to bf16 the way the kernels do: from the fp32 value, nearest even"""
    return t.to(torch.float32).to(torch.bfloat16).to(D)


def fp16(t):
    return t.to(torch.float32).to(torch.float16).to(D)


def ulp_bf16(t):
    """spacing of bf16 numbers at |t| (8 significant bits; below 2^-126 the subnormal spacing 2^-133)"""
    e = torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


def ulp_fp16(t):
    e = torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def act(a, scaled=False):
    """(SiLU(z), SiLU'(z), sigmoid(z)) in natural units of z; scaled: a = t = -log2(e) z as the fast path holds it
    (kernels.h:265-269 silu_grad_s: sg = 1 / (1 + 2^t), s = (t * -ln 2) sg, ds = s (1 - sg) + sg)"""
    if scaled:
        sg = 1.0 / (1.0 + torch.exp2(a))
        s = (a * K_NEG_LN2) * sg
    else:
        sg = torch.sigmoid(a)
        s = a * sg
    return s, sg + s * (1.0 - sg), sg


def geometry(x, dst, src, model=False):
    """diff = x_i - x_j and d2 = |diff|^2 (every kernel takes the difference of the fp32 coordinates in fp32:
    backward.hip:196, edge_bwd_first.hip:104, edge_bwd_dgrad.hip:167)"""
    diff = d(x)[dst] - d(x)[src]
    if model:
        diff = f32(diff)
    return diff, (diff * diff).sum(1)


# ---------------------------------------------------------------------------------------------------------------------------
def tables(h, W1, b1, H, model=False):
    """P = h W1[:, :H]^T + b1, Q = h W1[:, H:2H]^T, wd = W1[:, 2H] (egcl_backward_table; generic chain: autograd.py:_first_layer_operands).
    model: the fast path's table -- weights and bias times -log2(e) rounded to fp32 (pack.hip: egnn_pack_layer, scale_copy),
    entries clamped to +-32000 and rounded to fp16 (egnn_forward.hip: table_store); returns SCALED values."""
    h, W1, b1 = d(h), d(W1), d(b1)
    if model:
        W1, b1 = f32(W1 * K_NEG_LOG2E), f32(b1 * K_NEG_LOG2E)
    P = h @ W1[:, :H].t() + b1
    Q = h @ W1[:, H:2 * H].t()
    absP = h.abs() @ W1[:, :H].abs().t() + b1.abs()
    absQ = h.abs() @ W1[:, H:2 * H].abs().t()
    if model:
        P, Q = fp16(P.clamp(-32000.0, 32000.0)), fp16(Q.clamp(-32000.0, 32000.0))
    return NS(P=P, Q=Q, wd=W1[:, 2 * H].clone(), abs_P=absP, abs_Q=absQ, scaled=model)


def first_pre(tab, d2, dst, src, model=False):
    """a1 = P[i] + Q[j] + wd d2.  model (fast path): P + Q added in fp16, then one fp32 fma
    (edge_bwd_dgrad.hip:99,108; edge_bwd_dgrad_graph.hip:280-288 "added in fp16 as the forward adds them")"""
    pq = tab.P[dst] + tab.Q[src]
    if model and tab.scaled:
        pq = fp16(pq)
    a1 = pq + tab.wd * d2[:, None]
    return f32(a1) if model else a1


def l1_act(tab, d2, dst, src, model=False, store=None):
    """egcl_backward_l1_act: s1 = SiLU(P[i] + Q[j] + wd d2) (backward.hip:104-127; fp32 tables, unscaled);
    store = bf16 rounds the stored activation (backward.hip:24)"""
    s, _, _ = act(first_pre(tab, d2, dst, src, model), tab.scaled)
    return store(s) if store else s


def l1_grad(g_s1, tab, d2, dst, src, model=False, store=None):
    """egcl_backward_l1_grad: g_s1 * SiLU'(a1), in place on the stored buffer (backward.hip:119-126)"""
    _, ds, _ = act(first_pre(tab, d2, dst, src, model), tab.scaled)
    g = d(g_s1) * ds
    return store(g) if store else g


def forward_kept(tab_x, tab_m, d2, dst, src, W2x, b2x, W2m, b2m, w3, b3, model=False, s1x=None, s1m=None):
    """What egcl_forward_save keeps (include/egnn_amd.h, egcl_forward_save): s1 = -log2(e) SiLU(a1), t2 = -log2(e) (W2 SiLU(a1) + b2)
    for both MLPs and s_e = w3 . SiLU(a2x + b2x) + b3.  s1x / s1m given: start from those stored activations instead.
    model: s1 rounded to bf16 (the MFMA operand, kernels.h:256); W2 times -ln 2 rounded to bf16 (pack.hip: egnn_pack_layer);
    fp32 accumulation; t2 = fma(acc, -log2 e, b2 * -log2 e) (edge_x_m16.hip:324, bias scaled in pack.hip: egnn_pack_layer) stored
    as bf16 (edge_x_m16.hip:342); s_e from the UNROUNDED t2 with w3 * -ln 2 in fp32 (edge_x_m16.hip:379-385, pack.hip: egnn_pack_layer)."""
    out = NS()
    for name, tab, W2, b2, s1 in (("x", tab_x, W2x, b2x, s1x), ("m", tab_m, W2m, b2m, s1m)):
        W2, b2 = d(W2), d(b2)
        if s1 is None:
            a1 = first_pre(tab, d2, dst, src, model)
            if model:
                s1 = bf16(a1 / (1.0 + torch.exp2(a1)))                     # silu_s, kernels.h:16
            else:
                s1 = -LOG2E * act(a1)[0]
        else:
            s1 = d(s1)
        if model:
            W2s, b2s = bf16(W2 * K_NEG_LN2), f32(b2 * K_NEG_LOG2E)
            acc = s1 @ W2s.t()
            t2u = f32(acc * K_NEG_LOG2E + b2s)
            abs_t2 = (s1.abs() @ W2s.abs().t()) * LOG2E + b2s.abs()
            t2 = bf16(t2u)
        else:
            t2u = t2 = -LOG2E * ((s1 / -LOG2E) @ W2.t() + b2)
            abs_t2 = LOG2E * ((s1.abs() / LOG2E) @ W2.abs().t() + b2.abs())
        setattr(out, "s1" + name, s1)
        setattr(out, "t2" + name, t2)
        setattr(out, "t2" + name + "_unrounded", t2u)
        setattr(out, "abs_t2" + name, abs_t2)
    w3, b3 = d(w3).reshape(-1), d(b3).reshape(())
    if model:
        t = out.t2x_unrounded
        terms = f32(w3 * K_NEG_LN2) * (t / (1.0 + torch.exp2(t)))
    else:
        terms = w3 * act(out.t2x / -LOG2E)[0]
    out.s_e = terms.sum(1) + b3
    out.abs_s_e = terms.abs().sum(1) + b3.abs()
    return out


def heads(t2x, t2m, diff, dst, g_sum_x, g_sum_m, s_e, w3, wa, ba, scaled=False, model=False):
    """egcl_backward_heads / egcl_backward_heads_saved / the epilogue of egcl_backward_edge_recompute
    (edge_bwd_heads.hip:9-12): t2 = second-layer pre-activations INCLUDING the bias (scaled: times -log2 e, as kept).
    Returns dL/da2x, dL/da2m, g_diff and the six sums g_b2x, g_w3, g_b3, g_b2m, g_wa, g_ba.
    model (heads_saved): w3 and wa arrive times -ln 2 and are multiplied back by -log2 e in fp32 (edge_bwd_heads.hip:66,114 on
    pack.hip: egnn_pack_layer); dL/da2 stored as bf16 (edge_bwd_heads.hip:80,156) while the column sums take the unrounded
    values (edge_bwd_heads.hip:78,154)."""
    t2x, t2m, diff, s_e = d(t2x), d(t2m), d(diff), d(s_e)
    gx, gm = d(g_sum_x)[dst], d(g_sum_m)[dst]
    w3, wa, ba = d(w3).reshape(-1), d(wa).reshape(-1), d(ba).reshape(())
    if model and scaled:
        w3, wa = f32(f32(w3 * K_NEG_LN2) * K_NEG_LOG2E), f32(f32(wa * K_NEG_LN2) * K_NEG_LOG2E)
    o = NS()
    gsc_t = gx * diff
    gsc = gsc_t.sum(1)
    sx, dsx, _ = act(t2x, scaled)
    g_a2x = gsc[:, None] * w3 * dsx
    o.g_b2x, o.abs_g_b2x = g_a2x.sum(0), g_a2x.abs().sum(0)
    o.g_w3, o.abs_g_w3 = (gsc[:, None] * sx).sum(0), (gsc[:, None] * sx).abs().sum(0)
    o.g_b3, o.abs_g_b3 = gsc.sum(), gsc_t.abs().sum()
    m, dsm, _ = act(t2m, scaled)
    z = m @ wa + ba
    gate = torch.sigmoid(z)
    dot = (gm * m).sum(1)
    coef = dot * gate * (1.0 - gate)
    g_a2m = (gm * gate[:, None] + coef[:, None] * wa) * dsm
    o.g_b2m, o.abs_g_b2m = g_a2m.sum(0), g_a2m.abs().sum(0)
    o.g_wa, o.abs_g_wa = (coef[:, None] * m).sum(0), (coef[:, None] * m).abs().sum(0)
    o.g_ba, o.abs_g_ba = coef.sum(), coef.abs().sum()
    o.g_diff = gx * s_e[:, None]
    o.gsc, o.abs_gsc = gsc, gsc_t.abs().sum(1)
    o.coef, o.gate = coef, gate
    o.abs_dot, o.abs_z = (gm * m).abs().sum(1), (m * wa).abs().sum(1) + ba.abs()
    o.dsx, o.dsm, o.m, o.sx, o.w3, o.wa, o.gm, o.gx = dsx, dsm, m, sx, w3, wa, gm, gx
    o.g_a2x_unrounded, o.g_a2m_unrounded = g_a2x, g_a2m
    o.g_a2x, o.g_a2m = (bf16(g_a2x), bf16(g_a2m)) if model else (g_a2x, g_a2m)
    return o


def dgrad(g_a2, W2, a1, scaled=False, model=False, form="chain"):
    """g1 = (g_a2 . W2) * SiLU'(a1) (egcl_backward_dgrad, egcl_backward_dgrad_reduce, or GEMM + egcl_backward_l1_grad).
    model: W2 rounded to bf16 (pack.hip: pack_frags_bf16_T), fp32 accumulation;
      form "chain" (edge_bwd_dgrad.hip): the product is rounded to bf16 BEFORE SiLU' (:90) and g1 after it (:116-117);
      form "graph" (edge_bwd_dgrad_graph.hip): g1 stays fp32 (:294-297); the node sums take bf16(g1) (:308) -- see first_reduce."""
    g_a2, W2 = d(g_a2), d(W2)
    if model:
        W2 = bf16(W2)
    dot = g_a2 @ W2
    abs_dot = g_a2.abs() @ W2.abs()
    _, ds, sg = act(a1, scaled)
    if model and form == "chain":
        dot = bf16(dot)
    g1 = dot * ds
    if model:
        g1 = bf16(g1) if form == "chain" else f32(g1)
    return NS(g1=g1, dot=dot, abs_dot=abs_dot, ds=ds, sg=sg)


def first_reduce(g1, d2, wd, dst, src, node_graph, N, B, model=False, form="reduce", wd_scaled=False):
    """Gd[n] = sum of g1 over the edges n receives, Gs[n] = over the edges n sends, cd[graph] = sum_e g1[e] d2_e,
    gd2[e] = g1[e] . wd (egcl_backward_first_reduce; the epilogue of egcl_backward_dgrad_reduce), ONE MLP.
    model, form "graph": the node sums add bf16(g1) in fp32 and are stored as bf16 (edge_bwd_dgrad_graph.hip:308,346-347); cd and
    gd2 take the fp32 g1; wd is the scaled column and gd2 is multiplied by -ln 2 (:299,330).  form "reduce": g1 is bf16 as
    handed in, everything fp32 (edge_bwd_first.hip:132-143)."""
    g1, d2, wd = d(g1), d(d2), d(wd)
    W = g1.shape[1]
    gsum = bf16(g1) if (model and form == "graph") else g1
    z = lambda r: torch.zeros(r, W, dtype=D)
    o = NS()
    o.Gd, o.Gs = z(N).index_add_(0, dst, gsum), z(N).index_add_(0, src, gsum)
    o.abs_Gd, o.abs_Gs = z(N).index_add_(0, dst, gsum.abs()), z(N).index_add_(0, src, gsum.abs())
    if model and form == "graph":
        o.Gd_unrounded, o.Gs_unrounded = o.Gd, o.Gs
        o.Gd, o.Gs = bf16(o.Gd), bf16(o.Gs)
    eg = node_graph[dst]
    o.cd = z(B).index_add_(0, eg, g1 * d2[:, None])
    o.abs_cd = z(B).index_add_(0, eg, (g1 * d2[:, None]).abs())
    o.gd2 = (g1 * wd).sum(1) * (K_NEG_LN2 if wd_scaled else 1.0)
    o.abs_gd2 = (g1 * wd).abs().sum(1) * (abs(K_NEG_LN2) if wd_scaled else 1.0)
    return o


def scatter_geom(gd2, g_diff, g_S, node_seg, diff, dst, src, g_x):
    """egcl_backward_scatter_geom / the geometry half of egcl_backward_scatter: dL/d(x_i - x_j) = g_diff + 2 (gd2 + g_S[segment
    of i]) (x_i - x_j), added to g_x[i], subtracted from g_x[j] (edge_bwd_first.hip:206-211).  gd2 = the sum of the shares."""
    gS = d(g_S)[node_seg[dst]] if node_seg is not None else d(g_S).reshape(-1)[0]
    tot = d(gd2) + gS
    gv = d(g_diff) + 2.0 * tot[:, None] * d(diff)
    out = d(g_x).clone().index_add_(0, dst, gv).index_add_(0, src, -gv)
    abs_out = d(g_x).abs().index_add_(0, dst, gv.abs()).index_add_(0, src, gv.abs())
    return NS(g_x=out, abs_g_x=abs_out, gv=gv)


def gather_in(h, d2, dst, src, K1P):
    """egcl_backward_gather_in: in[e] = [h_i | h_j | d2 | 1 | 0 ...] (backward.hip:271-289)"""
    h = d(h)
    H = h.shape[1]
    inp = torch.zeros(dst.numel(), K1P, dtype=D)
    inp[:, :H], inp[:, H:2 * H], inp[:, 2 * H], inp[:, 2 * H + 1] = h[dst], h[src], d(d2), 1.0
    return inp


def scatter(g_in, g_diff, g_S, node_seg, diff, dst, src, H, g_h, g_x):
    """egcl_backward_scatter: g_h[i] += g_in[:H], g_h[j] += g_in[H:2H] and the geometry half with gd2 = g_in[2H]
    (backward.hip:368-399)"""
    g_in = d(g_in)
    gh = d(g_h).clone().index_add_(0, dst, g_in[:, :H]).index_add_(0, src, g_in[:, H:2 * H])
    abs_gh = d(g_h).abs().index_add_(0, dst, g_in[:, :H].abs()).index_add_(0, src, g_in[:, H:2 * H].abs())
    sg = scatter_geom(g_in[:, 2 * H], g_diff, g_S, node_seg, diff, dst, src, g_x)
    return NS(g_h=gh, abs_g_h=abs_gh, g_x=sg.g_x, abs_g_x=sg.abs_g_x)


# ---- compositions of the exact stages: the edge part of one layer's backward (what autograd.py:_edge_backward adds) -----------
def edge_backward(params, H, h, x, dst, src, node_graph, node_seg, B, g_sum_m, g_sum_x, g_S, form):
    """dL/dh, dL/dx (edge part) and the twelve parameter gradients from the stage functions in exact mode.
    params: dict with the keys mlp_x.0 / mlp_x.2 / mlp_x.4 / mlp_m.0 / mlp_m.2 / attention.0 + .weight / .bias.
    form "chain": gather -> wgrad GEMMs over the edges -> scatter (autograd.py:_first_own / _first_library);
    form "factorised": first_reduce + node-level products (autograd.py:_finish_graph / _finish_reduce)."""
    p = {k: d(v) for k, v in params.items()}
    h, N = d(h), h.shape[0]
    diff, d2 = geometry(x, dst, src)
    tx = tables(h, p["mlp_x.0.weight"], p["mlp_x.0.bias"], H)
    tm = tables(h, p["mlp_m.0.weight"], p["mlp_m.0.bias"], H)
    kept = forward_kept(tx, tm, d2, dst, src, p["mlp_x.2.weight"], p["mlp_x.2.bias"], p["mlp_m.2.weight"], p["mlp_m.2.bias"],
                        p["mlp_x.4.weight"], p["mlp_x.4.bias"])
    hd = heads(kept.t2x / -LOG2E, kept.t2m / -LOG2E, diff, dst, g_sum_x, g_sum_m, kept.s_e, p["mlp_x.4.weight"],
               p["attention.0.weight"], p["attention.0.bias"])
    g = {"mlp_x.2.bias": hd.g_b2x, "mlp_x.4.weight": hd.g_w3.reshape(1, -1), "mlp_x.4.bias": hd.g_b3.reshape(1),
         "mlp_m.2.bias": hd.g_b2m, "attention.0.weight": hd.g_wa.reshape(1, -1), "attention.0.bias": hd.g_ba.reshape(1)}
    g["mlp_x.2.weight"] = hd.g_a2x.t() @ (kept.s1x / -LOG2E)
    g["mlp_m.2.weight"] = hd.g_a2m.t() @ (kept.s1m / -LOG2E)
    g1x = dgrad(hd.g_a2x, p["mlp_x.2.weight"], first_pre(tx, d2, dst, src)).g1
    g1m = dgrad(hd.g_a2m, p["mlp_m.2.weight"], first_pre(tm, d2, dst, src)).g1
    g_h, g_x = torch.zeros(N, H, dtype=D), torch.zeros(N, 3, dtype=D)
    if form == "chain":
        K1P = 2 * H + 2
        inp = gather_in(h, d2, dst, src, K1P)
        g_in = torch.zeros(dst.numel(), K1P, dtype=D)
        for name, g1 in (("mlp_x.0", g1x), ("mlp_m.0", g1m)):
            gw = g1.t() @ inp
            g[name + ".weight"], g[name + ".bias"] = gw[:, :2 * H + 1], gw[:, 2 * H + 1]
            g_in[:, :2 * H + 1] += g1 @ p[name + ".weight"]
        sc = scatter(g_in, hd.g_diff, g_S, node_seg, diff, dst, src, H, g_h, g_x)
        g_h, g_x = sc.g_h, sc.g_x
    else:
        gd2 = torch.zeros(dst.numel(), dtype=D)
        for name, g1, tab in (("mlp_x.0", g1x, tx), ("mlp_m.0", g1m, tm)):
            fr = first_reduce(g1, d2, tab.wd, dst, src, node_graph, N, B)
            w1 = p[name + ".weight"]
            g[name + ".weight"] = torch.cat((fr.Gd.t() @ h, fr.Gs.t() @ h, fr.cd.sum(0)[:, None]), 1)
            g[name + ".bias"] = fr.Gd.sum(0)
            g_h = g_h + fr.Gd @ w1[:, :H] + fr.Gs @ w1[:, H:2 * H]
            gd2 = gd2 + fr.gd2
        g_x = scatter_geom(gd2, hd.g_diff, g_S, node_seg, diff, dst, src, g_x).g_x
    return g_h, g_x, g


# ---- bars ---------------------------------------------------------------------------------------------------------------
def acc_bound(K, abs_terms):
    """textbook bound of an fp32 accumulation of K terms: K 2^-24 sum|terms| (Higham, Accuracy and Stability, (3.5) to first order)"""
    return K * EPS32 * abs_terms


def worst_ratio(got, want, bound):
    """max over the elements of |got - want| / bound (0 / 0 counts as 0; anything over a zero bound as inf)"""
    err = (d(got) - d(want)).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def row_rel(got, want):
    """norm-wise error per row, relative to the largest row norm of `want` (rows of zeros must not divide by zero)"""
    got, want = d(got), d(want)
    if want.dim() < 2:
        return (got - want).norm() / want.norm().clamp_min(1e-300)
    return (got - want).norm(dim=1) / want.norm(dim=1).clamp_min(1e-6 * float(want.norm(dim=1).max()) + 1e-300)

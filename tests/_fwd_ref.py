"""float64 restatement of ONE EGCL layer's FORWARD, stage by stage (test infrastructure, no HIP), next to tests/_bwd_ref.py whose
geometry / tables / first_pre / act / forward_kept it builds on.  Two stages, cut where the C ABI cuts the layer
(include/egnn_amd.h: egcl_forward_begin / egcl_read_aggregates / egcl_forward_end):

    edge_pass    per edge e = (i <- j):  a1 = P[i] + Q[j] + wd d2,  a2 = W2 SiLU(a1) + b2  for both edge MLPs,
                 s_e = w3 . SiLU(a2x) + b3,  out_e = SiLU(a2m) sigmoid(wa . SiLU(a2m) + ba);
                 sum_m[i] = sum_e out_e,  sum_x[i] = sum_e (x_i - x_j) s_e  (BEFORE the 1/(G+1) factor),  sq = sum_e |x_i - x_j|^2
                 per graph or per call (EquivariantGraphNeuralNetwork.py:55-65)
    node_update  h' = mlp_h([h | sum_m]) (no residual, quirk Q2),  x' = x + sum_x / (sqrt(sq) + 1)   (:64, :69, :70)

Each has an exact mode and a rounding-model mode (model=True) that applies ONLY the roundings the kernels document, per precision
(edge_pass) or per node-kernel form (node_update); every one is cited where it is applied.  Values the kernels keep scaled by
-log2(e) (kernels.h:15-18) are kept in that scale exactly where the kernels keep them.  Every sum comes with the sum of |terms| it
was formed from, for the bound K 2^-24 sum|terms| of an fp32 accumulation (_bwd_ref.acc_bound).

The irregular CSR batches the forward stage tests run on are built here too (irregular_batch) together with the conditions on
row_ptr they must satisfy (csr_features / assert_features): the tests assert them before anything is launched.
"""
import torch

from tests import _bwd_ref as R
from tests._bwd_ref import D, NS, K_NEG_LN2, K_NEG_LOG2E, LOG2E, act, bf16, d, f32, first_pre, forward_kept, fp16, geometry, tables  # noqa: F401

E24 = R.EPS32
OPS = 8.0                 # fp32 operations of an element-wise chain (v_exp_f32 and v_rcp_f32 are 1-ulp instructions), as the backward tests
F16_MAX = 65504.0
F16_WSCALE = 256.0        # kF16WScale, kernels.h:218: every fp16 weight stream is packed times 2^8
SPLIT_K = 320             # kSplitK, node_bf16.hip:21 (node_post_split_k()): K of the split-operand node MLP
PRECISIONS = ("fp32", "bf16", "fp16", "bf16x3", "f16c8")
MODELS = PRECISIONS + ("bf16g",)   # + the generic edge kernel in bf16


# ---- irregular graphs ---------------------------------------------------------------------------------------------------------
def graph_in_degrees(R_, seed=0):
    """in-degrees of the five graphs of the irregular batch for tile height R_ (32 / 64 / 128 edges)"""
    n2 = {32: 20, 64: 40, 128: 70}[R_]
    n4 = {32: 24, 64: 48, 128: 60}[R_]
    g = torch.Generator().manual_seed(seed)
    small = [1, 2, 3, 5, 1, 1, 2, 7, 4, 1, 1, 3, 2, 6, 1, 2]
    g0 = [0, 2 * R_ + R_ // 2 + 3] + small + small
    g0.append((-sum(g0)) % R_)                         # pads the edge count up to a multiple of R: the next node starts a tile
    g0 += [R_, 0, 2 * R_, R_ + 1, 0, 0, R_ - 1]
    g0 += [9] * 12
    g0 += [0] * (max(66, 2 * R_ + R_ // 2 + 4) - len(g0))
    g4 = torch.randint(0, n4, (n4,), generator=g).tolist()
    g4[-1] = 0
    return [g0, [0], [n2 - 1] * n2, [0, 0, 0], g4], g


def irregular_batch(R_, seed=0):
    """CSR batch of five graphs built directly from in-degrees; the sources of a node are drawn uniformly inside its graph
    (duplicate edges and self loops occur).  -> NS(sizes, N, E, B, row_ptr, dst, src, graph_ptr, node_graph), int64 CPU tensors"""
    degs, g = graph_in_degrees(R_, seed)
    sizes = [len(x) for x in degs]
    deg = torch.tensor([v for x in degs for v in x])
    gp = torch.tensor([0] + torch.cumsum(torch.tensor(sizes), 0).tolist())
    node_graph = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    row_ptr = torch.zeros(deg.numel() + 1, dtype=torch.long)
    row_ptr[1:] = torch.cumsum(deg, 0)
    dst = torch.repeat_interleave(torch.arange(deg.numel()), deg)
    lo, n = gp[node_graph[dst]], torch.tensor(sizes)[node_graph[dst]]
    src = lo + (torch.rand(dst.numel(), generator=g, dtype=D) * n).long().clamp_max(n - 1)
    return NS(sizes=sizes, N=int(deg.numel()), E=int(dst.numel()), B=len(sizes), row_ptr=row_ptr, dst=dst, src=src, graph_ptr=gp,
              node_graph=node_graph, R=R_)


def fully_connected_batch(sizes):
    """the same record for fully connected graphs (i-major, the order of graph.fully_connected_edge_index)"""
    rows, cols, off = [], [], 0
    for n in sizes:
        i, j = torch.arange(n).repeat_interleave(n), torch.arange(n).repeat(n)
        keep = i != j
        rows.append(i[keep] + off)
        cols.append(j[keep] + off)
        off += n
    dst, src = torch.cat(rows), torch.cat(cols)
    N = sum(sizes)
    row_ptr = torch.zeros(N + 1, dtype=torch.long)
    row_ptr[1:] = torch.cumsum(torch.bincount(dst, minlength=N), 0)
    gp = torch.tensor([0] + torch.cumsum(torch.tensor(sizes), 0).tolist())
    return NS(sizes=list(sizes), N=N, E=int(dst.numel()), B=len(sizes), row_ptr=row_ptr, dst=dst, src=src, graph_ptr=gp,
              node_graph=torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)), R=None)


def csr_features(b, R_):
    """what the CSR of batch b offers a kernel that works on tiles of R_ edges (everything from row_ptr / the edge list)"""
    rp = b.row_ptr
    deg = rp[1:] - rp[:-1]
    has = deg > 0
    t0, t1 = rp[:-1] // R_, (rp[1:] - 1).clamp_min(0) // R_
    aligned = (rp[:-1] % R_) == 0
    ntiles = (b.E + R_ - 1) // R_
    tile_of = torch.arange(b.E) // R_
    starts = torch.ones(b.E, dtype=torch.bool)
    starts[1:] = (b.dst[1:] != b.dst[:-1]) | (tile_of[1:] != tile_of[:-1])
    segs = torch.bincount(tile_of[starts], minlength=ntiles)
    key = b.dst * b.N + b.src
    gdeg = torch.zeros(b.B, dtype=torch.long).index_add_(0, b.node_graph, deg)
    gsz = torch.tensor(b.sizes)
    iso = ~has
    f = dict(
        spans_three_tiles=bool((has & (t1 >= t0 + 2)).any()),
        fills_one_tile=bool((aligned & (deg == R_)).any()),
        fills_two_tiles=bool((aligned & (deg == 2 * R_)).any()),
        straddles_two_tiles=bool((has & (t1 == t0 + 1) & ~(aligned & (deg == 2 * R_))).any()),
        tile_over_8_segments=bool((segs > 8).any()), tile_2_to_8_segments=bool(((segs >= 2) & (segs <= 8)).any()),
        tile_one_segment=bool((segs == 1).any()), max_segments=int(segs.max()),
        first_isolated=bool(iso[0]), last_isolated=bool(iso[-1]), interior_isolated=bool(iso[1:-1].any()),
        partial_last_tile=b.E % R_ != 0,
        self_loop=bool((b.dst == b.src).any()), duplicate_edge=bool(torch.unique(key).numel() < b.E),
        edgeless_single=bool(((gsz == 1) & (gdeg == 0)).any()), edgeless_several=bool(((gsz > 1) & (gdeg == 0)).any()),
        graph_over_64=bool(((gsz > 64) & (gdeg > 0)).any()), graph_upto_64=bool(((gsz <= 64) & (gdeg > 0)).any()),
        sorted_by_receiver=bool((b.dst[1:] >= b.dst[:-1]).all()),
        edges_stay_in_graph=bool((b.node_graph[b.dst] == b.node_graph[b.src]).all()))
    return f


def assert_features(b, R_):
    f = csr_features(b, R_)
    missing = [k for k, v in f.items() if k != "max_segments" and not v]
    assert not missing, (R_, "the irregular batch lost", missing)
    return f


# ---- operand roundings ----------------------------------------------------------------------------------------------------------
def fp16s(t):
    """fp16 as the kernels produce it: from the fp32 value, nearest even, saturating (MODE.FP16_OVFL, kernels.h:216-224; the packs
    clamp explicitly, pack.hip: to_operand)"""
    return fp16(t.clamp(-F16_MAX, F16_MAX))


def split(t, rnd):
    """head + remainder of a split operand: hi = rnd(v), lo = rnd(v - hi) (edge_bf16x3.hip:35-38, node_bf16.hip:162-168,
    pack.hip: to_operand, pack_frags_bf16_lo)"""
    t = f32(t)
    hi = rnd(t)
    return hi, rnd(t - hi)


def q_e4m3(t, s):
    """tools/rounding_budget.py's emulation of v_cvt_scalef32_pk_fp8_f32 (t 2^s to OCP e4m3, nearest even, saturating at 448)"""
    from tools.rounding_budget import q_e4m3 as q
    return q(t.to(torch.float32), s).to(D)


def c8_shift(v):
    """scale exponent of a weight matrix's e4m3 heads: 2^s_hi max|v| in [112, 224] (edge_f16c8w.hip:626-631, c8_shift); the
    remainders take s_hi + 11 (:643-644)"""
    import math
    mx = min(float(v.abs().max()), F16_MAX)
    s = math.floor(math.log2(224.0 / mx)) if mx > 0 else 0
    return max(-40, min(40, s))


def second_layer(s1, W2, b2, prec, model):
    """a2 = W2 s1 + b2 of one edge MLP.  Exact: s1 = SiLU(a1), natural units.  model (every tiled path): s1 = silu_s(a1 scaled) =
    -log2(e) SiLU(a1) unrounded; the weights are W2 * -ln 2 [* 2^8] rounded to fp32 and then to the operand type
    (pack.hip: egnn_pack_layer, to_operand); fp32 accumulation; t2 = fma(acc, -log2(e) [/ 2^8], b2 * -log2(e))
    (edge_tile.h:188,228; edge_x_m16.hip:372; edge_small.hip:46) -- returned scaled and UNROUNDED (inference stores no t2).
      bf16    s1 and W2 rounded to bf16 (kernels.h:256)
      fp16    s1 and W2 2^8 rounded to fp16, saturating
      bf16x3  both split into bf16 head + bf16 remainder; lo.hi + hi.lo + hi.hi, lo.lo dropped (edge_bf16x3.hip:7)
      f16c8   fp16 heads; a_lo 2^12 and a 2 to e4m3 (edge_f16c8w.hip:88-99), W_hi 2^s and W_lo 2^(s+11) to e4m3 (:632-663);
              a_hi.W_hi + a_lo8.W_hi8 + a_hi8.W_lo8 (:7-8)
    -> NS(t2, abs_t2, Wabs = |effective weight operand| [W, K], scale = d t2 / d acc, op = per-element spacing of the activation
    operand's rounding as it reaches the product)"""
    W2, b2 = d(W2), d(b2)
    if not model:
        return NS(t2=s1 @ W2.t() + b2, abs_t2=s1.abs() @ W2.abs().t() + b2.abs(), Wabs=W2.abs(), scale=1.0, op=torch.zeros_like(s1))
    if prec == "bf16g":   # generic edge_kernel<BF16>: natural units, s1 and W2 rounded to bf16 (egnn_forward.hip: gemm_bf16, pack.hip: egnn_pack_layer)
        A, Wo = bf16(s1), bf16(W2)
        return NS(t2=A @ Wo.t() + b2, abs_t2=A.abs() @ Wo.abs().t() + b2.abs(), Wabs=Wo.abs(), scale=1.0, op=R.ulp_bf16(f32(s1)))
    b2s = f32(b2 * K_NEG_LOG2E)
    a = f32(s1)
    if prec == "bf16":
        A, Wo, scale = bf16(a), bf16(f32(W2 * K_NEG_LN2)), K_NEG_LOG2E
        acc, Wabs, op = A @ Wo.t(), Wo.abs(), R.ulp_bf16(a)
    elif prec == "fp16":
        A, Wo, scale = fp16s(a), fp16s(f32(W2 * (K_NEG_LN2 * F16_WSCALE))), K_NEG_LOG2E / F16_WSCALE
        acc, Wabs, op = A @ Wo.t(), Wo.abs(), R.ulp_fp16(a)
    elif prec == "bf16x3":
        (Ah, Al), (Wh, Wl), scale = split(a, bf16), split(f32(W2 * K_NEG_LN2), bf16), K_NEG_LOG2E
        acc = Al @ Wh.t() + Ah @ Wl.t() + Ah @ Wh.t()
        # a head that flips by ulp_bf16(a) <= 2^-7 |a| is made up by the remainder except in the dropped lo.lo product
        # (|W_lo| <= 2^-9 |W|); a remainder flips by ulp_bf16(a_lo) <= 2^-7 2^-9 |a|: together 2^-15 |a| per unit of |W|
        Wabs, op = Wh.abs() + Wl.abs(), 2.0 ** -15 * a.abs()
    elif prec == "f16c8":
        v = f32(W2 * (K_NEG_LN2 * F16_WSCALE)).clamp(-F16_MAX, F16_MAX)
        Wh = fp16(v)
        Wl = v - Wh
        sh = c8_shift(v)
        Wh8, Wl8 = q_e4m3(Wh, sh), q_e4m3(Wl, sh + 11)
        Ah = fp16s(a)
        Al8, Ah8 = q_e4m3(a - Ah, 12), q_e4m3(a, 1)
        scale = K_NEG_LOG2E / F16_WSCALE
        acc = Ah @ Wh.t() + Al8 @ Wh8.t() + Ah8 @ Wl8.t()
        # e4m3 has 4 significant bits (spacing <= 2^-3 |v|, 2^-9 / scale below its normal range): a_lo8 flips by 2^-3 2^-11 |a| (or
        # 2^-21), a_hi8 by 2^-3 |a| (or 2^-10) against |W_lo| <= 2^-11 |W|, and a head flip of 2^-10 |a| is made up except for
        # W_hi8 - W_hi <= 2^-4 |W|: three terms of 2^-14 |a| (1 + 2^-4) <= 2^-12 |a|, floor 2^-20
        Wabs, op = Wh.abs() + Wl.abs(), 2.0 ** -12 * a.abs() + 2.0 ** -20
    else:
        raise ValueError(prec)
    t2 = acc * scale + b2s
    return NS(t2=t2, abs_t2=(a.abs() @ Wabs.t()) * abs(scale) + b2s.abs(), Wabs=Wabs, scale=abs(scale), op=op)


def table(h, W1, b1, H, kind):
    """first-layer table of one edge MLP.  kind "exact"; "f16s" = the half-precision paths' table (_bwd_ref.tables(model=True):
    scaled, fp16); "f32s" = the fp32 table of bf16x3 / f16c8 on the scaled weights (egnn_forward.hip: plan_edge, set_edge_streams;
    pack.hip: egnn_pack_layer, scale_copy; node_pre_mfma_kernel<float>: exact fp32 MFMA, no rounding modelled)"""
    if kind in ("exact", "f16s"):
        t = tables(h, W1, b1, H, kind == "f16s")
        t.half = kind == "f16s"
        return t
    h, W1, b1 = d(h), f32(d(W1) * K_NEG_LOG2E), f32(d(b1) * K_NEG_LOG2E)
    return NS(P=h @ W1[:, :H].t() + b1, Q=h @ W1[:, H:2 * H].t(), wd=W1[:, 2 * H].clone(),
              abs_P=h.abs() @ W1[:, :H].abs().t() + b1.abs(), abs_Q=h.abs() @ W1[:, H:2 * H].abs().t(), scaled=True, half=False)


TABLE_KIND = {"fp32": "exact", "bf16g": "exact", "bf16": "f16s", "fp16": "f16s", "bf16x3": "f32s", "f16c8": "f32s"}


def silu_s(t):
    """kernels.h:16: -log2(e) SiLU(z) on t = -log2(e) z"""
    return t / (1.0 + torch.exp2(t))


def edge_pass(p, H, h, x, dst, src, node_graph, N, B, scope, prec="fp32", model=False):
    """One edge pass.  p: the layer's parameters (keys mlp_x.0.weight ... attention.0.bias).  prec "fp32" with model=True is the
    generic fp32 kernel: no operand rounding, natural units (egnn_forward.hip: edge_kernel); "bf16g" is the generic kernel in bf16 (message
    widths above 256, which no tiled kernel takes: fp32 table, bf16 operands); every other precision is its tiled path.
    -> NS(sum_m [N, M], sum_x [N, 3], sq [B] or [1], abs_sum_m, abs_sum_x, e = per-edge intermediates for the bounds)"""
    scaled = model and prec not in ("fp32", "bf16g")
    diff, d2 = geometry(x, dst, src, model)
    e = NS(diff=diff, d2=d2, scaled=scaled, prec=prec)
    for nm in ("x", "m"):
        tab = table(h, p[f"mlp_{nm}.0.weight"], p[f"mlp_{nm}.0.bias"], H, TABLE_KIND[prec] if model else "exact")
        pq = tab.P[dst] + tab.Q[src]
        if tab.half:
            pq = fp16(pq)                                 # packed-half add, kernels.h:251
        wd2 = tab.wd * d2[:, None]
        a1 = pq + wd2
        s1 = silu_s(a1) if scaled else act(a1)[0]
        sl = second_layer(s1, p[f"mlp_{nm}.2.weight"], p[f"mlp_{nm}.2.bias"], prec, scaled or (model and prec == "bf16g"))
        setattr(e, nm, NS(tab=tab, pq=pq, wd2=wd2, a1=a1, s1=s1, sl=sl, K=a1.shape[1]))
    w3, b3 = d(p["mlp_x.4.weight"]).reshape(-1), d(p["mlp_x.4.bias"]).reshape(())
    wa, ba = d(p["attention.0.weight"]).reshape(-1), d(p["attention.0.bias"]).reshape(())
    if scaled:   # heads on the scaled values: w3 and wa arrive times -ln 2 (pack.hip: egnn_pack_layer), edge_tile.h:171-243
        e.w3, e.wa = f32(w3 * K_NEG_LN2), f32(wa * K_NEG_LN2)
        e.sx, e.ms = silu_s(e.x.sl.t2), silu_s(e.m.sl.t2)
        e.c = K_NEG_LN2                                   # edge_tile.h:242: the gate also undoes the scale of mval
    else:
        e.w3, e.wa = w3, wa
        e.sx, e.ms = act(e.x.sl.t2)[0], act(e.m.sl.t2)[0]
        e.c = 1.0
    e.s_e = (e.sx * e.w3).sum(1) + b3
    e.abs_s_e = (e.sx * e.w3).abs().sum(1) + b3.abs()
    e.z = (e.ms * e.wa).sum(1) + ba
    e.abs_z = (e.ms * e.wa).abs().sum(1) + ba.abs()
    e.gate = torch.sigmoid(e.z)
    e.val = e.gate * e.c
    e.out = e.ms * e.val[:, None]
    e.xm = diff * e.s_e[:, None]
    M = e.out.shape[1]
    z = lambda w: torch.zeros(N, w, dtype=D)
    o = NS(e=e)
    o.sum_m, o.abs_sum_m = z(M).index_add_(0, dst, e.out), z(M).index_add_(0, dst, e.out.abs())
    o.sum_x, o.abs_sum_x = z(3).index_add_(0, dst, e.xm), z(3).index_add_(0, dst, e.xm.abs())
    dd = (diff * diff).sum(1)                             # plain squares (edge_tile.h:137,157; node_d2_kernel), not norm()**2
    o.sq = torch.zeros(B, dtype=D).index_add_(0, node_graph[dst], dd) if scope == "graph" else dd.sum().reshape(1)
    return o


def edge_bounds(o, H, dst, src, N, deg, nsplit):
    """[2, ...] uncertainties of sum_m, sum_x of a MODEL-mode edge_pass o: index 0 = `acc` (fp32 arithmetic only), 1 = acc + `prop`
    (documented re-roundings of values the test cannot read back, each of which may flip by one spacing between device and model).
      a1     fp16 table: one fp16 ulp per entry and for their fp16 sum + the table product's own error (2^-15 for the split-operand
             kernel H <= 48, egnn_forward.hip: node_pre_hilo_kernel; (H + 2) 2^-24 else) -- prop, as tests/test_gpu_bwd_stages.py;
             fp32 table: (H + 2) 2^-24 sum|terms| -- acc.  The fma and d2 = sqrtf(.)^2: 2^-24 (|P + Q| + 7 |wd d2|)
      s1     |SiLU'| <= 1.1, OPS operations (+ |a1| for __expf(-v) = exp2(-v log2 e), whose argument is rounded: generic kernel)
             + the operand rounding's spacing (second_layer.op) -- prop
      t2     (K + 2) 2^-24 sum|terms| + the s1 uncertainties through |W|
      heads  the same chain rule through SiLU, w3 / wa, the sigmoid (|sigma'| <= 1/4); sums: (deg + nsplit + 8) 2^-24 sum|terms|"""
    e = o.e
    st = lambda acc, prop: torch.stack((acc, acc + prop))
    zero = torch.zeros((), dtype=D)
    exp_arg = (lambda v: OPS + v.abs()) if not e.scaled else (lambda v: OPS)
    u = NS()
    for nm in ("x", "m"):
        b = getattr(e, nm)
        tab = b.tab
        if tab.half:
            pert = 2.0 ** -15 if H <= 48 else (H + 2) * E24
            dP, dQ = R.ulp_fp16(tab.P) + pert * tab.abs_P, R.ulp_fp16(tab.Q) + pert * tab.abs_Q
            da1 = st(E24 * (b.pq.abs() + 7.0 * b.wd2.abs()), dP[dst] + dQ[src] + R.ulp_fp16(b.pq))
        else:
            dt = (H + 2) * E24 * (tab.abs_P[dst] + tab.abs_Q[src])
            da1 = st(dt + E24 * (b.pq.abs() + 7.0 * b.wd2.abs()), zero)
        ds1 = 1.1 * da1 + exp_arg(b.a1) * E24 * b.s1.abs()
        ds1[1] += b.sl.op
        dt2 = (ds1 @ b.sl.Wabs.t()) * b.sl.scale + (b.K + 2) * E24 * b.sl.abs_t2
        setattr(u, "t2" + nm, dt2)
    dsx = 1.1 * u.t2x + exp_arg(e.x.sl.t2) * E24 * e.sx.abs()
    u.s_e = (dsx * e.w3.abs()).sum(2) + (e.w3.numel() + 10) * E24 * e.abs_s_e
    K = (deg + nsplit + 8.0)[:, None]
    zx, zm = torch.zeros(2, N, 3, dtype=D), torch.zeros(2, N, e.out.shape[1], dtype=D)
    u.sum_x = zx.index_add_(1, dst, e.diff.abs() * u.s_e[:, :, None] + E24 * e.xm.abs()) + K * E24 * o.abs_sum_x
    dms = 1.1 * u.t2m + exp_arg(e.m.sl.t2) * E24 * e.ms.abs()
    dz = (dms * e.wa.abs()).sum(2) + (e.wa.numel() + 8) * E24 * e.abs_z
    dval = abs(e.c) * (0.25 * dz + 4 * E24 * e.gate) + E24 * e.val.abs()
    dout = dms * e.val.abs()[:, None] + e.ms.abs() * dval[:, :, None] + E24 * e.out.abs()
    u.sum_m = zm.index_add_(1, dst, dout) + K * E24 * o.abs_sum_m
    return u


# ---- node update ------------------------------------------------------------------------------------------------------------------
def node_update(p, H, h, x, sum_m, sum_x, sq, node_graph, scope, form="fp32", model=False):
    """h' = mlp_h([h | sum_m]) and x' = x + sum_x / (sqrt(sq) + 1) from GIVEN aggregates.  model, per node-kernel form:
      bf16   [h | sum_m], both weight matrices and the hidden activation rounded to bf16 (node_bf16.hip:162,197,354;
             pack.hip: egnn_pack_layer), fp32 accumulation
      split  every operand a fp16 head + fp16 remainder, weights times 2^8, lo.hi + hi.lo + hi.hi (node_bf16.hip:35-41,320-322,
             364-367), accumulators divided by 2^8 where the biases are added (:353,:388); K padded to SPLIT_K with zeros
      fp32   exact (node_post_kernel: v_mfma_f32_32x32x2f32)
    -> NS(h_out, x_out, pre, hid, abs_pre, abs_out, W2abs, op = spacing of the hidden operand's rounding, g = 1 / (sqrt(sq) + 1))"""
    X = torch.cat((d(h), d(sum_m)), 1)
    W1, b1 = d(p["mlp_h.0.weight"]), d(p["mlp_h.0.bias"])
    W2, b2 = d(p["mlp_h.2.weight"]), d(p["mlp_h.2.bias"])
    o = NS()
    if not model or form == "fp32":
        o.pre, o.abs_pre = X @ W1.t() + b1, X.abs() @ W1.abs().t() + b1.abs()
        o.hid = act(o.pre)[0]
        o.h_out, o.abs_out = o.hid @ W2.t() + b2, o.hid.abs() @ W2.abs().t() + b2.abs()
        o.W2abs, o.op = W2.abs(), torch.zeros_like(o.hid)
    elif form == "bf16":
        Xo, W1o, W2o = bf16(X), bf16(W1), bf16(W2)
        o.pre, o.abs_pre = Xo @ W1o.t() + b1, Xo.abs() @ W1o.abs().t() + b1.abs()
        o.hid = act(o.pre)[0]
        ho = bf16(o.hid)
        o.h_out, o.abs_out = ho @ W2o.t() + b2, ho.abs() @ W2o.abs().t() + b2.abs()
        o.W2abs, o.op = W2o.abs(), R.ulp_bf16(o.hid)
    elif form == "split":
        pad = SPLIT_K - X.shape[1]
        assert pad >= 0
        X, W1 = torch.nn.functional.pad(X, (0, pad)), torch.nn.functional.pad(W1, (0, pad))
        (Xh, Xl), (Wh, Wl) = split(X, fp16s), split(W1 * F16_WSCALE, fp16s)
        acc = Xh @ Wl.t() + Xl @ Wh.t() + Xh @ Wh.t()
        o.pre = acc / F16_WSCALE + b1
        o.abs_pre = (Xh.abs() + Xl.abs()) @ (Wh.abs() + Wl.abs()).t() / F16_WSCALE + b1.abs()
        o.hid = act(o.pre)[0]
        (hh, hl), (Vh, Vl) = split(o.hid, fp16s), split(W2 * F16_WSCALE, fp16s)
        acc2 = hh @ Vl.t() + hl @ Vh.t() + hh @ Vh.t()
        o.h_out = acc2 / F16_WSCALE + b2
        o.W2abs = (Vh.abs() + Vl.abs()) / F16_WSCALE
        o.abs_out = (hh.abs() + hl.abs()) @ o.W2abs.t() + b2.abs()
        # a head flip (2^-10 |v|) is made up by the remainder except in the dropped lo.lo product (|W_lo| <= 2^-11 |W|); the remainder
        # flips by 2^-10 2^-11 |v|, or by fp16's subnormal spacing 2^-24
        o.op = 2.0 ** -20 * o.hid.abs() + 2.0 ** -24
    else:
        raise ValueError(form)
    sq = d(sq)
    o.g = 1.0 / (torch.sqrt(sq) + 1.0)
    gn = o.g[node_graph][:, None] if scope == "graph" else o.g.reshape(1, 1)
    o.gn = gn
    o.x_out = d(x) + d(sum_x) * gn
    return o


def node_bounds(o, K1, Wh, hs, sum_x, abs_sum_x, ntiles, nsplit):
    """[2, ...] uncertainties (acc, acc + prop) of h_out and x_out of a MODEL-mode node_update o whose inputs are the device's own
    aggregates: the first product's fp32 accumulation through |SiLU'| <= 1.1, OPS + |v| operations of silu_f (__expf(-v) rounds
    v log2 e), the hidden operand's rounding (prop), the second product's accumulation over Wh terms + 4 waves + hs splits;
    x_out: node_post adds the column-split copies and tile partials of sum_x in another order than agg_export_kernel
    (node_bf16.hip:261-270 against backward.hip:441-449): (nsplit + tiles + 2) 2^-24 sum|terms|, and six fp32 operations"""
    dpre = (K1 + 2) * E24 * o.abs_pre
    dhid = 1.1 * dpre + (OPS + o.pre.abs()) * E24 * o.hid.abs()
    dhid = torch.stack((dhid, dhid + o.op))
    u = NS()
    u.h_out = dhid @ o.W2abs.t() + (Wh + 8 + hs) * E24 * o.abs_out
    v = d(sum_x) * o.gn
    ux = (nsplit + ntiles[:, None] + 2.0) * E24 * abs_sum_x * o.gn + 6 * E24 * v.abs() + E24 * o.x_out.abs()
    u.x_out = torch.stack((ux, ux))
    return u

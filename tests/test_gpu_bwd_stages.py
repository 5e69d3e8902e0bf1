"""Every stage of the bf16 edge backward ALONE against the float64 restatement of that stage (tests/_bwd_ref.py, proven against
float64 autograd by tests/test_bwd_ref_cpu.py): the test feeds a stage operands it controls (or reads back from the device, so that
the reference starts from the very same bf16 values), and compares ELEMENT-WISE.  Per output:

 0. the PLAIN bound, recorded, not asserted: ulp_bf16(want) (bf16 outputs) + K 2^-24 sum|terms| with K the reduction length of the
    element itself and sum|terms| from the restatement.  The worst |error| / plain bound is printed as "plain".  It is above 1
    where an element depends on values that the device rounds again and the test cannot read back (below); profiles/
    bwd_stage_errors.txt and DESIGN.md 5.1 name those outputs.
 1. asserted against the ROUNDING MODEL:   |got - want| <= ulp_bf16(want) + acc + prop   (fp32 outputs and sums: acc + prop)
      acc  = fp32 arithmetic only: K 2^-24 sum|terms| of every fp32 accumulation the element goes through (its own and those of the
             values it is computed from), and OPS 2^-24 |value| for the fp32 operations of an element-wise chain (OPS = 8: v_exp_f32
             and v_rcp_f32 are 1-ulp instructions, the rest are correctly rounded), propagated with |SiLU'| <= 1.1, |SiLU''| <= 0.5;
      prop = the documented RE-ROUNDINGS of an input, which may flip between device and model because the value that is rounded
             differs by `acc`-sized amounts: one fp16 ulp per table entry and for their fp16 sum plus the perturbation of the table's
             split-operand product (egnn_forward.hip: launch_node_pre_f16 "2^-16"), one ulp_bf16 of the dgrad product that edge_bwd_dgrad.hip:90
             rounds before SiLU', one ulp_bf16 of every g1 that edge_bwd_dgrad_graph.hip:308 rounds before the node sums.
    The worst |error| / bound is printed as "model"; FACTOR[stage] would multiply the bound (none is needed).
 2. asserted against the EXACT restatement: the norm-wise error (per row of an [edges, W] output, per tensor for sums) is at most
    2 x the rounding model's own error against exact on the same inputs + the norm of `acc` ALONE (the model does not round fp32
    accumulations; prop is NOT allowed here: an undocumented extra rounding shows even if someone modelled it).  Printed as "exact".
    Outputs without assertion 2: the aggregates / x_out of the small-tile comparison in test_table_and_forward_save (device against
    device: there is no model error to compare with).  For first_reduce and scatter_geom the model rounds nothing but the fp32
    coordinate difference, so assertion 2 there is assertion 1 taken norm-wise.
No element is excluded from any comparison."""
import functools
import math
import os

import pytest
import torch

import diffusion_model_amd as dma
from tests import _bwd_ref as R
from tests._util import dims_for

pytestmark = pytest.mark.gpu

SIZES = (64, 1, 33, 2, 17, 50)          # 7,812 edges fully connected: a 64-node graph, one without edges, a 2-edge graph
RADIUS = 1.6
WIDTHS = [(36, 256, 256), (36, 512, 256), (36, 1024, 1024)]
WIDTH_IDS = ["Wx256", "Wx512", "Wx1024"]
GRAPHS = ["fully_connected", "radius"]
M = 256
OPS = 8.0
E24 = R.EPS32
LN2 = math.log(2.0)
SENT = 7.0                                # sentinel for "must not be written" (exact in bf16 and fp32)
FACTOR = {}                               # stage -> factor on the derived bound (none needed: see profiles/bwd_stage_errors.txt)
D = torch.float64
bf = torch.bfloat16
_PROP = [1.0]                             # 1: bounds include `prop` (re-rounded inputs); 0: `acc` only (see the module docstring)


def _both(fn):
    """(fn() with prop, fn() with acc only)"""
    try:
        _PROP[0] = 1.0
        full = fn()
        _PROP[0] = 0.0
        return full, fn()
    finally:
        _PROP[0] = 1.0


def _ru(v, m):
    return (v + m - 1) // m * m


class _Report:
    def __init__(self, stage, case):
        self.stage, self.case, self.fail = stage, case, []

    def check(self, name, got, want, unc, bf16_out=False, exact=None, acc=None, plain=None):
        """assertion 1 (element-wise, rounding model, bound unc = acc + prop), with `exact` assertion 2 (norm-wise, 2 x the model's
        own error + acc), and the recorded ratio against the plain bound"""
        got = R.d(got.cpu() if got.is_cuda else got)
        want, unc = torch.as_tensor(want, dtype=D), torch.as_tensor(unc, dtype=D)
        acc = unc if acc is None else torch.as_tensor(acc, dtype=D)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert bool(torch.isfinite(got).all()), (self.stage, self.case, name, "non-finite")
        ulp = R.ulp_bf16(want) if bf16_out else 0.0
        r1 = R.worst_ratio(got, want, unc + ulp)
        r0 = float("nan") if plain is None else R.worst_ratio(got, want, torch.as_tensor(plain, dtype=D) + ulp)
        r2 = float("nan")
        if exact is not None:
            exact = R.d(exact)
            rows = got.dim() == 2 and got.shape[0] > 8
            nrm = (lambda t: t.norm(dim=1)) if rows else (lambda t: t.norm())
            mod = R.bf16(want) if bf16_out else want          # the model's own output: rounded as the stage stores it
            e_dev, e_mod, flo = nrm(got - exact), nrm(mod - exact), nrm(acc.expand_as(got))
            lim = 2.0 * e_mod + flo
            q = torch.where(e_dev == 0, torch.zeros_like(e_dev), e_dev / lim.clamp_min(1e-300))
            r2 = float(q.max())
        f = FACTOR.get(self.stage, 1.0)
        print(f"bwd-stage-ratio {self.stage:<14s} {self.case:<28s} {name:<10s} plain {r0:9.3f}  model {r1:8.3f}  exact {r2:8.3f}")
        if not r1 <= f:
            self.fail.append((name, "rounding model", r1))
        if exact is not None and not r2 <= 1.0:
            self.fail.append((name, "2 x model error against exact", r2))

    def same(self, name, got, want):
        if not torch.equal(got, want):
            self.fail.append((name, "not bitwise equal", int((got != want).sum())))

    def done(self):
        assert not self.fail, (self.stage, self.case, self.fail)


# ---- one layer, one graph batch, one width set: built once -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(H, Wx, Wm, graphs):
    from diffusion_model_amd import _lib
    from diffusion_model_amd.egnn import _context, _plan_for
    dev = torch.device("cuda")
    with torch.random.fork_rng(devices=[]):   # (the global generator stays as the next test expects it)
        torch.manual_seed(31)
        net = dma.EquivariantGNN(1, **dims_for(H, M, Wm, Wx, 256))
    with torch.no_grad():   # pre-activations on both sides of SiLU's knee
        net.egcl_list[0].mlp_x[2].weight *= 3.0
        net.egcl_list[0].mlp_m[2].weight *= 3.0
    n = sum(SIZES)
    g = torch.Generator().manual_seed(17)
    h, x = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g) * 1.5
    c = R.NS(H=H, Wx=Wx, Wm=Wm, N=n, B=len(SIZES), g=g, lib=_lib, L=_lib.lib(), dev=dev)
    c.id = f"H{H}-Wx{Wx}-Wm{Wm}-{graphs}"
    net.to(dev)
    net.precision, net.norm_scope = "bf16", "graph"
    c.net, c.layers = net, list(net.egcl_list)
    c.hd, c.xd = h.to(dev), x.to(dev)
    if graphs == "radius":
        plan = dma.radius_plan(c.xd, list(SIZES), RADIUS)
        deg = (plan.row_ptr[1:] - plan.row_ptr[:-1]).cpu()
        assert int(deg.min()) == 0 and int(deg.max()) >= 8 and plan.E > 300       # uneven degrees, some isolated atoms
    else:
        plan = dma.fully_connected_plan(list(SIZES), dev)
        assert plan.E == 7812 and plan.E % 64 != 0
    c.plan = _plan_for(net, plan, n, None)
    c.ctx = _context(net, c.layers, dev)
    c.ctx.set_graph(plan)
    c.ctx.pack(c.layers)
    assert c.L.egcl_backward_fused_supported(c.ctx.handle) == 1
    c.E = plan.E
    c.h, c.x = h, x
    c.dst, c.src = plan.edge_dst.cpu().long(), plan.edge_src.cpu().long()
    c.node_graph = plan.node_graph.cpu().long()
    c.gep = list(plan.graph_edge_ptr)
    lay = c.layers[0]
    c.p = {k: v.detach().cpu() for k, v in lay.state_dict().items()}
    return c


def _ref(c):
    """reference pieces every stage of a case shares (computed once): geometry, tables, first-layer pre-activations in both modes
    and the uncertainty of the device's scaled a1 against the model's"""
    if hasattr(c, "ref"):
        return c.ref
    r = R.NS()
    H = c.H
    r.diff_m, r.d2_m = R.geometry(c.x, c.dst, c.src, True)
    r.diff_e, r.d2_e = R.geometry(c.x, c.dst, c.src, False)
    # product of the table: bf16 head + remainder operands for H <= 48 (2^-16 each, egnn_forward.hip: launch_node_pre_f16), fp32 MFMA otherwise
    pert = 2.0 ** -15 if H <= 48 else (H + 2) * E24
    for name in ("x", "m"):
        W1, b1 = c.p[f"mlp_{name}.0.weight"], c.p[f"mlp_{name}.0.bias"]
        tm, te = R.tables(c.h, W1, b1, H, True), R.tables(c.h, W1, b1, H, False)
        dP, dQ = R.ulp_fp16(tm.P) + pert * tm.abs_P, R.ulp_fp16(tm.Q) + pert * tm.abs_Q
        pq = tm.P[c.dst] + tm.Q[c.src]
        wd2 = tm.wd * r.d2_m[:, None]
        # d2 = sqrtf(dx^2 + dy^2 + dz^2)^2: five roundings; the fma one more
        da1 = (E24 * (pq.abs() + 7.0 * wd2.abs()), dP[c.dst] + dQ[c.src] + R.ulp_fp16(pq))   # (acc, prop)
        setattr(r, "tab_" + name, (tm, te))
        setattr(r, "a1_" + name, (R.first_pre(tm, r.d2_m, c.dst, c.src, True), R.first_pre(te, r.d2_e, c.dst, c.src, False)))
        setattr(r, "da1_" + name, da1)
        setattr(r, "a1abs_" + name, tm.P[c.dst].abs() + tm.Q[c.src].abs() + wd2.abs())     # sum|terms| of a1 = P + Q + wd d2
    c.ref = r
    return r


def _da1(r, nm):
    acc, prop = getattr(r, "da1_" + nm)
    return acc + prop if _PROP[0] else acc


def _P(c, t):
    return c.lib.ptr(t)


def _table(c):
    c.lib.check(c.L.egcl_backward_table(c.ctx.handle, c.lib.stream_ptr(), 0, _P(c, c.hd)))


def _aggregates(c):
    """egcl_read_aggregates of the layer that was just run: (sum_m [N, M], sum_x [N, 3], sums of d^2 [B])"""
    sm, sx, sq = torch.empty(c.N, M, device=c.dev), torch.empty(c.N, 3, device=c.dev), torch.empty(c.B, device=c.dev)
    c.lib.check(c.L.egcl_read_aggregates(c.ctx.handle, c.lib.stream_ptr(), c.lib.NORM_GRAPH, _P(c, sm), _P(c, sx), _P(c, sq)))
    return sm, sx, sq


# edge counts up to which egcl_forward in bf16 takes the 32 / 64-edge-tile kernels at hidden width 512 / 1024 (host_logic.cpp:
# plan_forward); the training forward always takes the 128-edge tiles
SMALL_TILE_EDGES = int(os.environ.get("EGNN_SMALL64_EDGES", 6144))   # (the library's own measurement switch moves the limit)


def _kept(c):
    """egcl_forward_save into sentinel-filled buffers (once per case); -> device buffers + outputs"""
    if hasattr(c, "kept"):
        return c.kept
    E, Epad, dev = c.E, _ru(c.E, 64), c.dev
    nsplit = max(c.Wx // 512, 1)
    k = R.NS(nsplit=nsplit, Epad=Epad)
    k.s1x, k.s1m = torch.full((Epad, c.Wx), SENT, dtype=bf, device=dev), torch.full((Epad, c.Wm), SENT, dtype=bf, device=dev)
    k.t2x, k.t2m = torch.full((Epad, c.Wx), SENT, dtype=bf, device=dev), torch.full((Epad, M), SENT, dtype=bf, device=dev)
    k.shares = torch.full((nsplit, E), SENT, device=dev)
    k.ho, k.xo = torch.empty_like(c.hd), torch.empty_like(c.xd)
    _table(c)
    c.lib.check(c.L.egcl_forward_save(c.ctx.handle, c.lib.stream_ptr(), 0, c.lib.NORM_GRAPH, _P(c, c.hd), _P(c, c.xd), _P(c, k.ho),
                                      _P(c, k.xo), _P(c, k.s1x), _P(c, k.s1m), _P(c, k.t2x), _P(c, k.t2m), _P(c, k.shares)))
    k.agg = _aggregates(c)
    torch.cuda.synchronize()
    k.cpu = R.NS(**{n: getattr(k, n).cpu() for n in ("s1x", "s1m", "t2x", "t2m", "shares")})
    c.kept = k
    return k


def _second_layer(c, model, s1x=None, s1m=None):
    r, p = _ref(c), c.p
    i = 0 if model else 1
    d2 = r.d2_m if model else r.d2_e
    return R.forward_kept(r.tab_x[i], r.tab_m[i], d2, c.dst, c.src, p["mlp_x.2.weight"], p["mlp_x.2.bias"], p["mlp_m.2.weight"],
                          p["mlp_m.2.bias"], p["mlp_x.4.weight"], p["mlp_x.4.bias"], model, s1x, s1m)


def _s1_unc(want_s1, da1):
    # s1 (scaled) = silu_s(a1 scaled): |d s1 / d a1| = |SiLU'| <= 1.1; the chain itself: OPS fp32 operations
    return 1.1 * da1 + OPS * E24 * want_s1.abs()


def _t2_unc(fk, name, K):
    return (K + 2) * E24 * getattr(fk, "abs_t2" + name)


def _se_unc(fk, c, dt2x):
    w3s = R.f32(R.d(c.p["mlp_x.4.weight"]).reshape(-1) * R.K_NEG_LN2).abs()
    # the accumulation errors of the Wx pre-activations are independent: they add in quadrature (each at its worst-case size)
    return (c.Wx + 10 + OPS) * E24 * fk.abs_s_e + torch.sqrt(((1.1 * dt2x * w3s) ** 2).sum(1))


def _heads_unc(o, E, dtx=None, dtm=None):
    """uncertainties of the unrounded outputs of the head stage (R.heads) per element, and of its six sums over E edges.
    dtx / dtm: uncertainty of the (scaled) pre-activations where the stage computes them itself (recompute)."""
    u = R.NS()
    w3, wa = o.w3.abs(), o.wa.abs()
    dgsc = 4 * E24 * o.abs_gsc
    zx = 0.0 if dtx is None else dtx * LN2
    u.g_a2x = dgsc[:, None] * (w3 * o.dsx.abs()) + OPS * E24 * 1.1 * (o.gsc[:, None] * o.w3).abs() + (o.gsc[:, None] * o.w3).abs() * 0.5 * zx
    u_w3 = dgsc[:, None] * o.sx.abs() + OPS * E24 * (o.gsc[:, None] * o.sx).abs() + o.gsc.abs()[:, None] * 1.1 * zx
    zm = 0.0 if dtm is None else dtm * LN2
    dm = OPS * E24 * o.m.abs() + 1.1 * zm
    Km = o.m.shape[1] + 8
    ddot = Km * E24 * o.abs_dot + (o.gm.abs() * dm).sum(1)
    dz = Km * E24 * o.abs_z + (wa * dm).sum(1)
    gate = o.gate
    dgate = 0.25 * dz + 4 * E24 * gate
    dot = o.coef / (gate * (1 - gate)).clamp_min(1e-300)
    dcoef = ddot * gate * (1 - gate) + dot.abs() * dgate + 4 * E24 * o.coef.abs()
    inner = (o.gm * gate[:, None]).abs() + (o.coef[:, None] * o.wa).abs()
    u.g_a2m = ((o.gm.abs() * dgate[:, None] + dcoef[:, None] * wa) * o.dsm.abs() + OPS * E24 * 1.1 * inner + inner * 0.5 * zm)
    u_wa = dcoef[:, None] * o.m.abs() + o.coef.abs()[:, None] * dm + 4 * E24 * (o.coef[:, None] * o.m).abs()
    K = E + 64     # terms of a column sum + the partial sums on the way (LDS, atomics, the accumulator's old value)
    u.sums = dict(g_b2x=u.g_a2x.sum(0) + K * E24 * o.abs_g_b2x, g_w3=u_w3.sum(0) + K * E24 * o.abs_g_w3,
                  g_b3=dgsc.sum() + K * E24 * o.abs_g_b3, g_b2m=u.g_a2m.sum(0) + K * E24 * o.abs_g_b2m,
                  g_wa=u_wa.sum(0) + K * E24 * o.abs_g_wa, g_ba=dcoef.sum() + K * E24 * o.abs_g_ba)
    return u


def _dsabs(t, scaled=False):
    """sum|terms| of SiLU' = sg + s (1 - sg)"""
    _, ds, sg = R.act(R.d(t), scaled)
    return sg + (ds - sg).abs()


def _heads_plain(o, t2x, t2m, scaled, Kx, Km):
    """plain bounds K 2^-24 sum|terms| of dL/da2x = gsc w3 SiLU'(a2x) and dL/da2m = (g gate + coef wa) SiLU'(a2m), the terms being
    those of gsc (three products), of g . m inside coef and of SiLU' itself"""
    px = Kx * E24 * o.abs_gsc[:, None] * o.w3.abs() * _dsabs(t2x, scaled)
    gt = o.gate
    pm = Km * E24 * (o.gm.abs() * gt[:, None] + (o.abs_dot * gt * (1 - gt))[:, None] * o.wa.abs()) * _dsabs(t2m, scaled)
    return px, pm


def _split(c):
    """two unequal chunks, the second starting at an e_first that is not a multiple of 64"""
    n1 = (c.E * 3 // 8) | 1
    assert n1 % 64 != 0 and 0 < n1 < c.E
    return [(0, n1), (n1, c.E - n1)]


def _graph_split(c):
    """two chunks of whole graphs, both with edges"""
    cuts = [e for e in c.gep[1:-1] if 0 < e < c.E]
    a = cuts[0] if c.gep[1] > 0 else cuts[len(cuts) // 2]
    return [(0, a), (a, c.E - a)]


def _sum_bufs(c, init):
    dev = c.dev
    shapes = dict(g_b2x=c.Wx, g_w3=c.Wx, g_b3=1, g_b2m=M, g_wa=M, g_ba=1)
    return {k: torch.full((v,), init, device=dev) for k, v in shapes.items()}


# =============================================================================================================================
_WITH_H63 = [(w, g) for w in WIDTHS for g in GRAPHS] + [((63, 512, 256), "fully_connected")]
_WITH_H63_IDS = [f"{i}-{g}" for i in WIDTH_IDS for g in GRAPHS] + ["H63-fully_connected"]


@pytest.mark.parametrize("widths,graphs", _WITH_H63, ids=_WITH_H63_IDS)
def test_table_and_forward_save(widths, graphs):
    """egcl_backward_table + egcl_forward_save: the kept s1 / t2 rows and the sum of the s_e shares; rows E..Epad keep what the
    caller put there; (h_out, x_out) bitwise those of egcl_forward in bf16 where that runs the same 128-edge-tile kernels (the
    header's contract said "bitwise" without the condition: corrected), else the aggregates they are functions of agree within the
    fp32 accumulation of the same terms.  H = 63: odd, the largest H with 2H + 2 <= 128 (the
    table product runs on the fp32 MFMA kernel there)."""
    c = _case(*widths, graphs)
    rep = _Report("forward_save", c.id)
    k, r = _kept(c), _ref(c)
    E = c.E
    for n_ in ("s1x", "s1m", "t2x", "t2m"):   # rows past E: untouched
        assert bool((getattr(k.cpu, n_)[E:].float() == SENT).all()), n_
    fm, fe = _second_layer(c, True), _second_layer(c, False)
    # t2 / s_e from the DEVICE's own s1 (bitwise the MFMA operand the device used)
    fd = _second_layer(c, True, k.cpu.s1x[:E], k.cpu.s1m[:E])
    p = c.p
    # ... and its exact continuation: fp32 weights, no rounding
    fx = R.forward_kept(None, None, None, c.dst, c.src, p["mlp_x.2.weight"], p["mlp_x.2.bias"], p["mlp_m.2.weight"], p["mlp_m.2.bias"],
                        p["mlp_x.4.weight"], p["mlp_x.4.bias"], False, k.cpu.s1x[:E], k.cpu.s1m[:E])
    for nm, K in (("x", c.Wx), ("m", c.Wm)):
        s1w = getattr(fm, "s1" + nm)
        u, a = _both(lambda: _s1_unc(s1w, _da1(r, nm)))
        rep.check("s1" + nm, getattr(k.cpu, "s1" + nm)[:E], s1w, u, True, getattr(fe, "s1" + nm), a, 3 * E24 * getattr(r, "a1abs_" + nm))
        rep.check("t2" + nm, getattr(k.cpu, "t2" + nm)[:E], getattr(fd, "t2" + nm + "_unrounded"), _t2_unc(fd, nm, K), True,
                  getattr(fx, "t2" + nm), None, K * E24 * getattr(fd, "abs_t2" + nm))
        # the whole chain from h: model and device are two roundings of the same exact values
        e_dev = (R.d(getattr(k.cpu, "t2" + nm)[:E]) - getattr(fe, "t2" + nm)).norm(dim=1)
        e_mod = (getattr(fm, "t2" + nm) - getattr(fe, "t2" + nm)).norm(dim=1)
        q = float((e_dev / (2 * e_mod).clamp_min(1e-300)).max())
        print(f"bwd-stage-ratio forward_save   {c.id:<28s} t2{nm}-chain model      nan  exact {q:8.3f}")
        if not q <= 1.0:
            rep.fail.append(("t2" + nm, "chain from h: 2 x model error against exact", q))
    s_e = R.d(k.cpu.shares).sum(0)
    rep.check("s_e", s_e, fd.s_e, _se_unc(fd, c, _t2_unc(fd, "x", c.Wx)), False, fx.s_e, None, c.Wx * E24 * fd.abs_s_e)
    # the same layer through egcl_forward (bf16): bitwise the same outputs
    ho, xo = torch.empty_like(c.hd), torch.empty_like(c.xd)
    c.lib.check(c.L.egcl_forward(c.ctx.handle, c.lib.stream_ptr(), 0, c.lib.PREC_BF16, c.lib.NORM_GRAPH, _P(c, c.hd), _P(c, c.xd),
                                 _P(c, ho), _P(c, xo)))
    if c.E > SMALL_TILE_EDGES or c.Wx == 256:
        rep.same("h_out", k.ho, ho)
        rep.same("x_out", k.xo, xo)
    else:
        # egcl_forward ran its small-tile kernels: the same products on other tile shapes.  The per-edge values differ by their fp32
        # accumulation, the segment sums by their association; (h_out, x_out) are functions of the three aggregates, which must
        # agree within exactly that
        sm1, sx1, sq1 = (t.cpu() for t in k.agg)
        sm2, sx2, sq2 = (t.cpu() for t in _aggregates(c))
        m, _, _ = R.act(R.d(k.cpu.t2m[:E]), True)
        wa = R.d(p["attention.0.weight"]).reshape(-1)
        gate = torch.sigmoid(m @ wa + R.d(p["attention.0.bias"])[0])
        dm = 1.1 * LN2 * _t2_unc(fd, "m", c.Wm) + OPS * E24 * m.abs()
        dgate = 0.25 * ((M + 8) * E24 * (m.abs() @ wa.abs()) + dm @ wa.abs()) + 4 * E24 * gate
        deg = torch.bincount(c.dst, minlength=c.N)[:, None] + 8.0
        zm, zx = torch.zeros(c.N, M, dtype=D), torch.zeros(c.N, 3, dtype=D)
        out_m = m * gate[:, None]
        u_m = zm.index_add(0, c.dst, dm * gate[:, None] + m.abs() * dgate[:, None]) + deg * E24 * zm.index_add(0, c.dst, out_m.abs())
        rep.check("sum_m", sm2, R.d(sm1), 2 * u_m, plain=deg * E24 * zm.index_add(0, c.dst, out_m.abs()))
        xm = r.diff_m * s_e[:, None]
        du = r.diff_m.abs() * _se_unc(fd, c, _t2_unc(fd, "x", c.Wx))[:, None]
        u_x = zx.index_add(0, c.dst, du) + (deg + k.nsplit) * E24 * zx.index_add(0, c.dst, xm.abs())
        rep.check("sum_x", sx2, R.d(sx1), 2 * u_x, plain=deg * E24 * zx.index_add(0, c.dst, xm.abs()))
        rep.check("sq_sums", sq2, R.d(sq1), 2 * (max(b - a for a, b in zip(c.gep[:-1], c.gep[1:])) + 8) * E24 * R.d(sq1).abs())
        scale = (1.0 / (torch.sqrt(R.d(sq1)) + 1.0))[c.node_graph][:, None]
        rep.check("x_out", xo, R.d(k.xo.cpu()), 2 * u_x * scale + 4 * E24 * R.d(k.xo.cpu()).abs())
    rep.done()


def _upstream(c):
    if not hasattr(c, "up"):
        g = torch.Generator().manual_seed(23)
        c.up = (torch.randn(c.N, 3, generator=g) * 0.3, torch.randn(c.N, M, generator=g) * 0.1)
    return c.up


@pytest.mark.parametrize("graphs", GRAPHS)
@pytest.mark.parametrize("widths", WIDTHS, ids=WIDTH_IDS)
def test_heads_saved(widths, graphs):
    """egcl_backward_heads_saved on the kept t2 / s_e shares READ BACK from the device (the reference starts from the very same
    bf16 values), random upstream gradients, two unequal chunks (e_first not a multiple of 64: the offset into s_shares), the six
    sums ADDED to a non-zero accumulator"""
    c = _case(*widths, graphs)
    rep = _Report("heads_saved", c.id)
    k, r = _kept(c), _ref(c)
    E = c.E
    gsx, gsm = _upstream(c)
    t2x, t2m = k.t2x.clone(), k.t2m.clone()
    g_diff = torch.full((E, 3), SENT, device=c.dev)
    init = 0.375
    sums = _sum_bufs(c, init)
    gsxd, gsmd = gsx.to(c.dev), gsm.to(c.dev)
    for a, n in _split(c):
        c.lib.check(c.L.egcl_backward_heads_saved(c.ctx.handle, c.lib.stream_ptr(), 0, _P(c, c.xd), _P(c, gsxd), _P(c, gsmd), a, n,
                                                  _P(c, t2x[a:]), _P(c, t2m[a:]), _P(c, k.shares), _P(c, g_diff[a:]),
                                                  *[_P(c, sums[s]) for s in ("g_b2x", "g_w3", "g_b3", "g_b2m", "g_wa", "g_ba")]))
    torch.cuda.synchronize()
    assert bool((t2x[E:].float() == SENT).all()) and bool((t2m[E:].float() == SENT).all())
    p = c.p
    s_e = R.d(k.cpu.shares).sum(0)
    args = (k.cpu.t2x[:E], k.cpu.t2m[:E])
    tail = (c.dst, gsx, gsm, s_e, p["mlp_x.4.weight"], p["attention.0.weight"], p["attention.0.bias"])
    om = R.heads(*args, r.diff_m, *tail, scaled=True, model=True)
    oe = R.heads(*args, r.diff_e, *tail, scaled=True, model=False)
    u = _heads_unc(om, E)
    px, pm = _heads_plain(om, args[0], args[1], True, 4, M)
    rep.check("g_a2x", t2x[:E], om.g_a2x_unrounded, u.g_a2x, True, oe.g_a2x, None, px)
    rep.check("g_a2m", t2m[:E], om.g_a2m_unrounded, u.g_a2m, True, oe.g_a2m, None, pm)
    sh = R.d(k.cpu.shares).abs().sum(0)
    rep.check("g_diff", g_diff, om.g_diff, (k.nsplit + 2) * E24 * om.gx.abs() * sh[:, None], False, oe.g_diff, None,
              (k.nsplit + 1) * E24 * om.gx.abs() * sh[:, None])
    for s in sums:
        want, unc = getattr(om, s) + init, u.sums[s] + (E + 64) * E24 * init
        rep.check(s, sums[s].reshape(want.shape), want, unc, False, getattr(oe, s) + init, None, E * E24 * (getattr(om, "abs_" + s) + init))
    rep.done()


@pytest.mark.parametrize("graphs", GRAPHS)
@pytest.mark.parametrize("widths", WIDTHS, ids=WIDTH_IDS)
def test_edge_recompute(widths, graphs):
    """egcl_backward_edge_recompute from h, x and the parameters: s1 against the table model, dL/da2 / g_diff / the six sums against
    the rounding model continued from the s1 rows the call itself wrote (the MFMA operand, bitwise)"""
    c = _case(*widths, graphs)
    rep = _Report("edge_recompute", c.id)
    r = _ref(c)
    E, dev = c.E, c.dev
    gsx, gsm = _upstream(c)
    gsxd, gsmd = gsx.to(dev), gsm.to(dev)
    Er = _ru(E, 64) + 64
    s1x, s1m = torch.full((Er, c.Wx), SENT, dtype=bf, device=dev), torch.full((Er, c.Wm), SENT, dtype=bf, device=dev)
    gax, gam = torch.full((Er, c.Wx), SENT, dtype=bf, device=dev), torch.full((Er, M), SENT, dtype=bf, device=dev)
    g_diff = torch.full((Er, 3), SENT, device=dev)
    init = -0.25
    sums = _sum_bufs(c, init)
    _table(c)
    for a, n in _split(c):
        c.lib.check(c.L.egcl_backward_edge_recompute(c.ctx.handle, c.lib.stream_ptr(), 0, _P(c, c.xd), _P(c, gsxd), _P(c, gsmd), a, n,
                                                     _P(c, s1x[a:]), _P(c, s1m[a:]), _P(c, gax[a:]), _P(c, gam[a:]), _P(c, g_diff[a:]),
                                                     *[_P(c, sums[s]) for s in ("g_b2x", "g_w3", "g_b3", "g_b2m", "g_wa", "g_ba")]))
    torch.cuda.synchronize()
    for t in (s1x, s1m, gax, gam, g_diff):   # the rows past the last chunk: untouched
        assert bool((t[E:].float() == SENT).all())
    fm, fe = _second_layer(c, True), _second_layer(c, False)
    s1xc, s1mc = s1x[:E].cpu(), s1m[:E].cpu()
    for nm, got_ in (("x", s1xc), ("m", s1mc)):
        s1w = getattr(fm, "s1" + nm)
        u_, a_ = _both(lambda: _s1_unc(s1w, _da1(r, nm)))
        rep.check("s1" + nm, got_, s1w, u_, True, getattr(fe, "s1" + nm), a_, 3 * E24 * getattr(r, "a1abs_" + nm))
    fd = _second_layer(c, True, s1xc, s1mc)
    dtx, dtm = _t2_unc(fd, "x", c.Wx), _t2_unc(fd, "m", c.Wm)
    p = c.p
    tail = (c.dst, gsx, gsm, fd.s_e, p["mlp_x.4.weight"], p["attention.0.weight"], p["attention.0.bias"])
    om = R.heads(fd.t2x_unrounded, fd.t2m_unrounded, r.diff_m, *tail, scaled=True, model=True)
    # exact continuation of the same stored activations: fp32 weights, no rounding
    fx = R.forward_kept(None, None, None, c.dst, c.src, p["mlp_x.2.weight"], p["mlp_x.2.bias"], p["mlp_m.2.weight"], p["mlp_m.2.bias"],
                        p["mlp_x.4.weight"], p["mlp_x.4.bias"], False, s1xc, s1mc)
    oe = R.heads(fx.t2x / -R.LOG2E, fx.t2m / -R.LOG2E, r.diff_e, c.dst, gsx, gsm, fx.s_e, *tail[4:])
    u = _heads_unc(om, E, dtx, dtm)
    px, pm = _heads_plain(om, fd.t2x_unrounded, fd.t2m_unrounded, True, c.Wx, c.Wm)
    rep.check("g_a2x", gax[:E], om.g_a2x_unrounded, u.g_a2x, True, oe.g_a2x, None, px)
    rep.check("g_a2m", gam[:E], om.g_a2m_unrounded, u.g_a2m, True, oe.g_a2m, None, pm)
    rep.check("g_diff", g_diff[:E], om.g_diff, om.gx.abs() * _se_unc(fd, c, dtx)[:, None] + 2 * E24 * om.g_diff.abs(), False, oe.g_diff,
              None, om.gx.abs() * (c.Wx * E24 * fd.abs_s_e)[:, None])
    for s in sums:
        want, unc = getattr(om, s) + init, u.sums[s] + (E + 64) * E24 * abs(init)
        rep.check(s, sums[s].reshape(want.shape), want, unc, False, getattr(oe, s) + init, None,
                  E * E24 * (getattr(om, "abs_" + s) + abs(init)))
    rep.done()


def _g_a2(c, sparse=False, chunks=None):
    """dL/da2 of both MLPs as bf16 the test chooses; sparse: one non-zero row per 128-edge tile position 0, 31, 32, 63, 64, 127 of
    every tile of a chunk and the chunk's last row"""
    g = torch.Generator().manual_seed(29)
    gx, gm = (torch.randn(c.E, c.Wx, generator=g) * 0.05).to(bf), (torch.randn(c.E, M, generator=g) * 0.05).to(bf)
    rows = None
    if sparse:
        keep = torch.zeros(c.E, dtype=torch.bool)
        for a, n in chunks:
            idx = torch.arange(n)
            pos = idx % 128
            keep[a:a + n] = (pos == 0) | (pos == 31) | (pos == 32) | (pos == 63) | (pos == 64) | (pos == 127) | (idx == n - 1)
        gx[~keep], gm[~keep] = 0, 0
        rows = keep
    return gx, gm, rows


def _padded(t, dev):
    """the rows of `t` on the device, followed by a tile of zero rows (no kernel is given a reason to read past an allocation)"""
    return torch.cat((t, torch.zeros(128, t.shape[1], dtype=t.dtype))).to(dev)


def _g1_unc(dg, da1, Kd, bf16_dot):
    """uncertainty of g1 = dot * SiLU'(a1) BEFORE its own final rounding: the fp32 accumulation of dot (and, chain form, the bf16
    rounding of dot that may flip), SiLU'' <= 0.5 on the uncertainty of the scaled a1 (d z = ln 2 d t), OPS element-wise operations"""
    ddot = (Kd + 2) * E24 * dg.abs_dot + (R.ulp_bf16(dg.dot) if bf16_dot and _PROP[0] else 0.0)
    return ddot * dg.ds.abs() + dg.dot.abs() * (0.5 * LN2 * da1 + OPS * E24 * 1.1)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "tile-rows"])
@pytest.mark.parametrize("graphs", GRAPHS)
@pytest.mark.parametrize("widths", WIDTHS, ids=WIDTH_IDS)
def test_dgrad(widths, graphs, sparse):
    """egcl_backward_dgrad: g1 = (g_a2 . W2) * SiLU'(a1) for both MLPs on g_a2 the test chooses, two chunks; tile-rows: every output
    row of a zero input row must be exactly zero, every other row must match"""
    c = _case(*widths, graphs)
    rep = _Report("dgrad", c.id + ("-rows" if sparse else ""))
    r = _ref(c)
    chunks = _split(c)
    gx, gm, rows = _g_a2(c, sparse, chunks)
    gxd, gmd = _padded(gx, c.dev), _padded(gm, c.dev)
    Er = _ru(c.E, 64) + 64
    o1x, o1m = torch.full((Er, c.Wx), SENT, dtype=bf, device=c.dev), torch.full((Er, c.Wm), SENT, dtype=bf, device=c.dev)
    _table(c)
    for a, n in chunks:
        c.lib.check(c.L.egcl_backward_dgrad(c.ctx.handle, c.lib.stream_ptr(), 0, _P(c, c.xd), a, n, _P(c, gxd[a:]), _P(c, gmd[a:]),
                                            _P(c, o1x[a:]), _P(c, o1m[a:])))
    torch.cuda.synchronize()
    assert bool((o1x[c.E:].float() == SENT).all()) and bool((o1m[c.E:].float() == SENT).all())
    for nm, g_a2, out, Kd in (("x", gx, o1x, c.Wx), ("m", gm, o1m, M)):
        W2 = c.p[f"mlp_{nm}.2.weight"]
        a1m, a1e = getattr(r, "a1_" + nm)
        dm_ = R.dgrad(g_a2, W2, a1m, True, True, "chain")
        de_ = R.dgrad(g_a2, W2, a1e, False, False)
        got = out[:c.E].cpu()
        if sparse:
            assert bool((got[~rows].float() == 0).all()), ("rows of zero input rows must be exactly zero", nm)
            assert bool((got[rows].float() != 0).any(dim=1).all()), nm
        u_, a_ = _both(lambda: _g1_unc(dm_, _da1(r, nm), Kd, True))
        rep.check("g1" + nm, got, dm_.dot * dm_.ds, u_, True, de_.g1, a_, Kd * E24 * dm_.abs_dot * (dm_.sg + (dm_.ds - dm_.sg).abs()))
    rep.done()


def _reduce_unc(fr, ug, g1, d2, wd, c, K_node, K_graph, W, bf16_terms, scaled):
    """bounds of Gd / Gs / cd / gd2 from the per-element uncertainty ug of g1"""
    z = lambda rws: torch.zeros(rws, W, dtype=D)
    ut = ug + (R.ulp_bf16(g1) if bf16_terms and _PROP[0] else 0.0)
    u = R.NS()
    u.Gd = z(c.N).index_add_(0, c.dst, ut) + K_node * E24 * fr.abs_Gd
    u.Gs = z(c.N).index_add_(0, c.src, ut) + K_node * E24 * fr.abs_Gs
    eg = c.node_graph[c.dst]
    u.cd = z(c.B).index_add_(0, eg, ug * d2[:, None]) + (K_graph + 8) * E24 * fr.abs_cd
    u.gd2 = (ug * wd.abs()).sum(1) * (LN2 if scaled else 1.0) + (W + 16) * E24 * fr.abs_gd2
    return u


@pytest.mark.parametrize("widths,graphs", _WITH_H63, ids=_WITH_H63_IDS)
def test_dgrad_reduce(widths, graphs):
    """egcl_backward_dgrad_reduce over two chunks of whole graphs (e_first > 0 for the second): G per block, cd per graph and the
    sum of the gd2 shares per edge; everything pre-filled with a sentinel: rows of graphs without edges and of graphs outside the
    chunk stay untouched, cd rows of the chunk's graphs are ASSIGNED"""
    c = _case(*widths, graphs)
    rep = _Report("dgrad_reduce", c.id)
    r = _ref(c)
    Wx, Wm, N, B, E, dev = c.Wx, c.Wm, c.N, c.B, c.E, c.dev
    gx, gm, _ = _g_a2(c)
    gxd, gmd = _padded(gx, dev), _padded(gm, dev)
    G = torch.full((N, 2 * Wx + 2 * Wm), SENT, dtype=bf, device=dev)
    cdx, cdm = torch.full((B, Wx), SENT, device=dev), torch.full((B, Wm), SENT, device=dev)
    nparts = (Wx + Wm) // 256
    chunks = _graph_split(c)
    parts = [torch.full((nparts, n), SENT, device=dev) for _, n in chunks]
    gptr = [0] + torch.cumsum(torch.tensor(SIZES), 0).tolist()
    has_edges = [c.gep[g + 1] > c.gep[g] for g in range(B)]
    assert not all(has_edges)
    _table(c)
    for ci, (a, n) in enumerate(chunks):
        c.lib.check(c.L.egcl_backward_dgrad_reduce(c.ctx.handle, c.lib.stream_ptr(), 0, _P(c, c.xd), a, n, _P(c, gxd[a:]), _P(c, gmd[a:]),
                                                   _P(c, G), _P(c, cdx), _P(c, cdm), _P(c, parts[ci])))
        if ci == 0:   # graphs outside the first chunk and graphs without edges: nothing written yet
            torch.cuda.synchronize()
            for g in range(B):
                inside = has_edges[g] and c.gep[g + 1] <= a + n
                rows_g = G[gptr[g]:gptr[g + 1]].float()
                if not inside:
                    assert bool((rows_g == SENT).all()) and bool((cdx[g] == SENT).all()) and bool((cdm[g] == SENT).all()), g
                else:
                    assert bool((rows_g != SENT).any()) and bool((cdx[g] != SENT).any()), g
    torch.cuda.synchronize()
    Gc, gd2_got = G.cpu(), torch.cat([R.d(pt.cpu()).sum(0) for pt in parts])
    for g in range(B):
        if not has_edges[g]:
            assert bool((Gc[gptr[g]:gptr[g + 1]].float() == SENT).all()) and bool((cdx[g] == SENT).all()) and bool((cdm[g] == SENT).all())
    live_n = torch.tensor([has_edges[int(g)] for g in c.node_graph])
    live_g = torch.tensor(has_edges)
    gd2_want, gd2_unc, gd2_exact, gd2_acc, gd2_plain = 0.0, 0.0, 0.0, 0.0, 0.0
    Kn, Kg = 2 * 64 + 2, max(c.gep[g + 1] - c.gep[g] for g in range(B)) + 2
    for nm, g_a2, Kd, W, off, cd in (("x", gx, Wx, Wx, 0, cdx), ("m", gm, M, Wm, 2 * Wx, cdm)):
        W2 = c.p[f"mlp_{nm}.2.weight"]
        a1m, a1e = getattr(r, "a1_" + nm)
        tm, te = getattr(r, "tab_" + nm)
        dm_ = R.dgrad(g_a2, W2, a1m, True, True, "graph")
        de_ = R.dgrad(g_a2, W2, a1e, False, False)
        fm = R.first_reduce(dm_.g1, r.d2_m, tm.wd, c.dst, c.src, c.node_graph, N, B, True, "graph", True)
        fe = R.first_reduce(de_.g1, r.d2_e, te.wd, c.dst, c.src, c.node_graph, N, B)
        u, a = _both(lambda: _reduce_unc(fm, _g1_unc(dm_, _da1(r, nm), Kd, False), dm_.g1, r.d2_m, tm.wd, c, Kn, Kg, W, True, True))
        rep.check("Gd_" + nm, Gc[:, off:off + W][live_n], fm.Gd_unrounded[live_n], u.Gd[live_n], True, fe.Gd[live_n], a.Gd[live_n],
                  64 * E24 * fm.abs_Gd[live_n])
        rep.check("Gs_" + nm, Gc[:, off + W:off + 2 * W][live_n], fm.Gs_unrounded[live_n], u.Gs[live_n], True, fe.Gs[live_n], a.Gs[live_n],
                  64 * E24 * fm.abs_Gs[live_n])
        rep.check("cd_" + nm, cd.cpu()[live_g], fm.cd[live_g], u.cd[live_g], False, fe.cd[live_g], a.cd[live_g], Kg * E24 * fm.abs_cd[live_g])
        gd2_want, gd2_unc, gd2_exact, gd2_acc = gd2_want + fm.gd2, gd2_unc + u.gd2, gd2_exact + fe.gd2, gd2_acc + a.gd2
        gd2_plain = gd2_plain + W * E24 * fm.abs_gd2
    rep.check("gd2", gd2_got, gd2_want, gd2_unc, False, gd2_exact, gd2_acc, gd2_plain)
    rep.done()


@pytest.mark.parametrize("graphs", GRAPHS)
@pytest.mark.parametrize("widths", WIDTHS, ids=WIDTH_IDS)
def test_first_reduce(widths, graphs):
    """egcl_backward_first_reduce on random bf16 g1, two chunks that cut through graphs: Gd / Gs / cd ACCUMULATE across the chunks
    (on top of a non-zero start), gd2_part is ASSIGNED; rows of graphs without edges stay untouched"""
    c = _case(*widths, graphs)
    rep = _Report("first_reduce", c.id)
    r = _ref(c)
    Wx, Wm, N, B, E, dev = c.Wx, c.Wm, c.N, c.B, c.E, c.dev
    g = torch.Generator().manual_seed(37)
    g1 = {"x": (torch.randn(E, Wx, generator=g) * 0.1).to(bf), "m": (torch.randn(E, Wm, generator=g) * 0.1).to(bf)}
    wd = {"x": torch.randn(Wx, generator=g) * 0.2, "m": torch.randn(Wm, generator=g) * 0.2}
    init = 0.5
    f = lambda rows, W: torch.full((rows, W), init, device=dev)
    Gd, Gs, cd = {"x": f(N, Wx), "m": f(N, Wm)}, {"x": f(N, Wx), "m": f(N, Wm)}, {"x": f(B, Wx), "m": f(B, Wm)}
    nparts = (Wx + Wm) // 256
    chunks = _split(c)
    if graphs == "fully_connected":
        assert chunks[0][1] not in c.gep      # the cut runs through a graph
    parts = [torch.full((nparts, n), SENT, device=dev) for _, n in chunks]
    g1d, wdd = {k: _padded(v, dev) for k, v in g1.items()}, {k: v.to(dev) for k, v in wd.items()}
    plan = c.ctx.plan
    for ci, (a, n) in enumerate(chunks):
        c.lib.check(c.L.egcl_backward_first_reduce(c.lib.stream_ptr(), B, plan.max_graph_nodes, a, n, _P(c, plan.graph_ptr),
                                                   _P(c, plan.row_ptr), _P(c, plan.edge_src), _P(c, c.xd), _P(c, g1d["x"][a:]), Wx,
                                                   _P(c, g1d["m"][a:]), Wm, _P(c, wdd["x"]), _P(c, wdd["m"]), _P(c, Gd["x"]), _P(c, Gs["x"]),
                                                   _P(c, Gd["m"]), _P(c, Gs["m"]), _P(c, cd["x"]), _P(c, cd["m"]), _P(c, parts[ci])))
    torch.cuda.synchronize()
    gptr = [0] + torch.cumsum(torch.tensor(SIZES), 0).tolist()
    gd2_got = torch.cat([R.d(pt.cpu()).sum(0) for pt in parts])
    gd2_want, gd2_unc = 0.0, 0.0
    Kn, Kg = 2 * 64 + 4, max(c.gep[i + 1] - c.gep[i] for i in range(B)) + 4
    for nm, W in (("x", Wx), ("m", Wm)):
        fm = R.first_reduce(g1[nm], r.d2_m, wd[nm], c.dst, c.src, c.node_graph, N, B, True, "reduce")
        u = _reduce_unc(fm, torch.zeros(E, W, dtype=D), R.d(g1[nm]), r.d2_m, R.d(wd[nm]), c, Kn, Kg, W, False, False)
        for gi in range(B):
            if c.gep[gi + 1] == c.gep[gi]:
                for t in (Gd[nm], Gs[nm]):
                    assert bool((t[gptr[gi]:gptr[gi + 1]] == init).all()), (nm, gi)
                assert bool((cd[nm][gi] == init).all()), (nm, gi)
        rep.check("Gd_" + nm, Gd[nm], fm.Gd + init, u.Gd + Kn * E24 * init, False, fm.Gd + init, None, 64 * E24 * (fm.abs_Gd + init))
        rep.check("Gs_" + nm, Gs[nm], fm.Gs + init, u.Gs + Kn * E24 * init, False, fm.Gs + init, None, 64 * E24 * (fm.abs_Gs + init))
        rep.check("cd_" + nm, cd[nm], fm.cd + init, u.cd + Kg * E24 * init, False, fm.cd + init, None, Kg * E24 * (fm.abs_cd + init))
        gd2_want, gd2_unc = gd2_want + fm.gd2, gd2_unc + u.gd2
    rep.check("gd2", gd2_got, gd2_want, gd2_unc, False, gd2_want, None, gd2_unc)
    rep.done()


@pytest.mark.parametrize("seg", ["segments", "one-sum"])
@pytest.mark.parametrize("nparts", [2, 3, 8])
@pytest.mark.parametrize("graphs", GRAPHS)
def test_scatter_geom(graphs, nparts, seg):
    """egcl_backward_scatter_geom against float64: nparts shares of dL/d(d2), node_segment given and NULL, g_x starts non-zero"""
    c = _case(36, 256, 256, graphs)
    rep = _Report("scatter_geom", f"{graphs}-{nparts}-{seg}")
    r = _ref(c)
    E, N, dev = c.E, c.N, c.dev
    g = torch.Generator().manual_seed(41 + nparts)
    part, g_diff = torch.randn(nparts, E, generator=g) * 0.2, torch.randn(E, 3, generator=g)
    g_S = torch.randn(c.B if seg == "segments" else 1, generator=g) * 0.3
    g_x0 = torch.randn(N, 3, generator=g)
    g_x = g_x0.to(dev)
    plan = c.ctx.plan
    partd, gdd, gSd = part.to(dev), g_diff.to(dev), g_S.to(dev)
    c.lib.check(c.L.egcl_backward_scatter_geom(c.lib.stream_ptr(), E, nparts, _P(c, plan.edge_dst), _P(c, plan.edge_src), _P(c, c.xd),
                                               _P(c, partd), _P(c, gdd), _P(c, gSd), _P(c, plan.node_graph) if seg == "segments" else None,
                                               _P(c, g_x)))
    torch.cuda.synchronize()
    node_seg = c.node_graph if seg == "segments" else None
    gd2 = R.d(part).sum(0)
    wm = R.scatter_geom(gd2, g_diff, g_S, node_seg, r.diff_m, c.dst, c.src, g_x0)
    we = R.scatter_geom(gd2, g_diff, g_S, node_seg, r.diff_e, c.dst, c.src, g_x0)
    gS_e = (R.d(g_S)[node_seg[c.dst]] if node_seg is not None else R.d(g_S)[0].expand(E)).abs()
    tot_abs = R.d(part).abs().sum(0) + gS_e
    u_e = ((nparts + 2) * E24 * tot_abs)[:, None] * 2 * r.diff_m.abs() + 3 * E24 * (wm.gv.abs() + R.d(g_diff).abs())
    z = torch.zeros(N, 3, dtype=D)
    deg = torch.bincount(c.dst, minlength=N) + torch.bincount(c.src, minlength=N)
    unc = z.index_add(0, c.dst, u_e).index_add(0, c.src, u_e) + ((deg + 2)[:, None] * E24) * wm.abs_g_x
    rep.check("g_x", g_x, wm.g_x, unc, False, we.g_x, None, ((deg + 2)[:, None] * E24) * wm.abs_g_x)
    rep.done()


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(256, 256, 256), (30, 22, 10)], ids=["vec", "odd"])
def test_generic_chain_stages(shape, prec):
    """egcl_backward_l1_act / _heads / _l1_grad (the generic chain, fp32 arithmetic, storage fp32 or bf16) on 1,001 edges of the
    ragged graphs that run across a graph boundary; l1_act / l1_grad at both first-layer widths; (30, 22), M = 10 take the
    scalar-access variants"""
    Wx_, Wm_, M_ = shape
    c = _case(36, 256, 256, "fully_connected")
    rep = _Report("generic_chain", f"W{Wx_}-{Wm_}-M{M_}-{prec}")
    lib, L, dev = c.lib, c.L, c.dev
    e0, n = 3500, 1001
    assert c.gep[1] in range(e0, e0 + n)
    dst, src = c.dst[e0:e0 + n], c.src[e0:e0 + n]
    plan = c.ctx.plan
    dstd, srcd = plan.edge_dst[e0:e0 + n].contiguous(), plan.edge_src[e0:e0 + n].contiguous()
    PREC = lib.PREC_F32 if prec == "f32" else lib.PREC_BF16
    sdt = torch.float32 if prec == "f32" else bf
    is_bf = prec == "bf16"
    g = torch.Generator().manual_seed(43)
    diff_m, d2_m = R.geometry(c.x, dst, src, True)
    diff_e, d2_e = R.geometry(c.x, dst, src, False)
    d2d = d2_m.float().to(dev)                      # the stage takes d2 as an operand
    d2_op = R.d(d2d.cpu())
    # ---- l1_act and l1_grad at both first-layer widths (mlp_x: 256 / 30, mlp_m: 256 / 22), fp32 tables the test chooses
    for tag, C_ in (("x", Wx_), ("m", Wm_)):
        P_, Q_ = torch.randn(c.N, C_, generator=g) * 1.5, torch.randn(c.N, C_, generator=g) * 1.5
        wd = torch.randn(C_, generator=g) * 0.1
        tab = R.NS(P=R.d(P_), Q=R.d(Q_), wd=R.d(wd), scaled=False)
        pq = R.f32(tab.P[dst] + tab.Q[src])
        a1 = R.f32(pq + tab.wd * d2_op[:, None])         # backward.hip:123 fmaf(w, d, p + q)
        s, ds, sg = R.act(a1)
        da1 = 2 * E24 * (pq.abs() + (tab.wd * d2_op[:, None]).abs())
        # exp(-a) of a rounded argument, 1-ulp exp and rcp: sigmoid carries (|a| + OPS) 2^-24 sg (1 - sg) + OPS 2^-24 sg
        dsg = E24 * ((a1.abs() + OPS) * sg * (1 - sg) + OPS * sg)
        out = torch.full((n + 1, C_), SENT, dtype=sdt, device=dev)
        Pd, Qd, wdd = P_.to(dev), Q_.to(dev), wd.to(dev)
        lib.check(L.egcl_backward_l1_act(lib.stream_ptr(), PREC, n, C_, _P(c, dstd), _P(c, srcd), _P(c, Pd), _P(c, Qd), _P(c, wdd), _P(c, d2d),
                                         _P(c, out)))
        torch.cuda.synchronize()
        assert bool((out[n].float() == SENT).all())
        s_exact = R.act(tab.P[dst] + tab.Q[src] + tab.wd * d2_op[:, None])[0]
        rep.check("s1" + tag, out[:n], s, 1.1 * da1 + a1.abs() * dsg + 2 * E24 * s.abs(), is_bf, s_exact, None,
                  4 * E24 * (tab.P[dst].abs() + tab.Q[src].abs() + (tab.wd * d2_op[:, None]).abs()))
        gs1 = (torch.randn(n, C_, generator=g)).to(sdt)
        buf = torch.full((n + 1, C_), SENT, dtype=sdt, device=dev)
        buf[:n] = gs1.to(dev)
        lib.check(L.egcl_backward_l1_grad(lib.stream_ptr(), PREC, n, C_, _P(c, dstd), _P(c, srcd), _P(c, Pd), _P(c, Qd), _P(c, wdd), _P(c, d2d),
                                          _P(c, buf)))
        torch.cuda.synchronize()
        assert bool((buf[n].float() == SENT).all())
        dds = 0.5 * da1 + dsg * (1 + a1.abs()) + (OPS * E24) * 1.1          # ds = sg (1 + a (1 - sg))
        ds_exact = R.act(tab.P[dst] + tab.Q[src] + tab.wd * d2_op[:, None])[1]
        rep.check("g_a1" + tag, buf[:n], R.d(gs1) * ds, R.d(gs1).abs() * dds, is_bf, R.d(gs1) * ds_exact, None,
                  4 * E24 * R.d(gs1).abs() * (sg + (ds - sg).abs()))
    # ---- heads on a2 (no bias) the test chooses
    a2x, a2m = (torch.randn(n, Wx_, generator=g) * 2).to(sdt), (torch.randn(n, M_, generator=g) * 2).to(sdt)
    b2x, w3, b3 = torch.randn(Wx_, generator=g) * 0.5, torch.randn(Wx_, generator=g) * 0.1, torch.randn(1, generator=g)
    b2m, wa, ba = torch.randn(M_, generator=g) * 0.5, torch.randn(M_, generator=g) * 0.2, torch.randn(1, generator=g)
    gsx, gsm = torch.randn(c.N, 3, generator=g) * 0.3, torch.randn(c.N, M_, generator=g) * 0.1
    ax, am = torch.full((n + 1, Wx_), SENT, dtype=sdt, device=dev), torch.full((n + 1, M_), SENT, dtype=sdt, device=dev)
    ax[:n], am[:n] = a2x.to(dev), a2m.to(dev)
    g_diff = torch.full((n + 1, 3), SENT, device=dev)
    init = 0.125
    shapes = dict(g_b2x=Wx_, g_w3=Wx_, g_b3=1, g_b2m=M_, g_wa=M_, g_ba=1)
    sums = {k: torch.full((v,), init, device=dev) for k, v in shapes.items()}
    dv = lambda t: t.to(dev)
    keep = [dv(t) for t in (gsx, gsm, b2x, w3, b3, b2m, wa, ba)]
    lib.check(L.egcl_backward_heads(lib.stream_ptr(), PREC, n, Wx_, M_, _P(c, dstd), _P(c, srcd), _P(c, c.xd), _P(c, keep[0]), _P(c, keep[1]),
                                    _P(c, ax), _P(c, am), *[_P(c, t) for t in keep[2:]], _P(c, g_diff),
                                    *[_P(c, sums[s_]) for s_ in ("g_b2x", "g_w3", "g_b3", "g_b2m", "g_wa", "g_ba")]))
    torch.cuda.synchronize()
    assert bool((ax[n].float() == SENT).all()) and bool((am[n].float() == SENT).all()) and bool((g_diff[n] == SENT).all())
    tx_m, tm_m = R.f32(R.d(a2x) + R.d(b2x)), R.f32(R.d(a2m) + R.d(b2m))       # backward.hip:223,249 a + b in fp32
    tx_e, tm_e = R.d(a2x) + R.d(b2x), R.d(a2m) + R.d(b2m)
    sx = R.act(tx_m)[0]
    s_e = (R.d(w3) * sx).sum(1) + R.d(b3)[0]
    abs_se = (R.d(w3) * sx).abs().sum(1) + R.d(b3)[0].abs()
    om = R.heads(tx_m, tm_m, diff_m, dst, gsx, gsm, s_e, w3, wa, ba)
    oe = R.heads(tx_e, tm_e, diff_e, dst, gsx, gsm, (R.d(w3) * R.act(tx_e)[0]).sum(1) + R.d(b3)[0], w3, wa, ba)
    dtx, dtm = E24 * tx_m.abs() / LN2, E24 * tm_m.abs() / LN2      # (the helper takes uncertainties of SCALED pre-activations)
    u = _heads_unc(om, n, dtx, dtm)
    own = 0.0 if is_bf else 1.0     # fp32 storage: the output's own rounding
    px, pm = _heads_plain(om, tx_m, tm_m, False, 4, M_ + 4)
    rep.check("g_a2x", ax[:n], om.g_a2x, u.g_a2x + own * E24 * om.g_a2x.abs(), is_bf, oe.g_a2x, None, px)
    rep.check("g_a2m", am[:n], om.g_a2m, u.g_a2m + own * E24 * om.g_a2m.abs(), is_bf, oe.g_a2m, None, pm)
    rep.check("g_diff", g_diff[:n], om.g_diff, om.gx.abs() * ((Wx_ + 10 + OPS) * E24 * abs_se)[:, None], False, oe.g_diff, None,
              om.gx.abs() * (Wx_ * E24 * abs_se)[:, None])
    for s_ in sums:
        want, unc = getattr(om, s_) + init, u.sums[s_] + (n + 64) * E24 * init
        rep.check(s_, sums[s_].reshape(want.shape), want, unc, False, getattr(oe, s_) + init, None, n * E24 * (getattr(om, "abs_" + s_) + init))
    rep.done()


@pytest.mark.parametrize("widths", [(36, 256, 256), (36, 512, 256)], ids=["Wx256", "Wx512"])
def test_store_staging_of_narrow_coordinate_kernels_regression(widths):
    """Regression, named defect: the 32x32x16 coordinate kernel (edge_bf16_v3.hip) stages its row-major bf16 stores in 36,864 bytes
    of LDS but was given 2 x 16,512 + 4 Wx bytes, which covers them only at Wx = 1024.  At Wx = 256 / 512 the last wave's rows
    14.. / 20.. of every 32-row block lay beyond the allocation and columns Wx - 32 .. Wx - 1 of those rows were stored as ZERO: in
    the kept t2x of the training forward (Wx = 256) and in dL/da2x of egcl_backward_edge_recompute (Wx = 256 and 512).  No end-to-end
    test ran bf16 training at these widths."""
    c = _case(*widths, "fully_connected")
    E, dev, Wx = c.E, c.dev, c.Wx
    gsx, gsm = _upstream(c)
    s1x, s1m = torch.empty(E, Wx, dtype=bf, device=dev), torch.empty(E, c.Wm, dtype=bf, device=dev)
    gax, gam = torch.zeros(E, Wx, dtype=bf, device=dev), torch.zeros(E, M, dtype=bf, device=dev)
    g_diff, sums = torch.empty(E, 3, device=dev), _sum_bufs(c, 0.0)
    _table(c)
    c.lib.check(c.L.egcl_backward_edge_recompute(c.ctx.handle, c.lib.stream_ptr(), 0, _P(c, c.xd), _P(c, gsx.to(dev)), _P(c, gsm.to(dev)), 0, E,
                                                 _P(c, s1x), _P(c, s1m), _P(c, gax), _P(c, gam), _P(c, g_diff),
                                                 *[_P(c, sums[s]) for s in ("g_b2x", "g_w3", "g_b3", "g_b2m", "g_wa", "g_ba")]))
    torch.cuda.synchronize()
    tail_rows = (torch.arange(E) % 32) >= 14
    outs = {"dL/da2x (recompute)": gax.cpu()}
    if Wx == 256:
        outs["kept t2x (training forward)"] = _kept(c).cpu.t2x[:E]
    for name, t in outs.items():
        blk = t[tail_rows][:, Wx - 32:].float()
        assert float((blk == 0).double().mean()) < 0.01, (name, "the last 32 columns of rows 14..31 of the 32-row blocks are zero")

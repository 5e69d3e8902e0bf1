"""Every forward stage of one EGCL layer ALONE against its float64 restatement (tests/_fwd_ref.py, proven against the float64
oracle by tests/test_fwd_ref_cpu.py), in every precision, on irregular CSR batches built for the tile height the library selects
and on the fully connected batch of the backward stage tests.  The layer is cut where the C ABI cuts it:

  edge pass    egcl_forward_begin + egcl_read_aggregates: EVERY element of sum_m [N, M] and sum_x [N, 3] (isolated nodes must read
               exactly 0) and every sum of d^2, against the edge_pass of the precision's rounding model and the exact one;
  node update  egcl_forward_end on the same context against node_update of the aggregates READ BACK from the device (the reference
               starts from the device's own values: the node kernels are judged alone), once with the context's own sums of d^2
               and once with caller-supplied ones (the device's times 4, exact): x_out must follow the supplied value;
  layers       egnn_forward over L layers (deferred hidden-split finish, fused into the next node_pre for H <= 48, in-kernel
               normaliser) against the same layers chained through egcl_forward: bitwise.

Per output three ratios |error| / bound (worst element) are printed as `fwd-stage-ratio <stage> <case> <name> plain .. model .. exact ..`
(kept in profiles/fwd_stage_errors.txt), built as tests/test_gpu_bwd_stages.py builds them:
 0. plain  (recorded): K 2^-24 sum|terms| of the element's own reduction;
 1. model  (asserted <= 1, element-wise, against the rounding model): acc + prop.  acc = K 2^-24 sum|terms| of every fp32
    accumulation on the way (table product, second-layer product, heads, segment sums and tile partials with their own term counts)
    and OPS 2^-24 per element-wise chain; prop = one spacing of each documented operand rounding whose operand the test cannot read
    back and which may therefore flip between device and model (fp16 table entries and their fp16 sum, the activation operand of
    the second-layer product in the precision's format, the hidden operand of the node MLP).  _fwd_ref.edge_bounds / node_bounds.
 2. exact  (asserted <= 1, norm-wise per node row, against the exact restatement): 2 x the model's own error + the norm of acc
    alone -- prop is not allowed here, so an undocumented rounding shows even if someone modelled it.
    The sums of d^2 have bar 1 only (the model rounds nothing there but the fp32 coordinate differences).
Nothing is fitted to the device's output; FACTOR (stage -> factor on bar 1) starts empty and an entry needs its cause by file:line.
The parameters are chosen from the library's own selection rules (egnn_forward.hip plan_edge / small_tiles / launch_layer_end,
node_bf16.hip launch_node_post_bf16; restated in _expect, which also picks the rounding model and the term counts) so that every
forward kernel instantiation runs at least once: profiles/fwd_stage_kernels.txt is a kernel trace of this file and names the
instantiations that do not appear in it (the persistent coordinate kernel, one node kernel that cannot be launched).  Three value-only mutations of csrc/ each turn tests of this file red (same record)."""
import functools

import pytest
import torch

import diffusion_model_amd as dma
from tests import _bwd_ref as R
from tests import _fwd_ref as F
from tests._util import dims_for

pytestmark = pytest.mark.gpu

SIZES = (64, 1, 33, 2, 17, 50)            # the fully connected batch of tests/test_gpu_bwd_stages.py: old and new tests share a shape
E24 = R.EPS32
D = torch.float64
FACTOR = {}                               # stage -> factor on bar 1 with its cause and measurement (none needed: profiles/fwd_stage_errors.txt)
PAD_ATOMS = 1920                          # "R32big": one more edgeless graph; N > 2047 selects node_pre_hilo_kernel<8>, N > 1024 no hidden split


def _pad256(w):
    k = 1
    while k < (w + 255) // 256:
        k *= 2
    return 256 * k


def _expect(prec, Wx, Wm, Mo, H, Wh, N, E):
    """the library's selection rules restated: tile height, column-split copies of sum_x, node-kernel form, hidden split"""
    WxP, WmP, MP = _pad256(Wx), _pad256(Wm), _pad256(Mo)
    ok3 = WxP in (256, 512, 1024) and MP == 256
    ok2 = WxP in (512, 1024) and MP == 256
    tiled = {"fp32": False, "bf16g": False, "bf16": ok3, "bf16x3": ok3, "fp16": ok2, "f16c8": ok2}[prec]   # *_supported of the edge kernels
    half = tiled and prec in ("bf16", "fp16")
    R_, nsplit = (128, 1) if tiled else (64, 1)
    if tiled:
        nsplit = WxP // 256 if prec == "bf16x3" else max(WxP // 512, 1)
    if half and ok2:                                                                          # egnn_forward.hip: small_tiles
        R_ = 32 if E <= 2048 else (64 if E <= 6144 else 128)
    K1 = H + MP
    if tiled and prec != "bf16" and H <= 64 and F.SPLIT_K // 2 < K1 <= F.SPLIT_K:             # node_post_split_supported
        form = "split"
    elif prec == "bf16" and (K1 + 15) // 16 * 16 <= 320:                                      # node_post_bf16_supported (kMaxKS1 = 20)
        form = "bf16"
    else:
        form = "fp32"
    WhP = (Wh + 127) // 128 * 128
    hs = 8 if form != "fp32" and N <= 1024 and (WhP // 32) % 32 == 0 else 1                   # launch_node_post_bf16, node_bf16.hip:447-448
    return R.NS(R=R_, nsplit=nsplit, form=form, hs=hs, tiled=tiled, K1=K1)


class _Report:
    def __init__(self, stage, case):
        self.stage, self.case, self.fail = stage, case, []

    def check(self, name, got, want, unc, exact=None, plain=None):
        """unc = [2, ...]: (acc, acc + prop).  Bar 1 element-wise against `want` (the rounding model) with unc[1]; bar 2 norm-wise per
        row against `exact` with 2 x the model's own error + |unc[0]|; the ratio against the plain bound is recorded"""
        got = R.d(got)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert bool(torch.isfinite(got).all()), (self.stage, self.case, name, "non-finite")
        r1 = R.worst_ratio(got, want, unc[1])
        r0 = float("nan") if plain is None else R.worst_ratio(got, want, plain)
        r2 = float("nan")
        if exact is not None:
            nrm = (lambda t: t.norm(dim=1)) if got.dim() == 2 else (lambda t: t.norm())
            e_dev, e_mod, flo = nrm(got - exact), nrm(want - exact), nrm(unc[0].expand_as(got))
            lim = 2.0 * e_mod + flo
            r2 = float(torch.where(e_dev == 0, torch.zeros_like(e_dev), e_dev / lim.clamp_min(1e-300)).max())
        print(f"fwd-stage-ratio {self.stage:<11s} {self.case:<46s} {name:<8s} plain {r0:9.3f}  model {r1:8.3f}  exact {r2:8.3f}")
        if not r1 <= FACTOR.get(self.stage, 1.0):
            self.fail.append((name, "rounding model", r1))
        if exact is not None and not r2 <= 1.0:
            self.fail.append((name, "2 x model error against exact", r2))

    def same(self, name, got, want):
        if not torch.equal(got, want):
            self.fail.append((name, "not bitwise equal", int((got != want).sum())))

    def done(self):
        assert not self.fail, (self.stage, self.case, self.fail)


# ---- graphs, networks, inputs: built once ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph(name):
    """CPU record + device plan; the irregular batches are checked for every CSR feature BEFORE anything is launched on them"""
    if name == "fc":
        b = F.fully_connected_batch(SIZES)
        assert b.E == 7812 and b.E % 64 != 0
    else:
        R_ = int(name[1:].replace("big", ""))
        b = F.irregular_batch(R_)
        if name.endswith("big"):
            b = R.NS(**vars(b))
            b.sizes, b.B, b.N = b.sizes + [PAD_ATOMS], b.B + 1, b.N + PAD_ATOMS
            b.row_ptr = torch.cat((b.row_ptr, b.row_ptr[-1:].expand(PAD_ATOMS)))
            b.graph_ptr = torch.cat((b.graph_ptr, torch.tensor([b.N])))
            b.node_graph = torch.cat((b.node_graph, torch.full((PAD_ATOMS,), b.B - 1)))
        b.features = F.assert_features(b, R_)
    dev = torch.device("cuda")
    b.plan = dma.GraphPlan(torch.stack((b.dst, b.src)).to(dev), b.N, sizes=b.sizes)
    assert torch.equal(b.plan.row_ptr.cpu().long(), b.row_ptr) and torch.equal(b.plan.edge_src.cpu().long(), b.src)
    b.deg = (b.row_ptr[1:] - b.row_ptr[:-1]).to(D)
    b.iso = b.deg == 0
    b.name = name
    return b


@functools.lru_cache(maxsize=None)
def _net(L, H, Wx, Wm, Mo, Wh):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(31)
        net = dma.EquivariantGNN(L, **dims_for(H, Mo, Wm, Wx, Wh))
    with torch.no_grad():   # pre-activations on both sides of SiLU's knee
        for lay in net.egcl_list:
            lay.mlp_x[2].weight *= 3.0
            lay.mlp_m[2].weight *= 3.0
    net.params = [{k: v.detach().clone() for k, v in lay.state_dict().items()} for lay in net.egcl_list]
    return net.to("cuda")


@functools.lru_cache(maxsize=None)
def _inputs(graph, H):
    b = _graph(graph)
    g = torch.Generator().manual_seed(17)
    h, x = torch.randn(b.N, H, generator=g), torch.randn(b.N, 3, generator=g) * 1.5
    return h, x, h.cuda(), x.cuda()


def _bind(net, b):
    """the network's context with graph b set.  A context that has once seen N > 1024 never splits the hidden units again
    (egnn_forward.hip: reserve allocates h_partial only then), so a network is used EITHER with batches above 1024 nodes OR below: the
    hidden split _expect predicts then does not depend on the order of the tests"""
    from diffusion_model_amd.egnn import _context
    big = b.N > 1024
    assert getattr(net, "big_batches", big) == big, "one network, batches on both sides of N = 1024"
    net.big_batches = big
    ctx = _context(net, list(net.egcl_list), torch.device("cuda"))
    ctx.set_graph(b.plan)
    ctx.pack(list(net.egcl_list))
    return ctx


# ---- float64 references: once per (widths, graph) and precision, shared by both scopes and both stages ----------------------------
def _tile_count(b, R_):
    rp = b.row_ptr
    return torch.where(b.deg > 0, (rp[1:] - 1).clamp_min(0) // R_ - rp[:-1] // R_ + 1, torch.zeros_like(rp[1:])).to(D)


@functools.lru_cache(maxsize=None)
def _edge_ref(H, Wx, Wm, Mo, Wh, graph, prec):
    """compact record of edge_pass: exact (prec None) or the precision's model with its bounds; per-graph sums of d^2 (the call's
    sum is their sum).  (Wh is part of the key because the network's attention weights are drawn after mlp_h's.)"""
    b = _graph(graph)
    p = _net(1, H, Wx, Wm, Mo, Wh).params[0]
    h, x, _, _ = _inputs(graph, H)
    args = (p, H, h, x, b.dst, b.src, b.node_graph, b.N, b.B, "graph")
    if prec is None:
        o = F.edge_pass(*args)
        return R.NS(sum_m=o.sum_m, sum_x=o.sum_x, sq=o.sq)
    o = F.edge_pass(*args, prec, True)
    ex = _expect(prec, Wx, Wm, Mo, H, Wh, b.N, b.E)
    u = F.edge_bounds(o, H, b.dst, b.src, b.N, b.deg, ex.nsplit)
    return R.NS(sum_m=o.sum_m, sum_x=o.sum_x, sq=o.sq, abs_sum_m=o.abs_sum_m, abs_sum_x=o.abs_sum_x, u_m=u.sum_m, u_x=u.sum_x)


# ---- cases -------------------------------------------------------------------------------------------------------------------------
# (precision, Wx, Wm, Wh, H, graph, norm scope[, M]); what each row adds is named on it.  Tile heights: bf16 / fp16 at hidden width
# 512 / 1024 take 32- / 64- / 128-edge tiles at E <= 2048 / <= 6144 / above (R32: 1,079, R64: 3,290, R128: 7,887, fc: 7,812 edges),
# bf16 at 256 and bf16x3 / f16c8 always 128, the generic kernel 64.  Wh = 1024 with N <= 1024: 8-way hidden split + finish launch.
CASES = [
    ("bf16", 1024, 1024, 1024, 36, "R128", "graph"),     # edge_x_m16<bf16> two shares + v4 message; hilo node_pre; hidden-split node_post
    ("bf16", 1024, 1024, 1024, 36, "fc", "call"),        # the shared fully connected shape
    ("bf16", 512, 256, 256, 63, "R128", "call"),         # one 512-column share; node_pre_mfma<fp16>; single-pass bf16 node_post
    ("bf16", 256, 256, 1024, 3, "R128", "graph"),        # edge_bf16_v3 coordinate kernel; H = 3
    ("bf16", 256, 256, 256, 36, "fc", "graph"),
    ("bf16", 512, 192, 1024, 80, "R128", "graph"),       # Wm no multiple of 128 (padded); H = 80: plain node_pre_kernel<fp16>, fp32 node_post
    ("bf16", 1024, 1024, 1024, 36, "R32", "graph"),      # 32-edge tiles
    ("bf16", 512, 256, 256, 36, "R64", "call"),          # 64-edge tiles
    ("bf16", 512, 256, 1024, 63, "R32", "call"),
    ("bf16", 1024, 1024, 256, 3, "R64", "graph"),
    ("bf16", 22, 30, 256, 36, "R128", "graph", 10),      # widths padded to 256: the tiled kernels with zero columns
    ("bf16", 256, 256, 256, 36, "R64", "graph", 300),    # M > 256 (MP = 512): outside every tiling, the generic edge_kernel<BF16> on
                                                         # 64-edge tiles, 4 message column blocks per wave; K1 = 548: fp32 node_post
    ("bf16", 512, 256, 1024, 63, "R64", "call", 300),    # the same kernel with 4 coordinate column blocks, 'call' scope
    ("bf16", 1024, 1024, 1024, 40, "R32big", "graph"),   # N = 2,052: node_pre_hilo_kernel<8>; single-pass node_post at Wh = 1024
                                                         # (a network of its own: a context that has seen N > 1024 drops the hidden split)
    ("fp16", 1024, 1024, 1024, 36, "R128", "graph"),     # edge_x_m16<f16> + v4 message on fp16; split-operand hidden-split node_post
    ("fp16", 512, 256, 256, 63, "R128", "call"),         # split-operand single pass
    ("fp16", 512, 256, 1024, 3, "fc", "graph"),
    ("fp16", 1024, 1024, 256, 36, "R32", "call"),        # 32-edge tiles, fp16
    ("fp16", 512, 192, 1024, 36, "R64", "graph"),        # 64-edge tiles, fp16
    ("fp16", 512, 256, 256, 80, "R32", "graph"),         # H = 80: fp32 node_post behind a half-precision edge pass
    ("fp16", 1024, 1024, 1024, 63, "R64", "graph"),
    ("fp16", 256, 256, 256, 36, "R64", "graph"),         # outside the fp16 tiling: runs as fp32 (generic kernel, 64-edge tiles)
    ("bf16x3", 1024, 1024, 1024, 36, "R128", "graph"),
    ("bf16x3", 512, 256, 256, 63, "R128", "call"),
    ("bf16x3", 256, 256, 1024, 3, "R128", "graph"),
    ("bf16x3", 512, 192, 256, 80, "fc", "call"),         # plain node_pre_kernel<float>
    ("f16c8", 1024, 1024, 1024, 36, "R128", "graph"),
    ("f16c8", 512, 256, 256, 63, "R128", "call"),
    ("f16c8", 512, 192, 1024, 3, "fc", "graph"),
    ("fp32", 256, 256, 256, 36, "R64", "graph"),         # generic edge_kernel<F32>, 2 / 4 / 8 column blocks per wave
    ("fp32", 512, 256, 1024, 63, "R64", "call"),
    ("fp32", 1024, 1024, 256, 80, "R64", "graph"),
    ("fp32", 22, 30, 256, 3, "R64", "call", 10),         # nothing aligned
    ("fp32", 256, 256, 1024, 36, "fc", "call"),
]
CASE_IDS = ["-".join(str(v) for v in (c[0], f"Wx{c[1]}", f"Wm{c[2]}", f"Wh{c[3]}", f"H{c[4]}", c[5], c[6]) + c[7:]) for c in CASES]


@functools.lru_cache(maxsize=None)
def _run(case):
    """the device side of one case, once: begin, read_aggregates, end, end with supplied sums, and the one-call layer"""
    from diffusion_model_amd import _lib
    prec, Wx, Wm, Wh, H, graph, scope = case[:7]
    Mo = case[7] if len(case) > 7 else 256
    b = _graph(graph)
    net = _net(1, H, Wx, Wm, Mo, Wh)
    ctx = _bind(net, b)
    _, _, hd, xd = _inputs(graph, H)
    L, P, st, dev = _lib.lib(), _lib.ptr, _lib.stream_ptr, hd.device
    pr, sc = _lib.PRECISIONS[prec], _lib.NORM_SCOPES[scope]
    nsq = b.B if scope == "graph" else 1
    o = R.NS(b=b, Mo=Mo, p=net.params[0], ex=_expect(prec, Wx, Wm, Mo, H, Wh, b.N, b.E))
    new = lambda *s: torch.empty(*s, device=dev)
    sq_b, sm, sx, sq_r = new(nsq), new(b.N, Mo), new(b.N, 3), new(nsq)
    _lib.check(L.egcl_forward_begin(ctx.handle, st(), 0, pr, sc, P(hd), P(xd), P(sq_b)))
    _lib.check(L.egcl_read_aggregates(ctx.handle, st(), sc, P(sm), P(sx), P(sq_r)))
    ho, xo, ho4, xo4, ho1, xo1 = new(b.N, H), new(b.N, 3), new(b.N, H), new(b.N, 3), new(b.N, H), new(b.N, 3)
    _lib.check(L.egcl_forward_end(ctx.handle, st(), 0, pr, sc, P(hd), P(xd), None, P(ho), P(xo)))
    sq4 = sq_r * 4.0
    _lib.check(L.egcl_forward_end(ctx.handle, st(), 0, pr, sc, P(hd), P(xd), P(sq4), P(ho4), P(xo4)))
    _lib.check(L.egcl_forward(ctx.handle, st(), 0, pr, sc, P(hd), P(xd), P(ho1), P(xo1)))
    torch.cuda.synchronize()
    for k, v in dict(sq_b=sq_b, sm=sm, sx=sx, sq_r=sq_r, ho=ho, xo=xo, ho4=ho4, xo4=xo4, ho1=ho1, xo1=xo1).items():
        setattr(o, k, v.cpu())
    return o


def _refs(case):
    prec, Wx, Wm, Wh, H, graph, scope = case[:7]
    Mo = case[7] if len(case) > 7 else 256
    b = _graph(graph)
    ex = _expect(prec, Wx, Wm, Mo, H, Wh, b.N, b.E)
    # a precision outside its tiling runs the generic kernel: bf16 as bf16, the others as the exact fp32 path (host_logic.cpp: plan_forward)
    ran = prec if ex.tiled else ("bf16g" if prec == "bf16" else "fp32")
    return _edge_ref(H, Wx, Wm, Mo, Wh, graph, ran), _edge_ref(H, Wx, Wm, Mo, Wh, graph, None), ex


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_edge_pass(case):
    """egcl_forward_begin + egcl_read_aggregates: sum_m, sum_x (every node, every element) and the sums of d^2"""
    graph, scope = case[5], case[6]
    b = _graph(graph)
    mo, exa, ex = _refs(case)
    if graph != "fc":        # the CSR features were asserted for the tile height this case runs on
        assert ex.R == int(graph[1:].replace("big", "")), (case, ex.R, "the batch was built for another tile height than the library selects")
    o = _run(case)
    rep = _Report("edge_pass", CASE_IDS[CASES.index(case)])
    rep.same("sq begin/read", o.sq_b, o.sq_r)
    assert bool((o.sm[b.iso] == 0).all()) and bool((o.sx[b.iso] == 0).all()), "isolated nodes must read exactly 0"
    K = (b.deg + 8.0)[:, None] * E24
    rep.check("sum_m", o.sm, mo.sum_m, mo.u_m, exa.sum_m, K * mo.abs_sum_m)
    rep.check("sum_x", o.sx, mo.sum_x, mo.u_x, exa.sum_x, K * mo.abs_sum_x)
    # sums of d^2: five roundings per edge, then the segment sum (<= 128 terms), the node's tile partials, the graph's nodes
    gn = torch.tensor(b.sizes, dtype=D)
    depth = max(128.0, float(b.deg.max())) + float(_tile_count(b, ex.R).max()) + 16.0
    if scope == "graph":
        want, usq = mo.sq, (depth + gn) * E24 * mo.sq
    else:
        want, usq = mo.sq.sum().reshape(1), (depth + b.N) * E24 * mo.sq.sum().reshape(1)
    rep.check("sq", o.sq_r, want, torch.stack((usq, usq)))
    assert bool((o.sq_r[(want == 0)] == 0).all()), "a graph without edges has the normaliser 1 / (0 + 1)"
    rep.done()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_node_update(case):
    """egcl_forward_end from the device's own aggregates: h_out and x_out; x_out with caller-supplied sums of d^2 (times 4);
    egcl_forward in one call gives the same bits as begin + end"""
    prec, Wx, Wm, Wh, H, graph, scope = case[:7]
    b = _graph(graph)
    mo, _, ex = _refs(case)
    o = _run(case)
    h, x, _, _ = _inputs(graph, H)
    rep = _Report("node_update", CASE_IDS[CASES.index(case)])
    nt = _tile_count(b, ex.R)
    for tag, sq, ho, xo in (("", o.sq_r, o.ho, o.xo), ("4sq", o.sq_r * 4.0, o.ho4, o.xo4)):
        nm = F.node_update(o.p, H, h, x, o.sm, o.sx, sq, b.node_graph, scope, ex.form, True)
        ne = F.node_update(o.p, H, h, x, o.sm, o.sx, sq, b.node_graph, scope)
        u = F.node_bounds(nm, ex.K1, Wh, ex.hs, o.sx, mo.abs_sum_x, nt, ex.nsplit)
        if not tag:
            rep.check("h_out", ho, nm.h_out, u.h_out, ne.h_out, (Wh + 8) * E24 * nm.abs_out)
        else:
            rep.same("h_out 4sq", ho, o.ho)
        rep.check("x_out" + tag, xo, nm.x_out, u.x_out, ne.x_out, 8 * E24 * (R.d(x).abs() + (R.d(o.sx) * nm.gn).abs()))
    assert bool((o.xo4 != o.xo)[~b.iso].any()), "x_out must follow the supplied sums"
    assert torch.equal(o.xo[b.iso], x[b.iso]) and torch.equal(o.xo4[b.iso], x[b.iso]), "a node without edges keeps its coordinates"
    rep.same("h_out one call", o.ho1, o.ho)
    rep.same("x_out one call", o.xo1, o.xo)
    rep.done()


# ---- several layers against one -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scope", ["call", "graph"])
@pytest.mark.parametrize("L,H", [(1, 36), (2, 36), (3, 36), (2, 63), (3, 63)])
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_layers_of_egnn_forward_equal_chained_single_layers(prec, L, H, scope):
    """egnn_forward defers the hidden-split finish of a layer (Wh = 1024, N <= 1024) to the next layer's begin -- fused into the
    half-precision node_pre for H <= 48 (egnn_forward.hip: node_pre_hilo_kernel, launch_layer_begin: "adds them up in split order", what
    node_post_finish_kernel does), a launch of node_post_finish_kernel for H = 63 -- and, in 'graph' scope, leaves the normaliser to
    node_post (sq_from_agg, egnn_forward.hip: launch_layer_begin).  Against the same layers chained through egcl_forward:
      * h: bitwise, every node, in 'call' scope and after ONE layer in 'graph' scope;
      * x: bitwise where both paths add the d^2 sums in the same order: 'call' scope (both launch graph_sq_sums_kernel), graphs of
        more than 64 nodes (node_bf16.hip:222-236 repeats graph_sq_sums_kernel's strided loop and tree, egnn_forward.hip: graph_sq_sums_kernel)
        and graphs without edges.  Graphs of <= 64 nodes go through graph_sq_sum8 (kernels.h:89-118: 8 lanes x 8 nodes, then a
        3-step butterfly), another association of the same terms: after one layer x agrees within (terms 2^-24 sum d^2) taken
        through 1 / (sqrt(.) + 1); from the second layer on such a graph's h and x inherit that difference through d^2, so only the
        first two classes are held to bitwise there (the third is reported: the ABI does not expose the per-node d^2 sums from
        which graph_sq_sum8's value could be restated, and a difference carried through a further layer has no bound that is
        derived rather than measured)."""
    assert _expect(prec, 512, 256, 256, H, 1024, 132, 1079).hs == 8
    _layers(prec, L, H, scope, 512, 256, 1024, "R32")


@pytest.mark.parametrize("prec,Wh,H", [("bf16", 256, 36), ("fp16", 256, 36), ("bf16", 1024, 36), ("bf16", 256, 80), ("bf16x3", 256, 63)],
                         ids=["bf16-single-pass", "split-single-pass", "bf16-hidden-split", "fp32-node-kernel", "bf16x3-split"])
def test_in_kernel_normaliser_on_128_edge_tiles(prec, Wh, H):
    """the single-layer C ABI always asks for the d^2 sums (egnn_forward.hip: egcl_forward, egcl_forward_begin), so only egnn_forward in 'graph' scope leaves
    them to node_post (sq_from_agg): here one layer on the R = 128 irregular batch (a node whose d^2 partials span three tiles, graphs
    above and below 64 nodes, graphs without edges) through the single-pass bf16 and split-operand node kernels, the hidden-split
    form, and the fp32 node kernel, for which launch_layer_end launches graph_sq_sums_kernel after all (egnn_forward.hip: launch_layer_end:
    x bitwise on every node)"""
    ex = _expect(prec, 512, 256, 256, H, Wh, 458, 7887)
    assert (ex.form, ex.hs, ex.R) == {("bf16", 256, 36): ("bf16", 1, 128), ("fp16", 256, 36): ("split", 1, 128), ("bf16", 1024, 36): ("bf16", 8, 128),
                                      ("bf16", 256, 80): ("fp32", 1, 128), ("bf16x3", 256, 63): ("split", 1, 128)}[(prec, Wh, H)]
    _layers(prec, 1, H, "graph", 512, 256, Wh, "R128")


def _layers(prec, L, H, scope, Wx, Wm, Wh, graph):
    from diffusion_model_amd import _lib
    b = _graph(graph)
    net = _net(L, H, Wx, Wm, 256, Wh)
    ctx = _bind(net, b)
    _, x, hd, xd = _inputs(graph, H)
    Lb, P, st = _lib.lib(), _lib.ptr, _lib.stream_ptr
    pr, sc = _lib.PRECISIONS[prec], _lib.NORM_SCOPES[scope]
    in_kernel = scope == "graph" and _expect(prec, Wx, Wm, 256, H, Wh, b.N, b.E).form != "fp32"
    hc, xc, keep = hd, xd, []
    for l in range(L):
        ho, xo = torch.empty_like(hd), torch.empty_like(xd)
        _lib.check(Lb.egcl_forward(ctx.handle, st(), l, pr, sc, P(hc), P(xc), P(ho), P(xo)))
        keep.append((hc, xc))
        hc, xc = ho, xo
    nsq = b.B if scope == "graph" else 1
    sm, sx, sq = torch.empty(b.N, 256, device=hd.device), torch.empty(b.N, 3, device=hd.device), torch.empty(nsq, device=hd.device)
    _lib.check(Lb.egcl_read_aggregates(ctx.handle, st(), sc, P(sm), P(sx), P(sq)))      # (of the chain's last layer)
    hw, xw = torch.empty_like(hd), torch.empty_like(xd)
    _lib.check(Lb.egnn_forward(ctx.handle, st(), pr, sc, P(hd), P(xd), P(hw), P(xw)))
    torch.cuda.synchronize()
    hc, xc, hw, xw = hc.cpu(), xc.cpu(), hw.cpu(), xw.cpu()
    assert bool(torch.isfinite(hw).all()) and bool(torch.isfinite(xw).all())
    gsz = torch.tensor(b.sizes)
    gdeg = torch.zeros(b.B, dtype=D).index_add_(0, b.node_graph, b.deg)
    same_order = ((gsz > 64) | (gdeg == 0))[b.node_graph] if in_kernel else torch.ones(b.N, dtype=torch.bool)
    assert bool(same_order.any()) and (not in_kernel or bool((~same_order).any()))
    dh, dx = (hw != hc).any(1), (xw != xc).any(1)
    print(f"fwd-stage-layers {prec} L{L} H{H} Wh{Wh} {graph} {scope}: nodes with other bits h {int(dh.sum())} x {int(dx.sum())} "
          f"(outside the same-order classes: h {int((dh & ~same_order).sum())} x {int((dx & ~same_order).sum())}; "
          f"max |dx| {float((xw - xc).abs().max()):.3e})")
    assert not bool((dh & same_order).any()), "h differs where both paths add in the same order"
    assert not bool((dx & same_order).any()), "x differs where both paths add in the same order"
    if L == 1:
        assert not bool(dh.any()), "h after one layer does not depend on the normaliser"
        if in_kernel:
            s = R.d(sq.cpu())[b.node_graph][:, None]
            g = 1.0 / (torch.sqrt(s) + 1.0)
            terms = gsz.to(D)[b.node_graph][:, None] + 8.0
            ds = 2.0 * terms * E24 * s
            bound = R.d(sx.cpu()).abs() * g * g * ds / (2.0 * torch.sqrt(s).clamp_min(1e-30)) + 4 * E24 * R.d(xc).abs()
            r = R.worst_ratio(xw, R.d(xc), bound)
            print(f"fwd-stage-ratio layers      {prec}-L1-H{H}-Wh{Wh}-{graph}-graph x_out   plain       nan  model {r:8.3f}  exact      nan")
            assert r <= 1.0, ("x after one layer, graphs of <= 64 nodes", r)


def test_case_list_reaches_every_node_form_and_tile_height():
    """by the selection rules restated in _expect, the case list runs the hidden-split and the single-pass launch of the bf16 and
    of the split-operand node kernel, the fp32 node kernel, 32- / 64- / 128-edge tiles and the generic edge kernel"""
    forms = set()
    for c in CASES:
        Mo = c[7] if len(c) > 7 else 256
        b = _graph(c[5])
        ex = _expect(c[0], c[1], c[2], Mo, c[4], c[3], b.N, b.E)
        forms.add((ex.form, ex.hs, ex.R, ex.tiled))
    for want in [("bf16", 8), ("bf16", 1), ("split", 8), ("split", 1), ("fp32", 1)]:
        assert any(f[:2] == want for f in forms), want
    for R_ in (32, 64, 128):
        assert any(f[2] == R_ and f[3] for f in forms), R_
    assert any(not f[3] for f in forms)


# ---- the packed parameters' arena: re-pack in place, release and re-carve ------------------------------------------------------------
# name -> (H, Wx, Wm, Wh, M, atoms per graph), two fully connected graphs each.  By the selection rules restated in _expect:
#   tiled    the smallest shape on which every precision but fp32 runs its 128-edge-tile kernels (2 x 64 x 63 = 8,064 edges is
#            beyond the 64-edge small-tile limit of 6,144);
#   padded   the padded widths of the goldens (WxP = 512, WmP = MP = 256, WhP = 256): fp32 on the generic kernel, bf16 / fp16 on
#            32-edge tiles, bf16x3 / f16c8 on 128-edge tiles, every one with zero columns;
#   generic  M = 300 (MP = 512) is outside every tiling: the generic kernel on its bf16 streams (bf16) and its fp32 ones (the rest).
PACK_SHAPES = {"tiled": (36, 512, 256, 256, 256, 64), "padded": (3, 300, 7, 130, 5, 8), "generic": (36, 256, 256, 256, 300, 8)}


@functools.lru_cache(maxsize=None)
def _pack_graph(shape):
    H, atoms = PACK_SHAPES[shape][0], PACK_SHAPES[shape][5]
    b = F.fully_connected_batch((atoms, atoms))
    plan = dma.GraphPlan(torch.stack((b.dst, b.src)).cuda(), b.N, sizes=b.sizes)
    g = torch.Generator().manual_seed(23)
    return b, plan, torch.randn(b.N, H, generator=g).cuda(), (torch.randn(b.N, 3, generator=g) * 1.5).cuda()


def _pack_net(shape, seed):
    H, Wx, Wm, Wh, Mo, _ = PACK_SHAPES[shape]
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return dma.EquivariantGNN(2, **dims_for(H, Mo, Wm, Wx, Wh)).cuda()


def _pack_forward(ctx, net, shape, prec):
    """set_model (a no-op while the dimensions stay), set_graph, pack (a no-op while no parameter changed) and egnn_forward"""
    from diffusion_model_amd import _lib
    _, plan, hd, xd = _pack_graph(shape)
    layers = list(net.egcl_list)
    d = layers[0].dims
    ctx.set_model(len(layers), d["H"], d["M"], d["Wm"], d["Wx"], d["Wh"])
    ctx.set_graph(plan)
    ctx.pack(layers)
    ho, xo = torch.empty_like(hd), torch.empty_like(xd)
    _lib.check(_lib.lib().egnn_forward(ctx.handle, _lib.stream_ptr(), _lib.PRECISIONS[prec], _lib.NORM_GRAPH, _lib.ptr(hd), _lib.ptr(xd),
                                       _lib.ptr(ho), _lib.ptr(xo)))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ho).all()) and bool(torch.isfinite(xo).all())
    return ho.cpu(), xo.cpu()


@pytest.mark.parametrize("shape", list(PACK_SHAPES))
@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3", "fp16", "f16c8"])
def test_repacked_and_recarved_context_equals_a_fresh_one(prec, shape):
    """a layer's packed streams live in one arena (pack.hip: egnn_pack_layer, host_logic.cpp: carve_layer_pack).  A context that
    re-packs changed parameters into the arena it has, and one whose arenas were released and carved again for other dimensions
    and back (pack.hip: egnn_set_model, free_layer), must both compute, bit for bit, what a fresh context packed once computes:
    a stream the re-pack misses, or one that overlaps its neighbour after the re-carve, changes the output"""
    from diffusion_model_amd.egnn import _Context
    H, Wx, Wm, Wh, Mo, _ = PACK_SHAPES[shape]
    b = _pack_graph(shape)[0]
    ex = _expect(prec, Wx, Wm, Mo, H, Wh, b.N, b.E)
    small = 32 if prec in ("bf16", "fp16") else 128          # padded: 112 edges, the half-precision paths take 32-edge tiles
    want = {"tiled": (prec != "fp32", 128), "padded": (prec != "fp32", small), "generic": (False, 64)}[shape]
    assert (ex.tiled, ex.R) == (want[0], want[1] if want[0] else 64), (prec, shape, ex.tiled, ex.R)
    dev = torch.device("cuda")
    net, ctx = _pack_net(shape, 41), _Context(dev)
    first = _pack_forward(ctx, net, shape, prec)
    with torch.no_grad():
        for p in net.parameters():          # every parameter, in place: the version counters make pack() run again
            p.mul_(1.25).add_(0.01)
    again = _pack_forward(ctx, net, shape, prec)
    fresh = _pack_forward(_Context(dev), net, shape, prec)
    assert not torch.equal(again[0], first[0]) and not torch.equal(again[1], first[1]), "the changed parameters were not packed"
    assert torch.equal(again[0], fresh[0]) and torch.equal(again[1], fresh[1]), "re-packed context differs from a fresh one"
    other = "padded" if shape != "padded" else "tiled"
    _pack_forward(ctx, _pack_net(other, 43), other, prec)      # the arenas are released and carved for the other dimensions ...
    back = _pack_forward(ctx, net, shape, prec)                # ... and again for these
    assert torch.equal(back[0], fresh[0]) and torch.equal(back[1], fresh[1]), "re-carved context differs from a fresh one"

"""The float64 restatement of the edge backward (tests/_bwd_ref.py) is proven before it judges a kernel: its exact-mode stages,
composed into the edge part of one layer's backward, must reproduce torch.autograd over the oracle's layer in float64 -- dL/dh,
dL/dx and all twelve parameter tensors of the two edge MLPs, every element to 1e-10 of the tensor's largest entry -- for the
chain composition (gather / GEMMs over the edges / scatter) and for the factorised one (per-node sums + node-level products), in
both norm scopes, on ragged fully connected graphs and on an asymmetric edge list with an isolated node and a duplicate edge."""
import pytest
import torch

from oracle.egnn_ref import egcl_forward, fully_connected_edge_index, init_state_dict
from tests import _bwd_ref as R

H, WX, WM, M, WH = 7, 24, 16, 8, 12
TIGHT = 1e-10
EDGE_KEYS = [f"{m}.{p}" for m in ("mlp_x.0", "mlp_x.2", "mlp_x.4", "mlp_m.0", "mlp_m.2", "attention.0") for p in ("weight", "bias")]


def _graphs(kind):
    if kind == "ragged":
        sizes = (5, 1, 9, 2)
        ei = fully_connected_edge_index(list(sizes))
    else:   # node 4 is isolated, node 7 only sends, edge (1 <- 0) is listed twice; sorted by receiving node
        sizes = (5, 3)
        ei = torch.tensor([[0, 0, 1, 1, 2, 3, 5, 6, 6], [1, 2, 0, 0, 3, 1, 6, 5, 7]])
        deg = torch.bincount(ei[0], minlength=8) + torch.bincount(ei[1], minlength=8)
        assert int(deg[4]) == 0 and (ei[:, 2] == ei[:, 3]).all()
    return sizes, ei


@pytest.fixture(scope="module", params=["ragged", "asymmetric"])
def problem(request):
    sizes, ei = _graphs(request.param)
    n = sum(sizes)
    g = torch.Generator().manual_seed(21)
    sd32 = init_state_dict(1, 2 * H + 1, WM, M, 2 * H + 1, WX, 1, H + M, WH, H, seed=4)
    sd = {k: (v.double() * (3.0 if ".2.weight" in k and "mlp_h" not in k else 1.0)) for k, v in sd32.items()}
    h = torch.randn(n, H, generator=g, dtype=torch.float64)
    x = torch.randn(n, 3, generator=g, dtype=torch.float64) * 1.5
    wh, wx = torch.randn(n, H, generator=g, dtype=torch.float64), torch.randn(n, 3, generator=g, dtype=torch.float64)
    ptr = torch.tensor([0] + torch.cumsum(torch.tensor(sizes), 0).tolist())
    node_graph = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return dict(sd=sd, h=h, x=x, wh=wh, wx=wx, ptr=ptr, node_graph=node_graph, ei=ei, B=len(sizes))


def _autograd(pb, scope):
    """(total gradients of the layer by autograd, the node part's own dL/dh, the gradients of the three segment sums)"""
    sd = {k: v.clone().requires_grad_(True) for k, v in pb["sd"].items()}
    h, x = pb["h"].clone().requires_grad_(True), pb["x"].clone().requires_grad_(True)
    ho, xo, (agg_m, raw_x, sq) = egcl_forward(sd, 0, pb["ei"], h, x, scope, pb["ptr"], return_aggregates=True)
    loss = (ho * pb["wh"]).sum() + (xo * pb["wx"]).sum()
    keys = ["egcl_list.0." + k for k in EDGE_KEYS]
    outs = torch.autograd.grad(loss, [h, x, agg_m] + [sd[k] for k in keys], retain_graph=True)
    total = dict(zip(["h", "x", "agg_m"] + EDGE_KEYS, outs))
    # the node part alone, as autograd.py differentiates it: h' = mlp_h([h | sum_m]), x' = x + sum_x / (sqrt(S) + 1)
    hn = pb["h"].clone().requires_grad_(True)
    am = agg_m.detach()
    w = lambda k: pb["sd"]["egcl_list.0." + k]
    hcat = torch.cat((hn, am), 1)
    h_new = torch.nn.functional.linear(torch.nn.functional.silu(torch.nn.functional.linear(hcat, w("mlp_h.0.weight"), w("mlp_h.0.bias"))),
                                       w("mlp_h.2.weight"), w("mlp_h.2.bias"))
    g_h_node, = torch.autograd.grad((h_new * pb["wh"]).sum(), [hn])
    ax, S = raw_x.detach().clone().requires_grad_(True), sq.detach().clone().requires_grad_(True)
    c = 1.0 / (torch.sqrt(S.clamp_min(1e-300)) + 1.0)
    scale = c[pb["node_graph"]].unsqueeze(1) if scope == "graph" else c
    g_ax, g_S = torch.autograd.grad(((ax * scale) * pb["wx"]).sum(), [ax, S])
    return total, g_h_node, total["agg_m"], g_ax, g_S


@pytest.mark.parametrize("form", ["chain", "factorised"])
@pytest.mark.parametrize("scope", ["graph", "call"])
def test_exact_stages_compose_to_float64_autograd(problem, scope, form):
    pb = problem
    total, g_h_node, g_am, g_ax, g_S = _autograd(pb, scope)
    dst, src = pb["ei"][0], pb["ei"][1]
    params = {k: pb["sd"]["egcl_list.0." + k] for k in EDGE_KEYS}
    node_seg = pb["node_graph"] if scope == "graph" else None
    g_h, g_x, g = R.edge_backward(params, H, pb["h"], pb["x"], dst, src, pb["node_graph"], node_seg, pb["B"], g_am, g_ax, g_S, form)
    got = dict(g, h=g_h + g_h_node, x=g_x + pb["wx"])          # x' = x + ...: the identity path adds dL/dx' itself
    for k in ["h", "x"] + EDGE_KEYS:
        want = total[k]
        assert got[k].shape == want.shape, k
        scale = float(want.abs().max())
        assert scale > 0, k
        err = float((got[k] - want).abs().max()) / scale
        assert err <= TIGHT, (scope, form, k, err)


@pytest.mark.parametrize("scope", ["graph", "call"])
def test_chain_and_factorised_compositions_agree(problem, scope):
    pb = problem
    _, _, g_am, g_ax, g_S = _autograd(pb, scope)
    dst, src = pb["ei"][0], pb["ei"][1]
    params = {k: pb["sd"]["egcl_list.0." + k] for k in EDGE_KEYS}
    node_seg = pb["node_graph"] if scope == "graph" else None
    a = R.edge_backward(params, H, pb["h"], pb["x"], dst, src, pb["node_graph"], node_seg, pb["B"], g_am, g_ax, g_S, "chain")
    b = R.edge_backward(params, H, pb["h"], pb["x"], dst, src, pb["node_graph"], node_seg, pb["B"], g_am, g_ax, g_S, "factorised")
    for name, u, v in [("h", a[0], b[0]), ("x", a[1], b[1])] + [(k, a[2][k], b[2][k]) for k in EDGE_KEYS]:
        assert float((u - v).abs().max()) <= TIGHT * float(u.abs().max()), (scope, name)


def test_rounding_model_stays_close_to_exact_and_differs_from_it():
    """the rounding-model mode is the exact mode plus bf16 / fp16 roundings: close (1e-2 row-wise) but not equal"""
    g = torch.Generator().manual_seed(3)
    n, E = 12, 40
    h, x = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g)
    dst, src = torch.randint(0, n, (E,), generator=g).sort().values, torch.randint(0, n, (E,), generator=g)
    W1, b1 = torch.randn(WX, 2 * H + 1, generator=g) * 0.3, torch.randn(WX, generator=g) * 0.3
    W2, b2 = torch.randn(WX, WX, generator=g) * 0.3, torch.randn(WX, generator=g) * 0.3
    w3, b3 = torch.randn(WX, generator=g), torch.randn(1, generator=g)
    out = {}
    for model in (False, True):
        diff, d2 = R.geometry(x, dst, src, model)
        t = R.tables(h, W1, b1, H, model)
        out[model] = R.forward_kept(t, t, d2, dst, src, W2, b2, W2, b2, w3, b3, model)
    for k in ("s1x", "t2x", "s_e"):
        e = float(R.row_rel(getattr(out[True], k), getattr(out[False], k)).max())
        assert 0 < e <= 1e-2, (k, e)
    assert torch.equal(R.bf16(out[True].t2x), out[True].t2x) and torch.equal(R.bf16(out[True].s1x), out[True].s1x)
    assert float(R.ulp_bf16(torch.tensor([1.0, 1.5, 2.0, 0.0], dtype=torch.float64))[0]) == 2.0 ** -7

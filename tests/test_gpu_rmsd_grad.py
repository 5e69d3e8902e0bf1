"""The differentiable Kabsch fit and the RMSD loss on the device (kabsch_backward_kernel of csrc/eval/kabsch.hip through
diffusion_model_amd.stats.kabsch / rmsd_loss), against the gradients of the EXECUTED reference (kabsch_torch under torch
autograd) stored in tests/golden/rmsd_grad_golden.npz.

Bars, as fractions of the graph's largest gradient element:
  * against the float64 gradients: 1e-6.  The device result is ONE float32 rounding (6e-8) of a float64 computation on the same
    float32 inputs; 1e-6 is 16 roundings and anything above it is a defect;
  * against the float32 gradients: ref_vs_f64_grad (the reference's own float32 noise, measured by the generator: 6.9e-5) + 1e-6.
Pairs of kind 1 (n >= 4, well-conditioned) are compared in all three cotangents with the reference's spelling; the others
through the RMSD alone with flip='row', where the executed reference returned the optimal rotation and finite values.

Measured on an MI355X: against float64 5.6e-8 (37 pairs) / 3.0e-8 (4 pairs through the RMSD); against float32 6.88e-5 (the
reference's own noise); against the host statement 5.4e-8 in the worst of the four spellings; composition with the EGNN: dL/dh
4.6e-7, dL/dx 2.2e-7, parameter tensors 2.8e-7, one-element parameters 2.2e-7 (bars 1e-4).
"""
import numpy as np
import pytest
import torch

import diffusion_model_amd as dma
from diffusion_model_amd import _lib
from tests import _rmsd_grad_util as GU
from tests import _rmsd_util as RU
from tests._util import dims_for, load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR64 = 1e-6


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _device_grads(P, Q, sizes, center, flip, g_R, g_t, g_rmsd, order=None):
    """dP, dQ (float64 numpy) of sum_g <g_R, R> + <g_t, t> + g_rmsd rmsd through stats.kabsch: one launch forward, one backward"""
    P, Q = _dev(P).requires_grad_(True), _dev(Q).requires_grad_(True)
    R, t, rmsd = dma.stats.kabsch(P, Q, sizes, center=center, flip=flip)
    ((R * _dev(g_R)).sum() + (t * _dev(g_t)).sum() + (rmsd * _dev(g_rmsd)).sum()).backward()
    return P.grad.cpu().double().numpy(), Q.grad.cpu().double().numpy()


_CACHE = {}


def _fixture():
    """the golden arrays and the device gradients of the whole fixture, one ragged launch per flip, computed once"""
    if not _CACHE:
        G = load_golden("rmsd_grad_golden.npz")
        sizes = G["sizes"].tolist()
        _CACHE["G"], _CACHE["sizes"], _CACHE["cut"] = G, sizes, np.cumsum(sizes)[:-1]
        for flip in ("column", "row"):
            _CACHE[flip] = _device_grads(G["P"], G["Q"], sizes, "centroid", flip, G["g_R"], G["g_t"], G["g_rmsd"])
    return _CACHE


def _compare(ref_P, ref_Q, bar, kinds):
    F = _fixture()
    G, cut = F["G"], F["cut"]
    worst, n = 0.0, 0
    for k in range(len(F["sizes"])):
        if not (G["kind"][k] if kinds == "full" else (not G["kind"][k] and G["defined"][k])):
            continue
        dP, dQ = F["column" if G["kind"][k] else "row"]
        r = max(GU.worst_ratio(np.split(dP, cut)[k], np.split(G[ref_P], cut)[k].astype(np.float64)),
                GU.worst_ratio(np.split(dQ, cut)[k], np.split(G[ref_Q], cut)[k].astype(np.float64)))
        worst, n = max(worst, r), n + 1
        assert r <= bar, (k, F["sizes"][k], r, bar)
    return worst, n


def test_device_gradients_match_the_float64_reference():
    worst, n = _compare("dP64", "dQ64", BAR64, "full")
    worst_r, n_r = _compare("dP64", "dQ64", BAR64, "rmsd only")
    print(f"device gradients vs executed float64 reference: worst {worst:.3e} of the largest element over {n} well-conditioned pairs, "
          f"{worst_r:.3e} over {n_r} pairs through the RMSD (bar {BAR64:.0e})")
    assert n >= 30 and n_r >= 1


def test_device_gradients_match_the_float32_reference():
    bar = float(_fixture()["G"]["ref_vs_f64_grad"]) + BAR64
    worst, n = _compare("dP32", "dQ32", bar, "full")
    print(f"device gradients vs executed float32 reference: worst {worst:.3e} over {n} pairs (bar {bar:.3e})")
    assert n >= 30


@pytest.mark.parametrize("center,flip", GU.COMBOS)
def test_device_gradients_match_the_host_statement(center, flip):
    """every spelling, every well-conditioned pair, against egnn_kabsch_grad_host in float64 on the same float32 inputs"""
    F = _fixture()
    G, sizes, cut = F["G"], F["sizes"], F["cut"]
    rng = np.random.default_rng(3)
    g_R, g_t, g_rmsd = (v.astype(np.float32).astype(np.float64)       # cotangents that float32 holds exactly
                        for v in (rng.standard_normal((len(sizes), 3, 3)), rng.standard_normal((len(sizes), 3)), rng.uniform(0.5, 1.5, len(sizes))))
    dP, dQ = _device_grads(G["P"], G["Q"], sizes, center, flip, g_R, g_t, g_rmsd)
    worst, n = 0.0, 0
    for k, (P, Q) in enumerate(zip(np.split(G["P"], cut), np.split(G["Q"], cut))):
        if sizes[k] < 4 or not RU.well_conditioned(RU.sigma_f64(P, Q, center)):
            continue
        wP, wQ = GU.grad_host(_lib.lib(), P, Q, center, flip, g_R[k], g_t[k], g_rmsd[k])
        r = max(GU.worst_ratio(np.split(dP, cut)[k], wP), GU.worst_ratio(np.split(dQ, cut)[k], wQ))
        worst, n = max(worst, r), n + 1
        assert r <= BAR64, (k, sizes[k], r)
    print(f"device vs host statement ({center}, {flip}): worst {worst:.3e} over {n} pairs (bar {BAR64:.0e})")
    assert n >= 25
    assert np.isfinite(dP).all() and np.isfinite(dQ).all()       # the rank-deficient pairs (n = 2, 3) included


def _backward_abi(P, Q, gp, B, center, flip, gout, order=None, with_dQ=True):
    dP = torch.full_like(P, float("nan"))
    dQ = torch.full_like(Q, float("nan")) if with_dQ else None
    _lib.check(_lib.lib().egnn_kabsch_backward(_lib.stream_ptr(), B, _lib.ptr(P), _lib.ptr(Q), _lib.ptr(gp), _lib.ptr(order),
                                               _lib.KABSCH_CENTERS[center], _lib.KABSCH_FLIPS[flip], _lib.ptr(gout), _lib.ptr(dP),
                                               _lib.ptr(dQ)))
    return dP, dQ


def test_nan_filled_buffers_come_back_fully_written_and_runs_are_bitwise_equal():
    G = _fixture()["G"]
    sizes = [1] + G["sizes"].tolist() + [1, 1]                   # one-atom graphs: zeros
    one = np.ones((1, 3), np.float32)
    P, Q = _dev(np.concatenate([one, G["P"], one, 2 * one])), _dev(np.concatenate([2 * one, G["Q"], one, one]))
    gp, B, N = dma.stats._graph_ptr(sizes, P.device)
    gout = torch.randn(B, 16, generator=torch.Generator().manual_seed(0)).to(DEV)
    for center, flip in GU.COMBOS:
        dP, dQ = _backward_abi(P, Q, gp, B, center, flip, gout)
        assert torch.isfinite(dP).all() and torch.isfinite(dQ).all(), (center, flip)
        assert not dP[0].any() and not dQ[0].any() and not dP[-2:].any() and not dQ[-2:].any()
        dP2, dQ2 = _backward_abi(P, Q, gp, B, center, flip, gout)
        assert torch.equal(dP, dP2) and torch.equal(dQ, dQ2)
        dP3, none = _backward_abi(P, Q, gp, B, center, flip, gout, with_dQ=False)     # dQ is optional
        assert none is None and torch.equal(dP, dP3)


def test_order_form_equals_the_permuted_input_scattered_back():
    rng = np.random.default_rng(8)
    sizes = [5, 1, 9, 64, 3, 70, 2]
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    P = np.concatenate([RU.silica_cloud(rng, n) for n in sizes]).astype(np.float32)
    Q = (P @ RU.random_rotation(rng).T + 0.2 * rng.standard_normal(P.shape)).astype(np.float32)
    order = np.concatenate([np.concatenate([[0], 1 + rng.permutation(n - 1)]) for n in sizes]).astype(np.int32)
    src = np.concatenate([first[g] + order[first[g]:first[g] + n] for g, n in enumerate(sizes)])
    w = _dev(rng.uniform(0.5, 1.5, len(sizes)))
    for center, flip in (("centroid", "column"), ("first", "row")):
        Pd, Qd = _dev(P).requires_grad_(True), _dev(Q).requires_grad_(True)
        loss = dma.stats.rmsd_loss(Pd, Qd, sizes, center=center, flip=flip, order=_dev(order, torch.int32), reduction="none")
        (loss * w).sum().backward()
        Pp, Qp = _dev(P[src]).requires_grad_(True), _dev(Q).requires_grad_(True)
        want = dma.stats.rmsd_loss(Pp, Qp, sizes, center=center, flip=flip, reduction="none")
        (want * w).sum().backward()
        assert torch.equal(loss.detach(), want.detach())
        scattered = torch.zeros_like(Pp.grad)
        scattered[_dev(src, torch.long)] = Pp.grad
        assert torch.equal(Pd.grad, scattered) and torch.equal(Qd.grad, Qp.grad)
        assert torch.equal(dma.stats.kabsch(_dev(P[src]), _dev(Q), sizes, center=center, flip=flip)[2], want.detach())
    # the address guard: entries that are no row of their graph are never used as an index; such a graph is taken in identity order
    bad = order.copy()
    bad[first[3]:first[3] + sizes[3]] = rng.integers(-2**31, 2**31 - 1, sizes[3])
    bad[first[2] + 4] = sizes[2]
    keep = order.copy()
    for g in (2, 3):
        keep[first[g]:first[g] + sizes[g]] = np.arange(sizes[g])
    # `searched`: what a search leaves for graphs it did not run on may be anything, zeros included (in range, no permutation);
    # with the mask those graphs get the identity
    left = order.copy()
    left[first[2]:first[2] + sizes[2]] = 0
    left[first[3]:first[3] + sizes[3]] = rng.integers(-2**31, 2**31 - 1, sizes[3])
    mask = torch.tensor([g not in (2, 3) for g in range(len(sizes))]).to(DEV)
    results = []
    for o, kw in ((keep, {}), (bad, {}), (left, {"searched": mask})):
        Pd = _dev(P).requires_grad_(True)
        loss = dma.stats.rmsd_loss(Pd, _dev(Q), sizes, order=_dev(o, torch.int32), reduction="sum", **kw)
        loss.backward()
        results.append((loss.detach(), Pd.grad))
    for got in results[1:]:
        assert torch.equal(got[0], results[0][0]) and torch.equal(got[1], results[0][1])
    # the real thing: a search that skips the graphs above max_atoms
    out = dma.stats.kabsch_min_over_permutations(_dev(P), _dev(Q), sizes, max_atoms=9)
    assert out[3].tolist() == [True, False, True, False, True, False, True]
    Pd = _dev(P).requires_grad_(True)
    loss = dma.stats.rmsd_loss(Pd, _dev(Q), sizes, "first", "row", order=out[1], searched=out[3], reduction="none")
    loss.sum().backward()
    plain = dma.stats.kabsch(_dev(P), _dev(Q), sizes, center="first", flip="row")[2]
    srch = out[3]
    assert torch.equal(loss.detach()[~srch], plain[~srch]) and torch.equal(loss.detach()[srch], out[0][srch])
    assert torch.isfinite(Pd.grad).all()
    with pytest.raises(ValueError):
        dma.stats.rmsd_loss(_dev(P), _dev(Q), sizes, order=torch.from_numpy(order))      # an ordering on another device


def test_rank_deficient_and_close_pairs_match_the_host_statement():
    """the pairs that are NOT well-conditioned (n = 2, n = 3: rank-deficient H; small singular gaps), which torch autograd cannot
    pin: through the RMSD and t with flip='row' (g_R = 0), both centres, device against egnn_kabsch_grad_host -- which
    tests/test_rmsd_grad_host.py holds to the closed form R^T e / (n rmsd) on these very pairs.  Same bar as the other
    comparisons with float64: the optimal rotation's RMSD does not depend on how a null direction is completed."""
    F = _fixture()
    G, sizes, cut = F["G"], F["sizes"], F["cut"]
    rng = np.random.default_rng(4)
    g_t = rng.standard_normal((len(sizes), 3)).astype(np.float32).astype(np.float64)
    g_rmsd = rng.uniform(0.5, 1.5, len(sizes)).astype(np.float32).astype(np.float64)
    worst, n = 0.0, 0
    for center in ("centroid", "first"):
        dP, dQ = _device_grads(G["P"], G["Q"], sizes, center, "row", np.zeros((len(sizes), 3, 3)), g_t, g_rmsd)
        for k, (P, Q) in enumerate(zip(np.split(G["P"], cut), np.split(G["Q"], cut))):
            if sizes[k] >= 4 and RU.well_conditioned(RU.sigma_f64(P, Q, center)):
                continue
            wP, wQ = GU.grad_host(_lib.lib(), P, Q, center, "row", None, g_t[k], g_rmsd[k])
            r = max(GU.worst_ratio(np.split(dP, cut)[k], wP), GU.worst_ratio(np.split(dQ, cut)[k], wQ))
            worst, n = max(worst, r), n + 1
            assert r <= BAR64, (center, k, sizes[k], r)
    print(f"device vs host statement on the pairs that are not well-conditioned (row flip, RMSD and t): worst {worst:.3e} over {n} (bar {BAR64:.0e})")
    assert n >= 20 and {2, 3} <= {sizes[k] for k in range(len(sizes)) if not G["kind"][k]}


def test_without_grad_kabsch_is_todays_launch():
    F = _fixture()
    G, sizes = F["G"], F["sizes"]
    P, Q = _dev(G["P"]), _dev(G["Q"])
    gp, B, _ = dma.stats._graph_ptr(sizes, P.device)
    for center, flip in GU.COMBOS:
        today = dma.stats._kabsch_launch(P, Q, gp, B, center, flip)
        with torch.no_grad():
            R, t, rmsd = dma.stats.kabsch(P.clone().requires_grad_(True), Q, sizes, center=center, flip=flip)
        assert not rmsd.requires_grad
        assert torch.equal(R.reshape(B, 9), today[:, :9]) and torch.equal(t, today[:, 9:12]) and torch.equal(rmsd, today[:, 12])
        R, t, rmsd = dma.stats.kabsch(P, Q, sizes, center=center, flip=flip)
        assert not rmsd.requires_grad and torch.equal(rmsd, today[:, 12])
        # the differentiable path returns the same forward values
        R2, t2, rmsd2 = dma.stats.kabsch(P.clone().requires_grad_(True), Q, sizes, center=center, flip=flip)
        assert rmsd2.requires_grad and torch.equal(R2.detach().reshape(B, 9), today[:, :9]) and torch.equal(rmsd2.detach(), today[:, 12])
    # reductions of the loss; a single graph without sizes
    r = today[:, 12]
    for red, want in (("mean", r.sum() / B), ("sum", r.sum()), ("none", r)):
        assert torch.equal(dma.stats.rmsd_loss(P, Q, sizes, center, flip, reduction=red), want)
    Ps = P[:sizes[0] + sizes[1] + sizes[2]][-sizes[2]:].clone().requires_grad_(True)
    Qs = Q[:sizes[0] + sizes[1] + sizes[2]][-sizes[2]:]
    R1, t1, rmsd1 = dma.stats.kabsch(Ps, Qs)
    assert R1.shape == (3, 3) and t1.shape == (3,) and rmsd1.dim() == 0
    rmsd1.backward()
    assert Ps.grad.shape == Ps.shape and torch.isfinite(Ps.grad).all() and Ps.grad.abs().sum() > 0
    with pytest.raises(RuntimeError):
        dma.stats.rmsd_loss(P.cpu(), Q.cpu(), sizes)


def test_rmsd_loss_composes_with_the_egnn_backward():
    """loss = rmsd_loss(x_out, target) on a 2-layer EquivariantGNN, fp32: parameter and input gradients against oracle/egnn_ref
    followed by the autograd restatement on the CPU, at the fp32 bars of tests/test_training.py (1e-4 each)"""
    from oracle.egnn_ref import egnn_forward as oracle_forward
    H, sizes = 36, [5, 1, 9, 3]
    d = dims_for(H, 128, 256, 256, 256)
    n = sum(sizes)
    g = torch.Generator().manual_seed(21)
    h0, x0 = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g) * 1.5
    target = x0 + 0.3 * torch.randn(n, 3, generator=g)
    plan = dma.fully_connected_plan(list(sizes), torch.device(DEV))
    ei = dma.plan_edge_index(plan).cpu()
    ptr = torch.tensor([0] + np.cumsum(sizes).tolist())
    torch.manual_seed(4)
    net = dma.EquivariantGNN(2, **d)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    hr, xr = h0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    _, xo_r = oracle_forward(sd, ei, hr, xr, "graph", ptr)
    loss_ref = GU.rmsd_loss_autograd(xo_r.double(), target.double(), sizes)
    loss_ref.backward()
    net.to(DEV).train()
    net.precision, net.norm_scope = "fp32", "graph"
    h, x = h0.to(DEV).requires_grad_(True), x0.to(DEV).requires_grad_(True)
    _, xo = net(plan, h, x)
    loss = dma.stats.rmsd_loss(xo, target.to(DEV), sizes)
    loss.backward()
    assert abs(float(loss.detach()) - float(loss_ref.detach())) <= 1e-4 * float(loss_ref.detach())
    multi, single = {}, {}
    for k, p in net.named_parameters():
        want = sd[k].grad
        if want is None or not want.any():        # the last layer's message / attention / h heads do not reach x_out
            assert p.grad is None or not p.grad.any(), k
            continue
        assert p.grad is not None, k
        (multi if want.numel() > 1 else single)[k] = rel_err(p.grad.cpu(), want)
    e_h, e_x = rel_err(h.grad.cpu(), hr.grad), rel_err(x.grad.cpu(), xr.grad)
    wm, ws = max(multi, key=multi.get), max(single, key=single.get)
    print(f"rmsd_loss through the EGNN vs oracle + autograd restatement: dL/dh {e_h:.2e} dL/dx {e_x:.2e} parameter tensors worst "
          f"{multi[wm]:.2e} ({wm}), one-element parameters worst {single[ws]:.2e} ({ws})")
    assert len(multi) >= 10 and multi[wm] <= 1e-4 and single[ws] <= 1e-4 and e_h <= 1e-4 and e_x <= 1e-4

"""The float64 restatement of the forward stages (tests/_fwd_ref.py) is proven before it judges a kernel: its exact edge_pass
followed by its exact node_update must reproduce the oracle's layer (oracle.egnn_ref.egcl_forward, return_aggregates=True) run in
float64 -- h', x' and the three aggregates, every element to 1e-10 of the tensor's largest entry -- in both norm scopes, on the
irregular CSR batches the GPU stage tests run on (all three tile heights) and on ragged fully connected graphs.  The irregular
batches themselves are checked here as well: the conditions on row_ptr that the GPU tests assert before launching hold, and the
sizes are the ones the tile-selection thresholds of the library were chosen against."""
import pytest
import torch

from oracle.egnn_ref import egcl_forward, init_state_dict
from tests import _bwd_ref as R
from tests import _fwd_ref as F

H, WX, WM, M, WH = 7, 24, 16, 8, 12
TIGHT = 1e-10
D = torch.float64


def _batch(kind):
    return F.fully_connected_batch((5, 1, 9, 2)) if kind == "ragged" else F.irregular_batch(int(kind[1:]))


@pytest.fixture(scope="module", params=["ragged", "R32", "R64", "R128"])
def problem(request):
    b = _batch(request.param)
    g = torch.Generator().manual_seed(21)
    sd32 = init_state_dict(1, 2 * H + 1, WM, M, 2 * H + 1, WX, 1, H + M, WH, H, seed=4)
    sd = {k: (v.double() * (3.0 if ".2.weight" in k and "mlp_h" not in k else 1.0)) for k, v in sd32.items()}
    h = torch.randn(b.N, H, generator=g, dtype=D)
    x = torch.randn(b.N, 3, generator=g, dtype=D) * 1.5
    return R.NS(b=b, sd=sd, p={k[len("egcl_list.0."):]: v for k, v in sd.items()}, h=h, x=x)


@pytest.mark.parametrize("scope", ["graph", "call"])
def test_exact_stages_compose_to_the_float64_oracle(problem, scope):
    pb, b = problem, problem.b
    ei = torch.stack((b.dst, b.src))
    h_ref, x_ref, (agg_m, raw_x, sq) = egcl_forward(pb.sd, 0, ei, pb.h, pb.x, scope, b.graph_ptr, return_aggregates=True)
    ep = F.edge_pass(pb.p, H, pb.h, pb.x, b.dst, b.src, b.node_graph, b.N, b.B, scope)
    nu = F.node_update(pb.p, H, pb.h, pb.x, ep.sum_m, ep.sum_x, ep.sq, b.node_graph, scope)
    for name, got, want in (("sum_m", ep.sum_m, agg_m), ("sum_x", ep.sum_x, raw_x), ("sq", ep.sq, sq), ("h_out", nu.h_out, h_ref),
                            ("x_out", nu.x_out, x_ref)):
        assert got.shape == want.shape, name
        scale = float(want.abs().max())
        assert scale > 0, name
        assert float((got - want).abs().max()) <= TIGHT * scale, (scope, name, float((got - want).abs().max()) / scale)
    iso = (b.row_ptr[1:] == b.row_ptr[:-1])
    assert bool((ep.sum_m[iso] == 0).all()) and bool((ep.sum_x[iso] == 0).all()) and bool((ep.abs_sum_m[iso] == 0).all())


def test_irregular_batches_have_the_features_and_sizes_the_gpu_tests_rely_on():
    want = {32: (1079, 132, 12), 64: (3290, 256, 22), 128: (7887, 458, 25)}
    for R_, (E, N, segs) in want.items():
        b = F.irregular_batch(R_)
        f = F.assert_features(b, R_)
        assert (b.E, b.N, f["max_segments"]) == (E, N, segs), (R_, b.E, b.N, f["max_segments"])
        assert b.N <= 1024                                   # the 8-way hidden split of node_post stays reachable
        assert torch.equal(b.row_ptr[b.graph_ptr][1:] - b.row_ptr[b.graph_ptr][:-1] > 0, torch.tensor([True, False, True, False, True]))
    # edge counts against the library's tile selection for bf16 / fp16 (egnn_forward.hip small_tiles: 2048 / 6144)
    assert want[32][0] <= 2048 < want[64][0] <= 6144 < want[128][0]
    # a fully connected batch has none of the tile features: the assertion is able to fail
    f = F.csr_features(F.fully_connected_batch((64, 1, 33, 2, 17, 50)), 128)
    assert not f["spans_three_tiles"] and not f["self_loop"] and not f["duplicate_edge"] and not f["fills_two_tiles"]


def _rel_rows(a, b):
    return float(R.row_rel(a, b).max())


def test_rounding_models_are_the_exact_pass_plus_roundings():
    """per precision: close to exact, not equal to it, and ordered as the operand formats are (bf16 8 bits, fp16 11, the two
    split forms ~16); the bf16 model is _bwd_ref.forward_kept(model=True) continued by the heads"""
    b = F.irregular_batch(32)
    g = torch.Generator().manual_seed(5)
    Hh, Wx, Wm, Mm = 6, 64, 64, 32
    sd = init_state_dict(1, 2 * Hh + 1, Wm, Mm, 2 * Hh + 1, Wx, 1, Hh + Mm, 128, Hh, seed=2)
    p = {k[len("egcl_list.0."):]: v * (3.0 if ".2.weight" in k and "mlp_h" not in k else 1.0) for k, v in sd.items()}
    h, x = torch.randn(b.N, Hh, generator=g), torch.randn(b.N, 3, generator=g) * 1.5
    args = (p, Hh, h, x, b.dst, b.src, b.node_graph, b.N, b.B, "graph")
    ex = F.edge_pass(*args)
    live = b.row_ptr[1:] > b.row_ptr[:-1]
    err = {}
    for prec in F.MODELS:
        mo = F.edge_pass(*args, prec, True)
        err[prec] = (_rel_rows(mo.sum_m[live], ex.sum_m[live]), _rel_rows(mo.sum_x[live], ex.sum_x[live]))
        assert 0 < err[prec][0] <= 2e-2 and 0 < err[prec][1] <= 5e-2, (prec, err[prec])
        assert torch.equal(mo.sq, F.edge_pass(*args, "bf16", True).sq)
        u = F.edge_bounds(mo, Hh, b.dst, b.src, b.N, (b.row_ptr[1:] - b.row_ptr[:-1]).to(D), 2)
        for t in (u.sum_m, u.sum_x):
            assert bool((t[1] >= t[0] * (1 - 1e-12)).all()) and bool((t[0][live] > 0).all()) and bool((t[:, ~live] == 0).all())
    assert err["fp32"][0] < 1e-6 and err["bf16x3"][0] < 2e-4 and err["f16c8"][0] < 2e-4
    assert err["bf16"][0] > err["fp16"][0] > max(err["bf16x3"][0], err["f16c8"][0]) > err["fp32"][0]
    assert err["fp16"][0] < err["bf16g"][0] < 2 * err["bf16"][0]          # bf16 operands on an exact table
    mo = F.edge_pass(*args, "bf16", True)
    diff, d2 = R.geometry(x, b.dst, b.src, True)
    tx, tm = (R.tables(h, p[f"mlp_{n}.0.weight"], p[f"mlp_{n}.0.bias"], Hh, True) for n in ("x", "m"))
    fk = R.forward_kept(tx, tm, d2, b.dst, b.src, p["mlp_x.2.weight"], p["mlp_x.2.bias"], p["mlp_m.2.weight"], p["mlp_m.2.bias"],
                        p["mlp_x.4.weight"], p["mlp_x.4.bias"], True)
    # (forward_kept rounds a1 and t2 to fp32 where this module keeps them unrounded: two realisations of the same documented
    # roundings, which is exactly what the element-wise bound of the GPU test has to cover)
    u = F.edge_bounds(mo, Hh, b.dst, b.src, b.N, (b.row_ptr[1:] - b.row_ptr[:-1]).to(D), 2)
    assert R.worst_ratio(fk.s_e, mo.e.s_e, u.s_e[1]) <= 1.0 and float((mo.e.s_e - fk.s_e).abs().max()) <= 1e-5
    assert R.worst_ratio(fk.t2m_unrounded, mo.e.m.sl.t2, u.t2m[1]) <= 1.0
    # node forms, on the exact aggregates
    nx = F.node_update(p, Hh, h, x, ex.sum_m, ex.sum_x, ex.sq, b.node_graph, "graph")
    e_form = {}
    for form in ("fp32", "bf16", "split"):
        nm = F.node_update(p, Hh, h, x, ex.sum_m, ex.sum_x, ex.sq, b.node_graph, "graph", form, True)
        e_form[form] = _rel_rows(nm.h_out, nx.h_out)
        assert torch.equal(nm.x_out, nx.x_out)
    assert e_form["fp32"] == 0 and 0 < e_form["split"] < 1e-5 < e_form["bf16"] < 3e-2, e_form
    # x' follows a supplied normaliser: four times the sums is exactly half the step where sqrt(sq) >> 1 is not assumed
    n4 = F.node_update(p, Hh, h, x, ex.sum_m, ex.sum_x, ex.sq * 4, b.node_graph, "graph")
    g1, g4 = 1.0 / (torch.sqrt(ex.sq) + 1.0), 1.0 / (2.0 * torch.sqrt(ex.sq) + 1.0)
    assert torch.allclose((n4.x_out - x.double()) * g1[b.node_graph][:, None], (nx.x_out - x.double()) * g4[b.node_graph][:, None],
                          rtol=1e-12, atol=1e-14)

"""The gradient of the Kabsch fit on the host (egnn_kabsch_grad_host: csrc/eval/kabsch_host.cpp over the 3x3 numerics the device
kernel uses, csrc/eval/kabsch_math.h), without a GPU:

  * against the float64 gradients of the EXECUTED reference (kabsch_torch under torch autograd) stored in
    tests/golden/rmsd_grad_golden.npz.  Bar 1e-9 of the graph's largest gradient element: both sides are float64; the slack is for
    torch's 1 / (s_i^2 - s_j^2) at a singular gap of 1e-2 sigma_1 (RU.well_conditioned), which the library's form does not have;
  * all four (center, flip) combinations against the float64 torch-autograd restatement of tests/_rmsd_grad_util.py, same bar;
  * degenerate inputs give finite results; the row-flip RMSD gradient equals its closed form R^T e_i / (n rmsd);
  * the same calls under AddressSanitizer + UBSan (make asan).
"""
import os

import numpy as np

from diffusion_model_amd import _lib
from tests import _rmsd_grad_util as GU
from tests import _rmsd_util as RU
from tests._util import load_golden
from tests.test_host_asan import _run as run_under_sanitizers

BAR = 1e-9


def _pairs(G):
    sizes = G["sizes"].tolist()
    cut = np.cumsum(sizes)[:-1]
    parts = {k: np.split(G[k], cut) for k in ("P", "Q", "dP64", "dQ64", "dP32", "dQ32")}
    return sizes, [{k: v[i] for k, v in parts.items()} for i in range(len(sizes))]


def test_fixture_satisfies_its_conditions():
    G = load_golden("rmsd_grad_golden.npz")
    sizes, kind = G["sizes"], G["kind"]
    assert len(sizes) >= 40 and {2, 3, 4, 5, 8, 17, 63, 64, 65, 130} <= set(sizes.tolist())
    assert int(kind.sum()) >= 30 and int((kind * G["reflection"]).sum()) >= 12
    assert {round(float(v), 6) for v in G["noise"]} == {0.01, 0.1, 0.5} and int(G["mirrored"].sum()) == len(sizes) // 3
    _, pairs = _pairs(G)
    for k, c in enumerate(pairs):
        assert c["P"].dtype == np.float32 and c["dP64"].dtype == np.float64
        if kind[k]:
            assert sizes[k] >= 4 and RU.well_conditioned(RU.sigma_f64(c["P"], c["Q"], "centroid")), k
        else:
            assert not G["g_R"][k].any() and not G["g_t"][k].any()
    assert 0.0 < float(G["ref_vs_f64_grad"]) < 1e-3


def test_host_gradient_matches_the_executed_reference():
    G = load_golden("rmsd_grad_golden.npz")
    sizes, pairs = _pairs(G)
    worst, n_full, n_rmsd = 0.0, 0, 0
    for k, c in enumerate(pairs):
        if not (G["kind"][k] or G["defined"][k]):
            continue
        flip = "column" if G["kind"][k] else "row"     # the rest: through g_rmsd only, where the reference's rotation is the optimal one
        dP, dQ = GU.grad_host(_lib.lib(), c["P"], c["Q"], "centroid", flip, G["g_R"][k], G["g_t"][k], float(G["g_rmsd"][k]))
        r = max(GU.worst_ratio(dP, c["dP64"]), GU.worst_ratio(dQ, c["dQ64"]))
        worst = max(worst, r)
        n_full += int(G["kind"][k])
        n_rmsd += int(not G["kind"][k])
        assert r <= BAR, (k, sizes[k], flip, r)
    print(f"host gradient vs executed float64 reference: worst {worst:.3e} of the largest element ({n_full} + {n_rmsd} pairs, bar {BAR:.0e})")
    assert n_full >= 30 and n_rmsd >= 1


def test_all_four_spellings_match_the_autograd_restatement():
    G = load_golden("rmsd_grad_golden.npz")
    sizes, pairs = _pairs(G)
    rng = np.random.default_rng(5)
    worst, count = {}, {}
    for k, c in enumerate(pairs):
        g_R, g_t, g_rmsd = rng.standard_normal((3, 3)), rng.standard_normal(3), float(rng.uniform(0.5, 1.5))
        for center, flip in GU.COMBOS:
            if sizes[k] < 4 or not RU.well_conditioned(RU.sigma_f64(c["P"], c["Q"], center)):
                continue
            want = GU.grads_autograd(lambda a, b: GU.kabsch_autograd(a, b, center, flip), c["P"], c["Q"], g_R, g_t, g_rmsd)
            got = GU.grad_host(_lib.lib(), c["P"], c["Q"], center, flip, g_R, g_t, g_rmsd)
            r = max(GU.worst_ratio(got[0], want[0]), GU.worst_ratio(got[1], want[1]))
            worst[center, flip] = max(worst.get((center, flip), 0.0), r)
            count[center, flip] = count.get((center, flip), 0) + 1
            assert r <= BAR, (k, sizes[k], center, flip, r)
    print("host gradient vs float64 autograd restatement:", {k: f"{v:.2e} ({count[k]})" for k, v in worst.items()})
    assert all(count.get(cf, 0) >= 25 for cf in GU.COMBOS), count
    # the restatement agrees with the executed reference in the reference's spelling
    c = pairs[int(np.argmax(G["kind"]))]
    k = int(np.argmax(G["kind"]))
    want = GU.grads_autograd(lambda a, b: GU.kabsch_autograd(a, b, "centroid", "column"), c["P"], c["Q"], G["g_R"][k], G["g_t"][k],
                             float(G["g_rmsd"][k]))
    assert GU.worst_ratio(want[0], c["dP64"]) <= 1e-12 and GU.worst_ratio(want[1], c["dQ64"]) <= 1e-12


def _degenerate_cases():
    rng = np.random.default_rng(11)
    tri = RU.silica_cloud(rng, 3)
    planar = RU.silica_cloud(rng, 9) * np.array([1.0, 1.0, 0.0])
    same = RU.silica_cloud(rng, 7)
    line = np.outer(np.arange(5.0), [1.0, 2.0, -1.0])
    move = lambda X, s: X @ RU.random_rotation(rng).T + rng.uniform(-2, 2, 3) + s * rng.standard_normal(X.shape)
    return {"two atoms": (RU.silica_cloud(rng, 2), move(RU.silica_cloud(rng, 2), 0.1)), "three atoms": (tri, move(tri, 0.1)),
            "planar": (planar, move(planar, 0.0)), "planar, noisy in the plane": (planar, planar + 0.1 * rng.standard_normal(planar.shape) * [1, 1, 0]),
            "collinear": (line, move(line, 0.0)), "P = Q": (same, same.copy()), "all atoms at one point": (np.ones((4, 3)), np.ones((4, 3))),
            "one atom": (np.ones((1, 3)), np.zeros((1, 3)))}


def test_degenerate_inputs_give_finite_gradients():
    rng = np.random.default_rng(12)
    for name, (P, Q) in _degenerate_cases().items():
        g_R, g_t = rng.standard_normal((3, 3)), rng.standard_normal(3)
        for center, flip in GU.COMBOS:
            dP, dQ = GU.grad_host(_lib.lib(), P, Q, center, flip, g_R, g_t, 1.0)
            assert np.isfinite(dP).all() and np.isfinite(dQ).all(), (name, center, flip)
            if name == "one atom":
                assert not dP.any() and not dQ.any()
            dP2, none = GU.grad_host(_lib.lib(), P, Q, center, flip, g_R, g_t, 1.0, want_dQ=False)     # dQ is optional
            assert none is None and np.array_equal(dP, dP2)
    # rmsd = 0 exactly (every atom at the centre) contributes nothing; P = Q in general leaves a residual of rounding size, whose
    # normalised direction is a gradient of the size every RMSD gradient has (|d rmsd / dP| = 1 / sqrt(n) for an optimal R)
    P, Q = _degenerate_cases()["all atoms at one point"]
    for center, flip in GU.COMBOS:
        dP, dQ = GU.grad_host(_lib.lib(), P, Q, center, flip, None, None, 1.0)
        assert not dP.any() and not dQ.any()
    P, Q = _degenerate_cases()["P = Q"]
    for center, flip in GU.COMBOS:
        dP, dQ = GU.grad_host(_lib.lib(), P, Q, center, flip, None, None, 1.0)
        assert np.linalg.norm(dP) <= 10.0 and np.linalg.norm(dQ) <= 10.0
        # t alone is a plain difference of centres
        g_t = np.array([1.0, -2.0, 0.5])
        dP, dQ = GU.grad_host(_lib.lib(), P, Q, center, flip, None, g_t, 0.0)
        want = np.tile(g_t / len(P), (len(P), 1)) if center == "centroid" else np.concatenate([g_t[None], np.zeros((len(P) - 1, 3))])
        assert np.abs(dQ - want).max() <= 1e-15 and np.abs(dP + want).max() <= 1e-15


def test_row_flip_rmsd_gradient_equals_its_closed_form():
    """R of flip='row' minimises the residual, so d rmsd / dR = 0 on the rotations and d rmsd / dp_i = R^T e_i / (n rmsd),
    d rmsd / dq_i = -e_i / (n rmsd), then the centring; for every pair of the fixture, the rank-deficient ones included"""
    G = load_golden("rmsd_grad_golden.npz")
    sizes, pairs = _pairs(G)
    worst = 0.0
    for k, c in enumerate(pairs):
        for center in ("centroid", "first"):
            P, Q = c["P"].astype(np.float64), c["Q"].astype(np.float64)
            p, q, _, _ = RU.covariance_f64(P, Q, center)
            R, _, rmsd = RU.kabsch_f64(P, Q, center, "row")
            e = p @ R.T - q
            pb, qb = e @ R / (len(P) * rmsd), -e / (len(P) * rmsd)
            if center == "centroid":
                pb, qb = pb - pb.mean(0), qb - qb.mean(0)
            else:
                pb[0], qb[0] = pb[0] - pb.sum(0), qb[0] - qb.sum(0)
            dP, dQ = GU.grad_host(_lib.lib(), P, Q, center, "row", None, None, 1.0)
            r = max(GU.worst_ratio(dP, pb), GU.worst_ratio(dQ, qb))
            worst = max(worst, r)
            assert r <= BAR, (k, sizes[k], center, r)
    print(f"row-flip RMSD gradient vs closed form: worst {worst:.3e} of the largest element")


def test_host_gradient_under_sanitizers():
    """the calls of the tests above in the instrumented build: the fixture's pairs in all four spellings against the values the
    product library returns, the degenerate cases, the optional arguments, the argument checks"""
    G = load_golden("rmsd_grad_golden.npz")
    sizes, pairs = _pairs(G)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rmsd_grad_golden.npz")
    want = []
    for k in (0, 1, 2, 5, 8, 9, 26, 47):
        c = pairs[k]
        for ci, center in enumerate(("centroid", "first")):
            for fi, flip in enumerate(("row", "column")):
                dP, dQ = GU.grad_host(_lib.lib(), c["P"], c["Q"], center, flip, G["g_R"][k], G["g_t"][k], float(G["g_rmsd"][k]))
                want.append((k, ci, fi, float(np.abs(dP).sum()), float(np.abs(dQ).sum())))
    run_under_sanitizers("""
        G = np.load(%r, allow_pickle=False)
        dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
        L.egnn_kabsch_grad_host.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int,
                                            C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double),
                                            C.POINTER(C.c_double)]
        cut = np.concatenate([[0], np.cumsum(G["sizes"])])
        for k, ci, fi, sP, sQ in %r:
            P, Q = (np.ascontiguousarray(G[n][cut[k]:cut[k + 1]], dtype=np.float64) for n in ("P", "Q"))
            dP, dQ = np.full_like(P, np.nan), np.full_like(Q, np.nan)
            gR, gt = np.ascontiguousarray(G["g_R"][k]), np.ascontiguousarray(G["g_t"][k])
            assert L.egnn_kabsch_grad_host(len(P), dp(P), dp(Q), ci, fi, dp(gR), dp(gt), float(G["g_rmsd"][k]), dp(dP), dp(dQ)) == OK
            assert np.isfinite(dP).all() and np.isfinite(dQ).all()
            assert abs(np.abs(dP).sum() - sP) <= 1e-9 * sP + 1e-300 and abs(np.abs(dQ).sum() - sQ) <= 1e-9 * sQ + 1e-300, (k, ci, fi)
            dP2 = np.full_like(P, np.nan)
            assert L.egnn_kabsch_grad_host(len(P), dp(P), dp(Q), ci, fi, None, None, 1.0, dp(dP2), None) == OK and np.isfinite(dP2).all()
        one, z = np.ones((4, 3)), np.zeros((4, 3))
        line = np.ascontiguousarray(np.outer(np.arange(5.0), [1.0, 2.0, -1.0]))
        for P, Q in ((one, one.copy()), (one[:1].copy(), z[:1].copy()), (line, line[::-1].copy()), (z, z.copy())):
            for ci in (0, 1):
                for fi in (0, 1):
                    dP, dQ = np.full_like(P, np.nan), np.full_like(Q, np.nan)
                    assert L.egnn_kabsch_grad_host(len(P), dp(P), dp(Q), ci, fi, dp(np.ones(9)), dp(np.ones(3)), 1.0, dp(dP), dp(dQ)) == OK
                    assert np.isfinite(dP).all() and np.isfinite(dQ).all()
        P, d = np.ones((2, 3)), np.zeros((2, 3))
        assert L.egnn_kabsch_grad_host(0, dp(P), dp(P), 0, 0, None, None, 1.0, dp(d), None) == EINVAL
        assert b"egnn_kabsch_grad_host" in L.egnn_last_error()
        assert L.egnn_kabsch_grad_host(2, None, dp(P), 0, 0, None, None, 1.0, dp(d), None) == EINVAL
        assert L.egnn_kabsch_grad_host(2, dp(P), dp(P), 0, 0, None, None, 1.0, None, None) == EINVAL
        assert L.egnn_kabsch_grad_host(2, dp(P), dp(P), 2, 0, None, None, 1.0, dp(d), None) == EINVAL
        assert L.egnn_kabsch_grad_host(2, dp(P), dp(P), 0, -1, None, None, 1.0, dp(d), None) == EINVAL
    """ % (path, want))

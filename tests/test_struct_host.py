"""The whole-structure statistics on the host (egnn_struct_counts_host: csrc/eval/structure_host.cpp over the definitions the
kernels compile, csrc/eval/structure_math.h), without a GPU:

  * the stored fixture tests/golden/struct_golden.npz (made by EXECUTING the reference's RDF and calculate_angle_for_CN2,
    tests/golden/make_struct_golden.py) satisfies its two gap conditions when recomputed;
  * the numpy restatement (tests/_struct_util.py) reproduces the executed reference: the mean RDF over the centres of a type within
    1e-12 * max(1, max|curve|) (both sides float64, sums of at most 65 terms in another order), the angles within 1e-4 degrees
    (the reference computes them in float32);
  * egnn_struct_counts_host equals the restatement EXACTLY in all three integer outputs, on the fixture and on seeded batches;
  * bad arguments return EGNN_EINVAL, from the host statement and -- before anything is launched -- from the device entries.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from diffusion_model_amd import _lib
from tests import _struct_util as SU
from tests._util import load_golden

EINVAL = -22
SIZES = [1, 2, 3, 64, 65, 129, 257, 7]


def _fixture():
    G = load_golden("struct_golden.npz")
    graphs = []
    for g, (n, A) in enumerate(zip(G["sizes"].tolist(), G["A"].tolist())):
        graphs.append(dict(n=n, A=A, pos=G[f"g{g}.pos"], types=G[f"g{g}.types"], rdf=[G[f"g{g}.rdf0"], G[f"g{g}.rdf1"]],
                           triplets=G[f"g{g}.triplets"], angles=G[f"g{g}.angles"]))
    settings = [(float(s), float(R), float(dR)) for s, R, dR in G["settings"]]
    return graphs, settings, float(G["cutoff"]), [float(v) for v in G["dthetas"]]


def test_fixture_satisfies_its_conditions():
    graphs, settings, cutoff, dthetas = _fixture()
    assert [c["n"] for c in graphs[:6]] == [2, 3, 7, 20, 64, 65] and all(c["A"] == 2 for c in graphs[:6]) and graphs[6]["A"] == 3
    assert settings == [(5.0, 5.0, 0.01), (3.0, 4.0, 0.02)] and cutoff == 2.0
    radial = [(R, dR) for _, R, dR in settings]
    n_angles = 0
    for c in graphs:
        pos, n = c["pos"], c["n"]
        assert pos.dtype == np.float32 and pos.shape == (n, 3) and set(c["types"].tolist()) == set(range(min(c["A"], n)))
        off = ~np.eye(n, dtype=bool)
        mine = SU.distances(pos)[off]
        p = torch.from_numpy(pos)
        theirs = np.array([[torch.norm(p[j] - p[i]).item() if i != j else 0.0 for j in range(n)] for i in range(n)], dtype=np.float32)[off]
        # condition 1: both float32 spellings clear every edge and the cutoff by more than 4 ulp, and agree on every bin
        assert SU.radial_gap_ok(mine, radial, cutoff) and SU.radial_gap_ok(theirs, radial, cutoff), n
        assert np.array_equal(mine < np.float32(cutoff), theirs < np.float32(cutoff))
        for R, dR in radial:
            nb = SU.nbins_of(R, dR)
            for a, b in zip(SU.radial_bins(mine, dR, nb), SU.radial_bins(theirs, dR, nb)):
                assert np.array_equal(a, b)
        # condition 2
        thetas = [r[3] for r in SU.bonded_angles(pos, c["types"], cutoff)[0]]
        n_angles += len(thetas)
        for dt in dthetas:
            assert SU.angle_gap(thetas, dt) >= 1e-9, (n, dt)
    assert n_angles >= 100
    # the gap check itself: a distance on an edge, 4 ulp from it, and 5 ulp from it
    lo, _ = SU.bin_edges(0.01, 500)
    on = lo[123]
    step = lambda x, k: (np.array([x], dtype=np.float32).view(np.int32) + k).view(np.float32)
    assert not SU.radial_gap_ok(step(on, 0), radial, cutoff) and not SU.radial_gap_ok(step(on, 4), radial, cutoff)
    assert not SU.radial_gap_ok(step(on, -4), radial, cutoff) and SU.radial_gap_ok(step(on, 5), radial, cutoff)
    assert not SU.radial_gap_ok(step(np.float32(cutoff), -2), radial, cutoff)


def test_restatement_reproduces_the_executed_reference():
    graphs, settings, cutoff, _ = _fixture()
    worst_curve, worst_angle = 0.0, 0.0
    for c in graphs:
        n_type = np.bincount(c["types"], minlength=c["A"])
        for (sigma, R, dR), want in zip(settings, c["rdf"]):
            g_ab = SU.partial_rdf(SU.pair_counts(c["pos"], c["types"], c["A"], R, dR), n_type, c["n"], sigma, R, dR)
            got = g_ab.sum(1)                      # sum over the neighbour type: the mean RDF of the centres of type a
            assert got.shape == want.shape
            err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
            worst_curve = max(worst_curve, err)
            assert err <= 1e-12, (c["n"], sigma, err)
        rows = SU.bonded_angles(c["pos"], c["types"], cutoff)[0]
        assert np.array_equal(np.array([r[:3] for r in rows], dtype=np.int32).reshape(-1, 3), c["triplets"])
        if rows:
            err = float(np.abs(np.array([r[3] for r in rows]) - c["angles"]).max())
            worst_angle = max(worst_angle, err)
            assert err <= 1e-4, (c["n"], err)
    print(f"restatement vs executed reference: curves {worst_curve:.3e} (bar 1e-12), angles {worst_angle:.3e} degrees (bar 1e-4)")


def _assert_host_equals_restatement(pos, types, sizes, A, **kw):
    want = SU.batch_statistics(pos, types, sizes, A, **kw)
    assert want[4] >= 1e-9, f"ambiguous input: an angle {want[4]:.1e} degrees from a bin edge"
    rc, counts, cn, ang, over = SU.host_counts(_lib.lib(), pos, types, sizes, A, **kw)
    assert rc == 0, _lib.lib().egnn_last_error()
    assert np.array_equal(counts, want[0]) and np.array_equal(cn, want[1]) and np.array_equal(ang, want[2])
    assert np.array_equal(over, want[3])
    return want


def test_host_statement_equals_the_restatement_on_the_fixture():
    graphs, settings, cutoff, dthetas = _fixture()
    for A in (2, 3):
        cs = [c for c in graphs if c["A"] == A]
        pos, types, sizes = np.concatenate([c["pos"] for c in cs]), np.concatenate([c["types"] for c in cs]), [c["n"] for c in cs]
        for (_, R, dR), dt in zip(settings, dthetas):
            want = _assert_host_equals_restatement(pos, types, sizes, A, R=R, dR=dR, cutoff=cutoff, dtheta=dt)
            assert want[0].sum() > 0 and want[2].sum() > 0


@pytest.mark.parametrize("A", [1, 2, 3])
def test_host_statement_equals_the_restatement_on_seeded_batches(A):
    pos, types = SU.random_batch(100 + A, SIZES, A)
    want = _assert_host_equals_restatement(pos, types, SIZES, A)
    assert want[2].sum() > 100 and want[3].sum() == 0 and want[1][..., 2:].sum() > 0
    _assert_host_equals_restatement(pos, types, SIZES, A, R=4.0, dR=0.02, cutoff=2.5, dtheta=2.5, max_cn=3)
    _assert_host_equals_restatement(pos, types, SIZES, A, R=10.24, dR=0.01)


def test_host_statement_counts_beyond_the_neighbour_cap():
    """65 points on a sphere about a centre: the centre's CN is counted, its angles are not, overflow says so"""
    rng = np.random.default_rng(3)
    v = rng.standard_normal((65, 3))
    pos = np.concatenate([np.zeros((1, 3)), 1.5 * v / np.linalg.norm(v, axis=1, keepdims=True)]).astype(np.float32)
    types = np.zeros(66, dtype=np.int32)
    want = _assert_host_equals_restatement(pos, types, [66], 1, max_cn=64)
    assert want[3].tolist() == [1] and want[1][0, 0, 0, 64] == 1


def test_argument_errors_return_einval():
    L = _lib.lib()
    pos, types = SU.random_batch(1, [5, 4], 2)
    ok = dict(R=5.0, dR=0.01, cutoff=2.0, dtheta=1.0, max_cn=16)
    assert SU.host_counts(L, pos, types, [5, 4], 2, **ok)[0] == 0
    for bad, word in ((dict(R=10.25), b"radial bins"), (dict(dtheta=0.4), b"dtheta"), (dict(cutoff=0.0), b"cutoff"),
                      (dict(cutoff=-1.0), b"cutoff"), (dict(max_cn=65), b"max_cn"), (dict(max_cn=0), b"max_cn")):
        assert SU.host_counts(L, pos, types, [5, 4], 2, **dict(ok, **bad))[0] == EINVAL, bad
        assert word in L.egnn_last_error(), (bad, L.egnn_last_error())
    assert SU.host_counts(L, np.zeros((9, 3), np.float32), np.zeros(9, np.int32), [5, 4], 5, **ok)[0] == EINVAL      # A > 4
    assert b"atom types" in L.egnn_last_error()
    assert SU.host_counts(L, pos, np.full(9, 2, np.int32), [5, 4], 2, **ok)[0] == EINVAL                              # a type outside [0, A)
    big = 32769
    assert SU.host_counts(L, np.zeros((big, 3), np.float32), np.zeros(big, np.int32), [big], 1, **ok)[0] == EINVAL
    assert b"32768" in L.egnn_last_error()
    # the device entries refuse the same arguments before they launch anything (no GPU is touched here)
    p = C.c_void_p(64)
    assert L.egnn_struct_pair_counts(None, 1, 2, p, p, p, 64, p, 1, 0.01, 1025, p) == EINVAL
    assert L.egnn_struct_pair_counts(None, 1, 5, p, p, p, 64, p, 1, 0.01, 500, p) == EINVAL
    assert L.egnn_struct_pair_counts(None, 1, 2, p, p, p, 32769, p, 1, 0.01, 500, p) == EINVAL
    assert L.egnn_struct_pair_counts(None, 1, 2, p, p, p, 64, None, 1, 0.01, 500, p) == EINVAL
    assert L.egnn_struct_bonds(None, 1, 2, p, p, p, 64, p, 1, 2.0, 0.49, 16, p, p, p) == EINVAL
    assert L.egnn_struct_bonds(None, 1, 2, p, p, p, 64, p, 1, 0.0, 1.0, 16, p, p, p) == EINVAL
    assert L.egnn_struct_bonds(None, 1, 5, p, p, p, 64, p, 1, 2.0, 1.0, 16, p, p, p) == EINVAL
    assert L.egnn_struct_bonds(None, 1, 2, p, p, p, 40000, p, 1, 2.0, 1.0, 16, p, p, p) == EINVAL
    assert L.egnn_struct_rdf_finish(None, 1, 2, p, p, p, 5.0, 0.01, 5.0, 1025, p) == EINVAL
    assert L.egnn_struct_rdf_finish(None, 1, 5, p, p, p, 5.0, 0.01, 5.0, 500, p) == EINVAL

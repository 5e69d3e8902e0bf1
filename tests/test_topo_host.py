"""The topological fingerprint on the host (egnn_topo_host: csrc/eval/topo_host.cpp over the definitions the kernels compile,
csrc/eval/topo_math.h), without a GPU:

  * the numpy restatement (tests/_topo_util.py) agrees with independent libraries: hop distances with
    scipy.sparse.csgraph.shortest_path(unweighted=True), fragments and components with connected_components;
  * egnn_topo_host equals the restatement EXACTLY in every integer output and in the fp64 similarity, on seeded clouds and on
    hand-made graphs (a 1024-atom chain, rings, two fragments, stars whose degree wraps the modulus, an overflowing crowd, a
    bondless graph, a graph of no atoms);
  * hand-computed similarities and the invariances of a fingerprint;
  * bad arguments return EGNN_EINVAL, from the host statement and -- before anything is launched -- from the device entries;
  * a stand-alone program runs egnn_topo_host under the address and undefined-behaviour sanitizers.

Every input first passes the gap check: no pair distance within 1e-9 (relative) of its bond threshold, so the bond decision
cannot hang on the last bit of a float64 square root.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from diffusion_model_amd import _lib
from tests import _topo_util as TU
from tests._host_program import build_and_run

EINVAL = -22
THR2 = TU.thresholds(TU.RADII[2])


@functools.lru_cache(maxsize=None)
def _cloud(A):
    """the seeded cloud batch of A types and its restatement (computed once, never changed)"""
    pos, types = TU.cloud(200 + A, TU.SIZES, A)
    thr = TU.thresholds(TU.RADII[A])
    lo = 0
    for n in TU.SIZES:
        assert TU.gap_ok(pos[lo:lo + n], types[lo:lo + n], thr), "ambiguous input: a distance on its threshold"
        lo += n
    return pos, types, thr, TU.batch(pos, types, TU.SIZES, A, thr)


@functools.lru_cache(maxsize=None)
def _specials():
    graphs = TU.special_graphs()
    for name, (p, t) in graphs.items():
        assert TU.gap_ok(p, t, THR2), name
    pos, types, sizes = TU.join(list(graphs.values()))
    return list(graphs), pos, types, sizes, TU.batch(pos, types, sizes, 2, THR2)


def _blocks(want, sizes):
    """the [n, n] distance matrices and local components of a restated batch"""
    at, lo = 0, 0
    for n in sizes:
        yield want["dist"][at:at + n * n].reshape(n, n), want["component"][lo:lo + n] - lo, lo, n
        at += n * n
        lo += n


def _assert_matches_scipy(want, sizes):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components, shortest_path
    for g, (dist, comp, lo, n) in enumerate(_blocks(want, sizes)):
        if want["overflow"][g]:
            continue
        if n == 0:                                                         # nothing for a library to compute
            assert want["fragments"][g] == 0 and dist.size == 0
            continue
        rp = want["row_ptr"][lo:lo + n + 1] - want["row_ptr"][lo]
        nb = want["neighbours"][want["row_ptr"][lo]:want["row_ptr"][lo + n]] - lo
        adj = csr_matrix((np.ones(len(nb)), nb, rp), shape=(n, n))
        sp = shortest_path(adj, unweighted=True, directed=False)
        assert np.array_equal(np.where(np.isinf(sp), TU.UNREACHABLE, sp).astype(np.int64), dist), g
        k, labels = connected_components(adj, directed=False)
        assert k == want["fragments"][g], g
        lowest = np.array([np.nonzero(labels == labels[i])[0][0] for i in range(n)]).reshape(n)
        assert np.array_equal(lowest, comp), g


@pytest.mark.parametrize("A", [1, 2, 3])
def test_restatement_agrees_with_scipy_on_clouds(A):
    _, _, _, want = _cloud(A)
    _assert_matches_scipy(want, TU.SIZES)
    assert want["fp"].sum() > 1000 and want["fragments"].max() > 1 and want["overflow"].sum() == 0


def test_restatement_agrees_with_scipy_on_the_hand_made_graphs():
    names, _, _, sizes, want = _specials()
    _assert_matches_scipy(want, sizes)
    g = {name: k for k, name in enumerate(names)}
    blocks = list(_blocks(want, sizes))
    assert blocks[g["chain1024"]][0][0, 1023] == 1023 and want["fragments"][g["chain1024"]] == 1
    assert blocks[g["ring6"]][0].max() == 3 and blocks[g["ring5"]][0].max() == 2
    assert want["fragments"][g["fragments"]] == 2 and blocks[g["fragments"]][1].tolist() == [0, 0, 0, 3, 3, 3]
    assert want["overflow"][g["crowd34"]] == 34 and want["fragments"][g["crowd34"]] == -1 and not want["fp"][g["crowd34"]].any()
    assert want["fragments"][g["bondless"]] == 5 and not want["fp"][g["bondless"]].any()
    assert sizes[g["empty"]] == 0 and want["fragments"][g["empty"]] == 0 and not want["fp"][g["empty"]].any()
    lo = int(np.cumsum([0] + sizes)[g["star7"]])
    assert want["degree"][lo] == 7 and want["degree"][int(np.cumsum([0] + sizes)[g["star8"]])] == 8
    # the modulus wraps: Si of degree 7 has the class of a lone Si, so star7's Si-O key is (O deg 1, Si class 7 + 0)
    key = TU.pair_index(0 * 7 + 1, 1 * 7 + 0, 14) * 30 + 0
    assert want["fp"][g["star7"]][key] == 7
    assert want["fp"][g["star8"]][TU.pair_index(1, 7 + 1, 14) * 30] == 8 and want["fp"][g["star6"]][TU.pair_index(1, 7 + 6, 14) * 30] == 6


def _pairs(B):
    return np.array([[g, (g + 1) % B] for g in range(B)] + [[0, 0], [B - 1, B - 1]], dtype=np.int32)


def _assert_host_equals_restatement(pos, types, sizes, A, thr, want, L=30):
    pairs = _pairs(len(sizes))
    rc, got = TU.host(_lib.lib(), pos, types, sizes, A, thr, L=L, pairs=pairs)
    assert rc == 0, _lib.lib().egnn_last_error()
    TU.assert_equal(got, want)
    for p, (a, b) in enumerate(pairs):
        sim, sa, sb = TU.tanimoto(want["fp"][a], want["fp"][b])
        assert got["sim"][p] == sim and got["sa"][p] == sa and got["sb"][p] == sb, p      # the fp64 value, bit for bit
    return got


@pytest.mark.parametrize("A", [1, 2, 3])
def test_host_statement_equals_the_restatement_on_clouds(A):
    pos, types, thr, want = _cloud(A)
    got = _assert_host_equals_restatement(pos, types, TU.SIZES, A, thr, want)
    assert 0.0 < got["sim"][5] < 1.0 and got["sim"][-1] == 1.0
    short = TU.batch(pos, types, TU.SIZES, A, thr, L=2)
    _assert_host_equals_restatement(pos, types, TU.SIZES, A, thr, short, L=2)
    # the nullable outputs are optional, and the lists do not depend on them
    rc, bare = TU.host(_lib.lib(), pos, types, TU.SIZES, A, thr, want=())
    assert rc == 0
    TU.assert_equal(bare, want, ("row_ptr", "neighbours", "degree", "overflow"))
    assert (bare["fp"] == -7).all() and (bare["component"] == -7).all() and (bare["dist"] == 7).all()


def test_host_statement_equals_the_restatement_on_the_hand_made_graphs():
    _, pos, types, sizes, want = _specials()
    _assert_host_equals_restatement(pos, types, sizes, 2, THR2, want)
    long = TU.batch(pos, types, sizes, 2, THR2, L=64)
    _assert_host_equals_restatement(pos, types, sizes, 2, THR2, long, L=64)


def _similarity(a, b, **kw):
    pos, types, sizes = TU.join([a, b])
    assert TU.gap_ok(a[0], a[1], THR2) and TU.gap_ok(b[0], b[1], THR2)
    rc, got = TU.host(_lib.lib(), pos, types, sizes, 2, THR2, pairs=[[0, 1]], **kw)
    assert rc == 0
    return float(got["sim"][0]), int(got["sa"][0]), int(got["sb"][0]), got


def test_hand_computed_similarities():
    osio, osi, osiosi = TU.line("OSiO"), TU.line("OSi"), TU.line("OSiOSi")
    assert _similarity(osio, osio)[:3] == (1.0, 3, 3)
    # O-Si-O: classes O1 Si2 O1 (type, degree) -> keys {(O1, Si2, d=1): 2, (O1, O1, d=2): 1}.  The dimer: O1 Si1 -> {(O1, Si1, 1): 1}.
    # Si's degree differs, so no key is shared.
    assert _similarity(osio, osi)[:3] == (0.0, 3, 1)
    # O-Si-O-Si: classes O1 Si2 O2 Si1 -> six keys, one pair each: (O1,Si2,1) (Si2,O2,1) (O2,Si1,1) (O1,O2,2) (Si2,Si1,2) (O1,Si1,3).
    # Against O-Si-O only (O1, Si2, 1) is shared: min(1, 2) = 1, so 1 / (6 + 3 - 1) = 0.125.
    sim, sa, sb, got = _similarity(osiosi, osio)
    assert (sim, sa, sb) == (0.125, 6, 3)
    assert got["fp"][0][TU.pair_index(1, 9, 14) * 30] == 1 and got["fp"][1][TU.pair_index(1, 9, 14) * 30] == 2
    assert got["fp"][0][TU.pair_index(1, 8, 14) * 30 + 2] == 1
    assert _similarity(TU.bondless(4), TU.bondless(3))[:3] == (0.0, 0, 0)


def test_fingerprint_is_invariant_under_permutation_and_rigid_motion():
    pos, types, thr, want = _cloud(2)
    lo, n = int(np.cumsum([0] + TU.SIZES)[6]), TU.SIZES[6]                  # the 129-atom cloud
    p, t = pos[lo:lo + n], types[lo:lo + n]
    rng = np.random.default_rng(1)
    perm = rng.permutation(n)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    moved = (p.astype(np.float64) @ q.T + [3.0, -2.0, 0.5]).astype(np.float32)
    assert TU.gap_ok(moved, t, thr)
    assert np.array_equal(TU.bond_matrix(moved, t, thr), TU.bond_matrix(p, t, thr)), "the motion's rounding moved a bond"
    P, T, sizes = TU.join([(p, t), (p[perm], t[perm]), (moved, t)])
    rc, got = TU.host(_lib.lib(), P, T, sizes, 2, thr, pairs=[[0, 1], [0, 2]])
    assert rc == 0 and got["fp"][0].sum() > 500
    assert np.array_equal(got["fp"][0], got["fp"][1]) and np.array_equal(got["fp"][0], got["fp"][2])
    assert got["sim"].tolist() == [1.0, 1.0] and np.array_equal(got["fp"][0], want["fp"][6])


def test_argument_errors_return_einval():
    L = _lib.lib()
    pos, types = TU.cloud(1, [5, 4], 2)
    err = lambda **kw: (TU.host(L, kw.get("pos", pos), kw.get("types", types), kw.get("sizes", [5, 4]), kw.get("A", 2),
                                kw.get("thr", THR2), L=kw.get("L", 30), pairs=kw.get("pairs"))[0], L.egnn_last_error())
    assert err()[0] == 0
    for kw, word in ((dict(A=5, thr=np.ones((5, 5))), b"atom types"), (dict(types=np.full(9, 2, np.int32)), b"has type 2"),
                     (dict(types=np.full(9, -1, np.int32)), b"has type -1"), (dict(L=0), b"max_length 0"), (dict(L=65), b"max_length 65"),
                     (dict(thr=np.array([[1.0, 0.0], [0.0, 1.0]])), b"threshold [0][1]"), (dict(thr=-THR2), b"threshold [0][0]"),
                     (dict(thr=np.array([[1.0, 1.0], [1.0, np.inf]])), b"threshold [1][1]"),
                     (dict(thr=np.array([[np.nan, 1.0], [1.0, 1.0]])), b"threshold [0][0]"), (dict(pairs=[[0, 2]]), b"names row 2"),
                     (dict(pos=np.zeros((1025, 3), np.float32), types=np.zeros(1025, np.int32), sizes=[1025]), b"1025 atoms (at most 1024")):
        rc, msg = err(**kw)
        assert rc == EINVAL and word in msg, (kw.keys(), msg)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    gp = np.array([0, 5, 9], np.int32)
    out = [np.zeros(400, np.int32) for _ in range(4)]
    full = [2, 2, vp(pos), vp(types), vp(gp), vp(THR2), 30] + [vp(o) for o in out] + [None] * 4 + [0, None, None, None, None]
    assert L.egnn_topo_host(*full) == 0
    for k in (2, 3, 4, 5, 7, 8, 9, 10):                                    # a required pointer missing
        args = list(full)
        args[k] = None
        assert L.egnn_topo_host(*args) == EINVAL and b"bad egnn_topo_host arguments" in L.egnn_last_error(), k
    args = list(full)
    args[15] = 1                                                           # a pair without its arrays
    assert L.egnn_topo_host(*args) == EINVAL

    # the device entries refuse the same arguments before they launch anything (no GPU is touched here)
    p, t2 = C.c_void_p(64), vp(THR2)
    bad_thr = np.array([[1.0, -1.0], [1.0, 1.0]])
    bonds = lambda B=1, N=8, A=2, pos=p, type=p, gp=p, mx=8, thr=t2, rp=p, nb=p, deg=p, over=p: \
        L.egnn_topo_bonds(None, B, N, A, pos, type, gp, mx, thr, rp, nb, deg, over)
    paths = lambda B=1, N=8, A=2, type=p, gp=p, mx=8, rp=p, nb=p, deg=p, over=p, Lmax=30, dist=None, dptr=None: \
        L.egnn_topo_paths(None, B, N, A, type, gp, mx, rp, nb, deg, over, Lmax, dist, dptr, p, p, p)
    for call, word in ((lambda: bonds(A=5), b"5 atom types"), (lambda: bonds(mx=1025), b"1025 atoms"), (lambda: bonds(thr=vp(bad_thr)), b"threshold [0][1]"),
                       (lambda: bonds(thr=None), b"thr given"), (lambda: bonds(pos=None), b"bad egnn_topo_bonds"), (lambda: bonds(type=None), b"bad egnn_topo_bonds"),
                       (lambda: bonds(gp=None), b"bad egnn_topo_bonds"), (lambda: bonds(rp=None), b"bad egnn_topo_bonds"), (lambda: bonds(nb=None), b"bad egnn_topo_bonds"),
                       (lambda: bonds(deg=None), b"bad egnn_topo_bonds"), (lambda: bonds(over=None), b"bad egnn_topo_bonds"), (lambda: bonds(B=0), b"bad egnn_topo_bonds"),
                       (lambda: bonds(N=0), b"0 atoms"), (lambda: paths(A=0), b"0 atom types"), (lambda: paths(mx=2000), b"2000 atoms"),
                       (lambda: paths(Lmax=0), b"max_length 0"), (lambda: paths(Lmax=65), b"max_length 65"), (lambda: paths(rp=None), b"bad egnn_topo_paths"),
                       (lambda: paths(nb=None), b"bad egnn_topo_paths"), (lambda: paths(deg=None), b"bad egnn_topo_paths"), (lambda: paths(over=None), b"bad egnn_topo_paths"),
                       (lambda: paths(type=None), b"bad egnn_topo_paths"), (lambda: paths(dist=p), b"dist_ptr given")):
        assert call() == EINVAL and word in L.egnn_last_error(), (word, L.egnn_last_error())
    for args in ((0, 10, p, 1, p, 1, None, p, p, p), (1, 0, p, 1, p, 1, None, p, p, p), (1, 10, None, 1, p, 1, None, p, p, p),
                 (1, 10, p, 1, None, 1, None, p, p, p), (1, 10, p, 0, p, 1, None, p, p, p), (1, 10, p, 1, p, 1, None, None, p, p),
                 (1, 10, p, 1, p, 1, None, p, None, p), (1, 10, p, 1, p, 1, None, p, p, None)):
        assert L.egnn_topo_tanimoto(None, *args) == EINVAL and b"bad egnn_topo_tanimoto" in L.egnn_last_error(), args


# ---- sanitizers ---------------------------------------------------------------------------------------------------------------------
def test_topo_host_under_sanitizers(tmp_path):
    """the executable links its own sanitizer runtime (statically), so nothing is preloaded"""
    r = build_and_run(tmp_path, "topo_main", ["eval/topo_host.cpp", "host_logic.cpp"])
    assert r.returncode == 0 and "TOPO-OK" in r.stdout, f"rc={r.returncode}\nstdout:\n{r.stdout}\nstderr:\n{r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]

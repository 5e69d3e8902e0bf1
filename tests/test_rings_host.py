"""Shortest-path ring statistics on the host (egnn_rings_host: csrc/eval/rings_host.cpp over the definitions the kernel compiles,
csrc/eval/rings_math.h), without a GPU:

  * known answers by restatement (i) of tests/_ring_util.py and by the host statement: beta-cristobalite and its triclinic
    distortion have (size, count) = (12, 2) through all 6 angles of every Si and (12, 6) through the one angle of every O, where a
    search that ignores the lattice shifts finds (8, 3) and (8, 9); the chain cell and the star have angles without a ring, the
    one-atom cell has no angle, ring(6) / ring(5) have (6, 1) / (5, 1), the crowd (33 bonds per atom) is reported as overflowed;
  * restatement (i) equals the independent check (ii) -- scipy shortest paths and integer adjacency-matrix powers on the explicit
    ball about the centre -- on every centre of the random 65- and 160-atom cells at cutoff 2.8 A and of the clouds at scale 1.5,
    and each fixture shows at least 5 distinct ring sizes, a count above 1 and an angle without a ring;
  * the host statement equals (i) EXACTLY in every integer output and in the histogram, on all of these, on mixed batches, on a
    centre list with duplicates and at max_size 3, 4, 12, 32;
  * the site limit: max_sites = L (the largest number of sites a search of a Si centre of cristobalite labels, taken from (i))
    succeeds, L - 1 marks those centres overflowed with size -1; the count saturates at 2^31 - 1 on a layered graph with 8^12 paths;
    the fan graph (2,594 sites labelled through levels of 1,024, the limit at 2,594 / 2,593) and the dense cells with 24-26 and
    exactly 32 bonds per atom equal (i) as well;
  * bad arguments return EGNN_EINVAL with a message naming the cause, from the host statement and -- before a GPU is touched --
    from the device entry;
  * the host statement runs clean under AddressSanitizer + UBSan as a stand-alone program (tests/host/rings_main.cpp)."""
import ctypes as C
import functools

import numpy as np
import pytest

from diffusion_model_amd import _lib
from tests import _cells_util as CU
from tests import _ring_util as RU
from tests import _topo_util as TU
from tests._host_program import build_and_run

EINVAL = -22


@functools.lru_cache(maxsize=None)
def _cells():
    return dict(chain=CU.chain_cell(), cristobalite=CU.cristobalite_cell(), triclinic=CU.triclinic_cell(), r65=CU.random_cell(65, 11),
                r160=CU.random_cell(160, 12), one=CU.one_atom_cell())


@functools.lru_cache(maxsize=None)
def _csr(name):
    """name -> (csr, max_size): the fixtures of this file"""
    if name in ("r65", "r160"):
        return RU.cells_csr([_cells()[name]], cutoff=2.8), 12
    if name == "cloud":
        pos, types = TU.cloud(3, TU.SIZES, 2)
        return RU.clusters_csr(pos, types, TU.SIZES, 2, scale=1.5), 16
    if name in ("ring6", "ring5", "star8", "crowd34"):
        pos, types = TU.special_graphs()[name]
        return RU.clusters_csr(pos, types, [len(types)], 2), 16
    if name == "mixed":
        return RU.cells_csr([_cells()[k] for k in ("chain", "cristobalite", "triclinic", "r65", "r160", "one")]), 16
    if name == "mixed-reversed":
        return RU.cells_csr([_cells()[k] for k in ("chain", "cristobalite", "triclinic", "r65", "r160", "one")][::-1]), 16
    return RU.cells_csr([_cells()[name]]), 16


@functools.lru_cache(maxsize=None)
def _restated(name, max_size=None):
    csr, default = _csr(name)
    return RU.restated(csr, max_size=default if max_size is None else max_size)


def _host(csr, **kw):
    rc, got = RU.host(_lib.lib(), csr, **kw)
    assert rc == 0, _lib.lib().egnn_last_error()
    return got


def _per_centre(res, m):
    lo, hi = res["angle_ptr"][m], res["angle_ptr"][m + 1]
    return list(zip(res["size"][lo:hi].tolist(), res["count"][lo:hi].tolist()))


# ---- known answers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cristobalite", "triclinic"])
def test_cristobalite_has_only_six_membered_rings(name):
    csr, _ = _csr(name)
    for res in (_restated(name), _host(csr)):
        for m in range(24):
            want = [(12, 2)] * 6 if csr["types"][m] == 1 else [(12, 6)]
            assert _per_centre(res, m) == want, (name, m)
        assert res["hist"][0].tolist() == [0] * 12 + [16] + [0] * 4 and res["hist"][1].tolist() == [0] * 12 + [48] + [0] * 4
    blind = RU.restated(csr, ignore_shifts=True)                           # what ignoring the lattice shifts would find
    for m in range(24):
        assert _per_centre(blind, m) == ([(8, 3)] * 6 if csr["types"][m] == 1 else [(8, 9)]), (name, m)


def test_small_fixtures():
    for res in (_restated("chain"), _host(_csr("chain")[0])):
        assert _per_centre(res, 1) == [(0, 0)] and _per_centre(res, 0) == [(0, 0)]
    for res in (_restated("one"), _host(_csr("one")[0])):
        assert len(res["size"]) == 0 and res["angle_ptr"].tolist() == [0, 0]
    for name, k in (("ring6", 6), ("ring5", 5)):
        for res in (_restated(name), _host(_csr(name)[0])):
            assert [_per_centre(res, m) for m in range(k)] == [[(k, 1)]] * k
    for res in (_restated("star8"), _host(_csr("star8")[0])):
        assert _per_centre(res, 0) == [(0, 0)] * 28 and len(res["size"]) == 28
    crowd, _ = _csr("crowd34")
    assert np.all(np.diff(crowd["row_ptr"]) == 33)
    for res in (_restated("crowd34"), _host(crowd)):
        assert np.all(res["overflow"] == 1) and np.all(res["size"] == -1) and np.all(res["count"] == 0) and len(res["size"]) == 34 * 528
        assert not res["hist"].any()


# ---- (i) against (ii) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["r65", "r160", "cloud"])
def test_search_restatement_equals_the_independent_check(name):
    csr, max_size = _csr(name)
    res = _restated(name)
    assert np.diff(csr["row_ptr"]).max() <= 12 and not res["overflow"].any()
    for m in range(csr["N"]):
        assert RU.independent(csr, m, max_size) == _per_centre(res, m), (name, m)
    sizes = set(res["size"].tolist())
    assert len(sizes - {0}) >= 5 and res["count"].max() > 1 and 0 in sizes, (sizes, res["count"].max())
    if csr["shift"] is not None:                                             # the lattice shifts matter on these cells
        blind = RU.restated(csr, max_size=max_size, ignore_shifts=True)
        assert sum(_per_centre(blind, m) != _per_centre(res, m) for m in range(csr["N"])) >= 10


# ---- the host statement against (i) --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain", "cristobalite", "triclinic", "one", "r65", "r160", "cloud", "ring6", "ring5", "star8", "crowd34",
                                  "mixed", "mixed-reversed"])
def test_host_statement_equals_the_restatement(name):
    RU.assert_equal(_host(_csr(name)[0], max_size=_csr(name)[1]), _restated(name))


@pytest.mark.parametrize("max_size", [3, 4, 12, 32])
def test_host_statement_equals_the_restatement_at_every_max_size(max_size):
    for name in ("r65", "cloud", "triclinic"):
        want = _restated(name, max_size)
        assert want["size"].max() <= max_size
        RU.assert_equal(_host(_csr(name)[0], max_size=max_size), want)


def test_host_statement_on_a_centre_list_with_duplicates():
    csr, _ = _csr("mixed")
    centres = np.random.default_rng(5).integers(0, csr["N"], 60)
    centres[7] = centres[3]
    RU.assert_equal(_host(csr, centres=centres, max_size=12), RU.restated(csr, centres=centres, max_size=12))


# ---- limits -----------------------------------------------------------------------------------------------------------------------------
def test_site_limit():
    csr, _ = _csr("cristobalite")
    si = np.nonzero(csr["types"] == 1)[0]
    full = RU.restated(csr, centres=si, max_size=16)
    L = int(full["labelled"].max())
    assert 64 < L < 1024 and np.all(full["labelled"] == L)
    RU.assert_equal(_host(csr, centres=si, max_size=16, max_sites=L), full)
    short = RU.restated(csr, centres=si, max_size=16, max_sites=L - 1)
    assert np.all(short["overflow"] == 1) and np.any(short["size"] == -1)
    got = _host(csr, centres=si, max_size=16, max_sites=L - 1)
    RU.assert_equal(got, short)
    assert np.all(got["count"][got["size"] == -1] == 0)


def test_count_saturates():
    csr, true, size = RU.layered_csr()
    assert true == 8 ** 12 >= 2 ** 31 and np.diff(csr["row_ptr"]).max() <= 17
    want = RU.restated(csr, centres=[0], max_size=16)
    assert want["size"].tolist() == [size] and want["count"].tolist() == [2 ** 31 - 1]
    RU.assert_equal(_host(csr, centres=[0], max_size=16), want)
    RU.assert_equal(_host(csr, max_size=16), RU.restated(csr, max_size=16))


# ---- beyond one workgroup of sites: the fan graph, and bond rows at the degree limit --------------------------------------------------
def test_fan_graph_labels_more_than_2048_sites():
    """one search labels 2,594 sites through levels of 1,024 -- a frontier four times the device's workgroup, slot numbers above
    2^12, a table a third full -- and fits exactly at max_sites = the number labelled"""
    csr, layer = RU.fan_csr()
    deg = np.diff(csr["row_ptr"])
    assert deg.max() == 32 and np.all(deg[layer[-1]] == 32)                                # passed sites at the degree limit
    want = RU.restated(csr, centres=[0], max_size=16)
    labelled = int(want["labelled"][0])
    assert 2048 < labelled <= 4096 and labelled == csr["N"] - 1 and max(RU.level_widths(csr, 0, 0)) > 256
    home = RU.home_slots(range(1, csr["N"]), 8192)                                          # the table at max_sites > 2048
    assert np.sum(np.bincount(home, minlength=8192) > 1) >= 100 and home.max() >= 4096      # probe chains; slots beyond 12 bits
    assert want["size"].tolist() == [len(layer) + 3] and 1 < want["count"][0] < RU.COUNT_MAX and not want["overflow"].any()
    for max_sites in (labelled, 4096):
        RU.assert_equal(_host(csr, centres=[0], max_size=16, max_sites=max_sites), want)
    short = RU.restated(csr, centres=[0], max_size=16, max_sites=labelled - 1)
    assert short["overflow"].tolist() == [1] and short["size"].tolist() == [-1]
    RU.assert_equal(_host(csr, centres=[0], max_size=16, max_sites=labelled - 1), short)
    centres = RU.fan_centres(layer)
    inside = RU.restated(csr, centres=centres, max_size=16)
    assert inside["labelled"].max() > 2048 and inside["count"].max() > 1 and len(set(inside["size"].tolist()) - {0}) >= 4
    RU.assert_equal(_host(csr, centres=centres, max_size=16), inside)


@pytest.mark.parametrize("name", ["g80", "g27"])
def test_host_statement_equals_the_restatement_at_the_degree_limit(name):
    """the dense cells of tests/_cells_util.py: 24-26 bonds per atom, and exactly 32 -- the limit, not the overflow"""
    c = CU.dense_cells()[name]
    csr = RU.cells_csr([c], cutoff=c["cutoff"])
    deg = np.diff(csr["row_ptr"])
    assert (deg.min() >= 24 and deg.max() <= 32) if name == "g80" else np.all(deg == 32)
    centres = RU.dense_ring_centres(name)
    want = RU.restated(csr, centres=centres, max_size=16)
    assert not want["overflow"].any() and want["labelled"].min() > 256 and want["size"].min() >= 3 and want["count"].max() > 1
    RU.assert_equal(_host(csr, centres=centres, max_size=16), want)


# ---- argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_einval():
    L = _lib.lib()
    csr, _ = _csr("cristobalite")
    assert RU.host(L, csr)[0] == 0

    def refused(word, **kw):
        assert RU.host(L, csr, **kw)[0] == EINVAL, (word, kw)
        assert word in L.egnn_last_error(), (word, L.egnn_last_error())

    refused(b"max_size 2", max_size=2)
    refused(b"max_size 33", max_size=33)
    refused(b"max_sites 0", max_sites=0)
    refused(b"max_sites 4097", max_sites=4097)
    for k in ("row_ptr", "atom", "types", "centre", "angle_ptr", "size", "count", "overflow"):
        refused(b"bad egnn_rings_host arguments", raw={k: None, "E": len(csr["atom"])})
    refused(b"outside the 24 atoms", centres=[3, 24])
    refused(b"outside the 24 atoms", centres=[-1])
    rp = csr["row_ptr"].copy()
    rp[5], rp[6] = rp[6], rp[5]
    refused(b"non-monotone row_ptr", raw=dict(row_ptr=rp))
    at = csr["atom"].copy()
    at[17] = 24
    refused(b"neighbour 24 outside [0, 24)", raw=dict(atom=at))
    at[17] = -1
    refused(b"neighbour -1 outside [0, 24)", raw=dict(atom=at))
    sh = csr["shift"].copy()
    sh[9, 1] = 2
    refused(b"shift component outside", raw=dict(shift=sh))
    refused(b"type 2 outside", raw=dict(types=np.full(24, 2, np.int32)))
    refused(b"angle_ptr", raw=dict(angle_ptr=np.zeros(25, np.int32)))

    # the device entry refuses the same arguments before it touches a GPU (none is here)
    p = C.c_void_p(64)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    ctr = np.arange(24, dtype=np.int32)
    E = len(csr["atom"])

    def dev(max_size=16, max_sites=4096, null=None, row_ptr=csr["row_ptr"], atom=csr["atom"], shift=csr["shift"], centre=ctr):
        args = [None, 24, p, E, p, p, p, 2, 24, p, p, 80, max_size, max_sites, p, p, p, p, vp(row_ptr), vp(atom), vp(shift), vp(centre)]
        if null is not None:
            args[null] = None
        return L.egnn_rings(*args)

    for kw, word in ((dict(max_size=2), b"max_size 2"), (dict(max_size=33), b"max_size 33"), (dict(max_sites=0), b"max_sites 0"),
                     (dict(max_sites=4097), b"max_sites 4097"), (dict(centre=np.array([24] * 24, np.int32)), b"outside the 24 atoms"),
                     (dict(row_ptr=rp), b"non-monotone row_ptr"), (dict(atom=at), b"neighbour -1 outside [0, 24)"),
                     (dict(shift=sh), b"shift component outside")):
        assert dev(**kw) == EINVAL and word in L.egnn_last_error(), (kw, L.egnn_last_error())
    for k in (2, 4, 6, 9, 10, 14, 15, 16):
        assert dev(null=k) == EINVAL and b"bad egnn_rings arguments" in L.egnn_last_error(), k


# ---- sanitizers ---------------------------------------------------------------------------------------------------------------------
def test_rings_host_under_sanitizers(tmp_path):
    """the executable links its own sanitizer runtime (statically), so nothing is preloaded"""
    r = build_and_run(tmp_path, "rings_main", ["eval/rings_host.cpp", "host_logic.cpp"])
    assert r.returncode == 0 and "RINGS-OK" in r.stdout, f"rc={r.returncode}\nstdout:\n{r.stdout}\nstderr:\n{r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]

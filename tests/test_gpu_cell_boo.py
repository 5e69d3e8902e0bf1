"""The bond-orientational order of periodic cells on the device (csrc/cells/cell_boo.hip through diffusion_model_amd.cells:
bond_order, bond_order_profile) against
  * the host statement egnn_cell_boo_host, which tests/test_cell_boo_host.py pins to the truth, the analytic anchors and the numpy
    restatement without a GPU: BITWISE -- the kernels execute the host statement's operations in its order (only +, -, *, /, sqrt,
    no contraction), so every float64 and every count must agree exactly;
  * the truth tests/golden/cell_boo_golden.npz (mpmath at 50 digits, complex basis) with the project's rule: the bar is 8 x E_host
    per fixture, E_host measured by the CPU test and capped at 1e-12 there; n and n_solid exactly.
Shapes are the smallest at which a kernel can go wrong: rows of 0, 1, 15, 16, 17 (the staged chunk of 16 sites of pass 1), 63, 64, 65
and 129 (the wave steps of pass 2) kept sites, reached by the radius and again through ``select`` with a longer raw row; image boxes
4, 2 and 1; l_max = 0, 1, 10.  Every input first passes the gap check: no site within 1e-9 (relative) of the cutoff.
"""
import functools

import numpy as np
import pytest
import torch

import diffusion_model_amd as dma
from diffusion_model_amd import _lib, cells as DC
from tests import _cell_boo_util as BU
from tests import _cell_grid_util as GU
from tests import _cell_soap_util as CSU

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = BU.FIELDS + ("n", "n_solid")


def _periodic(c, A=None):
    return dma.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=c["A"] if A is None else A, id=c.get("name"))


def _np(bo, qlm=False):
    out = {k: getattr(bo, k).cpu().numpy() for k in KEYS if getattr(bo, k) is not None}
    if qlm:
        out["qlm"] = bo.qlm.cpu().numpy()
    return out


def _same(got, want, keys=KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, float(np.abs(got[k] - want[k]).max()))


def _device_and_host(cells, cutoff, pairs, A, **kw):
    """bond_order of every atom of a batch of cell dicts == the host statement, bitwise -> the device's arrays"""
    rc, want = BU.host(_lib.lib(), cells, cutoff, pairs, A, l_max=kw.get("l_max", BU.L_MAX), l_solid=kw.get("l_solid", BU.L_SOLID),
                       threshold=kw.get("threshold", BU.THRESHOLD))
    assert rc == 0, _lib.lib().egnn_last_error()
    kw = dict(dict(l_max=BU.L_MAX, l_solid=BU.L_SOLID, threshold=BU.THRESHOLD, return_qlm=True, device=DEV), **kw)
    got = _np(DC.bond_order([_periodic(c, A) for c in cells], cutoff=cutoff, select=pairs, **kw), qlm=True)
    _same(got, want, KEYS + ("qlm",))
    return got


# ---- 1. the fixtures: host statement and truth ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,A", BU.CASES)
def test_a_fixture_alone_equals_host_and_truth(name, A):
    cell, cutoff, pairs = BU.checked_case(name, A)
    got, want = _device_and_host([cell], cutoff, pairs, A), BU.truth(name, A)
    assert np.array_equal(got["n"], want["n"]) and np.array_equal(got["n_solid"], want["n_solid"])
    E = BU.error(got, want)
    print(f"cell BOO {name} A={A}: device error {E:.3e}, bar {8 * BU.e_host(name):.3e}")
    assert E <= 8 * BU.e_host(name)
    again = _np(DC.bond_order(_periodic(cell, A), cutoff=cutoff, l_max=BU.L_MAX, select=pairs, device=DEV))
    _same(again, got)                                                  # two runs: the same bits
    if name == "crist34":                                              # n = 0 (O under the Si-Si select) beside n = 4
        assert got["n"].tolist() == [4] * 8 + [0] * 16 and np.all(got["q"][8:] == 0.0) and np.all(got["q_avg"][8:] == 0.0)
    if name == "one":                                                  # its own images only
        assert got["n"].tolist() == [6] and got["n_solid"].tolist() == [6]


def test_the_fixtures_in_one_batch_keep_their_bits():
    """one call, one select (the thin fixture's at A = 3), boxes 1 (no site), 4 / 1 / 2 and 1: every cell as alone"""
    thin, cutoff, pairs = BU.checked_case("thin", 3)
    cells = [BU.fixture("one", 1), thin, GU.displaced_cristobalite(1), BU.fixture("one", 1)]
    got = _device_and_host(cells, cutoff, pairs, 3)
    ptr = np.concatenate([[0], np.cumsum([len(c["frac"]) for c in cells])])
    for c, cell in enumerate(cells):
        alone = _np(DC.bond_order(_periodic(cell, 3), cutoff=cutoff, l_max=BU.L_MAX, select=pairs, return_qlm=True, device=DEV), qlm=True)
        _same({k: v[ptr[c]:ptr[c + 1]] for k, v in got.items()}, alone, KEYS + ("qlm",))
    assert BU.error({k: v[1:13] for k, v in got.items()}, BU.truth("thin", 3)) <= 8 * BU.e_host("thin")
    assert got["n"][0] == 0 and got["n"][-1] == 0 and np.all(got["q_avg"][0] == 0.0)


# ---- 2. row lengths at the chunk of pass 1 and the wave step of pass 2 ------------------------------------------------------------------
CENTRE = 8      # an oxygen of the displaced cristobalite


@functools.lru_cache(maxsize=None)
def _distances():
    cell = GU.displaced_cristobalite(1)
    j, _, r = CSU.sites(cell, 10.5, CENTRE)
    return np.sqrt((r * r).sum(1)), cell["types"][j]


def _radius_for(length, site_type=None):
    """a radius that keeps exactly ``length`` sites (of ``site_type``) about CENTRE, midway between two of their distances and at
    least 1e-9 (relative) from every site distance"""
    d, t = _distances()
    own = np.sort(d if site_type is None else d[t == site_type])
    radius = 0.5 * own[0] if length == 0 else 0.5 * (own[length - 1] + own[length])
    if length == 0 and site_type is not None:
        assert d.min() < own[0]
        radius = 0.5 * (d.min() + own[0])       # past the nearest site of the other type: the raw row is not empty
    assert np.abs(d - radius).min() > 1e-9 * radius, "a site on the cutoff"
    return float(radius)


@pytest.mark.parametrize("length", [0, 1, 15, 16, 17, 63, 64, 65, 129])
def test_row_lengths_by_radius(length):
    got = _device_and_host([GU.displaced_cristobalite(1)], _radius_for(length), None, 2)
    assert got["n"][CENTRE] == length


@pytest.mark.parametrize("length", [0, 1, 15, 16, 17, 63, 64, 65, 129])
def test_row_lengths_through_select(length):
    """oxygen sites only about oxygen centres: the raw row holds the silicon sites too"""
    radius = _radius_for(length, site_type=0)
    got = _device_and_host([GU.displaced_cristobalite(1)], radius, [(0, 0)], 2)
    d, _ = _distances()
    assert got["n"][CENTRE] == length and int((d < radius).sum()) > length and np.all(got["n"][:8] == 0)


# ---- 3. centres, options, l_max ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,A", [("thin", 2), ("crist34", 2)])
def test_centres_as_all_a_type_and_a_scrambled_list(name, A):
    cell, cutoff, pairs = BU.checked_case(name, A)
    pc, n = _periodic(cell, A), len(cell["frac"])
    kw = dict(cutoff=cutoff, l_max=BU.L_MAX, select=pairs, return_qlm=True, device=DEV)
    full = _np(DC.bond_order(pc, **kw), qlm=True)
    scrambled = np.random.default_rng(2).permutation(n)
    scrambled = np.concatenate([scrambled, scrambled[:1]])
    for centres, listed in ((1, np.nonzero(cell["types"] == 1)[0]), (torch.from_numpy(scrambled), scrambled)):
        bo = DC.bond_order(pc, centres=centres, **kw)
        _same(_np(bo, qlm=True), {k: v[listed] for k, v in full.items()}, KEYS + ("qlm",))
        assert np.array_equal(bo.centre_atom.numpy(), listed) and np.all(bo.centre_cell.numpy() == 0)
    empty = DC.bond_order(pc, centres=torch.zeros(0, dtype=torch.long), **kw)
    assert empty.q.shape == (0, BU.L_MAX + 1) and empty.n.shape == (0,)
    sliced = _np(DC.bond_order(pc, _slab_bytes=8 * 300, **kw), qlm=True)      # a few centres a slab
    _same(sliced, full, KEYS + ("qlm",))


def test_without_the_averages():
    cell, cutoff, pairs = BU.checked_case("thin", 2)
    full = BU.host_on_golden("thin", 2)
    bo = DC.bond_order(_periodic(cell, 2), cutoff=cutoff, l_max=BU.L_MAX, select=pairs, averaged=False, device=DEV)
    assert bo.q_avg is None and bo.w_avg is None and bo.w_hat_avg is None and bo.qlm is None
    _same(_np(bo), full, ("q", "w", "w_hat", "n", "n_solid"))


@pytest.mark.parametrize("l_max", [0, 1, 6])
def test_l_max_below_the_limit(l_max):
    cell, cutoff, pairs = BU.checked_case("thin", 2)
    got = _device_and_host([cell], cutoff, pairs, 2, l_max=l_max, l_solid=l_max)
    assert got["q"].shape == (12, l_max + 1) and got["qlm"].shape == (12, (l_max + 1) ** 2)
    assert np.allclose(got["q"][:, 0], 1.0, atol=1e-15)


def test_select_forms_agree():
    cell, cutoff, pairs = BU.checked_case("thin", 3)
    pc = _periodic(cell, 3)
    kw = dict(cutoff=cutoff, l_max=4, l_solid=4, device=DEV)
    want = _np(DC.bond_order(pc, select=pairs, **kw))
    mask = np.zeros((3, 3), dtype=bool)
    for a, b in pairs:
        mask[a, b] = True
    _same(_np(DC.bond_order(pc, select=mask, **kw)), want)
    _same(_np(DC.bond_order(pc, select="same", **kw)), _np(DC.bond_order(pc, select=[(0, 0), (1, 1), (2, 2)], **kw)))
    _same(_np(DC.bond_order(pc, select=None, **kw)), _np(DC.bond_order(pc, select=np.ones((3, 3), dtype=bool), **kw)))


# ---- 4. direct and grid routes ----------------------------------------------------------------------------------------------------------
def test_direct_and_grid_routes_give_the_same_bits():
    cell = GU.displaced_cristobalite(2)
    direct = _device_and_host([cell], BU.THIN_CUT, [(1, 1)], 2, method="direct")
    grid = _np(DC.bond_order(_periodic(cell), cutoff=BU.THIN_CUT, l_max=BU.L_MAX, select=[(1, 1)], return_qlm=True, method="grid", device=DEV),
               qlm=True)
    assert direct["n"][:3].tolist() == [4, 4, 4]
    _same(grid, direct, KEYS + ("qlm",))
    with pytest.raises(ValueError, match="not griddable"):
        DC.bond_order(_periodic(GU.displaced_cristobalite(1)), cutoff=BU.THIN_CUT, method="grid", device=DEV)


def test_a_mixed_batch_routes_cell_by_cell(monkeypatch):
    """"auto" with the threshold lowered: the 192-atom cell goes through the grid, the thin cell through the site kernels"""
    monkeypatch.setattr(DC, "_GRID_MIN_ATOMS", 100)
    cells = [CSU.fixture("thin", 2), GU.displaced_cristobalite(2)]
    pcs = [_periodic(c) for c in cells]
    kw = dict(cutoff=BU.THIN_CUT, l_max=6, select=[(1, 1)], return_qlm=True, device=DEV)
    auto, direct = DC.bond_order(pcs, method="auto", **kw), DC.bond_order(pcs, method="direct", **kw)
    _same(_np(auto, qlm=True), _np(direct, qlm=True), KEYS + ("qlm",))
    listed = torch.tensor([200, 3, 13, 200])
    _same(_np(DC.bond_order(pcs, centres=listed, method="auto", **kw)), {k: v[listed.numpy()] for k, v in _np(direct).items()})


# ---- 5. the profile ---------------------------------------------------------------------------------------------------------------------
def test_bond_order_profile():
    cells = [GU.displaced_cristobalite(1), CSU.fixture("thin", 2)]
    pcs = [_periodic(c) for c in cells]
    kw = dict(cutoff=3.4, l_max=6, select=[(1, 1)], device=DEV)
    prof = DC.bond_order_profile(pcs, bins=20, **kw)
    bo = _np(DC.bond_order(pcs, **kw))
    types = np.concatenate([c["types"] for c in cells])
    cell_of = np.repeat([0, 1], [24, 12])
    for c in range(2):
        for a in range(2):
            rows = np.nonzero((cell_of == c) & (types == a))[0]
            assert int(prof["count"][c, a]) == len(rows) and len(rows) > 0
            for key, src in (("q_mean", "q"), ("q_avg_mean", "q_avg"), ("w_hat_mean", "w_hat")):
                acc = np.zeros(7)
                for m in rows:
                    acc = acc + bo[src][m]
                assert np.array_equal(prof[key][c, a].numpy(), acc / float(len(rows))), (c, a, key)
            assert np.all(prof["q_avg_hist"][c, a].sum(-1).numpy() == len(rows))
            want = np.mean(bo["n_solid"][rows] >= bo["n"][rows])
            assert abs(float(prof["solid_fraction"][c, a]) - want) < 1e-15
    assert prof["q_avg_hist"].shape == (2, 2, 7, 20)
    for c in range(2):
        alone = DC.bond_order_profile(pcs[c], bins=20, **kw)
        for key in prof:
            assert torch.equal(alone[key][0], prof[key][c]), (c, key)
    strict = DC.bond_order_profile(pcs[0], min_solid=4, bins=20, **kw)
    assert float(strict["solid_fraction"][0, 0]) == 0.0                # an oxygen has no kept site, hence no solid bond


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    thin = _periodic(CSU.fixture("thin", 2))
    for kw in (dict(l_max=11), dict(l_max=-1), dict(l_solid=7), dict(l_solid=-1), dict(select="other"), dict(select=[(0, 2)]),
               dict(select=np.ones((3, 3), dtype=bool)), dict(method="fast"), dict(cutoff=5.3), dict(cutoff=float("nan"))):
        with pytest.raises(ValueError):
            DC.bond_order(thin, device=DEV, **{"cutoff": BU.THIN_CUT, **kw})
    with pytest.raises(ValueError, match="widths"):
        DC.bond_order(thin, cutoff=5.3, device=DEV)
    L, t = _lib.lib(), torch.zeros(64, dtype=torch.float64, device=DEV)
    p, i32 = _lib.ptr(t), _lib.ptr(torch.zeros(8, dtype=torch.int32))
    lat = torch.eye(3, dtype=torch.float64).reshape(9)
    for l_max, A, mask, want in ((11, 1, 1, b"l_max"), (2, 5, 1, b"atom types"), (2, 1, 2, b"select")):
        rc = L.egnn_cell_boo_qlm(_lib.stream_ptr(), 1, 0, A, i32, _lib.ptr(lat), p, p, p, p, 1.0, mask, l_max, p, 1, p, 0, None, None, 1, p, p, p, p)
        assert rc == -22 and want in L.egnn_last_error()

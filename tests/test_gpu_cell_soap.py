"""The SOAP descriptors of periodic cells on the device (csrc/cells/cell_soap.hip through diffusion_model_amd.cells: neighbour_sites,
soap_descriptors, average_soap, soap_similarity) against
  * the host statements egnn_cell_sites_host / egnn_cell_soap_host and the numpy restatement tests/_cell_soap_util.py, which
    tests/test_cell_soap_host.py pins to each other and to the truth without a GPU: site lists bitwise;
  * the truth tests/golden/cell_soap_golden.npz (mpmath at 60 digits) with the project's rule: the bar is 8 x E_host, E_host
    measured by the CPU test and capped at 1e-7 there; and the host statement within the same bar;
  * the cluster kernel (soap.soap_descriptors) on an explicit cluster whose vectors are exact in fp32: bitwise, the two kernels run
    one text after the staging (csrc/eval/soap_device.h);
  * the linked-cell route (method="grid") and cells.bond_list: bitwise.
Shapes are the smallest at which a kernel can go wrong: rows of 0, 63, 64, 65 and above 128 sites for the wave steps of the site
kernels; 30 .. 33, 63, 64 sites for the chunks of 32 of the descriptor kernel (the centre makes 31 .. 34, 64, 65); image boxes 4, 2
and 1.  Every input first passes the gap check: no site within 1e-9 (relative) of the cut.
"""
import functools

import numpy as np
import pytest
import torch

import diffusion_model_amd as dma
from diffusion_model_amd import _lib, cells as DC, soap as DS
from tests import _cell_grid_util as GU
from tests import _cell_soap_util as CSU
from tests import _cells_util as CU
from tests import _soap_util as SU

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = CSU.golden()
SMALL_CUT, DEFAULT_CUT = SU.neighbour_cut(SU.CONFIGS["small"]), SU.neighbour_cut(SU.CONFIGS["default"])


def _periodic(c, A=None):
    return dma.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=c["A"] if A is None else A, id=c["name"])


@functools.lru_cache(maxsize=None)
def _basis(cfg):
    return dma.SoapBasis(**SU.CONFIGS[cfg])


def _np(sl):
    return tuple(t.cpu().numpy() for t in (sl.row_ptr, sl.atom, sl.shift_code))


def _same_rows(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def _check_sites(cells, radius, centres, listed, method="direct"):
    """device == host statement == restatement, bitwise; ``centres`` is what the device is given, ``listed`` the same as indices"""
    want = CSU.site_lists(cells, radius, listed)
    assert want[3] > 1e-9, "ambiguous input: a site on the cut"
    rc, *host = CSU.host_sites(_lib.lib(), cells, radius, listed)
    assert rc == 0, _lib.lib().egnn_last_error()
    sl = DC.neighbour_sites([_periodic(c) for c in cells], radius, centres=centres, method=method, device=DEV)
    got = _np(sl)
    assert got[0].dtype == np.int32 and _same_rows(got, host) and _same_rows(got, want[:3])
    assert np.array_equal(sl.shift.cpu().numpy(), CU.shift_decode(got[2]))
    ptr = np.concatenate([[0], np.cumsum([len(c["frac"]) for c in cells])])
    cell_of = np.searchsorted(ptr, listed, side="right") - 1
    assert np.array_equal(sl.centre_cell.numpy(), cell_of) and np.array_equal(sl.centre_atom.numpy(), np.asarray(listed) - ptr[cell_of])
    return got


# ---- 1. site lists ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CSU.FIXTURES))
def test_site_lists_of_a_fixture_alone(name):
    cell, centres, cut = CSU.checked_fixture(name, CSU.FIXTURES[name][1][-1])
    n = len(cell["frac"])
    row_ptr, atom, code = _check_sites([cell], cut, None, np.arange(n))
    listed = G[f"{name}_centres"]
    keys = [atom[row_ptr[i]:row_ptr[i + 1]].astype(np.int64) * 729 + code[row_ptr[i]:row_ptr[i + 1]] for i in listed]
    assert np.array_equal(np.concatenate(keys), G[f"{name}_keys"]), "the truth's site keys"
    scrambled = np.random.default_rng(1).permutation(n)
    scrambled = np.concatenate([scrambled, scrambled[:1]])
    _check_sites([cell], cut, torch.from_numpy(scrambled), scrambled)
    for t in range(cell["A"]):
        _check_sites([cell], cut, t, np.nonzero(cell["types"] == t)[0])


def test_site_lists_of_the_fixtures_in_one_batch():
    cells = [CSU.fixture("one"), CSU.fixture("thin", 2), GU.displaced_cristobalite(1), CSU.fixture("one")]
    cells[0]["A"] = cells[3]["A"] = 2
    N = sum(len(c["frac"]) for c in cells)
    _check_sites(cells, SMALL_CUT, None, np.arange(N))        # boxes 1 (no site), 4 / 1 / 2, 1
    types = np.concatenate([c["types"] for c in cells])
    _check_sites(cells, SMALL_CUT, 1, np.nonzero(types == 1)[0])
    listed = np.array([N - 1, 30, 5, 0, 13, 5, 37])
    _check_sites(cells, SMALL_CUT, listed.tolist(), listed)
    sl = DC.neighbour_sites([_periodic(c) for c in cells], SMALL_CUT, centres=torch.zeros(0, dtype=torch.long), device=DEV)
    assert sl.row_ptr.tolist() == [0] and sl.num_sites == 0


@functools.lru_cache(maxsize=None)
def _crist_distances(centre):
    """the sorted site distances of fixture (b) about one centre, out to the default cut"""
    _, _, r = CSU.sites(GU.displaced_cristobalite(1), DEFAULT_CUT, centre)
    return np.sort(np.sqrt((r * r).sum(1)))


def _radius_for(centre, length):
    """a radius that gives ``centre`` of fixture (b) a row of exactly ``length`` sites, midway between two site distances"""
    d = _crist_distances(centre)
    radius = 0.5 * d[0] if length == 0 else 0.5 * (d[length - 1] + d[length])
    assert (length == 0 or d[length - 1] < radius * (1 - 1e-9)) and d[length] > radius * (1 + 1e-9), "two sites too close to separate"
    return float(radius)


@pytest.mark.parametrize("length", [0, 63, 64, 65, 129])
def test_row_lengths_at_the_wave_steps(length):
    cell = GU.displaced_cristobalite(1)
    radius = _radius_for(8, length)
    row_ptr, _, _ = _check_sites([cell], radius, None, np.arange(24))
    assert row_ptr[9] - row_ptr[8] == length


# ---- 2. direct and grid routes ------------------------------------------------------------------------------------------------------
def test_direct_and_grid_routes_give_the_same_bits():
    cell = GU.displaced_cristobalite(2)
    pc = _periodic(cell)
    direct = _np(DC.neighbour_sites(pc, SMALL_CUT, method="direct", device=DEV))
    grid = _np(DC.neighbour_sites(pc, SMALL_CUT, method="grid", device=DEV))
    bonds = DC.bond_list(pc, cutoff=SMALL_CUT, device=DEV, method="direct")
    assert len(direct[1]) > 192 * 15 and _same_rows(direct, grid) and _same_rows(direct, _np(bonds))
    listed = torch.tensor([191, 0, 77, 77, 3])
    assert _same_rows(_np(DC.neighbour_sites(pc, SMALL_CUT, centres=listed, method="direct", device=DEV)),
                      _np(DC.neighbour_sites(pc, SMALL_CUT, centres=listed, method="grid", device=DEV)))
    a = DC.soap_descriptors(pc, basis=_basis("small"), method="direct", device=DEV)
    b = DC.soap_descriptors(pc, basis=_basis("small"), method="grid", device=DEV)
    assert a.shape == (192, SU.features(2, 3, 2)) and torch.equal(a, b)
    with pytest.raises(ValueError, match="not griddable"):
        DC.neighbour_sites(_periodic(GU.displaced_cristobalite(1)), SMALL_CUT, method="grid", device=DEV)


def test_a_mixed_batch_routes_cell_by_cell(monkeypatch):
    """"auto" with the threshold lowered: the 192-atom cell goes through the grid, the thin cell and the 24-atom cell (not
    griddable) through the site kernels, in one call; every row equals the direct route's"""
    monkeypatch.setattr(DC, "_GRID_MIN_ATOMS", 100)
    cells = [CSU.fixture("thin", 2), GU.displaced_cristobalite(2), GU.displaced_cristobalite(1)]
    pcs = [_periodic(c) for c in cells]
    listed = torch.tensor([203, 5, 12, 100, 227, 100, 0, 204])
    for centres in (None, listed, 1):
        want = _np(DC.neighbour_sites(pcs, SMALL_CUT, centres=centres, method="direct", device=DEV))
        assert _same_rows(_np(DC.neighbour_sites(pcs, SMALL_CUT, centres=centres, method="auto", device=DEV)), want)
    a = DC.soap_descriptors(pcs, centres=listed, basis=_basis("small"), method="direct", device=DEV)
    assert torch.equal(DC.soap_descriptors(pcs, centres=listed, basis=_basis("small"), method="auto", device=DEV), a)


# ---- 3. accuracy --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,A", [(name, A) for name, (_, As, _) in CSU.FIXTURES.items() for A in As])
def test_descriptors_against_the_truth_and_the_host_statement(name, A):
    cfg = CSU.FIXTURES[name][0]
    cell, centres, _ = CSU.checked_fixture(name, A)
    bar = CSU.bar(cfg)
    desc, coeff = DC.soap_descriptors(_periodic(cell, A), centres=torch.from_numpy(centres.astype(np.int64)), basis=_basis(cfg),
                                      return_coefficients=True, device=DEV)
    desc, coeff = desc.cpu().numpy(), coeff.cpu().numpy()
    host_desc, host_coeff = CSU.host_on_golden(name, A)
    E, Eh = SU.descriptor_error(desc, G[f"{name}_A{A}_desc"]), SU.descriptor_error(desc, host_desc)
    Ech = SU.descriptor_error(coeff, host_coeff)
    print(f"cell SOAP {name} A={A} ({cfg}): device against truth {E:.3e}, against host {Eh:.3e} (coefficients {Ech:.3e}); bar {bar:.3e}")
    assert desc.shape == (len(centres), SU.features(A, SU.CONFIGS[cfg]["n_max"], SU.CONFIGS[cfg]["l_max"]))
    assert E <= bar and Eh <= bar and Ech <= bar
    if f"{name}_A{A}_coeff" in G.files:
        Ec = SU.descriptor_error(coeff, G[f"{name}_A{A}_coeff"])
        print(f"cell SOAP {name} A={A} ({cfg}): coefficients against truth {Ec:.3e}")
        assert Ec <= bar


# ---- 4. the same text as the cluster kernel -------------------------------------------------------------------------------------------
def test_cell_kernel_equals_the_cluster_kernel_on_exact_vectors():
    rng = np.random.default_rng(21)
    grid = rng.permutation(64 ** 3)[:58]
    frac = np.stack([grid // 4096, grid // 64 % 64, grid % 64], 1) / 64.0
    cell = dict(lattice=8.0 * np.eye(3), frac=frac, types=rng.integers(0, 2, 58).astype(np.int32), A=2, name="exact")
    centres = np.array([0, 17, 57, 17])
    pos, onehot, sizes = [], [], []
    for i in centres:                                           # the explicit cluster: the centre first, then ascending key
        j, _, r = CSU.sites(cell, SMALL_CUT, i)
        assert 25 <= len(j) <= 60, len(j)
        p = np.concatenate([np.zeros((1, 3)), r])
        assert np.array_equal(p.astype(np.float32).astype(np.float64), p), "a vector that float32 does not hold"
        pos.append(p.astype(np.float32))
        onehot.append(np.eye(2, dtype=np.int64)[np.concatenate([[cell["types"][i]], cell["types"][j]])])
        sizes.append(len(p))
    basis = _basis("small")
    want, want_c = DS.soap_descriptors(torch.from_numpy(np.concatenate(pos)).to(DEV), torch.from_numpy(np.concatenate(onehot)).to(DEV), sizes,
                                       centres="first", basis=basis, return_coefficients=True)
    got, got_c = DC.soap_descriptors(_periodic(cell), centres=torch.from_numpy(centres), basis=basis, return_coefficients=True, device=DEV)
    assert torch.equal(got, want) and torch.equal(got_c, want_c)


# ---- 5. chunk phases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [30, 31, 32, 33, 63, 64])
def test_chunk_boundary_on_and_next_to_the_last_site(length):
    cell = GU.displaced_cristobalite(1)
    radius = _radius_for(0, length)
    pc, basis, centre = _periodic(cell), _basis("default"), torch.tensor([0])
    sl = DC.neighbour_sites(pc, radius, centres=centre, device=DEV)
    assert sl.num_sites == length
    kw = dict(centres=centre, basis=basis, neighbour_cut=radius, device=DEV)
    desc, coeff = DC.soap_descriptors(pc, return_coefficients=True, **kw)
    again, coeff_again = DC.soap_descriptors(pc, return_coefficients=True, **kw)
    alone = DC.soap_descriptors(pc, **kw)                       # a NULL coefficient pointer
    assert torch.equal(desc, again) and torch.equal(coeff, coeff_again) and torch.equal(desc, alone)
    rc, host_desc, host_coeff = CSU.host_soap(_lib.lib(), [cell], 2, SU.CONFIGS["default"], SU.tables("default")[1], [0], cut=radius)
    assert rc == 0, _lib.lib().egnn_last_error()
    E, Ec, bar = SU.descriptor_error(desc.cpu().numpy(), host_desc), SU.descriptor_error(coeff.cpu().numpy(), host_coeff), CSU.bar("default")
    print(f"cell SOAP row of {length} sites: device against host {E:.3e} (coefficients {Ec:.3e}); bar {bar:.3e}")
    assert E <= bar and Ec <= bar


# ---- 6. images are handled, not folded ------------------------------------------------------------------------------------------------
def test_an_atom_sees_the_same_environment_in_a_supercell():
    cell = GU.displaced_cristobalite(1)
    off = np.array([[i, j, k] for i in range(2) for j in range(2) for k in range(2)], dtype=np.float64)
    big = dict(lattice=2.0 * cell["lattice"], frac=((CU.wrap(cell["frac"])[None] + off[:, None]) / 2.0).reshape(-1, 3),
               types=np.tile(cell["types"], 8), A=2, name="cristobalite-2x")
    assert CSU.box(cell["lattice"], DEFAULT_CUT).tolist() == [2, 2, 2] and CSU.box(big["lattice"], DEFAULT_CUT).tolist() == [1, 1, 1]
    centres, basis, bar = torch.tensor([8, 0]), _basis("default"), CSU.bar("default")
    small = DC.soap_descriptors(_periodic(cell), centres=centres, basis=basis, device=DEV).cpu().numpy()
    large = DC.soap_descriptors(_periodic(big), centres=centres, basis=basis, device=DEV).cpu().numpy()
    E = SU.descriptor_error(large, small)
    print(f"cell SOAP 1x1x1 (box 2) against 2x2x2 (box 1): {E:.3e}; bar 2 x {bar:.3e}")
    assert E <= 2 * bar
    # whole lattice vectors added to fractions that stay exact under the addition (multiples of 2^-40): the same bits
    exact = dict(cell, frac=np.round(cell["frac"] * 2.0 ** 40) / 2.0 ** 40)
    shifted = dict(exact, frac=exact["frac"] + np.random.default_rng(2).integers(-3, 4, exact["frac"].shape))
    assert np.array_equal(CU.wrap(shifted["frac"]), CU.wrap(exact["frac"])) and not np.array_equal(shifted["frac"], exact["frac"])
    a = DC.soap_descriptors(_periodic(exact), centres=centres, basis=basis, device=DEV)
    assert torch.equal(DC.soap_descriptors(_periodic(shifted), centres=centres, basis=basis, device=DEV), a)


# ---- 7. mean and similarity -----------------------------------------------------------------------------------------------------------
def _two_per_slab(pcs, basis):
    run = DC._CellSoap(pcs, basis, None, "direct", DEV)
    budget = next(b for b in range(64, 1 << 20, 64) if run.slab_centres(False, b) == 2)
    return budget


def test_average_is_the_running_sum_in_centre_order_for_any_slab():
    cells = [CSU.fixture("thin", 2), CSU.fixture("one"), CU.chain_cell(), GU.displaced_cristobalite(1)]
    cells[1]["A"] = 2
    pcs, basis = [_periodic(c) for c in cells], _basis("small")
    ptr = np.concatenate([[0], np.cumsum([len(c["frac"]) for c in cells])])
    types = np.concatenate([c["types"] for c in cells])
    budget = _two_per_slab(pcs, basis)
    for centres in (None, 0, 1):
        idx = np.arange(ptr[-1]) if centres is None else np.nonzero(types == centres)[0]
        rows = DC.soap_descriptors(pcs, centres=torch.from_numpy(idx), basis=basis, device=DEV).cpu().numpy()
        want, count = CSU.running_mean(rows, np.searchsorted(ptr, idx, side="right") - 1, len(cells))
        mean, n = DC.average_soap(pcs, centres=centres, basis=basis, device=DEV)
        assert n.dtype == torch.int64 and n.tolist() == count.tolist() and np.array_equal(mean.cpu().numpy(), want)
        slabbed, n2 = DC.average_soap(pcs, centres=centres, basis=basis, device=DEV, _slab_bytes=budget)
        assert torch.equal(slabbed, mean) and torch.equal(n2, n)
        assert torch.equal(DC.soap_descriptors(pcs, centres=torch.from_numpy(idx), basis=basis, device=DEV, _slab_bytes=budget).cpu(),
                           torch.from_numpy(rows))
        if centres == 1:                                        # the one-atom cell holds no atom of type 1
            assert count[1] == 0 and np.all(want[1] == 0.0)
    alone, _ = DC.average_soap(pcs[0], basis=basis, device=DEV)  # a cell gives the same bits in any batch
    assert torch.equal(alone[0], DC.average_soap(pcs, basis=basis, device=DEV)[0][0])


def test_similarity_of_cells():
    ideal, moved = CU.cristobalite_cell(), GU.displaced_cristobalite(1)
    one = CSU.fixture("one")
    one["A"] = 2
    a, b = [_periodic(ideal), _periodic(moved), _periodic(one)], [_periodic(ideal), _periodic(ideal), _periodic(one)]
    basis, bar = _basis("small"), CSU.bar("small")
    same = DC.soap_similarity(a, a, basis=basis, device=DEV).cpu().numpy()
    assert same.shape == (3,) and np.all(np.abs(same - 1.0) <= 4 * np.finfo(np.float64).eps)
    sim = DC.soap_similarity(a, b, basis=basis, device=DEV).cpu().numpy()
    ma, mb = (DC.average_soap(x, basis=basis, device=DEV)[0].cpu().numpy() for x in (a, b))
    want = SU.cosine(ma, mb)
    print(f"cell SOAP similarity: ideal/ideal {sim[0]:.17g}, displaced/ideal {sim[1]:.17g}, against numpy {np.abs(sim - want).max():.3e}")
    assert sim[1] < 1.0 and np.all(np.abs(sim - want) <= 4 * bar)
    typed = DC.soap_similarity(a, b, centres=1, basis=basis, device=DEV).cpu().numpy()
    assert np.isnan(typed[2]) and np.isfinite(typed[:2]).all()
    _, count = DC.average_soap(a, centres=1, basis=basis, device=DEV)
    assert count.tolist() == [8, 8, 0]


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------
def test_python_errors():
    thin, crist = _periodic(CSU.fixture("thin", 2)), _periodic(GU.displaced_cristobalite(1))
    basis = _basis("small")
    w = CU.widths(CSU.thin_cell()["lattice"])
    with pytest.raises(ValueError, match=rf"cell 1: perpendicular widths {w[0]:.6g}, {w[1]:.6g}, {w[2]:.6g}"):
        DC.neighbour_sites([crist, thin], DEFAULT_CUT, device=DEV)
    with pytest.raises(ValueError, match="cell 0: perpendicular widths"):
        DC.soap_descriptors(thin, basis=_basis("default"), device=DEV)
    with pytest.raises(ValueError, match="singular"):
        DC.neighbour_sites(dma.PeriodicCell([[1, 0, 0], [0, 1, 0], [2, 0, 0]], [[0, 0, 0]], types=[0]), 2.0, device=DEV)
    with pytest.raises(ValueError, match="same number of cells"):
        DC.soap_similarity([thin, crist], [thin], basis=basis, device=DEV)
    with pytest.raises(ValueError, match="number of atom types"):
        DC.soap_similarity([thin], [_periodic(CSU.fixture("thin", 3))], basis=basis, device=DEV)
    for call in (lambda: DC.neighbour_sites(thin, SMALL_CUT, device="cpu"), lambda: DC.soap_descriptors(thin, basis=basis, device="cpu"),
                 lambda: DC.average_soap(thin, basis=basis, device="cpu")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for call in (lambda: DC.neighbour_sites(thin, SMALL_CUT, method="fast", device=DEV),
                 lambda: DC.soap_descriptors(thin, basis=basis, method="fast", device=DEV)):
        with pytest.raises(ValueError, match="method must be one of"):
            call()
    with pytest.raises(ValueError, match="type index"):
        DC.average_soap(thin, centres=torch.tensor([0, 1]), basis=basis, device=DEV)
    with pytest.raises(ValueError, match="outside the"):
        DC.soap_descriptors(thin, centres=torch.tensor([12]), basis=basis, device=DEV)
    with pytest.raises(ValueError, match="atom types"):
        DC.soap_descriptors(dma.PeriodicCell(5.0 * np.eye(3), [[0, 0, 0]], types=[4]), basis=basis, device=DEV)

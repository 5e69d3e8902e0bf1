"""cells.lattice_energy(..., stress=True) on the device (csrc/cells/cell_ewald.hip, section 5) against the truth of the fixtures
(tests/golden/cell_stress_golden.npz) and the host statement egnn_cell_ewald_virial_host, at the smallest shapes at which a kernel
can go wrong: rows of 0 .. 129 sites, 0 .. 257 vectors, 1 .. 1,025 atoms, image boxes 1, 2 and 4 / 1 / 2, both site searches, with
and without charges and pair potential.

The bar of a value is 8 x E of the host statement on the same case against the same truncated sums in mpmath (the project's
bar); everything is bitwise reproducible and the same alone, in a batch and through any slab, and the outputs the energy had before
keep their bits with ``stress`` on."""
import functools

import numpy as np
import pytest
import torch

from diffusion_model_amd import _lib, cells
from tests import _cell_ewald_util as EU
from tests import _cell_grid_util as GU
from tests import _cell_soap_util as CSU
from tests import _cell_stress_util as XU
from tests import _sq_util as SQU

pytestmark = pytest.mark.gpu
FLOOR = 1e-16         # an E_host of exactly 0 (a case of no term) still allows the rounding of one operation
ENERGY = ("energy", "components", "energy_per_atom", "components_per_atom", "forces")
STRESS = ("strain_derivative", "strain_derivative_components", "strain_derivative_per_atom", "stress", "pressure")


def _cell(c, A=None):
    return cells.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=c["A"] if A is None else A)


def run(cases, stress=True, **kw):
    """cells.lattice_energy on the cells of ``cases`` with the parameters of the first"""
    c0, A = cases[0], max(c["cell"]["A"] for c in cases)
    pot = None if c0["pot"] is None else cells.PairTable(*c0["pot"], n=c0["n"])
    return cells.lattice_energy([_cell(c["cell"], A) for c in cases], c0["charges"], pot, r_cut=c0["r_cut"], short_cut=c0["short_cut"],
                                shift=c0["shift"], alpha=c0["alpha"], k_max=c0["k_max"], coulomb_constant=c0["kappa"], stress=stress, **kw)


def of_cell(res, cases, c):
    """the stress outputs of cell ``c`` in Voigt order, as the dict tests/_cell_stress_util.error reads"""
    ptr = np.concatenate([[0], np.cumsum([len(k["cell"]["types"]) for k in cases])])
    lo, hi = int(ptr[c]), int(ptr[c + 1])
    forms = [res.strain_derivative[c], res.strain_derivative_components[c], res.strain_derivative_per_atom[lo:hi], res.stress[c]]
    for f in forms:
        assert torch.equal(f, f.transpose(-1, -2)), "xy and yx are not the same bits"
    D, comp, atom, sigma = (XU.voigt(f.cpu().numpy()) for f in forms)
    return dict(per_atom=atom, components=comp, strain=D, stress=sigma, pressure=res.pressure[c].cpu().numpy())


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def energy_bits(res):
    return {k: None if getattr(res, k) is None else getattr(res, k).cpu().numpy() for k in ENERGY}


@functools.lru_cache(maxsize=None)
def host_and_bar(key):
    """-> (case, host statement of the cell, truth, 8 E_host) of a case built by ``CASES[key]``: computed once"""
    case = CASES[key]()
    rc, h = XU.host(_lib.lib(), [case])
    assert rc == 0, _lib.lib().egnn_last_error()
    member = EU.exact(case, wider=1 if len(case["cell"]["types"]) <= 256 else 0)     # the library's box is complete: a wider one only checks it
    assert member["gap"] > EU.GAP, (key, float(member["gap"]))
    ex, h0 = XU.exact_stress(case, ex=member), XU.of_cell(h, [case], 0)
    return case, h0, ex, 8 * max(XU.error(h0, ex), FLOOR)


def check_against_host(key):
    case, h, ex, bar = host_and_bar(key)
    res = run([case])
    got = of_cell(res, [case], 0)
    E = XU.error(got, dict(ex, **{k: h[k] for k in got}))
    print(f"{key}: E(device, host) = {E:.3e}  bar = {bar:.3e}")
    assert E <= bar
    return case, h, res, got


# ---- the small cells of the edge cases ----------------------------------------------------------------------------------------------------
def small_cell(n=8, seed=21, A=2):
    """n atoms in the triclinic lattice of the thin fixture (widths 1.14 / 4.74 / 3.1 A: no two reciprocal vectors of one length)"""
    rng = np.random.default_rng(seed)
    return dict(lattice=CSU.thin_cell()["lattice"], frac=rng.uniform(-0.5, 1.5, (n, 3)), types=rng.integers(0, A, n).astype(np.int32), A=A,
                name=f"small{n}")


def cut_for_row(cell, length, most=4.5):
    """a radius at which some centre has exactly ``length`` sites, midway between two consecutive site distances (an atom's own
    images come in pairs of one distance: the first centre whose two distances differ is taken)"""
    for centre in range(len(cell["types"])):
        _, _, r = CSU.sites(cell, most, centre)
        d = np.sort(np.sqrt(EU._norm2(r)))
        if d[length] - d[length - 1] > 1e-6:
            return float(0.5 * (d[length - 1] + d[length]))
    raise AssertionError(f"no centre with a row of {length} sites")


def k_for_vectors(cell, count):
    """a k_max below which the cell has exactly ``count`` half-space vectors"""
    hkl, k2 = SQU.box_candidates(cell["lattice"], 14.0)
    k = np.sort(np.sqrt(k2[SQU.half_space(hkl)]))
    assert count == 0 or k[count] - k[count - 1] > 1e-6
    return float(0.5 * ((k[count - 1] if count else 0.0) + k[count]))


def random_cell(n, seed, a):
    rng = np.random.default_rng(seed)
    return dict(lattice=np.array([[a, 0.0, 0.0], [0.1 * a, a, 0.0], [0.0, -0.2 * a, 1.1 * a]]), frac=rng.uniform(0.0, 1.0, (n, 3)),
                types=rng.integers(0, 2, n).astype(np.int32), A=2, name=f"random{n}")


def soft_tables():
    """the tables of the thin fixture without the D / r^n term and with C / 1000: the atoms of the small cells come as close as
    0.2 A, and the pair terms must not drown the Coulomb terms in the error scale"""
    pot = EU.generic_tables(2, 1)
    pot[2], pot[3] = pot[2] / 1000.0, 0.0
    return pot


def _row_case(length):
    cell = small_cell()
    return EU.make_case(cell, (-1.1, 2.3), soft_tables(), r_cut=cut_for_row(cell, length), shift=True, alpha=0.8, k_max=5.0)


def _vector_case(count):
    cell = small_cell()
    return EU.make_case(cell, (-1.1, 2.3), None, r_cut=2.0, alpha=1.0, k_max=k_for_vectors(cell, count))


def _atoms_case(n):
    a = 2.2 * n ** (1.0 / 3.0)          # about 0.09 atoms / A^3: a handful of sites inside 2.4 A, a handful of vectors below 1.3 k_min
    return EU.make_case(random_cell(n, 30 + n, a), (-1.0, 1.5), soft_tables(), r_cut=2.4, short_cut=2.0, alpha=0.9, k_max=1.3 * 2 * np.pi / a)


CASES = {f"row{n}": functools.partial(_row_case, n) for n in (1, 63, 64, 65, 129)}
CASES["row0"] = lambda: EU.make_case(EU.cube_cell(), (1.0,), None, r_cut=2.9, accuracy=1e-4)
CASES.update({f"vec{n}": functools.partial(_vector_case, n) for n in (0, 1, 63, 64, 65, 257)})
CASES.update({f"atoms{n}": functools.partial(_atoms_case, n) for n in (1, 63, 64, 65, _lib.EWALD_ATOM_CHUNK + 1)})
CASES["box1"] = lambda: EU.make_case(GU.displaced_cristobalite(1), EU.BKS_CHARGES, EU.bks_tables(), r_cut=3.1, short_cut=3.0, alpha=0.9, k_max=3.0)
CASES["coulomb"] = lambda: dict(EU.fixtures()["thin"], pot=None)
CASES["short"] = lambda: dict(EU.fixtures()["thin"], charges=np.zeros(2))


# ---- fixtures and truth -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EU.fixtures()))
def test_fixture_against_the_truth(name):
    case, want = EU.fixtures()[name], XU.truth(name)
    res = run([case])
    got = of_cell(res, [case], 0)
    E, bar = XU.error(got, want), 8 * XU.e_host(name)
    print(f"cell stress {name}: E(device) = {E:.3e}  bar 8 E_host = {bar:.3e}")
    assert E <= bar
    assert same_bits(of_cell(run([case]), [case], 0), got), "two runs differ"
    total = np.zeros(6)
    for row in got["per_atom"]:                                    # the cell's D: one ascending running sum over its atoms
        total = total + row
    assert np.array_equal(total, got["strain"])
    V = EU.volume(case["cell"]["lattice"])                         # the operation order of ewald_volume
    assert np.array_equal(got["strain"] / V, got["stress"])
    assert got["pressure"] == -(((got["stress"][0] + got["stress"][1]) + got["stress"][2]) / 3.0)
    assert np.all(got["components"][2] == 0.0)                     # self: 0
    assert res.strain_derivative.shape == (1, 3, 3) and res.strain_derivative_components.shape == (1, 5, 3, 3) and res.pressure.shape == (1,)
    assert res.strain_derivative_per_atom.shape == (len(case["cell"]["types"]), 3, 3) and res.stress.dtype == torch.float64
    bare = run([case], forces=False)                               # stress without forces: the same bits
    assert bare.forces is None and same_bits(of_cell(bare, [case], 0), got)
    if name == "thin":
        assert CSU.box(case["cell"]["lattice"], case["r_cut"]).tolist() == [4, 1, 2]      # triclinic, boxes 4 / 1 / 2
    if name == "crist":
        assert CSU.box(case["cell"]["lattice"], case["r_cut"]).tolist() == [2, 2, 2]


@pytest.mark.parametrize("name", ["thin", "crist"])
def test_existing_outputs_keep_their_bits(name):
    case = EU.fixtures()[name]
    on, off = run([case], stress=True), run([case], stress=False)
    assert all(getattr(off, k) is None for k in STRESS) and all(getattr(on, k) is not None for k in STRESS)
    a, b = energy_bits(on), energy_bits(off)
    assert all(np.array_equal(a[k], b[k]) for k in ENERGY)
    assert on.n_vectors.tolist() == off.n_vectors.tolist() and (on.alpha, on.k_max) == (off.alpha, off.k_max)


# ---- batching -----------------------------------------------------------------------------------------------------------------------------
def test_a_cell_gives_the_same_bits_in_any_batch_and_slab():
    base = EU.fixtures()["zero3"]                                  # three types: every fixture cell fits its tables
    cases = [dict(base, cell=EU.fixtures()[name]["cell"]) for name in EU.fixtures()]
    alone = [of_cell(run([dict(c, cell=dict(c["cell"], A=3))]), [c], 0) for c in cases]
    together = run(cases)
    slabs = run(cases, _slab_bytes=7 * 8 * cells._slab_sites(cells._CellBatch([_cell(c["cell"], 3) for c in cases], None), base["r_cut"]))
    for c in range(len(cases)):
        assert same_bits(of_cell(together, cases, c), alone[c]), c
        assert same_bits(of_cell(slabs, cases, c), alone[c]), c


# ---- rows, vectors, atoms, boxes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [0, 1, 63, 64, 65, 129])
def test_row_lengths(length):
    case, h, res, got = check_against_host(f"row{length}")
    rows = cells.neighbour_sites(_cell(case["cell"]), case["r_cut"]).row_ptr.cpu().numpy()
    assert length in np.diff(rows).tolist()


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_vector_counts(count):
    case, h, res, got = check_against_host(f"vec{count}")
    assert res.n_vectors.tolist() == [count]
    if count == 0:
        assert np.all(res.strain_derivative_components[:, 1].cpu().numpy() == 0.0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, _lib.EWALD_ATOM_CHUNK + 1])
def test_atoms_per_cell(n):
    case, h, res, got = check_against_host(f"atoms{n}")
    assert res.strain_derivative_per_atom.shape[0] == n and int(res.n_vectors[0]) > 0


def test_image_box_one():
    assert CSU.box(CASES["box1"]()["cell"]["lattice"], 3.1).tolist() == [1, 1, 1]      # boxes 2 and 4 / 1 / 2: the fixtures crist and thin
    check_against_host("box1")


# ---- methods ------------------------------------------------------------------------------------------------------------------------------
def test_grid_search_gives_the_bits_of_the_direct_search():
    case = EU.make_case(GU.displaced_cristobalite(3), EU.BKS_CHARGES, EU.bks_tables(), r_cut=5.0, short_cut=4.5, accuracy=1e-5)
    direct, grid = of_cell(run([case], method="direct"), [case], 0), of_cell(run([case], method="grid"), [case], 0)
    assert same_bits(direct, grid)
    assert np.all(np.isfinite(direct["strain"])) and np.all(direct["components"][4] != 0.0)


# ---- charges ------------------------------------------------------------------------------------------------------------------------------
def test_coulomb_only_and_short_only():
    thin = EU.fixtures()["thin"]
    full = of_cell(run([thin]), [thin], 0)
    case, h, res, got = check_against_host("coulomb")
    assert np.all(got["components"][4] == 0.0) and np.array_equal(got["components"][:4], full["components"][:4])      # the Coulomb blocks alone
    case, h, res, got = check_against_host("short")
    assert res.n_vectors.tolist() == [0]
    assert np.all(got["components"][:4] == 0.0) and np.array_equal(got["components"][4], full["components"][4])
    assert np.array_equal(got["strain"], got["components"][4])


# ---- coincident atoms -----------------------------------------------------------------------------------------------------------------------
def test_coincident_atoms_raise_naming_the_cell():
    good = EU.make_case(EU.cube_cell(5.0, [[0.25, 0.5, 0.75], [0.6, 0.1, 0.7]]), (1.0,), r_cut=6.0, accuracy=1e-4)
    bad = dict(good, cell=EU.cube_cell(5.0, [[0.25, 0.5, 0.75], [0.6, 0.1, 0.7], [1.25, 0.5, 0.75]]))
    with pytest.raises(ValueError, match="cell 1: coincident atoms"):
        run([good, bad, good])
    after = run([good])                                            # a flagged result, not a fault: the device goes on
    assert torch.isfinite(after.stress).all() and torch.isfinite(after.pressure).all()

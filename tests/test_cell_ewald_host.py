"""The lattice energy of periodic cells on the host (egnn_cell_ewald_host: csrc/cells/cell_ewald_host.cpp over the definitions the
kernels compile, csrc/cells/cell_ewald_math.h) against
  * the truth tests/golden/cell_ewald_golden.npz (the same truncated sums by mpmath at 50 digits): site and vector membership
    exactly, E_host = the largest |got - truth| / scale over atoms and outputs below the cap 1e-12 (measured: printed by the test,
    DESIGN.md 5.11);
  * the numpy restatement tests/_cell_ewald_util.restated (plain loops, the same orders);
  * analytic anchors at accuracy 1e-14: the Madelung constants of NaCl and CsCl and the energy of one charge in a unit cube;
  * what the sums must obey: no net force on a neutral cell, the same total at two r_cut, the shift, the short cut and the D / r^n
    term against direct sums.
Refusals of the host statement and of cells.lattice_energy (raised before a device is touched), and a stand-alone program under the
address and undefined-behaviour sanitizers.  No GPU.
"""
import numpy as np
import pytest

from diffusion_model_amd import _lib, cells
from tests import _cell_ewald_util as EU
from tests import _cells_util as CU

EINVAL = -22
NAMES = list(EU.fixtures())


@pytest.mark.parametrize("name", NAMES)
def test_host_against_the_truth(name):
    got, want = EU.host_on_golden(name), EU.truth(name)
    E = EU.e_host(name)
    print(f"cell Ewald {name}: E_host = {E:.3e}  sites = {got['n_sites'].min()}..{got['n_sites'].max()}  vectors = {int(got['n_vectors'][0])}")
    assert want["gap"] > EU.GAP
    assert E <= EU.CAP
    assert got["coincident"].tolist() == [0]
    assert not any(np.any(got[k] == -7.0) for k in ("energy", "components", "e_atom", "comp_atom", "force"))


@pytest.mark.parametrize("name", NAMES)
def test_membership_of_host_restatement_and_truth(name):
    got, want, mine = EU.host_on_golden(name), EU.truth(name), EU.restated(EU.fixtures()[name])
    assert np.array_equal(got["n_sites"], np.diff(want["row_ptr"])) and np.array_equal(mine["n_sites"], got["n_sites"])
    assert np.array_equal(np.concatenate([j for j, _ in mine["rows"]]), want["atom"])
    assert np.array_equal(np.concatenate([c for _, c in mine["rows"]]), want["code"])
    assert got["n_vectors"].tolist() == [len(want["hkl"])] and np.array_equal(mine["hkl"], want["hkl"])
    if name == "thin":
        from tests import _cell_soap_util as CSU
        assert CSU.box(EU.fixtures()[name]["cell"]["lattice"], 4.37).tolist() == [4, 1, 2]
    if name == "crist":
        assert got["n_sites"].min() > 129


@pytest.mark.parametrize("name", NAMES)
def test_host_against_the_restatement(name):
    got, mine = EU.host_on_golden(name), EU.restated(EU.fixtures()[name])
    bar = 8 * max(EU.e_host(name), 1e-16)
    want = dict(EU.truth(name), **{k: mine[k] for k in ("e_atom", "comp_atom", "force", "energy", "components")})
    assert EU.error(got, want) < bar


def test_analytic_anchors():
    L = _lib.lib()
    rc, nacl = EU.host(L, [EU.make_case(EU.nacl_cell(), (1.0, -1.0), r_cut=12.0, accuracy=1e-14, kappa=1.0)])
    assert rc == 0, L.egnn_last_error()
    assert abs(-nacl["energy"][0] / 4 * (5.64 / 2) - 1.7475645946) < 1e-9
    rc, cscl = EU.host(L, [EU.make_case(EU.cscl_cell(), (1.0, -1.0), r_cut=12.0, accuracy=1e-14, kappa=1.0)])
    assert rc == 0 and abs(-cscl["energy"][0] * (4.11 * np.sqrt(3.0) / 2) - 1.7626747731) < 1e-9
    rc, cube = EU.host(L, [EU.make_case(EU.cube_cell(1.0), (1.0,), r_cut=3.9, accuracy=1e-14, kappa=1.0)])
    assert rc == 0 and abs(2 * cube["energy"][0] + 2.8372974795) < 1e-9
    assert np.abs(cube["force"]).max() < 1e-12                    # a lattice of one atom: no force
    assert cube["comp_atom"][0, 3] < 0.0                              # the background of a charged cell


@pytest.mark.parametrize("name", ["crist", "nacl"])
def test_no_net_force_on_a_neutral_cell(name):
    got, want = EU.host_on_golden(name), EU.truth(name)
    assert np.all(np.abs(got["force"].sum(0)) <= EU.CAP * want["scale_f"].sum(0))


def test_two_cutoffs_give_the_same_total():
    L, acc = _lib.lib(), 1e-8
    runs = []
    for r_cut in (6.0, 7.9):
        rc, res = EU.host(L, [EU.make_case(EU.fixtures()["crist"]["cell"], EU.BKS_CHARGES, EU.bks_tables(), r_cut=r_cut, short_cut=5.5, accuracy=acc)])
        assert rc == 0, L.egnn_last_error()
        runs.append(res)
    bound = 10 * acc * np.abs(runs[0]["components"]).sum()
    print(f"two cutoffs: {runs[0]['energy'][0]:.12f} {runs[1]['energy'][0]:.12f}  bound {bound:.3e}")
    assert abs(runs[0]["energy"][0] - runs[1]["energy"][0]) <= bound
    assert runs[0]["components"][0, 4] == runs[1]["components"][0, 4]      # the short part does not see r_cut


def _short_direct(case, shift, short_cut, D=True):
    """the short component of a cell by a direct sum over the restated sites"""
    from tests import _cell_soap_util as CSU
    cell, A = case["cell"], case["cell"]["A"]
    pot = case["pot"].copy()
    if not D:
        pot[3] = 0.0
    c = dict(case, pot=pot, short_cut=short_cut, shift=shift)
    uc, total = EU.u_cut(c), 0.0
    for i in range(len(cell["types"])):
        j, _, r = CSU.sites(cell, case["r_cut"], i)
        d = np.sqrt(EU._norm2(r))
        for a, rr in zip(j, d):
            if rr < short_cut:
                ab = int(cell["types"][i]) * A + int(cell["types"][a])
                total += 0.5 * (EU.pair(c, ab, rr * rr, rr)[0] - uc[ab])
    return total


@pytest.mark.parametrize("shift,short_cut,D", [(True, 3.0, True), (False, 3.0, True), (True, 2.1, True), (True, 4.37, False), (False, 4.37, True)])
def test_shift_short_cut_and_power_term(shift, short_cut, D):
    L, case = _lib.lib(), EU.fixtures()["thin"]
    pot = case["pot"].copy()
    if not D:
        pot[3] = 0.0
    rc, got = EU.host(L, [case], shift=shift, short_cut=short_cut, pot=pot)
    assert rc == 0, L.egnn_last_error()
    want = _short_direct(case, shift, short_cut, D)
    assert abs(got["components"][0, 4] - want) <= 1e-12 * abs(want)
    base = EU.host_on_golden("thin")
    for k in (0, 1, 2, 3):                                            # the Coulomb parts do not see the pair potential
        assert got["components"][0, k] == base["components"][0, k]
    if (shift, short_cut, D) == (True, 3.0, True):
        assert np.array_equal(got["e_atom"], base["e_atom"])


def test_a_cell_gives_the_same_bits_in_any_batch_and_without_forces():
    L, case = _lib.lib(), EU.fixtures()["thin"]
    alone = EU.host_on_golden("thin")
    other = dict(case, cell=dict(EU.cube_cell(5.0, [[0.1, 0.2, 0.3], [0.6, 0.1, 0.7]]), A=2))
    rc, got = EU.host(L, [other, case, other])
    assert rc == 0, L.egnn_last_error()
    for k in ("e_atom", "comp_atom", "force", "n_sites"):
        assert np.array_equal(got[k][2:14], alone[k]), k
    assert got["energy"][1] == alone["energy"][0] and np.array_equal(got["components"][1], alone["components"][0])
    assert got["energy"][0] == got["energy"][2]
    rc, bare = EU.host(L, [case], forces=False)
    assert rc == 0 and np.array_equal(bare["e_atom"], alone["e_atom"]) and np.array_equal(bare["components"], alone["components"])


def test_zero_charges_leave_the_pair_potential_alone():
    L, case = _lib.lib(), EU.fixtures()["thin"]
    rc, got = EU.host(L, [case], charges=np.zeros(2))
    assert rc == 0 and got["n_vectors"].tolist() == [0]
    assert np.all(got["components"][0, :4] == 0.0) and got["components"][0, 4] == EU.host_on_golden("thin")["components"][0, 4]
    rc, coul = EU.host(L, [case], pot=None)
    assert rc == 0 and coul["components"][0, 4] == 0.0 and coul["components"][0, 0] == EU.host_on_golden("thin")["components"][0, 0]


def test_coincident_atoms_are_flagged():
    L = _lib.lib()
    cell = EU.cube_cell(5.0, [[0.25, 0.5, 0.75], [0.6, 0.1, 0.7], [1.25, 0.5, 0.75]])
    rc, got = EU.host(L, [EU.make_case(EU.cube_cell(5.0), (1.0,), r_cut=6.0), EU.make_case(cell, (1.0,), r_cut=6.0)])
    assert rc == 0 and got["coincident"].tolist() == [0, 1] and np.all(np.isfinite(got["energy"]))


def test_refusals_of_the_host_statement():
    L, case = _lib.lib(), EU.fixtures()["thin"]
    run = lambda cases=None, **kw: EU.host(L, cases or [case], **kw)[0]
    assert run() == 0
    assert run(short_cut=4.38) == EINVAL and b"short_cut" in L.egnn_last_error()
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert run(alpha=bad) == EINVAL and run(k_max=bad) == EINVAL and run(kappa=bad) == EINVAL and run(short_cut=bad) == EINVAL
    assert run(n=0) == EINVAL and run(n=65) == EINVAL and b"power" in L.egnn_last_error()
    assert run(A=5) == EINVAL and b"atom types" in L.egnn_last_error()
    assert run(charges=np.array([1.0, np.inf])) == EINVAL and b"charge" in L.egnn_last_error()
    pot = case["pot"].copy()
    pot[1, 0, 1] = np.nan
    assert run(pot=pot) == EINVAL and b"not finite" in L.egnn_last_error()
    pot = case["pot"].copy()
    pot[2, 0, 1] += 1.0
    assert run(pot=pot) == EINVAL and b"symmetric" in L.egnn_last_error()
    w = CU.widths(case["cell"]["lattice"])
    assert run(r_cut=4.0 * w.min() * (1 + 1e-12), short_cut=1.0) == EINVAL and b"cut / 4" in L.egnn_last_error()
    assert run(k_max=1025 * 2 * np.pi / 1.15) == EINVAL and b"Miller index" in L.egnn_last_error()
    nan = case["cell"]["frac"].copy()
    nan[3, 1] = np.inf
    assert run(cases=[dict(case, cell=dict(case["cell"], frac=nan))]) == EINVAL and b"not finite" in L.egnn_last_error()
    assert run(raw=dict(type=np.full(12, 2, np.int32))) == EINVAL and b"type" in L.egnn_last_error()


def test_refusals_of_lattice_energy_come_before_the_device():
    thin = EU.fixtures()["thin"]["cell"]
    cell = cells.PeriodicCell(thin["lattice"], thin["frac"], types=thin["types"], num_types=2)
    pot = cells.PairTable(*EU.fixtures()["thin"]["pot"][:3])
    with pytest.raises(ValueError, match="charges has 3 entries for 2 atom types"):
        cells.lattice_energy(cell, (1.0, 2.0, 3.0), r_cut=4.0)
    with pytest.raises(ValueError, match="short_cut > r_cut"):
        cells.lattice_energy(cell, (1.0, -1.0), pot, r_cut=4.0, short_cut=4.1)
    for acc in (0.0, 1.0, -1e-3, 2.0):
        with pytest.raises(ValueError, match="accuracy"):
            cells.lattice_energy(cell, (1.0, -1.0), r_cut=4.0, accuracy=acc)
    with pytest.raises(ValueError, match="cell 0: perpendicular widths"):
        cells.lattice_energy(cell, (1.0, -1.0), r_cut=4.7)
    with pytest.raises(ValueError, match="Miller index"):
        cells.lattice_energy(cell, (1.0, -1.0), r_cut=4.0, k_max=6000.0)
    with pytest.raises(ValueError, match="pair tables are"):
        cells.lattice_energy(cell, (1.0, -1.0), cells.PairTable([[1.0]], [[1.0]], [[1.0]]), r_cut=4.0)
    with pytest.raises(ValueError, match="not finite"):
        cells.PairTable([[1.0, np.nan], [np.nan, 1.0]], np.ones((2, 2)), np.ones((2, 2)))
    with pytest.raises(ValueError, match="not symmetric"):
        cells.PairTable([[1.0, 2.0], [3.0, 1.0]], np.ones((2, 2)), np.ones((2, 2)))
    with pytest.raises(ValueError, match="power n"):
        cells.PairTable(np.ones((2, 2)), np.ones((2, 2)), np.ones((2, 2)), n=0)


def test_bks_constants_and_defaults():
    assert cells.BKS.charges == (-1.2, 2.4)
    assert np.array_equal(cells.BKS.potential.tables(), EU.bks_tables()) and cells.BKS.potential.n == 24
    thin = EU.fixtures()["thin"]
    cell = cells.PeriodicCell(thin["cell"]["lattice"], thin["cell"]["frac"], types=thin["cell"]["types"], num_types=2)
    A, q, pot, n, r_cut, short_cut, alpha, k_max, kappa = cells._ewald_setup([cell], thin["charges"], None, 4.37, None, 1e-6, None, None, EU.KAPPA)
    assert (alpha, k_max, short_cut, kappa) == (thin["alpha"], thin["k_max"], 4.37, cells.COULOMB_CONSTANT) and pot is None


def test_cell_ewald_host_under_sanitizers(tmp_path):
    from tests._host_program import build_and_run
    r = build_and_run(tmp_path, "cell_ewald_main", ["cells/cell_ewald_host.cpp", "cells/cell_soap_host.cpp", "cells/cell_host.cpp",
                                                    "eval/sq_host.cpp", "host_logic.cpp"])
    assert r.returncode == 0 and "CELL-EWALD-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

"""The strain derivative of the lattice energy on the host (egnn_cell_ewald_virial_host: csrc/cells/cell_stress_host.cpp over the
definitions the kernels compile, csrc/cells/cell_stress_math.h) against
  * the truth tests/golden/cell_stress_golden.npz (the same truncated sums by mpmath at 50 digits, whose analytic D equals mpmath's
    numerical strain derivative of its own energy to DERIV_BOUND): E_host = the largest |got - truth| / scale over atoms, components
    and outputs below the cap 1e-12 (measured: printed by the test);
  * the numpy restatement tests/_cell_stress_util.restated (plain loops, the same orders);
  * what the sums must obey: Euler's theorem for a pure D / r^n table (tr D_short = -n E_short, membership held), the homogeneity
    of a converged Coulomb energy (tr D = -E: 3 P V = E) for NaCl, CsCl and one charge in a unit cube, the cubic symmetry of NaCl;
  * a central finite difference of the EXISTING egnn_cell_ewald_host over strained lattices, the only tie to earlier code.
The statement returns no energy output, so there is none to compare with egnn_cell_ewald_host.  Refusals of the host statement and
of cells.lattice_energy(..., stress=True) (raised before a device is touched), cells.strained, and a stand-alone program under the
address and undefined-behaviour sanitizers.  No GPU.

Measured on the CPU (x86-64, glibc), the bars below are 10 x these (libm differences between machines), under the caps stated:
  tr D + E:   NaCl 1.04e-13, CsCl 1.18e-13, unit cube 1.8e-14 (caps 1e-7 |E|);
  NaCl:       |D_aa - D_bb| 3.4e-16 at most, off-diagonals 2.3e-17 at most;
  difference: h = 1e-5, residual 1.12e-8 eV over the six directions (cap 1e-6 sum |components| = 5.4e-4 eV); at h >= 1e-4 sites
              cross short_cut inside the step (kinks of the shifted potential), at h <= 3e-6 the rounding of E / h takes over.
"""
import numpy as np
import pytest
import torch

from diffusion_model_amd import _lib, cells
from tests import _cell_ewald_util as EU
from tests import _cell_stress_util as XU
from tests import _cells_util as CU

EINVAL = -22
NAMES = list(EU.fixtures())
OUTPUTS = ("comp_atom", "per_atom", "components", "strain", "stress", "pressure")


@pytest.mark.parametrize("name", NAMES)
def test_host_against_the_truth(name):
    got, want = XU.host_on_golden(name), XU.truth(name)
    E = XU.e_host(name)
    print(f"cell stress {name}: E_host = {E:.3e}  pressure = {got['pressure'][0]:.9g} eV/A^3  derivative of the truth {float(want['deriv_error']):.1e}")
    assert EU.truth(name)["gap"] > EU.GAP                       # the condition recorded with the energy golden: the same inputs
    assert want["deriv_error"] <= XU.DERIV_BOUND                # a condition on the truth, not on the library
    assert E <= XU.CAP
    assert got["coincident"].tolist() == [0] and got["n_vectors"].tolist() == EU.host_on_golden(name)["n_vectors"].tolist()
    assert not any(np.any(got[k] == -7.0) for k in OUTPUTS)
    assert np.all(got["comp_atom"][:, 2] == 0.0) and np.all(got["components"][:, 2] == 0.0)          # self: 0
    assert np.all(got["comp_atom"][:, 3, 3:] == 0.0)                                                    # background: the diagonal only


@pytest.mark.parametrize("name", NAMES)
def test_host_against_the_restatement(name):
    case = EU.fixtures()[name]
    got, mine = XU.of_cell(XU.host_on_golden(name), [case], 0), XU.restated(case)
    want = dict(XU.truth(name), **{k: mine[k] for k in OUTPUTS})
    E = XU.error(got, want)
    print(f"cell stress {name}: E(host, restatement) = {E:.3e}")
    assert E <= 8 * max(XU.e_host(name), 1e-16)


def test_cell_sums_stress_and_pressure_follow_the_definitions():
    case = EU.fixtures()["crist"]
    got = XU.of_cell(XU.host_on_golden("crist"), [case], 0)
    run = np.zeros(6)
    for row in got["per_atom"]:
        run = run + row
    V = EU.volume(case["cell"]["lattice"])
    assert np.array_equal(run, got["strain"]) and np.array_equal(got["strain"] / V, got["stress"])
    assert got["pressure"] == -(((got["stress"][0] + got["stress"][1]) + got["stress"][2]) / 3.0)
    c = got["comp_atom"]
    assert np.array_equal((((c[:, 0] + c[:, 1]) + c[:, 2]) + c[:, 3]) + c[:, 4], got["per_atom"])


def test_euler_identity_of_a_pure_power_law():
    """charges 0, A = C = 0, a pure D / r^n table, no shift: every site term is 0.5 u' r = -(n / 2) D / r^n, so tr D_short =
    -n E_short with the membership held.  D > 0: all terms of both sums have one sign, the scale of the trace is n E_short itself."""
    L, thin = _lib.lib(), EU.fixtures()["thin"]
    pot = np.zeros_like(thin["pot"])
    pot[3] = thin["pot"][3]
    assert np.all(pot[3] > 0.0)
    kw = dict(charges=np.zeros(2), pot=pot, shift=False)
    rc, s = XU.host(L, [thin], **kw)
    assert rc == 0, L.egnn_last_error()
    rc, e = EU.host(L, [thin], **kw)
    assert rc == 0, L.egnn_last_error()
    trace, want = (s["components"][0, 4, 0] + s["components"][0, 4, 1]) + s["components"][0, 4, 2], -thin["n"] * e["components"][0, 4]
    scale = thin["n"] * e["components"][0, 4]
    print(f"Euler: tr D_short = {trace:.15g}  -n E_short = {want:.15g}  residual / scale = {abs(trace - want) / scale:.3e}")
    assert scale > 0.0 and abs(trace - want) <= 8 * XU.e_host("thin") * scale
    assert np.all(s["components"][0, :4] == 0.0) and np.array_equal(s["strain"][0], s["components"][0, 4])


def _anchor(cell, charges, r_cut):
    L = _lib.lib()
    case = EU.make_case(cell, charges, r_cut=r_cut, accuracy=1e-14, kappa=1.0)
    rc, s = XU.host(L, [case])
    assert rc == 0, L.egnn_last_error()
    rc, e = EU.host(L, [case])
    assert rc == 0, L.egnn_last_error()
    D, E = s["strain"][0], e["energy"][0]
    return D, E, abs(((D[0] + D[1]) + D[2]) + E), abs(3.0 * s["pressure"][0] * EU.volume(cell["lattice"]) - E)


def test_analytic_anchors():
    """a converged Coulomb energy is homogeneous of degree -1 in the lattice: tr D = -E, 3 P V = E (set-up of
    test_cell_ewald_host.test_analytic_anchors); bars 10 x the residuals measured on the CPU (the docstring of this file)"""
    D, E, res, res_p = _anchor(EU.nacl_cell(), (1.0, -1.0), 12.0)
    iso, off = max(abs(D[0] - D[1]), abs(D[1] - D[2]), abs(D[0] - D[2])), np.abs(D[3:]).max()
    print(f"NaCl: E = {E:.15g}  |tr D + E| = {res:.3e}  |3PV - E| = {res_p:.3e}  isotropy {iso:.3e}  off-diagonal {off:.3e}")
    assert res <= 1e-7 * abs(E) and res_p <= 1e-7 * abs(E)                   # the cap: above it the formula is wrong, not inexact
    assert res <= 10 * 1.04e-13 and res_p <= 10 * 1.04e-13
    assert iso <= 10 * 3.4e-16 and off <= 10 * 2.3e-17                       # the +0.013 of the fixture is a pure translation
    D, E, res, res_p = _anchor(EU.cscl_cell(), (1.0, -1.0), 12.0)
    print(f"CsCl: E = {E:.15g}  |tr D + E| = {res:.3e}  |3PV - E| = {res_p:.3e}")
    assert res <= 1e-7 * abs(E) and res <= 10 * 1.18e-13 and res_p <= 10 * 1.18e-13
    D, E, res, res_p = _anchor(EU.cube_cell(1.0), (1.0,), 3.9)               # a charged cell: the background term is part of it
    print(f"cube: E = {E:.15g}  |tr D + E| = {res:.3e}  |3PV - E| = {res_p:.3e}")
    assert res <= 1e-7 * abs(E) and res <= 10 * 1.8e-14 and res_p <= 10 * 1.8e-14


def test_finite_difference_of_the_existing_energy():
    """(E(+h) - E(-h)) / 2h of egnn_cell_ewald_host on strained lattices against D: the crist cell, BKS, shift, accuracy 1e-14 (the
    Coulomb membership changes are negligible, the short ones continuous); h = 1e-5 and the residual 1.12e-8 eV measured on the CPU"""
    L, h = _lib.lib(), 1e-5
    cell = EU.fixtures()["crist"]["cell"]
    base = EU.make_case(cell, EU.BKS_CHARGES, EU.bks_tables(), r_cut=8.2, short_cut=5.5, accuracy=1e-14)
    rc, s = XU.host(L, [base])
    assert rc == 0, L.egnn_last_error()
    rc, e0 = EU.host(L, [base], forces=False)
    assert rc == 0, L.egnn_last_error()
    worst = 0.0
    for v, (x, y) in enumerate(XU.VOIGT):
        eps = np.zeros((3, 3))
        eps[x, y] += h / 2
        eps[y, x] += h / 2
        E = []
        for sign in (1.0, -1.0):
            lattice = cells.strained(cells.PeriodicCell(cell["lattice"], cell["frac"], types=cell["types"]), sign * eps).lattice.numpy()
            rc, e = EU.host(L, [dict(base, cell=dict(cell, lattice=lattice))], forces=False)
            assert rc == 0, L.egnn_last_error()
            E.append(e["energy"][0])
        worst = max(worst, abs((E[0] - E[1]) / (2 * h) - s["strain"][0, v]))
    cap = 1e-6 * np.abs(e0["components"]).sum()
    print(f"finite difference: h = {h:g}  residual = {worst:.3e} eV  cap = {cap:.3e}")
    assert worst <= cap and worst <= 10 * 1.12e-8


def test_a_cell_gives_the_same_bits_in_any_batch_and_without_the_optional_output():
    L, case = _lib.lib(), EU.fixtures()["thin"]
    alone = XU.host_on_golden("thin")
    other = dict(case, cell=dict(EU.cube_cell(5.0, [[0.1, 0.2, 0.3], [0.6, 0.1, 0.7]]), A=2))
    rc, got = XU.host(L, [other, case, other])
    assert rc == 0, L.egnn_last_error()
    for k in ("per_atom", "comp_atom"):
        assert np.array_equal(got[k][2:14], alone[k]), k
    for k in ("strain", "components", "stress", "pressure"):
        assert np.array_equal(got[k][1], alone[k][0]), k
        assert np.array_equal(got[k][0], got[k][2]), k
    rc, bare = XU.host(L, [case], null=("comp_atom",))
    assert rc == 0 and all(np.array_equal(bare[k], alone[k]) for k in OUTPUTS if k != "comp_atom") and np.all(bare["comp_atom"] == -7.0)


def test_zero_charges_leave_the_short_part_alone():
    L, case = _lib.lib(), EU.fixtures()["thin"]
    full = XU.host_on_golden("thin")
    rc, got = XU.host(L, [case], charges=np.zeros(2))
    assert rc == 0 and got["n_vectors"].tolist() == [0]
    assert np.all(got["components"][0, :4] == 0.0) and np.array_equal(got["components"][0, 4], full["components"][0, 4])
    rc, coul = XU.host(L, [case], pot=None)
    assert rc == 0 and np.all(coul["components"][0, 4] == 0.0)
    for k in (0, 1, 3):
        assert np.array_equal(coul["components"][0, k], full["components"][0, k])


def test_coincident_atoms_are_flagged():
    L = _lib.lib()
    cell = EU.cube_cell(5.0, [[0.25, 0.5, 0.75], [0.6, 0.1, 0.7], [1.25, 0.5, 0.75]])
    rc, got = XU.host(L, [EU.make_case(EU.cube_cell(5.0), (1.0,), r_cut=6.0), EU.make_case(cell, (1.0,), r_cut=6.0)])
    assert rc == 0 and got["coincident"].tolist() == [0, 1] and np.all(np.isfinite(got["strain"])) and np.all(np.isfinite(got["pressure"]))


def test_refusals_of_the_host_statement():
    L, case = _lib.lib(), EU.fixtures()["thin"]
    run = lambda cases=None, **kw: XU.host(L, cases or [case], **kw)[0]
    assert run() == 0
    for out in ("strain", "components", "per_atom", "stress", "pressure", "n_vectors", "coincident"):
        assert run(null=(out,)) == EINVAL and b"egnn_cell_ewald_virial_host" in L.egnn_last_error(), out
    assert run(raw=dict(frac=None)) == EINVAL and run(raw=dict(type=None)) == EINVAL
    assert run(short_cut=4.38) == EINVAL and b"short_cut" in L.egnn_last_error()
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert run(alpha=bad) == EINVAL and run(k_max=bad) == EINVAL and run(kappa=bad) == EINVAL and run(short_cut=bad) == EINVAL
    assert run(n=0) == EINVAL and run(n=65) == EINVAL and b"power" in L.egnn_last_error()
    assert run(A=5) == EINVAL and b"atom types" in L.egnn_last_error()
    assert run(A=1) == EINVAL                                      # types outside [0, A)
    assert run(charges=np.array([1.0, np.inf])) == EINVAL and b"charge" in L.egnn_last_error()
    pot = case["pot"].copy()
    pot[2, 0, 1] += 1.0
    assert run(pot=pot) == EINVAL and b"symmetric" in L.egnn_last_error()
    w = CU.widths(case["cell"]["lattice"])
    assert run(r_cut=4.0 * w.min() * (1 + 1e-12), short_cut=1.0) == EINVAL and b"cut / 4" in L.egnn_last_error()       # a thin cell
    assert run(k_max=1025 * 2 * np.pi / 1.15) == EINVAL and b"Miller index" in L.egnn_last_error()
    nan = case["cell"]["frac"].copy()
    nan[3, 1] = np.inf
    assert run(cases=[dict(case, cell=dict(case["cell"], frac=nan))]) == EINVAL and b"not finite" in L.egnn_last_error()


def test_refusals_of_lattice_energy_with_stress_come_before_the_device():
    thin = EU.fixtures()["thin"]["cell"]
    cell = cells.PeriodicCell(thin["lattice"], thin["frac"], types=thin["types"], num_types=2)
    pot = cells.PairTable(*EU.fixtures()["thin"]["pot"][:3])
    with pytest.raises(ValueError, match="charges has 3 entries for 2 atom types"):
        cells.lattice_energy(cell, (1.0, 2.0, 3.0), r_cut=4.0, stress=True)
    with pytest.raises(ValueError, match="short_cut > r_cut"):
        cells.lattice_energy(cell, (1.0, -1.0), pot, r_cut=4.0, short_cut=4.1, stress=True, forces=False)
    with pytest.raises(ValueError, match="accuracy"):
        cells.lattice_energy(cell, (1.0, -1.0), r_cut=4.0, accuracy=1.0, stress=True)
    with pytest.raises(ValueError, match="cell 0: perpendicular widths"):
        cells.lattice_energy(cell, (1.0, -1.0), r_cut=4.7, stress=True)
    with pytest.raises(ValueError, match="Miller index"):
        cells.lattice_energy(cell, (1.0, -1.0), r_cut=4.0, k_max=6000.0, stress=True)


def test_strained_cells():
    thin = EU.fixtures()["thin"]["cell"]
    cell = cells.PeriodicCell(thin["lattice"], thin["frac"], types=thin["types"], num_types=3, id="thin")
    same = cells.strained(cell, np.zeros((3, 3)))
    assert isinstance(same, cells.PeriodicCell) and same is not cell and (same.num_types, same.id) == (3, "thin")
    assert torch.equal(same.lattice, cell.lattice) and torch.equal(same.frac, cell.frac) and torch.equal(same.types, cell.types)
    eps = np.array([[0.01, 0.002, -0.003], [0.002, -0.02, 0.004], [-0.003, 0.004, 0.005]])
    out = cells.strained([cell, cell], torch.tensor(eps))
    assert isinstance(out, list) and len(out) == 2 and out[0].lattice.shape == (3, 3) and out[0].frac.shape == cell.frac.shape
    assert torch.equal(out[0].frac, cell.frac) and torch.equal(out[1].types, cell.types)
    assert np.allclose(out[0].lattice.numpy(), thin["lattice"] @ (np.eye(3) + eps), rtol=1e-15, atol=0.0)
    ratio = EU.volume(out[0].lattice.numpy()) / EU.volume(thin["lattice"])
    assert abs(ratio - np.linalg.det(np.eye(3) + eps)) <= 1e-14
    for bad in (np.zeros(6), np.zeros((3, 4)), np.full((3, 3), np.nan)):
        with pytest.raises(ValueError, match="strain"):
            cells.strained(cell, bad)
    with pytest.raises(ValueError, match="PeriodicCell"):
        cells.strained([], np.zeros((3, 3)))


def test_constants_and_the_3x3_forms():
    assert cells.EV_PER_A3_IN_GPA == 160.2176634
    six = torch.arange(12, dtype=torch.float64).reshape(2, 6)
    form = cells._voigt_to_3x3(six)
    assert form.shape == (2, 3, 3) and torch.equal(form, form.transpose(1, 2))
    assert np.array_equal(XU.voigt(form.numpy()), six.numpy())
    assert form[1].tolist() == [[6.0, 11.0, 10.0], [11.0, 7.0, 9.0], [10.0, 9.0, 8.0]]


def test_cell_stress_host_under_sanitizers(tmp_path):
    from tests._host_program import build_and_run
    r = build_and_run(tmp_path, "cell_stress_main", ["cells/cell_stress_host.cpp", "cells/cell_ewald_host.cpp", "cells/cell_soap_host.cpp",
                                                     "cells/cell_host.cpp", "eval/sq_host.cpp", "host_logic.cpp"])
    assert r.returncode == 0 and "CELL-STRESS-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

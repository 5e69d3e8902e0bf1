"""The bond-orientational order of periodic cells on the host (egnn_cell_boo_host: csrc/cells/cell_boo_host.cpp over the definitions
the kernels compile, csrc/cells/cell_boo_math.h) against
  * the truth tests/golden/cell_boo_golden.npz (mpmath at 50 digits, complex harmonics and complex 3j sums, sites by exact rational
    arithmetic): n and n_solid exactly, E_host = the largest absolute difference of q, w, q_avg, w_avg (and of w_hat* where the
    truth's q_l >= 1e-3) below the cap 1e-12 (measured: printed by the test);
  * the analytic anchors: ideal sc, fcc, bcc, hcp, icosahedral and cristobalite shells to 5e-6;
  * the numpy restatement tests/_cell_boo_util.py (real basis, the same orders: bitwise) and the same through scipy.special;
  * rotated lattices (proper and improper): what catches a wrong G table.
Refusals and a stand-alone program under the address and undefined-behaviour sanitizers.  No GPU.
"""
import numpy as np
import pytest

from diffusion_model_amd import _lib
from tests import _cell_boo_util as BU
from tests import _cell_soap_util as CSU
from tests import _cells_util as CU
from tests._host_program import build_and_run

EINVAL = -22


@pytest.mark.parametrize("name,A", BU.CASES)
def test_host_against_the_truth(name, A):
    got, want = BU.host_on_golden(name, A), BU.truth(name, A)
    E = BU.error(got, want)
    print(f"cell BOO {name} A={A}: E_host = {E:.3e}  n = {got['n'].min()}..{got['n'].max()}")
    assert np.array_equal(got["n"], want["n"]) and np.array_equal(got["n_solid"], want["n_solid"])
    assert E < BU.CAP
    assert np.all(got["w"][:, 1::2] == 0.0) and np.all(got["w_avg"][:, 1::2] == 0.0) and np.all(got["w_hat"][:, 1::2] == 0.0)
    assert not any(np.any(got[k] == -7.0) for k in BU.FIELDS + ("qlm",))
    if name == "thin":
        assert CSU.box(BU.fixture(name, A)["lattice"], BU.THIN_CUT).tolist() == [4, 1, 2]
    if name == "one":
        assert got["n"].tolist() == [6]        # its own six images


@pytest.mark.parametrize("name", list(BU.FIXTURES))
def test_e_host_stays_below_the_cap(name):
    print(f"cell BOO {name}: E_host = {BU.e_host(name):.3e}")
    assert BU.e_host(name) < BU.CAP


@pytest.mark.parametrize("anchor", BU.anchors(), ids=lambda a: a[0])
def test_analytic_anchors(anchor):
    label, cell, cutoff, pairs, centre, sites, q_want, w_hat_want = anchor
    rc, res = BU.host(_lib.lib(), [cell], cutoff, pairs, cell["A"])
    assert rc == 0, _lib.lib().egnn_last_error()
    assert res["n"][centre] == sites
    for l, v in q_want.items():
        assert abs(res["q"][centre, l] - v) < 5e-6, (label, l, res["q"][centre, l])
    for l, v in w_hat_want.items():
        assert abs(res["w_hat"][centre, l] - v) < 5e-6, (label, l, res["w_hat"][centre, l])
    if label == "icosahedron":
        assert abs(res["w"][centre, 4]) < 5e-6                       # q_4 = 0: w_4 is compared, its normalised value is not
    if label == "Si<-Si":                                             # the diamond sublattice: s = +1 at l = 6, -1 at l = 3
        assert np.all(res["n_solid"][:8] == 4)
        assert np.all(BU.host(_lib.lib(), [cell], cutoff, pairs, 2, l_solid=3)[1]["n_solid"] == 0)
    if len(cell["frac"]) == 1 or label in ("Si<-Si", "hcp"):          # neighbours share the centre's q_lm (even l, where images of one
        even = slice(0, None, 2) if len(cell["frac"]) > 1 else slice(None)    # sublattice are inverted); a one-atom cell for every l
        rows = slice(0, 8) if label == "Si<-Si" else slice(None)
        assert np.abs(res["q_avg"][rows, even] - res["q"][rows, even]).max() < 1e-12


@pytest.mark.parametrize("name,A", [("thin", 3), ("crist34", 2), ("one", 1)])
def test_host_against_the_restatement(name, A):
    cell, cutoff, pairs = BU.checked_case(name, A)
    got = BU.host_on_golden(name, A)
    want = BU.restated(cell, cutoff, pairs, A)
    for k in BU.FIELDS + ("n", "n_solid", "qlm"):                    # the same operations in the same order
        assert np.array_equal(got[k], want[k]), k
    second = BU.restated(cell, cutoff, pairs, A, harmonics=BU.scipy_harmonics)
    assert np.array_equal(got["n"], second["n"]) and np.array_equal(got["n_solid"], second["n_solid"])
    assert BU.error(got, second) < 8 * max(BU.e_host(name), 1e-16) and np.abs(got["qlm"] - second["qlm"]).max() < 1e-14


def _rotations():
    out = []
    for seed, improper in ((1, False), (2, False), (3, True)):
        Q, R = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
        Q = Q * np.sign(np.diag(R))
        if (np.linalg.det(Q) < 0) != improper:
            Q[:, 0] = -Q[:, 0]
        out.append(Q)
    return out


@pytest.mark.parametrize("name,A", [("thin", 2), ("crist34", 2)])
def test_rotation_invariance(name, A):
    cell, cutoff, pairs = BU.checked_case(name, A)
    want = BU.host_on_golden(name, A)
    bar = 8 * BU.e_host(name)
    for R in _rotations():
        rc, got = BU.host(_lib.lib(), [dict(cell, lattice=cell["lattice"] @ R)], cutoff, pairs, A)
        assert rc == 0, _lib.lib().egnn_last_error()
        assert np.array_equal(got["n"], want["n"]), "a site crossed the cutoff under the rotation"
        for k in BU.FIELDS:
            ok = np.ones_like(want[k], dtype=bool) if "hat" not in k else (want["q" if k == "w_hat" else "q_avg"] >= 1e-3)
            assert np.abs(got[k] - want[k])[ok].max() < bar, (k, float(np.abs(got[k] - want[k])[ok].max()), bar)
        assert np.all(got["w"][:, 1::2] == 0.0) and np.all(got["w_avg"][:, 1::2] == 0.0)


def test_a_cell_gives_the_same_bits_in_any_batch_and_order():
    L = _lib.lib()
    thin, cutoff, pairs = BU.checked_case("thin", 2)
    alone = BU.host_on_golden("thin", 2)
    cells = [CU.one_atom_cell(), thin, CU.chain_cell()]
    rc, got = BU.host(L, cells, cutoff, pairs, 2)
    assert rc == 0
    for k in BU.FIELDS + ("n", "n_solid", "qlm"):
        assert np.array_equal(got[k][1:13], alone[k]), k
    assert got["n"][0] == 0 and np.all(got["q"][0] == 0.0) and np.all(got["q_avg"][0] == 0.0) and got["n_solid"][0] == 0
    rc, got = BU.host(L, cells, cutoff, pairs, 2, centres=[12, 1, 12, 5], averaged=False, qlm=False)
    assert rc == 0 and "q_avg" not in got
    for k in ("q", "w", "w_hat", "n", "n_solid"):
        assert np.array_equal(got[k], alone[k][[11, 0, 11, 4]]), k


def test_l_max_below_the_limit_gives_the_leading_columns():
    cell, cutoff, pairs = BU.checked_case("thin", 2)
    full = BU.host_on_golden("thin", 2)
    for l_max in (0, 1, 6):
        rc, got = BU.host(_lib.lib(), [cell], cutoff, pairs, 2, l_max=l_max, l_solid=min(l_max, 6))
        assert rc == 0
        for k in BU.FIELDS:
            assert np.array_equal(got[k], full[k][:, :l_max + 1]), (l_max, k)
        assert np.array_equal(got["qlm"], full["qlm"][:, :(l_max + 1) ** 2])
    assert np.allclose(BU.host(_lib.lib(), [cell], cutoff, pairs, 2, l_max=0, l_solid=0)[1]["q"], 1.0, atol=1e-15)


def test_refusals():
    L = _lib.lib()
    thin, cutoff, pairs = BU.checked_case("thin", 2)
    w = CU.widths(thin["lattice"])
    run = lambda cells=None, **kw: BU.host(L, cells or [thin], kw.pop("cutoff", cutoff), pairs, kw.pop("A", 2), **kw)[0]
    assert run() == 0
    assert run(l_max=11) == EINVAL and b"l_max" in L.egnn_last_error()
    assert run(l_max=-1, l_solid=0) == EINVAL and b"l_max" in L.egnn_last_error()
    assert run(l_solid=11) == EINVAL and b"l_solid" in L.egnn_last_error()
    assert run(l_solid=-1) == EINVAL and b"l_solid" in L.egnn_last_error()
    assert run(l_max=4, l_solid=5) == EINVAL and b"l_solid" in L.egnn_last_error()
    assert run(A=5) == EINVAL and b"atom types" in L.egnn_last_error()
    assert run(A=1, mask=1) == EINVAL and b"type" in L.egnn_last_error()
    assert run(mask=1 << 4) == EINVAL and b"select" in L.egnn_last_error()
    for c, ok in ((4.0 * w.min() * (1 - 1e-12), True), (4.0 * w.min() * (1 + 1e-12), False)):   # either side of width = cutoff / 4
        assert (run(cutoff=c, centres=[0]) == 0) == ok
    msg = L.egnn_last_error().decode()
    assert "cell 0" in msg and all(f"{v:.6g}" in msg for v in w) and "cut / 4" in msg
    assert run(cells=[CU.chain_cell(), thin], cutoff=5.3) == EINVAL and b"cell 1" in L.egnn_last_error()
    for c in (0.0, -1.0, np.nan, np.inf):
        assert run(cutoff=c) == EINVAL
    for bad in ([12], [-1]):
        assert run(centres=bad) == EINVAL and b"centre 0" in L.egnn_last_error()
    nan = thin["frac"].copy()
    nan[3, 1] = np.inf
    assert run(cells=[dict(thin, frac=nan)]) == EINVAL and b"not finite" in L.egnn_last_error()
    flat = dict(thin, lattice=np.array([[1.15, 0, 0], [0.4, 4.8, 0], [2.3, 0, 0]]))
    assert run(cells=[flat]) == EINVAL and b"singular" in L.egnn_last_error()


def test_g_tables_are_symmetric_tensors_of_even_l_only():
    norm, off, idx, val = BU.tables(10)
    assert off[0] == 0 and off[-1] == len(val) and all(off[l + 1] == off[l] for l in range(1, 11, 2))
    assert np.all(idx[:, 0] <= idx[:, 1]) and np.all(idx[:, 1] <= idx[:, 2]) and np.all(val != 0.0)
    for l in range(0, 11, 2):
        rows = idx[off[l]:off[l + 1]]
        assert rows.max() <= 2 * l and len({tuple(r) for r in rows}) == len(rows)
        assert [tuple(r) for r in rows] == sorted(tuple(r) for r in rows)
    assert abs(val[0] - 1.0) < 1e-15                                  # (0 0 0; 0 0 0) = 1


def test_cell_boo_host_under_sanitizers(tmp_path):
    r = build_and_run(tmp_path, "cell_boo_main", ["cells/cell_boo_host.cpp", "cells/cell_soap_host.cpp", "cells/cell_host.cpp", "host_logic.cpp"])
    assert r.returncode == 0 and "CELL-BOO-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

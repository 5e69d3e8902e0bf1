"""The relaxation of periodic cells on the host (egnn_cell_relax_step_host, egnn_cell_relax_host: csrc/cells/cell_relax_host.cpp over
the definitions the kernels compile, csrc/cells/cell_relax_math.h) against
  * a numpy restatement of the step (tests/_cell_relax_util.step_restated), bitwise, over a scripted sequence of forces that reaches
    every branch: P > 0 with and without a growing time step, P <= 0, the cap, the freeze, convergence, the step limit, a coincident
    site;
  * the same restatement driven by egnn_cell_ewald_host at every step, on the rocksalt fixture: bitwise where no coordinate leaves
    [0, 1) (the copy translated by +0.37), and within 8 times the measured difference on the untranslated fixture, whose atoms cross
    a face of the cell (there egnn_cell_ewald_host wraps, names the same sites by other shifts and so adds them in another order:
    DESIGN.md 5.13);
  * what a relaxation must reach: the ideal rocksalt sites (by symmetry stationary), with and without rebuilds, from translated copies.
The constructions of tests/test_gpu_cell_relax_held.py (held rows at moved coordinates): the entries that pass the re-test in numpy are
the rows of the truth, entries have entered and left r_cut where a case claims it, the gap and E_host conditions hold.
Refusals of cells.relax (raised before a device is touched) and of the host statements, and a stand-alone program under the address
and undefined-behaviour sanitizers.  No GPU.
"""
import numpy as np
import pytest

from diffusion_model_amd import _lib, cells
from tests import _cell_ewald_util as EU
from tests import _cell_relax_util as RU
from tests import _cell_soap_util as CSU
from tests import _cells_util as CU

EINVAL = -22
# the untranslated fixture against the restatement driven by egnn_cell_ewald_host, measured here: 2.3e-16 in a fractional coordinate
# and 7.2e-15 eV in an energy of the trajectory; the bars are 8 times that
ORDER_FRAC, ORDER_ENERGY = 8 * 2.3e-16, 8 * 7.2e-15


def test_step_against_the_restatement_bitwise():
    L = _lib.lib()
    cell_ptr, lattice, frac, calls = RU.script()
    p = RU.SCRIPT
    mine = RU.new_state(cell_ptr, frac, RU.FIRE, p["max_steps"])
    host = RU.copy_state(mine)
    seen = set()
    for k, (force, energy, coincident) in enumerate(calls):
        branch = RU.step_restated(mine, cell_ptr, lattice, force, energy, coincident, RU.FIRE, p["f_max"], p["max_steps"], p["skin"])
        rc = RU.step_host(L, host, cell_ptr, lattice, force, energy, coincident, RU.FIRE, p["f_max"], p["max_steps"], p["skin"])
        assert rc == 0, L.egnn_last_error()
        assert RU.same_state(mine, host) == [], (k, branch)
        seen.update(branch)
        if k % 2:                       # the caller's part of a rebuild, every other call: a frozen cell idles once in between
            RU.rebuild_restated(mine, cell_ptr)
            RU.rebuild_restated(host, cell_ptr)
    print("branches:", sorted(seen))
    assert {"move-", "move+", "move+g", "frozen", "idle", "converged", "limit", "coincident"} <= seen
    assert any(b.startswith("move") and b.endswith("c") for b in seen)
    assert set(mine["counters"][:, 2]) == {RU.CONVERGED, RU.STEP_LIMIT, RU.COINCIDENT} and mine["done"].all()


def test_step_leaves_a_frozen_cell_alone():
    L = _lib.lib()
    cell_ptr, lattice, frac, calls = RU.script()
    s = RU.new_state(cell_ptr, frac, RU.FIRE, 5)
    s["rebuild"][:] = 1
    before = RU.copy_state(s)
    assert RU.step_host(L, s, cell_ptr, lattice, *calls[0], RU.FIRE, 1e-3, 5, 0.6) == 0
    assert RU.same_state(s, before) == []


def test_a_cell_moves_after_a_rebuild_when_the_cap_is_active():
    """max_step == skin / 2 (accepted): the capped move right after a build has length max_step to a few ulp, above skin / 2 in a
    fraction of the cases.  It must be made all the same: a second freeze would change nothing and repeat for ever."""
    cell_ptr, lattice = np.array([0, 40], np.int32), np.ascontiguousarray(RU.SCRIPT_LATTICE.reshape(1, 9))
    rng = np.random.default_rng(17)
    L, above = _lib.lib(), 0
    for k in range(200):
        s = RU.new_state(cell_ptr, rng.uniform(size=(40, 3)), RU.FIRE, 5)
        force = np.ascontiguousarray(rng.normal(size=(40, 3)) * 10.0 ** rng.uniform(2, 5))
        mine = RU.copy_state(s)
        assert RU.step_host(L, s, cell_ptr, lattice, force, np.zeros(1), np.zeros(1, np.int32), RU.FIRE, 1e-3, 5, 0.4) == 0
        assert RU.step_restated(mine, cell_ptr, lattice, force, np.zeros(1), np.zeros(1, np.int32), RU.FIRE, 1e-3, 5, 0.4) == ["move-c"]
        assert RU.same_state(s, mine) == [] and s["rebuild"].tolist() == [0] and s["counters"][0, 1] == 1
        above += int(np.sqrt((s["since"] ** 2).sum(1)).max() > 0.2)
    print(f"capped first moves longer than skin / 2 by rounding: {above} of 200")
    assert above > 0                                                     # the case is met


@pytest.mark.parametrize("a,seed", [(3.8, 3), (3.2, 2), (3.2, 4)])
def test_a_strongly_compressed_cell_relaxes_at_max_step_equal_to_half_the_skin(a, seed):
    L = _lib.lib()
    case = RU.compressed_rocksalt(a, seed)
    rc, got = RU.relax_host(L, [case], f_max=1e-4, max_steps=2000, skin=0.4, trace=False)
    assert rc == 0, L.egnn_last_error()
    rc, wide = RU.relax_host(L, [case], f_max=1e-4, max_steps=2000, skin=0.41, trace=False)
    assert rc == 0
    print(f"a = {a}, seed {seed}: skin 0.4 {got['steps'][0]} moves, {got['n_rebuilds'][0]} rebuilds; skin 0.41 {wide['steps'][0]} moves, "
          f"{wide['n_rebuilds'][0]} rebuilds; |dE| = {abs(got['energy'][0] - wide['energy'][0]):.3e} eV")
    assert got["status"].tolist() == [RU.CONVERGED] and wide["status"].tolist() == [RU.CONVERGED]
    assert 1 <= got["n_rebuilds"][0] <= got["steps"][0]


def test_a_cell_that_freezes_twice_without_moving_is_stopped():
    """the guard: a caller that clears the flag without rebuilding (since left as it is) gets status stuck, not an endless loop"""
    L = _lib.lib()
    cell_ptr, lattice = np.array([0, 3], np.int32), np.ascontiguousarray(RU.SCRIPT_LATTICE.reshape(1, 9))
    s = RU.new_state(cell_ptr, np.full((3, 3), 0.5), RU.FIRE, 5)
    s["since"][:] = 0.1
    force = np.full((3, 3), 1e4)
    args = (cell_ptr, lattice, force, np.zeros(1), np.zeros(1, np.int32), RU.FIRE, 1e-3, 5, 0.4)
    mine = RU.copy_state(s)
    assert RU.step_host(L, s, *args) == 0 and RU.step_restated(mine, *args) == ["frozen"]
    assert s["rebuild"].tolist() == [1] and s["counters"][0].tolist() == [0, 0, 0, 1]
    s["rebuild"][:] = mine["rebuild"][:] = 0
    assert RU.step_host(L, s, *args) == 0 and RU.step_restated(mine, *args) == ["stuck"]
    assert RU.same_state(s, mine) == [] and s["done"].tolist() == [1] and s["counters"][0, 2] == RU.STUCK
    stale = RU.new_state(cell_ptr, np.full((3, 3), 0.5), RU.FIRE, 5)             # a stale step count writes no trace row
    stale["counters"][0, 1] = -3
    assert RU.step_host(L, stale, *args) == 0 and np.isnan(stale["energy_trace"]).all()


def test_whole_loop_against_the_ewald_host_bitwise():
    L = _lib.lib()
    case, _ = RU.rocksalt(0.37)
    rc, got = RU.relax_host(L, [case], skin=2.0, **RU.ROCKSALT)
    assert rc == 0, L.egnn_last_error()
    want = RU.restated_loop(L, case, RU.ROCKSALT["f_max"], RU.ROCKSALT["max_steps"], 2.0)
    assert got["n_rebuilds"].tolist() == [0] and got["steps"].tolist() == [want["steps"]] and got["status"].tolist() == [want["status"]]
    assert 0.0 <= np.nanmin(got["frac_trace"]) and np.nanmax(got["frac_trace"]) < 1.0          # no coordinate leaves [0, 1)
    assert np.array_equal(got["frac_trace"], want["frac_trace"], equal_nan=True)
    assert np.array_equal(got["energy_trace"][:, 0], want["energy_trace"], equal_nan=True)
    assert np.array_equal(got["frac"], want["frac"]) and got["energy"][0] == want["energy"]


def test_whole_loop_across_a_face_differs_by_summation_order_only():
    L = _lib.lib()
    case, _ = RU.rocksalt(0.0)
    got = RU.rocksalt_host(0.0, 2.0)[0]
    want = RU.restated_loop(L, case, RU.ROCKSALT["f_max"], RU.ROCKSALT["max_steps"], 2.0)
    assert np.nanmax(got["frac_trace"]) > 1.0                                                   # atoms do cross a face
    d_frac = float(np.nanmax(np.abs(got["frac_trace"] - want["frac_trace"])))
    d_e = float(np.nanmax(np.abs(got["energy_trace"][:, 0] - want["energy_trace"])))
    print(f"across a face: |d frac| = {d_frac:.3e}  |d E| = {d_e:.3e} eV")
    assert got["steps"].tolist() == [want["steps"]]
    assert d_frac <= ORDER_FRAC and d_e <= ORDER_ENERGY


def test_rocksalt_converges_to_the_ideal_sites():
    L = _lib.lib()
    got, D = RU.rocksalt_host(0.0, 2.0)
    case, ideal = RU.rocksalt(0.0)
    rc, e = EU.host(L, [dict(case, cell=ideal)])
    assert rc == 0
    excess = got["energy"][0] - e["energy"][0]
    print(f"rocksalt on the host: {got['steps'][0]} moves, D_host = {D:.3e} A, energy excess = {excess:.3e} eV, max |F| = {got['max_force'][0]:.3e}")
    assert got["status"].tolist() == [RU.CONVERGED] and got["steps"][0] <= RU.ROCKSALT["max_steps"]
    assert got["max_force"][0] < RU.ROCKSALT["f_max"] and D < RU.IDEAL_CAP
    assert got["energy"][0] < got["initial_energy"][0] and abs(excess) < 1e-9
    assert got["energy_trace"][0, 0] == got["initial_energy"][0]
    last = np.nonzero(np.isfinite(got["energy_trace"][:, 0]))[0][-1]
    assert last == got["steps"][0] and got["energy_trace"][last, 0] == got["energy"][0]


def test_rebuilds_do_not_change_the_end():
    held, _ = RU.rocksalt_host(0.0, 2.0)
    got, D = RU.rocksalt_host(0.0, 0.4)
    largest = float(np.sqrt((got["moved"] ** 2).sum(1)).max())
    print(f"skin 0.4: {got['n_rebuilds'][0]} rebuild(s), largest displacement {largest:.4f} A, D = {D:.3e} A")
    assert got["n_rebuilds"][0] >= 1 and largest > 0.2 and got["status"].tolist() == [RU.CONVERGED]
    assert np.sqrt(((got["moved"] - held["moved"]) ** 2).sum(1)).max() <= 8 * RU.d_host()
    assert D <= RU.IDEAL_CAP


@pytest.mark.parametrize("skin", [2.0, 0.4])
def test_translated_copies_end_alike(skin):
    base = RU.rocksalt_host(0.0, skin)[0]
    for t in (0.37, -0.02):
        got, D = RU.rocksalt_host(t, skin)
        assert got["status"].tolist() == [RU.CONVERGED] and D <= RU.IDEAL_CAP
        assert abs(got["energy"][0] - base["energy"][0]) <= 1e-11
        assert np.sqrt(((got["moved"] - base["moved"]) ** 2).sum(1)).max() <= 8 * RU.d_host()
    assert np.nanmin(RU.rocksalt_host(-0.02, skin)[0]["frac_trace"]) < 0.0 or skin == 0.4     # the -0.02 copy carries atoms across a face


def test_a_cell_gives_the_same_bits_in_any_batch_on_the_host():
    L = _lib.lib()
    case, _ = RU.rocksalt(0.0)
    other = dict(case, cell=dict(EU.cube_cell(5.0, [[0.1, 0.2, 0.3], [0.62, 0.7, 0.81]]), A=2, types=np.array([0, 1], np.int32)))
    alone = RU.rocksalt_host(0.0, 0.4)[0]
    rc, got = RU.relax_host(L, [other, case, other], skin=0.4, **RU.ROCKSALT)
    assert rc == 0, L.egnn_last_error()
    for k in ("frac", "moved", "force"):
        assert np.array_equal(got[k][2:10], alone[k]), k
    for k in ("energy", "steps", "n_rebuilds", "status"):
        assert got[k][1] == alone[k][0] and got[k][0] == got[k][2], k


def test_coincident_atoms_stop_the_host_loop():
    L = _lib.lib()
    cell = dict(EU.cube_cell(5.0, [[0.25, 0.5, 0.75], [0.6, 0.1, 0.7], [1.25, 0.5, 0.75]]), A=1)
    rc, got = RU.relax_host(L, [EU.make_case(cell, (1.0,), r_cut=6.0)], skin=1.0, max_steps=5)
    assert rc == 0 and got["status"].tolist() == [RU.COINCIDENT] and got["steps"].tolist() == [0]


def test_refusals_of_the_host_statements():
    L = _lib.lib()
    case, _ = RU.rocksalt(0.0)
    run = lambda **kw: RU.relax_host(L, [case], **dict(dict(skin=1.0, max_steps=3), **kw))[0]
    assert run() == 0
    assert run(f_max=0.0) == EINVAL and b"f_max" in L.egnn_last_error()
    assert run(max_steps=-1) == EINVAL and b"max_steps" in L.egnn_last_error()
    assert run(skin=0.0) == EINVAL and b"skin" in L.egnn_last_error()
    assert run(skin=0.3) == EINVAL and b"skin / 2" in L.egnn_last_error()
    assert run(skin=5.64 * 4 - 6.0 + 1e-9, fire=dict(max_step=0.2)) == EINVAL and b"cut / 4" in L.egnn_last_error()
    assert run(fire=dict(f_dec=1.0)) == EINVAL and b"FIRE" in L.egnn_last_error()
    assert run(short_cut=6.1) == EINVAL and b"short_cut" in L.egnn_last_error()
    cell_ptr, lattice, frac, calls = RU.script()
    s = RU.new_state(cell_ptr, frac, RU.FIRE, 5)
    assert RU.step_host(L, s, cell_ptr, lattice, *calls[0], RU.FIRE, 1e-3, 5, 0.3) == EINVAL and b"skin / 2" in L.egnn_last_error()
    bad = cell_ptr.copy()
    bad[0] = 1                          # must run from 0
    assert RU.step_host(L, s, bad, lattice, *calls[0], RU.FIRE, 1e-3, 5, 0.6) == EINVAL


def test_refusals_of_relax_come_before_the_device():
    case, _ = RU.rocksalt(0.0)
    c = case["cell"]
    cell = cells.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=2)
    pot = cells.PairTable(*RU.rocksalt_tables()[:3])
    run = lambda **kw: cells.relax(cell, (1.0, -1.0), pot, **dict(dict(r_cut=6.0), **kw))
    with pytest.raises(ValueError, match="f_max"):
        run(f_max=0.0)
    with pytest.raises(ValueError, match="max_steps"):
        run(max_steps=-1)
    with pytest.raises(ValueError, match="skin"):
        run(skin=0.0)
    with pytest.raises(ValueError, match=r"max_step = 0\.2 exceeds skin / 2 = 0\.15 \(skin = 0\.3\)"):
        run(skin=0.3)
    with pytest.raises(ValueError, match="cell 0: perpendicular widths"):
        run(skin=5.64 * 4 - 6.0 + 1e-9)
    with pytest.raises(ValueError, match="_RELAX_LIST_BYTES"):
        big = cells.PeriodicCell(40.0 * np.eye(3), np.random.default_rng(0).uniform(size=(200000, 3)), types=np.zeros(200000, np.int32), num_types=1)
        cells.relax(big, (0.0,), r_cut=9.0)
    with pytest.raises(ValueError, match="method must be one of"):
        run(method="cells")
    with pytest.raises(ValueError, match="short_cut > r_cut"):          # the refusals of lattice_energy are kept
        run(short_cut=6.1)
    with pytest.raises(ValueError, match="charges has 3 entries"):
        cells.relax(cell, (1.0, -1.0, 0.0), pot, r_cut=6.0)
    with pytest.raises(ValueError, match="FIRE needs"):
        cells.FireParameters(f_dec=1.5)
    f = cells.FireParameters()
    assert (f.dt, f.dt_max, f.n_min, f.f_inc, f.f_dec, f.a_start, f.f_a, f.max_step) == (0.1, 1.0, 5, 1.1, 0.5, 0.1, 0.99, 0.2)


# ---- the constructions of tests/test_gpu_cell_relax_held.py ---------------------------------------------------------------------------------
def _names(j, s, keep):
    return {(int(a), *map(int, b)) for a, b in zip(j[keep], s[keep])}


@pytest.mark.parametrize("name", list(RU.HELD_CASES))
def test_held_cases_are_what_they_claim(name):
    """every held case of the device tests, without a device: the entries of the held rows that pass the re-test in numpy are the rows
    of the truth, "entered" and "left" are met where claimed, and the conditions on the gap and on E_host hold"""
    h = RU.held(name)
    case, ref, skin = h["case"], h["ref"], h["skin"]
    ex, e_host = RU.held_truth(name)
    rows, truth = RU.held_retest(h), RU.truth_rows_as_held(h, ex)
    n_held, n_kept = [len(r[0]) for r in rows], [int(r[2].sum()) for r in rows]
    entered, left = [int((r[2] & ~r[3]).sum()) for r in rows], [int((r[3] & ~r[2]).sum()) for r in rows]
    print(f"{name}: r_cut = {case['r_cut']:.6f} skin = {skin} held {n_held} kept {n_kept} entered {entered} left {left} gap = {float(ex['gap']):.2e} "
          f"E_host = {e_host:.2e}")
    assert e_host <= EU.CAP and float(ex["gap"]) > EU.GAP                       # conditions, not measurements
    assert case["alpha"] * case["r_cut"] <= 3.0 and not case["shift"]
    length = np.sqrt((h["delta"] ** 2).sum(1))
    assert length.max() <= skin / 2 and (name in ("limit", "outside", "pair", "single") or (length.min() == 0.0 and length.max() > 0.99 * skin / 2))
    L = np.asarray(ref["lattice"], np.float64)
    assert CSU.box(L, case["r_cut"] + skin).max() <= 4                         # the range of the shift code
    for i, (j, s, now, then, d) in enumerate(rows):
        assert _names(j, s, now) == truth[i] and n_kept[i] == len(truth[i]) == int(ex["row_ptr"][i + 1] - ex["row_ptr"][i]), i
        own = j == i                                                           # an own image moves with its centre: s L whatever delta_i
        assert np.array_equal(d[own], CU.site_vectors(np.zeros(3), np.zeros(3), s[own], L))
    if name in RU.HELD_MOVED:                                                  # in EVERY row an entry has entered r_cut and one has left it
        assert min(entered) > 0 and min(left) > 0
    u = case["cell"]["frac"]
    if name.startswith("row"):
        assert int(name[3:]) in n_kept
    if ref["name"] == "thin8":
        assert ((u < 0.0) | (u >= 1.0)).any()                                  # a coordinate outside [0, 1)
        assert CSU.box(L, case["r_cut"] + skin).tolist() == ([2, 1, 1] if name == "row1" else [4, 1, 2])
    if name == "three":                                                        # three passes of a wavefront, less than one kept
        assert all(128 < a <= 192 for a in n_held) and all(0 < b < 64 for b in n_kept)
    if name == "outside":
        assert n_held == [6] and n_kept == [0]
    if name == "limit":                                                        # the outermost entry of its row counts; the inner one does not
        assert n_held == [1, 1, 1, 1] and n_kept == [1, 1, 0, 0] and entered == [1, 1, 0, 0] and left == [0, 0, 1, 1]
        built = [float(np.sqrt(EU._norm2(CSU.sites(ref, case["r_cut"] + skin, i)[2]))[0]) for i in range(4)]
        assert all(case["r_cut"] + skin - 2e-3 < b < case["r_cut"] + skin for b in built[:2])
        assert all(case["r_cut"] - skin < b < case["r_cut"] - skin + 2e-3 for b in built[2:])
    if name == "face":
        assert u[0, 0] > 1.0 and not h["delta"][1].any()
        j, s, now, _, _ = rows[0]
        assert (1, 1, 0, 0) in _names(j, s, now)                               # the unmoved neighbour across the face, named from w0
        assert any(a == 0 for a, *_ in _names(j, s, now))                      # an image of the centre itself


def test_held_coincidence_appears_only_after_the_move():
    L = _lib.lib()
    h = RU.held("coincide")
    u = h["case"]["cell"]["frac"]
    assert np.array_equal(u[0], u[1]) and np.abs(h["delta"]).max() <= h["skin"] / 2
    assert np.array_equal(h["ref"]["frac"] + h["delta"] / 4.0, u)              # exact in a cube of 4 A
    rc, now = EU.host(L, [h["case"]])
    rc0, then = EU.host(L, [dict(h["case"], cell=h["ref"])])
    assert rc == 0 and rc0 == 0 and now["coincident"].tolist() == [1] and then["coincident"].tolist() == [0]
    j, s, inside, _, d = RU.held_retest(h)[0]
    at = np.nonzero((j == 1) & (s == 0).all(1))[0]
    assert len(at) == 1 and inside[at[0]] and not d[at[0]].any()


@pytest.mark.parametrize("name", list(EU.fixtures()))
def test_fp64_scales_are_those_of_the_truth(name):
    """tests/_cell_relax_util.scales (the yardstick of a cell too large for 50 digits) against the scales of the five fixtures' truth: a
    sum of n positive fp64 terms is within n ulp of the sum at 50 digits, n below 1e4 here"""
    se, sf = RU.scales(EU.fixtures()[name])
    want = EU.truth(name)
    assert np.allclose(se, want["scale_e"], rtol=1e-12, atol=0.0) and np.allclose(sf, want["scale_f"], rtol=1e-12, atol=0.0)


def test_cell_relax_host_under_sanitizers(tmp_path):
    from tests._host_program import build_and_run
    r = build_and_run(tmp_path, "cell_relax_main", ["cells/cell_relax_host.cpp", "cells/cell_ewald_host.cpp", "cells/cell_soap_host.cpp",
                                                    "cells/cell_host.cpp", "eval/sq_host.cpp", "host_logic.cpp"])
    assert r.returncode == 0 and "CELL-RELAX-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

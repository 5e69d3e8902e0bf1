"""cells.relax on the device (csrc/cells/cell_relax.hip) against
  * the truth of the lattice-energy fixtures (tests/golden/cell_ewald_golden.npz) for the evaluation over a held row: the bar of
    cells.lattice_energy, 8 x E_host;
  * the host statement egnn_cell_relax_step_host for the step kernel, bitwise, over the scripted sequence of
    tests/_cell_relax_util.script in one batch of cells of 1, 63, 64, 65, 257 and 1,025 atoms (either side of a wavefront, beyond one
    stride of the workgroup);
  * the ideal rocksalt sites (stationary by symmetry), with and without rebuilds and from translated copies, within 8 x D_host, the
    deviation the host loop ends with;
  * BKS beta-cristobalite against a fresh cells.lattice_energy at the relaxed coordinates;
and for its bits: two runs, a cell alone and in a batch, check_every 1 and 16."""
import functools

import numpy as np
import pytest
import torch

from diffusion_model_amd import _lib, cells
from tests import _cell_ewald_util as EU
from tests import _cell_relax_util as RU

pytestmark = pytest.mark.gpu
FLOOR = 1e-16


def _cell(c, A=None):
    return cells.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=c["A"] if A is None else A)


def relax(cases, **kw):
    """cells.relax on the cells of ``cases`` with the model of the first"""
    c0, A = cases[0], max(c["cell"]["A"] for c in cases)
    pot = None if c0["pot"] is None else cells.PairTable(*c0["pot"], n=c0["n"])
    return cells.relax([_cell(c["cell"], A) for c in cases], c0["charges"], pot, r_cut=c0["r_cut"], short_cut=c0["short_cut"], shift=c0["shift"],
                       alpha=c0["alpha"], k_max=c0["k_max"], coulomb_constant=c0["kappa"], **kw)


@functools.lru_cache(maxsize=None)
def rocksalt_run(translate=0.0, skin=2.0, check_every=16):
    """cells.relax on the rocksalt fixture: computed once, never changed"""
    case, _ = RU.rocksalt(translate)
    return relax([case], skin=skin, check_every=check_every, trace=True, **RU.ROCKSALT)


def rocksalt_deviation(res, translate):
    case, ideal = RU.rocksalt(translate)
    return RU.deviation(case["cell"]["frac"], res.displacement.cpu().numpy(), ideal, ideal["lattice"])


# The skin of the evaluation test is 0.7 A wherever the cell admits it.  The two fixtures in the thin triclinic cell (widths 1.139 /
# 4.74 / 3.1 A) do not: (r_cut + 0.7) / 1.139 is above 4, the image box the shift code holds, and relax refuses them as it must.  They
# run at the largest skin of two digits under that limit, (4 x 1.139 - r_cut): 0.18 A at r_cut = 4.37 and 0.65 A at r_cut = 3.9.
SKIN = dict(thin=0.18, crist=0.7, one=0.7, nacl=0.7, zero3=0.65)


@pytest.mark.parametrize("name", list(EU.fixtures()))
@pytest.mark.parametrize("stop", ["max_steps", "f_max"])
def test_evaluation_over_a_held_row(name, stop):
    case, want = EU.fixtures()[name], EU.truth(name)
    how = dict(max_steps=0) if stop == "max_steps" else dict(f_max=1e30)
    if SKIN[name] != 0.7:
        with pytest.raises(ValueError, match="perpendicular widths"):
            relax([case], skin=0.7, **how)
    res = relax([case], skin=SKIN[name], fire=cells.FireParameters(max_step=min(0.2, SKIN[name] / 2)), **how)
    got = dict(e_atom=res.energy_per_atom.cpu().numpy(), comp_atom=res.components_per_atom.cpu().numpy(), force=res.forces.cpu().numpy(),
               energy=res.energy[0].cpu().numpy(), components=res.components[0].cpu().numpy())
    E, bar = EU.error(got, want), 8 * max(EU.e_host(name), FLOOR)
    print(f"{name}: E(held row, truth) = {E:.3e}  bar = {bar:.3e}")
    assert E <= bar
    assert res.steps.tolist() == [0] and res.n_rebuilds.tolist() == [0]
    assert res.converged.tolist() == [stop == "f_max" or float(res.max_force[0]) < 1e-3]      # one atom alone feels no force
    assert torch.equal(res.energy, res.initial_energy) and not bool(res.displacement.any())


def test_step_kernel_against_the_host_statement_bitwise():
    L = _lib.lib()
    cell_ptr, lattice, frac, calls = RU.script()
    p, C, N = RU.SCRIPT, len(cell_ptr) - 1, int(cell_ptr[-1])
    host = RU.new_state(cell_ptr, frac, RU.FIRE, p["max_steps"])
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    d_cell_ptr, d_lattice = torch.from_numpy(cell_ptr).cuda(), torch.from_numpy(lattice).cuda()
    branches = set()
    for k, (force, energy, coincident) in enumerate(calls):
        assert RU.step_host(L, host, cell_ptr, lattice, force, energy, coincident, RU.FIRE, p["f_max"], p["max_steps"], p["skin"]) == 0
        d_in = [torch.from_numpy(a).cuda() for a in (force, energy, coincident)]
        _lib.check(L.egnn_cell_relax_step(_lib.stream_ptr(), C, N, RU.vp(cell_ptr), RU.vp(lattice), _lib.ptr(d_cell_ptr), _lib.ptr(d_lattice),
                                          *(_lib.ptr(t) for t in d_in), *RU.fire_args(RU.FIRE), p["f_max"], p["max_steps"], p["skin"],
                                          *(_lib.ptr(dev[name]) for name in ("frac", "velocity", "since", "moved", "scalars", "counters", "done",
                                                                             "rebuild", "energy_trace", "force_trace"))))
        got = {name: t.cpu().numpy() for name, t in dev.items()}
        assert RU.same_state(host, got) == [], k
        branches.update(np.nonzero(host["rebuild"])[0].tolist())
        if k % 2:
            RU.rebuild_restated(host, cell_ptr)
            for name in ("frac", "since", "rebuild"):
                dev[name].copy_(torch.from_numpy(host[name]))
    assert branches, "no cell of the script froze"
    assert set(host["counters"][:, 2]) == {RU.CONVERGED, RU.STEP_LIMIT, RU.COINCIDENT} and host["done"].all()


def _device_step(L, state, cell_ptr, lattice, force, energy, coincident, f_max, max_steps, skin):
    """egnn_cell_relax_step on copies of the host arrays -> the state after it, as numpy"""
    C, N = len(cell_ptr) - 1, int(cell_ptr[-1])
    dev = {k: torch.from_numpy(v).cuda() for k, v in state.items()}
    ins = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (cell_ptr, lattice, force, energy, coincident)]
    _lib.check(L.egnn_cell_relax_step(_lib.stream_ptr(), C, N, RU.vp(cell_ptr), RU.vp(lattice), *(_lib.ptr(t) for t in ins), *RU.fire_args(RU.FIRE),
                                      f_max, max_steps, skin, *(_lib.ptr(dev[name]) for name in ("frac", "velocity", "since", "moved", "scalars",
                                                                                                 "counters", "done", "rebuild", "energy_trace",
                                                                                                 "force_trace"))))
    return {name: t.cpu().numpy() for name, t in dev.items()}


def test_step_kernel_moves_a_just_built_cell_and_stops_a_stuck_one():
    """64 cells of 40 atoms under forces of 1e2 .. 1e5 eV / A at max_step == skin / 2: the capped first move exceeds skin / 2 by rounding
    in some of them and is made in all; then the guard: the same cells, frozen once, meet the same evaluation with the flag cleared
    and nothing rebuilt"""
    L, rng, C, n = _lib.lib(), np.random.default_rng(17), 64, 40
    cell_ptr = (np.arange(C + 1) * n).astype(np.int32)
    lattice = np.ascontiguousarray(np.tile(RU.SCRIPT_LATTICE.reshape(1, 9), (C, 1)))
    force = np.ascontiguousarray(rng.normal(size=(C * n, 3)) * np.repeat(10.0 ** rng.uniform(2, 5, C), n)[:, None])
    args = (cell_ptr, lattice, force, np.zeros(C), np.zeros(C, np.int32), 1e-3, 5, 0.4)
    host = RU.new_state(cell_ptr, rng.uniform(size=(C * n, 3)), RU.FIRE, 5)
    got = _device_step(L, host, *args)
    assert RU.step_host(L, host, *args[:5], RU.FIRE, *args[5:]) == 0
    assert RU.same_state(host, got) == [] and not host["rebuild"].any() and host["counters"][:, 1].tolist() == [1] * C
    assert (np.sqrt((host["since"] ** 2).sum(1)).reshape(C, n).max(1) > 0.2).any()          # the case is met
    for want in ("frozen", "stuck"):            # since is 0.2 A now: the next capped move freezes; unrebuilt, it is stuck
        got = _device_step(L, host, *args)
        assert RU.step_host(L, host, *args[:5], RU.FIRE, *args[5:]) == 0
        assert RU.same_state(host, got) == []
        if want == "frozen":
            assert host["rebuild"].all() and not host["done"].any()
            host["rebuild"][:] = 0
    assert host["done"].all() and set(host["counters"][:, 2]) == {RU.STUCK}


def test_a_strongly_compressed_cell_relaxes_at_max_step_equal_to_half_the_skin():
    case, f_max = RU.compressed_rocksalt(3.8, 3), 1e-4
    res = relax([case], f_max=f_max, max_steps=2000, skin=0.4)
    rc, host = RU.relax_host(_lib.lib(), [case], f_max=f_max, max_steps=2000, skin=0.4, trace=False)
    assert rc == 0
    fresh = cells.lattice_energy(res.cells, case["charges"], cells.PairTable(*case["pot"], n=case["n"]), r_cut=case["r_cut"],
                                 short_cut=case["short_cut"], alpha=case["alpha"], k_max=case["k_max"], coulomb_constant=case["kappa"])
    print(f"compressed rocksalt: {int(res.steps[0])} moves, {int(res.n_rebuilds[0])} rebuilds (host {host['steps'][0]}, {host['n_rebuilds'][0]}), "
          f"E = {float(res.energy[0]):.9f} (host {host['energy'][0]:.9f}), fresh max |F| = {float(fresh.forces.norm(dim=1).max()):.3e}")
    assert res.converged.tolist() == [True] and 1 <= int(res.n_rebuilds[0]) <= int(res.steps[0]) <= 2000
    assert float(res.energy[0]) < float(res.initial_energy[0])
    assert float(fresh.forces.norm(dim=1).max()) < f_max * (1 + 1e-6)


@pytest.mark.parametrize("translate,skin", [(0.0, 2.0), (0.0, 0.4), (0.37, 2.0), (-0.02, 2.0), (0.37, 0.4), (-0.02, 0.4)])
def test_rocksalt_reaches_the_ideal_sites(translate, skin):
    res = rocksalt_run(translate, skin)
    D, bar = rocksalt_deviation(res, translate), 8 * RU.d_host()
    print(f"rocksalt {translate:+.2f} skin {skin}: {res.steps.tolist()} moves, {res.n_rebuilds.tolist()} rebuilds, D = {D:.3e} A (8 D_host = {bar:.3e}), "
          f"max |F| = {float(res.max_force[0]):.3e}")
    assert res.converged.tolist() == [True] and int(res.steps[0]) <= RU.ROCKSALT["max_steps"]
    assert float(res.max_force[0]) < RU.ROCKSALT["f_max"] and D <= bar
    if skin == 0.4:
        assert int(res.n_rebuilds[0]) >= 1
    base = rocksalt_run(0.0, skin)
    assert abs(float(res.energy[0]) - float(base.energy[0])) <= 1e-11
    assert float((res.displacement - base.displacement).norm(dim=1).max()) <= bar
    assert abs(float(res.rmsd[0]) - float(np.sqrt((res.displacement.cpu().numpy() ** 2).sum(1).mean()))) <= 1e-15


def test_bks_cristobalite():
    case, f_max = EU.fixtures()["crist"], 1e-2
    res = relax([case], f_max=f_max, max_steps=1800)
    fresh = cells.lattice_energy(res.cells, case["charges"], cells.PairTable(*case["pot"], n=case["n"]), r_cut=case["r_cut"],
                                 short_cut=case["short_cut"], shift=case["shift"], alpha=case["alpha"], k_max=case["k_max"],
                                 coulomb_constant=case["kappa"])
    fm = float(fresh.forces.norm(dim=1).max())
    bar = 8 * max(EU.e_host("crist"), FLOOR) * float(EU.truth("crist")["scale_e"].sum())
    largest = float(res.displacement.norm(dim=1).max())
    print(f"BKS cristobalite: {int(res.steps[0])} moves, {int(res.n_rebuilds[0])} rebuilds, E {float(res.initial_energy[0]):.6f} -> "
          f"{float(res.energy[0]):.6f} eV, fresh max |F| = {fm:.6e}, |E - fresh| = {abs(float(res.energy[0] - fresh.energy[0])):.3e} (bar {bar:.3e}), "
          f"largest move {largest:.3f} A, rmsd {float(res.rmsd[0]):.3f} A")
    assert res.converged.tolist() == [True] and int(res.steps[0]) <= 1800
    assert float(res.energy[0]) < float(res.initial_energy[0])
    assert fm < f_max * (1 + 1e-6)
    assert abs(float(res.energy[0] - fresh.energy[0])) <= bar
    assert int(res.n_rebuilds[0]) >= 1


def _bits(res, lo, hi, c):
    return (res.frac[lo:hi].cpu().numpy(), float(res.energy[c]), int(res.steps[c]), int(res.n_rebuilds[c]))


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def test_bits_do_not_depend_on_the_run_the_batch_or_check_every():
    salt, moving = RU.rocksalt(0.0)[0], RU.rocksalt(0.37)[0]
    still = dict(salt, cell=EU.nacl_cell(5.64))            # the ideal sites: converged at once
    kw = dict(skin=0.4, **RU.ROCKSALT)
    alone = rocksalt_run(0.37, 0.4)
    again = relax([moving], **kw)
    assert _same(_bits(alone, 0, 8, 0), _bits(again, 0, 8, 0)) and torch.equal(alone.forces, again.forces)
    assert int(alone.n_rebuilds[0]) >= 1
    batch = relax([salt, moving, still], **kw)
    assert _same(_bits(batch, 8, 16, 1), _bits(alone, 0, 8, 0))
    assert _same(_bits(batch, 0, 8, 0), _bits(rocksalt_run(0.0, 0.4), 0, 8, 0))
    assert int(batch.steps[2]) == 0 and bool(batch.converged[2]) and int(batch.n_rebuilds[2]) == 0
    one = relax([salt, moving, still], check_every=1, **kw)
    for c in range(3):
        assert _same(_bits(one, 8 * c, 8 * c + 8, c), _bits(batch, 8 * c, 8 * c + 8, c)), c


def test_the_grid_search_holds_the_same_lists():
    """192 atoms of displaced beta-cristobalite 2 x 2 x 2 under BKS at r_cut = 4 A with a skin of 0.2 A: the host loop rebuilds this
    cell 8 times in 40 moves; the rows of the linked-cell search, refreshed on the device at every rebuild, are those of the site
    kernels, so the trajectories agree bitwise"""
    from tests import _cell_grid_util as GU
    cell = GU.displaced_cristobalite(2)
    cell = dict(cell, frac=cell["frac"] + np.random.default_rng(9).uniform(-0.08, 0.08, cell["frac"].shape) / 14.32)
    case = EU.make_case(cell, EU.BKS_CHARGES, EU.bks_tables(), r_cut=4.0, short_cut=4.0, accuracy=1e-3)
    kw = dict(f_max=1e-2, max_steps=40, skin=0.2, fire=cells.FireParameters(max_step=0.1))
    direct, grid = relax([case], method="direct", **kw), relax([case], method="grid", **kw)
    assert int(direct.n_rebuilds[0]) >= 1 and int(direct.steps[0]) == 40
    assert _same(_bits(direct, 0, 192, 0), _bits(grid, 0, 192, 0)) and torch.equal(direct.forces, grid.forces)
    assert float(direct.energy[0]) < float(direct.initial_energy[0])


def test_trace():
    res = rocksalt_run(0.0, 0.4)
    e, f = res.energy_trace[:, 0].cpu().numpy(), res.max_force_trace[:, 0].cpu().numpy()
    steps = int(res.steps[0])
    assert e.shape == (RU.ROCKSALT["max_steps"] + 1,) and e[0] == float(res.initial_energy[0])
    last = np.nonzero(np.isfinite(e))[0][-1]
    assert last == steps and e[last] == float(res.energy[0]) and f[last] == float(res.max_force[0])
    assert np.all(np.isfinite(e[:steps + 1])) and np.all(np.isnan(e[steps + 1:])) and np.all(np.isnan(f[steps + 1:]))
    assert rocksalt_run(0.0, 2.0).energy_trace is not None and relax([RU.rocksalt(0.0)[0]], max_steps=0).energy_trace is None


def test_coincident_atoms_name_the_cell_and_the_step():
    good = EU.make_case(dict(EU.cube_cell(5.0, [[0.25, 0.5, 0.75], [0.6, 0.1, 0.7]]), A=1), (1.0,), r_cut=6.0)
    bad = dict(good, cell=dict(EU.cube_cell(5.0, [[0.25, 0.5, 0.75], [0.6, 0.1, 0.7], [1.25, 0.5, 0.75]]), A=1))
    with pytest.raises(ValueError, match="cell 1, step 0: coincident atoms"):
        relax([good, bad], max_steps=3)

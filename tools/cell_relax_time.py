"""Time the relaxation of periodic cells (csrc/cells/cell_relax.hip through cells.relax) on displaced beta-cristobalite with BKS at
the parameters of the energy record (profiles/cell_ewald_time.json): r_cut = 10 A, short_cut = 5.5 A, accuracy = 1e-8; skin 1 A, the
default FIRE parameters, f_max so small that every cell makes exactly ``moves`` moves:

  many-small   256 cells of 24 atoms: 6,144 atoms, 63 moves;
  x5           one 3,000-atom cell, 63 moves;
  x10          one 24,000-atom cell, 15 moves, the held lists through the grid rows.
(63 and 15: with the evaluation that meets the step limit a whole number of looks at check_every = 16, unless a cell freezes.)

Per shape, whole calls on PeriodicCell objects built before the clock starts, host clock, synchronised, alternated, best of 5 rounds
with the spread (max - min), divided by the moves:
  (a) cells.relax;
  (b) the only way to do it without it: a Python loop of cells.lattice_energy (new PeriodicCells from the current coordinates at
      every move: that is its interface) plus the same FIRE update as float64 torch ops on the device tensors, every cell of the
      batch at once; no lists to hold, so no freeze rule.  The final energies of (a) and (b) are compared.
By device events, on prepared arrays: the launches of one iteration alone (real over the held rows, amplitudes, reciprocal, finish,
step); by the host clock the search of the held lists at r_cut + skin.  No ratio is gated.  A run without a GPU fails.

  python tools/cell_relax_time.py                        # -> profiles/cell_relax_time.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 5
R_CUT, SHORT_CUT, ACCURACY, SKIN, F_MAX = 10.0, 5.5, 1e-8, 1.0, 1e-12


def _best(times, moves):
    return dict(ms_per_move=round(min(times) * 1e3 / moves, 4), call_ms=round(min(times) * 1e3, 3), spread_ms=round((max(times) - min(times)) * 1e3, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_relax_time.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/cell_relax_time.py measures on the GPU: no device visible")
    import diffusion_model_amd as dma
    from diffusion_model_amd import _lib, cells as DC
    from tests import _cell_ewald_util as EU
    from tests import _cell_grid_util as GU

    periodic = lambda c: dma.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=2, id=c["name"])
    BKS, fire = DC.BKS, DC.FireParameters()
    model = dict(r_cut=R_CUT, short_cut=SHORT_CUT, accuracy=ACCURACY, device="cuda")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def events(fn, reps=5, before=None):
        best = float("inf")
        for _ in range(reps):
            if before is not None:
                before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            best = min(best, a.elapsed_time(b))
        return round(best, 4)

    def python_loop(pcs, moves, method):
        """(b): lattice_energy at every move, FIRE as torch ops over [C, n, 3] -> the final energies [C]"""
        C, n = len(pcs), pcs[0].num_atoms
        L = torch.stack([c.lattice for c in pcs]).cuda()
        Li = torch.linalg.inv(L)
        u = torch.stack([c.frac for c in pcs]).cuda()
        v = torch.zeros_like(u)
        dt = torch.full((C,), fire.dt, dtype=torch.float64, device="cuda")
        a = torch.full((C,), fire.a_start, dtype=torch.float64, device="cuda")
        n_pos = torch.zeros(C, dtype=torch.int64, device="cuda")
        energy = None
        for k in range(moves + 1):
            u_h = u.cpu()
            now = [dma.PeriodicCell(c.lattice, u_h[i], types=c.types, num_types=2) for i, c in enumerate(pcs)]
            res = DC.lattice_energy(now, BKS.charges, BKS.potential, method=method, **model)
            energy, F = res.energy, res.forces.reshape(C, n, 3)
            if k == moves:
                break
            P, FF, vv = (F * v).sum((1, 2)), (F * F).sum((1, 2)), (v * v).sum((1, 2))
            up = P > 0
            mixed = (1 - a)[:, None, None] * v + (a * vv.sqrt() / FF.sqrt())[:, None, None] * F
            grow = up & (n_pos > fire.n_min)
            dt = torch.where(grow, torch.clamp(dt * fire.f_inc, max=fire.dt_max), torch.where(up, dt, dt * fire.f_dec))
            a = torch.where(grow, a * fire.f_a, torch.where(up, a, torch.full_like(a, fire.a_start)))
            n_pos = torch.where(up, n_pos + 1, torch.zeros_like(n_pos))
            v = torch.where(up[:, None, None], mixed, torch.zeros_like(v)) + dt[:, None, None] * F
            dr = dt[:, None, None] * v
            m = dr.norm(dim=2).amax(1)
            dr = dr * torch.where(m > fire.max_step, fire.max_step / m, torch.ones_like(m))[:, None, None]
            u = u + dr @ Li
        return energy

    rng = np.random.default_rng(0)
    shapes = [("many-small", [GU.displaced_cristobalite(1, seed=int(s)) for s in rng.integers(0, 1 << 30, 256)], "auto", 63),
              ("x5", [GU.displaced_cristobalite(5)], "auto", 63),
              ("x10", [GU.displaced_cristobalite(10)], "grid", 15)]
    warm = periodic(GU.displaced_cristobalite(1))
    DC.relax(warm, BKS.charges, BKS.potential, max_steps=2, **model)                                  # code objects loaded
    DC.lattice_energy(warm, BKS.charges, BKS.potential, **model)
    record = dict(r_cut=R_CUT, short_cut=SHORT_CUT, accuracy=ACCURACY, skin=SKIN, f_max=F_MAX, rounds=ROUNDS, fire=vars(fire), shapes={})
    lib = _lib.lib()
    for name, cell_dicts, method, moves in shapes:
        pcs = [periodic(c) for c in cell_dicts]
        case = EU.make_case(cell_dicts[0], BKS.charges, EU.bks_tables(), r_cut=R_CUT, short_cut=SHORT_CUT, accuracy=ACCURACY)
        out = dict(cells=len(pcs), atoms=sum(len(c["frac"]) for c in cell_dicts), method=method, moves=moves)
        run = lambda: DC.relax(pcs, BKS.charges, BKS.potential, f_max=F_MAX, max_steps=moves, skin=SKIN, method=method, **model)
        t_relax, t_loop = [], []
        for _ in range(ROUNDS):                                                                       # alternated
            t, res = wall(run)
            t_relax.append(t)
            t, e_loop = wall(lambda: python_loop(pcs, moves, method))
            t_loop.append(t)
        assert res.steps.tolist() == [moves] * len(pcs)
        out["relax"], out["python_loop"] = _best(t_relax, moves), _best(t_loop, moves)
        out["ratio_loop_over_relax"] = round(min(t_loop) / min(t_relax), 2)
        out["iterations"] = int(res.iterations)
        out["relax"]["ms_per_iteration"] = round(min(t_relax) * 1e3 / res.iterations, 4)
        out["rebuilds_max"], out["rebuilds_total"] = int(res.n_rebuilds.max()), int(res.n_rebuilds.sum())
        out["largest_move_A"] = float(res.displacement.norm(dim=1).max())
        out["energy_per_atom_eV"] = [float(res.initial_energy.sum() / out["atoms"]), float(res.energy.sum() / out["atoms"])]
        out["max_energy_difference_to_loop_eV"] = float((res.energy - e_loop).abs().max())
        assert out["max_energy_difference_to_loop_eV"] < 1e-3
        # the launches of one iteration alone, on prepared arrays
        cb = DC._CellBatch(pcs, "cuda")
        cb.frac.copy_(DC._wrap(cb.frac))
        search = DC._SiteSearch(cb, R_CUT + SKIN, method)
        idx_h, cell_h = DC._centres(cb, None)
        ts = []
        for _ in range(ROUNDS):
            t, (row_ptr, atom, code) = wall(lambda: search.rows(idx_h, cell_h))
            ts.append(t)
        out["held_list_search_ms"] = round(min(ts) * 1e3, 3)
        out["held_sites"] = T = int(atom.shape[0])
        N, C = cb.N, cb.C
        who = torch.cat([idx_h.to(torch.int32), torch.arange(N, dtype=torch.int32)]).cuda()
        rows = (N, _lib.ptr(row_ptr), T, _lib.ptr(atom), _lib.ptr(code), N, _lib.ptr(who[:N]), _lib.ptr(who[N:]))
        q_h, pot_h = np.ascontiguousarray(case["charges"]), case["pot"]
        q_ptr, pot_ptr = _lib.host_ptr(q_h), _lib.host_ptr(pot_h)
        ew = (case["kappa"], case["alpha"], R_CUT, case["k_max"])
        f64 = dict(dtype=torch.float64, device="cuda")
        real, flag = torch.empty(N, 5, **f64), torch.zeros(C, dtype=torch.int32, device="cuda")
        head = cb.args(A=True, types=True)
        out["real_ms"] = events(lambda: _lib.check(lib.egnn_cell_relax_real(*head, q_ptr, pot_ptr, 24, 1, case["kappa"], case["alpha"], R_CUT, SHORT_CUT,
                                                                            case["k_max"], SKIN, *rows, _lib.ptr(real), _lib.ptr(flag))))
        vecs = DC._SqVectors(cb, case["k_max"], "k_max")
        hkl = torch.empty(max(vecs.K, 1), 3, dtype=torch.int32, device="cuda")
        table, rec = torch.empty(max(vecs.K, 1), 5, **f64), torch.empty(N, 4, **f64)
        amp_head = cb.args(A=True, types=True, host=(_lib.ptr(vecs.plan_h), _lib.ptr(vecs.vec_ptr_h)), dev=(_lib.ptr(vecs.plan), _lib.ptr(vecs.vec_ptr)))
        out["amplitudes_ms"] = events(lambda: _lib.check(lib.egnn_cell_ewald_amplitudes(*amp_head, q_ptr, *ew, vecs.n_rows, _lib.ptr(vecs.row_ptr), vecs.K,
                                                                                        _lib.ptr(vecs.tiles), vecs.n_tiles, _lib.ptr(hkl), _lib.ptr(table))))
        rec_head = cb.args(A=True, types=True, host=(_lib.ptr(vecs.vec_ptr_h),), dev=(_lib.ptr(vecs.vec_ptr),))
        out["reciprocal_ms"] = events(lambda: _lib.check(lib.egnn_cell_ewald_recip(*rec_head, q_ptr, *ew, 1, vecs.K, _lib.ptr(hkl), _lib.ptr(table),
                                                                                   _lib.ptr(rec))))
        n_type = torch.empty(C, 2, dtype=torch.int32, device="cuda")
        comp_atom, e_atom, force = torch.empty(N, 5, **f64), torch.empty(N, **f64), torch.empty(N, 3, **f64)
        comp, energy = torch.empty(C, 5, **f64), torch.empty(C, **f64)
        out["finish_ms"] = events(lambda: _lib.check(lib.egnn_cell_ewald_finish(*cb.args(A=True, frac=False, types=True), q_ptr, *ew, _lib.ptr(real),
                                                                                _lib.ptr(rec), _lib.ptr(n_type), _lib.ptr(comp_atom), _lib.ptr(e_atom),
                                                                                _lib.ptr(force), _lib.ptr(comp), _lib.ptr(energy))))
        assert np.array_equal(energy.cpu().numpy(), res.initial_energy.cpu().numpy())                 # the held rows at the build: lattice_energy's sites
        state = [torch.zeros(N, 3, **f64) for _ in range(3)]
        scalars = torch.zeros(C, 5, **f64)
        scalars[:, 0], scalars[:, 1] = fire.dt, fire.a_start
        counters, flags = torch.zeros(C, _lib.RELAX_COUNTERS, dtype=torch.int32, device="cuda"), torch.ones(2, C, dtype=torch.int32, device="cuda")
        flags[0] = 0                # rebuild set: the kernel reads the flags of every cell and returns
        step = lambda: _lib.check(lib.egnn_cell_relax_step(_lib.stream_ptr(), C, N, *cb._host_ptrs, *cb._dev_ptrs[:2], _lib.ptr(force), _lib.ptr(energy),
                                                           _lib.ptr(flag), *fire.step_args(), F_MAX, 1 << 30, SKIN, _lib.ptr(cb.frac),
                                                           *(_lib.ptr(t) for t in state), _lib.ptr(scalars), _lib.ptr(counters), _lib.ptr(flags[0]),
                                                           _lib.ptr(flags[1]), None, None))
        out["step_idle_ms"] = events(step)
        def moving():               # every repeat starts as a cell does after a build; the coordinates of this prepared batch change
            state[1].zero_()
            flags.zero_()
        out["step_ms"] = events(step, before=moving)
        kernels = out["real_ms"] + out["amplitudes_ms"] + out["reciprocal_ms"] + out["finish_ms"] + out["step_ms"]
        out["launches_ms"] = round(kernels, 4)
        out["bound_by"] = ("the host side of an iteration (five library calls, their checks and ten launches)"
                           if out["relax"]["ms_per_move"] > 2 * kernels else "the kernels of the evaluation")
        record["shapes"][name] = out
        print(name, json.dumps(out), flush=True)
    record["not_measured"] = ["hardware counters", "cells above 24,000 atoms", "other cutoffs, accuracies and skins", "a relaxation to convergence "
                              "at 3,000 and 24,000 atoms (63 and 15 moves were timed)", "the iterations a frozen cell idles until the next look",
                              "a captured graph of the iteration (none is implemented)", "dropping finished cells from the launches (not implemented)"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

"""Time the strain derivative of the lattice energy (csrc/cells/cell_ewald.hip, section 5, through
cells.lattice_energy(..., stress=True)) on the shapes of tools/cell_ewald_time.py: displaced beta-cristobalite with BKS at
r_cut = 10 A, short_cut = 5.5 A, accuracy = 1e-8, forces included:

  many-small   256 cells of 24 atoms (image box 2): 6,144 atoms;
  x5           one 3,000-atom cell;
  x10          one 24,000-atom cell, the site search through the grid rows.

Whole calls on PeriodicCell objects built before the clock starts, host clock, synchronised: ``stress=True`` against ``stress=False``
of the same build, alternated, best of 5 rounds with the spread (max - min).  By device events, on prepared arrays: the three new
launches alone (virial real, virial reciprocal, virial finish) beside the two launches whose walk they repeat (real, reciprocal),
and one line on what bounds each.  The outputs of the prepared launches are asserted bitwise those of the whole call.

``--parent DIR`` names a checkout of the parent commit with its library built: ``stress=False`` of this build is then timed against
the parent's ``lattice_energy`` in fresh worker processes (one per build and round, alternated, one timed call a shape after a
warm-up call), best of 5 with the spread; the record states whether this build is slower than the parent by more than that spread,
the one time that is gated.  Without ``--parent`` the record says that the comparison was not made.  A run without a GPU fails.

  python tools/cell_stress_time.py [--parent DIR]        # -> profiles/cell_stress_time.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROUNDS = 5
R_CUT, SHORT_CUT, ACCURACY = 10.0, 5.5, 1e-8
BOUNDS = dict(virial_real="the VALU: erfc, exp and the pair potential in fp64 per site, as the real-space launch, plus twelve products",
              virial_recip="the VALU: one sincospi a (vector, atom) term, as the reciprocal launch; B_m is one division and a dozen products",
              virial_finish="latency: one thread an atom, then one wavefront a cell adding its atoms in ascending order (36 lanes busy)")


def _best(times):
    return dict(ms=round(min(times) * 1e3, 3), spread_ms=round((max(times) - min(times)) * 1e3, 3))


def _shapes():
    from tests import _cell_grid_util as GU
    rng = np.random.default_rng(0)
    return [("many-small", [GU.displaced_cristobalite(1, seed=int(s)) for s in rng.integers(0, 1 << 30, 256)], "auto"),
            ("x5", [GU.displaced_cristobalite(5)], "auto"),
            ("x10", [GU.displaced_cristobalite(10)], "grid")]


def _wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def worker(package_root):
    """one warm-up and one timed ``lattice_energy`` (the defaults of the parent: no stress) a shape with the package under
    ``package_root``; the shapes come from this tree's tests/ -> one JSON line {shape: seconds}"""
    sys.path.insert(0, package_root)
    import torch
    import diffusion_model_amd as dma
    from diffusion_model_amd import cells as DC
    assert os.path.realpath(os.path.dirname(os.path.dirname(dma.__file__))) == os.path.realpath(package_root), dma.__file__
    sys.path.append(ROOT)
    out = {}
    for name, cell_dicts, method in _shapes():
        pcs = [dma.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=2, id=c["name"]) for c in cell_dicts]
        call = lambda: DC.lattice_energy(pcs, DC.BKS.charges, DC.BKS.potential, method=method, r_cut=R_CUT, short_cut=SHORT_CUT, accuracy=ACCURACY,
                                         device="cuda")
        call()
        out[name] = _wall(torch, call)[0]
    print("WORKER " + json.dumps(out), flush=True)


def against_parent(parent):
    """stress=False of this build against the parent's lattice_energy: fresh processes, alternated"""
    times = {"this": {}, "parent": {}}
    for _ in range(ROUNDS):
        for who, root in (("this", ROOT), ("parent", parent)):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", root], capture_output=True, text=True, timeout=600)
            lines = [l for l in r.stdout.splitlines() if l.startswith("WORKER ")]
            if r.returncode != 0 or not lines:
                raise SystemExit(f"the worker of {who} failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            for shape, t in json.loads(lines[-1][7:]).items():
                times[who].setdefault(shape, []).append(t)
    out = {}
    for shape in times["this"]:
        a, b = _best(times["this"][shape]), _best(times["parent"][shape])
        spread = max(a["spread_ms"], b["spread_ms"])
        out[shape] = dict(this_build=a, parent=b, difference_ms=round(a["ms"] - b["ms"], 3), spread_ms=spread,
                          slower_than_the_parent_by_more_than_the_spread=bool(a["ms"] - b["ms"] > spread))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_stress_time.json"))
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker)
    # the workers run first, while this process has not opened the device: every process that touches it is then a fresh one
    parent_record = against_parent(os.path.abspath(args.parent)) if args.parent else "not measured: no --parent checkout was given"
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/cell_stress_time.py measures on the GPU: no device visible")
    import diffusion_model_amd as dma
    from diffusion_model_amd import _lib, cells as DC
    from tests import _cell_ewald_util as EU

    periodic = lambda c: dma.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=2, id=c["name"])
    kw = dict(r_cut=R_CUT, short_cut=SHORT_CUT, accuracy=ACCURACY, device="cuda")
    BKS = DC.BKS

    def events(fn, reps=5):
        best = float("inf")
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            best = min(best, a.elapsed_time(b))
        return round(best, 3)

    shapes = _shapes()
    for flag in (False, True):
        DC.lattice_energy(periodic(shapes[0][1][0]), BKS.charges, BKS.potential, stress=flag, **kw)      # code objects loaded
    record = dict(r_cut=R_CUT, short_cut=SHORT_CUT, accuracy=ACCURACY, rounds=ROUNDS, bounds=BOUNDS, shapes={})
    lib = _lib.lib()
    for name, cell_dicts, method in shapes:
        pcs = [periodic(c) for c in cell_dicts]
        case = EU.make_case(cell_dicts[0], BKS.charges, EU.bks_tables(), r_cut=R_CUT, short_cut=SHORT_CUT, accuracy=ACCURACY)
        out = dict(cells=len(pcs), atoms=sum(len(c["frac"]) for c in cell_dicts), method=method)
        off, on = [], []
        for _ in range(ROUNDS):                                     # alternated
            t, plain = _wall(torch, lambda: DC.lattice_energy(pcs, BKS.charges, BKS.potential, method=method, **kw))
            off.append(t)
            t, res = _wall(torch, lambda: DC.lattice_energy(pcs, BKS.charges, BKS.potential, method=method, stress=True, **kw))
            on.append(t)
        out["call_stress_off"], out["call_stress_on"] = _best(off), _best(on)
        out["stress_on_over_off"] = round(min(on) / min(off), 3)
        assert torch.equal(plain.energy, res.energy) and torch.equal(plain.forces, res.forces)
        out["pressure_GPa_mean"] = float(res.pressure.mean()) * DC.EV_PER_A3_IN_GPA
        out["vectors"] = int(res.n_vectors.sum())
        # the launches alone, on prepared arrays
        cb = DC._CellBatch(pcs, "cuda")
        search = DC._SiteSearch(cb, R_CUT, method)
        idx_h, cell_h = DC._centres(cb, None)
        row_ptr, atom, code = search.rows(idx_h, cell_h)
        out["sites"] = T = int(atom.shape[0])
        who = torch.cat([idx_h.to(torch.int32), torch.arange(cb.N, dtype=torch.int32)]).cuda()
        rows = (cb.N, _lib.ptr(row_ptr), T, _lib.ptr(atom), _lib.ptr(code), cb.N, _lib.ptr(who[:cb.N]), _lib.ptr(who[cb.N:]))
        q_h, pot_h = np.ascontiguousarray(case["charges"]), case["pot"]
        q_ptr, pot_ptr = _lib.host_ptr(q_h), _lib.host_ptr(pot_h)
        ew = (case["kappa"], case["alpha"], R_CUT, case["k_max"])
        f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device="cuda")
        real, v_real, flag = f64(cb.N, 5), f64(cb.N, 12), torch.zeros(cb.C, dtype=torch.int32, device="cuda")
        head = cb.args(A=True, types=True)
        out["real_ms"] = events(lambda: _lib.check(lib.egnn_cell_ewald_real(*head, q_ptr, pot_ptr, 24, 1, case["kappa"], case["alpha"], R_CUT, SHORT_CUT,
                                                                            case["k_max"], 1, *rows, _lib.ptr(real), _lib.ptr(flag))))
        out["virial_real_ms"] = events(lambda: _lib.check(lib.egnn_cell_ewald_virial_real(*head, q_ptr, pot_ptr, 24, 1, case["kappa"], case["alpha"], R_CUT,
                                                                                          SHORT_CUT, case["k_max"], *rows, _lib.ptr(v_real),
                                                                                          _lib.ptr(flag))))
        vecs = DC._SqVectors(cb, case["k_max"], "k_max")
        hkl = torch.empty(max(vecs.K, 1), 3, dtype=torch.int32, device="cuda")
        table, rec, v_rec = f64(max(vecs.K, 1), 5), f64(cb.N, 4), f64(cb.N, 6)
        amp_head = cb.args(A=True, types=True, host=(_lib.ptr(vecs.plan_h), _lib.ptr(vecs.vec_ptr_h)), dev=(_lib.ptr(vecs.plan), _lib.ptr(vecs.vec_ptr)))
        _lib.check(lib.egnn_cell_ewald_amplitudes(*amp_head, q_ptr, *ew, vecs.n_rows, _lib.ptr(vecs.row_ptr), vecs.K, _lib.ptr(vecs.tiles), vecs.n_tiles,
                                                  _lib.ptr(hkl), _lib.ptr(table)))
        rec_head = cb.args(A=True, types=True, host=(_lib.ptr(vecs.vec_ptr_h),), dev=(_lib.ptr(vecs.vec_ptr),))
        out["reciprocal_ms"] = events(lambda: _lib.check(lib.egnn_cell_ewald_recip(*rec_head, q_ptr, *ew, 1, vecs.K, _lib.ptr(hkl), _lib.ptr(table),
                                                                                   _lib.ptr(rec))))
        out["virial_recip_ms"] = events(lambda: _lib.check(lib.egnn_cell_ewald_virial_recip(*rec_head, q_ptr, *ew, vecs.K, _lib.ptr(hkl), _lib.ptr(table),
                                                                                            _lib.ptr(v_rec))))
        n_type = torch.empty(cb.C, 2, dtype=torch.int32, device="cuda")
        d_comp_atom, d_atom, d_comp = f64(cb.N, 5, 6), f64(cb.N, 6), f64(cb.C, 5, 6)
        d_cell, sigma, pressure = f64(cb.C, 6), f64(cb.C, 6), f64(cb.C)
        out["virial_finish_ms"] = events(lambda: _lib.check(lib.egnn_cell_ewald_virial_finish(
            *cb.args(A=True, frac=False, types=True), q_ptr, *ew, _lib.ptr(v_real), _lib.ptr(v_rec), _lib.ptr(n_type), _lib.ptr(d_comp_atom),
            _lib.ptr(d_atom), _lib.ptr(d_comp), _lib.ptr(d_cell), _lib.ptr(sigma), _lib.ptr(pressure))))
        assert torch.equal(DC._voigt_to_3x3(sigma), res.stress) and torch.equal(pressure, res.pressure)
        assert torch.equal(DC._voigt_to_3x3(d_atom), res.strain_derivative_per_atom)
        out["new_launches_ms"] = round(out["virial_real_ms"] + out["virial_recip_ms"] + out["virial_finish_ms"], 3)
        record["shapes"][name] = out
        print(name, json.dumps(out), flush=True)
    record["stress_off_against_the_parent"] = parent_record
    print("parent", json.dumps(parent_record), flush=True)
    record["not_measured"] = ["hardware counters", "other cutoffs and accuracies", "cells above 24,000 atoms",
                              "the host statement's time (tools/cell_ewald_time.py times the energy's)"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

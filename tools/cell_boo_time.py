"""Time the bond-orientational order of periodic cells (csrc/cells/cell_boo.hip through cells.bond_order) on displaced
beta-cristobalite, the Si-Si select at cutoff 3.4 A, l_max = 6, the averages and the solid bonds at l = 6 included, every atom a centre:

  many-small   256 cells of 24 atoms (image box 1): 6,144 atoms;
  x5           one 3,000-atom cell;
  x10          one 24,000-atom cell, method "direct" against "grid".

Whole calls on uploaded cells (the PeriodicCell objects are built before the clock starts; the call uploads them and builds nothing
else: the N_lm and G tables are cached by the warm-up call), host clock, synchronised, best of 5 alternated rounds with the spread
(max - min) reported.  Baselines, one thread each:
  (a) egnn_cell_boo_host, whole, on many-small and x5 (its site walk is quadratic in the cell: not run at 24,000 atoms, said so in
      the record); the device must equal it BITWISE, asserted;
  (b) the numpy restatement tests/_cell_boo_util.restated on ONE 24-atom cell, scaled by 256 for many-small (said so in the record);
      it must equal the device bitwise too.
By device events, on prepared arrays: pass 1 (egnn_cell_boo_qlm) and pass 2 (egnn_cell_boo_invariants) alone, and by the host clock
the site search (_SiteSearch.rows: the site kernels or the linked-cell bond list plus torch's prefix sums); the record says which
bounds the call.  Nothing here is an estimate except the scaling of (b): a run without a GPU fails.

  python tools/cell_boo_time.py                        # -> profiles/cell_boo_time.json
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
CUTOFF, L_MAX, SELECT = 3.4, 6, [(1, 1)]
FIELDS = ("q", "w", "w_hat", "q_avg", "w_avg", "w_hat_avg", "n", "n_solid")


def _best(times):
    return dict(ms=round(min(times) * 1e3, 3), spread_ms=round((max(times) - min(times)) * 1e3, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_boo_time.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/cell_boo_time.py measures on the GPU: no device visible")
    import diffusion_model_amd as dma
    from diffusion_model_amd import _lib, cells as DC
    from tests import _cell_boo_util as BU
    from tests import _cell_grid_util as GU

    periodic = lambda c: dma.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=2, id=c["name"])
    kw = dict(cutoff=CUTOFF, l_max=L_MAX, select=SELECT, l_solid=6, threshold=0.7, device="cuda")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

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

    def arrays(bo):
        return {k: getattr(bo, k).cpu().numpy() for k in FIELDS}

    rng = np.random.default_rng(0)
    shapes = [("many-small", [GU.displaced_cristobalite(1, seed=int(s)) for s in rng.integers(0, 1 << 30, 256)], ("auto",), True),
              ("x5", [GU.displaced_cristobalite(5)], ("auto",), True),
              ("x10", [GU.displaced_cristobalite(10)], ("direct", "grid"), False)]
    DC.bond_order(periodic(GU.displaced_cristobalite(1)), **kw)       # code objects loaded, tables built and cached
    mask = BU.select_mask(SELECT, 2)
    norm_h, off_h, gidx_h, gval_h = DC._boo_tables(L_MAX)
    norm, off, gidx, gval = (torch.from_numpy(a).cuda() for a in (norm_h, off_h, gidx_h, gval_h))
    record = dict(cutoff=CUTOFF, l_max=L_MAX, select=SELECT, rounds=ROUNDS, shapes={})
    for name, cells, methods, with_host in shapes:
        pcs = [periodic(c) for c in cells]
        out = dict(cells=len(cells), atoms=sum(len(c["frac"]) for c in cells))
        times, results = {m: [] for m in methods}, {}
        for _ in range(ROUNDS):                                       # alternated
            for m in methods:
                t, results[m] = wall(lambda: DC.bond_order(pcs, method=m, **kw))
                times[m].append(t)
        for m in methods:
            out[f"call_{m}"] = _best(times[m])
        first = arrays(results[methods[0]])
        for m in methods[1:]:
            same = all(np.array_equal(arrays(results[m])[k], first[k]) for k in FIELDS)
            out[f"{m}_equals_{methods[0]}_bitwise"] = bool(same)
            assert same
        out["kept_sites"] = int(first["n"].sum())
        out["solid_atoms"] = int((first["n_solid"][first["n"] > 0] == first["n"][first["n"] > 0]).sum())
        # the parts alone
        cb = DC._CellBatch(pcs, "cuda")
        search = DC._SiteSearch(cb, CUTOFF, methods[-1])
        idx_h, cell_h = DC._centres(cb, None)
        ts = []
        for _ in range(ROUNDS):
            t, (row_ptr, atom, code) = wall(lambda: search.rows(idx_h, cell_h))
            ts.append(t)
        out[f"site_search_{methods[-1]}"] = _best(ts)
        out["raw_sites"] = T = int(atom.shape[0])
        who = torch.cat([idx_h.to(torch.int32), torch.arange(cb.N, dtype=torch.int32)]).cuda()
        head = (_lib.stream_ptr(), cb.C, cb.N, cb.A, _lib.ptr(cb.cell_ptr_h), _lib.ptr(cb.lattice_h), _lib.ptr(cb.cell_ptr), _lib.ptr(cb.lattice),
                _lib.ptr(cb.frac), _lib.ptr(cb.types))
        rows = (cb.N, _lib.ptr(row_ptr), T, _lib.ptr(atom), _lib.ptr(code), cb.N, _lib.ptr(who[:cb.N]), _lib.ptr(who[cb.N:]))
        qlm = torch.empty(cb.N, (L_MAX + 1) ** 2, dtype=torch.float64, device="cuda")
        n = torch.empty(cb.N, dtype=torch.int32, device="cuda")
        ns = torch.empty(cb.N, dtype=torch.int32, device="cuda")
        inv = torch.empty(cb.N, 6, L_MAX + 1, dtype=torch.float64, device="cuda")
        lib = _lib.lib()
        out["pass1_qlm_ms"] = events(lambda: _lib.check(lib.egnn_cell_boo_qlm(*head, CUTOFF, mask, L_MAX, _lib.ptr(norm), *rows, _lib.ptr(qlm), _lib.ptr(n))))
        out["pass2_invariants_ms"] = events(lambda: _lib.check(lib.egnn_cell_boo_invariants(
            *head, mask, L_MAX, _lib.ptr(qlm), len(gval_h), _lib.host_ptr(off_h), _lib.ptr(off), _lib.ptr(gidx), _lib.ptr(gval), 6, 0.7, 1, *rows,
            _lib.ptr(inv), _lib.ptr(n), _lib.ptr(ns))))
        assert np.array_equal(inv[:, 0].cpu().numpy(), first["q"]) and np.array_equal(inv[:, 5].cpu().numpy(), first["w_hat_avg"])
        kernels = out["pass1_qlm_ms"] + out["pass2_invariants_ms"]
        out["bound_by"] = ("the site search and the host side of the call" if out[f"site_search_{methods[-1]}"]["ms"] > kernels
                           else "the two kernels")
        if with_host:                                                 # (a) the host statement, whole, one thread
            t0 = time.perf_counter()
            rc, host = BU.host(lib, cells, CUTOFF, SELECT, 2, l_max=L_MAX, l_solid=6, threshold=0.7, qlm=False)
            out["host_statement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            assert rc == 0
            same = all(np.array_equal(host[k], first[k]) for k in FIELDS)
            out["device_equals_host_bitwise"] = bool(same)
            assert same
        if name == "many-small":                                      # (b) the numpy restatement on one cell, scaled
            t0 = time.perf_counter()
            r = BU.restated(cells[0], CUTOFF, SELECT, 2, l_max=L_MAX, l_solid=6, threshold=0.7)
            out["numpy_restatement_ms_scaled"] = round((time.perf_counter() - t0) * 1e3 * len(cells), 1)
            out["numpy_restatement_cells_timed"] = 1
            assert all(np.array_equal(r[k], first[k][:24]) for k in FIELDS)
        record["shapes"][name] = out
        print(name, json.dumps(out), flush=True)
    record["not_measured"] = ["hardware counters", "the host statement and the numpy restatement at 24,000 atoms (their site walk is quadratic)",
                              "cells above 24,000 atoms", "l_max other than 6 and selects other than Si-Si",
                              "the crossover size between the direct and the grid route at this cutoff"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

"""Time the SOAP descriptors of periodic cells (csrc/cells/cell_soap.hip through cells.soap_descriptors) at the default basis
(r_cut 8, n_max 15, l_max 10, sigma 0.1; cut 8.37 A) on displaced beta-cristobalite:

  many-small   256 cells of 24 atoms (image box 2), every atom: 6,144 centres;
  x5-O, x5     one 3,000-atom cell (box 1): every O (2,000 centres), and every atom;
  x10-listed   one 24,000-atom cell: 256 listed centres, method "direct" against "grid".

Whole calls on uploaded cells (the PeriodicCell objects are built before the clock starts; the call uploads them), host clock,
synchronised, best of 5 alternated rounds with the spread (max - min) reported.  Baselines:
  (a) what a user could do before this path existed: the numpy site enumeration of tests/_cell_soap_util.py into explicit float32
      clusters plus soap.soap_descriptors(centres="first"), counted WITH its host work (run once: it takes seconds); its float32
      vectors are a different input, so the difference is reported and held to the 1e-3 that the rounding of the vectors allows;
  (b) egnn_cell_soap_host on one thread, on the first HOST_CENTRES centres of the shape, scaled to the shape (said so in the record);
      equal results within the bar 8 x E_host of the GPU tests are asserted.
By device events, on prepared arrays: the site entries (egnn_cell_sites_count + prefix sum + _fill) and the descriptor entry
(egnn_cell_soap_descriptor) alone; the record says which bounds the call.  Nothing here is an estimate except the scaling of (b): a
run without a GPU fails.

  python tools/cell_soap_time.py                        # -> profiles/cell_soap_time.json
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
HOST_CENTRES = 16


def _best(times):
    return dict(ms=round(min(times) * 1e3, 3), spread_ms=round((max(times) - min(times)) * 1e3, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_soap_time.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/cell_soap_time.py measures on the GPU: no device visible")
    import diffusion_model_amd as dma
    from diffusion_model_amd import _lib, cells as DC, soap as DS
    from tests import _cell_grid_util as GU
    from tests import _cell_soap_util as CSU
    from tests import _soap_util as SU

    basis = dma.SoapBasis()
    cut, cfg, flat = basis.neighbour_cut, SU.CONFIGS["default"], np.ascontiguousarray(basis.tables)
    bar = CSU.bar("default")
    periodic = lambda c: dma.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=2, id=c["name"])

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

    def cluster_baseline(cells, idx):
        """(a): sites on the host in numpy, float32 clusters, the cluster kernel"""
        ptr = np.concatenate([[0], np.cumsum([len(c["frac"]) for c in cells])])
        pos, onehot, sizes = [], [], []
        for i in idx:
            c = int(np.searchsorted(ptr, i, side="right")) - 1
            j, _, r = CSU.sites(cells[c], cut, int(i) - ptr[c])
            t = cells[c]["types"]
            pos.append(np.concatenate([np.zeros((1, 3)), r]).astype(np.float32))
            onehot.append(np.eye(2, dtype=np.int64)[np.concatenate([[t[int(i) - ptr[c]]], t[j]])])
            sizes.append(len(j) + 1)
        return DS.soap_descriptors(torch.from_numpy(np.concatenate(pos)).cuda(), torch.from_numpy(np.concatenate(onehot)).cuda(), sizes,
                                   centres="first", basis=basis)

    shapes = []
    rng = np.random.default_rng(0)
    shapes.append(("many-small", [GU.displaced_cristobalite(1, seed=int(s)) for s in rng.integers(0, 1 << 30, 256)], None, ("auto",)))
    x5 = [GU.displaced_cristobalite(5)]
    shapes.append(("x5-O", x5, 0, ("auto",)))
    shapes.append(("x5", x5, None, ("auto",)))
    shapes.append(("x10-listed", [GU.displaced_cristobalite(10)], torch.from_numpy(np.sort(np.random.default_rng(1).permutation(24000)[:256])),
                   ("direct", "grid")))

    small = periodic(GU.displaced_cristobalite(1))
    DC.soap_descriptors(small, basis=basis, device="cuda")       # code objects loaded, tables uploaded
    record = dict(basis=cfg, cut=cut, rounds=ROUNDS, bar=bar, shapes={})
    for name, cells, centres, methods in shapes:
        pcs = [periodic(c) for c in cells]
        cb = DC._CellBatch(pcs, "cuda")
        idx_h, cell_h = DC._centres(cb, centres)
        idx = idx_h.numpy()
        out = dict(cells=len(cells), atoms=cb.N, centres=len(idx))
        times = {m: [] for m in methods}
        results = {}
        for _ in range(ROUNDS):                                  # alternated
            for m in methods:
                t, results[m] = wall(lambda: DC.soap_descriptors(pcs, centres=centres, basis=basis, method=m, device="cuda"))
                times[m].append(t)
        for m in methods:
            out[f"call_{m}"] = _best(times[m])
        first = results[methods[0]]
        for m in methods[1:]:
            out[f"{m}_equals_{methods[0]}_bitwise"] = bool(torch.equal(results[m], first))
            assert out[f"{m}_equals_{methods[0]}_bitwise"]
        # the entries alone
        search = DC._SiteSearch(cb, cut, "direct")
        dev_idx = idx_h.to(torch.int32).cuda()
        M = len(idx)
        head = (_lib.stream_ptr(), cb.C, cb.N, _lib.ptr(cb.cell_ptr_h), _lib.ptr(cb.lattice_h), _lib.ptr(cb.cell_ptr), _lib.ptr(cb.lattice),
                _lib.ptr(cb.frac), cut, M, _lib.ptr(dev_idx))
        deg = torch.empty(M, dtype=torch.int32, device="cuda")
        row_ptr, atom, code = search.rows(idx_h, cell_h)
        T = int(atom.shape[0])

        def site_entries():
            _lib.check(_lib.lib().egnn_cell_sites_count(*head, _lib.ptr(deg)))
            rp = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
            rp[1:] = torch.cumsum(deg.long(), 0).to(torch.int32)
            _lib.check(_lib.lib().egnn_cell_sites_fill(*head, _lib.ptr(rp), T, _lib.ptr(atom), _lib.ptr(code)))

        run = DC._CellSoap(pcs, basis, None, "direct", "cuda")
        step = run.slab_centres(False, DC._SOAP_SLAB_BYTES)
        m1 = min(M, step)
        rp1, at1, co1 = search.rows(idx_h[:m1], cell_h[:m1])
        who = torch.cat([idx_h[:m1].to(torch.int32), torch.arange(m1, dtype=torch.int32)]).cuda()
        desc = torch.empty(m1, run.F, dtype=torch.float64, device="cuda")

        def descriptor_entry():
            _lib.check(_lib.lib().egnn_cell_soap_descriptor(
                _lib.stream_ptr(), cb.C, cb.N, cb.A, _lib.ptr(cb.cell_ptr_h), _lib.ptr(cb.lattice_h), _lib.ptr(cb.cell_ptr), _lib.ptr(cb.lattice),
                _lib.ptr(cb.frac), _lib.ptr(cb.types), basis.n_max, basis.l_max, _lib.ptr(run.tables), m1, _lib.ptr(rp1), int(at1.shape[0]),
                _lib.ptr(at1), _lib.ptr(co1), m1, _lib.ptr(who[:m1]), _lib.ptr(who[m1:]), _lib.ptr(desc), None))

        out["sites"] = T
        out["slabs"] = -(-M // step)
        out["site_entries_ms"] = events(site_entries)
        per_slab = events(descriptor_entry)
        out["descriptor_entry_ms"] = round(per_slab * M / m1, 3)
        out["descriptor_entry_centres_timed"] = m1
        out["bound_by"] = "descriptor entry" if out["descriptor_entry_ms"] > out["site_entries_ms"] else "site entries"
        # (a) the cluster route, once
        t, base = wall(lambda: cluster_baseline(cells, idx))
        E = SU.descriptor_error(first.cpu().numpy(), base.cpu().numpy())
        out["baseline_clusters_ms_once"] = round(t * 1e3, 1)
        out["against_clusters"] = E
        # the clusters hold float32 vectors, a different input: a component of up to 8.37 A moves by up to 2^-24 of itself, 5e-7 A,
        # and a Gaussian factor exp(-gamma d^2), gamma <= 1 / (2 sigma^2) = 50, by up to 2 gamma d 5e-7 = 4e-4 relative
        assert E <= 1e-3, (name, E)
        # (b) the host statement on a few centres, scaled
        k = min(HOST_CENTRES, M)
        t0 = time.perf_counter()
        rc, hd, _ = CSU.host_soap(_lib.lib(), cells, 2, cfg, flat, idx[:k], coeff=False)
        t = time.perf_counter() - t0
        assert rc == 0
        Eh = SU.descriptor_error(first[:k].cpu().numpy(), hd)
        assert Eh <= bar, (name, Eh, bar)
        out["host_statement_ms_scaled"] = round(t * 1e3 * M / k, 1)
        out["host_statement_centres_timed"] = k
        out["against_host"] = Eh
        record["shapes"][name] = out
        print(name, json.dumps(out), flush=True)
    record["not_measured"] = ["hardware counters", "cells above 24,000 atoms", "every atom of the 24,000-atom cell", "bases other than the default",
                              "the crossover size between the direct and the grid route"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

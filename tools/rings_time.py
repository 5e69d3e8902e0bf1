"""Time the shortest-path ring statistics (csrc/eval/rings.hip through stats.ring_statistics / cells.ring_statistics: bond list, one
search per (centre, row position), EVERY atom a centre, max_size = 16, max_sites = 4096) on three shapes:

  256 clouds of 64 atoms (scale 1.5)      32 clouds of 512 atoms (scale 1.5)      1 cell of 3000 atoms (cutoff 2.0)

The cell is beta-cristobalite replicated 5 x 5 x 5 (the largest replica below 4096 atoms) with every fractional coordinate
displaced by sigma = 0.002; the clouds are the silica-like clouds of the tests.

  device     the whole Python call on prepared inputs (bond list, index plumbing, one launch, the overflow read-back and the
             per-centre reductions), host clock, synchronised.  And egnn_rings alone (its three memsets and the kernel), device
             events around back-to-back launches on prepared device arrays, at the max_sites the Python call passes on: 4096
             for the cell, the size of the largest graph for clouds (a search cannot label more sites than its graph has).
  host (a)   egnn_rings_host, the plain C++ statement, one thread, on the bond list the device built.
  python (b) restatement (i) of tests/_ring_util.py (dicts, level by level), once.

Equal outputs are asserted between all three.  Best of 5 alternated rounds.  Nothing here is an estimate: a run without a GPU fails.

  python tools/rings_time.py                       # -> profiles/rings_time.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_SIZE, MAX_SITES, SCALE, CUTOFF, REPLICAS = 16, 4096, 1.5, 2.0, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rings_time.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import diffusion_model_amd as dma
    from diffusion_model_amd import _lib, cells as DC, stats
    from tests import _cells_util as CU
    from tests import _ring_util as RU
    from tests import _topo_util as TU
    if not torch.cuda.is_available():
        raise SystemExit("tools/rings_time.py measures on the GPU: no device visible")
    dev = "cuda"
    L = _lib.lib()
    record = {"rounds": args.rounds, "warmup_calls": args.warmup, "settings": dict(max_size=MAX_SIZE, max_sites=MAX_SITES, scale=SCALE, cutoff=CUTOFF),
              "gcn_arch": torch.cuda.get_device_properties(0).gcnArchName, "shapes": {}}

    def wall(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls

    def events(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls

    shapes = []
    for B, n in ((256, 64), (32, 512)):
        pos, types = TU.cloud(900 + n, [n] * B, 2)
        p, x = torch.from_numpy(pos).to(dev), torch.nn.functional.one_hot(torch.from_numpy(types).long(), 2).to(dev)
        inp = stats._TopoInput(p, x, [n] * B, stats.COVALENT_RADII, SCALE, "rings_time")
        E = int(inp.row_ptr[-1])
        csr = dict(N=B * n, row_ptr=inp.row_ptr.cpu().numpy(), atom=inp.neighbours[:E].cpu().numpy(), shift=None, types=types.astype(np.int32), A=2)
        flow = (lambda p=p, x=x, B=B, n=n: stats.ring_statistics(p, x, [n] * B, scale=SCALE, max_size=MAX_SIZE, max_sites=MAX_SITES))
        shapes.append((f"{B}x{n} clouds", csr, flow, min(MAX_SITES, n)))     # what stats.ring_statistics passes on: the largest graph
    frac, types = CU._cristobalite_frac()
    off = np.array([[i, j, k] for i in range(REPLICAS) for j in range(REPLICAS) for k in range(REPLICAS)], dtype=np.float64)
    big = ((frac[None, :, :] + off[:, None, :]) / REPLICAS).reshape(-1, 3) + 0.002 * np.random.default_rng(3).standard_normal((len(off) * len(frac), 3))
    cell = dma.PeriodicCell(7.16 * REPLICAS * np.eye(3), big, types=np.tile(types, len(off)), num_types=2, id="cristobalite-5x5x5")
    bonds = dma.bond_list(cell, cutoff=CUTOFF, device=dev)
    csr = dict(N=cell.num_atoms, row_ptr=bonds.row_ptr.cpu().numpy(), atom=bonds.atom.cpu().numpy(),
               shift=np.ascontiguousarray(bonds.shift.cpu().numpy().astype(np.int32)), types=cell.types.numpy().astype(np.int32), A=2)
    shapes.append((f"1x{cell.num_atoms} cell", csr,
                   lambda: DC.ring_statistics(cell, cutoff=CUTOFF, max_size=MAX_SIZE, max_sites=MAX_SITES, device=dev), MAX_SITES))

    for name, csr, device_flow, kernel_sites in shapes:
        got = device_flow()
        rc, host = RU.host(L, csr, max_size=MAX_SIZE, max_sites=MAX_SITES)
        assert rc == 0, L.egnn_last_error()
        t0 = time.perf_counter()
        want = RU.restated(csr, max_size=MAX_SIZE, max_sites=MAX_SITES)
        python_ms = (time.perf_counter() - t0) * 1e3
        RU.assert_equal(host, want)
        assert np.array_equal(got.size.cpu().numpy(), want["size"]) and np.array_equal(got.count.cpu().numpy(), want["count"])
        assert np.array_equal(got.histogram.cpu().numpy(), want["hist"])

        def host_flow():
            return RU.host(L, csr, max_size=MAX_SIZE, max_sites=MAX_SITES)

        ctr = RU.all_centres(csr)
        apn = RU.angle_ptr(csr, ctr)
        n_angles = int(apn[-1])
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d = {k: up(csr[k]) for k in ("row_ptr", "atom", "shift", "types")}
        d_ctr, d_ap = up(ctr), up(apn)
        out = [torch.empty(max(k, 1), dtype=torch.int32, device=dev) for k in (n_angles, n_angles, len(ctr))]
        hist = torch.empty(2, MAX_SIZE + 1, dtype=torch.int32, device=dev)

        def kernel_flow():
            _lib.check(L.egnn_rings(_lib.stream_ptr(), csr["N"], _lib.ptr(d["row_ptr"]), len(csr["atom"]), _lib.ptr(d["atom"]), _lib.ptr(d["shift"]),
                                    _lib.ptr(d["types"]), 2, len(ctr), _lib.ptr(d_ctr), _lib.ptr(d_ap), n_angles, MAX_SIZE, kernel_sites,
                                    _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.ptr(hist), None, None, None, None))

        kernel_flow()
        assert np.array_equal(out[0].cpu().numpy()[:n_angles], host["size"]) and np.array_equal(hist.cpu().numpy(), host["hist"])
        wall(device_flow, args.warmup)
        events(kernel_flow, args.warmup)
        ms = {"device": [], "host": [], "kernel": []}
        for _ in range(args.rounds):                            # alternating
            ms["device"].append(wall(device_flow, 5))
            ms["host"].append(wall(host_flow, 1))
            ms["kernel"].append(events(kernel_flow, 10))
        searches = int(np.maximum(np.diff(csr["row_ptr"]) - 1, 0).sum())
        rec = {"kernel_max_sites": kernel_sites, "atoms": csr["N"], "bonds": len(csr["atom"]), "angles": n_angles, "searches": searches,
               "largest_search_sites": int(want["labelled"].max()), "ring_sizes": sorted(set(want["size"].tolist())),
               "largest_count": int(want["count"].max()),
               "device_ms_per_call_rounds": [round(v, 3) for v in ms["device"]], "device_ms_per_call": round(min(ms["device"]), 3),
               "kernel_ms_rounds": [round(v, 4) for v in ms["kernel"]], "kernel_ms": round(min(ms["kernel"]), 4),
               "kernel_us_per_search": round(min(ms["kernel"]) * 1e3 / max(searches, 1), 3),
               "host_ms_per_call_rounds": [round(v, 2) for v in ms["host"]], "host_ms_per_call": round(min(ms["host"]), 2),
               "host_over_device": round(min(ms["host"]) / min(ms["device"]), 2), "host_over_kernel": round(min(ms["host"]) / min(ms["kernel"]), 2),
               "python_restatement_ms_once": round(python_ms, 0), "python_over_device": round(python_ms / min(ms["device"]), 0)}
        record["shapes"][name] = rec
        print(name, json.dumps(rec), flush=True)
    record["note"] = ("device / host: host clock around whole calls, synchronised, best of the alternated rounds; the device call includes "
                      "building the bond list, the host call starts from it.  kernel_ms: device events around 10 back-to-back egnn_rings "
                      "calls (three memsets and the kernel) on prepared device arrays.  python_restatement: one run, not repeated.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(record, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

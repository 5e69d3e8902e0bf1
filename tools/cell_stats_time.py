"""Time the real-space statistics of periodic cells (csrc/cells/cell_stats.hip through cells.structure_profile: pair counts over the
image box, the bond list, coordination numbers, angles and Q^n; R = 10, dR = 0.01, default bond arguments) on three shapes:

  1 cell of 3000 atoms (the displaced beta-cristobalite 5 x 5 x 5 of tools/rings_time.py)
  32 random cells of 512 atoms (tests/_cells_util.py: random_cell)      256 displaced beta-cristobalite cells of 24 atoms

  device     the whole Python call cells.structure_profile on prepared PeriodicCells (upload, work lists, pair kernel, bond list,
             bond kernels, the fp64 finish), host clock, synchronised.  And the entries alone, device events around back-to-back
             launches on prepared device arrays: egnn_cell_pair_counts (one memset and the kernel) and egnn_cell_bond_stats (six
             memsets and two kernels).
  torch (a)  the same pair counts as batched fp64 torch ops on the same device tensors: explicit images -> site vectors ->
             distances -> floor(r / dR) -> index_add_ into an int64 histogram, in blocks of centres that keep a temporary below
             2^23 elements.  (floor(r / dR) rather than bucketize against the edges k dR: the definition, so that the integers
             can be compared.)
  host (b)   egnn_cell_stats_host, the plain C++ statement of every output, one thread.

Equal integer outputs are asserted between all three.  Best of 5 alternated rounds.  Nothing here is an estimate: a run without a
GPU fails.

  python tools/cell_stats_time.py                       # -> profiles/cell_stats_time.json
"""
import argparse
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R, DR, CUTOFF, REPLICAS = 10.0, 0.01, 2.0, 5
FP64_LANE_RATE = 39.3e12          # fp64 vector lane-instructions per second (README, structure factors)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_stats_time.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import diffusion_model_amd as dma
    from diffusion_model_amd import _lib, cells as DC
    from tests import _cell_stats_util as SU
    from tests import _cells_util as CU
    if not torch.cuda.is_available():
        raise SystemExit("tools/cell_stats_time.py measures on the GPU: no device visible")
    dev = "cuda"
    L = _lib.lib()
    nbins = SU.nbins_of(R, DR)
    record = {"rounds": args.rounds, "warmup_calls": args.warmup, "settings": dict(R=R, dR=DR, nbins=nbins, cutoff=CUTOFF, dtheta=1.0, max_cn=16),
              "gcn_arch": torch.cuda.get_device_properties(0).gcnArchName, "fp64_lane_rate": FP64_LANE_RATE, "shapes": {}}

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

    frac, types = CU._cristobalite_frac()
    off = np.array([[i, j, k] for i in range(REPLICAS) for j in range(REPLICAS) for k in range(REPLICAS)], dtype=np.float64)
    big = ((frac[None, :, :] + off[:, None, :]) / REPLICAS).reshape(-1, 3) + 0.002 * np.random.default_rng(3).standard_normal((len(off) * len(frac), 3))
    plain = lambda lattice, fr, ty, name: dict(lattice=np.asarray(lattice, np.float64), frac=fr, types=np.asarray(ty, np.int32), A=2, name=name, cutoff=CUTOFF)
    shapes = [("1x3000 cell", [plain(7.16 * REPLICAS * np.eye(3), big, np.tile(types, len(off)), "cristobalite-5x5x5")]),
              ("32x512 cells", [CU.random_cell(512, 700 + s, check=False) for s in range(32)]),
              ("256x24 cells", [plain(7.16 * np.eye(3), frac + 0.002 * np.random.default_rng(100 + s).standard_normal(frac.shape), types, f"cristobalite-{s}")
                                for s in range(256)])]

    def torch_counts(cb, boxes):
        """baseline (a): int64 [C, A, A, nbins] from fp64 torch ops on the tensors of the _CellBatch"""
        A = cb.A
        hist = torch.zeros(cb.C * A * A * nbins, dtype=torch.int64, device=cb.dev)
        w_all = cb.frac - torch.floor(cb.frac)
        w_all = torch.where(w_all < 1.0, w_all, torch.zeros_like(w_all))
        ptr = cb.cell_ptr_h.tolist()
        for c in range(cb.C):
            lo, hi = ptr[c], ptr[c + 1]
            n = hi - lo
            w, ty, Lc = w_all[lo:hi], cb.types[lo:hi].long(), cb.lattice[c].view(3, 3)
            img = torch.tensor(list(itertools.product(*(range(-int(s), int(s) + 1) for s in boxes[c]))), dtype=torch.float64, device=cb.dev)
            zero = int(torch.nonzero((img == 0).all(1))[0])
            step = max(1, (1 << 23) // max(n * len(img), 1))
            for i0 in range(0, n, step):
                wi = w[i0:i0 + step]
                d = (w[None, :, None, :] - wi[:, None, None, :]) + img[None, None, :, :]
                r = (d[..., 0:1] * Lc[0] + d[..., 1:2] * Lc[1]) + d[..., 2:3] * Lc[2]
                r2 = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
                k = torch.floor(torch.sqrt(r2) / DR)
                ok = k < nbins
                ci = torch.arange(len(wi), device=cb.dev)
                ok[ci, i0 + ci, zero] = False
                flat = ((c * A + ty[i0:i0 + len(wi)])[:, None, None] * A + ty[None, :, None]) * nbins + k.clamp(0, nbins - 1).long()
                hist.index_add_(0, flat.reshape(-1), ok.reshape(-1).long())
        return hist.view(cb.C, A, A, nbins)

    for name, cells in shapes:
        pcs = [dma.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=2, id=c["name"]) for c in cells]
        device_flow = lambda: DC.structure_profile(pcs, R=R, dR=DR, cutoff=CUTOFF, device=dev)
        got = device_flow()
        rc, host = SU.host(L, cells, dR=DR, nbins=nbins, cutoff=CUTOFF)
        assert rc == 0, L.egnn_last_error()
        assert np.array_equal(got.counts.cpu().numpy(), host["counts"])
        for k in ("coordination", "cn", "angles", "qn", "qn_hist"):
            assert np.array_equal(getattr(got, k).cpu().numpy(), host[k]), k
        assert not host["overflow"].any()

        cb = DC._CellBatch(pcs, dev)
        boxes = [SU.image_box(c["lattice"], DR, nbins) for c in cells]
        assert torch.equal(torch_counts(cb, boxes), got.counts)
        bonds = DC._bond_list(cb, CUTOFF)
        tiles = torch.from_numpy(DC._pair_tiles(cb.sizes, DC._image_boxes(cb, DR, nbins))).to(dev)
        bond_tiles = torch.from_numpy(DC._stat_bond_tiles(cb.sizes)).to(dev)
        host_flow = lambda: SU.host(L, cells, dR=DR, nbins=nbins, cutoff=CUTOFF)
        pair_flow = lambda: DC._pair_counts(cb, DR, nbins, tiles=tiles)
        bond_flow = lambda: DC._bond_stats(cb, bonds, 1.0, 16, 1, 0, tiles=bond_tiles)
        torch_flow = lambda: torch_counts(cb, boxes)
        wall(device_flow, args.warmup)
        events(pair_flow, args.warmup)
        events(bond_flow, args.warmup)
        ms = {"device": [], "host": [], "pair": [], "bond": [], "torch": []}
        for _ in range(args.rounds):                            # alternating
            ms["device"].append(wall(device_flow, 3))
            ms["host"].append(wall(host_flow, 1))
            ms["pair"].append(events(pair_flow, 10))
            ms["bond"].append(events(bond_flow, 10))
            ms["torch"].append(wall(torch_flow, 1))
        sizes = np.array(cb.sizes, dtype=np.int64)
        images = np.array([int(np.prod(2 * b + 1)) for b in boxes], dtype=np.int64)
        box_terms = int((sizes * sizes * images).sum() - sizes.sum())
        counted = int(host["counts"].sum())
        best = {k: min(v) for k, v in ms.items()}
        rec = {"cells": len(cells), "atoms": int(sizes.sum()), "pair_tiles": int(len(tiles)), "images_per_cell": int(images.max()),
               "bonds": bonds.num_bonds, "box_terms": box_terms, "counted_terms": counted,
               "device_ms_per_call_rounds": [round(v, 3) for v in ms["device"]], "device_ms_per_call": round(best["device"], 3),
               "pair_entry_ms_rounds": [round(v, 4) for v in ms["pair"]], "pair_entry_ms": round(best["pair"], 4),
               "bond_entry_ms_rounds": [round(v, 4) for v in ms["bond"]], "bond_entry_ms": round(best["bond"], 4),
               "torch_pair_ms_rounds": [round(v, 2) for v in ms["torch"]], "torch_pair_ms": round(best["torch"], 2),
               "host_ms_per_call_rounds": [round(v, 2) for v in ms["host"]], "host_ms_per_call": round(best["host"], 2),
               "torch_over_pair_entry": round(best["torch"] / best["pair"], 1), "host_over_device": round(best["host"] / best["device"], 2),
               "host_over_entries": round(best["host"] / (best["pair"] + best["bond"]), 1),
               "box_terms_per_s": float(f"{box_terms / (best['pair'] * 1e-3):.4g}"), "counted_terms_per_s": float(f"{counted / (best['pair'] * 1e-3):.4g}")}
        record["shapes"][name] = rec
        print(name, json.dumps(rec), flush=True)
    record["note"] = ("device / host / torch: host clock around whole calls, synchronised, best of the alternated rounds; the pair and bond entries: "
                      "device events around 10 back-to-back calls (their output allocations, memsets and kernels) on prepared device arrays and "
                      "work lists.  box_terms: (pair, image) terms of the image box, most of them skipped by the axis "
                      "culls; counted_terms: the terms that land in a bin.  The torch baseline computes the pair counts only; the host "
                      "statement computes every output.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(record, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

"""Time the local environments of periodic cells (csrc/cells/cell_env.hip through cells.local_environments: periodic bond list,
then the shell cluster about EVERY atom, shells = 4, cutoff 2.0, max_atoms 256) on three batch shapes:

  1 cell of 4096 atoms          32 cells of 512 atoms          256 cells of 24 atoms

  device     cells.local_environments(cells, shells=4) on prepared PeriodicCell objects: the whole call (packing, one upload, four
             kernels, two prefix sums, the two size read-backs, one-hot / exO), host clock, synchronised.  And the four kernels
             alone, device events around back-to-back launches on prepared inputs.  The bond passes are quoted as NOMINAL image
             pairs per second, 27 n^2 per cell and pass: the kernel skips an image whose fractional offset along one axis already
             rules a bond out, so fewer distances than that are evaluated in full.
  host (a)   egnn_cell_env_host, the plain C++ statement, on the same host, one thread, one call with known capacities.
  numpy (b)  the reference's supercell rule (make_dataset.py:79-111, :258-272) where its distance matrix still fits, the 24-atom
             cells: the 648 x 648 minimum-image distance matrix of the 3x3x3 supercell, then the neighbour selection nested four
             deep in Python, for ONE centre per cell (the first oxygen), as the reference runs it.  Quoted PER CENTRE and compared
             with the device's time per centre of the 256 x 24 batch.

The 4096- and 512-atom cells are random cells of the tests' construction (minimum separation 1.45 A, about 21 cubic angstrom per
atom); the 24-atom cells are triclinic distortions of beta-cristobalite.  Best of 5 alternated rounds.  Nothing here is an
estimate: a run without a GPU fails.

  python tools/cells_time.py                       # -> profiles/cells_time.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHELLS, CUTOFF, MAX_ATOMS = 4, 2.0, 256


def reference_supercell(np, CU, L, frac, centre, levels=4, cutoff=CUTOFF):
    """competitor (b): the full distance matrix of the 27 n supercell sites (minimum image in the tripled lattice), then the
    reference's nested loops over its rows -> sorted site indices, the centre first"""
    w = CU.wrap(frac)
    n = len(w)
    images = CU.IMAGES.astype(np.float64)
    X = ((w @ L)[:, None, :] + images @ L + np.ones(3) @ L).reshape(27 * n, 3)
    L3 = 3.0 * L
    F = X @ np.linalg.inv(L3)
    df = F[None, :, :] - F[:, None, :]
    df -= np.round(df)
    dist = np.full((27 * n, 27 * n), np.inf)
    for t in images:                                           # the 27 images the cell library scans
        dist = np.minimum(dist, np.linalg.norm((df + t) @ L3, axis=2))

    def within(ref):                                           # the sites closer than the cutoff to `ref`, itself left out
        near = np.nonzero(dist[ref] < cutoff)[0]
        return near[near != ref].tolist()

    c = 27 * centre + 13
    found = []

    def descend(idx, depth):
        near = within(idx)
        found.extend(near)
        if depth < levels:
            for j in near:
                descend(j, depth + 1)

    descend(c, 1)
    return [c] + [i for i in sorted(set(found)) if i != c]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reference-cells", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cells_time.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import diffusion_model_amd as dma
    from diffusion_model_amd import _lib, cells as DC
    from tests import _cells_util as CU
    if not torch.cuda.is_available():
        raise SystemExit("tools/cells_time.py measures on the GPU: no device visible")
    dev = "cuda"
    record = {"rounds": args.rounds, "warmup_calls": args.warmup, "settings": dict(shells=SHELLS, cutoff=CUTOFF, max_atoms=MAX_ATOMS),
              "gcn_arch": torch.cuda.get_device_properties(0).gcnArchName, "batches": {}}

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

    for C, n, calls_dev in ((1, 4096, 10), (32, 512, 10), (256, 24, 10)):
        if n == 24:
            raw = [CU.triclinic_cell(seed=1000 + c, check=False) for c in range(C)]
        else:
            raw = [CU.random_cell(n, 7000 + 37 * n + c, check=False) for c in range(C)]
        cells = [dma.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=2, id=k) for k, c in enumerate(raw)]
        L = _lib.lib()
        rc, host = CU.host_environments(L, raw, shells=SHELLS, max_atoms=MAX_ATOMS)
        assert rc == 0, L.egnn_last_error()
        caps = (len(host["bond_atom"]), len(host["atom"]))

        def device_flow():
            return dma.local_environments(cells, shells=SHELLS, cutoff=CUTOFF, max_atoms=MAX_ATOMS, device=dev)

        def host_flow():
            return CU.host_environments(L, raw, shells=SHELLS, max_atoms=MAX_ATOMS, caps=caps)

        env = device_flow()                                     # the timed code computes what the host statement computes
        assert env.sizes == host["size"].tolist() and np.array_equal(env.shift_code.cpu().numpy(), host["shift"])
        assert np.array_equal(env.pos.cpu().numpy().view(np.int32), host["pos"].view(np.int32))
        wall(device_flow, args.warmup)
        ms = {"device": [], "host": []}
        for _ in range(args.rounds):                            # alternating
            ms["device"].append(wall(device_flow, calls_dev))
            ms["host"].append(wall(host_flow, 1))
        cb = DC._CellBatch(cells, dev)
        bonds = DC._bond_list(cb, CUTOFF)
        centres = torch.arange(cb.N)
        cell_of = torch.searchsorted(cb.cell_ptr_h.long(), centres, right=True) - 1
        cc = torch.stack((cell_of, centres)).to(torch.int32).to(dev)
        env_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.tensor(env.sizes), 0)]).to(torch.int32).to(dev)
        T = int(env_ptr[-1])
        kernels = {"bonds_count": lambda: DC._bonds_count(cb, CUTOFF), "bonds_fill": lambda: DC._bonds_fill(cb, CUTOFF, bonds.row_ptr, bonds.num_bonds),
                   "env_count": lambda: DC._env_count(cb, bonds, cc, SHELLS, MAX_ATOMS),
                   "env_fill": lambda: DC._env_fill(cb, bonds, cc, SHELLS, MAX_ATOMS, env_ptr, T)}
        ms_k = {}
        for name, fn in kernels.items():
            events(fn, args.warmup)
            ms_k[name] = [events(fn, 20) for _ in range(args.rounds)]
        image_pairs = 27 * C * n * n
        rec = {"cells": C, "atoms_per_cell": n, "centres": C * n, "bonds": bonds.num_bonds, "environment_rows": T,
               "largest_environment": max(env.sizes), "bond_tiles": cb.n_tiles, "nominal_image_pairs_per_bond_pass": image_pairs,
               "device_ms_per_call_rounds": [round(v, 3) for v in ms["device"]], "device_ms_per_call": round(min(ms["device"]), 3),
               "device_us_per_centre": round(min(ms["device"]) * 1e3 / (C * n), 3),
               "host_ms_per_call_rounds": [round(v, 1) for v in ms["host"]], "host_ms_per_call": round(min(ms["host"]), 1),
               "host_over_device": round(min(ms["host"]) / min(ms["device"]), 1)}
        for name, v in ms_k.items():
            rec[f"{name}_kernel_ms_rounds"] = [round(x, 4) for x in v]
            rec[f"{name}_kernel_ms"] = round(min(v), 4)
        rec["bonds_count_nominal_image_pairs_per_second"] = round(image_pairs / (min(ms_k["bonds_count"]) * 1e-3), 0)
        rec["bonds_fill_nominal_image_pairs_per_second"] = round(image_pairs / (min(ms_k["bonds_fill"]) * 1e-3), 0)
        if n == 24:
            ref_ms = []
            for k, c in enumerate(raw[:args.reference_cells]):
                centre = int(np.nonzero(c["types"] == 0)[0][0])
                t0 = time.perf_counter()
                sites = reference_supercell(np, CU, c["lattice"], c["frac"], centre)
                ref_ms.append((time.perf_counter() - t0) * 1e3)
                want, wrapped, _, _ = CU.reference_environment(c["lattice"], c["frac"], centre, SHELLS)
                assert not wrapped and len(sites) == len(want) == env.sizes[k * n + centre]
            rec.update({"reference_rule_numpy_ms_per_centre_each": [round(v, 1) for v in ref_ms],
                        "reference_rule_numpy_ms_per_centre": round(min(ref_ms), 1),
                        "reference_rule_per_centre_over_device_per_centre": round(min(ref_ms) * 1e3 / rec["device_us_per_centre"], 0)})
        record["batches"][f"{C}x{n}"] = rec
        print(f"{C} x {n}", json.dumps(rec), flush=True)
    record["note"] = ("device / host: host clock around whole calls, synchronised, best of the alternated rounds.  *_kernel_ms: device "
                      "events around 20 back-to-back launches on prepared inputs (bonds_count includes the memset of its output).  "
                      "reference_rule_numpy: one centre per cell, as the reference computes it; the ratio compares it with the device's "
                      "time per centre of the same batch, all centres.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(record, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

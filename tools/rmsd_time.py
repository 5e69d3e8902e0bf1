"""Time the structural RMSD evaluation (csrc/eval/kabsch.hip) with device events after a warm-up:

  (a) evaluate_by_rmsd on 256 graphs of 64 atoms (one launch, one download) against the reference-form loop on the SAME device
      tensors: per graph centroids, H, torch.linalg.svd, det, R, residual (kabsch_torch of evaluate_rmsd_for_pos_generate.py:11-51
      as parts/def_for_main.py:73-89 calls it), then the same sort;
  (b) the correspondence search (evaluate_rmsd.py:93-107) on 1, 64 and 1,024 graphs of ten atoms, as orderings per second
      (9! = 362,880 per graph), with the float64 numpy restatement of tests/_rmsd_util.py spread over 16 CPU threads as the
      baseline for one graph.

Bound of (b), written down before measuring.  Per ordering of a ten-atom graph the kernel issues, without pruning, about 260
fp64 vector instructions (no contraction: 36 adds for H from the shared prefix and the table, 17 for |H|^2, ~70 for det H and
tr((H^T H)^2), ~27 per Newton step with its division, ~5 steps) and reads 180 B of LDS (135 ds_read_b64 per lane and six
orderings).  fp64 vector rate of the chip: 78.6 TFLOP/s counted as FMA = 39.3e12 lane-instructions/s -> 1.5e11 orderings/s;
LDS at 150 TB/s -> 8.3e11 orderings/s.  The fp64 VALU is the limit.  An ordering that is pruned at the first upper bound
(sqrt(3) |H|_F below the best score so far) costs ~63 instructions -> 6.2e11 orderings/s is the ceiling with perfect pruning.

  python tools/rmsd_time.py                       # the record -> profiles/rmsd_time.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rmsd_time.py --search-only --rounds 1 --out DIR/t.json
                                                  # kernel times, in a run of its own
  python tools/rmsd_time.py --summarize DIR       # -> the kabsch kernels of that trace per launch geometry, as text
"""
import argparse
import json
import math
import os
import sys
import time
from multiprocessing.pool import ThreadPool
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_LANE_INSTR_PER_S = 78.6e12 / 2
INSTR_FULL, INSTR_PRUNED, LDS_BYTES, LDS_BPS = 260, 63, 180, 150e12


def reference_form_loop(originals, generated):
    """the reference's per-graph loop, on device tensors"""
    import torch
    rows = []
    for o, gl in zip(originals, generated):
        g = gl[-1]
        P, Q = o.pos, g.pos
        if P.shape[0] == 1:
            continue
        cP, cQ = P.mean(0), Q.mean(0)
        p, q = P - cP, Q - cQ
        U, S, Vt = torch.linalg.svd(p.T @ q)
        if torch.det(Vt.T @ U.T) < 0.0:
            Vt = Vt.clone()
            Vt[:, -1] *= -1.0
        R = Vt.T @ U.T
        rows.append((o.id, torch.sqrt(((p @ R.T - q) ** 2).sum() / P.shape[0]), o, g))
    return sorted(rows, key=lambda r: r[1])


def cpu_search_16_threads(gen, orig, threads=16):
    """float64 numpy restatement of the search of one graph, chunks of orderings over a thread pool -> (seconds, min rmsd)"""
    import numpy as np
    from tests import _rmsd_util as RU
    n = gen.shape[0]
    g, q = gen.astype(np.float64) - gen[0], orig.astype(np.float64) - orig[0]
    t0 = time.perf_counter()
    orders = RU.all_orders(n)

    def part(sl):
        p = g[orders[sl]]
        U, S, Vt = np.linalg.svd(np.einsum("mir,ic->mrc", p, q))
        neg = np.linalg.det(np.swapaxes(Vt, 1, 2) @ np.swapaxes(U, 1, 2)) < 0.0
        Vt[neg, -1, :] *= -1.0
        R = np.swapaxes(Vt, 1, 2) @ np.swapaxes(U, 1, 2)
        return np.sqrt(np.sum(np.square(p @ np.swapaxes(R, 1, 2) - q), axis=(1, 2)) / n).min()

    step = -(-orders.shape[0] // (4 * threads))
    with ThreadPool(threads) as pool:
        best = min(pool.map(part, [slice(lo, lo + step) for lo in range(0, orders.shape[0], step)]))
    return time.perf_counter() - t0, float(best)


def summarize(trace_dir):
    import collections
    import csv
    import glob
    import statistics
    by_launch = collections.defaultdict(list)
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "kabsch" in r["Kernel_Name"]:
                name = r["Kernel_Name"].split("(float")[0].split("::")[-1]
                by_launch[name, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Grid_Size_Y"])].append(
                    (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (name, gx, gy), us in sorted(by_launch.items()):
        print(f"{name} grid ({gx}, {gy}): {len(us)} launches, min {min(us):.1f} us, median {statistics.median(us):.1f} us, max {max(us):.1f} us")
    if not by_launch:
        print("no kabsch kernel rows under", trace_dir)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--search-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rmsd_time.json"))
    ap.add_argument("--summarize", metavar="DIR")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)

    import numpy as np
    import torch
    import diffusion_model_amd as dma
    from tests import _rmsd_util as RU
    if not torch.cuda.is_available():
        raise SystemExit("tools/rmsd_time.py measures on the GPU: no device visible")
    dev = "cuda"
    rng = np.random.default_rng(0)

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    record = {"steps_per_window": args.steps, "warmup_steps": args.warmup, "rounds": args.rounds,
              "gcn_arch": torch.cuda.get_device_properties(0).gcnArchName}

    if not args.search_only:
        B, n = 256, 64
        originals, generated = [], []
        for k in range(B):
            o = RU.silica_cloud(rng, n)
            g = o @ RU.random_rotation(rng).T + rng.uniform(-3, 3, 3) + 0.2 * rng.standard_normal((n, 3))
            originals.append(SimpleNamespace(pos=torch.from_numpy(o.astype(np.float32)).to(dev), id=k))
            generated.append([SimpleNamespace(pos=torch.from_numpy(g.astype(np.float32)).to(dev))])
        fused = lambda: dma.stats.evaluate_by_rmsd(originals, generated)
        loop = lambda: reference_form_loop(originals, generated)
        a, b = fused(), loop()
        worst = max(abs(x[1].item() - y[1].item()) for x, y in zip(sorted(a, key=lambda r: r[0]), sorted(b, key=lambda r: r[0])))
        steps_loop = max(1, args.steps // 10)
        timed(fused, args.warmup)
        timed(loop, 1)
        ms = {"fused": [], "loop": []}
        for _ in range(args.rounds):                            # alternating
            ms["fused"].append(timed(fused, args.steps))
            ms["loop"].append(timed(loop, steps_loop))
        record["evaluate_by_rmsd"] = {
            "graphs": B, "atoms_per_graph": n, "max_abs_rmsd_difference": worst,
            "device_ms_per_call_rounds": [round(v, 4) for v in ms["fused"]], "device_ms_per_call": round(min(ms["fused"]), 4),
            "reference_form_loop_ms_per_call_rounds": [round(v, 3) for v in ms["loop"]],
            "reference_form_loop_ms_per_call": round(min(ms["loop"]), 3), "loop_steps_per_window": steps_loop,
            "loop_over_device": round(min(ms["loop"]) / min(ms["fused"]), 1)}
        print("evaluate_by_rmsd", json.dumps(record["evaluate_by_rmsd"]), flush=True)

    n = 10
    per_graph = math.factorial(n - 1)
    search = {"atoms_per_graph": n, "orderings_per_graph": per_graph, "batches": {}}
    first = None
    for B in (1, 64, 1024):
        gens, origs = [], []
        for _ in range(B):
            o = RU.silica_cloud(rng, n)
            sh = np.concatenate([[0], 1 + rng.permutation(n - 1)])
            gens.append((o @ RU.random_rotation(rng).T + rng.uniform(-3, 3, 3) + 0.1 * rng.standard_normal((n, 3)))[sh].astype(np.float32))
            origs.append(o.astype(np.float32))
        if first is None:
            first = (gens[0], origs[0])
        P, Q = torch.from_numpy(np.concatenate(gens)).to(dev), torch.from_numpy(np.concatenate(origs)).to(dev)
        out = (torch.empty(B, device=dev), torch.empty(B * n, dtype=torch.int32, device=dev), torch.empty(B, 3, 3, device=dev))
        fn = lambda: dma.stats.kabsch_min_over_permutations(P, Q, [n] * B, max_atoms=n, out=out)
        timed(fn, args.warmup)
        ms = [timed(fn, args.steps) for _ in range(args.rounds)]
        rate = B * per_graph / (min(ms) * 1e-3)
        search["batches"][str(B)] = {"ms_per_call_rounds": [round(v, 4) for v in ms], "ms_per_call": round(min(ms), 4),
                                     "orderings_per_s": float(f"{rate:.4g}"),
                                     "share_of_fp64_valu_bound": round(rate / (FP64_LANE_INSTR_PER_S / INSTR_FULL), 3)}
        if B == 1:
            search["device_min_rmsd_first_graph"] = float(out[0][0])
        print("search", B, json.dumps(search["batches"][str(B)]), flush=True)
    secs, best = min(cpu_search_16_threads(*first) for _ in range(2))
    search["cpu_float64_16_threads"] = {"seconds_per_graph": round(secs, 3), "orderings_per_s": float(f"{per_graph / secs:.4g}"),
                                        "min_rmsd_first_graph": best}
    search["bounds_orderings_per_s"] = {"fp64_valu_every_ordering_scored": float(f"{FP64_LANE_INSTR_PER_S / INSTR_FULL:.3g}"),
                                        "fp64_valu_every_ordering_pruned_at_first_bound": float(f"{FP64_LANE_INSTR_PER_S / INSTR_PRUNED:.3g}"),
                                        "lds_read": float(f"{LDS_BPS / LDS_BYTES:.3g}")}
    best_rate = max(v["orderings_per_s"] for v in search["batches"].values())
    search["device_over_cpu"] = round(best_rate / search["cpu_float64_16_threads"]["orderings_per_s"], 1)
    record["search"] = search
    print("search baseline", json.dumps(search["cpu_float64_16_threads"]), "device / cpu", search["device_over_cpu"], flush=True)
    record["note"] = ("ms per call: device events around steps_per_window back-to-back calls of the Python entry point (host work of the "
                      "call included: collation, upload, launch, download), best of the rounds; the kernels' own time comes from a "
                      "rocprofv3 kernel trace (see the module docstring)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(record, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

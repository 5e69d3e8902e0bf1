"""Time the atom matching of large graphs (csrc/eval/assign.hip through stats.align_by_assignment) against the reference's
method on the same host, for the two batch shapes of BASELINE configs C2 and C3:

  256 graphs of 64 atoms  (one wavefront per graph)         32 graphs of 512 atoms  (one 256-thread workgroup per graph)

  device flow    stats.align_by_assignment(originals, generated): originals on the host, samples on the device as generate()
                 leaves them; collate, three launches (pre-alignment, assignment, Kabsch), ONE download.  Wall time of the call
                 (host clock; the call ends in the download, which synchronises), warmed up, best and all rounds.
  host loop      what create_xyz.py:116-192 does: download the samples, then per graph the pre-alignment, scipy's
                 linear_sum_assignment on the distance matrix and the final Kabsch fit (the float64 restatement of
                 tests/_assign_util.py), spread over 16 threads.  Same host clock.
  assignment only  stats.linear_assignment on the pre-aligned pairs as device tensors, device events around back-to-back calls:
                 the solver's launch alone.

The two flows are alternated round by round.  Nothing here is an estimate: a run without a GPU fails.

  python tools/assign_time.py                       # -> profiles/assign_time.json
"""
import argparse
import json
import os
import sys
import time
from multiprocessing.pool import ThreadPool
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cloud(rng, n):
    """atom 0 at the origin, the others 1.6 A and more away at the density of a 64-atom cloud of radius 5 A"""
    import numpy as np
    v = rng.standard_normal((n, 3))
    r = rng.uniform(1.6, 5.0 * max(1.0, (n / 64.0) ** (1.0 / 3.0)), n)
    pts = v / np.linalg.norm(v, axis=1, keepdims=True) * r[:, None]
    pts[0] = 0.0
    return pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_time.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import diffusion_model_amd as dma
    from tests import _assign_util as AU
    if not torch.cuda.is_available():
        raise SystemExit("tools/assign_time.py measures on the GPU: no device visible")
    dev = "cuda"
    rng = np.random.default_rng(0)
    record = {"rounds": args.rounds, "warmup_calls": args.warmup, "host_threads": args.threads, "noise": args.noise,
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

    for B, n, calls_dev, calls_host in ((256, 64, 20, 2), (32, 512, 5, 1)):
        originals, generated = [], []
        for k in range(B):
            orig, gen, _ = AU.pair_case(rng, n, args.noise, cloud(rng, n))
            x = torch.eye(2, dtype=torch.long)[torch.arange(n) % 2]
            originals.append(SimpleNamespace(pos=torch.from_numpy(orig), x=x, id=f"mp-{k}"))
            generated.append([SimpleNamespace(pos=torch.from_numpy(gen).to(dev), x=x.to(dev))])
        pool = ThreadPool(args.threads)

        def device_flow():
            return dma.stats.align_by_assignment(originals, generated)

        def host_loop():
            pairs = [(o.pos.numpy(), g[-1].pos.cpu().numpy()) for o, g in zip(originals, generated)]   # the download
            return pool.map(lambda p: AU.align_f64(*p), pairs)

        rows, ref = device_flow(), host_loop()
        same = sum(int(np.array_equal(r[3], f["col_ind"])) for r, f in zip(rows, ref))
        worst = max([abs(r[1] - f["rmsd"]) for r, f in zip(rows, ref) if np.array_equal(r[3], f["col_ind"])], default=None)
        wall(device_flow, args.warmup)
        ms = {"device": [], "host": []}
        for _ in range(args.rounds):                            # alternating
            ms["device"].append(wall(device_flow, calls_dev))
            ms["host"].append(wall(host_loop, calls_host))
        sizes = [n] * B
        P = torch.cat([o.pos - o.pos[0] for o in originals]).to(dev)                       # what the flow's own launch sees
        Q = torch.from_numpy(np.concatenate([f["aligned"] for f in ref]).astype(np.float32)).to(dev)
        out = (torch.empty(B * n, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float64, device=dev))
        solver = lambda: dma.stats.linear_assignment(P, Q, sizes, out=out)
        events(solver, args.warmup)
        ms_solver = [events(solver, calls_dev) for _ in range(args.rounds)]
        pool.close()
        rec = {"graphs": B, "atoms_per_graph": n, "assignments_equal_to_host_loop": f"{same} of {B}",
               "max_abs_rmsd_difference_where_equal": worst,
               "device_flow_ms_per_call_rounds": [round(v, 3) for v in ms["device"]], "device_flow_ms_per_call": round(min(ms["device"]), 3),
               "device_calls_per_window": calls_dev,
               "host_loop_ms_per_call_rounds": [round(v, 2) for v in ms["host"]], "host_loop_ms_per_call": round(min(ms["host"]), 2),
               "host_calls_per_window": calls_host,
               "host_over_device": round(min(ms["host"]) / min(ms["device"]), 2),
               "assignment_only_ms_per_call_rounds": [round(v, 3) for v in ms_solver],
               "assignment_only_ms_per_call": round(min(ms_solver), 3)}
        record["batches"][f"{B}x{n}"] = rec
        print(f"{B} x {n}", json.dumps(rec), flush=True)
    record["note"] = ("device_flow / host_loop: host clock around whole calls that end in a download or a synchronise, best of the "
                      "alternated rounds.  assignment_only: device events around stats.linear_assignment on the centred "
                      "originals and the pre-aligned samples, the launch the flow itself makes.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(record, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

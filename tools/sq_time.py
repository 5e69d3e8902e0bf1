"""Time the structure factors (csrc/eval/sq.hip through stats.debye_sums and cells.structure_factor; A = 2).

Clusters: 256 clouds of 64 atoms, 32 of 512 and 1 of 4096 at 15.6 cubic angstrom per atom, q = 0.05 ... 25 in steps of 0.05
(500 values).  Cell: beta-cristobalite replicated 5 x 5 x 5 (3000 atoms) with every fractional coordinate displaced by
sigma = 0.002 (the cell of tools/rings_time.py) at q_max = 15, dq = 0.05.

  device     the whole call on device tensors (checks, work lists, uploads, launches; for the cell also the count pass, its
             prefix sums and the finishing formulas), host clock, synchronised.  And the launches alone, device events around
             back-to-back calls on prepared inputs: egnn_sq_debye; egnn_sq_cell_rho (fill + rho); egnn_sq_cell_shells.
  torch (a)  the same quantity as batched float64 torch ops on the same device tensors: cdist -> sin -> one-hot matmuls for the
             Debye sums (q in slabs that keep the [B, n, n, q] intermediate below 1 GiB); hkl . frac -> exp -> a complex matmul with
             the one-hot types for rho (vectors in slabs below 1 GiB), given the device's vector list.
  host (b)   the numpy restatement of tests/_sq_util.py on 16 host threads (graphs, or slabs of vectors, spread over the threads),
             for the two smaller cluster shapes and the cell; not for the 4096-atom cloud, whose [pairs, q] intermediates do
             not fit the restatement.
Equal results within the caps of tests/_sq_util.py are asserted.  Best of 5 alternated rounds (the host in the first 2).

The kernels' (pair, q) and (vector, atom) terms per second are stated as a share of the fp64 vector rate of the chip, 39.3e12
lane-instructions/s (tools/rmsd_time.py), with the fp64 instructions per term read from the disassembly of the kernels: about
105 per (pair, q) term (library sin 66 to 83 by path, the quotient sin(x) / x and the window product 36, the sum 1) and 34 per
(vector, atom) term (the phase 6, sincospi 26, the two sums).  Nothing here is an estimate: a run without a GPU fails.

  python tools/sq_time.py                       # -> profiles/sq_time.json
"""
import argparse
import json
import os
import sys
import time
from multiprocessing.pool import ThreadPool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_LANE_RATE = 39.3e12
DEBYE_FP64_PER_TERM, RHO_FP64_PER_TERM = 105, 34
Q_MAX, DQ, REPLICAS = 15.0, 0.05, 5
SLAB_BYTES = 1 << 30


def torch_debye(torch, pos, types, B, n, A, q):
    """competitor (a): equal-sized graphs, everything batched; -> [B, A, A, Q]"""
    p = pos.view(B, n, 3).double()
    d = torch.cdist(p, p)
    T = torch.nn.functional.one_hot(types.view(B, n).long(), A).double()
    off = ~torch.eye(n, dtype=torch.bool, device=pos.device)
    out = torch.empty(B, A, A, q.numel(), dtype=torch.float64, device=pos.device)
    slab = max(1, SLAB_BYTES // (B * n * n * 8))
    for s in range(0, q.numel(), slab):
        x = d[..., None] * q[s:s + slab]
        sinc = torch.where(x == 0, torch.ones_like(x), torch.sin(x) / x) * off[None, :, :, None]
        out[..., s:s + slab] = torch.einsum("bia,bijq,bjc->bacq", T, sinc, T)
    return out


def torch_rho(torch, hkl, frac, types, A):
    """competitor (a) for the cell: -> complex128 [K, A]"""
    w = frac - torch.floor(frac)
    T = torch.nn.functional.one_hot(types.long(), A).to(torch.complex128)
    out = torch.empty(hkl.shape[0], A, dtype=torch.complex128, device=hkl.device)
    slab = max(1, SLAB_BYTES // (frac.shape[0] * 16))
    for s in range(0, hkl.shape[0], slab):
        t = hkl[s:s + slab].double() @ w.T
        t = t - torch.floor(t)
        out[s:s + slab] = torch.polar(torch.ones_like(t), -2.0 * torch.pi * t) @ T
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sq_time.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import diffusion_model_amd as dma
    from diffusion_model_amd import cells, stats
    from tests import _cells_util as CU
    from tests import _sq_util as SU
    if not torch.cuda.is_available():
        raise SystemExit("tools/sq_time.py measures on the GPU: no device visible")
    dev, A = "cuda", 2
    q_h = 0.05 * np.arange(1, 501)
    q = torch.from_numpy(q_h).to(dev)
    record = {"rounds": args.rounds, "host_rounds": args.host_rounds, "warmup_calls": args.warmup, "host_threads": args.threads, "types": A,
              "q": "0.05 ... 25.0 step 0.05 (500 values)", "fp64_lane_instructions_per_second": FP64_LANE_RATE,
              "gcn_arch": torch.cuda.get_device_properties(0).gcnArchName, "clusters": {}}

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

    pool = ThreadPool(args.threads)
    for B, n, calls, with_host in ((256, 64, 10, True), (32, 512, 5, True), (1, 4096, 3, False)):
        sizes = [n] * B
        parts = [SU.cloud(n, 7000 + 13 * g + n) for g in range(B)]
        pos_h, types_h = np.concatenate([p for p, _ in parts]), np.concatenate([t for _, t in parts])
        pos, types = torch.from_numpy(pos_h).to(dev), torch.from_numpy(types_h).to(dev)
        onehot = torch.eye(A, dtype=torch.int64, device=dev)[types.long()]

        def device_flow():
            return stats.debye_sums(pos, onehot, sizes, q_h)

        def torch_flow():
            return torch_debye(torch, pos, types, B, n, A, q)

        def host_loop():
            return np.concatenate(pool.map(lambda g: SU.debye_restated(pos_h[g * n:(g + 1) * n], types_h[g * n:(g + 1) * n], [n], A, q_h), range(B)))

        D, ref = device_flow().cpu().numpy(), torch_flow().cpu().numpy()
        nt = SU.n_types(types_h, sizes, A)
        err_torch = SU.debye_error(D, ref, nt)
        assert err_torch <= SU.CAP_DEBYE, err_torch
        err_host = None
        if with_host:
            err_host = SU.debye_error(D, host_loop(), nt)
            assert err_host <= SU.CAP_DEBYE, err_host
        wall(device_flow, args.warmup)
        wall(torch_flow, 1)
        ms = {"device": [], "torch": [], "host": []}
        for r in range(args.rounds):                            # alternating
            ms["device"].append(wall(device_flow, calls))
            ms["torch"].append(wall(torch_flow, 1))
            if with_host and r < args.host_rounds:
                ms["host"].append(wall(host_loop, 1))
        plan = stats._DebyePlan(stats._StructInput(pos, onehot, sizes, "sq_time"), q_h, None, None, "sq_time")
        events(plan.run, args.warmup)
        ms_k = [events(plan.run, calls) for _ in range(args.rounds)]
        terms = B * n * (n - 1) // 2 * len(q_h)
        rate = terms / (min(ms_k) * 1e-3)
        rec = {"graphs": B, "atoms_per_graph": n, "unordered_pair_q_terms": terms, "tiles": plan.n_tiles,
               "max_error_vs_torch_over_sqrt_NaNb": err_torch, "max_error_vs_host_over_sqrt_NaNb": err_host,
               "device_ms_per_call_rounds": [round(v, 3) for v in ms["device"]], "device_ms_per_call": round(min(ms["device"]), 3),
               "torch_ms_per_call_rounds": [round(v, 3) for v in ms["torch"]], "torch_ms_per_call": round(min(ms["torch"]), 3),
               "torch_over_device": round(min(ms["torch"]) / min(ms["device"]), 2),
               "launches_ms_rounds": [round(v, 4) for v in ms_k], "launches_ms": round(min(ms_k), 4),
               "terms_per_second": round(rate, 0), "fp64_instructions_per_term": DEBYE_FP64_PER_TERM,
               "share_of_fp64_vector_rate": round(rate * DEBYE_FP64_PER_TERM / FP64_LANE_RATE, 4)}
        if with_host:
            rec.update({"host_ms_per_call_rounds": [round(v, 1) for v in ms["host"]], "host_ms_per_call": round(min(ms["host"]), 1),
                        "host_over_device": round(min(ms["host"]) / min(ms["device"]), 1)})
        record["clusters"][f"{B}x{n}"] = rec
        print(f"{B} x {n}", json.dumps(rec), flush=True)

    # ---- the cell ----
    frac, types_c = CU._cristobalite_frac()
    off = np.array([[i, j, k] for i in range(REPLICAS) for j in range(REPLICAS) for k in range(REPLICAS)], dtype=np.float64)
    big = ((frac[None, :, :] + off[:, None, :]) / REPLICAS).reshape(-1, 3) + 0.002 * np.random.default_rng(3).standard_normal((len(off) * len(frac), 3))
    types_big = np.tile(types_c, len(off)).astype(np.int32)
    cell = dma.PeriodicCell(7.16 * REPLICAS * np.eye(3), big, types=types_big, num_types=2, id="cristobalite-5x5x5")

    def cell_flow():
        return cells.structure_factor(cell, q_max=Q_MAX, dq=DQ, vectors=True, device=dev)

    sf = cell_flow()
    K, N = int(sf.hkl.shape[0]), cell.num_atoms
    frac_d, types_d = torch.from_numpy(big).to(dev), torch.from_numpy(types_big).to(dev)
    hkl_h = sf.hkl.cpu().numpy()

    def torch_flow():
        return torch_rho(torch, sf.hkl, frac_d, types_d, A)

    def host_loop():
        step = -(-K // (4 * args.threads))
        return np.concatenate(pool.map(lambda s: SU.rho_restated(big, types_big, A, hkl_h[s:s + step]), range(0, K, step)))

    nt = np.bincount(types_big, minlength=A)
    rho = sf.rho.cpu().numpy()
    err_torch, err_host = SU.rho_error(rho, torch_flow().cpu().numpy(), nt), SU.rho_error(rho, host_loop(), nt)
    assert err_torch <= SU.CAP_RHO and err_host <= SU.CAP_RHO, (err_torch, err_host)
    wall(cell_flow, args.warmup)
    wall(torch_flow, 1)
    ms = {"device": [], "torch": [], "host": []}
    for r in range(args.rounds):
        ms["device"].append(wall(cell_flow, 3))
        ms["torch"].append(wall(torch_flow, 1))
        if r < args.host_rounds:
            ms["host"].append(wall(host_loop, 1))
    run = cells._SqCellRun(cells._CellBatch([cell], dev), Q_MAX, DQ, int(np.ceil(Q_MAX / DQ)))
    events(run.rho, args.warmup)
    ms_rho = [events(run.rho, 3) for _ in range(args.rounds)]
    events(run.shells, args.warmup)
    ms_shell = [events(run.shells, 3) for _ in range(args.rounds)]
    terms = K * N
    rate = terms / (min(ms_rho) * 1e-3)
    record["cell"] = {"atoms": N, "q_max": Q_MAX, "dq": DQ, "half_space_vectors": K, "vector_atom_terms": terms, "shell_bins": run.nbins,
                      "max_rho_error_vs_torch_over_sqrt_Na": err_torch, "max_rho_error_vs_host_over_sqrt_Na": err_host,
                      "device_ms_per_call_rounds": [round(v, 3) for v in ms["device"]], "device_ms_per_call": round(min(ms["device"]), 3),
                      "torch_rho_ms_rounds": [round(v, 3) for v in ms["torch"]], "torch_rho_ms": round(min(ms["torch"]), 3),
                      "host_rho_ms_rounds": [round(v, 1) for v in ms["host"]], "host_rho_ms": round(min(ms["host"]), 1),
                      "rho_launches_ms_rounds": [round(v, 4) for v in ms_rho], "rho_launches_ms": round(min(ms_rho), 4),
                      "shell_launch_ms_rounds": [round(v, 4) for v in ms_shell], "shell_launch_ms": round(min(ms_shell), 4),
                      "torch_rho_over_rho_launches": round(min(ms["torch"]) / min(ms_rho), 2),
                      "host_rho_over_rho_launches": round(min(ms["host"]) / min(ms_rho), 1),
                      "terms_per_second": round(rate, 0), "fp64_instructions_per_term": RHO_FP64_PER_TERM,
                      "share_of_fp64_vector_rate": round(rate * RHO_FP64_PER_TERM / FP64_LANE_RATE, 4)}
    print("cell", json.dumps(record["cell"]), flush=True)
    pool.close()
    record["note"] = ("device / torch / host: host clock around whole calls, synchronised, best of the alternated rounds (the host in the "
                      "first host_rounds only).  *launches_ms: device events around back-to-back launches on prepared inputs.  The cell's "
                      "torch and host figures are rho alone, given the device's vector list, and are compared with the rho launches; the "
                      "device call also counts and lists the vectors, takes the shell means and finishes the partials.  Not measured: the "
                      "numpy restatement on the 4096-atom cloud; hardware counters (the shares are launch time against instruction "
                      "counts read from the disassembly).")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(record, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

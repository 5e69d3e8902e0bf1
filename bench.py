#!/usr/bin/env python3
"""Headline benchmark: atoms x denoise-steps / second on 64-atom SiO2 cells (BASELINE.json configs[1]:
4-layer EGNN, widths 1024/1024/1024, m=256, H=36, T=1000 schedule, batch 256 graphs, bf16 MFMA).

A "step" is one reverse-diffusion step of the device-resident sampler over the whole batch: the
L-layer EGNN forward eps_theta(x_t, h_t, t) plus the fused eps -> mu -> noise -> state update kernel
(parts/train_per_iretation.py:335-373).  Inputs (state, conditioning, weights, schedule table) are
resident in HBM before the timed region.  With --gpus N every rank samples its own batch of graphs
(independent replicas: no data-path collective, weak scaling); only the timing uses a collective.  With
--full the same JSON line carries a `ddp_train` sub-record (BASELINE configs[3] per-rank shape: forward + backward +
per-layer RCCL gradient all-reduce + Adam), which is where the data-path collective of the N > 1 curve is.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A plain run sets up, warms up with W steps, times exactly K steps once and prints the headline line.  `--full` adds
everything else the benchmark measures: the median of `--reps` (default 5) repetitions, the hipGraph replay time,
the `ddp_train`, `slab_4096`, `tolerance_grade`, `fp16`, `c3`, `ddp_train_tolerance_grade`, `latency` and
`cpu_baseline` sub-records.  `--dump-outputs DIR` writes what the timed path computed in its last step (the
sampler state, or the loss and parameters with --mode train) as DIR/<name>.npy; the inputs are seeded, so two
builds run with the same arguments can be compared output for output.

`--gpus N` from a plain shell starts the N ranks itself (a torch.distributed.run child process, before
anything has touched the GPU); under torch.distributed.run it reads RANK / LOCAL_RANK / WORLD_SIZE.
Prints ONE JSON line on rank 0.  A state that went non-finite makes the line `"valid": false` with no value
and the exit code 3.
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, M, W, A, T = 36, 256, 1024, 2, 1000
# longest reverse chain from x_T the sampler legs run: the untrained weights overflow the state to inf / NaN after about 100
# steps (the fp32 oracle at the headline shape), and a non-finite state runs faster and invalidates the line
CHAIN_STEPS = 50
DUMP_LIMIT_BYTES = 60 * 10 ** 6      # under 64 MB with the .npy headers


def write_outputs(out_dir, arrays):
    """`--dump-outputs`: every array as out_dir/<name>.npy, float64 kept, everything else as float32.  If all of them together
    exceed DUMP_LIMIT_BYTES, an array over its even share of the limit is replaced by a fixed sample of its flattened
    elements (seed 0, sorted indices, the same for every run of the same shape)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrs = {}
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        arrs[name] = np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)
    if sum(a.nbytes for a in arrs.values()) > DUMP_LIMIT_BYTES:
        share = DUMP_LIMIT_BYTES // len(arrs)
        for name, a in arrs.items():
            if a.nbytes > share:
                idx = np.sort(np.random.default_rng(0).choice(a.size, share // a.itemsize, replace=False))
                arrs[name] = a.reshape(-1)[idx]
    for name, a in arrs.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


# algorithmic work of the fused edge kernel: per edge per layer
#   mlp_m 336,896 + gate 256 + mlp_x 1,124,352 = 1,461,504 MAC  (H=36, W=1024, M=256)
def edge_macs(H, M, Wm, Wx):
    inp = 2 * H + 1
    return (inp * Wm + Wm * M) + M + (inp * Wx + Wx * Wx + Wx)


def node_macs(H, M, Wh):
    return (H + M) * Wh + Wh * H


PEAK_TFLOPS = {"bf16": 2500.0, "fp16": 2500.0, "bf16x3": 2500.0, "f16c8": 2500.0, "fp32": 157.3}   # dense MFMA peaks, MI355X_MICROARCH.md (bf16x3 = three bf16
# MFMAs per algorithmic product: its `achieved` counts the ALGORITHMIC flops once, so at best 1/3 of the bf16 peak)


def synthetic_cond(batch, n_atoms, ncond, seed):
    """conditioning columns [compressed spectrum (N(0,1)) | exO one-hot on atom 0]"""
    g = torch.Generator().manual_seed(seed)
    cond = torch.randn(batch * n_atoms, ncond, generator=g)
    cond[:, -1] = 0.0
    cond[::n_atoms, -1] = 1.0
    return cond


def sio2_cells(batch, n_atoms, seed):
    """jittered cubic grid, spacing 1.6 A, jitter N(0, 0.1^2); atom 0 = O, then Si : O = 21 : 42 per 64"""
    g = torch.Generator().manual_seed(seed)
    side = round(n_atoms ** (1 / 3))
    grid = torch.stack(torch.meshgrid(*[torch.arange(side, dtype=torch.float32)] * 3, indexing="ij"), -1).reshape(-1, 3) * 1.6
    pos = grid[:n_atoms].repeat(batch, 1) + 0.1 * torch.randn(batch * n_atoms, 3, generator=g)
    types = torch.zeros(n_atoms, A)
    n_si = max(1, round(n_atoms * 21 / 64))
    types[0, 0] = 1
    types[1:1 + n_si, 1] = 1
    types[1 + n_si:, 0] = 1
    return pos, types.repeat(batch, 1)


def build_net(dma, L, n_atoms, finite_init=True):
    """Random-init weights of the named architecture (seed 2024, default nn.Linear init).  The untrained coordinate
    head (mlp_x.4, a [1, 1024] vector without any range clamp) makes the reverse chain overflow within a
    few steps; it is scaled by 1e-3 so the benchmark runs on finite, realistic magnitudes.  Graphs larger than the
    64-atom reference cell sum proportionally more messages per node; the message head is scaled by 64/atoms for
    them, again only to keep untrained weights in a finite regime.  The arithmetic per step is unchanged."""
    torch.manual_seed(2024)
    net = dma.EquivariantGNN(L, 2 * H + 1, W, M, 2 * H + 1, W, 1, H + M, W, H)
    if finite_init:
        with torch.no_grad():
            for layer in net.egcl_list:
                layer.mlp_x[4].weight.mul_(1e-3)
                layer.mlp_x[4].bias.mul_(1e-3)
                if n_atoms > 64:
                    layer.mlp_m[2].weight.mul_(64.0 / n_atoms)
                    layer.mlp_m[2].bias.mul_(64.0 / n_atoms)
    return net


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.lower().startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(sd, n_atoms, target_seconds=18.0):
    """The oracle (torch CPU fp32 restatement of the reference) on a bounded sample of the same workload: reverse steps
    from t = T on B graphs of 64 atoms for B in {1, 4, 16} (the reference itself samples ONE graph per
    call; larger batches fill the host's cores better), about `target_seconds` of CPU work in all; the best B is the
    reported baseline and every B is listed."""
    from oracle.diffusion_ref import DiffusionRef, remove_mean
    from oracle.egnn_ref import egnn_forward, fully_connected_edge_index
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    # a 1-GPU box's CPU share is 16 cores; more torch threads than that only oversubscribes the host
    cores = int(os.environ.get("BENCH_CPU_THREADS", min(avail, 16)))
    torch.set_num_threads(cores)
    ref = DiffusionRef(1e-5, 2.0, T)
    rows = []
    for B in (1, 4, 16):
        g = torch.Generator().manual_seed(0)
        sizes = [n_atoms] * B
        ei = fully_connected_edge_index(sizes)
        ptr = torch.arange(B + 1) * n_atoms
        bidx = torch.arange(B).repeat_interleave(n_atoms)
        pos = remove_mean(torch.randn(B * n_atoms, 3, generator=g), bidx)
        h = torch.cat((torch.randn(B * n_atoms, A, generator=g), synthetic_cond(B, n_atoms, H - A - 1, 1),
                       torch.ones(B * n_atoms, 1)), dim=1)
        steps, el = 0, 0.0
        with torch.no_grad():
            t = T
            for it in range(41):
                if it == 1:
                    t0 = time.perf_counter()          # the first step warms caches / thread pool and is not timed
                new_h, new_x = egnn_forward(sd, ei, h, pos, "graph", ptr)
                eps_x = remove_mean((new_x - pos).clone(), bidx)
                npos = remove_mean(torch.randn(pos.shape, generator=g), bidx)
                pos = ref.calculate_mu(pos, eps_x, t) + ref.step_std(t) * npos
                x = ref.calculate_mu(h[:, :A], new_h[:, :A], t) + ref.step_std(t) * torch.randn(B * n_atoms, A, generator=g)
                h = torch.cat((x, h[:, A:-1], torch.full((B * n_atoms, 1), (t - 1) / T)), dim=1)
                t -= 1
                if it >= 1:
                    steps += 1
                    el = time.perf_counter() - t0
                    if el >= target_seconds / 3:
                        break
        rows.append({"graphs": B, "steps": steps, "seconds": el, "atoms_steps_per_s": B * n_atoms * steps / el})
    best = max(rows, key=lambda r: r["atoms_steps_per_s"])
    return {"value": best["atoms_steps_per_s"], "unit": "atoms*denoise-steps/s", "cores": cores, "kind": "port",
            "cpu_model": _cpu_model(), "host_cores_visible": avail,
            "sample": f"best of B in {{1, 4, 16}} graphs x {n_atoms} atoms (B = {best['graphs']}: {best['steps']} reverse steps from "
                      f"t=T in {best['seconds']:.1f} s), fp32 torch-CPU oracle, {cores} threads",
            "per_batch": rows}


class Ranks:
    """process-group plumbing shared by the legs"""

    def __init__(self, args):
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        # BENCH_DEVICE / BENCH_BACKEND exist only to rehearse the N>1 code path on a one-GPU box
        # (all ranks on one device, gloo for the collectives); the driver's runs use one GPU per rank + RCCL.
        dev_index = int(os.environ.get("BENCH_DEVICE", local_rank))
        self.backend = os.environ.get("BENCH_BACKEND", "nccl")
        torch.cuda.set_device(dev_index)
        self.dev = torch.device("cuda", dev_index)
        if self.world > 1:
            import torch.distributed as dist
            if self.backend == "nccl":
                dist.init_process_group("nccl", device_id=self.dev)
            else:
                dist.init_process_group(self.backend)

    def barrier(self):
        torch.cuda.synchronize(self.dev)
        if self.world > 1:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize(self.dev)

    def max_over_ranks(self, seconds):
        if self.world == 1:
            return seconds
        import torch.distributed as dist
        tt = torch.tensor([seconds], device=self.dev if self.backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return float(tt.item())

    def timed(self, fn):
        """barrier + synchronize on both sides; MAX over ranks"""
        self.barrier()
        t0 = time.perf_counter()
        fn()
        self.barrier()
        return self.max_over_ranks(time.perf_counter() - t0)

    def close(self):
        if self.world > 1:
            import torch.distributed as dist
            dist.barrier()
            dist.destroy_process_group()


def train_leg(args, rk, steps, warmup, batch, dump_dir=None):
    """BASELINE configs[3] per-rank shape: 64-atom SiO2 training, `batch` graphs per rank (256 -> global 2048 on 8 GPUs);
    one step = diffuse_as_batch + EGNN forward + backward (HIP) + per-layer gradient all-reduce (RCCL, issued from inside
    the backward) + Adam.  Timed twice on N > 1: with the all-reduce and without it (what the same rank does alone)."""
    from types import SimpleNamespace
    import diffusion_model_amd as dma
    L, n = args.layers, args.atoms
    dev, world, rank = rk.dev, rk.world, rk.rank
    net = build_net(dma, L, n, finite_init=False).to(dev)
    net.precision, net.norm_scope = args.precision, "graph"
    proc = dma.E3DiffusionProcess(1e-5, 2.0, T)
    plan = dma.fully_connected_plan([n] * batch, dev)
    pos, types = sio2_cells(batch, n, seed=1 + rank)
    cond = synthetic_cond(batch, n, H - A - 1, 1 + rank).to(dev)
    data = SimpleNamespace(pos=pos.to(dev), x=types.to(dev), batch=plan.batch, edge_index=dma.plan_edge_index(plan))
    opt = torch.optim.Adam(net.parameters(), lr=1e-5)
    reducer = dma.GradAllReducer(list(net.egcl_list)) if world > 1 else None
    losses = []

    def step(reduce_grads):
        opt.zero_grad(set_to_none=True)
        noised = dma.diffuse_as_batch(data.pos, data.x, data.batch, proc, num_graphs=batch)
        if reducer is not None and reduce_grads:
            with reducer.armed():   # buckets are all-reduced from inside the backward, layer by layer
                loss, _, _ = dma.training_loss(net, data.edge_index, data.batch, noised, cond, A,
                                               num_graph_global=batch * world, num_graphs=batch)
                loss.backward()
        else:
            loss, _, _ = dma.training_loss(net, data.edge_index, data.batch, noised, cond, A, num_graph_global=batch * world,
                                           num_graphs=batch)
            loss.backward()
        opt.step()
        losses.append(loss.detach())

    def run(k, reduce_grads):
        for _ in range(k):
            step(reduce_grads)

    run(warmup, True)
    el = rk.timed(lambda: run(steps, True))
    out = {"metric": "atoms*(fwd+bwd) steps/sec, 64-atom SiO2 training", "unit": "atoms*train-steps/s",
           "value": world * batch * n * steps / el, "ms_per_step": el * 1e3 / steps, "steps": steps, "warmup": warmup,
           "graphs_per_rank": batch, "global_batch": batch * world, "rccl_ranks": world if rk.backend == "nccl" else 0,
           "collective_backend": rk.backend if world > 1 else None,
           "allreduce_bytes_per_step": sum(p.numel() for p in net.parameters()) * 4 if world > 1 else 0,
           "step": "diffuse_as_batch + HIP forward + HIP backward + per-layer gradient all-reduce + Adam"}
    # roofline of the whole step: forward + backward = 3 x the forward's algorithmic FLOP (2 x 1,461,504 MAC per
    # edge and layer + the node MLP) over the step time, against the dense bf16 MFMA peak
    E = batch * n * (n - 1)
    fwd_flop = L * (2.0 * edge_macs(H, M, W, W) * E + 2.0 * node_macs(H, M, W) * batch * n)
    # HBM bytes per step from separate rocprofv3 --pmc passes of this leg (profiles/traffic_train.json), as for the sampler
    train_traffic, train_traffic_src = None, None
    try:
        tj = json.load(open(os.path.join(ROOT, "profiles", "traffic_train.json")))
        if args.precision == "bf16" and batch == 256 and n == 64 and L == 4:
            from diffusion_model_amd import _lib as _l
            # (valid for the kernels AND the launch sequence it was measured on: fingerprint of csrc/, the flags, autograd.py, gemm.py)
            if tj.get("training_sources_sha256") == _l.training_sources_sha256():
                train_traffic = tj["bytes_per_step"]
                train_traffic_src = (f"profiles/traffic_train.json (rocprofv3 --pmc, separate passes of `bench.py --mode train` at git head "
                                     f"{tj.get('git_head', '?')}, source fingerprint {tj['training_sources_sha256'][:16]} == this tree's: "
                                     f"sum over the step's dispatches of FETCH_SIZE x 2 + WRITE_SIZE)")
            else:
                train_traffic_src = ("profiles/traffic_train.json was measured on other sources (fingerprint " +
                                     str(tj.get("training_sources_sha256"))[:12] + " vs " + _l.training_sources_sha256()[:12] +
                                     "): re-run tools/profile_train_pmc.sh")
    except Exception:
        pass
    out["roofline"] = {"bound": "mfma", "achieved": 3 * fwd_flop / (el / steps) / 1e12, "peak": PEAK_TFLOPS["bf16"],
                       "unit": "TFLOP/s", "frac": 3 * fwd_flop / (el / steps) / 1e12 / PEAK_TFLOPS["bf16"],
                       "algorithmic_flop_per_step": 3 * fwd_flop, "traffic": train_traffic, "traffic_source": train_traffic_src,
                       "backward_path": getattr(getattr(net, "_ctx", None), "last_backward_path", None)}
    # the world = 1 step of THIS visit: an N = 1 run leaves a small record on the node (host, time, source fingerprint); an N > 1 run
    # that finds a fresh one from the same host and the same sources takes value(1) from it
    n1_path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "egnn_bench_ddp_train_n1.json")
    from diffusion_model_amd import _lib as _l2
    if world == 1 and rank == 0 and batch == 256 and n == 64:
        try:
            json.dump({"value": out["value"], "ms_per_step": out["ms_per_step"], "host": socket.gethostname(), "time": time.time(),
                       "precision": args.precision, "training_sources_sha256": _l2.training_sources_sha256()}, open(n1_path, "w"))
        except OSError:
            pass
    if world > 1:
        el1 = rk.timed(lambda: run(steps, False))
        out["ms_per_step_without_allreduce"] = el1 * 1e3 / steps
        # cost of the collective alone: the same ranks, all running at once, with the reducer disabled (it cannot see any other
        # multi-rank loss, and with ranks sharing a device it is not an efficiency at all)
        out["efficiency_vs_no_collective"] = el1 / el
        import torch.distributed as dist
        devs = [None] * world
        dist.all_gather_object(devs, (socket.gethostname(), int(dev.index)))
        share = len(set(devs)) < world
        out["ranks_share_device"] = share
        # data-parallel efficiency = value(N) / (N x value(1)), value(1) from a GENUINE world = 1 run of this visit (same host, same
        # sources, less than two hours old: `bench.py` / `bench.py --mode train` at N = 1 leaves it); never printed when ranks share
        # a device (the one-GPU rehearsal), where N steps time-share one GPU
        out["ddp_efficiency"], out["ddp_efficiency_basis"] = None, None
        try:
            r1 = json.load(open(n1_path))
            fresh = (r1.get("host") == socket.gethostname() and time.time() - r1.get("time", 0) < 7200 and
                     r1.get("training_sources_sha256") == _l2.training_sources_sha256() and r1.get("precision") == args.precision)
        except (OSError, ValueError):
            r1, fresh = None, False
        if share:
            out["ddp_efficiency_basis"] = "not reported: ranks share a device (functional rehearsal)"
        elif fresh:
            out["ddp_efficiency"] = out["value"] / (world * r1["value"])
            out["single_gpu_value"] = r1["value"]
            out["ddp_efficiency_basis"] = (f"value(N) / (N x value(1)); value(1) = {r1['ms_per_step']:.2f} ms per step from the world = 1 run "
                                           f"of this visit on this host ({n1_path})")
        else:
            out["ddp_efficiency_basis"] = ("not reported: no world = 1 record of this visit (run `python bench.py --mode train` at N = 1 "
                                           "first); see efficiency_vs_no_collective")
        try:
            ref1 = json.load(open(os.path.join(ROOT, "profiles", "ddp_train_n1.json")))
            out["single_gpu_value_other_box"] = ref1["value"]
            out["single_gpu_source"] = f"profiles/ddp_train_n1.json (git head {ref1.get('git_head', '?')})"
            out["ddp_efficiency_cross_box"] = None if share else out["value"] / (world * ref1["value"])
        except Exception:
            out["ddp_efficiency_cross_box"] = None
    final = torch.stack(losses[-steps:]).float()
    out["final_loss"] = float(final[-1])
    out["finite"] = bool(torch.isfinite(final).all())
    if dump_dir and rank == 0:    # what the last timed step left: the losses of the timed steps and the updated parameters
        write_outputs(dump_dir, {"loss": final, **{f"param.{k}": p for k, p in net.named_parameters()}})
    return out


def golden_error_from_log(precision):
    """max-relative error of `precision` on the ten reference goldens, read from the newest committed log of tools/prec_errors.py
    whose header carries THIS tree's fingerprint of the forward kernels' sources (`forward_sources_sha256`): numbers measured on
    other kernels are not quoted (the test-suite asserts the same quantity on every run; the bench only quotes the measurement).
    -> (error, file) or None."""
    import glob
    from diffusion_model_amd import _lib
    want = _lib.forward_sources_sha256()
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_prec_errors*.log"))):
        ok = False
        for line in open(f):
            w = line.split()
            if len(w) >= 2 and w[0] == "#" and "forward_sources_sha256" in line:
                ok = line.strip().split("forward_sources_sha256=")[-1].split()[0] == want
            if ok and len(w) == 3 and w[0] == "golden_max_rel" and w[1] == precision:
                best = (float(w[2]), os.path.relpath(f, ROOT))     # the newest matching log wins (sorted by round tag)
    return best


def run_chains(smp, rk, warmup, steps):
    """init + `warmup` untimed steps, then `steps` timed ones (each timed piece bracketed by rk.timed).  A chain that has
    run CHAIN_STEPS steps from x_T starts again from the same seeded x_T (same noise), outside the timed pieces; with
    warmup + steps <= CHAIN_STEPS this is one chain and one timed piece.  -> (seconds, worst non-finite graph count,
    (pos, h, flags) after the last step)"""
    chain, bad_max, el = 0, 0, 0.0
    smp.init()
    for n_left, timed in ((warmup, False), (steps, True)):
        while n_left > 0:
            if chain == CHAIN_STEPS:
                bad_max = max(bad_max, int(smp.state()[2].sum()))
                smp.init()
                chain = 0
            n = min(n_left, CHAIN_STEPS - chain)
            if timed:
                el += rk.timed(lambda: smp.run(nsteps=n, use_graph=False, sync=True))
            else:
                smp.run(nsteps=n, use_graph=False)
            chain += n
            n_left -= n
    pos, h, flags = smp.state()
    return el, max(bad_max, int(flags.sum())), (pos, h, flags)


def sample_leg(args, rk, precision=None, batch=None, atoms=None, steps=None, warmup=None, reps=None, dump_dir=None):
    """the sampler leg at the headline shape (defaults from the command line) or at a sub-record's shape / precision;
    the hipGraph replay extra only with --full"""
    import ctypes as C
    import diffusion_model_amd as dma
    from diffusion_model_amd import _lib
    precision = precision or args.precision
    L, B, n = args.layers, batch or args.batch, atoms or args.atoms
    K, Wm = steps or args.steps, args.warmup if warmup is None else warmup
    dev, world, rank = rk.dev, rk.world, rk.rank
    net = build_net(dma, L, n)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net.to(dev).eval()
    net.precision = precision
    proc = dma.E3DiffusionProcess(1e-5, 2.0, T)
    cond = synthetic_cond(B, n, H - A - 1, seed=1 + rank)
    smp = dma.DeviceSampler(net, proc, [n] * B, cond, atom_type_size=A, seed=rank, norm_scope="graph", device=dev)
    lib = _lib.lib()
    reps = max(1, reps or args.reps)

    if reps > 1:
        # warm-up before the first of several repetitions (a single repetition is warmed up by its own Wm steps)
        run_chains(smp, rk, Wm, 0)
    # ---- timed region: `reps` repetitions (1 unless --full) of EXACTLY K steps from the same initial state (seeded x_T,
    # h_T after the warm-up steps; restarted from x_T every CHAIN_STEPS steps, run_chains), each bracketed by barrier +
    # synchronize, MAX over ranks; HIP events around every fused edge-kernel launch.  The median repetition is reported.
    _lib.check(lib.egnn_profile_enable(smp.ctx.handle, 1))
    rep_s = []
    bad_total = 0
    for _ in range(reps):
        el, bad, last = run_chains(smp, rk, Wm, K)
        rep_s.append(el)
        bad_total = max(bad_total, bad)
    if dump_dir and rank == 0:
        # the state the last timed step left: positions x_t, atom-type features h_t, per-graph non-finite flags
        write_outputs(dump_dir, dict(zip(("pos", "h", "nonfinite"), last)))
    edge_ms, edge_n, node_ms = C.c_float(0), C.c_int(0), C.c_float(0)
    _lib.check(lib.egnn_profile_read(smp.ctx.handle, C.byref(edge_ms), C.byref(edge_n), C.byref(node_ms)))
    _lib.check(lib.egnn_profile_enable(smp.ctx.handle, 0))
    elapsed = statistics.median(rep_s)
    # ---- extra: the same K steps replayed from the captured hipGraph (no events) ----
    graph_ms = None
    if args.full:
        # (from a fresh chain: 2 replays to capture, then up to K steps within CHAIN_STEPS)
        Kg = min(K, CHAIN_STEPS - 2)
        smp.init()
        smp.run(nsteps=2, use_graph=True)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        smp.run(nsteps=Kg, use_graph=True, sync=True)
        torch.cuda.synchronize(dev)
        graph_ms = (time.perf_counter() - t1) * 1e3 / Kg
        bad_total = max(bad_total, int(smp.state()[2].sum()))

    E = B * n * (n - 1)
    flops_per_launch = 2.0 * edge_macs(H, M, W, W) * E
    achieved = flops_per_launch / (edge_ms.value * 1e-3) / 1e12 if edge_ms.value > 0 else 0.0
    peak = PEAK_TFLOPS[precision]
    # HBM bytes per launch come from separate rocprofv3 --pmc passes (profiles/traffic.json, same workload); they cannot be
    # collected from inside this process.  The record carries a fingerprint of the edge kernels' SOURCES it was measured on
    # (a hash of the .so itself is not stable: hipcc derives symbol ids from the build path, and the driver rebuilds the
    # library in its own checkout); a line whose library was built from other sources prints no traffic.
    traffic, tj, traffic_note = None, {}, None
    try:
        tj = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
        if precision == "bf16" and B == 256 and n == 64 and L == 4:
            if tj.get("edge_kernel_sources_sha256") == _lib.edge_kernel_sources_sha256():
                traffic = tj["bytes_per_launch"]
            else:
                traffic_note = ("profiles/traffic.json was measured on other edge-kernel sources (" +
                                str(tj.get("edge_kernel_sources_sha256"))[:12] + " vs " + _lib.edge_kernel_sources_sha256()[:12] +
                                "): not quoted")
    except Exception:
        traffic = None
    out = {
        "metric": f"atoms*denoise-steps/sec, {n}-atom SiO2 T=1000",
        "value": world * B * n * K / elapsed,
        "unit": "atoms*denoise-steps/s",
        "n_gpus": world, "steps": K, "warmup": Wm,
        "ms_per_step": elapsed * 1e3 / K,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": precision, "data": "synthetic",
        "config": {"workload": f"{n}-atom SiO2 cells x {B} graphs/GPU, {L}-layer EGNN (H=36, W=1024, m=256), "
                               f"T=1000 reverse steps, fully connected (E={E}/GPU)",
                   "global_batch": world * B, "parallelism": f"replicas x{world} (no data-path collective)"},
        "timed_region": {"repetitions": reps, "steps_each": K, "ms_per_step_each": [s * 1e3 / K for s in rep_s],
                         "reported": "median repetition", "chain_restart_every": CHAIN_STEPS},
        "roofline": {"bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s",
                     "frac": achieved / peak, "traffic": traffic,
                     "traffic_source": (f"profiles/traffic.json (rocprofv3 --pmc, separate passes of this command at git head "
                                        f"{tj.get('git_head', '?')}, edge-kernel sources sha256 "
                                        f"{str(tj.get('edge_kernel_sources_sha256'))[:16]} == this library's: "
                                        f"FETCH_SIZE x 2 + WRITE_SIZE)") if traffic else traffic_note,
                     "kernel": {"bf16": "fused edge pass of one EGCL layer: coordinate kernel edge_x_m16_kernel "
                                        "(v_mfma_f32_16x16x32_bf16) + message kernel edge_kernel_bf16_v4<1,true>",
                                "fp16": "fused edge pass of one EGCL layer: coordinate kernel edge_x_m16_kernel<false, f16x8> "
                                        "(v_mfma_f32_16x16x32_f16) + message kernel edge_kernel_bf16_v4<1,true,..,f16x8>",
                                "bf16x3": "fused edge pass of one EGCL layer: edge_x3_kernel<false> + edge_x3_kernel<true> "
                                          "(head/remainder operands, 3 bf16 MFMAs per product)",
                                "f16c8": ("fused edge pass of one EGCL layer: edge_c8_kernel<false> + edge_c8_kernel<true> (fp16 heads on "
                                          "v_mfma_f32_16x16x32_f16 + both remainder products on one v_mfma_scale_f32_16x16x128_f8f6f4 "
                                          "with e4m3 operands and fixed block scales)") if os.environ.get("EGNN_C8_TILE") == "16" else
                                         ("fused edge pass of one EGCL layer: edge_c8w_kernel<false, 2> + edge_c8wk_kernel (fp16 heads on "
                                          "v_mfma_f32_32x32x16_f16 + both remainder products on one v_mfma_scale_f32_32x32x64_f8f6f4 "
                                          "with e4m3 operands and fixed block scales)"),
                                "fp32": "fused edge pass of one EGCL layer: edge_kernel<F32> (v_mfma_f32_32x32x2_f32)"}[precision],
                     "avg_launch_ms": edge_ms.value, "launches": edge_n.value,
                     "algorithmic_flop_per_launch": flops_per_launch,
                     # the first Linear layers are evaluated per node (factorised), so the matrix cores execute
                     # only the second-layer products of the count above
                     "mfma_executed_flop_per_launch": 2.0 * (W * M + W * W) * E},
        "node_kernels_ms_per_layer": node_ms.value * 2,
        "nonfinite_graphs": bad_total,
    }
    if args.full:
        out["graph_replay_ms_per_step"] = graph_ms
    del smp
    return out, sd


def _sub(rec, extra=None):
    """a sampler-leg record reduced to what a sub-record of the headline line needs"""
    keep = ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "dtype", "graph_replay_ms_per_step",
            "node_kernels_ms_per_layer", "nonfinite_graphs")
    o = {k: rec[k] for k in keep}
    o["workload"] = rec["config"]["workload"]
    o["timed_region"] = rec["timed_region"]
    o["roofline"] = {k: rec["roofline"][k] for k in ("bound", "achieved", "peak", "unit", "frac", "kernel", "avg_launch_ms", "launches",
                                                      "algorithmic_flop_per_launch")}
    if extra:
        o.update(extra)
    return o


def precision_legs(args, rk):
    """Sub-records of the default line (N = 1), every one timed in this process by the same harness as the headline:
      tolerance_grade  the FASTEST precision that meets north_star's 1e-4 against the reference goldens (bf16x3: head +
                       remainder operands on the bf16 matrix cores, split-operand node MLP), configs[1] shape, >= 10 timed
                       steps, with the measured golden error quoted from the committed log; plus its configs[2] (C3) time;
      fp16             the bf16 path's kernels on fp16 operands (11 significant bits; golden error from the same log);
      c3               configs[2] (32 x 512 atoms) on the headline precision, 3 timed steps."""
    out = {}
    cands = []
    for prec in ("f16c8", "bf16x3"):
        ge = golden_error_from_log(prec)
        rec, _ = sample_leg(args, rk, precision=prec, steps=10, warmup=3, reps=3)
        cands.append((prec, ge, rec))
    ok = [c for c in cands if c[1] and c[1][0] <= 1e-4] or [c for c in cands if c[0] == "bf16x3"]
    prec, ge, tg = min(ok, key=lambda c: c[2]["ms_per_step"])
    tg3, _ = sample_leg(args, rk, precision=prec, batch=32, atoms=512, steps=3, warmup=1, reps=1)
    out["tolerance_grade"] = _sub(tg, {
        "precision": prec, "tolerance": 1e-4,
        "golden_max_rel_err": ge[0] if ge else None, "golden_err_source": ge[1] if ge else None,
        "meets_tolerance": bool(ge and ge[0] <= 1e-4),
        "why_this_precision": "the fastest precision whose measured error on the ten reference goldens is <= 1e-4: f16c8 = fp16 heads + both "
                              "remainder products on one block-scaled e4m3 MFMA (2 bf16-equivalents per product), bf16x3 = three bf16 "
                              "products; fp32 (exact-f32 MFMA, 1/16 of the bf16 rate) also qualifies and is ~4x slower; fp16 and bf16 do "
                              "not (profiles/r05_rounding_budget.txt)",
        "candidates": {c[0]: {"ms_per_step": c[2]["ms_per_step"], "golden_max_rel_err": c[1][0] if c[1] else None,
                              "edge_pass_ms": c[2]["roofline"]["avg_launch_ms"]} for c in cands},
        "c3": _sub(tg3)})
    f16, _ = sample_leg(args, rk, precision="fp16", steps=10, warmup=3, reps=3)
    ge = golden_error_from_log("fp16")
    out["fp16"] = _sub(f16, {"precision": "fp16", "golden_max_rel_err": ge[0] if ge else None,
                             "golden_err_source": ge[1] if ge else None})
    c3, _ = sample_leg(args, rk, batch=32, atoms=512, steps=3, warmup=1, reps=1)
    ge = golden_error_from_log(args.precision)
    out["c3"] = _sub(c3)
    out["golden_max_rel_err"] = ge[0] if ge else None
    out["golden_err_source"] = ge[1] if ge else None
    return out


def slab_leg(args, rk, steps, warmup, dump_dir=None):
    """BASELINE configs[4]: one 4096-atom slab (16x16x16 jittered grid, spacing 1.6 A), fixed radius graph with ~10
    neighbours per atom (~40 k directed edges; the reference only has fully connected graphs), T = 1000 sampling.
    N = 1: the device-resident sampler on the one graph (hipGraph replay).  N > 1: the graph's receiving nodes are
    partitioned over the ranks (PartitionedSampler: per layer one all-reduce of the d^2 sum and one all-gather of the
    updated rows, strong scaling -- total work fixed); the unpartitioned sampler is timed beside it on rank 0's GPU."""
    import diffusion_model_amd as dma
    dev, world, rank = rk.dev, rk.world, rk.rank
    L, n = args.layers, 4096
    g = torch.Generator().manual_seed(7)
    grid = torch.stack(torch.meshgrid(*[torch.arange(16, dtype=torch.float32)] * 3, indexing="ij"), -1).reshape(-1, 3) * 1.6
    x0 = (grid + 0.1 * torch.randn(n, 3, generator=g)).to(dev)
    d = torch.cdist(x0, x0)
    d.fill_diagonal_(float("inf"))
    radius = float(torch.kthvalue(d.reshape(-1), 10 * n).values) + 1e-6      # the 40,960 closest ordered pairs
    i, j = (d < radius).nonzero(as_tuple=True)
    ei = torch.stack((i, j))
    del d
    net = build_net(dma, L, 64).to(dev).eval()
    net.precision = args.precision
    proc = dma.E3DiffusionProcess(1e-5, 2.0, T)
    cond = synthetic_cond(1, n, H - A - 1, seed=3)
    out = {"metric": "atoms*denoise-steps/sec, 4096-atom slab, radius graph", "unit": "atoms*denoise-steps/s",
           "atoms": n, "directed_edges": int(ei.shape[1]), "radius": radius, "steps": steps, "warmup": warmup,
           "scaling": "strong" if world > 1 else None}

    def time_single(dump_dir=None):
        smp = dma.DeviceSampler(net, proc, [n], cond, atom_type_size=A, seed=0, norm_scope="graph", device=dev, edge_index=ei)
        smp.init()
        smp.run(nsteps=warmup, use_graph=True)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        smp.run(nsteps=steps, use_graph=True, sync=True)
        torch.cuda.synchronize(dev)
        el = time.perf_counter() - t0
        pos_out, h_out, flags = smp.state()
        bad = int(flags.sum())
        if dump_dir:
            write_outputs(dump_dir, {"pos": pos_out, "h": h_out, "nonfinite": flags})
        del smp
        return el, bad

    if world == 1:
        el, bad = time_single(dump_dir)
        out.update({"value": n * steps / el, "ms_per_step": el * 1e3 / steps, "nonfinite_graphs": bad,
                    "implementation": "DeviceSampler on one GPU, hipGraph replay"})
        return out
    smp = dma.PartitionedSampler(net, proc, [n], cond, ei, rank, world, atom_type_size=A, seed=0, norm_scope="graph", device=dev)
    smp.init()
    smp.run(nsteps=warmup)
    el = rk.timed(lambda: smp.run(nsteps=steps))
    nonfinite = int(smp.bad.sum())
    local_edges = smp.plan.E
    del smp
    single_ms = None
    if rank == 0:     # the unpartitioned sampler on the same graph, after the collective part
        el1, _ = time_single()
        single_ms = el1 * 1e3 / steps
    rk.barrier()
    out.update({"value": n * steps / el, "ms_per_step": el * 1e3 / steps, "nonfinite_graphs": nonfinite,
                "implementation": f"PartitionedSampler, receiving nodes over {world} ranks, 2 collectives per layer "
                                  f"({rk.backend})", "local_edges_rank0": local_edges,
                "single_gpu_ms_per_step": single_ms,
                "note": "at 40 k edges one GPU runs a step in about the time of the 2 x L latency-bound collectives a "
                        "partitioned step adds; the partition pays for graphs two orders of magnitude larger"})
    return out


def latency_leg(args, rk, steps=64, warmup=16):
    """Small-batch latency (the reference's actual use: generate() samples ONE 20-64-atom graph per call, T + 1 forwards,
    parts/train_per_iretation.py:288-364; its only timing trace is ~6.9 ms per reverse step on an unnamed NVIDIA GPU,
    model_flex.ipynb:218 -- context, not a same-node number).  ms per reverse step of the device-resident sampler,
    eager launches vs hipGraph replay (8 steps per graph)."""
    import diffusion_model_amd as dma
    dev = rk.dev
    rows = []
    proc = dma.E3DiffusionProcess(1e-5, 2.0, T)

    def run(name, net, sizes, ncond, launches):
        cond = torch.randn(sum(sizes), ncond, generator=torch.Generator().manual_seed(1)) if ncond else None
        smp = dma.DeviceSampler(net, proc, sizes, cond, atom_type_size=A, seed=0, norm_scope="graph", device=dev)
        row = {"workload": name, "graphs": len(sizes), "atoms": sum(sizes), "launches_per_step": launches}
        for key, graph in (("eager_ms_per_step", False), ("graph_replay_ms_per_step", True)):
            smp.init()
            smp.run(nsteps=warmup, use_graph=graph)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            smp.run(nsteps=steps, use_graph=graph, sync=True)
            torch.cuda.synchronize(dev)
            row[key] = (time.perf_counter() - t0) * 1e3 / steps
        row["nonfinite_graphs"] = int(smp.state()[2].sum())
        rows.append(row)
        del smp

    net = build_net(dma, args.layers, 64).to(dev).eval()
    net.precision = args.precision
    per_step = args.layers * 4 + 1            # L x {node_pre, edge X, edge M, node_post} + fused update
    run("1 x 64-atom cell, fully connected (the reference's per-call workload)", net, [64], H - A - 1, per_step)
    run("5 x 64-atom cells (gen_num_per_spectrum = 5, one device batch)", net, [64] * 5, H - A - 1, per_step)
    run("1 x 20-atom cell", net, [20], H - A - 1, per_step)
    torch.manual_seed(2025)
    toy = dma.EquivariantGNN(args.layers, 7, W, M, 7, W, 1, 3 + M, W, 3)     # unconditional variant: H = 2 + 1
    with torch.no_grad():
        for layer in toy.egcl_list:
            layer.mlp_x[4].weight.mul_(1e-3)
            layer.mlp_x[4].bias.mul_(1e-3)
    toy.to(dev).eval()
    toy.precision = args.precision
    run("configs[0] shape: 4 x 2-atom Si-O graphs, H = 3", toy, [2] * 4, 0, per_step)
    return {"unit": "ms per reverse step", "steps": steps, "rows": rows,
            "reference_trace_ms_per_step": 6.9,
            "reference_trace_note": "model_flex.ipynb:218, 34.64 s per 5 samples x (T+1) forwards if T = 1000; unknown NVIDIA GPU"}


def self_launch(args):
    """`python bench.py --gpus N` from a plain shell: start the N ranks as a child torch.distributed.run (nothing in
    this process has touched the GPU; the child is a new process, not an exec of this one)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=None,
                    help="repetitions of the K timed steps; the median is reported (default 1, with --full 5)")
    ap.add_argument("--batch", type=int, default=256, help="graphs per GPU")
    ap.add_argument("--atoms", type=int, default=64)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "bf16x3", "f16c8", "fp32"])
    ap.add_argument("--mode", default="sample", choices=["sample", "train", "slab"],
                    help="sample = headline metric (default; with --full also the ddp_train and the other sub-records); train = BASELINE configs[3] "
                         "shape only (fwd+bwd+all-reduce+Adam) as the headline of the line; slab = BASELINE configs[4] only")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-train-leg", action="store_true")
    ap.add_argument("--no-slab-leg", action="store_true")
    ap.add_argument("--no-latency-leg", action="store_true")
    ap.add_argument("--no-precision-legs", action="store_true", help="skip the tolerance_grade / fp16 / c3 sub-records")
    ap.add_argument("--train-steps", type=int, default=8)
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline figure: the median of --reps repetitions, hipGraph replay, "
                         "and the ddp_train / slab / precision / latency / CPU-baseline sub-records (the --no-* options select)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step as DIR/<name>.npy (float32)")
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 5 if args.full else 1

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args))
    rk = Ranks(args)
    if rk.world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={rk.world}")
    valid = True
    if args.mode == "train":
        tr = train_leg(args, rk, args.steps, args.warmup, args.batch, dump_dir=args.dump_outputs)
        out = dict(tr)
        out.update({"n_gpus": rk.world, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                    "dtype": args.precision, "data": "synthetic",
                    "config": {"workload": f"{args.atoms}-atom SiO2 cells x {args.batch} graphs/GPU, {args.layers}-layer EGNN, "
                                           f"{tr['step']}", "global_batch": rk.world * args.batch,
                               "parallelism": f"dp{rk.world}"}})
        valid = tr["finite"]
    elif args.mode == "slab":
        out = slab_leg(args, rk, args.steps, args.warmup, dump_dir=args.dump_outputs)
        out.update({"n_gpus": rk.world, "higher_is_better": True, "vs_baseline": None, "dtype": args.precision,
                    "data": "synthetic", "config": {"workload": "4096-atom slab, radius graph ~40k directed edges, "
                                                                f"{args.layers}-layer EGNN, T=1000 reverse steps",
                                                    "parallelism": f"node-partitioned x{rk.world}"}})
        valid = out["nonfinite_graphs"] == 0
    else:
        out, sd = sample_leg(args, rk, dump_dir=args.dump_outputs)
        valid = out["nonfinite_graphs"] == 0
    if args.mode == "sample" and args.full:
        if not args.no_train_leg:
            if args.atoms == 64:
                tr = train_leg(args, rk, args.train_steps, 2, 256)
                out["ddp_train"] = tr
                valid = valid and tr["finite"]
                if rk.world > 1:   # what a scaling table of the data-PARALLEL path needs, at the top level of the N > 1 line
                    out["ddp_train_value"] = tr["value"]
                    out["ddp_train_unit"] = tr["unit"]
                    out["ddp_efficiency"] = tr.get("ddp_efficiency")
                    out["rccl_ranks"] = tr["rccl_ranks"]
        if not args.no_slab_leg and args.atoms == 64:
            sl = slab_leg(args, rk, 50, 10)
            out["slab_4096"] = sl
            valid = valid and sl["nonfinite_graphs"] == 0
        if rk.world == 1 and not args.no_precision_legs and args.atoms == 64 and args.batch == 256 and args.precision == "bf16":
            out.update(precision_legs(args, rk))
            valid = valid and all(out[k]["nonfinite_graphs"] == 0 for k in ("tolerance_grade", "fp16", "c3"))
        if (rk.world == 1 and not args.no_train_leg and not args.no_precision_legs and args.atoms == 64 and args.batch == 256 and
                args.precision == "bf16" and "tolerance_grade" in out):
            # the same training step at the tolerance grade: forward on the tolerance-grade precision's kernels, backward = the fp32
            # chain of stage kernels with head + remainder products on the library's own GEMM kernels (no BLAS library in the step)
            import copy
            a2 = copy.copy(args)
            a2.precision = out["tolerance_grade"]["precision"]
            tg_tr = train_leg(a2, rk, 3, 1, 256)
            tg_tr["precision"] = a2.precision
            tg_tr["backward"] = ("fp32 chain of stage kernels, every product as head + remainder bf16 operands on egnn_gemm_tn_bf16 / "
                                 "egnn_gemm_rows_bf16 (gemm.mm_tn_split / mm_nn_split): no BLAS library in the step")
            out["ddp_train_tolerance_grade"] = tg_tr
            valid = valid and tg_tr["finite"]
        if rk.world == 1 and not args.no_latency_leg and args.atoms == 64:
            out["latency"] = latency_leg(args, rk)
        if rk.world == 1 and rk.rank == 0 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(sd, args.atoms, args.cpu_seconds)
            out["gpu_over_cpu"] = out["value"] / out["cpu_baseline"]["value"]
    if rk.world > 1:
        # any rank with a non-finite state invalidates the line
        import torch.distributed as dist
        flag = torch.tensor([0 if valid else 1], device=rk.dev if rk.backend == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        valid = int(flag.item()) == 0
    if rk.rank == 0:
        out["valid"] = valid
        if not valid:
            out["invalid_value"] = out.pop("value", None)
            out["value"] = None
        print(json.dumps(out), flush=True)
    rk.close()
    if not valid:
        sys.exit(3)


if __name__ == "__main__":
    main()

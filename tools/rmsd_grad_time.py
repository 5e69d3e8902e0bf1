"""Time forward + backward of the RMSD loss (diffusion_model_amd.stats.rmsd_loss: kabsch_kernel + kabsch_backward_kernel of
csrc/eval/kabsch.hip) with device events after a warm-up, for 256 graphs of 64 atoms (silica-like clouds) and 32 graphs of 512
atoms (uniform random points in a 12 A cube), each rigidly moved with 0.2 A of noise, against the
reference's method on the SAME device tensors: a per-graph loop spelled as kabsch_torch (evaluate_rmsd_for_pos_generate.py:11-51;
centroids, H, torch.linalg.svd, the sign fix on a clone of Vt, R, the residual), summed and divided by the number of graphs as
train_2024_11.py:233-236 does, with torch autograd for the backward.

Both kernels run one wavefront per graph: 256 graphs are 256 waves on 256 CUs, 32 graphs use an eighth of the chip, and each
wave walks its atoms 64 at a time through three passes with a 3x3 Jacobi SVD in fp64 between them.  The launch is latency-bound
(dependent fp64 chains, butterfly reductions), not bandwidth-bound: a 64-atom pair is 768 B.

  python tools/rmsd_grad_time.py                  # the record -> profiles/rmsd_grad_time.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def reference_form_loss(P, Q, sizes):
    """the reference's per-graph loop, on device tensors, under autograd"""
    import torch
    total, lo = 0.0, 0
    for n in sizes:
        p_, q_ = P[lo:lo + n], Q[lo:lo + n]
        lo += n
        p, q = p_ - p_.mean(0), q_ - q_.mean(0)
        U, S, Vt = torch.linalg.svd(p.T @ q)
        if torch.det(Vt.T @ U.T) < 0.0:
            Vt = Vt.clone()
            Vt[:, -1] *= -1.0
        R = Vt.T @ U.T
        total = total + torch.sqrt(((p @ R.T - q) ** 2).sum() / n)
    return total / len(sizes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rmsd_grad_time.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import diffusion_model_amd as dma
    from tests import _rmsd_util as RU
    if not torch.cuda.is_available():
        raise SystemExit("tools/rmsd_grad_time.py measures on the GPU: no device visible")
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
              "gcn_arch": torch.cuda.get_device_properties(0).gcnArchName, "cases": {}}
    for B, n in ((256, 64), (32, 512)):
        sizes = [n] * B
        # 64 atoms: silica-like clouds (rejection-sampled, atoms at least 1.2 A apart); 512 atoms: uniform points in a 12 A cube
        # (the rejection sampling is quadratic in n).  The kernels' work does not depend on the coordinates.
        silica = n <= 64
        base = np.concatenate([RU.silica_cloud(rng, n) for _ in range(B)]) if silica else rng.uniform(-6, 6, (B * n, 3))
        Q = torch.from_numpy(base.astype(np.float32)).to(dev)
        rot = np.stack([RU.random_rotation(rng) for _ in range(B)])
        moved = np.einsum("bij,bnj->bni", rot, base.reshape(B, n, 3)).reshape(-1, 3) + 0.2 * rng.standard_normal((B * n, 3))
        P = torch.from_numpy(moved.astype(np.float32)).to(dev).requires_grad_(True)

        def fused():
            P.grad = None
            dma.stats.rmsd_loss(P, Q, sizes).backward()

        def loop():
            P.grad = None
            reference_form_loss(P, Q, sizes).backward()

        fused()
        g_fused, l_fused = P.grad.clone(), float(dma.stats.rmsd_loss(P, Q, sizes).detach())
        loop()
        g_loop, l_loop = P.grad.clone(), float(reference_form_loss(P, Q, sizes).detach())
        steps_loop = max(1, args.steps // 10)
        timed(fused, args.warmup)
        timed(loop, 1)
        ms = {"fused": [], "loop": []}
        for _ in range(args.rounds):                            # alternating
            ms["fused"].append(timed(fused, args.steps))
            ms["loop"].append(timed(loop, steps_loop))
        case = {"graphs": B, "atoms_per_graph": n,
                "coordinates": ("silica-like clouds (tests/_rmsd_util.silica_cloud)" if silica else "uniform random points in a 12 A cube") +
                               ", rigidly moved, noise 0.2 A", "loss": l_fused, "loss_difference": abs(l_fused - l_loop),
                "max_abs_gradient_difference": float((g_fused - g_loop).abs().max()), "max_abs_gradient": float(g_loop.abs().max()),
                "device_ms_per_step_rounds": [round(v, 4) for v in ms["fused"]], "device_ms_per_step": round(min(ms["fused"]), 4),
                "reference_form_loop_ms_per_step_rounds": [round(v, 3) for v in ms["loop"]],
                "reference_form_loop_ms_per_step": round(min(ms["loop"]), 3), "loop_steps_per_window": steps_loop,
                "loop_over_device": round(min(ms["loop"]) / min(ms["fused"]), 1)}
        record["cases"][f"{B}x{n}"] = case
        print(f"{B} x {n}", json.dumps(case), flush=True)
    record["note"] = ("ms per step: device events around steps_per_window back-to-back forward + backward calls of the Python entry point "
                      "(host work of the call and of autograd included), best of the rounds, the two forms alternating; one wavefront "
                      "per graph in both kernels: latency-bound")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(record, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

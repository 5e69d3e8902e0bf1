"""Time ONE optimizer step on the production parameter list (L = 4, H = 36, W = 1024, m = 256 EquivariantGNN +
SpectrumCompressor: 72 tensors, 7,258,996 fp32 elements) with seeded gradients: the fused HIP classes against the unfused
classes of the same name, alternating in one process, for Adam, AdamW(amsgrad) and RAdamScheduleFree.  Device events around
--steps steps after a warm-up, --rounds rounds; writes ms per step, the bytes a step has to move (from the shapes), the share
of the 6.29 TB/s streaming figure and the launch count of the fused plan to --out (profiles/optim_step.json).

  python tools/optim_time.py                                   # the record
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/optim_time.py --fused-only --rounds 1 --out DIR/t.json
                                                               # kernel time of optim_step_kernel, in a run of its own
  python tools/optim_time.py --summarize DIR                   # -> the kernel rows of that trace as text
"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_TBPS = 6.29       # float4 copy on this chip
STREAMS = {"Adam": 7, "AdamW": 9, "RAdamScheduleFree": 7}      # fp32 streams per element: read p, g, states; write p, states


def summarize(trace_dir):
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "optim_step_kernel" in r.get("Name", ""):
                rows.append(r)
    print("# optim_step_kernel<0> = Adam, <1> = AdamW-amsgrad, <2> = RAdamScheduleFree (EGNN_OPTIM_* of include/egnn_amd.h)")
    for r in sorted(rows, key=lambda r: r["Name"]):
        print(f"{r['Name']}: calls {r['Calls']}, average {float(r['AverageNs']) / 1e3:.2f} us, min {float(r['MinNs']) / 1e3:.2f} us, "
              f"max {float(r['MaxNs']) / 1e3:.2f} us")
    if not rows:
        print("no optim_step_kernel rows under", trace_dir)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step.json"))
    ap.add_argument("--summarize", metavar="DIR")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)

    import torch
    import diffusion_model_amd as dma
    from diffusion_model_amd import optim as dopt
    if not torch.cuda.is_available():
        raise SystemExit("tools/optim_time.py measures on the GPU: no device visible")
    dev = "cuda"
    H, M, W = 36, 256, 1024
    torch.manual_seed(0)
    net = dma.EquivariantGNN(args.layers, 2 * H + 1, W, M, 2 * H + 1, W, 1, H + M, W, H)
    comp = dma.SpectrumCompressor(200, [150, 100, 50], 32)
    init = [p.detach().clone() for p in list(net.parameters()) + list(comp.parameters())]
    numels = [p.numel() for p in init]
    gen = torch.Generator(device=dev).manual_seed(1)
    grads = [torch.randn(p.shape, device=dev, generator=gen) * 1e-2 for p in init]
    hyper = dict(lr=1e-5, weight_decay=1e-12)                   # the reference's
    classes = {"Adam": (torch.optim.Adam, dma.FusedAdam, hyper), "AdamW": (torch.optim.AdamW, dma.FusedAdamW, dict(hyper, amsgrad=True)),
               "RAdamScheduleFree": (dma.RAdamScheduleFree, dma.FusedRAdamScheduleFree, dict(lr=1e-5))}

    def timed(opt, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            opt.step()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    record = {"tensors": len(numels), "elements": sum(numels), "steps_per_window": args.steps, "warmup_steps": args.warmup,
              "stream_tb_per_s": STREAM_TBPS, "gcn_arch": torch.cuda.get_device_properties(0).gcnArchName, "optimizers": {}}
    for name, (unfused_cls, fused_cls, kw) in classes.items():
        opts = {}
        for tag, cls in (("unfused", unfused_cls), ("fused", fused_cls)):
            if tag == "unfused" and args.fused_only:
                continue
            ps = [torch.nn.Parameter(p.to(dev)) for p in init]
            for p, g in zip(ps, grads):
                p.grad = g                                      # gradients are read, never written: shared by both
            opts[tag] = cls(ps, **kw)
            if name == "RAdamScheduleFree":
                opts[tag].train()
        for opt in opts.values():
            timed(opt, args.warmup)
        ms = {tag: [] for tag in opts}
        for _ in range(args.rounds):
            for tag, opt in opts.items():                       # alternating
                ms[tag].append(timed(opt, args.steps))
        nbytes = STREAMS[name] * 4 * sum(numels)
        floor_us = nbytes / (STREAM_TBPS * 1e12) * 1e6
        row = {"bytes_per_step": nbytes, "streaming_floor_us": round(floor_us, 2),
               "fused_launches_per_step": len(dopt.plan_launches(numels)),
               "fused_ms_per_step_rounds": [round(v, 5) for v in ms["fused"]], "fused_ms_per_step": round(min(ms["fused"]), 5),
               "fused_step_share_of_streaming_floor": round(floor_us / (min(ms["fused"]) * 1e3), 3)}
        if "unfused" in ms:
            row.update({"unfused_ms_per_step_rounds": [round(v, 5) for v in ms["unfused"]], "unfused_ms_per_step": round(min(ms["unfused"]), 5),
                        "unfused_over_fused": round(min(ms["unfused"]) / min(ms["fused"]), 2)})
        record["optimizers"][name] = row
        print(name, json.dumps(row), flush=True)
    record["note"] = ("ms per step: device events around steps_per_window back-to-back optimizer steps (host launch cost included when "
                      "the host is the bottleneck), best of the rounds; the kernel's own time comes from a rocprofv3 kernel trace")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(record, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

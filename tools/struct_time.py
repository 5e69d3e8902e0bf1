"""Time the whole-structure statistics (csrc/eval/structure.hip through stats.structure_profile: pair counts over every centre,
partial RDFs, coordination numbers, bond angles; A = 2, default settings) on three batch shapes:

  256 graphs of 64 atoms (C2)        32 graphs of 512 atoms (C3)        1 graph of 4096 atoms (C5)

  device     stats.structure_profile(pos, onehot, sizes) on device tensors: the whole call (one-hot check, tile lists, one upload,
             three kernels, the overflow check), host clock, synchronised.  And the kernels alone, device events around
             back-to-back launches on prepared inputs: pair counts (ordered pairs per second), bonds, the RDF finish.
  torch (a)  the same statistics as a batched torch formulation on the same device tensors: cdist -> bucketize -> index_add_ for
             the pair counts, a bond matrix for CN, padded neighbour lists -> acos -> index_add_ for the angles.  Its float32
             distances are torch's, so a count can differ where a distance sits within rounding of an edge; the number of
             differing histogram entries is recorded, nothing is asserted.
  host (b)   the reference's method on the host, for the two smaller shapes: per centre, the distances to all other atoms, the
             bin search, the bonded neighbours and their angles (the numpy restatement of tests/_struct_util.py, centre by centre
             as RDF(roll(position, i)) would be called), graphs spread over 16 threads.

Best of 5 alternated rounds.  Nothing here is an estimate: a run without a GPU fails.

  python tools/struct_time.py                       # -> profiles/struct_time.json
"""
import argparse
import json
import os
import sys
import time
from multiprocessing.pool import ThreadPool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R, DR, SIGMA, CUTOFF, DTHETA, MAX_CN = 5.0, 0.01, 5, 2.0, 1.0, 16


def torch_profile(torch, pos, types, B, n, A, nbins, edges_lo, edges_hi, nth):
    """competitor (a): equal-sized graphs, everything batched"""
    dev = pos.device
    p = pos.view(B, n, 3)
    t = types.view(B, n).long()
    d = torch.cdist(p, p)
    eye = torch.eye(n, dtype=torch.bool, device=dev)
    k = torch.bucketize(d, edges_lo, right=False) - 1                       # the last bin whose lower edge lies below d
    kk = k.clamp(0, nbins - 1)
    ok = (k >= 0) & (k < nbins) & (edges_lo[kk] < d) & (d < edges_hi[kk]) & ~eye
    g = torch.arange(B, device=dev)[:, None, None]
    row = ((g * A + t[:, :, None]) * A + t[:, None, :]) * nbins + kk
    counts = torch.zeros(B * A * A * nbins, dtype=torch.int64, device=dev)
    counts.index_add_(0, row[ok], torch.ones((), dtype=torch.int64, device=dev).expand(int(ok.sum())))
    bond = (d < CUTOFF) & ~eye
    per_type = torch.stack([(bond & (t[:, None, :] == b)).sum(-1) for b in range(A)], -1).clamp(max=MAX_CN)      # [B, n, A]
    cn = torch.zeros(B * A * A * (MAX_CN + 1), dtype=torch.int64, device=dev)
    cn_row = ((g[:, :, 0][..., None] * A + t[:, :, None]) * A + torch.arange(A, device=dev)) * (MAX_CN + 1) + per_type
    cn.index_add_(0, cn_row.reshape(-1), torch.ones(cn_row.numel(), dtype=torch.int64, device=dev))
    deg = bond.sum(-1)
    m = int(deg.max())
    P = A * (A + 1) // 2
    ang = torch.zeros(B * A * P * nth, dtype=torch.int64, device=dev)
    if m >= 2:
        idx = bond.to(torch.int8).argsort(dim=-1, descending=True, stable=True)[..., :m]                         # [B, n, m]
        valid = torch.arange(m, device=dev) < deg[..., None]
        pd = p.double()
        v = torch.gather(pd[:, None].expand(B, n, n, 3), 2, idx[..., None].expand(B, n, m, 3)) - pd[:, :, None]
        tn = torch.gather(t[:, None].expand(B, n, n), 2, idx)
        norm = torch.linalg.vector_norm(v, dim=-1)
        cos = (torch.einsum("bnjx,bnkx->bnjk", v, v) / (norm[..., :, None] * norm[..., None, :])).clamp(-1, 1)
        kth = torch.floor(torch.rad2deg(torch.acos(cos)) / DTHETA + 0.5).long().clamp(max=nth - 1)
        upper = torch.triu(torch.ones(m, m, dtype=torch.bool, device=dev), 1)
        keep = valid[..., :, None] & valid[..., None, :] & upper & (norm[..., :, None] > 0) & (norm[..., None, :] > 0)
        lo_t, hi_t = torch.minimum(tn[..., :, None], tn[..., None, :]), torch.maximum(tn[..., :, None], tn[..., None, :])
        pair = lo_t * A - lo_t * (lo_t - 1) // 2 + (hi_t - lo_t)
        a_row = ((g[..., None] * A + t[:, :, None, None]) * P + pair) * nth + kth
        ang.index_add_(0, a_row[keep], torch.ones((), dtype=torch.int64, device=dev).expand(int(keep.sum())))
    return counts.view(B, A, A, nbins), cn.view(B, A, A, MAX_CN + 1), ang.view(B, A, P, nth)


def host_graph(SU, np, pos, types, A, nbins, nth):
    """competitor (b): one graph, centre by centre"""
    n = len(pos)
    counts = np.zeros((A, A, nbins), dtype=np.int64)
    cn = np.zeros((A, A, MAX_CN + 1), dtype=np.int64)
    ang = np.zeros((A, A * (A + 1) // 2, nth), dtype=np.int64)
    for i in range(n):
        others = np.arange(n) != i
        dv = pos[others] - pos[i]
        d = np.sqrt((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
        tj = types[others]
        for k in SU.radial_bins(d, DR, nbins):
            keep = k >= 0
            np.add.at(counts[types[i]], (tj[keep], k[keep]), 1)
        bonded = d < np.float32(CUTOFF)
        for b in range(A):
            cn[types[i], b, min(int((bonded & (tj == b)).sum()), MAX_CN)] += 1
        nb = np.nonzero(bonded)[0]
        if 2 <= len(nb) <= SU.MAX_NEIGHBOURS:
            v = dv[nb].astype(np.float64)
            a, b = np.triu_indices(len(nb), 1)
            norm = np.sqrt((v * v).sum(1))
            cos = np.clip((v[a] * v[b]).sum(1) / (norm[a] * norm[b]), -1.0, 1.0)
            kth = np.minimum(np.floor(np.degrees(np.arccos(cos)) / DTHETA + 0.5).astype(np.int64), nth - 1)
            tb, tc = np.minimum(tj[nb][a], tj[nb][b]), np.maximum(tj[nb][a], tj[nb][b])
            np.add.at(ang[types[i]], (tb * A - tb * (tb - 1) // 2 + (tc - tb), kth), 1)
    return counts, cn, ang


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "struct_time.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from diffusion_model_amd import stats
    from tests import _struct_util as SU
    if not torch.cuda.is_available():
        raise SystemExit("tools/struct_time.py measures on the GPU: no device visible")
    dev, A = "cuda", 2
    nbins, nth = SU.nbins_of(R, DR), SU.n_angle_bins(DTHETA)
    lo, hi = SU.bin_edges(DR, nbins)
    edges_lo, edges_hi = torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev)
    record = {"rounds": args.rounds, "warmup_calls": args.warmup, "host_threads": args.threads, "types": A,
              "settings": dict(sigma=SIGMA, R=R, dR=DR, cutoff=CUTOFF, dtheta=DTHETA, max_cn=MAX_CN),
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

    for B, n, calls_dev, with_host in ((256, 64, 20, True), (32, 512, 20, True), (1, 4096, 20, False)):
        sizes = [n] * B
        pos_h, types_h = SU.random_batch(B * 1000 + n, sizes, A)       # 27 cubic angstrom per atom: a few bonds per centre
        pos, types = torch.from_numpy(pos_h).to(dev), torch.from_numpy(types_h).to(dev)
        onehot = torch.eye(A, dtype=torch.int64, device=dev)[types.long()]
        pool = ThreadPool(args.threads)

        def device_flow():
            return stats.structure_profile(pos, onehot, sizes, sigma=SIGMA, R=R, dR=DR, cutoff=CUTOFF, dtheta=DTHETA, max_cn=MAX_CN)

        def torch_flow():
            return torch_profile(torch, pos, types, B, n, A, nbins, edges_lo, edges_hi, nth)

        def host_loop():
            graphs = [(pos_h[g * n:(g + 1) * n], types_h[g * n:(g + 1) * n]) for g in range(B)]
            return pool.map(lambda pt: host_graph(SU, np, pt[0], pt[1], A, nbins, nth), graphs)

        prof, ref = device_flow(), torch_flow()
        differ = [int((a != b).sum()) for a, b in zip((prof.pair_counts, prof.cn, prof.angles), ref)]
        wall(device_flow, args.warmup)
        wall(torch_flow, args.warmup)
        ms = {"device": [], "torch": [], "host": []}
        for _ in range(args.rounds):                            # alternating
            ms["device"].append(wall(device_flow, calls_dev))
            ms["torch"].append(wall(torch_flow, 3))
            if with_host:
                ms["host"].append(wall(host_loop, 1))
        inp = stats._StructInput(pos, onehot, sizes, "struct_time")
        counts = stats._pair_counts(inp, R, DR)
        kernels = {"pair_counts": lambda: stats._pair_counts(inp, R, DR), "bonds": lambda: stats._bonds(inp, CUTOFF, DTHETA, MAX_CN),
                   "rdf_finish": lambda: stats._rdf_finish(inp, counts, SIGMA, R, DR)}
        ms_k = {}
        for name, fn in kernels.items():
            events(fn, args.warmup)
            ms_k[name] = [events(fn, calls_dev) for _ in range(args.rounds)]
        pool.close()
        pairs = B * n * (n - 1)
        rec = {"graphs": B, "atoms_per_graph": n, "ordered_pairs": pairs, "pair_tiles": inp.n_pair, "bond_tiles": inp.n_bond,
               "histogram_entries_differing_from_torch": dict(zip(("pair_counts", "cn", "angles"), differ)),
               "device_ms_per_call_rounds": [round(v, 3) for v in ms["device"]], "device_ms_per_call": round(min(ms["device"]), 3),
               "torch_ms_per_call_rounds": [round(v, 3) for v in ms["torch"]], "torch_ms_per_call": round(min(ms["torch"]), 3),
               "torch_over_device": round(min(ms["torch"]) / min(ms["device"]), 2)}
        if with_host:
            rec.update({"host_ms_per_call_rounds": [round(v, 1) for v in ms["host"]], "host_ms_per_call": round(min(ms["host"]), 1),
                        "host_over_device": round(min(ms["host"]) / min(ms["device"]), 1)})
        for name, v in ms_k.items():
            rec[f"{name}_kernel_ms_rounds"] = [round(x, 4) for x in v]
            rec[f"{name}_kernel_ms"] = round(min(v), 4)
        rec["pair_kernel_ordered_pairs_per_second"] = round(pairs / (min(ms_k["pair_counts"]) * 1e-3), 0)
        record["batches"][f"{B}x{n}"] = rec
        print(f"{B} x {n}", json.dumps(rec), flush=True)
    record["note"] = ("device / torch / host: host clock around whole calls, synchronised, best of the alternated rounds.  *_kernel_ms: "
                      "device events around back-to-back launches on prepared inputs (the pair-count and bond figures include the "
                      "memset of their outputs).")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(record, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

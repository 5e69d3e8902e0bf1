"""Time the SOAP entries (csrc/eval/soap.hip through diffusion_model_amd.soap; A = 2, the default basis r_cut=8, n_max=15, l_max=10,
sigma=0.1: 5,115 features) on three shapes:

  256 graphs of 64 atoms, atom 0 of each     32 graphs of 512 atoms, every atom     template_matching of 1,024 targets x 1,024
                                                                                     references (64 atoms, 200 spectrum points)

  device   the whole call, host clock, synchronised: soap.soap_similarity(originals, samples) for the first shape; two
           soap.soap_descriptors(centres="all") and one soap.cosine for the second; soap.template_matching for the third (records on
           the host, as a data set holds them: collation and upload are inside).  And the four entries alone, device events around
           back-to-back launches on prepared inputs: egnn_soap_descriptor, egnn_soap_cosine, egnn_soap_gram, egnn_spectrum_nearest.
  host     the same scores from a float64 numpy restatement over the same exact tables (neighbours of a centre summed by einsum,
           the power spectrum as one Gram matrix per l), centres spread over 16 threads.  Its similarities must equal the device's
           within the cosine bar of tests/test_gpu_soap.py, 4 (8 E_host + 8 E_host) (asserted).

Best of 5 alternated rounds.  Nothing here is an estimate: a run without a GPU fails.  The tool sets no threshold.

  python tools/soap_time.py                       # -> profiles/soap_time.json
  python tools/soap_time.py --quick --out /dev/null   # the same flows on small shapes: a check of the tool, not a measurement
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


class HostSoap:
    """float64 numpy restatement, vectorised over the neighbours of a centre"""

    def __init__(self, np, basis, A):
        self.np, self.A, self.b = np, A, basis
        L1 = basis.l_max + 1
        self.l_of = np.repeat(np.arange(L1), 2 * np.arange(L1) + 1)
        from tests import _soap_util as SU
        self.SU = SU
        z1, z2, n1, n2, ll = SU.feature_index(A, basis.n_max, basis.l_max)
        self.rows, self.cols, self.ll = z1 * basis.n_max + n1, z2 * basis.n_max + n2, ll
        self.cut2 = basis.neighbour_cut ** 2

    def descriptor(self, pos, types, i):
        """the power spectrum of atom i of ONE graph (pos float64 [n, 3])"""
        np, b = self.np, self.b
        d = pos - pos[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        keep = d2 < self.cut2
        d, d2, t = d[keep], d2[keep], types[keep]
        R = self.SU.solid_harmonics(d, b.l_max, b.norm)
        rad = (b.K[None] * np.exp(-(b.gamma[None] * d2[:, None, None])))[:, :, self.l_of]          # [P, n, lm]
        prim = np.stack([np.einsum("jnq,jq->nq", rad[t == z], R[t == z]) for z in range(self.A)])
        c = np.einsum("lnq,zql->znl", b.beta[self.l_of], prim).reshape(self.A * b.n_max, -1)
        P = np.stack([c[:, l * l:(l + 1) ** 2] @ c[:, l * l:(l + 1) ** 2].T for l in range(b.l_max + 1)], -1)
        return b.weight[self.ll] * P[self.rows, self.cols, self.ll]

    @staticmethod
    def cosine(np, a, b):
        return (a * b).sum(-1) / (np.sqrt((a * a).sum(-1)) * np.sqrt((b * b).sum(-1)))


def clouds(np, seed, B, n, A, jitter=None):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, 2.2 * np.cbrt(n), (B * n, 3))                                            # 10.6 cubic angstrom per atom
    types = rng.integers(0, A, B * n)
    if jitter is not None:
        pos = pos + jitter * np.random.default_rng(seed + 1).standard_normal(pos.shape)
    return pos.astype(np.float32), types


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--quick", action="store_true", help="small shapes: a check of the tool itself, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soap_time.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from diffusion_model_amd import _lib, soap
    from tests._soap_util import e_host
    if not torch.cuda.is_available():
        raise SystemExit("tools/soap_time.py measures on the GPU: no device visible")
    dev, A = "cuda", 2
    basis = soap.SoapBasis()
    host = HostSoap(np, basis, A)
    bar = 4 * (8 * e_host("default") + 8 * e_host("default"))
    F = basis.features(A)
    record = {"quick": args.quick, "rounds": args.rounds, "warmup_calls": args.warmup, "host_threads": args.threads, "types": A, "features": F,
              "basis": dict(r_cut=basis.r_cut, n_max=basis.n_max, l_max=basis.l_max, sigma=basis.sigma), "cosine_bar": bar,
              "gcn_arch": torch.cuda.get_device_properties(0).gcnArchName, "shapes": {}}
    eye = torch.eye(A, dtype=torch.int64)
    pool = ThreadPool(args.threads)

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

    def measure(name, device_flow, host_flow, calls_dev, extra):
        got, want = np.asarray(device_flow(), dtype=np.float64), np.asarray(host_flow(), dtype=np.float64)
        worst = float(np.abs(got - want).max())
        assert got.shape == want.shape and worst <= bar, f"{name}: device and host similarities differ by {worst:.3e} (bar {bar:.3e})"
        wall(device_flow, args.warmup)
        ms = {"device": [], "host": []}
        for _ in range(args.rounds):                            # alternating
            ms["device"].append(wall(device_flow, calls_dev))
            ms["host"].append(wall(host_flow, 1))
            print(f"  {name}: device {ms['device'][-1]:.3f} ms, host {ms['host'][-1]:.1f} ms", flush=True)
        rec = dict(extra, similarities=int(got.size), mean_similarity=round(float(got.mean()), 4), worst_similarity_difference=worst,
                   device_ms_per_call_rounds=[round(v, 3) for v in ms["device"]], device_ms_per_call=round(min(ms["device"]), 3),
                   host_ms_per_call_rounds=[round(v, 1) for v in ms["host"]], host_ms_per_call=round(min(ms["host"]), 1),
                   host_over_device=round(min(ms["host"]) / min(ms["device"]), 2))
        record["shapes"][name] = rec
        print(name, json.dumps(rec), flush=True)
        return rec

    def kernel_ms(rec, kernels, calls):
        for name, fn in kernels.items():
            events(fn, args.warmup)
            v = [events(fn, calls) for _ in range(args.rounds)]
            rec[f"{name}_ms_rounds"], rec[f"{name}_ms"] = [round(x, 4) for x in v], round(min(v), 4)

    def host_first(sides, B, n):
        def one(g):
            rows = [host.descriptor(p[g * n:(g + 1) * n].astype(np.float64), t[g * n:(g + 1) * n], 0) for p, t in sides]
            return HostSoap.cosine(np, rows[0], rows[1])
        return pool.map(one, range(B))

    # ---- 256 x 64, atom 0 ------------------------------------------------------------------------------------------------------------
    B, n = (8, 64) if args.quick else (256, 64)
    sides = [clouds(np, 1, B, n, A), clouds(np, 1, B, n, A, jitter=0.03)]
    recs = [[SimpleNamespace(pos=torch.from_numpy(p[g * n:(g + 1) * n]).to(dev), x=eye[torch.from_numpy(t[g * n:(g + 1) * n])].to(dev), id=f"g{g}")
             for g in range(B)] for p, t in sides]
    originals, samples = recs[0], [[s] for s in recs[1]]
    rec = measure(f"{B}x{n}_first", lambda: soap.soap_similarity(originals, samples, basis=basis)[0], lambda: host_first(sides, B, n), 10,
                  dict(graphs=B, atoms_per_graph=n, centres=B))
    pos, onehot = torch.from_numpy(sides[0][0]).to(dev), eye[torch.from_numpy(sides[0][1])].to(dev)
    desc = soap.soap_descriptors(pos, onehot, [n] * B, "first", basis)
    kernel_ms(rec, {"descriptor": lambda: soap.soap_descriptors(pos, onehot, [n] * B, "first", basis), "cosine": lambda: soap.cosine(desc, desc),
                    "gram": lambda: soap.cosine_matrix(desc, desc)}, 10)

    # ---- 32 x 512, every atom --------------------------------------------------------------------------------------------------------
    B, n = (2, 128) if args.quick else (32, 512)
    sides = [clouds(np, 2, B, n, A), clouds(np, 2, B, n, A, jitter=0.03)]
    dsides = [(torch.from_numpy(p).to(dev), eye[torch.from_numpy(t)].to(dev)) for p, t in sides]

    def device_all():
        a, b = (soap.soap_descriptors(p, x, [n] * B, "all", basis) for p, x in dsides)
        return soap.cosine(a, b).cpu().numpy()

    def host_all():
        def one(k):
            g, i = divmod(k, n)
            rows = [host.descriptor(p[g * n:(g + 1) * n].astype(np.float64), t[g * n:(g + 1) * n], i) for p, t in sides]
            return HostSoap.cosine(np, rows[0], rows[1])
        return pool.map(one, range(B * n), chunksize=64)

    rec = measure(f"{B}x{n}_all", device_all, host_all, 3, dict(graphs=B, atoms_per_graph=n, centres=B * n))
    kernel_ms(rec, {"descriptor": lambda: soap.soap_descriptors(dsides[0][0], dsides[0][1], [n] * B, "all", basis)}, 3)

    # ---- template matching, 1,024 x 1,024 ----------------------------------------------------------------------------------------
    T = R = 32 if args.quick else 1024
    n, S = 64, 200
    sides = [clouds(np, 3, T, n, A, jitter=0.03), clouds(np, 3, R, n, A)]
    rng = np.random.default_rng(4)
    base = rng.uniform(0.0, 1.5, (16, S))
    spectra = [(base[rng.integers(0, 16, count)] + 0.2 * rng.standard_normal((count, S))).astype(np.float32) for count in (T, R)]
    recs = [[SimpleNamespace(pos=torch.from_numpy(p[g * n:(g + 1) * n]), x=eye[torch.from_numpy(t[g * n:(g + 1) * n])], id=f"{tag}{g}" if g % 7 else f"shared{g}",
                             spectrum=torch.from_numpy(sp[g:g + 1])) for g in range(len(sp))] for (p, t), sp, tag in zip(sides, spectra, "tr")]

    def device_tm():
        return soap.template_matching(recs[0], recs[1], k=3, basis=basis, device=dev)[3].numpy()

    def host_tm():
        rows = [pool.map(lambda g, p=p, t=t: host.descriptor(p[g * n:(g + 1) * n].astype(np.float64), t[g * n:(g + 1) * n], 0), range(len(sp)))
                for (p, t), sp in zip(sides, spectra)]
        r64 = spectra[1].astype(np.float64)

        def one(q):
            m = ((r64 - spectra[0][q].astype(np.float64)) ** 2).mean(1)
            if q % 7 == 0:
                m[q] = np.inf                                   # the reference of the same id
            best = np.argsort(m, kind="stable")[:3]
            return HostSoap.cosine(np, rows[0][q][None], np.stack([rows[1][j] for j in best]))
        return np.stack(pool.map(one, range(T)))

    rec = measure(f"template_matching_{T}x{R}", device_tm, host_tm, 3, dict(targets=T, references=R, atoms_per_record=n, spectrum_points=S, k=3))
    dt, dr = torch.from_numpy(spectra[0]).to(dev), torch.from_numpy(spectra[1]).to(dev)
    d1 = soap.soap_descriptors(torch.from_numpy(sides[0][0]).to(dev), eye[torch.from_numpy(sides[0][1])].to(dev), [n] * T, "first", basis)
    pairs = torch.stack([torch.arange(T).repeat_interleave(3), torch.arange(3 * T) % R], 1).to(dev)
    kernel_ms(rec, {"nearest": lambda: soap.nearest_spectra(dt, dr, 3), "cosine": lambda: soap.cosine(d1, d1, pairs),
                    "gram": lambda: soap.cosine_matrix(d1, d1)}, 10)
    pool.close()
    record["note"] = ("device / host: host clock around whole calls, synchronised, best of the alternated rounds; measured on the shapes named by "
                      "the keys.  *_ms: device events around back-to-back calls of the Python wrapper on prepared device inputs (descriptor_ms "
                      "includes the one-hot check and the upload of graph_ptr and the centre list; cosine_ms with a pair list its bounds check; "
                      "gram_ms the two norm launches).")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(record, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

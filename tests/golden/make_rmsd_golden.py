#!/usr/bin/env python3
"""Generate tests/golden/rmsd_golden.npz by EXECUTING the reference's RMSD code in the build container (same method as
make_golden.py; run only where the read-only reference tree exists):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_rmsd_golden.py

What is executed:
  * evaluate_rmsd_for_pos_generate.py is imported as it is: kabsch_torch (:11-51) and kabsch_numpy (:53-92).  Its `import wandb`
    (the logging service client: absent, unused by these functions; the driver body is under __main__) is satisfied by an
    EMPTY module object, as in make_golden.py.
  * evaluate_rmsd.py is imported as it is (empty wandb again): kabsch_numpy (:10-42).  Its search loop (:93-107) is part of the
    driver body under __main__, so the TEXT of those lines is read from the reference file at generation time, dedented and
    executed on stand-in `original_graph` / `generated_graph` records (kabsch_numpy is wrapped to record every ordering's RMSD,
    which gives the second-best value).  Nothing of it is stored.
  * parts/def_for_main.py is imported as it is: evaluate_by_rmsd (:73-89).  It imports `kabsch_torch` from a module
    `loss_calculation` that does not exist in the reference tree, and RAdamScheduleFree from `schedulefree` (not installed): a
    module object that carries the only surviving kabsch_torch (the one of evaluate_rmsd_for_pos_generate.py, executed above)
    is registered under the first name and an empty one under the second.  evaluate_by_rmsd_and_atom_type_eval (:91-117) moves
    its atom types to 'cuda' and cannot run here; its RMSD part is the same call, its atom fractions are integer counts.
Only inputs and outputs (arrays) are written.  No reference source is copied.
"""
import os
import sys
import textwrap
import types

os.environ.setdefault("MKL_CBWR", "COMPATIBLE,STRICT")
import numpy as np  # noqa: E402
import torch  # noqa: E402

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import _rmsd_util as RU  # noqa: E402

torch.set_num_threads(8)


def load_reference():
    import importlib
    sys.modules.setdefault("wandb", types.ModuleType("wandb"))
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "parts"))
    pos_generate = importlib.import_module("evaluate_rmsd_for_pos_generate")
    search = importlib.import_module("evaluate_rmsd")
    loss_calculation = types.ModuleType("loss_calculation")
    loss_calculation.kabsch_torch = pos_generate.kabsch_torch
    sys.modules["loss_calculation"] = loss_calculation
    if "schedulefree" not in sys.modules:
        sf = types.ModuleType("schedulefree")
        sf.RAdamScheduleFree = None
        sys.modules["schedulefree"] = sf
    def_for_main = importlib.import_module("def_for_main")
    with open(os.path.join(REF, "evaluate_rmsd.py"), encoding="utf-8") as f:
        lines = f.read().splitlines()
    body = lines[92:107]                                   # :93-107
    assert "original_graph_pos = original_graph.pos - original_graph.pos[0]" in body[0] and "min_R = R" in body[-1]
    return pos_generate, search, def_for_main, textwrap.dedent("\n".join(body))


def run_search(search_mod, body, gen, orig):
    """the reference's loop body on one pair -> (min_rmsd, order, second-best rmsd)"""
    import itertools
    seen = []

    def recording(P, Q):
        R, rmsd = search_mod.kabsch_numpy(P, Q)
        seen.append(float(rmsd))
        return R, rmsd

    ns = {"np": np, "itertools": itertools, "torch": torch, "kabsch_numpy": recording,
          "original_graph": types.SimpleNamespace(pos=torch.from_numpy(orig)),
          "generated_graph": types.SimpleNamespace(pos=torch.from_numpy(gen))}
    exec(body, ns)
    second = float(np.partition(np.array(seen), 1)[1]) if len(seen) > 1 else float("inf")
    return float(ns["min_rmsd"]), [int(v) for v in ns["min_order"]], second, np.asarray(ns["min_R"], dtype=np.float32)


def main():
    pos_generate, search_mod, def_for_main, body = load_reference()
    rng = np.random.default_rng(20250)
    out = {}

    # ---- the three spellings on ~40 pairs ----
    sizes = [2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 10, 12, 14, 16, 18, 20, 22, 24, 27, 30, 33, 36, 40, 44, 48, 52, 56, 60,
             62, 63, 64, 64, 64, 5, 9, 17, 33, 64, 3]
    noises = (0.01, 0.1, 0.5)
    P_all, Q_all, meta = [], [], []
    res = {k: {"R": [], "t": [], "rmsd": []} for k in RU.SPELLINGS}
    sig = {"centroid": [], "first": []}
    floor = {"rmsd": 0.0, "t": 0.0, "R": 0.0}
    for k, n in enumerate(sizes):
        P = RU.silica_cloud(rng, n)
        mirrored = k % 3 == 2
        noise = noises[k % 3] if k < 36 else noises[(k // 2) % 3]
        Q = P * np.array([1.0, 1.0, -1.0]) if mirrored else P.copy()
        Q = Q @ RU.random_rotation(rng).T + rng.uniform(-4, 4, 3) + noise * rng.standard_normal((n, 3))
        P32, Q32 = P.astype(np.float32), Q.astype(np.float32)
        P_all.append(P32)
        Q_all.append(Q32)
        meta.append((n, int(mirrored), noise))
        got = {}
        R, t, rmsd = pos_generate.kabsch_torch(torch.from_numpy(P32), torch.from_numpy(Q32))
        got["torch"] = (R.numpy(), t.numpy(), float(rmsd))
        R, t, rmsd = pos_generate.kabsch_numpy(P32.copy(), Q32.copy())
        got["numpy_centroid"] = (R, t, float(rmsd))
        R, rmsd = search_mod.kabsch_numpy(P32.copy(), Q32.copy())
        got["numpy_first"] = (R, Q32[0] - P32[0], float(rmsd))
        for c in sig:
            sig[c].append(RU.sigma_f64(P32, Q32, c))
        for name, (center, flip) in RU.SPELLINGS.items():
            R, t, rmsd = got[name]
            res[name]["R"].append(np.asarray(R, dtype=np.float32))
            res[name]["t"].append(np.asarray(t, dtype=np.float32))
            res[name]["rmsd"].append(np.float32(rmsd))
            R64, t64, rmsd64 = RU.kabsch_f64(P32, Q32, center, flip)
            s = sig[center][-1]
            # the column fix of a rank-deficient H follows LAPACK's null vector in both precisions: not a noise measurement
            if flip == "row" or RU.full_rank(s):
                floor["rmsd"] = max(floor["rmsd"], abs(rmsd - rmsd64))
            floor["t"] = max(floor["t"], float(np.abs(np.asarray(t, dtype=np.float64) - t64).max()))
            if RU.well_conditioned(s):
                floor["R"] = max(floor["R"], float(np.abs(np.asarray(R, dtype=np.float64) - R64).max()))
    out["kabsch.sizes"] = np.array([m[0] for m in meta], dtype=np.int32)
    out["kabsch.mirrored"] = np.array([m[1] for m in meta], dtype=np.int32)
    out["kabsch.noise"] = np.array([m[2] for m in meta], dtype=np.float64)
    out["kabsch.P"], out["kabsch.Q"] = np.concatenate(P_all), np.concatenate(Q_all)
    for name in res:
        out[f"kabsch.{name}.R"] = np.stack(res[name]["R"])
        out[f"kabsch.{name}.t"] = np.stack(res[name]["t"])
        out[f"kabsch.{name}.rmsd"] = np.array(res[name]["rmsd"], dtype=np.float32)
    for c in sig:
        out[f"kabsch.sigma_{c}"] = np.stack(sig[c])

    # ---- correspondence search, n = 2 .. 8, by the executed loop body ----
    s_sizes, s_gen, s_orig, s_order, s_best, s_second, s_R = [], [], [], [], [], [], []
    for n in (2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8):
        for attempt in range(50):
            orig = RU.silica_cloud(rng, n)
            shuffle = np.concatenate([[0], 1 + rng.permutation(n - 1)])
            noise = (0.02, 0.1, 0.3)[len(s_sizes) % 3] * (0.5 if attempt >= 10 else 1.0)
            gen = (orig @ RU.random_rotation(rng).T + rng.uniform(-3, 3, 3) + noise * rng.standard_normal((n, 3)))[shuffle]
            orig32, gen32 = orig.astype(np.float32), gen.astype(np.float32)
            best, order, second, R = run_search(search_mod, body, gen32, orig32)
            if second - best >= RU.GAP * best:
                break
        else:
            raise SystemExit("no unambiguous search case found: lower the noise")
        assert second - best >= RU.GAP * best
        b64, o64, _ = RU.search_f64(gen32, orig32)
        assert o64 == order, "the float64 restatement picks another ordering than the executed reference"
        floor["rmsd"] = max(floor["rmsd"], abs(best - b64))
        s_sizes.append(n); s_gen.append(gen32); s_orig.append(orig32); s_order.append(np.array(order, dtype=np.int32))
        s_best.append(best); s_second.append(second); s_R.append(R)
    out["search.sizes"] = np.array(s_sizes, dtype=np.int32)
    out["search.gen"], out["search.orig"] = np.concatenate(s_gen), np.concatenate(s_orig)
    out["search.order"] = np.concatenate(s_order)
    out["search.min_rmsd"] = np.array(s_best, dtype=np.float64)
    out["search.second_rmsd"] = np.array(s_second, dtype=np.float64)
    out["search.R"] = np.stack(s_R)

    # ---- evaluate_by_rmsd of parts/def_for_main.py on a list shaped like generate()'s output ----
    # no graphs of 2 or 3 atoms here: about the centroid their H is rank deficient and kabsch_torch's column fix follows LAPACK's
    # null vector (the spellings' golden cases above keep such graphs, with sigma stored so that a test can tell)
    e_sizes = [5, 1, 9, 4, 9, 12, 6, 9, 30, 64, 7]
    e_ids = ["mp-10", "mp-11", "mp-12", "mp-10", "mp-12", "mp-13", "mp-14", "mp-12", "mp-15", "mp-16", "mp-17"]
    originals, generated = [], []
    for k, n in enumerate(e_sizes):
        if k == 7:                                           # an exact repeat of graph 4: equal RMSD, the stable sort decides
            o, g = originals[4], generated[4][-1]
            originals.append(types.SimpleNamespace(pos=o.pos.clone(), x=o.x.clone(), id=e_ids[k], idx=k))
            generated.append([types.SimpleNamespace(pos=g.pos.clone(), x=g.x.clone())])
            continue
        orig = RU.silica_cloud(rng, n)
        noise = 0.03 * (k + 1)
        gen = orig @ RU.random_rotation(rng).T + rng.uniform(-3, 3, 3) + noise * rng.standard_normal((n, 3))
        xo = np.eye(2, dtype=np.int64)[np.concatenate([[0], rng.integers(0, 2, n - 1)])]
        xg = np.eye(2, dtype=np.int64)[rng.integers(0, 2, n)]
        originals.append(types.SimpleNamespace(pos=torch.from_numpy(orig.astype(np.float32)), x=torch.from_numpy(xo), id=e_ids[k], idx=k))
        generated.append([types.SimpleNamespace(pos=torch.from_numpy(gen.astype(np.float32)), x=torch.from_numpy(xg))])
    ranked = def_for_main.evaluate_by_rmsd(originals, generated)
    r = np.array([float(row[1]) for row in ranked])
    gaps = np.diff(r)
    assert all(g == 0.0 or g >= 1e-3 * v for g, v in zip(gaps, r[1:])), "two different graphs closer than 1e-3: redraw"
    out["eval.sizes"] = np.array(e_sizes, dtype=np.int32)
    out["eval.ids"] = np.array(e_ids)
    out["eval.orig_pos"] = torch.cat([o.pos for o in originals]).numpy()
    out["eval.gen_pos"] = torch.cat([g[-1].pos for g in generated]).numpy()
    out["eval.orig_x"] = torch.cat([o.x for o in originals]).numpy()
    out["eval.gen_x"] = torch.cat([g[-1].x for g in generated]).numpy()
    out["eval.ranked_index"] = np.array([row[2].idx for row in ranked], dtype=np.int32)
    out["eval.ranked_id"] = np.array([row[0] for row in ranked])
    out["eval.ranked_rmsd"] = r.astype(np.float32)
    for row in ranked:
        floor["rmsd"] = max(floor["rmsd"], abs(float(row[1]) - RU.kabsch_f64(row[2].pos.numpy(), row[3].pos.numpy())[2]))

    out["ref_vs_f64"] = np.array([floor["rmsd"], floor["t"], floor["R"]], dtype=np.float64)   # rmsd, t, R
    print("ref_vs_f64 (executed fp32 reference against the float64 restatement): "
          f"rmsd {floor['rmsd']:.3e}  t {floor['t']:.3e}  R (well-conditioned cases) {floor['R']:.3e}")
    print("well-conditioned:", {c: int(sum(RU.well_conditioned(s) for s in sig[c])) for c in sig}, "of", len(sizes))
    path = os.path.join(OUT, "rmsd_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/assign_golden.npz by EXECUTING the reference's atom matching in the build container (same method as
make_rmsd_golden.py; run only where the read-only reference tree exists):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_assign_golden.py

What is executed:
  * create_xyz.py is imported as it is: kabsch_numpy (:48-80), hungarian_algorithm (:82-85), return_near_from_exO (:87-96).  Its
    `import wandb` (the logging service client: absent, unused by these functions) is satisfied by an EMPTY module object.
  * The branch for graphs of six atoms or more (:158-192) is part of the driver body under __main__, so the TEXT of those lines
    is read from the reference file at generation time, dedented and executed on stand-in `original_graph` / `generated_graph`
    records; the file writes that follow (:193-196) are not executed.  kabsch_numpy is wrapped to record every fit's RMSD (the first 24
    are the pairings: their second-best value), hungarian_algorithm to keep the two arrays it was given.  Nothing of the text is
    stored.
Only inputs and outputs (arrays) are written.  No reference source is copied.

A case is kept only where the executed reference is unambiguous (redrawn otherwise, with half the noise after ten attempts):
  1. the five smallest distances to atom 0 are separated by more than NEAR_GAP = 1e-4 relative in both structures;
  2. second-best minus best pre-alignment RMSD >= RU.GAP x best;
  3. the cheapest assignment that avoids at least one edge of the optimum costs >= (1 + ASSIGN_GAP = 1e-5) x the optimum
     (n re-solves with one entry forbidden);
and where the float64 restatement of tests/_assign_util.py picks the same pairing and the same assignment as the executed
float32 reference (a disagreement is an ambiguity of the reference at its own precision).
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
from tests import _assign_util as AU  # noqa: E402
from tests import _rmsd_util as RU  # noqa: E402

torch.set_num_threads(8)
NEAR_GAP, ASSIGN_GAP = 1e-4, 1e-5
SIZES = [6, 6, 7, 7, 8, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 22, 24, 26, 28, 30, 32, 34, 36, 40, 44, 48, 52, 56, 60, 62,
         63, 64, 64, 65, 96, 100, 128, 200, 256, 512]
NOISES = (0.02, 0.1, 0.3)


def load_reference():
    import importlib
    sys.modules.setdefault("wandb", types.ModuleType("wandb"))
    sys.path.insert(0, REF)
    mod = importlib.import_module("create_xyz")
    with open(os.path.join(REF, "create_xyz.py"), encoding="utf-8") as f:
        lines = f.read().splitlines()
    body = lines[157:192]                                  # :158-192
    assert "generated_index_list = return_near_from_exO(generated_graph.pos)" in body[0] and "comment = f'{id} {rmsd}'" in body[-1]
    return mod, textwrap.dedent("\n".join(body))


def run_branch(mod, body, orig, gen, xo, xg):
    """the reference's branch on one pair -> dict of what it computed"""
    import itertools
    seen, given = [], {}

    def recording(P, Q):
        R, rmsd = mod.kabsch_numpy(P, Q)
        seen.append(float(rmsd))
        return R, rmsd

    def keeping(P, Q):
        given["P"], given["Q"] = np.array(P, copy=True), np.array(Q, copy=True)
        return mod.hungarian_algorithm(P, Q)

    ns = {"np": np, "itertools": itertools, "torch": torch, "os": os, "kabsch_numpy": recording, "hungarian_algorithm": keeping,
          "return_near_from_exO": mod.return_near_from_exO, "id": "golden",
          "original_graph": types.SimpleNamespace(pos=torch.from_numpy(orig.copy()), x=torch.from_numpy(xo.copy())),
          "generated_graph": types.SimpleNamespace(pos=torch.from_numpy(gen.copy()), x=torch.from_numpy(xg.copy()))}
    exec(body, ns)
    assert len(seen) == 25
    fits = np.sort(np.array(seen[:24]))
    return dict(R=np.asarray(ns["min_R"], dtype=np.float32), perm=AU.PERMS4.index(tuple(ns["min_perm"])), best=float(fits[0]),
                second=float(fits[1]), row_ind=np.asarray(ns["row_ind"]), col_ind=np.asarray(ns["col_ind"]),
                centred=given["P"], aligned=given["Q"], orig_reordered=ns["original_graph"].pos.numpy(),
                gen_reordered=ns["generated_graph"].pos.numpy(), orig_x_reordered=ns["original_graph"].x.numpy(),
                gen_x_reordered=ns["generated_graph"].x.numpy(), rmsd=float(ns["rmsd"]))


def main():
    mod, body = load_reference()
    rng = np.random.default_rng(20251)
    keys = ("orig", "gen", "orig_x", "gen_x", "centred", "aligned", "orig_reordered", "gen_reordered", "row_ind", "col_ind")
    cat = {k: [] for k in keys}
    per = {k: [] for k in ("noise", "R", "perm", "prealign_best", "prealign_second", "near_gap", "opt_cost", "runner_up_cost", "rmsd",
                           "attempts")}
    floor, floor_pos, floor_R, n_R = 0.0, 0.0, 0.0, 0
    for k, n in enumerate(SIZES):
        cloud = RU.silica_cloud(rng, n)
        while AU.near_gap(cloud.astype(np.float32)) <= NEAR_GAP:
            cloud = RU.silica_cloud(rng, n)
        for attempt in range(60):
            noise = NOISES[k % 3] * (0.5 ** (attempt // 10))
            orig, gen, _ = AU.pair_case(rng, n, noise, cloud)   # a redraw keeps the cloud: new motion, shuffle and noise
            gap1 = min(AU.near_gap(orig), AU.near_gap(gen))
            if gap1 <= NEAR_GAP:
                continue
            xo = np.eye(2, dtype=np.int64)[np.concatenate([[0], rng.integers(0, 2, n - 1)])]
            xg = np.eye(2, dtype=np.int64)[np.concatenate([[0], rng.integers(0, 2, n - 1)])]
            got = run_branch(mod, body, orig, gen, xo, xg)
            if got["second"] - got["best"] < RU.GAP * got["best"]:
                continue
            D = AU.distance_matrix(got["centred"], got["aligned"], np.float32).astype(np.float64)   # what scipy was handed
            opt = float(D[got["row_ind"], got["col_ind"]].sum())
            second = AU.runner_up_cost(D, got["col_ind"])
            if second < (1.0 + ASSIGN_GAP) * opt:
                continue
            f64 = AU.align_f64(orig, gen)
            if f64["perm"] != got["perm"] or not np.array_equal(f64["col_ind"], got["col_ind"]):
                continue
            break
        else:
            raise SystemExit(f"no unambiguous case of {n} atoms found")
        assert np.array_equal(got["row_ind"], np.arange(n))
        assert np.array_equal(got["gen_x_reordered"], xg[got["col_ind"]]) and np.array_equal(got["orig_x_reordered"], xo)
        floor = max(floor, abs(got["rmsd"] - f64["rmsd"]))
        floor_pos = max(floor_pos, float(np.abs(got["gen_reordered"] - f64["gen_reordered"]).max()),
                        float(np.abs(got["orig_reordered"] - f64["orig_reordered"]).max()))
        if RU.well_conditioned(RU.sigma_f64(*AU.prealign_points(orig, gen, got["perm"]), "first")):
            n_R += 1
            floor_R = max(floor_R, float(np.abs(got["R"].astype(np.float64) - f64["R"]).max()))
        print(f"n {n:4d} noise {noise:.3f} attempts {attempt + 1:2d}  prealign {got['best']:.4f} / {got['second']:.4f}  "
              f"assignment gap {second / opt - 1:.3e}  rmsd {got['rmsd']:.6f} (f64 {f64['rmsd']:.6f})", flush=True)
        for name, val in (("orig", orig), ("gen", gen), ("orig_x", xo), ("gen_x", xg), ("centred", got["centred"]),
                          ("aligned", got["aligned"]), ("orig_reordered", got["orig_reordered"]),
                          ("gen_reordered", got["gen_reordered"]), ("row_ind", got["row_ind"].astype(np.int32)),
                          ("col_ind", got["col_ind"].astype(np.int32))):
            cat[name].append(val)
        for name, val in (("noise", noise), ("R", got["R"]), ("perm", got["perm"]), ("prealign_best", got["best"]),
                          ("prealign_second", got["second"]), ("near_gap", gap1), ("opt_cost", opt), ("runner_up_cost", second),
                          ("rmsd", got["rmsd"]), ("attempts", attempt + 1)):
            per[name].append(val)
    out = {"sizes": np.array(SIZES, dtype=np.int32),
           "ref_vs_f64": np.array([floor, floor_pos, floor_R], dtype=np.float64),   # rmsd, reordered positions, R
           "gaps": np.array([NEAR_GAP, RU.GAP, ASSIGN_GAP], dtype=np.float64)}
    for name in keys:
        out[name] = np.concatenate(cat[name])
    for name, vals in per.items():
        out[name] = np.stack(vals) if name == "R" else np.array(vals, dtype=np.int32 if name in ("perm", "attempts") else np.float64)
    for name in ("orig", "gen", "centred", "aligned", "orig_reordered", "gen_reordered"):
        assert out[name].dtype == np.float32, name
    print(f"ref_vs_f64 (executed fp32 reference against the float64 restatement): rmsd {floor:.3e}  positions {floor_pos:.3e}  "
          f"R ({n_R} well-conditioned five-point fits) {floor_R:.3e}")
    print(f"smallest assignment gap {np.min(np.array(per['runner_up_cost']) / np.array(per['opt_cost'])) - 1:.3e}")
    path = os.path.join(OUT, "assign_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

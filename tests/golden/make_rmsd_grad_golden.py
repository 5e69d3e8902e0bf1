#!/usr/bin/env python3
"""Generate tests/golden/rmsd_grad_golden.npz by EXECUTING the reference's kabsch_torch under torch autograd in the build
container (same method and module stubs as make_rmsd_golden.py; run only where the read-only reference tree exists):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_rmsd_grad_golden.py

What is executed: evaluate_rmsd_for_pos_generate.py is imported as it is (its `import wandb` satisfied by an EMPTY module
object) and its kabsch_torch (:11-51: centroid, `Vt[:, -1] *= -1` on a clone of Vt, written to be differentiable and used as
the training loss of train_2024_11.py:233-236) is called on tensors that require grad, in float64 and in float32;
L = <g_R, R> + <g_t, t> + g_rmsd rmsd is back-propagated for fixed random cotangents.  Only inputs, cotangents and the resulting
gradients (arrays) are written.  No reference source is copied.

Pairs: RU.silica_cloud, rigidly moved, noise 0.01 / 0.1 / 0.5, every third pair mirrored; sizes include the lane-stride edges of
the one-wavefront kernel (2, 3, 4, 5, 8, 17, 63, 64, 65, 130).  Two kinds, stored in `kind`:
  1  n >= 4 and RU.well_conditioned: all three cotangents; compared in every gradient, against both precisions.
  0  the rest (n = 2, n = 3: rank-deficient H; small singular gaps): g_R = g_t = 0, so only the RMSD is differentiated.  Their
     reflection decision is LAPACK's null-vector sign, so the gradient is stored (`defined` = 1) only where the executed reference
     returned the OPTIMAL rotation (its RMSD equals the row-flip RMSD) and finite gradients: there it is comparable with
     flip='row'.  Elsewhere torch returns NaN / follows the arbitrary sign and nothing is compared.
ref_vs_f64_grad: the reference's own float32 noise, the largest |float32 gradient - float64 gradient| over the pairs of kind 1 as
a fraction of the graph's largest float64 gradient element.
Conditions (asserted, not measured): >= 40 pairs, >= 12 reflection cases among kind 1, >= 30 pairs of kind 1.
"""
import importlib
import os
import sys
import types

os.environ.setdefault("MKL_CBWR", "COMPATIBLE,STRICT")
import numpy as np  # noqa: E402
import torch  # noqa: E402

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import _rmsd_grad_util as GU  # noqa: E402
from tests import _rmsd_util as RU  # noqa: E402

torch.set_num_threads(8)

SIZES = [2, 3, 4, 5, 8, 17, 63, 64, 65, 130] * 4 + [4, 5, 8, 17, 33, 64, 65, 130]
NOISES = (0.01, 0.1, 0.5)


def main():
    sys.modules.setdefault("wandb", types.ModuleType("wandb"))
    sys.path.insert(0, REF)
    kabsch_torch = importlib.import_module("evaluate_rmsd_for_pos_generate").kabsch_torch
    rng = np.random.default_rng(20251)
    P_all, Q_all, rows = [], [], {k: [] for k in ("g_R", "g_t", "g_rmsd", "kind", "defined", "mirrored", "reflection", "noise")}
    grads = {k: [] for k in ("dP64", "dQ64", "dP32", "dQ32")}
    noise32 = 0.0
    for k, n in enumerate(SIZES):
        P = RU.silica_cloud(rng, n)
        mirrored = k % 3 == 2
        noise = NOISES[(k // 3) % 3]
        Q = P * np.array([1.0, 1.0, -1.0]) if mirrored else P.copy()
        Q = Q @ RU.random_rotation(rng).T + rng.uniform(-4, 4, 3) + noise * rng.standard_normal((n, 3))
        P32, Q32 = P.astype(np.float32), Q.astype(np.float32)
        sig = RU.sigma_f64(P32, Q32, "centroid")
        kind = int(n >= 4 and RU.well_conditioned(sig))
        # cotangents that float32 holds exactly: the device takes them as float32
        g_R, g_t, g_rmsd = (np.float64(np.float32(v)) for v in (rng.standard_normal((3, 3)), rng.standard_normal(3), rng.uniform(0.5, 1.5)))
        g_rmsd = float(g_rmsd)
        if not kind:
            g_R, g_t = np.zeros((3, 3)), np.zeros(3)
        dP64, dQ64 = GU.grads_autograd(kabsch_torch, P32, Q32, g_R, g_t, g_rmsd, torch.float64)
        dP32, dQ32 = GU.grads_autograd(kabsch_torch, P32, Q32, g_R, g_t, g_rmsd, torch.float32)
        defined = 1
        if kind:
            noise32 = max(noise32, GU.worst_ratio(dP32, dP64), GU.worst_ratio(dQ32, dQ64))
        else:
            with torch.no_grad():
                r_ref = float(kabsch_torch(torch.from_numpy(P32).double(), torch.from_numpy(Q32).double())[2])
            r_row = RU.kabsch_f64(P32, Q32, "centroid", "row")[2]
            defined = int(np.isfinite(dP64).all() and np.isfinite(dQ64).all() and abs(r_ref - r_row) <= 1e-12 * max(r_row, 1.0))
            if not defined:
                dP64, dQ64 = np.zeros((n, 3)), np.zeros((n, 3))
            dP32, dQ32 = np.zeros((n, 3)), np.zeros((n, 3))      # float32 is compared on kind 1 only
        P_all.append(P32)
        Q_all.append(Q32)
        for key, v in (("g_R", g_R), ("g_t", g_t), ("g_rmsd", g_rmsd), ("kind", kind), ("defined", defined), ("mirrored", int(mirrored)),
                       ("reflection", int(np.linalg.det(RU.covariance_f64(P32, Q32, "centroid")[3]) < 0.0)), ("noise", noise)):
            rows[key].append(v)
        for key, v in (("dP64", dP64), ("dQ64", dQ64), ("dP32", dP32), ("dQ32", dQ32)):
            grads[key].append(v)
    kind, refl = np.array(rows["kind"]), np.array(rows["reflection"])
    assert len(SIZES) >= 40 and int(kind.sum()) >= 30 and int((refl * kind).sum()) >= 12, (len(SIZES), kind.sum(), (refl * kind).sum())
    out = {"sizes": np.array(SIZES, dtype=np.int32), "P": np.concatenate(P_all), "Q": np.concatenate(Q_all),
           "g_R": np.stack(rows["g_R"]), "g_t": np.stack(rows["g_t"]), "g_rmsd": np.array(rows["g_rmsd"]),
           "kind": kind.astype(np.int32), "defined": np.array(rows["defined"], dtype=np.int32),
           "mirrored": np.array(rows["mirrored"], dtype=np.int32), "reflection": refl.astype(np.int32),
           "noise": np.array(rows["noise"]), "ref_vs_f64_grad": np.array(noise32)}
    for key, v in grads.items():
        out[key] = np.concatenate(v).astype(np.float64 if key.endswith("64") else np.float32)
    print(f"{len(SIZES)} pairs, {int(kind.sum())} well-conditioned with n >= 4 ({int((refl * kind).sum())} reflections), "
          f"{int((np.array(rows['defined']) * (1 - kind)).sum())} of the other {int((1 - kind).sum())} comparable through the RMSD; "
          f"ref_vs_f64_grad {noise32:.3e}")
    path = os.path.join(OUT, "rmsd_grad_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

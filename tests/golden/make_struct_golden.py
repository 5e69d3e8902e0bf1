#!/usr/bin/env python3
"""Generate tests/golden/struct_golden.npz by EXECUTING the reference's RDF and CN2 angle code in the build container (same method as
make_rmsd_golden.py; run only where the read-only reference tree exists):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_struct_golden.py

What is executed:
  * evaluate_RDF.py is imported as it is (its `import wandb` is satisfied by an EMPTY module object, as in make_golden.py):
    RDF (:48-60) with length_from_exO (:39-45).  The RDF of centre i is RDF(roll(position, i)): the graph rolled so that the centre
    comes first.  Per fixture graph and atom type a the MEAN over the centres of type a is stored, for (sigma=5, R=5, dR=0.01) and
    (sigma=3, R=4, dR=0.02), the two settings of stats_golden.npz.
  * CN2_evaluate.py cannot be imported here (it imports the training data set-up at module level), so the TEXT of
    calculate_angle_for_CN2 (:12-16) is read from the reference file at generation time and executed; for every bonded triplet
    (centre i, neighbours j < k within the cutoff 2.0) its angle is stored.  Nothing of the text is stored.
A case is kept only if (1) every ordered-pair distance, in both float32 spellings (the reference's torch.norm and the library's
fixed order), falls in the same bins and on the same side of the cutoff and lies more than 4 float32 ulp from every bin edge and
from the cutoff, and (2) no angle lies within 1e-9 degrees of an angle-bin edge (dtheta 1.0 and 2.5); otherwise it is redrawn.
Only inputs and outputs (arrays) are written.  No reference source is copied.
"""
import os
import sys
import textwrap
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import _rmsd_util as RU  # noqa: E402
from tests import _struct_util as SU  # noqa: E402

SETTINGS = ((5, 5.0, 0.01), (3, 4.0, 0.02))     # sigma, R, dR
CUTOFF = 2.0
DTHETAS = (1.0, 2.5)
CASES = ((2, 2), (3, 2), (7, 2), (20, 2), (64, 2), (65, 2), (20, 3))   # atoms, types


def load_reference():
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.modules.setdefault("wandb", types.ModuleType("wandb"))
    sys.path.insert(0, REF)
    import evaluate_RDF as ER
    with open(os.path.join(REF, "CN2_evaluate.py"), encoding="utf-8") as f:
        lines = f.read().splitlines()
    body = lines[11:16]                                   # :12-16
    assert body[0].startswith("def calculate_angle_for_CN2(") and "np.degrees" in body[-1]
    ns = {"np": np, "torch": torch}
    exec(textwrap.dedent("\n".join(body)), ns)
    return ER.RDF, ns["calculate_angle_for_CN2"]


def torch_norm_distances(pos):
    """d[i,j] = torch.norm(position[j] - position[i]), the spelling of length_from_exO, pair by pair"""
    p = torch.from_numpy(pos)
    n = len(pos)
    d = np.zeros((n, n), dtype=np.float32)
    for i in range(n):
        for j in range(n):
            if i != j:
                d[i, j] = torch.norm(p[j] - p[i]).item()
    return d


def acceptable(pos, tps):
    n = len(pos)
    off = ~np.eye(n, dtype=bool)
    mine, theirs = SU.distances(pos)[off], torch_norm_distances(pos)[off]
    radial = [(R, dR) for _, R, dR in SETTINGS]
    if not (SU.radial_gap_ok(mine, radial, CUTOFF) and SU.radial_gap_ok(theirs, radial, CUTOFF)):
        return False
    if not np.array_equal(mine < np.float32(CUTOFF), theirs < np.float32(CUTOFF)):
        return False
    for R, dR in radial:
        nb = SU.nbins_of(R, dR)
        if any(not np.array_equal(a, b) for a, b in zip(SU.radial_bins(mine, dR, nb), SU.radial_bins(theirs, dR, nb))):
            return False
    thetas = [r[3] for r in SU.bonded_angles(pos, tps, CUTOFF)[0]]
    return all(SU.angle_gap(thetas, dt) >= 1e-9 for dt in DTHETAS)


def main():
    RDF, angle_cn2 = load_reference()
    rng = np.random.default_rng(20261)
    out = {"sizes": np.array([c[0] for c in CASES], dtype=np.int32), "A": np.array([c[1] for c in CASES], dtype=np.int32),
           "settings": np.array(SETTINGS, dtype=np.float64), "cutoff": np.float64(CUTOFF), "dthetas": np.array(DTHETAS)}
    worst_angle = 0.0
    for g, (n, A) in enumerate(CASES):
        for attempt in range(200):
            pos = RU.silica_cloud(rng, n).astype(np.float32)
            tps = rng.integers(0, A, n).astype(np.int32)
            tps[:min(A, n)] = np.arange(min(A, n))         # every type present where the graph is large enough
            if acceptable(pos, tps):
                break
        else:
            raise SystemExit(f"no acceptable case of {n} atoms in 200 draws")
        print(f"graph {g}: {n} atoms, {A} types, accepted at draw {attempt + 1}", flush=True)
        out[f"g{g}.pos"], out[f"g{g}.types"] = pos, tps
        for s, (sigma, R, dR) in enumerate(SETTINGS):
            curves = np.zeros((A, SU.nbins_of(R, dR)))
            for a in range(A):
                centres = np.nonzero(tps == a)[0]
                rdfs = [np.asarray(RDF(torch.from_numpy(np.roll(pos, -int(i), axis=0).copy()), sigma, R, dR), dtype=np.float64)
                        for i in centres]
                if rdfs:
                    curves[a] = np.mean(rdfs, axis=0)
            out[f"g{g}.rdf{s}"] = curves
        rows = SU.bonded_angles(pos, tps, CUTOFF)[0]
        tri = np.array([r[:3] for r in rows], dtype=np.int32).reshape(-1, 3)
        ref = np.array([angle_cn2(torch.from_numpy(pos[[i, j, k]])) for i, j, k in tri], dtype=np.float64)
        if len(rows):
            worst_angle = max(worst_angle, float(np.abs(ref - np.array([r[3] for r in rows])).max()))
        out[f"g{g}.triplets"], out[f"g{g}.angles"] = tri, ref
        print(f"  {len(tri)} bonded triplets", flush=True)
    print(f"reference angle (float32) against the float64 restatement: worst {worst_angle:.3e} degrees")
    path = os.path.join(OUT, "struct_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

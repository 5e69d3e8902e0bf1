"""Writes tests/golden/sq_golden.npz: the truth of the reciprocal-space statistics at 50 digits (mpmath), from the same float32
positions / float64 lattices and fractional coordinates the library reads.  Run from the repository root:
    python tests/golden/make_sq_golden.py
Clusters: D_ab(q) at q = 0, 0.05, 1.5, 7.3, 25 of graphs of 1, 2, 3 and 65 atoms (one lacking a type), of a graph with a coincident
pair, and of 65 atoms with r_max = 5 and the Lorch window.  Cells: the 24-atom triclinic cell with displaced atoms and a two-atom
cubic cell at q_max = 6, dq = 0.25: rho_a per vector (the vectors themselves from the restatement, whose gap check guards them) and
the shell means of Re(rho_a rho_b*)."""
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import _sq_util as SU  # noqa: E402

mp.mp.dps = 50


def sinc(x):
    return mp.mpf(1) if x == 0 else mp.sin(x) / x


def debye_truth(pos, types, sizes, A, q, r_max, window):
    out = np.zeros((len(sizes), A, A, len(q)))
    lo = 0
    for g, n in enumerate(sizes):
        acc = [[[mp.mpf(0)] * len(q) for _ in range(A)] for _ in range(A)]
        for i in range(lo, lo + n):
            for j in range(lo, lo + n):
                if i == j:
                    continue
                d = [mp.mpf(float(pos[j, x])) - mp.mpf(float(pos[i, x])) for x in range(3)]
                r = mp.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
                if not r < r_max:
                    continue
                w = sinc(mp.pi * r / mp.mpf(r_max)) if window else mp.mpf(1)
                row = acc[int(types[i])][int(types[j])]
                for k, qk in enumerate(q):
                    row[k] = row[k] + w * sinc(mp.mpf(float(qk)) * r)
        for a in range(A):
            for b in range(A):
                out[g, a, b] = [float(v) for v in acc[a][b]]
        lo += n
    return out


def cell_truth(cell, q_max, dq):
    L = mp.matrix(cell["lattice"].tolist())
    Bm = 2 * mp.pi * (L ** -1).T
    hkl, ka, bins = SU.vectors_restated(cell["lattice"], q_max, dq)
    A, nbins = cell["A"], int(np.ceil(q_max / dq))
    k_true = np.zeros(len(hkl))
    rho = np.zeros((len(hkl), A), dtype=np.complex128)
    prod = [[[mp.mpf(0)] * nbins for _ in range(A)] for _ in range(A)]
    half = np.bincount(bins, minlength=nbins)
    f = [[mp.mpf(float(v)) for v in row] for row in cell["frac"]]
    for v, m in enumerate(hkl):
        kv = mp.matrix([[int(m[0]), int(m[1]), int(m[2])]]) * Bm
        k_true[v] = float(mp.sqrt(kv[0] ** 2 + kv[1] ** 2 + kv[2] ** 2))
        r = [mp.mpc(0)] * A
        for j, fj in enumerate(f):
            r[int(cell["types"][j])] += mp.expjpi(-2 * (int(m[0]) * fj[0] + int(m[1]) * fj[1] + int(m[2]) * fj[2]))
        for a in range(A):
            rho[v, a] = complex(r[a])
            for b in range(A):
                prod[a][b][bins[v]] += (r[a] * mp.conj(r[b])).real
    s = np.full((A, A, nbins), np.nan)
    for a in range(A):
        for b in range(A):
            for n in range(nbins):
                if half[n]:
                    s[a, b, n] = float(prod[a][b][n] / int(half[n]))
    assert np.max(np.abs(k_true - ka)) < 1e-13 * q_max
    return hkl, k_true, rho, s


def main():
    clusters, cells, par = SU.golden_inputs()
    out = dict(q=SU.Q_GOLDEN, q_max=par["q_max"], dq=par["dq"])
    for name, c in clusters.items():
        assert SU.debye_gap_ok(c["pos"], c["sizes"], c["r_max"]), name
        truth = debye_truth(c["pos"], c["types"], c["sizes"], 2, SU.Q_GOLDEN, c["r_max"], c["window"])
        mine = SU.debye_restated(c["pos"], c["types"], c["sizes"], 2, SU.Q_GOLDEN, c["r_max"], "lorch" if c["window"] else None)
        print(f"{name}: restatement vs truth {SU.debye_error(mine, truth, SU.n_types(c['types'], c['sizes'], 2)):.2e}")
        out.update({f"{name}_pos": c["pos"], f"{name}_types": c["types"], f"{name}_sizes": np.array(c["sizes"]),
                    f"{name}_r_max": c["r_max"], f"{name}_window": c["window"], f"{name}_debye": truth})
    for name, c in cells.items():
        assert SU.cell_gap_ok(c["lattice"], par["q_max"], par["dq"]), name
        hkl, k, rho, s = cell_truth(c, par["q_max"], par["dq"])
        mine = SU.rho_restated(c["frac"], c["types"], 2, hkl)
        print(f"{name}: {len(hkl)} vectors, restatement vs truth {SU.rho_error(mine, rho, np.bincount(c['types'], minlength=2)):.2e}")
        out.update({f"{name}_lattice": c["lattice"], f"{name}_frac": c["frac"], f"{name}_types": c["types"], f"{name}_hkl": hkl,
                    f"{name}_k": k, f"{name}_rho": rho, f"{name}_s": s})
    np.savez_compressed(SU.GOLDEN, **out)
    print("wrote", SU.GOLDEN, os.path.getsize(SU.GOLDEN), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/cell_boo_golden.npz: the bond-orientational order of the fixtures of tests/_cell_boo_util.py in mpmath at 50
digits, from the textbook definition in the COMPLEX basis -- Y_l^m by mpmath.spherharm and the Wigner 3j symbols by
sympy.physics.wigner.wigner_3j -- so that neither the real-basis recurrence of soap_solid_column nor the G tables of the package
take part.  Nothing of the package is imported and no library is executed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cell_boo_golden.py

Sites come from make_cell_soap_golden.exact_sites: exact rational arithmetic on the float64 inputs, which also asserts that no site
lies within 1e-9 (relative) of the cutoff.  Per atom i with kept sites (centre type, site type allowed by the fixture's select):
    q_lm(i) = mean Y_l^m(theta, phi),   q_l = sqrt(4 pi / (2l+1) sum_m |q_lm|^2),
    w_l = sum_{m1+m2+m3=0} (l l l; m1 m2 m3) q_lm1 q_lm2 q_lm3,   w^_l = w_l / (sum_m |q_lm|^2)^(3/2)   (0 where the sum is 0),
    qbar_lm(i) = (q_lm(i) + sum over kept sites q_lm(atom)) / (1 + n_i),
    s_ik = Re sum_m q_lm(i) conj(q_lm(k)) / (|q(i)| |q(k)|) at l = 6, n_solid = #(s_ik > 0.7).
It asserts that no s_ik lies within 1e-9 of the threshold, that the imaginary part of every w_l vanishes, and that on the displaced
fixtures every even-l q_l and qbar_l (l = 2 .. 10) of an atom with a kept site is at least 1e-3.  Stored, rounded to float64 only then.  Only arrays are written.
"""
import os
import sys

import mpmath as mp
import numpy as np
from sympy.physics.wigner import wigner_3j

OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
sys.path.insert(0, OUT)
from make_cell_soap_golden import exact_sites  # noqa: E402
from tests import _cell_boo_util as BU  # noqa: E402  (fixtures only)

mp.mp.dps = 50
L1 = BU.L_MAX + 1


def harmonics(r):
    """complex Y_l^m of the direction of r (fractions) -> {(l, m)}, m = -l .. l"""
    x, y, z = (mp.mpf(v.numerator) / v.denominator for v in r)
    theta, phi = mp.acos(z / mp.sqrt(x * x + y * y + z * z)), mp.atan2(y, x)
    out = {}
    for l in range(L1):
        for m in range(l + 1):
            v = mp.spherharm(l, m, theta, phi)
            out[l, m] = v
            out[l, -m] = (-1) ** m * mp.conj(v)
    return out


def three_j(l):
    """the non-zero (m1, m2, m3, value) of (l l l; m1 m2 m3), the values exact in sympy, then at 50 digits"""
    out = []
    for m1 in range(-l, l + 1):
        for m2 in range(-l, l + 1):
            if abs(m1 + m2) <= l:
                v = wigner_3j(l, l, l, m1, m2, -m1 - m2)
                if v != 0:
                    out.append((m1, m2, -m1 - m2, mp.mpf(v.evalf(60))))
    return out


def invariants(q, tj):
    """q: {(l, m)} -> (q_l, w_l, w^_l) lists"""
    ql, wl, wh = [], [], []
    for l in range(L1):
        s2 = mp.fsum(abs(q[l, m]) ** 2 for m in range(-l, l + 1))
        w = mp.fsum(v * q[l, a] * q[l, b] * q[l, c] for a, b, c, v in tj[l])
        assert abs(mp.im(w)) < mp.mpf(10) ** -40, "w_l is not real"
        w = mp.re(w)
        ql.append(mp.sqrt(4 * mp.pi / (2 * l + 1) * s2))
        wl.append(w)
        wh.append(w / s2 ** mp.mpf("1.5") if s2 != 0 else mp.mpf(0))
    return ql, wl, wh


def main():
    out, tj = {}, [three_j(l) for l in range(L1)]
    zero = {(l, m): mp.mpc(0) for l in range(L1) for m in range(-l, l + 1)}
    for name, (cutoff, per_a) in BU.FIXTURES.items():
        first = BU.fixture(name, next(iter(per_a)))
        natoms = len(first["frac"])
        found = [exact_sites(first, cutoff, i) for i in range(natoms)]      # [(key, atom, r)], ascending
        Y = [[harmonics(r) for _, _, r in rows] for rows in found]
        out[f"{name}_lattice"], out[f"{name}_frac"] = first["lattice"], first["frac"]
        print(name, "sites per centre", [len(rows) for rows in found], flush=True)
        for A, pairs in per_a.items():
            types = BU.fixture(name, A)["types"]
            mask = BU.select_mask(pairs, A)
            kept = [[k for k, (_, j, r) in enumerate(rows) if (mask >> (int(types[i]) * A + int(types[j]))) & 1 and any(v != 0 for v in r)]
                    for i, rows in enumerate(found)]
            q = [{key: mp.fsum(Y[i][k][key] for k in kept[i]) / len(kept[i]) for key in zero} if kept[i] else dict(zero) for i in range(natoms)]
            res = {k: [] for k in BU.FIELDS}
            n_solid = []
            for i in range(natoms):
                nb = [found[i][k][1] for k in kept[i]]
                bar = {key: (q[i][key] + mp.fsum(q[j][key] for j in nb)) / (1 + len(nb)) for key in zero}
                for keys, vals in ((BU.FIELDS[:3], invariants(q[i], tj)), (BU.FIELDS[3:], invariants(bar, tj))):
                    for key, v in zip(keys, vals):
                        res[key].append(v)
                l, count = BU.L_SOLID, 0
                ni = mp.sqrt(mp.fsum(abs(q[i][l, m]) ** 2 for m in range(-l, l + 1)))
                for j in nb:
                    nj = mp.sqrt(mp.fsum(abs(q[j][l, m]) ** 2 for m in range(-l, l + 1)))
                    s = mp.re(mp.fsum(q[i][l, m] * mp.conj(q[j][l, m]) for m in range(-l, l + 1))) / (ni * nj) if ni != 0 and nj != 0 else mp.mpf(0)
                    assert abs(s - mp.mpf(repr(BU.THRESHOLD))) > mp.mpf(10) ** -9, "a solid bond on the threshold"
                    count += s > mp.mpf(repr(BU.THRESHOLD))
                n_solid.append(count)
            arr = {k: np.array(v, dtype=object).astype(np.float64) for k, v in res.items()}
            if name in BU.DISPLACED:
                has = np.array([len(k) > 0 for k in kept])          # an atom without a kept site (O under the Si-Si select) has q = 0
                for k in ("q", "q_avg"):
                    assert float(arr[k][has][:, 2::2].min()) >= 1e-3, (name, k, float(arr[k][has][:, 2::2].min()))
            out[f"{name}_A{A}_types"] = types
            out[f"{name}_A{A}_n"] = np.array([len(k) for k in kept], dtype=np.int32)
            out[f"{name}_A{A}_n_solid"] = np.array(n_solid, dtype=np.int32)
            for k, v in arr.items():
                out[f"{name}_A{A}_{k}"] = v
            print(name, "A", A, "n", out[f"{name}_A{A}_n"], "n_solid", n_solid, "q6", arr["q"][:3, 6], flush=True)
    path = os.path.join(OUT, "cell_boo_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()

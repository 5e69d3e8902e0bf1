#!/usr/bin/env python3
"""Generate tests/golden/cell_soap_golden.npz: the SOAP power spectrum of atoms of periodic cells (the fixtures of
tests/_cell_soap_util.py) in pure mpmath at 60 digits, from the DEFINITION in csrc/cells/cell_soap_math.h and csrc/eval/soap_math.h.
Nothing of the package is imported and no library is executed; `Basis` is make_soap_golden.py's, so the tables and their asserts
(quadrature, harmonics, beta S beta^T = 1) are the same.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cell_soap_golden.py

The sites of a centre are enumerated over a box one image wider on every axis than floor(cut / w_k) + 1, with exact rational
arithmetic on the float64 inputs: w = f - floor(f), d = w_j - w_i + s, r = d L and |r|^2 < cut^2 as fractions.  The centre itself
enters at r = 0.  Stored, rounded to float64 only then: the descriptors, the coefficients for A = 2 (A = 1 for the one-atom cell) and
the site keys atom * 729 + code of every centre (ascending) with their row pointer.  It asserts the gap condition -- no site within
1e-9 (relative) of the cut: change THIN_SEED if it fails -- that no site leaves the stated box, and that the file stays below 1 MiB.
Only arrays are written.
"""
import itertools
import os
import sys
from fractions import Fraction

import mpmath as mp
import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
sys.path.insert(0, OUT)
from make_soap_golden import Basis, check_harmonics, check_quadrature  # noqa: E402
from tests import _cell_soap_util as CSU  # noqa: E402  (fixtures only)
from tests import _soap_util as SU  # noqa: E402

mp.mp.dps = 60


def exact_sites(cell, cut, centre):
    """-> [(key, atom, (rx, ry, rz) as fractions)] ascending by key, the centre left out; asserts the gap and the box"""
    L = [[Fraction(float(v)) for v in row] for row in np.asarray(cell["lattice"], dtype=np.float64)]
    f = [[Fraction(float(v)) for v in row] for row in np.asarray(cell["frac"], dtype=np.float64)]
    w = [[v - (v.numerator // v.denominator) for v in row] for row in f]
    b = CSU.box(cell["lattice"], cut)
    c2 = Fraction(float(cut)) ** 2
    out = []
    for j in range(len(w)):
        for s in itertools.product(*(range(-int(k) - 1, int(k) + 2) for k in b)):
            if j == centre and s == (0, 0, 0):
                continue
            d = [w[j][k] - w[centre][k] + s[k] for k in range(3)]
            r = tuple(d[0] * L[0][x] + d[1] * L[1][x] + d[2] * L[2][x] for x in range(3))
            r2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
            assert abs(float(mp.sqrt(mp.mpf(r2.numerator) / r2.denominator)) - cut) > 1e-9 * cut, "a site on the cut: change the seed"
            if r2 < c2:
                assert all(abs(s[k]) <= int(b[k]) for k in range(3)), "a site outside the stated box"
                out.append((j * 729 + ((s[0] + 4) * 9 + (s[1] + 4)) * 9 + (s[2] + 4), j, r))
    return sorted(out)


def truth(basis, types, A, rows):
    """rows: per centre (its atom, its exact sites) -> (desc, coeff) as float64 arrays"""
    n_max, l_max = basis.n_max, basis.l_max
    LM = (l_max + 1) ** 2
    l_of = [l for l in range(l_max + 1) for _ in range(2 * l + 1)]
    z1, z2, n1, n2, ll = SU.feature_index(A, n_max, l_max)
    desc, coeff = [], []
    for centre, found in rows:
        prim = [[[mp.mpf(0)] * LM for _ in range(n_max)] for _ in range(A)]
        for j, r in [(centre, (Fraction(0),) * 3)] + [(j, r) for _, j, r in found]:
            x, y, z = (mp.mpf(v.numerator) / v.denominator for v in r)
            R, rad = basis.solid(x, y, z), basis.radial(x * x + y * y + z * z)
            for n in range(n_max):
                row = prim[types[j]][n]
                for lm in range(LM):
                    row[lm] += rad[n][l_of[lm]] * R[lm]
        c = [[[mp.fsum(basis.beta[l_of[lm]][n, q] * prim[z][q][lm] for q in range(n_max)) for lm in range(LM)] for n in range(n_max)]
             for z in range(A)]
        coeff.append(c)
        desc.append([basis.weight[ll[f]] * mp.fsum(c[z1[f]][n1[f]][ll[f] ** 2 + m] * c[z2[f]][n2[f]][ll[f] ** 2 + m]
                                                   for m in range(2 * ll[f] + 1)) for f in range(len(ll))])
    tofloat = lambda a: np.array(a, dtype=object).astype(np.float64)
    return tofloat(desc), tofloat(coeff)


def main():
    out, bases = {}, {}
    for name, (cfg, As, _) in CSU.FIXTURES.items():
        if cfg not in bases:
            bases[cfg] = Basis(**SU.CONFIGS[cfg])
            check_quadrature(bases[cfg])
            check_harmonics(bases[cfg])
        basis, cut = bases[cfg], CSU.cut_of(name)
        cell = CSU.fixture(name, As[0])
        centres = CSU.centres_of(name, cell)
        rows = [(int(i), exact_sites(cell, cut, int(i))) for i in centres]
        out[f"{name}_lattice"], out[f"{name}_frac"], out[f"{name}_centres"] = cell["lattice"], cell["frac"], centres
        out[f"{name}_keys"] = np.array([k for _, found in rows for k, _, _ in found], dtype=np.int64)
        out[f"{name}_row_ptr"] = np.concatenate([[0], np.cumsum([len(found) for _, found in rows])]).astype(np.int64)
        print(name, "box", CSU.box(cell["lattice"], cut), "sites per centre", np.diff(out[f"{name}_row_ptr"]))
        for A in As:
            types = CSU.fixture(name, A)["types"]
            desc, coeff = truth(basis, types, A, rows)
            out[f"{name}_A{A}_types"], out[f"{name}_A{A}_desc"] = types, desc
            if A == max(a for a in As if a <= 2):
                out[f"{name}_A{A}_coeff"] = coeff
            print(name, "A", A, desc.shape, float(np.abs(desc).max()))
    path = os.path.join(OUT, "cell_soap_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()

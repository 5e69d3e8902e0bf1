#!/usr/bin/env python3
"""Generate tests/golden/soap_golden.npz: the SOAP power spectrum of the fixture graphs (tests/_soap_util.py) in pure mpmath at 60
digits, from the DEFINITION in csrc/eval/soap_math.h.  Nothing of the package is imported and no library is executed: there is no
reference implementation on hand (dscribe is not installed, and its own numbers depend on a float64 matrix root of an overlap
matrix of condition number 4e15), so the truth is the mathematics.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_soap_golden.py

What is computed, all in mpmath and rounded to float64 only when stored:
  * the tables K, gamma, beta = S^(-1/2) (symmetric eigenproblem at 60 digits), the harmonic norms N and the weights w;
  * for every centre the primitive coefficients (closed form), the orthonormalised coefficients with the UNROUNDED beta, the
    power spectrum, and the cosine of every descriptor row with the next one (cyclically); the coefficients are stored for A = 2;
  * the default configuration on the three smallest graphs (atom 0 of each), the small configuration (r_cut=4, n_max=3, l_max=2)
    on all of them (every atom), for A = 1, 2, 3 atom types.
Before anything is written it asserts
  * that primitive radial coefficients K_nl exp(-gamma_nl d^2) d^l equal mpmath.quad integrals of the defining expression
    4 pi r^2 phi_nl(r) exp(-a (r^2 + d^2)) i_l(2 a d r) to 1e-25 relative, on cases of magnitude above 1e-100;
  * that the real solid harmonics of the recurrence equal d^l times mpmath.spherharm combined to real form, to 1e-45;
  * that beta S beta^T = 1 to 1e-25 for every l.
Only arrays are written.
"""
import os
import sys

import mpmath as mp
import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import _soap_util as SU  # noqa: E402  (fixtures only)

mp.mp.dps = 60
QUAD_CASES = ((0, "3.1", 5), (3, "4.7", 8), (10, "8.3", 14), (10, "3.1", 7), (5, "6.2", 12), (1, "7.5", 13))   # l, d, n


class Basis:
    def __init__(self, r_cut, n_max, l_max, sigma):
        self.n_max, self.l_max, L1 = n_max, l_max, l_max + 1
        self.a = 1 / (2 * mp.mpf(repr(sigma)) ** 2)
        rc = mp.mpf(repr(r_cut))
        r = [1 + (rc - 1) * k / (n_max - 1) for k in range(n_max)] if n_max > 1 else [mp.mpf(1)]
        self.alpha = [[-mp.log(mp.mpf("1e-3") / rn ** l) / rn ** 2 for l in range(L1)] for rn in r]
        self.K = [[mp.pi ** mp.mpf("1.5") * (self.alpha[n][l] + self.a) ** mp.mpf("-1.5") * (self.a / (self.alpha[n][l] + self.a)) ** l
                   for l in range(L1)] for n in range(n_max)]
        self.gamma = [[self.a * self.alpha[n][l] / (self.alpha[n][l] + self.a) for l in range(L1)] for n in range(n_max)]
        self.beta = []
        for l in range(L1):
            e = l + mp.mpf("1.5")
            S = mp.matrix(n_max, n_max)
            for n in range(n_max):
                for q in range(n_max):
                    S[n, q] = mp.gamma(e) / 2 * (self.alpha[n][l] + self.alpha[q][l]) ** (-e)
            lam, V = mp.eigsy(S)
            b = V * mp.diag([1 / mp.sqrt(x) for x in lam]) * V.T
            resid = b * S * b.T - mp.eye(n_max)
            assert max(abs(x) for x in resid) < mp.mpf("1e-25"), (l, max(abs(x) for x in resid))
            self.beta.append(b)
        self.norm = [None] * (L1 * L1)
        for l in range(L1):
            for m in range(-l, l + 1):
                v = mp.sqrt((2 * l + 1) / (4 * mp.pi) * mp.factorial(l - abs(m)) / mp.factorial(l + abs(m)))
                self.norm[l * l + l + m] = v * mp.sqrt(2) if m else v
        self.weight = [mp.pi * mp.sqrt(mp.mpf(8) / (2 * l + 1)) for l in range(L1)]

    def arrays(self):
        f = lambda rows: np.array([[float(x) for x in row] for row in rows])
        beta = np.array([[[float(b[n, q]) for q in range(self.n_max)] for n in range(self.n_max)] for b in self.beta])
        return dict(K=f(self.K), gamma=f(self.gamma), beta=beta, norm=np.array([float(x) for x in self.norm]),
                    weight=np.array([float(x) for x in self.weight]))

    def solid(self, x, y, z):
        """R_lm by the recurrence stated in soap_math.h, in mpmath"""
        l_max = self.l_max
        r2 = x * x + y * y + z * z
        out = [mp.mpf(0)] * ((l_max + 1) ** 2)
        ca, sa, pmm = mp.mpf(1), mp.mpf(0), mp.mpf(1)
        for m in range(l_max + 1):
            if m:
                ca, sa = ca * x - sa * y, ca * y + sa * x
                pmm *= 2 * m - 1
            p2, p1 = mp.mpf(0), pmm
            for l in range(m, l_max + 1):
                if l > m:
                    p2, p1 = p1, ((2 * l - 1) * z * p1 - (l + m - 1) * r2 * p2) / (l - m)
                out[l * l + l + m] = self.norm[l * l + l + m] * p1 * ca
                if m:
                    out[l * l + l - m] = self.norm[l * l + l - m] * p1 * sa
        return out

    def radial(self, d2):
        return [[self.K[n][l] * mp.exp(-self.gamma[n][l] * d2) for l in range(self.l_max + 1)] for n in range(self.n_max)]


def check_quadrature(basis):
    for l, d, n in QUAD_CASES:
        if l > basis.l_max or n >= basis.n_max:
            continue
        d, a, al = mp.mpf(d), basis.a, basis.alpha[n][l]
        closed = basis.K[n][l] * mp.exp(-basis.gamma[n][l] * d * d) * d ** l
        assert abs(closed) > mp.mpf("1e-100"), (l, d, n, closed)
        il = lambda x: mp.sqrt(mp.pi / (2 * x)) * mp.besseli(l + mp.mpf("0.5"), x)
        f = lambda r: 4 * mp.pi * r * r * r ** l * mp.exp(-al * r * r) * mp.exp(-a * (r * r + d * d)) * il(2 * a * d * r)
        peak = a * d / (a + al)
        cuts = sorted({mp.mpf(0), max(peak - 1, mp.mpf("0.01")), max(peak - mp.mpf("0.3"), mp.mpf("0.02")), peak, peak + mp.mpf("0.3"),
                       peak + 1, peak + 4})
        with mp.workdps(80):
            num = mp.quad(f, cuts, maxdegree=10)
        rel = abs(num / closed - 1)
        print(f"quadrature l={l} d={d} n={n}: closed form {mp.nstr(closed, 8)}, relative difference {mp.nstr(rel, 3)}")
        assert rel < mp.mpf("1e-25"), (l, d, n, rel)


def check_harmonics(basis):
    rng = np.random.default_rng(5)
    for _ in range(3):
        x, y, z = (mp.mpf(float(v)) for v in rng.uniform(-3, 3, 3))
        d = mp.sqrt(x * x + y * y + z * z)
        theta, phi = mp.acos(z / d), mp.atan2(y, x)
        got = basis.solid(x, y, z)
        for l in range(basis.l_max + 1):
            for m in range(-l, l + 1):
                Y = mp.spherharm(l, abs(m), theta, phi)
                want = Y.real if m == 0 else mp.sqrt(2) * (-1) ** m * (Y.real if m > 0 else Y.imag)
                assert abs(got[l * l + l + m] - d ** l * want) < mp.mpf("1e-45") * d ** l, (l, m)


def truth(basis, pos, types, sizes, A, centres, cut, cache):
    n_max, l_max = basis.n_max, basis.l_max
    LM = (l_max + 1) ** 2
    l_of = [l for l in range(l_max + 1) for _ in range(2 * l + 1)]
    gp = SU.graph_ptr(sizes)
    z1, z2, n1, n2, ll = SU.feature_index(A, n_max, l_max)
    p = [[mp.mpf(float(v)) for v in row] for row in pos]          # the float32 values, exactly
    desc, coeff = [], []
    for i in centres:
        g = int(np.searchsorted(gp, i, side="right")) - 1
        prim = [[[mp.mpf(0)] * LM for _ in range(n_max)] for _ in range(A)]
        for j in range(gp[g], gp[g + 1]):
            if (i, j) not in cache:
                dx, dy, dz = (p[j][k] - p[i][k] for k in range(3))
                d2 = dx * dx + dy * dy + dz * dz
                cache[(i, j)] = (basis.solid(dx, dy, dz), basis.radial(d2)) if d2 < cut * cut else None
            if cache[(i, j)] is None:
                continue
            R, rad = cache[(i, j)]
            for n in range(n_max):
                row = prim[types[j]][n]
                for lm in range(LM):
                    row[lm] += rad[n][l_of[lm]] * R[lm]
        c = [[[mp.fsum(basis.beta[l_of[lm]][n, q] * prim[z][q][lm] for q in range(n_max)) for lm in range(LM)] for n in range(n_max)]
             for z in range(A)]
        coeff.append(c)
        desc.append([basis.weight[ll[f]] * mp.fsum(c[z1[f]][n1[f]][ll[f] ** 2 + m] * c[z2[f]][n2[f]][ll[f] ** 2 + m]
                                                   for m in range(2 * ll[f] + 1)) for f in range(len(ll))])
    dot = lambda u, v: mp.fsum(x * y for x, y in zip(u, v))
    cos = [dot(desc[k], desc[(k + 1) % len(desc)]) / mp.sqrt(dot(desc[k], desc[k]) * dot(desc[(k + 1) % len(desc)], desc[(k + 1) % len(desc)]))
           for k in range(len(desc))]
    tofloat = lambda a: np.array(a, dtype=object).astype(np.float64)
    return tofloat(desc), tofloat(coeff), tofloat(cos)


def main():
    out = {}
    for name, cfg in SU.CONFIGS.items():
        basis = Basis(**cfg)
        check_quadrature(basis)
        check_harmonics(basis)
        for k, v in basis.arrays().items():
            out[f"{name}_{k}"] = v
        cut = mp.mpf(float(SU.neighbour_cut(cfg)))
        cache = {}
        for A in SU.TYPES:
            pos, types, sizes = SU.fixture(A, SU.GOLDEN_GRAPHS[name])
            assert SU.gap_ok(pos, sizes, SU.neighbour_cut(cfg)), "a pair distance on the neighbour cut: change POSITION_SEED"
            centres = SU.first_centres(sizes) if name == "default" else np.arange(len(types), dtype=np.int32)
            desc, coeff, cos = truth(basis, pos, types, sizes, A, centres, cut, cache)
            out[f"{name}_A{A}_pos"], out[f"{name}_A{A}_types"], out[f"{name}_A{A}_centres"] = pos, types, centres.astype(np.int32)
            out[f"{name}_A{A}_desc"], out[f"{name}_A{A}_cos"] = desc, cos
            if A == 2:                                            # the coefficients of one A only: the file has a size limit
                out[f"{name}_A{A}_coeff"] = coeff
            print(name, "A", A, desc.shape, coeff.shape, float(np.abs(desc).max()))
    path = os.path.join(OUT, "soap_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()

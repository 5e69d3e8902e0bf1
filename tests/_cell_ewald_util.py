"""The lattice energy of periodic cells (csrc/cells/cell_ewald_math.h) for the CPU and GPU tests (test infrastructure): the cases,
a numpy restatement in fp64, the same truncated sums in mpmath at 50 digits (the truth), the ctypes wrapper of the host statement
egnn_cell_ewald_host and the error metric.

  * case: a cell dict (lattice, frac, types, A) with charges per type, the pair tables pot [4, A, A] or None, n, r_cut, short_cut,
    shift, alpha, k_max, kappa; ``make_case`` fills alpha and k_max from ``accuracy`` as ``cells.lattice_energy`` does;
  * restatement (``restated``): sites by tests/_cell_soap_util.sites (the box walk without a cull, ascending (atom, shift code), fp64
    vectors in the library's operation order), vectors by tests/_sq_util.box_candidates, plain Python loops, every sum ascending;
  * truth (``exact``): the wrapped fp64 coordinates, lattice and parameters taken as exact numbers, membership by comparison at 50
    digits with the gap to every cutoff recorded, the sums of cell_ewald_math.h term by term, and per atom the sum of the absolute
    values of the elementary terms of its energy and of each force component (the error scale: real and short terms per site,
    reciprocal terms per product of a (vector, atom) pair, |cos cos| + |sin sin| and |sin cos| + |cos sin|, self and background);
  * error: E = max over atoms and outputs of |got - truth| / scale, the cell sums against the sum of their atoms' scales;
  * fixtures: tests/golden/cell_ewald_golden.npz holds ``exact`` of the five fixtures (make_cell_ewald_golden.py).
"""
import functools
import math
import os

import numpy as np

from tests import _cell_grid_util as GU
from tests import _cell_soap_util as CSU
from tests import _cell_stats_util as STU
from tests import _cells_util as CU
from tests import _soap_util as SU
from tests import _sq_util as SQU

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cell_ewald_golden.npz")
KAPPA = 14.3996454784
CAP = 1e-12           # E_host must stay below it (a condition, not a measurement)
GAP = 1e-9            # no site or vector of a fixture lies this close (relative) to a cutoff
COMPONENTS = ("real", "reciprocal", "self", "background", "short")
BKS_CHARGES = (-1.2, 2.4)
TWO_OVER_SQRT_PI, ONE_OVER_SQRT_PI, FOUR_PI, EIGHT_PI = 1.1283791670955126, 0.5641895835477563, 12.566370614359172, 25.132741228718345
vp = SU.vp


def bks_tables():
    pot = np.zeros((4, 2, 2))
    pot[0] = [[1388.7730, 18003.7572], [18003.7572, 0.0]]
    pot[1] = [[2.76000, 4.87318], [4.87318, 0.0]]
    pot[2] = [[175.0000, 133.5381], [133.5381, 0.0]]
    return pot


def make_case(cell, charges, pot=None, n=24, r_cut=10.0, short_cut=None, shift=True, accuracy=1e-8, alpha=None, k_max=None, kappa=KAPPA):
    root = math.sqrt(-math.log(accuracy))
    alpha = root / r_cut if alpha is None else float(alpha)
    k_max = 2.0 * alpha * root if k_max is None else float(k_max)
    return dict(cell=cell, charges=np.asarray(charges, dtype=np.float64), pot=None if pot is None else np.ascontiguousarray(pot, dtype=np.float64),
                n=int(n), r_cut=float(r_cut), short_cut=float(r_cut if short_cut is None else short_cut), shift=bool(shift), alpha=alpha,
                k_max=k_max, kappa=float(kappa))


def cube_cell(a=3.0, frac=((0.3, 0.6, 0.9),)):
    f = np.asarray(frac, dtype=np.float64).reshape(-1, 3)
    return dict(lattice=a * np.eye(3), frac=f, types=np.zeros(len(f), np.int32), A=1, name="cube")


def nacl_cell(a=5.64):
    na = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]], dtype=np.float64)
    return dict(lattice=a * np.eye(3), frac=np.concatenate([na, na + [.5, .5, .5]]) + 0.013, types=np.repeat([0, 1], 4).astype(np.int32), A=2,
                name="nacl")


def cscl_cell(a=4.11):
    return dict(lattice=a * np.eye(3), frac=np.array([[0.1, 0.2, 0.3], [0.6, 0.7, 0.8]]), types=np.array([0, 1], np.int32), A=2, name="cscl")


def generic_tables(A, seed):
    """symmetric Buckingham tables with a D / r^n term for the dense random fixtures: soft enough to stay finite at 0.2 A"""
    rng = np.random.default_rng(seed)
    sym = lambda lo, hi: (lambda m: np.triu(m) + np.triu(m, 1).T)(rng.uniform(lo, hi, (A, A)))
    return np.stack([sym(100.0, 900.0), sym(1.5, 3.5), sym(1.0, 20.0), sym(0.01, 0.2)])


@functools.lru_cache(maxsize=None)
def fixtures():
    """name -> case: the five fixtures of the truth"""
    return {
        "thin": make_case(CSU.fixture("thin", 2), (-1.1, 2.3), generic_tables(2, 1), n=12, r_cut=4.37, short_cut=3.0, accuracy=1e-6),
        "crist": make_case(GU.displaced_cristobalite(1), BKS_CHARGES, bks_tables(), n=24, r_cut=8.2, short_cut=5.5, accuracy=1e-8),
        "one": make_case(cube_cell(), (1.0,), None, r_cut=7.3, accuracy=1e-8),
        "nacl": make_case(nacl_cell(), (1.0, -1.0), None, r_cut=6.0, accuracy=1e-8, kappa=1.0),
        "zero3": make_case(CSU.fixture("thin", 3), (-0.9, 1.7, 0.0), generic_tables(3, 2), n=9, r_cut=3.9, short_cut=3.9, shift=False, accuracy=1e-5),
    }


def _norm2(r):
    return (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]


def volume(L):
    a, b, c = np.asarray(L, dtype=np.float64).reshape(3, 3)
    bc = np.array([b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]])
    return abs((a[0] * bc[0] + a[1] * bc[1]) + a[2] * bc[2])


def vectors(case):
    """-> (hkl int64 [K, 3] ascending, k float64 [K, 3], k2 [K]) in the library's operation order; none where every charge is 0"""
    L = case["cell"]["lattice"]
    hkl, k2 = SQU.box_candidates(L, case["k_max"])
    m = SQU.half_space(hkl) & (k2 < case["k_max"] * case["k_max"])
    if not np.any(case["charges"] != 0.0):
        m[:] = False
    Bm, f = SQU.reciprocal(L), hkl[m].astype(np.float64)
    kv = np.stack([(f[:, 0] * Bm[0, x] + f[:, 1] * Bm[1, x]) + f[:, 2] * Bm[2, x] for x in range(3)], 1)
    return hkl[m], kv, k2[m]


def ipow(r, n):
    p, s, first = 1.0, r, True
    while n > 0:
        if n & 1:
            p, first = (s if first else p * s), False
        s, n = s * s, n >> 1
    return p


def pair(case, ab, r2, r):
    A_, b_, C_, D_ = (case["pot"][t].reshape(-1)[ab] for t in range(4))
    ex, r6 = math.exp(-(b_ * r)), (r2 * r2) * r2
    u, du = A_ * ex - C_ / r6, (-(A_ * b_)) * ex + (6.0 * C_) / (r6 * r)
    if D_ != 0.0:
        rn = ipow(r, case["n"])
        u, du = u + D_ / rn, du - (float(case["n"]) * D_) / (rn * r)
    return u, du


def u_cut(case):
    A = case["cell"]["A"]
    if case["pot"] is None or not case["shift"]:
        return np.zeros(A * A)
    return np.array([pair(case, ab, case["short_cut"] * case["short_cut"], case["short_cut"])[0] for ab in range(A * A)])


# ---- restatement in fp64 ----------------------------------------------------------------------------------------------------------------
def restated(case):
    cell, q_t, A = case["cell"], case["charges"], case["cell"]["A"]
    L, t, w = np.asarray(cell["lattice"], np.float64), np.asarray(cell["types"]), CU.wrap(cell["frac"])
    N, V, al, kap, uc = len(t), volume(cell["lattice"]), case["alpha"], case["kappa"], u_cut(case)
    hkl, kv, k2 = vectors(case)
    f = hkl.astype(np.float64)
    phase = lambda wi: [(lambda x: x - math.floor(x))((f[v, 0] * wi[0] + f[v, 1] * wi[1]) + f[v, 2] * wi[2]) for v in range(len(hkl))]
    g = [math.exp(-(k2[v] / ((4.0 * al) * al))) / k2[v] for v in range(len(hkl))]
    sc, ss = np.zeros(len(hkl)), np.zeros(len(hkl))
    for j in range(N):
        for v, ph in enumerate(phase(w[j])):
            sc[v] += q_t[t[j]] * math.cos(SQU.TWO_PI * ph)
            ss[v] += q_t[t[j]] * math.sin(SQU.TWO_PI * ph)
    Q = 0.0
    for a in range(A):
        Q += float(np.sum(t == a)) * q_t[a]
    out = dict(n_sites=np.zeros(N, np.int32), rows=[], hkl=hkl.astype(np.int32), comp_atom=np.zeros((N, 5)), e_atom=np.zeros(N), force=np.zeros((N, 3)),
               coincident=0)
    for i in range(N):
        j, code, r = CSU.sites(cell, case["r_cut"], i)
        out["n_sites"][i] = len(j)
        out["rows"].append((j, code))
        qi, er, es, F = q_t[t[i]], 0.0, 0.0, np.zeros(3)
        for a, d in zip(j, r):
            r2 = float(_norm2(d))
            if r2 == 0.0:
                out["coincident"] = 1
                continue
            rr = math.sqrt(r2)
            ar = al * rr
            ec, qj = math.erfc(ar) / rr, q_t[t[a]]
            er += qj * ec
            fs = (-(kap * qi)) * ((qj * (ec + (TWO_OVER_SQRT_PI * al) * math.exp(-(ar * ar)))) / r2)
            if case["pot"] is not None and rr < case["short_cut"]:
                ab = int(t[i]) * A + int(t[a])
                u, du = pair(case, ab, r2, rr)
                es += u - uc[ab]
                fs = fs + du / rr
            F += fs * d
        rec, R = 0.0, np.zeros(3)
        for v, ph in enumerate(phase(w[i])):
            sn, cs = math.sin(SQU.TWO_PI * ph), math.cos(SQU.TWO_PI * ph)
            gc, gs = g[v] * sc[v], g[v] * ss[v]
            rec += cs * gc + sn * gs
            R += kv[v] * (sn * gc - cs * gs)
        comp = [((0.5 * kap) * qi) * er, (((FOUR_PI * kap) / V) * qi) * rec, -(((kap * al) * (qi * qi)) * ONE_OVER_SQRT_PI),
                -((((kap * math.pi) * qi) * Q) / ((2.0 * (al * al)) * V)), 0.5 * es]
        out["comp_atom"][i] = comp
        out["e_atom"][i] = (((comp[0] + comp[1]) + comp[2]) + comp[3]) + comp[4]
        out["force"][i] = F + (((EIGHT_PI * kap) / V) * qi) * R
    out["components"] = np.array([functools.reduce(lambda s, x: s + x, out["comp_atom"][:, k], 0.0) for k in range(5)])
    out["energy"] = functools.reduce(lambda s, x: s + x, out["e_atom"], 0.0)
    return out


# ---- the truth: the same truncated sums at 50 digits --------------------------------------------------------------------------------------
def exact(case, derivative=False, wider=1):
    """-> dict of float64 arrays (rounded once from 50 digits): rows (row_ptr, atom, code), hkl, comp_atom, e_atom, force, scale_e [N],
    scale_f [N, 3], components, energy, gap (the smallest relative distance of a site or vector to a cutoff) and, with ``derivative``,
    deriv_error: the largest |analytic force + dE/dx| / scale_f over atoms and axes, dE/dx by mpmath's numerical derivative of the
    energy with the membership held.  The sites are sought in a box ``wider`` than the library's (which is complete already)."""
    import mpmath as mp
    mp.mp.dps = 50
    cell, A = case["cell"], case["cell"]["A"]
    t = np.asarray(cell["types"])
    N = len(t)
    X = lambda v: mp.mpf(float(v))
    Lm = mp.matrix([[X(v) for v in row] for row in np.asarray(cell["lattice"], np.float64)])
    w64 = CU.wrap(cell["frac"])
    wm = [[X(v) for v in row] for row in w64]
    q = [X(case["charges"][a]) for a in range(A)]
    kap, al, rc, sc_, km = X(case["kappa"]), X(case["alpha"]), X(case["r_cut"]), X(case["short_cut"]), X(case["k_max"])
    pot = None if case["pot"] is None else [[X(v) for v in case["pot"][k].reshape(-1)] for k in range(4)]
    n = case["n"]

    def u_of(ab, r):
        u = pot[0][ab] * mp.exp(-pot[1][ab] * r) - pot[2][ab] / r ** 6 + pot[3][ab] / r ** n
        du = -pot[0][ab] * pot[1][ab] * mp.exp(-pot[1][ab] * r) + 6 * pot[2][ab] / r ** 7 - n * pot[3][ab] / r ** (n + 1)
        return u, du
    ucut = [u_of(ab, sc_)[0] if (pot is not None and case["shift"]) else mp.mpf(0) for ab in range(A * A)]
    det = mp.det(Lm)
    V = abs(det)
    gap = [mp.mpf(1)]
    # sites: candidates by fp64 over a box one wider than the library's, membership at 50 digits
    Lf = np.asarray(cell["lattice"], np.float64)
    shifts = CSU.box_shifts(CSU.box(Lf, case["r_cut"]) + wider)
    rows = []
    for i in range(N):
        rf = CU.site_vectors(w64[:, None, :], w64[i], shifts[None, :, :], Lf)
        near = np.sqrt(_norm2(rf)) < case["r_cut"] * (1 + 1e-6)
        row = []
        for j, s in zip(*np.nonzero(near)):
            if j == i and not shifts[s].any():
                continue
            dfrac = [wm[j][k] - wm[i][k] + int(shifts[s][k]) for k in range(3)]
            d = [sum(dfrac[k] * Lm[k, x] for k in range(3)) for x in range(3)]
            r = mp.sqrt(sum(v * v for v in d))
            gap.append(abs(r / rc - 1))
            if pot is not None:
                gap.append(abs(r / sc_ - 1))
            if r < rc:
                row.append((int(j), int(CU.shift_code(shifts[s])), d, r))
        rows.append(row)
    # vectors
    charged = bool(np.any(case["charges"] != 0.0))
    hkl_c, k2_c = SQU.box_candidates(Lf, case["k_max"], extra=2)
    cand = hkl_c[SQU.half_space(hkl_c) & (np.sqrt(k2_c) < case["k_max"] * (1 + 1e-6))] if charged else np.zeros((0, 3), np.int64)
    Li = Lm ** -1          # columns of 2 pi L^-1 are the reciprocal rows
    vec = []
    for h, k, l in cand:
        kv = [2 * mp.pi * (int(h) * Li[x, 0] + int(k) * Li[x, 1] + int(l) * Li[x, 2]) for x in range(3)]
        kk = mp.sqrt(sum(v * v for v in kv))
        gap.append(abs(kk / km - 1))
        if kk < km:
            vec.append(((int(h), int(k), int(l)), kv, mp.exp(-kk * kk / (4 * al * al)) / (kk * kk)))
    phi = [[2 * mp.pi * (m[0] * wm[i][0] + m[1] * wm[i][1] + m[2] * wm[i][2]) for m, _, _ in vec] for i in range(N)]
    cs = [[mp.cos(p) for p in phi[i]] for i in range(N)]
    sn = [[mp.sin(p) for p in phi[i]] for i in range(N)]
    Sc = [sum(q[t[j]] * cs[j][v] for j in range(N)) for v in range(len(vec))]
    Ss = [sum(q[t[j]] * sn[j][v] for j in range(N)) for v in range(len(vec))]
    Q = sum(q[t[j]] for j in range(N))
    ph64 = np.array([[float(p) for p in phi[i]] for i in range(N)], dtype=np.float64).reshape(N, len(vec))
    g64, k64 = np.array([float(g) for _, _, g in vec]), np.array([[float(v) for v in kv] for _, kv, _ in vec]).reshape(len(vec), 3)
    aq64 = np.abs(case["charges"][t])
    comp, force, scale_e, scale_f = [], [], [], []
    pair_f = lambda ti, tj, r: (-kap * q[ti] * q[tj] * (mp.erfc(al * r) / r + 2 * al / mp.sqrt(mp.pi) * mp.exp(-al * al * r * r)) / (r * r),
                                (u_of(ti * A + tj, r)[1] / r) if (pot is not None and r < sc_) else mp.mpf(0))
    for i in range(N):
        ti, qi = int(t[i]), q[int(t[i])]
        e_r = e_s = mp.mpf(0)
        F, se, sf = [mp.mpf(0)] * 3, mp.mpf(0), [mp.mpf(0)] * 3
        for j, _, d, r in rows[i]:
            tj = int(t[j])
            a = kap * qi * q[tj] * mp.erfc(al * r) / r / 2
            b = (u_of(ti * A + tj, r)[0] - ucut[ti * A + tj]) / 2 if (pot is not None and r < sc_) else mp.mpf(0)
            e_r, e_s, se = e_r + a, e_s + b, se + abs(a) + abs(b)
            fr, fs = pair_f(ti, tj, r)
            F = [F[x] + (fr + fs) * d[x] for x in range(3)]
            sf = [sf[x] + (abs(fr) + abs(fs)) * abs(d[x]) for x in range(3)]
        pre = 4 * mp.pi * kap / V * qi
        e_k = pre * sum(g * (cs[i][v] * Sc[v] + sn[i][v] * Ss[v]) for v, (_, _, g) in enumerate(vec))
        if vec:                                         # the scale of the (vector, atom) products: a yardstick, fp64 is enough for it
            ci, si = np.abs(np.cos(ph64[i]))[None, :], np.abs(np.sin(ph64[i]))[None, :]
            cj, sj = np.abs(np.cos(ph64)), np.abs(np.sin(ph64))
            se += X(abs(float(pre)) * float((g64[None, :] * aq64[:, None] * (ci * cj + si * sj)).sum()))
            per_v = (g64[None, :] * aq64[:, None] * (si * cj + ci * sj)).sum(0)
            sf = [sf[x] + X(2 * abs(float(pre)) * float((per_v * np.abs(k64[:, x])).sum())) for x in range(3)]
        F = [F[x] + 2 * pre * sum(g * kv[x] * (sn[i][v] * Sc[v] - cs[i][v] * Ss[v]) for v, (_, kv, g) in enumerate(vec)) for x in range(3)]
        e_self, e_bg = -kap * al * qi * qi / mp.sqrt(mp.pi), -kap * mp.pi * qi * Q / (2 * al * al * V)
        comp.append([e_r, e_k, e_self, e_bg, e_s])
        force.append(F)
        scale_e.append(se + abs(e_self) + abs(e_bg))
        scale_f.append(sf)
    fl = lambda rowsf: np.array([[float(v) for v in row] for row in rowsf], dtype=np.float64).reshape(len(rowsf), -1)
    out = dict(row_ptr=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32),
               atom=np.array([j for r in rows for j, _, _, _ in r], np.int32), code=np.array([c for r in rows for _, c, _, _ in r], np.int32),
               hkl=np.array([m for m, _, _ in vec], np.int32).reshape(-1, 3), comp_atom=fl(comp), e_atom=np.array([float(sum(c)) for c in comp]),
               force=fl(force), scale_e=np.array([float(v) for v in scale_e]), scale_f=fl(scale_f),
               components=np.array([float(sum(c[k] for c in comp)) for k in range(5)]), energy=np.float64(float(sum(sum(c) for c in comp))),
               gap=np.float64(float(min(gap))))
    if derivative:
        worst = mp.mpf(0)
        for i in range(N):
            ti, qi = int(t[i]), q[int(t[i])]
            for x in range(3):
                def energy(delta):      # the part of the cell energy that depends on atom i moved by delta along x
                    e = mp.mpf(0)
                    for j, _, d, _ in rows[i]:
                        if j == i:
                            continue      # an own image moves with the atom
                        dd = [d[y] - (delta if y == x else 0) for y in range(3)]
                        r = mp.sqrt(sum(v * v for v in dd))
                        e += kap * qi * q[int(t[j])] * mp.erfc(al * r) / r
                        if pot is not None and r < sc_:
                            e += u_of(ti * A + int(t[j]), r)[0]
                    for v, (_, kv, g) in enumerate(vec):
                        p = phi[i][v] + kv[x] * delta
                        c2 = Sc[v] + qi * (mp.cos(p) - cs[i][v])
                        s2 = Ss[v] + qi * (mp.sin(p) - sn[i][v])
                        e += 4 * mp.pi * kap / V * g * (c2 * c2 + s2 * s2)
                    return e
                worst = max(worst, abs(force[i][x] + mp.diff(energy, 0)) / max(scale_f[i][x], mp.mpf(10) ** -300))
        out["deriv_error"] = np.float64(float(worst))
    return out


# ---- the host statement -----------------------------------------------------------------------------------------------------------------
def host(L, cases, forces=True, raw=None, **override):
    """egnn_cell_ewald_host on the cells of ``cases`` with the parameters of the first (``override`` replaces some) -> (rc, dict).
    Every output starts at -7: the statement writes all of them."""
    c0 = dict(cases[0], **override)
    a = STU.batch_arrays([c["cell"] for c in cases])
    a.update(raw or {})
    C, N, A = len(a["cell_ptr"]) - 1, int(a["cell_ptr"][-1]), int(override.get("A", max(c["cell"]["A"] for c in cases)))
    out = dict(energy=np.full(C, -7.0), components=np.full((C, 5), -7.0), e_atom=np.full(N, -7.0), comp_atom=np.full((N, 5), -7.0),
               force=np.full((N, 3), -7.0) if forces else None, n_sites=np.full(N, -7, np.int32), n_vectors=np.full(C, -7, np.int64),
               coincident=np.full(C, -7, np.int32))
    q = np.ascontiguousarray(c0["charges"], dtype=np.float64)
    rc = L.egnn_cell_ewald_host(C, A, vp(a["cell_ptr"]), vp(a["lattice"]), vp(a["frac"]), vp(a["type"]), vp(q), vp(c0["pot"]), c0["n"],
                                int(c0["shift"]), c0["kappa"], c0["alpha"], c0["r_cut"], c0["short_cut"], c0["k_max"], int(forces),
                                vp(out["energy"]), vp(out["components"]), vp(out["e_atom"]), vp(out["comp_atom"]), vp(out["force"]),
                                vp(out["n_sites"]), vp(out["n_vectors"]), vp(out["coincident"]))
    return rc, out


# ---- the truth of the fixtures and the host statement on it (computed once, never changed) ----------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    return np.load(GOLDEN)


@functools.lru_cache(maxsize=None)
def truth(name):
    G, case = golden(), fixtures()[name]
    cell = case["cell"]
    assert np.array_equal(cell["lattice"], G[f"{name}_lattice"]) and np.array_equal(cell["frac"], G[f"{name}_frac"]), "the fixture moved"
    assert np.array_equal(cell["types"], G[f"{name}_types"]), "the fixture moved"
    want = np.array([case["kappa"], case["alpha"], case["r_cut"], case["short_cut"], case["k_max"], case["n"], case["shift"]], np.float64)
    assert np.array_equal(want, G[f"{name}_params"]) and np.array_equal(case["charges"], G[f"{name}_charges"]), "the fixture moved"
    return {k: G[f"{name}_{k}"] for k in ("row_ptr", "atom", "code", "hkl", "comp_atom", "e_atom", "force", "scale_e", "scale_f", "components",
                                          "energy", "gap")}


@functools.lru_cache(maxsize=None)
def host_on_golden(name):
    from diffusion_model_amd import _lib
    truth(name)
    rc, res = host(_lib.lib(), [fixtures()[name]])
    assert rc == 0, _lib.lib().egnn_last_error()
    return res


def error(got, want, forces=True):
    """E of one cell: ``got`` with e_atom [N], comp_atom [N, 5], force [N, 3], energy, components [5]; ``want`` from ``exact``"""
    se = want["scale_e"]
    tot = float(se.sum()) if len(se) else 1.0
    parts = [np.abs(got["e_atom"] - want["e_atom"]) / se, (np.abs(got["comp_atom"] - want["comp_atom"]) / se[:, None]).reshape(-1),
             np.abs(np.asarray(got["energy"]).reshape(-1)[:1] - want["energy"]) / tot,
             np.abs(np.asarray(got["components"]).reshape(-1, 5)[0] - want["components"]) / tot]
    if forces:
        diff, sf = np.abs(got["force"] - want["force"]), want["scale_f"]
        parts.append(np.where(sf > 0.0, diff / np.where(sf > 0.0, sf, 1.0), np.where(diff == 0.0, 0.0, np.inf)).reshape(-1))
    return max(float(p.max(initial=0.0)) for p in parts)


@functools.lru_cache(maxsize=None)
def e_host(name):
    """E_host of one fixture: the host statement against the truth"""
    return error(host_on_golden(name), truth(name))

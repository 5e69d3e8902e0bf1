"""Float64 restatement of the reference's three Kabsch spellings and of its correspondence search, shared by the RMSD tests and
by tests/golden/make_rmsd_golden.py (test infrastructure, not product).

  kabsch_torch   evaluate_rmsd_for_pos_generate.py:11-51   centroid, `Vt[:, -1] *= -1`  -> kabsch_f64(P, Q, "centroid", "column")
  kabsch_numpy   evaluate_rmsd_for_pos_generate.py:53-92   centroid, `Vt[-1, :] *= -1`  -> kabsch_f64(P, Q, "centroid", "row")
  kabsch_numpy   evaluate_rmsd.py:10-42                    atom 0,   `Vt[-1, :] *= -1`  -> kabsch_f64(P, Q, "first", "row")
  the loop       evaluate_rmsd.py:93-107                   minimum over [0] + perm(1..n-1), first strict minimum -> search_f64
"""
import itertools
import math

import numpy as np

SPELLINGS = {"torch": ("centroid", "column"), "numpy_centroid": ("centroid", "row"), "numpy_first": ("first", "row")}


def covariance_f64(P, Q, center):
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    cp, cq = (P.mean(0), Q.mean(0)) if center == "centroid" else (P[0], Q[0])
    p, q = P - cp, Q - cq
    return p, q, cq - cp, p.T @ q


def kabsch_f64(P, Q, center="centroid", flip="column"):
    """-> (R, t, rmsd) in float64, formula by formula as the reference writes it"""
    p, q, t, H = covariance_f64(P, Q, center)
    U, S, Vt = np.linalg.svd(H)
    if np.linalg.det(Vt.T @ U.T) < 0.0:
        if flip == "row":
            Vt[-1, :] *= -1.0
        else:
            Vt[:, -1] *= -1.0
    R = Vt.T @ U.T
    return R, t, float(np.sqrt(np.sum(np.square(p @ R.T - q)) / P.shape[0]))


def sigma_f64(P, Q, center):
    return np.linalg.svd(covariance_f64(P, Q, center)[3], compute_uv=False)


# A singular direction is defined to about eps * sigma_1 / gap.  The fixes are functions of the polar factor (needs sigma_3 away
# from 0) and, for 'row' in a reflection case, of the smallest singular direction (needs sigma_3 away from sigma_2): with both
# gaps >= 1e-2 sigma_1 float32 noise (6e-8) is amplified at most 100-fold, which is the size ref_vs_f64 is measured at.
WELL_CONDITIONED_GAP = 1e-2


def well_conditioned(sigma):
    s = np.asarray(sigma, dtype=np.float64)
    return bool(s[2] >= WELL_CONDITIONED_GAP * s[0] and s[1] - s[2] >= WELL_CONDITIONED_GAP * s[0])


def full_rank(sigma, tol=1e-6):
    """sigma_3 clearly above float32 rounding of sigma_1: the reflection decision itself is defined"""
    s = np.asarray(sigma, dtype=np.float64)
    return bool(s[2] > tol * s[0])


def rank_to_order(rank, n):
    """the ordering [0] + perm of lexicographic rank `rank` among the (n-1)! permutations of 1..n-1 (factorial number system)"""
    free, order = list(range(1, n)), [0]
    for i in range(1, n):
        f = math.factorial(n - 1 - i)
        order.append(free.pop(rank // f))
        rank %= f
    return order


def order_to_rank(order):
    n, free, rank = len(order), list(range(1, len(order))), 0
    for i in range(1, n):
        k = free.index(order[i])
        rank += k * math.factorial(n - 1 - i)
        free.pop(k)
    return rank


def all_orders(n):
    """[(n-1)!, n] int64 in itertools.permutations order"""
    perms = np.array(list(itertools.permutations(range(1, n))), dtype=np.int64).reshape(-1, n - 1)
    return np.concatenate([np.zeros((perms.shape[0], 1), dtype=np.int64), perms], axis=1)


def search_rmsds_f64(gen, orig, chunk=40000):
    """RMSD of every ordering (evaluate_rmsd.py:93-102 with kabsch_numpy of :10-42), float64, vectorised over orderings with batched
    numpy.linalg.svd -> [(n-1)!]"""
    gen, orig = np.asarray(gen, dtype=np.float64), np.asarray(orig, dtype=np.float64)
    n = gen.shape[0]
    g, q = gen - gen[0], orig - orig[0]
    orders = all_orders(n)
    out = np.empty(orders.shape[0])
    for lo in range(0, orders.shape[0], chunk):
        p = g[orders[lo:lo + chunk]]                       # [m, n, 3]
        H = np.einsum("mir,ic->mrc", p, q)
        U, S, Vt = np.linalg.svd(H)
        neg = np.linalg.det(np.swapaxes(Vt, 1, 2) @ np.swapaxes(U, 1, 2)) < 0.0
        Vt[neg, -1, :] *= -1.0
        R = np.swapaxes(Vt, 1, 2) @ np.swapaxes(U, 1, 2)
        out[lo:lo + chunk] = np.sqrt(np.sum(np.square(p @ np.swapaxes(R, 1, 2) - q), axis=(1, 2)) / n)
    return out


def search_f64(gen, orig):
    """-> (min_rmsd, order, second smallest rmsd or inf): the first strict minimum in itertools.permutations order"""
    r = search_rmsds_f64(gen, orig)
    k = int(np.argmin(r))                                   # numpy returns the first occurrence
    second = float(np.partition(r, 1)[1]) if r.size > 1 else float("inf")
    return float(r[k]), rank_to_order(k, gen.shape[0]), second


GAP = 1e-3   # (second - best) >= GAP * best: below it "the same order" is not testable for the reference itself


def random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def silica_cloud(rng, n):
    """n points on a silica-like length scale: atom 0 at the origin, the others 1.6 A (a Si-O bond) to 5 A away, no two closer
    than 1.2 A where that can be had"""
    pts = [np.zeros(3)]
    for _ in range(n - 1):
        for attempt in range(200):
            v = rng.standard_normal(3)
            cand = v / np.linalg.norm(v) * rng.uniform(1.6, 5.0)
            if attempt == 199 or min(np.linalg.norm(cand - p) for p in pts) >= 1.2:
                pts.append(cand)
                break
    return np.array(pts)

"""Float64 restatement of the reference's atom matching of graphs of six atoms or more (create_xyz.py:157-192), shared by the
assignment tests and by tests/golden/make_assign_golden.py (test infrastructure, not product).

  return_near_from_exO   create_xyz.py:87-96    the atoms nearest to atom 0, stable sort            -> near_f64
  the pairing loop       create_xyz.py:158-176  best of the 24 five-point fits, first strict minimum -> prealign_f64
  hungarian_algorithm    create_xyz.py:82-85    scipy linear_sum_assignment on the distance matrix  -> assign_f64
  the whole branch       create_xyz.py:157-192                                                      -> align_f64

sap_lowest_index is the device solver's algorithm (csrc/eval/assign.hip) written out in numpy: shortest augmenting paths, rows in
index order, equal path costs to the lowest column index.  It is what the tie rule of csrc/eval/assign.h means, executable.
"""
import itertools

import numpy as np

from tests import _rmsd_util as RU

PERMS4 = list(itertools.permutations(range(4)))


def near_f64(pos):
    """indices of the (up to five) atoms nearest to atom 0, ascending, equal distances in index order"""
    pos = np.asarray(pos, dtype=np.float64)
    d = np.linalg.norm(pos[1:] - pos[0], axis=1)
    return (1 + np.argsort(d, kind="stable"))[:5]


def near_gap(pos):
    """smallest relative separation among the five smallest distances to atom 0 (the sixth does not matter to the first four,
    the fifth does: it must not overtake the fourth)"""
    pos = np.asarray(pos, dtype=np.float64)
    d = np.sort(np.linalg.norm(pos[1:] - pos[0], axis=1))[:5]
    return float(np.min(np.diff(d) / d[1:]))


def prealign_f64(orig, gen):
    """-> (R, perm index of the winner, sorted rmsds of the 24 fits)"""
    orig, gen = np.asarray(orig, dtype=np.float64), np.asarray(gen, dtype=np.float64)
    io, ig = near_f64(orig), near_f64(gen)
    o5 = np.concatenate([orig[:1], orig[io[:4]]])
    best, best_R, best_k, seen = 1e10, None, None, []
    for k, perm in enumerate(PERMS4):
        g5 = np.concatenate([gen[:1], gen[ig[list(perm)]]])
        R, _, rmsd = RU.kabsch_f64(g5, o5, "first", "row")
        seen.append(rmsd)
        if rmsd < best:
            best, best_R, best_k = rmsd, R, k
    return best_R, best_k, np.sort(np.array(seen))


def prealign_points(orig, gen, k):
    """the five points of pairing k (index into PERMS4) -> (generated_near, original_near), float64"""
    orig, gen = np.asarray(orig, dtype=np.float64), np.asarray(gen, dtype=np.float64)
    io, ig = near_f64(orig), near_f64(gen)
    return np.concatenate([gen[:1], gen[ig[list(PERMS4[k])]]]), np.concatenate([orig[:1], orig[io[:4]]])


def distance_matrix(P, Q, dtype=np.float64):
    P, Q = np.asarray(P, dtype=dtype), np.asarray(Q, dtype=dtype)
    return np.linalg.norm(P[:, None, :] - Q[None, :, :], axis=-1)


def assignment_cost_f64(P, Q, col):
    """sum_i |P_i - Q_col[i]| in float64 from the given coordinates"""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    return float(np.linalg.norm(P - Q[np.asarray(col)], axis=1).sum())


def is_permutation(col, n):
    return sorted(np.asarray(col).tolist()) == list(range(n))


def assign_f64(P, Q):
    from scipy.optimize import linear_sum_assignment
    return linear_sum_assignment(distance_matrix(P, Q))


def runner_up_cost(D, col):
    """cost of the cheapest assignment that avoids at least one edge of `col`: n re-solves with one entry forbidden"""
    from scipy.optimize import linear_sum_assignment
    D = np.asarray(D, dtype=np.float64)
    big = D.sum() + 1.0
    best = np.inf
    for i, j in enumerate(col):
        keep = D[i, j]
        D[i, j] = big
        r, c = linear_sum_assignment(D)
        best = min(best, D[r, c].sum())
        D[i, j] = keep
    return float(best)


def align_f64(orig, gen):
    """the branch :157-192 in float64 -> dict(R, row_ind, col_ind, orig_reordered, gen_reordered, aligned, rmsd)"""
    orig, gen = np.asarray(orig, dtype=np.float64), np.asarray(gen, dtype=np.float64)
    R, k, _ = prealign_f64(orig, gen)
    o, g = orig - orig[0], gen - gen[0]
    aligned = g @ R.T
    row, col = assign_f64(o, aligned)
    go, oo = aligned[col], o[row]
    return dict(R=R, perm=k, row_ind=row, col_ind=col, orig_reordered=oo, gen_reordered=go, aligned=aligned,
                rmsd=RU.kabsch_f64(go, oo, "first", "row")[2])


def sap_lowest_index(D):
    """the device solver on a cost matrix D [n, n] (float64): -> (col4row, u, v)"""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    u, v = np.zeros(n), np.zeros(n)
    row4col, col4row = -np.ones(n, dtype=np.int64), -np.ones(n, dtype=np.int64)
    for cur in range(n):
        sp = np.full(n, np.inf)
        pred = -np.ones(n, dtype=np.int64)
        scanned = np.zeros(n, dtype=bool)
        min_val, i, sink = 0.0, cur, -1
        while sink < 0:
            r = ((min_val + D[i]) - u[i]) - v
            upd = ~scanned & (r < sp)
            sp[upd] = r[upd]
            pred[upd] = i
            key = np.where(scanned, np.inf, sp)
            j = int(np.argmin(key))                       # numpy returns the first occurrence: the lowest index
            if scanned[j]:
                raise ValueError("no column left")
            min_val = key[j]
            scanned[j] = True
            if row4col[j] < 0:
                sink = j
            else:
                i = row4col[j]
        for j in np.nonzero(scanned)[0]:
            delta = min_val - sp[j]
            if row4col[j] >= 0:
                u[row4col[j]] += delta
            v[j] -= delta
        u[cur] += min_val
        j = sink
        while True:
            r = pred[j]
            row4col[j] = r
            col4row[r], j = j, col4row[r]
            if r == cur:
                break
    return col4row, u, v


def pair_case(rng, n, noise, orig=None):
    """a silica-like cloud (drawn here unless given) and its shuffled, rotated, translated, noised copy (atom 0 stays atom 0: it
    is the excited O both structures are anchored at) -> (orig float32 [n,3], gen float32 [n,3], shuffle)"""
    orig = RU.silica_cloud(rng, n) if orig is None else np.asarray(orig, dtype=np.float64)
    shuffle = np.concatenate([[0], 1 + rng.permutation(n - 1)])
    gen = (orig @ RU.random_rotation(rng).T + rng.uniform(-3, 3, 3) + noise * rng.standard_normal((n, 3)))[shuffle]
    return orig.astype(np.float32), gen.astype(np.float32), shuffle

"""Numpy restatement of the SOAP entries (csrc/eval/soap_math.h), shared by the CPU and GPU tests (test infrastructure), the
fixtures both use, and the ctypes wrapper of the host statement egnn_soap_host.

  * fixtures: seeded clouds of SIZES atoms -- a lone centre, a pair, sizes below a neighbour chunk of 32, straddling one, just
    past a wavefront, a graph above two chunks whose far atoms fall outside the cut -- the SAME positions for A = 1, 2, 3 types
    (types drawn per A; small graphs miss a species); two configurations, the default one and a small one;
  * the truth is tests/golden/soap_golden.npz (make_soap_golden.py: mpmath at 60 digits); this restatement is float64 numpy over
    the golden's exact tables, so it is as good as the host statement, not better;
  * row sums (dot products, norms, squared spectrum differences) in the one order of soap_math.h: element f to partial f % 64,
    partials ascending, then the butterfly 32, 16, .., 1 -- numpy rounds every operation, so they are BITWISE the library's.
  * the basis limits and the degenerate bases (LIMIT_CONFIGS, each with its own A up to 4): their truth is
    tests/golden/soap_limits_golden.npz (make_soap_limits_golden.py), atom 0 of the listed fixture graphs.
Gap conditions (asserted by every test for its inputs): no pair distance within 1e-9 (relative) of the neighbour cut; for every
target no two candidate MSEs within 1e-9 (relative) of each other -- or, where the tie rule is the subject
(mse_gap_ok_with_ties), no two DISTINCT ones.
"""
import ctypes as C
import functools
import os

import numpy as np

SIZES = [1, 2, 5, 17, 64, 65, 130]
TYPES = (1, 2, 3)
CONFIGS = {"default": dict(r_cut=8.0, n_max=15, l_max=10, sigma=0.1), "small": dict(r_cut=4.0, n_max=3, l_max=2, sigma=0.1)}
GOLDEN_GRAPHS = {"default": 3, "small": len(SIZES)}       # the default configuration's truth covers the three smallest graphs
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "soap_golden.npz")
POSITION_SEED = 11
# The basis limits and the degenerate bases, each with ITS number of types A (a table of its own: CONFIGS x TYPES keep their
# meaning).  "graphs": the fixture graphs whose atom 0 the truth covers (tests/golden/soap_limits_golden.npz); the 17-atom graph is
# the first that holds all four species.  limit: kSoapMaxTypes, kSoapMaxN, kSoapMaxL of soap_math.h and the largest LDS request.
LIMIT_CONFIGS = {
    "limit": dict(r_cut=8.0, n_max=16, l_max=10, sigma=0.1, A=4, graphs=4),
    "n16l0": dict(r_cut=8.0, n_max=16, l_max=0, sigma=0.1, A=2, graphs=5),       # LM = 1, L1 = 1: task / L1 and o / LM degenerate
    "n1l0": dict(r_cut=4.0, n_max=1, l_max=0, sigma=0.1, A=4, graphs=7),         # a 1 x 1 beta on r = [1]
    "n1l10": dict(r_cut=4.0, n_max=1, l_max=10, sigma=0.1, A=3, graphs=5),
    "n7l5": dict(r_cut=6.0, n_max=7, l_max=5, sigma=0.1, A=4, graphs=4),         # odd, mid-size: nL = 42, LM = 36
}
LIMITS_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "soap_limits_golden.npz")


def basis_of(cfg):
    """the four parameters of SoapBasis / Basis out of an entry of CONFIGS or LIMIT_CONFIGS"""
    return {k: cfg[k] for k in ("r_cut", "n_max", "l_max", "sigma")}


def neighbour_cut(cfg):
    return cfg["r_cut"] + cfg["sigma"] * np.sqrt(2.0 * np.log(1000.0))


def fixture(A, n_graphs=len(SIZES)):
    """-> (pos float32 [N, 3], types int32 [N], sizes): graph g fills a box of edge 2.2 cbrt(n), atom 0 near its middle"""
    rng = np.random.default_rng(POSITION_SEED)
    pos = []
    for n in SIZES:
        box = 2.2 * np.cbrt(n)
        p = rng.uniform(0.0, box, (n, 3))
        p[0] = box / 2 + rng.uniform(-0.2, 0.2, 3)
        pos.append(p)
    types = np.random.default_rng(100 + A).integers(0, A, sum(SIZES))
    sizes = SIZES[:n_graphs]
    N = sum(sizes)
    return np.concatenate(pos)[:N].astype(np.float32), types[:N].astype(np.int32), list(sizes)


def graph_ptr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def first_centres(sizes):
    return graph_ptr(sizes)[:-1].copy()


def dist2(pos, i, js):
    p = np.asarray(pos, dtype=np.float32).astype(np.float64)
    d = p[js] - p[i]
    return d, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def gap_ok(pos, sizes, cut, rel=1e-9):
    gp = graph_ptr(sizes)
    for g in range(len(sizes)):
        for i in range(gp[g], gp[g + 1]):
            _, d2 = dist2(pos, i, np.arange(gp[g], gp[g + 1]))
            if np.any(np.abs(np.sqrt(d2) - cut) <= rel * cut):
                return False
    return True


def features(A, n_max, l_max):
    return (A * (n_max * (n_max + 1) // 2) + A * (A - 1) // 2 * n_max * n_max) * (l_max + 1)


def feature_index(A, n_max, l_max):
    """-> int arrays (z1, z2, n, n', l) of every feature in order"""
    rows = []
    for z1 in range(A):
        for z2 in range(z1, A):
            for n in range(n_max):
                for q in range(n if z1 == z2 else 0, n_max):
                    for l in range(l_max + 1):
                        rows.append((z1, z2, n, q, l))
    return np.array(rows).T


def tables_of(golden, name):
    """(K, gamma, beta, norm, weight) and the flat buffer of soap_math.h from the golden file"""
    parts = [golden[f"{name}_{k}"] for k in ("K", "gamma", "beta", "norm", "weight")]
    return parts, np.ascontiguousarray(np.concatenate([p.reshape(-1) for p in parts]))


def solid_harmonics(d, l_max, norm):
    """R_lm of the rows of d [P, 3] -> [P, (l_max+1)^2], by the recurrence of soap_solid_column"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    r2 = (x * x + y * y) + z * z
    out = np.zeros((len(d), (l_max + 1) ** 2))
    ca, sa, pmm = np.ones(len(d)), np.zeros(len(d)), 1.0
    for m in range(l_max + 1):
        if m:
            ca, sa = ca * x - sa * y, ca * y + sa * x
            pmm *= 2 * m - 1
        p2, p1 = np.zeros(len(d)), np.full(len(d), pmm)
        for l in range(m, l_max + 1):
            if l > m:
                p = (((2 * l - 1) * z) * p1 - ((l + m - 1) * r2) * p2) / (l - m)
                p2, p1 = p1, p
            at = l * l + l
            out[:, at + m] = (norm[at + m] * p1) * ca
            if m:
                out[:, at - m] = (norm[at - m] * p1) * sa
    return out


def descriptors(pos, types, sizes, A, centres, tables, cut):
    """float64 restatement -> (desc [C, F], coeff [C, A, n_max, LM])"""
    K, gamma, beta, norm, weight = tables
    n_max, L1 = K.shape
    l_max, LM = L1 - 1, L1 * L1
    l_of = np.repeat(np.arange(L1), 2 * np.arange(L1) + 1)
    gp = graph_ptr(sizes)
    z1, z2, n1, n2, ll = feature_index(A, n_max, l_max)
    desc, coeff = np.empty((len(centres), len(ll))), np.empty((len(centres), A, n_max, LM))
    for ci, i in enumerate(centres):
        g = int(np.searchsorted(gp, i, side="right")) - 1
        js = np.arange(gp[g], gp[g + 1])
        d, d2 = dist2(pos, i, js)
        keep = d2 < cut * cut
        d, d2, tj = d[keep], d2[keep], np.asarray(types)[js][keep]
        R = solid_harmonics(d, l_max, norm)                                     # [P, LM]
        rad = K[None] * np.exp(-(gamma[None] * d2[:, None, None]))              # [P, n, l]
        prim = np.zeros((A, n_max, LM))
        for j in range(len(d2)):                                                # ascending, as the library
            prim[tj[j]] += rad[j][:, l_of] * R[j][None, :]
        c = np.einsum("lnq,zql->znl", beta[l_of], prim)                         # c[z, n, lm] = sum_n' beta[l][n, n'] prim[z, n', lm]
        coeff[ci] = c
        prod = c[z1, n1] * c[z2, n2]                                            # [F, LM]
        mask = l_of[None, :] == ll[:, None]
        desc[ci] = weight[ll] * np.where(mask, prod, 0.0).sum(1)
    return desc, coeff


def _butterfly(partial):
    q = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        partial = partial + partial[..., q ^ off]
    return partial[..., 0]


def row_sum(v):
    """the one summation order of soap_math.h over the last axis of v (float64), for every leading index at once"""
    v = np.asarray(v, dtype=np.float64)
    F = v.shape[-1]
    pad = (-F) % 64
    v = np.concatenate([v, np.zeros(v.shape[:-1] + (pad,))], -1).reshape(v.shape[:-1] + (-1, 64))
    partial = np.zeros(v.shape[:-2] + (64,))
    for t in range(v.shape[-2]):
        partial = partial + v[..., t, :]
    return _butterfly(partial)


def cosine(a, b):
    """rows of a against the same rows of b"""
    return row_sum(a * b) / (np.sqrt(row_sum(a * a)) * np.sqrt(row_sum(b * b)))


def cosine_matrix(a, b):
    return row_sum(a[:, None, :] * b[None, :, :]) / (np.sqrt(row_sum(a * a))[:, None] * np.sqrt(row_sum(b * b))[None, :])


def mse_matrix(target, reference):
    t = np.asarray(target, dtype=np.float32).astype(np.float64)
    r = np.asarray(reference, dtype=np.float32).astype(np.float64)
    d = t[:, None, :] - r[None, :, :]
    return row_sum(d * d) / t.shape[1]


def nearest(target, reference, k, tg=None, rg=None):
    """-> (idx [T, k], mse [T, k], the candidate matrix with excluded entries +inf)"""
    m = mse_matrix(target, reference)
    if tg is not None:
        tg, rg = np.asarray(tg), np.asarray(rg)
        m = np.where((tg[:, None] == rg[None, :]) & (tg[:, None] >= 0), np.inf, m)
    T, R = m.shape
    idx, out = np.full((T, k), -1, dtype=np.int64), np.full((T, k), np.inf)
    for t in range(T):
        order = np.argsort(m[t], kind="stable")                                 # ties to the lower index
        order = order[np.isfinite(m[t][order])][:k]
        idx[t, :len(order)], out[t, :len(order)] = order, m[t][order]
    return idx, out, m


def mse_gap_ok(m, rel=1e-9):
    for row in m:
        v = np.sort(row[np.isfinite(row)])
        if len(v) > 1 and np.any(np.diff(v) <= rel * v[1:]):
            return False
    return True


def mse_gap_ok_with_ties(m, rel=1e-9):
    """mse_gap_ok where exact duplicates are allowed: the DISTINCT finite values of a row stay rel apart, so the only ambiguity left
    is the one the tie rule (the lower reference index first) decides"""
    for row in m:
        v = np.unique(row[np.isfinite(row)])
        if len(v) > 1 and np.any(np.diff(v) <= rel * v[1:]):
            return False
    return True


def spectra(seed, T, R, S):
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.0, 1.5, (8, S))
    pick = lambda n: (base[rng.integers(0, 8, n)] + 0.2 * rng.standard_normal((n, S))).astype(np.float32)
    return pick(T), pick(R)


TIE_ROWS, TIE_PAIR = (3, 17, 18, 40), (5, 6)


def tie_spectra(S=200):
    """5 targets, 70 references with exact duplicates: rows TIE_ROWS are one row, a float32 neighbour of target 0 (so the four-fold
    tie takes the first places of target 0 and straddles the k-th place for k = 1, 2, 3), rows TIE_PAIR another, near target 1.  No
    target equals a reference."""
    t, r = spectra(77, 5, 70, S)
    r = r.copy()
    r[list(TIE_ROWS)] = t[0] + np.float32(0.015625) * np.cos(np.arange(S, dtype=np.float32))
    r[list(TIE_PAIR)] = t[1] - np.float32(0.03125) * np.sin(1 + np.arange(S, dtype=np.float32))
    assert not np.array_equal(r[3], t[0]) and not np.array_equal(r[5], t[1])
    return t, r


def nonfinite_spectra(S=65):
    """4 targets, 12 references: reference 2 holds a NaN, reference 7 a +inf, target 1 a NaN"""
    t, r = spectra(78, 4, 12, S)
    t, r = t.copy(), r.copy()
    r[2, S // 2], r[7, S - 1], t[1, 0] = np.nan, np.inf, np.nan
    return t, r


def cosine_rows(seed, rows, F):
    """float64 rows with entries of either sign and magnitudes 1e-8 .. 1e3"""
    rng = np.random.default_rng(seed)
    return rng.choice([-1.0, 1.0], (rows, F)) * 10.0 ** rng.uniform(-8.0, 3.0, (rows, F))


COSINE_F = (1, 63, 64, 65, 128, 129)
COSINE_SHAPES = ((1, 1), (3, 7), (4, 8), (5, 9), (9, 17))


def cosine_pairs(P, rows_a, rows_b):
    """P listed pairs with a repeat where P allows one"""
    rng = np.random.default_rng(P)
    pairs = np.stack([rng.integers(0, rows_a, P), rng.integers(0, rows_b, P)], 1)
    if P > 2:
        pairs[P - 1] = pairs[0]
    return pairs.astype(np.int32)


# ---- the host statement -------------------------------------------------------------------------------------------------------------
def vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def host_descriptors(L, pos, types, sizes, A, centres, cfg, flat, cut=None, coeff=True):
    """egnn_soap_host, descriptor part -> (rc, desc, coeff | None)"""
    pos, types = np.ascontiguousarray(pos, dtype=np.float32), np.ascontiguousarray(types, dtype=np.int32)
    gp, cs = graph_ptr(sizes), np.ascontiguousarray(centres, dtype=np.int32)
    n_max, l_max = cfg["n_max"], cfg["l_max"]
    F = features(A, n_max, l_max) if 1 <= A <= 4 and 1 <= n_max <= 16 and 0 <= l_max <= 10 else 1
    desc = np.full((len(cs), F), -7.0)
    co = np.full((len(cs), max(A, 1), max(n_max, 1), (max(l_max, 0) + 1) ** 2), -7.0) if coeff else None
    rc = L.egnn_soap_host(len(sizes), len(types), A, vp(pos), vp(types), vp(gp), n_max, l_max, neighbour_cut(cfg) if cut is None else cut,
                          vp(flat), len(cs), vp(cs), vp(desc), vp(co), 0, None, 0, None, 0, 0, None, None, None, 0, 0, 0, 0, None, None,
                          None, None, None, None)
    return rc, desc, co


def host_cosines(L, a, b, pairs=None, n_pairs=None, gram=False):
    """egnn_soap_host, cosine part -> (rc, cos [P] | None, gram [n_a, n_b] | None)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    pr = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32)
    P = (len(pr) if pr is not None else 0) if n_pairs is None else n_pairs
    cos = np.full(max(P, 1), -7.0)
    G = np.full((a.shape[0], b.shape[0]), -7.0) if gram else None
    rc = L.egnn_soap_host(0, 0, 0, None, None, None, 0, 0, 0.0, None, 0, None, None, None, a.shape[1], vp(a), a.shape[0], vp(b), b.shape[0],
                          P, vp(pr), vp(cos), vp(G), 0, 0, 0, 0, None, None, None, None, None, None)
    return rc, cos[:P], G


def host_nearest(L, target, reference, k, tg=None, rg=None):
    """egnn_soap_host, nearest part -> (rc, idx [T, k], mse [T, k])"""
    t, r = np.ascontiguousarray(target, dtype=np.float32), np.ascontiguousarray(reference, dtype=np.float32)
    tg = None if tg is None else np.ascontiguousarray(tg, dtype=np.int32)
    rg = None if rg is None else np.ascontiguousarray(rg, dtype=np.int32)
    kk = k if 1 <= k <= 8 else 1
    idx, mse = np.full((t.shape[0], kk), -7, dtype=np.int32), np.full((t.shape[0], kk), -7.0)
    rc = L.egnn_soap_host(0, 0, 0, None, None, None, 0, 0, 0.0, None, 0, None, None, None, 0, None, 0, None, 0, 0, None, None, None,
                          t.shape[0], r.shape[0], t.shape[1], k, vp(t), vp(r), vp(tg), vp(rg), vp(idx), vp(mse))
    return rc, idx, mse


def descriptor_error(got, truth):
    """E = max |p - p_truth| / max |p_truth|"""
    return float(np.abs(got - truth).max() / np.abs(truth).max())


# ---- the truth and the host statement on it (computed once, never changed) ------------------------------------------------------------
CAP = 1e-7          # E_host must stay below it: tables built in float64 land between 4e-5 and 2e-2, exact ones near 1e-10


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(GOLDEN)


@functools.lru_cache(maxsize=None)
def tables(name):
    return tables_of(golden(), name)


@functools.lru_cache(maxsize=None)
def host_on_golden(name, A):
    """the host statement on the golden's centres of one configuration and A -> (desc, coeff)"""
    from diffusion_model_amd import _lib
    G, cfg = golden(), CONFIGS[name]
    pos, types, sizes = fixture(A, GOLDEN_GRAPHS[name])
    assert np.array_equal(pos, G[f"{name}_A{A}_pos"]) and np.array_equal(types, G[f"{name}_A{A}_types"]), "the fixture moved"
    assert gap_ok(pos, sizes, neighbour_cut(cfg)), "ambiguous input: a distance on the neighbour cut"
    rc, desc, coeff = host_descriptors(_lib.lib(), pos, types, sizes, A, G[f"{name}_A{A}_centres"], cfg, tables(name)[1])
    assert rc == 0, _lib.lib().egnn_last_error()
    return desc, coeff


@functools.lru_cache(maxsize=None)
def e_host(name):
    """E_host of one configuration: the host statement against the truth, the largest over A = 1, 2, 3"""
    G = golden()
    return max(descriptor_error(host_on_golden(name, A)[0], G[f"{name}_A{A}_desc"]) for A in TYPES)


# ---- the limits: their truth and the host statement on it -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def limits_golden():
    return np.load(LIMITS_GOLDEN)


@functools.lru_cache(maxsize=None)
def limit_tables(name):
    return tables_of(limits_golden(), name)


@functools.lru_cache(maxsize=None)
def limit_fixture(name):
    """the fixture graphs the truth of one limit configuration covers, at its A, checked against what the truth was computed on
    -> (pos, types, sizes)"""
    G, cfg = limits_golden(), LIMIT_CONFIGS[name]
    pos, types, sizes = fixture(cfg["A"], cfg["graphs"])
    assert np.array_equal(pos, G[f"{name}_pos"]) and np.array_equal(types, G[f"{name}_types"]), "the fixture moved"
    assert np.array_equal(G[f"{name}_centres"], first_centres(sizes))
    assert gap_ok(pos, sizes, neighbour_cut(cfg)), "ambiguous input: a distance on the neighbour cut"
    return pos, types, sizes


@functools.lru_cache(maxsize=None)
def host_on_limit(name):
    """the host statement on EVERY atom of limit_fixture(name) -> (desc, coeff)"""
    from diffusion_model_amd import _lib
    cfg = LIMIT_CONFIGS[name]
    pos, types, sizes = limit_fixture(name)
    rc, desc, coeff = host_descriptors(_lib.lib(), pos, types, sizes, cfg["A"], np.arange(len(types)), cfg, limit_tables(name)[1])
    assert rc == 0, _lib.lib().egnn_last_error()
    return desc, coeff


@functools.lru_cache(maxsize=None)
def e_host_limit(name):
    """E_host of one limit configuration: the host statement against the truth on the golden's centres"""
    G = limits_golden()
    return descriptor_error(host_on_limit(name)[0][G[f"{name}_centres"]], G[f"{name}_desc"])

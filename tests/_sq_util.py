"""Numpy float64 restatement of the reciprocal-space statistics (csrc/eval/sq_math.h), shared by the CPU and GPU tests and by the
fixture generator tests/golden/make_sq_golden.py (test infrastructure).

  * Debye sums: r in float64 from the float32 positions in the fixed order sqrt((dx*dx + dy*dy) + dz*dz), sinc(0) = 1, the cut
    r < r_max and the Lorch window sinc((pi r) / r_max); every ordered pair summed by numpy (its own order).
  * cells: reciprocal rows b_i = (2 pi (a_j x a_k)) / det, k = (h b_1 + k b_2) + l b_3, k2 = (kx kx + ky ky) + kz kz, member iff
    half space and k2 < q_max q_max, bin floor(sqrt(k2) / dq): numpy's float64 arithmetic rounds every operation, so the integer
    outputs are bitwise what the library computes (built with -ffp-contract=off); rho_a = sum exp(-2 pi i t), t the phase mod 1.
and the gap conditions under which integer outputs and cut sums can be compared:
  1. no r_ij within 1e-6 of r_max (debye_gap_ok);
  2. no |k_m| within 1e-9 (relative) of q_max or of a shell edge (cell_gap_ok).
The caps are conditions, from a few-ulp error per term times the term count at <= 4096 atoms.
"""
import ctypes as C
import os

import numpy as np

CAP_DEBYE = 1e-10    # max |D - D_truth| / sqrt(N_a N_b)
CAP_RHO = 1e-9       # max |rho_a - rho_truth| / sqrt(N_a)
CAP_SHELL = 1e-9     # |S_ab - S_truth| <= CAP_SHELL (sqrt(N_a) + sqrt(N_b)), S_ab = mean Re(rho_a rho_b*) / sqrt(N_a N_b)
MAX_INDEX = 1023
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sq_golden.npz")
TWO_PI = 6.283185307179586476925286766559
Q_GOLDEN = np.array([0.0, 0.05, 1.5, 7.3, 25.0])


def pair_index(b, c, A):
    lo, hi = min(b, c), max(b, c)
    return lo * A - lo * (lo - 1) // 2 + (hi - lo)


# ---- clusters ------------------------------------------------------------------------------------------------------------------------
def distances(pos):
    """float32 [n, 3] -> float64 [n, n] in the library's order"""
    p = np.asarray(pos, dtype=np.float32).astype(np.float64)
    d = p[None, :, :] - p[:, None, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def sinc(x):
    x = np.asarray(x, dtype=np.float64)
    safe = np.where(x == 0.0, 1.0, x)
    return np.where(x == 0.0, 1.0, np.sin(safe) / safe)


def debye_gap_ok(pos, sizes, r_max, gap=1e-6):
    if r_max is None or not np.isfinite(r_max):
        return True
    lo = 0
    for n in sizes:
        if n and np.any(np.abs(distances(pos[lo:lo + n]) - r_max) < gap):
            return False
        lo += n
    return True


def debye_restated(pos, types, sizes, A, q, r_max=None, window=None):
    """-> float64 [B, A, A, Q]"""
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    types = np.asarray(types)
    out = np.zeros((len(sizes), A, A, q.size))
    lo = 0
    for g, n in enumerate(sizes):
        r = distances(pos[lo:lo + n])
        t = types[lo:lo + n]
        keep = ~np.eye(n, dtype=bool)
        w = np.ones_like(r)
        if r_max is not None and np.isfinite(r_max):
            keep &= r < r_max
            if window == "lorch":
                w = sinc((np.pi * r) / r_max)
        for a in range(A):
            for b in range(A):
                m = keep & (t[:, None] == a) & (t[None, :] == b)
                rr, ww = r[m], w[m]
                for k0 in range(0, q.size, 64):
                    out[g, a, b, k0:k0 + 64] = (ww[:, None] * sinc(rr[:, None] * q[None, k0:k0 + 64])).sum(0)
        lo += n
    return out


def n_types(types, sizes, A):
    out, lo = np.zeros((len(sizes), A), dtype=np.int64), 0
    for g, n in enumerate(sizes):
        out[g] = np.bincount(np.asarray(types[lo:lo + n], dtype=np.int64), minlength=A)[:A]
        lo += n
    return out


def debye_error(D, truth, n_type):
    """max |D - truth| / sqrt(N_a N_b) over the present type pairs (an absent pair must be exactly zero)"""
    nn = np.sqrt(n_type[:, :, None] * n_type[:, None, :]).astype(np.float64)
    absent = nn == 0
    assert np.all(D[absent] == 0.0) and np.all(truth[absent] == 0.0)
    err = np.abs(D - truth) / np.where(absent, 1.0, nn)[..., None]
    return float(err.max()) if err.size else 0.0


def cloud(n, seed, A=2, volume=15.6):
    """n atoms uniform in a cube of ``volume`` A^3 per atom -> (float32 [n, 3], int32 [n])"""
    rng = np.random.default_rng(seed)
    box = (volume * max(n, 1)) ** (1.0 / 3.0)
    return (box * rng.uniform(0.0, 1.0, (n, 3))).astype(np.float32), rng.integers(0, A, n).astype(np.int32)


def finish_restated(D, n_type, weights, form):
    """the finishing formulas of stats._sf_finish in numpy: (partial [B, A, A, Q], total [B, Q])"""
    B, A, _, Q = D.shape
    n = n_type.astype(np.float64)
    N = n.sum(1)
    partial, total = np.zeros_like(D), np.zeros((B, Q))
    b = np.asarray(weights, dtype=np.float64)
    b = np.broadcast_to(b[:, None], (A, Q)) if b.ndim == 1 else b
    for g in range(B):
        if N[g] == 0:
            continue
        for a in range(A):
            for c in range(A):
                if n[g, a] * n[g, c] == 0:
                    continue
                if form == "faber-ziman":
                    partial[g, a, c] = 1.0 + N[g] / (n[g, a] * n[g, c]) * D[g, a, c]
                else:
                    partial[g, a, c] = (a == c) + D[g, a, c] / np.sqrt(n[g, a] * n[g, c])
        mean_b = (n[g] / N[g]) @ b
        total[g] = 1.0 + np.einsum("aq,cq,acq->q", b, b, D[g]) / (N[g] * mean_b ** 2)
    return partial, total


# ---- cells ---------------------------------------------------------------------------------------------------------------------------
def reciprocal(L):
    a, b, c = np.asarray(L, dtype=np.float64).reshape(3, 3)
    bc = np.array([b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]])
    ca = np.array([c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]])
    ab = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    det = (a[0] * bc[0] + a[1] * bc[1]) + a[2] * bc[2]
    return np.stack([(TWO_PI * bc) / det, (TWO_PI * ca) / det, (TWO_PI * ab) / det])


def index_need(L, q_max):
    L = np.asarray(L, dtype=np.float64).reshape(3, 3)
    norm = np.sqrt((L[:, 0] * L[:, 0] + L[:, 1] * L[:, 1]) + L[:, 2] * L[:, 2])
    return np.floor((q_max * norm) / TWO_PI).astype(np.int64)


def box_candidates(L, q_max, extra=1):
    """every (h, k, l) of the index box (``extra`` wider than the bound) in ascending order, and k2 in the library's order"""
    H, K, Lb = (int(min(v + extra, MAX_INDEX)) for v in index_need(L, q_max))
    h, k, l = np.meshgrid(np.arange(0, H + 1), np.arange(-K, K + 1), np.arange(-Lb, Lb + 1), indexing="ij")
    hkl = np.stack([h.ravel(), k.ravel(), l.ravel()], 1)
    Bm = reciprocal(L)
    f = hkl.astype(np.float64)
    kv = [(f[:, 0] * Bm[0, x] + f[:, 1] * Bm[1, x]) + f[:, 2] * Bm[2, x] for x in range(3)]
    return hkl, (kv[0] * kv[0] + kv[1] * kv[1]) + kv[2] * kv[2]


def half_space(hkl):
    h, k, l = hkl[:, 0], hkl[:, 1], hkl[:, 2]
    return (h > 0) | ((h == 0) & ((k > 0) | ((k == 0) & (l > 0))))


def vectors_restated(L, q_max, dq):
    """-> (hkl int32 [K, 3] ascending, |k| float64 [K], bin int32 [K])"""
    hkl, k2 = box_candidates(L, q_max)
    m = half_space(hkl) & (k2 < q_max * q_max)
    ka = np.sqrt(k2[m])
    nbins = int(np.ceil(q_max / dq))
    return hkl[m].astype(np.int32), ka, np.minimum(np.floor(ka / dq), nbins - 1).astype(np.int32)


def cell_gap_ok(L, q_max, dq, gap=1e-9):
    """condition 2, over a box two wider than the bound"""
    hkl, k2 = box_candidates(L, q_max, extra=2)
    ka = np.sqrt(k2[half_space(hkl)])
    near = ka[ka < q_max * (1 + 1e-6) + dq]
    edge = np.round(near / dq) * dq
    return bool(np.all(np.abs(near - q_max) > gap * near) and np.all(np.abs(near - edge) > gap * near))


def wrap(frac):
    w = np.asarray(frac, dtype=np.float64) - np.floor(frac)
    return np.where(w < 1.0, w, 0.0)


def rho_restated(frac, types, A, hkl):
    """-> complex128 [K, A]"""
    w, f = wrap(frac), hkl.astype(np.float64)
    out = np.zeros((len(hkl), A), dtype=np.complex128)
    for v0 in range(0, len(hkl), 4096):
        fv = f[v0:v0 + 4096]
        t = (fv[:, 0:1] * w[None, :, 0] + fv[:, 1:2] * w[None, :, 1]) + fv[:, 2:3] * w[None, :, 2]
        e = np.exp(-1j * TWO_PI * (t - np.floor(t)))
        for a in range(A):
            out[v0:v0 + 4096, a] = e[:, np.asarray(types) == a].sum(1)
    return out


def shells_restated(ka, bins, rho, nbins):
    """-> (count int64 [nbins] over the full sphere, mean |k| [nbins], mean Re(rho_a rho_b*) [A, A, nbins]); NaN where empty"""
    A = rho.shape[1]
    half = np.bincount(bins, minlength=nbins).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_k = np.bincount(bins, weights=ka, minlength=nbins) / half
        s = np.zeros((A, A, nbins))
        for a in range(A):
            for b in range(A):
                s[a, b] = np.bincount(bins, weights=(rho[:, a] * np.conj(rho[:, b])).real, minlength=nbins) / half
    return (2 * half).astype(np.int64), mean_k, s


def cell_dict(lattice, frac, types, name, A=2):
    return dict(lattice=np.asarray(lattice, dtype=np.float64).reshape(3, 3), frac=np.asarray(frac, dtype=np.float64).reshape(-1, 3),
                types=np.asarray(types, dtype=np.int32), A=A, name=name)


def simple_cubic_supercell(a=2.5, reps=4):
    g = np.arange(reps) / reps
    frac = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return cell_dict(a * reps * np.eye(3), frac, np.zeros(len(frac), dtype=np.int32), "sc-supercell", A=1)


# ---- the host statement through ctypes -----------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_debye(lib, pos, types, sizes, A, q, r_max=None, window=None, raw=False):
    """egnn_sq_host on clusters -> float64 [B, A, A, Q] (``raw``: (rc, out))"""
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    types = np.ascontiguousarray(types, dtype=np.int32)
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    gp = np.zeros(len(sizes) + 1, dtype=np.int32)
    gp[1:] = np.cumsum(sizes)
    out = np.full((len(sizes), A, A, q.size), -7.0)
    pad = np.zeros(3, dtype=np.float32)
    rc = lib.egnn_sq_host(len(sizes), len(types), A, _p(pos if len(pos) else pad), _p(types if len(types) else np.zeros(1, np.int32)), _p(gp),
                          q.size, _p(q), float("inf") if r_max is None else float(r_max), {None: 0, "lorch": 1}[window], _p(out), 0, 0, 0,
                          None, None, None, None, 0.0, 0.0, 0, 0, None, None, None, None, None, None, None, None)
    if raw:
        return rc, out
    assert rc == 0, lib.egnn_last_error()
    return out


def host_cells(lib, cells, q_max, dq, A=None, raw=False):
    """egnn_sq_host on cells (two calls: sizes, then lists) -> dict(vec_ptr, hkl, k, bin, rho complex [K, A], count, mean_k, s)"""
    A = max(c["A"] for c in cells) if A is None else A
    cell_ptr = np.zeros(len(cells) + 1, dtype=np.int32)
    cell_ptr[1:] = np.cumsum([len(c["types"]) for c in cells])
    lattice = np.ascontiguousarray(np.stack([c["lattice"].reshape(9) for c in cells]))
    frac = np.ascontiguousarray(np.concatenate([c["frac"] for c in cells]))
    types = np.ascontiguousarray(np.concatenate([c["types"] for c in cells]).astype(np.int32))
    nbins = int(np.ceil(q_max / dq)) if dq > 0 and np.isfinite(q_max / dq) else 1
    vec_ptr = np.zeros(len(cells) + 1, dtype=np.int64)

    def call(cap, hkl, ka, bn, rho, count, mean_k, s):
        return lib.egnn_sq_host(0, 0, 0, None, None, None, 0, None, 0.0, 0, None, len(cells), len(types), A, _p(cell_ptr), _p(lattice),
                                _p(frac if len(frac) else np.zeros((1, 3))), _p(types if len(types) else np.zeros(1, np.int32)),
                                float(q_max), float(dq), nbins, cap, _p(vec_ptr), _p(hkl), _p(ka), _p(bn), _p(rho), _p(count), _p(mean_k), _p(s))

    rc = call(0, None, None, None, None, None, None, None)
    if raw:
        return rc
    assert rc == 0, lib.egnn_last_error()
    K = int(vec_ptr[-1])
    hkl, ka, bn = np.full((K, 3), -7, np.int32), np.full(K, -7.0), np.full(K, -7, np.int32)
    rho = np.full((K, A, 2), -7.0)
    count, mean_k = np.full((len(cells), nbins), -7, np.int64), np.full((len(cells), nbins), -7.0)
    s = np.full((len(cells), A, A, nbins), -7.0)
    assert call(K, hkl, ka, bn, rho, count, mean_k, s) == 0, lib.egnn_last_error()
    return dict(vec_ptr=vec_ptr.copy(), hkl=hkl, k=ka, bin=bn, rho=rho[..., 0] + 1j * rho[..., 1], count=count, mean_k=mean_k, s=s, nbins=nbins)


# ---- the golden ----------------------------------------------------------------------------------------------------------------------
def golden_inputs():
    """the inputs of tests/golden/sq_golden.npz (stored there too; the tests read the stored ones)"""
    clusters = {}
    sizes = [1, 2, 3, 65]
    parts = [cloud(n, 100 + n) for n in sizes]
    pos, types = np.concatenate([p for p, _ in parts]), np.concatenate([t for _, t in parts])
    types[3:6] = 0                                  # the 3-atom graph lacks type 1
    clusters["ragged"] = dict(pos=pos, types=types, sizes=sizes, r_max=np.inf, window=0)
    p, t = cloud(6, 7)
    p[4] = p[1]                                      # a coincident pair
    clusters["coincident"] = dict(pos=p, types=t, sizes=[6], r_max=np.inf, window=0)
    p, t = cloud(65, 11)
    clusters["lorch"] = dict(pos=p, types=t, sizes=[65], r_max=5.0, window=1)
    from tests import _cells_util as CU
    tri = CU.triclinic_cell(check=False)
    cells = dict(triclinic=cell_dict(tri["lattice"], tri["frac"], tri["types"], "triclinic"),
                 pair=cell_dict(3.2 * np.eye(3), [[0.1, 0.2, 0.3], [0.6, 0.15, 0.35]], [1, 0], "pair"))
    return clusters, cells, dict(q_max=6.0, dq=0.25)


def golden():
    return dict(np.load(GOLDEN))


def golden_cluster(G, name):
    c = dict(pos=G[f"{name}_pos"], types=G[f"{name}_types"], sizes=[int(v) for v in G[f"{name}_sizes"]], truth=G[f"{name}_debye"],
             r_max=None if np.isinf(G[f"{name}_r_max"]) else float(G[f"{name}_r_max"]), window="lorch" if int(G[f"{name}_window"]) else None)
    assert debye_gap_ok(c["pos"], c["sizes"], c["r_max"]), name
    return c


def golden_cell(G, name):
    c = cell_dict(G[f"{name}_lattice"], G[f"{name}_frac"], G[f"{name}_types"], name)
    c.update(hkl=G[f"{name}_hkl"], k=G[f"{name}_k"], rho=G[f"{name}_rho"], s=G[f"{name}_s"], q_max=float(G["q_max"]), dq=float(G["dq"]))
    assert cell_gap_ok(c["lattice"], c["q_max"], c["dq"]), name
    return c


def rho_error(rho, truth, n_type):
    """max |rho_a - truth| / sqrt(N_a) (an absent type must be exactly zero)"""
    n = np.asarray(n_type, dtype=np.float64)
    assert np.all(rho[:, n == 0] == 0)
    return float((np.abs(rho - truth) / np.sqrt(np.where(n == 0, 1.0, n))[None, :]).max()) if rho.size else 0.0


def shell_error(s, truth, n_type):
    """max over the shells with vectors of |S_ab - S_truth| / (sqrt(N_a) + sqrt(N_b)), S_ab = s_ab / sqrt(N_a N_b), present types"""
    n = np.asarray(n_type, dtype=np.float64)
    worst = 0.0
    for a in range(len(n)):
        for b in range(len(n)):
            if n[a] * n[b] == 0:
                continue
            ok = ~np.isnan(truth[a, b])
            assert np.array_equal(np.isnan(s[a, b]), ~ok)
            if ok.any():
                worst = max(worst, float(np.abs(s[a, b][ok] - truth[a, b][ok]).max() / np.sqrt(n[a] * n[b]) / (np.sqrt(n[a]) + np.sqrt(n[b]))))
    return worst

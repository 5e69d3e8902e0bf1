"""Numpy restatement, written from reading, of the real-space statistics of periodic cells (csrc/cells/cell_stats_math.h), shared by
the CPU and GPU tests and by tools/cell_stats_time.py (test infrastructure).  float64 throughout, in the library's operation order
(site vector of tests/_cells_util.py, r2 = (x x + y y) + z z, r = sqrt(r2), k = floor(r / dR)), and WITHOUT any of the library's
culls: every atom pair and every image of the box is evaluated.

  pair_counts      c[a, b, k] over ordered (i, (j, s)), (j, s) != (i, 0), |s_k| <= S_k = ceil(nbins dR / w_k)
  bond_statistics  coordination, CN histogram, angles (p < q in row order, at most 64 bonds), Q^n, from the restated bond list
  finish           g, n, total (and the smoothing filter) from the counts
  host             egnn_cell_stats_host on a batch of cell dicts
"""
import ctypes as C
import itertools

import numpy as np

from tests import _cells_util as CU

MAX_NEIGHBOURS = 64
NEUTRON_LENGTHS = (5.803, 4.1491)


def nbins_of(R, dR):
    return int(np.floor(R / dR + 0.5))


def image_box(L, dR, nbins):
    return np.ceil(nbins * dR / CU.widths(np.asarray(L, dtype=np.float64))).astype(np.int64)


def pair_counts(cell, dR, nbins, A=None, box=None):
    """-> int64 [A, A, nbins]; ``box`` overrides the image box (a larger one must give the same counts)"""
    L, w, types = np.asarray(cell["lattice"], np.float64), CU.wrap(cell["frac"]), np.asarray(cell["types"], np.int64)
    A = cell["A"] if A is None else A
    n = len(w)
    S = image_box(L, dR, nbins) if box is None else np.asarray(box)
    images = np.array(list(itertools.product(*(range(-int(s), int(s) + 1) for s in S))), dtype=np.int64)
    zero = int(np.nonzero(~images.any(1))[0][0])
    out = np.zeros(A * A * nbins, dtype=np.int64)
    step = max(1, int(4e6 // max(n * len(images), 1)))
    for i0 in range(0, n, step):
        wi = w[i0:i0 + step]
        r = CU.site_vectors(w[None, :, None, :], wi[:, None, None, :], images[None, None, :, :], L)      # [c, n, images, 3]
        r2 = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
        k = np.floor(np.sqrt(r2) / dR)
        ok = k < nbins
        ci = np.arange(len(wi))
        ok[ci, i0 + ci, zero] = False
        c, j, _ = np.nonzero(ok)
        flat = (types[i0 + c] * A + types[j]) * nbins + k[ok].astype(np.int64)
        out += np.bincount(flat, minlength=A * A * nbins)
    return out.reshape(A, A, nbins)


def batch_pair_counts(cells, dR, nbins, A=None):
    A = max(c["A"] for c in cells) if A is None else A
    return np.stack([pair_counts(c, dR, nbins, A=A) for c in cells])


def angle_bins(dtheta):
    return int(np.floor(180.0 / dtheta + 0.5)) + 1


def pair_index(b, c, A):
    lo, hi = min(b, c), max(b, c)
    return lo * A - lo * (lo - 1) // 2 + (hi - lo)


def bond_statistics(cell, dtheta=1.0, max_cn=16, former=1, bridge=0, A=None):
    """from cell["bonds"] (the restated bond list of the cell's cutoff) -> dict(coordination int32 [n, A], cn int64 [A, A, max_cn+1],
    angles int64 [A, P, nth], qn int32 [n], qn_hist int64 [max_cn+1], overflow int, degree int64 [n])"""
    L, w, types = np.asarray(cell["lattice"], np.float64), CU.wrap(cell["frac"]), np.asarray(cell["types"], np.int64)
    A = cell["A"] if A is None else A
    n = len(w)
    row_ptr, atom, code, _ = cell["bonds"]
    shift = CU.shift_decode(code)
    nth, P, ncn = angle_bins(dtheta), A * (A + 1) // 2, max_cn + 1
    coordination = np.zeros((n, A), dtype=np.int32)
    cn, ang = np.zeros((A, A, ncn), dtype=np.int64), np.zeros((A, P, nth), dtype=np.int64)
    overflow = 0
    for i in range(n):
        e0, e1 = int(row_ptr[i]), int(row_ptr[i + 1])
        tj = types[atom[e0:e1]]
        coordination[i] = np.bincount(tj, minlength=A)
        for b in range(A):
            cn[types[i], b, min(int(coordination[i, b]), max_cn)] += 1
        m = e1 - e0
        if m > MAX_NEIGHBOURS:
            overflow += 1
            continue
        if m < 2:
            continue
        v = CU.site_vectors(w[atom[e0:e1]], w[i], shift[e0:e1], L)
        vv = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        p, q = np.triu_indices(m, 1)
        vw = (v[p, 0] * v[q, 0] + v[p, 1] * v[q, 1]) + v[p, 2] * v[q, 2]
        ok = (vv[p] > 0) & (vv[q] > 0)
        cosv = np.clip(vw[ok] / (np.sqrt(vv[p][ok]) * np.sqrt(vv[q][ok])), -1.0, 1.0)
        k = np.minimum(np.floor(np.arccos(cosv) * (180.0 / np.pi) / dtheta + 0.5).astype(np.int64), nth - 1)
        pi = np.array([pair_index(int(a), int(b), A) for a, b in zip(tj[p][ok], tj[q][ok])], dtype=np.int64)
        np.add.at(ang[types[i]], (pi, k), 1)
    qn = np.full(n, -1, dtype=np.int32)
    qn_hist = np.zeros(ncn, dtype=np.int64)
    for i in np.nonzero(types == former)[0]:
        nb = atom[row_ptr[i]:row_ptr[i + 1]]
        q = int(np.sum((types[nb] == bridge) & (coordination[nb, former] >= 2)))
        qn[i] = q
        qn_hist[min(q, max_cn)] += 1
    return dict(coordination=coordination, cn=cn, angles=ang, qn=qn, qn_hist=qn_hist, overflow=overflow, degree=np.diff(row_ptr))


def batch_bond_statistics(cells, A=None, **kw):
    A = max(c["A"] for c in cells) if A is None else A
    parts = [bond_statistics(c, A=A, **kw) for c in cells]
    return dict(coordination=np.concatenate([p["coordination"] for p in parts]), qn=np.concatenate([p["qn"] for p in parts]),
                cn=np.stack([p["cn"] for p in parts]), angles=np.stack([p["angles"] for p in parts]),
                qn_hist=np.stack([p["qn_hist"] for p in parts]), overflow=np.array([p["overflow"] for p in parts], dtype=np.int32))


def smooth(g, sigma):
    """gaussian_filter1d(mode='reflect', truncate=4) along the last axis, as struct_smooth_* spells it"""
    nbins = g.shape[-1]
    lw = int(4.0 * sigma + 0.5)
    k = np.arange(nbins)
    acc, wsum = np.zeros_like(g), 0.0
    for t in range(-lw, lw + 1):
        wt = np.exp(-0.5 * float(t) * t / (sigma * sigma))
        idx = np.mod(k + t, 2 * nbins)
        idx = np.where(idx >= nbins, 2 * nbins - 1 - idx, idx)
        acc = acc + g[..., idx] * wt
        wsum += wt
    return acc / wsum


def finish(cells, counts, dR, sigma=0.0, weights=None):
    """counts int64 [C, A, A, nbins] -> dict(r, g, n, total, n_type, volume) in float64"""
    Cn, A, _, nbins = counts.shape
    wt = np.asarray((NEUTRON_LENGTHS if A == 2 else (1.0,) * A) if weights is None else weights, dtype=np.float64)
    n_type = np.stack([np.bincount(np.asarray(c["types"], np.int64), minlength=A)[:A] for c in cells]).astype(np.float64)
    volume = np.array([abs(np.linalg.det(np.asarray(c["lattice"], np.float64))) for c in cells])
    k = np.arange(nbins, dtype=np.float64)
    shell = (4.0 * np.pi / 3.0) * ((k + 1.0) ** 3 - k ** 3) * dR ** 3
    g, n = np.zeros(counts.shape), np.zeros(counts.shape)
    for c in range(Cn):
        for a in range(A):
            if n_type[c, a] > 0:
                n[c, a] = np.cumsum(counts[c, a].astype(np.float64), -1) / n_type[c, a]
            for b in range(A):
                if n_type[c, a] > 0 and n_type[c, b] > 0:
                    g[c, a, b] = volume[c] * counts[c, a, b] / (n_type[c, a] * n_type[c, b] * shell)
    if sigma > 0:
        g = smooth(g, sigma)
    cw = n_type / n_type.sum(1, keepdims=True) * wt
    total = (cw[:, :, None, None] * cw[:, None, :, None] * g).sum((1, 2)) / (cw.sum(1) ** 2)[:, None]
    return dict(r=(k + 0.5) * dR, g=g, n=n, total=total, n_type=n_type.astype(np.int64), volume=volume)


def batch_arrays(cells):
    sizes = [len(c["frac"]) for c in cells]
    return dict(cell_ptr=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                lattice=np.ascontiguousarray(np.stack([np.asarray(c["lattice"], np.float64).reshape(9) for c in cells])),
                frac=np.ascontiguousarray(np.concatenate([np.asarray(c["frac"], np.float64).reshape(-1, 3) for c in cells])),
                type=np.ascontiguousarray(np.concatenate([np.asarray(c["types"]) for c in cells]).astype(np.int32)))


def host(lib, cells, dR=0.01, nbins=1000, cutoff=CU.CUTOFF, dtheta=1.0, max_cn=16, former=1, bridge=0, A=None, pairs=True, bonds=True,
         raw=None):
    """egnn_cell_stats_host on a batch of cell dicts -> (rc, dict).  Every output starts at -7: the statement writes all of them.
    ``raw`` overrides input arrays by name for the argument tests."""
    a = batch_arrays(cells)
    a.update(raw or {})
    Cn, N = len(cells), int(a["cell_ptr"][-1])
    A = max(c["A"] for c in cells) if A is None else A
    nth, P, ncn = (angle_bins(dtheta) if dtheta >= 0.5 else 1), A * (A + 1) // 2, max(max_cn, 0) + 1
    out = dict(counts=np.full((Cn, A, A, max(nbins, 1)), -7, np.int64), coordination=np.full((max(N, 1), A), -7, np.int32)[:N],
               cn=np.full((Cn, A, A, ncn), -7, np.int64), angles=np.full((Cn, A, P, nth), -7, np.int64), qn=np.full(max(N, 1), -7, np.int32)[:N],
               qn_hist=np.full((Cn, ncn), -7, np.int64), overflow=np.full(Cn, -7, np.int32))
    vp = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
    names = ("coordination", "cn", "angles", "qn", "qn_hist", "overflow")
    rc = lib.egnn_cell_stats_host(Cn, A, vp(a["cell_ptr"]), vp(a["lattice"]), vp(a["frac"]), vp(a["type"]), float(dR), int(nbins),
                                  vp(out["counts"]) if pairs else None, float(cutoff), float(dtheta), int(max_cn), int(former), int(bridge),
                                  *((vp(out[k]) if bonds else None) for k in names))
    if not pairs:
        out.pop("counts")
    if not bonds:
        for k in names:
            out.pop(k)
    return rc, out

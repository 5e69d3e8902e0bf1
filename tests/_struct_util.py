"""Numpy restatement of the whole-structure statistics (csrc/eval/structure_math.h), shared by the CPU and GPU tests and by the
fixture generator (test infrastructure).

  * distance: float32 in the fixed order sqrt((dx*dx + dy*dy) + dz*dz), dx = p_j.x - p_i.x: numpy's float32 arithmetic rounds
    every operation, so this is bitwise what the library computes (built with -ffp-contract=off);
  * radial bin k holds d iff float32(dR + k dR) < d < float32(dR + k dR + dR), edges in float64 first (rdf_kernel's rule);
  * bond iff d < float32(cutoff); angle in float64 from the float32 positions, bin floor(theta/dtheta + 0.5).
and the two gap conditions under which integer outputs can be compared EXACTLY:
  1. no distance within 4 float32 ulp of a bin edge or of the cutoff (radial_gap_ok);
  2. no angle within 1e-9 degrees of an angle-bin edge (angle_gap).
"""
import numpy as np

MAX_NEIGHBOURS = 64   # kMaxNeighbours


def nbins_of(R, dR):
    return len(np.arange(0 + dR, R + dR, dR))


def n_angle_bins(dtheta):
    return int(np.floor(180.0 / dtheta + 0.5)) + 1


def pair_index(b, c, A):
    lo, hi = min(b, c), max(b, c)
    return lo * A - lo * (lo - 1) // 2 + (hi - lo)


def distances(pos):
    """float32 [n,3] -> float32 [n,n], d[i,j] from dx = p_j - p_i in the fixed order"""
    pos = np.asarray(pos, dtype=np.float32)
    d = pos[None, :, :] - pos[:, None, :]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    out = np.sqrt((dx * dx + dy * dy) + dz * dz)
    assert out.dtype == np.float32
    return out


def bin_edges(dR, nbins):
    k = np.arange(nbins).astype(np.float64)
    rk = dR + k * dR
    return rk.astype(np.float32), (rk + dR).astype(np.float32)


def radial_bins(d, dR, nbins):
    """float32 distances (any shape) -> (first, second) int arrays: the bins that hold each distance, -1 for none.  Two bins can
    hold one distance only where rounding makes float32(r_k + dR) exceed float32(r_{k+1}); the rule counts it in both."""
    lo, hi = bin_edges(dR, nbins)
    assert np.all(np.diff(lo) >= 0)
    d = np.asarray(d, dtype=np.float32)
    out = []
    top = np.searchsorted(lo, d, side="left") - 1          # the last bin whose lower edge lies below d
    for k in (top, top - 1):
        kk = np.clip(k, 0, nbins - 1)
        ok = (k >= 0) & (k < nbins) & (lo[kk] < d) & (d < hi[kk])
        out.append(np.where(ok, k, -1))
    return out[0], out[1]


def _ordered(x):
    """float32 >= 0 -> int64 that counts ulps"""
    return np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)


def radial_gap_ok(d, settings, cutoff, ulps=4):
    """condition 1 for the distances ``d`` (float32, all finite and positive): none within ``ulps`` float32 steps of a bin edge of
    any (R, dR) of ``settings`` or of the cutoff"""
    marks = [np.array([cutoff], dtype=np.float32)]
    for R, dR in settings:
        lo, hi = bin_edges(dR, nbins_of(R, dR))
        marks += [lo, hi]
    marks = np.unique(_ordered(np.concatenate(marks)))
    v = _ordered(np.asarray(d, dtype=np.float32).reshape(-1))
    at = np.searchsorted(marks, v)
    below = np.abs(v - marks[np.clip(at - 1, 0, len(marks) - 1)])
    above = np.abs(v - marks[np.clip(at, 0, len(marks) - 1)])
    return bool(np.all(np.minimum(below, above) > ulps))


def pair_counts(pos, types, A, R, dR):
    """one graph -> int64 [A, A, nbins]"""
    nbins = nbins_of(R, dR)
    n = len(pos)
    c = np.zeros((A, A, nbins), dtype=np.int64)
    if n < 2:
        return c
    d = distances(pos)
    off = ~np.eye(n, dtype=bool)
    ti = np.broadcast_to(np.asarray(types)[:, None], (n, n))[off]
    tj = np.broadcast_to(np.asarray(types)[None, :], (n, n))[off]
    for k in radial_bins(d[off], dR, nbins):
        keep = k >= 0
        np.add.at(c, (ti[keep], tj[keep], k[keep]), 1)
    return c


def bonded_angles(pos, types, cutoff):
    """one graph -> list of (centre, j, k, theta in degrees, float64) over every centre and bonded neighbours j < k with non-zero
    bond vectors, and the bond matrix; centres above MAX_NEIGHBOURS bonds are left out (and listed)"""
    pos = np.asarray(pos, dtype=np.float32)
    n = len(pos)
    bond = (distances(pos) < np.float32(cutoff)) & ~np.eye(n, dtype=bool)
    rows, over = [], []
    for i in range(n):
        nb = np.nonzero(bond[i])[0]
        if len(nb) > MAX_NEIGHBOURS:
            over.append(i)
            continue
        if len(nb) < 2:
            continue
        v = pos[nb].astype(np.float64) - pos[i].astype(np.float64)
        a, b = np.triu_indices(len(nb), 1)
        va, vb = v[a], v[b]
        vv = (va[:, 0] * va[:, 0] + va[:, 1] * va[:, 1]) + va[:, 2] * va[:, 2]
        ww = (vb[:, 0] * vb[:, 0] + vb[:, 1] * vb[:, 1]) + vb[:, 2] * vb[:, 2]
        vw = (va[:, 0] * vb[:, 0] + va[:, 1] * vb[:, 1]) + va[:, 2] * vb[:, 2]
        ok = (vv > 0) & (ww > 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            c = np.clip(vw / (np.sqrt(vv) * np.sqrt(ww)), -1.0, 1.0)
        theta = np.arccos(c) * (180.0 / np.pi)
        for t in np.nonzero(ok)[0]:
            rows.append((i, int(nb[a[t]]), int(nb[b[t]]), float(theta[t])))
    return rows, bond, over


def angle_gap(thetas, dtheta):
    """condition 2: the smallest distance, in degrees, of an angle to an edge of the centred bins (inf without angles)"""
    t = np.asarray(thetas, dtype=np.float64) / dtheta + 0.5
    return float(np.min(np.abs(t - np.round(t))) * dtheta) if t.size else float("inf")


def bond_statistics(pos, types, A, cutoff, dtheta, max_cn):
    """one graph -> (cn int64 [A, A, max_cn+1], angles int64 [A, A(A+1)/2, nth], overflow, thetas)"""
    types = np.asarray(types)
    nth = n_angle_bins(dtheta)
    cn = np.zeros((A, A, max_cn + 1), dtype=np.int64)
    ang = np.zeros((A, A * (A + 1) // 2, nth), dtype=np.int64)
    rows, bond, over = bonded_angles(pos, types, cutoff)
    for i in range(len(types)):
        for b in range(A):
            cn[types[i], b, min(int((bond[i] & (types == b)).sum()), max_cn)] += 1
    for i, j, k, theta in rows:
        ang[types[i], pair_index(int(types[j]), int(types[k]), A), min(int(np.floor(theta / dtheta + 0.5)), nth - 1)] += 1
    return cn, ang, len(over), np.array([r[3] for r in rows])


def batch_statistics(pos, types, sizes, A, R=5.0, dR=0.01, cutoff=2.0, dtheta=1.0, max_cn=16):
    """a ragged batch -> (counts [B,A,A,nbins], cn [B,A,A,max_cn+1], angles [B,A,P,nth], overflow [B], smallest angle gap)"""
    c, n_, a_, o_, gap, lo = [], [], [], [], float("inf"), 0
    for n in sizes:
        p, t = pos[lo:lo + n], types[lo:lo + n]
        lo += n
        c.append(pair_counts(p, t, A, R, dR))
        cn, ang, over, thetas = bond_statistics(p, t, A, cutoff, dtheta, max_cn)
        n_.append(cn); a_.append(ang); o_.append(over)
        gap = min(gap, angle_gap(thetas, dtheta))
    return np.stack(c), np.stack(n_), np.stack(a_), np.array(o_), gap


def gaussian_filter_reflect(raw, sigma):
    """scipy.ndimage.gaussian_filter1d(raw, sigma) (reflect boundary, truncate 4 sigma), restated in float64"""
    raw = np.asarray(raw, dtype=np.float64)
    n = raw.shape[-1]
    lw = int(4.0 * sigma + 0.5)
    t = np.arange(-lw, lw + 1)
    w = np.exp(-0.5 * t.astype(np.float64) ** 2 / (sigma * sigma))
    w /= w.sum()
    idx = (np.arange(n)[:, None] + t[None, :]) % (2 * n)
    idx = np.where(idx >= n, 2 * n - 1 - idx, idx)
    return (raw[..., idx] * w).sum(-1)


def partial_rdf(counts, n_type, n, sigma, R, dR):
    """counts [A,A,nbins] of one graph of n atoms, n_type [A] -> g_ab float64 [A,A,nbins]"""
    nbins = counts.shape[-1]
    rk = dR + np.arange(nbins).astype(np.float64) * dR
    rho = n / (4 / 3 * np.pi * R ** 3)
    raw = counts.astype(np.float64) / np.maximum(np.asarray(n_type), 1)[:, None, None] / (4 * np.pi * rho * rk ** 2 * dR)
    return gaussian_filter_reflect(raw, sigma)


def random_batch(seed, sizes, A, box_per_atom=3.0):
    """seeded uniform positions, each graph in a box of volume box_per_atom^3 per atom (so that at cutoff 2.0 a centre has a few
    bonds, far from the cap of 64), float32, and uniform types"""
    rng = np.random.default_rng(seed)
    pos = np.concatenate([rng.uniform(0.0, box_per_atom * max(n, 1) ** (1 / 3), (n, 3)) for n in sizes]).astype(np.float32)
    types = rng.integers(0, A, sum(sizes)).astype(np.int32)
    return pos, types


def host_counts(lib, pos, types, sizes, A, R=5.0, dR=0.01, cutoff=2.0, dtheta=1.0, max_cn=16):
    """egnn_struct_counts_host on a ragged batch -> (rc, counts, cn, angles, overflow)"""
    import ctypes as C
    B, nbins, nth = len(sizes), nbins_of(R, dR), n_angle_bins(dtheta)
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    types = np.ascontiguousarray(types, dtype=np.int32)
    counts = np.full((B, A, A, max(nbins, 1)), -7, dtype=np.int32)
    cn = np.full((B, A, A, max(max_cn, 0) + 1), -7, dtype=np.int32)
    ang = np.full((B, A, A * (A + 1) // 2, max(min(nth, 4000), 1)), -7, dtype=np.int32)
    over = np.full(B, -7, dtype=np.int32)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    rc = lib.egnn_struct_counts_host(B, A, vp(pos), vp(types), vp(gp), float(dR), nbins, float(cutoff), float(dtheta), int(max_cn),
                                     vp(counts), vp(cn), vp(ang), vp(over))
    return rc, counts, cn, ang, over

"""Numpy restatement of the topological fingerprint (csrc/eval/topo_math.h), shared by the CPU and GPU tests (test
infrastructure), and the inputs both use.

  * bond: i != j bonded iff d < thr[type i, type j], d = sqrt((dx*dx + dy*dy) + dz*dz) in float64 from the float32 positions
    (numpy rounds every operation and float64 sqrt is correctly rounded, so the decision is the library's wherever the gap
    condition holds), thr = scale * (radius_a + radius_b) in float64;
  * bond lists: row i = the first min(degree, 32) neighbours ascending, row_ptr their prefix sum, degree the full count;
    a graph with an atom above 32 bonds overflows: distances 0xFFFF, components -1, fragments -1, fingerprint 0;
  * hop distance by repeated boolean frontier expansion, 0xFFFF = unreachable;
  * class = type * 7 + degree % 7; key = pair_index(c_lo, c_hi) * L + d - 1 for i < j, 1 <= d <= L; np.add.at;
  * Tanimoto in Python ints, one float division, 0.0 on a zero denominator.
Gap condition (gap_ok): no pair distance within 1e-9 (relative) of its threshold.  Every test asserts it for its inputs.
"""
import ctypes as C

import numpy as np

MAX_DEGREE, MODULUS, UNREACHABLE = 32, 7, 0xFFFF
RADII = {1: (1.11,), 2: (0.66, 1.11), 3: (0.66, 1.11, 1.21)}   # (O, Si[, Al]); one type: Si alone
SIZES = [1, 2, 3, 63, 64, 65, 129, 257, 7]


def thresholds(radii, scale=1.2):
    r = np.asarray(radii, dtype=np.float64)
    return scale * (r[:, None] + r[None, :])


def n_keys(A, L):
    Cn = MODULUS * A
    return Cn * (Cn + 1) // 2 * L


def pair_index(c1, c2, Cn):
    lo, hi = np.minimum(c1, c2), np.maximum(c1, c2)
    return lo * Cn - lo * (lo - 1) // 2 + (hi - lo)


def distances(pos):
    p = np.asarray(pos, dtype=np.float32).astype(np.float64)
    d = p[None, :, :] - p[:, None, :]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def gap_ok(pos, types, thr, rel=1e-9):
    n = len(pos)
    if n < 2:
        return True
    t = thr[np.asarray(types)[:, None], np.asarray(types)[None, :]]
    off = ~np.eye(n, dtype=bool)
    return bool(np.all(np.abs(distances(pos) - t)[off] > rel * t[off]))


def bond_matrix(pos, types, thr):
    n = len(pos)
    t = thr[np.asarray(types)[:, None], np.asarray(types)[None, :]].reshape(n, n)
    return (distances(pos).reshape(n, n) < t) & ~np.eye(n, dtype=bool)


def hop_distances(bond):
    """all searches at once: the frontier is the list of (source, atom) pairs of one level, ``seen`` the boolean matrix of the
    pairs of all earlier levels; a level's work is the size of its frontier (a 1024-atom chain has 1023 levels of two atoms)"""
    n = len(bond)
    dist = np.full((n, n), UNREACHABLE, dtype=np.int64)
    seen = np.eye(n, dtype=bool)
    deg = bond.sum(1)
    first = np.cumsum(deg) - deg
    flat = np.nonzero(bond)[1]                 # the neighbours of atom 0, then of atom 1, ...
    src = at = np.arange(n)
    level = 0
    while len(src):
        dist[src, at] = level
        level += 1
        cnt = deg[at]
        step = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        s2, a2 = np.repeat(src, cnt), flat[np.repeat(first[at], cnt) + step]
        key = np.unique((s2 * n + a2)[~seen[s2, a2]])
        seen.reshape(-1)[key] = True
        src, at = key // n, key % n
    return dist


def fingerprint(dist, types, degree, A, L):
    n = len(dist)
    cls = np.asarray(types, dtype=np.int64) * MODULUS + np.asarray(degree, dtype=np.int64) % MODULUS
    fp = np.zeros(n_keys(A, L), dtype=np.int64)
    i, j = np.triu_indices(n, 1)
    d = dist[i, j]
    keep = (d >= 1) & (d <= L)
    np.add.at(fp, pair_index(cls[i[keep]], cls[j[keep]], MODULUS * A) * L + (d[keep] - 1), 1)
    return fp


def tanimoto(a, b):
    a, b = [int(v) for v in a], [int(v) for v in b]
    both, sa, sb = sum(min(x, y) for x, y in zip(a, b)), sum(a), sum(b)
    den = sa + sb - both
    return (both / den if den else 0.0), sa, sb


def batch(pos, types, sizes, A, thr, L=30):
    """a ragged batch -> dict of every output in the layout of egnn_topo_host"""
    rp, nb, deg, over, dist, comp, frag, fps = [0], [], [], [], [], [], [], []
    lo = 0
    for n in sizes:
        p, t = pos[lo:lo + n], np.asarray(types[lo:lo + n])
        bond = bond_matrix(p, t, thr)
        d_full = bond.sum(1)
        for i in range(n):
            row = np.nonzero(bond[i])[0][:MAX_DEGREE]
            nb.append(row + lo)
            rp.append(rp[-1] + len(row))
        deg.append(d_full)
        over.append(int((d_full > MAX_DEGREE).sum()))
        if over[-1]:
            dist.append(np.full(n * n, UNREACHABLE, dtype=np.int64))
            comp.append(np.full(n, -1, dtype=np.int64))
            frag.append(-1)
            fps.append(np.zeros(n_keys(A, L), dtype=np.int64))
        else:
            d = hop_distances(bond)
            c = np.array([np.nonzero(d[i] != UNREACHABLE)[0][0] for i in range(n)], dtype=np.int64).reshape(n)
            dist.append(d.reshape(-1))
            comp.append(c + lo)
            frag.append(int((c == np.arange(n)).sum()))
            fps.append(fingerprint(d, t, d_full, A, L))
        lo += n
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, dtype=np.int64)
    return dict(row_ptr=np.array(rp), neighbours=cat(nb), degree=cat(deg), overflow=np.array(over), dist=cat(dist),
                component=cat(comp), fragments=np.array(frag), fp=np.stack(fps))


INT_KEYS = ("row_ptr", "neighbours", "degree", "overflow", "dist", "component", "fragments", "fp")


def host(lib, pos, types, sizes, A, thr, L=30, pairs=None, want=("dist", "component", "fragments", "fp")):
    """egnn_topo_host on a ragged batch -> (rc, dict of outputs in batch()'s layout plus sim, sa, sb)"""
    B, N = len(sizes), int(sum(sizes))
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    types = np.ascontiguousarray(types, dtype=np.int32)
    thr = np.ascontiguousarray(thr, dtype=np.float64)
    K = n_keys(min(max(A, 1), 4), min(max(L, 1), 64))
    o = dict(row_ptr=np.full(N + 1, -7, np.int32), neighbours=np.full(MAX_DEGREE * max(N, 1), -7, np.int32),
             degree=np.full(N, -7, np.int32), overflow=np.full(B, -7, np.int32),
             dist=np.full(int(sum(n * n for n in sizes)), 7, np.uint16), component=np.full(N, -7, np.int32),
             fragments=np.full(B, -7, np.int32), fp=np.full((B, K), -7, np.int32))
    pairs = np.zeros((0, 2), np.int32) if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    o.update(sim=np.full(len(pairs), -7.0), sa=np.full(len(pairs), -7, np.int64), sb=np.full(len(pairs), -7, np.int64))
    vp = lambda a: C.c_void_p(a.ctypes.data)
    opt = lambda k: vp(o[k]) if k in want else None
    rc = lib.egnn_topo_host(B, A, vp(pos), vp(types), vp(gp), vp(thr), int(L), vp(o["row_ptr"]), vp(o["neighbours"]), vp(o["degree"]),
                            vp(o["overflow"]), opt("dist"), opt("component"), opt("fragments"), opt("fp"), len(pairs),
                            vp(pairs) if len(pairs) else None, vp(o["sim"]), vp(o["sa"]), vp(o["sb"]))
    if rc == 0:
        o["neighbours"] = o["neighbours"][:o["row_ptr"][-1]]
    return rc, o


def assert_equal(got, want, keys=INT_KEYS):
    for k in keys:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), want[k]), k


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def cloud(seed, sizes, A, box_per_atom=2.5):
    """silica-like clouds: the generator of tests/_struct_util.py (uniform positions at a fixed density, uniform types)"""
    from tests._struct_util import random_batch
    return random_batch(seed, sizes, A, box_per_atom=box_per_atom)


def chain(n):
    """O-Si-O-Si-... zig-zag: 1.664 A between neighbours (< 2.124), 2.8 A between second neighbours (> 2.664)"""
    i = np.arange(n)
    return np.stack([1.4 * i, 0.9 * (i % 2), np.zeros(n)], 1).astype(np.float32), (i % 2).astype(np.int32)


def ring(k):
    """a regular k-gon: alternating O/Si with side 1.6 A for even k, all O with side 1.5 A for odd k"""
    side = 1.6 if k % 2 == 0 else 1.5
    r = side / (2 * np.sin(np.pi / k))
    a = 2 * np.pi * np.arange(k) / k + 0.1
    types = (np.arange(k) % 2 if k % 2 == 0 else np.zeros(k)).astype(np.int32)
    return np.stack([r * np.cos(a), r * np.sin(a), 0.3 * np.ones(k)], 1).astype(np.float32), types


def star(k):
    """Si with k <= 8 oxygens on the corners of a cube, 1.9 A away (corners 2.19 A apart: no O-O bond)"""
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * (1.9 / np.sqrt(3))
    return np.concatenate([np.zeros((1, 3)), corners[:k]]).astype(np.float32), np.array([1] + [0] * k, dtype=np.int32)


def crowd(n=34, seed=5):
    """n Si inside a cube of side 1.5 A (diagonal 2.6 < 2.664): everybody is bonded to everybody"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1.5, (n, 3)).astype(np.float32), np.ones(n, dtype=np.int32)


def two_fragments():
    a = np.array([[-1.6, 0, 0], [0, 0, 0], [1.6, 0, 0]])
    return np.concatenate([a, a + [0, 10, 0]]).astype(np.float32), np.array([0, 1, 0, 0, 1, 0], dtype=np.int32)


def bondless(n=5):
    return (5.0 * np.arange(n)[:, None] * np.ones((1, 3))).astype(np.float32), (np.arange(n) % 2).astype(np.int32)


def empty():
    """a graph of no atoms: no fragment, a zero fingerprint, and nothing else to write"""
    return np.zeros((0, 3), dtype=np.float32), np.zeros(0, dtype=np.int32)


def line(symbols, step=1.6):
    """atoms on a straight line, `step` apart: 'OSiO' -> O-Si-O (second neighbours 3.2 A apart: unbonded)"""
    types = np.array([{"O": 0, "S": 1}[s] for s in symbols.replace("Si", "S")], dtype=np.int32)
    return np.stack([step * np.arange(len(types)), np.zeros(len(types)), np.zeros(len(types))], 1).astype(np.float32), types


def special_graphs():
    """name -> (pos, types): the hand-made graphs of the host test, A = 2"""
    return {"chain1024": chain(1024), "ring6": ring(6), "ring5": ring(5), "fragments": two_fragments(), "star6": star(6),
            "star7": star(7), "star8": star(8), "crowd34": crowd(34), "bondless": bondless(), "empty": empty()}


def join(graphs):
    """[(pos, types)] -> (pos, types, sizes)"""
    return np.concatenate([g[0] for g in graphs]), np.concatenate([g[1] for g in graphs]), [len(g[1]) for g in graphs]

"""Restatements of the shortest-path ring statistics, written from the definition (csrc/eval/rings_math.h states it), shared by
the CPU and GPU tests and by tools/rings_time.py (test infrastructure):

  (i)   ``search`` / ``restated``: a pure-Python level-by-level search over sites (atom, sx, sy, sz) with dicts: one search per
        (centre, row position p) from site row[p] with the site (centre, 0) removed, targets row[q], q > p; a new site's path
        count is the sum of the counts of its neighbours one level below, cut at 2^31 - 1; a search that labels more than
        max_sites sites, or a centre above 32 bonds, gives size -1, count 0 and overflow 1;
  (ii)  ``independent``: the ball of max_size // 2 bonds about the centre as an explicit graph with the centre removed; size - 2
        from scipy.sparse.csgraph.shortest_path, count from the integer adjacency-matrix power A^(size - 2) in int64 (walks of
        shortest length are paths).  A shortest closing path of size <= max_size lies inside that ball: a site i bonds along it
        from j is at most min(i, size - 2 - i) + 1 <= max_size // 2 bonds from the centre;
  (iii) ctypes wrappers of egnn_rings_host (``host``) and egnn_rings (``device``) over raw CSR arrays;
  and the bond lists the tests use, as dicts ``csr`` = (N, row_ptr, atom, shift | None, types, A, ptr): periodic cells of
  tests/_cells_util.py at any cutoff, clusters of tests/_topo_util.py at any scale, the hand-made saturation graph and the fan
  graph whose one search labels 2,594 sites through levels of 1,024."""
import ctypes as C

import numpy as np

from tests import _cells_util as CU
from tests import _topo_util as TU

MAX_DEGREE, COUNT_MAX, MAX_SITES = 32, 2 ** 31 - 1, 4096


# ---- bond lists ---------------------------------------------------------------------------------------------------------------------
def cells_csr(cells, cutoff=CU.CUTOFF, min_gap=1e-9):
    """a batch of cell dicts -> csr over the concatenated atoms; the bond list is restatement (i) of tests/_cells_util.py, rebuilt
    where the cutoff is not the cells' own, with the gap condition asserted"""
    rp, at, sh, ty, ptr = [np.zeros(1, np.int64)], [], [], [], [0]
    for c in cells:
        b = c["bonds"] if cutoff == CU.CUTOFF else CU.bonds(c["lattice"], c["frac"], cutoff)
        assert np.all(CU.widths(c["lattice"]) >= cutoff) and b[3] >= min_gap, (c["name"], b[3])
        rp.append(b[0][1:] + rp[-1][-1])
        at.append(b[1] + ptr[-1])
        sh.append(CU.shift_decode(b[2]).reshape(-1, 3))
        ty.append(c["types"])
        ptr.append(ptr[-1] + len(c["types"]))
    return dict(N=ptr[-1], row_ptr=np.concatenate(rp).astype(np.int32), atom=np.concatenate(at).astype(np.int32),
                shift=np.ascontiguousarray(np.concatenate(sh).astype(np.int32)), types=np.concatenate(ty).astype(np.int32),
                A=max(c["A"] for c in cells), ptr=np.array(ptr))


def clusters_csr(pos, types, sizes, A, scale=1.2, cap=None):
    """a ragged batch of clusters -> csr (no shifts): rows ascending, bonds by tests/_topo_util.py; ``cap`` keeps the first
    ``cap`` neighbours of a row (None: all of them, so that a crowd shows its 33 bonds)"""
    thr = TU.thresholds(TU.RADII[A], scale)
    rp, at, lo = [0], [], 0
    for n in sizes:
        assert TU.gap_ok(pos[lo:lo + n], types[lo:lo + n], thr)
        bond = TU.bond_matrix(pos[lo:lo + n], types[lo:lo + n], thr)
        for i in range(n):
            row = np.nonzero(bond[i])[0][:cap]
            at.append(row + lo)
            rp.append(rp[-1] + len(row))
        lo += n
    atom = np.concatenate(at).astype(np.int32) if at else np.zeros(0, np.int32)
    return dict(N=lo, row_ptr=np.array(rp, np.int32), atom=atom, shift=None, types=np.asarray(types, np.int32), A=A,
                ptr=np.concatenate([[0], np.cumsum(sizes)]))


def layered_csr(layers=12, width=8):
    """centre 0 - j = 1 - `layers` fully connected layers of `width` atoms - k = 2: -> (csr, the number of shortest paths from j to
    k in Python integers, the ring size)"""
    first = 3
    layer = [list(range(first + i * width, first + (i + 1) * width)) for i in range(layers)]
    nb = {0: [1, 2], 1: [0] + layer[0], 2: [0] + layer[-1]}
    for i, L in enumerate(layer):
        for a in L:
            nb[a] = sorted(([1] if i == 0 else layer[i - 1]) + ([2] if i == layers - 1 else layer[i + 1]))
    N = first + layers * width
    rp = np.concatenate([[0], np.cumsum([len(nb[a]) for a in range(N)])]).astype(np.int32)
    paths = [1] * width                                   # shortest paths from j to every atom of the layer, in Python integers
    for _ in range(layers - 1):
        paths = [sum(paths)] * width
    true = sum(paths)
    csr = dict(N=N, row_ptr=rp, atom=np.concatenate([nb[a] for a in range(N)]).astype(np.int32), shift=None,
               types=(np.arange(N) % 2).astype(np.int32), A=2, ptr=np.array([0, N]))
    return csr, true, layers + 3


def fan_csr(widths=(16, 256, 1024, 1024, 256, 16), extra=3):
    """centre 0 - j = 1 - layers of ``widths`` atoms - k = 2, in the style of layered_csr but wide: j is bonded to the whole first
    layer and k to the whole last.  Where the next layer is r times as wide (r >= 1), node i is bonded to nodes (i r + t) mod w' for
    t < r + extra; where it is r times narrower, to node i // r and, unless r divides i, to node (i // r + 1) mod w'.  One search
    from j labels every atom but the centre, level by level: a frontier of max(widths) sites, a table load of a third, and a node of
    the last layer carries 2 r bonds.  -> (csr, the layers as index arrays); every degree is asserted <= 32"""
    first, layer = 3, []
    for w in widths:
        layer.append(np.arange(first, first + w))
        first += w
    nb = {a: set() for a in range(first)}

    def bond(a, b):
        nb[int(a)].add(int(b))
        nb[int(b)].add(int(a))

    bond(0, 1), bond(0, 2)
    for a in layer[0]:
        bond(1, a)
    for a in layer[-1]:
        bond(2, a)
    for lo, hi in zip(layer[:-1], layer[1:]):
        w, w2 = len(lo), len(hi)
        if w2 >= w:
            assert w2 % w == 0
            r = w2 // w
            for i in range(w):
                for t in range(r + extra):
                    bond(lo[i], hi[(i * r + t) % w2])
        else:
            assert w % w2 == 0
            r = w // w2
            for i in range(w):
                bond(lo[i], hi[i // r])
                if i % r:
                    bond(lo[i], hi[(i // r + 1) % w2])
    deg = np.array([len(nb[a]) for a in range(first)])
    assert deg.max() <= MAX_DEGREE, (int(deg.max()), int(np.argmax(deg)))
    csr = dict(N=first, row_ptr=np.concatenate([[0], np.cumsum(deg)]).astype(np.int32),
               atom=np.concatenate([sorted(nb[a]) for a in range(first)]).astype(np.int32), shift=None,
               types=(np.arange(first) % 2).astype(np.int32), A=2, ptr=np.array([0, first]))
    return csr, layer


def fan_centres(layer):
    """centres of the fan graph beside atom 0: j, k and atoms inside every layer, the wide ones included"""
    return np.array([0, 1, 2, layer[0][7], layer[1][100], layer[2][5], layer[2][1023], layer[3][700], layer[4][17], layer[5][3]], dtype=np.int32)


def dense_ring_centres(name):
    """six centres of a dense cell of tests/_cells_util.py (the pure-Python restatement takes 0.1-0.2 s per centre there)"""
    n = len(CU.dense_cells()[name]["frac"])
    return np.arange(0, n, n // 6, dtype=np.int32)[:6]


def home_slots(atoms, slots):
    """the slot a cluster site (atom, shift 0) hashes to in a table of ``slots`` entries (csrc/eval/rings_math.h: ring_key, ring_hash
    = the finaliser of splitmix64), restated in Python integers.  Two sites with one home slot make a probe chain whatever the
    order of insertion"""
    m64 = (1 << 64) - 1
    out = []
    for a in atoms:
        k = (int(a) << 18) | (32 << 12) | (32 << 6) | 32
        k ^= k >> 30
        k = (k * 0xbf58476d1ce4e5b9) & m64
        k ^= k >> 27
        k = (k * 0x94d049bb133111eb) & m64
        k ^= k >> 31
        out.append((k & 0xFFFFFFFF) & (slots - 1))
    return np.array(out)


def level_widths(csr, c, p):
    """the number of sites a search from row position p of centre c labels at level 0, 1, ..: plain breadth-first over the CSR
    with the centre removed (clusters: no shifts), to the end"""
    assert csr["shift"] is None
    rp, at = csr["row_ptr"], csr["atom"]
    source = int(at[rp[c] + p])
    seen, frontier, out = {int(c), source}, [source], []
    while frontier:
        out.append(len(frontier))
        nxt = []
        for a in frontier:
            for b in at[rp[a]:rp[a + 1]].tolist():
                if b not in seen:
                    seen.add(b)
                    nxt.append(b)
        frontier = nxt
    return out


def angle_ptr(csr, centres):
    d = np.diff(csr["row_ptr"].astype(np.int64))[np.asarray(centres, dtype=np.int64)]
    return np.concatenate([[0], np.cumsum(d * (d - 1) // 2)]).astype(np.int32)


def all_centres(csr):
    return np.arange(csr["N"], dtype=np.int32)


# ---- (i) the search restatement -------------------------------------------------------------------------------------------------------
def _neighbours(csr, site):
    a, sx, sy, sz = site
    rp, at, sh = csr["row_ptr"], csr["atom"], csr["shift"]
    if sh is None:
        return [(int(at[e]), 0, 0, 0) for e in range(rp[a], rp[a + 1])]
    return [(int(at[e]), sx + int(sh[e, 0]), sy + int(sh[e, 1]), sz + int(sh[e, 2])) for e in range(rp[a], rp[a + 1])]


def search(csr, c, p, max_size, max_sites, ignore_shifts=False):
    """one search -> (list of (size, count) for q = p + 1 .. d - 1, or None if it overflowed; sites labelled)"""
    if ignore_shifts:
        csr = dict(csr, shift=None)
    centre = (int(c), 0, 0, 0)
    row = _neighbours(csr, centre)
    source, targets = row[p], row[p + 1:]
    level, count, frontier = {}, {}, []
    if source != centre:
        level[source], count[source], frontier = 0, 1, [source]
    res = [None] * len(targets)

    def settle(l):
        for i, t in enumerate(targets):
            if res[i] is None and t in level:
                res[i] = (l + 2, count[t])

    settle(0)
    l = 0
    while l < max_size - 2 and frontier and any(r is None for r in res):
        l += 1
        new = []
        for s in frontier:
            for nb in _neighbours(csr, s):
                if nb != centre and nb not in level:
                    level[nb] = l
                    new.append(nb)
        if len(level) > max_sites:
            return None, len(level)
        for s in new:
            count[s] = min(sum(count[nb] for nb in _neighbours(csr, s) if level.get(nb) == l - 1), COUNT_MAX)
        settle(l)
        frontier = new
    return [r or (0, 0) for r in res], len(level)


def restated(csr, centres=None, max_size=16, max_sites=MAX_SITES, ignore_shifts=False):
    """(i) over a centre list -> dict(size, count, overflow, hist int64; angle_ptr; labelled = the largest number of sites one
    search of each centre labelled)"""
    centres = all_centres(csr) if centres is None else np.asarray(centres).reshape(-1)
    ap = angle_ptr(csr, centres)
    size, count = np.zeros(ap[-1], np.int64), np.zeros(ap[-1], np.int64)
    over, labelled = np.zeros(len(centres), np.int64), np.zeros(len(centres), np.int64)
    hist = np.zeros((csr["A"], max_size + 1), np.int64)
    for m, c in enumerate(centres):
        d = int(csr["row_ptr"][c + 1] - csr["row_ptr"][c])
        at = int(ap[m])
        if d > MAX_DEGREE:
            size[ap[m]:ap[m + 1]], over[m] = -1, 1
            continue
        for p in range(d - 1):
            res, n = search(csr, c, p, max_size, max_sites, ignore_shifts)
            labelled[m] = max(labelled[m], n)
            k = d - 1 - p
            if res is None:
                size[at:at + k], over[m] = -1, 1
            else:
                size[at:at + k], count[at:at + k] = [r[0] for r in res], [r[1] for r in res]
                np.add.at(hist[csr["types"][c]], [r[0] for r in res], 1)
            at += k
    return dict(size=size, count=count, overflow=over, hist=hist, angle_ptr=ap, labelled=labelled)


# ---- (ii) the independent check -------------------------------------------------------------------------------------------------------
def independent(csr, c, max_size):
    """-> list of (size, count) over the angles of centre c in lexicographic order, from an explicit graph, scipy's shortest paths
    and integer matrix powers"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import shortest_path
    centre = (int(c), 0, 0, 0)
    row = _neighbours(csr, centre)
    index, frontier = {}, [centre]
    seen = {centre}
    for _ in range(max_size // 2):
        nxt = []
        for s in frontier:
            for nb in _neighbours(csr, s):
                if nb not in seen:
                    seen.add(nb)
                    nxt.append(nb)
        frontier = nxt
    for s in sorted(seen - {centre}):
        index[s] = len(index)
    n = len(index)
    if n == 0:
        return []
    i, j = [], []
    for s, a in index.items():
        for nb in _neighbours(csr, s):
            if nb in index:
                i.append(a)
                j.append(index[nb])
    adj = sp.csr_matrix((np.ones(len(i), np.int64), (i, j)), shape=(n, n))
    assert (adj.nnz == 0 or adj.data.max() <= 1) and (adj != adj.T).nnz == 0          # a simple undirected graph
    src = [index[s] for s in row]
    dist = shortest_path(adj, method="D", unweighted=True, indices=src) if len(src) else np.zeros((0, n))
    out = []
    for p in range(len(row)):
        walks = [np.zeros(n, np.int64)]
        walks[0][src[p]] = 1
        for q in range(p + 1, len(row)):
            dq = dist[p, src[q]]
            if not np.isfinite(dq) or dq + 2 > max_size:
                out.append((0, 0))
                continue
            dq = int(dq)
            while len(walks) <= dq:
                walks.append(adj.T @ walks[-1])                          # row src[p] of A^t, in int64
            assert walks[dq].max() < 2 ** 62
            out.append((dq + 2, int(min(walks[dq][src[q]], COUNT_MAX))))
    return out


# ---- (iii) the entries ----------------------------------------------------------------------------------------------------------------
def _vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def host(lib, csr, centres=None, max_size=16, max_sites=MAX_SITES, hist=True, raw=None):
    """egnn_rings_host -> (rc, dict of int32 arrays).  ``raw`` overrides arguments by name (the argument tests)"""
    a = dict(csr)
    a["centre"] = all_centres(csr) if centres is None else np.ascontiguousarray(centres, dtype=np.int32).reshape(-1)
    a["angle_ptr"] = angle_ptr(csr, np.clip(a["centre"], 0, csr["N"] - 1))
    M, n = len(a["centre"]), int(a["angle_ptr"][-1])
    a.update(raw or {})
    o = dict(size=np.full(max(n, 1), -7, np.int32), count=np.full(max(n, 1), -7, np.int32), overflow=np.full(max(M, 1), -7, np.int32),
             hist=np.full((a["A"], max_size + 1), -7, np.int32) if hist else None)
    o.update({k: v for k, v in (raw or {}).items() if k in o})
    rc = lib.egnn_rings_host(a["N"], _vp(a["row_ptr"]), a.get("E", len(csr["atom"])), _vp(a["atom"]), _vp(a["shift"]),
                             _vp(a["types"]), a["A"], M, _vp(a["centre"]), _vp(a["angle_ptr"]), n, int(max_size), int(max_sites),
                             _vp(o["size"]), _vp(o["count"]), _vp(o["overflow"]), _vp(o["hist"]))
    if rc != 0:
        return rc, None
    return rc, dict(size=o["size"][:n], count=o["count"][:n], overflow=o["overflow"][:M], hist=o["hist"], angle_ptr=a["angle_ptr"])


def device(lib, csr, centres=None, max_size=16, max_sites=MAX_SITES, mirrors=True):
    """egnn_rings on the current device -> (rc, dict of int32 numpy arrays); the host copies of the lists go along unless
    ``mirrors`` is False"""
    import torch
    from diffusion_model_amd import _lib
    ctr = all_centres(csr) if centres is None else np.ascontiguousarray(centres, dtype=np.int32).reshape(-1)
    ap = angle_ptr(csr, ctr)
    M, n = len(ctr), int(ap[-1])
    up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d = {k: up(csr[k]) for k in ("row_ptr", "atom", "shift", "types")}
    d_ctr, d_ap = up(ctr), up(ap)
    out = [torch.full((max(k, 1),), -7, dtype=torch.int32, device="cuda") for k in (n, n, M)]
    hist = torch.full((csr["A"], max_size + 1), -7, dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None or t.numel() == 0 else _lib.ptr(t)
    host_copies = [_vp(csr["row_ptr"]), _vp(csr["atom"]), _vp(csr["shift"]), _vp(ctr)] if mirrors else [None] * 4
    rc = lib.egnn_rings(_lib.stream_ptr(), csr["N"], p(d["row_ptr"]), len(csr["atom"]), p(d["atom"]), p(d["shift"]), p(d["types"]),
                        csr["A"], M, p(d_ctr), p(d_ap), n, int(max_size), int(max_sites), p(out[0]), p(out[1]), p(out[2]), p(hist),
                        *host_copies)
    torch.cuda.synchronize()
    return rc, dict(size=out[0][:n].cpu().numpy(), count=out[1][:n].cpu().numpy(), overflow=out[2][:M].cpu().numpy(),
                    hist=hist.cpu().numpy(), angle_ptr=ap)


def assert_equal(got, want, keys=("size", "count", "overflow", "hist")):
    for k in keys:
        assert np.asarray(got[k]).dtype == np.int32, k
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), want[k]), k

"""Numpy restatements, written from reading, for the periodic-cell environments (csrc/cells/cell_math.h), shared by the CPU and
GPU tests and by tools/cells_time.py (test infrastructure):

  (i)   the infinite-lattice definition: wrapped fractions w = f - floor(f); site (j, s) is bonded to atom i iff (j, s) != (i, 0),
        s in {-1,0,1}^3 and |(w_j - w_i + s) L|^2 < cutoff^2 in float64, in the library's operation order; the environment of a
        centre is what `shells` bonds reach, the centre first, then ascending (atom, shift code); positions float32 of the float64
        vector (``bonds``, ``environment``);
  (ii)  the reference's supercell rule (make_dataset.py:79-111, :177-188, :258-272): 27 n sites of the 3x3x3 supercell offset by
        one lattice diagonal, minimum-image distances in the TRIPLED lattice, return_index_within_2ang nested to 2 / 3 / 4 levels,
        positions float32(X_site) - float32(X_centre), plus a flag raised when a bond it used wraps round the supercell
        (``reference_environment``);
  (iii) seeded cell generators (chain, beta-cristobalite, its triclinic distortion, random cells, the one-atom cell; the dense
        jittered grids, the ladder that reaches shift +-4 and the 60-degree zincblende cell), each asserting the gap condition: no
        pair distance within 1e-9 A of the cutoff, so that the float64 comparison is unambiguous on every side.
"""
import ctypes as C
import functools
import itertools

import numpy as np

CUTOFF = 2.0
SHIFT_CODES = 729
CENTRE_CODE = 364
IMAGES = np.array(list(itertools.product((-1, 0, 1), repeat=3)), dtype=np.int64)   # ascending shift code


def lattice_from_parameters(a, b, c, alpha, beta, gamma):
    """float64 [3, 3], rows a, b, c: c along z, a in the xz-plane (restated from the documentation of the library the reference
    uses; diffusion_model_amd.cells.lattice_from_parameters is checked against its six parameters, not against this)"""
    al, be, ga = np.radians([alpha, beta, gamma])
    val = np.clip((np.cos(al) * np.cos(be) - np.cos(ga)) / (np.sin(al) * np.sin(be)), -1.0, 1.0)
    gs = np.arccos(val)
    return np.array([[a * np.sin(be), 0.0, a * np.cos(be)],
                     [-b * np.sin(al) * np.cos(gs), b * np.sin(al) * np.sin(gs), b * np.cos(al)],
                     [0.0, 0.0, c]], dtype=np.float64)


def shift_code(s):
    s = np.asarray(s, dtype=np.int64)
    return ((s[..., 0] + 4) * 9 + (s[..., 1] + 4)) * 9 + (s[..., 2] + 4)


def shift_decode(code):
    code = np.asarray(code, dtype=np.int64)
    return np.stack([code // 81 - 4, code // 9 % 9 - 4, code % 9 - 4], -1)


def wrap(frac):
    f = np.asarray(frac, dtype=np.float64)
    w = f - np.floor(f)
    return np.where(w < 1.0, w, 0.0)


def site_vectors(w_j, w_i, s, L):
    """float64 [..., 3]: d_k = (w_j - w_i) + s_k, r_x = (d_0 L[0,x] + d_1 L[1,x]) + d_2 L[2,x]"""
    d = (np.asarray(w_j, dtype=np.float64) - np.asarray(w_i, dtype=np.float64)) + np.asarray(s, dtype=np.float64)
    return (d[..., 0:1] * L[0] + d[..., 1:2] * L[1]) + d[..., 2:3] * L[2]


def widths(L):
    a, b, c = L
    det = abs(np.dot(a, np.cross(b, c)))
    return np.array([det / np.linalg.norm(np.cross(b, c)), det / np.linalg.norm(np.cross(c, a)), det / np.linalg.norm(np.cross(a, b))])


def bonds(L, frac, cutoff=CUTOFF):
    """(i) -> (row_ptr int64 [n+1], atom int64 [E], code int64 [E], gap): rows ascending by (atom, shift code); gap = the smallest
    | |r| - cutoff | over every pair and image"""
    L = np.asarray(L, dtype=np.float64)
    w = wrap(frac)
    n = len(w)
    codes = shift_code(IMAGES)
    deg, atoms, shifts, gap = np.zeros(n, dtype=np.int64), [], [], np.inf
    for i0 in range(0, n, 32):
        wi = w[i0:i0 + 32]
        r = site_vectors(w[None, :, None, :], wi[:, None, None, :], IMAGES[None, None, :, :], L)   # [c, n, 27, 3]
        r2 = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
        ok = r2 < cutoff * cutoff
        ci = np.arange(len(wi))
        ok[ci, i0 + ci, 13] = False
        r2[ci, i0 + ci, 13] = np.inf
        gap = min(gap, float(np.abs(np.sqrt(r2) - cutoff).min()))
        c, j, s = np.nonzero(ok)          # ascending (centre, atom, image)
        deg[i0:i0 + len(wi)] = np.bincount(c, minlength=len(wi))
        atoms.append(j)
        shifts.append(codes[s])
    row_ptr = np.concatenate([[0], np.cumsum(deg)])
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return row_ptr, cat(atoms), cat(shifts), gap


def environment(L, frac, bond, centre, shells):
    """(i) -> (atom int64 [m], code int64 [m], pos float32 [m, 3]), the centre first, then ascending (atom, shift code)"""
    L = np.asarray(L, dtype=np.float64)
    row_ptr, b_atom, b_code, _ = bond
    b_shift = shift_decode(b_code)
    start = (int(centre), 0, 0, 0)
    seen, frontier = {start}, [start]
    for _ in range(shells):
        nxt = []
        for (a, sx, sy, sz) in frontier:
            for e in range(row_ptr[a], row_ptr[a + 1]):
                site = (int(b_atom[e]), sx + int(b_shift[e, 0]), sy + int(b_shift[e, 1]), sz + int(b_shift[e, 2]))
                if site not in seen:
                    seen.add(site)
                    nxt.append(site)
        frontier = nxt
    rest = sorted(seen - {start})
    sites = np.array([start] + rest, dtype=np.int64).reshape(-1, 4)
    w = wrap(frac)
    r = site_vectors(w[sites[:, 0]], w[int(centre)], sites[:, 1:], L)
    return sites[:, 0], shift_code(sites[:, 1:]), r.astype(np.float32)


def reference_environment(L, frac, centre, levels, cutoff=CUTOFF, rows=None):
    """(ii) -> (set of (atom, sx, sy, sz) with the centre as (centre, 0, 0, 0), wrapped flag, pos dict site -> float32 [3],
    max |X|): the supercell site of image u of atom j is X = w_j L + u L + (1,1,1) L; distances are minimum-image in the lattice
    3 L (rows of the distance matrix, computed when first read); a site found through a bond whose minimum image is not the
    direct one sets the flag.  ``rows``: a dict the caller keeps per cell, so that rows of the matrix already computed for
    another centre or depth are read again, not recomputed"""
    L = np.asarray(L, dtype=np.float64)
    w = wrap(frac)
    n = len(w)
    X = ((w @ L)[:, None, :] + IMAGES.astype(np.float64) @ L + np.ones(3) @ L).reshape(27 * n, 3)   # site index = 27 atom + image
    L3 = 3.0 * L
    F = X @ np.linalg.inv(L3)
    t_img = IMAGES.astype(np.float64)

    rows = {} if rows is None else rows

    def row(p):
        if p not in rows:
            df = F - F[p]
            df -= np.round(df)
            d = np.linalg.norm((df[:, None, :] + t_img[None, :, :]) @ L3, axis=2).min(1)        # minimum image of the tripled lattice
            direct = np.linalg.norm(X - X[p], axis=1)
            near = np.nonzero(d < cutoff)[0]
            near = near[near != p]
            rows[p] = (near, bool(np.any(direct[near] >= cutoff)))
        return rows[p]

    centre_site = 27 * int(centre) + 13
    found, wrapped, frontier = [], False, [centre_site]
    for _ in range(levels):
        nxt = []
        for p in frontier:
            near, wr = row(p)
            wrapped |= wr
            nxt.extend(near.tolist())
        found += nxt
        frontier = sorted(set(nxt))   # the reference's nested loops revisit sites; the set below is the same
    sites = [centre_site] + [p for p in sorted(set(found)) if p != centre_site]
    X32 = X.astype(np.float32)
    out, pos = set(), {}
    for p in sites:
        key = (p // 27,) + tuple(int(v) for v in IMAGES[p % 27])
        out.add(key)
        pos[key] = X32[p] - X32[centre_site]
    return out, wrapped, pos, float(np.abs(X).max())


# ---- (iii) seeded cells: dicts with lattice float64 [3,3], frac float64 [n,3], types int32 [n], A ---------------------------------
def _cell(lattice, frac, types, name, cutoff=CUTOFF, check=True):
    """``check=False`` (tools/cells_time.py, cells too large for the numpy bond list) leaves out the restated bond list and its gap"""
    cell = dict(lattice=np.asarray(lattice, dtype=np.float64), frac=np.asarray(frac, dtype=np.float64).reshape(-1, 3),
                types=np.asarray(types, dtype=np.int32), A=2, name=name, cutoff=float(cutoff))
    assert np.all(widths(cell["lattice"]) >= cutoff), name
    if not check:
        return cell
    cell["bonds"] = bonds(cell["lattice"], cell["frac"], cutoff)
    assert cell["bonds"][3] >= 1e-9, f"{name}: a pair distance within 1e-9 of the cutoff; reseed"
    return cell


def chain_cell():
    """cubic a = 3.2 A, atoms at (0,0,0) and (1/2,0,0): a chain of 1.6 A bonds along x"""
    return _cell(3.2 * np.eye(3), [[0, 0, 0], [0.5, 0, 0]], [1, 0], "chain")


def one_atom_cell():
    return _cell(5.0 * np.eye(3), [[0.3, 0.6, 0.9]], [0], "one-atom")


def _cristobalite_frac():
    fcc = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
    si = np.concatenate([fcc, fcc + 0.25])
    arms = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) / 8.0
    o = (fcc[:, None, :] + arms[None, :, :]).reshape(-1, 3)
    return np.concatenate([si, o]), np.array([1] * 8 + [0] * 16)      # types: O = 0, Si = 1 (the reference's one-hot columns)


def cristobalite_cell():
    """ideal beta-cristobalite, a = 7.16 A, 8 Si + 16 O (Si-O 1.55 A, O-O 2.53 A)"""
    frac, types = _cristobalite_frac()
    return _cell(7.16 * np.eye(3), frac, types, "cristobalite")


def triclinic_cell(seed=7, check=True):
    """beta-cristobalite in a 7.3 / 7.0 / 7.5 A, 84 / 97 / 92 degree cell, displaced by sigma = 0.01 in fractional coordinates; some
    coordinates fall outside [0, 1)"""
    frac, types = _cristobalite_frac()
    rng = np.random.default_rng(seed)
    return _cell(lattice_from_parameters(7.3, 7.0, 7.5, 84.0, 97.0, 92.0), frac + 0.01 * rng.standard_normal(frac.shape), types, "triclinic",
                 check=check)


def random_cell(n, seed, spread=0.0, check=True):
    """n atoms placed one after the other, each at least 1.45 A from every earlier atom and image, in a triclinic box of about
    11 x 12 x 10.5 A at n = 65 (the same density at any n); ``spread`` moves the fractions outside [0, 1)"""
    rng = np.random.default_rng(seed)
    k = (n / 65.0) ** (1.0 / 3.0)
    L = lattice_from_parameters(11.0 * k, 12.0 * k, 10.5 * k, 86.0, 95.0, 91.0)
    shifts = IMAGES.astype(np.float64)
    w = np.zeros((0, 3))
    while len(w) < n:
        f = rng.uniform(0.0, 1.0, 3)
        if len(w):
            d = np.linalg.norm(((w - f)[:, None, :] + shifts[None, :, :]) @ L, axis=2)
            if d.min() < 1.45:
                continue
        w = np.concatenate([w, f[None, :]])
    frac = w + (np.floor(rng.uniform(-spread, spread + 1.0, w.shape)) if spread else 0.0)
    return _cell(L, frac, rng.integers(0, 2, n), f"random-{n}", check=check)


def grid_cell(nx, ny, nz, a, cutoff, seed=1, jitter=0.02, drop=0, skew=False):
    """a jittered simple-cubic block of nx x ny x nz atoms, spacing a: fractions g / dims + jitter N(0, 1) / dims (g ascending in
    (x, y, z)), types drawn after the jitter; ``skew`` tilts b by 0.3 A along x and c by -0.2 A along y; ``drop`` removes the
    first ``drop`` atoms (vacancies).  With a well below the cutoff this is the dense regime: two dozen bonds per atom and several
    hundred sites at 4 shells"""
    dims = np.array([nx, ny, nz], dtype=np.float64)
    g = np.array(list(itertools.product(range(nx), range(ny), range(nz))), dtype=np.float64)
    rng = np.random.default_rng(seed)
    frac = g / dims + jitter * rng.standard_normal(g.shape) / dims
    types = rng.integers(0, 2, len(g))
    L = np.diag(dims * a)
    if skew:
        L[1, 0], L[2, 1] = 0.3, -0.2
    name = f"grid-{nx}x{ny}x{nz}-{a}" + ("-skew" if skew else "") + (f"-drop{drop}" if drop else "")
    return _cell(L, frac[drop:], types[drop:], name, cutoff=cutoff)


def ladder_cell():
    """cubic a = 2.05 A, five atoms 0.41 A apart along x: 8 bonds per atom, all along x (the images in y and z are 2.05 A away), so
    that four hops from atom 0 reach shift -4 and from atom 4 shift +4: the ends of the shift code's range"""
    return _cell(2.05 * np.eye(3), [[x, 0.3, 0.3] for x in (0.0, 0.2, 0.4, 0.6, 0.8)], [0, 1, 0, 1, 0], "ladder")


def zincblende_cell():
    """the primitive fcc cell of zincblende, a_conv = 2.6 A: 60 degree angles, perpendicular widths 2.123 A just above the cutoff,
    one coordinate below 0"""
    L = 2.6 / np.sqrt(2.0) * np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
    return _cell(L, [[0.02, 0.01, -0.03], [0.25, 0.25, 0.25]], [1, 0], "zincblende")


def cscl_cell():
    """cubic a = 2.05 A, atoms near (0, 0, 0) and at (1/2, 1/2, 1/2), 1.78 A apart: each atom is bonded to EIGHT images of the
    other and to nothing else -- the most images of one atom a cell whose widths reach the cutoff can bond, so one lane of the
    bond kernel sets eight bits of its mask"""
    return _cell(2.05 * np.eye(3), [[0.01, 0.02, -0.01], [0.5, 0.5, 0.5]], [0, 1], "cscl")


def frontier_sizes(bond, centre, shells):
    """(i) -> the number of sites first reached at hop 0 (the centre: 1), 1, .., shells - 1: the frontiers a breadth-first search
    of ``shells`` hops expands"""
    row_ptr, b_atom, b_code, _ = bond
    b_shift = shift_decode(b_code)
    start = (int(centre), 0, 0, 0)
    seen, frontier, out = {start}, [start], []
    for _ in range(shells):
        out.append(len(frontier))
        nxt = []
        for (a, sx, sy, sz) in frontier:
            for e in range(row_ptr[a], row_ptr[a + 1]):
                site = (int(b_atom[e]), sx + int(b_shift[e, 0]), sy + int(b_shift[e, 1]), sz + int(b_shift[e, 2]))
                if site not in seen:
                    seen.add(site)
                    nxt.append(site)
        frontier = nxt
    return out


@functools.lru_cache(maxsize=None)
def dense_cells():
    """the cells of the dense regime, by name -- environments of several hundred sites, frontiers of several wavefronts, bond rows
    at the ring search's degree limit: the 80-atom skewed grid (24-26 bonds per atom), the 27-atom grid at cutoff 1.6 (32 bonds per
    atom, more than 1024 sites at 4 shells), the same grid with 5 vacancies, the ladder, the zincblende and the CsCl cell"""
    return dict(g80=grid_cell(5, 4, 4, 1.1, 2.0, skew=True), g22=grid_cell(3, 3, 3, 0.75, 1.6, drop=5), g27=grid_cell(3, 3, 3, 0.75, 1.6),
                ladder=ladder_cell(), zincblende=zincblende_cell(), cscl=cscl_cell())


def dense_centres(name):
    """the centres the restatement is run on (pure Python, 10 ms per centre of 700-1,000 sites): every third atom of a grid, every
    atom of the two small cells"""
    n = len(dense_cells()[name]["frac"])
    return np.arange(0, n, 3 if n > 5 else 1)


@functools.lru_cache(maxsize=None)
def dense_reach(name, shells):
    """what restatement (i) says a search of ``shells`` hops about dense_centres(name) meets: dict(env = restated_environments of
    those centres, sizes, frontier = the largest frontier expanded per centre, max_shift = the largest |s| in an environment)"""
    c = dense_cells()[name]
    ctr = dense_centres(name)
    env = restated_environments([c], centres=ctr, shells=shells)
    return dict(env=env, sizes=env["size"].astype(np.int64), frontier=np.array([max(frontier_sizes(c["bonds"], i, shells)) for i in ctr]),
                max_shift=int(np.abs(shift_decode(env["shift"])).max()))


def host_environments(lib, cells, centres=None, shells=2, cutoff=CUTOFF, max_atoms=256, A=None, centre_cell=None, raw=None, caps=None):
    """egnn_cell_env_host on a batch of cell dicts -> (rc, dict of arrays): centres = indices into the concatenated atoms (default:
    all), two calls (sizes, then lists).  ``raw`` overrides arrays by name for the argument tests; ``caps`` = (bonds, rows) known
    from an earlier call makes it ONE call (tools/cells_time.py times that)."""
    sizes = [len(c["frac"]) for c in cells]
    cp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    a = dict(cell_ptr=cp, lattice=np.ascontiguousarray(np.stack([c["lattice"].reshape(9) for c in cells])),
             frac=np.ascontiguousarray(np.concatenate([c["frac"] for c in cells])),
             type=np.ascontiguousarray(np.concatenate([c["types"] for c in cells]).astype(np.int32)))
    N = int(cp[-1])
    ctr = np.arange(N, dtype=np.int32) if centres is None else np.asarray(centres, dtype=np.int32).reshape(-1)
    a["centre"] = ctr
    a["centre_cell"] = (np.searchsorted(cp, ctr, side="right") - 1).astype(np.int32) if centre_cell is None else np.asarray(centre_cell, np.int32)
    a.update(raw or {})
    M = len(ctr)
    A = max(c["A"] for c in cells) if A is None else A
    vp = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
    bond_ptr, env_size = np.full(N + 1, -7, dtype=np.int32), np.full(max(M, 1), -7, dtype=np.int32)

    def call(bc, ba, bs, ec, ea, es, et, ep):
        return lib.egnn_cell_env_host(len(cells), A, vp(a["cell_ptr"]), vp(a["lattice"]), vp(a["frac"]), vp(a["type"]), float(cutoff), M,
                                      vp(a["centre_cell"]), vp(a["centre"]), int(shells), int(max_atoms), vp(bond_ptr), bc, vp(ba), vp(bs),
                                      vp(env_size), ec, vp(ea), vp(es), vp(et), vp(ep))

    if caps is None:
        rc = call(0, None, None, 0, None, None, None, None)
        if rc != 0:
            return rc, None
        E = int(bond_ptr[-1])
        sz = env_size[:M].astype(np.int64)
        T = int(np.where(sz > max_atoms, 0, sz).sum())
    else:
        E, T = caps
    ba, bs = np.full(max(E, 1), -7, dtype=np.int32), np.full(max(E, 1), -7, dtype=np.int32)
    ea, es, et = (np.full(max(T, 1), -7, dtype=np.int32) for _ in range(3))
    ep = np.full((max(T, 1), 3), np.nan, dtype=np.float32)
    rc = call(E, ba, bs, T, ea, es, et, ep)
    return rc, dict(bond_ptr=bond_ptr, bond_atom=ba[:E], bond_shift=bs[:E], size=env_size[:M].copy(), atom=ea[:T], shift=es[:T],
                    type=et[:T], pos=ep[:T], cell_ptr=cp, centre=ctr, centre_cell=a["centre_cell"])


def restated_environments(cells, centres=None, shells=2):
    """(i) on a batch of cell dicts, in the layout of host_environments (atoms counted over the whole batch)"""
    sizes = [len(c["frac"]) for c in cells]
    cp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(cp[-1])
    ctr = np.arange(N) if centres is None else np.asarray(centres).reshape(-1)
    bond_ptr, b_atom, b_shift = [np.zeros(1, dtype=np.int64)], [], []
    for c, lo in zip(cells, cp[:-1]):
        rp, at, code, _ = c["bonds"]
        bond_ptr.append(rp[1:] + bond_ptr[-1][-1])
        b_atom.append(at + lo)
        b_shift.append(code)
    size, atom, shift, typ, pos = [], [], [], [], []
    for g in ctr:
        ci = int(np.searchsorted(cp, g, side="right") - 1)
        c = cells[ci]
        at, code, p = environment(c["lattice"], c["frac"], c["bonds"], int(g - cp[ci]), shells)
        size.append(len(at)); atom.append(at + cp[ci]); shift.append(code); typ.append(c["types"][at]); pos.append(p)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    return dict(bond_ptr=np.concatenate(bond_ptr).astype(np.int32), bond_atom=cat(b_atom, np.int32), bond_shift=cat(b_shift, np.int32),
                size=np.array(size, dtype=np.int32), atom=cat(atom, np.int32), shift=cat(shift, np.int32), type=cat(typ, np.int32),
                pos=np.concatenate(pos).astype(np.float32) if pos else np.zeros((0, 3), np.float32))


def ulp_distance(a, b):
    """float32 arrays -> int64 array of the distance in units in the last place (signed zeros coincide)"""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))

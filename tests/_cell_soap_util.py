"""Numpy restatement of the SOAP descriptors of periodic cells (csrc/cells/cell_soap_math.h), shared by the CPU and GPU tests (test
infrastructure), the fixtures both use, and the ctypes wrappers of the host statements egnn_cell_sites_host, egnn_cell_soap_host and
egnn_cell_soap_mean_host.

  * sites: the box walk without a cull -- b_k = floor(cut / w_k) + 1, every (atom, shift of the box) in ascending (atom, shift code),
    fp64 vectors (tests/_cells_util.site_vectors: the library's operation order), d2 < cut^2, (i, 0) left out;
  * descriptor: the centre at d = 0 first, then the sites in that order, through the formulas of tests/_soap_util (solid_harmonics,
    the radial values, the ascending sum, beta, the power spectrum) on the fp64 vectors;
  * fixtures (cell dicts of tests/_cells_util, types drawn per A): "thin", a 12-atom triclinic cell with widths 1.14 / 4.74 / 3.1 A
    (boxes 4 / 1 / 2 at the small basis's cut 4.37 A); "crist", the displaced 24-atom beta-cristobalite cell of
    tests/_cell_grid_util.displaced_cristobalite(1) (box 2 at the default cut 8.37 A, about 160 sites a row); "one", the one-atom cell
    (its own images only);
  * the truth is tests/golden/cell_soap_golden.npz (make_cell_soap_golden.py: mpmath at 60 digits, sites by exact rational
    arithmetic); the tables are those of tests/golden/soap_golden.npz.
Gap condition (asserted for every input): no site distance within 1e-9 (relative) of the cut.
"""
import ctypes as C
import functools
import itertools
import os

import numpy as np

from tests import _cell_grid_util as GU
from tests import _cell_stats_util as STU
from tests import _cells_util as CU
from tests import _soap_util as SU

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cell_soap_golden.npz")
THIN_SEED = 3
# fixture -> (configuration of tests/_soap_util.CONFIGS, the A values of the truth, centres: None = every atom)
FIXTURES = {"thin": ("small", (1, 2, 3), None), "crist": ("default", (2,), (8, 0)), "one": ("default", (1,), None)}


def thin_cell():
    """12 atoms in a triclinic cell of widths 1.14 / 4.74 / 3.1 A; some fractions lie outside [0, 1)"""
    L = np.array([[1.15, 0.0, 0.0], [0.4, 4.8, 0.0], [0.3, -0.5, 3.1]])
    frac = np.random.default_rng(THIN_SEED).uniform(-0.5, 1.5, (12, 3))
    return dict(lattice=L, frac=frac, types=np.zeros(12, np.int32), A=1, name="thin", cutoff=CU.CUTOFF)


def fixture(name, A=None):
    """the cell dict of one fixture with the types of ``A`` (the cristobalite keeps its own: A = 2)"""
    if name == "thin":
        cell = thin_cell()
        cell["types"] = np.random.default_rng(100 + A).integers(0, A, 12).astype(np.int32)
        cell["A"] = A
        return cell
    if name == "crist":
        return GU.displaced_cristobalite(1)
    cell = dict(CU.one_atom_cell())
    cell["A"] = 1
    return cell


def centres_of(name, cell):
    listed = FIXTURES[name][2]
    return np.arange(len(cell["frac"]), dtype=np.int32) if listed is None else np.array(listed, dtype=np.int32)


def cut_of(name):
    return SU.neighbour_cut(SU.CONFIGS[FIXTURES[name][0]])


def box(L, cut):
    return (np.floor(cut / CU.widths(np.asarray(L, dtype=np.float64))) + 1.0).astype(np.int64)


def box_shifts(b):
    """the shifts of the box ascending in (s_x, s_y, s_z): ascending shift code"""
    return np.array(list(itertools.product(*(range(-int(k), int(k) + 1) for k in b))), dtype=np.int64)


def sites(cell, cut, centre, gap=None):
    """-> (atom int64 [P] inside the cell, code int64 [P], r float64 [P, 3]) ascending by (atom, shift code), the centre left out.
    ``gap``: a list that receives the smallest | |r| - cut | / cut over every candidate."""
    L = np.asarray(cell["lattice"], dtype=np.float64)
    w = CU.wrap(cell["frac"])
    sh = box_shifts(box(L, cut))
    r = CU.site_vectors(w[:, None, :], w[int(centre)], sh[None, :, :], L)          # [n, nbox, 3]
    r2 = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
    if gap is not None:
        gap.append(float(np.abs(np.sqrt(r2) - cut).min() / cut))
    ok = r2 < cut * cut
    ok[int(centre), int(np.nonzero((sh == 0).all(1))[0][0])] = False
    j, t = np.nonzero(ok)                                                          # ascending (atom, shift)
    return j, CU.shift_code(sh[t]), r[j, t]


def site_lists(cells, cut, centres):
    """the CSR of a batch: ``centres`` index the concatenated atoms -> (row_ptr int32 [M+1], atom int32 [T] into the batch, code int32
    [T], the smallest relative gap)"""
    ptr = np.concatenate([[0], np.cumsum([len(c["frac"]) for c in cells])])
    rows, atoms, codes, gap = [0], [], [], []
    for i in centres:
        c = int(np.searchsorted(ptr, i, side="right")) - 1
        j, code, _ = sites(cells[c], cut, int(i) - ptr[c], gap)
        atoms.append(j + ptr[c])
        codes.append(code)
        rows.append(rows[-1] + len(j))
    cat = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    return np.array(rows, dtype=np.int32), cat(atoms), cat(codes), min(gap) if gap else np.inf


def descriptor_of_vectors(d, tj, A, tables):
    """the descriptor over neighbours at vectors d [P, 3] of species tj [P], summed in their order -> (desc [F], coeff [A, n_max, LM])"""
    K, gamma, beta, norm, weight = tables
    n_max, L1 = K.shape
    l_max, LM = L1 - 1, L1 * L1
    l_of = np.repeat(np.arange(L1), 2 * np.arange(L1) + 1)
    z1, z2, n1, n2, ll = SU.feature_index(A, n_max, l_max)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    R = SU.solid_harmonics(d, l_max, norm)
    rad = K[None] * np.exp(-(gamma[None] * d2[:, None, None]))
    prim = np.zeros((A, n_max, LM))
    for j in range(len(d2)):
        prim[tj[j]] += rad[j][:, l_of] * R[j][None, :]
    c = np.einsum("lnq,zql->znl", beta[l_of], prim)
    prod = c[z1, n1] * c[z2, n2]
    mask = l_of[None, :] == ll[:, None]
    return weight[ll] * np.where(mask, prod, 0.0).sum(1), c


def descriptors(cells, A, centres, tables, cut):
    """float64 restatement on a batch -> (desc [M, F], coeff [M, A, n_max, LM])"""
    ptr = np.concatenate([[0], np.cumsum([len(c["frac"]) for c in cells])])
    desc, coeff = [], []
    for i in centres:
        c = int(np.searchsorted(ptr, i, side="right")) - 1
        j, _, r = sites(cells[c], cut, int(i) - ptr[c])
        types = np.asarray(cells[c]["types"])
        d = np.concatenate([np.zeros((1, 3)), r])
        tj = np.concatenate([[types[int(i) - ptr[c]]], types[j]])
        p, co = descriptor_of_vectors(d, tj, A, tables)
        desc.append(p)
        coeff.append(co)
    return np.array(desc), np.array(coeff)


def running_mean(desc, cell_of_row, C):
    """the mean of egnn_cell_soap_mean: rows added in ascending order into a running sum, divided once"""
    out, count = np.zeros((C, desc.shape[1])), np.bincount(cell_of_row, minlength=C)
    for m in range(len(desc)):
        out[cell_of_row[m]] = out[cell_of_row[m]] + desc[m]
    nz = count > 0
    out[nz] = out[nz] / count[nz, None].astype(np.float64)
    return out, count


# ---- the host statements ------------------------------------------------------------------------------------------------------------
vp = SU.vp


def host_sites(L, cells, cut, centres, raw=None):
    """egnn_cell_sites_host (two calls: sizes, then lists) -> (rc, row_ptr, atom, code)"""
    a = STU.batch_arrays(cells)
    a.update(raw or {})
    cs = np.ascontiguousarray(centres, dtype=np.int32)
    row_ptr = np.full(len(cs) + 1, -7, np.int32)
    head = (len(a["cell_ptr"]) - 1, vp(a["cell_ptr"]), vp(a["lattice"]), vp(a["frac"]), float(cut), len(cs), vp(cs), vp(row_ptr))
    rc = L.egnn_cell_sites_host(*head, 0, None, None)
    if rc != 0:
        return rc, None, None, None
    T = int(row_ptr[-1])
    atom, code = np.full(max(T, 1), -7, np.int32), np.full(max(T, 1), -7, np.int32)
    rc = L.egnn_cell_sites_host(*head, T, vp(atom), vp(code))
    return rc, row_ptr, atom[:T], code[:T]


def host_soap(L, cells, A, cfg, flat, centres, cut=None, coeff=True, raw=None):
    """egnn_cell_soap_host -> (rc, desc, coeff | None)"""
    a = STU.batch_arrays(cells)
    a.update(raw or {})
    cs = np.ascontiguousarray(centres, dtype=np.int32)
    n_max, l_max = cfg["n_max"], cfg["l_max"]
    F = SU.features(A, n_max, l_max) if 1 <= A <= 4 else 1
    desc = np.full((len(cs), F), -7.0)
    co = np.full((len(cs), max(A, 1), n_max, (l_max + 1) ** 2), -7.0) if coeff else None
    rc = L.egnn_cell_soap_host(len(a["cell_ptr"]) - 1, A, vp(a["cell_ptr"]), vp(a["lattice"]), vp(a["frac"]), vp(a["type"]), n_max, l_max,
                               SU.neighbour_cut(cfg) if cut is None else float(cut), vp(flat), len(cs), vp(cs), vp(desc), vp(co))
    return rc, desc, co


def host_mean(L, desc, cell_rows, count, first, final, total):
    """egnn_cell_soap_mean_host: continues ``total`` [C, F] in place -> rc"""
    desc = np.ascontiguousarray(desc, dtype=np.float64)
    rows, cnt = np.ascontiguousarray(cell_rows, dtype=np.int32), np.ascontiguousarray(count, dtype=np.int64)
    return L.egnn_cell_soap_mean_host(len(rows) - 1, total.shape[1], vp(rows), vp(desc), vp(cnt), int(first), int(final), vp(total))


# ---- the truth and the host statement on it (computed once, never changed) ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    return np.load(GOLDEN)


@functools.lru_cache(maxsize=None)
def checked_fixture(name, A):
    """the fixture, checked against what the truth was computed on -> (cell, centres, cut)"""
    G, cell = golden(), fixture(name, A)
    assert np.array_equal(cell["lattice"], G[f"{name}_lattice"]) and np.array_equal(cell["frac"], G[f"{name}_frac"]), "the fixture moved"
    assert np.array_equal(cell["types"], G[f"{name}_A{A}_types"]), "the fixture moved"
    centres = centres_of(name, cell)
    assert np.array_equal(centres, G[f"{name}_centres"])
    return cell, centres, cut_of(name)


@functools.lru_cache(maxsize=None)
def host_on_golden(name, A):
    from diffusion_model_amd import _lib
    cell, centres, cut = checked_fixture(name, A)
    cfg = FIXTURES[name][0]
    rc, desc, coeff = host_soap(_lib.lib(), [cell], A, SU.CONFIGS[cfg], SU.tables(cfg)[1], centres)
    assert rc == 0, _lib.lib().egnn_last_error()
    return desc, coeff


@functools.lru_cache(maxsize=None)
def e_host(cfg):
    """E_host of one configuration: the host statement against the truth, the largest over its fixtures and their A"""
    G = golden()
    return max(SU.descriptor_error(host_on_golden(name, A)[0], G[f"{name}_A{A}_desc"])
               for name, (c, As, _) in FIXTURES.items() if c == cfg for A in As)


def bar(cfg):
    """the project's rule for the device: 8 x E_host, E_host capped at CAP by tests/test_cell_soap_host.py"""
    return 8.0 * e_host(cfg)

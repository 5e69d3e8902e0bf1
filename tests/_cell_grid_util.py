"""Callers of the linked-cell host entries (egnn_cell_grid_dims, egnn_cell_grid_host: csrc/cells/cell_grid_host.cpp) on batches of the
cell dicts of tests/_cells_util.py, and the cells the grid tests share (test infrastructure).  The expected values come from
elsewhere: tests/_cells_util.bonds, tests/_cell_stats_util.pair_counts and numpy's lexsort."""
import ctypes as C
import functools

import numpy as np

from tests import _cell_stats_util as SU
from tests import _cells_util as CU

_vp = lambda x: None if x is None else C.c_void_p(x.ctypes.data)


def dims(lib, cells, radius, reach=1, min_width=0.0, lattice=None):
    """egnn_cell_grid_dims -> (rc, nb int32 [C, 3])"""
    lat = np.ascontiguousarray(np.stack([np.asarray(c["lattice"], np.float64).reshape(9) for c in cells])) if lattice is None else lattice
    nb = np.full((len(lat), 3), -7, np.int32)
    rc = lib.egnn_cell_grid_dims(len(lat), _vp(lat), float(radius), int(reach), float(min_width), _vp(nb))
    return rc, nb


def host(lib, cells, radius, reach=1, min_width=0.0, bonds=False, dR=0.0, nbins=0, A=None):
    """egnn_cell_grid_host -> (rc, dict): nb, n_bins, atom_bin, bin_start, sorted_atom, sorted_frac; with ``bonds`` bond_ptr,
    bond_atom, bond_shift (two calls: sizes, then lists); with ``nbins`` counts.  Every output starts at -7 / NaN."""
    a = SU.batch_arrays(cells)
    Cn, N = len(cells), int(a["cell_ptr"][-1])
    A = max(c["A"] for c in cells) if A is None else A
    rc0, nb0 = dims(lib, cells, radius, reach, min_width)
    B = int(np.prod(nb0.astype(np.int64), axis=1).sum()) if rc0 == 0 else 0
    out = dict(nb=np.full((Cn, 3), -7, np.int32), n_bins=np.full(1, -7, np.int64), atom_bin=np.full(max(N, 1), -7, np.int32)[:N],
               bin_start=np.full(B + 1, -7, np.int32), sorted_atom=np.full(max(N, 1), -7, np.int32)[:N],
               sorted_frac=np.full((max(N, 1), 3), np.nan)[:N])
    bond_ptr = np.full(N + 1, -7, np.int32) if bonds else None
    counts = np.full((Cn, A, A, max(nbins, 1)), -7, np.int64) if nbins else None

    def call(cap, ba, bs):
        return lib.egnn_cell_grid_host(Cn, A, _vp(a["cell_ptr"]), _vp(a["lattice"]), _vp(a["frac"]), _vp(a["type"]), float(radius), int(reach),
                                       float(min_width), _vp(out["nb"]), _vp(out["n_bins"]), _vp(out["atom_bin"]) if N else None, B + 1,
                                       _vp(out["bin_start"]), _vp(out["sorted_atom"]) if N else None, _vp(out["sorted_frac"]) if N else None,
                                       _vp(bond_ptr), cap, _vp(ba), _vp(bs), float(dR), int(nbins), _vp(counts))

    rc = call(0, None, None)
    if rc != 0:
        return rc, None
    if bonds:
        E = int(bond_ptr[-1])
        ba, bs = np.full(max(E, 1), -7, np.int32), np.full(max(E, 1), -7, np.int32)
        rc = call(E, ba, bs)
        out.update(bond_ptr=bond_ptr, bond_atom=ba[:E], bond_shift=bs[:E])
    if nbins:
        out["counts"] = counts
    out["cell_ptr"] = a["cell_ptr"]
    return rc, out


def restated_bins(cell, nb):
    """numpy: flat bin of every atom, b_k = min(nb_k - 1, floor(wrap(f_k) nb_k))"""
    nb = np.asarray(nb, np.int64)
    b = np.minimum(np.floor(CU.wrap(cell["frac"]) * nb).astype(np.int64), nb - 1)
    return (b[:, 0] * nb[1] + b[:, 1]) * nb[2] + b[:, 2]


@functools.lru_cache(maxsize=None)
def cells():
    """the fixtures of the grid tests, by name"""
    return dict(cristobalite=CU.cristobalite_cell(), triclinic=CU.triclinic_cell(), r65=CU.random_cell(65, 11, spread=2.0),
                r160=CU.random_cell(160, 12), one=CU.one_atom_cell(), chain=CU.chain_cell(), dense9=CU.grid_cell(9, 9, 9, 0.75, 2.0))


@functools.lru_cache(maxsize=None)
def dense11():
    """1,331 atoms 0.6 A apart: 157-170 bonds per atom, beyond the 128 keys the fill kernel stages per row (3 s to build)"""
    return CU.grid_cell(11, 11, 11, 0.6, 2.0)


def displaced_cristobalite(m, seed=5):
    """beta-cristobalite m x m x m (a = 7.16 A), every fraction displaced by sigma = 0.01 / m: 24 m^3 atoms, built in numpy, without
    the restated bond list"""
    frac, types = CU._cristobalite_frac()
    off = np.array([[i, j, k] for i in range(m) for j in range(m) for k in range(m)], dtype=np.float64)
    f = ((frac[None, :, :] + off[:, None, :]) / m).reshape(-1, 3)
    f = f + (0.01 / m) * np.random.default_rng(seed).standard_normal(f.shape)
    return dict(lattice=7.16 * m * np.eye(3), frac=f, types=np.tile(types, len(off)).astype(np.int32), A=2, name=f"cristobalite-x{m}",
                cutoff=CU.CUTOFF)

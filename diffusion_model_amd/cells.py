"""Local environments of periodic cells: the constructor of the records everything else here consumes.

Every record the reference trains on is the excited oxygen plus the atoms reachable from it in 2, 3 or 4 hops of the "closer than
2.0 A" relation, cut out of a periodic cell (``make_dataset.py:79-142``: 3x3x3 supercell, full distance matrix,
``return_index_within_2ang``, nested Python loops, ONE centre per cell).  Here the cut is made on the device, about every centre
of a batch of cells (or every atom of one type, or any list of atoms), by ``csrc/cells/cell_env.hip``:

* ``bond_list``          -- the periodic bond list (CSR of (neighbour atom, lattice shift) per atom);
* ``local_environments`` -- the shell cluster about each centre, as one batch that goes straight into the model
  (``.batch()``), the samplers and ``stats.compare_structures`` (``.to_data_list()``).

``structure_factor`` (``csrc/eval/sq.hip``) is the reciprocal-space statistic of whole cells: rho_a on the reciprocal lattice and
its shell averages, finished to partial and total S(q); no file of the reference computes it.  ``pair_counts``, ``partial_rdf``,
``bond_statistics``, ``structure_profile`` and ``compare_structures`` (``csrc/cells/cell_stats.hip``) are its real-space
counterpart: g_ab(r) and the running coordination numbers over every image, CN histograms, bond angles and Q^n speciation of whole
cells; the reference has them about atom 0 of one cluster only.

The bond list and the pair counts come from kernels that test every atom of a cell against every centre, or -- ``method="grid"``,
and ``"auto"`` for large cells -- from ``csrc/cells/cell_grid.hip``, which bins the atoms on a grid and searches the neighbouring
bins only: O(n) instead of O(n^2), and bitwise the same outputs (``csrc/cells/cell_grid_math.h``).

``neighbour_sites`` / ``soap_descriptors`` (``csrc/cells/cell_soap.hip``) reach every image inside a radius; ``bond_order`` and
``bond_order_profile`` (``csrc/cells/cell_boo.hip``) compute Steinhardt's bond-orientational order over those sites: q_l, w_l, the
Lechner-Dellago averages and the ten Wolde-Frenkel solid-bond count (an extension: no file of the reference computes them).
``lattice_energy`` (``csrc/cells/cell_ewald.hip``) is the energy and the forces of a cell of point charges with a short-range pair
potential (``PairTable``; ``BKS`` for silica): an Ewald sum over those sites and over the reciprocal vectors of
``structure_factor`` (an extension: no file of the reference computes an energy); with ``stress=True`` also the strain derivative of
that energy, the stress tensor and the pressure (``csrc/cells/cell_stress_math.h``; ``strained`` builds the strained cells).
``relax`` (``csrc/cells/cell_relax.hip``) moves the atoms of fixed cells down that energy by FIRE, on the device, over site lists
that are held while no atom has moved further than half a skin (an extension: no file of the reference relaxes a structure).

The definitions (``csrc/cells/cell_math.h``) are those of the INFINITE lattice: a site is (atom, integer shift), a bond joins
sites closer than the cutoff, an environment is what ``shells`` bonds reach.  Wherever the reference's search uses no bond that
wraps round its 3x3x3 supercell the two site sets are identical; where it does, the reference aliases an image onto a site on the
far side of the supercell (a position about three cell lengths away) and this module does not follow it (INTEGRATION.md,
"Periodic cells").  Rows are ordered centre first, then by (atom index, shift): the reference's order is the iteration order of a
Python ``set``.

There is no CPU fallback: the functions need a ROCm device.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from ._batch import block_index
from .data import Batch, GraphData, make_graph


def lattice_from_parameters(a: float, b: float, c: float, alpha: float, beta: float, gamma: float) -> torch.Tensor:
    """Lattice vectors (rows a, b, c; float64 [3, 3]) from lengths in Angstrom and angles in degrees, in the convention of
    ``pymatgen.core.Lattice.from_parameters`` (what ``make_dataset.py:19,79`` calls): c along z, a in the xz-plane,
    a = (a sin beta, 0, a cos beta), b = (-b sin alpha cos gamma*, b sin alpha sin gamma*, b cos alpha) with
    cos gamma* = (cos alpha cos beta - cos gamma) / (sin alpha sin beta).  That library is not installed where this project is
    built: the convention is pinned by its documentation only, not by execution."""
    al, be, ga = (math.radians(float(v)) for v in (alpha, beta, gamma))
    val = (math.cos(al) * math.cos(be) - math.cos(ga)) / (math.sin(al) * math.sin(be))
    gs = math.acos(max(-1.0, min(1.0, val)))
    va = [a * math.sin(be), 0.0, a * math.cos(be)]
    vb = [-b * math.sin(al) * math.cos(gs), b * math.sin(al) * math.sin(gs), b * math.cos(al)]
    vc = [0.0, 0.0, float(c)]
    return torch.tensor([va, vb, vc], dtype=torch.float64)


class PeriodicCell:
    """One periodic cell: ``lattice`` float64 [3, 3] (rows a, b, c), ``frac`` float64 [n, 3] (any real value; wrapped to [0, 1)
    when used), ``types`` int32 [n] in [0, num_types).  The species are given either as ``species_onehot`` [n, A] (the reference's
    node feature: O = [1, 0], Si = [0, 1]) or as ``types`` (``num_types`` defaults to max + 1)."""

    def __init__(self, lattice, frac_coords, species_onehot=None, types=None, id=None, num_types: Optional[int] = None):
        self.lattice = torch.as_tensor(lattice, dtype=torch.float64).detach().cpu().reshape(3, 3).clone()
        self.frac = torch.as_tensor(frac_coords, dtype=torch.float64).detach().cpu().reshape(-1, 3).clone()
        n = self.frac.shape[0]
        if (species_onehot is None) == (types is None):
            raise ValueError("give species_onehot or types, not both")
        if species_onehot is not None:
            oh = torch.as_tensor(species_onehot).detach().cpu()
            if oh.dim() != 2 or oh.shape[0] != n or oh.shape[1] < 1:
                raise ValueError("species_onehot must be [n, A]")
            if n and not bool((((oh == 0) | (oh == 1)).all(1) & (oh.sum(1) == 1)).all()):
                raise ValueError("every row of species_onehot must be exactly one-hot")
            self.num_types = int(oh.shape[1]) if num_types is None else int(num_types)
            self.types = (oh.argmax(1) if n else torch.zeros(0, dtype=torch.long)).to(torch.int32)
        else:
            self.types = torch.as_tensor(types).detach().cpu().reshape(-1).to(torch.int32).clone()
            if self.types.shape[0] != n:
                raise ValueError("types must be [n]")
            self.num_types = (int(self.types.max()) + 1 if n else 1) if num_types is None else int(num_types)
        if n and (int(self.types.min()) < 0 or int(self.types.max()) >= self.num_types):
            raise ValueError(f"types must lie in [0, {self.num_types})")
        if not bool(torch.isfinite(self.frac).all()) or not bool(torch.isfinite(self.lattice).all()):
            raise ValueError("lattice and coordinates must be finite")
        self.id = id

    @classmethod
    def from_cartesian(cls, lattice, cart_coords, species_onehot=None, types=None, id=None, num_types=None) -> "PeriodicCell":
        """the same cell from Cartesian coordinates in Angstrom: frac = cart L^-1 in float64"""
        L = torch.as_tensor(lattice, dtype=torch.float64).detach().cpu().reshape(3, 3)
        cart = torch.as_tensor(cart_coords, dtype=torch.float64).detach().cpu().reshape(-1, 3)
        frac = torch.linalg.solve(L.T, cart.T).T if cart.shape[0] else cart
        return cls(L, frac, species_onehot=species_onehot, types=types, id=id, num_types=num_types)

    @property
    def num_atoms(self) -> int:
        return int(self.frac.shape[0])

    def __repr__(self):
        return f"PeriodicCell(n={self.num_atoms}, A={self.num_types}, id={self.id!r})"


def _as_cells(cells) -> List[PeriodicCell]:
    cells = [cells] if isinstance(cells, PeriodicCell) else list(cells)
    if not cells or not all(isinstance(c, PeriodicCell) for c in cells):
        raise ValueError("cells must be a PeriodicCell or a non-empty sequence of them")
    return cells


def _bond_tiles(sizes) -> np.ndarray:
    """the work list of egnn_cell_bonds_count / _fill (include/egnn_amd.h): {cell, first centre} for every block of 64 centres"""
    sz = np.asarray(sizes, dtype=np.int64)
    ci, t = block_index(-(-sz // _lib.CELL_CENTRE_BLOCK))
    return np.stack([ci, t * _lib.CELL_CENTRE_BLOCK], 1).astype(np.int32).reshape(-1, 2)


def _empty(n: int, *shape, dtype, device) -> torch.Tensor:
    """uninitialised [n, *shape]; a tensor of no rows still has storage behind it"""
    t = torch.empty(max(n, 1), *shape, dtype=dtype, device=device)
    return t if n else t[:0]   # no view in the common case: these calls run at a rate where one shows


def _ptr_or_none(t: Optional[torch.Tensor], n: Optional[int] = None):
    """the pointer of ``t`` for the library, None (NULL) where it holds nothing: ``n`` entries, by default its rows"""
    return _lib.ptr(t) if (t is not None and (t.shape[0] if n is None else n)) else None


class _CellBatch:
    """a batch of cells on the device: host and device copies of cell_ptr and the lattices, device copies of the coordinates,
    the types and the bond tiles"""

    def __init__(self, cells, device):
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError("periodic-cell environments need an AMD GPU ('cuda' device); there is no CPU fallback")
        self.cells, self.dev = cells, dev
        self.sizes = [c.num_atoms for c in cells]
        self.C, self.N = len(cells), sum(self.sizes)
        self.A = max(c.num_types for c in cells)
        self.cell_ptr_h = torch.zeros(self.C + 1, dtype=torch.int32)
        self.cell_ptr_h[1:] = torch.cumsum(torch.tensor(self.sizes, dtype=torch.int64), 0).to(torch.int32)
        self.lattice_h = torch.stack([c.lattice.reshape(9) for c in cells]).contiguous()
        self.types_h = torch.cat([c.types for c in cells]).contiguous()
        tiles = _bond_tiles(self.sizes)
        self.n_tiles = len(tiles)
        self.cell_ptr = self.cell_ptr_h.to(dev)
        self.lattice = self.lattice_h.to(dev)
        self.frac = torch.cat([c.frac for c in cells]).contiguous().to(dev)
        self.types = self.types_h.to(dev)
        self.tiles = torch.from_numpy(tiles).to(dev)
        self._host_ptrs = (_lib.ptr(self.cell_ptr_h), _lib.ptr(self.lattice_h))
        self._dev_ptrs = (_lib.ptr(self.cell_ptr), _lib.ptr(self.lattice), _ptr_or_none(self.frac, self.N), _ptr_or_none(self.types, self.N))

    def args(self, A: bool = False, lattice=True, frac: bool = True, types: bool = False, host=(), dev=()):
        """the argument prefix the entries of include/egnn_amd.h share: (stream, C, N[, A], the HOST copies cell_ptr[, lattice],
        *host, the device arrays cell_ptr[, lattice], *dev[, frac][, types]).  ``lattice``: True, False, or "host" for an entry
        that reads no lattice on the device; ``host`` / ``dev``: what an entry takes right after the two groups (grids, plans)."""
        hp, dp = self._host_ptrs, self._dev_ptrs   # taken once: the entries are called at a rate where building them shows
        return ((_lib.stream_ptr(), self.C, self.N) + ((self.A,) if A else ()) + (hp if lattice else hp[:1]) + tuple(host) +
                (dp[:2] if lattice is True else dp[:1]) + tuple(dev) + (dp[2:3] if frac else ()) + (dp[3:] if types else ()))


# ---- linked-cell search (csrc/cells/cell_grid.hip) ---------------------------------------------------------------------------------
# "auto" sends a cell to the grid kernels when it is griddable and holds at least this many atoms; the results are bitwise the same
# either way.  Measured by tools/cell_grid_time.py (profiles/cell_grid_time.json, README "Periodic cells") on one cell of 3,000 /
# 24,000 / 192,000 atoms, whole calls: the bond list wins from 3,000 atoms (0.33 against 0.74 ms; 0.35 against 5.1 ms at 24,000), the
# pair counts lose at 3,000 (0.37 against 0.30 ms) and win at 24,000 (0.40 against 1.41 ms).  24,000 is the smallest measured size at
# which both win by more than the spread of the rounds; rounded up to a power of two.  Never below 2,048.
_GRID_MIN_ATOMS = 32768
_GRID_BOND_MIN_WIDTH = 0.0    # bond list: bins at least this thick (A); 0 = as fine as the cutoff allows (fastest of 0 / 3 / 4 A at 24,000 atoms)
_GRID_PAIR_REACH = 2          # pair counts: bins of R / 2 walked two to each side (fastest of reach 1 / 2 / 3 at every measured size)
_GRID_PAIR_MIN_WIDTH = 0.0
_METHODS = ("auto", "direct", "grid")


def _check_method(method: str) -> str:
    if method not in _METHODS:
        raise ValueError(f"method must be one of {_METHODS}, not {method!r}")
    return method


def _widths(lattice):
    """cell_widths (csrc/cells/cell_math.h) restated in numpy, for messages and work lists only: lattices [..., 3, 3] -> (the
    perpendicular widths float64 [C, 3], singular bool [C]: |det| <= 1e-9 |a||b||c| or not finite; its widths mean nothing)"""
    L = np.asarray(lattice, dtype=np.float64).reshape(-1, 3, 3)
    det, faces = _width_parts(L, (0, 1, 2))
    scale = np.prod(np.linalg.norm(L, axis=2), axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = det[:, None] / np.stack(faces, 1)
    return w, ~(scale < 1e300) | ~(det > 1e-9 * scale)


def _width_parts(L: np.ndarray, axes):
    """lattices [C, 3, 3] -> (|det| [C], the face areas |a_{k+1} x a_{k+2}| [C] of the axes k asked for): w_k = |det| / face_k.
    The work lists are built on every call and ask for the one axis they need."""
    cross = {k: np.cross(L[:, (k + 1) % 3], L[:, (k + 2) % 3]) for k in set(axes) | {0}}
    det = np.abs(np.einsum("ck,ck->c", L[:, 0], cross[0]))
    return det, [np.linalg.norm(cross[k], axis=1) for k in axes]


def _grid_cells(cb: "_CellBatch", method: str, radius: float, reach: int, min_width: float) -> Optional[np.ndarray]:
    """the grids of the cells that take the grid path: int32 [C, 3], rows of zeros for the cells left to the direct kernels; None
    where no cell takes it.  "grid" raises ValueError for a cell that is not griddable; "auto" takes a cell that is griddable and
    holds at least _GRID_MIN_ATOMS atoms."""
    if _check_method(method) == "direct":
        return None
    nb = torch.zeros(cb.C, 3, dtype=torch.int32)
    _lib.check(_lib.lib().egnn_cell_grid_dims(cb.C, _lib.ptr(cb.lattice_h), float(radius), int(reach), float(min_width), _lib.ptr(nb)))
    nb = nb.numpy()
    ok = nb[:, 0] > 0
    if method == "grid":
        if not ok.all():
            c = int(np.nonzero(~ok)[0][0])
            w = _widths(cb.lattice_h[c].numpy())[0][0]
            raise ValueError(f"cell {c}: perpendicular widths {w[0]:.6g}, {w[1]:.6g}, {w[2]:.6g} A hold fewer than {2 * int(reach) + 1} bins of "
                             f"{max(float(radius) / int(reach), float(min_width)):.6g} A on an axis: not griddable at radius {float(radius):.6g} "
                             f"and reach {int(reach)} (use method='direct' or 'auto')")
    else:
        ok = ok & (np.asarray(cb.sizes, dtype=np.int64) >= _GRID_MIN_ATOMS)
    if not ok.any():
        return None
    return np.where(ok[:, None], nb, 0).astype(np.int32)


class _CellGrid:
    """the cells of a batch that take the grid path, binned and sorted on the device (egnn_cell_grid_count, the prefix sum over all
    bins, egnn_cell_grid_fill), and their {cell, first sorted centre} tiles"""

    def __init__(self, cb: "_CellBatch", nb: np.ndarray, radius: float, reach: int):
        lib, dev, N = _lib.lib(), cb.dev, cb.N
        self.mask = nb[:, 0] > 0
        self.radius, self.reach = float(radius), int(reach)
        self.nb_h = torch.from_numpy(np.ascontiguousarray(nb, dtype=np.int32))
        bin_ptr = np.zeros(cb.C + 1, dtype=np.int64)
        bin_ptr[1:] = np.cumsum(np.prod(nb.astype(np.int64), axis=1))
        if bin_ptr[-1] >= 2 ** 31 - 1:
            raise ValueError("more than 2^31 - 2 bins in the batch (fewer cells per call)")
        self.n_bins = B = int(bin_ptr[-1])
        self.nb, self.bin_ptr = self.nb_h.to(dev), torch.from_numpy(bin_ptr.astype(np.int32)).to(dev)
        self.atom_bin = atom_bin = _empty(N, dtype=torch.int32, device=dev)
        bin_count = _empty(B, dtype=torch.int32, device=dev)
        head = cb.args(lattice="host", host=(_lib.ptr(self.nb_h), self.radius, self.reach), dev=(_lib.ptr(self.nb), _lib.ptr(self.bin_ptr)))
        _lib.check(lib.egnn_cell_grid_count(*head, B, _ptr_or_none(atom_bin), _ptr_or_none(bin_count)))
        self.bin_start = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        if B:
            self.bin_start[1:] = torch.cumsum(bin_count.long(), 0).to(torch.int32)
        work = _empty(B + N, dtype=torch.int32, device=dev)
        # the walking kernels index the sorted arrays: they keep their storage where N = 0
        self.sorted_atom = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
        self.sorted_frac = torch.empty(max(N, 1), 3, dtype=torch.float64, device=dev)
        self.sorted_type = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
        _lib.check(lib.egnn_cell_grid_fill(*head, _ptr_or_none(cb.types, N), B, _lib.ptr(self.bin_start), _ptr_or_none(atom_bin), _lib.ptr(work),
                                           *(_ptr_or_none(t, N) for t in (self.sorted_atom, self.sorted_frac, self.sorted_type))))
        self.tiles_h = torch.from_numpy(_bond_tiles(np.where(self.mask, np.asarray(cb.sizes, dtype=np.int64), 0)))
        self.n_tiles, self.tiles = len(self.tiles_h), self.tiles_h.to(dev)

    def args(self, cb: "_CellBatch", A: bool = False):
        """the arguments the walking entries share: the batch's prefix with the HOST copies of the grids and tiles, and the device
        arrays up to n_bins and bin_start"""
        return cb.args(A=A, frac=False, host=(_lib.ptr(self.nb_h), _ptr_or_none(self.tiles_h)),
                       dev=(_lib.ptr(self.nb), _lib.ptr(self.bin_ptr), self.n_bins, _lib.ptr(self.bin_start)))


class BondList:
    """CSR of the periodic bonds of a batch of cells: ``row_ptr`` int32 [N+1]; ``atom`` int32 [E], the neighbour as an index into
    the concatenated atoms of the batch; ``shift`` int32 [E, 3], the lattice shift of the neighbour's image relative to the wrapped
    atoms; ``shift_code`` int32 [E] (csrc/cells/cell_math.h); ``cell_ptr`` int32 [C+1] (host).  Rows ascend by (atom, shift)."""

    def __init__(self, row_ptr, atom, shift_code, cell_ptr):
        self.row_ptr, self.atom, self.shift_code, self.cell_ptr = row_ptr, atom, shift_code, cell_ptr

    @property
    def shift(self) -> torch.Tensor:
        return decode_shift(self.shift_code)

    @property
    def num_bonds(self) -> int:
        return int(self.atom.shape[0])


def decode_shift(code: torch.Tensor) -> torch.Tensor:
    """shift codes ((sx + 4) 9 + (sy + 4)) 9 + (sz + 4) -> int32 [..., 3]"""
    c = code.to(torch.int32)
    return torch.stack((c // 81 - 4, c // 9 % 9 - 4, c % 9 - 4), -1)


def _bond_args(cb: _CellBatch, cutoff: float, tiles: Optional[torch.Tensor] = None):
    tiles = cb.tiles if tiles is None else tiles
    return (*cb.args(), float(cutoff), _ptr_or_none(tiles), len(tiles))


def _grid_bond_args(cb: _CellBatch, grid: _CellGrid, cutoff: float):
    return (*grid.args(cb), _lib.ptr(grid.sorted_atom), _lib.ptr(grid.sorted_frac), float(cutoff), grid.reach, _ptr_or_none(grid.tiles), grid.n_tiles)


def _bonds_count(cb: _CellBatch, cutoff: float) -> torch.Tensor:
    deg = torch.empty(cb.N, dtype=torch.int32, device=cb.dev)
    _lib.check(_lib.lib().egnn_cell_bonds_count(*_bond_args(cb, cutoff), _lib.ptr(deg)))
    return deg


def _bonds_fill(cb: _CellBatch, cutoff: float, row_ptr: torch.Tensor, E: int):
    atom, code = (_empty(E, dtype=torch.int32, device=cb.dev) for _ in range(2))
    _lib.check(_lib.lib().egnn_cell_bonds_fill(*_bond_args(cb, cutoff), _lib.ptr(row_ptr), E, _ptr_or_none(atom), _ptr_or_none(code)))
    return atom, code


def _row_ptr(cb: _CellBatch, deg: torch.Tensor):
    row_ptr = torch.zeros(cb.N + 1, dtype=torch.int32, device=cb.dev)
    total = torch.cumsum(deg.long(), 0)
    E = int(total[-1]) if cb.N else 0
    if E >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 bonds")
    row_ptr[1:] = total.to(torch.int32)
    return row_ptr, E


def _bond_list(cb: _CellBatch, cutoff: float, method: str = "direct", reach: int = 1, min_width: Optional[float] = None) -> BondList:
    """``method`` chooses per cell between the direct kernels and the linked-cell ones (the same bits either way); ``reach`` and
    ``min_width`` are the knobs of the grid (private: tests and tools/cell_grid_time.py pin every branch with them)"""
    nb = _grid_cells(cb, method, cutoff, reach, _GRID_BOND_MIN_WIDTH if min_width is None else min_width)
    if nb is None:
        deg = _bonds_count(cb, cutoff)
        row_ptr, E = _row_ptr(cb, deg)
        atom, code = _bonds_fill(cb, cutoff, row_ptr, E)
        return BondList(row_ptr, atom, code, cb.cell_ptr_h)
    # a mixed batch: two launches into the same degrees, two into the same lists
    lib = _lib.lib()
    grid = _CellGrid(cb, nb, cutoff, reach)
    direct = torch.from_numpy(_bond_tiles(np.where(grid.mask, 0, np.asarray(cb.sizes, dtype=np.int64)))).to(cb.dev)
    deg = torch.zeros(max(cb.N, 1), dtype=torch.int32, device=cb.dev)[:cb.N]
    if len(direct):
        _lib.check(lib.egnn_cell_bonds_count(*_bond_args(cb, cutoff, direct), _lib.ptr(deg)))   # zeroes every degree, then its own centres
    _lib.check(lib.egnn_cell_bonds_grid_count(*_grid_bond_args(cb, grid, cutoff), _lib.ptr(deg)))
    row_ptr, E = _row_ptr(cb, deg)
    atom, code = (_empty(E, dtype=torch.int32, device=cb.dev) for _ in range(2))
    lists = (_lib.ptr(row_ptr), E, _ptr_or_none(atom), _ptr_or_none(code))
    if len(direct):
        _lib.check(lib.egnn_cell_bonds_fill(*_bond_args(cb, cutoff, direct), *lists))
    _lib.check(lib.egnn_cell_bonds_grid_fill(*_grid_bond_args(cb, grid, cutoff), *lists))
    return BondList(row_ptr, atom, code, cb.cell_ptr_h)


def _env_args(cb: _CellBatch, bonds: BondList, cc: torch.Tensor, shells: int, max_atoms: int):
    """the arguments the two environment entries share after the cell arrays: the bond list, the centres ``cc`` int32 [2, M] =
    (cell, atom) on the device, shells, max_atoms"""
    E, M = bonds.num_bonds, int(cc.shape[1])
    return (_lib.ptr(bonds.row_ptr), E, _ptr_or_none(bonds.atom, E), _ptr_or_none(bonds.shift_code, E), M, _ptr_or_none(cc[0], M),
            _ptr_or_none(cc[1], M), int(shells), int(max_atoms))


def _env_count(cb: _CellBatch, bonds: BondList, cc: torch.Tensor, shells: int, max_atoms: int) -> torch.Tensor:
    M = int(cc.shape[1])
    size = _empty(M, dtype=torch.int32, device=cb.dev)
    _lib.check(_lib.lib().egnn_cell_env_count(*cb.args(lattice=False, frac=False), *_env_args(cb, bonds, cc, shells, max_atoms), _ptr_or_none(size, M)))
    return size


def _env_fill(cb: _CellBatch, bonds: BondList, cc: torch.Tensor, shells: int, max_atoms: int, env_ptr: torch.Tensor, T: int):
    """-> (atom, shift code, type: int32 [T]; pos float32 [T, 3])"""
    e_atom, e_code, e_type = (_empty(T, dtype=torch.int32, device=cb.dev) for _ in range(3))
    pos = _empty(T, 3, dtype=torch.float32, device=cb.dev)
    _lib.check(_lib.lib().egnn_cell_env_fill(*cb.args(A=True, types=True), *_env_args(cb, bonds, cc, shells, max_atoms), _lib.ptr(env_ptr), T,
                                             *(_ptr_or_none(t, T) for t in (e_atom, e_code, e_type, pos))))
    return e_atom, e_code, e_type, pos


def bond_list(cells: Union[PeriodicCell, Sequence[PeriodicCell]], cutoff: float = 2.0, device=None, method: str = "auto") -> BondList:
    """The periodic bond list of every atom of a batch of cells (``return_index_within_2ang`` over the distance matrix of
    ``make_dataset.py:50-57,99``, without the matrix): image (j, s), s in {-1, 0, 1}^3, of atom j is bonded to atom i iff it is
    closer than ``cutoff`` in fp64 and is not i itself.  A cell with a perpendicular width below ``cutoff`` (27 images would not
    hold every bond) or a singular lattice is refused (``EgnnError``, naming the cell).

    ``method``: "direct" tests every atom of a cell against every centre; "grid" bins the atoms and searches the neighbouring bins
    (csrc/cells/cell_grid.hip; O(n), and ValueError naming the cell and its widths where a cell is too thin to be gridded); "auto"
    (the default) chooses per cell -- the grid for a griddable cell of at least ``_GRID_MIN_ATOMS`` atoms.  The outputs are bitwise
    the same whichever way a cell goes."""
    _check_method(method)
    return _bond_list(_CellBatch(_as_cells(cells), device), cutoff, method)


def _centres(cb: _CellBatch, centres):
    """-> (int64 [M] indices into the concatenated atoms, int64 [M] cells), on the host"""
    if centres is None:
        idx = torch.arange(cb.N, dtype=torch.int64)
    elif isinstance(centres, (int, np.integer)) and not isinstance(centres, bool):
        if not 0 <= int(centres) < cb.A:
            raise ValueError(f"centre type {int(centres)} outside [0, {cb.A})")
        idx = torch.nonzero(cb.types_h == int(centres)).reshape(-1)
    else:
        idx = torch.as_tensor(centres).detach().cpu().reshape(-1).to(torch.int64)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= cb.N):
            raise ValueError(f"a centre lies outside the {cb.N} atoms of the batch")
    cell = torch.searchsorted(cb.cell_ptr_h.long(), idx, right=True) - 1
    return idx, cell


class EnvironmentBatch:
    """The environments of M centres, concatenated (T rows): ``pos`` float32 [T, 3] relative to the centre, ``x`` int64 [T, A]
    one-hot species, ``exO`` float32 [T, 1] (1 for the centre, row 0 of every environment) on the device; ``sizes`` (list) and
    ``ptr`` int64 [M+1] on the host; the provenance of every row, ``atom`` int64 [T] (index inside its cell) and ``shift`` int32
    [T, 3] (lattice shift of the image, relative to the wrapped atoms; ``shift_code`` int32 [T] is its code), on the device; ``centre_cell`` / ``centre_atom`` int64 [M]
    on the host; ``id`` (list of (cell id, atom)); ``bonds``, the ``BondList`` of the cells."""

    def __init__(self, pos, x, exO, sizes, ptr, atom, shift, shift_code, centre_cell, centre_atom, id, bonds):
        self.pos, self.x, self.exO, self.sizes, self.ptr = pos, x, exO, sizes, ptr
        self.atom, self.shift, self.shift_code = atom, shift, shift_code
        self.centre_cell, self.centre_atom, self.id, self.bonds = centre_cell, centre_atom, id, bonds

    @property
    def num_graphs(self) -> int:
        return len(self.sizes)

    def to_data_list(self) -> List[GraphData]:
        """one ``GraphData`` per centre in ``make_graph``'s schema (make_dataset.py:121-142 without the spectrum)"""
        x, pos = self.x.cpu(), self.pos.cpu()
        out = []
        for m in range(self.num_graphs):
            lo, hi = int(self.ptr[m]), int(self.ptr[m + 1])
            out.append(make_graph(x[lo:hi], pos[lo:hi], graph_id=self.id[m]))
        return out

    def batch(self) -> Batch:
        """the fully connected ``data.Batch`` of these environments, its graph plan built on the device from the sizes: no edge
        list is made on, or copied from, the host"""
        from .graph import fully_connected_plan, plan_edge_index
        if self.num_graphs == 0:
            raise ValueError("no environment to batch")
        dev = self.pos.device
        out = Batch()
        out.x, out.pos, out.exO = self.x, self.pos, self.exO
        out.fully_connected = True
        out._plan = fully_connected_plan(self.sizes, dev)
        out.edge_index = plan_edge_index(out._plan)
        out.batch = out._plan.batch
        out.ptr, out.sizes, out.num_graphs, out.id = self.ptr.clone(), list(self.sizes), self.num_graphs, list(self.id)
        return out


def local_environments(cells: Union[PeriodicCell, Sequence[PeriodicCell]], centres=None, shells: int = 2, cutoff: float = 2.0,
                       max_atoms: int = 256, device=None, method: str = "auto") -> EnvironmentBatch:
    """The environment of every requested centre: the centre plus the sites (atom, lattice shift) reachable from it in at most
    ``shells`` (1..4) bonds of the infinite lattice -- ``make_dataset.py:101-107`` (2NN), ``:177-188`` (3NN), ``:258-272`` (4NN)
    -- with positions ``float32((frac_j - frac_i + shift) L)`` relative to the centre (``:111``).

    ``centres``: None = every atom of every cell; an int = every atom of that type index (0 = O in the reference's one-hot);
    or an index tensor into the concatenated atoms of ``cells`` -- any order, duplicates allowed; the outputs follow its order.
    A centre without a bond yields a one-atom environment (the reference's drivers skip those; filter on ``sizes``).  A centre
    whose environment exceeds ``max_atoms`` (<= 1024) raises ValueError naming cell and atom.  ``method`` chooses how the bond list
    is built (``bond_list``)."""
    _check_method(method)
    cb = _CellBatch(_as_cells(cells), device)
    shells, max_atoms = int(shells), int(max_atoms)
    bonds = _bond_list(cb, cutoff, method)
    idx_h, cell_h = _centres(cb, centres)
    M = int(idx_h.numel())
    cc = torch.stack((cell_h, idx_h)).to(torch.int32).to(cb.dev)
    size_h = _env_count(cb, bonds, cc, shells, max_atoms).cpu().long()
    local_h = idx_h - cb.cell_ptr_h.long()[cell_h]
    over = torch.nonzero(size_h > max_atoms).reshape(-1)
    if over.numel():
        m = int(over[0])
        raise ValueError(f"cell {int(cell_h[m])}, atom {int(local_h[m])}: the environment of {shells} shells holds more than "
                         f"max_atoms = {max_atoms} sites ({int(over.numel())} such centre(s)); raise max_atoms (at most "
                         f"{_lib.CELL_MAX_ENV_ATOMS}) or lower shells / cutoff")
    ptr_h = torch.zeros(M + 1, dtype=torch.int64)
    ptr_h[1:] = torch.cumsum(size_h, 0)
    T = int(ptr_h[-1])
    if T >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 rows")
    env_ptr = ptr_h.to(torch.int32).to(cb.dev)
    e_atom, e_code, e_type, pos = _env_fill(cb, bonds, cc, shells, max_atoms, env_ptr, T)
    row_cell = torch.repeat_interleave(cell_h.to(cb.dev), size_h.to(cb.dev), output_size=T)
    exO = torch.zeros(T, 1, dtype=torch.float32, device=cb.dev)
    if M:
        exO[ptr_h[:-1].to(cb.dev)] = 1.0
    ids = [(cb.cells[c].id, a) for c, a in zip(cell_h.tolist(), local_h.tolist())]
    return EnvironmentBatch(pos=pos, x=torch.nn.functional.one_hot(e_type.long(), cb.A), exO=exO, sizes=size_h.tolist(), ptr=ptr_h,
                            atom=e_atom.long() - cb.cell_ptr.long()[row_cell], shift=decode_shift(e_code), shift_code=e_code,
                            centre_cell=cell_h, centre_atom=local_h, id=ids, bonds=bonds)


def ring_statistics(cells: Union[PeriodicCell, Sequence[PeriodicCell]], centres=None, cutoff: float = 2.0, max_size: int = 16,
                    max_sites: int = 4096, device=None, method: str = "auto"):
    """Shortest-path ring statistics on the infinite lattice of every cell (``stats.ring_statistics`` states the definition; not in
    the reference): the bond list is ``bond_list``'s, a site is (atom, lattice shift), and a ring closes only where the very same
    site is reached -- an image is never folded onto its atom, so a cell smaller than its rings gives the rings of the crystal,
    not of the torus (ideal beta-cristobalite in its 24-atom cell: size 12 through every angle).  ``centres`` as in
    ``local_environments``: None, a type index, or an index tensor into the concatenated atoms.  -> ``RingStatistics``.  Raises
    ValueError naming cell and atom where an atom has more than 32 bonds or a search labels more than ``max_sites`` (<= 4096)
    sites.  ``method`` chooses how the bond list is built (``bond_list``)."""
    from . import _rings
    _check_method(method)
    cb = _CellBatch(_as_cells(cells), device)
    bonds = _bond_list(cb, cutoff, method)
    idx_h, cell_h = _centres(cb, centres)
    local_h = idx_h - cb.cell_ptr_h.long()[cell_h]

    def describe(m, limit):
        head = f"cell {int(cell_h[m])}, atom {int(local_h[m])}: "
        if limit == "degree":
            return head + "more than 32 bonds; no ring is searched (lower the cutoff)"
        return head + (f"a ring search labelled more than max_sites = {int(max_sites)} sites; raise max_sites (at most "
                       f"{_lib.RING_MAX_SITES}) or lower max_size / cutoff")

    return _rings.run(bonds.row_ptr, bonds.atom, bonds.shift.contiguous(), cb.types, cb.A, idx_h, max_size, max_sites, describe)


# ---- structure factors of periodic cells (csrc/eval/sq.hip) ---------------------------------------------------------
def _sq_vector_tiles(counts) -> np.ndarray:
    """the work list of egnn_sq_cell_rho (include/egnn_amd.h): {cell, first vector (local)} for every block of 256 vectors"""
    cnt = np.asarray(counts, dtype=np.int64)
    ci, t = block_index(-(-cnt // _lib.SQ_VECTOR_BLOCK))
    return np.stack([ci, t * _lib.SQ_VECTOR_BLOCK], 1).astype(np.int32).reshape(-1, 2)


class _SqVectors:
    """the reciprocal vectors of a batch of cells below ``q_max``: plan, count pass, prefix sums and the work list of blocks of 256
    vectors; ``name`` is what the caller calls the bound"""

    def __init__(self, cb: _CellBatch, q_max: float, name: str = "q_max"):
        lib = _lib.lib()
        self.cb, self.q_max = cb, q_max
        self.plan_h, n_rows_h = torch.zeros(cb.C, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
        _lib.check(lib.egnn_sq_cell_plan(cb.C, _lib.ptr(cb.lattice_h), q_max, _lib.ptr(self.plan_h), _lib.ptr(n_rows_h)))
        self.n_rows, self.plan = int(n_rows_h), self.plan_h.to(cb.dev)
        row_count = torch.empty(self.n_rows, dtype=torch.int32, device=cb.dev)
        _lib.check(lib.egnn_sq_cell_count(_lib.stream_ptr(), cb.C, _lib.ptr(cb.lattice_h), _lib.ptr(self.plan_h), _lib.ptr(cb.lattice),
                                          _lib.ptr(self.plan), q_max, self.n_rows, _lib.ptr(row_count)))
        row_ptr64 = torch.zeros(self.n_rows + 1, dtype=torch.int64, device=cb.dev)
        row_ptr64[1:] = torch.cumsum(row_count.long(), 0)
        first = torch.cat([self.plan_h[:, 3].long(), torch.tensor([self.n_rows])]).to(cb.dev)
        self.vec_ptr64 = row_ptr64[first].cpu()
        self.counts = (self.vec_ptr64[1:] - self.vec_ptr64[:-1]).tolist()
        for c, n in enumerate(self.counts):
            if n > _lib.SQ_MAX_VECTORS:
                raise ValueError(f"cell {c}: {n} reciprocal vectors below {name} = {q_max} (at most {_lib.SQ_MAX_VECTORS}; lower {name})")
        self.K = K = int(self.vec_ptr64[-1])
        if K >= 2 ** 31:
            raise ValueError("more than 2^31 - 1 reciprocal vectors in the batch (fewer cells per call)")
        self.vec_ptr_h = self.vec_ptr64.to(torch.int32)
        self.vec_ptr, self.row_ptr = self.vec_ptr_h.to(cb.dev), row_ptr64.to(torch.int32)
        tiles_h = _sq_vector_tiles(self.counts)
        self.n_tiles, self.tiles = len(tiles_h), torch.from_numpy(tiles_h).to(cb.dev)


class _SqCellRun(_SqVectors):
    """the vectors of a batch of cells and the outputs of the structure-factor launches, allocated; ``rho()`` and ``shells()`` are the
    launches alone"""

    def __init__(self, cb: _CellBatch, q_max: float, dq: float, nbins: int):
        super().__init__(cb, q_max)
        self.dq, self.nbins, K = dq, nbins, self.K
        self.hkl = _empty(K, 3, dtype=torch.int32, device=cb.dev)
        self.kabs = _empty(K, dtype=torch.float64, device=cb.dev)
        self.bins = _empty(K, dtype=torch.int32, device=cb.dev)
        self.rho_out = _empty(K, cb.A, 2, dtype=torch.float64, device=cb.dev)

    def rho(self):
        cb = self.cb
        head = cb.args(A=True, types=True, host=(_lib.ptr(self.plan_h), _lib.ptr(self.vec_ptr_h)), dev=(_lib.ptr(self.plan), _lib.ptr(self.vec_ptr)))
        _lib.check(_lib.lib().egnn_sq_cell_rho(*head, self.q_max, self.dq, self.nbins, self.n_rows, _lib.ptr(self.row_ptr), self.K,
                                               _ptr_or_none(self.tiles), self.n_tiles,
                                               *(_ptr_or_none(t) for t in (self.hkl, self.kabs, self.bins, self.rho_out))))

    def shells(self):
        cb, K, A, nbins = self.cb, self.K, self.cb.A, self.nbins
        count = torch.empty(cb.C, nbins, dtype=torch.int64, device=cb.dev)
        mean_k = torch.empty(cb.C, nbins, dtype=torch.float64, device=cb.dev)
        s = torch.empty(cb.C, A, A, nbins, dtype=torch.float64, device=cb.dev)
        _lib.check(_lib.lib().egnn_sq_cell_shells(_lib.stream_ptr(), cb.C, A, nbins, _lib.ptr(self.vec_ptr_h), _lib.ptr(self.vec_ptr), K,
                                                  *(_ptr_or_none(t) for t in (self.kabs, self.bins, self.rho_out)), _lib.ptr(count),
                                                  _lib.ptr(mean_k), _lib.ptr(s)))
        return count, mean_k, s


def structure_factor(cells, q_max: float = 15.0, dq: float = 0.05, weights=None, form: str = "faber-ziman", vectors: bool = False,
                     device=None):
    """Static structure factors of periodic cells on their reciprocal lattices (csrc/eval/sq_math.h): for every integer vector
    m = (h, k, l) of the half space with |k_m| < q_max, k_m = 2 pi m L^-T, rho_a(m) = sum_{j in a} exp(-i k_m . r_j); shell bin
    floor(|k_m| / dq), nbins = ceil(q_max / dq) <= 4096.  -> a namespace with q float64 [nbins] (bin centres), mean_k and count
    (int64, over the full sphere) [C, nbins], s [C, A, A, nbins] = the shell mean of Re(rho_a rho_b*), partial [C, A, A, nbins] and
    total [C, nbins] from D_ab = s_ab - delta_ab N_a in the forms and with the weights of stats.structure_factor, n_type [C, A],
    sizes; an empty shell has count 0 and NaN means.  ``vectors=True`` adds hkl int32 [K, 3], k float64 [K], bin int32 [K], rho
    complex128 [K, A] and vec_ptr int64 [C+1] (host), cell by cell and ascending (h, k, l).  q_max must keep
    floor(q_max |a_i| / 2 pi) <= 1023 and at most 2^24 vectors per cell."""
    from types import SimpleNamespace
    from .stats import _sf_finish, _sf_weights
    cells = _as_cells(cells)
    q_max, dq = float(q_max), float(dq)
    if not (q_max > 0 and math.isfinite(q_max) and dq > 0 and math.isfinite(dq)):
        raise ValueError("q_max and dq must be positive and finite")
    nbins = math.ceil(q_max / dq)
    if nbins > _lib.SQ_MAX_BINS:
        raise ValueError(f"ceil(q_max / dq) = {nbins} shell bins (at most {_lib.SQ_MAX_BINS})")
    for c, cell in enumerate(cells):
        if cell.num_types > _lib.SQ_MAX_TYPES:
            raise ValueError(f"cell {c}: {cell.num_types} atom types (at most {_lib.SQ_MAX_TYPES})")
        L = cell.lattice
        if abs(float(torch.linalg.det(L))) <= 1e-9 * float(L.norm(dim=1).prod()):
            raise ValueError(f"cell {c}: singular lattice")
        need = int(math.floor(q_max * float(L.norm(dim=1).max()) / (2 * math.pi)))
        if need > 1023:
            raise ValueError(f"cell {c}: q_max = {q_max} needs a Miller index of {need} (at most 1023)")
    cb = _CellBatch(cells, device)
    _sf_weights(weights, cb.A, nbins, cb.dev)   # a bad shape fails before the launch
    run = _SqCellRun(cb, q_max, dq, nbins)
    run.rho()
    count, mean_k, s = run.shells()
    A, K, hkl, kabs, bins, rho, vec_ptr64 = cb.A, run.K, run.hkl, run.kabs, run.bins, run.rho_out, run.vec_ptr64
    n_type_h = torch.stack([torch.bincount(c.types.long(), minlength=A)[:A] for c in cells])
    n_type = n_type_h.to(cb.dev)
    D = s - torch.diag_embed(n_type.to(torch.float64))[..., None]
    partial, total = _sf_finish(D, n_type, weights, form)
    out = SimpleNamespace(q=(torch.arange(nbins, dtype=torch.float64, device=cb.dev) + 0.5) * dq, mean_k=mean_k, count=count, s=s,
                          partial=partial, total=total, n_type=n_type, sizes=list(cb.sizes))
    if vectors:
        out.hkl, out.k, out.bin, out.rho, out.vec_ptr = hkl, kabs, bins, torch.view_as_complex(rho), vec_ptr64
    return out


# ---- real-space statistics of periodic cells (csrc/cells/cell_stats.hip) -------------------------------------------------------
_PAIR_TILES_WANTED = 512   # two workgroups per CU: below that the values of the first shift component are dealt over several tiles


def _pair_tiles(sizes, boxes) -> np.ndarray:
    """the work list of egnn_cell_pair_counts (include/egnn_amd.h): {cell, first centre, first neighbour, piece, pieces} for every
    (64-centre block, 1024-atom chunk) of every cell, times ``pieces`` pieces of the 2 S_0 + 1 values of the first shift component
    (``boxes`` int [C]: S_0 per cell).  A batch that fills the device as it is (256 cells of 24 atoms: 256 blocks) is cut in two at
    the most; one 3,000-atom cell (141 blocks) in three, 423 tiles.  No tile is empty: a cell contributes its own blocks only, and
    never more pieces than it has shift values."""
    sz = np.asarray(sizes, dtype=np.int64)
    n_cb, n_jb = -(-sz // _lib.CELL_STAT_CENTRE_BLOCK), -(-sz // _lib.CELL_STAT_CHUNK)
    blocks = n_cb * n_jb
    want = -(-_PAIR_TILES_WANTED // max(int(blocks.sum()), 1))
    pieces = np.minimum(2 * np.asarray(boxes, dtype=np.int64) + 1, want)
    ci, t = block_index(blocks * pieces)
    p, b = t % pieces[ci], t // pieces[ci]
    tiles = np.stack([ci, (b // n_jb[ci]) * _lib.CELL_STAT_CENTRE_BLOCK, (b % n_jb[ci]) * _lib.CELL_STAT_CHUNK, p, pieces[ci]], 1)
    return tiles.astype(np.int32).reshape(-1, 5)


def _stat_bond_tiles(sizes) -> np.ndarray:
    """the work list of egnn_cell_bond_stats: {cell, first centre} for every block of 8 centres"""
    sz = np.asarray(sizes, dtype=np.int64)
    ci, t = block_index(-(-sz // _lib.CELL_STAT_BOND_CENTRES))
    return np.stack([ci, t * _lib.CELL_STAT_BOND_CENTRES], 1).astype(np.int32).reshape(-1, 2)


def _pair_nbins(R: float, dR: float) -> int:
    R, dR = float(R), float(dR)
    if not (dR > 0 and math.isfinite(dR) and R > 0 and math.isfinite(R)):
        raise ValueError("R and dR must be positive and finite")
    return int(math.floor(R / dR + 0.5))


def _image_boxes(cb: _CellBatch, dR: float, nbins: int) -> np.ndarray:
    """S_0 = ceil(nbins dR / w_0) per cell, for the work list only (the library takes the box from its own arithmetic and refuses
    a cell it finds too wide or singular): clipped to [0, 16]"""
    with np.errstate(divide="ignore", invalid="ignore"):
        det, (face,) = _width_parts(cb.lattice_h.numpy().reshape(-1, 3, 3), (0,))
        s = np.ceil(nbins * dR * face / det)
    return np.clip(np.nan_to_num(s, nan=0.0, posinf=_lib.CELL_STAT_MAX_IMAGES), 0, _lib.CELL_STAT_MAX_IMAGES).astype(np.int64)


def _pair_counts(cb: _CellBatch, dR: float, nbins: int, tiles: Optional[torch.Tensor] = None, method: str = "direct",
                 reach: Optional[int] = None, min_width: Optional[float] = None) -> torch.Tensor:
    """-> int64 [C, A, A, nbins]: the raw output of egnn_cell_pair_counts; ``tiles``: the work list where the caller has it on the
    device already.  ``method`` chooses per cell between that entry and egnn_cell_pair_counts_grid, which adds the cells it is given
    into the same array (the same integers either way); ``reach`` and ``min_width`` are the knobs of the grid (private)."""
    reach = _GRID_PAIR_REACH if reach is None else int(reach)
    nb = None if nbins < 1 else _grid_cells(cb, method, nbins * float(dR), reach, _GRID_PAIR_MIN_WIDTH if min_width is None else min_width)
    sizes = np.asarray(cb.sizes, dtype=np.int64)
    if tiles is None:
        direct_sizes = sizes if nb is None else np.where(nb[:, 0] > 0, 0, sizes)
        tiles = torch.from_numpy(_pair_tiles(direct_sizes, _image_boxes(cb, dR, nbins))).to(cb.dev)
    counts = torch.empty(cb.C, cb.A, cb.A, max(nbins, 1), dtype=torch.int64, device=cb.dev)
    if nb is None or len(tiles):
        _lib.check(_lib.lib().egnn_cell_pair_counts(*cb.args(A=True, types=True), float(dR), int(nbins), _ptr_or_none(tiles), len(tiles),
                                                    _lib.ptr(counts)))
    else:
        counts.zero_()
    if nb is not None:
        grid = _CellGrid(cb, nb, nbins * float(dR), reach)
        _lib.check(_lib.lib().egnn_cell_pair_counts_grid(*grid.args(cb, A=True), _lib.ptr(grid.sorted_frac), _lib.ptr(grid.sorted_type), float(dR),
                                                         int(nbins), grid.reach, _ptr_or_none(grid.tiles), grid.n_tiles, _lib.ptr(counts)))
    return counts


def _bond_stats(cb: _CellBatch, bonds: BondList, dtheta: float, max_cn: int, former: int, bridge: int, tiles: Optional[torch.Tensor] = None):
    """-> (coordination int32 [N, A], cn, angles int64, qn int32 [N], qn_hist int64, overflow int32 [C]): the raw outputs of
    egnn_cell_bond_stats; ``tiles``: the work list where the caller has it on the device already"""
    dtheta, max_cn = float(dtheta), int(max_cn)
    nth = int(np.floor(180.0 / dtheta + 0.5)) + 1 if dtheta > 0 else 1
    A, C, N, E, ncn = cb.A, cb.C, cb.N, bonds.num_bonds, max(max_cn, 0) + 1
    if tiles is None:
        tiles = torch.from_numpy(_stat_bond_tiles(cb.sizes)).to(cb.dev)
    coordination = _empty(N, A, dtype=torch.int32, device=cb.dev)
    qn = _empty(N, dtype=torch.int32, device=cb.dev)
    cn = torch.empty(C, A, A, ncn, dtype=torch.int64, device=cb.dev)
    ang = torch.empty(C, A, A * (A + 1) // 2, max(nth, 1), dtype=torch.int64, device=cb.dev)
    qn_hist = torch.empty(C, ncn, dtype=torch.int64, device=cb.dev)
    over = torch.empty(C, dtype=torch.int32, device=cb.dev)
    _lib.check(_lib.lib().egnn_cell_bond_stats(
        *cb.args(A=True, types=True), _lib.ptr(bonds.row_ptr), E, _ptr_or_none(bonds.atom), _ptr_or_none(bonds.shift_code), dtheta, max_cn,
        int(former), int(bridge), _ptr_or_none(tiles), len(tiles), _ptr_or_none(coordination), _lib.ptr(cn), _lib.ptr(ang), _ptr_or_none(qn),
        _lib.ptr(qn_hist), _lib.ptr(over)))
    return coordination, cn, ang, qn, qn_hist, over


def _raise_on_cell_overflow(over: torch.Tensor):
    bad = torch.nonzero(over > 0)
    if bad.numel():
        c = int(bad[0])
        raise RuntimeError(f"cell {c}: {int(over[c])} centre(s) with more than 64 bonds; their angles are not taken (lower the cutoff)")


def _smooth(g: torch.Tensor, sigma: float) -> torch.Tensor:
    """the filter of struct_smooth_* (csrc/eval/structure_math.h) along the last axis in fp64: reflect boundary, truncation at
    4 sigma, the taps added in ascending order"""
    nbins = g.shape[-1]
    lw = int(4.0 * sigma + 0.5)
    taps = torch.arange(-lw, lw + 1, dtype=torch.float64)
    w = torch.exp(-0.5 * taps * taps / (sigma * sigma)).tolist()
    k = torch.arange(nbins, device=g.device)
    acc, wsum = torch.zeros_like(g), 0.0
    for t, wt in zip(range(-lw, lw + 1), w):
        idx = torch.remainder(k + t, 2 * nbins)
        idx = torch.where(idx >= nbins, 2 * nbins - 1 - idx, idx)
        acc = acc + g[..., idx] * wt
        wsum = wsum + wt
    return acc / wsum


def _n_type(cb: _CellBatch) -> torch.Tensor:
    return torch.stack([torch.bincount(c.types.long(), minlength=cb.A)[:cb.A] for c in cb.cells]).to(cb.dev)


def _rdf_weights(cb: _CellBatch, weights) -> torch.Tensor:
    """float64 [A] on the device; a bad shape fails before the launch"""
    from .stats import NEUTRON_LENGTHS
    if weights is None:
        weights = NEUTRON_LENGTHS if cb.A == 2 else (1.0,) * cb.A
    wt = torch.as_tensor(weights, dtype=torch.float64).detach().cpu().reshape(-1)
    if wt.numel() != cb.A:
        raise ValueError(f"weights must hold one value per atom type ({cb.A})")
    return wt.to(cb.dev)


def _rdf_finish(cb: _CellBatch, counts: torch.Tensor, dR: float, sigma: float, wt: torch.Tensor):
    from types import SimpleNamespace
    nbins = int(counts.shape[-1])
    n_type = _n_type(cb)
    nt = n_type.to(torch.float64)
    Lh = cb.lattice_h.view(-1, 3, 3)
    volume = (Lh[:, 0] * torch.linalg.cross(Lh[:, 1], Lh[:, 2])).sum(1).abs().to(cb.dev)
    k = torch.arange(nbins, dtype=torch.float64, device=cb.dev)
    shell = (4.0 * math.pi / 3.0) * ((k + 1.0) ** 3 - k ** 3) * dR ** 3
    denom = nt[:, :, None, None] * nt[:, None, :, None] * shell
    c64 = counts.to(torch.float64)
    g = torch.where(denom > 0, volume[:, None, None, None] * c64 / denom.clamp(min=1e-300), torch.zeros_like(c64))
    n = torch.where(nt[:, :, None, None] > 0, torch.cumsum(c64, -1) / nt[:, :, None, None].clamp(min=1.0), torch.zeros_like(c64))
    if sigma > 0:
        g = _smooth(g, float(sigma))
    conc = nt / nt.sum(1, keepdim=True).clamp(min=1.0)
    cw = conc * wt
    total = (cw[:, :, None, None] * cw[:, None, :, None] * g).sum((1, 2)) / (cw.sum(1) ** 2)[:, None]
    return SimpleNamespace(r=(k + 0.5) * dR, counts=counts, g=g, n=n, total=total, n_type=n_type, volume=volume, sizes=list(cb.sizes))


def pair_counts(cells: Union[PeriodicCell, Sequence[PeriodicCell]], R: float = 10.0, dR: float = 0.01, device=None,
                method: str = "auto") -> torch.Tensor:
    """Ordered-pair counts by type over every centre AND every image of the infinite lattice: int64 [C, A, A, nbins],
    c[cell, a, b, k] = pairs (i, (j, s)), s in Z^3, (j, s) != (i, 0), with type(i) = a, type(j) = b and
    floor(|(w_j - w_i + s) L| / dR) = k in fp64 (csrc/cells/cell_stats_math.h).  An atom pairs with its own images, and
    c[a, b] == c[b, a] bitwise.  nbins = floor(R / dR + 0.5) and bin k is [k dR, (k + 1) dR): NOT the reference's open bins
    (dR + k dR, dR + (k + 1) dR) that ``stats.rdf`` and ``stats.pair_counts`` keep for clusters.  An extension: the reference counts
    about atom 0 of one cluster (evaluate_RDF.py:39-60).  Refused (``EgnnError``, naming the cell): a singular lattice, a cell that
    needs more than 16 images along an axis to reach R, A A nbins > 16384.

    ``method``: "direct" tests every atom of a cell against every centre; "grid" bins the atoms and searches the neighbouring bins
    (csrc/cells/cell_grid.hip; O(n), and ValueError naming the cell and its widths where a cell is too thin to be gridded); "auto"
    (the default) chooses per cell -- the grid for a griddable cell of at least ``_GRID_MIN_ATOMS`` atoms.  The outputs are bitwise
    the same whichever way a cell goes."""
    _check_method(method)
    cb = _CellBatch(_as_cells(cells), device)
    return _pair_counts(cb, float(dR), _pair_nbins(R, dR), method=method)


def partial_rdf(cells: Union[PeriodicCell, Sequence[PeriodicCell]], R: float = 10.0, dR: float = 0.01, sigma: float = 0.0, weights=None,
                device=None, method: str = "auto"):
    """Partial pair distributions of periodic cells, the real-space counterpart of ``structure_factor``.  -> a namespace with
    r float64 [nbins] (bin centres, the bins of ``pair_counts``, not the reference's); counts int64 [C, A, A, nbins];
    g float64 [C, A, A, nbins] = V c_ab(k) / (N_a N_b (4 pi / 3) ((k + 1)^3 - k^3) dR^3) with V = |det L| -- the TRUE density of the
    cell, not the reference's sphere n / (4/3 pi R^3) -- so g_ab -> 1 at large r; an absent type gives zeros; n float64, the running
    coordination cumsum_k c_ab / N_a; total float64 [C, nbins] = sum_ab c_a c_b w_a w_b g_ab / (sum_a c_a w_a)^2 with the
    concentrations c_a = N_a / N and ``weights`` [A] (default ``stats.NEUTRON_LENGTHS`` for A = 2, ones otherwise); n_type int64
    [C, A], volume float64 [C], sizes.  ``sigma > 0`` smooths g (and total through it) along k with the filter of ``stats.rdf``
    (reflect boundary, truncated at 4 sigma bins); counts and n stay raw.  ``method`` chooses how the pairs are counted
    (``pair_counts``)."""
    _check_method(method)
    cb = _CellBatch(_as_cells(cells), device)
    nbins, wt = _pair_nbins(R, dR), _rdf_weights(cb, weights)
    return _rdf_finish(cb, _pair_counts(cb, float(dR), nbins, method=method), float(dR), float(sigma), wt)


def _bond_statistics(cb: _CellBatch, bonds: BondList, dtheta, max_cn, former, bridge):
    from types import SimpleNamespace
    coordination, cn, ang, qn, qn_hist, over = _bond_stats(cb, bonds, dtheta, max_cn, former, bridge)
    _raise_on_cell_overflow(over)
    return SimpleNamespace(coordination=coordination, cn=cn, angles=ang, qn=qn, qn_hist=qn_hist, bonds=bonds)


def bond_statistics(cells: Union[PeriodicCell, Sequence[PeriodicCell]], cutoff: float = 2.0, dtheta: float = 1.0, max_cn: int = 16,
                    former: int = 1, bridge: int = 0, device=None, method: str = "auto"):
    """Coordination numbers, bond angles and Q^n speciation of periodic cells over the periodic bond list (``bond_list``: image
    (j, s) is bonded to i iff closer than ``cutoff`` in fp64).  -> a namespace with coordination int32 [N, A] (bonds of every atom
    by neighbour type; its row sums are the degrees of ``bonds``); cn int64 [C, A, A, max_cn + 1] and angles int64
    [C, A, A(A+1)/2, ntheta] in the layout of ``stats.bond_statistics`` (cn[c, a, b, m] = atoms of type a with m bonds to type b, the
    last bin max_cn or more; angles[c, a, p, k] = bonded pairs about centres of type a with neighbour types (b <= c),
    p = b A - b(b-1)/2 + c - b, in the bin centred on k dtheta degrees, ntheta = floor(180 / dtheta + 0.5) + 1); qn int32 [N] = for an
    atom of type ``former`` (default 1 = Si) its bonds to atoms of type ``bridge`` (default 0 = O) that are bonded to two or more
    formers, -1 for every other atom; qn_hist int64 [C, max_cn + 1], the last bin saturating; bonds, the ``BondList``.  Raises
    RuntimeError, naming the first such cell, if a centre has more than 64 bonds.  ``method`` chooses how the bond list is built
    (``bond_list``)."""
    _check_method(method)
    cb = _CellBatch(_as_cells(cells), device)
    return _bond_statistics(cb, _bond_list(cb, cutoff, method), dtheta, max_cn, former, bridge)


def structure_profile(cells: Union[PeriodicCell, Sequence[PeriodicCell]], R: float = 10.0, dR: float = 0.01, sigma: float = 0.0,
                      weights=None, cutoff: float = 2.0, dtheta: float = 1.0, max_cn: int = 16, former: int = 1, bridge: int = 0,
                      device=None, method: str = "auto"):
    """``partial_rdf`` and ``bond_statistics`` of one batch from one upload and one bond list: a namespace with every field of
    both.  ``method`` as in ``pair_counts`` and ``bond_list``, chosen per cell and per statistic."""
    from types import SimpleNamespace
    _check_method(method)
    cb = _CellBatch(_as_cells(cells), device)
    nbins, wt = _pair_nbins(R, dR), _rdf_weights(cb, weights)
    rdf = _rdf_finish(cb, _pair_counts(cb, float(dR), nbins, method=method), float(dR), float(sigma), wt)
    bs = _bond_statistics(cb, _bond_list(cb, cutoff, method), dtheta, max_cn, former, bridge)
    return SimpleNamespace(**vars(rdf), **vars(bs))


def compare_structures(cells_a, cells_b, R: float = 10.0, dR: float = 0.01, sigma: float = 0.0, weights=None, cutoff: float = 2.0,
                       dtheta: float = 1.0, max_cn: int = 16, former: int = 1, bridge: int = 0, device=None, method: str = "auto"):
    """Cell-by-cell comparison of two batches (paired by index; atom counts may differ): both sides are profiled
    (``structure_profile``) and ``stats``' curve metrics {cos, l2, mse, wasserstein} are taken of every g_ab ('g' [C, A, A]), of the
    total g(r) ('total' [C]) and of the angle, CN and Q^n histograms, each normalised to sum 1 per curve the way
    ``stats.compare_rings`` normalises ('angles' [C, A, A(A+1)/2], 'cn' [C, A, A], 'qn' [C]); cos is NaN where a curve is all zero.
    -> dict with those, 'r', 'sizes_a', 'sizes_b' and the two profiles 'a', 'b'.  ``method`` as in ``structure_profile``."""
    from .stats import _curve_metrics
    a_cells, b_cells = _as_cells(cells_a), _as_cells(cells_b)
    if len(a_cells) != len(b_cells):
        raise ValueError("the two batches must hold the same number of cells")
    kw = dict(R=R, dR=dR, sigma=sigma, weights=weights, cutoff=cutoff, dtheta=dtheta, max_cn=max_cn, former=former, bridge=bridge, device=device,
              method=_check_method(method))
    a, b = structure_profile(a_cells, **kw), structure_profile(b_cells, **kw)
    if a.g.shape != b.g.shape:
        raise ValueError("the two batches differ in the number of atom types")

    def unit(h):
        h = h.double()
        total = h.sum(-1, keepdim=True)
        return torch.where(total > 0, h / total.clamp(min=1.0), h)

    return dict(r=a.r, sizes_a=a.sizes, sizes_b=b.sizes, g=_curve_metrics(a.g, b.g), total=_curve_metrics(a.total, b.total),
                angles=_curve_metrics(unit(a.angles), unit(b.angles)), cn=_curve_metrics(unit(a.cn), unit(b.cn)),
                qn=_curve_metrics(unit(a.qn_hist), unit(b.qn_hist)), a=a, b=b)


# ---- SOAP descriptors of periodic cells (csrc/cells/cell_soap.hip) ---------------------------------------------------------------
# One launch lists the sites of, and describes, a slab of centres: the site list (two int32 per site) and the descriptor rows (and
# coefficients) of a slab stay within this many bytes, the sites estimated from the densest cell's number density with a quarter
# to spare.  The outputs do not depend on the slabs.
_SOAP_SLAB_BYTES = 256 << 20


class SiteList:
    """CSR of the sites about M listed centres of a batch of cells, over every image inside the radius: ``row_ptr`` int32 [M+1];
    ``atom`` int32 [T], the site's atom as an index into the concatenated atoms of the batch; ``shift_code`` int32 [T]
    (csrc/cells/cell_math.h) and ``shift`` int32 [T, 3], its lattice shift relative to the wrapped atoms, |s_k| <= 4, on the device;
    ``centre_cell`` / ``centre_atom`` int64 [M] (atom counted inside its cell) on the host.  Rows ascend by (atom, shift) and leave
    the centre itself out; a row has the format of a ``BondList`` row."""

    def __init__(self, row_ptr, atom, shift_code, centre_cell, centre_atom):
        self.row_ptr, self.atom, self.shift_code, self.centre_cell, self.centre_atom = row_ptr, atom, shift_code, centre_cell, centre_atom

    @property
    def shift(self) -> torch.Tensor:
        return decode_shift(self.shift_code)

    @property
    def num_sites(self) -> int:
        return int(self.atom.shape[0])


def _check_site_boxes(cb: _CellBatch, radius: float):
    """the refusals of csrc/cells/cell_soap_math.h, as ValueError naming the cell and its widths: the image box
    floor(radius / w_k) + 1 must stay within 4, the range of the shift code"""
    _check_lattice_boxes(cb.lattice_h.numpy(), radius)


def _check_lattice_boxes(lattices: np.ndarray, radius: float):
    """``_check_site_boxes`` on the lattices [C, 9] alone: no device"""
    if not (math.isfinite(radius) and radius > 0.0):
        raise ValueError("the radius must be positive and finite")
    widths, singular = _widths(lattices)
    for c, w in enumerate(widths):
        if singular[c]:
            raise ValueError(f"cell {c}: singular lattice")
        if not bool(np.all(np.floor(radius / w) + 1.0 <= _lib.CELL_SOAP_MAX_BOX)):
            raise ValueError(f"cell {c}: perpendicular widths {w[0]:.6g}, {w[1]:.6g}, {w[2]:.6g} A and one is at most radius / 4 = "
                             f"{radius / 4:.6g} A: its sites need more than {_lib.CELL_SOAP_MAX_BOX} images to a side (use a supercell)")


class _SiteSearch:
    """how the sites about centres of a batch are found at one radius, decided once per cell: "direct" by the site kernels
    (egnn_cell_sites_count / _fill: any image box up to 4, work for the listed centres only), "grid" through the linked-cell bond
    list of the whole cell at cutoff = radius (``_bond_list(.., "grid")``; ValueError for a cell that is not griddable), "auto" the
    grid for a griddable cell of at least ``_GRID_MIN_ATOMS`` atoms.  That constant was measured for bond lists at 2 A, NOT at this
    radius.  The one comparison at this radius (tools/cell_soap_time.py, profiles/cell_soap_time.json: 256 listed centres of a
    24,000-atom cell at 8.37 A, whole calls, best of 5) has the grid at 3.0 ms against 9.3 ms direct, with a spread of the grid's
    rounds (33.8 ms, the first call) above the difference and no smaller cell compared: no crossover, so no constant of its own.
    The rows are bitwise the same either way."""

    def __init__(self, cb: _CellBatch, radius: float, method: str):
        self.cb, self.radius = cb, float(radius)
        _check_method(method)
        _check_site_boxes(cb, self.radius)
        nb = _grid_cells(cb, method, self.radius, 1, _GRID_BOND_MIN_WIDTH)
        self.grid_mask = None
        if nb is not None:
            mask = nb[:, 0] > 0
            gc = np.nonzero(mask)[0]
            self.grid_mask = torch.from_numpy(mask)
            self.sub = _CellBatch([cb.cells[int(c)] for c in gc], cb.dev)
            self.bonds = _bond_list(self.sub, self.radius, "grid")
            first = torch.zeros(cb.C, dtype=torch.int64)   # the first atom of a gridded cell inside the sub-batch
            first[torch.from_numpy(gc)] = self.sub.cell_ptr_h[:-1].long()
            self.sub_first = first

    def rows(self, idx_h: torch.Tensor, cell_h: torch.Tensor):
        """-> (row_ptr int32 [m+1], atom int32 [T], shift code int32 [T]) on the device, for centres ``idx_h`` (into the batch) of cells
        ``cell_h``, in their order"""
        cb, dev, m = self.cb, self.cb.dev, int(idx_h.numel())
        lib = _lib.lib()
        gridded = torch.zeros(m, dtype=torch.bool) if self.grid_mask is None else self.grid_mask[cell_h]
        direct = torch.where(gridded, torch.full_like(idx_h, -1), idx_h).to(torch.int32).to(dev)   # -1: an empty row from the site kernels
        head = (*cb.args(), self.radius, m, _ptr_or_none(direct))
        deg = torch.zeros(max(m, 1), dtype=torch.int32, device=dev)[:m]
        any_direct = bool((~gridded).any())
        if any_direct:
            _lib.check(lib.egnn_cell_sites_count(*head, _lib.ptr(deg)))
        lens = deg.long()
        if bool(gridded.any()):
            gm = torch.nonzero(gridded).reshape(-1)
            first_full = cb.cell_ptr_h.long()[cell_h[gm]]
            sub_atom = (idx_h[gm] - first_full + self.sub_first[cell_h[gm]]).to(dev)
            offset = (first_full - self.sub_first[cell_h[gm]]).to(dev)
            rp = self.bonds.row_ptr.long()
            src0, glen = rp[sub_atom], rp[sub_atom + 1] - rp[sub_atom]
            gm = gm.to(dev)
            lens[gm] = glen
        row_ptr = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        row_ptr[1:] = torch.cumsum(lens, 0)
        T = int(row_ptr[-1])
        if T >= 2 ** 31:
            raise ValueError(f"more than 2^31 - 1 sites in one slab of {m} centres (lower the slab budget or the radius)")
        row_ptr32 = row_ptr.to(torch.int32)
        atom, code = (_empty(T, dtype=torch.int32, device=dev) for _ in range(2))
        if any_direct and T:
            _lib.check(lib.egnn_cell_sites_fill(*head, _lib.ptr(row_ptr32), T, _lib.ptr(atom), _lib.ptr(code)))
        if bool(gridded.any()) and int(glen.sum()):
            rep = torch.repeat_interleave(torch.arange(gm.numel(), device=dev), glen)
            within = torch.arange(rep.numel(), device=dev) - (torch.cumsum(glen, 0) - glen)[rep]
            src, dst = src0[rep] + within, row_ptr[gm][rep] + within
            atom[dst] = (self.bonds.atom[src].long() + offset[rep]).to(torch.int32)
            code[dst] = self.bonds.shift_code[src]
        return row_ptr32, atom, code


def neighbour_sites(cells: Union[PeriodicCell, Sequence[PeriodicCell]], radius: float, centres=None, method: str = "auto",
                    device=None) -> SiteList:
    """The sites about every requested centre over EVERY image inside ``radius``: site (j, s), s in Z^3, belongs to centre i iff
    |(w_j - w_i + s) L| < radius in fp64 and it is not (i, 0) (csrc/cells/cell_soap_math.h) -- ``bond_list`` without its limit of 27
    images, so that a cell narrower than the radius is served: the image box floor(radius / w_k) + 1 may reach 4 on an axis.  A cell
    with a perpendicular width <= radius / 4, or a singular lattice, raises ValueError naming the cell and its widths.  ``centres`` as
    in ``local_environments``: None, a type index, or an index tensor into the concatenated atoms (any order, repeats allowed; the
    rows follow it).  ``method``: "direct" (the site kernels: work for the listed centres only), "grid" (the linked-cell bond list of
    the whole cell; ValueError for a cell too thin to be gridded at ``radius``), "auto" (the grid for a griddable cell of at least
    ``_GRID_MIN_ATOMS`` atoms); the rows are bitwise the same either way."""
    cb = _CellBatch(_as_cells(cells), device)
    search = _SiteSearch(cb, float(radius), method)
    idx_h, cell_h = _centres(cb, centres)
    row_ptr, atom, code = search.rows(idx_h, cell_h)
    return SiteList(row_ptr, atom, code, cell_h, idx_h - cb.cell_ptr_h.long()[cell_h])


def _slab_sites(cb: _CellBatch, radius: float) -> int:
    """the sites about one centre inside ``radius``, estimated from the densest cell's number density with a quarter to spare:
    what the slabs of the SOAP and bond-order launches are sized by"""
    vol = np.abs(np.linalg.det(cb.lattice_h.numpy().reshape(-1, 3, 3)))
    density = float(np.max(np.asarray(cb.sizes, dtype=np.float64) / vol)) if cb.C else 0.0
    return int(math.ceil(1.25 * density * 4.0 / 3.0 * math.pi * radius ** 3)) + 1


def _row_args(search: _SiteSearch, atoms_h: torch.Tensor, cells_of: torch.Tensor):
    """the site rows of centres ``atoms_h`` as the entries over a site CSR take them -> ((n_rows, row_ptr, T, site atom, site shift, M,
    centre atom, centre row), the tensors behind the pointers): row m is centre m's"""
    m = int(atoms_h.numel())
    row_ptr, atom, code = search.rows(atoms_h, cells_of)
    who = torch.cat([atoms_h.to(torch.int32), torch.arange(m, dtype=torch.int32)]).to(search.cb.dev)   # one upload: the centres, then their rows
    return (m, _lib.ptr(row_ptr), int(atom.shape[0]), _ptr_or_none(atom), _ptr_or_none(code), m, _lib.ptr(who[:m]), _lib.ptr(who[m:])), \
        (row_ptr, atom, code, who)


class _CellSoap:
    """one batch of cells, one basis, one cut: the site search and the descriptor launches of slabs of centres"""

    def __init__(self, cells, basis, neighbour_cut, method, device):
        from .soap import SoapBasis
        self.cb = cb = _CellBatch(_as_cells(cells), device)
        if cb.A > _lib.SOAP_MAX_TYPES:
            raise ValueError(f"{cb.A} atom types (at most {_lib.SOAP_MAX_TYPES})")
        self.basis = SoapBasis() if basis is None else basis
        self.cut = self.basis.neighbour_cut if neighbour_cut is None else float(neighbour_cut)
        if not (math.isfinite(self.cut) and self.cut > 0.0):
            raise ValueError("neighbour_cut must be positive and finite")
        self.search = _SiteSearch(cb, self.cut, method)
        self.F = self.basis.features(cb.A)
        self.coeff_shape = (cb.A, self.basis.n_max, (self.basis.l_max + 1) ** 2)
        self.tables = self.basis.device_tables(cb.dev)

    def slab_centres(self, coefficients: bool, budget: int) -> int:
        """centres per launch under ``budget`` bytes: descriptor row, coefficients, and the estimated sites of one centre"""
        per = 8 * self.F + (8 * int(np.prod(self.coeff_shape)) if coefficients else 0) + 8 * _slab_sites(self.cb, self.cut)
        return max(1, int(budget) // per)

    def describe(self, idx_h, cell_h, desc, coeff):
        """the descriptors of one slab of centres into ``desc`` [m, F] (and ``coeff``)"""
        if int(idx_h.numel()) == 0:
            return
        rows, keep = _row_args(self.search, idx_h, cell_h)
        _lib.check(_lib.lib().egnn_cell_soap_descriptor(*self.cb.args(A=True, types=True), self.basis.n_max, self.basis.l_max, _lib.ptr(self.tables),
                                                        *rows, _lib.ptr(desc), _lib.ptr(coeff)))


def soap_descriptors(cells: Union[PeriodicCell, Sequence[PeriodicCell]], centres=None, basis=None, neighbour_cut=None,
                     return_coefficients: bool = False, method: str = "auto", device=None, _slab_bytes: Optional[int] = None):
    """The SOAP power spectrum of atoms of periodic cells, over the sites of every image inside the neighbour cut
    (``neighbour_sites`` at ``neighbour_cut``, default ``basis.neighbour_cut`` = r_cut + sigma sqrt(2 ln 1000); the centre itself
    included): -> float64 [M, F] in the feature order of ``soap.soap_descriptors``, with ``return_coefficients`` also float64
    [M, A, n_max, (l_max+1)^2].  The site vectors and distances stay in fp64 from the fractional coordinates; the tables, formulas
    and summation orders are those of the cluster descriptor (csrc/eval/soap_device.h), the sum running over the centre first and
    then its sites by ascending (atom, shift).  A <= 4.  ``centres`` and ``method`` as in ``neighbour_sites``.  dscribe's
    ``periodic=True`` is the behaviour restated, from its description ("SOAP").  Centres are processed in slabs of
    at most ``_SOAP_SLAB_BYTES`` of site lists and rows; the outputs do not depend on the slabs."""
    run = _CellSoap(cells, basis, neighbour_cut, method, device)
    cb = run.cb
    idx_h, cell_h = _centres(cb, centres)
    M = int(idx_h.numel())
    desc = _empty(M, run.F, dtype=torch.float64, device=cb.dev)
    coeff = _empty(M, *run.coeff_shape, dtype=torch.float64, device=cb.dev) if return_coefficients else None
    step = run.slab_centres(return_coefficients, _SOAP_SLAB_BYTES if _slab_bytes is None else _slab_bytes)
    for m0 in range(0, M, step):
        m1 = min(M, m0 + step)
        run.describe(idx_h[m0:m1], cell_h[m0:m1], desc[m0:m1], coeff[m0:m1] if coeff is not None else None)
    return (desc, coeff) if return_coefficients else desc


def average_soap(cells: Union[PeriodicCell, Sequence[PeriodicCell]], centres=None, basis=None, neighbour_cut=None, method: str = "auto",
                 device=None, _slab_bytes: Optional[int] = None):
    """The mean SOAP power spectrum of every cell over its centres -- None = every atom, or a type index: -> (float64 [C, F],
    count int64 [C]).  The rows of a cell's centres (``soap_descriptors``) are added in ascending atom order into one running fp64
    sum and divided once by their number (egnn_cell_soap_mean; no atomic: a cell gives the same bits in any batch and for any slab
    size).  A cell without a centre of the type gives a row of zeros and count 0."""
    if centres is not None and not (isinstance(centres, (int, np.integer)) and not isinstance(centres, bool)):
        raise ValueError("average_soap takes centres=None (every atom) or a type index")
    run = _CellSoap(cells, basis, neighbour_cut, method, device)
    cb = run.cb
    idx_h, cell_h = _centres(cb, centres)   # ascending atoms: the centres of a cell are contiguous
    M = int(idx_h.numel())
    count_h = torch.bincount(cell_h, minlength=cb.C)[:cb.C].to(torch.int64)
    mean = torch.zeros(cb.C, run.F, dtype=torch.float64, device=cb.dev)
    if M == 0:
        return mean, count_h.to(cb.dev)
    step = run.slab_centres(False, _SOAP_SLAB_BYTES if _slab_bytes is None else _slab_bytes)
    count = count_h.to(cb.dev)
    rows = torch.empty(min(step, M), run.F, dtype=torch.float64, device=cb.dev)
    cells_edge = torch.arange(cb.C + 1, dtype=torch.int64)
    for m0 in range(0, M, step):
        m1 = min(M, m0 + step)
        run.describe(idx_h[m0:m1], cell_h[m0:m1], rows[:m1 - m0], None)
        cell_rows = torch.searchsorted(cell_h[m0:m1].contiguous(), cells_edge).to(torch.int32).to(cb.dev)
        _lib.check(_lib.lib().egnn_cell_soap_mean(_lib.stream_ptr(), cb.C, run.F, m1 - m0, _lib.ptr(rows), _lib.ptr(cell_rows), _lib.ptr(count),
                                                  int(m0 == 0), int(m1 == M), _lib.ptr(mean)))
    return mean, count


def soap_similarity(cells_a, cells_b, centres=None, basis=None, neighbour_cut=None, method: str = "auto", device=None):
    """Cell-by-cell SOAP similarity of two batches (paired by index; atom counts may differ): -> float64 [C], ``soap.cosine`` of
    the two ``average_soap`` rows; NaN where either cell has no centre of the type.  ValueError for batches of unequal length or
    unequal numbers of atom types, as ``compare_structures``."""
    from . import soap
    a_cells, b_cells = _as_cells(cells_a), _as_cells(cells_b)
    if len(a_cells) != len(b_cells):
        raise ValueError("the two batches must hold the same number of cells")
    if max(c.num_types for c in a_cells) != max(c.num_types for c in b_cells):
        raise ValueError("the two batches differ in the number of atom types")
    kw = dict(centres=centres, basis=basis, neighbour_cut=neighbour_cut, method=method, device=device)
    (a, na), (b, nb) = average_soap(a_cells, **kw), average_soap(b_cells, **kw)
    cos = soap.cosine(a, b)
    return torch.where((na > 0) & (nb > 0), cos, torch.full_like(cos, float("nan")))


# ---- bond-orientational order (csrc/cells/cell_boo.hip; definitions in csrc/cells/cell_boo_math.h) ----------------------------------
_BOO_DIGITS = 60
_BOO_SLAB_BYTES = 256 << 20   # site lists of one slab of pass 1 or pass 2; the outputs do not depend on the slabs


def _boo_norm(l_max: int) -> np.ndarray:
    """N_lm of csrc/eval/soap_math.h, float64 [(l_max+1)^2], as ``soap.build_tables`` builds it: mpmath, rounded once"""
    import mpmath as mp
    from .soap import DIGITS
    norm = np.empty((l_max + 1) ** 2)
    with mp.workdps(int(DIGITS)):
        for l in range(l_max + 1):
            for m in range(-l, l + 1):
                v = mp.sqrt((2 * l + 1) / (4 * mp.pi) * mp.factorial(l - abs(m)) / mp.factorial(l + abs(m)))
                norm[l * l + l + m] = float(v * mp.sqrt(2) if m else v)
    return norm


def _wigner3j_lll(l: int, m1: int, m2: int, m3: int):
    """the 3j symbol (l l l; m1 m2 m3), m1 + m2 + m3 = 0, by Racah's formula in exact arithmetic -> (s, r), Fractions with
    3j = s sqrt(r): s the alternating sum with the phase (-1)^(l - l - m3), r the triangle coefficient times the six factorials"""
    from fractions import Fraction
    f = math.factorial
    r = Fraction(f(l) ** 3, f(3 * l + 1)) * f(l + m1) * f(l - m1) * f(l + m2) * f(l - m2) * f(l + m3) * f(l - m3)
    s = Fraction(0)
    for t in range(max(0, -m1, m2), min(l, l - m1, l + m2) + 1):
        s += Fraction((-1) ** t, f(t) * f(t + m1) * f(t - m2) * f(l - t) * f(l - t - m1) * f(l - t + m2))
    return (-1) ** (m3 % 2) * s, r


_BOO_TABLES = {}


def _boo_tables(l_max: int):
    """-> (norm float64 [(l_max+1)^2], g_off int32 [l_max+2], g_idx int32 [E, 3], g_val float64 [E]): N_lm and the tensors G^l of
    csrc/cells/cell_boo_math.h.  With q^c_m the coefficients in the complex harmonics (Condon-Shortley phase) and q_mu those in the
    real basis, q^c_0 = q_0, q^c_m = (-1)^m (q_m + i q_-m) / sqrt 2 and q^c_-m = (q_m - i q_-m) / sqrt 2 (m > 0), so
    w_l = sum_{m1+m2+m3=0} 3j q^c_m1 q^c_m2 q^c_m3 = sum_abc T_abc q_a q_b q_c; G_abc (a <= b <= c, as l + mu) is the sum of T over the
    orderings of (a, b, c).  The 3j symbols are exact (Racah); the square roots and the basis change are taken in mpmath at 60 digits
    and every entry is rounded once.  Even l only: for odd l the contraction of the antisymmetric symbol with a symmetric product
    vanishes identically and the table is empty.  Built once per l_max."""
    if l_max in _BOO_TABLES:
        return _BOO_TABLES[l_max]
    import mpmath as mp
    off, idx, val = [0], [], []
    with mp.workdps(_BOO_DIGITS):
        half = 1 / mp.sqrt(2)

        def real_parts(m):   # q^c_m = sum of coefficient * q_mu over these (mu, coefficient)
            if m == 0:
                return [(0, mp.mpc(1))]
            if m > 0:
                return [(m, (-1) ** m * half * mp.mpc(1)), (-m, (-1) ** m * half * mp.mpc(0, 1))]
            return [(-m, half * mp.mpc(1)), (m, -half * mp.mpc(0, 1))]

        for l in range(l_max + 1):
            entries = {}
            if l % 2 == 0:
                for m1 in range(-l, l + 1):
                    for m2 in range(max(-l, -l - m1), min(l, l - m1) + 1):
                        m3 = -m1 - m2
                        s, r = _wigner3j_lll(l, m1, m2, m3)
                        if s == 0:
                            continue
                        tj = mp.mpf(s.numerator) / s.denominator * mp.sqrt(mp.mpf(r.numerator) / r.denominator)
                        for a, ca in real_parts(m1):
                            for b, cb_ in real_parts(m2):
                                for c, cc in real_parts(m3):
                                    key = tuple(sorted((l + a, l + b, l + c)))
                                    entries[key] = entries.get(key, mp.mpc(0)) + tj * ca * cb_ * cc
            for key in sorted(entries):
                v = entries[key]
                if abs(v.imag) > mp.mpf(10) ** -40:
                    raise AssertionError(f"G^{l}{key} is not real")
                if abs(v.real) > mp.mpf(10) ** -40:
                    idx.append(key)
                    val.append(float(v.real))
            off.append(len(idx))
    out = (_boo_norm(l_max), np.asarray(off, dtype=np.int32), np.asarray(idx, dtype=np.int32).reshape(-1, 3), np.asarray(val, dtype=np.float64))
    _BOO_TABLES[l_max] = out
    return out


def _boo_select(select, A: int) -> int:
    """-> the bit mask of csrc/cells/cell_boo_math.h: bit type_i * A + type_j set where sites of type j about centres of type i are kept"""
    if select is None:
        return (1 << (A * A)) - 1
    if isinstance(select, str):
        if select != "same":
            raise ValueError('select must be None, "same", a list of (centre type, site type) pairs or a bool [A, A] array')
        return sum(1 << (a * A + a) for a in range(A))
    arr = np.asarray(select.detach().cpu() if isinstance(select, torch.Tensor) else select)
    if arr.dtype == np.bool_:
        if arr.shape != (A, A):
            raise ValueError(f"a bool select must be [{A}, {A}]")
        return sum(1 << (a * A + b) for a in range(A) for b in range(A) if arr[a, b])
    pairs = arr.reshape(-1, 2) if arr.size else np.zeros((0, 2), np.int64)
    if pairs.size and (pairs.min() < 0 or pairs.max() >= A):
        raise ValueError(f"a select pair names a type outside [0, {A})")
    return int(np.bitwise_or.reduce([1 << (int(a) * A + int(b)) for a, b in pairs], initial=0))


class BondOrder:
    """Bond-orientational order of M centres, rows in the caller's centre order, on the device: ``q``, ``w``, ``w_hat`` float64
    [M, l_max+1] (Steinhardt's q_l, w_l and w_l / (sum_m q_lm^2)^(3/2)); ``q_avg``, ``w_avg``, ``w_hat_avg`` the same from the
    Lechner-Dellago averaged q_lm (None without ``averaged``); ``n`` int32 [M], the kept sites, and ``n_solid`` int32 [M], those
    with a solid bond; ``qlm`` float64 [M, (l_max+1)^2] in the real basis (index l^2 + l + m) or None; ``centre_cell`` /
    ``centre_atom`` int64 [M] (atom counted inside its cell) on the host."""

    def __init__(self, q, w, w_hat, q_avg, w_avg, w_hat_avg, n, n_solid, qlm, centre_cell, centre_atom):
        self.q, self.w, self.w_hat, self.q_avg, self.w_avg, self.w_hat_avg = q, w, w_hat, q_avg, w_avg, w_hat_avg
        self.n, self.n_solid, self.qlm, self.centre_cell, self.centre_atom = n, n_solid, qlm, centre_cell, centre_atom


def bond_order(cells: Union[PeriodicCell, Sequence[PeriodicCell]], cutoff: float = 2.0, l_max: int = 6, centres=None, select=None,
               averaged: bool = True, l_solid: int = 6, threshold: float = 0.7, return_qlm: bool = False, method: str = "auto", device=None,
               _slab_bytes: Optional[int] = None) -> BondOrder:
    """Steinhardt's bond-orientational order of atoms of periodic cells (csrc/cells/cell_boo_math.h): the neighbours of an atom are
    its ``neighbour_sites`` at ``cutoff`` over every image, kept where ``select`` allows the pair (centre type, site type): None = all
    pairs, "same" = equal types, a list of pairs, or a bool [A, A] array; ``select=[(1, 1)]`` is the Si sublattice of silica.
    q_lm = mean of the real orthonormal Y_lm over the kept sites, q_l = sqrt(4 pi / (2l+1) sum_m q_lm^2), w_l the contraction with
    the Wigner 3j symbol (exactly 0 for odd l) and w_hat_l = w_l / (sum_m q_lm^2)^(3/2); with ``averaged`` the same from
    qbar_lm(i) = (q_lm(i) + sum over kept sites q_lm(atom)) / (1 + n_i) (Lechner and Dellago); ``n_solid`` counts the kept sites with
    q(i).q(k) / (|q(i)| |q(k)|) > ``threshold`` at ``l_solid`` <= ``l_max`` (ten Wolde and Frenkel).  l_max <= 10.  ``centres`` and
    ``method`` as in ``neighbour_sites``.  Pass 1 (q_lm) always covers every atom of the batch, since the averages and the solid
    bonds read the neighbours' rows.  All fp64, every sum in one stated order: results are bitwise reproducible, the same for a cell
    alone and in a batch, and do not depend on the slabs the site rows go through in."""
    cb = _CellBatch(_as_cells(cells), device)
    l_max, l_solid = int(l_max), int(l_solid)
    if cb.A > _lib.CELL_MAX_TYPES:
        raise ValueError(f"{cb.A} atom types (at most {_lib.CELL_MAX_TYPES})")
    if not 0 <= l_max <= _lib.SOAP_MAX_L:
        raise ValueError(f"l_max {l_max} outside [0, {_lib.SOAP_MAX_L}]")
    if not 0 <= l_solid <= l_max:
        raise ValueError(f"l_solid {l_solid} outside [0, l_max = {l_max}]")
    cutoff = float(cutoff)
    mask = _boo_select(select, cb.A)
    search = _SiteSearch(cb, cutoff, method)
    idx_h, cell_h = _centres(cb, centres)
    M, LM, L1, dev = int(idx_h.numel()), (l_max + 1) ** 2, l_max + 1, cb.dev
    norm_h, off_h, gidx_h, gval_h = _boo_tables(l_max)
    norm, off = torch.from_numpy(norm_h).to(dev), torch.from_numpy(off_h).to(dev)
    E = int(gval_h.shape[0])
    gidx = torch.from_numpy(gidx_h).to(dev) if E else None
    gval = torch.from_numpy(gval_h).to(dev) if E else None
    lib = _lib.lib()
    # centres per launch under the budget in bytes of site lists
    step = max(1, int(_BOO_SLAB_BYTES if _slab_bytes is None else _slab_bytes) // (8 * _slab_sites(cb, cutoff)))
    head = cb.args(A=True, types=True)
    all_qlm = _empty(cb.N, LM, dtype=torch.float64, device=dev)
    all_n = _empty(cb.N, dtype=torch.int32, device=dev)
    every, every_cell = _centres(cb, None)
    kept_rows = None
    for a0 in range(0, cb.N, step):   # pass 1: every atom
        a1 = min(cb.N, a0 + step)
        args, keep = _row_args(search, every[a0:a1], every_cell[a0:a1])
        _lib.check(lib.egnn_cell_boo_qlm(*head, cutoff, mask, l_max, _lib.ptr(norm), *args, _lib.ptr(all_qlm[a0:a1]), _lib.ptr(all_n[a0:a1])))
        if centres is None and a0 == 0 and a1 == cb.N:
            kept_rows = (args, keep)   # one slab of every atom: pass 2 reads the same rows
    blocks = 6 if averaged else 3
    out = _empty(M, blocks, L1, dtype=torch.float64, device=dev)
    n, n_solid = (_empty(M, dtype=torch.int32, device=dev) for _ in range(2))
    for m0 in range(0, M, step):      # pass 2: the listed centres
        m1 = min(M, m0 + step)
        args, keep = kept_rows if kept_rows is not None else _row_args(search, idx_h[m0:m1], cell_h[m0:m1])
        _lib.check(lib.egnn_cell_boo_invariants(*head, mask, l_max, _lib.ptr(all_qlm), E, _lib.host_ptr(off_h), _lib.ptr(off), _lib.ptr(gidx), _lib.ptr(gval),
                                                l_solid, float(threshold), int(bool(averaged)), *args, _lib.ptr(out[m0:m1]), _lib.ptr(n[m0:m1]),
                                                _lib.ptr(n_solid[m0:m1])))
    qlm = all_qlm[idx_h.to(dev)] if return_qlm else None
    avg = (out[:, 3], out[:, 4], out[:, 5]) if averaged else (None, None, None)
    return BondOrder(out[:, 0], out[:, 1], out[:, 2], *avg, n, n_solid, qlm, cell_h, idx_h - cb.cell_ptr_h.long()[cell_h])


def bond_order_profile(cells: Union[PeriodicCell, Sequence[PeriodicCell]], cutoff: float = 2.0, l_max: int = 6, select=None, l_solid: int = 6,
                       threshold: float = 0.7, min_solid: Optional[int] = None, bins: int = 50, method: str = "auto", device=None) -> dict:
    """Per cell and centre type, from ``bond_order`` of every atom: ``count`` int64 [C, A]; ``q_mean``, ``q_avg_mean`` and
    ``w_hat_mean`` float64 [C, A, l_max+1], each a running fp64 sum over the centres in ascending atom order divided once by the
    count (zeros where there is no centre); ``solid_fraction`` float64 [C, A], the share of centres with ``n_solid >= min_solid``
    (default: all of ``n``, i.e. every kept site a solid bond; an atom without a site counts); ``q_avg_hist`` int64
    [C, A, l_max+1, bins], histograms of qbar_l on [0, 1] (the last bin closed).  Torch ops on the arrays of ``bond_order``, not a hot
    path; a cell gives the same values alone and in a batch."""
    cell_list = _as_cells(cells)
    bo = bond_order(cell_list, cutoff=cutoff, l_max=l_max, select=select, averaged=True, l_solid=l_solid, threshold=threshold, method=method,
                    device=device)
    C, A, L1, bins = len(cell_list), max(c.num_types for c in cell_list), int(l_max) + 1, int(bins)
    if bins < 1:
        raise ValueError("bins must be positive")
    types = torch.cat([c.types for c in cell_list]).long()
    q, q_avg, w_hat = bo.q.cpu(), bo.q_avg.cpu(), bo.w_hat.cpu()
    n, n_solid = bo.n.cpu().long(), bo.n_solid.cpu().long()
    solid = n_solid >= (n if min_solid is None else int(min_solid))
    count = torch.zeros(C, A, dtype=torch.int64)
    means = {k: torch.zeros(C, A, L1, dtype=torch.float64) for k in ("q_mean", "q_avg_mean", "w_hat_mean")}
    frac = torch.zeros(C, A, dtype=torch.float64)
    hist = torch.zeros(C, A, L1, bins, dtype=torch.int64)
    for c in range(C):
        for a in range(A):
            rows = torch.nonzero((bo.centre_cell == c) & (types == a)).reshape(-1)   # ascending atoms
            count[c, a] = rows.numel()
            if rows.numel() == 0:
                continue
            for key, src in (("q_mean", q), ("q_avg_mean", q_avg), ("w_hat_mean", w_hat)):
                means[key][c, a] = torch.cumsum(src[rows], 0)[-1] / float(rows.numel())   # cumsum: the running sum, in order
            frac[c, a] = float(solid[rows].sum()) / float(rows.numel())
            b = torch.clamp((q_avg[rows] * bins).floor().long(), 0, bins - 1)          # [m, L1]
            hist[c, a] = torch.zeros(L1, bins, dtype=torch.int64).scatter_add_(1, b.T.contiguous(), torch.ones_like(b.T))
    return dict(count=count, solid_fraction=frac, q_avg_hist=hist, **means)


# ---- lattice energy of periodic cells (csrc/cells/cell_ewald.hip) ---------------------------------------------------------------
_EWALD_SLAB_BYTES = 256 << 20   # site lists of one slab of the real-space launch; the outputs do not depend on the slabs
COULOMB_CONSTANT = 14.3996454784   # e^2 / (4 pi eps_0) in eV A


class PairTable:
    """Short-range pair potential u_ab(r) = A_ab exp(-b_ab r) - C_ab / r^6 + D_ab / r^n between atom types: ``A`` (eV), ``b`` (1/A),
    ``C`` (eV A^6) and ``D`` (eV A^n; default none) are symmetric, finite [types, types] tables, ``n`` one integer in [1, 64] for
    the whole table (24 is the customary repulsive fix of BKS)."""

    def __init__(self, A, b, C, D=None, n: int = 24):
        tabs = [np.array(t, dtype=np.float64) for t in (A, b, C)]
        tabs.append(np.zeros_like(tabs[0]) if D is None else np.array(D, dtype=np.float64))
        shape = tabs[0].shape
        if len(shape) != 2 or shape[0] != shape[1] or not 1 <= shape[0] <= _lib.CELL_MAX_TYPES or any(t.shape != shape for t in tabs):
            raise ValueError(f"the pair tables A, b, C, D must share one shape [types, types], 1 <= types <= {_lib.CELL_MAX_TYPES}")
        for name, t in zip("AbCD", tabs):
            if not np.all(np.isfinite(t)):
                raise ValueError(f"pair table {name} is not finite")
            if not np.array_equal(t, t.T):
                raise ValueError(f"pair table {name} is not symmetric")
        if int(n) != n or not 1 <= int(n) <= _lib.EWALD_MAX_POWER:
            raise ValueError(f"the power n of D / r^n must be an integer in [1, {_lib.EWALD_MAX_POWER}]")
        self.A, self.b, self.C, self.D, self.n = *tabs, int(n)

    @property
    def num_types(self) -> int:
        return int(self.A.shape[0])

    def tables(self) -> np.ndarray:
        """float64 [4, types, types]: what the entries of include/egnn_amd.h take as ``pot``"""
        return np.ascontiguousarray(np.stack([self.A, self.b, self.C, self.D]))


class _Bks:
    """van Beest, Kramer and van Santen's silica potential (Phys. Rev. Lett. 64, 1955 (1990)), type order (O, Si): ``charges`` and
    the Buckingham ``potential`` (no Si-Si term, no D / r^n repulsion).  The numbers are stated from the publication, not pinned by
    execution ("Lattice energy")."""
    charges = (-1.2, 2.4)
    potential = PairTable(A=[[1388.7730, 18003.7572], [18003.7572, 0.0]], b=[[2.76000, 4.87318], [4.87318, 0.0]],
                          C=[[175.0000, 133.5381], [133.5381, 0.0]])


BKS = _Bks()


class CellEnergy:
    """Lattice energy of C cells of N atoms in all, float64 on the device: ``energy`` [C] (eV), ``energy_per_atom`` [N],
    ``forces`` [N, 3] (eV / A) or None, ``components`` [C, 5] and ``components_per_atom`` [N, 5] in the order real, reciprocal, self,
    background, short; ``n_vectors`` int64 [C] on the host (half-space vectors below ``k_max``; zeros where no charge is set);
    ``alpha`` (1 / A) and ``k_max`` (1 / A), the Ewald parameters used.  With ``stress=True`` (None otherwise):
    ``strain_derivative`` [C, 3, 3] (eV: dE / d eps_xy under L -> L (1 + eps), fractional coordinates and membership held),
    ``strain_derivative_components`` [C, 5, 3, 3] (the same component order; the self block is zeros),
    ``strain_derivative_per_atom`` [N, 3, 3], ``stress`` [C, 3, 3] = strain_derivative / V (eV / A^3, tension positive) and
    ``pressure`` [C] = -tr stress / 3; every 3 x 3 form is filled from six stored numbers, so xy and yx are the same bits."""

    def __init__(self, energy, energy_per_atom, forces, components, components_per_atom, n_vectors, alpha, k_max, strain_derivative=None,
                 strain_derivative_components=None, strain_derivative_per_atom=None, stress=None, pressure=None):
        self.energy, self.energy_per_atom, self.forces, self.components = energy, energy_per_atom, forces, components
        self.components_per_atom, self.n_vectors, self.alpha, self.k_max = components_per_atom, n_vectors, alpha, k_max
        self.strain_derivative, self.strain_derivative_components = strain_derivative, strain_derivative_components
        self.strain_derivative_per_atom, self.stress, self.pressure = strain_derivative_per_atom, stress, pressure


EV_PER_A3_IN_GPA = 160.2176634   # 1 eV / A^3 in GPa: e = 1.602176634e-19 C exactly
_VOIGT_3X3 = (0, 5, 4, 5, 1, 3, 4, 3, 2)   # the Voigt index (xx, yy, zz, yz, xz, xy) of every entry of a row-major 3 x 3 form


def _voigt_to_3x3(six: torch.Tensor) -> torch.Tensor:
    """[..., 6] -> [..., 3, 3], a gather: xy and yx are the same stored number"""
    return six[..., list(_VOIGT_3X3)].reshape(*six.shape[:-1], 3, 3)


def strained(cells: Union[PeriodicCell, Sequence[PeriodicCell]], strain):
    """New ``PeriodicCell``s with lattice L (1 + eps) = L + L eps, the same fractional coordinates, types and id: the homogeneous
    strain ``lattice_energy(..., stress=True)`` differentiates by.  ``strain`` is a finite [3, 3] form (float64).  A cell for a cell,
    a list for a sequence.  Pure Python: no device."""
    eps = torch.as_tensor(strain, dtype=torch.float64).detach().cpu()
    if tuple(eps.shape) != (3, 3) or not bool(torch.isfinite(eps).all()):
        raise ValueError("strain must be a finite [3, 3] form")
    out = [PeriodicCell(c.lattice + c.lattice @ eps, c.frac, types=c.types, id=c.id, num_types=c.num_types) for c in _as_cells(cells)]
    return out[0] if isinstance(cells, PeriodicCell) else out


def _ewald_setup(cell_list, charges, potential, r_cut, short_cut, accuracy, alpha, k_max, coulomb_constant):
    """the host-side checks of ``lattice_energy`` and its parameters -> (A, charges float64 [A], pot [4, A, A] | None, n, r_cut,
    short_cut, alpha, k_max, kappa).  No device."""
    A = max(c.num_types for c in cell_list)
    if A > _lib.CELL_MAX_TYPES:
        raise ValueError(f"{A} atom types (at most {_lib.CELL_MAX_TYPES})")
    q = np.array(charges.detach().cpu() if isinstance(charges, torch.Tensor) else charges, dtype=np.float64).reshape(-1)
    if q.shape[0] != A:
        raise ValueError(f"charges has {q.shape[0]} entries for {A} atom types (one charge per type)")
    if not np.all(np.isfinite(q)):
        raise ValueError("charges must be finite")
    if potential is not None:
        if not isinstance(potential, PairTable):
            raise ValueError("potential must be a PairTable or None")
        if potential.num_types != A:
            raise ValueError(f"the pair tables are [{potential.num_types}, {potential.num_types}] for {A} atom types")
    r_cut, accuracy, kappa = float(r_cut), float(accuracy), float(coulomb_constant)
    short_cut = r_cut if short_cut is None else float(short_cut)
    if not (math.isfinite(r_cut) and r_cut > 0.0):
        raise ValueError("r_cut must be positive and finite")
    if not (math.isfinite(short_cut) and 0.0 < short_cut <= r_cut):
        raise ValueError(f"short_cut = {short_cut} must lie in (0, r_cut = {r_cut}]: short_cut > r_cut is not served")
    if not 0.0 < accuracy < 1.0:
        raise ValueError(f"accuracy = {accuracy} must lie in (0, 1)")
    if not (math.isfinite(kappa) and kappa > 0.0):
        raise ValueError("coulomb_constant must be positive and finite")
    root = math.sqrt(-math.log(accuracy))
    alpha = root / r_cut if alpha is None else float(alpha)
    if not (math.isfinite(alpha) and alpha > 0.0):
        raise ValueError("alpha must be positive and finite")
    k_max = 2.0 * alpha * root if k_max is None else float(k_max)
    if not (math.isfinite(k_max) and k_max > 0.0):
        raise ValueError("k_max must be positive and finite")
    lattices = np.stack([c.lattice.numpy().reshape(9) for c in cell_list])
    _check_lattice_boxes(lattices, r_cut)
    for c, L in enumerate(lattices.reshape(-1, 3, 3)):
        need = int(math.floor(k_max * float(np.sqrt((L * L).sum(1)).max()) / (2 * math.pi)))
        if need > 1023:
            raise ValueError(f"cell {c}: k_max = {k_max} needs a Miller index of {need} (at most 1023; lower the accuracy demand or raise r_cut)")
    pot = None if potential is None else potential.tables()
    return A, np.ascontiguousarray(q), pot, (24 if potential is None else potential.n), r_cut, short_cut, alpha, k_max, kappa


def lattice_energy(cells: Union[PeriodicCell, Sequence[PeriodicCell]], charges, potential: Optional[PairTable] = None, r_cut: float = 10.0,
                   short_cut: Optional[float] = None, shift: bool = True, accuracy: float = 1e-8, alpha: Optional[float] = None,
                   k_max: Optional[float] = None, coulomb_constant: float = COULOMB_CONSTANT, forces: bool = True, method: str = "auto",
                   device=None, _slab_bytes: Optional[int] = None, stress: bool = False) -> CellEnergy:
    """Energy (eV) and forces (eV / A) of periodic cells of point charges with a short-range pair potential
    (csrc/cells/cell_ewald_math.h): ``charges`` one per atom type, ``potential`` a ``PairTable`` or None (Coulomb only);
    ``lattice_energy(cells, BKS.charges, BKS.potential, short_cut=5.5)`` is BKS silica (types O, Si).  The Coulomb part is an Ewald
    sum: real space over the ``neighbour_sites`` at ``r_cut`` (erfc(alpha r) / r), reciprocal space over the half-space vectors below
    ``k_max`` (those of ``structure_factor`` at ``q_max = k_max``), the self term and the neutralising background of a charged cell;
    ``alpha = sqrt(-ln accuracy) / r_cut`` and ``k_max = 2 alpha sqrt(-ln accuracy)`` unless given.  The pair potential acts on the
    sites with r < ``short_cut`` (default ``r_cut``), shifted by u_ab(short_cut) with ``shift``.  ``method`` as in
    ``neighbour_sites``.  ValueError: a wrong ``charges`` length, tables that do not fit, ``short_cut > r_cut``, ``accuracy`` outside
    (0, 1), a cell too thin for the image box of 4, an index need above 1023, coincident atoms (naming the cell).  All fp64, every
    sum in one fixed order: results are bitwise reproducible, the same for a cell alone and in a batch, and do not depend on the
    slabs the site rows go through in; ``forces=False`` skips the force sums and leaves the energy bits unchanged.  The reciprocal
    part is a direct sum, O(atoms x vectors) per cell.  ``stress=True`` adds the strain derivative of the energy, the stress tensor
    and the pressure (csrc/cells/cell_stress_math.h; the attributes of ``CellEnergy``) by one more walk of the sites and one more of
    the vectors, with or without ``forces``; every other output keeps its bits."""
    cell_list = _as_cells(cells)
    A, q_h, pot_h, n, r_cut, short_cut, alpha, k_max, kappa = _ewald_setup(cell_list, charges, potential, r_cut, short_cut, accuracy, alpha,
                                                                          k_max, coulomb_constant)
    cb = _CellBatch(cell_list, device)
    search = _SiteSearch(cb, r_cut, method)
    lib, dev, N, C = _lib.lib(), cb.dev, cb.N, cb.C
    forces, stress = bool(forces), bool(stress)
    q_ptr, pot_ptr = _lib.host_ptr(q_h), (None if pot_h is None else _lib.host_ptr(pot_h))
    ewald = (kappa, alpha, r_cut, k_max)
    real = _empty(N, 5, dtype=torch.float64, device=dev)
    flag = torch.zeros(C, dtype=torch.int32, device=dev)
    v_real = _empty(N, 12, dtype=torch.float64, device=dev) if stress else None
    every, every_cell = _centres(cb, None)
    step = max(1, int(_EWALD_SLAB_BYTES if _slab_bytes is None else _slab_bytes) // (8 * _slab_sites(cb, r_cut)))
    head = cb.args(A=True, types=True)
    for a0 in range(0, N, step):
        a1 = min(N, a0 + step)
        args, keep = _row_args(search, every[a0:a1], every_cell[a0:a1])
        _lib.check(lib.egnn_cell_ewald_real(*head, q_ptr, pot_ptr, n, int(bool(shift)), kappa, alpha, r_cut, short_cut, k_max, int(forces), *args,
                                            _lib.ptr(real[a0:a1]), _lib.ptr(flag)))
        if stress:
            _lib.check(lib.egnn_cell_ewald_virial_real(*head, q_ptr, pot_ptr, n, int(bool(shift)), kappa, alpha, r_cut, short_cut, k_max, *args,
                                                       _lib.ptr(v_real[a0:a1]), _lib.ptr(flag)))
    v_rec = None
    rec, n_vectors = None, torch.zeros(C, dtype=torch.int64)
    if bool(np.any(q_h != 0.0)):
        vecs = _SqVectors(cb, k_max, "k_max")
        n_vectors = torch.tensor(vecs.counts, dtype=torch.int64)
        hkl = _empty(vecs.K, 3, dtype=torch.int32, device=dev)
        table = _empty(vecs.K, 5, dtype=torch.float64, device=dev)
        rec = _empty(N, 4, dtype=torch.float64, device=dev)
        amp_head = cb.args(A=True, types=True, host=(_lib.ptr(vecs.plan_h), _lib.ptr(vecs.vec_ptr_h)), dev=(_lib.ptr(vecs.plan), _lib.ptr(vecs.vec_ptr)))
        _lib.check(lib.egnn_cell_ewald_amplitudes(*amp_head, q_ptr, *ewald, vecs.n_rows, _lib.ptr(vecs.row_ptr), vecs.K, _ptr_or_none(vecs.tiles),
                                                  vecs.n_tiles, _ptr_or_none(hkl), _ptr_or_none(table)))
        rec_head = cb.args(A=True, types=True, host=(_lib.ptr(vecs.vec_ptr_h),), dev=(_lib.ptr(vecs.vec_ptr),))
        _lib.check(lib.egnn_cell_ewald_recip(*rec_head, q_ptr, *ewald, int(forces), vecs.K, _ptr_or_none(hkl), _ptr_or_none(table),
                                             _ptr_or_none(rec)))
        if stress:
            v_rec = _empty(N, 6, dtype=torch.float64, device=dev)
            _lib.check(lib.egnn_cell_ewald_virial_recip(*rec_head, q_ptr, *ewald, vecs.K, _ptr_or_none(hkl), _ptr_or_none(table),
                                                        _ptr_or_none(v_rec)))
    n_type = torch.empty(C, A, dtype=torch.int32, device=dev)
    comp_atom = _empty(N, 5, dtype=torch.float64, device=dev)
    e_atom = _empty(N, dtype=torch.float64, device=dev)
    force = _empty(N, 3, dtype=torch.float64, device=dev) if forces else None
    comp = torch.empty(C, 5, dtype=torch.float64, device=dev)
    energy = torch.empty(C, dtype=torch.float64, device=dev)
    _lib.check(lib.egnn_cell_ewald_finish(*cb.args(A=True, frac=False, types=True), q_ptr, *ewald, _ptr_or_none(real), _ptr_or_none(rec),
                                          _lib.ptr(n_type), _ptr_or_none(comp_atom), _ptr_or_none(e_atom), _lib.ptr(force), _lib.ptr(comp),
                                          _lib.ptr(energy)))
    extra = {}
    if stress:
        d_comp_atom = _empty(N, 5, 6, dtype=torch.float64, device=dev)
        d_atom = _empty(N, 6, dtype=torch.float64, device=dev)
        d_comp = torch.empty(C, 5, 6, dtype=torch.float64, device=dev)
        d_cell, sigma = torch.empty(C, 6, dtype=torch.float64, device=dev), torch.empty(C, 6, dtype=torch.float64, device=dev)
        pressure = torch.empty(C, dtype=torch.float64, device=dev)
        _lib.check(lib.egnn_cell_ewald_virial_finish(*cb.args(A=True, frac=False, types=True), q_ptr, *ewald, _ptr_or_none(v_real),
                                                     _ptr_or_none(v_rec), _lib.ptr(n_type), _ptr_or_none(d_comp_atom), _ptr_or_none(d_atom),
                                                     _lib.ptr(d_comp), _lib.ptr(d_cell), _lib.ptr(sigma), _lib.ptr(pressure)))
        extra = dict(strain_derivative=_voigt_to_3x3(d_cell), strain_derivative_components=_voigt_to_3x3(d_comp),
                     strain_derivative_per_atom=_voigt_to_3x3(d_atom), stress=_voigt_to_3x3(sigma), pressure=pressure)
    bad = torch.nonzero(flag.cpu()).reshape(-1).tolist()
    if bad:
        raise ValueError(f"cell {bad[0]}: coincident atoms (a site at distance 0 from its centre); the energy is not defined" +
                         (f" (also cells {bad[1:]})" if len(bad) > 1 else ""))
    return CellEnergy(energy, e_atom, force, comp, comp_atom, n_vectors, alpha, k_max, **extra)


# ---- relaxation of periodic cells (csrc/cells/cell_relax.hip) -------------------------------------------------------------------
_RELAX_LIST_BYTES = 1 << 30   # the held site lists of one call (atom and shift code, 8 bytes a site), all cells together


class FireParameters:
    """The parameters of FIRE (Bitzek, Koskinen, Gaehler, Moseler and Gumbsch, Phys. Rev. Lett. 97, 170201 (2006)) as commonly used,
    unit mass 1: first time step ``dt`` and its bound ``dt_max``, ``n_min`` downhill steps before the step grows by ``f_inc``, the
    cut ``f_dec`` after an uphill step, the mixing ``a_start`` and its decay ``f_a``, and ``max_step`` (A), the largest move of one
    atom in one step.  The numbers are stated from the publication, not pinned by execution ("Relaxation")."""

    def __init__(self, dt: float = 0.1, dt_max: float = 1.0, n_min: int = 5, f_inc: float = 1.1, f_dec: float = 0.5, a_start: float = 0.1,
                 f_a: float = 0.99, max_step: float = 0.2):
        self.dt, self.dt_max, self.n_min, self.f_inc = float(dt), float(dt_max), int(n_min), float(f_inc)
        self.f_dec, self.a_start, self.f_a, self.max_step = float(f_dec), float(a_start), float(f_a), float(max_step)
        pos = lambda v: math.isfinite(v) and v > 0.0
        if not (pos(self.dt) and pos(self.dt_max) and self.dt <= self.dt_max):
            raise ValueError("FIRE needs 0 < dt <= dt_max")
        if n_min != self.n_min or self.n_min < 0:
            raise ValueError("FIRE needs an integer n_min >= 0")
        if not (pos(self.f_inc) and self.f_inc >= 1.0 and 0.0 < self.f_dec < 1.0 and 0.0 < self.a_start <= 1.0 and 0.0 < self.f_a <= 1.0):
            raise ValueError("FIRE needs f_inc >= 1, 0 < f_dec < 1, 0 < a_start <= 1 and 0 < f_a <= 1")
        if not pos(self.max_step):
            raise ValueError("max_step must be positive and finite")

    def step_args(self):
        """(dt_max, n_min, f_inc, f_dec, a_start, f_a, max_step): what the step entries of include/egnn_amd.h take"""
        return (self.dt_max, self.n_min, self.f_inc, self.f_dec, self.a_start, self.f_a, self.max_step)


class Relaxation:
    """What ``relax`` returns for C cells of N atoms in all, float64 on the device unless noted: ``cells`` (new ``PeriodicCell``s at the
    final coordinates, on the host), ``frac`` [N, 3] (unwrapped since a cell's last list build), ``energy`` and ``initial_energy`` [C]
    (eV), ``forces`` [N, 3] at the final coordinates, ``max_force`` [C], ``steps`` int32 [C] (the moves made), ``converged`` bool [C],
    ``displacement`` [N, 3] (A: the net move of every atom, never folded into the cell), ``rmsd`` [C] from it, ``n_rebuilds`` int32
    [C]; with ``trace=True`` ``energy_trace`` and ``max_force_trace`` [max_steps + 1, C], entry k the values before move k and NaN
    beyond a cell's last evaluation (None otherwise).  Of the final evaluation, as in ``CellEnergy`` (what the accuracy tests
    compare): ``energy_per_atom`` [N], ``components`` [C, 5], ``components_per_atom`` [N, 5].  ``iterations`` (int): the
    evaluate-and-step iterations launched, a multiple of ``check_every`` (what tools/cell_relax_time.py divides by)."""

    def __init__(self, **kw):
        self.energy_trace = self.max_force_trace = None
        self.__dict__.update(kw)


def _relax_list_need(cell_list, radius: float) -> int:
    """the bytes of the held lists of a call, estimated from every cell's number density: no device"""
    need = 0.0
    for c in cell_list:
        vol = abs(float(np.linalg.det(c.lattice.numpy())))
        need += 8.0 * c.num_atoms * (c.num_atoms / vol) * 4.0 / 3.0 * math.pi * radius ** 3
    return int(need)


def _relax_check(cell_list, r_cut, f_max, max_steps, skin, fire, check_every, method):
    """the refusals of ``relax`` beyond those of ``_ewald_setup`` -> (f_max, max_steps, skin, fire, check_every).  No device."""
    f_max, skin = float(f_max), float(skin)
    if not (math.isfinite(f_max) and f_max > 0.0):
        raise ValueError(f"f_max = {f_max} must be positive and finite")
    if int(max_steps) != max_steps or int(max_steps) < 0:
        raise ValueError(f"max_steps = {max_steps} must be an integer >= 0")
    if not (math.isfinite(skin) and skin > 0.0):
        raise ValueError(f"skin = {skin} must be positive and finite")
    fire = FireParameters() if fire is None else fire
    if not isinstance(fire, FireParameters):
        raise ValueError("fire must be a FireParameters or None")
    if fire.max_step > skin / 2:
        raise ValueError(f"max_step = {fire.max_step} exceeds skin / 2 = {skin / 2} (skin = {skin}): one move could outrun the held lists")
    if int(check_every) != check_every or int(check_every) < 1:
        raise ValueError("check_every must be an integer >= 1")
    _check_method(method)
    _check_lattice_boxes(np.stack([c.lattice.numpy().reshape(9) for c in cell_list]), r_cut + skin)   # the held lists reach r_cut + skin
    need = _relax_list_need(cell_list, r_cut + skin)
    if need > _RELAX_LIST_BYTES:
        raise ValueError(f"the held site lists need about {need} bytes at radius r_cut + skin = {r_cut + skin} (at most _RELAX_LIST_BYTES = "
                         f"{_RELAX_LIST_BYTES}; fewer cells per call, or a smaller r_cut or skin)")
    return f_max, int(max_steps), skin, fire, int(check_every)


def _wrap(frac: torch.Tensor) -> torch.Tensor:
    """cell_wrap of csrc/cells/cell_math.h on a tensor: w = f - floor(f), 0 where that rounds to 1"""
    w = frac - torch.floor(frac)
    return torch.where(w < 1.0, w, torch.zeros_like(w))


def relax(cells: Union[PeriodicCell, Sequence[PeriodicCell]], charges, potential: Optional[PairTable] = None, r_cut: float = 10.0,
          short_cut: Optional[float] = None, shift: bool = True, accuracy: float = 1e-8, alpha: Optional[float] = None,
          k_max: Optional[float] = None, coulomb_constant: float = COULOMB_CONSTANT, f_max: float = 1e-3, max_steps: int = 1000,
          skin: float = 1.0, fire: Optional[FireParameters] = None, check_every: int = 16, trace: bool = False, method: str = "auto",
          device=None) -> Relaxation:
    """Relaxes the atoms of periodic cells in their fixed lattices down the energy of ``lattice_energy`` (the same model arguments,
    the same refusals) by FIRE, on the device: every cell of the batch on its own, until its largest force is below ``f_max`` (eV / A)
    or it has made ``max_steps`` moves (csrc/cells/cell_relax_math.h).  The real-space sites come from lists searched at ``r_cut +
    skin`` and held: a cell whose next move would bring an atom further than ``skin / 2`` from where it stood when its list was
    built does not move until the list has been rebuilt, so no evaluation misses a site; a cell whose list has just been built
    always moves.  ``method`` as in ``neighbour_sites``: the same rows either way.  The loop launches ``check_every`` iterations
    (evaluate, step) without a synchronisation, reads two flag arrays back, rebuilds where asked (no coordinate goes through the
    host; every row is searched again, and a cell that did not ask gets its rows back bit for bit) and stops when every cell is
    done.  All fp64, every sum in one fixed order: two runs agree bitwise, and a cell's trajectory does not depend on the batch it
    is in or on ``check_every``.  ValueError beyond those of ``lattice_energy``: ``f_max <= 0``, ``max_steps < 0``, ``skin <= 0``,
    ``fire.max_step > skin / 2``, a cell too thin for the image box of 4 at ``r_cut + skin``, held lists above
    ``_RELAX_LIST_BYTES``, coincident atoms at an evaluation (naming the cell and the step), forces that are not finite.
    RuntimeError: a cell froze twice without moving in between (a guard; the freeze rule excludes it).  The cell itself is not
    relaxed, finished cells stay in the launches, and the reciprocal part is the direct sum of ``lattice_energy``."""
    cell_list = _as_cells(cells)
    A, q_h, pot_h, n, r_cut, short_cut, alpha, k_max, kappa = _ewald_setup(cell_list, charges, potential, r_cut, short_cut, accuracy, alpha,
                                                                          k_max, coulomb_constant)
    f_max, max_steps, skin, fire, check_every = _relax_check(cell_list, r_cut, f_max, max_steps, skin, fire, check_every, method)
    cb = _CellBatch(cell_list, device)      # cb.frac: the REFERENCE coordinates the lists are searched on
    lib, dev, N, C = _lib.lib(), cb.dev, cb.N, cb.C
    cb.frac.copy_(_wrap(cb.frac))
    u = cb.frac.clone()                      # the unwrapped coordinates the evaluations read
    search = _SiteSearch(cb, r_cut + skin, method)
    every, every_cell = _centres(cb, None)
    gridded = None                           # the atoms of the cells whose rows come from the linked-cell bond list, as the sub-batch holds them
    if search.grid_mask is not None:
        gridded = torch.cat([torch.arange(cb.cell_ptr_h[c], cb.cell_ptr_h[c + 1]) for c in torch.nonzero(search.grid_mask).reshape(-1).tolist()]).to(dev)
    f64 = dict(dtype=torch.float64, device=dev)
    velocity, since, moved = (torch.zeros(max(N, 1), 3, **f64)[:N] for _ in range(3))
    scalars = torch.zeros(C, _lib.RELAX_SCALARS, **f64)
    scalars[:, 0], scalars[:, 1] = fire.dt, fire.a_start
    counters = torch.zeros(C, _lib.RELAX_COUNTERS, dtype=torch.int32, device=dev)
    flags = torch.zeros(2, C, dtype=torch.int32, device=dev)     # done, rebuild: one download
    n_rebuilds = torch.zeros(C, dtype=torch.int32, device=dev)
    coincident = torch.zeros(C, dtype=torch.int32, device=dev)
    traces = torch.full((2, max_steps + 1, C), float("nan"), **f64) if trace else None
    real, rec = _empty(N, 5, **f64), None
    comp_atom, e_atom, force = _empty(N, 5, **f64), _empty(N, **f64), _empty(N, 3, **f64)
    n_type = torch.empty(C, A, dtype=torch.int32, device=dev)
    comp, energy = torch.empty(C, 5, **f64), torch.empty(C, **f64)
    q_ptr, pot_ptr = _lib.host_ptr(q_h), (None if pot_h is None else _lib.host_ptr(pot_h))
    ewald = (kappa, alpha, r_cut, k_max)
    hp, dp, up = cb._host_ptrs, cb._dev_ptrs, _ptr_or_none(u, N)
    head = (_lib.stream_ptr(), C, N, A, *hp, dp[0], dp[1], up, dp[3])     # cb.args(A=True, types=True) on u
    calls = []                                                              # the launches of one evaluation after the real part
    if bool(np.any(q_h != 0.0)):
        vecs = _SqVectors(cb, k_max, "k_max")                               # the vectors of a fixed cell: counted once
        hkl, table = _empty(vecs.K, 3, dtype=torch.int32, device=dev), _empty(vecs.K, 5, **f64)
        rec = _empty(N, 4, **f64)
        calls.append((lib.egnn_cell_ewald_amplitudes,
                      (*head[:6], _lib.ptr(vecs.plan_h), _lib.ptr(vecs.vec_ptr_h), dp[0], dp[1], _lib.ptr(vecs.plan), _lib.ptr(vecs.vec_ptr), up,
                       dp[3], q_ptr, *ewald, vecs.n_rows, _lib.ptr(vecs.row_ptr), vecs.K, _ptr_or_none(vecs.tiles), vecs.n_tiles,
                       _ptr_or_none(hkl), _ptr_or_none(table))))
        calls.append((lib.egnn_cell_ewald_recip,
                      (*head[:6], _lib.ptr(vecs.vec_ptr_h), dp[0], dp[1], _lib.ptr(vecs.vec_ptr), up, dp[3], q_ptr, *ewald, 1, vecs.K,
                       _ptr_or_none(hkl), _ptr_or_none(table), _ptr_or_none(rec))))
    calls.append((lib.egnn_cell_ewald_finish,
                  (*head[:6], dp[0], dp[1], dp[3], q_ptr, *ewald, _ptr_or_none(real), _ptr_or_none(rec), _lib.ptr(n_type),
                   _ptr_or_none(comp_atom), _ptr_or_none(e_atom), _ptr_or_none(force), _lib.ptr(comp), _lib.ptr(energy))))
    calls.append((lib.egnn_cell_relax_step,
                  (_lib.stream_ptr(), C, N, *hp, dp[0], dp[1], _ptr_or_none(force), _lib.ptr(energy), _lib.ptr(coincident), *fire.step_args(),
                   f_max, max_steps, skin, up, _ptr_or_none(velocity), _ptr_or_none(since), _ptr_or_none(moved), _lib.ptr(scalars),
                   _lib.ptr(counters), _lib.ptr(flags[0]), _lib.ptr(flags[1]), _lib.ptr(traces[0]) if trace else None,
                   _lib.ptr(traces[1]) if trace else None)))
    cell_ptr_l = cb.cell_ptr_h.tolist()

    def held_rows(again=True):
        if again and gridded is not None:     # the grid's own copy of the references, then its bond list again: all on the device
            search.sub.frac.copy_(cb.frac[gridded])
            search.bonds = _bond_list(search.sub, search.radius, "grid")
        args, keep = _row_args(search, every, every_cell)
        if 8 * int(keep[1].shape[0]) > _RELAX_LIST_BYTES:
            raise ValueError(f"the held site lists need {8 * int(keep[1].shape[0])} bytes at radius r_cut + skin = {r_cut + skin} (at most "
                             f"_RELAX_LIST_BYTES = {_RELAX_LIST_BYTES}; fewer cells per call, or a smaller r_cut or skin)")
        return (lib.egnn_cell_relax_real, (*head, q_ptr, pot_ptr, n, int(bool(shift)), kappa, alpha, r_cut, short_cut, k_max, skin, *args,
                                           _ptr_or_none(real), _lib.ptr(coincident))), keep

    real_call, keep = held_rows(again=False)     # the search was built on these coordinates (the grid wraps on read)
    iterations = 0
    while N:
        iterations += check_every
        for _ in range(check_every):
            _lib.check(real_call[0](*real_call[1]))
            for fn, a in calls:
                _lib.check(fn(*a))
        done_h, ask_h = flags.cpu().bool()
        if bool(done_h.all()):
            break
        ask = torch.nonzero(ask_h & ~done_h).reshape(-1)
        if ask.numel():
            atoms = torch.cat([torch.arange(cell_ptr_l[c], cell_ptr_l[c + 1]) for c in ask.tolist()]).to(dev)   # indices, not coordinates
            ask = ask.to(dev)
            w = _wrap(u[atoms])
            u[atoms] = w
            cb.frac[atoms] = w
            since[atoms] = 0.0
            flags[1, ask] = 0
            n_rebuilds[ask] += 1
            real_call, keep = held_rows()        # every row again, on the references: a cell that did not ask gets its rows back
    status_h, steps_h = counters[:, 2].cpu(), counters[:, 1].cpu()
    for code, what in ((_lib.RELAX_COINCIDENT, "coincident atoms (a site at distance 0 from its centre); the energy is not defined"),
                       (_lib.RELAX_NOT_FINITE, "the forces are not finite")):
        bad = torch.nonzero(status_h == code).reshape(-1).tolist()
        if bad:
            raise ValueError(f"cell {bad[0]}, step {int(steps_h[bad[0]])}: {what}" + (f" (also cells {bad[1:]})" if len(bad) > 1 else ""))
    stuck = torch.nonzero(status_h == _lib.RELAX_STUCK).reshape(-1).tolist()
    if stuck:
        raise RuntimeError(f"cell {stuck[0]}, step {int(steps_h[stuck[0]])}: froze twice without moving in between (skin = {skin}, max_step = "
                           f"{fire.max_step})")
    frac_h, moved_h = u.cpu(), moved.cpu()
    out = [PeriodicCell(c.lattice, frac_h[cell_ptr_l[k]:cell_ptr_l[k + 1]], types=c.types, id=c.id, num_types=c.num_types)
           for k, c in enumerate(cell_list)]
    d2 = (moved_h * moved_h).sum(1).numpy()
    rmsd = np.array([math.sqrt(float(np.mean(d2[cell_ptr_l[k]:cell_ptr_l[k + 1]]))) if cell_ptr_l[k + 1] > cell_ptr_l[k] else 0.0
                     for k in range(C)])
    return Relaxation(cells=out, frac=u, energy=scalars[:, 2].clone(), initial_energy=scalars[:, 3].clone(), forces=force,
                      max_force=scalars[:, 4].clone(), steps=counters[:, 1].clone(), converged=(counters[:, 2] == _lib.RELAX_CONVERGED),
                      displacement=moved, rmsd=torch.from_numpy(rmsd).to(dev), n_rebuilds=n_rebuilds, energy_per_atom=e_atom,
                      components=comp, components_per_atom=comp_atom, iterations=iterations,
                      energy_trace=traces[0] if trace else None, max_force_trace=traces[1] if trace else None)

"""The linked-cell kernels of periodic cells on the device (csrc/cells/cell_grid.hip through diffusion_model_amd.cells) against the
direct kernels (cell_env.hip, cell_stats.hip), which tests/test_gpu_cells.py and tests/test_gpu_cell_stats.py pin to their host
statements, and against the host statement egnn_cell_grid_host, which tests/test_cell_grid_host.py pins to numpy without a GPU.
Every output is an integer (or a coordinate copied, not computed): every comparison in this file is exact.

  * binning: bins, bin starts, sorted order and sorted coordinates equal the host statement bitwise, in a batch that holds a cell
    that is not gridded;
  * bond list, method="grid" against method="direct": nb = 3 (every neighbour bin wraps, every shift is used), coordinates outside
    [0, 1), 18 tiles, and the two dense cells on either side of the 128 keys the fill kernel stages per row (80 and 157-170 bonds per
    atom); coarser grids (min_width) and a reach of 2 (125 offsets: two passes of the 64 lanes over the offsets);
  * a 24,000-atom cell: the only shape above one chunk of everything;
  * pair counts, grid against direct, at reach 1, 2 and 3, where nb = 2 m + 1 exactly and on the 1,100-atom cell;
  * a mixed batch under method="auto": both kinds of cell in one call, each cell the same bits alone, two runs the same bits;
  * downstream: local_environments, ring_statistics, bond_statistics and structure_profile give the same tensors either way.
"""
import functools

import numpy as np
import pytest
import torch

import diffusion_model_amd as dma
from diffusion_model_amd import _lib, cells as DC
from tests import _cell_grid_util as GU
from tests import _cell_stats_util as SU
from tests import _cells_util as CU

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _periodic(c):
    return dma.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=c["A"], id=c["name"])


@functools.lru_cache(maxsize=None)
def _cell(name):
    if name == "r1100":
        return CU.random_cell(1100, 13, check=False)
    if name == "dense11":
        return GU.dense11()
    if name == "x10":
        return GU.displaced_cristobalite(10)
    return GU.cells()[name]


def _np(bl):
    return tuple(t.cpu().numpy() for t in (bl.row_ptr, bl.atom, bl.shift_code))


@functools.lru_cache(maxsize=None)
def _direct_bonds(names):
    """the reference, computed once per batch and left unchanged"""
    return _np(DC.bond_list([_periodic(_cell(n)) for n in names], device=DEV, method="direct"))


@functools.lru_cache(maxsize=None)
def _direct_pairs(names, R, dR):
    return DC.pair_counts([_periodic(_cell(n)) for n in names], R=R, dR=dR, device=DEV, method="direct").cpu().numpy()


def _assert_bonds(names, **kw):
    want = _direct_bonds(tuple(names))
    cb = DC._CellBatch([_periodic(_cell(n)) for n in names], DEV)
    got = _np(DC._bond_list(cb, 2.0, "grid", **kw))
    for g, w, what in zip(got, want, ("row_ptr", "atom", "shift_code")):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (names, kw, what)
    return got


def _grid_pairs(names, R, dR, method="grid", **kw):
    cb = DC._CellBatch([_periodic(_cell(n)) for n in names], DEV)
    return DC._pair_counts(cb, dR, SU.nbins_of(R, dR), method=method, **kw).cpu().numpy()


def _nb(names, radius, reach=1, min_width=0.0):
    rc, nb = GU.dims(_lib.lib(), [_cell(n) for n in names], radius, reach, min_width)
    assert rc == 0
    return nb.tolist()


# ---- binning ---------------------------------------------------------------------------------------------------------------------------
def test_binning_equals_the_host_statement(monkeypatch):
    monkeypatch.setattr(DC, "_GRID_MIN_ATOMS", 0)
    names = ("chain", "r65", "cristobalite", "r160")
    cells = [_cell(n) for n in names]
    cb = DC._CellBatch([_periodic(c) for c in cells], DEV)
    nb = DC._grid_cells(cb, "auto", 2.0, 1, 0.0)
    assert nb.tolist() == [[0, 0, 0], [5, 5, 5], [3, 3, 3], [7, 8, 7]]
    grid = DC._CellGrid(cb, nb, 2.0, 1)
    rc, want = GU.host(_lib.lib(), cells, 2.0)
    assert rc == 0 and grid.n_bins == int(want["n_bins"][0]) == 125 + 27 + 392
    assert np.array_equal(grid.atom_bin.cpu().numpy(), want["atom_bin"])
    assert np.array_equal(grid.bin_start.cpu().numpy(), want["bin_start"])
    order = grid.sorted_atom.cpu().numpy()
    assert np.array_equal(order, want["sorted_atom"]) and order[:2].tolist() == [-1, -1]
    got_frac = grid.sorted_frac.cpu().numpy()
    assert got_frac.dtype == np.float64 and np.array_equal(got_frac.view(np.int64), want["sorted_frac"].view(np.int64))      # bitwise
    types = np.concatenate([c["types"] for c in cells])
    assert np.array_equal(grid.sorted_type.cpu().numpy()[2:], types[order[2:]])
    assert grid.tiles_h.tolist() == [[1, 0], [1, 64], [2, 0], [3, 0], [3, 64], [3, 128]]


# ---- bond list -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cristobalite", "triclinic", "r65", "r160", "r1100", "dense9", "dense11"])
def test_bond_list_grid_equals_direct(name):
    row_ptr, atom, code = _assert_bonds((name,))
    deg = np.diff(row_ptr)
    if name == "dense9":          # one staged piece per row ...
        assert np.all(deg == 80) and deg.max() < _lib.CELL_GRID_ROW_KEYS and _nb((name,), 2.0) == [[3, 3, 3]]
    if name == "dense11":         # ... and two
        assert deg.min() == 157 and deg.max() == 170 and deg.min() > _lib.CELL_GRID_ROW_KEYS
    if name == "r1100":
        assert len(deg) == 1100 and all(13 <= v <= 15 for v in _nb((name,), 2.0)[0])
    if name == "r65":
        assert _cell(name)["frac"].min() < 0.0 and _cell(name)["frac"].max() > 1.0


# cells that stay griddable at bins of min_width A (the others hold fewer than three such bins on an axis and are refused)
COARSE = {3.0: ("r65", "r160", "r1100"), 5.0: ("r1100",)}


@pytest.mark.parametrize("min_width", [3.0, 5.0])
def test_bond_list_on_coarser_grids(min_width):
    for name in ("cristobalite", "triclinic", "r65", "r160", "r1100", "dense9", "dense11"):
        if name in COARSE[min_width]:
            assert max(_nb((name,), 2.0, min_width=min_width)[0]) < min(_nb((name,), 2.0)[0])          # coarser on every axis
            _assert_bonds((name,), min_width=min_width)
        else:
            assert _nb((name,), 2.0, min_width=min_width) == [[0, 0, 0]]
            with pytest.raises(ValueError, match="cell 0: perpendicular widths"):
                _assert_bonds((name,), min_width=min_width)


def test_bond_list_with_a_reach_of_two():
    assert _nb(("r160",), 2.0, reach=2) == [[14, 16, 14]]
    _assert_bonds(("r160", "cristobalite"), reach=2)
    _assert_bonds(("r1100",), reach=2, min_width=1.5)


def test_a_24000_atom_cell():
    cell = _cell("x10")
    assert len(cell["frac"]) == 24000 and _nb(("x10",), 2.0) == [[35, 35, 35]]
    row_ptr, _, _ = _assert_bonds(("x10",))
    deg = np.diff(row_ptr)
    assert np.array_equal(deg[cell["types"] == 1], np.full(8000, 4)) and np.array_equal(deg[cell["types"] == 0], np.full(16000, 2))
    want = _direct_pairs(("x10",), 10.0, 0.05)
    got = _grid_pairs(("x10",), 10.0, 0.05)
    assert got.dtype == np.int64 and np.array_equal(got, want) and want.sum() > 24000 * 250
    assert np.array_equal(got, got.transpose(0, 2, 1, 3))


# ---- pair counts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R, reach", [(2.3, 1), (2.7, 2), (2.9, 3)])
def test_pair_counts_where_the_walk_covers_every_bin_once(R, reach):
    names = ("cristobalite", "triclinic")
    nbins = SU.nbins_of(R, 0.1)
    assert _nb(names, nbins * 0.1, reach=reach) == [[2 * reach + 1] * 3] * 2
    got = _grid_pairs(names, R, 0.1, reach=reach)
    assert got.dtype == np.int64 and np.array_equal(got, _direct_pairs(names, R, 0.1)) and got.sum() > 0
    assert np.array_equal(got, got.transpose(0, 2, 1, 3))                      # c[a, b] == c[b, a] on the grid path too


@pytest.mark.parametrize("reach, nb", [(2, [5, 6, 5]), (3, [8, 9, 8])])
def test_pair_counts_on_the_1100_atom_cell(reach, nb):
    assert _nb(("r1100",), 200 * 0.05, reach=reach) == [nb]
    got = _grid_pairs(("r1100",), 10.0, 0.05, reach=reach)
    assert np.array_equal(got, _direct_pairs(("r1100",), 10.0, 0.05)) and np.array_equal(got, got.transpose(0, 2, 1, 3))


def test_pair_counts_refuse_a_cell_too_thin_for_the_reach():
    assert _nb(("r1100",), 200 * 0.05, reach=1) == [[0, 0, 0]]                # widths 26.8 - 30.7 A: two bins of 10 A
    with pytest.raises(ValueError, match="cell 0: perpendicular widths 28.1"):
        _grid_pairs(("r1100",), 10.0, 0.05, reach=1)
    with pytest.raises(ValueError, match="method must be one of"):
        DC.pair_counts([_periodic(_cell("r65"))], device=DEV, method="cells")


# ---- mixed batches ---------------------------------------------------------------------------------------------------------------------
def test_mixed_batch_under_auto(monkeypatch):
    names = ("chain", "cristobalite", "r160", "one")
    cells = [_periodic(_cell(n)) for n in names]
    R, dR = 2.3, 0.05          # 7.16 A hold 2 m + 1 bins of 2.3 / m A at any reach m; 3.2 A (chain) and 5.0 A (one) do at none: direct
    assert _nb(names, 2.0) == [[0, 0, 0], [3, 3, 3], [7, 8, 7], [0, 0, 0]]
    pair_nb = _nb(names, 46 * dR, reach=DC._GRID_PAIR_REACH, min_width=DC._GRID_PAIR_MIN_WIDTH)
    assert pair_nb[0] == pair_nb[3] == [0, 0, 0] and pair_nb[1][0] > 0 and pair_nb[2][0] > 0
    want_b, want_p = _direct_bonds(names), _direct_pairs(names, R, dR)
    assert np.array_equal(_np(DC.bond_list(cells, device=DEV))[1], want_b[1])   # the default threshold: every cell goes direct
    monkeypatch.setattr(DC, "_GRID_MIN_ATOMS", 0)
    cb = DC._CellBatch(cells, DEV)
    assert (DC._grid_cells(cb, "auto", 2.0, 1, 0.0)[:, 0] > 0).tolist() == [False, True, True, False]
    for run in range(2):                                                        # two runs give the same bits
        got_b = _np(DC.bond_list(cells, device=DEV, method="auto"))
        for g, w in zip(got_b, want_b):
            assert np.array_equal(g, w)
        assert np.array_equal(DC.pair_counts(cells, R=R, dR=dR, device=DEV, method="auto").cpu().numpy(), want_p)
    at, e = 0, 0
    for c, n in enumerate(names):                                               # each cell alone gives the bits it gives in the batch
        rp, atom, code = _np(DC.bond_list([cells[c]], device=DEV, method="auto"))
        size, E = len(rp) - 1, len(atom)
        assert np.array_equal(rp, want_b[0][at:at + size + 1] - e) and np.array_equal(atom, want_b[1][e:e + E] - at), n
        assert np.array_equal(code, want_b[2][e:e + E]), n
        assert np.array_equal(DC.pair_counts([cells[c]], R=R, dR=dR, device=DEV, method="auto").cpu().numpy()[0, :cells[c].num_types, :cells[c].num_types],
                              want_p[c, :cells[c].num_types, :cells[c].num_types]), n
        at, e = at + size, e + E


# ---- downstream ------------------------------------------------------------------------------------------------------------------------
def _downstream_cells():
    return [_periodic(_cell("triclinic")), _periodic(_cell("r160"))]


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), what


def test_local_environments_grid_equals_direct():
    a = DC.local_environments(_downstream_cells(), shells=4, device=DEV, method="grid")
    b = DC.local_environments(_downstream_cells(), shells=4, device=DEV, method="direct")
    assert a.sizes == b.sizes and len(a.sizes) == 184
    for k in ("atom", "shift", "shift_code", "pos", "x"):
        _same(getattr(a, k), getattr(b, k), k)


def test_ring_statistics_grid_equals_direct():
    a = DC.ring_statistics(_downstream_cells(), device=DEV, method="grid")
    b = DC.ring_statistics(_downstream_cells(), device=DEV, method="direct")
    for k in ("size", "count"):
        _same(torch.as_tensor(getattr(a, k)), torch.as_tensor(getattr(b, k)), k)


def test_bond_statistics_grid_equals_direct():
    a = DC.bond_statistics(_downstream_cells(), device=DEV, method="grid")
    b = DC.bond_statistics(_downstream_cells(), device=DEV, method="direct")
    for k in ("coordination", "cn", "angles", "qn", "qn_hist"):
        _same(getattr(a, k), getattr(b, k), k)
    for g, w in zip(_np(a.bonds), _np(b.bonds)):
        assert np.array_equal(g, w)


def test_structure_profile_grid_equals_direct():
    kw = dict(R=2.3, dR=0.05, sigma=1.5, device=DEV)                            # 6.96 A hold 2 m + 1 bins of 2.3 / m A at any reach m
    assert _nb(("triclinic", "r160"), 46 * 0.05, reach=DC._GRID_PAIR_REACH)[0][1] >= 2 * DC._GRID_PAIR_REACH + 1
    a = DC.structure_profile(_downstream_cells(), method="grid", **kw)
    b = DC.structure_profile(_downstream_cells(), method="direct", **kw)
    for k, v in vars(b).items():
        if torch.is_tensor(v):
            _same(getattr(a, k), v, k)
    assert a.sizes == b.sizes and int(a.counts.sum()) > 0

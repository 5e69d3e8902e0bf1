"""The linked-cell grid of periodic cells on the host (egnn_cell_grid_dims and egnn_cell_grid_host: csrc/cells/cell_grid_host.cpp over
the definitions the kernels compile, csrc/cells/cell_grid_math.h), without a GPU:

  * the grid rule nb_k = floor(m w_k / max(rho, m min_width)), its cap at 256, griddable iff nb_k >= 2 m + 1, min_width coarsening
    and never refining;
  * the bin of an atom at the two ends of [0, 1) and for coordinates outside it; the sorted order against numpy's lexsort;
  * the bond list found THROUGH THE GRID WALK equals tests/_cells_util.bonds (all pairs, 27 images) exactly, and the pair counts
    found through it equal tests/_cell_stats_util.pair_counts (all pairs, the whole image box, no cull) exactly -- every output is an
    integer, so there is no tolerance anywhere in this file;
  * a cell too thin for its radius and reach is refused, naming the cell; the device entries refuse -- before anything is launched --
    a tile that names a cell with nb = 0, a grid finer than radius and reach allow, and an n_bins that is not the grids' total;
  * the host statement runs clean under AddressSanitizer + UBSan as a stand-alone program (tests/host/cell_grid_main.cpp).
"""
import numpy as np
import pytest

from diffusion_model_amd import _lib
from tests import _cell_grid_util as GU
from tests import _cell_stats_util as SU
from tests import _cells_util as CU
from tests._host_program import build_and_run

EINVAL = -22


def _dims(cells, radius, reach=1, min_width=0.0):
    rc, nb = GU.dims(_lib.lib(), cells, radius, reach, min_width)
    assert rc == 0, _lib.lib().egnn_last_error()
    return nb.tolist()


def _host(cells, radius, **kw):
    rc, got = GU.host(_lib.lib(), cells, radius, **kw)
    assert rc == 0, _lib.lib().egnn_last_error()
    return got


# ---- the grid rule ---------------------------------------------------------------------------------------------------------------------
def test_dims_rule():
    cs = GU.cells()
    assert _dims([cs["cristobalite"]], 2.38) == [[3, 3, 3]]           # 7.16 / (2.38 (1 + 1e-6)) = 3.008
    assert _dims([cs["cristobalite"]], 2.39) == [[0, 0, 0]]           # 2.996: two bins, not griddable
    assert _dims([cs["chain"]], 2.0) == [[0, 0, 0]]                   # 3.2 A wide
    assert _dims([cs["r160"]], 2.0) == [[7, 8, 7]]                    # widths 14.79 / 16.16 / 14.09
    assert _dims([cs["chain"], cs["r160"], cs["cristobalite"]], 2.0) == [[0, 0, 0], [7, 8, 7], [3, 3, 3]]
    # the reach: m bins of thickness rho / m to each side
    assert _dims([cs["cristobalite"]], 2.7, reach=2) == [[5, 5, 5]] and _dims([cs["cristobalite"]], 2.9, reach=3) == [[7, 7, 7]]
    assert _dims([cs["cristobalite"]], 3.0, reach=2) == [[0, 0, 0]] and _dims([cs["triclinic"]], 3.0, reach=2) == [[0, 0, 0]]
    big = dict(cs["chain"], lattice=np.diag([600.0, 511.9, 512.1]))
    assert _dims([big], 2.0) == [[256, 255, 256]]                      # the cap at 256; 511.9 / 2.000002 = 255.9
    assert _dims([big], 1.0, reach=3) == [[256, 256, 256]]


def test_min_width_coarsens_and_never_refines():
    r160 = GU.cells()["r160"]
    assert _dims([r160], 2.0, min_width=1.0) == [[7, 8, 7]]            # below rho: no effect
    assert _dims([r160], 2.0, min_width=3.0) == [[4, 5, 4]]
    assert _dims([r160], 2.0, min_width=5.0) == [[0, 0, 0]]            # 2, 3, 2 bins: not griddable, whatever the radius
    assert _dims([r160], 2.0, reach=2, min_width=1.5) == [[9, 10, 9]]  # m w / max(rho, m min_width) = w / 1.5
    last = None
    for mw in (0.0, 2.0, 2.5, 3.0, 4.0):
        nb = np.array(_dims([r160], 2.0, min_width=mw))
        assert last is None or np.all(nb <= last)
        last = nb


def test_dims_argument_errors():
    L = _lib.lib()
    cs = GU.cells()
    flat = dict(cs["chain"], lattice=np.array([[3.2, 0, 0], [0, 3.2, 0], [3.2, 3.2, 0.0]]))
    for kw, word in ((dict(radius=0.0), b"radius must be positive"), (dict(radius=float("nan")), b"radius must be positive"),
                     (dict(radius=2.0, reach=0), b"reach 0"), (dict(radius=2.0, reach=4), b"reach 4"),
                     (dict(radius=2.0, min_width=-1.0), b"min_width")):
        assert GU.dims(L, [cs["r160"]], **kw)[0] == EINVAL and word in L.egnn_last_error(), (kw, L.egnn_last_error())
    assert GU.dims(L, [cs["r160"], flat], 2.0)[0] == EINVAL and b"cell 1 has a singular lattice" in L.egnn_last_error()


# ---- bins and sorted order -------------------------------------------------------------------------------------------------------------
def test_bins_at_the_ends_of_the_unit_interval():
    below_one = np.nextafter(1.0, 0.0)
    cell = dict(lattice=7.0 * np.eye(3), frac=np.array([[-1e-18, 0.5, below_one], [below_one, -1e-18, 0.0], [1.0, 2.0, -3.0]]),
                types=np.zeros(3, np.int32), A=1, name="ends", cutoff=2.0)
    got = _host([cell], 2.0)
    assert got["nb"].tolist() == [[3, 3, 3]] and int(got["n_bins"][0]) == 27
    # -1e-18 wraps to 0.0: bin 0; the largest double below 1 stays in bin nb - 1 = 2 (the clamp)
    assert got["atom_bin"].tolist() == [(0 * 3 + 1) * 3 + 2, (2 * 3 + 0) * 3 + 0, 0]
    assert got["sorted_atom"].tolist() == [2, 0, 1]
    assert np.array_equal(got["sorted_frac"], CU.wrap(cell["frac"])[[2, 0, 1]])


@pytest.mark.parametrize("name, radius, nb", [("r65", 2.0, (5, 5, 5)), ("r160", 2.0, (7, 8, 7)), ("triclinic", 2.0, (3, 3, 3))])
def test_bins_and_sorted_order(name, radius, nb):
    cell = GU.cells()[name]
    got = _host([cell], radius)
    assert tuple(got["nb"][0]) == nb
    bins = GU.restated_bins(cell, nb)
    assert np.array_equal(got["atom_bin"], bins)
    order = np.lexsort((np.arange(len(bins)), bins))
    assert np.array_equal(got["sorted_atom"], order)
    assert np.array_equal(got["bin_start"], np.concatenate([[0], np.cumsum(np.bincount(bins, minlength=int(np.prod(nb))))]))
    assert np.array_equal(got["sorted_frac"], CU.wrap(cell["frac"])[order])


def test_batch_with_a_cell_that_is_not_griddable():
    cs = GU.cells()
    batch = [cs["chain"], cs["r65"], cs["one"], cs["cristobalite"]]
    got = _host(batch, 2.0)
    assert got["nb"].tolist() == [[0, 0, 0], [5, 5, 5], [0, 0, 0], [3, 3, 3]] and int(got["n_bins"][0]) == 125 + 27
    assert got["atom_bin"][:2].tolist() == [-1, -1] and got["sorted_atom"][:2].tolist() == [-1, -1] and got["sorted_atom"][67] == -1
    alone = _host([cs["r65"]], 2.0)
    assert np.array_equal(got["sorted_atom"][2:67], alone["sorted_atom"] + 2) and np.array_equal(got["bin_start"][:126], alone["bin_start"])
    crist = _host([cs["cristobalite"]], 2.0)
    assert np.array_equal(got["sorted_atom"][68:], crist["sorted_atom"] + 68)
    assert np.array_equal(got["bin_start"][125:] - 65, crist["bin_start"])


# ---- the walk --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cristobalite", "triclinic", "r65", "r160", "dense9"])
def test_grid_walk_bonds_equal_the_restated_bond_list(name):
    cell = GU.cells()[name]
    got = _host([cell], 2.0, bonds=True)
    row_ptr, atom, code, _ = cell["bonds"]
    assert np.array_equal(got["bond_ptr"], row_ptr) and np.array_equal(got["bond_atom"], atom) and np.array_equal(got["bond_shift"], code)
    if name == "dense9":
        assert got["nb"].tolist() == [[3, 3, 3]] and len(atom) == 58320 and np.all(np.diff(row_ptr) == 80)


def test_grid_walk_bonds_in_a_batch_and_on_coarser_grids():
    cs = GU.cells()
    batch = [cs["r65"], cs["cristobalite"], cs["r160"]]
    want_ptr = np.concatenate([[0]] + [c["bonds"][0][1:] + off for c, off in zip(batch, np.cumsum([0] + [len(c["bonds"][1]) for c in batch[:-1]]))])
    want_atom = np.concatenate([c["bonds"][1] + lo for c, lo in zip(batch, (0, 65, 89))])
    want_code = np.concatenate([c["bonds"][2] for c in batch])
    for kw in (dict(), dict(min_width=2.3), dict(reach=2), dict(reach=3, min_width=0.8)):
        got = _host(batch, 2.0, bonds=True, **kw)
        assert np.array_equal(got["bond_ptr"], want_ptr) and np.array_equal(got["bond_atom"], want_atom), kw
        assert np.array_equal(got["bond_shift"], want_code), kw


@pytest.mark.parametrize("name", ["cristobalite", "triclinic"])
@pytest.mark.parametrize("R, reach, nb", [(2.3, 1, 3), (2.7, 2, 5), (2.9, 3, 7)])
def test_grid_walk_pair_counts_where_the_walk_covers_every_bin_once(name, R, reach, nb):
    cell = GU.cells()[name]
    dR, nbins = 0.1, SU.nbins_of(R, 0.1)
    got = _host([cell], nbins * dR, reach=reach, dR=dR, nbins=nbins)
    assert got["nb"].tolist() == [[nb, nb, nb]]
    want = SU.pair_counts(cell, dR, nbins)
    assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"][0], want) and want.sum() > 0
    assert np.array_equal(got["counts"], got["counts"].transpose(0, 2, 1, 3))


@pytest.mark.parametrize("R, reach", [(4.6, 1), (5.6, 2), (6.0, 3)])
def test_grid_walk_pair_counts_on_the_random_cell(R, reach):
    cell = GU.cells()["r160"]
    dR, nbins = 0.05, SU.nbins_of(R, 0.05)
    got = _host([cell], nbins * dR, reach=reach, dR=dR, nbins=nbins)
    assert np.array_equal(got["counts"][0], SU.pair_counts(cell, dR, nbins))


def test_cells_too_thin_for_the_walk_are_refused():
    L = _lib.lib()
    cs = GU.cells()
    for name in ("cristobalite", "triclinic"):
        rc, _ = GU.host(L, [cs["r160"], cs[name]], 30 * 0.1, reach=2, dR=0.1, nbins=30)
        assert rc == EINVAL and b"cell 1 (widths" in L.egnn_last_error() and b"not griddable" in L.egnn_last_error(), L.egnn_last_error()
    rc, _ = GU.host(L, [cs["cristobalite"]], 2.39, bonds=True)
    assert rc == EINVAL and b"cell 0 (widths 7.16, 7.16, 7.16) is not griddable" in L.egnn_last_error()
    rc, _ = GU.host(L, [cs["cristobalite"]], 2.0, dR=0.1, nbins=21)      # pairs beyond the radius the grid was made for
    assert rc == EINVAL and b"beyond the radius" in L.egnn_last_error()
    assert GU.host(L, [cs["cristobalite"]], 2.39)[0] == 0                # bins alone: nothing to refuse


def test_device_entries_refuse_bad_grids_before_they_launch():
    """no GPU is touched here: every device pointer is a fake and each call returns before it would be read"""
    import ctypes as C
    L = _lib.lib()
    cs = GU.cells()
    p = C.c_void_p(64)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    cp = np.array([0, 2, 162], np.int32)                                        # the chain (not griddable) and r160
    lat = np.ascontiguousarray(np.stack([cs["chain"]["lattice"].reshape(9), cs["r160"]["lattice"].reshape(9)]))
    good = np.array([[0, 0, 0], [7, 8, 7]], np.int32)

    def bonds(nb=good, tiles=np.array([[1, 0], [1, 64], [1, 128]], np.int32), n_bins=392, reach=1, fill=False, lattice=lat):
        head = (None, 2, 162, vp(cp), None if lattice is None else vp(lattice), vp(nb), vp(tiles), p, p, p, p, n_bins, p, p, p, 2.0, reach, p, len(tiles))
        return L.egnn_cell_bonds_grid_fill(*head, p, 5, p, p) if fill else L.egnn_cell_bonds_grid_count(*head, p)

    def pairs(nb, tiles, n_bins, dR=0.05, nbins=92, reach=1, A=2):
        return L.egnn_cell_pair_counts_grid(None, 2, 162, A, vp(cp), vp(lat), vp(nb), vp(tiles), p, p, p, p, n_bins, p, p, p, dR, nbins, reach, p, len(tiles), p)

    tile1 = np.array([[1, 0]], np.int32)
    for call, word in ((lambda: bonds(tiles=np.array([[1, 0], [0, 0]], np.int32)), b"tile 1 names cell 0, which is not gridded"),
                       (lambda: bonds(tiles=np.array([[2, 0]], np.int32), fill=True), b"tile 0 names cell 2 outside [0, 2)"),
                       (lambda: bonds(nb=np.array([[0, 0, 0], [8, 8, 7]], np.int32), n_bins=448), b"cell 1 (widths 14.79"),   # finer than 14.79 / 2 allows
                       (lambda: bonds(nb=np.array([[0, 0, 0], [7, 8, 2]], np.int32), n_bins=112, fill=True), b"is not complete on"),
                       (lambda: bonds(nb=np.array([[3, 3, 3], [7, 8, 7]], np.int32), n_bins=419), b"cell 0 (widths 3.2"),
                       (lambda: bonds(n_bins=391), b"n_bins 391, but the grids of the batch hold 392 bins"),
                       (lambda: bonds(reach=4), b"reach 4"), (lambda: bonds(lattice=None), b"bad egnn_cell_bonds_grid_count arguments"),
                       (lambda: pairs(np.array([[0, 0, 0], [3, 3, 3]], np.int32), tile1, 27, A=5), b"5 atom types"),
                       (lambda: pairs(np.array([[0, 0, 0], [3, 3, 3]], np.int32), tile1, 27, nbins=0), b"nbins 0"),
                       (lambda: pairs(np.array([[0, 0, 0], [3, 3, 3]], np.int32), tile1, 27, dR=0.001, nbins=4600, A=2), b"histogram bins"),
                       (lambda: pairs(np.array([[0, 0, 0], [4, 3, 3]], np.int32), tile1, 36), b"cell 1 (widths 14.79")):   # 14.79 / 4.6 = 3.2 bins
        rc = call()
        assert rc == EINVAL and word in L.egnn_last_error(), (word, L.egnn_last_error())
    # a coarser grid than the radius allows is accepted by the checks: dims with min_width gives one
    assert _dims([cs["r160"]], 2.0, min_width=3.0) == [[4, 5, 4]]
    rc = L.egnn_cell_grid_count(None, 2, 162, vp(cp), vp(lat), vp(np.array([[0, 0, 0], [8, 8, 7]], np.int32)), 2.0, 1, p, p, p, p, 448, p, p)
    assert rc == EINVAL and b"cell 1 (widths 14.79" in L.egnn_last_error()


# ---- sanitizers ------------------------------------------------------------------------------------------------------------------------
def test_cell_grid_host_under_sanitizers(tmp_path):
    """the executable links its own sanitizer runtime (statically), so nothing is preloaded"""
    r = build_and_run(tmp_path, "cell_grid_main", ["cells/cell_grid_host.cpp", "cells/cell_stats_host.cpp", "cells/cell_host.cpp", "host_logic.cpp"])
    assert r.returncode == 0 and "CELL-GRID-OK" in r.stdout, f"rc={r.returncode}\nstdout:\n{r.stdout}\nstderr:\n{r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]

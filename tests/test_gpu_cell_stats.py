"""Real-space statistics of periodic cells on the device (csrc/cells/cell_stats.hip through diffusion_model_amd.cells) against the host
statement egnn_cell_stats_host, which tests/test_cell_stats_host.py pins to the numpy restatement without a GPU.  Every integer
output equals the host statement bitwise; g, n and total of the Python layer equal the restated finish within 1e-12 relative.

  * pair kernel: cells of 63, 64 and 65 atoms (the edge of the 64-centre block) and of 1,100 atoms at R = 3 (a second neighbour
    chunk); the one-atom cubic cell (1,331 images, 11 per axis, all of them the atom itself); cristobalite at R = 10 (125 images);
    the triclinic cell with an image box of (2, 2, 2) and of (1, 2, 1); A = 4 with nbins = 1024 (the histogram at the LDS limit) and
    nbins = 1; a mixed batch of all of these against each alone; two runs bitwise equal;
  * bond kernels: the dense cells of tests/_cells_util.py (32 bonds per atom: 496 angle pairs, several passes of the 64 lanes), the
    grid with more than 64 bonds per atom (the overflow, CN still exact, RuntimeError naming the cell), centres with 0 and 1 bonds,
    former and bridge swapped;
  * Python layer: structure_profile equals the separate calls, compare_structures of a batch with itself gives cos = 1 and l2 = 0
    wherever a curve is non-zero, and the refused arguments surface as ValueError / EgnnError before any launch.
"""
import functools

import numpy as np
import pytest
import torch

import diffusion_model_amd as dma
from diffusion_model_amd import _lib, cells as DC
from tests import _cell_stats_util as SU
from tests import _cells_util as CU

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL = 1e-12
INT_KEYS = ("coordination", "cn", "angles", "qn", "qn_hist", "overflow")


def _periodic(c):
    return dma.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=c["A"], id=c["name"])


def _typed(c, A, seed):
    return dict(c, types=np.random.default_rng(seed).integers(0, A, len(c["frac"])).astype(np.int32), A=A)


def _two_atom_cell():
    """two atoms 1.6 A apart in a 5 A cell: one bond each"""
    return dict(lattice=5.0 * np.eye(3), frac=np.array([[0.1, 0.2, 0.3], [0.42, 0.2, 0.3]]), types=np.array([1, 0], np.int32), A=2, name="two-atom",
                cutoff=CU.CUTOFF)


@functools.lru_cache(maxsize=None)
def _cells():
    cubic = dict(lattice=2.0 * np.eye(3), frac=np.array([[0.25, 0.5, 0.75]]), types=np.zeros(1, np.int32), A=1, name="cubic", cutoff=CU.CUTOFF)
    return dict(r63=CU.random_cell(63, 21), r64=CU.random_cell(64, 22), r65=CU.random_cell(65, 11, spread=2.0),
                big=CU.random_cell(1100, 13, check=False), cubic=cubic, cristobalite=CU.cristobalite_cell(), triclinic=CU.triclinic_cell(),
                one=CU.one_atom_cell(), two=_two_atom_cell(), overflow=CU.grid_cell(3, 3, 3, 0.75, 2.0))


# name -> (cell, R, dR): the settings of the pair tests
PAIR_CASES = dict(r63=("r63", 10.0, 0.01), r64=("r64", 10.0, 0.01), r65=("r65", 10.0, 0.01), big=("big", 3.0, 0.01), cubic=("cubic", 8.125, 0.0625),
                  cristobalite=("cristobalite", 10.0, 0.01), triclinic=("triclinic", 10.0, 0.01), triclinic_121=("triclinic", 7.1, 0.01))


def _host(cells, **kw):
    rc, got = SU.host(_lib.lib(), cells, **kw)
    assert rc == 0, _lib.lib().egnn_last_error()
    return got


def _close(got, want):
    return bool(np.all(np.abs(got - want) <= REL * np.abs(want)))


def _assert_rdf(cells, R, dR, sigma=0.0, A=None):
    """partial_rdf of the device against the host statement (counts, bitwise) and the restated finish (g, n, total)"""
    nbins = SU.nbins_of(R, dR)
    want = _host(cells, dR=dR, nbins=nbins, bonds=False, A=A)["counts"]
    out = DC.partial_rdf([_periodic(c) for c in cells], R=R, dR=dR, sigma=sigma, device=DEV)
    got = out.counts.cpu().numpy()
    assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(got, got.transpose(0, 2, 1, 3))
    fin = SU.finish(cells, want, dR, sigma=sigma)
    for k in ("r", "g", "n", "total", "volume"):
        g = getattr(out, k).cpu().numpy()
        assert g.dtype == np.float64 and g.shape == fin[k].shape and np.all(np.isfinite(g)) and _close(g, fin[k]), k
    assert np.array_equal(out.n_type.cpu().numpy(), fin["n_type"]) and out.sizes == [len(c["frac"]) for c in cells]
    return got


# ---- pair kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(PAIR_CASES))
def test_pair_counts_equal_the_host_statement(case):
    name, R, dR = PAIR_CASES[case]
    c = _cells()[name]
    nbins = SU.nbins_of(R, dR)
    box = SU.image_box(c["lattice"], dR, nbins).tolist()
    if case == "big":
        assert len(c["frac"]) > 1024                                          # a second neighbour chunk
    if case == "cubic":
        assert nbins == 130 and box == [5, 5, 5]                               # 11 per axis: 1,331 images
    if case == "cristobalite":
        assert box == [2, 2, 2]                                                # 125 images
    if case == "triclinic_121":
        assert box == [1, 2, 1]
    got = _assert_rdf([c], R, dR)
    if case == "cubic":
        assert got.sum() == 256                                                # the theta series up to n = 16
    if case == "cristobalite":
        assert got[0].sum(-1).tolist() == [[2976, 1376], [1376, 688]]


def test_pair_counts_at_the_histogram_limits():
    c = _typed(_cells()["r65"], 4, 3)
    got = _assert_rdf([c], 10.24, 0.01)                                       # 4 x 4 x 1024 bins: 64 KiB of LDS
    assert got.shape == (1, 4, 4, 1024)
    one = _assert_rdf([c], 5.0, 5.0)
    assert one.shape == (1, 4, 4, 1) and one.sum() == got[..., :500].sum()
    _assert_rdf([c], 5.0, 0.05, sigma=2.5)                                     # the smoothing filter of the Python layer
    three = _typed(_cells()["r64"], 3, 4)
    lacking = dict(three, types=np.minimum(three["types"], 1).astype(np.int32))
    out = _assert_rdf([three, lacking], 6.0, 0.05)
    assert not out[1, 2].any() and not out[1, :, 2].any()                      # a cell lacking a type: zeros, and finite g (asserted above)


def test_pair_counts_of_a_mixed_batch_equal_each_cell_alone():
    cs = _cells()
    names = ("r63", "cubic", "r64", "big", "cristobalite", "r65", "triclinic", "one")
    R, dR = 5.0, 0.01
    batch = [cs[k] for k in names]
    got = DC.pair_counts([_periodic(c) for c in batch], R=R, dR=dR, device=DEV)
    again = DC.pair_counts([_periodic(c) for c in batch], R=R, dR=dR, device=DEV)
    assert got.dtype == torch.int64 and torch.equal(got, again)               # two runs, bitwise
    want = _host(batch, dR=dR, nbins=500, bonds=False)["counts"]
    assert np.array_equal(got.cpu().numpy(), want)
    for c, k in enumerate(names):
        alone = DC.pair_counts(_periodic(dict(cs[k], A=2)), R=R, dR=dR, device=DEV)
        assert torch.equal(alone[0], got[c]), k
    rev = DC.pair_counts([_periodic(c) for c in batch[::-1]], R=R, dR=dR, device=DEV)
    assert torch.equal(rev.flip(0), got)


# ---- bond kernels --------------------------------------------------------------------------------------------------------------------
def _assert_bonds(cells, cutoff, **kw):
    want = _host(cells, pairs=False, cutoff=cutoff, **kw)
    cb = DC._CellBatch([_periodic(c) for c in cells], DEV)
    bonds = DC._bond_list(cb, cutoff)
    raw = DC._bond_stats(cb, bonds, kw.get("dtheta", 1.0), kw.get("max_cn", 16), kw.get("former", 1), kw.get("bridge", 0))
    got = {k: v.cpu().numpy() for k, v in zip(INT_KEYS, raw)}
    for k in INT_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["coordination"].sum(1), np.diff(bonds.row_ptr.cpu().numpy()))
    return got


@pytest.mark.parametrize("name", ["g27", "g80", "g22", "cscl"])
def test_bond_statistics_of_dense_cells(name):
    c = CU.dense_cells()[name]
    deg = np.diff(c["bonds"][0])
    if name == "g27":
        assert np.all(deg == 32)                                               # 496 pairs per centre: eight passes of the 64 lanes
    got = _assert_bonds([c], c["cutoff"], max_cn=40)
    assert got["overflow"].tolist() == [0] and got["angles"].sum() == int((deg * (deg - 1) // 2).sum())
    _assert_bonds([c], c["cutoff"], dtheta=0.5, max_cn=8, former=0, bridge=1)  # the roles swapped, the last CN bin saturating


def test_bond_statistics_mixed_batch_with_few_and_too_many_bonds():
    cs = _cells()
    batch = [cs["two"], cs["overflow"], cs["one"], cs["cristobalite"], cs["r65"], cs["triclinic"]]
    assert all(c["cutoff"] == CU.CUTOFF for c in batch)
    got = _assert_bonds(batch, CU.CUTOFF, max_cn=64)
    assert got["coordination"][:2].tolist() == [[1, 0], [0, 1]] and got["qn"][:2].tolist() == [0, -1]          # one bond each; the O is no bridge
    assert got["overflow"].tolist() == [0, 27, 0, 0, 0, 0] and not got["angles"][1].any()
    assert got["coordination"][29].tolist() == [0, 0] and got["cn"][2].sum() == 2                                # the one-atom cell: no bond
    assert got["qn_hist"][3, 4] == 8
    swapped = _assert_bonds(batch, CU.CUTOFF, former=0, bridge=1)
    assert swapped["qn_hist"][3, 2] == 16
    for c, cell in enumerate(batch):                                          # every cell alone gives the same bits
        alone = _assert_bonds([cell], CU.CUTOFF, max_cn=64)
        for k in ("cn", "angles", "qn_hist", "overflow"):
            assert np.array_equal(alone[k][0], got[k][c]), (cell["name"], k)


# ---- Python layer ---------------------------------------------------------------------------------------------------------------------
def test_overflow_raises_naming_the_cell():
    cs = _cells()
    with pytest.raises(RuntimeError, match=r"cell 1: 27 centre\(s\) with more than 64 bonds"):
        DC.bond_statistics([_periodic(cs["cristobalite"]), _periodic(cs["overflow"])], device=DEV)


def test_structure_profile_equals_the_separate_calls():
    cs = _cells()
    cells = [_periodic(cs[k]) for k in ("cristobalite", "r65", "triclinic")]
    kw = dict(R=6.0, dR=0.02, sigma=1.5)
    prof = DC.structure_profile(cells, cutoff=2.0, dtheta=2.0, max_cn=8, device=DEV, **kw)
    rdf = DC.partial_rdf(cells, device=DEV, **kw)
    bs = DC.bond_statistics(cells, cutoff=2.0, dtheta=2.0, max_cn=8, device=DEV)
    for k in ("r", "counts", "g", "n", "total", "n_type", "volume"):
        assert torch.equal(getattr(prof, k), getattr(rdf, k)), k
    for k in ("coordination", "cn", "angles", "qn", "qn_hist"):
        assert torch.equal(getattr(prof, k), getattr(bs, k)), k
    assert torch.equal(prof.counts, DC.pair_counts(cells, R=6.0, dR=0.02, device=DEV))
    assert prof.cn.dtype == torch.int64 and prof.angles.shape == (3, 2, 3, 91) and prof.qn.dtype == torch.int32 and prof.coordination.dtype == torch.int32
    assert torch.equal(prof.bonds.row_ptr, bs.bonds.row_ptr) and prof.sizes == [24, 65, 24]


def test_compare_structures_of_a_batch_with_itself():
    cs = _cells()
    cells = [_periodic(cs[k]) for k in ("cristobalite", "r65")]
    cmp = DC.compare_structures(cells, cells, R=6.0, dR=0.02, sigma=1.0, device=DEV)
    assert cmp["g"]["cos"].shape == (2, 2, 2) and cmp["total"]["cos"].shape == (2,) and cmp["angles"]["cos"].shape == (2, 2, 3)
    assert cmp["cn"]["cos"].shape == (2, 2, 2) and cmp["qn"]["cos"].shape == (2,)
    curves = dict(g=cmp["a"].g, total=cmp["a"].total, angles=cmp["a"].angles, cn=cmp["a"].cn, qn=cmp["a"].qn_hist)
    for k, curve in curves.items():
        nonzero = curve.double().abs().sum(-1) > 0
        assert bool(nonzero.any()), k
        assert float((cmp[k]["cos"][nonzero] - 1.0).abs().max()) <= 1e-12 and bool(torch.isnan(cmp[k]["cos"][~nonzero]).all()), k
        assert float(cmp[k]["l2"].abs().max()) == 0.0 and float(cmp[k]["wasserstein"].abs().max()) == 0.0, k
    other = DC.compare_structures(cells, cells[::-1], R=6.0, dR=0.02, device=DEV)          # atom counts differ
    assert other["sizes_a"] == [24, 65] and other["sizes_b"] == [65, 24] and float(other["total"]["l2"].min()) > 0.0


def test_refused_arguments_surface_before_any_launch():
    cs = _cells()
    cell = _periodic(cs["cristobalite"])
    for kw, word in ((dict(dR=0.0), "positive"), (dict(R=-1.0), "positive")):
        with pytest.raises(ValueError, match=word):
            DC.pair_counts(cell, device=DEV, **kw)
    with pytest.raises(_lib.EgnnError, match="nbins 0"):
        DC.pair_counts(cell, R=0.001, dR=0.01, device=DEV)
    with pytest.raises(_lib.EgnnError, match="cell 1 needs more than 16 images along axis 0"):
        DC.pair_counts([cell, _periodic(cs["cubic"])], R=40.0, dR=0.1, device=DEV)
    with pytest.raises(_lib.EgnnError, match="histogram bins"):
        DC.pair_counts(_periodic(_typed(cs["r65"], 4, 3)), R=10.25, dR=0.01, device=DEV)
    flat = dma.PeriodicCell(np.array([[3.2, 0, 0], [0, 3.2, 0], [3.2, 3.2, 0.0]]), np.zeros((1, 3)), types=[0], num_types=2)
    with pytest.raises(_lib.EgnnError, match="cell 1 has a singular lattice"):
        DC.partial_rdf([cell, flat], device=DEV)
    for kw, word in ((dict(dtheta=0.25), "dtheta"), (dict(max_cn=65), "max_cn 65"), (dict(former=2), "former 2 and bridge 0"),
                     (dict(bridge=1), "former 1 and bridge 1")):
        with pytest.raises(_lib.EgnnError, match=word):
            DC.bond_statistics(cell, device=DEV, **kw)
    with pytest.raises(ValueError, match="weights"):
        DC.partial_rdf(cell, weights=[1.0, 2.0, 3.0], device=DEV)

"""GPU tests of the shortest-path ring statistics (csrc/eval/rings.hip: egnn_rings) and of their Python surface
(stats.ring_statistics, cells.ring_statistics, stats.compare_rings):

  * the device equals the host statement (egnn_rings_host, which tests/test_rings_host.py holds to the restatements) BITWISE in
    size, count, overflow and histogram: on the mixed cell batch at cutoff 2.0, on the random 65- and 160-atom cells at 2.8 with
    max_size 12, on the clouds of 1 .. 257 atoms at scale 1.5 (sizes on either side of 64 lanes and 128 / 256 rows), on the
    1,100-atom cell (atoms on either side of the 1024-atom chunk of the bond kernels), at the site limit L and L - 1 (the
    overflow path), on the saturating layered graph, and on the crowd (33 bonds per atom).  None of these labels more than 589
    sites in a search, has a frontier above the 256 threads or a centre above 12 bonds;
  * beyond one workgroup of sites, the reach asserted from the restatement first: the fan graph (tests/_ring_util.py: fan_csr) --
    levels of 1,024 sites, 2,594 sites labelled in 8,192 slots with shared home slots (probe chains) and slot numbers above 2^12 in
    the uint16 lists, max_sites = 2,594 (fits), 2,593 (overflow) and 4,096, centres inside the wide layers -- equals the host
    statement and the restatement; the dense cells with 24-26 and with exactly 32 bonds per atom (the limit, searched) equal the
    host statement on every centre and the restatement on six, and cells.ring_statistics accepts the 32-bond cell;
  * two runs of one call are bitwise equal;
  * the Python functions return the known answers of cristobalite and of ring(6), select centres by type, compare a list with
    itself at L1 = 0 and cosine = 1, raise on the crowd and refuse CPU tensors."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import diffusion_model_amd as dma
from diffusion_model_amd import _lib, stats
from tests import _cells_util as CU
from tests import _ring_util as RU
from tests import _topo_util as TU

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _cells():
    return dict(chain=CU.chain_cell(), cristobalite=CU.cristobalite_cell(), triclinic=CU.triclinic_cell(), r65=CU.random_cell(65, 11),
                r160=CU.random_cell(160, 12), one=CU.one_atom_cell())


def _pcell(c):
    return dma.PeriodicCell(c["lattice"], c["frac"], types=c["types"], num_types=c["A"], id=c["name"])


def _onehot(types, A):
    return torch.nn.functional.one_hot(torch.from_numpy(np.asarray(types)).long(), A)


def _assert_device_equals_host(csr, **kw):
    L = _lib.lib()
    rc, want = RU.host(L, csr, **kw)
    assert rc == 0, L.egnn_last_error()
    rc, got = RU.device(L, csr, **kw)
    assert rc == 0, L.egnn_last_error()
    for k in ("size", "count", "overflow", "hist"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    return got


def test_device_equals_host_on_the_mixed_cell_batch():
    csr = RU.cells_csr([_cells()[k] for k in ("chain", "cristobalite", "triclinic", "r65", "r160", "one")])
    got = _assert_device_equals_host(csr, max_size=16)
    assert got["hist"][0, 12] >= 32 and got["hist"][1, 12] >= 96          # the two cristobalite cells at least
    centres = np.random.default_rng(5).integers(0, csr["N"], 60)
    _assert_device_equals_host(csr, centres=centres, max_size=32)


@pytest.mark.parametrize("name", ["r65", "r160"])
def test_device_equals_host_on_random_cells(name):
    csr = RU.cells_csr([_cells()[name]], cutoff=2.8)
    got = _assert_device_equals_host(csr, max_size=12)
    assert len(set(got["size"].tolist()) - {0}) >= 5 and got["count"].max() > 1 and not got["overflow"].any()
    again = RU.device(_lib.lib(), csr, max_size=12, mirrors=False)[1]
    for k in ("size", "count", "overflow", "hist"):
        assert np.array_equal(got[k], again[k]), k                              # two runs, bitwise


def test_device_equals_host_on_clouds():
    pos, types = TU.cloud(3, TU.SIZES, 2)
    csr = RU.clusters_csr(pos, types, TU.SIZES, 2, scale=1.5)
    got = _assert_device_equals_host(csr, max_size=16)
    assert got["size"].max() == 16 and got["count"].max() > 1
    for max_size in (3, 4):
        _assert_device_equals_host(csr, max_size=max_size)


def test_device_equals_host_across_the_chunk():
    csr = RU.cells_csr([CU.random_cell(1100, 13)])
    assert csr["N"] > 1024
    got = _assert_device_equals_host(csr, max_size=16)
    assert len(got["overflow"]) == 1100


def test_device_equals_host_at_the_site_limit():
    csr = RU.cells_csr([_cells()["cristobalite"]])
    si = np.nonzero(csr["types"] == 1)[0]
    L = int(RU.restated(csr, centres=si[:1], max_size=16)["labelled"].max())
    fits = _assert_device_equals_host(csr, centres=si, max_size=16, max_sites=L)
    assert not fits["overflow"].any() and np.all(fits["size"] == 12) and np.all(fits["count"] == 2)
    short = _assert_device_equals_host(csr, centres=si, max_size=16, max_sites=L - 1)
    assert np.all(short["overflow"] == 1) and np.any(short["size"] == -1) and not short["hist"][:, 0].any()
    _assert_device_equals_host(csr, max_size=16, max_sites=1)
    _assert_device_equals_host(csr, max_size=16, max_sites=64)


def test_device_saturates_and_reports_the_crowd():
    csr, true, size = RU.layered_csr()
    got = _assert_device_equals_host(csr, centres=[0], max_size=16)
    assert true >= 2 ** 31 and got["size"].tolist() == [size] and got["count"].tolist() == [2 ** 31 - 1]
    _assert_device_equals_host(csr, max_size=16)
    pos, types = TU.crowd(34)
    crowd = RU.clusters_csr(pos, types, [34], 2)
    got = _assert_device_equals_host(crowd, max_size=16)
    assert np.all(got["overflow"] == 1) and np.all(got["size"] == -1) and not got["hist"].any()


# ---- beyond one workgroup of sites -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fan():
    """the fan graph and what the restatement says of the search from its centre (tests/test_rings_host.py holds the host
    statement to it)"""
    csr, layer = RU.fan_csr()
    want = RU.restated(csr, centres=[0], max_size=16)
    return csr, layer, want, int(want["labelled"][0])


def test_device_equals_host_on_the_fan_graph():
    """frontiers of 1,024 sites for 256 threads, 2,594 labelled sites in 8,192 slots (probe chains; slot numbers above 2^12 in the
    uint16 lists), the site limit at exactly the number labelled and one below"""
    csr, layer, want, labelled = _fan()
    assert 2048 < labelled <= 4096 and max(RU.level_widths(csr, 0, 0)) > 256                 # preconditions, from the restatement
    assert 1 < want["count"][0] < RU.COUNT_MAX and want["size"].tolist() == [len(layer) + 3] and np.diff(csr["row_ptr"]).max() == 32
    home = RU.home_slots(range(1, csr["N"]), 8192)
    assert np.sum(np.bincount(home, minlength=8192) > 1) >= 100 and home.max() >= 4096        # probe chains; slots beyond 12 bits
    for max_sites in (labelled, 4096):
        got = _assert_device_equals_host(csr, centres=[0], max_size=16, max_sites=max_sites)
        RU.assert_equal(got, want)
    short = _assert_device_equals_host(csr, centres=[0], max_size=16, max_sites=labelled - 1)
    RU.assert_equal(short, RU.restated(csr, centres=[0], max_size=16, max_sites=labelled - 1))
    assert short["overflow"].tolist() == [1] and short["size"].tolist() == [-1] and short["count"].tolist() == [0]
    centres = RU.fan_centres(layer)
    inside = RU.restated(csr, centres=centres, max_size=16)
    assert inside["labelled"].max() > 2048 and inside["count"].max() > 1
    got = _assert_device_equals_host(csr, centres=centres, max_size=16)
    RU.assert_equal(got, inside)
    again = RU.device(_lib.lib(), csr, centres=centres, max_size=16, mirrors=False)[1]
    for k in ("size", "count", "overflow", "hist"):
        assert np.array_equal(got[k], again[k]), k                                             # two runs, bitwise
    spread = _assert_device_equals_host(csr, centres=np.arange(0, csr["N"], 16), max_size=12)    # 163 centres over every layer
    assert not spread["overflow"].any() and len(set(spread["size"].tolist())) >= 4


@pytest.mark.parametrize("name", ["g80", "g27"])
def test_device_equals_host_at_the_degree_limit(name):
    """the dense cells: 24-26 bonds per atom (up to 325 angles a centre), and exactly 32 bonds -- the limit, searched, not the
    overflow -- about every atom"""
    c = CU.dense_cells()[name]
    csr = RU.cells_csr([c], cutoff=c["cutoff"])
    deg = np.diff(csr["row_ptr"])
    assert (deg.min() >= 24 and deg.max() <= 32) if name == "g80" else np.all(deg == 32)
    got = _assert_device_equals_host(csr, max_size=16)                                         # all centres
    assert not got["overflow"].any() and got["size"].min() >= 3 and got["count"].max() > 1
    centres = RU.dense_ring_centres(name)
    want = RU.restated(csr, centres=centres, max_size=16)
    assert want["labelled"].min() > 256
    RU.assert_equal(_assert_device_equals_host(csr, centres=centres, max_size=16), want)


def test_cells_ring_statistics_at_the_degree_limit():
    c = CU.dense_cells()["g27"]
    csr = RU.cells_csr([c], cutoff=1.6)
    assert np.all(np.diff(csr["row_ptr"]) == 32)
    centres = RU.dense_ring_centres("g27")
    want = RU.restated(csr, centres=centres, max_size=16)
    rs = dma.cells.ring_statistics(_pcell(c), centres=torch.from_numpy(centres.astype(np.int64)), cutoff=1.6, device=DEV)      # does not raise
    assert np.array_equal(rs.size.cpu().numpy(), want["size"]) and np.array_equal(rs.count.cpu().numpy(), want["count"])
    ap = want["angle_ptr"]
    smallest = [int(want["size"][ap[m]:ap[m + 1]][want["size"][ap[m]:ap[m + 1]] > 0].min()) for m in range(len(centres))]
    assert rs.per_centre_smallest.tolist() == smallest and rs.angle_ptr.tolist() == ap.tolist() and ap[1] == 496


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def test_cells_ring_statistics_on_cristobalite():
    cell = _pcell(_cells()["cristobalite"])
    rs = dma.cells.ring_statistics(cell, device=DEV)
    assert rs.size.dtype == torch.int64 and rs.size.tolist() == [12] * 64
    assert rs.count.tolist() == [2] * 48 + [6] * 16                                  # 8 Si with 6 angles, then 16 O with one
    assert rs.angle_ptr.tolist() == list(range(0, 49, 6)) + list(range(49, 65))
    assert rs.neighbours[:7].tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3], [0, 1]] and rs.neighbours[-1].tolist() == [0, 1]
    assert rs.centre.tolist() == list(range(24)) and rs.per_centre_smallest.tolist() == [12] * 24
    assert rs.histogram.dtype == torch.int64 and rs.histogram.shape == (2, 17)
    assert rs.histogram[0].tolist() == [0] * 12 + [16] + [0] * 4 and rs.histogram[1].tolist() == [0] * 12 + [48] + [0] * 4
    si = dma.cells.ring_statistics(cell, centres=1, device=DEV)
    assert si.centre.tolist() == list(range(8)) and si.size.tolist() == [12] * 48 and si.histogram[0].sum() == 0
    low = dma.cells.ring_statistics([_pcell(_cells()["chain"]), cell], centres=torch.tensor([25, 1, 25]), max_size=10, device=DEV)
    assert low.size.tolist() == [0, 0, 0] and low.per_centre_smallest.tolist() == [0, 0, 0] and low.histogram[0, 0] == 3
    with pytest.raises(ValueError, match="cell 1, atom 0: .*max_sites = 64"):
        dma.cells.ring_statistics([_pcell(_cells()["chain"]), cell], max_sites=64, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dma.cells.ring_statistics(cell, device="cpu")


def test_stats_ring_statistics_and_compare_rings():
    pos, types = TU.ring(6)
    rs = stats.ring_statistics(torch.from_numpy(pos).to(DEV), _onehot(types, 2).to(DEV), [6])
    assert rs.size.tolist() == [6] * 6 and rs.count.tolist() == [1] * 6 and rs.per_centre_smallest.tolist() == [6] * 6
    assert rs.histogram[:, 6].tolist() == [3, 3] and rs.neighbours.tolist() == [[0, 1]] * 6
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stats.ring_statistics(torch.from_numpy(pos), _onehot(types, 2), [6])
    cpos, ctypes_ = TU.crowd(34)
    with pytest.raises(ValueError, match="graph 1, atom 0: more than 32 bonds"):
        stats.ring_statistics(torch.from_numpy(np.concatenate([pos, cpos])).to(DEV), _onehot(np.concatenate([types, ctypes_]), 2).to(DEV), [6, 34])
    # the Python path equals the restatement on the clouds, whose bond graph the device builds itself
    cp, ct = TU.cloud(3, TU.SIZES, 2)
    csr = RU.clusters_csr(cp, ct, TU.SIZES, 2, scale=1.5)
    want = RU.restated(csr, max_size=16)
    got = stats.ring_statistics(torch.from_numpy(cp).to(DEV), _onehot(ct, 2).to(DEV), TU.SIZES, scale=1.5)
    assert np.array_equal(got.size.cpu().numpy(), want["size"]) and np.array_equal(got.count.cpu().numpy(), want["count"])
    assert np.array_equal(got.histogram.cpu().numpy(), want["hist"])
    # a list against itself; a graph without a ring on both sides (the star, the 7-atom cloud) gets L1 = 0 and cosine = 1
    graphs = [TU.ring(6), TU.star(8), (cp[-7:], ct[-7:]), (cp[6:69], ct[6:69])]
    rec = lambda pt, on: SimpleNamespace(pos=torch.from_numpy(pt[0]).to(on), x=_onehot(pt[1], 2).to(on))
    out = stats.compare_rings([rec(g, "cpu") for g in graphs], [[rec(g, DEV)] for g in graphs])
    assert out["l1"] == [0.0] * 4 and out["cosine"] == pytest.approx([1.0] * 4, abs=1e-12)
    assert out["original"][0, 6] == 1.0 and not out["original"][1].any() and not out["generated"][2].any() and out["original"][3].sum() == pytest.approx(1.0)

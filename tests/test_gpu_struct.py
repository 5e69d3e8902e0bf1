"""GPU tests of the whole-structure statistics (csrc/eval/structure.hip through diffusion_model_amd.stats): pair counts,
coordination numbers and bond angles over every centre, exact against the numpy restatement of tests/_struct_util.py; partial
RDFs against the executed reference (tests/golden/struct_golden.npz); cross-checks against stats.rdf and stats.si_o_si.

Integer outputs are compared EXACTLY.  That is meaningful because the float32 distance is bitwise the restatement's (fixed
order, no contraction) and every test first asserts that no angle of its input lies within 1e-9 degrees of an angle-bin edge (the
float64 acos of two libraries may differ in the last bit): an ambiguous input fails loudly instead of hiding a miscount.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import diffusion_model_amd as dma
from diffusion_model_amd import _lib, stats
from tests import _struct_util as SU
from tests._util import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
# cross the 64 lanes of a wavefront (= the 64-centre block of a pair tile), 128 and the 256-thread workgroup; tiles meet graph
# boundaries and the last centre block and neighbour chunk of a graph are partial
SIZES = [1, 2, 3, 64, 65, 129, 257, 7]
RADIAL = ((5.0, 0.01), (4.0, 0.02), (10.24, 0.01))            # defaults, the second golden setting, the limit nbins = 1024
BONDS = (dict(cutoff=2.0, dtheta=1.0, max_cn=16), dict(cutoff=2.5, dtheta=2.5, max_cn=3))


def _onehot(types, A):
    return torch.eye(A, dtype=torch.int64)[torch.from_numpy(np.asarray(types)).long()]


def _device_counts(pos, types, sizes, A, R=5.0, dR=0.01, **bond):
    p, oh = torch.from_numpy(pos).to(DEV), _onehot(types, A).to(DEV)
    c = stats.pair_counts(p, oh, sizes, R=R, dR=dR)
    cn, ang = stats.bond_statistics(p, oh, sizes, **bond)
    assert c.dtype == cn.dtype == ang.dtype == torch.int64
    return c.cpu().numpy(), cn.cpu().numpy(), ang.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _mixed(A):
    """the seeded mixed batch and its restatement (computed once, never changed)"""
    pos, types = SU.random_batch(100 + A, SIZES, A)
    radial = {(R, dR): np.stack([SU.pair_counts(p, t, A, R, dR) for p, t in _split(pos, types, SIZES)]) for R, dR in RADIAL}
    bonds = [SU.batch_statistics(pos, types, SIZES, A, **kw)[1:] for kw in BONDS]
    return pos, types, radial, bonds


def _split(pos, types, sizes):
    lo = 0
    for n in sizes:
        yield pos[lo:lo + n], types[lo:lo + n]
        lo += n


@pytest.mark.parametrize("A", [1, 2, 3])
def test_integer_outputs_equal_the_restatement_on_a_mixed_batch(A):
    pos, types, radial, bonds = _mixed(A)
    for kw, (cn_w, ang_w, over_w, gap) in zip(BONDS, bonds):
        assert gap >= 1e-9 and over_w.sum() == 0 and ang_w.sum() > 50, "ambiguous or empty input"
        for R, dR in (RADIAL if kw is BONDS[0] else RADIAL[:1]):
            c, cn, ang = _device_counts(pos, types, SIZES, A, R=R, dR=dR, **kw)
            want = radial[R, dR]
            assert c.shape == want.shape and want.sum() > 0
            assert np.array_equal(c, want), (A, R, dR, int(np.abs(c - want).sum()))
            assert np.array_equal(cn, cn_w), (A, kw)
            assert np.array_equal(ang, ang_w), (A, kw, int(np.abs(ang - ang_w).sum()))
    assert radial[10.24, 0.01].shape[-1] == 1024


def test_a_graph_of_more_than_one_neighbour_chunk():
    n, A = 1100, 2
    pos, types = SU.random_batch(7, [n], A)
    c_w, cn_w, ang_w, over_w, gap = SU.batch_statistics(pos, types, [n], A)
    assert gap >= 1e-9 and over_w.sum() == 0 and ang_w.sum() > 500
    c, cn, ang = _device_counts(pos, types, [n], A)
    assert np.array_equal(c, c_w) and np.array_equal(cn, cn_w) and np.array_equal(ang, ang_w)
    assert c.sum() < n * (n - 1)          # the box is wider than R: pairs beyond the last bin are in no bin


def _fixture(A):
    G = load_golden("struct_golden.npz")
    keep = [g for g, a in enumerate(G["A"].tolist()) if a == A]
    pos = np.concatenate([G[f"g{g}.pos"] for g in keep])
    types = np.concatenate([G[f"g{g}.types"] for g in keep])
    return G, keep, pos, types, [int(G["sizes"][g]) for g in keep]


@pytest.mark.parametrize("A", [2, 3])
def test_partial_rdf_matches_the_executed_reference(A):
    """sum over the neighbour type of g_ab = the mean over the centres of type a of the reference's RDF(roll(position, i)); the
    bar of test_statistics_match_executed_reference_goldens: float32 storage of values computed in fp64"""
    G, keep, pos, types, sizes = _fixture(A)
    p, oh = torch.from_numpy(pos).to(DEV), _onehot(types, A).to(DEV)
    for s, (sigma, R, dR) in enumerate(G["settings"].tolist()):
        got = stats.partial_rdf(p, oh, sizes, sigma=sigma, R=R, dR=dR)
        assert got.dtype == torch.float32 and got.shape == (len(sizes), A, A, SU.nbins_of(R, dR))
        got = got.double().sum(2).cpu().numpy()
        for k, g in enumerate(keep):
            want = G[f"g{g}.rdf{s}"]
            err = np.abs(got[k] - want).max()
            assert err <= 1e-6 * max(1.0, np.abs(want).max()), (g, s, err)
    # and the integer outputs of the fixture, whose two conditions hold by construction
    c_w, cn_w, ang_w, _, gap = SU.batch_statistics(pos, types, sizes, A)
    assert gap >= 1e-9
    c, cn, ang = _device_counts(pos, types, sizes, A)
    assert np.array_equal(c, c_w) and np.array_equal(cn, cn_w) and np.array_equal(ang, ang_w)


def test_partial_rdf_of_a_lone_centre_type_is_the_rdf_about_atom_0():
    sizes = [64, 17, 30, 2]
    pos, _ = SU.random_batch(11, sizes, 2, box_per_atom=2.0)
    types = np.ones(sum(sizes), dtype=np.int32)
    types[np.cumsum([0] + sizes[:-1])] = 0                     # atom 0 of every graph is its only atom of type 0
    p, oh = torch.from_numpy(pos).to(DEV), _onehot(types, 2).to(DEV)
    for sigma, R, dR in ((5, 5.0, 0.01), (3, 4.0, 0.02)):
        got = stats.partial_rdf(p, oh, sizes, sigma=sigma, R=R, dR=dR)[:, 0].double().sum(1).cpu().numpy()
        want = stats.rdf(p, sizes, sigma=sigma, R=R, dR=dR).double().cpu().numpy()
        assert np.abs(want).max() > 0.1
        for g in range(len(sizes)):
            assert np.abs(got[g] - want[g]).max() <= 1e-6 * max(1.0, np.abs(want[g]).max()), g


def test_angle_of_a_triangle_lands_in_the_bin_of_si_o_si():
    G = load_golden("stats_golden.npz")
    names = [str(n) for n in G["names"]]
    tri = np.concatenate([G[f"{n}.pos"][:3] for n in names]).astype(np.float32)
    types = np.tile(np.array([0, 1, 1], dtype=np.int32), len(names))
    sizes = [3] * len(names)
    p, oh = torch.from_numpy(tri).to(DEV), _onehot(types, 2).to(DEV)
    valid, ang, _ = stats.si_o_si(p, oh, sizes, cutoff=100.0)
    cn, angles = stats.bond_statistics(p, oh, sizes, cutoff=100.0)
    pair = SU.pair_index(1, 1, 2)
    for g, name in enumerate(names):
        theta = [r[3] for r in SU.bonded_angles(tri[3 * g:3 * g + 3], types[:3], 100.0)[0] if r[0] == 0]
        # si_o_si's angle is float32 (2e-3 degrees, 5e-2 next to 180): the comparison needs the angle that far inside its bin
        assert len(theta) == 1 and SU.angle_gap(theta, 1.0) > (5e-2 if theta[0] > 179.0 else 5e-3), name
        row = angles[g, 0, pair].cpu().numpy()
        assert bool(valid[g]) and row.sum() == 1 and row[int(np.floor(float(ang[g]) / 1.0 + 0.5))] == 1, name
        assert int(angles[g, 0].sum()) == 1 and int(cn[g, 0, 1, 2]) == 1 and int(cn[g, 1, 0, 1]) == 2


def _sphere(n_points, seed=3):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n_points, 3))
    return np.concatenate([np.zeros((1, 3)), 1.5 * v / np.linalg.norm(v, axis=1, keepdims=True)]).astype(np.float32)


def test_neighbour_cap():
    """a centre with 64 bonds is exact; with 65 its angles are not taken, bond_statistics raises, CN still counts all 65"""
    pos = _sphere(64)
    types = np.array([0] + [1] * 32 + [2] * 32, dtype=np.int32)
    c_w, cn_w, ang_w, over_w, gap = SU.batch_statistics(pos, types, [65], 3, max_cn=64)
    assert gap >= 1e-9 and over_w.tolist() == [0] and cn_w[0, 0, 1, 32] == 1 and cn_w[0, 0, 2, 32] == 1
    assert ang_w[0, 0].sum() == 64 * 63 // 2 and ang_w[0, 1:].sum() > 64 * 100       # each sphere point has about 30 bonds
    c, cn, ang = _device_counts(pos, types, [65], 3, max_cn=64)
    assert np.array_equal(c, c_w) and np.array_equal(cn, cn_w) and np.array_equal(ang, ang_w)

    pos = _sphere(65)
    types = np.array([0] + [1] * 33 + [2] * 32, dtype=np.int32)
    c_w, cn_w, ang_w, over_w, gap = SU.batch_statistics(pos, types, [66], 3, max_cn=64)
    assert gap >= 1e-9 and over_w.tolist() == [1] and ang_w[0, 0].sum() == 0
    p, oh = torch.from_numpy(pos).to(DEV), _onehot(types, 3).to(DEV)
    with pytest.raises(RuntimeError, match="graph 0"):
        stats.bond_statistics(p, oh, [66], max_cn=64)
    cn, ang, over = stats._bonds(stats._StructInput(p, oh, [66], "test"), 2.0, 1.0, 64)
    assert over.tolist() == [1] and int(cn[0, 0, 1, 33]) == 1 and int(cn[0, 0, 2, 32]) == 1      # 33 + 32 = 65 bonds counted
    assert np.array_equal(cn.cpu().numpy(), cn_w) and np.array_equal(ang.cpu().numpy(), ang_w)


def test_exact_invariances():
    A = 2
    pos, types, _, _ = _mixed(A)
    base = _device_counts(pos, types, SIZES, A)
    again = _device_counts(pos, types, SIZES, A)
    assert all(np.array_equal(a, b) for a, b in zip(base, again))
    p, oh = torch.from_numpy(pos).to(DEV), _onehot(types, A).to(DEV)
    assert torch.equal(stats.partial_rdf(p, oh, SIZES), stats.partial_rdf(p, oh, SIZES))         # two runs are bitwise equal
    # permuting the atoms inside each graph changes nothing
    rng = np.random.default_rng(0)
    perm = np.concatenate([lo + rng.permutation(n) for lo, n in zip(np.cumsum([0] + SIZES[:-1]), SIZES)])
    shuffled = _device_counts(pos[perm], types[perm], SIZES, A)
    assert all(np.array_equal(a, b) for a, b in zip(base, shuffled))
    # a graph's rows do not depend on which other graphs share the batch
    lo = 0
    for g, n in enumerate(SIZES):
        alone = _device_counts(pos[lo:lo + n], types[lo:lo + n], [n], A)
        assert all(np.array_equal(a[0], b[g]) for a, b in zip(alone, base)), g
        lo += n
    order = [5, 0, 7, 3, 6, 1, 4, 2]
    parts = list(_split(pos, types, SIZES))
    mixed = _device_counts(np.concatenate([parts[g][0] for g in order]), np.concatenate([parts[g][1] for g in order]),
                           [SIZES[g] for g in order], A)
    assert all(np.array_equal(a, b[order]) for a, b in zip(mixed, base))


def test_absent_type_and_one_atom_graph():
    sizes = [1, 40, 1]
    pos, types = SU.random_batch(5, sizes, 2)                  # types 0 and 1 only, declared as A = 3
    types[0], types[-1] = 1, 0
    p, oh = torch.from_numpy(pos).to(DEV), _onehot(types, 3).to(DEV)
    prof = stats.structure_profile(p, oh, sizes)
    g = prof.partial_rdf
    assert torch.isfinite(g).all() and float(g[1, :2, :2].abs().max()) > 0
    assert not g[:, 2].any() and not g[:, :, 2].any() and not prof.pair_counts[:, 2].any() and not prof.angles[:, 2].any()
    assert prof.n_type.tolist() == [[0, 1, 0], [int((types[1:41] == 0).sum()), int((types[1:41] == 1).sum()), 0], [1, 0, 0]]
    for k, a in ((0, 1), (2, 0)):                              # a one-atom graph: zeros, and one centre without neighbours
        assert not prof.pair_counts[k].any() and not prof.angles[k].any() and not g[k].any()
        assert prof.cn[k, a, :, 0].tolist() == [1, 1, 1] and int(prof.cn[k].sum()) == 3
    with pytest.raises(ValueError):
        stats.pair_counts(p, torch.ones(42, 3, device=DEV), sizes)
    with pytest.raises(RuntimeError):
        stats.pair_counts(p.cpu(), oh.cpu(), sizes)


def test_compare_structures():
    G, keep, _, _, _ = _fixture(2)
    a = (G["g4.pos"], G["g4.types"])                           # 64 atoms
    b = (G["g5.pos"][:64], G["g5.types"][:64])                 # the first 64 atoms of the 65-atom graph
    c = (G["g3.pos"], G["g3.types"])                           # 20 atoms
    graph = lambda pt, on, k=0: SimpleNamespace(pos=torch.from_numpy(pt[0]).to(on), x=_onehot(pt[1], 2).to(on), id=f"mp-{k}")
    originals = [graph(a, "cpu", 0), graph(c, "cpu", 1), graph(b, "cpu", 2)]
    same = stats.compare_structures(originals, [[graph(a, DEV)], [graph(c, DEV)], [graph(b, DEV)]])
    for key in ("rdf", "angles"):
        curves = getattr(same["original"], "partial_rdf" if key == "rdf" else key)
        live = curves.abs().sum(-1) > 0
        assert int(live.sum()) >= 6
        assert float((same[key]["cos"][live] - 1).abs().max()) <= 1e-12 and torch.isnan(same[key]["cos"][~live]).all()
        for m in ("l2", "mse", "wasserstein"):
            assert float(same[key][m].abs().max()) == 0.0
        total_live = curves.double().sum(0).abs().sum(-1) > 0
        assert float((same["total"][key]["cos"][total_live] - 1).abs().max()) <= 1e-12
    assert torch.equal(same["cn_original"], same["cn_generated"]) and same["sizes"] == [64, 20, 64]

    res = stats.compare_structures(originals, [[graph(b, DEV)], [graph(c, DEV)], [graph(a, DEV)]])
    o, g = res["original"], res["generated"]
    scalar = dict(cos=stats.cos_similarity, l2=stats.rdf_l2, mse=stats.rdf_mse, wasserstein=stats.wasserstein)
    checked = 0
    for key, co, cg in (("rdf", o.partial_rdf, g.partial_rdf), ("angles", o.angles, g.angles)):
        for k in (0, 2):
            for idx in np.ndindex(*co.shape[1:3]):
                x, y = co[(k,) + idx].double(), cg[(k,) + idx].double()
                if not (x.any() and y.any()):
                    continue
                for m, fn in scalar.items():
                    want = fn(x, y)
                    assert abs(float(res[key][m][(k,) + idx]) - want) <= 1e-5 * max(1.0, abs(want)), (key, k, idx, m)
                    checked += 1
        x, y = co.double().sum(0)[0, 1], cg.double().sum(0)[0, 1]
        assert abs(float(res["total"][key]["l2"][0, 1]) - stats.rdf_l2(x, y)) <= 1e-5 * max(1.0, stats.rdf_l2(x, y))
    assert checked >= 32 and float(res["rdf"]["l2"][0].max()) > 0.1 and float(res["rdf"]["l2"][1].max()) == 0.0


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_the_lds_limit_is_raised_on_every_device_of_a_process():
    """both kernels at their largest dynamic LDS (A = 4 with nbins = 1024; dtheta = 0.5 with max_cn = 64: above the 64 KiB a function
    is given by default), first on cuda:0, then on cuda:1 of the same process, each equal to the host statement: the limit belongs
    to the function on one device, so the second device needs a raise of its own"""
    sizes, A = [5, 1, 70], 4   # 70 crosses the 64-centre block
    kw = dict(R=10.24, dR=0.01, cutoff=2.0, dtheta=0.5, max_cn=64)
    pos, types = SU.random_batch(11, sizes, A)
    assert SU.nbins_of(kw["R"], kw["dR"]) == 1024 and SU.batch_statistics(pos, types, sizes, A, **kw)[4] >= 1e-9, "ambiguous input"
    rc, c_w, cn_w, ang_w, over_w = SU.host_counts(_lib.lib(), pos, types, sizes, A, **kw)
    assert rc == 0 and over_w.sum() == 0 and c_w.sum() > 0 and ang_w.sum() > 0
    for dev in ("cuda:0", "cuda:1"):
        with torch.cuda.device(dev):
            p, oh = torch.from_numpy(pos).to(dev), _onehot(types, A).to(dev)
            c = stats.pair_counts(p, oh, sizes, R=kw["R"], dR=kw["dR"])
            cn, ang = stats.bond_statistics(p, oh, sizes, cutoff=kw["cutoff"], dtheta=kw["dtheta"], max_cn=kw["max_cn"])
        assert np.array_equal(c.cpu().numpy(), c_w), dev
        assert np.array_equal(cn.cpu().numpy(), cn_w) and np.array_equal(ang.cpu().numpy(), ang_w), dev

"""Structural RMSD evaluation on the device (csrc/eval/kabsch.hip through diffusion_model_amd.stats): the three Kabsch
spellings of the reference, evaluate_by_rmsd / evaluate_by_rmsd_and_atom_type_eval of parts/def_for_main.py:73-117 and the
correspondence search of evaluate_rmsd.py:93-107, against the EXECUTED reference stored in tests/golden/rmsd_golden.npz and,
beyond the sizes a CPU loop finishes, against the float64 restatement of tests/_rmsd_util.py.

Bar of every comparison with the reference: 4 x ref_vs_f64, the reference's own float32 noise measured by the generator
(rmsd 6.19e-07, t 6.37e-07, R 6.53e-07 -> bars 2.48e-06, 2.55e-06, 2.61e-06): the device computes in float64 from the same
float32 inputs, so its distance to the float32 reference is the reference's rounding; 4 x covers float32 storage of the outputs
and another SVD route.  R is compared where the singular directions are defined (tests/_rmsd_util.py: well_conditioned), the
column-flip RMSD where the reflection decision is (full_rank); in rank-deficient cases the device returns the optimal proper
rotation for both flips (include/egnn_amd.h).

Measured maxima on an MI355X: the MEASURED table below (also in DESIGN.md); evaluate_by_rmsd 2.68e-07.
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import diffusion_model_amd as dma
from tests import _rmsd_util as RU
from tests import _stats_util as SU
from tests._util import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"

# MEASURED (MI355X, this suite): largest |device - golden| per quantity, bar in brackets
#   kabsch torch           rmsd 4.77e-07 (2.48e-06)  t 4.77e-07 (2.55e-06)  R 5.36e-07 (2.61e-06)
#   kabsch numpy_centroid  rmsd 4.77e-07 (2.48e-06)  t 7.15e-07 (2.55e-06)  R 4.17e-07 (2.61e-06)
#   kabsch numpy_first     rmsd 3.18e-07 (2.48e-06)  t 0        (2.55e-06)  R 6.56e-07 (2.61e-06)
#   search n = 2..8        min_rmsd 3.83e-07 (2.48e-06), 13 of 13 orders equal
#   search n = 9, 10       min_rmsd 1.55e-08 (2.48e-06) against the float64 restatement, orders equal


def _golden():
    G = load_golden("rmsd_golden.npz")
    f = G["ref_vs_f64"]
    return G, {"rmsd": 4 * float(f[0]), "t": 4 * float(f[1]), "R": 4 * float(f[2])}


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _split(a, sizes):
    return np.split(np.asarray(a), np.cumsum(sizes)[:-1])


@pytest.mark.parametrize("name", ["torch", "numpy_centroid", "numpy_first"])
def test_kabsch_matches_executed_reference(name):
    """all 42 golden pairs (n = 2 .. 64, ragged) in ONE launch, per spelling"""
    G, bar = _golden()
    center, flip = RU.SPELLINGS[name]
    sizes = G["kabsch.sizes"].tolist()
    R, t, rmsd = dma.stats.kabsch(_dev(G["kabsch.P"]), _dev(G["kabsch.Q"]), sizes, center=center, flip=flip)
    R, t, rmsd = R.cpu().double().numpy(), t.cpu().double().numpy(), rmsd.cpu().double().numpy()
    sig = G[f"kabsch.sigma_{center}"]
    worst = {"rmsd": 0.0, "t": 0.0, "R": 0.0}
    n_rmsd = n_R = 0
    for k in range(len(sizes)):
        if flip == "row" or RU.full_rank(sig[k]):
            n_rmsd += 1
            worst["rmsd"] = max(worst["rmsd"], abs(rmsd[k] - float(G[f"kabsch.{name}.rmsd"][k])))
        worst["t"] = max(worst["t"], float(np.abs(t[k] - G[f"kabsch.{name}.t"][k]).max()))
        if RU.well_conditioned(sig[k]):
            n_R += 1
            worst["R"] = max(worst["R"], float(np.abs(R[k] - G[f"kabsch.{name}.R"][k]).max()))
    print(f"kabsch {name}: rmsd {worst['rmsd']:.3e} ({n_rmsd} cases, bar {bar['rmsd']:.3e})  t {worst['t']:.3e} (bar {bar['t']:.3e})  "
          f"R {worst['R']:.3e} ({n_R} cases, bar {bar['R']:.3e})")
    assert n_rmsd >= 37 and n_R >= 30    # 5 of the 42 graphs have 2 or 3 atoms
    assert worst["rmsd"] <= bar["rmsd"] and worst["t"] <= bar["t"] and worst["R"] <= bar["R"], worst


def _rigid(Q, seed):
    rng = np.random.default_rng(seed)
    return (Q.double().cpu().numpy() @ RU.random_rotation(rng).T + rng.uniform(-3, 3, 3)).astype(np.float32)


def test_kabsch_properties():
    G, _ = _golden()
    sizes = G["kabsch.sizes"].tolist()
    P, Q = _dev(G["kabsch.P"]), _dev(G["kabsch.Q"])
    eye = torch.eye(3, dtype=torch.float64)
    rm = {}
    for center in ("centroid", "first"):
        for flip in ("row", "column"):
            R, t, rmsd = dma.stats.kabsch(P, Q, sizes, center=center, flip=flip)
            assert bool(torch.isfinite(R).all() and torch.isfinite(t).all() and torch.isfinite(rmsd).all())
            Rd = R.cpu().double()
            assert float((Rd @ Rd.transpose(1, 2) - eye).abs().max()) <= 1e-6
            assert float((torch.linalg.det(Rd) - 1).abs().max()) <= 1e-6
            rm[center, flip] = rmsd.cpu()
            # a batch equals its graphs evaluated one by one, bitwise
            lo = 0
            for k, n in enumerate(sizes):
                R1, t1, r1 = dma.stats.kabsch(P[lo:lo + n], Q[lo:lo + n], center=center, flip=flip)
                assert torch.equal(R1, R[k]) and torch.equal(t1, t[k]) and torch.equal(r1, rmsd[k])
                lo += n
        # the row fix is the optimal proper rotation (1e-6: float32 storage of two O(1) values)
        assert bool((rm[center, "row"] <= rm[center, "column"] + 1e-6).all())
    # invariance under a rigid motion of Q.  The moved coordinates (up to ~16 A) are rounded to float32 again: 2^-24 * 16 = 1e-6
    # per coordinate, and an RMSD with a fixed or optimal rotation is 1-Lipschitz in the RMS displacement: sqrt(3) * 1e-6 +
    # output rounding -> 5e-6.  'row' (the optimal proper rotation): every case, any rigid motion.  'column' in a reflection
    # case is diag(1,1,-1) V U^T, which singles out the z axis of Q's frame: it is invariant under TRANSLATIONS of Q only (the
    # reference's kabsch_torch has the same dependence on the frame), and under any rigid motion where no reflection is taken,
    # i.e. where it equals 'row'.
    lo, moved, shifted = 0, [], []
    for k, n in enumerate(sizes):
        moved.append(_rigid(Q[lo:lo + n], 100 + k))
        shifted.append((Q[lo:lo + n].double().cpu().numpy() + np.random.default_rng(200 + k).uniform(-3, 3, 3)).astype(np.float32))
        lo += n
    r_row = dma.stats.kabsch(P, _dev(np.concatenate(moved)), sizes, center="centroid", flip="row")[2].cpu()
    assert float((r_row - rm["centroid", "row"]).abs().max()) <= 5e-6
    r_col = dma.stats.kabsch(P, _dev(np.concatenate(moved)), sizes, center="centroid", flip="column")[2].cpu()
    unreflected = (rm["centroid", "column"] - rm["centroid", "row"]).abs() <= 1e-6
    assert int(unreflected.sum()) >= 24 and int((~unreflected).sum()) >= 10
    assert float((r_col - rm["centroid", "column"]).abs()[unreflected].max()) <= 5e-6
    # translated Q, reflection cases: the non-optimal RMSD moves in first order with R, and R's singular directions amplify
    # the 1e-6 rounding by at most 1 / WELL_CONDITIONED_GAP = 100: dR ~ 1e-6 * 100 / |p|, times |p| -> 1e-4
    r_col = dma.stats.kabsch(P, _dev(np.concatenate(shifted)), sizes, center="centroid", flip="column")[2].cpu()
    well = torch.from_numpy(np.array([RU.well_conditioned(s) for s in G["kabsch.sigma_centroid"]]))
    diff = (r_col - rm["centroid", "column"]).abs()
    assert float(diff[unreflected].max()) <= 5e-6 and float(diff[~unreflected & well].max()) <= 1e-4
    assert int((~unreflected & well).sum()) >= 8
    # Q = P: the residual must vanish (E0 - 2 sum(sigma) would leave ~1e-3 here)
    for center in ("centroid", "first"):
        for flip in ("row", "column"):
            R, t, rmsd = dma.stats.kabsch(P, P.clone(), sizes, center=center, flip=flip)
            assert float(rmsd.max()) <= 1e-6
    with pytest.raises(RuntimeError):
        dma.stats.kabsch(P.cpu(), Q.cpu(), sizes)


def _eval_lists(G):
    sizes = G["eval.sizes"].tolist()
    ids = G["eval.ids"].tolist()
    originals, generated = [], []
    for k, (po, pg, xo, xg) in enumerate(zip(_split(G["eval.orig_pos"], sizes), _split(G["eval.gen_pos"], sizes),
                                             _split(G["eval.orig_x"], sizes), _split(G["eval.gen_x"], sizes))):
        # the originals are the caller's host records, the samples live on the device as generate() leaves them
        originals.append(SimpleNamespace(pos=torch.from_numpy(po), x=torch.from_numpy(xo), id=ids[k], idx=k))
        generated.append([SimpleNamespace(pos=torch.from_numpy(pg).to(DEV), x=torch.from_numpy(xg).to(DEV))])
    return sizes, originals, generated


def test_evaluate_by_rmsd_matches_executed_reference():
    G, bar = _golden()
    sizes, originals, generated = _eval_lists(G)
    want_idx, want_id, want_rmsd = G["eval.ranked_index"].tolist(), G["eval.ranked_id"].tolist(), G["eval.ranked_rmsd"]
    ranked = dma.stats.evaluate_by_rmsd(originals, generated)
    assert [row[2].idx for row in ranked] == want_idx          # one-atom graph skipped, repeated id kept, stable ties
    assert [row[0] for row in ranked] == want_id
    assert all(torch.is_tensor(row[1]) and row[1].dim() == 0 for row in ranked)
    got = np.array([row[1].item() for row in ranked])
    print(f"evaluate_by_rmsd: max |rmsd - reference| {np.abs(got - want_rmsd).max():.3e} (bar {bar['rmsd']:.3e})")
    assert np.abs(got - want_rmsd).max() <= bar["rmsd"]
    for row in ranked:
        assert row[3] is generated[row[2].idx][-1]
    ranked2 = dma.stats.evaluate_by_rmsd_and_atom_type_eval(originals, generated)
    assert [row[3].idx for row in ranked2] == want_idx
    assert [row[1].item() for row in ranked2] == [row[1].item() for row in ranked]
    for row in ranked2:
        k = row[3].idx
        n = sizes[k]
        xo, xg = originals[k].x, generated[k][-1].x.cpu()
        want = [sum(1 for i in range(n) if xo[i].tolist() == [1, 0]) / n, sum(1 for i in range(n) if xg[i].tolist() == [1, 0]) / n]
        assert row[2] == want                                   # exact
        assert row[4] is generated[k][-1]


def _search_batch(G):
    sizes = G["search.sizes"].tolist()
    return sizes, _dev(G["search.gen"]), _dev(G["search.orig"])


def test_search_matches_executed_reference():
    """n = 2 .. 8: the executed evaluate_rmsd.py loop; all 13 graphs (different n) in one launch"""
    G, bar = _golden()
    sizes, gen, orig = _search_batch(G)
    rmsd, order, R, searched = dma.stats.kabsch_min_over_permutations(gen, orig, sizes, max_atoms=10)
    assert bool(searched.all())
    orders = _split(order.cpu().numpy(), sizes)
    want = _split(G["search.order"], sizes)
    same = [orders[k].tolist() == want[k].tolist() for k in range(len(sizes))]
    err = np.abs(rmsd.cpu().double().numpy() - G["search.min_rmsd"])
    print(f"search n = 2..8: max |min_rmsd - reference| {err.max():.3e} (bar {bar['rmsd']:.3e}), {sum(same)} of {len(same)} orders equal")
    assert all(same)
    assert err.max() <= bar["rmsd"]
    well = np.array([RU.well_conditioned(RU.sigma_f64(g[w], o, "first")) for g, o, w in
                     zip(_split(G["search.gen"], sizes), _split(G["search.orig"], sizes), want)])
    assert np.abs(R.cpu().double().numpy() - G["search.R"])[well].max() <= bar["R"]
    # two runs are bitwise equal
    rmsd2, order2, R2, _ = dma.stats.kabsch_min_over_permutations(gen, orig, sizes, max_atoms=10)
    assert torch.equal(rmsd, rmsd2) and torch.equal(order, order2) and torch.equal(R, R2)


def _search_case(rng, n, noise):
    orig = RU.silica_cloud(rng, n)
    shuffle = np.concatenate([[0], 1 + rng.permutation(n - 1)])
    gen = (orig @ RU.random_rotation(rng).T + rng.uniform(-3, 3, 3) + noise * rng.standard_normal((n, 3)))[shuffle]
    return gen.astype(np.float32), orig.astype(np.float32)


def test_search_nine_and_ten_atoms_match_float64_restatement():
    _, bar = _golden()
    rng = np.random.default_rng(910)
    cases = [_search_case(rng, n, noise) for n, noise in ((9, 0.05), (9, 0.3), (10, 0.05), (10, 0.3))]
    sizes = [c[0].shape[0] for c in cases]
    gen, orig = _dev(np.concatenate([c[0] for c in cases])), _dev(np.concatenate([c[1] for c in cases]))
    rmsd, order, R, searched = dma.stats.kabsch_min_over_permutations(gen, orig, sizes, max_atoms=10)
    assert bool(searched.all())
    rmsd2, order2, R2, _ = dma.stats.kabsch_min_over_permutations(gen, orig, sizes, max_atoms=10)
    assert torch.equal(rmsd, rmsd2) and torch.equal(order, order2) and torch.equal(R, R2)
    orders = _split(order.cpu().numpy(), sizes)
    worst = 0.0
    for k, (g, o) in enumerate(cases):
        best, want, second = RU.search_f64(g, o)
        worst = max(worst, abs(float(rmsd[k]) - best))
        if second - best >= RU.GAP * best:
            assert orders[k].tolist() == want, (k, orders[k].tolist(), want)
        # alone in a launch (another grid) the result is the same, bitwise
        r1, o1, R1, _ = dma.stats.kabsch_min_over_permutations(_dev(g), _dev(o), [sizes[k]], max_atoms=10)
        assert torch.equal(r1[0], rmsd[k]) and o1.cpu().tolist() == orders[k].tolist() and torch.equal(R1[0], R[k])
    print(f"search n = 9, 10: max |min_rmsd - float64 restatement| {worst:.3e} (bar {bar['rmsd']:.3e})")
    assert worst <= bar["rmsd"]


def test_search_exact_tie_returns_first_order():
    """two coincident atoms in the generated structure: two orderings have bitwise equal sums, the lexicographically first
    wins whatever the launch geometry (the reference keeps the first strict minimum)"""
    rng = np.random.default_rng(5)
    for n, (a, b) in ((7, (2, 5)), (10, (3, 8)), (10, (8, 9)), (4, (1, 3))):
        gen, orig = _search_case(rng, n, 0.05)
        gen[b] = gen[a]
        for batch in (1, 3):
            rmsd, order, R, searched = dma.stats.kabsch_min_over_permutations(_dev(np.tile(gen, (batch, 1))), _dev(np.tile(orig, (batch, 1))),
                                                                              [n] * batch, max_atoms=10)
            for got in _split(order.cpu().numpy(), [n] * batch):
                got = got.tolist()
                assert sorted(got) == list(range(n)) and got[0] == 0
                assert got.index(a) < got.index(b), (n, a, b, got)
        if n <= 7:
            assert got == RU.search_f64(gen, orig)[1]


def test_search_mixed_batch_and_unsearched_outputs():
    rng = np.random.default_rng(77)
    sizes = [1, 5, 10, 40]
    cases = [_search_case(rng, n, 0.1) if n > 1 else (np.ones((1, 3), np.float32), np.zeros((1, 3), np.float32)) for n in sizes]
    gen, orig = _dev(np.concatenate([c[0] for c in cases])), _dev(np.concatenate([c[1] for c in cases]))
    N = sum(sizes)
    out = (torch.full((4,), -7.0, device=DEV), torch.full((N,), -3, dtype=torch.int32, device=DEV), torch.full((4, 3, 3), 9.0, device=DEV))
    rmsd, order, R, searched = dma.stats.kabsch_min_over_permutations(gen, orig, sizes, max_atoms=10, out=out)
    assert searched.cpu().tolist() == [False, True, True, False]
    orders = _split(order.cpu().numpy(), sizes)
    for k in (0, 3):   # left as the caller filled them
        assert float(rmsd[k]) == -7.0 and (orders[k] == -3).all() and bool((R[k] == 9.0).all())
    for k in (1, 2):
        best, want, second = RU.search_f64(*cases[k])
        assert abs(float(rmsd[k]) - best) <= _golden()[1]["rmsd"]
        assert orders[k].tolist() == want or second - best < RU.GAP * best
    # the list interface: ids with the reference's occurrence suffix, aligned positions, reordered atom types
    originals = [SimpleNamespace(pos=torch.from_numpy(c[1]), x=torch.eye(2, dtype=torch.long)[torch.arange(n) % 2], id="mp-1")
                 for c, n in zip(cases, sizes)]
    generated = [[SimpleNamespace(pos=torch.from_numpy(c[0]).to(DEV), x=torch.eye(2, dtype=torch.long)[(torch.arange(n) // 2) % 2].to(DEV))]
                 for c, n in zip(cases, sizes)]
    rows = dma.stats.min_rmsd_over_permutations(originals, generated, max_atoms=10)
    assert [r[0] for r in rows] == ["mp-1_2", "mp-1_3"]
    for row, k in zip(rows, (1, 2)):
        n = sizes[k]
        assert row[1] == float(rmsd[k]) and row[2] == orders[k].tolist()
        assert torch.equal(row[4], generated[k][-1].x.cpu()[row[2]])
        q = originals[k].pos - originals[k].pos[0]
        assert abs(math.sqrt(float(((row[3] - q) ** 2).sum()) / n) - row[1]) <= 1e-5


def test_generate_then_evaluate_by_rmsd():
    """end to end: generate() on the small trained model of the statistics tests -> evaluate_by_rmsd"""
    sd, d, L, A, T, s, p = SU.load_stat_model()
    net = dma.EquivariantGNN(L, **d)
    net.load_state_dict(sd)
    params = dict(num_diffusion_timestep=T, conditional=False, atom_type_size=A, onehot_scaling_factor=1.0, to_compress_spectrum=False,
                  give_exO=False, noise_schedule="predefined", seed=11)
    rng = np.random.default_rng(3)
    data = []
    for k, n in enumerate((3, 9, 9, 3)):
        x = torch.eye(2, dtype=torch.long)[torch.tensor([0] + [1, 0] * (n // 2))[:n]]
        data.append(SimpleNamespace(x=x, pos=torch.from_numpy(RU.silica_cloud(rng, n).astype(np.float32)), id=f"mp-{k}"))
    _, gen = dma.generate({"egnn": net}, data, params, dma.E3DiffusionProcess(s, p, T), gen_num_per_spectrum=4)
    assert len(gen) == 4 * len(data)
    originals = [datum for datum in data for _ in range(4)]     # generate()'s order: datum by datum
    ranked = dma.stats.evaluate_by_rmsd(originals, gen)
    assert len(ranked) == 16
    vals = [row[1].item() for row in ranked]
    assert all(math.isfinite(v) and v >= 0 for v in vals) and vals == sorted(vals)
    ranked2 = dma.stats.evaluate_by_rmsd_and_atom_type_eval(originals, gen)
    assert [row[1].item() for row in ranked2] == vals
    assert all(0.0 <= f <= 1.0 for row in ranked2 for f in row[2])

"""Atom matching of large graphs on the device (csrc/eval/assign.hip through diffusion_model_amd.stats.linear_assignment and
align_by_assignment) against the EXECUTED reference (create_xyz.py:157-192) stored in tests/golden/assign_golden.npz, against
scipy's optimum where no fixture exists, and against itself (reproducibility, batch position).

Bars.
  * Assignments: equal to the golden col_ind.  The generator kept only cases whose runner-up costs >= (1 + 1e-5) x the optimum.
  * Optimality, independent of equality: cost of the device assignment, evaluated on the host in float64 from the float32
    coordinates, <= (1 + 1e-6) x scipy's optimum.  Derived, not measured: an entry of either cost matrix (numpy's float32 norm,
    the device's float32 norm, the float64 norm) is within 3 ulp of float32 = 3.6e-7 relative of the true distance, and optimal
    assignments under two matrices that differ by eps per entry differ in cost by at most 2 eps.
  * RMSD, reordered positions and pre-alignment rotation of align_by_assignment: 4 x ref_vs_f64, the reference's own float32
    noise measured by the generator against the float64 restatement (RMSD 1.78e-07 -> 7.1e-07), the bar tests/test_gpu_rmsd.py
    uses.  The rotation is compared where its singular directions are defined (tests/_rmsd_util.py: well_conditioned).
  * Exact ties (integer distances): every dual update is exact, so the cost EQUALS scipy's optimum.
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import diffusion_model_amd as dma
from diffusion_model_amd import _lib
from tests import _assign_util as AU
from tests import _rmsd_util as RU
from tests import _stats_util as SU
from tests._util import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
COST_BAR = 1e-6
MAX_ATOMS = 1024


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _split(a, sizes):
    return np.split(np.asarray(a), np.cumsum(sizes)[:-1])


def _golden():
    G = load_golden("assign_golden.npz")
    sizes = G["sizes"].tolist()
    f = G["ref_vs_f64"]                                   # rmsd, reordered positions, R of the five-point fit
    return G, sizes, {"rmsd": 4 * float(f[0]), "pos": 4 * float(f[1]), "R": 4 * float(f[2])}


def _solve(P, Q, sizes, **kw):
    col, cost, solved = dma.stats.linear_assignment(_dev(np.concatenate(P)), _dev(np.concatenate(Q)), sizes, **kw)
    return col, cost, solved


def test_limits_agree():
    assert _lib.ASSIGN_MAX_ATOMS == MAX_ATOMS >= 512


def test_linear_assignment_matches_executed_reference():
    """all golden cases (n = 6 .. 512, ragged) in ONE launch, on the arrays the reference handed to scipy"""
    G, sizes, _ = _golden()
    P, Q = _split(G["centred"], sizes), _split(G["aligned"], sizes)
    col, cost, solved = _solve(P, Q, sizes)
    assert col.dtype == torch.int32 and cost.dtype == torch.float64 and solved.dtype == torch.bool
    assert bool(solved.all())
    cols, want = _split(col.cpu().numpy(), sizes), _split(G["col_ind"], sizes)
    cost = cost.cpu().numpy()
    worst_opt, worst_cost, same = 0.0, 0.0, 0
    for k, n in enumerate(sizes):
        assert AU.is_permutation(cols[k], n), k
        host = AU.assignment_cost_f64(P[k], Q[k], cols[k])
        worst_opt = max(worst_opt, host / float(G["opt_cost"][k]) - 1.0)
        worst_cost = max(worst_cost, abs(cost[k] - host) / host)
        same += int(np.array_equal(cols[k], want[k]))
    print(f"linear_assignment: {same} of {len(sizes)} assignments equal, host cost / scipy optimum - 1 <= {worst_opt:.3e} "
          f"(bar {COST_BAR:.0e}), |device cost - host cost| / cost <= {worst_cost:.3e}")
    assert worst_opt <= COST_BAR
    assert same == len(sizes)
    assert worst_cost <= COST_BAR      # the device's own float32 norms summed in float64
    # the graphs of up to 64 atoms alone: the one-wavefront launch; one graph alone: another grid.  Bitwise the same.
    small = [k for k, n in enumerate(sizes) if n <= 64]
    col_s, cost_s, solved_s = _solve([P[k] for k in small], [Q[k] for k in small], [sizes[k] for k in small])
    assert bool(solved_s.all())
    for got, k in zip(_split(col_s.cpu().numpy(), [sizes[k] for k in small]), small):
        assert np.array_equal(got, cols[k])
    assert np.array_equal(cost_s.cpu().numpy(), cost[small])
    for k in (0, len(sizes) - 1):
        c1, v1, s1 = _solve([P[k]], [Q[k]], [sizes[k]])
        assert bool(s1[0]) and np.array_equal(c1.cpu().numpy(), cols[k]) and float(v1[0]) == cost[k]


def _lists(G, sizes):
    originals, generated = [], []
    for k, (po, pg, xo, xg) in enumerate(zip(_split(G["orig"], sizes), _split(G["gen"], sizes), _split(G["orig_x"], sizes),
                                             _split(G["gen_x"], sizes))):
        originals.append(SimpleNamespace(pos=torch.from_numpy(po.copy()), x=torch.from_numpy(xo.copy()), id=f"mp-{k // 3}"))
        generated.append([SimpleNamespace(pos=torch.from_numpy(pg.copy()).to(DEV), x=torch.from_numpy(xg.copy()).to(DEV))])
    return originals, generated


def test_align_by_assignment_matches_executed_reference():
    G, sizes, bar = _golden()
    originals, generated = _lists(G, sizes)
    rows = dma.stats.align_by_assignment(originals, generated)
    assert len(rows) == len(sizes)
    assert [r[0] for r in rows] == [f"mp-{k // 3}_{k % 5 + 1}" for k in range(len(sizes))]
    want_col, want_o, want_g = _split(G["col_ind"], sizes), _split(G["orig_reordered"], sizes), _split(G["gen_reordered"], sizes)
    xo, xg = _split(G["orig_x"], sizes), _split(G["gen_x"], sizes)
    worst, worst_pos = 0.0, 0.0
    for k, (id_, rmsd, row_ind, col_ind, po, pg, xor_, xgr) in enumerate(rows):
        n = sizes[k]
        assert isinstance(rmsd, float)
        assert np.array_equal(row_ind, np.arange(n)) and np.array_equal(col_ind, want_col[k]), k
        assert torch.equal(xor_, torch.from_numpy(xo[k])) and torch.equal(xgr, torch.from_numpy(xg[k][want_col[k]]))
        assert xgr.dtype == torch.int64 and not po.is_cuda and not pg.is_cuda
        worst = max(worst, abs(rmsd - float(G["rmsd"][k])))
        worst_pos = max(worst_pos, float(np.abs(po.numpy() - want_o[k]).max()), float(np.abs(pg.numpy() - want_g[k]).max()))
        # the returned RMSD is the atom-0-anchored fit of the returned arrays
        assert abs(RU.kabsch_f64(pg.numpy(), po.numpy(), "first", "row")[2] - rmsd) <= 1e-6
    print(f"align_by_assignment: max |rmsd - reference| {worst:.3e} (bar {bar['rmsd']:.3e}), max |position - reference| "
          f"{worst_pos:.3e} (bar {bar['pos']:.3e})")
    assert worst <= bar["rmsd"]
    assert worst_pos <= bar["pos"]


def test_prealignment_rotation_matches_executed_reference():
    """the rotation of the best of the 24 pairings; compared where its singular directions are defined"""
    G, sizes, bar = _golden()
    po, pg = _dev(G["orig"]), _dev(G["gen"])
    gp, B, _ = dma.stats._graph_ptr(sizes, po.device)
    R = torch.full((B, 9), 7.0, device=DEV)
    flag = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().egnn_assign_prealign(_lib.stream_ptr(), B, _lib.ptr(po), _lib.ptr(pg), _lib.ptr(gp), 6, _lib.ptr(R),
                                               _lib.ptr(flag)))
    assert flag.cpu().tolist() == [1] * B
    R = R.cpu().double().numpy().reshape(B, 3, 3)
    checked = 0
    for k, (o, g) in enumerate(zip(_split(G["orig"], sizes), _split(G["gen"], sizes))):
        R64, perm, fits = AU.prealign_f64(o, g)
        assert perm == int(G["perm"][k])
        assert np.abs(R[k] - R64).max() <= 1e-6          # float32 storage of a float64 fit of the same float32 inputs
        if RU.well_conditioned(RU.sigma_f64(*AU.prealign_points(o, g, perm), "first")):
            checked += 1
            assert np.abs(R[k] - G["R"][k]).max() <= bar["R"], k
    assert checked >= len(sizes) // 2
    # graphs below min_atoms: flag 0, R untouched
    R2 = torch.full((B, 9), 7.0, device=DEV)
    _lib.check(_lib.lib().egnn_assign_prealign(_lib.stream_ptr(), B, _lib.ptr(po), _lib.ptr(pg), _lib.ptr(gp), 8, _lib.ptr(R2),
                                               _lib.ptr(flag)))
    assert flag.cpu().tolist() == [int(n >= 8) for n in sizes]
    assert all(bool((R2[k] == 7.0).all()) for k, n in enumerate(sizes) if n < 8)


def test_prealignment_without_a_finite_fit_is_flagged():
    """an infinite coordinate in one of the four neighbours still orders them (its distance is +inf, the largest), but none of
    the 24 fits has a finite residual: flag 0 and R untouched, as for a graph below min_atoms; the graph beside it is fitted"""
    G, sizes, _ = _golden()
    o, g = _split(G["orig"], sizes)[0], _split(G["gen"], sizes)[0]
    assert sizes[0] == 6
    bad = g[:5].copy()
    bad[3, 1] = np.inf
    po, pg = _dev(np.concatenate([o[:5], o])), _dev(np.concatenate([bad, g]))
    gp, B, _ = dma.stats._graph_ptr([5, 6], po.device)
    R = torch.full((B, 9), 7.0, device=DEV)
    flag = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().egnn_assign_prealign(_lib.stream_ptr(), B, _lib.ptr(po), _lib.ptr(pg), _lib.ptr(gp), 5, _lib.ptr(R),
                                               _lib.ptr(flag)))
    assert flag.cpu().tolist() == [0, 1]
    assert bool((R[0] == 7.0).all())
    assert np.abs(R[1].cpu().double().numpy().reshape(3, 3) - AU.prealign_f64(o, g)[0]).max() <= 1e-6
    # through the public flow the graph is dropped, the other is returned
    x = torch.zeros(5, 2, dtype=torch.long)
    rows = dma.stats.align_by_assignment(
        [SimpleNamespace(pos=torch.from_numpy(o[:5].copy()), x=x, id="a"), SimpleNamespace(pos=torch.from_numpy(o[:5].copy()), x=x, id="a")],
        [[SimpleNamespace(pos=torch.from_numpy(bad).to(DEV), x=x.to(DEV))], [SimpleNamespace(pos=torch.from_numpy(g[:5].copy()).to(DEV), x=x.to(DEV))]],
        min_atoms=5)
    assert [r[0] for r in rows] == ["a_2"] and math.isfinite(rows[0][1])


def _lattice(rng, n, axis):
    P, Q = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    P[:, axis], Q[:, axis] = rng.integers(0, 7, n), rng.integers(0, 7, n)
    return P, Q


def test_exact_ties_are_optimal_and_reproducible():
    """points on an integer lattice along one axis: every distance is a small integer, massively tied.  Integer costs make
    every dual update exact, so the cost equals scipy's optimum exactly"""
    rng = np.random.default_rng(12)
    sizes = [1, 2, 7, 33, 64, 65, 150, 300, 64, 300]
    cases = [_lattice(rng, n, k % 3) for k, n in enumerate(sizes)]
    cases[8], cases[9] = cases[4], cases[7]                 # the same graphs again, at other batch positions
    P, Q = [c[0] for c in cases], [c[1] for c in cases]
    col, cost, solved = _solve(P, Q, sizes)
    assert bool(solved.all())
    cols = _split(col.cpu().numpy(), sizes)
    for k, n in enumerate(sizes):
        assert AU.is_permutation(cols[k], n)
        D = AU.distance_matrix(P[k], Q[k])
        r, c = AU.assign_f64(P[k], Q[k])
        assert D[np.arange(n), cols[k]].sum() == D[r, c].sum() == float(cost[k]), k
        assert np.array_equal(cols[k], AU.sap_lowest_index(D)[0]), k        # the tie rule of csrc/eval/assign.h
    assert np.array_equal(cols[8], cols[4]) and np.array_equal(cols[9], cols[7])
    assert float(cost[8]) == float(cost[4]) and float(cost[9]) == float(cost[7])
    col2, cost2, _ = _solve(P, Q, sizes)
    assert torch.equal(col, col2) and torch.equal(cost, cost2)
    # reversed batch: every graph at another position and, for the small ones, next to other neighbours
    col3, cost3, _ = _solve(P[::-1], Q[::-1], sizes[::-1])
    for got, k in zip(_split(col3.cpu().numpy(), sizes[::-1]), range(len(sizes) - 1, -1, -1)):
        assert np.array_equal(got, cols[k])
    assert torch.equal(cost3.flip(0), cost)


def test_mixed_batch_solved_flags_and_untouched_outputs():
    rng = np.random.default_rng(31)
    sizes = [1, 5, 0, 6, 64, 65, MAX_ATOMS, MAX_ATOMS + 1]
    P = [rng.uniform(-5, 5, (n, 3)).astype(np.float32) for n in sizes]
    Q = [(p + 0.3 * rng.standard_normal(p.shape))[rng.permutation(len(p))].astype(np.float32) for p in P]
    N, B = sum(sizes), len(sizes)
    out = (torch.full((N,), -3, dtype=torch.int32, device=DEV), torch.full((B,), -7.0, dtype=torch.float64, device=DEV))
    col, cost, solved = _solve(P, Q, sizes, out=out)
    assert col is out[0] and cost is out[1]
    assert solved.cpu().tolist() == [True, True, False, True, True, True, True, False]
    cols = _split(col.cpu().numpy(), sizes)
    for k, n in enumerate(sizes):
        if not bool(solved[k]):                             # left as the caller filled them
            assert (cols[k] == -3).all() and float(cost[k]) == -7.0
            continue
        assert AU.is_permutation(cols[k], n)
        r, c = AU.assign_f64(P[k], Q[k])
        opt = AU.distance_matrix(P[k], Q[k])[r, c].sum()
        host = AU.assignment_cost_f64(P[k], Q[k], cols[k])
        assert host <= (1 + COST_BAR) * opt, (k, host, opt)
        assert abs(float(cost[k]) - host) <= COST_BAR * max(host, 1e-30)
    # non-finite coordinates have no optimum: not solved, nothing written, no hang
    bad = P[4].copy()
    bad[3, 1] = np.nan
    col, cost, solved = _solve([bad, P[3]], [Q[4], Q[3]], [64, 6], out=(torch.full((70,), -3, dtype=torch.int32, device=DEV),
                                                                     torch.full((2,), -7.0, dtype=torch.float64, device=DEV)))
    assert solved.cpu().tolist() == [False, True] and bool((col[:64] == -3).all()) and float(cost[0]) == -7.0
    assert np.array_equal(col[64:].cpu().numpy(), cols[3])
    with pytest.raises(RuntimeError):
        dma.stats.linear_assignment(torch.zeros(6, 3), torch.zeros(6, 3), [6])
    with pytest.raises(ValueError):
        dma.stats.linear_assignment(torch.zeros(6, 3, device=DEV), torch.zeros(7, 3, device=DEV), [6])
    with pytest.raises(ValueError):
        dma.stats.linear_assignment(torch.zeros(6, 3, device=DEV), torch.zeros(6, 3, device=DEV), [5])
    with pytest.raises(_lib.EgnnError):
        z = torch.zeros(6, 3, device=DEV)
        _lib.check(_lib.lib().egnn_assign(_lib.stream_ptr(), 1, _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), MAX_ATOMS + 1, _lib.ptr(z),
                                          _lib.ptr(z), _lib.ptr(z)))


def test_noiseless_shuffled_copy_is_recovered():
    """a rotated, translated, shuffled copy without noise: the assignment is the shuffle and the RMSD is float32 rounding of
    coordinates up to ~10 A (6e-7 per coordinate; the bound of tests/test_gpu_rmsd.py's rigid-motion check, 5e-6)"""
    G, gsizes, _ = _golden()
    rng = np.random.default_rng(8)
    clouds = [RU.silica_cloud(rng, n) for n in (6, 17, 64, 130)] + [_split(G["orig"], gsizes)[-1].astype(np.float64)]
    originals, generated, shuffles = [], [], []
    for k, cloud in enumerate(clouds):
        n = cloud.shape[0]
        orig, gen, shuffle = AU.pair_case(rng, n, 0.0, cloud)
        assert min(AU.near_gap(orig), AU.near_gap(gen)) > 1e-4          # the neighbour order is defined
        x = np.eye(2, dtype=np.int64)[np.arange(n) % 2]
        originals.append(SimpleNamespace(pos=torch.from_numpy(orig), x=torch.from_numpy(x), id="mp-7"))
        generated.append([SimpleNamespace(pos=torch.from_numpy(gen).to(DEV), x=torch.from_numpy(x[shuffle]).to(DEV))])
        shuffles.append(shuffle)
    rows = dma.stats.align_by_assignment(originals, generated)
    assert [r[0] for r in rows] == [f"mp-7_{k + 1}" for k in range(5)]
    for k, row in enumerate(rows):
        assert np.array_equal(shuffles[k][row[3]], np.arange(len(shuffles[k]))), k      # gen[col[i]] is atom i of the original
        assert row[1] <= 5e-6, (k, row[1])
        assert torch.equal(row[7], row[6])                                               # so are the atom types


def test_generate_then_align_by_assignment():
    """end to end: generate() on the small trained model of the statistics tests -> align_by_assignment"""
    sd, d, L, A, T, s, p = SU.load_stat_model()
    net = dma.EquivariantGNN(L, **d)
    net.load_state_dict(sd)
    params = dict(num_diffusion_timestep=T, conditional=False, atom_type_size=A, onehot_scaling_factor=1.0, to_compress_spectrum=False,
                  give_exO=False, noise_schedule="predefined", seed=11)
    rng = np.random.default_rng(3)
    data = []
    for k, n in enumerate((3, 9, 12, 6)):
        x = torch.eye(2, dtype=torch.long)[torch.tensor([0] + [1, 0] * (n // 2))[:n]]
        data.append(SimpleNamespace(x=x, pos=torch.from_numpy(RU.silica_cloud(rng, n).astype(np.float32)), id=f"mp-{k}"))
    _, gen = dma.generate({"egnn": net}, data, params, dma.E3DiffusionProcess(s, p, T), gen_num_per_spectrum=4)
    assert len(gen) == 4 * len(data)
    originals = [datum for datum in data for _ in range(4)]     # generate()'s order: datum by datum
    rows = dma.stats.align_by_assignment(originals, gen)
    big = [i for i, o in enumerate(originals) if o.pos.shape[0] >= 6]
    assert len(rows) == len(big) == 12
    assert [r[0] for r in rows] == [f"{originals[i].id}_{i % 5 + 1}" for i in big]
    for row, i in zip(rows, big):
        n = originals[i].pos.shape[0]
        assert math.isfinite(row[1]) and row[1] >= 0 and AU.is_permutation(row[3], n)
        po, pg = row[4].numpy(), row[5].numpy()
        assert np.abs(po - (originals[i].pos - originals[i].pos[0]).numpy()).max() == 0.0
        # the returned order is an optimal assignment of the returned arrays: the identity
        r, c = AU.assign_f64(po, pg)
        assert AU.assignment_cost_f64(po, pg, np.arange(n)) <= (1 + COST_BAR) * AU.distance_matrix(po, pg)[r, c].sum()
        assert abs(RU.kabsch_f64(pg, po, "first", "row")[2] - row[1]) <= 1e-6
        assert torch.equal(row[7], gen[i][-1].x.cpu()[row[3]])
    assert len(dma.stats.evaluate_by_rmsd(originals, gen)) == 16     # the plain ranking is untouched by the new flow

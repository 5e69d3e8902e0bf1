"""The float64 restatement the GPU assignment tests compare against (tests/_assign_util.py) reproduces the EXECUTED reference
stored in tests/golden/assign_golden.npz (made by tests/golden/make_assign_golden.py from create_xyz.py:157-192): the same
pairing of the four neighbours, the same assignment, the RMSD within the reference's own float32 noise `ref_vs_f64`.  The
stored gaps satisfy the generator's three conditions, and the numpy spelling of the device solver (rows in index order, equal
path costs to the lowest column index) finds the same assignments.  No GPU, no kernel: passes with and without the library's
solver; the argument checks of the two new entry points run in the sanitizer build of the host logic."""
import numpy as np

from tests import _assign_util as AU
from tests import _rmsd_util as RU
from tests._util import load_golden
from tests.test_host_asan import _run as run_under_sanitizers


def _split(a, sizes):
    return np.split(np.asarray(a), np.cumsum(sizes)[:-1])


def _cases(G):
    sizes = G["sizes"].tolist()
    parts = {k: _split(G[k], sizes) for k in ("orig", "gen", "centred", "aligned", "orig_reordered", "gen_reordered", "row_ind",
                                              "col_ind", "orig_x", "gen_x")}
    return sizes, [{k: v[i] for k, v in parts.items()} for i in range(len(sizes))]


def test_fixture_covers_wavefront_and_workgroup_sizes():
    G = load_golden("assign_golden.npz")
    sizes = G["sizes"]
    assert len(sizes) >= 40 and sizes.min() == 6
    assert set(range(6, 19)) <= set(sizes.tolist())                 # dense at the small end
    assert {64, 65, 100, 128, 256, 512} <= set(sizes.tolist())      # one wavefront up to 64, a workgroup above
    assert (sizes <= 64).sum() >= 30 and (sizes > 64).sum() >= 5
    # the three noise levels (a redraw may have halved one)
    assert len({round(float(v), 6) for v in G["noise"]}) >= 3 and G["noise"].max() == 0.3 and G["noise"].min() <= 0.02
    for k in ("orig", "gen", "centred", "aligned", "orig_reordered", "gen_reordered"):
        assert G[k].dtype == np.float32 and G[k].shape == (int(sizes.sum()), 3)


def test_stored_gaps_satisfy_the_redraw_conditions():
    G = load_golden("assign_golden.npz")
    near_gap, rmsd_gap, assign_gap = G["gaps"]
    assert (near_gap, rmsd_gap, assign_gap) == (1e-4, RU.GAP, 1e-5)
    sizes, cases = _cases(G)
    for k, c in enumerate(cases):
        assert min(AU.near_gap(c["orig"]), AU.near_gap(c["gen"])) > near_gap, k                      # 1
        assert abs(min(AU.near_gap(c["orig"]), AU.near_gap(c["gen"])) - G["near_gap"][k]) <= 1e-12
        assert G["prealign_second"][k] - G["prealign_best"][k] >= rmsd_gap * G["prealign_best"][k], k  # 2
        assert G["runner_up_cost"][k] >= (1.0 + assign_gap) * G["opt_cost"][k], k                    # 3
        # the stored optimum is the cost of the stored assignment on the float32 matrix scipy was handed
        D = AU.distance_matrix(c["centred"], c["aligned"], np.float32).astype(np.float64)
        assert abs(D[c["row_ind"], c["col_ind"]].sum() - G["opt_cost"][k]) <= 1e-9 * G["opt_cost"][k]
    # the runner-up of a few cases, recomputed (n re-solves each)
    for k in (0, 9, 20, 33):
        c = cases[k]
        D = AU.distance_matrix(c["centred"], c["aligned"], np.float32).astype(np.float64)
        assert abs(AU.runner_up_cost(D, c["col_ind"]) - G["runner_up_cost"][k]) <= 1e-9 * G["opt_cost"][k]


def test_restatement_reproduces_the_executed_reference():
    G = load_golden("assign_golden.npz")
    floor, floor_pos, floor_R = (float(v) for v in G["ref_vs_f64"])
    assert 0.0 < floor < 1e-5 and 0.0 < floor_R < 1e-5
    sizes, cases = _cases(G)
    n_R = 0
    for k, c in enumerate(cases):
        n = sizes[k]
        got = AU.align_f64(c["orig"], c["gen"])
        assert got["perm"] == int(G["perm"][k]), k
        assert np.array_equal(got["row_ind"], c["row_ind"]) and np.array_equal(c["row_ind"], np.arange(n))
        assert np.array_equal(got["col_ind"], c["col_ind"]), k                     # exactly
        assert AU.is_permutation(c["col_ind"], n)
        assert abs(got["rmsd"] - float(G["rmsd"][k])) <= floor * (1 + 1e-6) + 1e-12, k
        # the reference's reordered arrays are its centred / aligned arrays in the stored order
        assert np.array_equal(c["gen_reordered"], c["aligned"][c["col_ind"]]) and np.array_equal(c["orig_reordered"], c["centred"])
        assert np.abs(got["gen_reordered"] - c["gen_reordered"]).max() <= floor_pos * (1 + 1e-6) + 1e-12
        if RU.well_conditioned(RU.sigma_f64(*AU.prealign_points(c["orig"], c["gen"], got["perm"]), "first")):
            n_R += 1
            assert np.abs(got["R"] - G["R"][k]).max() <= floor_R * (1 + 1e-6) + 1e-12
        # scipy on the float32 matrix and on the float64 matrix of the same float32 coordinates agree
        assert np.array_equal(AU.assign_f64(c["centred"], c["aligned"])[1], c["col_ind"])
    assert n_R >= len(sizes) // 2


def test_numpy_spelling_of_the_device_solver_finds_the_same_assignments():
    """unique optima (condition 3): any exact solver returns scipy's assignment, whatever its tie rule"""
    G = load_golden("assign_golden.npz")
    sizes, cases = _cases(G)
    for k, c in enumerate(cases):
        if sizes[k] > 128:
            continue
        D = AU.distance_matrix(c["centred"], c["aligned"], np.float32).astype(np.float64)
        col, u, v = AU.sap_lowest_index(D)
        assert np.array_equal(col, c["col_ind"]), k
        # dual feasibility and complementary slackness, to rounding: the certificate of optimality
        red = D - u[:, None] - v[None, :]
        assert red.min() >= -1e-9 and np.abs(red[np.arange(sizes[k]), col]).max() <= 1e-9
    # exact ties: integer distances, every operation exact -> an optimal cost, a valid permutation
    rng = np.random.default_rng(4)
    for n in (7, 40, 90):
        P = np.zeros((n, 3))
        Q = np.zeros((n, 3))
        P[:, 0], Q[:, 0] = rng.integers(0, 6, n), rng.integers(0, 6, n)
        D = AU.distance_matrix(P, Q)
        col, _, _ = AU.sap_lowest_index(D)
        r, c = AU.assign_f64(P, Q)
        assert AU.is_permutation(col, n) and D[np.arange(n), col].sum() == D[r, c].sum()


def test_argument_checks_of_the_new_entry_points_under_sanitizers():
    run_under_sanitizers("""
        p = C.c_void_p(64)      # never dereferenced by the checks
        assert L.egnn_host_assign_args_check(3, p, p, p, 1024, p, p, p) == OK
        assert L.egnn_host_assign_args_check(3, p, p, p, 1, p, p, p) == OK
        assert L.egnn_host_assign_args_check(3, p, p, p, 1025, p, p, p) == EINVAL
        assert b"max_atoms <= 1024" in L.egnn_last_error()
        assert L.egnn_host_assign_args_check(3, p, p, p, 0, p, p, p) == EINVAL
        assert L.egnn_host_assign_args_check(0, p, p, p, 64, p, p, p) == EINVAL
        for hole in range(6):
            args = [p] * 6
            args[hole] = None
            assert L.egnn_host_assign_args_check(3, args[0], args[1], args[2], 64, args[3], args[4], args[5]) == EINVAL
        assert L.egnn_host_assign_prealign_args_check(3, p, p, p, 6, p, p) == OK
        assert L.egnn_host_assign_prealign_args_check(3, p, p, p, 5, p, p) == OK
        assert L.egnn_host_assign_prealign_args_check(3, p, p, p, 4, p, p) == EINVAL
        assert b"min_atoms >= 5" in L.egnn_last_error()
        assert L.egnn_host_assign_prealign_args_check(0, p, p, p, 6, p, p) == EINVAL
        for hole in range(5):
            args = [p] * 5
            args[hole] = None
            assert L.egnn_host_assign_prealign_args_check(3, args[0], args[1], args[2], 6, args[3], args[4]) == EINVAL
    """)

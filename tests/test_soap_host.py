"""The SOAP entries on the host (egnn_soap_host: csrc/eval/soap_host.cpp over the definitions the kernels compile,
csrc/eval/soap_math.h), without a GPU:

  * the tables of SoapBasis equal the golden file's (tests/golden/soap_golden.npz: mpmath at 60 digits) and do not move at 90;
  * the host statement against the truth at E_host = max |p - p_truth| / max |p_truth|, which must stay below 1e-7 (tables built
    in float64 land between 4e-5 and 2e-2, exact ones near 1e-10: the cap tells a wrong basis from a right one);
  * hand cases (a lone atom, a pair on the z axis), invariances under EXACTLY representable motions (signed axis permutations,
    proper and improper; a translation of positions on a 2^-10 grid) and neighbour permutation within 8 E_host, and exact
    properties: species relabelling, the cut, centre lists, the solid harmonics against scipy.special.sph_harm_y;
  * cosines and nearest spectra against the restatement (tests/_soap_util.py), bitwise where the order is fixed;
  * the basis limits (A = 4, n_max = 16, l_max = 10) and the degenerate bases (l_max = 0, n_max = 1, an odd one) against
    tests/golden/soap_limits_golden.npz; exact ties of the nearest spectra (the lower index first), non-finite rows, and the
    cosines at F, row and pair counts around a wavefront, the 4 x 8 tile and the 4 wavefronts of a workgroup;
  * bad arguments return EGNN_EINVAL, from the host statement and -- before anything is launched -- from the device entries;
  * a stand-alone program runs egnn_soap_host under the address and undefined-behaviour sanitizers.

Every input first passes the gap checks of tests/_soap_util.py.
"""
import ctypes as C

import numpy as np
import pytest

from diffusion_model_amd import _lib
from diffusion_model_amd.soap import SoapBasis, build_tables
from tests import _soap_util as SU
from tests._host_program import build_and_run

EINVAL = -22
CAP = SU.CAP
G = SU.golden()


_tables, _host, e_host = SU.tables, SU.host_on_golden, SU.e_host


# ---- tables -----------------------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def _config(name):
    """-> (the four basis parameters, (parts, flat) of the golden that holds the configuration)"""
    if name in SU.CONFIGS:
        return SU.CONFIGS[name], _tables(name)
    return SU.basis_of(SU.LIMIT_CONFIGS[name]), SU.limit_tables(name)


@pytest.mark.parametrize("name", list(SU.CONFIGS) + list(SU.LIMIT_CONFIGS))
def test_basis_tables_equal_the_golden_within_one_ulp(name):
    cfg, (parts, flat) = _config(name)
    basis = SoapBasis(**cfg)
    assert SoapBasis(**cfg) is basis, "the basis is cached per process"
    assert basis.tables.shape == flat.shape == (_lib.lib().egnn_soap_table_doubles(cfg["n_max"], cfg["l_max"]),)
    for got, want in zip((basis.K, basis.gamma, basis.beta, basis.norm, basis.weight), parts):
        assert got.shape == want.shape and float(_ulps(got, want).max()) <= 1.0
    assert float(_ulps(basis.tables, flat).max()) <= 1.0
    assert basis.neighbour_cut == pytest.approx(SU.neighbour_cut(cfg), rel=1e-15)
    # the overlap matrix is so ill-conditioned that beta has entries above 1e6 which cancel to O(1) coefficients
    if name in ("default", "limit"):
        assert np.abs(basis.beta).max() > 1e6


@pytest.mark.parametrize("name", list(SU.CONFIGS))
def test_tables_rebuilt_at_90_digits_round_to_the_same_float64(name):
    for got, want in zip(build_tables(**SU.CONFIGS[name], digits=90), _tables(name)[0]):
        assert np.array_equal(got, want)


def test_feature_count_and_order():
    L = _lib.lib()
    assert L.egnn_soap_features(2, 15, 10) == 5115 == SU.features(2, 15, 10)
    for A, n, l in ((1, 1, 0), (1, 16, 10), (3, 3, 2), (4, 16, 10), (2, 15, 10)):
        assert L.egnn_soap_features(A, n, l) == SU.features(A, n, l) == SU.feature_index(A, n, l).shape[1]


# ---- host against truth -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SU.CONFIGS))
def test_host_statement_against_the_truth(name):
    E = e_host(name)
    print(f"E_host[{name}] = {E:.3e}")
    assert E <= CAP
    for A in SU.TYPES:
        desc, coeff = _host(name, A)
        truth = G[f"{name}_A{A}_desc"]
        assert desc.shape == truth.shape and SU.descriptor_error(desc, truth) <= E
        if A == 2:
            assert SU.descriptor_error(coeff, G[f"{name}_A2_coeff"]) <= CAP
        # the cosine of every row with the next one: |delta cos| <= 2 (eps_a + eps_b), so 4 E
        rc, cos, _ = SU.host_cosines(_lib.lib(), desc, np.roll(desc, -1, 0), n_pairs=len(desc))
        assert rc == 0 and float(np.abs(cos - G[f"{name}_A{A}_cos"]).max()) <= 4 * max(E, np.finfo(float).eps)
        assert np.array_equal(cos, SU.cosine(desc, np.roll(desc, -1, 0)))                  # the fixed order, bitwise
    # the float64 numpy restatement over the same tables is as good as the host statement
    pos, types, sizes = SU.fixture(2, SU.GOLDEN_GRAPHS[name])
    d2, c2 = SU.descriptors(pos, types, sizes, 2, G[f"{name}_A2_centres"], _tables(name)[0], SU.neighbour_cut(SU.CONFIGS[name]))
    assert SU.descriptor_error(d2, G[f"{name}_A2_desc"]) <= 8 * E and SU.descriptor_error(d2, _host(name, 2)[0]) <= 8 * E


@pytest.mark.parametrize("name", list(SU.LIMIT_CONFIGS))
def test_host_statement_against_the_truth_at_the_limits(name):
    """the basis limits (A = 4, n_max = 16, l_max = 10) and the degenerate bases (l_max = 0, n_max = 1, an odd mid-size one): atom 0
    of the fixture graphs against tests/golden/soap_limits_golden.npz"""
    L, LG, cfg = _lib.lib(), SU.limits_golden(), SU.LIMIT_CONFIGS[name]
    A, n_max, l_max = cfg["A"], cfg["n_max"], cfg["l_max"]
    pos, types, sizes = SU.limit_fixture(name)
    cs, truth = LG[f"{name}_centres"], LG[f"{name}_desc"]
    desc, coeff = SU.host_on_limit(name)
    E = SU.e_host_limit(name)
    F = SU.features(A, n_max, l_max)
    assert L.egnn_soap_features(A, n_max, l_max) == F == SU.feature_index(A, n_max, l_max).shape[1] == truth.shape[1]
    assert L.egnn_soap_table_doubles(n_max, l_max) == SU.limit_tables(name)[1].size == 2 * n_max * (l_max + 1) + (l_max + 1) * n_max ** 2 + (l_max + 1) ** 2 + l_max + 1
    rest, rest_coeff = SU.descriptors(pos, types, sizes, A, cs, SU.limit_tables(name)[0], SU.neighbour_cut(cfg))
    E_rest = SU.descriptor_error(rest, truth)
    print(f"E_host[{name}] = {E:.3e}, the float64 restatement {E_rest:.3e}")
    assert desc.shape == (len(types), F) and E <= CAP and E_rest <= CAP
    if name == "limit":
        assert coeff[cs].shape == LG["limit_coeff"].shape and SU.descriptor_error(coeff[cs], LG["limit_coeff"]) <= CAP
        assert SU.descriptor_error(rest_coeff, LG["limit_coeff"]) <= CAP
    # a lone atom (graph 0): the l = 0 entries of its own species' block and nothing else; every species present in the 17-atom graph
    assert sizes[0] == 1 and np.count_nonzero(desc[0]) == n_max * (n_max + 1) // 2
    z1, z2, _, _, ll = SU.feature_index(A, n_max, l_max)
    assert np.array_equal(desc[0] != 0.0, (z1 == types[0]) & (z2 == types[0]) & (ll == 0))
    assert set(types[cs[3]:cs[3] + 17].tolist()) == set(range(A))
    # the list of centres, and no coefficient output: the same rows, bitwise
    rc, listed, none = SU.host_descriptors(L, pos, types, sizes, A, cs[::-1], cfg, SU.limit_tables(name)[1], coeff=False)
    assert rc == 0 and none is None and np.array_equal(listed, desc[cs[::-1]])


def _describe(name, pos, types, sizes, A, centres, cut=None, flat=None):
    cfg = SU.CONFIGS[name]
    if len(pos) > 1:
        assert SU.gap_ok(pos, sizes, SU.neighbour_cut(cfg) if cut is None else cut)
    rc, desc, coeff = SU.host_descriptors(_lib.lib(), pos, types, sizes, A, centres, cfg, _tables(name)[1] if flat is None else flat, cut=cut)
    assert rc == 0, _lib.lib().egnn_last_error()
    return desc, coeff


@pytest.mark.parametrize("name", list(SU.CONFIGS))
def test_a_lone_atom_has_l0_of_its_own_species_only(name):
    (K, gamma, beta, norm, weight), _ = _tables(name)
    desc, coeff = _describe(name, np.zeros((1, 3), np.float32), [1], [1], 2, [0])
    c = beta[0] @ (K[:, 0] * norm[0])                                                      # d = 0: exp(0) = 1, R_00 = N_00
    z1, z2, n1, n2, ll = SU.feature_index(2, K.shape[0], K.shape[1] - 1)
    want = np.where((z1 == 1) & (z2 == 1) & (ll == 0), weight[0] * c[n1] * c[n2], 0.0)
    assert np.array_equal(desc[0] == 0.0, want == 0.0), "only the (Si, Si) block at l = 0"
    assert SU.descriptor_error(desc[0], want) <= max(8 * e_host(name), 8 * np.finfo(float).eps)
    assert not coeff[0, 0].any() and not coeff[0, 1][:, 1:].any()


def test_two_atoms_on_the_z_axis_have_m0_only():
    pos = np.array([[0, 0, 0], [0, 0, 1.75]], np.float32)
    desc, coeff = _describe("default", pos, [0, 1], [2], 2, [0, 1])
    l_of = np.repeat(np.arange(11), 2 * np.arange(11) + 1)
    m0 = np.arange(121) == l_of * l_of + l_of
    assert not coeff[..., ~m0].any() and np.all(coeff[0, 1][:, m0] != 0.0)
    # seen from the other atom the neighbour is at -z: Y_l0 changes sign with l, the power spectrum of one species does not
    assert np.array_equal(np.sign(coeff[0, 1][0, m0]), np.sign(coeff[1, 0][0, m0]) * (-1.0) ** np.arange(11))


def _grid_fixture(A, graph):
    """graph ``graph`` of the fixture with positions on a 2^-10 grid: signed axis permutations and the translation below are exact"""
    pos, types, sizes = SU.fixture(A)
    lo = int(np.cumsum([0] + sizes)[graph])
    p = (np.round(pos[lo:lo + sizes[graph]].astype(np.float64) * 1024) / 1024).astype(np.float32)
    return p, types[lo:lo + sizes[graph]]


@pytest.mark.parametrize("name,graph", [("default", 3), ("small", 5)])
def test_invariance_under_rotation_reflection_translation_and_permutation(name, graph):
    p, t = _grid_fixture(2, graph)
    n = len(p)
    base, _ = _describe(name, p, t, [n], 2, [0])
    bar = 8 * e_host(name)
    proper = p[:, [1, 2, 0]] * np.array([1, -1, -1], np.float32)                           # det +1
    improper = p[:, [1, 0, 2]]                                                             # det -1
    moved = p + np.array([3.5, -2.25, 0.5], np.float32)
    assert np.array_equal(moved.astype(np.float64) - moved[0].astype(np.float64), p.astype(np.float64) - p[0].astype(np.float64))
    perm = np.concatenate([[0], 1 + np.random.default_rng(3).permutation(n - 1)])
    for q, tq in ((proper, t), (improper, t), (moved, t), (p[perm], t[perm])):
        got, _ = _describe(name, q, tq, [n], 2, [0])
        assert SU.descriptor_error(got, base) <= bar
    # and a rotation is not nothing: the coefficients do change
    assert not np.array_equal(_describe(name, proper, t, [n], 2, [0])[1], _describe(name, p, t, [n], 2, [0])[1])


def test_swapping_the_species_labels_permutes_the_blocks_exactly():
    pos, types, sizes = SU.fixture(2, 4)
    cs = SU.first_centres(sizes)
    a, _ = _describe("small", pos, types, sizes, 2, cs)
    b, _ = _describe("small", pos, 1 - types, sizes, 2, cs)
    z1, z2, n1, n2, ll = SU.feature_index(2, 3, 2)
    key = {tuple(k): f for f, k in enumerate(zip(z1, z2, n1, n2, ll))}
    src = np.array([key[(1 - z2[f], 1 - z1[f], n2[f], n1[f], ll[f])] if z1[f] != z2[f] else key[(1 - z1[f], 1 - z2[f], n1[f], n2[f], ll[f])]
                    for f in range(len(ll))])
    assert np.array_equal(b, a[:, src]) and not np.array_equal(a, b)


def test_solid_harmonics_against_scipy():
    """K = 1, gamma = 0, beta = 1 make the coefficient of a neighbour of another species its R_lm; R_lm / d^l must be the real
    orthonormal spherical harmonics (scipy's complex ones combined: sqrt 2 (-1)^m Re / Im)"""
    from scipy.special import sph_harm_y
    (K, gamma, beta, norm, weight), _ = _tables("default")
    flat = np.concatenate([np.ones(K.size), np.zeros(K.size), np.tile(np.eye(15), (11, 1, 1)).reshape(-1), norm, weight])
    rng = np.random.default_rng(9)
    for _ in range(4):
        d = rng.uniform(-3, 3, 3).astype(np.float32)
        _, coeff = _describe("default", np.stack([np.zeros(3, np.float32), d]), [0, 1], [2], 2, [0], flat=flat)
        x, y, z = d.astype(np.float64)
        r = np.sqrt(x * x + y * y + z * z)
        theta, phi = np.arccos(z / r), np.arctan2(y, x)
        for l in range(11):
            for m in range(-l, l + 1):
                Y = sph_harm_y(l, abs(m), theta, phi)
                want = Y.real if m == 0 else np.sqrt(2) * (-1) ** m * (Y.real if m > 0 else Y.imag)
                assert coeff[0, 1, 0, l * l + l + m] / r ** l == pytest.approx(want, rel=1e-11, abs=1e-13), (l, m)
        assert np.array_equal(coeff[0, 1, 0], SU.solid_harmonics(d.astype(np.float64)[None], 10, norm)[0])   # the restatement, bitwise


def test_the_cut_decides_inside_and_outside():
    cut = SU.neighbour_cut(SU.CONFIGS["small"])
    lone, _ = _describe("small", np.zeros((1, 3), np.float32), [0], [1], 2, [0])
    for scale, inside in ((1 - 1e-6, True), (1 + 1e-6, False)):
        pos = np.array([[0, 0, 0], [cut * scale, 0, 0]], np.float32)
        got, _ = _describe("small", pos, [0, 1], [2], 2, [0])
        assert np.array_equal(got, lone) != inside
    # a caller's own cut: the second atom at 2.0 leaves with a cut of 1.9
    pos = np.array([[0, 0, 0], [0, 2.0, 0]], np.float32)
    assert np.array_equal(_describe("small", pos, [0, 1], [2], 2, [0], cut=1.9)[0], lone)
    assert not np.array_equal(_describe("small", pos, [0, 1], [2], 2, [0], cut=2.1)[0], lone)


def test_centre_lists_with_repeats_and_reversed_order():
    pos, types, sizes = SU.fixture(3)
    every, _ = _describe("small", pos, types, sizes, 3, np.arange(len(types)))
    assert np.array_equal(every, _host("small", 3)[0])
    cs = np.array([len(types) - 1, 7, 7, 0, 150, 7, 3], np.int32)
    assert np.array_equal(_describe("small", pos, types, sizes, 3, cs)[0], every[cs])
    assert np.array_equal(_describe("small", pos, types, sizes, 3, np.arange(len(types))[::-1])[0], every[::-1])


# ---- cosines and nearest spectra ----------------------------------------------------------------------------------------------------
def test_cosines_hand_values_and_the_matrix():
    L = _lib.lib()
    a = np.array([[1.0, 0.0], [1.0, 1.0], [3.0, 4.0], [2.0, 0.0]])
    b = np.array([[0.0, 1.0], [1.0, 0.0], [4.0, 3.0], [5.0, 0.0]])
    rc, cos, gram = SU.host_cosines(L, a, b, n_pairs=4, gram=True)
    assert rc == 0 and cos[0] == 0.0 and cos[1] == pytest.approx(1 / np.sqrt(2), rel=1e-15) and cos[2] == pytest.approx(0.96, rel=1e-15)
    assert cos[3] == 1.0 and np.array_equal(np.diag(gram), cos)
    desc = _host("small", 3)[0]
    bar = 4 * max(e_host("small"), np.finfo(float).eps)
    rc, cos, gram = SU.host_cosines(L, desc[:70], desc[100:133], pairs=[[0, 0], [69, 32], [5, 7]], gram=True)
    assert rc == 0 and np.array_equal(cos, gram[[0, 69, 5], [0, 32, 7]])
    assert np.array_equal(gram, SU.cosine_matrix(desc[:70], desc[100:133]))                 # the fixed order, bitwise
    rc, one, _ = SU.host_cosines(L, desc, desc, n_pairs=len(desc))
    assert rc == 0 and float(np.abs(one - 1.0).max()) <= bar
    assert -1.0 <= gram.min() and gram.max() <= 1.0 and gram.std() > 0.01


@pytest.mark.parametrize("S", [200, 7])
def test_nearest_spectra_against_the_restatement(S):
    L = _lib.lib()
    t, r = SU.spectra(40 + S, 5, 70, S)
    tg, rg = np.array([0, 1, -1, 2, 70], np.int32), (np.arange(70) % 3).astype(np.int32)
    for groups in ((None, None), (tg, rg)):
        for k in (1, 3, 8):
            idx, mse, m = SU.nearest(t, r, k, *groups)
            assert SU.mse_gap_ok(m)
            rc, gi, gm = SU.host_nearest(L, t, r, k, *groups)
            assert rc == 0 and np.array_equal(gi, idx) and np.array_equal(gm, mse)          # indices exactly, mse bitwise
            assert np.all(np.diff(gm, axis=1) >= 0)
    gi = SU.host_nearest(L, t, r, 8, tg, rg)[1]
    assert not np.any(rg[gi[0]] == 0) and not np.any(rg[gi[1]] == 1) and np.any(rg[gi[2]] == 0)
    # ties go to the lower index; k above the candidates; nothing left after the exclusion
    rc, gi, gm = SU.host_nearest(L, t[:1], np.concatenate([r[3:4], r[:3], r[3:4]]), 8)
    first = int(gi[0].tolist().index(0))
    assert rc == 0 and gi[0, first + 1] == 4 and gm[0, first] == gm[0, first + 1] and gi[0, 5:].tolist() == [-1] * 3 and np.isinf(gm[0, 5:]).all()
    rc, gi, gm = SU.host_nearest(L, t, r, 3, np.zeros(5, np.int32), np.zeros(70, np.int32))
    assert rc == 0 and (gi == -1).all() and np.isinf(gm).all()


def test_nearest_spectra_with_exact_ties_go_to_the_lower_index():
    """the one rule without a numerical symptom: rows 3, 17, 18, 40 of the references are one row, rows 5, 6 another"""
    L = _lib.lib()
    t, r = SU.tie_spectra()
    tg, rg = np.array([0, 1, -1, 2, 70], np.int32), (np.arange(70) % 3).astype(np.int32)   # rows 3, 18 in group 0: excluded for target 0
    straddles = []
    for groups in ((None, None), (tg, rg)):
        for k in range(1, 9):
            idx, mse, m = SU.nearest(t, r, k, *groups)
            assert SU.mse_gap_ok_with_ties(m) and not SU.mse_gap_ok(m)
            for rows in (SU.TIE_ROWS, SU.TIE_PAIR):                                         # the tie is really there, bitwise
                assert all(len({m[q, j].tobytes() for j in rows if np.isfinite(m[q, j])}) <= 1 for q in range(5))
            rc, gi, gm = SU.host_nearest(L, t, r, k, *groups)
            assert rc == 0 and np.array_equal(gi, idx) and np.array_equal(gm.view(np.int64), mse.view(np.int64))
            order = np.argsort(m, axis=1, kind="stable")
            if k < 70:
                straddles += [(groups[0] is not None, k, q) for q in range(5) if m[q, order[q, k - 1]] == m[q, order[q, k]] and np.isfinite(m[q, order[q, k]])]
    assert straddles, "no tie straddles a k-th place"
    idx, _, m = SU.nearest(t, r, 8)
    assert m[0, 17].tobytes() == m[0, 18].tobytes() and idx[0, :4].tolist() == [3, 17, 18, 40] and idx[1, :2].tolist() == [5, 6]
    assert SU.nearest(t, r, 8, tg, rg)[0][0, :2].tolist() == [17, 40]                       # 3 and 18 share target 0's group


def test_nearest_spectra_at_the_wavefront_and_workgroup_edges_and_non_finite_rows():
    L = _lib.lib()
    for S in (1, 63, 64, 65):
        for T in (1, 3, 4, 5):
            for R in (1, 2, 9):
                t, r = SU.spectra(1000 * S + 10 * T + R, T, R, S)
                idx, mse, m = SU.nearest(t, r, 8)
                assert SU.mse_gap_ok(m)
                rc, gi, gm = SU.host_nearest(L, t, r, 8)
                assert rc == 0 and np.array_equal(gi, idx) and np.array_equal(gm.view(np.int64), mse.view(np.int64))
                assert (gi[:, min(R, 8):] == -1).all() and (gi[:, :min(R, 8)] >= 0).all()
    t, r = SU.nonfinite_spectra()
    for k in (1, 8):
        with np.errstate(invalid="ignore"):
            idx, mse, m = SU.nearest(t, r, k)
        assert SU.mse_gap_ok(m)
        rc, gi, gm = SU.host_nearest(L, t, r, k)
        assert rc == 0 and np.array_equal(gi, idx) and np.array_equal(gm.view(np.int64), mse.view(np.int64))
        assert not np.isin(gi, (2, 7)).any() and (gi[1] == -1).all() and np.isposinf(gm[1]).all()
        assert (gi[[0, 2, 3]] >= 0).all() and np.isfinite(gm[[0, 2, 3]]).all()


@pytest.mark.parametrize("F", SU.COSINE_F)
def test_cosines_at_the_row_pair_and_column_edges(F):
    """F around the 64 lanes of a row sum, row counts around the 4 x 8 tile of the matrix, pair counts around the 4 wavefronts of a
    workgroup; entries of magnitude 1e-8 .. 1e3"""
    L = _lib.lib()
    eps = np.finfo(float).eps
    for rows_a, rows_b in SU.COSINE_SHAPES:
        a, b = SU.cosine_rows(F, rows_a, F), SU.cosine_rows(F + 1000, rows_b, F)
        want = SU.cosine_matrix(a, b)
        rc, _, gram = SU.host_cosines(L, a, b, gram=True)
        assert rc == 0 and float(np.abs(gram - want).max()) <= 4 * eps
        for P in (1, 3, 4, 5):
            pairs = SU.cosine_pairs(P, rows_a, rows_b)
            rc, cos, _ = SU.host_cosines(L, a, b, pairs=pairs)
            assert rc == 0 and float(np.abs(cos - SU.cosine(a[pairs[:, 0]], b[pairs[:, 1]])).max()) <= 4 * eps
            assert np.array_equal(cos.view(np.int64), gram[pairs[:, 0], pairs[:, 1]].view(np.int64))       # one order: bitwise
        if rows_a >= 3:
            a[1] = 0.0                                                                     # a zero row: NaN in its row, nowhere else
            rc, _, gram = SU.host_cosines(L, a, b, gram=True)
            with np.errstate(invalid="ignore"):
                want = SU.cosine_matrix(a, b)
            assert rc == 0 and np.array_equal(np.isnan(gram), np.isnan(want)) and np.isnan(gram[1]).all() and np.isnan(gram).sum() == rows_b
            rc, _, gram = SU.host_cosines(L, b, a, gram=True)                              # ... and in its column
            assert rc == 0 and np.isnan(gram[:, 1]).all() and np.isnan(gram).sum() == rows_b


def test_row_sums_bitwise_through_unit_rows():
    """cosine(a, e) with e = (1, 0, .., 0) scaled by 4 has norm_b exactly 16 and dot exactly 4 a_0, so cos = 4 a_0 / (sqrt(sum a^2) * 4):
    the host statement's squared norm is the restatement's bitwise exactly when these quotients are"""
    L = _lib.lib()
    for F in SU.COSINE_F:
        a = SU.cosine_rows(7 * F, 9, F)
        e = np.zeros((1, F))
        e[0, 0] = 4.0
        rc, _, gram = SU.host_cosines(L, a, e, gram=True)
        want = (4.0 * a[:, 0]) / (np.sqrt(SU.row_sum(a * a)) * 4.0)
        assert rc == 0 and np.array_equal(gram[:, 0].view(np.int64), want.view(np.int64))


def test_empty_graphs_first_in_the_middle_and_last():
    pos, types, sizes = SU.fixture(3, 4)
    want, _ = _describe("small", pos, types, sizes, 3, np.arange(len(types)))
    holes = [0, 1, 2, 0, 0, 5, 17, 0]
    got, _ = _describe("small", pos, types, holes, 3, np.arange(len(types)))
    assert np.array_equal(got, want)


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_einval():
    L = _lib.lib()
    cfg, flat = SU.CONFIGS["small"], _tables("small")[1]
    pos, types, sizes = SU.fixture(2, 4)
    N = len(types)

    def err(**kw):
        c = dict(cfg, **{k: kw[k] for k in ("n_max", "l_max") if k in kw})
        rc = SU.host_descriptors(L, kw.get("pos", pos), kw.get("types", types), kw.get("sizes", sizes), kw.get("A", 2),
                                 kw.get("centres", [0, 3]), c, flat, cut=kw.get("cut"))[0]
        return rc, L.egnn_last_error()
    assert err()[0] == 0
    for kw, word in ((dict(A=5), b"5 atom types"), (dict(A=0), b"0 atom types"), (dict(n_max=0), b"n_max 0"), (dict(n_max=17), b"n_max 17"),
                     (dict(l_max=-1), b"l_max -1"), (dict(l_max=11), b"l_max 11"), (dict(cut=0.0), b"neighbour_cut"), (dict(cut=-1.0), b"neighbour_cut"),
                     (dict(cut=np.inf), b"neighbour_cut"), (dict(cut=np.nan), b"neighbour_cut"), (dict(centres=[0, N]), b"outside [0,"),
                     (dict(centres=[-1]), b"is atom -1"), (dict(types=np.full(N, 2, np.int32)), b"has type 2"),
                     (dict(types=np.full(N, -1, np.int32)), b"has type -1"), (dict(sizes=[1, 2, 5, 16]), b"graph_ptr")):
        rc, msg = err(**kw)
        assert rc == EINVAL and word in msg, (kw.keys(), msg)
    vp, p = SU.vp, C.c_void_p(64)
    gp, cs = SU.graph_ptr(sizes), np.array([0, 3], np.int32)
    desc = np.zeros((2, SU.features(2, 3, 2)))
    full = [4, N, 2, vp(pos), vp(types), vp(gp), 3, 2, 4.37, vp(flat), 2, vp(cs), vp(desc), None] + [0, None, 0, None, 0, 0, None, None, None] + \
           [0, 0, 0, 0] + [None] * 6
    assert L.egnn_soap_host(*full) == 0
    for k in (3, 4, 5, 9, 11, 12):                                                     # a required pointer missing
        args = list(full)
        args[k] = None
        assert L.egnn_soap_host(*args) == EINVAL and b"bad egnn_soap_host arguments" in L.egnn_last_error(), k
    a = np.ones((3, 4))
    assert SU.host_cosines(L, a, a, pairs=[[0, 3]])[0] == EINVAL and b"names a row" in L.egnn_last_error()
    assert SU.host_cosines(L, a, a, n_pairs=4)[0] == EINVAL
    t, r = SU.spectra(1, 2, 5, 7)
    for k in (0, 9, -1):
        assert SU.host_nearest(L, t, r, k)[0] == EINVAL and b"(1 <= k <= 8)" in L.egnn_last_error()
    assert L.egnn_soap_features(5, 3, 2) == EINVAL and L.egnn_soap_features(2, 17, 2) == EINVAL and L.egnn_soap_features(2, 3, 11) == EINVAL
    assert L.egnn_soap_table_doubles(0, 2) == EINVAL

    # the device entries refuse the same arguments before they launch anything (no GPU is touched here)
    good = np.array([0, 7], np.int32)
    d = lambda B=1, N=8, A=2, pos=p, type=p, gp=p, n=3, l=2, cut=4.37, tab=p, nc=2, c=vp(good), dc=p, desc=p: \
        L.egnn_soap_descriptor(None, B, N, A, pos, type, gp, n, l, cut, tab, nc, c, dc, desc, None)
    for call, word in ((lambda: d(A=5), b"5 atom types"), (lambda: d(n=0), b"n_max 0"), (lambda: d(n=17), b"n_max 17"), (lambda: d(l=-1), b"l_max -1"),
                       (lambda: d(l=11), b"l_max 11"), (lambda: d(cut=0.0), b"neighbour_cut"), (lambda: d(cut=float("nan")), b"neighbour_cut"),
                       (lambda: d(cut=float("inf")), b"neighbour_cut"), (lambda: d(N=7), b"centre 1 is atom 7"),
                       (lambda: d(c=vp(np.array([-2, 0], np.int32))), b"is atom -2"), (lambda: d(pos=None), b"bad egnn_soap_descriptor"),
                       (lambda: d(type=None), b"bad egnn_soap_descriptor"), (lambda: d(gp=None), b"bad egnn_soap_descriptor"),
                       (lambda: d(tab=None), b"bad egnn_soap_descriptor"), (lambda: d(c=None), b"bad egnn_soap_descriptor"),
                       (lambda: d(desc=None), b"bad egnn_soap_descriptor"), (lambda: d(dc=None), b"d_centres given"),
                       (lambda: d(B=0), b"bad egnn_soap_descriptor"), (lambda: d(nc=0), b"bad egnn_soap_descriptor")):
        assert call() == EINVAL and word in L.egnn_last_error(), (word, L.egnn_last_error())
    for args in ((0, 5, p, 1, p, 1, None, p), (1, 0, p, 1, p, 1, None, p), (1, 5, None, 1, p, 1, None, p), (1, 5, p, 0, p, 1, None, p),
                 (1, 5, p, 1, None, 1, None, p), (1, 5, p, 1, p, 0, None, p), (1, 5, p, 1, p, 1, None, None)):
        assert L.egnn_soap_cosine(None, *args) == EINVAL and b"bad egnn_soap_cosine" in L.egnn_last_error(), args
    for args in ((0, p, 1, p, 1, p, p), (5, None, 1, p, 1, p, p), (5, p, 0, p, 1, p, p), (5, p, 1, None, 1, p, p), (5, p, 1, p, 0, p, p),
                 (5, p, 1, p, 1, None, p), (5, p, 1, p, 1, p, None)):
        assert L.egnn_soap_gram(None, *args) == EINVAL and b"bad egnn_soap_gram" in L.egnn_last_error(), args
    for args, word in (((0, 5, 7, 3, p, p, None, None, p, p), b"bad egnn_spectrum_nearest"), ((2, 0, 7, 3, p, p, None, None, p, p), b"bad egnn_spectrum_nearest"),
                       ((2, 5, 0, 3, p, p, None, None, p, p), b"bad egnn_spectrum_nearest"), ((2, 5, 7, 0, p, p, None, None, p, p), b"k 0"),
                       ((2, 5, 7, 9, p, p, None, None, p, p), b"k 9"), ((2, 5, 7, 3, None, p, None, None, p, p), b"bad egnn_spectrum_nearest"),
                       ((2, 5, 7, 3, p, None, None, None, p, p), b"bad egnn_spectrum_nearest"), ((2, 5, 7, 3, p, p, None, None, None, p), b"bad egnn_spectrum_nearest"),
                       ((2, 5, 7, 3, p, p, None, None, p, None), b"bad egnn_spectrum_nearest")):
        assert L.egnn_spectrum_nearest(None, *args) == EINVAL and word in L.egnn_last_error(), (args, L.egnn_last_error())


# ---- sanitizers ---------------------------------------------------------------------------------------------------------------------
def test_soap_host_under_sanitizers(tmp_path):
    """the executable links its own sanitizer runtime (statically), so nothing is preloaded"""
    r = build_and_run(tmp_path, "soap_main", ["eval/soap_host.cpp", "host_logic.cpp"])
    assert r.returncode == 0 and "SOAP-OK" in r.stdout, f"rc={r.returncode}\nstdout:\n{r.stdout}\nstderr:\n{r.stderr[-4000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]

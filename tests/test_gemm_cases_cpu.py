"""The case tables of tests/_gemm_cases.py (no GPU): they reach every edge of the ring pipelines they were written for, every case
satisfies the exactness condition, and the restatements (split-K plan, workgroup order, fragment layout) are sound.  The plan
features are asserted on the plans the HOST CODE printed (tests/host/gemm_plan_main.cpp) and on the Python restatement alike."""
import pytest
import torch

from tests import _gemm_cases as GC
from tests.test_gemm_plan_host import host_plans


def _plans():
    """[(case, restated plan)], after checking that the host code plans every case the same way"""
    host = host_plans()
    out = []
    for c in GC.TN_CASES:
        p = GC.plan_gemm_tn(c.E, c.M, c.N)
        assert host[(c.E, c.M, c.N)] == (p.BN, p.tiles_n, p.S, p.steps_per_slice), c
        out.append((c, p))
    return out


def test_gemm_tn_cases_reach_the_ring_and_slice_edges():
    plans = _plans()
    # every step count 1 .. 7 in a single slice, for both tile widths: below, at and above the ring depths 6 / 5 and the
    # NBUF - 1 steps the prologue issues
    for BN, nbuf in ((128, 6), (256, 5)):
        single = {p.last_steps for _, p in plans if p.BN == BN and p.S == 1}
        assert p_nbuf(plans, BN) == nbuf
        assert set(range(1, 8)) <= single, (BN, single)
    assert any(c.E < 32 for c, _ in plans) and any(c.E == 32 for c, _ in plans)          # fewer rows than a step / exactly one
    assert any(c.E % 32 not in (0, 1) and p.total_steps > 1 for c, p in plans)           # a ragged last step
    # split-K: a last slice of ONE step and of two steps behind full slices, for both tile widths where the issue names them
    assert {p.BN for _, p in plans if p.S == 17 and p.last_steps == 1} == {128, 256}
    assert any(p.S > 1 and p.last_steps == 2 and p.tiles_n > 1 and p.ntiles > p.tiles_n for _, p in plans)   # tiles both ways
    assert any(p.S == 2 and p.ntiles == 9 and p.BN == 128 for _, p in plans)
    assert any(p.ntiles == 16 and p.BN == 256 and p.S == p.total_steps // 16 for _, p in plans)   # slices limited by 16 steps each
    # grid remainders of the XCD order
    mods = {p.grid_mod8 for _, p in plans}
    assert len(mods) >= 5 and {6, 7} <= mods, mods
    # strides equal to the width and wider; real widths equal to the padded width and smaller
    assert {c.lda - c.M for c, _ in plans} == {0, 8} and {c.ldb - c.N for c, _ in plans} == {0, 8}
    assert any(c.rows == c.M for c, _ in plans) and any(c.rows < c.M for c, _ in plans)
    assert any(c.cols == c.N for c, _ in plans) and any(c.cols < c.N for c, _ in plans)
    assert any((c.rows, c.M) == (292, 512) for c, _ in plans) and any((c.cols, c.N) == (74, 128) for c, _ in plans)
    assert max(c.E for c, _ in plans) == 11999                                          # tests stay quick
    assert len(set(GC.TN_CASES)) == len(GC.TN_CASES)


def p_nbuf(plans, BN):
    (n,) = {p.nbuf for _, p in plans if p.BN == BN}
    return n


def test_the_issue_table_of_gemm_tn_features():
    """the table the cases were chosen from, feature by feature, on the restated plan"""
    P = GC.plan_gemm_tn
    for E, M, N in ((1, 256, 128), (31, 256, 128), (32, 256, 256)):
        assert P(E, M, N).total_steps == 1 and P(E, M, N).S == 1
    for M, N in ((256, 128), (256, 256)):
        assert [P(E, M, N).total_steps for E in (33, 96, 128, 160, 161, 199, 224)] == [2, 3, 4, 5, 6, 7, 7]
    for M, N in ((256, 128), (256, 256), (512, 384)):
        p = P(8705, M, N)
        assert (p.S, p.steps_per_slice, p.last_steps) == (17, 17, 1)
    assert P(8705, 512, 384).grid_mod8 == 6
    p = P(8737, 512, 512)
    assert (p.S, p.last_steps, p.tiles_n, p.ntiles) == (17, 2, 2, 4)
    assert P(11999, 256, 128).grid_mod8 == 7 and P(11999, 256, 128).last_steps == 1
    p = P(1061, 768, 384)
    assert (p.S, p.ntiles, p.BN) == (2, 9, 128)
    p = P(3000, 1024, 1024)
    assert (p.ntiles, p.BN, p.S, p.total_steps) == (16, 256, 5, 94)
    have = {(c.E, c.M, c.N) for c in GC.TN_CASES}
    want = {(1, 256, 128), (31, 256, 128), (32, 256, 256), (8705, 256, 128), (8705, 256, 256), (8705, 512, 384), (8737, 512, 512),
            (11999, 256, 128), (1061, 768, 384), (3000, 1024, 1024)}
    want |= {(E, 256, N) for E in (33, 96, 128, 160, 161, 199, 224) for N in (128, 256)}
    assert have == want


def test_workgroup_order_is_a_permutation_for_every_grid():
    """xcd_tile maps the workgroups of a grid ONE to one onto the (slice, tile) positions: no slab tile is left unwritten or
    written twice, for the grids of the cases and for every small grid"""
    for nwg in sorted({p.grid for _, p in _plans()} | set(range(1, 130))):
        assert sorted(GC.xcd_tile(b, nwg) for b in range(nwg)) == list(range(nwg)), nwg


def test_gemm_rows_and_split_cases_reach_their_edges():
    C = GC.ROWS_CASES
    assert {c.E for c in C} == set(GC.ROWS_E)
    assert {(c.K0, c.K1) for c in C if c.E == 257} == set(GC.ROWS_K) == {(c.K0, c.K1) for c in C}
    assert {1, 2, 3} <= {(c.K0 + c.K1) // 64 for c in C}                       # shorter than, equal to, the ring of 3 ...
    assert any((c.K0 + c.K1) // 64 > 3 for c in C)                             # ... and longer
    assert {c.ncols for c in C} == set(GC.ROWS_NCOLS) and {GC.chunks_of(c.ncols) for c in C} == {1, 2, 3}
    assert {c.f32 for c in C} == {False, True} and {c.ldo_extra for c in C} == {0, 8}
    for f32 in (False, True):                                                  # both outputs at both strides
        assert {c.ldo_extra for c in C if c.f32 == f32} == {0, 8}
    assert sum(c.view for c in C) == 1
    for c in C:
        lda0, lda1, ldo = GC.rows_strides(c)
        assert lda0 > c.K0 and lda0 % 8 == 0 and ldo % 8 == 0
        if c.K1 and not c.view:
            assert lda1 > c.K1 and lda1 % 8 == 0 and lda1 != lda0
    # E on both sides of a wave's 32 rows and of a workgroup's 256 rows, and exactly at them
    E = set(GC.ROWS_E) | set(GC.SPLIT_E) | {c.E for c in GC.TN_CASES}
    assert min(E) == 1 and {31, 33, 255, 256, 257} <= E
    assert set(GC.SPLIT_E) == {1, 33, 257}
    for a, b in GC.SPLIT_TN:
        assert a % 256 and b % 128
    for k, n in GC.SPLIT_NN:
        assert k % 64 and n % 128
    assert set(GC.PACK_CASES) == {(K, n) for K in (64, 192) for n in (1, 74, 128, 130)}


@pytest.mark.parametrize("case", GC.TN_CASES, ids=lambda c: f"E{c.E}-{c.M}x{c.N}")
def test_gemm_tn_case_is_exact_in_fp32(case):
    a, b, want = GC.tn_operands(case)
    assert a.shape == (case.E, case.rows) and b.shape == (case.E, case.cols) and want.shape == (case.rows, case.cols)
    assert int(a.abs().max()) <= 4 and int(b.abs().max()) <= 4
    assert 16 * case.E + 6 < GC.LIMIT and int(want.abs().max()) + 6 < GC.LIMIT         # any order of partial sums; 3 - v / 2
    assert torch.equal(want.float().long(), want)                                     # fp32 holds the result
    assert torch.equal((3.0 - 0.5 * want.float()).double(), 3.0 - 0.5 * want.double())
    assert torch.equal(a.to(torch.bfloat16).long(), a)                                # bf16 holds the operands


@pytest.mark.parametrize("case", GC.ROWS_CASES, ids=lambda c: f"E{c.E}-K{c.K0}+{c.K1}-n{c.ncols}-{'f32' if c.f32 else 'bf16'}")
def test_gemm_rows_case_is_exact_in_fp32(case):
    a0, w0, a1, w1, want = GC.rows_operands(case)
    assert want.shape == (case.E, case.ncols) and (a1 is None) == (case.K1 == 0)
    assert 16 * (case.K0 + case.K1) + 6 < GC.LIMIT and int(want.abs().max()) < GC.LIMIT
    assert torch.equal(want.float().long(), want)
    r = GC.to_bf16_rne(want)      # one rounding to 8 significant bits: half a unit in the last place is <= 2^-8 of the value
    assert bool(((r.double() - want.double()).abs() <= want.double().abs() * 2.0 ** -8).all())

def test_split_cases_are_exact():
    """integer fp32 inputs of the split products: the bf16 head is the value, the remainder zero, and the sums stay below 2^24"""
    for E in GC.SPLIT_E:
        for x, y in GC.SPLIT_TN + GC.SPLIT_NN:
            GC.assert_terms_bound(max(E, x))
    a = GC.int_matrix(33, 36, 1).float()
    assert torch.equal(a.to(torch.bfloat16).float(), a)


@pytest.mark.parametrize("K,ncols", GC.PACK_CASES)
def test_pack_layout_restatement(K, ncols):
    """the vectorised restatement of the fragment layout against the scalar formula of the kernel's comment, element by element,
    with NaN beyond ncols in the source: padding fragments are exactly zero and nothing beyond ncols is read"""
    ldw = ncols + 5
    w = torch.full((K, ldw), float("nan"))
    w[:, :ncols] = torch.randn(K, ncols, generator=torch.Generator().manual_seed(K + ncols))
    got = GC.pack_rows_layout(w, ncols)
    assert got.dtype == torch.bfloat16 and got.numel() == GC.chunks_of(ncols) * K * 128 and not bool(got.isnan().any())
    idx = torch.randperm(got.numel(), generator=torch.Generator().manual_seed(1))[:4000].tolist() + [0, got.numel() - 1]
    for i in idx:
        assert float(got[i]) == GC.pack_rows_element(w, ncols, i), i
    # every source element of the real columns appears exactly once, everything else is zero
    assert int((got != 0).sum()) == int((w[:, :ncols].to(torch.bfloat16) != 0).sum())
    assert torch.equal(got.float().sort().values, torch.cat([w[:, :ncols].to(torch.bfloat16).float().reshape(-1),
                                                             torch.zeros(got.numel() - K * ncols)]).sort().values)


def test_case_table_prints():
    t = GC.case_table()
    assert len(t.splitlines()) == 4 + len(GC.TN_CASES) + len(GC.ROWS_CASES)

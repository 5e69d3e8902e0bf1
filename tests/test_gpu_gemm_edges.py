"""The training GEMMs at the edges of their rings, slices and tiles, EXACTLY (tests/_gemm_cases.py): gemm_tn.hip (split-K over
rows, LDS-DMA ring of 5 / 6 step buffers, counted vmcnt waits), gemm_rows.hip (row streaming, ring of 3), the fragment pack, and
the split products built on them.

The operands are small integers, so fp32 accumulation is exact in any order and the device result must EQUAL the integer
product (torch.equal; a bf16 output equals the integer result rounded once to nearest even).  Every case is set in hostile
surroundings: operands inside taller and wider NaN-filled buffers (rows at and past E, columns at and past the real widths),
a NaN-filled workspace with guard bytes behind the reported size, outputs inside sentinel-filled matrices.  A read past E, a
read of padding that reaches a kept element, or a slab tile nobody wrote shows as NaN; a write outside the promised region
breaks a sentinel.  One random-real case per kernel keeps the bars of the older tests (1e-5 / 6e-3 / 3e-5), so the integer cases
do not hide a value-dependent path."""
import ctypes as C

import pytest
import torch

from diffusion_model_amd import _lib
from diffusion_model_amd.gemm import gemm_rows, gemm_tn, mm_nn_split, mm_tn_split, pack_rows_weights
from tests import _gemm_cases as GC
from tests._util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def _sentinel_everywhere_but(parent, r0, r1, c0, c1):
    """every element of `parent` outside [r0, r1) x [c0, c1) still holds the sentinel"""
    p = parent.clone()
    p[r0:r1, c0:c1] = GC.SENTINEL
    return bool((p == GC.SENTINEL).all())


class _TnSetup:
    """device buffers of one gemm_tn case: operands in NaN surroundings, guarded workspace, out block in a sentinel matrix"""

    def __init__(self, case, a_vals, b_vals):
        E, self.case = case.E, case
        self.bufA = GC.embed_nan(a_vals, 3, case.lda - case.rows, torch.bfloat16).to(DEV)      # [E + 3, lda]
        self.bufB = GC.embed_nan(b_vals, 5, case.ldb - case.cols, torch.bfloat16).to(DEV)      # [E + 5, ldb]
        self.a, self.b = self.bufA[:E], self.bufB[:E]
        self.need = int(_lib.lib().egnn_gemm_tn_workspace_bytes(E, case.M, case.N))
        p = GC.plan_gemm_tn(E, case.M, case.N)
        assert self.need == p.S * case.M * case.N * 4
        self.ws = torch.full((self.need + GC.GUARD_BYTES,), 0xFF, dtype=torch.uint8, device=DEV)   # 0xFFFFFFFF: a NaN as fp32
        self.ldc = (case.cols + 8 + 3) // 4 * 4
        self.parent = torch.full((case.rows + 2, self.ldc), GC.SENTINEL, dtype=torch.float32, device=DEV)
        self.out = self.parent[1:1 + case.rows, 4:4 + case.cols]          # interior block, ldc > cols, 16-byte aligned
        assert self.out.data_ptr() % 16 == 0

    def launch(self, scale, accumulate):
        """through the C ABI with exactly the reported workspace size"""
        c = self.case
        _lib.check(_lib.lib().egnn_gemm_tn_bf16(_lib.stream_ptr(), c.E, c.M, c.N, _lib.ptr(self.a), c.lda, _lib.ptr(self.b), c.ldb,
                                                float(scale), _lib.ptr(self.out), self.ldc, c.rows, c.cols, 1 if accumulate else 0,
                                                _lib.ptr(self.ws), self.need))

    def surroundings_intact(self):
        c = self.case
        assert bool((self.ws[self.need:] == 0xFF).all()), "workspace written beyond the reported size"
        assert _sentinel_everywhere_but(self.parent, 1, 1 + c.rows, 4, 4 + c.cols), "out written outside [rows, cols]"
        assert bool(self.bufA[c.E:].isnan().all()) and bool(self.bufA[:, c.rows:].isnan().all())   # (the kernels only read them)


@pytest.mark.parametrize("case", GC.TN_CASES, ids=lambda c: f"E{c.E}-{c.M}x{c.N}-r{c.rows}c{c.cols}-ld{c.lda}x{c.ldb}")
def test_gemm_tn_edge_case_is_exact(case):
    """out[:rows, :cols] equals the integer product; with accumulate onto 3 and scale -0.5 equals 3 - v / 2; twice the same
    bits; nothing outside the block, and no workspace byte beyond the reported size, is written; NaN never leaks in"""
    a, b, want = GC.tn_operands(case)
    s = _TnSetup(case, a, b)
    want_f = want.to(torch.float32).to(DEV)
    s.out.fill_(NAN)
    s.launch(1.0, False)                                   # accumulate = False must not read the NaN block
    first = s.out.clone()
    assert torch.equal(first, want_f), f"{int((first != want_f).sum())} of {want_f.numel()} elements differ (NaN: {int(first.isnan().sum())})"
    s.surroundings_intact()
    s.out.fill_(3.0)
    got = gemm_tn(s.a, s.b, rows=case.rows, cols=case.cols, scale=-0.5, out=s.out, accumulate=True)   # the Python wrapper's path
    assert got.data_ptr() == s.out.data_ptr()
    assert torch.equal(s.out, 3.0 - 0.5 * want_f)
    s.surroundings_intact()
    s.ws.fill_(0xFF)
    s.out.fill_(NAN)
    s.launch(1.0, False)
    assert torch.equal(s.out, first)                       # slices are added in a fixed order: bitwise repeatable
    s.surroundings_intact()


def test_gemm_tn_random_real_case_keeps_the_fp64_bar():
    """random reals in the same surroundings at a case with 17 slices and a one-step last slice: 1e-5 of the largest entry against
    a float64 product of the same bf16 values (the bar of test_gemm_tn_matches_fp64_reference)"""
    case = next(c for c in GC.TN_CASES if (c.E, c.M, c.N) == (8705, 512, 384))
    g = torch.Generator().manual_seed(11)
    a = torch.randn(case.E, case.rows, generator=g).to(torch.bfloat16)
    b = (torch.randn(case.E, case.cols, generator=g) * torch.linspace(0.5, 2.0, case.cols)).to(torch.bfloat16)
    want = a.double().t() @ b.double()
    s = _TnSetup(case, a, b)
    s.out.fill_(NAN)
    s.launch(1.0, False)
    err = float((s.out.cpu().double() - want).abs().max() / want.abs().max())
    print(f"gemm_tn random E={case.E} {case.M}x{case.N}: max err / max |C| = {err:.2e}")
    assert err <= 1e-5
    s.surroundings_intact()


def _rows_setup(case, a0, w0, a1, w1):
    """device operands of a gemm_rows case in NaN surroundings -> (a0, p0, a1, p1, out parent [E + 8, ldo])"""
    E = case.E
    lda0, lda1, ldo = GC.rows_strides(case)
    if case.view:       # A1 as a column-offset view of A0's buffer
        buf = torch.full((E + 3, lda0), NAN, dtype=torch.bfloat16)
        buf[:E, :case.K0] = a0.to(torch.bfloat16)
        off = case.K0 + GC.VIEW_GAP
        buf[:E, off:off + case.K1] = a1.to(torch.bfloat16)
        buf = buf.to(DEV)
        d0, d1 = buf[:E, :case.K0], buf[:E, off:off + case.K1]
    else:
        d0 = GC.embed_nan(a0, 3, lda0 - case.K0, torch.bfloat16).to(DEV)[:E, :case.K0]
        d1 = None if a1 is None else GC.embed_nan(a1, 5, lda1 - case.K1, torch.bfloat16).to(DEV)[:E, :case.K1]
    assert d0.stride(0) == lda0 and (d1 is None or d1.stride(0) == lda1)
    p0 = pack_rows_weights(GC.embed_nan(w0, 0, 3, torch.float32).to(DEV), case.ncols)        # fp32 source: ldw > ncols, NaN beyond
    p1 = None if w1 is None else pack_rows_weights(GC.embed_nan(w1, 0, 7, torch.float32).to(DEV), case.ncols)
    parent = torch.full((E + 8, ldo), GC.SENTINEL, dtype=torch.float32 if case.f32 else torch.bfloat16, device=DEV)
    return d0, p0, d1, p1, parent


def _check_rows_out(case, parent, want_dev):
    """rows [0, E): columns [0, ncols) = want, [ncols, 128 chunks) exactly 0; everything else keeps the sentinel"""
    E, wide = case.E, 128 * GC.chunks_of(case.ncols)
    got = parent[:E, :case.ncols]
    assert torch.equal(got, want_dev), f"{int((got != want_dev).sum())} of {want_dev.numel()} elements differ (NaN: {int(got.isnan().sum())})"
    assert bool((parent[:E, case.ncols:wide] == 0).all())
    assert _sentinel_everywhere_but(parent, 0, E, 0, wide), "out written at or past row E, or past column 128 * chunks"


@pytest.mark.parametrize("case", GC.ROWS_CASES, ids=lambda c: f"E{c.E}-K{c.K0}+{c.K1}-n{c.ncols}-{'f32' if c.f32 else 'bf16'}-ldo+{c.ldo_extra}{'-view' if c.view else ''}")
def test_gemm_rows_edge_case_is_exact(case):
    a0, w0, a1, w1, want = GC.rows_operands(case)
    d0, p0, d1, p1, parent = _rows_setup(case, a0, w0, a1, w1)
    want_dev = (want.to(torch.float32) if case.f32 else GC.to_bf16_rne(want)).to(DEV)
    out = gemm_rows(d0, p0, d1, p1, out=parent, chunks=GC.chunks_of(case.ncols))
    assert out.data_ptr() == parent.data_ptr()
    _check_rows_out(case, parent, want_dev)
    first = parent.clone()
    parent.fill_(GC.SENTINEL)
    gemm_rows(d0, p0, d1, p1, out=parent, chunks=GC.chunks_of(case.ncols))
    assert torch.equal(parent, first)


def test_gemm_rows_random_real_case_keeps_the_fp64_bar():
    """random reals, bf16 output, 5 steps, 3 chunks, E = 257: 6e-3 of the largest entry (one bf16 rounding of the output; the bar
    of test_gemm_rows_matches_fp64_reference)"""
    case = next(c for c in GC.ROWS_CASES if (c.E, c.K0, c.K1, c.f32) == (257, 256, 64, False))
    g = torch.Generator().manual_seed(12)
    a0, a1 = torch.randn(case.E, case.K0, generator=g).to(torch.bfloat16), torch.randn(case.E, case.K1, generator=g).to(torch.bfloat16)
    w0 = (torch.randn(case.K0, case.ncols, generator=g) * torch.linspace(0.5, 2.0, case.ncols))
    w1 = torch.randn(case.K1, case.ncols, generator=g)
    want = a0.double() @ w0.to(torch.bfloat16).double() + a1.double() @ w1.to(torch.bfloat16).double()
    d0, p0, d1, p1, parent = _rows_setup(case, a0, w0, a1, w1)
    gemm_rows(d0, p0, d1, p1, out=parent, chunks=GC.chunks_of(case.ncols))
    err = float((parent[:case.E, :case.ncols].double().cpu() - want).abs().max() / want.abs().max())
    print(f"gemm_rows random E={case.E} K={case.K0}+{case.K1} n={case.ncols}: max err / max |out| = {err:.2e}")
    assert err <= 6e-3
    wide = 128 * GC.chunks_of(case.ncols)
    assert bool((parent[:case.E, case.ncols:wide] == 0).all()) and _sentinel_everywhere_but(parent, 0, case.E, 0, wide)


@pytest.mark.parametrize("K,ncols", GC.PACK_CASES)
def test_pack_rows_weights_equals_the_restated_layout(K, ncols):
    """bit for bit, from an fp32 source with ldw > ncols and NaN in the columns past ncols: padding fragments are exactly +0"""
    w = torch.full((K, ncols + 5), NAN)
    w[:, :ncols] = torch.randn(K, ncols, generator=torch.Generator().manual_seed(K + ncols))
    got = pack_rows_weights(w.to(DEV), ncols).cpu()
    want = GC.pack_rows_layout(w, ncols)
    assert got.shape == want.shape and torch.equal(got.view(torch.int16), want.view(torch.int16))


# ---- split products ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", GC.SPLIT_E)
def test_split_products_integer_inputs_are_exact(E):
    """integer fp32 inputs: the bf16 heads hold them, the remainders are zero, and all three (two) products are exact"""
    for i, (Ma, Nb) in enumerate(GC.SPLIT_TN):
        a, b = GC.int_matrix(E, Ma, 70 + i + E), GC.int_matrix(E, Nb, 80 + i + E)
        bufa = GC.embed_nan(a, 7, 0, torch.float32).to(DEV)              # a taller buffer's first rows, as autograd._wgrad passes
        got = mm_tn_split(bufa[:E], b.float().to(DEV))
        assert got.shape == (Ma, Nb) and torch.equal(got.cpu(), GC.int_product(a.t(), b).float()), (E, Ma, Nb)
    for i, (K, N) in enumerate(GC.SPLIT_NN):
        a, w = GC.int_matrix(E, K, 90 + i + E), GC.int_matrix(K, N, 95 + i + E)
        got = mm_nn_split(a.float().to(DEV), w.float().to(DEV))
        assert got.shape == (E, N) and torch.equal(got.cpu(), GC.int_product(a, w).float()), (E, K, N)


@pytest.mark.parametrize("E", GC.SPLIT_E)
def test_split_products_random_inputs_keep_the_fp64_bar(E):
    """2^-16 per operand -> <= 3e-5 relative against float64 products (the bar of test_split_products_match_fp64)"""
    g = torch.Generator().manual_seed(40 + E)
    for Ma, Nb in GC.SPLIT_TN:
        a, b = torch.randn(E, Ma, generator=g) * torch.logspace(-2, 1, Ma), torch.randn(E, Nb, generator=g)
        e = rel_err(mm_tn_split(a.to(DEV), b.to(DEV)).cpu(), a.double().t() @ b.double())
        print(f"mm_tn_split [{E}, {Ma}]^T [{E}, {Nb}]: {e:.2e}")
        assert e <= 3e-5
    for K, N in GC.SPLIT_NN:
        a, w = torch.randn(E, K, generator=g), torch.randn(K, N, generator=g) * 0.05
        e = rel_err(mm_nn_split(a.to(DEV), w.to(DEV)).cpu(), a.double() @ w.double())
        print(f"mm_nn_split [{E}, {K}] [{K}, {N}]: {e:.2e}")
        assert e <= 3e-5


def _nn_inputs(E, K, N, seed):
    a, w = GC.int_matrix(E, K, seed), GC.int_matrix(K, N, seed + 1)
    return a.float().to(DEV), w.float().to(DEV), GC.int_product(a, w).float().to(DEV)


def test_mm_nn_split_out_direct_view():
    """an fp32 view that owns all 128 * chunks columns is written in place: the result aliases it, and the parent around it keeps
    its sentinel"""
    E, K, N = 33, 100, 130
    a, w, want = _nn_inputs(E, K, N, 21)
    parent = torch.full((E + 2, 256 + 8), GC.SENTINEL, dtype=torch.float32, device=DEV)
    out = parent[1:1 + E, 4:4 + 256]
    res = mm_nn_split(a, w, out=out)
    assert res.data_ptr() == out.data_ptr() and res.shape == (E, N) and torch.equal(res, want)
    assert bool((out[:, N:] == 0).all()) and _sentinel_everywhere_but(parent, 1, 1 + E, 4, 4 + 256)


@pytest.mark.parametrize("E,K,N", [(33, 100, 130), (257, 36, 74)])
def test_mm_nn_split_out_narrow_view_leaves_its_neighbours_alone(E, K, N):
    """an [E, N] view of a wider matrix with N % 128 != 0: the kernel's whole chunks of 128 columns would overwrite the parent's
    columns N .. 128 chunks - 1, so this out must receive a copy.  (The direct path of the version before this test zeroed
    them: the test was red on it.)"""
    a, w, want = _nn_inputs(E, K, N, 22)
    wide = 128 * GC.chunks_of(N)
    parent = torch.full((E + 2, wide + 12), GC.SENTINEL, dtype=torch.float32, device=DEV)
    out = parent[1:1 + E, 4:4 + N]
    res = mm_nn_split(a, w, out=out)
    assert res.shape == (E, N) and torch.equal(out, want) and torch.equal(res, want)
    assert _sentinel_everywhere_but(parent, 1, 1 + E, 4, 4 + N), "mm_nn_split wrote outside its out"


def test_mm_nn_split_out_other_dtype_takes_the_copy():
    E, K, N = 33, 100, 130
    a, w, want = _nn_inputs(E, K, N, 23)
    out = torch.full((E, N), GC.SENTINEL, dtype=torch.float64, device=DEV)
    res = mm_nn_split(a, w, out=out)
    assert res.data_ptr() == out.data_ptr() and torch.equal(out, want.double())


# ---- refusals: decided on the host, nothing is launched ----------------------------------------------------------------------------
def test_misaligned_views_and_bf16_strides_are_refused():
    """operands or outputs that start inside a 16-byte piece, and a bf16 output whose row stride is no multiple of 8, raise
    ValueError in gemm.py; the C ABI refuses the same (EGNN_EINVAL) before any launch"""
    bf = dict(dtype=torch.bfloat16, device=DEV)
    a, b = torch.zeros(40, 264, **bf), torch.zeros(40, 136, **bf)
    out = torch.zeros(256, 132, device=DEV)
    gemm_tn(a, b, rows=256, cols=128, out=out)                                        # aligned: fine
    with pytest.raises(ValueError, match="16-byte"):
        gemm_tn(a[:, 4:], b, rows=256, cols=128)
    with pytest.raises(ValueError, match="16-byte"):
        gemm_tn(a, b[:, 1:], rows=256, cols=128)
    with pytest.raises(ValueError, match="16-byte"):
        gemm_tn(a, b, rows=256, cols=128, out=out[:, 1:])
    w = torch.zeros(64, 133, device=DEV)
    pack = pack_rows_weights(w, 128)
    with pytest.raises(ValueError, match="16-byte"):
        pack_rows_weights(w[:, 1:], 128)
    a0 = torch.zeros(40, 72, **bf)
    gemm_rows(a0[:, :64], pack)
    gemm_rows(a0[:, 8:], pack)                                                        # a view at a multiple of 16 bytes: fine
    with pytest.raises(ValueError, match="16-byte"):
        gemm_rows(a0[:, 4:68], pack)
    with pytest.raises(ValueError, match="16-byte"):
        gemm_rows(a0[:, :64], pack[4:])
    with pytest.raises(ValueError, match="16-byte"):
        gemm_rows(a0[:, :64], pack, a0[:, 4:68], pack)
    with pytest.raises(ValueError, match="16-byte"):
        gemm_rows(a0[:, :64], pack, out=torch.zeros(40, 136, **bf)[:, 4:132])
    with pytest.raises(ValueError, match="multiple of 8"):
        gemm_rows(a0[:, :64], pack, out=torch.zeros(40, 132, **bf)[:, :128])
    gemm_rows(a0[:, :64], pack, out=torch.zeros(40, 132, device=DEV)[:, :128])        # fp32: a stride of 4 floats is enough
    L, st = _lib.lib(), _lib.stream_ptr()
    o = torch.zeros(40, 136, **bf)
    args = lambda op, ldo, f32: (st, 40, _lib.ptr(a0), 72, 64, _lib.ptr(pack), None, 0, 0, None, C.c_void_p(op), ldo, f32, 1)
    assert L.egnn_gemm_rows_bf16(*args(o.data_ptr(), 136, 0)) == 0
    assert L.egnn_gemm_rows_bf16(*args(o.data_ptr(), 132, 0)) == -22 and b"16-byte" in L.egnn_last_error()
    assert L.egnn_gemm_rows_bf16(*args(o.data_ptr() + 8, 128, 0)) == -22
    ws = torch.zeros(int(L.egnn_gemm_tn_workspace_bytes(40, 256, 128)), dtype=torch.uint8, device=DEV)
    tn = lambda pa: L.egnn_gemm_tn_bf16(st, 40, 256, 128, C.c_void_p(pa), 264, _lib.ptr(b), 136, 1.0, _lib.ptr(out), 132, 256, 128, 0,
                                        _lib.ptr(ws), ws.numel())
    assert tn(a.data_ptr()) == 0 and tn(a.data_ptr() + 8) == -22 and b"16-byte" in L.egnn_last_error()
    torch.cuda.synchronize()

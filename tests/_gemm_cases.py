"""Cases of the training GEMMs (csrc/gemm_tn.hip, csrc/gemm_rows.hip) at the edges of their rings, slices and tiles, with
EXACT references (tests/test_gemm_cases_cpu.py, tests/test_gemm_plan_host.py, tests/test_gpu_gemm_edges.py).

Exactness.  The operands are bf16 tensors of small integers, uniform in [-4, 4].  Every product is an integer of magnitude
<= 16 and every partial sum, in whatever order the kernel adds it, is an integer of magnitude <= 16 * (terms) < 2^24, which
fp32 holds exactly.  So fp32 accumulation is exact in ANY order and the device result must EQUAL the integer product: nothing
below is fitted to what the device returns.  `check_exact` asserts the condition on the CPU for every case before anything is
launched.  (The integer products are formed in float64, which is exact below 2^53, and converted to int64; a plain int64
matmul of the largest case takes seconds on the CPU.)

The plan restatement (`plan_gemm_tn`, `xcd_tile`) says in Python what plan_gemm_tn (host_logic.cpp) and xcd_tile (kernels.h)
decide; tests/test_gemm_plan_host.py compares it with the host code's own answers for every case.  The fragment
layout of `pack_rows_weights` is restated from the comment above pack_rows_weights_kernel (gemm_rows.hip)."""
import functools
from collections import namedtuple

import torch

SENTINEL = -0.75            # exact in fp32 and bf16; no integer v and no 3 - v / 2 equals it (a quarter)
LIMIT = 1 << 24             # integers of magnitude below this are exact in fp32
GUARD_BYTES = 4096          # workspace bytes past the reported need that must come back untouched


# ---- the split-K plan of gemm_tn, restated ------------------------------------------------------------------------------------
Plan = namedtuple("Plan", "BN tiles_n S steps_per_slice total_steps last_steps ntiles grid grid_mod8 nbuf")


def plan_gemm_tn(E, M, N):
    """column tile 256 where N allows it, else 128; 32 rows per step; as many slices as give ~768 workgroups, but at least 16
    steps per slice; the slice count is then recomputed from the rounded-up steps per slice (no empty slice)"""
    BN = 256 if N % 256 == 0 else 128
    tiles_n = N // BN
    ntiles = (M // 256) * tiles_n
    total = -(-E // 32)
    want = -(-768 // ntiles)
    S = max(1, min(want, max(total // 16, 1)))
    sps = -(-total // S)
    S = -(-total // sps)
    nbuf = (160 * 1024) // (32 * 256 * 2 + 32 * BN * 2)          # ring depth: 5 (BN = 256) / 6 (BN = 128)
    return Plan(BN, tiles_n, S, sps, total, total - (S - 1) * sps, ntiles, S * ntiles, (S * ntiles) % 8, nbuf)


def xcd_tile(b, nwg):
    """workgroup b of nwg -> position in (slice, tile) order: workgroups b, b + 8, b + 16 ... share an XCD and take consecutive
    positions; the first nwg % 8 XCDs take one position more"""
    xcd, q, r = b % 8, nwg // 8, nwg % 8
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + b // 8


# ---- case tables --------------------------------------------------------------------------------------------------------------
# gemm_tn: E rows, operand widths M / N (padded), real widths rows / cols, row strides lda / ldb
TnCase = namedtuple("TnCase", "E M N rows cols lda ldb")


def _tn(E, M, N, rows=None, cols=None, da=0, db=0):
    return TnCase(E, M, N, M if rows is None else rows, N if cols is None else cols, M + da, N + db)


TN_CASES = (
    # one step, fewer rows than a step
    _tn(1, 256, 128, cols=74, da=8), _tn(31, 256, 128, rows=201, db=8), _tn(32, 256, 256, rows=255, cols=255, da=8, db=8),
    # 2 .. 7 steps around both ring depths (6 for the 128-column tile, 5 for the 256-column tile)
    _tn(33, 256, 128, da=8), _tn(96, 256, 128, cols=74), _tn(128, 256, 128, rows=201, db=8), _tn(160, 256, 128, da=8, db=8),
    _tn(161, 256, 128, rows=1, cols=1), _tn(199, 256, 128, cols=127, da=8), _tn(224, 256, 128, rows=130, cols=74, db=8),
    _tn(33, 256, 256, db=8), _tn(96, 256, 256, rows=201, cols=130), _tn(128, 256, 256, da=8), _tn(160, 256, 256, cols=129, da=8, db=8),
    _tn(161, 256, 256, rows=255), _tn(199, 256, 256, rows=7, cols=250, db=8), _tn(224, 256, 256, da=8),
    # last slice of ONE step, 17 slices
    _tn(8705, 256, 128, cols=74, da=8), _tn(8705, 256, 256, rows=201, db=8), _tn(8705, 512, 384, rows=292, cols=300, da=8, db=8),
    # last slice of two steps, tiles in both directions
    _tn(8737, 512, 512, rows=292, cols=390, da=8),
    # 23 workgroups: grid mod 8 = 7
    _tn(11999, 256, 128, cols=74, db=8),
    # two slices, 9 tiles of 128 columns
    _tn(1061, 768, 384, rows=700, cols=300, da=8, db=8),
    # 16 tiles of 256 columns, the slice count limited by the 16 steps per slice
    _tn(3000, 1024, 1024, rows=1000, cols=1001),
)

# gemm_rows: E rows, reduction widths K0 (+ K1), ncols real output columns, fp32 or bf16 output, ldo = 128 chunks + ldo_extra,
# view: A1 is a column-offset view of A0's buffer (as autograd._finish_graph passes [Gd_x | Gs_x | Gd_m | Gs_m])
RowsCase = namedtuple("RowsCase", "E K0 K1 ncols f32 ldo_extra view")


def _rows(E, K0, K1, ncols, f32, ldo_extra, view=False):
    return RowsCase(E, K0, K1, ncols, bool(f32), ldo_extra, view)


ROWS_CASES = (
    _rows(257, 64, 0, 74, 0, 0), _rows(257, 128, 0, 128, 1, 8), _rows(257, 64, 64, 130, 0, 8), _rows(257, 192, 0, 300, 1, 0),
    _rows(257, 64, 192, 74, 1, 8, view=True), _rows(257, 256, 64, 300, 0, 8),
    _rows(1, 64, 0, 74, 1, 0), _rows(1, 64, 64, 128, 0, 0), _rows(31, 128, 0, 130, 0, 0), _rows(33, 64, 64, 74, 0, 8),
    _rows(255, 192, 0, 128, 1, 8), _rows(256, 64, 192, 300, 0, 0), _rows(513, 256, 64, 130, 1, 0), _rows(513, 64, 0, 300, 0, 8),
)
ROWS_E = (1, 31, 33, 255, 256, 257, 513)
ROWS_K = ((64, 0), (128, 0), (64, 64), (192, 0), (64, 192), (256, 64))
ROWS_NCOLS = (74, 128, 130, 300)

PACK_CASES = tuple((K, n) for K in (64, 192) for n in (1, 74, 128, 130))   # (K, ncols) of pack_rows_weights alone

# split products: E rows, widths that are no multiples of 64 / 128 / 256
SPLIT_E = (1, 33, 257)
SPLIT_TN = ((36, 74), (292, 130), (100, 300))       # (Ma, Nb) of mm_tn_split
SPLIT_NN = ((36, 74), (100, 130), (292, 300))       # (K, N) of mm_nn_split


def chunks_of(ncols):
    return (ncols + 127) // 128


VIEW_GAP = 8   # columns (NaN) between A0's K0 columns and the view A1 in the shared buffer: keeps A1 16-byte aligned


def rows_strides(case):
    """(lda0, lda1, ldo) of a gemm_rows case: operands of width + 8 and + 16 (different even for K0 == K1); the view case shares
    one buffer [A0 | gap | A1 | 8 more columns]"""
    ldo = 128 * chunks_of(case.ncols) + case.ldo_extra
    if case.view:
        w = case.K0 + VIEW_GAP + case.K1 + 8
        return w, w, ldo
    return case.K0 + 8, (case.K1 + 16 if case.K1 else 0), ldo


def host_case_lines():
    """the cases as tests/host/gemm_plan_main.cpp reads them"""
    lines = [f"tn {c.E} {c.M} {c.N} {c.rows} {c.cols} {c.lda} {c.ldb}" for c in TN_CASES]
    for c in ROWS_CASES:
        lda0, lda1, ldo = rows_strides(c)
        lines.append(f"rows {c.E} {c.K0} {c.K1} {lda0} {lda1} {ldo} {int(c.f32)} {chunks_of(c.ncols)}")
    return "\n".join(lines) + "\n"


# ---- integer operands and exact references ------------------------------------------------------------------------------------
def int_matrix(rows, cols, seed):
    """[rows, cols] int64, uniform in [-4, 4]"""
    return torch.randint(-4, 5, (rows, cols), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)


def int_product(a, b):
    """a @ b for int64 matrices of small integers, exactly (float64 holds every partial sum: they stay far below 2^53)"""
    p = a.double() @ b.double()
    out = p.to(torch.int64)
    assert torch.equal(out.double(), p)
    return out


def check_exact(*int_results):
    """the exactness condition: every result, and 3 - result / 2 (= (6 - result) / 2: a halving is exact), below 2^24.  The
    bound on the RESULT bounds every partial sum of it only together with the bound on the terms; both are asserted."""
    for r in int_results:
        assert int(r.abs().max()) + 6 < LIMIT


def assert_terms_bound(n_terms):
    """|partial sum| <= 16 * terms for operands in [-4, 4]: the order-independent bound"""
    assert 16 * n_terms + 6 < LIMIT, n_terms


@functools.lru_cache(maxsize=None)
def tn_operands(case):
    """(a [E, M] int64, b [E, N] int64, want [rows, cols] int64) of a gemm_tn case; columns past rows / cols take part in
    nothing that is kept.  Cached: the tests of one case share them and leave them unchanged."""
    a = int_matrix(case.E, case.rows, 1000 + case.E + case.M)
    b = int_matrix(case.E, case.cols, 2000 + case.E + case.N)
    assert_terms_bound(case.E)
    want = int_product(a.t(), b)
    check_exact(want)
    return a, b, want


@functools.lru_cache(maxsize=None)
def rows_operands(case):
    """(a0 [E, K0], w0 [K0, ncols], a1, w1, want [E, ncols]) int64 of a gemm_rows case (a1 = w1 = None for one operand)"""
    a0, w0 = int_matrix(case.E, case.K0, 3000 + case.E + case.K0), int_matrix(case.K0, case.ncols, 4000 + case.K0 + case.ncols)
    want = int_product(a0, w0)
    a1 = w1 = None
    if case.K1:
        a1, w1 = int_matrix(case.E, case.K1, 5000 + case.E + case.K1), int_matrix(case.K1, case.ncols, 6000 + case.K1 + case.ncols)
        want = want + int_product(a1, w1)
    assert_terms_bound(case.K0 + case.K1)
    check_exact(want)
    return a0, w0, a1, w1, want


def to_bf16_rne(int_result):
    """the int64 result as the device's bf16 output must hold it: exact in fp32 (< 2^24), then ONE rounding to nearest even"""
    return int_result.to(torch.float32).to(torch.bfloat16)


def embed_nan(values, tall, wide, dtype):
    """`values` [r, c] in the top-left corner of a NaN-filled [r + tall, c + wide] matrix of `dtype`"""
    r, c = values.shape
    buf = torch.full((r + tall, c + wide), float("nan"), dtype=dtype)
    buf[:r, :c] = values.to(dtype)
    return buf


# ---- the fragment layout of pack_rows_weights, restated -----------------------------------------------------------------------
def pack_rows_layout(w, ncols):
    """w [K, >= ncols] fp32 -> bf16 fragments [chunks][K / 64 steps][4 k-steps][4 column blocks][64 lanes][8], flattened: lane l,
    element j of fragment (chunk, step, ks, nb) holds w[64 step + 16 ks + 8 (l >> 5) + j][128 chunk + 32 nb + (l & 31)], zero
    where that column is >= ncols"""
    K = w.shape[0]
    assert K % 64 == 0
    ch = chunks_of(ncols)
    wp = torch.zeros(K, 128 * ch, dtype=torch.bfloat16)
    wp[:, :ncols] = w[:, :ncols].to(torch.bfloat16)
    # k = ((step * 4 + ks) * 2 + lh) * 8 + j,  n = (chunk * 4 + nb) * 32 + ll,  lane = 32 lh + ll
    v = wp.view(K // 64, 4, 2, 8, ch, 4, 32)          # [step, ks, lh, j, chunk, nb, ll]
    return v.permute(4, 0, 1, 5, 2, 6, 3).contiguous().view(-1)   # [chunk, step, ks, nb, lh, ll, j]


def pack_rows_element(w, ncols, i):
    """element i of the pack, one at a time (the same statement as a scalar formula: checks the vectorised one)"""
    K = w.shape[0]
    chunk, i = divmod(i, K * 128)
    j, lane, f = i & 7, (i >> 3) & 63, i >> 9
    nb, ks, step = f & 3, (f >> 2) & 3, f >> 4
    n, k = 128 * chunk + 32 * nb + (lane & 31), 64 * step + 16 * ks + 8 * (lane >> 5) + j
    return float(w[k, n].to(torch.bfloat16)) if n < ncols else 0.0


# ---- the printed case table (profiles/gemm_edge_cases.txt) --------------------------------------------------------------------
def case_table():
    lines = ["gemm_tn cases: E M N rows cols lda ldb | BN tiles S steps/slice total last-slice-steps ring grid grid%8"]
    for c in TN_CASES:
        p = plan_gemm_tn(c.E, c.M, c.N)
        lines.append(f"  {c.E:6d} {c.M:5d} {c.N:5d} {c.rows:5d} {c.cols:5d} {c.lda:5d} {c.ldb:5d} | {p.BN:4d} {p.ntiles:3d} {p.S:3d} "
                     f"{p.steps_per_slice:3d} {p.total_steps:4d} {p.last_steps:3d} {p.nbuf:2d} {p.grid:4d} {p.grid_mod8}")
    lines.append("gemm_rows cases: E K0 K1 ncols out ldo A1 | steps chunks row-blocks")
    for c in ROWS_CASES:
        lines.append(f"  {c.E:4d} {c.K0:4d} {c.K1:4d} {c.ncols:4d} {'fp32' if c.f32 else 'bf16'} {128 * chunks_of(c.ncols) + c.ldo_extra:4d} "
                     f"{'view' if c.view else 'own '} | {(c.K0 + c.K1) // 64:2d} {chunks_of(c.ncols)} {(c.E + 255) // 256}")
    lines.append("pack_rows_weights cases (K, ncols): " + " ".join(str(c) for c in PACK_CASES))
    lines.append(f"split products: E in {SPLIT_E}, mm_tn_split (Ma, Nb) in {SPLIT_TN}, mm_nn_split (K, N) in {SPLIT_NN}")
    return "\n".join(lines)


if __name__ == "__main__":
    print(case_table())

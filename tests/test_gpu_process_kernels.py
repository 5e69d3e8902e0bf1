"""The kernels around the network, one by one through the C ABI (or the thin Python wrapper) against tests/_process_ref.py:

  csrc/sampler.hip      center_kernel + slice_cols_kernel (egnn_remove_mean, egnn_eps), reverse_step_kernel (ddpm_reverse_step)
  csrc/aux_mlp.hip      gamma_tilde_kernel (egnn_gamma_tilde), dense_rows_kernel (egnn_dense_rows)
  csrc/graph_stats.hip  fc_rowptr / fc_fill (egnn_fc_graph_build), radius_count / radius_fill, rdf_kernel, sio_si_kernel

Every input and output sits inside a larger buffer (Guard): 7.0 around it, NaN where a stray read would poison the result.  What
lies outside the documented extent must come back bit-identical and inputs must be unchanged.  Errors are judged element by
element against the bound functions of tests/_process_ref.py (built from 2^-24 and the number of roundings, never from a device
result); each comparison prints `proc-kernel-ratio <kernel> <case> <output> <worst |error| / bound>` and asserts ratio <= 1
(profiles/process_kernel_errors.txt is that output from an MI355X).  Integer results and exact cases are compared bitwise.
"""
import functools

import numpy as np
import pytest
import torch

import diffusion_model_amd as dma
from diffusion_model_amd import _lib
from oracle import egnn_ref
from tests import _process_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -22                # EGNN_EINVAL of include/egnn_amd.h
SENT = 7.0
NAN = float("nan")
PAD = 64                    # guard elements on either side of every buffer
# kernel -> (factor on its bound, cause by file:line, measurement).  Empty: every kernel meets its derived bound as it stands.
FACTOR = {}


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _biteq(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Guard:
    """a tensor inside a larger flat buffer: .t is the documented extent, the PAD elements on either side hold ``pad``"""

    def __init__(self, shape, value=None, fill=NAN, pad=SENT, dtype=torch.float32):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), pad, dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + n].view(*shape)
        if value is None:
            self.t.fill_(fill)
        else:
            self.t.copy_(torch.as_tensor(value).to(dtype).reshape(shape))
        self.before = self.buf.clone()

    @property
    def p(self):
        return _lib.ptr(self.t)

    def outside_ok(self):
        torch.cuda.synchronize()
        return _biteq(self.buf[:PAD], self.before[:PAD]) and _biteq(self.buf[-PAD:], self.before[-PAD:])

    def unchanged(self):
        torch.cuda.synchronize()
        return _biteq(self.buf, self.before)


def _all_ok(*guards, inputs=(), what=""):
    for k, g in enumerate(guards):
        assert g.outside_ok(), (what, "a kernel wrote outside output", k)
    for k, g in enumerate(inputs):
        assert g.unchanged(), (what, "a kernel wrote to input", k)


def _ratio(kernel, case, output, got, want, bound):
    """element-wise |got - want| / bound; an element whose bound is 0 must be exact.  NaN in got fails."""
    got, want, bound = R.f64(got), R.f64(want), np.broadcast_to(R.f64(bound), np.shape(want))
    assert got.shape == want.shape, (kernel, case, output, got.shape, want.shape)
    err = np.abs(got - want)
    assert np.isfinite(got).all(), (kernel, case, output, "non-finite output")
    assert (err[bound == 0] == 0).all(), (kernel, case, output, "inexact where the bound is 0")
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"proc-kernel-ratio {kernel} {case} {output} {ratio:.3f}")
    assert ratio <= FACTOR.get(kernel, (1.0,))[0], (kernel, case, output, ratio)
    return ratio


def _ptr_of(sizes):
    return torch.tensor(R.bounds_of(sizes), dtype=torch.int32, device=DEV)


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- 1. center_kernel ------------------------------------------------------------------------------------------------------
def _remove_mean(x, ptr, B=None, N=None, D=None):
    gin, gout = Guard(x.shape, x), Guard(x.shape)
    N, D = (x.shape[0] if N is None else N), (x.shape[1] if D is None else D)
    rc = _lib.lib().egnn_remove_mean(_lib.stream_ptr(), N, D, _lib.ptr(ptr), (0 if ptr is None else ptr.numel() - 1) if B is None else B,
                                     gin.p, gout.p)
    _all_ok(gout, inputs=(gin,), what="egnn_remove_mean")
    return rc, gout


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 7])
@pytest.mark.parametrize("scope", ["graph", "global", "one_graph_ptr"])
def test_remove_mean_every_column_chunk(scope, D):
    """D = 1, 2 end inside the first chunk of three columns, 3 fills it, 4, 5 and 7 end inside a later one; per graph on the size
    batch, one mean over all rows, and B = 1 with a graph_ptr.  The second input is 1000 + noise: the mean cancels."""
    sizes = {"graph": R.SIZES, "global": R.SIZES, "one_graph_ptr": (300,)}[scope]
    N = sum(sizes)
    ptr = None if scope == "global" else _ptr_of(sizes)
    ref_ptr = None if scope == "global" else R.bounds_of(sizes)
    for name, x in (("normal", _randn(10 + D, N, D) * 2.0), ("offset1000", 1000.0 + _randn(20 + D, N, D))):
        rc, out = _remove_mean(x, ptr)
        _lib.check(rc)
        _ratio("center", f"{scope}-D{D}-{name}", "out", out.t, R.center(x, None, ref_ptr), R.center_bound(x, None, ref_ptr))
        if scope == "graph":
            assert (out.t[0] == 0).all(), "a one-atom graph minus its own mean is exactly 0"


def test_remove_mean_exact_on_integers():
    """a 256-atom graph of small integers whose column sums are multiples of 256: every partial sum, the mean and the result are
    integers that fp32 holds exactly, so the device must return the integer result bit for bit (between two other graphs)"""
    g = torch.Generator().manual_seed(3)
    for D in (3, 5):
        half = torch.randint(-8, 9, (128, D), generator=g)
        c = 2 * torch.randint(-3, 4, (1, D), generator=g)                  # row n and row 128 + n add up to c: the sum is 128 c
        block = torch.cat((half, c - half))[torch.randperm(256, generator=g)]
        assert (block.sum(0) % 256 == 0).all()
        x = torch.cat((_randn(4, 7, D), block.float(), _randn(5, 9, D)))
        rc, out = _remove_mean(x, _ptr_of((7, 256, 9)))
        _lib.check(rc)
        want = (block - block.sum(0) // 256).float()
        assert _biteq(out.t[7:263].cpu(), want), D


@pytest.mark.parametrize("H", [7, 36])
def test_eps_slices_bitwise_and_centres_under_the_bound(H):
    """eps_h must be h_out[:, :A] bit for bit (A = 1, 2, 5, H; N A under, at and over one 256-thread block of slice_cols_kernel);
    eps_x = remove_mean(x_out - x_in) under the bound of center_kernel"""
    for sizes, per_graph in ((R.SIZES, True), ((51,), False), ((128,), False), ((257,), True), ((256,), False)):
        N = sum(sizes)
        ptr, ref_ptr = (_ptr_of(sizes), R.bounds_of(sizes)) if per_graph else (None, None)
        h_out, x_out, x_in = Guard((N, H), _randn(30 + H, N, H)), Guard((N, 3), _randn(31, N, 3) * 3.0), Guard((N, 3), _randn(32, N, 3))
        for A in (1, 2, 5, H):
            eps_x, eps_h = Guard((N, 3)), Guard((N, A))
            _lib.check(_lib.lib().egnn_eps(_lib.stream_ptr(), N, H, A, _lib.ptr(ptr), len(sizes) if per_graph else 0, h_out.p, x_out.p,
                                           x_in.p, eps_x.p, eps_h.p))
            _all_ok(eps_x, eps_h, inputs=(h_out, x_out, x_in), what=("egnn_eps", N, H, A))
            assert _biteq(eps_h.t, h_out.t[:, :A]), ("eps_h", N, H, A)
            _ratio("center", f"eps-N{N}-H{H}-A{A}", "eps_x", eps_x.t, R.center(x_out.t, x_in.t, ref_ptr), R.center_bound(x_out.t, x_in.t, ref_ptr))


def test_center_argument_checks_write_nothing():
    N, H = 20, 7
    ptr = _ptr_of((20,))
    h_out, x_out, x_in, eps_x, eps_h = Guard((N, H), fill=1.0), Guard((N, 3), fill=1.0), Guard((N, 3), fill=1.0), Guard((N, 3)), Guard((N, H + 1))
    L, s = _lib.lib(), _lib.stream_ptr()
    assert L.egnn_eps(s, N, H, H + 1, None, 0, h_out.p, x_out.p, x_in.p, eps_x.p, eps_h.p) == EINVAL          # A > H
    assert L.egnn_eps(s, N, H, 2, _lib.ptr(ptr), 0, h_out.p, x_out.p, x_in.p, eps_x.p, eps_h.p) == EINVAL     # B < 1 with a pointer
    assert eps_x.unchanged() and eps_h.unchanged()
    x = torch.ones(N, 3)
    for kw in (dict(D=0), dict(B=0)):                                                                          # D < 1; B < 1 with a pointer
        rc, out = _remove_mean(x, ptr, **kw)
        assert rc == EINVAL and out.unchanged(), kw


# ---- 2. reverse_step_kernel ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _step_constants():
    """(name, c0, c1, c2, noise is eps): a real row of the step table, the diffuse form, the calculate_mu form"""
    proc = dma.E3DiffusionProcess(0.2, 2.0, 6)
    row = [float(v) for v in proc.step_table()[4, :3]]
    return (("table_row", *row, False), ("diffuse", float(proc.alpha(4)), 0.0, float(proc.sigma(4)), False),
            ("calculate_mu", row[0], row[1], 0.0, True))


def _reverse_step(N, D, mode_pos, ptr, B, c, z, ldz, eps, noise, zo, ldo):
    return _lib.lib().ddpm_reverse_step(_lib.stream_ptr(), N, D, mode_pos, _lib.ptr(ptr), B, c[0], c[1], c[2], z.p, ldz, eps.p, noise.p, zo.p, ldo)


@pytest.mark.parametrize("D", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("mode_pos", [0, 1])
@pytest.mark.parametrize("per_graph", [False, True])
def test_reverse_step_strided_rows_and_per_graph_means(per_graph, mode_pos, D):
    """the full cross of graph_ptr NULL / given, mode_pos, D and the row strides (ldz, ldo) in {(D, D), (D + 3, D), (D, 36)} on
    the size batch, for three sets of constants.  The padding columns of z hold NaN (never read), those of the output 7.0 (kept)."""
    sizes, N, B = R.SIZES, sum(R.SIZES), len(R.SIZES)
    ptr, ref_ptr = (_ptr_of(sizes), R.bounds_of(sizes)) if per_graph else (None, None)
    zv, ev, nv = _randn(40 + D, N, D) * 2.0, _randn(50 + D, N, D), _randn(60 + D, N, D) + 0.5
    eps, noise = Guard((N, D), ev), Guard((N, D), nv)
    for ldz, ldo in ((D, D), (D + 3, D), (D, 36)):
        zfull = torch.full((N, ldz), NAN)
        zfull[:, :D] = zv
        z = Guard((N, ldz), zfull)
        for name, c0, c1, c2, noise_is_eps in _step_constants():
            nz, nzv = (eps, ev) if noise_is_eps else (noise, nv)
            zo = Guard((N, ldo), fill=SENT)
            _lib.check(_reverse_step(N, D, mode_pos, ptr, B if per_graph else 0, (c0, c1, c2), z, ldz, eps, nz, zo, ldo))
            case = f"{'graph' if per_graph else 'global'}-pos{mode_pos}-D{D}-ld{ldz}.{ldo}-{name}"
            _all_ok(zo, inputs=(z, eps, noise), what=case)
            assert _biteq(zo.t[:, D:], torch.full((N, ldo - D), SENT, device=DEV)), (case, "padding columns of the output")
            _ratio("reverse_step", case, "z_out", zo.t[:, :D], R.reverse_step(zv, ev, nzv, c0, c1, c2, mode_pos, ref_ptr),
                   R.reverse_step_bound(zv, ev, nzv, c0, c1, c2, mode_pos, ref_ptr))
            if per_graph and mode_pos:
                # the one-atom graph: its noise minus its own mean is 0, so the row is z c0 - eps c1, each operation rounded once
                f = np.float32
                want = f(zv[0].numpy() * f(c0)) - f(ev[0].numpy() * f(c1))
                assert want.dtype == np.float32 and _biteq(zo.t[0, :D].cpu(), torch.from_numpy(want)), (case, "one-atom graph")


def test_reverse_step_argument_checks_write_nothing():
    N, D = 10, 3
    z, eps, noise, zo = Guard((N, D), fill=1.0), Guard((N, D), fill=1.0), Guard((N, D), fill=1.0), Guard((N, D))
    assert _reverse_step(N, D, 1, None, 0, (1.0, 1.0, 1.0), z, D - 1, eps, noise, zo, D) == EINVAL             # ldz < D
    assert _reverse_step(N, D, 1, None, 0, (1.0, 1.0, 1.0), z, D, eps, noise, zo, D - 1) == EINVAL             # ldo < D
    assert _reverse_step(N, D, 1, _ptr_of((10,)), 0, (1.0, 1.0, 1.0), z, D, eps, noise, zo, D) == EINVAL       # B < 1 with a pointer
    assert zo.unchanged()


# ---- 3. gamma_tilde_kernel -------------------------------------------------------------------------------------------------
def _gamma_weights(hidden, kind):
    """'init': the module's own initialisation at this width; 'wide': w2, w3 uniform in [-30, 25] and w1 = 3 -- both sides of the
    softplus threshold (x > 20), log1pf of 1e-13 and saturated sigmoids"""
    g = torch.Generator().manual_seed(hidden)
    if kind == "wide":
        return torch.tensor([3.0]), torch.rand(hidden, generator=g) * 55.0 - 30.0, torch.rand(hidden, generator=g) * 55.0 - 30.0
    torch.manual_seed(hidden)
    return tuple(dma.snr.PositiveLinear(*s).weight.detach().reshape(-1).clone() for s in ((1, 1), (1, hidden), (hidden, 1)))


def _gamma_times(n):
    if n == 1:
        return torch.tensor([1.0])
    if n == 3:
        return torch.tensor([0.0, 0.5, 1.0])
    return torch.cat((torch.tensor([0.0, 1.0]), torch.linspace(0, 1, n - 2)))


def _gamma_launch(t, w1, w2, w3, hidden=None):
    gt, g1, g2, g3, out = Guard(t.shape, t), Guard(1, w1), Guard(w2.shape, w2), Guard(w3.shape, w3), Guard(t.shape)
    rc = _lib.lib().egnn_gamma_tilde(_lib.stream_ptr(), t.numel(), w2.numel() if hidden is None else hidden, gt.p, g1.p, g2.p, g3.p, out.p)
    _all_ok(out, inputs=(gt, g1, g2, g3), what="egnn_gamma_tilde")
    return rc, out


@pytest.mark.parametrize("hidden", [1, 255, 256, 257, 1024, 1500])
def test_gamma_tilde_every_width_and_both_softplus_branches(hidden):
    """hidden under / at / over one 256-thread pass, the module's 1024 and a width that is no multiple of 256; n = 1, 3, 1002"""
    for kind in ("init", "wide"):
        w1, w2, w3 = _gamma_weights(hidden, kind)
        for n in (1, 3, 1002):
            t = _gamma_times(n)
            rc, out = _gamma_launch(t, w1, w2, w3)
            _lib.check(rc)
            _ratio("gamma_tilde", f"h{hidden}-{kind}-n{n}", "out", out.t, R.gamma_tilde(t, w1, w2, w3), R.gamma_tilde_bound(t, w1, w2, w3))


@pytest.mark.parametrize("which", ["w1", "w3"])
def test_gamma_tilde_softplus_threshold_side(which):
    """one hidden unit, the weight under test just above 10, around 20 and beyond: at x = 20 both branches of the softplus agree
    to 2e-9, so which side the threshold falls on shows only in where it sits -- log1p(exp(x)) - x is 4.5e-5 at x = 10, four times
    the bound of these cases, and a threshold moved to 10 is caught; w2 = -30 keeps the sigmoid at 1 / 2"""
    for x in (10.001, 19.999, 20.0, 20.001, 25.0):
        w1 = torch.tensor([x if which == "w1" else -2.0])
        w2, w3 = torch.tensor([-30.0]), torch.tensor([x if which == "w3" else -2.0])
        t = torch.tensor([0.0, 1.0])
        rc, out = _gamma_launch(t, w1, w2, w3)
        _lib.check(rc)
        _ratio("gamma_tilde", f"threshold-{which}-{x}", "out", out.t, R.gamma_tilde(t, w1, w2, w3), R.gamma_tilde_bound(t, w1, w2, w3))


def test_gamma_tilde_bound_shows_one_hidden_unit():
    """at hidden = 1024 with the module's initialisation a term is sp(-2) sigmoid(.) = 0.06 .. 0.07 and the bound about 9e-5: a
    dropped or doubled unit is off by more than 500 times the bound (the margin asserted here is 100)"""
    w1, w2, w3 = _gamma_weights(1024, "init")
    t = _gamma_times(3)
    rc, out = _gamma_launch(t, w1, w2, w3)
    _lib.check(rc)
    got, bound = R.f64(out.t), R.gamma_tilde_bound(t, w1, w2, w3)
    dropped = R.gamma_tilde(t, w1, w2[:-1], w3[:-1])
    doubled = R.gamma_tilde(t, w1, torch.cat((w2, w2[-1:])), torch.cat((w3, w3[-1:])))
    for name, wrong in (("dropped", dropped), ("doubled", doubled)):
        margin = float((np.abs(got - wrong) / bound).min())
        print(f"gamma_tilde hidden 1024: a {name} unit is {margin:.0f} x the bound away")
        assert margin > 100, (name, margin)
    rc, short = _gamma_launch(t, w1, w2, w3, hidden=1023)                   # the kernel itself told to leave the last unit out
    _lib.check(rc)
    _ratio("gamma_tilde", "h1023-of-1024", "out", short.t, dropped, R.gamma_tilde_bound(t, w1, w2[:-1], w3[:-1]))


def test_gamma_network_forward_endpoints_bitwise_and_monotone_table():
    torch.manual_seed(11)
    net = dma.GammaNetwork().to(DEV)
    with torch.no_grad():
        net.gamma_0.fill_(-4.75)
        net.gamma_1.fill_(9.5)
    T = 1000
    t = torch.linspace(0, 1, T + 1).view(-1, 1).to(DEV)
    with torch.no_grad():
        gamma = net(t).reshape(-1)
        gt, g0, g1 = net._gamma_tilde_device(t)
    # t = 0 and t = 1 are evaluated twice in the same launch by a deterministic kernel: (gt - g0) / (g1 - g0) is exactly 0 and 1
    assert float(t[0]) == 0.0 and float(t[-1]) == 1.0
    assert _biteq(gt[0].reshape(1), g0.reshape(1)) and _biteq(gt[-1].reshape(1), g1.reshape(1))
    assert _biteq(gamma[:1], net.gamma_0.detach()) and _biteq(gamma[-1:], net.gamma_1.detach())
    w1, w2, w3 = (m.weight.detach().cpu().reshape(-1) for m in (net.l1, net.l2, net.l3))
    bound = R.gamma_tilde_bound(t.cpu(), w1, w2, w3)
    _ratio("gamma_tilde", "module-T1000", "gamma_tilde", gt.reshape(-1), R.gamma_tilde(t.cpu(), w1, w2, w3), bound)
    # non-decreasing up to twice the bound (two neighbours, one bound each)
    step = np.diff(R.f64(gt.reshape(-1)))
    assert (step >= -(bound[1:] + bound[:-1])).all(), float(step.min())
    # and through the affine map to [gamma_0, gamma_1]: the bound times its slope, + the map's own roundings on |gamma| <= 9.5
    ref = R.gamma_tilde(t.cpu(), w1, w2, w3)
    slope = (9.5 + 4.75) / (ref[-1] - ref[0])
    stepg = np.diff(R.f64(gamma))
    assert (stepg >= -(slope * (bound[1:] + bound[:-1]) + 8 * R.U * 14.25)).all(), float(stepg.min())


# ---- 4. dense_rows_kernel --------------------------------------------------------------------------------------------------
def _dense(x, W, b, relu, K=None):
    N, J = x.shape[0], W.shape[0]
    gx, gW, gb, out = Guard(x.shape, x), Guard(W.shape, W), Guard(b.shape, b), Guard((N, J))
    rc = _lib.lib().egnn_dense_rows(_lib.stream_ptr(), N, x.shape[1] if K is None else K, J, gx.p, gW.p, gb.p, relu, out.p)
    _all_ok(out, inputs=(gx, gW, gb), what=("egnn_dense_rows", N, x.shape[1], J))
    return rc, out


# (N, K, J, relu): what the case reaches.  Tiles hold 16 rows; the staged rows take 64 K bytes of LDS; one pass of the output
# loop covers 256 columns.
DENSE_EXACT = [
    (1, 1, 1, 0),           # the smallest call: a last tile of 1 row, one column, one product
    (1, 3, 32, 1),          # one row
    (15, 200, 255, 0),      # a last (only) tile of 15 rows; J one short of a pass
    (16, 200, 256, 1),      # a full tile; exactly one pass
    (17, 3, 257, 0),        # two tiles, the last of 1 row; a second pass for one column
    (33, 200, 600, 1),      # three tiles, the last of 1 row; three passes
    (15, 1024, 32, 0),      # LDS exactly 64 KiB, the most a kernel gets without the attribute
    (16, 1024, 256, 0),     # the same with a full tile and a full pass
    (17, 1025, 32, 1),      # LDS just over 64 KiB: the first launch that needs hipFuncSetAttribute
    (15, 1025, 255, 1),     # the same, last tile of 15
    (16, 1025, 1, 1),       # the same, one column
    (16, 2048, 1, 0),       # the documented maximum K: 128 KiB of LDS
    (33, 2048, 257, 1),     # the maximum with three tiles and two passes
    (1, 2048, 600, 0),      # the maximum with one row and three passes
    (17, 2048, 32, 1),      # the maximum, last tile of 1 row
    (33, 1, 600, 1),        # K = 1 across tiles and passes
    (17, 200, 1, 0),        # J = 1 across tiles
    (1, 1024, 257, 1),      # one row at 64 KiB, two passes
    (15, 3, 600, 0),        # short rows, three passes
    (33, 1024, 255, 0),     # 64 KiB with three tiles
]


@pytest.mark.parametrize("N,K,J,relu", DENSE_EXACT)
def test_dense_rows_exact_on_integers(N, K, J, relu):
    """inputs in {-2..2}, weights in {-1, 0, 1}, integer biases: every fmaf is exact (|sum| <= 2 K + 9 < 2^24), so the device must
    equal the integer product bit for bit"""
    g = torch.Generator().manual_seed(N * 100003 + K * 101 + J)
    x = torch.randint(-2, 3, (N, K), generator=g)
    W = torch.randint(-1, 2, (J, K), generator=g)
    b = torch.randint(-9, 10, (J,), generator=g)
    want = b[None, :] + x @ W.t()
    if relu:
        want = want.clamp(min=0)
    rc, out = _dense(x.float(), W.float(), b.float(), relu)
    _lib.check(rc)
    assert _biteq(out.t.cpu(), want.float()), (N, K, J, relu)


@pytest.mark.parametrize("N,K,J", [(33, 200, 150), (17, 2048, 64)])
def test_dense_rows_real_values(N, K, J):
    x, W, b = _randn(70, N, K), _randn(71, J, K) / K ** 0.5, _randn(72, J)
    for relu in (0, 1):
        rc, out = _dense(x, W, b, relu)
        _lib.check(rc)
        _ratio("dense_rows", f"N{N}-K{K}-J{J}-relu{relu}", "out", out.t, R.dense_rows(x, W, b, relu), R.dense_rows_bound(x, W, b))


def test_spectrum_compressor_chain_under_the_chained_bound():
    """200 -> 150 -> 100 -> 50 -> 32 on 33 rows through the module's device path: layer l's error is its own bound (on the
    reference's activations) plus the previous layer's error carried through |W| (ReLU does not stretch an error)"""
    torch.manual_seed(13)
    c = dma.SpectrumCompressor(200, [150, 100, 50], 32)
    x = torch.rand(33, 200, generator=torch.Generator().manual_seed(14))
    lins = [m for m in c.mlp if isinstance(m, torch.nn.Linear)]
    act, err = R.f64(x), np.zeros((33, 200))
    for i, lin in enumerate(lins):
        W, b = lin.weight.detach(), lin.bias.detach()
        err = R.dense_rows_bound(act, W, b) * (1 + (act.shape[1] + 1) * R.U) + err @ np.abs(R.f64(W)).T
        act = R.dense_rows(act, W, b, i + 1 < len(lins))
    c.to(DEV).eval()
    gx = Guard(x.shape, x)
    with torch.no_grad():
        got = c(gx.t)
    assert gx.unchanged()
    _ratio("dense_rows", "compressor-33rows", "out", got, act, err)


def test_dense_rows_rejects_k_above_the_limit():
    rc, out = _dense(torch.ones(3, 2049), torch.ones(4, 2049), torch.ones(4), 0)
    assert rc == EINVAL and out.unchanged()


# ---- 5. fc_rowptr_kernel / fc_fill_kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[1, 1, 1], [1, 5, 1], [65], [64, 66, 1, 130], [257], [100, 155], [128, 127, 1], [256, 1]],
                         ids=lambda s: "-".join(map(str, s)))
def test_fc_graph_build_bitwise(sizes):
    """graphs above 64 atoms give fc_fill_kernel's 64-thread loop a second (65, 66), third (130) and fifth (257) pass; N = 255 /
    256 / 257 put fc_rowptr_kernel's extra i == N thread at the end of a block, alone in a block of its own, and behind one
    more node there"""
    N, B = sum(sizes), len(sizes)
    ei = egnn_ref.fully_connected_edge_index(sizes)
    ref = dma.GraphPlan(ei, N, sizes=sizes)
    E = ei.shape[1]
    per = torch.tensor(sizes, dtype=torch.int64) * (torch.tensor(sizes, dtype=torch.int64) - 1)
    base = torch.zeros(B, dtype=torch.int64)
    base[1:] = torch.cumsum(per, 0)[:-1]
    i32 = dict(dtype=torch.int32)
    gp = Guard(B + 1, R.bounds_of(sizes), pad=-1, **i32)
    ng = Guard(N, np.repeat(np.arange(B), sizes), pad=-1, **i32)
    gb = Guard(B, base, pad=-1, dtype=torch.int64)
    row_ptr, dst, src = Guard(N + 1, fill=-7, pad=7, **i32), Guard(max(E, 1), fill=-7, pad=7, **i32), Guard(max(E, 1), fill=-7, pad=7, **i32)
    _lib.check(_lib.lib().egnn_fc_graph_build(_lib.stream_ptr(), N, B, gp.p, ng.p, gb.p, row_ptr.p, dst.p if E else None, src.p if E else None))
    _all_ok(row_ptr, dst, src, inputs=(gp, ng, gb), what=sizes)
    assert torch.equal(row_ptr.t.cpu(), ref.row_ptr)
    if E:
        assert torch.equal(dst.t.cpu(), ref.edge_dst) and torch.equal(src.t.cpu(), ref.edge_src)
        assert torch.equal(dst.t.cpu().long(), ei[0]) and torch.equal(src.t.cpu().long(), ei[1])
    else:
        assert dst.unchanged() and src.unchanged()
    only = Guard(N + 1, fill=-7, pad=7, **i32)                              # the row_ptr-only form
    _lib.check(_lib.lib().egnn_fc_graph_build(_lib.stream_ptr(), N, B, gp.p, ng.p, gb.p, only.p, None, None))
    _all_ok(only, inputs=(gp, ng, gb), what=sizes)
    assert torch.equal(only.t.cpu(), ref.row_ptr)
    plan = dma.fully_connected_plan(sizes, DEV)                             # and the wrapper
    assert plan.E == E and torch.equal(plan.row_ptr.cpu(), ref.row_ptr) and torch.equal(dma.plan_edge_index(plan).cpu(), ei)
    assert plan.graph_edge_ptr == ref.graph_edge_ptr


# ---- 6. radius_count_kernel / radius_fill_kernel ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _radius_cases():
    return R.radius_cases()


@pytest.mark.parametrize("name", ["random", "N127", "N128", "N129", "lattice", "duplicates", "one_empty_graph"])
def test_radius_graph_bitwise_order_included(name):
    """deg, edge_dst and edge_src equal the exact float32 restatement, order included: the lattice has pairs at exactly r (absent)
    and at d^2 = 3 (present), the duplicates pairs at d = 0 (present, j != i), one batch a whole graph without an edge"""
    x, sizes, r = _radius_cases()[name]
    N, B = sum(sizes), len(sizes)
    wdeg, wdst, wsrc = R.radius_edges(x, sizes, r)
    E = len(wdst)
    i32 = dict(dtype=torch.int32)
    gx = Guard((N, 3), x)
    gp, ng = Guard(B + 1, R.bounds_of(sizes), pad=-1, **i32), Guard(N, np.repeat(np.arange(B), sizes), pad=-1, **i32)
    deg = Guard(N, fill=-7, pad=7, **i32)
    _lib.check(_lib.lib().egnn_radius_graph_count(_lib.stream_ptr(), N, gx.p, gp.p, ng.p, float(r), deg.p))
    _all_ok(deg, inputs=(gx, gp, ng), what=name)
    assert np.array_equal(deg.t.cpu().numpy(), wdeg), name
    row = np.zeros(N + 1, dtype=np.int32)
    row[1:] = np.cumsum(wdeg)
    row_ptr = Guard(N + 1, row, pad=-1, **i32)
    dst, src = Guard(E, fill=-7, pad=7, **i32), Guard(E, fill=-7, pad=7, **i32)
    _lib.check(_lib.lib().egnn_radius_graph_fill(_lib.stream_ptr(), N, gx.p, gp.p, ng.p, float(r), row_ptr.p, dst.p, src.p))
    _all_ok(dst, src, inputs=(gx, gp, ng, row_ptr), what=name)
    assert np.array_equal(dst.t.cpu().numpy(), wdst) and np.array_equal(src.t.cpu().numpy(), wsrc), name
    plan = dma.radius_plan(torch.from_numpy(x).to(DEV), sizes, r)           # and the wrapper
    assert plan.E == E and np.array_equal(plan.row_ptr.cpu().numpy(), row)
    assert np.array_equal(plan.edge_dst.cpu().numpy(), wdst) and np.array_equal(plan.edge_src.cpu().numpy(), wsrc)
    assert plan.graph_edge_ptr == [int(row[b]) for b in R.bounds_of(sizes)]


def test_radius_plan_without_an_edge_and_radius_checks():
    x, sizes, r = _radius_cases()["no_edges"]
    plan = dma.radius_plan(torch.from_numpy(x).to(DEV), sizes, r)
    assert plan.E == 0 and plan.edge_dst.shape == (0,) and plan.edge_src.shape == (0,)
    assert plan.edge_dst.dtype == torch.int32 and plan.edge_src.dtype == torch.int32
    assert plan.graph_edge_ptr == [0, 0, 0] and plan.row_ptr.cpu().tolist() == [0] * (sum(sizes) + 1)
    assert dma.plan_edge_index(plan).shape == (2, 0)
    N = sum(sizes)
    gx, deg = Guard((N, 3), x), Guard(N, fill=-7, pad=7, dtype=torch.int32)
    for bad in (0.0, -1.0, NAN):
        assert _lib.lib().egnn_radius_graph_count(_lib.stream_ptr(), N, gx.p, _lib.ptr(plan.graph_ptr), _lib.ptr(plan.node_graph), bad, deg.p) == EINVAL
    assert deg.unchanged()


# ---- 7. rdf_kernel ---------------------------------------------------------------------------------------------------------
RDF_SIZES = (1, 2, 64, 257, 600)            # one atom (all zeros); one distance; under, over and a third pass of the 256-thread atom loop


def _rdf_positions(Rmax, seed):
    """atom 0 of every graph at the origin, the others N(0, (R / 2.15)^2 I): P(chi_3 > 2.15) = 0.2, a fifth lie beyond R"""
    pos = _randn(seed, sum(RDF_SIZES), 3) * (Rmax / 2.15)
    pos[R.bounds_of(RDF_SIZES)[:-1]] = 0.0
    return pos


def _rdf(pos, sizes, Rmax, dR, sigma, normalize, nbins=None):
    nbins = R.rdf_nbins(Rmax, dR) if nbins is None else nbins
    gpos, gp, out = Guard(pos.shape, pos), Guard(len(sizes) + 1, R.bounds_of(sizes), pad=-1, dtype=torch.int32), Guard((len(sizes), nbins))
    rc = _lib.lib().egnn_rdf(_lib.stream_ptr(), len(sizes), gpos.p, gp.p, float(Rmax), float(dR), float(sigma), int(normalize), nbins, out.p)
    _all_ok(out, inputs=(gpos, gp), what=("egnn_rdf", Rmax, dR, sigma))
    return rc, out


@pytest.mark.parametrize("Rmax,dR,sigma,nbins", [(5.0, 0.01, 5, 500), (4.0, 0.02, 3, 200), (1.0, 0.02, 12, 50), (5.12, 0.005, 0.5, 1024)])
def test_rdf_every_atom_pass_and_filter_width(Rmax, dR, sigma, nbins):
    """the default; the golden's second setting; 50 bins under a filter of half-width 48 (the reflection wraps more than twice);
    1024 bins, the limit.  Integer counts and a correctly rounded sqrtf: the curve equals the oracle to 1e-6 max(1, max |ref|),
    the bar of the golden test, graph by graph"""
    assert R.rdf_nbins(Rmax, dR) == nbins
    pos = _rdf_positions(Rmax, 80 + nbins)
    far = (pos.norm(dim=1) >= Rmax).float().mean()
    assert 0.1 < float(far) < 0.3
    rc, out = _rdf(pos, RDF_SIZES, Rmax, dR, sigma, 0)
    _lib.check(rc)
    want = R.rdf(pos, RDF_SIZES, sigma=sigma, R=Rmax, dR=dR)
    assert _biteq(out.t[0], torch.zeros(nbins, device=DEV)), "a one-atom graph has no distance"
    for g, n in enumerate(RDF_SIZES):
        _ratio("rdf", f"R{Rmax}-dR{dR}-s{sigma}-n{n}", "curve", out.t[g], want[g], 1e-6 * max(1.0, float(np.abs(want[g]).max())))
        assert n <= 2 or want[g].max() > 0


def test_rdf_normalised_and_bin_limit():
    pos = _rdf_positions(5.0, 90)
    b = R.bounds_of(RDF_SIZES)
    one = pos[b[3]:b[4]]                                                    # the 257-atom graph
    rc, out = _rdf(one, (257,), 5.0, 0.01, 5, 1)
    _lib.check(rc)
    want = R.rdf(one, (257,), normalize=True)
    assert abs(float(out.t.max()) - 1.0) <= 2.0 ** -23
    _ratio("rdf", "normalised-n257", "curve", out.t, want, 1e-6)
    # the normalised one-atom graph is 0 / 0: all-NaN, as the oracle's numpy division gives (not a value anyone should use)
    rc, nan = _rdf(pos[:1], (1,), 5.0, 0.01, 5, 1)
    _lib.check(rc)
    assert np.isnan(R.rdf(pos[:1], (1,), normalize=True)).all() and bool(torch.isnan(nan.t).all())
    # one bin too many: nbins as stats.rdf computes it
    assert R.rdf_nbins(5.125, 0.005) == 1025
    rc, out = _rdf(pos[:2], (2,), 5.125, 0.005, 0.5, 0)
    assert rc == EINVAL and out.unchanged()
    with pytest.raises(_lib.EgnnError):
        dma.stats.rdf(pos[:2].to(DEV), R=5.125, dR=0.005, sigma=0.5)


# ---- 8. sio_si_kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 2, 3])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_si_o_si_across_the_64_graph_boundary(B, A):
    """one workgroup handles 64 graphs behind a g >= B guard: B under, at and over it and a third workgroup, graphs drawn
    cyclically from the catalogue of tests/_process_ref.py (valid at 90 / 109.47 / 120 / 144 degrees; a third neighbour before,
    between, after; an O neighbour; a neighbour at exactly the cutoff; one and two atoms).  A = 1 is never valid; at A = 3 every
    second valid graph gets a neighbour typed [0, 1, 1], which is not Si."""
    pos, oh, sizes, names = R.si_o_si_batch(B, A, bad_every=2 if A == 3 else 0)
    want = R.si_o_si(pos, oh, sizes)
    gpos, goh = Guard(pos.shape, pos), Guard(oh.shape, oh, pad=1, dtype=torch.int32)
    gp, out = Guard(B + 1, R.bounds_of(sizes), pad=-1, dtype=torch.int32), Guard((B, 4))
    _lib.check(_lib.lib().egnn_si_o_si(_lib.stream_ptr(), B, A, gpos.p, goh.p, gp.p, 2.0, out.p))
    _all_ok(out, inputs=(gpos, goh, gp), what=("egnn_si_o_si", B, A))
    got = out.t.cpu().numpy()
    assert [bool(v) for v in got[:, 0] > 0.5] == [w[0] for w in want], [(n, g, w[0]) for n, g, w in zip(names, got[:, 0], want) if (g > 0.5) != w[0]]
    assert set(got[:, 0].tolist()) <= {0.0, 1.0}
    nvalid = sum(w[0] for w in want)
    assert nvalid == 0 if A == 1 else (nvalid > 0 or B == 1)
    for g, (valid, ang, l1, l2) in enumerate(want):
        if not valid:
            assert (got[g] == 0).all(), (names[g], got[g])
            continue
        assert 10.0 < ang < 170.0
        assert abs(got[g, 1] - ang) <= 2e-3, (names[g], got[g, 1], ang)
        assert abs(got[g, 2] - l1) <= 4 * R.U * l1 and abs(got[g, 3] - l2) <= 4 * R.U * l2, (names[g], got[g], l1, l2)
    if A == 2:                                                              # and the wrapper
        v, ang, ln = dma.stats.si_o_si(torch.from_numpy(pos).to(DEV), torch.from_numpy(oh).to(DEV), sizes)
        assert v.cpu().tolist() == [w[0] for w in want]

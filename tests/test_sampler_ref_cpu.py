"""Anchors of tests/_sampler_ref.py (the float64 restatement tests/test_gpu_sampler_stages.py compares the sampler's fused
kernels with), no GPU: Random123's known answers for Philox4x32-10, the oracle's reverse step and decode
(oracle/diffusion_ref.py, oracle/sampler_ref.py:62-70) and the share of ill-conditioned draws among those the GPU test makes."""
import numpy as np
import pytest
import torch

from oracle.diffusion_ref import DiffusionRef, remove_mean
from tests import _sampler_ref as R

KAT = [   # Random123 kat_vectors, philox4x32 10 rounds: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert R.philox4x32_10(ctr, key) == want
    assert tuple(int(v) for v in R.philox4x32_10_array(ctr, key)) == want


def test_array_generator_equals_the_integer_one():
    """normal4 on arrays (what the references draw from) == the scalar Philox + the fp32 uniforms + float64 Box-Muller, word by
    word; counter layout (node, slot, step, tag), key (seed lo, seed hi)"""
    seed, step = R.PHILOX_SEEDS[1], 5
    nodes, slots = np.array([0, 1, 255, 256, 1370, 2 ** 31 + 3])[:, None], np.array([0, 1, 2])[None, :]
    z, ur = R.normal4(seed, step, nodes, slots)
    assert z.shape == (6, 3, 4) and ur.shape == (6, 3, 2)
    for i, n in enumerate(nodes[:, 0]):
        for j, s in enumerate(slots[0]):
            w = R.philox4x32_10((int(n), int(s), step, 0x45474E4E), (seed & 0xFFFFFFFF, seed >> 32))
            u = [max((np.float32(r) + np.float32(0.5)) * np.float32(2.0 ** -32), np.float32(1e-37)) for r in w]
            assert all(type(v) is np.float32 for v in u)
            u = [float(v) for v in u]
            want = []
            for a, b in ((u[0], u[1]), (u[2], u[3])):
                rad = np.sqrt(-2.0 * np.log(a))
                want += [rad * np.cos(2 * np.pi * b), rad * np.sin(2 * np.pi * b)]
            assert np.array_equal(z[i, j], np.array(want)) and np.array_equal(ur[i, j], np.array([u[0], u[2]]))
    # the largest word rounds to 2^32 in fp32: u = 1 exactly, never above; the smallest gives 2^-33, far above the clamp
    assert R.uniforms([0xFFFFFFFF])[0] == np.float32(1.0) and R.uniforms([0])[0] == np.float32(2.0 ** -33)


def test_noise_layout():
    """positions: outputs 0..2 of slot 0; type column a: output a % 4 of slot 1 + a // 4; ill marks follow the radial uniform"""
    seed, step, N = R.PHILOX_SEEDS[0], 3, 40
    zp, ip = R.pos_noise(seed, step, N)
    zt, it = R.type_noise(seed, step, N, 7)
    assert zp.shape == ip.shape == (N, 3) and zt.shape == it.shape == (N, 7)
    for n in (0, 17, 39):
        z0, u0 = R.normal4(seed, step, n, 0)
        assert np.array_equal(zp[n], z0[:3])
        assert list(ip[n]) == [u0[0] > R.ILL_U, u0[0] > R.ILL_U, u0[1] > R.ILL_U]
        for a in range(7):
            z, u = R.normal4(seed, step, n, 1 + a // 4)
            assert zt[n, a] == z[a % 4] and it[n, a] == (u[(a % 4) // 2] > R.ILL_U)


def _double_oracle(T):
    """DiffusionRef with its fp32 schedule carried in float64, and the [T+1, 4] table of DiffusionRef.step_table in float64"""
    ref = DiffusionRef(0.2, 2.0, T)
    table32 = ref.step_table()
    ref.alpha_schedule = ref.alpha_schedule.double()
    ref.sigma_schedule = torch.sqrt(1 - ref.alpha_schedule ** 2)
    tab = torch.zeros(T + 1, 4, dtype=torch.float64)
    for t in range(1, T + 1):
        _, _, sq_t, _, alpha_ts, sq_ts = ref._consts(t)
        tab[t] = torch.stack([1.0 / alpha_ts, sq_ts / alpha_ts / torch.sqrt(sq_t), ref.step_std(t), torch.tensor(t / T, dtype=torch.float64)])
    a0, s0 = ref.alpha(0), ref.sigma(0)
    tab[0] = torch.stack([1.0 / a0, s0 / a0, s0 / a0, torch.tensor(0.0, dtype=torch.float64)])
    # the same layout as the oracle's own fp32 table (fp32 schedule arithmetic: a few ulp through 1 - alpha^2)
    assert torch.allclose(tab.float(), table32, rtol=1e-5, atol=1e-7)
    assert float(tab[0, 3]) == 0.0 and float(tab[T, 3]) == 1.0
    return ref, tab


@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_step_and_final_equal_the_oracle(scale):
    """step_ref / final_ref with explicit noise == DiffusionRef.reverse_diffuse_one_step and the decode lines of
    oracle/sampler_ref.py:62-70 for one graph, at float64 rounding"""
    T, n, A, C = R.T_STEPS, 7, 3, 2
    H = A + C + 1
    ref, tab = _double_oracle(T)
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ptr = np.array([0, n])
    cond = rn(n, C)
    close = lambda a, b: np.allclose(np.asarray(a), b.numpy(), rtol=1e-12, atol=1e-13)
    for t in (T, 2, 1):
        pos, x = remove_mean(rn(n, 3)), rn(n, A)
        h = torch.cat([scale * x, cond, torch.full((n, 1), t / T, dtype=torch.float64)], dim=1)
        h_out, x_out, npos, nh = rn(n, H), rn(n, 3), rn(n, 3), rn(n, A)
        want_pos = ref.reverse_diffuse_one_step(pos, remove_mean(x_out - pos), t, npos, "pos")
        want_x = ref.reverse_diffuse_one_step(h[:, :A], h_out[:, :A], t, nh, "h")
        p2, h2, bad = R.step_ref(ptr, tab, t, A, scale, 0, h_out, x_out, pos, h, [0], npos, nh)
        assert close(p2, want_pos) and close(h2[:, :A], scale * want_x)
        assert np.array_equal(h2[:, A:A + C], cond.numpy()) and (h2[:, -1] == (t - 1) / T).all() and list(bad) == [0]
    # decode (oracle/sampler_ref.py:62-70)
    pos, x = remove_mean(rn(n, 3)), rn(n, A)
    h = torch.cat([scale * x, cond, torch.zeros(n, 1, dtype=torch.float64)], dim=1)
    h_out, x_out, npos, nh = rn(n, H), rn(n, 3), rn(n, 3), rn(n, A)
    eps_x, hh, eps_h = remove_mean(x_out - pos), h[:, :A], h_out[:, :A]
    a0, s0 = ref.alpha(0), ref.sigma(0)
    want_pos = pos / a0 - s0 * eps_x / a0 + s0 * remove_mean(npos) / a0
    want_hc = hh / a0 - s0 * eps_h / a0 + s0 * nh / a0
    want_oh = torch.nn.functional.one_hot(torch.argmax(want_hc, dim=1), num_classes=A)
    po, hc, oh, bad = R.final_ref(ptr, tab, A, 0, h_out, x_out, pos, h, [0], npos, nh)
    assert close(po, want_pos) and close(hc, want_hc) and np.array_equal(oh, want_oh.numpy()) and list(bad) == [0]


def test_init_ref_layout_and_flags():
    T, A, C = R.T_STEPS, 5, 2
    H = A + C + 1
    _, tab = _double_oracle(T)
    ptr = np.array([0, 1, 4, 9])
    g = torch.Generator().manual_seed(3)
    cond, p0, x0 = (torch.randn(9, k, generator=g) for k in (C, 3, A))
    pos, h, bad = R.init_ref(ptr, tab, T, H, A, 3.0, 0, cond, p0, x0)
    assert (pos[0] == 0).all() and np.abs(pos[1:4].sum(0)).max() < 1e-15 and np.abs(pos[4:].sum(0)).max() < 1e-15
    assert np.array_equal(h[:, :A], 3.0 * x0.double().numpy()) and np.array_equal(h[:, A:A + C], cond.double().numpy())
    assert (h[:, -1] == 1.0).all() and list(bad) == [0, 0, 0]
    # generator form: the raw normals of step T + 1
    pos, h, _ = R.init_ref(ptr, tab, T, H, A, 3.0, 99)
    assert np.array_equal(h[:, :A], 3.0 * R.type_noise(99, T + 1, 9, A)[0])
    z = R.pos_noise(99, T + 1, 9)[0]
    assert np.allclose(pos[1:4], z[1:4] - z[1:4].sum(0) / 3, rtol=0, atol=1e-15)
    # a non-finite input flags its own graph only, stays flagged, and the one-hot of a tie sits on the first maximum
    h_out, x_out = np.zeros((9, H)), np.zeros((9, 3))
    x_out[2, 1] = np.inf
    p2, h2, bad = R.step_ref(ptr, tab, 3, A, 3.0, 99, h_out, x_out, pos, h, [0, 0, 0])
    assert list(bad) == [0, 1, 0] and np.isfinite(p2[0]).all() and np.isfinite(p2[4:]).all() and not np.isfinite(p2[1:4, 1]).any()
    h_out[7, 0] = np.nan
    _, _, bad = R.step_ref(ptr, tab, 2, A, 3.0, 99, h_out, np.zeros((9, 3)), pos, h, bad)
    assert list(bad) == [0, 1, 1]
    assert list(R.first_argmax(np.array([[1.0, 2.0, 2.0], [5.0, 5.0, 5.0], [np.nan, 1.0, 1.0], [np.nan, np.nan, np.nan],
                                         [-np.inf, -np.inf, -np.inf]]))) == [1, 0, 1, 0, 0]


def test_share_of_ill_conditioned_draws_among_the_gpu_tests_draws():
    """Every draw tests/test_gpu_sampler_stages.py makes with the device generator: both seeds, steps T + 1 (init), the reverse
    steps and 0 (decode), all nodes of the batch, slot 0 (positions) and the type slots of every A.  The draws whose radial uniform
    lies above 1 - 2^-10 (expected share 2^-10) stay under the 0.5 % cap in every comparison the GPU test makes, and none falls
    into the position draws of the graphs below 255 atoms (where one draw moves the graph's mean visibly)."""
    N = sum(R.SIZES)
    small = sum(s for s in R.SIZES if s < 255)
    assert list(R.SIZES[:2]) == [1, 2] and small == 3          # the small graphs come first
    tot = ill = 0
    for seed in R.PHILOX_SEEDS:
        for step in (R.T_STEPS + 1,) + R.STEP_TS + (0,):
            _, ip = R.pos_noise(seed, step, N)
            assert ip.mean() <= R.ILL_CAP, (seed, step)
            assert not ip[:small].any(), (seed, step)
            tot, ill = tot + ip.size, ill + int(ip.sum())
            for A in R.PHILOX_A:
                _, it = R.type_noise(seed, step, N, A)
                assert it.mean() <= R.ILL_CAP, (seed, step, A)
                tot, ill = tot + it.size, ill + int(it.sum())
    print(f"ill-conditioned draws: {ill} of {tot} ({ill / tot:.3%})")
    assert 0 < ill <= R.ILL_CAP * tot

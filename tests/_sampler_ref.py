"""float64 restatement of the sampler's fused kernels (csrc/sampler.hip: sampler_init_kernel, sampler_step_kernel,
sampler_final_kernel and the Philox4x32-10 / Box-Muller generator normal4) in plain numpy -- test infrastructure, no GPU.

The contract restated (one workgroup per graph on the device, one vectorised pass here):

  init   pos = z - mean_g(z);  h = [scale * x | cond | table[T][3]];  bad[g] = 0
  step   eps = (x_out - pos) - mean_g(x_out - pos)
         pos <- (pos c0 - eps c1) + c2 (z - mean_g(z))
         h[:, :A] <- scale ((h[:, :A] c0 - h_out[:, :A] c1) + c2 z_h);  h[:, H-1] <- table[t-1][3]
         with (c0, c1, c2) = table[t][:3]
  final  pos_out = (pos ia - sa eps) + sa (z - mean_g(z));  hc = (h[:, :A] ia - sa h_out[:, :A]) + sa z_h
         with (ia, sa) = table[0][:2];  one-hot on the FIRST maximum of hc
  bad[g] is set (never cleared, except by init) iff a new value of graph g is non-finite.

Noise is the caller's array where one is given, else normal4(seed, step, node, slot): the positions take outputs 0..2 of
slot 0, the type columns 4k..4k+3 the four outputs of slot 1 + k; step = T + 1 for init, t for a reverse step, 0 for the decode.
``table`` is the [T+1, 4] step table of E3DiffusionProcess.step_table() (any float dtype; the arithmetic is float64).

tests/test_sampler_ref_cpu.py ties this file to Random123's known answers and to oracle/diffusion_ref.py;
tests/test_gpu_sampler_stages.py compares the kernels with it.
"""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57            # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # key bumps (Weyl sequence)
TAG = 0x45474E4E                           # the fourth counter word of every sampler draw
MASK = 0xFFFFFFFF
ILL_U = 1.0 - 2.0 ** -10                   # a radial uniform above this makes log(u) ill-conditioned
TWO_PI = 2.0 * math.pi

# ---- the shapes the GPU tests use (shared with the CPU test, which bounds the ill-conditioned share on exactly these draws) ----
SIZES = (1, 2, 255, 256, 257, 600)         # single atom; under / at / over one pass of the 256-thread node loop; a third pass
T_STEPS = 6                                # E3DiffusionProcess(0.2, 2.0, 6)
STEP_TS = (T_STEPS, 2, 1)                  # the reverse steps every chain runs
PHILOX_A = (2, 5, 8)
PHILOX_SEEDS = (20240611, 0x9E3779B97F4A7C15)   # the second has a non-zero high word
ILL_CAP = 0.005                            # at most 0.5 % of the draws may be left out as ill-conditioned (expected: 2^-10)


def philox4x32_10(ctr, key):
    """Philox4x32-10 on Python integers: ctr = (x, y, z, w), key = (k0, k1) -> 4 words.  The round function of sampler.hip."""
    x, y, z, w = (int(v) & MASK for v in ctr)
    k0, k1 = (int(v) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * x, M1 * z
        x, y, z, w = (p1 >> 32) ^ y ^ k0, p1 & MASK, (p0 >> 32) ^ w ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return x, y, z, w


def philox4x32_10_array(ctr, key):
    """the same on uint64 arrays (32-bit values; a 32 x 32 product fits): ctr = 4 broadcastable arrays -> [..., 4] uint64"""
    x, y, z, w = np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in ctr])
    k0, k1 = np.uint64(int(key[0]) & MASK), np.uint64(int(key[1]) & MASK)
    m, s32 = np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * x, np.uint64(M1) * z
        x, y, z, w = (p1 >> s32) ^ y ^ k0, p1 & m, (p0 >> s32) ^ w ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return np.stack([x, y, z, w], axis=-1)


def uniforms(words):
    """the kernel's fp32 uniforms: ((float)r + 0.5f) * 2^-32, clamped at 1e-37 (float32 in, float32 out, every step rounded)"""
    r = np.asarray(words, dtype=np.uint64).astype(np.uint32).astype(np.float32)
    u = (r + np.float32(0.5)) * np.float32(2.0 ** -32)
    return np.maximum(u, np.float32(1e-37))


def normal4(seed, step, node, slot):
    """four N(0, 1) draws for (seed, step, node, slot); ``node`` and ``slot`` may be (broadcastable) arrays.
    -> (z [..., 4] float64, radial uniforms [..., 2] float64).  Counter (node, slot, step, TAG), key (seed lo, seed hi);
    Box-Muller in float64 on the fp32 uniforms: (u0, u1) -> z0 = r cos, z1 = r sin; (u2, u3) -> z2, z3."""
    seed = int(seed)
    words = philox4x32_10_array((node, slot, int(step), TAG), (seed & MASK, (seed >> 32) & MASK))
    u = uniforms(words).astype(np.float64)
    r0, r1 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    a0, a1 = TWO_PI * u[..., 1], TWO_PI * u[..., 3]
    z = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)
    return z, np.stack([u[..., 0], u[..., 2]], axis=-1)


def pos_noise(seed, step, N):
    """-> (z [N, 3], ill [N, 3] bool): outputs 0..2 of slot 0; ill marks the draws whose radial uniform is ill-conditioned"""
    z, ur = normal4(seed, step, np.arange(N), 0)
    ill = ur > ILL_U
    return z[:, :3], np.stack([ill[:, 0], ill[:, 0], ill[:, 1]], axis=-1)


def type_noise(seed, step, N, A):
    """-> (z [N, A], ill [N, A] bool): columns 4k..4k+3 are the four outputs of slot 1 + k"""
    nslot = (A + 3) // 4
    z, ur = normal4(seed, step, np.arange(N)[:, None], 1 + np.arange(nslot)[None, :])     # [N, nslot, 4], [N, nslot, 2]
    ill = np.repeat(ur > ILL_U, 2, axis=-1)                                               # outputs (0, 1) <- u0, (2, 3) <- u2
    return z.reshape(N, 4 * nslot)[:, :A], ill.reshape(N, 4 * nslot)[:, :A]


# ---- the three kernels ------------------------------------------------------------------------------------------------------
def f64(a):
    """float64 numpy copy of an array or a (device) tensor"""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.array(a, dtype=np.float64)


def _graphs(graph_ptr):
    ptr = np.asarray(graph_ptr.detach().cpu().numpy() if hasattr(graph_ptr, "detach") else graph_ptr, dtype=np.int64)
    cnt = np.diff(ptr)
    assert ptr[0] == 0 and (cnt > 0).all()
    return ptr, cnt, np.repeat(np.arange(len(cnt)), cnt)


def graph_mean(v, ptr, cnt, gi):
    """per-graph mean of the rows of v, broadcast back to the rows"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.add.reduceat(v, ptr[:-1], axis=0) / cnt[:, None])[gi]


def _flag(bad, gi, *new):
    out = np.array(bad, dtype=np.int64)
    for v in new:
        rows = ~np.isfinite(v).all(axis=1)
        out[np.unique(gi[rows])] = 1
    return out


def init_ref(graph_ptr, table, T, H, A, scale, seed, cond=None, pos_init=None, x_init=None):
    """-> (pos [N, 3], h [N, H], bad [B])"""
    ptr, cnt, gi = _graphs(graph_ptr)
    N, C = int(ptr[-1]), H - A - 1
    table = f64(table).reshape(-1, 4)
    z = f64(pos_init) if pos_init is not None else pos_noise(seed, T + 1, N)[0]
    x = f64(x_init) if x_init is not None else type_noise(seed, T + 1, N, A)[0]
    h = np.empty((N, H))
    h[:, :A] = float(scale) * x
    if C > 0:
        h[:, A:A + C] = f64(cond)
    h[:, H - 1] = table[T, 3]
    return z - graph_mean(z, ptr, cnt, gi), h, np.zeros(len(cnt), dtype=np.int64)


def step_ref(graph_ptr, table, t, A, scale, seed, h_out, x_out, pos, h, bad, noise_pos=None, noise_h=None):
    """one reverse step t -> t - 1 on float64 copies -> (pos, h, bad)"""
    ptr, cnt, gi = _graphs(graph_ptr)
    N = int(ptr[-1])
    table = f64(table).reshape(-1, 4)
    c0, c1, c2 = table[t, :3]
    pos, h, h_out, x_out = f64(pos), f64(h), f64(h_out), f64(x_out)
    z = f64(noise_pos) if noise_pos is not None else pos_noise(seed, t, N)[0]
    zh = f64(noise_h) if noise_h is not None else type_noise(seed, t, N, A)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        e = x_out - pos
        eps = e - graph_mean(e, ptr, cnt, gi)
        new_pos = (pos * c0 - eps * c1) + c2 * (z - graph_mean(z, ptr, cnt, gi))
        v = (h[:, :A] * c0 - h_out[:, :A] * c1) + c2 * zh
        new_h = h.copy()
        new_h[:, :A] = float(scale) * v
    new_h[:, -1] = table[t - 1, 3]
    return new_pos, new_h, _flag(bad, gi, new_pos, v)


def first_argmax(v):
    """the kernel's rule: the first column that exceeds every earlier one, starting from -inf (a NaN never exceeds)"""
    return np.argmax(np.where(np.isnan(v), -np.inf, v), axis=1)


def final_ref(graph_ptr, table, A, seed, h_out, x_out, pos, h, bad, noise_pos=None, noise_h=None):
    """the t = 0 decode -> (pos_out [N, 3], hc [N, A], one-hot [N, A] int, bad); the state itself is not changed"""
    ptr, cnt, gi = _graphs(graph_ptr)
    N = int(ptr[-1])
    table = f64(table).reshape(-1, 4)
    ia, sa = table[0, 0], table[0, 1]
    pos, h, h_out, x_out = f64(pos), f64(h), f64(h_out), f64(x_out)
    z = f64(noise_pos) if noise_pos is not None else pos_noise(seed, 0, N)[0]
    zh = f64(noise_h) if noise_h is not None else type_noise(seed, 0, N, A)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        e = x_out - pos
        eps = e - graph_mean(e, ptr, cnt, gi)
        pos_out = (pos * ia - sa * eps) + sa * (z - graph_mean(z, ptr, cnt, gi))
        hc = (h[:, :A] * ia - sa * h_out[:, :A]) + sa * zh
    onehot = (np.arange(A)[None, :] == first_argmax(hc)[:, None]).astype(np.int64)
    return pos_out, hc, onehot, _flag(bad, gi, pos_out, hc)

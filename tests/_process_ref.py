"""Restatements of the kernels around the network -- the diffusion-process arithmetic (csrc/sampler.hip: center_kernel,
slice_cols_kernel, reverse_step_kernel), the two small networks (csrc/aux_mlp.hip: gamma_tilde_kernel, dense_rows_kernel) and
the graph builders and evaluation scores (csrc/graph_stats.hip) -- in plain numpy: test infrastructure, no GPU.

Values are float64 computed from the fp32 values the device reads; the radius graph is exact float32 in the kernel's operation
order; RDF and the Si-O-Si selector are thin wrappers over oracle/aux_ref.py (pinned by tests/golden/stats_golden.npz).
Every value function has a bound function beside it: the first-order rounding bound of the kernel's fp32 arithmetic, made of the
precision of the format (U = 2^-24, half an ulp) and the number of roundings on the longest path, never of a device result.

tests/test_process_ref_cpu.py ties this file to the oracle; tests/test_gpu_process_kernels.py compares the kernels with it.
"""
import math

import numpy as np
import torch

from oracle import aux_ref

U = 2.0 ** -24                              # unit roundoff of fp32
SIZES = (1, 2, 255, 256, 257, 600)          # the sampler-stage batch: one atom; under / at / over one 256-thread pass; a third pass
THREADS = 256                               # kThreads of csrc/common.h: the node loop's stride and the width of block_sum3
TREE_LEVELS = 8                             # log2(THREADS): the levels of block_sum3's tree
OPS = 8                                     # roundings granted to a softplus / sigmoid chain (expf, log1pf: few-ulp functions)


def f64(a):
    """float64 numpy copy of an array or a (device) tensor"""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.array(a, dtype=np.float64)


def bounds_of(sizes):
    return [0] + [int(v) for v in np.cumsum(list(sizes))]


def _ranges(graph_ptr, N):
    """[(lo, hi)] of every graph; one range over all rows without a graph_ptr"""
    if graph_ptr is None:
        return [(0, N)]
    ptr = [int(v) for v in (graph_ptr.detach().cpu().numpy() if hasattr(graph_ptr, "detach") else np.asarray(graph_ptr))]
    assert ptr[0] == 0 and ptr[-1] == N and all(b > a for a, b in zip(ptr, ptr[1:]))
    return list(zip(ptr[:-1], ptr[1:]))


def sum_roundings(cnt):
    """K of the bounds: the roundings on the longest path of a block-wide sum over cnt rows -- the serial adds of one thread
    (ceil(cnt / 256)) plus the eight levels of block_sum3's tree"""
    return -(-int(cnt) // THREADS) + TREE_LEVELS


def mean_and_error(v, graph_ptr=None):
    """v float64 [N, D] -> (mean broadcast to the rows, bound of the fp32 sum's error / cnt): K U sum_n |v_n| / cnt"""
    mean, err = np.empty_like(v), np.empty_like(v)
    for lo, hi in _ranges(graph_ptr, v.shape[0]):
        mean[lo:hi] = v[lo:hi].mean(axis=0)
        err[lo:hi] = sum_roundings(hi - lo) * U * np.abs(v[lo:hi]).sum(axis=0) / (hi - lo)
    return mean, err


# ---- center_kernel ---------------------------------------------------------------------------------------------------------
def center(a, b=None, graph_ptr=None):
    """out[n][d] = (a[n][d] - b[n][d]) - mean over the graph (over all rows without graph_ptr); b None = 0"""
    v = f64(a) - (0.0 if b is None else f64(b))
    return v - mean_and_error(v, graph_ptr)[0]


def center_bound(a, b=None, graph_ptr=None):
    """per element: U (|a| + |b| + |a - b| + |mean| + |out|) + K U sum_n |a_n - b_n| / cnt -- the difference, the division and
    the final subtraction round once each (|a| + |b| is slack), the sum K times"""
    a = f64(a)
    b = np.zeros_like(a) if b is None else f64(b)
    v = a - b
    mean, err = mean_and_error(v, graph_ptr)
    return U * (np.abs(a) + np.abs(b) + np.abs(v) + np.abs(mean) + np.abs(v - mean)) + err


# ---- reverse_step_kernel ---------------------------------------------------------------------------------------------------
def reverse_step(z, eps, noise, c0, c1, c2, mode_pos, graph_ptr=None):
    """z_out = (z c0 - eps c1) + c2 (noise - m), m = the graph's (or global) mean of noise where mode_pos, else 0.
    z [N, D] already cut out of its strided buffer; c0, c1, c2 the fp32 values the kernel receives."""
    z, eps, noise = f64(z), f64(eps), f64(noise)
    m = mean_and_error(noise, graph_ptr)[0] if mode_pos else 0.0
    return (z * float(c0) - eps * float(c1)) + float(c2) * (noise - m)


def reverse_step_bound(z, eps, noise, c0, c1, c2, mode_pos, graph_ptr=None):
    """4 U (|z c0| + |eps c1| + |c2| (|noise| + |m|)) for the element's own roundings (two products, the difference, noise - m,
    the product with c2, the final sum: at most three on any one term, the fourth is slack) + |c2| times the mean's error"""
    z, eps, noise = f64(z), f64(eps), f64(noise)
    c0, c1, c2 = abs(float(c0)), abs(float(c1)), abs(float(c2))
    m, err = mean_and_error(noise, graph_ptr) if mode_pos else (np.zeros_like(noise), np.zeros_like(noise))
    return 4 * U * (np.abs(z) * c0 + np.abs(eps) * c1 + c2 * (np.abs(noise) + np.abs(m))) + c2 * err


# ---- gamma_tilde_kernel ----------------------------------------------------------------------------------------------------
def softplus(x):
    """torch's threshold form, x > 20 ? x : log1p(exp(x)), in float64"""
    x = f64(x)
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def _gamma_parts(t, w1, w2, w3):
    t, s1 = f64(t).reshape(-1, 1), float(softplus(f64(w1).reshape(-1)[:1])[0])
    arg = softplus(f64(w2).reshape(1, -1)) * (s1 * t)                      # [n, hidden]
    term = softplus(f64(w3).reshape(1, -1)) / (1.0 + np.exp(-arg))
    return s1 * t[:, 0] + term.sum(axis=1), arg, term


def gamma_tilde(t, w1, w2, w3):
    """out[i] = sp(w1) t_i + sum_k sp(w3[k]) sigmoid(sp(w2[k]) sp(w1) t_i); w1 [1], w2 / w3 [hidden] the RAW parameters"""
    return _gamma_parts(t, w1, w2, w3)[0]


def gamma_tilde_bound(t, w1, w2, w3):
    """per output: U [(K + 1) sum |term_k| + sum (OPS + 3 |arg_k|) |term_k| + 2 |out|], K = ceil(hidden / 256) + 8: the sum's
    roundings (+ 1: the product that makes a term), OPS for the term's two softplus / one sigmoid chains, 3 |arg_k| for the
    relative error of the sigmoid's argument (d sigmoid / sigmoid <= |arg| d arg / arg), l1 and the final sum on |out|"""
    out, arg, term = _gamma_parts(t, w1, w2, w3)
    K = -(-term.shape[1] // THREADS) + TREE_LEVELS
    return U * ((K + 1) * np.abs(term).sum(axis=1) + ((OPS + 3 * np.abs(arg)) * np.abs(term)).sum(axis=1) + 2 * np.abs(out))


# ---- dense_rows_kernel -----------------------------------------------------------------------------------------------------
def dense_rows(x, W, b, relu):
    """out [N, J] = act(b + x W^T), W in nn.Linear layout [J, K]"""
    out = f64(b)[None, :] + f64(x) @ f64(W).T
    return np.maximum(out, 0.0) if relu else out


def dense_rows_bound(x, W, b):
    """(K + 1) U (|b_j| + sum_k |x_k W_jk|): one fmaf rounding per k on a partial sum that never exceeds the sum of magnitudes"""
    x, W = f64(x), f64(W)
    return (x.shape[1] + 1) * U * (np.abs(f64(b))[None, :] + np.abs(x) @ np.abs(W).T)


# ---- radius_count_kernel / radius_fill_kernel ------------------------------------------------------------------------------
def radius_edges(x, sizes, r):
    """-> (deg int32 [N], edge_dst int32 [E], edge_src int32 [E]): i ascending, inside a row j ascending, j != i, same graph, and
    ((dx*dx + dy*dy) + dz*dz) < float32(r) * float32(r) with dx = x_i - x_j, every operation rounded to float32 (the library is
    built without contraction and without fast-math)"""
    x = np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x)
    assert x.dtype == np.float32
    r2 = np.float32(r) * np.float32(r)
    assert r2.dtype == np.float32
    deg, dst, src = [], [], []
    for lo, hi in zip(bounds_of(sizes)[:-1], bounds_of(sizes)[1:]):
        p = x[lo:hi]
        dx, dy, dz = (p[:, None, k] - p[None, :, k] for k in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        m = (d2 < r2) & ~np.eye(hi - lo, dtype=bool)
        i, j = np.nonzero(m)                                               # row-major: i ascending, then j ascending
        deg.append(m.sum(axis=1))
        dst.append(i + lo)
        src.append(j + lo)
    return tuple(np.concatenate(v).astype(np.int32) for v in (deg, dst, src))


# ---- rdf_kernel / sio_si_kernel: oracle/aux_ref.py -------------------------------------------------------------------------
def rdf_nbins(R, dR):
    """the number of bins as stats.rdf counts them"""
    return len(np.arange(0 + dR, R + dR, dR))


def rdf(pos, sizes, sigma=5, R=5.0, dR=0.01, normalize=False):
    """-> float64 [B, nbins]: aux_ref.rdf_about_atom0 graph by graph (a normalised all-zero curve is 0 / 0 = NaN, as numpy gives)"""
    pos = torch.as_tensor(pos.detach().cpu() if hasattr(pos, "detach") else pos, dtype=torch.float32)
    b = bounds_of(sizes)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.stack([aux_ref.rdf_about_atom0(pos[lo:hi], sigma=sigma, R=R, dR=dR, normalize=normalize) for lo, hi in zip(b[:-1], b[1:])])


def si_o_si(pos, onehot, sizes, cutoff=2.0):
    """-> [(valid, angle in degrees, length 1, length 2)] per graph from aux_ref.select_si_o_si / angle_cn2 / bond_lengths_cn2.
    The oracle compares a row with [0, 1] (two columns).  The kernel's rule for A columns is `column 1 set, every other column
    0`, never with A = 1; it is restated by handing the oracle a two-column surrogate, [0, 1] where that rule holds and [1, 0]
    elsewhere -- the rows themselves at A = 2."""
    pos = torch.as_tensor(pos.detach().cpu() if hasattr(pos, "detach") else pos, dtype=torch.float32)
    oh = torch.as_tensor(onehot.detach().cpu() if hasattr(onehot, "detach") else onehot).long()
    A = oh.shape[1]
    want = torch.tensor([1 if a == 1 else 0 for a in range(A)])
    si = (oh == want).all(dim=1) if A >= 2 else torch.zeros(oh.shape[0], dtype=torch.bool)
    two = torch.stack((~si, si), dim=1).long()
    out, b = [], bounds_of(sizes)
    for lo, hi in zip(b[:-1], b[1:]):
        sel = aux_ref.select_si_o_si(pos[lo:hi], two[lo:hi], cutoff=cutoff)
        if sel is None:
            out.append((False, 0.0, 0.0, 0.0))
        else:
            out.append((True, aux_ref.angle_cn2(sel)) + tuple(aux_ref.bond_lengths_cn2(sel)))
    return out


# ---- the Si-O-Si catalogue (shared with the CPU test, which checks what each entry is meant to be) -------------------------
def _bent(angle_deg, l1=1.62, l2=1.6):
    a = math.radians(angle_deg)
    return [[0.0, 0.0, 0.0], [l1, 0.0, 0.0], [l2 * math.cos(a), l2 * math.sin(a), 0.0]]


FAR = [4.0, 4.0, 4.0]
THIRD = [0.0, 0.0, 1.5]                      # a third neighbour inside the cutoff
SI, OX = 1, 0                                # type codes: Si = column 1 set alone; O = column 0 set alone
SI_BAD = 2                                   # A = 3 only: [0, 1, 1] (column 1 set, but not alone)
# name -> (positions, type codes, valid at A >= 2)
CATALOGUE = {
    "valid90": (_bent(90.0) + [FAR], [OX, SI, SI, OX], True),
    "valid109": (_bent(109.47) + [FAR], [OX, SI, SI, SI], True),
    "valid144": (_bent(144.0), [OX, SI, SI], True),
    "valid_far_between": ([_bent(120.0)[0], _bent(120.0)[1], FAR, _bent(120.0)[2]], [OX, SI, OX, SI], True),
    "third_before": ([[0.0, 0.0, 0.0], THIRD] + _bent(90.0)[1:], [OX, SI, SI, SI], False),
    "third_between": ([[0.0, 0.0, 0.0], _bent(90.0)[1], THIRD, _bent(90.0)[2]], [OX, SI, SI, SI], False),
    "third_after": (_bent(90.0) + [THIRD], [OX, SI, SI, SI], False),
    "o_neighbour": (_bent(109.47), [OX, SI, OX], False),
    "at_cutoff": ([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 1.6, 0.0]], [OX, SI, SI], False),      # |(2, 0, 0)| = 2.0 is not < 2.0
    "one_atom": ([[0.5, -0.25, 1.0]], [OX], False),
    "two_atoms": ([[0.0, 0.0, 0.0], [1.6, 0.0, 0.0]], [OX, SI], False),
}
CATALOGUE_ORDER = ("valid90", "third_before", "valid109", "o_neighbour", "one_atom", "valid144", "at_cutoff", "third_between",
                   "two_atoms", "valid_far_between", "third_after")


def si_o_si_batch(B, A, bad_every=0):
    """B graphs drawn cyclically from the catalogue (11 entries: coprime with 64, so valid and invalid graphs interleave
    differently on each side of a 64-graph boundary) -> (pos float32 [N, 3], onehot int32 [N, A], sizes, names).  Graph g is
    shifted by a small exactly-representable offset so no two graphs share coordinates.  bad_every > 0 (A = 3): every
    bad_every-th VALID graph gets its first Si neighbour typed [0, 1, 1], which makes it invalid."""
    pos, oh, sizes, names, nvalid = [], [], [], [], 0
    for g in range(B):
        name = CATALOGUE_ORDER[g % len(CATALOGUE_ORDER)]
        p, types, valid = CATALOGUE[name]
        types = list(types)
        if bad_every and valid:
            nvalid += 1
            if nvalid % bad_every == 0:
                types[types.index(SI)] = SI_BAD
                name += "+bad_si"
        shift = np.array([0.25 * (g % 5), -0.5 * (g % 3), 0.125 * (g % 7)])
        pos.append(np.asarray(p, dtype=np.float64) + shift)
        for tcode in types:
            row = [0] * A
            if tcode == OX:
                row[0] = 1
            elif A >= 2:
                row[1] = 1
                if tcode == SI_BAD:
                    assert A >= 3
                    row[2] = 1
            oh.append(row)
        sizes.append(len(types))
        names.append(name)
    return np.concatenate(pos).astype(np.float32), np.asarray(oh, dtype=np.int32).reshape(-1, A), sizes, names


# ---- the radius-graph inputs (shared with the CPU test, which proves the properties claimed here) --------------------------
def min_gap_to_radius(x, sizes, r):
    """the smallest | |x_i - x_j| - r | over the pairs of every graph, in float64"""
    x, best, b = f64(x), np.inf, bounds_of(sizes)
    for lo, hi in zip(b[:-1], b[1:]):
        if hi - lo > 1:
            d = np.sqrt(((x[lo:hi, None, :] - x[None, lo:hi, :]) ** 2).sum(-1))[np.triu_indices(hi - lo, 1)]
            best = min(best, float(np.abs(d - r).min()))
    return best


def _random_positions(sizes, r, box):
    """uniform positions in [0, box)^3 from the first seed that leaves no pair within 1e-4 of r (so that a float64 brute force
    and the float32 rule agree: tests/test_process_ref_cpu.py)"""
    for seed in range(64):
        x = (torch.rand(sum(sizes), 3, generator=torch.Generator().manual_seed(seed)) * box).numpy()
        if min_gap_to_radius(x, sizes, r) > 1e-4:
            return x
    raise AssertionError("no seed below 64 keeps every pair 1e-4 away from r")


def _lattice(n):
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def radius_cases():
    """name -> (x float32 [N, 3], sizes, r)"""
    far = 10.0 * _lattice(2)[:5]                                            # five atoms 10 apart: a graph without an edge
    dense = _random_positions([30], 2.2, 4.0)
    dup = _random_positions([20], 1.5, 3.0)
    return {
        "random": (_random_positions([40, 130, 7, 1], 2.2, 6.0), [40, 130, 7, 1], 2.2),
        "N127": (_random_positions([60, 67], 2.0, 5.0), [60, 67], 2.0),       # one block of 128 threads, one idle
        "N128": (_random_positions([64, 64], 2.0, 5.0), [64, 64], 2.0),       # exactly one block
        "N129": (_random_positions([128, 1], 2.0, 6.0), [128, 1], 2.0),       # a second block for a single one-atom graph
        # integer coordinates: every d^2 is an exact integer, so the pairs at d^2 = 4 = r^2 are ties (absent) and d^2 = 3 present
        "lattice": (np.concatenate([_lattice(4), _lattice(3) + np.float32(7.0)]), [64, 27], 2.0),
        "duplicates": (np.concatenate([dup, dup[:10], dup[:5]]).astype(np.float32), [35], 1.5),   # d = 0 counts, j != i
        "one_empty_graph": (np.concatenate([dense, far, dense + np.float32(1.0)]).astype(np.float32), [30, 5, 30], 2.2),
        "no_edges": (np.concatenate([far, far[:3]]).astype(np.float32), [5, 3], 2.2),
    }

"""Acceptance statistics of sampled structures on the device: RDF about the excited O
(atom 0) with its similarity metrics cos / L2 / MSE / Wasserstein (evaluate_RDF.py:13-83) and the Si-O-Si angle / bond-length comparison
with R^2 (evaluate_Si-O-Si.py:23-53, CN2_evaluate.py:12-37)."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import _lib
from ._batch import block_index, typed_batch


def _graph_ptr(sizes, device):
    sz = torch.as_tensor(list(sizes), dtype=torch.long)
    gp = torch.zeros(sz.numel() + 1, dtype=torch.int64)
    gp[1:] = torch.cumsum(sz, 0)
    return gp.to(torch.int32).to(device), int(sz.numel()), int(sz.sum())


def rdf(position: torch.Tensor, sizes: Sequence[int] | None = None, sigma=5, R=5.0, dR=0.01, Normalize=False) -> torch.Tensor:
    """RDF(position, sigma, R, dR, Normalize) of evaluate_RDF.py:48-60 for one graph ([n,3] -> [nbins]) or a
    batch of graphs (``sizes`` given: [N,3] -> [B, nbins])."""
    if not position.is_cuda:
        raise RuntimeError("rdf needs a CUDA(ROCm) tensor; there is no CPU fallback")
    single = sizes is None
    if single:
        sizes = [position.shape[0]]
    gp, B, N = _graph_ptr(sizes, position.device)
    if position.shape != (N, 3):
        raise ValueError("position must be [sum(sizes), 3]")
    nbins = _nbins(R, dR)
    pos = position.detach().to(torch.float32).contiguous()
    out = torch.empty(B, nbins, device=position.device)
    _lib.check(_lib.lib().egnn_rdf(_lib.stream_ptr(), B, _lib.ptr(pos), _lib.ptr(gp), float(R), float(dR), float(sigma),
                                   1 if Normalize else 0, nbins, _lib.ptr(out)))
    return out[0] if single else out


def cos_similarity(a, b):
    """evaluate_RDF.py:62-63"""
    a, b = _np(a), _np(b)
    return float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))


def _np(a):
    return a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)


def rdf_l2(a, b):
    """euclidean_distance(a, b) of evaluate_RDF.py:82-83 (the L2 the reference ranks RDF pairs by, :105-123)"""
    return float(np.linalg.norm(_np(a) - _np(b)))


def wasserstein(a, b):
    """calculate_wasserstein_distance(rdf1, rdf2) of evaluate_RDF.py:13-24 = scipy.stats.wasserstein_distance(u_values,
    v_values): the two arrays are taken as SAMPLES of two 1-D distributions (the RDF values themselves, not weights
    over r), W1 = integral |U(x) - V(x)| dx over the merged support; for equal lengths mean |sort(a) - sort(b)|.
    Tensors stay on their device (sort + searchsorted), numpy inputs are computed on the host."""
    if torch.is_tensor(a) or torch.is_tensor(b):
        dev = a.device if torch.is_tensor(a) else b.device
        u = torch.as_tensor(a, device=dev).double().reshape(-1).sort().values
        v = torch.as_tensor(b, device=dev).double().reshape(-1).sort().values
        allv = torch.cat((u, v)).sort().values
        deltas = allv[1:] - allv[:-1]
        ucdf = torch.searchsorted(u, allv[:-1], right=True).double() / u.numel()
        vcdf = torch.searchsorted(v, allv[:-1], right=True).double() / v.numel()
        return float(((ucdf - vcdf).abs() * deltas).sum())
    u, v = np.sort(_np(a).reshape(-1)), np.sort(_np(b).reshape(-1))
    allv = np.sort(np.concatenate((u, v)))
    deltas = np.diff(allv)
    ucdf = np.searchsorted(u, allv[:-1], side="right") / u.size
    vcdf = np.searchsorted(v, allv[:-1], side="right") / v.size
    return float(np.sum(np.abs(ucdf - vcdf) * deltas))


def rdf_mse(a, b):
    """mean_squared_error(rdf1, rdf2) of evaluate_RDF.py:26-37"""
    return float(np.mean((_np(a) - _np(b)) ** 2))


def si_o_si(position: torch.Tensor, onehot: torch.Tensor, sizes: Sequence[int], cutoff=2.0):
    """Per graph: atoms within ``cutoff`` of atom 0; valid iff exactly two, both Si (one-hot [0,1])
    (evaluate_Si-O-Si.py:23-41).  Returns (valid bool [B], angle_deg [B], mean_bond_length [B]) as in
    :42-50 (angle of CN2_evaluate.py:12-16, lengths :18-21)."""
    if not position.is_cuda:
        raise RuntimeError("si_o_si needs CUDA(ROCm) tensors; there is no CPU fallback")
    gp, B, N = _graph_ptr(sizes, position.device)
    pos = position.detach().to(torch.float32).contiguous()
    oh = onehot.detach().to(position.device).to(torch.int32).contiguous()
    out = torch.empty(B, 4, device=position.device)
    _lib.check(_lib.lib().egnn_si_o_si(_lib.stream_ptr(), B, int(oh.shape[1]), _lib.ptr(pos), _lib.ptr(oh), _lib.ptr(gp),
                                       float(cutoff), _lib.ptr(out)))
    return out[:, 0] > 0.5, out[:, 1], 0.5 * (out[:, 2] + out[:, 3])


def r2score(a, b) -> float:
    """CN2_evaluate.py:23-37: R^2 of the least-squares line b ~ a."""
    x, y = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    mx, my = x.mean(), y.mean()
    txx, tyy, txy = ((x - mx) ** 2).sum(), ((y - my) ** 2).sum(), ((x - mx) * (y - my)).sum()
    slope = txy / txx
    res = y - ((my - slope * mx) + slope * x)
    return float(1 - (res ** 2).sum() / tyy)


def compare_si_o_si(orig_pos, orig_onehot, gen_pos, gen_onehot, sizes):
    """evaluate_Si-O-Si.py:23-53 on two batches of graphs with identical sizes: graphs where BOTH the original
    and the generated structure pass the selector; returns dict(angle_orig, angle_gen, length_orig, length_gen,
    r2_angle, r2_length, n_selected)."""
    vo, ao, lo = si_o_si(orig_pos, orig_onehot, sizes)
    vg, ag, lg = si_o_si(gen_pos, gen_onehot, sizes)
    keep = (vo & vg).cpu()
    ao, ag, lo, lg = (t.cpu()[keep].numpy() for t in (ao, ag, lo, lg))
    out = dict(angle_orig=ao, angle_gen=ag, length_orig=lo, length_gen=lg, n_selected=int(keep.sum()))
    if out["n_selected"] >= 2:
        out["r2_angle"], out["r2_length"] = r2score(ao, ag), r2score(lo, lg)
    return out


# ---- structural RMSD evaluation (csrc/eval/kabsch.hip) -------------------------------------------------------------
def _kabsch_launch(P, Q, gp, B, center, flip, x_p=None, x_q=None):
    """-> device float [B, 16]: R [9], t [3], rmsd, O rows of x_p, O rows of x_q, 0 (egnn_kabsch)"""
    if center not in _lib.KABSCH_CENTERS or flip not in _lib.KABSCH_FLIPS:
        raise ValueError("center must be 'centroid' or 'first', flip 'row' or 'column'")
    out = torch.empty(B, 16, device=P.device)
    A = 0 if x_p is None else int(x_p.shape[1])
    _lib.check(_lib.lib().egnn_kabsch(_lib.stream_ptr(), B, _lib.ptr(P), _lib.ptr(Q), _lib.ptr(gp), _lib.KABSCH_CENTERS[center],
                                      _lib.KABSCH_FLIPS[flip], _lib.ptr(x_p), _lib.ptr(x_q), A, _lib.ptr(out)))
    return out


class _KabschFit(torch.autograd.Function):
    """(P, Q) float32 [N,3] -> the forward's [B,16] block (R [9], t [3], rmsd, ...), differentiable with respect to P and Q: one
    launch forward (egnn_kabsch, or egnn_kabsch_ordered with an ordering), one launch backward (egnn_kabsch_backward), which
    recomputes the fit from P and Q.  The slices the caller takes of the block hand back zeros for the outputs it does not use."""

    @staticmethod
    def forward(ctx, P, Q, gp, B, center, flip, order):
        if order is None:
            out = _kabsch_launch(P, Q, gp, B, center, flip)
        else:
            out = torch.empty(B, 16, device=P.device)
            _lib.check(_lib.lib().egnn_kabsch_ordered(_lib.stream_ptr(), B, _lib.ptr(P), _lib.ptr(Q), _lib.ptr(gp), _lib.ptr(order),
                                                      _lib.KABSCH_CENTERS[center], _lib.KABSCH_FLIPS[flip], _lib.ptr(out)))
        ctx.save_for_backward(P, Q, gp)
        ctx.order, ctx.B, ctx.center, ctx.flip = order, B, center, flip
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        P, Q, gp = ctx.saved_tensors
        gout = gout.to(torch.float32).contiguous()
        # the kernel always writes dP (it has no path without it), also where only Q requires grad; every row is written, except
        # under an ordering that is no permutation, so those buffers start at zero
        dP = torch.empty_like(P) if ctx.order is None else torch.zeros_like(P)
        dQ = torch.empty_like(Q) if ctx.needs_input_grad[1] else None
        _lib.check(_lib.lib().egnn_kabsch_backward(_lib.stream_ptr(), ctx.B, _lib.ptr(P), _lib.ptr(Q), _lib.ptr(gp), _lib.ptr(ctx.order),
                                                   _lib.KABSCH_CENTERS[ctx.center], _lib.KABSCH_FLIPS[ctx.flip], _lib.ptr(gout),
                                                   _lib.ptr(dP), _lib.ptr(dQ)))
        return (dP if ctx.needs_input_grad[0] else None), dQ, None, None, None, None, None


def _kabsch_differentiable(P, Q, gp, B, center, flip, order=None):
    if center not in _lib.KABSCH_CENTERS or flip not in _lib.KABSCH_FLIPS:
        raise ValueError("center must be 'centroid' or 'first', flip 'row' or 'column'")
    return _KabschFit.apply(P.to(torch.float32).contiguous(), Q.to(torch.float32).contiguous(), gp, B, center, flip, order)


def kabsch(P: torch.Tensor, Q: torch.Tensor, sizes: Sequence[int] | None = None, center="centroid", flip="column"):
    """Kabsch fit of P onto Q -> (R, t, rmsd) with R p_i ~ q_i, for one graph ([n,3] -> [3,3], [3], 0-dim) or a batch of
    graphs (``sizes`` given: [N,3] -> [B,3,3], [B,3], [B]) in one launch.  The defaults are kabsch_torch of
    evaluate_rmsd_for_pos_generate.py:11-51, which parts/def_for_main.py:82,101 call; (center, flip) = ('centroid', 'row') is
    kabsch_numpy of the same file (:53-92) and ('first', 'row') kabsch_numpy of evaluate_rmsd.py:10-42 (t = Q[0] - P[0], which
    that spelling does not return).  'row' is the optimal proper rotation; 'column' reproduces the reference's non-optimal
    reflection fix.  Where p^T q is rank deficient both return the optimal proper rotation (include/egnn_amd.h).
    Like the reference's kabsch_torch, the fit is differentiable: where P or Q requires grad all three outputs carry gradients
    to both (one more launch in backward; egnn_kabsch_backward of include/egnn_amd.h says what it returns where autograd through
    an SVD would return NaN)."""
    if not (P.is_cuda and Q.is_cuda):
        raise RuntimeError("kabsch needs CUDA(ROCm) tensors; there is no CPU fallback")
    if P.shape != Q.shape:
        raise ValueError("Matrix dimensions must match")
    single = sizes is None
    if single:
        sizes = [P.shape[0]]
    gp, B, N = _graph_ptr(sizes, P.device)
    if P.shape != (N, 3):
        raise ValueError("P and Q must be [sum(sizes), 3]")
    if torch.is_grad_enabled() and (P.requires_grad or Q.requires_grad):
        out = _kabsch_differentiable(P, Q, gp, B, center, flip)
    else:
        out = _kabsch_launch(P.detach().to(torch.float32).contiguous(), Q.detach().to(torch.float32).contiguous(), gp, B, center, flip)
    R, t, rmsd = out[:, :9].reshape(B, 3, 3), out[:, 9:12], out[:, 12]
    return (R[0], t[0], rmsd[0]) if single else (R, t, rmsd)


def rmsd_loss(P: torch.Tensor, Q: torch.Tensor, sizes: Sequence[int], center="centroid", flip="column", order=None,
              reduction="mean", searched=None):
    """The structural RMSD of a batch as a loss term: the batch form of train_2024_11.py:233-235 (`_, _, loss_coords =
    kabsch_torch(pos_to_gen, pos)` per graph, summed, divided by num_graph).  P (e.g. the model's output) is fitted onto Q per
    graph in one launch, backward is one launch; gradients flow to P and to Q where they require grad.  reduction 'mean' divides
    the sum by the number of graphs, 'sum' does not, 'none' returns the RMSDs [B].  ``order`` (int32 [N], indices local to each
    graph, as kabsch_min_over_permutations and linear_assignment return them: row order[i] of a graph's P is paired with row i
    of its Q) is a constant of the loss and must be a permutation of every graph's rows.  Those two functions leave the rows of
    graphs they did not search / solve UNWRITTEN: pass their third or fourth result (bool [B]) as ``searched`` and such graphs are
    taken in identity order, or fill the identity there yourself.  The kernels never use an entry outside [0, n) as an address (a
    graph that holds one is fitted in identity order), but that guards memory only: an in-range ordering that is no permutation
    (all zeros, say) is fitted as it stands, and its gradient rows are unspecified."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError("reduction must be 'mean', 'sum' or 'none'")
    if not (P.is_cuda and Q.is_cuda):
        raise RuntimeError("rmsd_loss needs CUDA(ROCm) tensors; there is no CPU fallback")
    if P.shape != Q.shape or P.device != Q.device:
        raise ValueError("Matrix dimensions (and devices) must match")
    gp, B, N = _graph_ptr(sizes, P.device)
    if P.shape != (N, 3):
        raise ValueError("P and Q must be [sum(sizes), 3]")
    if B < 1:
        raise ValueError("rmsd_loss needs at least one graph")
    if order is not None:
        if not (torch.is_tensor(order) and order.device == P.device and order.shape == (N,) and not order.dtype.is_floating_point):
            raise ValueError("order must be an integer tensor [sum(sizes)] on the device of P")
        order = order.detach().to(torch.int32)
        if searched is not None:
            if not (torch.is_tensor(searched) and searched.device == P.device and searched.shape == (B,)):
                raise ValueError("searched must be a bool tensor [len(sizes)] on the device of P")
            gid = torch.repeat_interleave(torch.arange(B, device=P.device), gp[1:].long() - gp[:-1].long(), output_size=N)
            local = torch.arange(N, device=P.device, dtype=torch.int32) - gp[:-1][gid]
            order = torch.where(searched.bool()[gid], order, local)
        order = order.contiguous()
    elif searched is not None:
        raise ValueError("searched goes with order")
    rmsd = _kabsch_differentiable(P, Q, gp, B, center, flip, order)[:, 12]
    return rmsd if reduction == "none" else (rmsd.sum() / B if reduction == "mean" else rmsd.sum())


def _collate_pairs(original_graph_list, generated_graph_list, with_types):
    """positions (and atom types) of the originals -- the caller's records, possibly on the host: concatenated there and uploaded
    once -- and of the samples (``generated_graph_list[i][-1]``, on the device as generate() leaves them)"""
    if len(original_graph_list) != len(generated_graph_list):
        raise ValueError("original_graph_list and generated_graph_list differ in length")
    if not original_graph_list:
        return None
    gens = [g[-1] for g in generated_graph_list]
    dev = gens[0].pos.device
    if dev.type != "cuda":
        raise RuntimeError("RMSD evaluation needs the samples on a CUDA(ROCm) device; there is no CPU fallback")
    for o in original_graph_list:
        if not hasattr(o, "pos"):
            raise ValueError("RMSD evaluation needs the original structures (generate() of a conditional model)")
    sizes = [int(o.pos.shape[0]) for o in original_graph_list]
    if sizes != [int(g.pos.shape[0]) for g in gens]:
        raise ValueError("Matrix dimensions must match")
    po = torch.cat([o.pos.detach().to(torch.float32) for o in original_graph_list]).to(dev).contiguous()
    pg = torch.cat([g.pos.detach().to(device=dev, dtype=torch.float32) for g in gens]).contiguous()
    xo = xg = None
    if with_types:
        xo = torch.cat([o.x.detach().to(torch.int32) for o in original_graph_list]).to(dev).contiguous()
        xg = torch.cat([g.x.detach().to(device=dev, dtype=torch.int32) for g in gens]).contiguous()
    return sizes, gens, po, pg, xo, xg


def _evaluate(original_graph_list, generated_graph_list, with_types):
    col = _collate_pairs(original_graph_list, generated_graph_list, with_types)
    if col is None:
        return []
    sizes, gens, po, pg, xo, xg = col
    gp, B, _ = _graph_ptr(sizes, po.device)
    out = _kabsch_launch(po, pg, gp, B, "centroid", "column", xo, xg).cpu()   # ONE launch, ONE download
    rows = []
    for i, n in enumerate(sizes):
        if n == 1:
            continue
        original = original_graph_list[i]
        row = (original.id, out[i, 12])
        if with_types:
            row += ([int(out[i, 13]) / n, int(out[i, 14]) / n],)
        rows.append(row + (original, gens[i]))
    return sorted(rows, key=lambda r: r[1])   # stable, as the reference's


def evaluate_by_rmsd(original_graph_list, generated_graph_list):
    """evaluate_by_rmsd(original_graph_list, generated_graph_list) of parts/def_for_main.py:73-89 on what generate() returns:
    [(id, rmsd, original_graph, generated_graph)] sorted by RMSD (kabsch_torch: centroid, column flip), one-atom graphs
    skipped; ``rmsd`` is a 0-dim tensor.  All graphs go through one launch and one download."""
    return _evaluate(original_graph_list, generated_graph_list, False)


def evaluate_by_rmsd_and_atom_type_eval(original_graph_list, generated_graph_list):
    """parts/def_for_main.py:91-117: as evaluate_by_rmsd with [fraction of O rows ([1, 0]) in the original, in the sample]
    after the RMSD: [(id, rmsd, [frac_original, frac_generated], original_graph, generated_graph)]."""
    return _evaluate(original_graph_list, generated_graph_list, True)


def kabsch_min_over_permutations(P: torch.Tensor, Q: torch.Tensor, sizes: Sequence[int], max_atoms=10, out=None):
    """The correspondence search of evaluate_rmsd.py:93-107 on a batch: per graph with 2 <= n <= max_atoms (<= 12) the minimum
    over all orderings [0] + perm(1..n-1) of the rows of P (generated) of the atom-0-anchored, row-flip Kabsch RMSD against Q
    (original).  -> (min_rmsd [B], order int32 [N], R [B,3,3], searched bool [B]) on the device; rows of graphs that were not
    searched keep what ``out`` = (min_rmsd, order, R) held (uninitialised without ``out``)."""
    if not (P.is_cuda and Q.is_cuda):
        raise RuntimeError("kabsch_min_over_permutations needs CUDA(ROCm) tensors; there is no CPU fallback")
    gp, B, N = _graph_ptr(sizes, P.device)
    if P.shape != (N, 3) or Q.shape != (N, 3):
        raise ValueError("P and Q must be [sum(sizes), 3]")
    P, Q = (t.detach().to(torch.float32).contiguous() for t in (P, Q))
    if out is None:
        out = (torch.empty(B, device=P.device), torch.empty(N, dtype=torch.int32, device=P.device), torch.empty(B, 3, 3, device=P.device))
    rmsd, order, R = out
    searched = torch.empty(B, dtype=torch.int32, device=P.device)
    nbytes = int(_lib.lib().egnn_kabsch_perm_workspace_bytes(B, int(max_atoms)))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=P.device)
    _lib.check(_lib.lib().egnn_kabsch_perm(_lib.stream_ptr(), B, _lib.ptr(P), _lib.ptr(Q), _lib.ptr(gp), int(max_atoms), _lib.ptr(rmsd),
                                           _lib.ptr(order), _lib.ptr(R), _lib.ptr(searched), _lib.ptr(ws), nbytes))
    return rmsd, order, R, searched != 0


def min_rmsd_over_permutations(original_graph_list, generated_graph_list, max_atoms=10):
    """What evaluate_rmsd.py:82-109 computes before it writes files: per graph with 2 <= n <= max_atoms
    (id, min_rmsd, order, aligned_pos, x_reordered) -- id with the reference's occurrence suffix ``f'{id}_{k}'`` (k counts the
    graphs of at most max_atoms atoms with that id, :88-92), min_rmsd a float, order a list, aligned_pos = the reordered sample
    about its atom 0 rotated onto the original ([n,3]), x_reordered = sample.x[order]; host tensors, in list order."""
    col = _collate_pairs(original_graph_list, generated_graph_list, True)
    if col is None:
        return []
    sizes, gens, po, pg, xo, xg = col
    rmsd, order, R, searched = kabsch_min_over_permutations(pg, po, sizes, max_atoms)
    dev = pg.device
    sz = torch.tensor(sizes, device=dev)
    gid = torch.repeat_interleave(torch.arange(len(sizes), device=dev), sz)
    first = torch.cumsum(sz, 0) - sz
    atom_ok = searched[gid]
    src = torch.where(atom_ok, first[gid] + order.long(), torch.arange(pg.shape[0], device=dev))
    aligned = torch.einsum("nij,nj->ni", torch.where(atom_ok[:, None, None], R[gid], torch.zeros((), device=dev)),
                           pg[src] - pg[first[gid]])
    rmsd, order, searched, aligned, xr = (t.cpu() for t in (rmsd, order, searched, aligned, xg[src]))
    seen, rows, lo = {}, [], 0
    for i, n in enumerate(sizes):
        sl = slice(lo, lo + n)
        lo += n
        if n > max_atoms:
            continue
        gid_ = original_graph_list[i].id
        seen[gid_] = seen.get(gid_, 0) + 1
        if not bool(searched[i]):
            continue
        rows.append((f"{gid_}_{seen[gid_]}", float(rmsd[i]), order[sl].tolist(), aligned[sl].clone(),
                     xr[sl].to(gens[i].x.dtype)))
    return rows


# ---- atom matching of large graphs (csrc/eval/assign.hip) ----------------------------------------------------------
def linear_assignment(P: torch.Tensor, Q: torch.Tensor, sizes: Sequence[int], out=None):
    """Batched linear sum assignment on the Euclidean distance matrices of a batch of graphs (hungarian_algorithm of
    create_xyz.py:82-85 = scipy.optimize.linear_sum_assignment(norm(P[:, None] - Q[None, :]))), one launch:
    -> (col int32 [N], cost float64 [B], solved bool [B]) on the device.  Row i of a graph's P is matched to row col[i] of its
    Q (local indices; scipy's row_ind is 0..n-1), cost = sum_i |P_i - Q_col[i]| is minimal.  Exact (shortest augmenting paths,
    fp64 duals, fp32 distances as numpy computes them on float32 arrays); equal path costs go to the lowest column index, so
    the result is bitwise reproducible and, where the optimum is unique, scipy's.  Graphs with 1 <= n <= 1024 (_lib.ASSIGN_MAX_ATOMS)
    are solved; rows of the others keep what ``out`` = (col, cost) held (uninitialised without ``out``)."""
    if not (P.is_cuda and Q.is_cuda):
        raise RuntimeError("linear_assignment needs CUDA(ROCm) tensors; there is no CPU fallback")
    if P.shape != Q.shape:
        raise ValueError("Matrix dimensions must match")
    gp, B, N = _graph_ptr(sizes, P.device)
    if P.shape != (N, 3):
        raise ValueError("P and Q must be [sum(sizes), 3]")
    if B < 1:
        raise ValueError("linear_assignment needs at least one graph")
    P, Q = (t.detach().to(torch.float32).contiguous() for t in (P, Q))
    if out is None:
        out = (torch.empty(N, dtype=torch.int32, device=P.device), torch.empty(B, dtype=torch.float64, device=P.device))
    col, cost = out
    if col.shape != (N,) or col.dtype != torch.int32 or cost.shape != (B,) or cost.dtype != torch.float64 or not (
            col.is_cuda and cost.is_cuda and col.is_contiguous() and cost.is_contiguous()):
        raise ValueError("out must be (int32 [N], float64 [B]) contiguous device tensors")
    solved = torch.empty(B, dtype=torch.int32, device=P.device)
    max_atoms = max(1, min(max(int(s) for s in sizes), _lib.ASSIGN_MAX_ATOMS))   # <= 64: the one-wavefront launch
    _lib.check(_lib.lib().egnn_assign(_lib.stream_ptr(), B, _lib.ptr(P), _lib.ptr(Q), _lib.ptr(gp), max_atoms, _lib.ptr(col),
                                      _lib.ptr(cost), _lib.ptr(solved)))
    return col, cost, solved != 0


def align_by_assignment(original_graph_list, generated_graph_list, min_atoms=6):
    """What create_xyz.py:157-192 computes before it writes files, on what generate() returns: per graph with
    min_atoms <= n <= 1024 the sample is pre-aligned on the best of the 24 pairings of the four atoms nearest to atom 0 of either
    structure (:158-181), its atoms are matched to the original's by a linear sum assignment on the distances (:182), both
    structures are reordered (:183-190) and the atom-0-anchored, row-flip Kabsch RMSD of the matched pair is taken (:191).
    -> [(id, rmsd, row_ind, col_ind, original_pos_reordered, generated_pos_aligned_reordered, original_x_reordered,
    generated_x_reordered)] in list order: id = f'{original.id}_{i % 5 + 1}' (i the list index, :120), rmsd a float, row_ind /
    col_ind int64 arrays (scipy's: row_ind = 0..n-1), positions about atom 0 (the sample's rotated), host tensors.  The whole list
    is collated once, goes through three launches (pre-alignment, assignment, Kabsch) and is downloaded once; graphs below
    min_atoms are min_rmsd_over_permutations' (the reference's exhaustive branch, :131-156)."""
    if int(min_atoms) < _lib.PREALIGN_MIN_ATOMS:
        raise ValueError(f"min_atoms must be at least {_lib.PREALIGN_MIN_ATOMS}: atom 0 and its four nearest neighbours")
    col_ = _collate_pairs(original_graph_list, generated_graph_list, True)
    if col_ is None:
        return []
    sizes, gens, po, pg, xo, xg = col_
    dev = pg.device
    gp, B, N = _graph_ptr(sizes, dev)
    R = torch.zeros(B, 9, device=dev)
    prealigned = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().egnn_assign_prealign(_lib.stream_ptr(), B, _lib.ptr(po), _lib.ptr(pg), _lib.ptr(gp), int(min_atoms),
                                               _lib.ptr(R), _lib.ptr(prealigned)))
    sz = torch.tensor(sizes, device=dev)
    gid = torch.repeat_interleave(torch.arange(B, device=dev), sz)
    first = torch.cumsum(sz, 0) - sz
    oc = po - po[first[gid]]
    aligned = torch.einsum("nij,nj->ni", R.reshape(B, 3, 3)[gid], pg - pg[first[gid]]).contiguous()
    col = torch.zeros(N, dtype=torch.int32, device=dev)
    col, _, solved = linear_assignment(oc, aligned, sizes, out=(col, torch.empty(B, dtype=torch.float64, device=dev)))
    src = first[gid] + col.long()
    matched = aligned[src].contiguous()
    fit = _kabsch_launch(matched, oc, gp, B, "first", "row")
    # one download: every result is 4 bytes wide, so they travel bit-cast in one int32 buffer
    parts = ((solved & (prealigned != 0)).to(torch.int32), fit[:, 12], col, oc, matched, xg[src])
    blob = torch.cat([t.contiguous().view(torch.int32).reshape(-1) for t in parts]).cpu()
    keep, rmsd, col, oc, matched, xr = (piece.view(t.dtype).reshape(t.shape)
                                        for piece, t in zip(blob.split([t.numel() for t in parts]), parts))
    rows, lo = [], 0
    for i, n in enumerate(sizes):
        sl = slice(lo, lo + n)
        lo += n
        if n < min_atoms or not bool(keep[i]):
            continue
        original = original_graph_list[i]
        rows.append((f"{original.id}_{i % 5 + 1}", float(rmsd[i]), np.arange(n), col[sl].numpy().astype(np.int64), oc[sl].clone(),
                     matched[sl].clone(), original.x.detach().cpu().clone(), xr[sl].to(gens[i].x.dtype)))
    return rows


# ---- whole-structure statistics (csrc/eval/structure.hip) ----------------------------------------------------------
def _struct_tiles(sizes):
    """The work lists of egnn_struct_pair_counts and egnn_struct_bonds (include/egnn_amd.h) from the graph sizes, on the host:
    pair tiles {g, c0, j0} for every (64-centre block, 1024-atom neighbour chunk) of every graph -- so that 256 graphs of 64 atoms,
    32 of 512 and one of 4096 atoms all give 256 workgroups -- and bond tiles {g, c0, 0} for every block of 8 centres.
    -> (int32 [n_pair, 3], int32 [n_bond, 3])"""
    sz = np.asarray(list(sizes), dtype=np.int64)
    n_cb, n_jb = -(-sz // _lib.STRUCT_CENTRE_BLOCK), -(-sz // _lib.STRUCT_CHUNK)
    gi, t = block_index(n_cb * n_jb)
    pair = np.stack([gi, (t // n_jb[gi]) * _lib.STRUCT_CENTRE_BLOCK, (t % n_jb[gi]) * _lib.STRUCT_CHUNK], 1)
    gi, t = block_index(-(-sz // _lib.STRUCT_BOND_CENTRES))
    bond = np.stack([gi, t * _lib.STRUCT_BOND_CENTRES, np.zeros_like(t)], 1)
    return pair.astype(np.int32).reshape(-1, 3), bond.astype(np.int32).reshape(-1, 3)


class _StructInput:
    """positions, type indices and the work lists of a batch on the device (one upload of graph_ptr and both tile lists)"""

    def __init__(self, pos, onehot, sizes, what):
        vars(self).update(vars(typed_batch(pos, onehot, sizes, what, min_atoms=0)))   # sizes, B, N, A, max_atoms, dev, pos, type
        pair, bond = _struct_tiles(self.sizes)
        gp = np.zeros(self.B + 1, dtype=np.int64)
        gp[1:] = np.cumsum(self.sizes)
        blob = torch.from_numpy(np.concatenate([gp.astype(np.int32), pair.reshape(-1), bond.reshape(-1)])).to(self.dev)
        self.gp, self.pair_tiles, self.bond_tiles = blob.split([self.B + 1, pair.size, bond.size])
        self.n_pair, self.n_bond = len(pair), len(bond)

    def n_type(self):
        gid = torch.repeat_interleave(torch.arange(self.B, device=self.dev), torch.tensor(self.sizes, device=self.dev), output_size=self.N)
        return torch.zeros(self.B * self.A, dtype=torch.int64, device=self.dev).index_add_(
            0, gid * self.A + self.type.long(), torch.ones(self.N, dtype=torch.int64, device=self.dev)).view(self.B, self.A)


def _nbins(R, dR):
    return len(np.arange(0 + dR, R + dR, dR))


def _pair_counts(inp, R, dR):
    nbins = _nbins(R, dR)
    counts = torch.empty(inp.B, inp.A, inp.A, nbins, dtype=torch.int32, device=inp.dev)
    _lib.check(_lib.lib().egnn_struct_pair_counts(_lib.stream_ptr(), inp.B, inp.A, _lib.ptr(inp.pos), _lib.ptr(inp.type), _lib.ptr(inp.gp),
                                                  inp.max_atoms, _lib.ptr(inp.pair_tiles), inp.n_pair, float(dR), nbins, _lib.ptr(counts)))
    return counts


def _rdf_finish(inp, counts, sigma, R, dR):
    out = torch.empty(counts.shape, dtype=torch.float32, device=inp.dev)
    _lib.check(_lib.lib().egnn_struct_rdf_finish(_lib.stream_ptr(), inp.B, inp.A, _lib.ptr(counts), _lib.ptr(inp.type), _lib.ptr(inp.gp),
                                                 float(R), float(dR), float(sigma), int(counts.shape[-1]), _lib.ptr(out)))
    return out


def _bonds(inp, cutoff, dtheta, max_cn):
    """-> (cn int32, angles int32, overflow int32 [B]): the raw outputs of egnn_struct_bonds"""
    dtheta, max_cn = float(dtheta), int(max_cn)
    nth = int(np.floor(180.0 / dtheta + 0.5)) + 1 if dtheta > 0 else 1
    cn = torch.empty(inp.B, inp.A, inp.A, max(max_cn, 0) + 1, dtype=torch.int32, device=inp.dev)
    ang = torch.empty(inp.B, inp.A, inp.A * (inp.A + 1) // 2, max(nth, 1), dtype=torch.int32, device=inp.dev)
    over = torch.empty(inp.B, dtype=torch.int32, device=inp.dev)
    _lib.check(_lib.lib().egnn_struct_bonds(_lib.stream_ptr(), inp.B, inp.A, _lib.ptr(inp.pos), _lib.ptr(inp.type), _lib.ptr(inp.gp),
                                            inp.max_atoms, _lib.ptr(inp.bond_tiles), inp.n_bond, float(cutoff), dtheta, max_cn,
                                            _lib.ptr(cn), _lib.ptr(ang), _lib.ptr(over)))
    return cn, ang, over


def _raise_on_overflow(over):
    bad = torch.nonzero(over > 0)
    if bad.numel():
        g = int(bad[0])
        raise RuntimeError(f"graph {g}: {int(over[g])} centre(s) with more than 64 bonded neighbours; their angles are not taken "
                           "(lower the cutoff)")


def pair_counts(pos: torch.Tensor, onehot: torch.Tensor, sizes: Sequence[int], R=5.0, dR=0.01) -> torch.Tensor:
    """Ordered-pair counts by type over EVERY centre: int64 [B, A, A, nbins], c[g, a, b, k] = number of pairs i != j of graph g
    with type(i) = a, type(j) = b and |p_j - p_i| in radial bin k -- length_from_exO and the counting loop of RDF
    (evaluate_RDF.py:39-56) taken about every atom instead of atom 0, with rdf()'s bins (nbins = len(np.arange(dR, R + dR, dR)))
    and its edge rule.  ``onehot`` [N, A] must be exactly one-hot (A <= 4); graphs of at most 32768 atoms."""
    inp = _StructInput(pos, onehot, sizes, "pair_counts")
    return _pair_counts(inp, R, dR).long()


def partial_rdf(pos: torch.Tensor, onehot: torch.Tensor, sizes: Sequence[int], sigma=5, R=5.0, dR=0.01) -> torch.Tensor:
    """Partial pair distributions g_ab of every graph: float32 [B, A, A, nbins], g[g, a, b] = gaussian_filter1d(c[g, a, b] /
    max(n_a, 1) / (4 pi rho r^2 dR), sigma) with the reference's normaliser rho = n / (4/3 pi R^3) over ALL atoms of the graph
    (evaluate_RDF.py:50-57).  The sum over b is the mean over the centres i of type a of the reference's RDF(roll(position, i));
    an absent type gives rows of zeros."""
    inp = _StructInput(pos, onehot, sizes, "partial_rdf")
    return _rdf_finish(inp, _pair_counts(inp, R, dR), sigma, R, dR)


def bond_statistics(pos: torch.Tensor, onehot: torch.Tensor, sizes: Sequence[int], cutoff=2.0, dtheta=1.0, max_cn=16):
    """Coordination numbers and bond angles over every centre (j is bonded to i iff |p_j - p_i| < cutoff, the selection of
    evaluate_Si-O-Si.py:23-41; the angle of CN2_evaluate.py:12-16 in fp64):
    -> (cn int64 [B, A, A, max_cn+1], angles int64 [B, A, A(A+1)/2, ntheta]).  cn[g, a, b, m] = centres of type a with m bonded
    neighbours of type b (the last bin: max_cn or more); angles[g, a, p, k] = bonded pairs j < k about centres of type a with
    neighbour types (b <= c), p = b A - b(b-1)/2 + c - b, whose angle falls in the bin centred on k dtheta degrees
    (ntheta = floor(180/dtheta + 0.5) + 1).  Raises RuntimeError, naming the first such graph, if a centre has more than 64 bonds."""
    inp = _StructInput(pos, onehot, sizes, "bond_statistics")
    cn, ang, over = _bonds(inp, cutoff, dtheta, max_cn)
    _raise_on_overflow(over)
    return cn.long(), ang.long()


def structure_profile(pos: torch.Tensor, onehot: torch.Tensor, sizes: Sequence[int], sigma=5, R=5.0, dR=0.01, cutoff=2.0, dtheta=1.0,
                      max_cn=16):
    """pair_counts, partial_rdf, bond_statistics of one batch from one collation: a namespace with pair_counts, partial_rdf, cn,
    angles (as those functions return them) and n_type int64 [B, A], the atoms of every type."""
    from types import SimpleNamespace
    inp = _StructInput(pos, onehot, sizes, "structure_profile")
    counts = _pair_counts(inp, R, dR)
    rdf_ = _rdf_finish(inp, counts, sigma, R, dR)
    cn, ang, over = _bonds(inp, cutoff, dtheta, max_cn)
    _raise_on_overflow(over)
    return SimpleNamespace(pair_counts=counts.long(), partial_rdf=rdf_, cn=cn.long(), angles=ang.long(), n_type=inp.n_type(),
                           sizes=list(inp.sizes))


def _curve_metrics(a, b):
    """cos_similarity / rdf_l2 / rdf_mse / wasserstein of curves along the last axis, batched on the device in float64 (equal
    lengths: W1 of two samples is the mean distance of their sorted values)"""
    a, b = a.double(), b.double()
    diff = a - b
    return dict(cos=(a * b).sum(-1) / (torch.linalg.vector_norm(a, dim=-1) * torch.linalg.vector_norm(b, dim=-1)),
                l2=torch.linalg.vector_norm(diff, dim=-1), mse=(diff * diff).mean(-1),
                wasserstein=(a.sort(-1).values - b.sort(-1).values).abs().mean(-1))


def compare_structures(original_graph_list, generated_graph_list, sigma=5, R=5.0, dR=0.01, cutoff=2.0, dtheta=1.0, max_cn=16):
    """Whole-structure comparison of what generate() returns with the originals (the list conventions of evaluate_by_rmsd): both
    sides are collated once and profiled (structure_profile), then every partial RDF g_ab and every angle distribution of a sample
    is compared with the original's by the reference's curve metrics (evaluate_RDF.py:13-37, :62-63, :82-83).
    -> dict: 'rdf' and 'angles' = {cos, l2, mse, wasserstein} per graph (float64 [B, A, A] and [B, A, A(A+1)/2]; cos is NaN where
    a curve is all zero), 'total' = the same metrics of the curves summed over all graphs ({'rdf': [A, A], 'angles': [A, P]}),
    'cn_original' / 'cn_generated' int64 [B, A, A, max_cn+1], 'original' / 'generated' the two profiles, 'sizes'."""
    col = _collate_pairs(original_graph_list, generated_graph_list, True)
    if col is None:
        return {}
    sizes, _, po, pg, xo, xg = col
    kw = dict(sigma=sigma, R=R, dR=dR, cutoff=cutoff, dtheta=dtheta, max_cn=max_cn)
    o, g = structure_profile(po, xo, sizes, **kw), structure_profile(pg, xg, sizes, **kw)
    if o.partial_rdf.shape != g.partial_rdf.shape:
        raise ValueError("originals and samples differ in the number of atom types")
    return dict(sizes=sizes, rdf=_curve_metrics(o.partial_rdf, g.partial_rdf), angles=_curve_metrics(o.angles, g.angles),
                total=dict(rdf=_curve_metrics(o.partial_rdf.double().sum(0), g.partial_rdf.double().sum(0)),
                           angles=_curve_metrics(o.angles.sum(0), g.angles.sum(0))),
                cn_original=o.cn, cn_generated=g.cn, original=o, generated=g)


# ---- topological fingerprint (csrc/eval/topo.hip) ------------------------------------------------------------------
COVALENT_RADII = (0.66, 1.11)   # (O, Si), Cordero et al. 2008, in the order of the one-hot columns ([1, 0] is O)


class _TopoInput:
    """positions, type indices, graph_ptr and the bond lists of a batch on the device (egnn_topo_bonds: three launches)"""

    def __init__(self, pos, onehot, sizes, radii, scale, what):
        vars(self).update(vars(typed_batch(pos, onehot, sizes, what, min_atoms=1)))   # sizes, B, N, A, max_atoms, dev, pos, type
        radii = np.asarray(radii, dtype=np.float64).reshape(-1)
        if radii.size != self.A:
            raise ValueError(f"{radii.size} radii for {self.A} atom types")
        self.thr = np.ascontiguousarray(float(scale) * (radii[:, None] + radii[None, :]))   # fp64, once per type pair
        sz = np.asarray(self.sizes, dtype=np.int64)
        head = np.concatenate([[0], np.cumsum(sz), [0], np.cumsum(sz * sz)])   # graph_ptr [B+1], then dist_ptr [B+1]
        blob = torch.from_numpy(head).to(self.dev)                              # one upload
        self.gp = blob[:self.B + 1].to(torch.int32)
        self.dist_ptr = blob[self.B + 1:].contiguous()
        self.n_dist = int(head[-1])
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=self.dev)
        self.row_ptr, self.neighbours, self.degree, self.overflow = i32(self.N + 1), i32(_lib.TOPO_MAX_DEGREE * self.N), i32(self.N), i32(self.B)
        _lib.check(_lib.lib().egnn_topo_bonds(_lib.stream_ptr(), self.B, self.N, self.A, _lib.ptr(self.pos), _lib.ptr(self.type),
                                              _lib.ptr(self.gp), self.max_atoms, _lib.host_ptr(self.thr), _lib.ptr(self.row_ptr),
                                              _lib.ptr(self.neighbours), _lib.ptr(self.degree), _lib.ptr(self.overflow)))

    def paths(self, max_length, dist=False, component=False, fp=True):
        """egnn_topo_paths -> (dist [sum n^2], the uint16 values in an int16 tensor | None, component | None, fragments | None, fp int32 [B, K] | None)"""
        L = int(max_length)
        Cn = _lib.TOPO_BRANCH_MODULUS * self.A
        d = torch.empty(self.n_dist, dtype=torch.int16, device=self.dev) if dist else None
        c = torch.empty(self.N, dtype=torch.int32, device=self.dev) if component else None
        f = torch.empty(self.B, dtype=torch.int32, device=self.dev) if component else None
        k = torch.empty(self.B, Cn * (Cn + 1) // 2 * max(L, 1), dtype=torch.int32, device=self.dev) if fp else None
        _lib.check(_lib.lib().egnn_topo_paths(_lib.stream_ptr(), self.B, self.N, self.A, _lib.ptr(self.type), _lib.ptr(self.gp), self.max_atoms,
                                              _lib.ptr(self.row_ptr), _lib.ptr(self.neighbours), _lib.ptr(self.degree), _lib.ptr(self.overflow),
                                              L, _lib.ptr(d), _lib.ptr(self.dist_ptr), _lib.ptr(c), _lib.ptr(f), _lib.ptr(k)))
        return d, c, f, k


def _raise_on_topo_overflow(over, side=""):
    """``side`` names the list a graph belongs to where a call looks at two ('original' / 'generated')"""
    bad = torch.nonzero(over > 0)
    if bad.numel():
        g = int(bad[0])
        raise RuntimeError(f"{side + ' ' if side else ''}graph {g}: {int(over[g])} atom(s) with more than 32 bonds; the graph has no "
                           "bond list, distances or fingerprint (lower the scale or the radii)")


def bond_graph(pos: torch.Tensor, onehot: torch.Tensor, sizes: Sequence[int], radii=COVALENT_RADII, scale=1.2):
    """The bond graph guess_bonds draws (evaluate_fingerprint.py:49-84), for a ragged batch: atoms i != j of one graph are bonded
    iff |p_i - p_j| < scale * (radii[type i] + radii[type j]), the distance in fp64 from the float32 positions.
    -> (row_ptr int64 [N+1], neighbours int64 [n_bonds], degree int64 [N]): a CSR list over the atoms of the whole batch, every row
    ascending, atom indices counting over the batch.  ``onehot`` [N, A] exactly one-hot, A <= 4 = len(radii); graphs of at most
    1024 atoms.  Raises RuntimeError, naming the first such graph, if an atom has more than 32 bonds."""
    inp = _TopoInput(pos, onehot, sizes, radii, scale, "bond_graph")
    _raise_on_topo_overflow(inp.overflow)
    row_ptr = inp.row_ptr.long()
    return row_ptr, inp.neighbours[:int(row_ptr[-1])].long(), inp.degree.long()


def topological_distances(pos: torch.Tensor, onehot: torch.Tensor, sizes: Sequence[int], radii=COVALENT_RADII, scale=1.2):
    """Hop distances on the bond graph of bond_graph: -> (list of int64 [n, n], one per graph, the number of bonds on a shortest
    path and -1 where there is none; fragments int64 [B], the connected components of each graph; component int64 [N], the lowest
    atom index -- counted over the batch -- reachable from each atom)."""
    inp = _TopoInput(pos, onehot, sizes, radii, scale, "topological_distances")
    _raise_on_topo_overflow(inp.overflow)
    d, comp, frag, _ = inp.paths(1, dist=True, component=True, fp=False)
    d = d.long() & 0xFFFF
    d = torch.where(d == 0xFFFF, torch.full_like(d, -1), d)
    return [b.view(n, n) for b, n in zip(d.split([n * n for n in inp.sizes]), inp.sizes)], frag.long(), comp.long()


def atom_pair_fingerprint(pos: torch.Tensor, onehot: torch.Tensor, sizes: Sequence[int], radii=COVALENT_RADII, scale=1.2, max_length=30):
    """The atom-pair count vector of every graph's bond graph (AllChem.GetAtomPairFingerprint, evaluate_fingerprint.py:109-110,
    restated): int32 [B, K], K = C (C + 1) / 2 * max_length with C = 7 A.  Every pair of atoms i < j joined by a shortest path of
    1 <= d <= max_length bonds counts once under the key (class lo, class hi, d), class = type * 7 + degree % 7:
    fp[g, (c_lo C - c_lo (c_lo - 1) / 2 + c_hi - c_lo) * max_length + d - 1]."""
    inp = _TopoInput(pos, onehot, sizes, radii, scale, "atom_pair_fingerprint")
    _raise_on_topo_overflow(inp.overflow)
    return inp.paths(max_length)[3]


def _tanimoto(fp_a, fp_b):
    n, K = fp_a.shape
    sim = torch.empty(n, dtype=torch.float64, device=fp_a.device)
    sa, sb = torch.empty(n, dtype=torch.int64, device=fp_a.device), torch.empty(n, dtype=torch.int64, device=fp_a.device)
    _lib.check(_lib.lib().egnn_topo_tanimoto(_lib.stream_ptr(), n, K, _lib.ptr(fp_a), n, _lib.ptr(fp_b), n, None, _lib.ptr(sim),
                                             _lib.ptr(sa), _lib.ptr(sb)))
    return sim, sa, sb


def tanimoto(fp_a: torch.Tensor, fp_b: torch.Tensor):
    """Tanimoto similarity of count vectors, row by row (DataStructs.TanimotoSimilarity, evaluate_fingerprint.py:96-97):
    -> (sim float64 [B], sa int64 [B], sb int64 [B]); sim = sum min(a, b) / (sa + sb - sum min(a, b)), integer sums and one fp64
    division; 0.0 where both rows are empty (sa = sb = 0 tells)."""
    if not fp_a.is_cuda or not fp_b.is_cuda:
        raise RuntimeError("tanimoto needs CUDA(ROCm) tensors; there is no CPU fallback")
    if fp_a.dim() != 2 or fp_a.shape != fp_b.shape or fp_a.shape[0] < 1 or fp_a.shape[1] < 1:
        raise ValueError("fp_a and fp_b must be [B, K] of one shape")
    return _tanimoto(fp_a.to(torch.int32).contiguous(), fp_b.to(torch.int32).contiguous())


def fingerprint_similarity(original_graph_list, generated_graph_list, radii=COVALENT_RADII, scale=1.2, max_length=30):
    """The loop of evaluate_fingerprint.py:127-134 on what generate() returns (the list conventions of evaluate_by_rmsd): for every
    original and the LAST element of its generated entry, guess the bonds, take the atom-pair fingerprints and their Tanimoto
    similarity; one-atom graphs are skipped.  Both sides are collated once; two fingerprint passes, one Tanimoto launch, one
    download.  -> (similarities: list of float in list order, one per graph that was not skipped; skipped: list of the indices
    that were).  Raises RuntimeError naming the side ('original' / 'generated') and the first graph with an atom above 32 bonds."""
    col = _collate_pairs(original_graph_list, generated_graph_list, True)
    if col is None:
        return [], []
    sizes, _, po, pg, xo, xg = col
    if xo.shape[1:] != xg.shape[1:]:
        raise ValueError("originals and samples differ in the number of atom types")
    a = _TopoInput(po, xo, sizes, radii, scale, "fingerprint_similarity")
    b = _TopoInput(pg, xg, sizes, radii, scale, "fingerprint_similarity")
    sim, _, _ = _tanimoto(a.paths(max_length)[3], b.paths(max_length)[3])
    out = torch.cat([sim, a.overflow.double(), b.overflow.double()]).cpu()   # ONE download
    B = len(sizes)
    _raise_on_topo_overflow(out[B:2 * B], "original")      # (such a graph's fingerprint is zero: the launches above were harmless)
    _raise_on_topo_overflow(out[2 * B:], "generated")
    skipped = [i for i, n in enumerate(sizes) if n == 1]
    return [float(out[i]) for i, n in enumerate(sizes) if n != 1], skipped


# ---- shortest-path ring statistics (csrc/eval/rings.hip) ------------------------------------------------------------
def _ring_statistics(inp, centres, max_size, max_sites, side=""):
    from . import _rings
    what = f"{side + ' ' if side else ''}graph"
    gp_h = np.concatenate([[0], np.cumsum(inp.sizes)])
    where = lambda i: (int(np.searchsorted(gp_h, i, side="right") - 1), int(i - gp_h[np.searchsorted(gp_h, i, side="right") - 1]))
    crowded = torch.nonzero(inp.degree > _lib.TOPO_MAX_DEGREE).reshape(-1)
    if crowded.numel():
        g, a = where(int(crowded[0]))
        raise ValueError(f"{what} {g}, atom {a}: more than 32 bonds; no ring is searched (lower the scale or the radii)")
    if centres is None:
        idx = torch.arange(inp.N, dtype=torch.int64)
    else:
        idx = torch.as_tensor(centres).detach().cpu().reshape(-1).to(torch.int64)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= inp.N):
            raise ValueError(f"a centre lies outside the {inp.N} atoms of the batch")

    def describe(m, limit):
        g, a = where(int(idx[m]))
        return (f"{what} {g}, atom {a}: a ring search labelled more than max_sites = {int(max_sites)} sites; raise max_sites (at most "
                f"{_lib.RING_MAX_SITES}) or lower max_size")

    E = int(inp.row_ptr[-1])
    # a search inside a graph of n atoms labels at most n sites: a table sized for the largest graph gives the same result as a
    # larger one and leaves room for more searches per CU (the kernel's LDS grows with max_sites)
    sites = min(int(max_sites), max(inp.max_atoms, 1)) if int(max_sites) >= 1 else int(max_sites)
    return _rings.run(inp.row_ptr, inp.neighbours[:E], None, inp.type, inp.A, idx, max_size, sites, describe)


def ring_statistics(pos: torch.Tensor, onehot: torch.Tensor, sizes: Sequence[int], radii=COVALENT_RADII, scale=1.2, centres=None,
                    max_size=16, max_sites=4096):
    """Shortest-path ring statistics of the bond graph of ``bond_graph`` (King's criterion per angle, as Rino et al. apply it to
    silica; not in the reference): for every pair (p, q), p < q, of neighbours of a centre, the size of the smallest ring through
    centre and both -- 2 + the bonds on a shortest path from one neighbour to the other that avoids the centre, so it counts ATOMS:
    a "6-membered" silica ring has size 12 -- and the number of such shortest paths.  ``centres``: None = every atom, or an index
    tensor into the concatenated atoms (any order, duplicates allowed).  3 <= max_size <= 32; a ring above max_size is no ring
    (size 0).  -> ``RingStatistics`` (size, count, angle_ptr, neighbours, centre, histogram, per_centre_smallest).  Raises
    ValueError naming graph and atom where an atom has more than 32 bonds or a search labels more than ``max_sites`` (<= 4096)
    sites."""
    inp = _TopoInput(pos, onehot, sizes, radii, scale, "ring_statistics")
    return _ring_statistics(inp, centres, max_size, max_sites)


def _ring_histograms(inp, rs):
    """per graph: ring sizes 1 .. max_size over every angle of the graph's atoms, normalised to sum 1 (zeros where it has no ring)"""
    gp = inp.gp.long()
    graph = torch.searchsorted(gp, rs.centre[rs.angle_centre], right=True) - 1
    bins = rs.max_size + 1
    keep = rs.size > 0
    h = torch.bincount(graph[keep] * bins + rs.size[keep], minlength=inp.B * bins).view(inp.B, bins).double()
    total = h.sum(1, keepdim=True)
    return torch.where(total > 0, h / total.clamp(min=1.0), h)


def compare_rings(original_graph_list, generated_graph_list, radii=COVALENT_RADII, scale=1.2, max_size=16, max_sites=4096):
    """Ring statistics of both sides of what generate() returns (the list conventions of evaluate_by_rmsd): for every original and the
    LAST element of its generated entry, the ring-size histogram over every angle of every atom (bins 0 .. max_size, bin 0 unused),
    normalised to sum 1.  -> dict(sizes; original, generated: float64 [B, max_size + 1]; l1: list of float, sum |a - b|; cosine:
    list of float, ``cos_similarity``).  A pair with no ring on both sides gets l1 = 0 and cosine = 1; a pair with rings on one
    side only gets l1 = 1 and cosine = 0."""
    col = _collate_pairs(original_graph_list, generated_graph_list, True)
    if col is None:
        return dict(sizes=[], original=None, generated=None, l1=[], cosine=[])
    sizes, _, po, pg, xo, xg = col
    if xo.shape[1:] != xg.shape[1:]:
        raise ValueError("originals and samples differ in the number of atom types")
    a = _TopoInput(po, xo, sizes, radii, scale, "compare_rings")
    b = _TopoInput(pg, xg, sizes, radii, scale, "compare_rings")
    ha = _ring_histograms(a, _ring_statistics(a, None, max_size, max_sites, "original"))
    hb = _ring_histograms(b, _ring_statistics(b, None, max_size, max_sites, "generated"))
    both = torch.stack([ha, hb]).cpu()      # ONE download
    l1, cosine = [], []
    for x, y in zip(both[0], both[1]):
        l1.append(float((x - y).abs().sum()))
        empty_x, empty_y = not bool(x.any()), not bool(y.any())
        cosine.append(1.0 if empty_x and empty_y else (0.0 if empty_x or empty_y else cos_similarity(x, y)))
    return dict(sizes=sizes, original=both[0], generated=both[1], l1=l1, cosine=cosine)


# ---- structure factors (csrc/eval/sq.hip) --------------------------------------------------------------------------
NEUTRON_LENGTHS = (5.803, 4.1491)   # coherent neutron scattering lengths in fm, (O, Si), in the order of the one-hot columns
_SQ_PARTIAL_BYTES = 256 << 20       # workspace of one egnn_sq_debye call; a longer q list is taken in slabs
SQ_FORMS = ("faber-ziman", "ashcroft-langreth")


def _sq_tiles(sizes):
    """The work list of egnn_sq_debye (include/egnn_amd.h) from the graph sizes, on the host: {g, c0, j0} for every block of 64
    atoms i and 256 atoms j of a graph that holds a pair i < j, graph by graph -- 256 graphs of 64 atoms give 256 workgroups, 32
    of 512 atoms 384 and one of 4096 atoms 544 -- and tile_ptr [B+1], the first tile of each graph.
    -> (int32 [n_tiles, 3], int32 [B+1])"""
    sz = np.asarray(list(sizes), dtype=np.int64)
    n_cb, n_jb = -(-sz // _lib.SQ_ROW_BLOCK), -(-sz // _lib.SQ_CHUNK)
    gi, t = block_index(n_cb * n_jb)
    c0, j0 = (t // np.maximum(n_jb[gi], 1)) * _lib.SQ_ROW_BLOCK, (t % np.maximum(n_jb[gi], 1)) * _lib.SQ_CHUNK
    keep = np.minimum(j0 + _lib.SQ_CHUNK, sz[gi]) - 1 > c0   # the last j of the block lies above its first i
    tiles = np.stack([gi[keep], c0[keep], j0[keep]], 1).astype(np.int32).reshape(-1, 3)
    tile_ptr = np.zeros(sz.size + 1, dtype=np.int64)
    tile_ptr[1:] = np.cumsum(np.bincount(gi[keep], minlength=sz.size))
    return tiles, tile_ptr.astype(np.int32)


def _sq_q(q):
    qh = np.ascontiguousarray(np.asarray(q.detach().cpu() if isinstance(q, torch.Tensor) else q, dtype=np.float64).reshape(-1))
    if qh.size < 1:
        raise ValueError("q must hold at least one value")
    if qh.size > _lib.SQ_MAX_Q:
        raise ValueError(f"{qh.size} q values (at most {_lib.SQ_MAX_Q} per call)")
    if not np.all(np.isfinite(qh)) or np.any(qh < 0):
        raise ValueError("every q must be finite and not negative")
    return qh


class _DebyePlan:
    """everything one Debye call needs on the device (checks, the tile list, q and the workspace uploaded / allocated once);
    ``run()`` is the launches alone"""

    def __init__(self, inp, qh, r_max, window, what):
        if inp.A > _lib.SQ_MAX_TYPES:
            raise ValueError(f"{what}: {inp.A} atom types (at most {_lib.SQ_MAX_TYPES})")
        for g, n in enumerate(inp.sizes):
            if n > _lib.SQ_MAX_ATOMS:
                raise ValueError(f"{what}: graph {g} has {n} atoms (at most {_lib.SQ_MAX_ATOMS})")
        if window not in _lib.SQ_WINDOWS:
            raise ValueError(f"window must be None or 'lorch', not {window!r}")
        self.r_max = float("inf") if r_max is None else float(r_max)
        if not self.r_max > 0:
            raise ValueError("r_max must be positive (None: no cut)")
        self.window = _lib.SQ_WINDOWS[window]
        if self.window == 1 and not np.isfinite(self.r_max):
            raise ValueError("the Lorch window needs a finite r_max")
        tiles, tile_ptr = _sq_tiles(inp.sizes)
        self.inp, self.qh, self.n_tiles, self.Q = inp, qh, len(tiles), int(qh.size)
        P = inp.A * (inp.A + 1) // 2
        blob = torch.from_numpy(np.concatenate([tile_ptr, tiles.reshape(-1)])).to(inp.dev)
        self.tile_ptr, self.tiles = blob.split([inp.B + 1, tiles.size])
        self.q = torch.from_numpy(qh).to(inp.dev)
        self.slab = max(1, min(self.Q, _SQ_PARTIAL_BYTES // max(1, self.n_tiles * P * 8)))
        self.partial = torch.empty(max(self.n_tiles * P * self.slab, 1), dtype=torch.float64, device=inp.dev)

    def run(self):
        inp, Q = self.inp, self.Q
        out = torch.empty(inp.B, inp.A, inp.A, Q, dtype=torch.float64, device=inp.dev)
        for s in range(0, Q, self.slab):
            m = min(self.slab, Q - s)
            piece = out if m == Q else torch.empty(inp.B, inp.A, inp.A, m, dtype=torch.float64, device=inp.dev)
            _lib.check(_lib.lib().egnn_sq_debye(_lib.stream_ptr(), inp.B, inp.A, _lib.ptr(inp.pos), _lib.ptr(inp.type), _lib.ptr(inp.gp),
                                                inp.max_atoms, m, self.qh[s:].ctypes.data, _lib.ptr(self.q[s:]), self.r_max, self.window,
                                                _lib.ptr(self.tiles) if self.n_tiles else None, self.n_tiles, _lib.ptr(self.tile_ptr),
                                                _lib.ptr(self.partial), _lib.ptr(piece)))
            if m != Q:
                out[..., s:s + m] = piece
        return out


def _debye_sums(inp, qh, r_max, window, what):
    return _DebyePlan(inp, qh, r_max, window, what).run()


def debye_sums(pos: torch.Tensor, onehot: torch.Tensor, sizes: Sequence[int], q, r_max=None, window=None) -> torch.Tensor:
    """Debye sums of every graph: float64 [B, A, A, Q], D[g, a, b, k] = sum over the pairs i != j of graph g with type(i) = a,
    type(j) = b and r_ij < r_max of w(r_ij) sinc(q_k r_ij) (csrc/eval/sq_math.h): r in fp64 from the float32 positions, sinc(0) = 1,
    ``r_max=None`` no cut, ``window`` None (w = 1) or 'lorch' (w = sinc(pi r / r_max), needs r_max).  ``q``: up to 4096 finite
    values >= 0 in any order.  D is symmetric in (a, b) and D(0) without a cut is exactly N_a N_b - delta_ab N_a.  No file of the
    reference computes this ("Structure factors")."""
    inp = _StructInput(pos, onehot, sizes, "debye_sums")
    return _debye_sums(inp, _sq_q(q), r_max, window, "debye_sums")


def _sf_weights(weights, A, Q, dev):
    """scattering lengths -> float64 [A, Q] on the device ([A] is broadcast along q)"""
    if weights is None:
        if A != 2:
            raise ValueError(f"weights is required for {A} atom types (the default NEUTRON_LENGTHS is (O, Si))")
        weights = NEUTRON_LENGTHS
    b = torch.as_tensor(weights, dtype=torch.float64).detach().to(dev)
    if b.dim() == 1 and b.shape[0] == A:
        return b[:, None].expand(A, Q)
    if b.shape != (A, Q):
        raise ValueError(f"weights must be [A] or [A, Q] = [{A}] or [{A}, {Q}], not {list(b.shape)}")
    return b


def _sf_finish(D, n_type, weights, form):
    """partials and total of ``form`` from D [B, A, A, Q] (float64) and n_type [B, A]: float64 element-wise ops on the device.
    faber-ziman: 1 + N / (N_a N_b) D_ab; ashcroft-langreth: delta_ab + D_ab / sqrt(N_a N_b); an absent type gives rows of zeros;
    total = 1 + sum_ab b_a b_b D_ab / (N <b>^2), <b> = sum_a (N_a / N) b_a (zeros for a graph without atoms)."""
    if form not in SQ_FORMS:
        raise ValueError(f"form must be one of {SQ_FORMS}, not {form!r}")
    B, A, _, Q = D.shape
    n = n_type.to(torch.float64)
    N = n.sum(1)
    nn = n[:, :, None] * n[:, None, :]
    present = nn > 0
    safe = torch.where(present, nn, torch.ones_like(nn))
    if form == "faber-ziman":
        partial = 1.0 + (N[:, None, None] / safe)[..., None] * D
    else:
        partial = torch.eye(A, dtype=torch.float64, device=D.device)[None, :, :, None] + D / safe.sqrt()[..., None]
    partial = torch.where(present[..., None], partial, torch.zeros_like(partial))
    b = _sf_weights(weights, A, Q, D.device)
    some = N > 0
    Ns = torch.where(some, N, torch.ones_like(N))
    mean_b = (n / Ns[:, None]) @ b                                      # [B, Q]
    mean_b = torch.where(some[:, None], mean_b, torch.ones_like(mean_b))
    total = 1.0 + torch.einsum("aq,bq,gabq->gq", b, b, D) / (Ns[:, None] * mean_b * mean_b)
    return partial, torch.where(some[:, None], total, torch.zeros_like(total))


def structure_factor(pos: torch.Tensor, onehot: torch.Tensor, sizes: Sequence[int], q, weights=None, r_max=None, window=None,
                     form="faber-ziman"):
    """Static structure factors of every graph from its Debye sums: a namespace with q float64 [Q], debye [B, A, A, Q],
    partial [B, A, A, Q] (``form`` 'faber-ziman': 1 + N / (N_a N_b) D_ab, or 'ashcroft-langreth': delta_ab + D_ab / sqrt(N_a N_b);
    zeros for an absent type), total [B, Q] = 1 + sum_ab b_a b_b D_ab / (N <b>^2), n_type int64 [B, A] and sizes.  ``weights``:
    scattering lengths [A], or [A, Q] for q-dependent form factors; default NEUTRON_LENGTHS for (O, Si) when A = 2.  The Debye
    sum of a finite cluster carries the cluster's shape at small q ("Structure factors")."""
    from types import SimpleNamespace
    inp = _StructInput(pos, onehot, sizes, "structure_factor")
    qh = _sq_q(q)
    _sf_weights(weights, inp.A, int(qh.size), inp.dev)   # a bad shape fails before the launch
    D = _debye_sums(inp, qh, r_max, window, "structure_factor")
    n_type = inp.n_type()
    partial, total = _sf_finish(D, n_type, weights, form)
    return SimpleNamespace(q=torch.from_numpy(qh).to(inp.dev), debye=D, partial=partial, total=total, n_type=n_type, sizes=list(inp.sizes))


def compare_structure_factors(original_graph_list, generated_graph_list, q=None, weights=None, r_max=None, window=None,
                              form="faber-ziman"):
    """Reciprocal-space comparison of what generate() returns with the originals (the list conventions and the collation of
    compare_structures): both sides get structure_factor on ``q`` (default 0.5 ... 25.0 in steps of 0.05), then every partial and
    the total of a sample are compared with the original's by the reference's curve metrics.
    -> dict: 'partial' and 'total_curve' = {cos, l2, mse, wasserstein} per graph (float64 [B, A, A] and [B]), 'total' = the same
    metrics of the curves summed over all graphs ({'partial': [A, A], 'total_curve': scalar}), 'original' / 'generated' the two
    profiles, 'q', 'sizes'.  Originals and samples are clusters of the same size and shape, so the small-q shape term of the
    Debye sum is compared like for like."""
    col = _collate_pairs(original_graph_list, generated_graph_list, True)
    if col is None:
        return {}
    sizes, _, po, pg, xo, xg = col
    if q is None:
        q = 0.5 + 0.05 * np.arange(491)
    kw = dict(weights=weights, r_max=r_max, window=window, form=form)
    o, g = structure_factor(po, xo, sizes, q, **kw), structure_factor(pg, xg, sizes, q, **kw)
    if o.partial.shape != g.partial.shape:
        raise ValueError("originals and samples differ in the number of atom types")
    return dict(sizes=sizes, q=o.q, partial=_curve_metrics(o.partial, g.partial), total_curve=_curve_metrics(o.total, g.total),
                total=dict(partial=_curve_metrics(o.partial.sum(0), g.partial.sum(0)),
                           total_curve=_curve_metrics(o.total.sum(0), g.total.sum(0))),
                original=o, generated=g)

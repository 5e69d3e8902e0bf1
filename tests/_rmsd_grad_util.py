"""Differentiable torch statement of the three Kabsch spellings, shared by the RMSD gradient tests and by
tests/golden/make_rmsd_grad_golden.py (test infrastructure, not product).

kabsch_autograd(P, Q, center, flip) is tests/_rmsd_util.kabsch_f64 on torch tensors: covariance_torch (the centre 'centroid' |
'first', H = p^T q), torch.linalg.svd, the reflection fix as a product with diag(1, 1, -1) -- from the right of V for 'row' (the
optimal proper rotation), from the left for 'column' (the fix of kabsch_torch, evaluate_rmsd_for_pos_generate.py:11-51) -- and
the residual.  It is independent of the reference by construction only; that it agrees with the reference is what the golden file,
made by EXECUTING the reference's function, shows (tests/test_rmsd_grad_host.py).
"""
import ctypes as C

import numpy as np
import torch

CENTERS = {"centroid": 0, "first": 1}
FLIPS = {"row": 0, "column": 1}
COMBOS = [(c, f) for c in ("centroid", "first") for f in ("row", "column")]


def covariance_torch(P, Q, center):
    """tests/_rmsd_util.covariance_f64 on torch tensors -> (p, q, t, H)"""
    cp, cq = (P.mean(0), Q.mean(0)) if center == "centroid" else (P[0], Q[0])
    p, q = P - cp, Q - cq
    return p, q, cq - cp, p.T @ q


def kabsch_autograd(P, Q, center="centroid", flip="column"):
    p, q, t, H = covariance_torch(P, Q, center)
    U, _, Vt = torch.linalg.svd(H)
    V = Vt.T
    if torch.linalg.det(V @ U.T) < 0:
        J = torch.diag(H.new_tensor([1.0, 1.0, -1.0]))
        V = V @ J if flip == "row" else J @ V
    R = V @ U.T
    return R, t, (((p @ R.T - q) ** 2).sum() / len(P)).sqrt()


def grads_autograd(fn, P, Q, g_R, g_t, g_rmsd, dtype=torch.float64):
    """(dP, dQ) of <g_R, R> + <g_t, t> + g_rmsd rmsd for (R, t, rmsd) = fn(P, Q), by torch autograd in `dtype`, as float64 numpy
    arrays"""
    P = torch.tensor(np.asarray(P), dtype=dtype, requires_grad=True)
    Q = torch.tensor(np.asarray(Q), dtype=dtype, requires_grad=True)
    R, t, rmsd = fn(P, Q)
    L = (R * torch.tensor(np.asarray(g_R), dtype=dtype)).sum() + (t * torch.tensor(np.asarray(g_t), dtype=dtype)).sum() + float(g_rmsd) * rmsd
    L.backward()
    return P.grad.double().numpy(), Q.grad.double().numpy()


def rmsd_loss_autograd(P, Q, sizes, center="centroid", flip="column", reduction="mean"):
    """the batch form of train_2024_11.py:233-235 under autograd: per graph kabsch_autograd's rmsd (0 for a one-atom graph, whose
    sqrt(0) has no finite derivative), summed and divided by the number of graphs"""
    vals, lo = [], 0
    for n in sizes:
        vals.append(kabsch_autograd(P[lo:lo + n], Q[lo:lo + n], center, flip)[2] if n > 1 else P.new_zeros(()))
        lo += n
    vals = torch.stack(vals)
    return {"mean": vals.sum() / len(sizes), "sum": vals.sum(), "none": vals}[reduction]


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def grad_host(lib, P, Q, center, flip, g_R=None, g_t=None, g_rmsd=0.0, want_dQ=True):
    """egnn_kabsch_grad_host of `lib` (a ctypes handle with the argument types set, e.g. diffusion_model_amd._lib.lib())"""
    P, Q = np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(Q, dtype=np.float64)
    g_R = None if g_R is None else np.ascontiguousarray(g_R, dtype=np.float64)
    g_t = None if g_t is None else np.ascontiguousarray(g_t, dtype=np.float64)
    dP, dQ = np.full_like(P, np.nan), (np.full_like(Q, np.nan) if want_dQ else None)
    rc = lib.egnn_kabsch_grad_host(P.shape[0], _dp(P), _dp(Q), CENTERS[center], FLIPS[flip], _dp(g_R), _dp(g_t), float(g_rmsd),
                                   _dp(dP), _dp(dQ))
    assert rc == 0, rc
    return dP, dQ


def worst_ratio(got, want):
    """largest |got - want| as a fraction of the largest element of `want` (one graph)"""
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())

"""SOAP power spectra, their cosine similarity and spectrum template matching on the device (csrc/eval/soap.hip; every formula and
summation order in csrc/eval/soap_math.h).  Restates template_matching.py:41-68 -- dscribe's SOAP(species=["O","Si"], r_cut=8,
n_max=15, l_max=10, sigma=0.1) of atom 0, cosine similarity, MSE of spectrum[0] -- for ragged batches without ASE or dscribe.

The descriptor is the mathematically exact one: the orthonormalising matrices beta^l = (S^l)^(-1/2) have condition numbers up to
4e15, so they are built in mpmath at 60 digits and rounded once to float64 (SoapBasis).  There is no CPU fallback."""
from __future__ import annotations

import functools
import math
from typing import Sequence

import numpy as np
import torch

from . import _lib
from ._batch import typed_batch

DIGITS = 60   # working precision of the tables (decimal digits)


def neighbour_cut_default(r_cut, sigma):
    return float(r_cut) + float(sigma) * math.sqrt(2.0 * math.log(1000.0))


def build_tables(r_cut, n_max, l_max, sigma, digits=DIGITS):
    """K [n][l], gamma [n][l], beta [l][n][n'], N [lm], w [l] of csrc/eval/soap_math.h as float64 arrays, every entry computed in
    mpmath at ``digits`` decimal digits and rounded once.  beta^l = V diag(lambda^-1/2) V^T from the symmetric eigenproblem of the
    overlap matrix at that precision (its condition number, up to 4e15, costs 16 of the digits)."""
    import mpmath as mp   # lazily, and only here (a dependency of sympy, hence of torch)
    with mp.workdps(int(digits)):
        L1 = l_max + 1
        a = 1 / (2 * mp.mpf(repr(float(sigma))) ** 2)
        rc = mp.mpf(repr(float(r_cut)))
        r = [mp.mpf(1) + (rc - 1) * k / (n_max - 1) for k in range(n_max)] if n_max > 1 else [mp.mpf(1)]
        alpha = [[-mp.log(mp.mpf("1e-3") / rn ** l) / rn ** 2 for l in range(L1)] for rn in r]
        K = np.empty((n_max, L1))
        gamma = np.empty((n_max, L1))
        for n in range(n_max):
            for l in range(L1):
                p = alpha[n][l] + a
                K[n, l] = float(mp.pi ** mp.mpf("1.5") * p ** mp.mpf("-1.5") * (a / p) ** l)
                gamma[n, l] = float(a * alpha[n][l] / p)
        beta = np.empty((L1, n_max, n_max))
        for l in range(L1):
            e = mp.mpf(l) + mp.mpf("1.5")
            S = mp.matrix(n_max, n_max)
            for n in range(n_max):
                for q in range(n_max):
                    S[n, q] = mp.gamma(e) / 2 * (alpha[n][l] + alpha[q][l]) ** (-e)
            lam, V = mp.eigsy(S)
            for n in range(n_max):
                for q in range(n_max):
                    beta[l, n, q] = float(mp.fsum(V[n, k] * V[q, k] / mp.sqrt(lam[k]) for k in range(n_max)))
        norm = np.empty(L1 * L1)
        for l in range(L1):
            for m in range(-l, l + 1):
                v = mp.sqrt((2 * l + 1) / (4 * mp.pi) * mp.factorial(l - abs(m)) / mp.factorial(l + abs(m)))
                norm[l * l + l + m] = float(v * mp.sqrt(2) if m else v)
        weight = np.array([float(mp.pi * mp.sqrt(mp.mpf(8) / (2 * l + 1))) for l in range(L1)])
    return K, gamma, beta, norm, weight


class SoapBasis:
    """The tables of one configuration (r_cut, n_max <= 16, l_max <= 10, sigma): built once per process (SoapBasis(...) of equal
    parameters returns the cached object; the defaults take about two seconds of mpmath) and uploaded once per device as one
    buffer.  ``tables`` is the host buffer in the layout of soap_math.h: K | gamma | beta | N | w."""
    _cache: dict = {}

    def __new__(cls, r_cut=8.0, n_max=15, l_max=10, sigma=0.1):
        key = (float(r_cut), int(n_max), int(l_max), float(sigma))
        if key in cls._cache:
            return cls._cache[key]
        r_cut, n_max, l_max, sigma = key
        if not (1 <= n_max <= _lib.SOAP_MAX_N) or not (0 <= l_max <= _lib.SOAP_MAX_L):
            raise ValueError(f"SoapBasis: n_max {n_max} (1 .. {_lib.SOAP_MAX_N}), l_max {l_max} (0 .. {_lib.SOAP_MAX_L})")
        if not (math.isfinite(r_cut) and math.isfinite(sigma) and sigma > 0.0 and (r_cut > 1.0 or (n_max == 1 and r_cut > 0.0))):
            raise ValueError("SoapBasis: r_cut must exceed 1 (the radial functions sit on linspace(1, r_cut, n_max)) and sigma be positive")
        self = super().__new__(cls)
        self.r_cut, self.n_max, self.l_max, self.sigma = r_cut, n_max, l_max, sigma
        self.K, self.gamma, self.beta, self.norm, self.weight = build_tables(r_cut, n_max, l_max, sigma)
        self.tables = np.ascontiguousarray(np.concatenate([a.reshape(-1) for a in (self.K, self.gamma, self.beta, self.norm, self.weight)]))
        assert self.tables.size == _lib.lib().egnn_soap_table_doubles(n_max, l_max)
        self.neighbour_cut = neighbour_cut_default(r_cut, sigma)
        self._device = {}
        cls._cache[key] = self
        return self

    def features(self, A):
        F = _lib.lib().egnn_soap_features(int(A), self.n_max, self.l_max)
        if F < 0:
            _lib.check(F)
        return F

    def device_tables(self, device):
        device = torch.device(device)
        key = (device.type, torch.cuda.current_device() if device.index is None else device.index)
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.tables).to(device)
        return self._device[key]


def _centre_list(centres, sizes, N):
    """-> int32 numpy list of batch-wide atom indices"""
    if isinstance(centres, str):
        starts = np.concatenate([[0], np.cumsum(sizes)])[:-1]
        if centres == "first":
            if min(sizes) < 1:
                raise ValueError("centres='first' needs every graph to have an atom")
            return starts.astype(np.int32)
        if centres == "all":
            return np.arange(N, dtype=np.int32)
        raise ValueError("centres must be 'first', 'all' or a list of atom indices")
    c = centres.detach().cpu().numpy() if isinstance(centres, torch.Tensor) else np.asarray(centres)
    c = c.reshape(-1).astype(np.int64)
    if c.size < 1 or c.min() < 0 or c.max() >= N:
        raise ValueError(f"centres must name at least one atom, all inside [0, {N})")
    return c.astype(np.int32)


def soap_descriptors(pos: torch.Tensor, onehot: torch.Tensor, sizes: Sequence[int], centres="first", basis: SoapBasis | None = None,
                     neighbour_cut=None, return_coefficients=False):
    """The SOAP power spectrum of chosen atoms of a ragged batch: -> float64 [C, F], F = basis.features(A) (5,115 for two species
    and the defaults), in dscribe's order: species pairs (Z1 <= Z2) outermost, then n, n' (n' >= n where Z1 = Z2), l innermost.
    ``onehot`` [N, A] exactly one-hot, A <= 4, its columns in ascending atomic number ([1, 0] is O).  ``centres``: 'first' (atom 0
    of every graph, the excited oxygen of the reference's records), 'all', or a list / LongTensor of atom indices counted over the
    batch, any order, repeats allowed.  Neighbours of a centre: the atoms of its graph closer than ``neighbour_cut`` (default
    r_cut + sigma sqrt(2 ln 1000)), itself included.  With return_coefficients also the orthonormalised coefficients, float64
    [C, A, n_max, (l_max+1)^2] at [l*l + l + m]."""
    batch = typed_batch(pos, onehot, sizes, "soap_descriptors", min_atoms=1, max_types=_lib.SOAP_MAX_TYPES)
    sizes, B, N, A, dev = batch.sizes, batch.B, batch.N, batch.A, batch.dev
    basis = SoapBasis() if basis is None else basis
    cut = basis.neighbour_cut if neighbour_cut is None else float(neighbour_cut)
    if not (math.isfinite(cut) and cut > 0.0):
        raise ValueError("neighbour_cut must be positive and finite")
    c_host = _centre_list(centres, sizes, N)
    head = np.concatenate([np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), c_host])
    blob = torch.from_numpy(head).to(dev)   # one upload: graph_ptr, then the centres
    gp, c_dev = blob[:B + 1], blob[B + 1:]
    C, F = int(c_host.size), basis.features(A)
    desc = torch.empty(C, F, dtype=torch.float64, device=dev)
    coeff = torch.empty(C, A, basis.n_max, (basis.l_max + 1) ** 2, dtype=torch.float64, device=dev) if return_coefficients else None
    tables = basis.device_tables(dev)
    _lib.check(_lib.lib().egnn_soap_descriptor(_lib.stream_ptr(), B, N, A, _lib.ptr(batch.pos), _lib.ptr(batch.type), _lib.ptr(gp), basis.n_max, basis.l_max,
                                               cut, _lib.ptr(tables), C, _lib.host_ptr(c_host), _lib.ptr(c_dev), _lib.ptr(desc), _lib.ptr(coeff)))
    return (desc, coeff) if return_coefficients else desc


def _rows(a, b, what):
    if not a.is_cuda or not b.is_cuda:
        raise RuntimeError(f"{what} needs CUDA(ROCm) tensors; there is no CPU fallback")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1] or a.shape[0] < 1 or b.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("a and b must be [rows_a, F] and [rows_b, F] with at least one row and one column")
    return a.detach().to(torch.float64).contiguous(), b.detach().to(device=a.device, dtype=torch.float64).contiguous()


def _cosine(a, b, pairs, n):
    out = torch.empty(n, dtype=torch.float64, device=a.device)
    _lib.check(_lib.lib().egnn_soap_cosine(_lib.stream_ptr(), n, a.shape[1], _lib.ptr(a), a.shape[0], _lib.ptr(b), b.shape[0],
                                           _lib.ptr(pairs), _lib.ptr(out)))
    return out


def cosine(a: torch.Tensor, b: torch.Tensor, pairs=None) -> torch.Tensor:
    """Cosine similarity of rows of two descriptor matrices (cos_similarity of template_matching.py:8-9): -> float64 [P].
    ``pairs`` [P, 2] names (row of a, row of b); None compares row p with row p (a and b of one shape).  Every sum is taken in
    fp64 in the one fixed order of soap_math.h."""
    a, b = _rows(a, b, "cosine")
    if pairs is None:
        if a.shape != b.shape:
            raise ValueError("without pairs, a and b must have one shape")
        return _cosine(a, b, None, a.shape[0])
    pr = torch.as_tensor(pairs)
    if pr.dim() != 2 or pr.shape[1] != 2 or pr.shape[0] < 1:
        raise ValueError("pairs must be [P, 2]")
    host = pr.detach().cpu()
    if int(host.min()) < 0 or int(host[:, 0].max()) >= a.shape[0] or int(host[:, 1].max()) >= b.shape[0]:
        raise ValueError("a pair names a row outside the matrices")
    return _cosine(a, b, pr.to(device=a.device, dtype=torch.int32).contiguous(), pr.shape[0])


def cosine_matrix(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """All cosines of the rows of a [rows_a, F] against the rows of b [rows_b, F]: -> float64 [rows_a, rows_b]; entry (i, j) is
    bitwise cosine(a, b, [[i, j]])."""
    a, b = _rows(a, b, "cosine_matrix")
    norms = torch.empty(a.shape[0] + b.shape[0], dtype=torch.float64, device=a.device)
    gram = torch.empty(a.shape[0], b.shape[0], dtype=torch.float64, device=a.device)
    _lib.check(_lib.lib().egnn_soap_gram(_lib.stream_ptr(), a.shape[1], _lib.ptr(a), a.shape[0], _lib.ptr(b), b.shape[0], _lib.ptr(norms),
                                         _lib.ptr(gram)))
    return gram


def _groups(target_ids, reference_ids, T, R):
    """ids of any hashable kind -> int32 groups (equal ids, equal group); None on both sides = no exclusion"""
    if target_ids is None and reference_ids is None:
        return None, None
    if target_ids is None or reference_ids is None:
        raise ValueError("give target_ids and reference_ids together")
    target_ids, reference_ids = list(target_ids), list(reference_ids)
    if len(target_ids) != T or len(reference_ids) != R:
        raise ValueError("one id per target and one per reference")
    table: dict = {}
    code = lambda ids: np.array([table.setdefault(i, len(table)) for i in ids], dtype=np.int32)
    return code(target_ids), code(reference_ids)


def _nearest(target, reference, k, tg, rg):
    T, S = target.shape
    dev = target.device
    idx = torch.empty(T, k, dtype=torch.int32, device=dev)
    mse = torch.empty(T, k, dtype=torch.float64, device=dev)
    g = torch.from_numpy(np.concatenate([tg, rg])).to(dev) if tg is not None else None
    _lib.check(_lib.lib().egnn_spectrum_nearest(_lib.stream_ptr(), T, reference.shape[0], S, k, _lib.ptr(target), _lib.ptr(reference),
                                                _lib.ptr(g[:T] if g is not None else None), _lib.ptr(g[T:] if g is not None else None),
                                                _lib.ptr(idx), _lib.ptr(mse)))
    return idx, mse


def nearest_spectra(target: torch.Tensor, reference: torch.Tensor, k=3, target_ids=None, reference_ids=None):
    """For every row of target [T, S] the k <= 8 rows of reference [R, S] of smallest mean squared difference (template_matching.py:
    49-58): -> (idx int64 [T, k], mse float64 [T, k]), ascending, ties to the lower index; the differences and the sum in fp64 from
    the float32 rows.  A reference whose id equals the target's is skipped (ids of any hashable kind); where fewer than k
    references remain the missing entries are index -1, mse +inf.  The [T, R] matrix is never stored."""
    if not target.is_cuda or not reference.is_cuda:
        raise RuntimeError("nearest_spectra needs CUDA(ROCm) tensors; there is no CPU fallback")
    if target.dim() != 2 or reference.dim() != 2 or target.shape[1] != reference.shape[1] or min(target.shape) < 1 or reference.shape[0] < 1:
        raise ValueError("target and reference must be [T, S] and [R, S] with at least one row and one point")
    k = int(k)
    if not 1 <= k <= _lib.SOAP_MAX_K:
        raise ValueError(f"k {k} (1 .. {_lib.SOAP_MAX_K})")
    tg, rg = _groups(target_ids, reference_ids, target.shape[0], reference.shape[0])
    t = target.detach().to(torch.float32).contiguous()
    r = reference.detach().to(device=t.device, dtype=torch.float32).contiguous()
    idx, mse = _nearest(t, r, k, tg, rg)
    return idx.long(), mse


def _collate_records(records, dev, what):
    recs = [r for r in records if int(r.pos.shape[0]) > 1]   # template_matching.py:35,38
    if not recs:
        raise ValueError(f"template_matching: no {what} record of more than one atom")
    sizes = [int(r.pos.shape[0]) for r in recs]
    pos = torch.cat([r.pos.detach().to(torch.float32) for r in recs]).to(dev).contiguous()
    x = torch.cat([r.x.detach().to(torch.int32) for r in recs]).to(dev).contiguous()
    spec = torch.stack([r.spectrum[0].detach().to(torch.float32).reshape(-1) for r in recs]).to(dev).contiguous()
    return recs, sizes, pos, x, spec


def template_matching(targets, references, k=3, basis: SoapBasis | None = None, device=None):
    """The whole of template_matching.py:43-68 on record lists (objects with pos [n, 3], x one-hot [n, A], spectrum [.., S] and id):
    for every target the k references of nearest spectrum[0] whose id differs, and the SOAP cosine of atom 0 against atom 0 of each.
    Records of one atom are dropped on both sides.  Both sides are collated once and every descriptor is computed once: two
    descriptor launches, one nearest launch, one cosine launch, one download.
    -> (result, index int64 [T, k] into the kept references, mse float64 [T, k], similarity float64 [T, k]); result is the
    reference's structure {target id: [{reference id: [mse, similarity]}, ...]} (fewer than k entries where fewer references remain;
    similarity there is NaN in the tensor).  Differences from the reference: INTEGRATION.md, "SOAP"."""
    targets, references = list(targets), list(references)
    if device is None:
        device = next((r.pos.device for r in targets + references if r.pos.is_cuda), None)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if device is None or torch.device(device).type != "cuda":
        raise RuntimeError("template_matching needs a CUDA(ROCm) device; there is no CPU fallback")
    k = int(k)
    if not 1 <= k <= _lib.SOAP_MAX_K:
        raise ValueError(f"k {k} (1 .. {_lib.SOAP_MAX_K})")
    basis = SoapBasis() if basis is None else basis
    tr, ts, tp, tx, tspec = _collate_records(targets, device, "target")
    rr, rs, rp, rx, rspec = _collate_records(references, device, "reference")
    if tx.shape[1] != rx.shape[1] or tspec.shape[1] != rspec.shape[1]:
        raise ValueError("targets and references differ in the number of atom types or of spectrum points")
    tg, rg = _groups([r.id for r in tr], [r.id for r in rr], len(tr), len(rr))
    dt = soap_descriptors(tp, tx, ts, "first", basis)
    dr = soap_descriptors(rp, rx, rs, "first", basis)
    idx, mse = _nearest(tspec, rspec, k, tg, rg)
    T = len(tr)
    pairs = torch.stack([torch.arange(T, device=idx.device, dtype=torch.int32).repeat_interleave(k), idx.reshape(-1)], 1).contiguous()
    sim = _cosine(dt, dr, pairs, T * k).view(T, k)   # index -1 names no row: NaN
    out = torch.cat([idx.double(), mse, sim], 1).cpu()   # ONE download
    idx_h, mse_h, sim_h = out[:, :k].long(), out[:, k:2 * k], out[:, 2 * k:]
    result = {}
    for t, rec in enumerate(tr):
        result[rec.id] = [{rr[int(idx_h[t, q])].id: [float(mse_h[t, q]), float(sim_h[t, q])]} for q in range(k) if int(idx_h[t, q]) >= 0]
    return result, idx_h, mse_h, sim_h


def soap_similarity(original_graph_list, generated_graph_list, basis: SoapBasis | None = None):
    """The SOAP cosine of atom 0 of every original against atom 0 of the LAST element of its generated entry, on what generate()
    returns (the list conventions of stats.fingerprint_similarity); one-atom graphs are skipped.  Both sides are collated once;
    two descriptor launches, one cosine launch, one download.  -> (similarities: list of float in list order, one per graph that
    was not skipped; skipped: list of the indices that were)."""
    from .stats import _collate_pairs
    col = _collate_pairs(original_graph_list, generated_graph_list, True)
    if col is None:
        return [], []
    sizes, _, po, pg, xo, xg = col
    if xo.shape[1:] != xg.shape[1:]:
        raise ValueError("originals and samples differ in the number of atom types")
    basis = SoapBasis() if basis is None else basis
    a = soap_descriptors(po, xo, sizes, "first", basis)
    b = soap_descriptors(pg, xg, sizes, "first", basis)
    out = _cosine(a, b, None, len(sizes)).cpu()
    skipped = [i for i, n in enumerate(sizes) if n == 1]
    return [float(out[i]) for i, n in enumerate(sizes) if n != 1], skipped

"""Shortest-path ring statistics over a bond list on the device (csrc/eval/rings.hip): what ``stats.ring_statistics`` (clusters) and
``cells.ring_statistics`` (periodic cells) share.  The definition is that of csrc/eval/rings_math.h: King's shortest-path criterion
per angle of a centre, sizes counting ATOMS on the ring (a "6-membered" silica ring has size 12).  No reference file computes
rings: an extension beyond the reference ("Rings")."""
from __future__ import annotations

import torch

from . import _lib

MAX_DEGREE = 32   # kRingMaxDegree of csrc/eval/rings_math.h


class RingStatistics:
    """The rings through every angle of M centres (n_angles = sum d (d - 1) / 2 over their degrees d), on the device:
    ``size`` int64 [n_angles] (0 = no ring of at most max_size atoms), ``count`` int64 [n_angles] (shortest closing paths,
    saturating at 2^31 - 1), ``angle_ptr`` int64 [M+1], ``neighbours`` int64 [n_angles, 2] (the two positions p < q in the centre's
    bond-list row, lexicographic inside a centre), ``centre`` int64 [M] (indices into the concatenated atoms), ``histogram`` int64
    [A, max_size + 1] (angles by centre type and size, bin 0 = no ring) and ``per_centre_smallest`` int64 [M] (the smallest
    non-zero size at each centre, 0 if none); ``angle_centre`` int64 [n_angles] is the position in ``centre`` every angle belongs to."""

    def __init__(self, size, count, angle_ptr, neighbours, centre, histogram, per_centre_smallest, max_size, angle_centre):
        self.size, self.count, self.angle_ptr, self.neighbours, self.centre = size, count, angle_ptr, neighbours, centre
        self.histogram, self.per_centre_smallest, self.max_size, self.angle_centre = histogram, per_centre_smallest, max_size, angle_centre


def _pair_table(dev):
    """row positions (p, q) of every angle of a centre of degree 0 .. 32, degree after degree: -> (pairs int64 [*, 2], first int64 [33])"""
    parts = [torch.triu_indices(d, d, 1).t() for d in range(MAX_DEGREE + 1)]
    first = torch.tensor([0] + [int(p.shape[0]) for p in parts[:-1]], dtype=torch.int64).cumsum(0)
    return torch.cat(parts).to(dev), first.to(dev)


def run(row_ptr, atom, shift, types, A, centre_h, max_size, max_sites, describe):
    """``row_ptr`` int32 [N+1], ``atom`` int32 [E], ``shift`` int32 [E, 3] | None, ``types`` int32 [N] on the device; ``centre_h``
    int64 [M] on the host (already checked against N); ``describe(m, limit)`` -> the message of the ValueError an overflowed centre
    raises, limit = 'degree' | 'sites'.  One launch, one download (the overflow flags)."""
    dev = row_ptr.device
    N, E, M = int(row_ptr.numel()) - 1, int(atom.numel()), int(centre_h.numel())
    max_size, max_sites = int(max_size), int(max_sites)
    centre32_h = centre_h.to(torch.int32).contiguous()
    centre = centre_h.to(dev)
    centre32 = centre.to(torch.int32)
    deg = (row_ptr[1:] - row_ptr[:-1]).long()[centre]
    angle_ptr = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    angle_ptr[1:] = torch.cumsum(deg * (deg - 1) // 2, 0)
    n = int(angle_ptr[-1])
    if n >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 angles")
    ap32 = angle_ptr.to(torch.int32)
    i32 = lambda k: torch.empty(max(k, 1), dtype=torch.int32, device=dev)
    size, count, over = i32(n), i32(n), i32(M)
    hist = torch.empty(A, max(max_size, 0) + 1, dtype=torch.int32, device=dev)
    shift = None if shift is None else shift.to(torch.int32).contiguous()
    _lib.check(_lib.lib().egnn_rings(_lib.stream_ptr(), N, _lib.ptr(row_ptr), E, _lib.ptr(atom) if E else None,
                                     _lib.ptr(shift) if shift is not None and E else None, _lib.ptr(types), A, M,
                                     _lib.ptr(centre32) if M else None, _lib.ptr(ap32), n, max_size, max_sites, _lib.ptr(size),
                                     _lib.ptr(count), _lib.ptr(over), _lib.ptr(hist), None, None, None,
                                     _lib.ptr(centre32_h) if M else None))
    bad = torch.nonzero(over[:M].cpu()).reshape(-1)
    if bad.numel():
        m = int(bad[0])
        raise ValueError(describe(m, "degree" if int(deg[m]) > MAX_DEGREE else "sites"))
    size, count = size[:n].long(), count[:n].long()
    which = torch.repeat_interleave(torch.arange(M, device=dev), angle_ptr[1:] - angle_ptr[:-1], output_size=n)
    pairs, first = _pair_table(dev)
    neighbours = pairs[first[deg[which]] + (torch.arange(n, device=dev) - angle_ptr[which])]
    big = max_size + 1
    smallest = torch.full((M,), big, dtype=torch.int64, device=dev)
    if n:
        smallest.scatter_reduce_(0, which, torch.where(size > 0, size, torch.full_like(size, big)), "amin")
    smallest = torch.where(smallest == big, torch.zeros_like(smallest), smallest)
    return RingStatistics(size, count, angle_ptr, neighbours, centre, hist.long(), smallest, max_size, which)

"""What the evaluation entries (stats.py, soap.py, cells.py) share on the host side of a ragged batch: the validation of a typed
batch and the index arithmetic of the work lists."""
from types import SimpleNamespace

import numpy as np
import torch


def typed_batch(pos, onehot, sizes, what, min_atoms, max_types=None):
    """Checks the (positions, one-hot types, graph sizes) of entry ``what`` and -> a namespace of sizes, B, N, A, max_atoms, dev,
    pos (float32, contiguous) and type (int32 indices).  The batch holds at least ``min_atoms`` atoms (0 or 1) and, where
    ``max_types`` is given, at most that many types."""
    if not pos.is_cuda:
        raise RuntimeError(f"{what} needs CUDA(ROCm) tensors; there is no CPU fallback")
    sizes = [int(s) for s in sizes]
    B, N = len(sizes), sum(sizes)
    if B < 1 or min(sizes) < 0 or N < min_atoms:
        raise ValueError(f"{what} needs at least one graph{', at least one atom' if min_atoms else ''} and no negative size")
    if pos.shape != (N, 3):
        raise ValueError("position must be [sum(sizes), 3]")
    oh = onehot.detach().to(pos.device)
    if oh.dim() != 2 or oh.shape[0] != N or oh.shape[1] < 1:
        raise ValueError("onehot must be [sum(sizes), A]")
    A = int(oh.shape[1])
    if max_types is not None and A > max_types:
        raise ValueError(f"{A} atom types (at most {max_types})")
    if N and not bool((((oh == 0) | (oh == 1)).all(1) & (oh.sum(1) == 1)).all()):
        raise ValueError("every row of onehot must be exactly one-hot")
    type_ = (oh.argmax(1) if N else torch.zeros(0, dtype=torch.long, device=pos.device)).to(torch.int32).contiguous()
    return SimpleNamespace(sizes=sizes, B=B, N=N, A=A, max_atoms=max(sizes), dev=pos.device,
                           pos=pos.detach().to(torch.float32).contiguous(), type=type_)


def block_index(per):
    """owner and local index of every block, where owner o has per[o] blocks: -> (int64 [sum(per)], int64 [sum(per)])"""
    per = np.asarray(per, dtype=np.int64)
    owner = np.repeat(np.arange(per.size, dtype=np.int64), per)
    return owner, np.arange(int(per.sum()), dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)

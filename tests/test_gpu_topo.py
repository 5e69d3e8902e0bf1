"""GPU tests of the topological fingerprint (csrc/eval/topo.hip): egnn_topo_bonds, egnn_topo_paths and egnn_topo_tanimoto
against the host statement egnn_topo_host, BITWISE in every output (bond lists, degrees, overflow, distances, components,
fragments, fingerprints, the fp64 similarity), and diffusion_model_amd.stats on top of them against the numpy restatement of
tests/_topo_util.py.

The comparison is exact because both sides compile one text (csrc/eval/topo_math.h), every sum is an integer, and every input
first passes the gap check of the host test: no pair distance within 1e-9 (relative) of its bond threshold.
"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from diffusion_model_amd import _lib, stats
from tests import _topo_util as TU

pytestmark = pytest.mark.gpu
DEV = "cuda"
THR2 = TU.thresholds(TU.RADII[2])


def _onehot(types, A):
    return torch.eye(A, dtype=torch.int64)[torch.from_numpy(np.asarray(types)).long()]


def _device(pos, types, sizes, A, thr, L=30, want=("dist", "component", "fragments", "fp")):
    """the raw outputs of egnn_topo_bonds + egnn_topo_paths in the layout of TU.host (numpy); outputs not in ``want`` are not passed"""
    lib, B, N = _lib.lib(), len(sizes), int(sum(sizes))
    sz = np.asarray(sizes, dtype=np.int64)
    p = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32)).to(DEV)
    t = torch.from_numpy(np.ascontiguousarray(types, dtype=np.int32)).to(DEV)
    gp = torch.from_numpy(np.concatenate([[0], np.cumsum(sz)]).astype(np.int32)).to(DEV)
    dptr = torch.from_numpy(np.concatenate([[0], np.cumsum(sz * sz)]).astype(np.int64)).to(DEV)
    thr = np.ascontiguousarray(thr, dtype=np.float64)
    i32 = lambda n, fill=-7: torch.full((n,), fill, dtype=torch.int32, device=DEV)
    o = dict(row_ptr=i32(N + 1), neighbours=i32(TU.MAX_DEGREE * N), degree=i32(N), overflow=i32(B),
             dist=torch.full((int((sz * sz).sum()),), 7, dtype=torch.int16, device=DEV), component=i32(N), fragments=i32(B),
             fp=torch.full((B, TU.n_keys(A, L)), -7, dtype=torch.int32, device=DEV))
    mx, st = int(max(sizes)), _lib.stream_ptr()
    _lib.check(lib.egnn_topo_bonds(st, B, N, A, _lib.ptr(p), _lib.ptr(t), _lib.ptr(gp), mx, C.c_void_p(thr.ctypes.data), _lib.ptr(o["row_ptr"]),
                                   _lib.ptr(o["neighbours"]), _lib.ptr(o["degree"]), _lib.ptr(o["overflow"])))
    opt = lambda k: _lib.ptr(o[k]) if k in want else None
    _lib.check(lib.egnn_topo_paths(st, B, N, A, _lib.ptr(t), _lib.ptr(gp), mx, _lib.ptr(o["row_ptr"]), _lib.ptr(o["neighbours"]),
                                   _lib.ptr(o["degree"]), _lib.ptr(o["overflow"]), L, opt("dist"), _lib.ptr(dptr), opt("component"),
                                   opt("fragments"), opt("fp")))
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["dist"] = out["dist"].view(np.uint16)
    out["neighbours"] = out["neighbours"][:out["row_ptr"][-1]]
    out["fp_device"] = o["fp"]
    return out


@functools.lru_cache(maxsize=None)
def _inputs(A):
    """every input of the host test with A types, as a list of graphs: the seeded clouds, and for A = 2 the hand-made graphs and
    the hand-computed lines too; every batch holds a graph of no atoms.  Each passes the gap check."""
    pos, types = TU.cloud(200 + A, TU.SIZES, A)
    thr = TU.thresholds(TU.RADII[A])
    graphs, lo = [], 0
    for n in TU.SIZES:
        graphs.append((pos[lo:lo + n], types[lo:lo + n]))
        lo += n
    if A == 2:
        graphs += list(TU.special_graphs().values()) + [TU.line("OSiO"), TU.line("OSi"), TU.line("OSiOSi"), TU.bondless(4)]
    else:
        graphs.append(TU.empty())                                          # (the hand-made graphs hold one too)
    for p, t in graphs:
        assert TU.gap_ok(p, t, thr), "ambiguous input: a distance on its threshold"
    return graphs, thr


@functools.lru_cache(maxsize=None)
def _host(A, reverse):
    graphs, thr = _inputs(A)
    pos, types, sizes = TU.join(graphs[::-1] if reverse else graphs)
    B = len(sizes)
    pairs = np.array([[g, (g + 1) % B] for g in range(B)] + [[g, g] for g in range(B)], dtype=np.int32)
    rc, want = TU.host(_lib.lib(), pos, types, sizes, A, thr, pairs=pairs)
    assert rc == 0
    return pos, types, sizes, thr, pairs, want


def _assert_bitwise(got, want, keys=TU.INT_KEYS):
    for k in keys:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("A", [1, 2, 3])
def test_device_equals_the_host_statement(A, reverse):
    pos, types, sizes, thr, pairs, want = _host(A, reverse)
    got = _device(pos, types, sizes, A, thr)
    _assert_bitwise(got, want)
    assert want["fp"].sum() > 1000 and (A != 2 or (want["overflow"].sum() == 34 and want["dist"].max() == 0xFFFF))
    k = sizes.index(0)                                                      # the empty graph: no fragment, written by the device too
    assert want["fragments"][k] == 0 and got["fragments"][k] == 0 and not got["fp"][k].any()
    n, fp = len(pairs), got["fp_device"]
    sim = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
    sa, sb = torch.full((n,), -7, dtype=torch.int64, device=DEV), torch.full((n,), -7, dtype=torch.int64, device=DEV)
    pr = torch.from_numpy(pairs).to(DEV)
    _lib.check(_lib.lib().egnn_topo_tanimoto(_lib.stream_ptr(), n, fp.shape[1], _lib.ptr(fp), len(sizes), _lib.ptr(fp), len(sizes),
                                             _lib.ptr(pr), _lib.ptr(sim), _lib.ptr(sa), _lib.ptr(sb)))
    assert np.array_equal(sim.cpu().numpy().view(np.int64), want["sim"].view(np.int64))      # the fp64 value, bit for bit
    assert np.array_equal(sa.cpu().numpy(), want["sa"]) and np.array_equal(sb.cpu().numpy(), want["sb"])
    B = len(sizes)
    own = want["sim"][B:]                                                   # a graph against itself: 1, or 0 where it has no pair
    assert np.array_equal(own, (want["sa"][B:] > 0).astype(np.float64)) and 0.0 in own and 1.0 in own
    assert 0.0 < want["sim"][5 if not reverse else B - 7] < 1.0


def test_long_paths_and_short_fingerprints():
    """L = 64 (the longest) and L = 1 on the hand-made graphs: the chain's distances go far beyond both"""
    pos, types, sizes = TU.join(list(TU.special_graphs().values()))
    for L in (64, 1):
        rc, want = TU.host(_lib.lib(), pos, types, sizes, 2, THR2, L=L)
        assert rc == 0
        _assert_bitwise(_device(pos, types, sizes, 2, THR2, L=L), want)
        assert want["fp"][0].sum() == sum(1024 - d for d in range(1, L + 1))


def test_a_large_graph_among_small_ones():
    """the 1024-atom chain first, then 2-atom graphs: uneven work per workgroup, and 14 of a small graph's 16 wavefronts idle"""
    graphs = [TU.chain(1024)] + [TU.line("OSi"), TU.line("OO", step=1.5), TU.line("SiSi", step=3.0)] * 7
    pos, types, sizes = TU.join(graphs)
    assert all(TU.gap_ok(p, t, THR2) for p, t in graphs)
    rc, want = TU.host(_lib.lib(), pos, types, sizes, 2, THR2)
    assert rc == 0 and want["dist"][1023] == 1023 and want["fragments"].tolist() == [1] + [1, 1, 2] * 7
    _assert_bitwise(_device(pos, types, sizes, 2, THR2), want)


def test_nullable_outputs_and_reproducibility():
    pos, types, sizes, thr, _, want = _host(2, False)
    full = _device(pos, types, sizes, 2, thr)
    again = _device(pos, types, sizes, 2, thr)
    _assert_bitwise(again, full)                                            # two calls are bitwise identical
    only_fp = _device(pos, types, sizes, 2, thr, want=("fp",))
    _assert_bitwise(only_fp, want, ("row_ptr", "neighbours", "degree", "overflow", "fp"))
    assert (only_fp["dist"] == 7).all() and (only_fp["component"] == -7).all() and (only_fp["fragments"] == -7).all()
    no_fp = _device(pos, types, sizes, 2, thr, want=("dist", "component", "fragments"))
    _assert_bitwise(no_fp, want, ("dist", "component", "fragments"))
    assert (no_fp["fp"] == -7).all()
    none = _device(pos, types, sizes, 2, thr, want=())
    _assert_bitwise(none, want, ("row_ptr", "neighbours", "degree", "overflow"))


def test_python_layer():
    graphs, thr = _inputs(2)
    keep = [g for g in graphs if len(g[1]) != 34]                           # all but the overflowing crowd
    pos, types, sizes = TU.join(keep)
    want = TU.batch(pos, types, sizes, 2, thr)
    p, oh = torch.from_numpy(pos).to(DEV), _onehot(types, 2).to(DEV)
    row_ptr, nb, deg = stats.bond_graph(p, oh, sizes)
    assert row_ptr.dtype == nb.dtype == deg.dtype == torch.int64
    assert np.array_equal(row_ptr.cpu().numpy(), want["row_ptr"]) and np.array_equal(nb.cpu().numpy(), want["neighbours"])
    assert np.array_equal(deg.cpu().numpy(), want["degree"])
    dist, frag, comp = stats.topological_distances(p, oh, sizes)
    flat = np.concatenate([d.cpu().numpy().reshape(-1) for d in dist])
    assert [tuple(d.shape) for d in dist] == [(n, n) for n in sizes] and flat.min() == -1
    assert np.array_equal(np.where(flat < 0, TU.UNREACHABLE, flat), want["dist"])
    assert np.array_equal(frag.cpu().numpy(), want["fragments"]) and np.array_equal(comp.cpu().numpy(), want["component"])
    assert 0 in sizes and int(frag[sizes.index(0)]) == 0                    # an empty graph among the others: no fragment
    fp = stats.atom_pair_fingerprint(p, oh, sizes)
    assert fp.dtype == torch.int32 and fp.shape == (len(sizes), 3150) and np.array_equal(fp.cpu().numpy(), want["fp"])
    assert stats.atom_pair_fingerprint(p, oh, sizes, max_length=3).shape == (len(sizes), 315)
    sim, sa, sb = stats.tanimoto(fp, fp.roll(1, 0))
    assert sim.dtype == torch.float64 and sa.dtype == torch.int64
    for g in range(len(sizes)):
        assert (float(sim[g]), int(sa[g]), int(sb[g])) == TU.tanimoto(want["fp"][g], want["fp"][g - 1]), g
    # wider radii change the graph; an atom above 32 bonds raises, naming the graph
    assert stats.bond_graph(p, oh, sizes, radii=(0.8, 1.3))[0][-1] > row_ptr[-1]
    crowd_p, crowd_t = TU.crowd(34)
    cp, coh = torch.from_numpy(np.concatenate([pos[:3], crowd_p])).to(DEV), _onehot(np.concatenate([types[:3], crowd_t]), 2).to(DEV)
    for fn in (stats.bond_graph, stats.topological_distances, stats.atom_pair_fingerprint):
        with pytest.raises(RuntimeError, match="graph 2"):
            fn(cp, coh, [1, 2, 34])
    with pytest.raises(ValueError, match="radii"):
        stats.bond_graph(p, oh, sizes, radii=(0.66, 1.11, 1.21))
    with pytest.raises(RuntimeError):
        stats.bond_graph(p.cpu(), oh.cpu(), sizes)
    with pytest.raises(_lib.EgnnError, match="max_length"):
        stats.atom_pair_fingerprint(p, oh, sizes, max_length=65)


def test_fingerprint_similarity():
    graphs, thr = _inputs(2)
    cloud65, cloud129, one_atom = graphs[5], graphs[6], graphs[0]
    rng = np.random.default_rng(2)
    perm = rng.permutation(129)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    moved = ((cloud129[0].astype(np.float64) @ q.T + [1.0, 2.0, -3.0]).astype(np.float32)[perm], cloud129[1][perm])
    assert TU.gap_ok(*moved, thr)
    assert np.array_equal(TU.bond_matrix(*moved, thr), TU.bond_matrix(*cloud129, thr)[perm][:, perm]), "rounding moved a bond"
    chain4 = TU.line("OSiOSi")
    stretched = (chain4[0] + np.array([[0, 0, 0]] * 3 + [[0.7, 0, 0]], dtype=np.float32), chain4[1])     # the last Si-O: 2.3 A > 2.124
    other65 = TU.cloud(77, [65], 2)
    originals = [cloud129, one_atom, chain4, chain4, cloud65]
    samples = [moved, one_atom, stretched, chain4, other65]
    assert all(TU.gap_ok(p, t, thr) for p, t in samples)
    rec = lambda pt, on, k=0: SimpleNamespace(pos=torch.from_numpy(pt[0]).to(on), x=_onehot(pt[1], 2).to(on), id=f"mp-{k}")
    decoy = rec(TU.line("OSiOSi", step=9.0), DEV)                           # an earlier state of a chain: only the LAST element counts
    sims, skipped = stats.fingerprint_similarity([rec(o, "cpu", k) for k, o in enumerate(originals)],
                                                 [[decoy, rec(s, DEV)] if len(s[1]) == 4 else [rec(s, DEV)] for s in samples])
    assert skipped == [1] and len(sims) == 4
    want = []
    for o, s in zip(originals, samples):
        if len(o[1]) == 1:
            continue
        fo, fs = (TU.batch(p, t, [len(t)], 2, thr)["fp"][0] for p, t in (o, s))
        want.append(TU.tanimoto(fo, fs)[0])
    assert sims == want
    assert sims[0] == 1.0 and sims[2] == 1.0 and sims[1] < 1.0 and 0.0 < sims[3] < 1.0
    # O-Si-O-Si against O-Si-O + a lone Si: {(O1,Si2,1): 2, (O1,O1,2): 1} shares (O1,Si2,1) once with the six keys of the chain
    assert sims[1] == 1 / 8
    assert stats.fingerprint_similarity([], []) == ([], [])
    # an atom above 32 bonds: the error names the side and the graph
    crowd, spread = TU.crowd(34), (TU.crowd(34)[0] * 4, TU.crowd(34)[1])
    assert TU.gap_ok(*spread, thr) and TU.batch(*spread, [34], 2, thr)["overflow"][0] == 0
    with pytest.raises(RuntimeError, match="generated graph 1"):
        stats.fingerprint_similarity([rec(chain4, "cpu"), rec(spread, "cpu")], [[rec(chain4, DEV)], [rec(crowd, DEV)]])
    with pytest.raises(RuntimeError, match="original graph 0"):
        stats.fingerprint_similarity([rec(crowd, "cpu"), rec(chain4, "cpu")], [[rec(spread, DEV)], [rec(chain4, DEV)]])

"""The paired walk of the persistent coordinate kernel (csrc/edge_x_m16.hip, csrc/x_walk.h): a workgroup runs share 0 and then share 1
of a tile and share 1 multiplies the first six activation chunks from the LDS buffers share 0 built them in; the remainder of fewer
tiles than workgroups is handed out as single units that build everything.  Arithmetic and order are those of the one-workgroup-per-unit
form (EGNN_X_PERSIST=0), so every output bit must agree -- checked at tile counts chosen from the device's CU count G, where the walk
changes shape: T = G + 1 (one sweep, remainder of one tile per XCD or none), 2G - 1 (remainder G - 1: nearly every workgroup runs single
units next to kept ones), 2G (no remainder at all), 2G + G/2 (remainder of half a sweep: one unit per workgroup).

tests/test_gpu_parity.py::test_persistent_coordinate_kernel_is_bitwise_the_per_tile_kernel keeps pinning ragged and irregular batches."""
import functools

import pytest
import torch

import diffusion_model_amd as dma
from oracle import egnn_ref
from tests._util import dims_for, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 36
TAIL = [37, 29, 5, 1, 2]          # ragged tail: 2,166 edges, a single-atom graph, a two-atom graph
ORACLE_GRAPHS = [64, 37]          # the first two graphs of every batch: compared with the fp32 oracle
TOL = {"bf16": 1e-2, "fp16": 2.5e-3}   # the bars of tests/test_gpu_parity.py (width sweep) against the fp32 oracle


def _edges(n):
    return n * (n - 1)


def sizes_for_tiles(T):
    """A fully connected batch of exactly T 128-edge tiles whose last tile is half full: a 64-atom graph, the ragged tail, as many 64-atom
    graphs (4,032 edges = 31.5 tiles each: tiles straddle graphs) as fit, then ever smaller graphs up to the target edge count."""
    target = T * 128 - 64
    sizes = [64] + TAIL
    rem = target - sum(_edges(n) for n in sizes)
    assert rem >= 0, T
    sizes += [64] * (rem // _edges(64))
    rem -= (rem // _edges(64)) * _edges(64)
    while rem >= 2:
        n = 63
        while _edges(n) > rem:
            n -= 1
        sizes.append(n)
        rem -= _edges(n)
    E = sum(_edges(n) for n in sizes)
    assert (E + 127) // 128 == T and E % 128 != 0, (T, E)
    return sizes, E


def _net(sd, d, precision):
    net = dma.EquivariantGNN(2, d["m_input"], d["m_hidden"], d["m_output"], d["x_input"], d["x_hidden"], d["x_output"], d["h_input"],
                             d["h_hidden"], d["h_output"])
    net.load_state_dict(sd)
    net.to(DEV).eval()
    net.precision, net.norm_scope = precision, "graph"
    net.egcl_list[0].precision, net.egcl_list[0].norm_scope = precision, "graph"   # (a layer called alone runs on its own settings)
    return net


@functools.lru_cache(maxsize=None)
def _model(wx):
    d = dims_for(H, 256, wx, wx, 128)
    return d, egnn_ref.init_state_dict(2, **d, seed=5)


@functools.lru_cache(maxsize=None)
def _oracle_inputs():
    g = torch.Generator().manual_seed(11)
    n = sum(ORACLE_GRAPHS)
    return torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g)


@functools.lru_cache(maxsize=None)
def _oracle(wx):
    """fp32 oracle of the first two graphs (per-graph normalisation: their outputs do not depend on the rest of the batch), after one
    layer and after two; computed once for all tile counts and precisions"""
    d, sd = _model(wx)
    h, x = _oracle_inputs()
    ptr = torch.tensor([0, ORACLE_GRAPHS[0], sum(ORACLE_GRAPHS)])
    _, _, outs = egnn_ref.egnn_forward(sd, egnn_ref.fully_connected_edge_index(ORACLE_GRAPHS), h, x, norm_scope="graph", graph_ptr=ptr,
                                       return_layers=True)
    return outs


def _batch(sizes):
    n, n0 = sum(sizes), sum(ORACLE_GRAPHS)
    h0, x0 = _oracle_inputs()
    g = torch.Generator().manual_seed(4)
    h = torch.cat([h0, torch.randn(n - n0, H, generator=g)]).to(DEV)
    x = torch.cat([x0, torch.randn(n - n0, 3, generator=g)]).to(DEV)
    ei = dma.fully_connected_edge_index(sizes, device=DEV)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
    return ei, h, x, batch


def _run(net, ei, h, x, batch):
    with torch.no_grad():
        h1, x1 = net.egcl_list[0](ei, h, x, batch=batch)
        h2, x2 = net(ei, h, x, batch=batch)
    torch.cuda.synchronize()
    return [t.cpu() for t in (h1, x1, h2, x2)]


NAMES = ("h layer 1", "x layer 1", "h", "x")


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("which", ["G+1", "2G-1", "2G", "2G+G/2"])
def test_paired_walk_is_bitwise_the_per_unit_kernel(which, precision, monkeypatch):
    """wx = 1024 (two shares), one layer and two: persistent == per-unit form bit for bit, and both graphs of the oracle within the
    precision's bar.  The remainder as single units (G + 1, 2G - 1, 2G + G/2), an empty remainder (2G), kept-chunk and plain units in
    one launch, a half-full last tile, tiles that straddle graphs."""
    G = torch.cuda.get_device_properties(0).multi_processor_count
    T = {"G+1": G + 1, "2G-1": 2 * G - 1, "2G": 2 * G, "2G+G/2": 2 * G + G // 2}[which]
    assert 2 * T > 2 * G, "above the persistent threshold"
    sizes, _ = sizes_for_tiles(T)
    assert sizes[:2] == ORACLE_GRAPHS
    d, sd = _model(1024)
    net = _net(sd, d, precision)
    ei, h, x, batch = _batch(sizes)
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("EGNN_X_PERSIST", flag)
        out[flag] = _run(net, ei, h, x, batch)
    for a, b, name in zip(out["1"], out["0"], NAMES):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), f"T = {T}, {name}: paired walk and per-unit kernel differ (max {float((a - b).abs().max()):.3e})"
    n0 = sum(ORACLE_GRAPHS)
    (h1r, x1r), (h2r, x2r) = _oracle(1024)
    x0 = _oracle_inputs()[1]
    h1, x1, h2, x2 = (t[:n0] for t in out["1"])
    for got, ref, name in ((h1, h1r, "h layer 1"), (x1 - x0, x1r - x0, "eps_x layer 1"), (h2, h2r, "h"), (x2 - x0, x2r - x0, "eps_x")):
        e = rel_err(got, ref)
        print(f"x pair T = {T} {precision} {name}: rel err {e:.2e}")
        assert e <= TOL[precision], (T, precision, name, e)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_paired_walk_run_to_run(precision, monkeypatch):
    """two calls on the same inputs: bitwise equal (the kept buffers of one launch leave nothing behind for the next)"""
    monkeypatch.setenv("EGNN_X_PERSIST", "1")
    G = torch.cuda.get_device_properties(0).multi_processor_count
    sizes, _ = sizes_for_tiles(2 * G - 1)
    d, sd = _model(1024)
    net = _net(sd, d, precision)
    ei, h, x, batch = _batch(sizes)
    first, second = _run(net, ei, h, x, batch), _run(net, ei, h, x, batch)
    for a, b, name in zip(first, second, NAMES):
        assert torch.isfinite(a).all() and torch.equal(a, b), name


def test_one_share_still_walks_persistently_and_bitwise(monkeypatch):
    """wx = 512: one share per tile, no kept chunks; the persistent form is still chosen (more than two units per CU) and still bitwise
    the per-unit form"""
    G = torch.cuda.get_device_properties(0).multi_processor_count
    T = 2 * G + G // 2 + 1
    assert T * 1 > 2 * G
    sizes, _ = sizes_for_tiles(T)
    d, sd = _model(512)
    net = _net(sd, d, "bf16")
    ei, h, x, batch = _batch(sizes)
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("EGNN_X_PERSIST", flag)
        out[flag] = _run(net, ei, h, x, batch)
    for a, b, name in zip(out["1"], out["0"], NAMES):
        assert torch.isfinite(a).all() and torch.equal(a, b), name

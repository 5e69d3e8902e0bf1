"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI, against
the CPU oracle and the committed golden vectors.

Tolerances
  fp32 path  : 1e-4 relative (BASELINE.json north_star); measured errors are ~1e-6.
  bf16 path  : MFMA operands are rounded to bf16 (8 significant bits) with fp32 accumulation;
               1e-2 relative to the oracle on eps (measured 2-4e-3), stated in each test.
  bf16x3 path: head + remainder operands on the bf16 matrix cores: 1e-4 as the fp32 path.
"""
import math

import numpy as np
import pytest
import torch

import diffusion_model_amd as dma
from oracle import egnn_ref
from oracle.diffusion_ref import DiffusionRef
from oracle.sampler_ref import sample_one_graph
from tests._util import dims_for, golden_case, load_golden, max_rel, rel_err

pytestmark = pytest.mark.gpu
G_EGNN = load_golden("egnn_golden.npz")
G_DIFF = load_golden("diffusion_golden.npz")
EGNN_CASES = [str(c) for c in G_EGNN["cases"]]
DEV = "cuda"


def build_net(sd, d, L, precision="fp32", norm_scope="call"):
    net = dma.EquivariantGNN(L, d["m_input"], d["m_hidden"], d["m_output"], d["x_input"], d["x_hidden"],
                             d["x_output"], d["h_input"], d["h_hidden"], d["h_output"])
    net.load_state_dict(sd)
    net.to(DEV).eval()
    net.precision, net.norm_scope = precision, norm_scope
    return net


@pytest.mark.parametrize("tag", EGNN_CASES)
def test_egnn_fp32_matches_reference_golden(tag):
    sd, h, x, sizes, layers, d = golden_case(G_EGNN, tag)
    L = len(layers)
    net = build_net(sd, d, L)
    ei = dma.fully_connected_edge_index(sizes, device=DEV)
    with torch.no_grad():
        h_o, x_o = net(ei, h.to(DEV), x.to(DEV))
    assert max_rel(h_o.cpu(), layers[-1][0]) <= 1e-4
    assert max_rel(x_o.cpu(), layers[-1][1]) <= 1e-4
    # per-layer: run the single-layer module chain
    hh, xx = h.to(DEV), x.to(DEV)
    with torch.no_grad():
        for l in range(L):
            hh, xx = net.egcl_list[l](ei, hh, xx)
            assert max_rel(hh.cpu(), layers[l][0]) <= 1e-4, f"layer {l} h"
            assert max_rel(xx.cpu(), layers[l][1]) <= 1e-4, f"layer {l} x"


@pytest.mark.parametrize("tag", EGNN_CASES)
def test_egnn_bf16_close_to_oracle(tag):
    """every golden case: the full-width ones of <= 2,048 / 6,144 edges (full_g16x3, full_toy2x4_H3 / full_g64) run the 32- / 64-row
    small-graph kernels of csrc/edge_small.hip in bf16, the narrow ones the generic bf16 kernel"""
    sd, h, x, sizes, layers, d = golden_case(G_EGNN, tag)
    net = build_net(sd, d, len(layers), precision="bf16")
    ei = dma.fully_connected_edge_index(sizes, device=DEV)
    with torch.no_grad():
        h_o, x_o = net(ei, h.to(DEV), x.to(DEV))
    # bf16 operands (8 significant bits), fp32 accumulation: 1e-2 on the layer outputs / eps (measured 2-4e-3)
    eh, ex = rel_err(h_o.cpu(), layers[-1][0]), rel_err(x_o.cpu() - x, layers[-1][1] - x)
    print(f"bf16 {tag}: h {eh:.2e} eps_x {ex:.2e}")
    assert eh <= 1e-2 and ex <= 1e-2
    assert torch.isfinite(h_o).all() and torch.isfinite(x_o).all()


@pytest.mark.parametrize("tag", EGNN_CASES)
def test_egnn_bf16x3_matches_reference_golden(tag):
    """precision 'bf16x3' (head + remainder operands on the bf16 matrix cores; shapes outside the 128-edge tiling run the
    fp32 kernels) against the reference goldens at north_star's 1e-4, final outputs and every layer."""
    sd, h, x, sizes, layers, d = golden_case(G_EGNN, tag)
    L = len(layers)
    net = build_net(sd, d, L, precision="bf16x3")
    ei = dma.fully_connected_edge_index(sizes, device=DEV)
    with torch.no_grad():
        h_o, x_o = net(ei, h.to(DEV), x.to(DEV))
    eh, ex = max_rel(h_o.cpu(), layers[-1][0]), max_rel(x_o.cpu(), layers[-1][1])
    print(f"bf16x3 {tag}: h {eh:.2e} x {ex:.2e}")
    assert eh <= 1e-4 and ex <= 1e-4
    hh, xx = h.to(DEV), x.to(DEV)
    with torch.no_grad():
        for l in range(L):
            net.egcl_list[l].precision = "bf16x3"   # the single-layer modules carry their own precision attribute
            hh, xx = net.egcl_list[l](ei, hh, xx)
            assert max_rel(hh.cpu(), layers[l][0]) <= 1e-4, f"layer {l} h"
            assert max_rel(xx.cpu(), layers[l][1]) <= 1e-4, f"layer {l} x"


# precision 'f16c8' (csrc/edge_f16c8.hip): fp16 heads on v_mfma_f32_16x16x32_f16 + both remainder products on one block-scaled
# e4m3 instruction: north_star's 1e-4 for two bf16-equivalents of matrix work per product.  Measured (profiles/r05b_prec_errors_
# f16c8_first.log, tools/prec_errors.py): 9.2e-6 / 5.6e-6 / 3.5e-5 max-relative on the three full-width goldens (the CPU emulation
# of its roundings, tools/rounding_budget.py, predicts 6e-6 / 5e-6 / 4e-5); the bar here is 5e-5, per layer 1e-4.
F16C8_TOL = 5e-5
@pytest.mark.parametrize("tag", EGNN_CASES)
def test_egnn_f16c8_matches_reference_golden(tag):
    sd, h, x, sizes, layers, d = golden_case(G_EGNN, tag)
    L = len(layers)
    net = build_net(sd, d, L, precision="f16c8")
    ei = dma.fully_connected_edge_index(sizes, device=DEV)
    with torch.no_grad():
        h_o, x_o = net(ei, h.to(DEV), x.to(DEV))
    eh, ex = max_rel(h_o.cpu(), layers[-1][0]), max_rel(x_o.cpu(), layers[-1][1])
    ee = rel_err(x_o.cpu() - x, layers[-1][1] - x)
    print(f"f16c8 {tag}: h {eh:.2e} x {ex:.2e} eps_x {ee:.2e}")
    assert eh <= F16C8_TOL and ex <= F16C8_TOL and ee <= F16C8_TOL
    hh, xx = h.to(DEV), x.to(DEV)
    with torch.no_grad():
        for l in range(L):
            net.egcl_list[l].precision = "f16c8"   # the single-layer modules carry their own precision attribute
            hh, xx = net.egcl_list[l](ei, hh, xx)
            assert max_rel(hh.cpu(), layers[l][0]) <= 1e-4, f"layer {l} h"
            assert max_rel(xx.cpu(), layers[l][1]) <= 1e-4, f"layer {l} x"


def test_f16c8_saturates_instead_of_overflowing():
    """the fp16 and e4m3 conversions saturate (MODE.FP16_OVFL) instead of producing inf / the e4m3 NaN on overflow: activations
    beyond both ranges stay finite, as in precision fp16 (test_fp16_saturates_instead_of_overflowing).  (Like every half-precision
    path of the library -- the fp16 table of bf16 / fp16 clamps, the split node MLP clamps -- f16c8 does NOT promise that a NaN in
    the INPUT of a forward call comes out as a NaN: tools/nan_probe.py; the sampler checks its state after every step instead,
    INTEGRATION.md.)"""
    sd, h, x, sizes, layers, d = golden_case(G_EGNN, "full_g64")
    net = build_net(sd, d, len(layers), precision="f16c8")
    ei = dma.fully_connected_edge_index(sizes, device=DEV)
    with torch.no_grad():
        h_o, x_o = net(ei, (h * 3.0e4).to(DEV), x.to(DEV))
    assert torch.isfinite(h_o).all() and torch.isfinite(x_o).all()


# precision 'fp16': the bf16 path's kernels on fp16 MFMA operands (11 significant bits instead of 8, same matrix-core rate)
# + the split-operand node MLP.  Tolerances set from tools/prec_errors.py on the GPU (profiles/r04b_prec_errors.log: the
# three full-width goldens 3.1e-4 / 2.2e-4 / 1.1e-3 max-relative, eps_x L2 3.4e-4 / 5.2e-4 / 1.7e-3; bf16: 3.7-4.5e-3 / 5-7e-3).
FP16_TOL = 2.5e-3
@pytest.mark.parametrize("tag", EGNN_CASES)
def test_egnn_fp16_against_reference_golden(tag):
    """Full-width cases run the fp16-operand kernels (edge_x_m16_kernel<false, f16x8>, edge_kernel_bf16_v4<1, true, false, false, f16x8>,
    node_post_bf16_kernel<., f16x8>); the other widths fall to the exact fp32 kernels (include/egnn_amd.h EGNN_PREC_F16)."""
    sd, h, x, sizes, layers, d = golden_case(G_EGNN, tag)
    net = build_net(sd, d, len(layers), precision="fp16")
    ei = dma.fully_connected_edge_index(sizes, device=DEV)
    with torch.no_grad():
        h_o, x_o = net(ei, h.to(DEV), x.to(DEV))
    eh, ex = max_rel(h_o.cpu(), layers[-1][0]), max_rel(x_o.cpu(), layers[-1][1])
    ee = rel_err(x_o.cpu() - x, layers[-1][1] - x)
    print(f"fp16 {tag}: h {eh:.2e} x {ex:.2e} eps_x {ee:.2e}")
    full_width = d["x_hidden"] in (512, 1024) and d["m_hidden"] % 64 == 0 and d["m_output"] == 256
    tol = FP16_TOL if full_width else 1e-4
    assert eh <= tol and ex <= tol and ee <= tol
    assert torch.isfinite(h_o).all() and torch.isfinite(x_o).all()


def test_fp16_saturates_instead_of_overflowing():
    """Activations beyond the fp16 range (65504) must saturate (MODE.FP16_OVFL in the fp16 kernels), not become inf: an
    infinite operand times a zero weight would be NaN where the bf16 path stays finite."""
    sd, h, x, sizes, layers, d = golden_case(G_EGNN, "full_g64")
    net = build_net(sd, d, len(layers), precision="fp16")
    big = build_net(sd, d, len(layers), precision="bf16")
    ei = dma.fully_connected_edge_index(sizes, device=DEV)
    hh = (h * 3.0e4).to(DEV)      # first-layer pre-activations ~1e5: the fp16 table saturates at 32000, SiLU outputs ~6e4..1e5
    with torch.no_grad():
        h_o, x_o = net(ei, hh, x.to(DEV))
        h_b, x_b = big(ei, hh, x.to(DEV))
    assert torch.isfinite(h_o).all() and torch.isfinite(x_o).all()
    assert torch.isfinite(h_b).all() and torch.isfinite(x_b).all()


def test_norm_scope_graph_equals_single_graph_calls_on_gpu():
    sd, h, x, sizes, layers, d = golden_case(G_EGNN, "g16x3_H36")
    L = len(layers)
    net = build_net(sd, d, L, norm_scope="graph")
    ei = dma.fully_connected_edge_index(sizes, device=DEV)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
    with torch.no_grad():
        hb, xb = net(ei, h.to(DEV), x.to(DEV), batch=batch)
    ptr = torch.tensor([0] + list(np.cumsum(sizes)))
    ho, xo = egnn_ref.egnn_forward(sd, egnn_ref.fully_connected_edge_index(sizes), h, x, "graph", ptr)
    assert max_rel(hb.cpu(), ho) <= 1e-4 and max_rel(xb.cpu(), xo) <= 1e-4
    single = build_net(sd, d, L, norm_scope="call")
    off = 0
    for n in sizes:
        e1 = dma.fully_connected_edge_index(n, device=DEV)
        with torch.no_grad():
            h1, x1 = single(e1, h[off:off + n].to(DEV), x[off:off + n].to(DEV))
        assert max_rel(hb[off:off + n], h1) <= 1e-4 and max_rel(xb[off:off + n], x1) <= 1e-4
        off += n


def _random_graph(n, e, seed, self_loops=True):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, e), generator=g)
    if not self_loops:
        ei = ei[:, ei[0] != ei[1]]
    return ei


@pytest.mark.parametrize("n,e,seed", [(40, 300, 1), (200, 9000, 2), (7, 0, 3), (130, 129 * 130, 4)])
def test_generic_edge_lists_unsorted_duplicates_isolated(n, e, seed):
    """Arbitrary edge_index: unsorted, duplicate edges, self loops, nodes without edges, nodes whose
    degree exceeds the tile (partial-sum path), and E = 0."""
    sd, _, _, _, layers, d = golden_case(G_EGNN, "g8_H36")
    L = len(layers)
    net = build_net(sd, d, L)
    g = torch.Generator().manual_seed(100 + seed)
    h, x = torch.randn(n, 36, generator=g), torch.randn(n, 3, generator=g)
    if e == 129 * 130:
        ei = egnn_ref.fully_connected_edge_index(n)       # degree 129 > 64-row tile
    else:
        ei = _random_graph(n, e, seed)
        if e:
            ei[0, : e // 3] = 5                            # one hub node with a very large in-degree
    with torch.no_grad():
        h_o, x_o = net(ei.to(DEV), h.to(DEV), x.to(DEV))
    ho, xo = egnn_ref.egnn_forward(sd, ei, h, x)
    assert max_rel(h_o.cpu(), ho) <= 1e-4
    assert max_rel(x_o.cpu(), xo) <= 1e-4


def test_bitwise_deterministic_and_inputs_untouched():
    sd, h, x, sizes, layers, d = golden_case(G_EGNN, "g64_H36")
    net = build_net(sd, d, len(layers), precision="bf16")
    ei = dma.fully_connected_edge_index(sizes, device=DEV)
    hd, xd = h.to(DEV), x.to(DEV)
    with torch.no_grad():
        a = net(ei, hd, xd)
        b = net(ei, hd, xd)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(hd.cpu(), h) and torch.equal(xd.cpu(), x)


def _rot(seed):
    g = torch.Generator().manual_seed(seed)
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g))
    q = q * torch.sign(torch.diagonal(r))
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def c2_inputs(batch, n_atoms=64, H=36, seed=0):
    """Synthetic 64-atom SiO2-like cells of SURVEY 8(d): jittered 4x4x4 grid, spacing 1.6 A."""
    g = torch.Generator().manual_seed(seed)
    side = round(n_atoms ** (1 / 3))
    grid = torch.stack(torch.meshgrid(*[torch.arange(side, dtype=torch.float32)] * 3, indexing="ij"), -1).reshape(-1, 3) * 1.6
    pos = grid.repeat(batch, 1) + 0.1 * torch.randn(batch * n_atoms, 3, generator=g)
    pos = pos - pos.view(batch, n_atoms, 3).mean(1, keepdim=True).repeat_interleave(n_atoms, 0).view(-1, 3)
    types = torch.zeros(n_atoms, 2)
    types[0, 0] = 1
    types[1:22, 1] = 1
    types[22:, 0] = 1
    h = torch.zeros(batch * n_atoms, H)
    h[:, :2] = types.repeat(batch, 1)
    h[:, 2:H - 2] = torch.randn(batch * n_atoms, H - 4, generator=g)
    h[::n_atoms, H - 2] = 1.0
    h[:, H - 1] = 0.5
    return h, pos


# tolerances: fp32 and bf16x3 1e-4 (north_star; measured 2e-6 / 4e-6).  bf16 on this UNTRAINED, untamed 4-layer stack
# (default init: the coordinate head amplifies): 3e-2 against the oracle (measured 1.1e-2), 1e-2 under a rotation
# (measured 3.1e-3), 4e-3 under a permutation of graphs (measured 1.3e-3: fp32 summation-order differences of tile
# partials flip the bf16 rounding of later layers' operands); r03c run, printed by the test
# fp16 (profiles/r04b_prec_errors.log): oracle 4.6e-4 -> 1.5e-3, rotation 1.7e-4 -> 6e-4, permutation 4.2e-5 -> 2e-4.
# The permutation difference of the half-precision paths is an avalanche of operand-rounding flips seeded by fp32
# re-association (a graph's 4032 edges start at another tile offset): per layer, bf16 -- segment sums 4e-8 (pure fp32
# re-association) -> h' 2.9e-5 (node MLP operands re-rounded) -> 2.4e-4 -> 5.3e-4 -> 1.2e-3; the 32x32x16 kernels of commit
# aadce9a give the same table (profiles/r04a_perm_table_aadce9a_32x32x16.log), fp32 and bf16x3 stay at 0 / 3e-7;
# test_graph_permutation_seed_is_fp32_reassociation asserts the seed.
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16x3", 1e-4), ("f16c8", 1e-4), ("bf16", 3e-2), ("fp16", 1.5e-3)])
def test_full_size_c2_properties(precision, tol):
    """BASELINE configs[1] size (256 graphs x 64 atoms, L=4, widths 1024/256): size-independent
    properties -- E(3) equivariance, graph-permutation equivariance, batch == single-graph calls --
    plus a spot check of two graphs against the oracle."""
    B, n = 256, 64
    d = dims_for(36, 256, 1024, 1024, 1024)
    torch.manual_seed(2024)
    net = dma.EquivariantGNN(4, **d).to(DEV).eval()
    net.precision, net.norm_scope = precision, "graph"
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    h, x = c2_inputs(B)
    sizes = [n] * B
    ei = dma.fully_connected_edge_index(sizes, device=DEV)
    batch = torch.arange(B).repeat_interleave(n).to(DEV)
    with torch.no_grad():
        h0, x0 = net(ei, h.to(DEV), x.to(DEV), batch=batch)
        R, tvec = _rot(5), torch.tensor([0.7, -0.2, 1.1])
        h1, x1 = net(ei, h.to(DEV), (x @ R.T + tvec).to(DEV), batch=batch)
    assert torch.isfinite(h0).all() and torch.isfinite(x0).all()
    etol = {"bf16": 1e-2, "fp16": 6e-4}.get(precision, 1e-4)
    e_rot = max(rel_err(h1.cpu(), h0.cpu()), rel_err((x1.cpu() - (x @ R.T + tvec)), (x0.cpu() - x) @ R.T))
    # permuting whole graphs permutes the outputs (up to the fp32 summation order of tile partials: a
    # graph's 4032 edges need not start on a tile boundary)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3))
    idx = (perm.repeat_interleave(n) * n + torch.arange(n).repeat(B))
    with torch.no_grad():
        h2, x2 = net(ei, h[idx].to(DEV), x[idx].to(DEV), batch=batch)
    ptol = {"bf16": 4e-3, "fp16": 2e-4}.get(precision, 1e-5)
    e_perm = max(rel_err(h2.cpu(), h0.cpu()[idx]), rel_err(x2.cpu(), x0.cpu()[idx]))
    # oracle spot check on graphs 0 and 137
    e1 = egnn_ref.fully_connected_edge_index(n)
    e_or = 0.0
    for gidx in (0, 137):
        sl = slice(gidx * n, (gidx + 1) * n)
        ho, xo = egnn_ref.egnn_forward(sd, e1, h[sl], x[sl])
        e_or = max(e_or, rel_err(h0[sl].cpu(), ho), rel_err(x0[sl].cpu() - x[sl], xo - x[sl]))
    print(f"C2 {precision}: rotation {e_rot:.2e}  permutation {e_perm:.2e}  oracle {e_or:.2e}")
    assert e_rot <= etol and e_perm <= ptol and e_or <= tol


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_graph_permutation_seed_is_fp32_reassociation(precision):
    """a permutation of whole graphs changes a half-precision result by ~1e-3 after four layers.  The
    cause must be rounding flips seeded by fp32 re-association, not position-dependent indexing: after ONE edge pass on
    identical (permuted) inputs the three segment sums -- the only thing a graph's tile offset can touch -- agree to 1e-6
    (measured 4.4e-8 / 4.7e-8 / 2.9e-8: profiles/r04a_prec_errors.log), in every graph, wherever it sits."""
    from diffusion_model_amd import _lib
    B, n = 256, 64
    d = dims_for(36, 256, 1024, 1024, 1024)
    torch.manual_seed(2024)
    net = dma.EquivariantGNN(4, **d).to(DEV).eval()
    layer = net.egcl_list[0]
    layer.precision, layer.norm_scope = precision, "graph"
    h, x = c2_inputs(B)
    ei = dma.fully_connected_edge_index([n] * B, device=DEV)
    batch = torch.arange(B).repeat_interleave(n).to(DEV)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3))
    idx = (perm.repeat_interleave(n) * n + torch.arange(n).repeat(B))

    def sums(hh, xx):
        with torch.no_grad():
            layer(ei, hh.to(DEV), xx.to(DEV), batch=batch)
        sm, sx, S = torch.empty(B * n, 256, device=DEV), torch.empty(B * n, 3, device=DEV), torch.empty(B, device=DEV)
        _lib.check(_lib.lib().egcl_read_aggregates(layer._ctx.handle, _lib.stream_ptr(), _lib.NORM_GRAPH, _lib.ptr(sm),
                                                   _lib.ptr(sx), _lib.ptr(S)))
        return sm.cpu(), sx.cpu(), S.cpu()

    a, b = sums(h, x), sums(h[idx], x[idx])
    errs = (rel_err(b[0], a[0][idx]), rel_err(b[1], a[1][idx]), rel_err(b[2], a[2][perm]))
    per_graph = ((b[0] - a[0][idx]).view(B, -1).norm(dim=1) / a[0][idx].view(B, -1).norm(dim=1)).max()
    print(f"permutation, layer-1 segment sums {precision}: m {errs[0]:.1e} x {errs[1]:.1e} d2 {errs[2]:.1e}; worst graph {float(per_graph):.1e}")
    assert max(errs) <= 1e-6 and float(per_graph) <= 1e-6


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16x3", 1e-4), ("f16c8", 1e-4), ("bf16", 3e-2), ("fp16", 3e-3)])
def test_full_size_c3_properties(precision, tol):
    """BASELINE configs[2] size at FULL width (32 graphs x 512 atoms, E = 8,372,224, L=4, widths 1024/256: for bf16
    the persistent edge_x_m16_kernel<false, bf16x8, true> and edge_kernel_bf16_v4<1, true> on degree-511 rows, 4 tiles per
    receiving node): E(3)
    equivariance, graph-permutation equivariance, run-to-run bitwise determinism, and one whole 512-atom graph
    against the oracle (261,632 edges x 4 layers on the CPU)."""
    B, n = 32, 512
    d = dims_for(36, 256, 1024, 1024, 1024)
    torch.manual_seed(2024)
    net = dma.EquivariantGNN(4, **d)
    with torch.no_grad():      # 8x more messages per node than the 64-atom cell: keep the untrained stack in range
        for layer in net.egcl_list:
            layer.mlp_m[2].weight.mul_(64.0 / n)
            layer.mlp_m[2].bias.mul_(64.0 / n)
    net.to(DEV).eval()
    net.precision, net.norm_scope = precision, "graph"
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(1234)
    grid = torch.stack(torch.meshgrid(*[torch.arange(8, dtype=torch.float32)] * 3, indexing="ij"), -1).reshape(-1, 3) * 1.6
    x = grid.repeat(B, 1) + 0.1 * torch.randn(B * n, 3, generator=g)
    x = x - x.view(B, n, 3).mean(1, keepdim=True).expand(B, n, 3).reshape(-1, 3)
    h = torch.randn(B * n, 36, generator=g)
    h[:, 35] = 0.5
    plan = dma.fully_connected_plan([n] * B, DEV)
    assert plan.E == 8372224
    ei, batch = dma.plan_edge_index(plan), plan.batch
    with torch.no_grad():
        h0, x0 = net(ei, h.to(DEV), x.to(DEV), batch=batch)
        h0b, x0b = net(ei, h.to(DEV), x.to(DEV), batch=batch)
        R, tvec = _rot(6), torch.tensor([-0.3, 0.9, 0.4])
        h1, x1 = net(ei, h.to(DEV), (x @ R.T + tvec).to(DEV), batch=batch)
    assert torch.isfinite(h0).all() and torch.isfinite(x0).all()
    assert torch.equal(h0, h0b) and torch.equal(x0, x0b)
    etol = {"bf16": 1e-2, "fp16": 2e-3}.get(precision, 1e-4)
    e_rot = max(rel_err(h1.cpu(), h0.cpu()), rel_err((x1.cpu() - (x @ R.T + tvec)), (x0.cpu() - x) @ R.T))
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(4))
    idx = (perm.repeat_interleave(n) * n + torch.arange(n).repeat(B))
    with torch.no_grad():
        h2, x2 = net(ei, h[idx].to(DEV), x[idx].to(DEV), batch=batch)
    # every 512-atom graph starts on a tile boundary (261,632 = 2044 x 128), so a permutation of graphs is exact
    e_perm = max(rel_err(h2.cpu(), h0.cpu()[idx]), rel_err(x2.cpu(), x0.cpu()[idx]))
    gidx = 17
    sl = slice(gidx * n, (gidx + 1) * n)
    ho, xo = egnn_ref.egnn_forward(sd, egnn_ref.fully_connected_edge_index(n), h[sl], x[sl])
    e_or = max(rel_err(h0[sl].cpu(), ho), rel_err(x0[sl].cpu() - x[sl], xo - x[sl]))
    print(f"C3 {precision}: rotation {e_rot:.2e}  permutation {e_perm:.2e}  oracle {e_or:.2e}")
    assert e_rot <= etol and e_perm <= 1e-5 and e_or <= tol


@pytest.mark.parametrize("tag", ["T1000", "T50", "T200"])
def test_diffusion_steps_match_reference_golden(tag):
    T, p, s = G_DIFF[f"{tag}.params"]
    proc = dma.E3DiffusionProcess(float(s), float(p), int(T))
    z3, e3 = torch.from_numpy(G_DIFF[f"{tag}.z3"]).to(DEV), torch.from_numpy(G_DIFF[f"{tag}.e3"]).to(DEV)
    z2, e2 = torch.from_numpy(G_DIFF[f"{tag}.z2"]).to(DEV), torch.from_numpy(G_DIFF[f"{tag}.e2"]).to(DEV)
    for t in [int(v) for v in G_DIFF[f"{tag}.ts"]]:
        f = lambda k: torch.from_numpy(G_DIFF[f"{tag}.{k}.t{t}"])
        # fp32 elementwise arithmetic with pre-divided constants: 1e-5 relative to the largest entry
        assert max_rel(proc.calculate_mu(z3, e3, t).cpu(), f("mu3")) <= 1e-5
        assert max_rel(proc.calculate_mu(z2, e2, t).cpu(), f("mu2")) <= 1e-5
        got = proc.reverse_diffuse_one_step(z3, e3, t, mode="pos", noise=f("noise_pos").to(DEV))
        assert max_rel(got.cpu(), f("rev_pos")) <= 1e-5
        got = proc.reverse_diffuse_one_step(z2, e2, t, mode="h", noise=f("noise_h").to(DEV))
        assert max_rel(got.cpu(), f("rev_h")) <= 1e-5
    xo = dma.diffusion.E3DiffusionProcessXOnly(float(s), float(p), int(T))
    t = int(G_DIFF[f"{tag}.ts"][2])
    mu = xo.calculate_mu(z3, e3, t)
    assert max_rel(mu.cpu(), torch.from_numpy(G_DIFF[f"{tag}.mu3_xhat.t{t}"])) <= 1e-4
    got = xo.reverse_diffuse_one_step(mu, t, noise=torch.from_numpy(G_DIFF[f"{tag}.noise_xhat.t{t}"]).to(DEV))
    assert max_rel(got.cpu(), torch.from_numpy(G_DIFF[f"{tag}.rev_xhat.t{t}"])) <= 1e-4
    # forward noising with torch's RNG on the device: statistics only
    zt, noise = proc.diffuse_zero_to_t(z3, t, mode="pos")
    assert noise.mean(0).abs().max() < 1e-5
    assert max_rel(zt.cpu(), (proc.alpha(t) * z3.cpu() + proc.sigma(t) * noise.cpu())) <= 1e-5
    # ... and with the reference's own recorded draw (goldens fwd_*: executed diffuse_zero_to_t, :51-59)
    z2 = torch.from_numpy(G_DIFF[f"{tag}.z2"]).to(DEV)
    for t in [int(v) for v in G_DIFF[f"{tag}.ts"]]:
        for mode, z in (("pos", z3), ("h", z2)):
            draw = torch.from_numpy(G_DIFF[f"{tag}.fwd_noise_{mode}.t{t}"]).to(DEV)
            zt, used = proc.diffuse_zero_to_t(z, t, mode=mode, noise=draw)
            assert max_rel(used.cpu(), torch.from_numpy(G_DIFF[f"{tag}.fwd_used_{mode}.t{t}"])) <= 1e-6, (mode, t)
            assert max_rel(zt.cpu(), torch.from_numpy(G_DIFF[f"{tag}.fwd_{mode}.t{t}"])) <= 1e-5, (mode, t)


def test_egnn_eps_matches_reference_callers():
    """egnn_eps of the C ABI: eps_x = remove_mean(x_L - x_in [, batch]), eps_h = h_L[:, :A]
    (parts/train_per_iretation.py:161-163, :367-369) against the oracle's remove_mean (pinned by the rm.* goldens)."""
    from diffusion_model_amd import _lib
    from oracle.diffusion_ref import remove_mean as rm_ref
    g = torch.Generator().manual_seed(31)
    sizes = [5, 1, 9, 300]
    n, Hh, A = sum(sizes), 36, 2
    h_out, x_out, x_in = torch.randn(n, Hh, generator=g), torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)
    bidx = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    ptr = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int32, device=DEV)
    hd, xd, xi = h_out.to(DEV), x_out.to(DEV), x_in.to(DEV)
    for per_graph in (True, False):
        ex, eh = torch.empty(n, 3, device=DEV), torch.empty(n, A, device=DEV)
        _lib.check(_lib.lib().egnn_eps(_lib.stream_ptr(), n, Hh, A, _lib.ptr(ptr) if per_graph else None, len(sizes),
                                       _lib.ptr(hd), _lib.ptr(xd), _lib.ptr(xi), _lib.ptr(ex), _lib.ptr(eh)))
        want = rm_ref((x_out - x_in).clone(), bidx) if per_graph else rm_ref((x_out - x_in).clone())
        assert max_rel(ex.cpu(), want) <= 1e-5
        assert torch.equal(eh.cpu(), h_out[:, :A])


def test_remove_mean_matches_reference_golden():
    v = torch.from_numpy(G_DIFF["rm.in"]).to(DEV)
    bi = torch.from_numpy(G_DIFF["rm.batch"]).to(DEV)
    assert max_rel(dma.remove_mean(v.clone()).cpu(), torch.from_numpy(G_DIFF["rm.global"])) <= 1e-6
    w = v.clone()
    out = dma.remove_mean(w, bi)
    assert out is w                                              # in place, like the reference
    assert max_rel(w.cpu(), torch.from_numpy(G_DIFF["rm.per_graph"])) <= 1e-6


def _noise_bank(T, n, A, seed):
    g = torch.Generator().manual_seed(seed)
    bank = {"init_pos": torch.randn(n, 3, generator=g), "init_h": torch.randn(n, A, generator=g)}
    bank["pos"] = torch.randn(T + 1, n, 3, generator=g)
    bank["h"] = torch.randn(T + 1, n, A, generator=g)
    return bank


@pytest.mark.parametrize("use_cond", [False, True])
def test_sampler_loop_matches_oracle_with_explicit_noise(use_cond):
    """generate()'s reverse loop + final decode for T=12 with the SAME noise fed to the oracle loop and
    to the device sampler (two graphs in one device batch == two oracle runs)."""
    # s = 0.2 keeps the 12-step chain numerically tame with untrained weights (alpha_T ~ 0.2); the
    # reference's s = 1e-5 at T = 12 overflows in the oracle too -- see test_sampler_nan_flag below
    T, n, A, S = 12, 6, 2, 0.2
    H = 36 if use_cond else 3
    d = dims_for(H, 128, 256, 256, 256)
    torch.manual_seed(77)
    net = dma.EquivariantGNN(2, **d).to(DEV).eval()
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    proc = dma.E3DiffusionProcess(S, 2.0, T)
    ref = DiffusionRef(S, 2.0, T)
    banks = [_noise_bank(T, n, A, 10), _noise_bank(T, n, A, 11)]
    g = torch.Generator().manual_seed(5)
    conds = [torch.randn(n, H - A - 1, generator=g) if use_cond else None for _ in range(2)]
    outs = []
    for bank, cond in zip(banks, conds):
        fn = lambda tag, step, shape, bank=bank: (bank[tag].clone() if tag.startswith("init") else bank[tag][step].clone())
        outs.append(sample_one_graph(sd, ref, n, cond, fn, atom_type_size=A))
    cond = torch.cat(conds) if use_cond else None
    smp = dma.DeviceSampler(net, proc, [n, n], cond, atom_type_size=A, norm_scope="graph", precision="fp32")
    smp.init(pos_init=torch.cat([b["init_pos"] for b in banks]), x_init=torch.cat([b["init_h"] for b in banks]))
    # step-major noise, first entry = t = T
    npos = torch.stack([torch.cat([b["pos"][t] for b in banks]) for t in range(T, 0, -1)])
    nh = torch.stack([torch.cat([b["h"][t] for b in banks]) for t in range(T, 0, -1)])
    smp.run(noise_pos=npos, noise_h=nh)
    assert smp.t == 0
    pos, hc, onehot, bad = smp.final(noise_pos=torch.cat([b["pos"][0] for b in banks]),
                                     noise_h=torch.cat([b["h"][0] for b in banks]))
    assert int(bad.sum()) == 0
    for gi, (p_ref, hc_ref, oh_ref, ok) in enumerate(outs):
        assert ok
        sl = slice(gi * n, (gi + 1) * n)
        # 13 chained EGNN evaluations: 1e-3 relative
        assert rel_err(pos[sl].cpu(), p_ref) <= 1e-3
        assert rel_err(hc[sl].cpu(), hc_ref) <= 1e-3
        assert torch.equal(onehot[sl].cpu(), oh_ref)


def test_sampler_first_steps_of_T1000_and_nan_flag():
    """(a) the reference schedule (T=1000, s=1e-5): first 6 reverse steps from t=T against the oracle;
    (b) failure detection: a schedule that overflows in the oracle (T=12, s=1e-5, untrained weights)
    raises the device's sticky per-graph non-finite flag (train_per_iretation.py:376-389)."""
    n, A, H = 8, 2, 36
    d = dims_for(H, 128, 256, 256, 256)
    torch.manual_seed(78)
    net = dma.EquivariantGNN(2, **d).to(DEV).eval()
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    cond = torch.randn(n, H - A - 1, generator=torch.Generator().manual_seed(2))
    T, K = 1000, 6
    bank = _noise_bank(T, n, A, 20)
    fn = lambda tag, step, shape: (bank[tag].clone() if tag.startswith("init") else bank[tag][step].clone())
    p_ref, x_ref, _, ok = sample_one_graph(sd, DiffusionRef(1e-5, 2.0, T), n, cond, fn, atom_type_size=A, n_steps=K)
    assert ok
    smp = dma.DeviceSampler(net, dma.E3DiffusionProcess(1e-5, 2.0, T), [n], cond, atom_type_size=A, precision="fp32")
    smp.init(pos_init=bank["init_pos"], x_init=bank["init_h"])
    smp.run(nsteps=K, noise_pos=torch.stack([bank["pos"][t] for t in range(T, T - K, -1)]),
            noise_h=torch.stack([bank["h"][t] for t in range(T, T - K, -1)]))
    assert smp.t == T - K
    pos, xt, bad = smp.state()
    assert int(bad.sum()) == 0
    assert rel_err(pos.cpu(), p_ref) <= 1e-3 and rel_err(xt.cpu(), x_ref) <= 1e-3
    # (b)
    T2 = 12
    bank = _noise_bank(T2, n, A, 21)
    out = sample_one_graph(sd, DiffusionRef(1e-5, 2.0, T2), n, cond, fn, atom_type_size=A)
    assert out[3] is False
    smp = dma.DeviceSampler(net, dma.E3DiffusionProcess(1e-5, 2.0, T2), [n], cond, atom_type_size=A, precision="fp32")
    smp.init(pos_init=bank["init_pos"], x_init=bank["init_h"])
    smp.run(noise_pos=torch.stack([bank["pos"][t] for t in range(T2, 0, -1)]),
            noise_h=torch.stack([bank["h"][t] for t in range(T2, 0, -1)]))
    assert int(smp.state()[2][0]) == 1


def _tame(net, f=1e-2):
    """untrained weights make the reverse chain explode; shrink the coordinate head"""
    with torch.no_grad():
        for layer in net.egcl_list:
            layer.mlp_x[4].weight.mul_(f)
            layer.mlp_x[4].bias.mul_(f)
    return net


def test_sampler_graph_replay_equals_eager_and_is_seed_deterministic():
    T, n, A, H = 20, 16, 2, 36
    d = dims_for(H, 128, 256, 256, 256)
    torch.manual_seed(3)
    net = _tame(dma.EquivariantGNN(2, **d)).to(DEV).eval()
    net.precision = "bf16"
    proc = dma.E3DiffusionProcess(0.2, 2.0, T)
    cond = torch.randn(3 * n, H - A - 1, generator=torch.Generator().manual_seed(1))
    res = []
    for use_graph in (True, False, True):
        smp = dma.DeviceSampler(net, proc, [n] * 3, cond, atom_type_size=A, seed=1234)
        res.append(smp.sample(use_graph=use_graph))
    pos = res[0][0]
    assert torch.isfinite(pos).all() and int(res[0][3].sum()) == 0
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    for a, b in zip(res[0], res[2]):
        assert torch.equal(a, b)
    # positions stay mean-free per graph (noise and eps_x are mean-removed, x_T is mean-free)
    assert pos.view(3, n, 3).mean(1).abs().max() < 1e-3
    smp2 = dma.DeviceSampler(net, proc, [n] * 3, cond, atom_type_size=A, seed=999)
    assert not torch.equal(smp2.sample()[0], pos)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "f16c8", "bf16", "fp16"])
def test_no_scratch_read_before_write(precision, monkeypatch):
    """The library's own device buffers (context scratch, weight packs, sampler state) come from hipMalloc, which hands out zeros
    in a fresh process and the previous owner's bytes afterwards.  With EGNN_DEBUG_POISON=1 every such buffer starts as 0xFF
    bytes (NaN as fp32 / fp16 / bf16, -1 as an index): the forward of every precision on every graph-size regime (2-atom toys,
    20- and 64-atom single graphs on the small-graph kernels, a batch on the 128-row tiles, ragged graphs incl. a single atom)
    and a device sampler run must reproduce the unpoisoned results BITWISE -- and torch's own fill of uninitialised tensors
    (NaN in every torch.empty) covers the host side's workspaces."""
    H, A = 36, 2
    d = dims_for(H, 256, 1024, 1024, 1024)
    cases = {"toys": [2, 2, 2, 2], "one20": [20], "one64": [64], "batch": [64] * 6, "ragged": [33, 64, 1, 17, 50]}
    res = {}
    old_fill = torch.utils.deterministic.fill_uninitialized_memory
    try:
        for poison in ("0", "1"):
            monkeypatch.setenv("EGNN_DEBUG_POISON", poison)
            torch.use_deterministic_algorithms(poison == "1", warn_only=True)
            torch.utils.deterministic.fill_uninitialized_memory = poison == "1"
            for name, sizes in cases.items():
                n = sum(sizes)
                g = torch.Generator().manual_seed(5)
                h, x = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g) * 1.5
                torch.manual_seed(11)
                net = _tame(dma.EquivariantGNN(3, **d)).to(DEV).eval()       # (a new context, new packs per case)
                net.precision, net.norm_scope = precision, "graph"
                with torch.no_grad():
                    ho, xo = net(dma.fully_connected_plan(sizes, torch.device(DEV)), h.to(DEV), x.to(DEV))
                    ho2, xo2 = net(dma.fully_connected_edge_index(sizes, device=DEV), h.to(DEV), x.to(DEV),
                                   batch=torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV))
                assert torch.equal(ho, ho2) and torch.equal(xo, xo2)
                res[(poison, name)] = (ho.cpu(), xo.cpu())
            T, na = 12, 16
            torch.manual_seed(3)
            snet = _tame(dma.EquivariantGNN(2, **dims_for(H, 128, 256, 256, 256))).to(DEV).eval()
            snet.precision = precision
            cond = torch.randn(3 * na, H - A - 1, generator=torch.Generator().manual_seed(1))
            smp = dma.DeviceSampler(snet, dma.E3DiffusionProcess(0.2, 2.0, T), [na] * 3, cond, atom_type_size=A, seed=77)
            res[(poison, "sampler")] = tuple(t.cpu() for t in smp.sample(use_graph=True))
    finally:
        torch.use_deterministic_algorithms(False)
        torch.utils.deterministic.fill_uninitialized_memory = old_fill
    for name in list(cases) + ["sampler"]:
        for a, b in zip(res[("0", name)], res[("1", name)]):
            assert torch.isfinite(b.float()).all(), (precision, name)
            assert torch.equal(a, b), (precision, name)


def test_device_noise_statistics():
    """Philox / Box-Muller draws used by the sampler: mean 0, variance 1, no cross-step correlation."""
    T, n, A, H = 4, 4096, 2, 3
    d = dims_for(H, 128, 256, 256, 256)
    net = dma.EquivariantGNN(1, **d).to(DEV).eval()
    proc = dma.E3DiffusionProcess(1e-5, 2.0, T)
    ei = torch.zeros(2, 0, dtype=torch.long, device=DEV)               # no edges: state init only
    smp = dma.DeviceSampler(net, proc, [n], None, atom_type_size=A, seed=7, edge_index=ei)
    smp.init()
    pos, xt, _ = smp.state()
    for v in (pos, xt):
        assert abs(float(v.mean())) < 0.05 and abs(float(v.var()) - 1.0) < 0.05
    assert pos.mean(0).abs().max() < 1e-5
    k = float(((pos - pos.mean()) ** 4).mean() / pos.var() ** 2)
    assert abs(k - 3.0) < 0.25


def test_generate_interface():
    from types import SimpleNamespace
    params = dict(num_diffusion_timestep=8, conditional=True, atom_type_size=2, spectrum_size=200,
                  onehot_scaling_factor=1.0, to_compress_spectrum=True, give_exO=True, noise_schedule="predefined",
                  seed=2024)
    H = 2 + 32 + 1 + 1
    d = dims_for(H, 128, 256, 256, 256)
    torch.manual_seed(0)
    nn_dict = {"egnn": _tame(dma.EquivariantGNN(2, **d)), "spectrum_compressor": dma.SpectrumCompressor(200, [150, 100, 50], 32)}
    proc = dma.E3DiffusionProcess(0.2, 2.0, 8)
    data = []
    for n in (5, 9):
        spec = torch.zeros(n, 200)
        spec[0] = torch.rand(200)
        exo = torch.zeros(n, 1)
        exo[0] = 1
        data.append(SimpleNamespace(x=torch.zeros(n, 2), pos=torch.zeros(n, 3), spectrum=spec, exO=exo))
    orig, gen = dma.generate(nn_dict, data, params, proc, gen_num_per_spectrum=3)
    assert len(orig) == len(gen) == 6
    for o, gl in zip(orig, gen):
        g = gl[-1]
        n = o.x.shape[0]
        assert g.pos.shape == (n, 3) and g.x.shape == (n, 2)
        assert torch.isfinite(g.pos).all() and bool((g.x.sum(1) == 1).all())


def test_generate_batches_across_data():
    """generate() draws the samples of several conditioning data (different atom counts) as one device batch; the lists
    come back datum by datum as in the reference whatever the batch size, and with one datum per batch the result is the
    per-datum loop of the reference (same seeds -> same samples as a call on that datum alone)."""
    from types import SimpleNamespace
    params = dict(num_diffusion_timestep=8, conditional=True, atom_type_size=2, spectrum_size=200,
                  onehot_scaling_factor=1.0, to_compress_spectrum=True, give_exO=True, noise_schedule="predefined",
                  seed=7)
    d = dims_for(36, 128, 256, 256, 256)
    torch.manual_seed(0)
    nn_dict = {"egnn": _tame(dma.EquivariantGNN(2, **d)), "spectrum_compressor": dma.SpectrumCompressor(200, [150, 100, 50], 32)}
    proc = dma.E3DiffusionProcess(0.2, 2.0, 8)
    data = []
    for n in (5, 9, 4, 7):
        spec = torch.zeros(n, 200)
        spec[0] = torch.rand(200)
        exo = torch.zeros(n, 1)
        exo[0] = 1
        data.append(SimpleNamespace(x=torch.zeros(n, 2), pos=torch.zeros(n, 3), spectrum=spec, exO=exo))
    for gpb in (256, 4, 1):
        orig, gen = dma.generate(nn_dict, data, params, proc, gen_num_per_spectrum=2, graphs_per_batch=gpb)
        assert [o.x.shape[0] for o in orig] == [5, 5, 9, 9, 4, 4, 7, 7]
        for o, gl in zip(orig, gen):
            g = gl[-1]
            assert g.pos.shape == (o.x.shape[0], 3) and torch.isfinite(g.pos).all() and bool((g.x.sum(1) == 1).all())
            assert g.spectrum is o.spectrum
    # one datum per batch == that datum generated alone (the batch seed is keyed by the first datum of the batch)
    _, gen_all = dma.generate(nn_dict, data, params, proc, gen_num_per_spectrum=2, graphs_per_batch=2)
    _, gen_one = dma.generate(nn_dict, data[:1], params, proc, gen_num_per_spectrum=2, graphs_per_batch=2)
    assert torch.equal(gen_all[0][-1].pos, gen_one[0][-1].pos) and torch.equal(gen_all[1][-1].pos, gen_one[1][-1].pos)


# every bf16 edge-kernel variant: v3 <2,false> (x_hidden >= 512), v3 <1,false> (x_hidden = 256), v3 <1,true>,
# and the generic fallbacks taken when the widths do not fit the v3 tiling (m_size != 256, odd widths)
@pytest.mark.parametrize("H,m_size,wm,wx,wh", [
    (36, 256, 1024, 1024, 256),   # reference widths: v3 X (two column blocks) + M
    (36, 256, 128, 256, 64),      # v3 X with one column block, narrow message MLP
    (3, 256, 64, 512, 128),       # unconditional variant (H = 3) on the v3 path
    (36, 250, 192, 512, 96),      # m_size padded to 256, message width 192 padded to 256 (f16c8: the 32x32-tile kernels)
    (36, 256, 256, 512, 128),     # f16c8 on 32x32 tiles with ONE 512-column share (4 chunks in the K-split message kernel)
    (36, 64, 128, 128, 64),       # m_size 64: fallback kernels
    (5, 10, 30, 22, 18),          # nothing aligned
])
def test_width_sweep_all_edge_kernel_variants(H, m_size, wm, wx, wh):
    d = dims_for(H, m_size, wm, wx, wh)
    sd = egnn_ref.init_state_dict(2, **d, seed=123)
    sizes = [33, 5, 70, 1, 12]   # ragged batch, a single-atom graph (no edges), segments across tile borders
    n = sum(sizes)
    g = torch.Generator().manual_seed(9)
    h, x = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g)
    ei_cpu = egnn_ref.fully_connected_edge_index(sizes)
    ptr = torch.tensor([0] + list(np.cumsum(sizes)))
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
    for scope in ("call", "graph"):
        h_ref, x_ref = egnn_ref.egnn_forward(sd, ei_cpu, h, x, norm_scope=scope, graph_ptr=ptr)
        # fp16 / f16c8: the reference widths run their own kernels, every other shape the exact fp32 kernels (include/egnn_amd.h)
        for precision, tol in (("fp32", 1e-4), ("bf16x3", 1e-4), ("f16c8", 1e-4), ("bf16", 1e-2), ("fp16", 2.5e-3)):
            net = build_net(sd, d, 2, precision=precision, norm_scope=scope)
            with torch.no_grad():
                h_o, x_o = net(ei_cpu.to(DEV), h.to(DEV), x.to(DEV), batch=batch)
            eh, ex = rel_err(h_o.cpu(), h_ref), rel_err(x_o.cpu() - x, x_ref - x)
            print(f"width sweep {(H, m_size, wm, wx, wh)} {scope} {precision}: h {eh:.2e} eps_x {ex:.2e}")
            assert eh <= tol, (scope, precision, "h")
            assert ex <= tol, (scope, precision, "eps_x")


# (the fully connected cases keep the ids they had before the graph parameter was added)
@pytest.mark.parametrize("wx,precision,graph", [(wx, p, g) for g in ("fully_connected", "irregular") for p in ("bf16", "fp16") for wx in (1024, 512)],
                         ids=[f"{wx}-{p}" + ("" if g == "fully_connected" else "-" + g) for g in ("fully_connected", "irregular")
                              for p in ("bf16", "fp16") for wx in (1024, 512)])
def test_persistent_coordinate_kernel_is_bitwise_the_per_tile_kernel(precision, wx, graph, monkeypatch):
    """csrc/edge_x_m16.hip, PERSIST form (one workgroup per CU walking over its units with the next unit's prologue requested under
    the current epilogue; chosen when there are more than two units per CU) against the one-workgroup-per-unit form (EGNN_X_PERSIST=0,
    read per launch): the same arithmetic in the same order, so every output bit must agree -- on a ragged batch whose tile count is
    no multiple of anything (a last tile of a few rows, graphs that straddle tiles, a single-atom graph), one layer and two.
    graph "irregular": the 128-edge-tile irregular batch of the forward stage tests (tests/_fwd_ref.py: nodes whose edges span three
    tiles, fill exactly one / two, tiles of 1 ... 25 segments, isolated nodes, graphs without edges, duplicates, self loops), repeated
    until the persistent form is chosen."""
    props = torch.cuda.get_device_properties(0)
    if graph == "irregular":
        from tests import _fwd_ref
        b = _fwd_ref.irregular_batch(128)
        _fwd_ref.assert_features(b, 128)
        reps = 2 * props.multi_processor_count * 128 // (b.E * (wx // 512)) + 2
        sizes, E = b.sizes * reps, b.E * reps
        ei_irregular = torch.cat([torch.stack((b.dst, b.src)) + r * b.N for r in range(reps)], 1)
    else:
        sizes = [61, 64, 1, 57, 64, 33, 64, 64, 50, 64, 64, 63, 64, 17, 64, 64, 64, 59, 64, 64, 64, 64, 2, 64, 64, 64, 64, 64, 64, 64] * (1 if wx == 1024 else 2)
        E = sum(n * (n - 1) for n in sizes)
    assert (E + 127) // 128 * (wx // 512) > 2 * props.multi_processor_count, "the batch must be large enough for the persistent form"
    H = 36
    d = dims_for(H, 256, wx, wx, 128)
    sd = egnn_ref.init_state_dict(2, **d, seed=5)
    n = sum(sizes)
    g = torch.Generator().manual_seed(4)
    h, x = torch.randn(n, H, generator=g).to(DEV), torch.randn(n, 3, generator=g).to(DEV)
    ei = ei_irregular.to(DEV) if graph == "irregular" else dma.fully_connected_edge_index(sizes, device=DEV)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
    net = build_net(sd, d, 2, precision=precision, norm_scope="graph")
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("EGNN_X_PERSIST", flag)
        with torch.no_grad():
            h1, x1 = net.egcl_list[0](ei, h, x, batch=batch)
            h2, x2 = net(ei, h, x, batch=batch)
        torch.cuda.synchronize()
        out[flag] = [t.cpu() for t in (h1, x1, h2, x2)]
    for a, b, name in zip(out["1"], out["0"], ("h layer 1", "x layer 1", "h", "x")):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), f"{name}: persistent and per-tile coordinate kernels differ (max {float((a - b).abs().max()):.3e})"


_FALLBACK_SNIPPET = r"""
import sys, torch, numpy as np
sys.path.insert(0, {root!r})
import diffusion_model_amd as dma
from oracle import egnn_ref
from tests._util import dims_for, rel_err
H = 36
d = dims_for(H, 256, 1024, 1024, 256)
sd = egnn_ref.init_state_dict(1, **d, seed=7)
sizes = [40, 9, 70]
n = sum(sizes)
g = torch.Generator().manual_seed(1)
h, x = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g)
ei = egnn_ref.fully_connected_edge_index(sizes)
h_ref, x_ref = egnn_ref.egnn_forward(sd, ei, h, x)
net = dma.EquivariantGNN(1, d["m_input"], d["m_hidden"], d["m_output"], d["x_input"], d["x_hidden"], d["x_output"],
                         d["h_input"], d["h_hidden"], d["h_output"])
net.load_state_dict(sd); net.to("cuda").eval(); net.precision = "bf16"
with torch.no_grad():
    h_o, x_o = net(ei.cuda(), h.cuda(), x.cuda())
eh, ex = rel_err(h_o.cpu(), h_ref), rel_err(x_o.cpu(), x_ref)
print("ERR", eh, ex)
assert eh <= 1e-2 and ex <= 1e-2
"""


@pytest.mark.parametrize("edge", ["1"])
def test_non_default_bf16_edge_kernels(edge):
    """EGNN_EDGE=1 runs the reference widths on the generic 64-edge-tile bf16 kernel that shapes outside the 128-edge tiling
    fall back to; the switch is read once per process, hence the child process."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EGNN_EDGE=edge)
    out = subprocess.run([sys.executable, "-c", _FALLBACK_SNIPPET.format(root=root)], env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]

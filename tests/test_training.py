"""Training path: gradients of the HIP-forward / library-GEMM-backward EGNN against the oracle's
autograd (GPU), and the data-parallel gradient exchange with gloo on CPU (world_size 2)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import diffusion_model_amd as dma
from oracle.diffusion_ref import DiffusionRef
from oracle.egnn_ref import fully_connected_edge_index
from oracle.sampler_ref import training_loss as oracle_training_loss
from tests._util import dims_for, rel_err


def _problem(seed=0, sizes=(6, 4, 7), H=36, A=2):
    g = torch.Generator().manual_seed(seed)
    n = sum(sizes)
    pos0 = torch.randn(n, 3, generator=g)
    x0 = torch.nn.functional.one_hot(torch.randint(0, A, (n,), generator=g), A).float()
    cond = torch.randn(n, H - A - 1, generator=g)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    ei = fully_connected_edge_index(list(sizes))
    noise_pos, noise_h = torch.randn(n, 3, generator=g), torch.randn(n, A, generator=g)
    times = [17, 3, 40, 9, 28, 33, 1, 22][: len(sizes)]
    return pos0, x0, cond, batch, ei, noise_pos, noise_h, times


@pytest.mark.gpu
def test_read_aggregates_matches_oracle():
    """egcl_read_aggregates: the segment sums the forward kernels produced, against the oracle's (fp32 1e-4, bf16 3e-2)"""
    from diffusion_model_amd import _lib
    from diffusion_model_amd.egnn import _context, _plan_for
    from oracle.egnn_ref import egcl_forward as oracle_layer
    H = 36
    d = dims_for(H, 64, 128, 128, 64)
    torch.manual_seed(11)
    net = dma.EquivariantGNN(1, **d)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    sizes = (40, 3, 70)   # 70 * 69 edges per node span several edge tiles
    n = sum(sizes)
    g = torch.Generator().manual_seed(3)
    h, x = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g)
    ei = fully_connected_edge_index(list(sizes))
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    ptr = torch.tensor([0, 40, 43, 113])
    dev = "cuda"
    net.to(dev)
    layers = list(net.egcl_list)
    L = _lib.lib()
    for scope in ("call", "graph"):
        _, _, (sm_ref, sx_ref, sq_ref) = oracle_layer(sd, 0, ei, h, x, scope, ptr, return_aggregates=True)
        for prec, tol in (("fp32", 1e-4), ("bf16", 3e-2)):
            net.precision, net.norm_scope = prec, scope
            plan = _plan_for(net, ei.to(dev), n, batch.to(dev))
            c = _context(net, layers, torch.device(dev))
            c.set_graph(plan)
            c.pack(layers)
            hd, xd = h.to(dev), x.to(dev)
            ho, xo = torch.empty_like(hd), torch.empty_like(xd)
            sc = _lib.NORM_SCOPES[scope]
            _lib.check(L.egcl_forward(c.handle, _lib.stream_ptr(), 0, _lib.PRECISIONS[prec], sc, _lib.ptr(hd), _lib.ptr(xd),
                                      _lib.ptr(ho), _lib.ptr(xo)))
            sm, sx = torch.empty(n, 64, device=dev), torch.empty(n, 3, device=dev)
            sq = torch.empty(sq_ref.numel(), device=dev)
            _lib.check(L.egcl_read_aggregates(c.handle, _lib.stream_ptr(), sc, _lib.ptr(sm), _lib.ptr(sx), _lib.ptr(sq)))
            assert rel_err(sm.cpu(), sm_ref) <= tol, (scope, prec)
            assert rel_err(sx.cpu(), sx_ref) <= tol, (scope, prec)
            assert rel_err(sq.cpu(), sq_ref) <= 1e-5, (scope, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("widths", [(128, 256, 256, 256), (10, 30, 22, 18)], ids=["vec4", "odd"])
@pytest.mark.parametrize("norm_scope", ["graph", "call"])
def test_gradients_match_oracle_autograd(norm_scope, widths, monkeypatch):
    # "odd": widths that are not multiples of 4 take the scalar-access variants of the backward stage kernels
    # 100-edge chunks: several backward chunks per layer, alternating between the two side streams
    from diffusion_model_amd import autograd as _ag
    monkeypatch.setattr(_ag, "EDGE_CHUNK", 100)
    H, A, T = 36, 2, 50
    d = dims_for(H, *widths)
    torch.manual_seed(5)
    net = dma.EquivariantGNN(2, **d)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    pos0, x0, cond, batch, ei, npos, nh, times = _problem()
    ref = DiffusionRef(1e-5, 2.0, T)
    ptr = torch.tensor([0, 6, 10, 17])
    loss_ref, ex_ref, eh_ref, _, _ = oracle_training_loss(sd, ref, pos0, x0, cond, ei, batch, times, npos.clone(), nh.clone(),
                                                         atom_type_size=A, norm_scope=norm_scope, graph_ptr=ptr)
    loss_ref.backward()
    dev = "cuda"
    net.to(dev).train()
    net.precision, net.norm_scope = "fp32", norm_scope
    proc = dma.E3DiffusionProcess(1e-5, 2.0, T)
    noised = dma.diffuse_as_batch(pos0.to(dev), x0.to(dev), batch.to(dev), proc, times=times,
                                  noise_pos=npos.to(dev), noise_h=nh.to(dev))
    loss, ex, eh = dma.training_loss(net, ei.to(dev), batch.to(dev), noised, cond.to(dev), A)
    loss.backward()
    assert abs(float(loss.detach()) - float(loss_ref.detach())) <= 1e-4 * abs(float(loss_ref.detach()))
    assert rel_err(ex.detach().cpu(), ex_ref.detach()) <= 1e-4 and rel_err(eh.detach().cpu(), eh_ref.detach()) <= 1e-4
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        assert rel_err(p.grad.cpu(), sd[k].grad) <= 2e-3, k


@pytest.mark.gpu
@pytest.mark.parametrize("first_layer,sizes", [("chain", (64, 64, 64)), ("factorised", (64, 64, 64)), ("graph", (64, 64, 64)),
                                               ("graph", (40, 64, 7, 1, 25))], ids=["chain", "factorised", "graph", "graph-ragged"])
def test_gradients_full_width_64_atom_graphs(first_layer, sizes, monkeypatch):
    """BASELINE configs[3] shape per graph: 64-atom fully connected graphs at the reference widths (W = 1024, m = 256,
    H = 36), three graphs = 12,096 edges in backward chunks of 5,000 (so a layer spans several chunks).  EVERY precision
    against the ORACLE's autograd (no self-comparison): fp32 and bf16x3 (whose backward is the fp32 chain) at 2e-3; bf16
    (bf16 MFMA forward, saved bf16 activations / bf16 dgrad + wgrad operands) and fp16 (fp16 forward, bf16 backward kernels)
    at the tolerance below, set from the printed measurement (profiles/r04d_gpu_tests.log)."""
    from diffusion_model_amd import autograd as _ag
    # "factorised": the opt-in one-pass first-layer backward (csrc/edge_bwd_first.hip: per-node receive / send sums of dL/da1,
    # node-level products); the 5,000-edge chunks cut through the graphs, so its accumulation across chunks is exercised too
    # "graph" (the default form): the same sums inside the dgrad kernel (csrc/edge_bwd_dgrad_graph.hip, no dL/da1 in memory); its
    # chunks are cut at graph boundaries (one 4,032-edge graph per chunk here; ragged: graphs of 40 / 64 / 7 / 1 / 25 atoms, the
    # single atom has no edges at all)
    monkeypatch.setenv("EGNN_BWD_FIRST", "1" if first_layer == "factorised" else "0")
    monkeypatch.setenv("EGNN_BWD_GRAPH", "1" if first_layer == "graph" else "0")
    H, A, T = 36, 2, 50
    d = dims_for(H, 256, 1024, 1024, 1024)
    torch.manual_seed(6)
    net = dma.EquivariantGNN(2, **d)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    pos0, x0, cond, batch, ei, npos, nh, times = _problem(seed=2, sizes=sizes)
    pos0 = pos0 * 2.0
    ref = DiffusionRef(1e-5, 2.0, T)
    ptr = torch.tensor([0] + torch.cumsum(torch.tensor(sizes), 0).tolist())
    loss_ref, ex_ref, eh_ref, _, _ = oracle_training_loss(sd, ref, pos0, x0, cond, ei, batch, times, npos.clone(), nh.clone(),
                                                         atom_type_size=A, norm_scope="graph", graph_ptr=ptr)
    loss_ref.backward()
    dev = "cuda"
    proc = dma.E3DiffusionProcess(1e-5, 2.0, T)
    grads = {}
    old_chunk = _ag.EDGE_CHUNK
    _ag.EDGE_CHUNK = 5000
    try:
        for prec in ("fp32", "bf16x3", "f16c8", "bf16", "fp16"):
            m = dma.EquivariantGNN(2, **d)
            m.load_state_dict({k: v.detach() for k, v in sd.items()})
            m.to(dev).train()
            m.precision, m.norm_scope = prec, "graph"
            noised = dma.diffuse_as_batch(pos0.to(dev), x0.to(dev), batch.to(dev), proc, times=times,
                                          noise_pos=npos.to(dev), noise_h=nh.to(dev), num_graphs=len(sizes))
            loss, ex, eh = dma.training_loss(m, ei.to(dev), batch.to(dev), noised, cond.to(dev), A, num_graphs=len(sizes))
            loss.backward()
            grads[prec] = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
            if prec in ("bf16", "fp16"):   # the form under test is the one that ran
                assert _ag.LAST_FIRST_LAYER_FORM == {"chain": None, "factorised": "reduce", "graph": "graph"}[first_layer]
                bp = _ag.LAST_PLAN
                assert (bp.first, bp.fused, bp.hip_gemms, bp.node, bp.kept) == (_ag.LAST_FIRST_LAYER_FORM, True, True, "hip", prec == "bf16")
            if prec in ("fp32", "bf16x3", "f16c8"):
                assert abs(float(loss.detach()) - float(loss_ref.detach())) <= 1e-4 * abs(float(loss_ref.detach()))
                assert rel_err(ex.detach().cpu(), ex_ref.detach()) <= 1e-4 and rel_err(eh.detach().cpu(), eh_ref.detach()) <= 1e-4
    finally:
        _ag.EDGE_CHUNK = old_chunk
    # measured (profiles/r05r_gpu_tests.log, worst parameter tensor over the four forms): fp32 6.2e-6, bf16x3 2.4e-5, f16c8 as
    # bf16x3 (same backward), bf16 6.8e-3, fp16 4.4e-3.  Bars: north_star's 1e-4 for the fp32-grade precisions, 1.5 x the
    # measurement for the half-precision ones (they were 3-5 x, wide enough to hide a dropped term)
    GRAD_TOL = {"fp32": 1e-4, "bf16x3": 1e-4, "f16c8": 1e-4, "bf16": 1.0e-2, "fp16": 6.5e-3}
    for prec, gr in grads.items():
        errs = {k: rel_err(gr[k], sd[k].grad) for k in gr}
        worst = max(errs, key=errs.get)
        print(f"gradients vs oracle autograd, W = 1024, {prec}: worst {errs[worst]:.2e} ({worst}), median {sorted(errs.values())[len(errs) // 2]:.2e}")
        for k, e in errs.items():
            assert e <= GRAD_TOL[prec], (prec, k, e)


@pytest.mark.gpu
def test_train_step_reduces_loss():
    from types import SimpleNamespace
    H, A, T = 36, 2, 50
    params = dict(conditional=True, to_compress_spectrum=True, give_exO=True, atom_type_size=A)
    d = dims_for(H, 128, 256, 256, 256)
    torch.manual_seed(1)
    dev = "cuda"
    nn_dict = {"egnn": dma.EquivariantGNN(2, **d).to(dev), "spectrum_compressor": dma.SpectrumCompressor(200, [150, 100, 50], 32).to(dev)}
    nn_dict["egnn"].norm_scope = "graph"
    pos0, x0, _, batch, ei, *_ = _problem()
    spec = torch.zeros(pos0.shape[0], 200)
    spec[[0, 6, 10]] = torch.rand(3, 200)
    exo = torch.zeros(pos0.shape[0], 1)
    exo[[0, 6, 10]] = 1
    data = SimpleNamespace(pos=pos0.to(dev), x=x0.to(dev), batch=batch.to(dev), edge_index=ei.to(dev),
                           spectrum=spec.to(dev), exO=exo.to(dev))
    proc = dma.E3DiffusionProcess(1e-5, 2.0, T)
    opt = torch.optim.Adam(list(nn_dict["egnn"].parameters()) + list(nn_dict["spectrum_compressor"].parameters()), lr=1e-4)
    losses = [float(dma.train_step(nn_dict, data, params, proc, opt, times=[20, 20, 20])) for _ in range(12)]
    assert all(l == l for l in losses)
    assert min(losses[-3:]) < losses[0]
    assert all(p.grad is not None for p in nn_dict["spectrum_compressor"].parameters())


@pytest.mark.gpu
def test_learned_schedule_receives_gradient():
    """noise_schedule='learned': alpha(t) / sigma(t) are differentiable in the reference (diffusion_x_h.py:36-46) and
    the loss reaches gamma_0 / gamma_1 through pos_at_t / h_at_t (train_per_iretation.py:130-150; SURVEY Q7: only
    these two ever train).  One train_step must leave a non-zero gradient on them and move them."""
    from types import SimpleNamespace
    H, A, T = 3, 2, 50
    params = dict(conditional=False, to_compress_spectrum=False, give_exO=False, atom_type_size=A)
    d = dims_for(H, 32, 64, 64, 64)
    torch.manual_seed(1)
    dev = "cuda"
    nn_dict = {"egnn": dma.EquivariantGNN(2, **d).to(dev)}
    nn_dict["egnn"].norm_scope = "graph"
    pos0, x0, _, batch, ei, *_ = _problem(H=H)
    data = SimpleNamespace(pos=pos0.to(dev), x=x0.to(dev), batch=batch.to(dev), edge_index=ei.to(dev))
    proc = dma.E3DiffusionProcess(1e-5, 2.0, T, noise_schedule="learned").to(dev)
    opt = torch.optim.SGD(list(nn_dict["egnn"].parameters()) + list(proc.parameters()), lr=1e-3)
    g0, g1 = float(proc.gamma.gamma_0), float(proc.gamma.gamma_1)
    a_before = float(proc.alpha(20))
    loss = dma.train_step(nn_dict, data, params, proc, opt, times=[20, 5, 45], num_graphs=3, num_graphs_global=3)
    assert torch.isfinite(loss)
    assert proc.gamma.gamma_0.grad is not None and float(proc.gamma.gamma_0.grad.abs()) > 0
    assert proc.gamma.gamma_1.grad is not None and float(proc.gamma.gamma_1.grad.abs()) > 0
    assert (float(proc.gamma.gamma_0), float(proc.gamma.gamma_1)) != (g0, g1)
    assert float(proc.alpha(20)) != a_before      # the tabulated schedule follows the updated parameters


# ---------------- data-parallel exchange, gloo on CPU ----------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_grads(params, rank):
    g = torch.Generator().manual_seed(1234 + rank)
    return [torch.randn(p.shape, generator=g) for p in params]


def _ddp_worker(rank, world, port, out):
    """GradAllReducer on the bucket structure of the real EquivariantGNN (one bucket per EGCL layer + one for the
    spectrum compressor): per-rank gradients are injected in the order the backward produces them (last layer
    first, through the overlapped layer_ready hook; the compressor through .grad), and every bucket must come back
    as the sum over ranks."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    d = dims_for(36, 16, 32, 32, 24)
    net = dma.EquivariantGNN(3, **d)
    comp = dma.SpectrumCompressor(200, [150, 100, 50], 32)
    red = dma.GradAllReducer(list(net.egcl_list) + [comp])
    assert len(red.buckets) == 4 and [len(b) for b in red.buckets[:3]] == [16, 16, 16]
    n_global = dma.training.global_graph_count(3 if rank == 0 else 5, "cpu")      # uneven shards: 3 + 5 graphs
    errs = []
    for rep in range(2):       # two steps: buckets must not alias the previous step's gradients
        red.arm()
        got = {}
        for layer in reversed(list(net.egcl_list)):
            ps = red.buckets[red.bucket_of[id(layer)]]
            views = red.layer_ready(layer, _rank_grads(ps, rank + 10 * rep))
            for p_, v in zip(ps, views):
                got[p_] = v
        red.sync()
        for p_, v in got.items():
            p_.grad = v
        for p_, g_ in zip(comp.parameters(), _rank_grads(list(comp.parameters()), rank + 10 * rep)):
            p_.grad = g_
        red.finish()
        for m in list(net.egcl_list) + [comp]:
            ps = [q for q in m.parameters()]
            want = [a + b for a, b in zip(_rank_grads(ps, 0 + 10 * rep), _rank_grads(ps, 1 + 10 * rep))]
            errs += [float((q.grad - w).abs().max()) for q, w in zip(ps, want)]
    # the plain (un-overlapped) form on .grad
    for p_, g_ in zip(net.parameters(), _rank_grads(list(net.parameters()), rank)):
        p_.grad = g_
    dma.GradAllReducer(list(net.egcl_list)).reduce()
    ps = list(net.parameters())
    want = [a + b for a, b in zip(_rank_grads(ps, 0), _rank_grads(ps, 1))]
    errs += [float((q.grad - w).abs().max()) for q, w in zip(ps, want)]
    # ---- learned schedule under data parallelism: gamma_0 / gamma_1 train, so the process's
    # GammaNetwork must be one of the reducer's modules; a reducer that leaves optimizer parameters out is refused
    proc = dma.E3DiffusionProcess(1e-5, 2.0, 20, noise_schedule="learned")
    opt = torch.optim.SGD(list(net.parameters()) + list(proc.gamma.parameters()), lr=0.1)
    covers = True
    try:
        dma.GradAllReducer(list(net.egcl_list)).check_covers(opt)
        covers = False
    except RuntimeError:
        pass
    red2 = dma.GradAllReducer(list(net.egcl_list) + [proc.gamma])
    red2.check_covers(opt)
    gps = [q for q in proc.gamma.parameters() if q.requires_grad]
    for q, g_ in zip(gps, _rank_grads(gps, rank + 50)):
        q.grad = g_
    for p_ in net.parameters():
        p_.grad = torch.zeros_like(p_)
    red2.arm()
    red2.finish()                      # nothing came through the backward hook: every bucket is reduced from .grad
    want = [a + b for a, b in zip(_rank_grads(gps, 50), _rank_grads(gps, 51))]
    errs += [float((q.grad - w).abs().max()) for q, w in zip(gps, want)]
    # ---- an exception inside an armed step leaves no hook behind; a layer handed in twice is refused
    from diffusion_model_amd import autograd as _ag
    try:
        with red.armed():
            raise ValueError("boom")
    except ValueError:
        pass
    hook_cleared = _ag.ACTIVE_REDUCER is None
    twice = False
    with red.armed():
        layer = net.egcl_list[0]
        ps = red.buckets[red.bucket_of[id(layer)]]
        red.layer_ready(layer, _rank_grads(ps, rank))
        try:
            red.layer_ready(layer, _rank_grads(ps, rank))
        except RuntimeError:
            twice = True
        for p_ in list(net.parameters()) + list(comp.parameters()):
            p_.grad = torch.zeros_like(p_)
    if rank == 0:
        torch.save({"n_global": n_global, "errs": errs, "covers": covers, "hook_cleared": hook_cleared, "twice": twice}, out)
    dist.barrier()
    dist.destroy_process_group()


def test_gradient_allreduce_world_size_2_gloo(tmp_path):
    out = str(tmp_path / "r.pt")
    mp.spawn(_ddp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    res = torch.load(out, weights_only=True)
    assert res["n_global"] == 8
    assert max(res["errs"]) < 1e-6
    assert res["covers"] and res["hook_cleared"] and res["twice"]


def _part_worker(rank, world, port, out):
    """partitioned_forward's communication pattern with gloo on CPU: the two stage calls are replaced by an
    oracle-based stand-in (no GPU here); checks that all-reduced sums + all-gathered rows reproduce the
    unpartitioned layer stack."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import egnn_ref
    from diffusion_model_amd import partition
    torch.manual_seed(0)
    n, H = 23, 5
    d = dims_for(H, 8, 16, 16, 16)
    sd = egnn_ref.init_state_dict(2, **d, seed=3)
    g = torch.Generator().manual_seed(4)
    h, x = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g)
    ei = egnn_ref.fully_connected_edge_index(n)
    ranges = partition.node_ranges(n, world)
    lo, hi = ranges[rank]
    keep = (ei[0] >= lo) & (ei[0] < hi)
    ei_loc = ei[:, keep]
    hc, xc = h, x
    for l in range(2):
        diff = xc[ei_loc[0]] - xc[ei_loc[1]]
        S = (diff * diff).sum().reshape(1)
        S = partition._allreduce_default(S, None)
        # one layer with the GLOBAL normaliser: run the oracle on the local edges with G patched in
        ho, xo = egnn_ref.egcl_forward(sd, l, ei_loc, hc, xc)
        G_loc = torch.norm(diff)
        xo = xc + (xo - xc) * (G_loc + 1) / (torch.sqrt(S[0]) + 1)
        hc = partition._allgather_default(ho[lo:hi], ranges, None)
        xc = partition._allgather_default(xo[lo:hi], ranges, None)
    if rank == 0:
        h_ref, x_ref = egnn_ref.egnn_forward(sd, ei, h, x)
        torch.save({"eh": float((hc - h_ref).abs().max()), "ex": float((xc - x_ref).abs().max())}, out)
    dist.barrier()
    dist.destroy_process_group()


def test_partitioned_exchange_world_size_2_gloo(tmp_path):
    out = str(tmp_path / "p.pt")
    mp.spawn(_part_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    res = torch.load(out, weights_only=True)
    assert res["eh"] < 1e-4 and res["ex"] < 1e-4


@pytest.mark.gpu
def test_half_precision_training_gradients_against_oracle():
    """Width 256 (the generic backward chain of csrc/backward.hip with bf16 stage buffers around library GEMMs): bf16 and fp16
    gradients against the ORACLE's autograd, tolerance from the printed measurement."""
    H, A, T = 36, 2, 50
    d = dims_for(H, 128, 256, 256, 256)
    pos0, x0, cond, batch, ei, npos, nh, times = _problem()
    torch.manual_seed(5)
    net0 = dma.EquivariantGNN(2, **d)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in net0.state_dict().items()}
    ref = DiffusionRef(1e-5, 2.0, T)
    loss_ref, *_ = oracle_training_loss(sd, ref, pos0, x0, cond, ei, batch, times, npos.clone(), nh.clone(), atom_type_size=A,
                                        norm_scope="graph", graph_ptr=torch.tensor([0, 6, 10, 17]))
    loss_ref.backward()
    dev = "cuda"
    proc = dma.E3DiffusionProcess(1e-5, 2.0, T)
    for prec, tol in (("bf16", 2.5e-2), ("fp16", 2.5e-2)):   # measured 7.7e-3 / 4.3e-3 (profiles/r04d_gpu_tests.log)
        net = dma.EquivariantGNN(2, **d)
        net.load_state_dict({k: v.detach() for k, v in sd.items()})
        net.to(dev).train()
        net.precision, net.norm_scope = prec, "graph"
        noised = dma.diffuse_as_batch(pos0.to(dev), x0.to(dev), batch.to(dev), proc, times=times,
                                      noise_pos=npos.to(dev), noise_h=nh.to(dev))
        loss, _, _ = dma.training_loss(net, ei.to(dev), batch.to(dev), noised, cond.to(dev), A)
        loss.backward()
        errs = {k: rel_err(p.grad.detach().cpu(), sd[k].grad) for k, p in net.named_parameters()}
        worst = max(errs, key=errs.get)
        print(f"gradients vs oracle autograd, W = 256, {prec}: loss {float(loss):.6f} (oracle {float(loss_ref):.6f}), worst {errs[worst]:.2e} ({worst})")
        assert abs(float(loss.detach()) - float(loss_ref.detach())) <= 2e-2 * abs(float(loss_ref.detach()))
        for k, e in errs.items():
            assert e <= tol, (prec, k, e)


@pytest.mark.gpu
def test_saved_activation_backward_matches_recompute(monkeypatch):
    """bf16 training at the reference widths: the forward that keeps the edge activations (egcl_forward_save, default) and the
    backward that recomputes them (EGNN_BWD_SAVE=0) see the same loss bitwise and gradients that differ only by the bf16
    rounding of the kept pre-activations (3e-2); ragged sizes so that E is not a multiple of the 64-row padding and a layer
    spans several backward chunks.  A second backward through a retained graph falls back to the recompute path."""
    from diffusion_model_amd import autograd as _ag
    H, A, T = 36, 2, 50
    d = dims_for(H, 256, 1024, 1024, 1024)
    sizes = (64, 63, 62)
    pos0, x0, cond, batch, ei, npos, nh, times = _problem(seed=4, sizes=sizes)
    assert ei.shape[1] % 64 != 0
    dev = "cuda"
    proc = dma.E3DiffusionProcess(1e-5, 2.0, T)
    monkeypatch.setattr(_ag, "EDGE_CHUNK", 5000)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("EGNN_BWD_SAVE", mode)
        torch.manual_seed(8)
        m = dma.EquivariantGNN(2, **d).to(dev).train()
        m.precision, m.norm_scope = "bf16", "graph"
        noised = dma.diffuse_as_batch(pos0.to(dev) * 2.0, x0.to(dev), batch.to(dev), proc, times=times, noise_pos=npos.to(dev),
                                      noise_h=nh.to(dev), num_graphs=3)
        loss, _, _ = dma.training_loss(m, ei.to(dev), batch.to(dev), noised, cond.to(dev), A, num_graphs=3)
        loss.backward(retain_graph=(mode == "1"))
        g1 = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
        out[mode] = (float(loss.detach()), g1)
        if mode == "1":   # the kept buffers are spent: the second pass recomputes, and accumulates the same gradients again
            loss.backward()
            for k, p in m.named_parameters():
                assert rel_err((p.grad - g1[k]).cpu(), g1[k].cpu()) <= 3e-2, k
    assert out["1"][0] == out["0"][0]
    for k in out["1"][1]:
        assert torch.isfinite(out["1"][1][k]).all()
        assert rel_err(out["1"][1][k].cpu(), out["0"][1][k].cpu()) <= 3e-2, k


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["graph", "chain"])
def test_kept_buffers_are_fully_written(form, monkeypatch):
    """Every element of the kept-activation buffers (s1, t2 of both edge MLPs, the column shares of s_e) that the backward reads
    must have been written by egcl_forward_save: with the buffers filled with NaN before the forward (EGNN_DEBUG_POISON_KEPT=1)
    all gradients stay finite and equal those of the plain run (up to the order of the fp32 atomics of the column sums).
    Regression test: up to r04m the 16x16x32 coordinate kernel's training mode never stored its share of s_e -- the backward's
    dL/d(x_i - x_j) = dL/d(sum_x[i]) * s_e read zeros in a fresh process (the term silently dropped) and stale values after
    another training step.  Ragged graphs: E is not a multiple of the 64-row padding, several chunks."""
    from diffusion_model_amd import autograd as _ag
    H = 36
    d = dims_for(H, 256, 1024, 1024, 1024)
    sizes = [33, 64, 1, 17, 50]
    n = sum(sizes)
    dev = "cuda"
    g = torch.Generator().manual_seed(12)
    h0, x0 = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g) * 1.5
    wh, wx = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g)
    monkeypatch.setattr(_ag, "EDGE_CHUNK", 4300)
    monkeypatch.setenv("EGNN_BWD_GRAPH", "1" if form == "graph" else "0")
    out = {}
    for poison in ("0", "1"):
        monkeypatch.setenv("EGNN_DEBUG_POISON_KEPT", poison)
        torch.manual_seed(9)
        m = dma.EquivariantGNN(2, **d).to(dev).train()
        m.precision, m.norm_scope = "bf16", "graph"
        h = h0.to(dev).requires_grad_(True)
        x = x0.to(dev).requires_grad_(True)
        ho, xo = m(dma.fully_connected_plan(sizes, torch.device(dev)), h, x)
        ((ho * wh.to(dev)).sum() + (xo * wx.to(dev)).sum()).backward()
        assert m._ctx.last_backward_path == "kept activations"
        out[poison] = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
        out[poison]["input.h"], out[poison]["input.x"] = h.grad.detach().cpu(), x.grad.detach().cpu()
    for k in out["0"]:
        assert torch.isfinite(out["1"][k]).all(), k
        assert rel_err(out["1"][k], out["0"][k]) <= 1e-4, k


@pytest.mark.gpu
@pytest.mark.parametrize("prec,env", [("bf16", {}), ("bf16", {"EGNN_BWD_GRAPH": "0"}), ("bf16", {"EGNN_BWD_SAVE": "0"}),
                                      ("bf16", {"EGNN_BWD_FIRST": "1"}), ("fp16", {}), ("fp32", {}), ("bf16x3", {})],
                         ids=["bf16-graph", "bf16-chain", "bf16-recompute", "bf16-reduce", "fp16", "fp32", "bf16x3"])
def test_no_backward_reads_uninitialised_memory(prec, env, monkeypatch):
    """Every workspace the host side hands to the library comes from torch.empty: with torch's debug fill of uninitialised
    memory (NaN in every fresh tensor: torch.utils.deterministic.fill_uninitialized_memory under use_deterministic_algorithms)
    a forward + backward must give the gradients of the plain run -- an element read before it is written would turn them NaN.
    All backward forms of every precision, ragged graphs, several chunks."""
    from diffusion_model_amd import autograd as _ag
    H = 36
    d = dims_for(H, 256, 1024, 1024, 1024)
    sizes = [33, 64, 1, 17, 50]
    n = sum(sizes)
    dev = "cuda"
    g = torch.Generator().manual_seed(13)
    h0, x0 = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g) * 1.5
    wh, wx = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g)
    monkeypatch.setattr(_ag, "EDGE_CHUNK", 4300)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = {}
    old_fill = torch.utils.deterministic.fill_uninitialized_memory
    try:
        for fill in (False, True):
            monkeypatch.setenv("EGNN_DEBUG_POISON", "1" if fill else "0")   # the library's own hipMalloc'ed buffers as 0xFF bytes
            torch.use_deterministic_algorithms(fill, warn_only=True)
            torch.utils.deterministic.fill_uninitialized_memory = fill
            torch.manual_seed(9)
            m = dma.EquivariantGNN(2, **d).to(dev).train()
            m.precision, m.norm_scope = prec, "graph"
            h = h0.to(dev).requires_grad_(True)
            x = x0.to(dev).requires_grad_(True)
            ho, xo = m(dma.fully_connected_plan(sizes, torch.device(dev)), h, x)
            ((ho * wh.to(dev)).sum() + (xo * wx.to(dev)).sum()).backward()
            out[fill] = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
            out[fill]["input.h"], out[fill]["input.x"], out[fill]["out.h"] = h.grad.detach().cpu(), x.grad.detach().cpu(), ho.detach().cpu()
    finally:
        torch.use_deterministic_algorithms(False)
        torch.utils.deterministic.fill_uninitialized_memory = old_fill
    for k in out[False]:
        assert torch.isfinite(out[True][k]).all(), k
        assert rel_err(out[True][k], out[False][k]) <= 1e-4, k


def test_backward_chunks_are_cut_at_graph_boundaries():
    """host logic of the graph-form backward: chunks of WHOLE graphs with at most `rows` edges; None when one graph alone has
    more (the caller then takes the chain that may cut anywhere)"""
    from types import SimpleNamespace
    from diffusion_model_amd.autograd import _graph_chunks
    plan = SimpleNamespace(graph_edge_ptr=[0, 12, 12, 42, 48, 104])      # five graphs, the second without edges
    assert _graph_chunks(plan, 1000) == [(0, 104)]
    assert _graph_chunks(plan, 60) == [(0, 48), (48, 56)]
    assert _graph_chunks(plan, 56) == [(0, 48), (48, 56)]
    assert _graph_chunks(plan, 42) is None                                              # the last graph alone has 56
    assert _graph_chunks(plan, 12) is None
    assert _graph_chunks(SimpleNamespace(), 100) is None                                # a plan without the host copy
    got = _graph_chunks(SimpleNamespace(graph_edge_ptr=[0, 30, 60, 90, 120]), 64)
    assert got == [(0, 60), (60, 60)] and sum(n for _, n in got) == 120
    cpu_plan = dma.GraphPlan(fully_connected_edge_index([3, 1, 4]), 8, sizes=[3, 1, 4])
    assert cpu_plan.graph_edge_ptr == [0, 6, 6, 18] and cpu_plan.max_graph_nodes == 4


@pytest.mark.gpu
@pytest.mark.parametrize("graphs", ["fully_connected", "radius"])
def test_graph_form_backward_against_the_chain_and_fp32_incl_input_gradients(graphs, monkeypatch):
    """the per-graph fused dgrad (csrc/edge_bwd_dgrad_graph.hip: dL/da1 never stored, per-node sums on the matrix cores, node-level
    products) against the round-3 chain (dL/da1 stored, gather / GEMMs over all edges / scatter) on the SAME kept activations and
    against the fp32 backward: every parameter gradient AND the gradients with respect to the inputs h and x, ragged graphs (one
    without edges, one of 64 nodes), chunks of one or two graphs.  "radius": sparse graphs of uneven degree (atoms without any
    edge inside a graph, tiles with dozens of receivers) from the device radius-graph builder.  The bar: the graph form is as
    close to the fp32 gradients as the chain is (it is closer where the chain rounds dL/d(d^2) to bf16: input x, layer 0's
    coordinate MLP -- measured 7.5e-3 against 2.6e-2 on the radius graphs), and within 5e-2 of the chain."""
    from diffusion_model_amd import autograd as _ag
    H = 36
    d = dims_for(H, 256, 1024, 1024, 1024)
    sizes = (33, 64, 1, 17, 50)
    n = sum(sizes)
    dev = "cuda"
    g = torch.Generator().manual_seed(12)
    h0, x0 = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g) * 1.5
    wh, wx = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g)
    plan_sizes = list(sizes)
    monkeypatch.setattr(_ag, "EDGE_CHUNK", 4300)          # 64 x 63 = 4032 edges: the big graph alone; the others in pairs
    out = {}
    for form, prec in (("1", "bf16"), ("0", "bf16"), ("0", "fp32")):
        monkeypatch.setenv("EGNN_BWD_GRAPH", form)
        torch.manual_seed(9)
        m = dma.EquivariantGNN(2, **d).to(dev).train()
        m.precision, m.norm_scope = prec, "graph"
        h = h0.to(dev).requires_grad_(True)
        x = x0.to(dev).requires_grad_(True)
        if graphs == "radius":
            plan = dma.radius_plan(x0.to(dev), plan_sizes, 1.6)
            deg = (plan.row_ptr[1:] - plan.row_ptr[:-1]).cpu()
            assert int(deg.min()) == 0 and int(deg.max()) >= 8 and plan.E > 300       # uneven degrees, some isolated atoms
        else:
            plan = dma.fully_connected_plan(plan_sizes, torch.device(dev))
        assert plan.graph_edge_ptr == plan.row_ptr[plan.graph_ptr.long()].tolist()
        ho, xo = m(plan, h, x)
        ((ho * wh.to(dev)).sum() + (xo * wx.to(dev)).sum()).backward()
        assert _ag.LAST_FIRST_LAYER_FORM == ("graph" if form == "1" else None)
        assert _ag.LAST_PLAN.first == _ag.LAST_FIRST_LAYER_FORM and _ag.LAST_PLAN.fused == _ag.LAST_PLAN.kept == (prec == "bf16")
        grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
        grads["input.h"], grads["input.x"] = h.grad.detach().cpu(), x.grad.detach().cpu()
        out[(form, prec)] = (ho.detach().cpu(), grads)
    assert torch.equal(out[("1", "bf16")][0], out[("0", "bf16")][0])         # same forward
    gg, gc, gf = out[("1", "bf16")][1], out[("0", "bf16")][1], out[("0", "fp32")][1]
    worst = (0.0, None)
    for k in gg:
        assert torch.isfinite(gg[k]).all(), k
        e_g, e_c, e_gc = rel_err(gg[k], gf[k]), rel_err(gc[k], gf[k]), rel_err(gg[k], gc[k])
        worst = max(worst, (e_g, k))
        assert e_g <= e_c + 5e-3, (k, e_g, e_c)
        assert e_gc <= 5e-2, (k, e_gc)
    print(f"{graphs}: graph form vs fp32 worst {worst[0]:.2e} ({worst[1]}); input x: graph {rel_err(gg['input.x'], gf['input.x']):.2e}, "
          f"chain {rel_err(gc['input.x'], gf['input.x']):.2e}")


# Input gradients against the ORACLE.  The round-4 bug (a dropped dL/d(x_i - x_j) term of the kept-activation
# backward) lived exactly in dL/dx of a layer's input, and the test that found it compared HIP with HIP.  Here dL/dh and dL/dx of
# EVERY precision and EVERY backward form are held against the oracle's autograd on the same inputs and the same loss, together
# with the parameter gradients, on ragged fully connected graphs and on sparse radius graphs of uneven degree.
# Bars: fp32-grade precisions north_star's 1e-4 (measured 1e-6 .. 2e-5); bf16 / fp16 1.5 x the worst printed measurement over
# both graph kinds and all backward forms (profiles/r05*_gpu_tests.log), per quantity: (parameter tensors, ONE-element parameters,
# dL/dh, dL/dx).  The one-element parameters (attention.0.bias, mlp_x.4.bias) are sums over all edges of terms of both signs: their
# RELATIVE error is several times that of the weight tensors the same terms feed.
_INPUT_GRAD_TOL = {
    "fp32": (1e-4, 1e-4, 1e-4, 1e-4), "bf16x3": (1e-4, 1e-4, 1e-4, 1e-4), "f16c8": (1e-4, 1e-4, 1e-4, 1e-4),
    # measured worst over graphs x forms (profiles/r05r_gpu_tests.log): bf16 1.29e-2 / 5.9e-2 / 8.2e-3 / 4.3e-3, fp16 7.9e-3 / 7.3e-2 / 7.0e-3 / 4.0e-3
    "bf16": (1.9e-2, 9e-2, 1.25e-2, 6.5e-3), "fp16": (1.2e-2, 1.1e-1, 1.05e-2, 6e-3),
}


@pytest.mark.gpu
@pytest.mark.parametrize("graphs", ["fully_connected", "radius"])
@pytest.mark.parametrize("form", ["graph", "chain", "factorised", "recompute"])
def test_input_and_parameter_gradients_match_oracle_autograd(form, graphs, monkeypatch):
    from diffusion_model_amd import autograd as _ag
    from oracle.egnn_ref import egnn_forward as oracle_forward
    H = 36
    d = dims_for(H, 256, 1024, 1024, 1024)
    sizes = (33, 64, 1, 17, 50)
    n = sum(sizes)
    dev = "cuda"
    g = torch.Generator().manual_seed(12)
    h0, x0 = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g) * 1.5
    wh, wx = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g)
    monkeypatch.setattr(_ag, "EDGE_CHUNK", 4300)          # 64 x 63 = 4032 edges: the big graph alone; the others in pairs
    monkeypatch.setenv("EGNN_BWD_FIRST", "1" if form == "factorised" else "0")
    monkeypatch.setenv("EGNN_BWD_GRAPH", "0" if form in ("chain", "factorised") else "1")
    monkeypatch.setenv("EGNN_BWD_SAVE", "0" if form == "recompute" else "1")
    if graphs == "radius":
        plan = dma.radius_plan(x0.to(dev), list(sizes), 1.6)
    else:
        plan = dma.fully_connected_plan(list(sizes), torch.device(dev))
    ei = dma.plan_edge_index(plan).cpu()
    ptr = torch.tensor([0] + torch.cumsum(torch.tensor(sizes), 0).tolist())
    torch.manual_seed(9)
    ref_net = dma.EquivariantGNN(2, **d)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in ref_net.state_dict().items()}
    hr, xr = h0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    ho_r, xo_r = oracle_forward(sd, ei, hr, xr, "graph", ptr)
    ((ho_r * wh).sum() + (xo_r * wx).sum()).backward()
    want = {k: v.grad for k, v in sd.items()}
    # the fp32-grade precisions share one backward (the fp32 chain): they run under the default form only
    precisions = ("bf16", "fp16") if form != "graph" else ("fp32", "bf16x3", "f16c8", "bf16", "fp16")
    results = {}
    for prec in precisions:
        m = dma.EquivariantGNN(2, **d)
        m.load_state_dict({k: v.detach() for k, v in sd.items()})
        m.to(dev).train()
        m.precision, m.norm_scope = prec, "graph"
        h = h0.to(dev).requires_grad_(True)
        x = x0.to(dev).requires_grad_(True)
        ho, xo = m(plan, h, x)
        ((ho * wh.to(dev)).sum() + (xo * wx.to(dev)).sum()).backward()
        if prec == "bf16":     # the form under test is the one that ran (fp16 forwards recompute on the bf16 kernels)
            assert _ag.LAST_FIRST_LAYER_FORM == {"graph": "graph", "chain": None, "factorised": "reduce", "recompute": "graph"}[form]
            assert m._ctx.last_backward_path == ("recompute" if form == "recompute" else "kept activations")
            bp = _ag.LAST_PLAN
            assert (bp.first, bp.kept, bp.fused, bp.hip_gemms, bp.node) == (_ag.LAST_FIRST_LAYER_FORM, form != "recompute", True, True, "hip")
        e_par = {k: rel_err(p.grad.detach().cpu(), want[k]) for k, p in m.named_parameters()}
        e_h, e_x = rel_err(h.grad.detach().cpu(), hr.grad), rel_err(x.grad.detach().cpu(), xr.grad)
        multi = {k: e for k, e in e_par.items() if want[k].numel() > 1}
        single = {k: e for k, e in e_par.items() if want[k].numel() == 1}
        wm, ws1 = max(multi, key=multi.get), max(single, key=single.get)
        print(f"input gradients vs oracle autograd [{graphs}, {form}] {prec}: dL/dh {e_h:.2e} dL/dx {e_x:.2e} "
              f"parameter tensors worst {multi[wm]:.2e} ({wm}), one-element parameters worst {single[ws1]:.2e} ({ws1})")
        assert torch.isfinite(h.grad).all() and torch.isfinite(x.grad).all()
        results[prec] = (multi[wm], single[ws1], e_h, e_x)
    for prec, got in results.items():
        for name, g_, t_ in zip(("parameter tensors", "one-element parameters", "dL/dh", "dL/dx"), got, _INPUT_GRAD_TOL[prec]):
            assert g_ <= t_, (graphs, form, prec, name, g_, t_)


# Fused kernels WITHOUT the library's own GEMMs: H = 64 makes in = [h_i | h_j | d2 | 1] 130 columns wide, more than the 128 of
# gemm_tn.hip / gemm_rows.hip, so the context-handle kernels (heads_saved / edge_recompute, dgrad) run between library products
# (_wgrad, _mm on bf16 buffers, the -ln 2 fix-up of the second-layer weight gradients) and torch's node MLP.
# Bars: 1.5 x the measurement of the four quantities on the commit before the backward plan, which runs the same path
# (profiles/bwd_plan_ab.txt), per case (parameter tensors, one-element parameters, dL/dh, dL/dx):
#   kept      8.22e-3 (egcl_list.1.mlp_x.0.bias) / 7.16e-3 (egcl_list.0.attention.0.bias) / 4.94e-3 / 2.59e-3
#   recompute 8.54e-3 (egcl_list.1.mlp_x.0.bias) / 8.19e-3 (egcl_list.0.attention.0.bias) / 4.89e-3 / 2.79e-3
_H64_TOL = {"1": (1.23e-2, 1.07e-2, 7.4e-3, 3.87e-3), "0": (1.28e-2, 1.22e-2, 7.3e-3, 4.18e-3)}


@pytest.mark.gpu
@pytest.mark.parametrize("save", ["1", "0"], ids=["kept", "recompute"])
def test_fused_kernels_without_own_gemms_match_oracle_autograd(save, monkeypatch):
    from diffusion_model_amd import autograd as _ag
    from oracle.egnn_ref import egnn_forward as oracle_forward
    H = 64
    d = dims_for(H, 256, 256, 256, 256)
    sizes = (64, 1, 33, 2, 17, 50)                        # the fully connected batch of tests/test_gpu_bwd_stages.py: 7,812 edges
    n = sum(sizes)
    dev = "cuda"
    g = torch.Generator().manual_seed(12)
    h0, x0 = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g) * 1.5
    wh, wx = torch.randn(n, H, generator=g), torch.randn(n, 3, generator=g)
    monkeypatch.setattr(_ag, "EDGE_CHUNK", 4300)          # two chunks, the second not a multiple of 64 rows
    monkeypatch.setenv("EGNN_BWD_SAVE", save)
    plan = dma.fully_connected_plan(list(sizes), torch.device(dev))
    ei = dma.plan_edge_index(plan).cpu()
    ptr = torch.tensor([0] + torch.cumsum(torch.tensor(sizes), 0).tolist())
    torch.manual_seed(9)
    ref_net = dma.EquivariantGNN(2, **d)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in ref_net.state_dict().items()}
    hr, xr = h0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    ho_r, xo_r = oracle_forward(sd, ei, hr, xr, "graph", ptr)
    ((ho_r * wh).sum() + (xo_r * wx).sum()).backward()
    want = {k: v.grad for k, v in sd.items()}
    m = dma.EquivariantGNN(2, **d)
    m.load_state_dict({k: v.detach() for k, v in sd.items()})
    m.to(dev).train()
    m.precision, m.norm_scope = "bf16", "graph"
    h = h0.to(dev).requires_grad_(True)
    x = x0.to(dev).requires_grad_(True)
    ho, xo = m(plan, h, x)
    ((ho * wh.to(dev)).sum() + (xo * wx.to(dev)).sum()).backward()
    bp = _ag.LAST_PLAN
    assert bp.fused and not bp.hip_gemms and bp.first is None and bp.kept == (save == "1")
    assert (bp.node, bp.K1P, bp.chunks) == ("torch", 136, ((0, 4352), (4352, 3460)))
    assert m._ctx.last_backward_path == ("kept activations" if save == "1" else "recompute")
    e_par = {k: rel_err(p.grad.detach().cpu(), want[k]) for k, p in m.named_parameters()}
    e_h, e_x = rel_err(h.grad.detach().cpu(), hr.grad), rel_err(x.grad.detach().cpu(), xr.grad)
    multi = {k: e for k, e in e_par.items() if want[k].numel() > 1}
    single = {k: e for k, e in e_par.items() if want[k].numel() == 1}
    wm, ws1 = max(multi, key=multi.get), max(single, key=single.get)
    print(f"input gradients vs oracle autograd [H = 64, fused without own GEMMs, SAVE={save}] bf16: dL/dh {e_h:.2e} dL/dx {e_x:.2e} "
          f"parameter tensors worst {multi[wm]:.2e} ({wm}), one-element parameters worst {single[ws1]:.2e} ({ws1})")
    assert torch.isfinite(h.grad).all() and torch.isfinite(x.grad).all()
    for name, g_, t_ in zip(("parameter tensors", "one-element parameters", "dL/dh", "dL/dx"), (multi[wm], single[ws1], e_h, e_x),
                            _H64_TOL[save]):
        assert g_ <= t_, (save, name, g_, t_)


@pytest.mark.gpu
def test_split_products_match_fp64():
    """gemm.mm_tn_split / mm_nn_split (head + remainder bf16 operands, three products on the library's own kernels: the products of
    the tolerance-grade backward) against float64 products: 2^-16 per operand -> <= 3e-5 relative (measured
    ~6e-6); odd sizes exercise the padding (rows not a multiple of 64, widths not multiples of 64 / 128 / 256)."""
    from diffusion_model_amd.gemm import mm_nn_split, mm_tn_split
    g = torch.Generator().manual_seed(4)
    for E, Ma, Nb in ((5000, 1024, 1024), (4097, 36, 1024), (3001, 1024, 74), (777, 292, 130)):
        a = (torch.randn(E, Ma, generator=g) * torch.logspace(-2, 1, Ma)).cuda()      # columns of very different magnitude
        b = torch.randn(E, Nb, generator=g).cuda()
        got = mm_tn_split(a, b)
        want = a.double().t() @ b.double()
        e = rel_err(got.cpu(), want.cpu())
        print(f"mm_tn_split [{E}, {Ma}]^T [{E}, {Nb}]: {e:.2e}")
        assert e <= 3e-5
    for E, K, N in ((5000, 1024, 1024), (4097, 36, 1024), (3001, 1024, 74), (777, 292, 292)):
        a = torch.randn(E, K, generator=g).cuda()
        w = (torch.randn(K, N, generator=g) * 0.05).cuda()
        got = mm_nn_split(a, w)
        want = a.double() @ w.double()
        e = rel_err(got.cpu(), want.cpu())
        print(f"mm_nn_split [{E}, {K}] [{K}, {N}]: {e:.2e}")
        assert e <= 3e-5 and got.shape == (E, N)


@pytest.mark.gpu
def test_node_activation_stage_matches_torch():
    """egcl_backward_node_act: s = SiLU(z + b1), dL/dz = dL/ds * SiLU'(z + b1) as bf16 and the bias gradient, against float64
    torch on the same inputs (row strides wider than W, N not a multiple of the 64-row block, W not a multiple of 256)"""
    from diffusion_model_amd import _lib
    N, W, ld = 1000, 320, 384
    g = torch.Generator().manual_seed(2)
    z = (torch.randn(N, ld, generator=g) * 3).cuda()
    gs = torch.randn(N, ld, generator=g).cuda()
    b1 = torch.randn(W, generator=g).cuda()
    gz = torch.full((N, ld), 7.0, dtype=torch.bfloat16, device="cuda")
    so = torch.full((N, ld), 7.0, dtype=torch.bfloat16, device="cuda")
    gb = torch.zeros(W, device="cuda")
    _lib.check(_lib.lib().egcl_backward_node_act(_lib.stream_ptr(), N, W, _lib.ptr(z), ld, _lib.ptr(b1), _lib.ptr(gs), ld, _lib.ptr(gz),
                                                 _lib.ptr(so), ld, _lib.ptr(gb)))
    a = (z[:, :W] + b1).double()
    sg = torch.sigmoid(a)
    want_s, want_g = a * sg, gs[:, :W].double() * (sg * (1 + a * (1 - sg)))
    assert rel_err(so[:, :W].double().cpu(), want_s.cpu()) <= 4e-3 and rel_err(gz[:, :W].double().cpu(), want_g.cpu()) <= 4e-3   # bf16
    assert rel_err(gb.double().cpu(), want_g.sum(0).cpu()) <= 1e-5
    assert float(gz[:, W:].float().min()) == 7.0 and float(so[:, W:].float().min()) == 7.0      # columns past W untouched
    assert _lib.lib().egcl_backward_node_act(_lib.stream_ptr(), N, 322, _lib.ptr(z), ld, _lib.ptr(b1), _lib.ptr(gs), ld, _lib.ptr(gz),
                                             _lib.ptr(so), ld, _lib.ptr(gb)) != 0            # W % 4 != 0 is refused


# ---------------- data-parallel training step on RCCL (needs >= 2 GPUs: skipped on a one-GPU box) ----------------
def _nccl_worker(rank, world, port, out, force_active=False):
    """one rank per GPU, backend nccl (= RCCL on ROCm): each rank runs the real forward + backward on its shard of the
    graphs with the overlapped per-layer all-reduce (GradAllReducer.armed), the loss divided by the GLOBAL graph count"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(rank)
    dev = torch.device("cuda", rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    H, A, T = 36, 2, 50
    d = dims_for(H, 128, 256, 256, 256)
    torch.manual_seed(3)
    net = dma.EquivariantGNN(2, **d).to(dev)
    net.norm_scope = "graph"
    sizes = (6, 4, 7, 5)
    pos0, x0, cond, batch, ei, npos, nh, _ = _problem(seed=5, sizes=sizes)
    times = [17, 3, 40, 22]
    mine = [g for g in range(len(sizes)) if g % world == rank]
    sel = torch.cat([(batch == g).nonzero().flatten() for g in mine])
    lsizes = [sizes[g] for g in mine]
    lbatch = torch.repeat_interleave(torch.arange(len(mine)), torch.tensor(lsizes)).to(dev)
    lei = fully_connected_edge_index(lsizes).to(dev)
    proc = dma.E3DiffusionProcess(1e-5, 2.0, T)
    red = dma.GradAllReducer(list(net.egcl_list))
    if force_active:   # one-rank rehearsal: issue the collectives although a single rank has nothing to exchange
        red._active = lambda: True
    assert red.stream is not None          # backend nccl: the buckets go out on the process's communication stream
    noised = dma.diffuse_as_batch(pos0[sel].to(dev), x0[sel].to(dev), lbatch, proc, times=[times[g] for g in mine],
                                  noise_pos=npos[sel].to(dev), noise_h=nh[sel].to(dev), num_graphs=len(mine))
    with red.armed():
        loss, _, _ = dma.training_loss(net, lei, lbatch, noised, cond[sel].to(dev), A, num_graph_global=len(sizes),
                                       num_graphs=len(mine))
        loss.backward()
    tot = loss.detach().clone()
    dist.all_reduce(tot)
    torch.cuda.synchronize(dev)
    if rank == 0:
        torch.save({"loss": float(tot), "grads": {k: p.grad.cpu() for k, p in net.named_parameters()},
                    "world": dist.get_world_size(), "backend": dist.get_backend()}, out)
    dist.barrier()
    dist.destroy_process_group()


def _single_process_reference():
    dev = "cuda:0"
    H, A, T = 36, 2, 50
    d = dims_for(H, 128, 256, 256, 256)
    torch.manual_seed(3)
    net = dma.EquivariantGNN(2, **d).to(dev)
    net.norm_scope = "graph"
    sizes = (6, 4, 7, 5)
    pos0, x0, cond, batch, ei, npos, nh, _ = _problem(seed=5, sizes=sizes)
    proc = dma.E3DiffusionProcess(1e-5, 2.0, T)
    noised = dma.diffuse_as_batch(pos0.to(dev), x0.to(dev), batch.to(dev), proc, times=[17, 3, 40, 22], noise_pos=npos.to(dev),
                                  noise_h=nh.to(dev), num_graphs=4)
    loss, _, _ = dma.training_loss(net, ei.to(dev), batch.to(dev), noised, cond.to(dev), A, num_graphs=4)
    loss.backward()
    return float(loss.detach()), {k: p.grad.cpu() for k, p in net.named_parameters()}


@pytest.mark.gpu
def test_reducer_collectives_on_rccl_one_rank_rehearsal(tmp_path):
    """What a one-GPU box can rehearse of the RCCL path: ONE rank under backend nccl with the reducer forced to issue its
    per-layer all-reduces (communication stream, record_stream, wait_stream, dist.all_reduce on the RCCL communicator) from
    inside the real backward; a sum over one rank must leave the gradients exactly those of the plain step."""
    out = str(tmp_path / "nccl1.pt")
    mp.spawn(_nccl_worker, args=(1, _free_port(), out, True), nprocs=1, join=True)
    res = torch.load(out, weights_only=True)
    assert res["world"] == 1 and res["backend"] == "nccl"
    loss, grads = _single_process_reference()
    assert abs(loss - res["loss"]) <= 1e-6 * abs(loss)
    for k, g in grads.items():
        assert rel_err(res["grads"][k], g) <= 1e-5, k   # same kernels, same order; the fp32 atomics of the scatter reorder


@pytest.mark.gpu
def test_ddp_gradients_on_rccl_equal_single_process(tmp_path):
    """BASELINE configs[3]'s exchange on real RCCL: 2 ranks x 2 graphs each == one process on the 4 graphs (2e-3: the
    segment sums of the two shards associate differently).  Needs two visible GPUs; the round's one-GPU box skips it."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs (RCCL over xGMI); the gloo world_size-2 tests cover the logic on CPU")
    out = str(tmp_path / "nccl.pt")
    mp.spawn(_nccl_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    res = torch.load(out, weights_only=True)
    assert res["world"] == 2 and res["backend"] == "nccl"
    dev = "cuda:0"
    H, A, T = 36, 2, 50
    d = dims_for(H, 128, 256, 256, 256)
    torch.manual_seed(3)
    net = dma.EquivariantGNN(2, **d).to(dev)
    net.norm_scope = "graph"
    sizes = (6, 4, 7, 5)
    pos0, x0, cond, batch, ei, npos, nh, _ = _problem(seed=5, sizes=sizes)
    proc = dma.E3DiffusionProcess(1e-5, 2.0, T)
    noised = dma.diffuse_as_batch(pos0.to(dev), x0.to(dev), batch.to(dev), proc, times=[17, 3, 40, 22], noise_pos=npos.to(dev),
                                  noise_h=nh.to(dev), num_graphs=4)
    loss, _, _ = dma.training_loss(net, ei.to(dev), batch.to(dev), noised, cond.to(dev), A, num_graphs=4)
    loss.backward()
    assert abs(float(loss.detach()) - res["loss"]) <= 1e-4 * abs(res["loss"])
    for k, p in net.named_parameters():
        assert rel_err(res["grads"][k], p.grad.cpu()) <= 2e-3, k

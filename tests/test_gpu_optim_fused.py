"""GPU tests of the fused optimizer step (csrc/optim/optim_step.hip): the kernel against its numpy mirror bit for bit (every
element of p and of every state, aligned and misaligned layouts, the memory around the tensors untouched), the fused classes
over whole trajectories, state_dict interchange with the unfused classes, train() / eval(), and the training loop."""
import ctypes as C
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import diffusion_model_amd as dma
from diffusion_model_amd import _lib
from tests import _optim_cases as cases
from tests import _optim_mirror as mirror
from tests._util import dims_for
from tests.test_training import _problem

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 777.25
PAD = 8          # sentinel elements kept on both sides of every view


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.int32)


def _same_bits(got, want):
    return np.array_equal(_bits(got), _bits(want))


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _abi_step(kind, consts, p, g, s0, s1, s2=None):
    n = len(p)
    _lib.check(_lib.lib().egnn_optim_step(_lib.stream_ptr(), kind, n, _ptrs(p), _ptrs(g), _ptrs(s0), _ptrs(s1),
                                          _ptrs(s2) if s2 is not None else None, (C.c_int64 * n)(*[t.numel() for t in p]),
                                          _lib.OptimConsts(**consts)))


class Placed:
    """host arrays placed on the device as 1-D views inside sentinel-filled buffers.  layout: 'separate' = one 16-byte aligned
    allocation per tensor; 'offset' = every tensor in a buffer of its own at element offset 1, 2 or 3 (chosen per tensor and per
    stream, so the streams of one tensor are misaligned independently); 'flat' = all tensors of the stream in ONE buffer at
    offsets that are equal across streams up to the stream's own misalignment (equal state spacing: one launch)."""

    def __init__(self, arrays, layout, stream_id):
        self.bufs, self.views, self.ranges = [], [], []
        if layout == "flat":
            offs, total = [], PAD + (stream_id * 2 + 1) % 4
            for a in arrays:
                offs.append(total)
                total += (a.size + 3) // 4 * 4
            buf = torch.full((total + PAD,), SENTINEL, device=DEV)
            self.bufs = [buf]
            for a, o in zip(arrays, offs):
                self.ranges.append((0, o, o + a.size))
        else:
            for i, a in enumerate(arrays):
                o = 4 * (PAD // 4) + (0 if layout == "separate" else 1 + (i + stream_id) % 3)
                self.bufs.append(torch.full((o + a.size + PAD,), SENTINEL, device=DEV))
                self.ranges.append((i, o, o + a.size))
        for a, (b, lo, hi) in zip(arrays, self.ranges):
            v = self.bufs[b][lo:hi]
            v.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
            self.views.append(v)

    def surroundings_untouched(self):
        keep = [torch.ones_like(b, dtype=torch.bool) for b in self.bufs]
        for b, lo, hi in self.ranges:
            keep[b][lo:hi] = False
        return all(bool((b[k] == SENTINEL).all()) for b, k in zip(self.bufs, keep))


def _mirror_snapshots(name, at):
    """mirror state BEFORE and AFTER each step in ``at``, with the step's constants and gradients"""
    m, out = cases.MirrorRun(name), {}
    for k in range(1, max(at) + 1):
        before = ([a.copy() for a in m.p], [[a.copy() for a in st] for st in m.s]) if k in at else None
        gs = cases.grads(k)
        m.step(gs)
        if k in at:
            out[k] = dict(before=before, after=([a.copy() for a in m.p], [[a.copy() for a in st] for st in m.s]), consts=m.last_consts,
                          grads=[g.numpy() for g in gs])
    return out


@pytest.mark.parametrize("name", list(cases.CONFIGS))
def test_single_steps_equal_the_mirror_bit_for_bit(name):
    """6(a): one kernel step from the mirror's state at k = 1 (fresh states), 4 (silent), 5 (first rectified) and 40, through the
    C ABI, in three memory layouts; every element of p and of every state equals the mirror's, and nothing around them moved"""
    kind = cases.KINDS[cases.CONFIGS[name][0]]
    snaps = _mirror_snapshots(name, (1, 4, 5, 40))
    for k, sn in snaps.items():
        for layout in ("separate", "offset", "flat"):
            (p0, s_before), (p1, s_after) = sn["before"], sn["after"]
            P, G = Placed(p0, layout, 0), Placed(sn["grads"], layout, 1)
            S = [Placed(st, layout, 2 + j) for j, st in enumerate(s_before)]
            _abi_step(kind, sn["consts"], P.views, G.views, S[0].views, S[1].views, S[2].views if len(S) > 2 else None)
            torch.cuda.synchronize()
            for i in range(len(p0)):
                assert _same_bits(P.views[i], p1[i]), (name, k, layout, "p", i)
                assert _same_bits(G.views[i], sn["grads"][i]), (name, k, layout, "g", i)
                for j in range(len(S)):
                    assert _same_bits(S[j].views[i], s_after[j][i]), (name, k, layout, "state", j, i)
            assert all(x.surroundings_untouched() for x in [P, G] + S), (name, k, layout)


@pytest.mark.parametrize("name", ["radam_decay", "adam", "adamw"])
def test_missing_gradient_and_long_list(name):
    """a NULL gradient leaves its tensor alone; a list of capacity + 3 tensors (two launches) is stepped completely"""
    kind = cases.KINDS[cases.CONFIGS[name][0]]
    cap = _lib.lib().egnn_optim_tensors_per_launch()
    shapes = [((i * 613) % 4500 + 1,) for i in range(cap + 3)]
    shapes[5], shapes[cap + 1] = (1,), (2 * 2048 + 3,)
    skip = {2, cap + 2}
    m = cases.MirrorRun(name, shapes)
    P = Placed(m.p, "flat", 0)
    S = [Placed(st, "flat", 2 + j) for j, st in enumerate(m.s)]
    adam = kind != cases.KINDS["RAdamScheduleFree"]
    for k in range(1, 7):                                  # through the silent phase into the rectified one
        gs = cases.grads(k, shapes)
        G = Placed([g.numpy() for g in gs], "flat", 1)
        m.step(gs, skip=skip if k == 3 else ())            # step 3: two tensors without a gradient
        states = (S[0].views, S[1].views, S[2].views if len(S) > 2 else None)
        main = [None if (i in skip and (k == 3 or (adam and k > 3))) else v for i, v in enumerate(G.views)]
        _abi_step(kind, m.last_consts, P.views, main, *states)
        if adam and k > 3:
            # torch's Adam counts steps per tensor: the two tensors are one step behind from here on, so they take a call of their
            # own with their step's constants (as FusedAdam issues it), every other gradient NULL
            late = [v if i in skip else None for i, v in enumerate(G.views)]
            late_consts = dma.optim.adam_scalars(k - 1, m.group["lr"], m.group["betas"], m.group["eps"], m.group["weight_decay"])
            _abi_step(kind, late_consts, P.views, late, *states)
    torch.cuda.synchronize()
    for i in range(len(shapes)):
        assert _same_bits(P.views[i], m.p[i]), (name, "p", i)
        for j in range(len(S)):
            assert _same_bits(S[j].views[i], m.s[j][i]), (name, "state", j, i)
    assert all(x.surroundings_untouched() for x in [P] + S)


def _device_params():
    return [torch.nn.Parameter(p.to(DEV)) for p in cases.init_params()]


def _fused_steps(opt, params, first, steps, skip_at=None):
    for k in range(first, first + steps):
        for i, (p, g) in enumerate(zip(params, cases.grads(k))):
            p.grad = None if skip_at == (k, i) else g.to(DEV)
        opt.step()


@pytest.mark.parametrize("name", list(cases.CONFIGS))
def test_fused_trajectory_equals_the_mirror_bit_for_bit(name):
    """6(b) + 7: the fused class over all 40 steps (states created by the class at step 1, one gradient None at step 3) against
    the mirror: p and every state bitwise; RAdamScheduleFree's silent phase leaves p and z bitwise untouched"""
    kind, kw = cases.CONFIGS[name]
    params = _device_params()
    opt = cases.make_fused(name, params)
    m = cases.MirrorRun(name)
    if kind == "RAdamScheduleFree":
        opt.train()
    p_start = [p.detach().clone() for p in params]
    for k in range(1, cases.K + 1):
        skip = {6} if k == 3 else ()
        _fused_steps(opt, params, k, 1, skip_at=(3, 6))
        m.step(cases.grads(k), skip=skip)
        if kind == "RAdamScheduleFree" and kw.get("silent_sgd_phase", True) and k == 4:
            for p, q in zip(params, p_start):
                assert _same_bits(p, q) and _same_bits(opt.state[p]["z"], q)
            assert opt.param_groups[0]["scheduled_lr"] == 0.0
    keys = cases.STATE_KEYS[kind]
    for i, p in enumerate(params):
        assert _same_bits(p, m.p[i]), (name, "p", i)
        for j, key in enumerate(keys):
            assert _same_bits(opt.state[p][key], m.s[j][i]), (name, key, i)
        if kind != "RAdamScheduleFree":
            assert float(opt.state[p]["step"]) == m.steps[i] and not opt.state[p]["step"].is_cuda
    if kind == "RAdamScheduleFree":
        assert all(opt.param_groups[0][f] == m.group[f] for f in ("k", "weight_sum", "lr_max", "scheduled_lr"))
    # states are views of the group's flat buffers, and leave through state_dict() as tensors of their own
    sd = opt.state_dict()
    assert sorted(sd["state"][0]) == sorted(keys + (() if kind == "RAdamScheduleFree" else ("step",)))
    assert sd["state"][4][keys[0]].untyped_storage().nbytes() == params[4].numel() * 4


def test_two_param_groups_step_with_their_own_constants():
    """several param_groups = one launch per group, each with its own hyper-parameters and flat state buffers"""
    shapes = (cases.SHAPES[:3], cases.SHAPES[5:])
    names = ("radam_decay", "radam_loud")
    params = [[torch.nn.Parameter(p.to(DEV)) for p in cases.init_params(sh)] for sh in shapes]
    opt = dma.FusedRAdamScheduleFree([dict(params=ps, **cases.CONFIGS[n][1]) for ps, n in zip(params, names)])
    mirrors = [cases.MirrorRun(n, sh) for n, sh in zip(names, shapes)]
    opt.train()
    for k in range(1, 8):
        for ps, sh, m in zip(params, shapes, mirrors):
            gs = cases.grads(k, sh)
            for p, g in zip(ps, gs):
                p.grad = g.to(DEV)
            m.step(gs)
        opt.step()
    for ps, m, group in zip(params, mirrors, opt.param_groups):
        assert group["k"] == 7 and group["weight_sum"] == m.group["weight_sum"]
        for i, p in enumerate(ps):
            assert _same_bits(p, m.p[i]) and _same_bits(opt.state[p]["z"], m.s[0][i]) and _same_bits(opt.state[p]["exp_avg_sq"], m.s[1][i])


@pytest.mark.parametrize("name", list(cases.CONFIGS))
def test_state_dict_moves_between_fused_and_unfused(name):
    """8: 10 steps of one class -> the other class loads its state_dict -> 10 more steps on both, in both directions.  Each end
    is within 2 x the all-unfused fp32 run's distance from the float64 run (the criterion of the CPU accuracy test); the group
    fields survive the move exactly."""
    kind = cases.CONFIGS[name][0]
    p0 = cases.init_params()
    p64, _ = cases.run_unfused(name, 20, torch.float64)
    pu, optu = cases.run_unfused(name, 10, torch.float32, device=DEV)
    fields = ("k", "weight_sum", "lr_max", "train_mode", "scheduled_lr") if kind == "RAdamScheduleFree" else ("lr", "betas", "eps", "weight_decay")
    # unfused -> fused
    pf = [torch.nn.Parameter(p.detach().clone()) for p in pu]
    optf = cases.make_fused(name, pf)
    optf.load_state_dict(optu.state_dict())
    assert all(optf.param_groups[0][f] == optu.param_groups[0][f] for f in fields)
    _fused_steps(optf, pf, 11, 10)
    cases.run_unfused(name, 10, torch.float32, device=DEV, first=11, params=pu, opt=optu)
    e_unfused = cases.update_error(pu, p64, p0)
    e_moved = cases.update_error(pf, p64, p0)
    print(f"state interchange {name}: all unfused {e_unfused:.3e}, unfused -> fused {e_moved:.3e}")
    assert e_unfused > 0 and e_moved <= 2 * e_unfused
    # fused -> unfused
    pf2 = _device_params()
    optf2 = cases.make_fused(name, pf2)
    if kind == "RAdamScheduleFree":
        optf2.train()
    _fused_steps(optf2, pf2, 1, 10)
    pu2 = [torch.nn.Parameter(p.detach().clone()) for p in pf2]
    optu2 = cases.make_unfused(name, pu2)
    optu2.load_state_dict(optf2.state_dict())
    assert all(optu2.param_groups[0][f] == optf2.param_groups[0][f] for f in fields)
    cases.run_unfused(name, 10, torch.float32, device=DEV, first=11, params=pu2, opt=optu2)
    _fused_steps(optf2, pf2, 11, 10)
    e_back, e_fused = cases.update_error(pu2, p64, p0), cases.update_error(pf2, p64, p0)
    print(f"state interchange {name}: fused -> unfused {e_back:.3e}, all fused {e_fused:.3e}")
    assert e_back <= 2 * e_unfused and e_fused <= 2 * e_unfused
    if kind == "RAdamScheduleFree":
        assert all(optu2.param_groups[0][f] == optf2.param_groups[0][f] for f in fields)


@pytest.mark.parametrize("name", ["adamw", "radam_decay"])
def test_a_deep_copy_goes_on_stepping_alike(name):
    """copy.deepcopy (the pickle protocol: only defaults, state and param_groups travel) gives an optimizer of its own whose next
    steps are bitwise those of the original"""
    import copy
    params = _device_params()
    opt = cases.make_fused(name, params)
    if cases.CONFIGS[name][0] == "RAdamScheduleFree":
        opt.train()
    _fused_steps(opt, params, 1, 6)
    twin = copy.deepcopy(opt)
    twin_params = twin.param_groups[0]["params"]
    assert all(a is not b and a.data_ptr() != b.data_ptr() for a, b in zip(params, twin_params))
    _fused_steps(opt, params, 7, 3)
    _fused_steps(twin, twin_params, 7, 3)
    for a, b in zip(params, twin_params):
        assert _same_bits(a, b)
        for key in cases.STATE_KEYS[cases.CONFIGS[name][0]]:
            assert _same_bits(opt.state[a][key], twin.state[b][key])
            assert opt.state[a][key].data_ptr() != twin.state[b][key].data_ptr()


def test_train_eval_switch():
    """9: eval() is the mirror's interpolation bitwise, eval() then train() returns y within the unfused property test's 1e-6,
    step() in eval mode raises as the unfused class does"""
    params = _device_params()
    opt = cases.make_fused("radam_loud", params)
    with pytest.raises(RuntimeError, match="eval mode"):
        opt.step()
    opt.train()
    _fused_steps(opt, params, 1, 12)
    y = [p.detach().clone() for p in params]
    beta1 = opt.param_groups[0]["betas"][0]
    opt.eval()
    assert opt.param_groups[0]["train_mode"] is False
    for p, y_ in zip(params, y):
        want = y_.cpu().numpy().copy()
        mirror.interp(want, opt.state[p]["z"].cpu().numpy(), 1 - 1 / beta1)
        assert _same_bits(p, want)
    assert any(not torch.equal(p.detach(), y_) for p, y_ in zip(params, y))
    with pytest.raises(RuntimeError, match="eval mode"):
        opt.step()
    x = [p.detach().clone() for p in params]
    opt.eval()                                              # already in eval mode: nothing moves
    assert all(torch.equal(p.detach(), x_) for p, x_ in zip(params, x))
    opt.train()
    for p, y_ in zip(params, y):
        assert torch.allclose(p.detach(), y_, atol=1e-6)
    opt.eval()
    for p, x_ in zip(params, x):
        assert torch.allclose(p.detach(), x_, atol=1e-6)


def _small_training_problem():
    """the network and batch of tests/test_training.py::test_train_step_reduces_loss"""
    H, A, T = 36, 2, 50
    params = dict(conditional=True, to_compress_spectrum=True, give_exO=True, atom_type_size=A, lr=1e-4, weight_decay=1e-12,
                  noise_schedule="predefined")
    d = dims_for(H, 128, 256, 256, 256)
    torch.manual_seed(1)
    nn_dict = {"egnn": dma.EquivariantGNN(2, **d).to(DEV), "spectrum_compressor": dma.SpectrumCompressor(200, [150, 100, 50], 32).to(DEV)}
    nn_dict["egnn"].norm_scope = "graph"
    pos0, x0, _, batch, ei, *_ = _problem()
    spec = torch.zeros(pos0.shape[0], 200)
    spec[[0, 6, 10]] = torch.rand(3, 200)
    exo = torch.zeros(pos0.shape[0], 1)
    exo[[0, 6, 10]] = 1
    data = SimpleNamespace(pos=pos0.to(DEV), x=x0.to(DEV), batch=batch.to(DEV), edge_index=ei.to(DEV), spectrum=spec.to(DEV),
                           exO=exo.to(DEV))
    return nn_dict, data, params, dma.E3DiffusionProcess(1e-5, 2.0, T)


@pytest.mark.parametrize("kind,lr,steps", [("Adam", 1e-4, 12), ("AdamW", 1e-4, 12), ("RAdamScheduleFree", 2.5e-3, 20)])
def test_fused_optimizers_in_the_training_loop(kind, lr, steps):
    """10: train_step with each fused optimizer on the small network and batch of tests/test_training.py.  The first-step loss is
    the unfused run's bitwise (same forward, parameters and noise draw), parameters stay finite, the loss falls by that test's
    own criterion after ``steps`` steps (20 for RAdamScheduleFree: 4 silent steps, then the rectified rate climbs from 0.02 lr),
    and GradAllReducer.check_covers accepts the optimizer."""
    first = {}
    for fused in (False, True):
        nn_dict, data, params, proc = _small_training_problem()
        params["lr"] = lr
        opt = dma.define_optimizer(params, nn_dict, proc, kind, fused=fused)
        assert type(opt).__name__ == ("Fused" if fused else "") + {"AdamW": "AdamW", "Adam": "Adam"}.get(kind, kind)
        if kind == "RAdamScheduleFree":
            opt.train()
        first[fused] = float(dma.train_step(nn_dict, data, params, proc, opt, times=[20, 20, 20]))
    assert first[True] == first[False]
    # (the fused run of the loop above is the one left alive: go on with it)
    red = dma.GradAllReducer(list(nn_dict["egnn"].egcl_list) + [nn_dict["spectrum_compressor"]])
    red.check_covers(opt)
    losses = [first[True]] + [float(dma.train_step(nn_dict, data, params, proc, opt, reducer=red, times=[20, 20, 20])) for _ in range(steps - 1)]
    print(f"fused {kind} in train_step: losses {losses[0]:.4f} -> {losses[-3:]}")
    assert all(l == l for l in losses)
    assert min(losses[-3:]) < losses[0]
    every = list(nn_dict["egnn"].parameters()) + list(nn_dict["spectrum_compressor"].parameters())
    assert all(bool(torch.isfinite(p).all()) for p in every)
    assert all(p.grad is not None for p in nn_dict["spectrum_compressor"].parameters())


def test_fused_radam_in_train_and_eval_epoch():
    """10: train_epoch / eval_epoch drive train() / eval() of the fused RAdamScheduleFree as they drive the unfused one's"""
    nn_dict, data, params, proc = _small_training_problem()
    params.update(optimizer="RAdamScheduleFree", lr=2.5e-3, fused_optimizer=True)
    opt = dma.define_optimizer(params, nn_dict, proc, "RAdamScheduleFree")
    assert isinstance(opt, dma.FusedRAdamScheduleFree) and isinstance(opt, dma.RAdamScheduleFree)
    random.seed(3)
    losses = []
    for epoch in range(3):
        tl = dma.train_epoch(nn_dict, [data] * 4, params, proc, opt)
        assert opt.param_groups[0]["train_mode"] is True
        y = [p.detach().clone() for p in nn_dict["egnn"].parameters()]
        el = dma.eval_epoch(nn_dict, [data], params, proc, opt)
        assert opt.param_groups[0]["train_mode"] is False
        losses.append((tl, el))
        assert tl == tl and el == el
        if epoch > 0:      # after the silent phase x (the averaged iterate) differs from y
            assert any(not torch.equal(p.detach(), y_) for p, y_ in zip(nn_dict["egnn"].parameters(), y))
    assert opt.param_groups[0]["k"] == 12
    assert all(bool(torch.isfinite(p).all()) for p in nn_dict["egnn"].parameters())

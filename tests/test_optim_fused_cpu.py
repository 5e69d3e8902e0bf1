"""CPU tests of the fused optimizer step (csrc/optim/optim_step.hip behind FusedAdam / FusedAdamW / FusedRAdamScheduleFree):
the arithmetic the kernel performs (through its numpy mirror) against the unfused classes in float64, the per-step scalar
functions, the launch plan, the interface, and the source fingerprints the committed measurements are valid for.  The kernel
itself runs in tests/test_gpu_optim_fused.py."""
import json
import os
import re

import pytest
import torch

import diffusion_model_amd as dma
from diffusion_model_amd import _lib
from diffusion_model_amd import optim as dopt
from tests import _optim_cases as cases
from tests._util import dims_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(cases.CONFIGS))
def test_mirror_arithmetic_is_as_accurate_as_the_unfused_fp32_classes(name):
    """Yardstick: the unfused class in float64.  The update Delta = p_K - p_0 of the kernel's arithmetic (numpy mirror, fp32)
    may be at most 2 x as far from it as the same unfused class run in fp32 on the same inputs, at K = 5 and K = 40: both round
    p and the states to fp32 once per step, which dominates; what differs is the order of the operations in between."""
    p0 = cases.init_params()
    for K in (5, cases.K):
        p64, _ = cases.run_unfused(name, K, torch.float64)
        p32, _ = cases.run_unfused(name, K, torch.float32)
        m = cases.MirrorRun(name).run(K)
        e32, em = cases.update_error(p32, p64, p0), cases.update_error(m.p, p64, p0)
        print(f"optimizer update error vs float64, {name}, K = {K}: unfused fp32 {e32:.3e}, kernel arithmetic {em:.3e}, ratio {em / e32:.2f}")
        assert e32 > 0
        assert em <= 2 * e32, (name, K, em, e32)


@pytest.mark.parametrize("kw", [dict(lr=1e-5), dict(lr=2.5e-3, weight_decay=1e-2), dict(lr=1e-3, silent_sgd_phase=False),
                                dict(lr=0.2, r=0.5, weight_lr_power=1.0, betas=(0.95, 0.99))],
                         ids=["ref", "decay", "loud", "weighted"])
def test_radam_scalars_match_the_unfused_class_bit_for_bit(kw):
    """radam_schedule_free_scalars beside RAdamScheduleFree.step on a 1-element parameter for 2,000 steps: the group fields
    (scheduled_lr, lr_max, weight_sum) are equal as doubles, the silent phase gives exact zeros, and c_{k+1} / adaptive_y_lr
    are the expressions of the class on those fields."""
    w = torch.nn.Parameter(torch.ones(1, dtype=torch.float64))
    opt = dma.RAdamScheduleFree([w], **kw)
    opt.train()
    gr = opt.param_groups[0]
    lr_max, weight_sum = gr["lr_max"], gr["weight_sum"]
    beta1 = gr["betas"][0]
    for k in range(2000):
        s = dopt.radam_schedule_free_scalars(k, gr["lr"], gr["betas"], gr["r"], gr["weight_lr_power"], gr["silent_sgd_phase"],
                                             lr_max, weight_sum)
        w.grad = torch.ones(1, dtype=torch.float64)
        opt.step()
        assert gr["k"] == s["step"] == k + 1
        assert (gr["scheduled_lr"], gr["lr_max"], gr["weight_sum"]) == (s["scheduled_lr"], s["lr_max"], s["weight_sum"]), k
        weight = ((k + 1) ** gr["r"]) * (gr["lr_max"] ** gr["weight_lr_power"])
        ckp1 = weight / gr["weight_sum"] if gr["weight_sum"] != 0 else 0.0
        assert s["ckp1"] == ckp1 and s["adaptive_y_lr"] == gr["scheduled_lr"] * (beta1 * (1 - ckp1) - 1), k
        if k < 4 and gr["betas"][1] == 0.999:
            assert not s["rectified"]
            if gr["silent_sgd_phase"]:
                assert s["scheduled_lr"] == 0.0 and s["lr_max"] == 0.0 and s["weight_sum"] == 0.0 and s["ckp1"] == 0.0 and s["adaptive_y_lr"] == 0.0
        if k == 4 and gr["betas"][1] == 0.999:
            assert s["rectified"]                     # step 5 is the first rectified one
        lr_max, weight_sum = s["lr_max"], s["weight_sum"]


def test_adam_scalars_are_torchs():
    """adam_scalars restates the doubles of torch/optim/adam.py's single-tensor step"""
    for step in (1, 2, 5, 40, 1000):
        s = dopt.adam_scalars(step, 1e-5, (0.9, 0.999), 1e-8, 1e-12)
        bc1, bc2 = 1 - 0.9 ** float(step), 1 - 0.999 ** float(step)
        assert s["step_size"] == 1e-5 / bc1 and s["bias_correction2_sqrt"] == bc2 ** 0.5
        assert s["one_minus_beta1"] == 1 - 0.9 and s["one_minus_beta2"] == 1 - 0.999 and s["decay_mul"] == 1 - 1e-5 * 1e-12
    assert set(dopt.adam_scalars(1, 1e-3, (0.9, 0.999), 1e-8, 0.0)) <= {n for n, _ in _lib.OptimConsts._fields_}
    gr = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    sc = dopt.radam_schedule_free_scalars(0, 1e-3, (0.9, 0.999), 0.0, 2.0, True, -1.0, 0.0)
    assert set(dopt.radam_schedule_free_consts(gr, sc)) <= {n for n, _ in _lib.OptimConsts._fields_}


def _production_numels(L, learned):
    d = dims_for(36, 256, 1024, 1024, 1024)
    ps = list(dma.EquivariantGNN(L, **d).parameters()) + list(dma.SpectrumCompressor(200, [150, 100, 50], 32).parameters())
    if learned:
        ps += list(dma.E3DiffusionProcess(1e-5, 2.0, 50, noise_schedule="learned").parameters())
    return [p.numel() for p in ps]


def test_launch_plan_and_capacity():
    C = _lib.lib().egnn_optim_tensors_per_launch()      # pure host: callable without a GPU
    n72, n88, n88g = _production_numels(4, False), _production_numels(5, False), _production_numels(5, True)
    assert len(n72) == 72 and sum(n72) == 7258996 and len(n88) == 88 and len(n88g) > 88
    for numels in (n72, n88, n88g):
        assert len(numels) <= C and len(dopt.plan_launches(numels)) == 1
    assert len(dopt.plan_launches([5] * (C + 3))) == 2 and [len(l) for l in dopt.plan_launches([5] * (C + 3))] == [C, 3]
    assert len(dopt.plan_launches([5] * C)) == 1 and dopt.plan_launches([]) == [] and dopt.plan_launches([0, 0]) == []
    # every element of every tensor belongs to exactly one workgroup, and workgroups are numbered without gaps
    numels = [int(torch.Size(s).numel()) for s in cases.SHAPES]
    (launch,) = dopt.plan_launches(numels)
    assert [i for i, _, _ in launch] == list(range(len(numels)))
    next_wg = 0
    for i, first, nwg in launch:
        assert first == next_wg
        next_wg += nwg
        covered = torch.zeros(numels[i], dtype=torch.int32)
        for w in range(nwg):
            lo = w * dopt.OPTIM_CHUNK
            assert lo < numels[i]                        # no empty workgroup
            covered[lo:min(lo + dopt.OPTIM_CHUNK, numels[i])] += 1
        assert bool((covered == 1).all())
    # the Python plan quotes the kernel's constants
    hdr = open(os.path.join(ROOT, "diffusion_model_amd", "csrc", "optim", "optim_step.h")).read()
    assert int(re.search(r"kOptimCapacity = (\d+);", hdr).group(1)) == C
    threads, quads = (int(re.search(rf"{n} = (\d+);", hdr).group(1)) for n in ("kOptimThreads", "kOptimQuads"))
    assert threads * quads * 4 == dopt.OPTIM_CHUNK


def test_interface():
    hdr = open(os.path.join(ROOT, "include", "egnn_amd.h")).read()
    handle = __import__("ctypes").CDLL(_lib.LIB_PATH)
    for name in ("egnn_optim_step", "egnn_optim_interp", "egnn_optim_tensors_per_launch"):
        assert re.search(rf"^int {name}\(", hdr, flags=re.M) and hasattr(handle, name) and name in _lib.SIGNATURES
    params = dict(lr=1e-5, weight_decay=1e-12, to_compress_spectrum=False, noise_schedule="predefined")
    nn_dict = {"egnn": torch.nn.Linear(3, 3)}
    for kind, cls in (("Adam", torch.optim.Adam), ("AdamW", torch.optim.AdamW), ("RAdamScheduleFree", dma.RAdamScheduleFree)):
        opt = dma.define_optimizer(params, nn_dict, None, kind)          # the default stays the unfused class
        assert type(opt) is cls
        assert type(dma.define_optimizer(dict(params, fused_optimizer=False), nn_dict, None, kind)) is cls
    # the fused classes are selected by the keyword or the params entry -- and refuse CPU parameters: no CPU fallback
    for kind, cls in (("Adam", "FusedAdam"), ("AdamW", "FusedAdamW"), ("RAdamScheduleFree", "FusedRAdamScheduleFree")):
        with pytest.raises(RuntimeError, match=cls + ".*no CPU fallback"):
            dma.define_optimizer(params, nn_dict, None, kind, fused=True)
        with pytest.raises(RuntimeError, match=cls + ".*no CPU fallback"):
            dma.define_optimizer(dict(params, fused_optimizer=True), nn_dict, None, kind)
    assert issubclass(dma.FusedRAdamScheduleFree, dma.RAdamScheduleFree) and issubclass(dma.FusedAdam, torch.optim.Optimizer)
    assert issubclass(dma.FusedAdamW, torch.optim.Optimizer)
    w = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dma.FusedAdam([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    # options the reference never sets
    for cls in (dma.FusedAdam, dma.FusedAdamW):
        for opt in ("maximize", "capturable", "differentiable"):
            with pytest.raises(ValueError, match=opt):
                cls(w, **{opt: True})
        with pytest.raises(ValueError, match="lr"):
            cls(w, lr=torch.tensor(1e-3))
    with pytest.raises(ValueError, match="amsgrad"):
        dma.FusedAdamW(w, amsgrad=False)
    with pytest.raises(ValueError, match="amsgrad"):
        dma.FusedAdam(w, amsgrad=True)


def test_measurement_fingerprints_are_unchanged():
    """the optimizer kernel lives outside the sources the committed traffic / error records fingerprint: bench.py keeps quoting
    them"""
    tj = json.load(open(os.path.join(ROOT, "profiles", "traffic_train.json")))
    assert _lib.training_sources_sha256() == tj["training_sources_sha256"]
    tj = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
    assert _lib.edge_kernel_sources_sha256() == tj["edge_kernel_sources_sha256"]
    head = open(os.path.join(ROOT, "profiles", "r09a_prec_errors.log")).readline()
    assert head.split("forward_sources_sha256=")[-1].split()[0] == _lib.forward_sources_sha256()

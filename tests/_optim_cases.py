"""Shared inputs of the fused-optimizer tests (test infrastructure, not product): parameter shapes, seeded gradients that do
not depend on the parameters (so trajectories do not diverge chaotically), the five optimizer configurations, and the three
ways a trajectory is produced on the CPU: the unfused classes in float64 (the yardstick) and float32, and the numpy mirror of
the kernel driven by the package's scalar functions."""
import math

import numpy as np
import torch

import diffusion_model_amd as dma
from diffusion_model_amd import optim as dopt
from tests import _optim_mirror as mirror

SHAPES = [(1,), (1, 256), (36, 1024), (1024, 73), (1024, 1024), (7,), (4099,), (1024, 292)]
K = 40          # steps 1-4 are RAdam's silent phase at beta2 = 0.999, step 5 is the first rectified one

# name -> (optimizer, constructor arguments)
CONFIGS = {
    "radam_ref": ("RAdamScheduleFree", dict(lr=1e-5)),                                    # the reference's
    "radam_decay": ("RAdamScheduleFree", dict(lr=2.5e-3, weight_decay=1e-2)),
    "radam_loud": ("RAdamScheduleFree", dict(lr=1e-3, silent_sgd_phase=False)),
    "adam": ("Adam", dict(lr=1e-5, weight_decay=1e-12)),                                  # the reference's
    "adamw": ("AdamW", dict(lr=1e-5, weight_decay=1e-12, amsgrad=True)),
}
KINDS = {"Adam": 0, "AdamW": 1, "RAdamScheduleFree": 2}                                   # EGNN_OPTIM_* of include/egnn_amd.h
STATE_KEYS = {"Adam": ("exp_avg", "exp_avg_sq"), "AdamW": ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"),
              "RAdamScheduleFree": ("z", "exp_avg_sq")}


def init_params(shapes=SHAPES, seed=0):
    """uniform +-1/sqrt(fan_in), fp32"""
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand(s, generator=g, dtype=torch.float64) * 2 - 1) / math.sqrt(s[-1])).float() for s in shapes]


def grads(k, shapes=SHAPES):
    """gradient of step k (1-based): randn x 10^((i mod 4) - 3) for tensor i, 5 % of the elements exactly 0, fp32"""
    g = torch.Generator().manual_seed(100 + k)
    out = []
    for i, s in enumerate(shapes):
        v = torch.randn(s, generator=g, dtype=torch.float32) * (10.0 ** ((i % 4) - 3))
        v[torch.rand(s, generator=g) < 0.05] = 0.0
        out.append(v.float())
    return out


def make_unfused(name, params):
    kind, kw = CONFIGS[name]
    if kind == "Adam":
        return torch.optim.Adam(params, foreach=False, **kw)
    if kind == "AdamW":
        return torch.optim.AdamW(params, foreach=False, **kw)
    return dma.RAdamScheduleFree(params, **kw)


def make_fused(name, params):
    kind, kw = CONFIGS[name]
    return {"Adam": dma.FusedAdam, "AdamW": dma.FusedAdamW, "RAdamScheduleFree": dma.FusedRAdamScheduleFree}[kind](params, **kw)


def run_unfused(name, steps, dtype, device="cpu", shapes=SHAPES, first=1, params=None, opt=None):
    """the unfused class of the configuration for ``steps`` steps -> (parameter tensors, optimizer)"""
    if params is None:
        params = [torch.nn.Parameter(p.to(dtype).to(device)) for p in init_params(shapes)]
        opt = make_unfused(name, params)
    if CONFIGS[name][0] == "RAdamScheduleFree":
        opt.train()
    for k in range(first, first + steps):
        for p, g in zip(params, grads(k, shapes)):
            p.grad = g.to(dtype).to(device)
        opt.step()
    return params, opt


class MirrorRun:
    """the numpy fp32 mirror of the kernel over the same inputs; the per-step scalars come from the package's pure functions"""

    def __init__(self, name, shapes=SHAPES):
        self.kind, kw = CONFIGS[name]
        self.shapes = shapes
        self.p = [p.numpy().copy() for p in init_params(shapes)]
        n_states = len(STATE_KEYS[self.kind])
        self.s = [[np.zeros(s, np.float32) for s in shapes] for _ in range(n_states)]
        if self.kind == "RAdamScheduleFree":
            self.s[0] = [p.copy() for p in self.p]
            self.group = dict(lr=0.0025, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, r=0.0, weight_lr_power=2.0,
                              silent_sgd_phase=True, k=0, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0)
        else:
            self.group = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
            self.steps = [0] * len(shapes)
        self.group.update({k: v for k, v in kw.items() if k != "amsgrad"})

    def step(self, gs, skip=()):
        """one step; tensors in ``skip`` have no gradient (torch's Adam counts steps per tensor, RAdamScheduleFree per group)"""
        gr = self.group
        if self.kind == "RAdamScheduleFree":
            s = dopt.radam_schedule_free_scalars(gr["k"], gr["lr"], gr["betas"], gr["r"], gr["weight_lr_power"], gr["silent_sgd_phase"],
                                                 gr["lr_max"], gr["weight_sum"])
            gr["scheduled_lr"], gr["lr_max"], gr["weight_sum"] = s["scheduled_lr"], s["lr_max"], s["weight_sum"]
            gr["k"] += 1
            per_tensor = [dopt.radam_schedule_free_consts(gr, s)] * len(self.p)
        else:
            self.steps = [n + (i not in skip) for i, n in enumerate(self.steps)]
            per_tensor = [dopt.adam_scalars(n, gr["lr"], gr["betas"], gr["eps"], gr["weight_decay"]) for n in self.steps]
        self.last_consts = per_tensor[0]     # the step's constants where no tensor was ever skipped
        for i in range(len(self.p)):
            if i in skip:
                continue
            states = [st[i] for st in self.s] + [None] * (3 - len(self.s))
            mirror.step(KINDS[self.kind], per_tensor[i], self.p[i], gs[i].numpy(), *states)

    def run(self, steps, first=1):
        for k in range(first, first + steps):
            self.step(grads(k, self.shapes))
        return self


def update_error(p_end, p_ref_end, p0):
    """|| (p_K - p_0) - (p_K - p_0)_64 ||_2 / || (p_K - p_0)_64 ||_2 over the concatenation of all tensors, in float64"""
    cat = lambda ts: torch.cat([torch.as_tensor(np.asarray(t.detach().cpu()) if torch.is_tensor(t) else t).double().reshape(-1) for t in ts])
    d, d64 = cat(p_end) - cat(p0), cat(p_ref_end) - cat(p0)
    return float((d - d64).norm() / d64.norm())

"""Optimizers of the reference's define_optimizer (parts/def_for_main.py:119-139): Adam, AdamW(amsgrad) from
torch, and RAdamScheduleFree.

RAdamScheduleFree comes from the third-party package ``schedulefree`` (un-pinned in the reference, absent
offline).  It is restated here from the published algorithm (Defazio et al., "The Road Less Scheduled",
2024, schedule-free wrapper of RAdam: interpolation y = (1 - beta1) z + beta1 x, Polyak-style averaging
weights c_{k+1} = lr_max^p / sum, RAdam rectification of the step size with a silent SGD phase).
PARITY UNPINNED: neither the package nor any fixture of it is available; the tests check the algebraic
properties only (train/eval round trip, equivalence with plain SGD-free averaging identities, convergence).

FusedAdam, FusedAdamW and FusedRAdamScheduleFree (second half of this file) are the same three optimizers with the step as
one multi-tensor HIP launch; ``define_optimizer(..., fused=True)`` selects them.
"""
from __future__ import annotations

import torch

from . import _lib


class RAdamScheduleFree(torch.optim.Optimizer):
    def __init__(self, params, lr=0.0025, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, r=0.0,
                 weight_lr_power=2.0, silent_sgd_phase=True):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, r=r, weight_lr_power=weight_lr_power,
                        silent_sgd_phase=silent_sgd_phase, k=0, train_mode=False, weight_sum=0.0, lr_max=-1.0,
                        scheduled_lr=0.0)
        super().__init__(params, defaults)

    @torch.no_grad()
    def eval(self):
        """parameters hold y while training; switch them to the averaged iterate x (train_per_iretation.py:189-190)"""
        for group in self.param_groups:
            if group["train_mode"]:
                beta1, _ = group["betas"]
                for p in group["params"]:
                    st = self.state[p]
                    if "z" in st:
                        p.lerp_(end=st["z"].to(p.device), weight=1 - 1 / beta1)   # y -> x
                group["train_mode"] = False

    @torch.no_grad()
    def train(self):
        """x -> y (train_per_iretation.py:103-104)"""
        for group in self.param_groups:
            if not group["train_mode"]:
                beta1, _ = group["betas"]
                for p in group["params"]:
                    st = self.state[p]
                    if "z" in st:
                        p.lerp_(end=st["z"].to(p.device), weight=1 - beta1)       # x -> y
                group["train_mode"] = True

    @torch.no_grad()
    def step(self, closure=None):
        if not self.param_groups[0]["train_mode"]:
            raise RuntimeError("RAdamScheduleFree.step() called in eval mode: call optimizer.train() first")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            eps, (beta1, beta2), decay = group["eps"], group["betas"], group["weight_decay"]
            step = group["k"] + 1
            beta2_t = beta2 ** step
            bias_correction2 = 1 - beta2_t
            rho_inf = 2 / (1 - beta2) - 1                         # maximum length of the approximated SMA
            rho_t = rho_inf - 2 * step * beta2_t / bias_correction2
            if rho_t > 4.0:
                rect = ((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) ** 0.5
            else:
                rect = float(not group["silent_sgd_phase"])
            lr = group["scheduled_lr"] = group["lr"] * rect
            group["lr_max"] = lr_max = max(lr, group["lr_max"])
            weight = (step ** group["r"]) * (lr_max ** group["weight_lr_power"])
            weight_sum = group["weight_sum"] = group["weight_sum"] + weight
            ckp1 = weight / weight_sum if weight_sum != 0 else 0.0
            adaptive_y_lr = lr * (beta1 * (1 - ckp1) - 1)
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if "z" not in st:
                    st["z"] = p.detach().clone(memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                z, v = st["z"], st["exp_avg_sq"]
                g = p.grad
                v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
                if rho_t > 4.0:
                    gn = g / v.div(bias_correction2).sqrt_().add_(eps)
                else:
                    gn = g.clone()
                if decay != 0:
                    gn.add_(p, alpha=decay)                         # decay at y
                p.lerp_(end=z, weight=ckp1)                         # y <- (1 - c) y + c z
                p.add_(gn, alpha=adaptive_y_lr)
                z.sub_(gn, alpha=lr)                                # z <- z - lr * g
            group["k"] = step
        return loss


# ---------------------------------------------------------------------------------------------------------------------
# Fused forms: the same three optimizers as ONE multi-tensor HIP launch per step and parameter group
# (csrc/optim/optim_step.hip behind egnn_optim_step / egnn_optim_interp).  The kernel holds no step-count logic: the
# per-step scalars are computed here, in double, by the pure functions below (no tensors, no GPU), exactly as
# RAdamScheduleFree.step above and torch's single-tensor Adam compute them, and are rounded to fp32 once.

def radam_schedule_free_scalars(k, lr, betas, r, weight_lr_power, silent_sgd_phase, lr_max, weight_sum):
    """Scalars of step k + 1 of RAdamScheduleFree (the group loop's head above, same expressions in the same order): the new
    group fields ``scheduled_lr``, ``lr_max``, ``weight_sum`` and the step's ``ckp1``, ``adaptive_y_lr``,
    ``bias_correction2``, ``rectified`` (rho_t > 4)."""
    beta1, beta2 = betas
    step = k + 1
    beta2_t = beta2 ** step
    bias_correction2 = 1 - beta2_t
    rho_inf = 2 / (1 - beta2) - 1
    rho_t = rho_inf - 2 * step * beta2_t / bias_correction2
    rectified = rho_t > 4.0
    if rectified:
        rect = ((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) ** 0.5
    else:
        rect = float(not silent_sgd_phase)
    scheduled_lr = lr * rect
    lr_max = max(scheduled_lr, lr_max)
    weight = (step ** r) * (lr_max ** weight_lr_power)
    weight_sum = weight_sum + weight
    ckp1 = weight / weight_sum if weight_sum != 0 else 0.0
    adaptive_y_lr = scheduled_lr * (beta1 * (1 - ckp1) - 1)
    return dict(step=step, rectified=rectified, bias_correction2=bias_correction2, scheduled_lr=scheduled_lr, lr_max=lr_max,
                weight_sum=weight_sum, ckp1=ckp1, adaptive_y_lr=adaptive_y_lr)


def radam_schedule_free_consts(group, scalars):
    """the fields of egnn_optim_consts for one RAdamScheduleFree step (doubles; the binding rounds them to fp32)"""
    beta2 = group["betas"][1]
    return dict(beta2=beta2, one_minus_beta2=1 - beta2, eps=group["eps"], weight_decay=group["weight_decay"],
                bias_correction2=scalars["bias_correction2"], ckp1=scalars["ckp1"], adaptive_y_lr=scalars["adaptive_y_lr"],
                lr=scalars["scheduled_lr"], rectified=int(scalars["rectified"]))


def adam_scalars(step, lr, betas, eps, weight_decay):
    """the fields of egnn_optim_consts for step ``step`` of torch.optim.Adam / AdamW (torch/optim/adam.py, _single_tensor_adam:
    bias corrections, step size and the square root in Python doubles)"""
    beta1, beta2 = betas
    step = float(step)
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return dict(beta2=beta2, one_minus_beta2=1 - beta2, eps=eps, weight_decay=weight_decay, one_minus_beta1=1 - beta1,
                bias_correction2_sqrt=bias_correction2 ** 0.5, step_size=lr / bias_correction1, decay_mul=1 - lr * weight_decay)


OPTIM_CHUNK = 2048   # elements of one tensor per workgroup (csrc/optim/optim_step.h: kOptimChunk)


def plan_launches(numels, capacity=None):
    """How a list of tensors with flat (equally spaced) states is cut into launches, as egnn_optim_step cuts it: at most
    ``capacity`` tensors per launch, one workgroup per OPTIM_CHUNK elements of ONE tensor.  -> list of launches, each a list of
    (tensor index, first workgroup, number of workgroups); tensors without elements take no workgroup."""
    if capacity is None:
        capacity = _lib.lib().egnn_optim_tensors_per_launch()
    launches, cur, chunks = [], [], 0
    for i, n in enumerate(numels):
        if n == 0:
            continue
        if len(cur) == capacity:
            launches.append(cur)
            cur, chunks = [], 0
        nwg = (n + OPTIM_CHUNK - 1) // OPTIM_CHUNK
        cur.append((i, chunks, nwg))
        chunks += nwg
    if cur:
        launches.append(cur)
    return launches


class _FusedStates:
    """What the three fused optimizers share: parameter checks, the flat state buffers and the launch.

    The states of a parameter group live in one flat fp32 buffer per state kind, every tensor's slice starting at a multiple
    of 4 elements and at the SAME offset in each buffer; ``state[p][key]`` is a view of the slice.  Equal spacing is what
    lets a launch carry 112 tensors in its arguments (csrc/optim/optim_step.h), so the production lists are one launch."""
    _STATE_KEYS = ()    # flat per-parameter states in the kernel's s0, s1, s2 order
    _KIND = None

    def _reject_options(self, **opts):
        for name, value in opts.items():
            if value:
                raise ValueError(f"{type(self).__name__}: {name}={value!r} is not supported by the fused HIP step")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        if isinstance(group["lr"], torch.Tensor):
            raise ValueError(f"{type(self).__name__}: a tensor lr is not supported by the fused HIP step")
        for p in group["params"]:
            if not (p.is_cuda and p.dtype == torch.float32 and p.layout == torch.strided and p.is_contiguous()):
                raise RuntimeError(f"{type(self).__name__} steps contiguous fp32 parameters on a ROCm device with a HIP kernel; got "
                                   f"{p.dtype} {tuple(p.shape)} on {p.device}.  There is no CPU fallback.")
        self._flat = {}

    def __setstate__(self, state):
        super().__setstate__(state)
        self._flat = {}    # loaded states are standalone tensors: adopted into flat buffers at the next launch

    def state_dict(self):
        """as the unfused classes', but every tensor leaves as a copy of its own: a saved view would drag the whole flat buffer
        along, and an optimizer that loads the dict (torch keeps loaded tensors that already fit) must not share them"""
        sd = super().state_dict()
        sd["state"] = {k: {n: (v.clone() if torch.is_tensor(v) else v) for n, v in st.items()} for k, st in sd["state"].items()}
        return sd

    def _init_state(self, p, st, views):
        raise NotImplementedError

    def _group_flat(self, gi, group):
        fl = self._flat.get(gi)
        if fl is not None:
            return fl
        import ctypes as C
        params = group["params"]
        dev = params[0].device
        if any(p.device != dev for p in params):
            raise RuntimeError(f"{type(self).__name__}: the parameters of one group must live on one device")
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4
        bufs = [torch.zeros(total, dtype=torch.float32, device=dev) for _ in self._STATE_KEYS]
        views = [[b[o:o + p.numel()].view_as(p) for b in bufs] for p, o in zip(params, offs)]
        ready = [False] * len(params)
        for i, p in enumerate(params):   # states that exist already (load_state_dict, a re-made group list) move into the buffers
            st = self.state.get(p)
            if st and all(k in st for k in self._STATE_KEYS):
                for k, v in zip(self._STATE_KEYS, views[i]):
                    v.copy_(st[k])
                    st[k] = v
                ready[i] = True
        n = len(params)
        PtrArr = C.c_void_p * n
        fl = dict(bufs=bufs, views=views, ready=ready, n_ready=sum(ready), PtrArr=PtrArr, device=dev,
                  numel=(C.c_int64 * n)(*[p.numel() for p in params]),
                  states=[PtrArr(*[v[j].data_ptr() for v in views]) for j in range(len(bufs))])
        self._flat[gi] = fl
        return fl

    def _grads(self, group, fl):
        """gradient pointers of the group (0 where p.grad is None), after creating the states of parameters seen for the first
        time"""
        ptrs = []
        for i, p in enumerate(group["params"]):
            g = p.grad
            if g is None:
                ptrs.append(None)
                continue
            if not (g.is_cuda and g.dtype == torch.float32 and g.layout == torch.strided and g.is_contiguous() and g.device == p.device):
                raise RuntimeError(f"{type(self).__name__}: the gradient of a {tuple(p.shape)} parameter is {g.dtype} / {g.layout} on "
                                   f"{g.device}, contiguous={g.is_contiguous()}; the fused step takes dense contiguous fp32 gradients "
                                   "on the parameter's device.  There is no CPU fallback.")
            if not fl["ready"][i]:
                st = self.state[p]
                self._init_state(p, st, fl["views"][i])
                for k, v in zip(self._STATE_KEYS, fl["views"][i]):
                    st[k] = v
                fl["ready"][i] = True
                fl["n_ready"] += 1
            ptrs.append(g.data_ptr())
        return ptrs

    def _launch(self, group, fl, grad_ptrs, consts):
        L = _lib.lib()
        c = _lib.OptimConsts(**consts)
        PtrArr = fl["PtrArr"]
        s = fl["states"] + [None] * (3 - len(fl["states"]))
        _lib.check(L.egnn_optim_step(torch.cuda.current_stream(fl["device"]).cuda_stream, self._KIND, len(grad_ptrs),
                                     PtrArr(*[p.data_ptr() for p in group["params"]]), PtrArr(*grad_ptrs), s[0], s[1], s[2],
                                     fl["numel"], c))


class FusedRAdamScheduleFree(_FusedStates, RAdamScheduleFree):
    """RAdamScheduleFree with ``step()`` as one HIP launch per parameter group and ``train()`` / ``eval()`` as one launch
    each; same constructor, group fields and state_dict as the class above (states ``z``, ``exp_avg_sq``), so the two load each
    other's state_dict in either direction."""
    _STATE_KEYS = ("z", "exp_avg_sq")
    _KIND = _lib.OPTIM_RADAM_SF

    def __init__(self, params, lr=0.0025, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, r=0.0, weight_lr_power=2.0,
                 silent_sgd_phase=True):
        self._flat = {}
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, r=r, weight_lr_power=weight_lr_power,
                         silent_sgd_phase=silent_sgd_phase)

    def _init_state(self, p, st, views):
        views[0].copy_(p.detach())     # z = y at creation; exp_avg_sq: the buffer's zeros

    @torch.no_grad()
    def _switch(self, to_train):
        import ctypes as C
        for gi, group in enumerate(self.param_groups):
            if group["train_mode"] == to_train:
                continue
            beta1, _ = group["betas"]
            weight = 1 - beta1 if to_train else 1 - 1 / beta1          # x -> y / y -> x
            ps = [p for p in group["params"] if "z" in self.state.get(p, ())]
            if ps:
                self._group_flat(gi, group)
                PtrArr = C.c_void_p * len(ps)
                _lib.check(_lib.lib().egnn_optim_interp(torch.cuda.current_stream(ps[0].device).cuda_stream, len(ps),
                                                        PtrArr(*[p.data_ptr() for p in ps]),
                                                        PtrArr(*[self.state[p]["z"].data_ptr() for p in ps]),
                                                        (C.c_int64 * len(ps))(*[p.numel() for p in ps]), weight))
            group["train_mode"] = to_train

    def eval(self):
        self._switch(False)

    def train(self):
        self._switch(True)

    @torch.no_grad()
    def step(self, closure=None):
        if not self.param_groups[0]["train_mode"]:
            raise RuntimeError("RAdamScheduleFree.step() called in eval mode: call optimizer.train() first")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            s = radam_schedule_free_scalars(group["k"], group["lr"], group["betas"], group["r"], group["weight_lr_power"],
                                            group["silent_sgd_phase"], group["lr_max"], group["weight_sum"])
            group["scheduled_lr"], group["lr_max"], group["weight_sum"] = s["scheduled_lr"], s["lr_max"], s["weight_sum"]
            fl = self._group_flat(gi, group)
            self._launch(group, fl, self._grads(group, fl), radam_schedule_free_consts(group, s))
            group["k"] = s["step"]
        return loss


class _FusedAdamStep(_FusedStates):
    """step() of FusedAdam / FusedAdamW: torch's single-tensor Adam (torch/optim/adam.py) as one launch per group.  ``step`` stays
    a per-parameter CPU scalar tensor as in torch; parameters of one group whose counts differ (a gradient was None for some
    steps) take one launch per distinct count."""

    def _init_state(self, p, st, views):
        st["step"] = torch.tensor(0.0, dtype=torch.float32)

    def _check_group(self, group):
        self._reject_options(maximize=group.get("maximize"), capturable=group.get("capturable"),
                             differentiable=group.get("differentiable"), fused=group.get("fused"))

    def _check_ctor(self, lr, kw):
        """options the reference never sets, refused before anything else is looked at"""
        self._reject_options(**{k: kw.get(k) for k in ("maximize", "capturable", "differentiable", "fused")})
        if isinstance(lr, torch.Tensor):
            raise ValueError(f"{type(self).__name__}: a tensor lr is not supported by the fused HIP step")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])

    def _group_flat(self, gi, group):
        if gi in self._flat:
            return self._flat[gi]
        fl = super()._group_flat(gi, group)
        for i, p in enumerate(group["params"]):     # a loaded step count lives on the host, as torch keeps it
            if fl["ready"][i]:
                st = self.state[p]
                st["step"] = torch.as_tensor(st.get("step", 0.0), dtype=torch.float32).reshape(()).cpu().clone()   # never shared
        # host copy of the counts (the tensors are advanced with one foreach add per step, not read back one by one)
        fl["steps"] = [float(self.state[p]["step"]) if fl["ready"][i] else 0.0 for i, p in enumerate(group["params"])]
        return fl

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
            fl = self._group_flat(gi, group)
            grad_ptrs = self._grads(group, fl)
            steps, params = fl["steps"], group["params"]
            ids = [i for i, g in enumerate(grad_ptrs) if g is not None]
            if not ids:
                continue
            torch._foreach_add_([self.state[params[i]]["step"] for i in ids], 1.0)
            by_step = {}
            for i in ids:
                steps[i] += 1.0
                by_step.setdefault(steps[i], []).append(i)
            for step, members in by_step.items():
                ptrs = grad_ptrs
                if len(by_step) > 1:
                    keep = set(members)
                    ptrs = [g if i in keep else None for i, g in enumerate(grad_ptrs)]
                self._launch(group, fl, ptrs, adam_scalars(step, group["lr"], group["betas"], group["eps"], group["weight_decay"]))
        return loss


class FusedAdam(_FusedAdamStep, torch.optim.Adam):
    """torch.optim.Adam (L2 weight decay, no amsgrad) with ``step()`` as one HIP launch per parameter group; same constructor
    arguments, group keys and state_dict (``step``, ``exp_avg``, ``exp_avg_sq``)."""
    _STATE_KEYS = ("exp_avg", "exp_avg_sq")
    _KIND = _lib.OPTIM_ADAM

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, **kw):
        self._flat = {}
        self._reject_options(amsgrad=amsgrad)
        self._check_ctor(lr, kw)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, **kw)

    def _check_group(self, group):
        super()._check_group(group)
        self._reject_options(amsgrad=group.get("amsgrad"), decoupled_weight_decay=group.get("decoupled_weight_decay"))


class FusedAdamW(_FusedAdamStep, torch.optim.AdamW):
    """torch.optim.AdamW(amsgrad=True) -- the only AdamW define_optimizer constructs -- with ``step()`` as one HIP launch per
    parameter group; state_dict keys ``step``, ``exp_avg``, ``exp_avg_sq``, ``max_exp_avg_sq``.  ``amsgrad`` defaults to True
    here and anything else raises."""
    _STATE_KEYS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")
    _KIND = _lib.OPTIM_ADAMW_AMSGRAD

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=True, **kw):
        self._flat = {}
        if not amsgrad:
            raise ValueError("FusedAdamW: only amsgrad=True has a fused HIP step (the form define_optimizer constructs)")
        self._check_ctor(lr, kw)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=True, **kw)

    def _check_group(self, group):
        super()._check_group(group)
        if not group.get("amsgrad"):
            raise ValueError("FusedAdamW: only amsgrad=True has a fused HIP step (the form define_optimizer constructs)")


def define_optimizer(params, nn_dict, diffusion_process, optim_type: str, fused=None):
    """define_optimizer(params, nn_dict, diffusion_process, optim_type) of parts/def_for_main.py:119-139.  ``fused=True`` (or
    ``params["fused_optimizer"]``) selects the HIP forms of the same three optimizers; the default is torch's / the restated
    class, as in the reference."""
    assert optim_type in ["Adam", "AdamW", "RAdamScheduleFree"]
    if fused is None:
        fused = bool(params.get("fused_optimizer", False))
    lr, weight_decay = params["lr"], params["weight_decay"]
    plist = list(nn_dict["egnn"].parameters())
    if params["to_compress_spectrum"]:
        plist += list(nn_dict["spectrum_compressor"].parameters())
    if params["noise_schedule"] == "learned":
        plist += list(diffusion_process.parameters())
    if optim_type == "Adam":
        return (FusedAdam if fused else torch.optim.Adam)(plist, lr=lr, weight_decay=weight_decay)
    if optim_type == "AdamW":
        return (FusedAdamW if fused else torch.optim.AdamW)(plist, lr=lr, weight_decay=weight_decay, amsgrad=True)
    return (FusedRAdamScheduleFree if fused else RAdamScheduleFree)(plist, lr=lr)

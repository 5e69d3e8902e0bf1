"""numpy fp32 mirror of csrc/optim/optim_step.hip (test infrastructure, not product): the kernel's exact operation order, ONE
IEEE fp32 operation per line, on whole arrays.  numpy, not torch: numpy's float32 sqrt and division are the correctly rounded
SSE ones (tests/test_cabi_and_host.py records that torch's vectorised CPU sqrt is not always).  There is no indexing logic
here, so this file cannot share a tail or alignment mistake with the kernel."""
import numpy as np

ADAM, ADAMW_AMSGRAD, RADAM_SF = 0, 1, 2
f32 = np.float32


def step(kind, consts, p, g, s0, s1, s2=None):
    """one step on fp32 arrays, in place (p, s0, s1, s2); ``consts``: egnn_optim_consts fields as doubles, rounded to fp32 here
    as the ctypes binding rounds them"""
    k = {n: f32(v) for n, v in consts.items() if n != "rectified"}
    assert all(a is None or a.dtype == np.float32 for a in (p, g, s0, s1, s2))
    if kind == RADAM_SF:
        a, b = s0, s1                               # z, exp_avg_sq
        t = g * g
        t = t * k["one_minus_beta2"]
        b[...] = b * k["beta2"]
        b[...] = b + t
        gn = g
        if consts["rectified"]:
            d = b / k["bias_correction2"]
            d = np.sqrt(d)
            d = d + k["eps"]
            gn = g / d
        if k["weight_decay"] != 0:
            w = k["weight_decay"] * p
            gn = gn + w
        d = a - p
        d = k["ckp1"] * d
        p[...] = p + d
        u = k["adaptive_y_lr"] * gn
        p[...] = p + u
        u = k["lr"] * gn
        a[...] = a - u
        return
    a, b, c = s0, s1, s2                            # exp_avg, exp_avg_sq, max_exp_avg_sq
    if kind == ADAMW_AMSGRAD:
        p[...] = p * k["decay_mul"]
    elif k["weight_decay"] != 0:
        w = k["weight_decay"] * p
        g = g + w
    d = g - a
    d = k["one_minus_beta1"] * d
    a[...] = a + d
    t = g * g
    t = t * k["one_minus_beta2"]
    b[...] = b * k["beta2"]
    b[...] = b + t
    if kind == ADAMW_AMSGRAD:
        c[...] = np.maximum(c, b)
        d = np.sqrt(c)
    else:
        d = np.sqrt(b)
    d = d / k["bias_correction2_sqrt"]
    d = d + k["eps"]
    q = a / d
    q = k["step_size"] * q
    p[...] = p - q


def interp(p, z, weight):
    """p <- p + weight (z - p), in place"""
    d = z - p
    d = f32(weight) * d
    p[...] = p + d

"""fp64 statement of one ``torch.optim.SGD`` step as ``bpx_sgd_step`` computes it (csrc/optim.hip: torch's ``_multi_tensor_sgd``, every scalar rounded
to float once as a foreach op rounds its ``alpha``), and the per-element bound on an fp32 evaluation of that statement.  Pure numpy / torch on the CPU.

    d = g + wd p                  (wd != 0)
    b' = b mom + (1 - dampening) d         (momentum != 0; the first step of a fresh torch optimizer: b' = d)
    u = d + mom b'  (nesterov)    u = b'  (momentum)    u = d  (no momentum)
    p' = p + (-lr) u

The bound, in the manner of tests/loss_bounds.py: every fp32 operation rounds once, by at most u = 2^-24 relative to the magnitude of its result; a
product and a sum are TWO operations (whether or not a compiler contracts them: a contraction only drops a rounding); the inputs p, g, b are fp32
values as stored and carry no error.  The error of every stage is pushed through the next on absolute values:

    e_d  = u (|wd p| + |d|)
    e_b' = u |b mom| + (omd e_d + u |omd d|) + u |b'|                      (first step: e_b' = e_d, a copy)
    e_u  = e_d + (mom e_b' + u |mom b'|) + u |u|   (nesterov)      e_b' (momentum)      e_d (none)
    e_p' = (lr e_u + u |lr u|) + u |p'|

evaluated at the fp64 magnitudes.  The fp32 magnitudes differ from those by the errors themselves, i.e. by terms of order u times the bound; SAFETY
= 1.25 covers them with room (nothing here is fitted to a measured value), and FLOOR = 2^-126 covers results in the denormal range.
"""
from __future__ import annotations

import numpy as np
import torch

U32 = 2.0 ** -24
SAFETY = 1.25
FLOOR = 2.0 ** -126


def f32(v) -> float:
    """The double that equals float32(v): what the kernel (and a foreach op on fp32 tensors) makes of a host double."""
    return float(np.float32(v))


def _scalars(lr, momentum, dampening, wd):
    return f32(lr), f32(momentum), f32(1.0 - float(dampening)), f32(wd)


def _d(t):
    return None if t is None else t.detach().cpu().double()


def sgd_reference(p, g, buf, lr, momentum, dampening, wd, nesterov, first):
    """(p', b') of one step in float64 on the operands as stored; b' is None without momentum.  ``first``: torch's first step of a fresh
    optimizer, which seeds the buffer with d (``buf`` is not read)."""
    lr, mom, omd, wd = _scalars(lr, momentum, dampening, wd)
    p, g, buf = _d(p), _d(g), _d(buf)
    d = g + wd * p if wd != 0 else g
    nb = None
    if momentum != 0:
        nb = d.clone() if first else buf * mom + omd * d
        u = d + mom * nb if nesterov else nb
    else:
        u = d
    return p + (-lr) * u, nb


def sgd_bound(p, g, buf, lr, momentum, dampening, wd, nesterov, first):
    """(bound on |p' - reference|, bound on |b' - reference| or None): see the module docstring."""
    lr, mom, omd, wd = _scalars(lr, momentum, dampening, wd)
    p, g, buf = _d(p), _d(g), _d(buf)
    u = U32
    if wd != 0:
        d = g + wd * p
        e_d = u * ((wd * p).abs() + d.abs())
    else:
        d, e_d = g, torch.zeros_like(g)
    e_b = None
    if momentum != 0:
        if first:
            nb, e_b = d, e_d
        else:
            nb = buf * mom + omd * d
            e_b = u * (buf * mom).abs() + (omd * e_d + u * (omd * d).abs()) + u * nb.abs()
        if nesterov:
            uu = d + mom * nb
            e_u = e_d + (mom * e_b + u * (mom * nb).abs()) + u * uu.abs()
        else:
            uu, e_u = nb, e_b
    else:
        uu, e_u = d, e_d
    pn = p + (-lr) * uu
    e_p = (lr * e_u + u * (lr * uu).abs()) + u * pn.abs()
    return SAFETY * e_p + FLOOR, None if e_b is None else SAFETY * e_b + FLOOR


def worst_ratio(got, ref, bound) -> float:
    """max over the elements of |got - ref| / bound (a NaN anywhere gives inf)."""
    r = ((got.detach().cpu().double() - ref).abs() / bound)
    return float("inf") if torch.isnan(r).any() else float(r.max())


# lr, momentum, dampening, weight decay, nesterov - the five configurations of the issue; dampening is the double whose 1 - dampening is float32(0.9)
# exactly (0.1 to 2.4e-8), so that torch's float64 step and the float-rounded statement use the same numbers
DAMP = 1.0 - f32(0.9)
CONFIGS = {
    "plain": dict(lr=f32(0.05), momentum=0.0, dampening=0.0, wd=0.0, nesterov=False),
    "wd": dict(lr=f32(0.05), momentum=0.0, dampening=0.0, wd=f32(1e-2), nesterov=False),
    "momentum": dict(lr=f32(0.05), momentum=f32(0.9), dampening=0.0, wd=0.0, nesterov=False),
    "nesterov_wd": dict(lr=f32(0.05), momentum=f32(0.9), dampening=0.0, wd=f32(1e-2), nesterov=True),
    "dampening": dict(lr=f32(0.05), momentum=f32(0.9), dampening=DAMP, wd=0.0, nesterov=False),
}


def torch_sgd(params, cfg, **kw):
    return torch.optim.SGD(params, lr=cfg["lr"], momentum=cfg["momentum"], dampening=cfg["dampening"], weight_decay=cfg["wd"],
                           nesterov=cfg["nesterov"], **kw)

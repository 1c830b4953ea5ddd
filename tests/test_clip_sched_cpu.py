"""Gradient clipping and per-step schedules on the graphed train step - what can be checked without a GPU: the fp64 statement the device tests measure
against (optim_bounds.clip_reference) is torch's clip_grad_norm_, the device copy of beta1 follows the host double exactly, and the new keywords of
optim.fused_step / optim.step decline host tensors and fall through to torch's own clip + step."""
import math
import os
import re

import numpy as np
import pytest
import torch
from torch.nn.utils import clip_grad_norm_

import optim_bounds as OB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(16,), (1,), (5, 7), (16, 1, 3, 3, 3), (300,)]        # at most 432 elements per tensor


def _params(grads):
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    return ps


# torch's CPU clip_grad_norm_ works in float32 throughout: a norm per tensor (n <= 432 squares summed in float32: relative error <= n 2^-24 = 2.6e-5
# in the worst case), the norm of those, `norm + 1e-6`, a reciprocal and a product - a handful of roundings of 2^-24 each on top.  The fp64 statement
# has one rounding.  3e-5 relative covers the two; the clipped gradients inherit the coefficient's error plus their own product's rounding.
TORCH_F32 = 3e-5


@pytest.mark.parametrize("scale", [0.25, 4.0], ids=["clips", "inactive"])
def test_fp64_statement_is_torchs_clip_grad_norm(scale):
    grads, _ = OB.make_grads(SIZES, seed=3)
    true_norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    max_norm = scale * true_norm
    norm, coef, clipped = OB.clip_reference(grads, max_norm)
    ps = _params(grads)
    total = clip_grad_norm_(ps, max_norm=max_norm)
    assert abs(float(total) - float(norm)) <= TORCH_F32 * float(norm)
    if scale > 1:                                         # inactive: the coefficient is exactly 1 and nothing moves, on both sides
        assert coef == np.float32(1.0)
        for p, g, c in zip(ps, grads, clipped):
            assert torch.equal(p.grad, g) and torch.equal(c, g)
    else:
        assert abs(float(coef) - scale) <= 2 * TORCH_F32 * scale
        for p, c in zip(ps, clipped):
            assert (p.grad - c).abs().max().item() <= 2 * TORCH_F32 * c.abs().max().item()


def test_fp64_statement_zero_and_nan_gradients():
    zeros = [torch.zeros(s) for s in SIZES]
    norm, coef, clipped = OB.clip_reference(zeros, 0.5)
    ps = _params(zeros)
    total = clip_grad_norm_(ps, max_norm=0.5)
    assert float(norm) == 0.0 == float(total) and coef == np.float32(1.0)         # 0.5 / 1e-6 clamps to 1
    assert all(torch.equal(p.grad, z) and torch.equal(c, z) for p, z, c in zip(ps, zeros, clipped))
    grads, _ = OB.make_grads(SIZES, seed=4)
    grads = [g.clone() for g in grads]
    grads[3].view(-1)[17] = float("nan")
    norm, coef, clipped = OB.clip_reference(grads, 0.5)
    ps = _params(grads)
    total = clip_grad_norm_(ps, max_norm=0.5)                                        # error_if_nonfinite=False: NaN everywhere, no exception
    assert math.isnan(float(total)) and np.isnan(norm) and np.isnan(coef)
    assert all(torch.isnan(p.grad).all() and torch.isnan(c).all() for p, c in zip(ps, clipped))
    assert OB.ulps(np.float32("nan"), np.float32("nan")) == 0 and OB.ulps(1.0, np.nextafter(np.float32(1.0), np.float32(2.0))) == 1
    assert OB.ulps(np.float32(-0.0), np.float32(0.0)) == 0 and OB.ulps(1.0, float("nan")) > 1


def test_lr_tensors_sync_carries_beta1_as_a_double():
    """graphs._LrTensors: the 0-d float64 copy of beta1 equals the host double OneCycleLR assigned, bit for bit; group['betas'] stays Python floats;
    an unchanged beta1 launches nothing (the flag stays down)."""
    from biapy_amd.graphs import _LrTensors

    values = OB.onecycle_beta1(steps=10)
    assert len(values) == 10 and len(set(values)) > 5 and values[0] == 0.95
    assert any(float(np.float32(v)) != v for v in values)                           # a float32 copy would not do
    p = [torch.nn.Parameter(torch.zeros(3))]
    opt = torch.optim.AdamW(p, lr=1e-3, betas=(values[0], 0.999))
    lt = _LrTensors(opt, "cpu")
    (b1,) = lt.beta1s
    assert b1.dtype == torch.float64 and b1.dim() == 0 and b1.item() == values[0]
    lt.sync()
    assert lt.beta1_moved is False
    for v in values[1:]:
        opt.param_groups[0]["betas"] = (v, *opt.param_groups[0]["betas"][1:])        # what OneCycleLR.get_lr does
        before = b1.data_ptr()
        lt.sync()
        assert b1.item() == v and b1.data_ptr() == before and lt.beta1s[0] is b1
        assert all(type(b) is float for b in opt.param_groups[0]["betas"])
    assert lt.beta1_moved is True
    assert opt.param_groups[0]["lr"] is lt.lrs[0]
    sgd = torch.optim.SGD(p, lr=0.1)                                                  # no betas: nothing to carry
    assert _LrTensors(sgd, "cpu").beta1s == [None]


def test_new_keywords_decline_host_tensors_and_fall_through_to_torch():
    from biapy_amd import optim as O

    def make():
        gen = torch.Generator().manual_seed(7)
        ps = [torch.nn.Parameter(torch.randn(*s, generator=gen)) for s in SIZES]
        return ps, torch.optim.AdamW(ps, lr=1e-2, weight_decay=1e-2)

    (pa, oa), (pb, ob) = make(), make()
    c = 0.5
    for it in range(3):
        grads, _ = OB.make_grads(SIZES, seed=10 + it)
        for a, b, g in zip(pa, pb, grads):
            a.grad, b.grad = g.clone(), g.clone()
        before = [b.detach().clone() for b in pb]
        beta = [torch.tensor(0.9, dtype=torch.float64)]
        out = torch.zeros(2)
        assert O.fused_step(ob, max_norm=c, beta1_d=beta, norm_out=out) is False
        assert all(torch.equal(x, y) for x, y in zip(before, pb)) and all(torch.equal(b.grad, g) for b, g in zip(pb, grads))
        assert float(out.abs().sum()) == 0.0
        total = clip_grad_norm_(pa, max_norm=c)
        oa.step()
        assert O.step(ob, max_norm=c, norm_out=out) is False
        for a, b in zip(pa, pb):
            assert torch.equal(a, b) and torch.equal(a.grad, b.grad)
            assert torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]) and torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])
        assert float(out[0]) == float(total) and float(total) > c and 0 < float(out[1]) < 1


def test_new_entry_points_are_declared_and_bound():
    from biapy_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    for sym, ret in (("bpx_grad_norm_workspace", "int64_t"), ("bpx_grad_norm", "int"), ("bpx_adam_step_dev", "int")):
        assert re.search(r"^%s %s\(" % (ret, sym), header, re.M), sym
        assert sym in L.EXPORTS and getattr(L.lib._raw, sym) is not None
    assert "optim.hip" in open(os.path.join(ROOT, "biapy_amd", "csrc", "Makefile")).read()
    arr = (L.AdamTensor * 3)()
    for i, n in enumerate((1, 4096, 4097)):
        arr[i].numel = n
    assert L.lib.bpx_grad_norm_workspace(3, arr) == 8 * 4 and L.lib.bpx_grad_norm_workspace(0, None) == 8
    arr[1].numel = -1
    assert L.lib.bpx_grad_norm_workspace(3, arr) == -1
    assert L.lib.bpx_grad_norm(0, None, 1.0, None, 0, None, None) != 0 and b"null pointer" in L.lib.bpx_last_error()


def test_graph_on_still_refuses_a_cpu_device():
    import types

    from biapy_amd import train_engine as TE

    cfg = types.SimpleNamespace(DATA=types.SimpleNamespace(PATCH_SIZE=(8, 8, 8, 1)),
                                TRAIN=types.SimpleNamespace(GRADIENT_CLIP_NORM=1.0, LR_SCHEDULER=types.SimpleNamespace(NAME="onecycle"), VERBOSE=False))
    net = torch.nn.Conv3d(1, 1, 1)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match=r"^graph='on'"):
        TE.train_one_epoch(cfg, net, None, torch.nn.BCEWithLogitsLoss(), None, None, [], [opt], torch.device("cpu"), 0, graph="on")

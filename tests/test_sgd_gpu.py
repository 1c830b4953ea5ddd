"""SGD on the replayed step, on the device: bpx_sgd_step against the fp64 statement and bound of sgd_bounds and against torch's foreach SGD, its
device scalars (clip coefficient, one-cycle momentum) bit for bit against their host forms, optim.step against torch over four steps, and the
captured steps - GraphedTrainStep, train_one_epoch(graph="on") under clipping and a momentum-cycling one-cycle schedule, DataParallelTrainStep -
against their eager forms."""
import functools
import os
import types

import numpy as np
import pytest
import torch
from torch.nn.utils import clip_grad_norm_

import optim_bounds as OB
import sgd_bounds as SB

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = os.path.join(ROOT, "profiles", "sgd_values.txt")
_rows = {}


def _L():
    from biapy_amd import _lib as L

    return L


def _record(key, text):
    """profiles/sgd_values.txt: one row per measured case, rewritten whole so that a partial run leaves a readable file."""
    _rows[key] = text
    try:
        with open(VALUES, "w") as f:
            f.write("bpx_sgd_step on the device: worst |got - fp64 statement| / bound over all elements (tests/test_sgd_gpu.py; bound: tests/sgd_bounds.py)\n")
            for k in sorted(_rows):
                f.write(_rows[k] + "\n")
    except OSError:
        pass                                                               # a read-only checkout: the assertions do not depend on the record


def _sgd(ps, gs, ms, cfg, *, lr_d=None, mom_d=None, gscale_d=None, mom_h=None):
    L = _L()
    arr = (L.AdamTensor * len(ps))()
    for i, (p, g) in enumerate(zip(ps, gs)):
        arr[i].p, arr[i].g, arr[i].numel = p.data_ptr(), g.data_ptr(), p.numel()
        if ms is not None:
            arr[i].m = ms[i].data_ptr()
    ptr = lambda t: None if t is None else t.data_ptr()                   # noqa: E731
    L.check(L.lib.bpx_sgd_step(len(ps), arr, ptr(lr_d), cfg["lr"], ptr(mom_d), cfg["momentum"] if mom_h is None else mom_h, cfg["dampening"], cfg["wd"],
                               1 if cfg["nesterov"] else 0, ptr(gscale_d), L.stream_ptr()))


@functools.lru_cache(maxsize=None)
def _base(many):
    """(parameters, momentum buffers) on the CPU for ADAM_SIZES / MANY_SIZES - made once, never written."""
    sizes = OB.MANY_SIZES if many else OB.ADAM_SIZES
    gen = torch.Generator().manual_seed(0)
    return [torch.randn(*s, generator=gen) for s in sizes], [torch.randn(*s, generator=gen) for s in sizes]


def _dev(ts):
    return [t.clone().to(DEV) for t in ts]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


KERNEL_CONFIGS = dict(SB.CONFIGS, null_m=SB.CONFIGS["plain"])             # the five of sgd_bounds + the no-momentum form with a null .m


def _kernel_run(name, offset):
    """One bpx_sgd_step over the 67 tensors from the shared state; the fp64 statement and its bound, computed once per case and used by both
    comparisons of the test below."""
    cfg = KERNEL_CONFIGS[name]
    p0, b0 = _base(True)
    grads, slab = OB.make_grads(OB.MANY_SIZES, seed=1, offset=offset, device=DEV)
    keep = slab.clone()
    ps, ms = _dev(p0), _dev(b0)
    _sgd(ps, grads, None if name == "null_m" else ms, cfg)
    torch.cuda.synchronize()
    assert torch.equal(slab, keep), "no gscale_d: .g must not be written"
    g_cpu = [g.cpu() for g in grads]
    mom = cfg["momentum"] != 0
    ref = [SB.sgd_reference(p, g, b if mom else None, first=False, **cfg) for p, g, b in zip(p0, g_cpu, b0)]
    bound = [SB.sgd_bound(p, g, b if mom else None, first=False, **cfg) for p, g, b in zip(p0, g_cpu, b0)]
    return dict(cfg=cfg, p0=p0, b0=b0, g=g_cpu, p1=[p.cpu() for p in ps], b1=[b.cpu() for b in ms], ref=ref, bound=bound)


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 3], ids=["aligned", "slab+3"])
@pytest.mark.parametrize("name", list(KERNEL_CONFIGS))
def test_sgd_kernel_against_fp64_and_torch_foreach(name, offset):
    """67 tensors of 1 ... 1.77 M elements (two launches), gradients as views of one slab at offsets 0 (16-byte path where the view lands aligned)
    and 3 (scalar path): every element of p and of the momentum buffer within sgd_bound of the fp64 statement.  Then the same step by
    torch.optim.SGD(foreach=True) from the same state: both sides lie within the bound of the statement, so they differ by at most twice the
    bound; the number of elements that differ at all is recorded, not asserted."""
    r = _kernel_run(name, offset)
    mom = r["cfg"]["momentum"] != 0
    wp = max(SB.worst_ratio(p1, ref[0], bd[0]) for p1, ref, bd in zip(r["p1"], r["ref"], r["bound"]))
    if mom:
        wb = max(SB.worst_ratio(b1, ref[1], bd[1]) for b1, ref, bd in zip(r["b1"], r["ref"], r["bound"]))
    else:
        wb = 0.0
        assert _same(r["b1"], r["b0"]), "no momentum: the buffer must not be touched"
    row = f"{name:12s} offset {offset}: p {wp:.3f}  buf {wb:.3f}  (err / bound, bar 1)"
    print(row)
    _record(("fp64", name, offset), row)
    assert wp <= 1.0 and wb <= 1.0
    cfg = r["cfg"]
    ps = [torch.nn.Parameter(p) for p in _dev(r["p0"])]
    opt = SB.torch_sgd(ps, cfg, foreach=True)
    for p, g, b in zip(ps, r["g"], r["b0"]):
        p.grad = g.to(DEV)
        if cfg["momentum"] != 0:
            opt.state[p]["momentum_buffer"] = b.clone().to(DEV)
    opt.step()
    torch.cuda.synchronize()
    worst, differ, total = 0.0, 0, 0
    for i, p in enumerate(ps):
        pairs = [(p.detach().cpu(), r["p1"][i], r["bound"][i][0])]
        if cfg["momentum"] != 0:
            pairs.append((opt.state[p]["momentum_buffer"].cpu(), r["b1"][i], r["bound"][i][1]))
        for theirs, ours, bd in pairs:
            worst = max(worst, SB.worst_ratio(ours, theirs.double(), 2.0 * bd))
            differ += int((theirs != ours).sum())
            total += theirs.numel()
    row = f"{name:12s} offset {offset}: vs torch foreach {worst:.3f} (err / (2 bound), bar 1); {differ} of {total} elements differ"
    print(row)
    _record(("torch", name, offset), row)
    assert worst <= 1.0


@pytest.mark.parametrize("offset", [0, 3], ids=["aligned", "slab+3"])
def test_sgd_gscale_is_mul_then_plain_step(offset):
    """gscale_d: .g afterwards is g * c (one fp32 product), p and the buffer are those of a plain step on the pre-multiplied gradient - bit for bit."""
    cfg = SB.CONFIGS["nesterov_wd"]
    p0, b0 = _base(False)
    c = torch.tensor(0.37, dtype=torch.float32, device=DEV)
    ga, _ = OB.make_grads(OB.ADAM_SIZES, seed=30, offset=offset, device=DEV)
    gb, _ = OB.make_grads(OB.ADAM_SIZES, seed=30, offset=offset, device=DEV)
    for g in ga:
        g.mul_(c)
    A, B = (_dev(p0), _dev(b0)), (_dev(p0), _dev(b0))
    _sgd(A[0], ga, A[1], cfg)
    _sgd(B[0], gb, B[1], cfg, gscale_d=c)
    torch.cuda.synchronize()
    assert _same(ga, gb), "p.grad after the step is not g * c"
    assert _same(A[0], B[0]) and _same(A[1], B[1])


def test_sgd_device_momentum_and_lr_are_the_host_arguments():
    """momentum_d holding a one-cycle double no float32 holds, lr_d holding float32(lr): bit for bit the call with those values as host arguments
    (the host arguments beside the device ones are deliberately wrong)."""
    cfg = SB.CONFIGS["nesterov_wd"]
    mom = 0.8999999999999999
    assert float(np.float32(mom)) != mom
    p0, b0 = _base(False)
    grads, _ = OB.make_grads(OB.ADAM_SIZES, seed=31, offset=3, device=DEV)
    A, B = (_dev(p0), _dev(b0)), (_dev(p0), _dev(b0))
    _sgd(A[0], grads, A[1], dict(cfg, momentum=mom))
    _sgd(B[0], grads, B[1], dict(cfg, lr=7.0), mom_d=torch.tensor(mom, dtype=torch.float64, device=DEV), mom_h=0.5,
         lr_d=torch.tensor(cfg["lr"], dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    assert _same(A[0], B[0]) and _same(A[1], B[1])


def test_sgd_two_runs_are_bit_identical():
    cfg = SB.CONFIGS["nesterov_wd"]
    p0, b0 = _base(True)
    out = []
    for _ in range(2):
        grads, _ = OB.make_grads(OB.MANY_SIZES, seed=32, offset=3, device=DEV)
        ps, ms = _dev(p0), _dev(b0)
        _sgd(ps, grads, ms, cfg)
        torch.cuda.synchronize()
        out.append((ps, ms))
    assert _same(out[0][0], out[1][0]) and _same(out[0][1], out[1][1])
    assert not _same(out[0][0], _dev(p0))


# ---- the launch scaffold all update kernels share -------------------------------------------------------------------------------------------------------
# 300 tensors: five update launches of at most 64 tensors and two step-increment launches of at most 256, sizes of 1 element ... two 4096-element
# chunks, (4099,) = one chunk + 3, the gradients views of one slab 3 elements in (all but a few unaligned).
SCAFFOLD_SIZES = [((1,), (16,), (4099,), (8192,), (5, 7))[i % 5] for i in range(300)]
SCAFFOLD_CLIP = 100.0                                                      # ||g|| ~ sqrt(740 580) = 860: every step clips


@functools.lru_cache(maxsize=None)
def _scaffold_base():
    """(parameters, momentum buffers) on the CPU - made once, never written."""
    gen = torch.Generator().manual_seed(7)
    return [torch.randn(*s, generator=gen) for s in SCAFFOLD_SIZES], [torch.randn(*s, generator=gen) for s in SCAFFOLD_SIZES]


def _torch_clip(params):
    """clip_grad_norm_ on the reference's gradients; returns the coefficient it multiplied by as a device float (the same two torch ops on the same
    norm as torch.nn.utils.clip_grad), which the kernels under test are then handed: both sides form the same fp32 product g * c."""
    total = clip_grad_norm_(params, SCAFFOLD_CLIP, foreach=True)
    return torch.clamp(SCAFFOLD_CLIP / (total + 1e-6), max=1.0).float()


@pytest.mark.parametrize("path", ["bpx_adam_step", "bpx_adam_step_dev", "bpx_sgd_step"])
def test_update_kernels_across_launch_batches_against_torch(path):
    """Three steps over the 300 tensors through each entry point, against torch's own step on cloned tensors.  Adam: AdamW(fused, capturable) from
    the same zero state, p, m, v within the 2e-6 of kernel_checks.check_fused_adam, every `step` 3.0 exactly; the _dev form reads beta1 from a
    device double (the host argument is wrong on purpose) and clips.  SGD (Nesterov, weight decay, clipped): torch.optim.SGD(foreach=True) started
    from this side's state at every step, so both sides lie within sgd_bound of the fp64 statement of that step and differ by at most twice the
    bound.  With clipping, .g afterwards is what clip_grad_norm_ leaves, bit for bit.  No tensor keeps its initial value."""
    from kernel_checks import relerr

    L = _L()
    p0, b0 = _scaffold_base()
    ps = _dev(p0)
    ref = [torch.nn.Parameter(p) for p in _dev(p0)]
    clip = path != "bpx_adam_step"
    if path == "bpx_sgd_step":
        cfg = SB.CONFIGS["nesterov_wd"]
        ms = _dev(b0)
        opt = SB.torch_sgd(ref, cfg, foreach=True)
        for r, b in zip(ref, b0):
            opt.state[r]["momentum_buffer"] = b.clone().to(DEV)
    else:
        beta1 = 0.8999999999999999 if clip else 0.9                      # a one-cycle double that no float32 holds
        ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
        steps = [torch.zeros((), dtype=torch.float32, device=DEV) for _ in ps]
        opt = torch.optim.AdamW(ref, lr=1e-2, betas=(beta1, 0.999), weight_decay=1e-2, fused=True, capturable=True)
        beta1_d = torch.tensor(beta1, dtype=torch.float64, device=DEV)
        arr = (L.AdamTensor * len(ps))()
    worst = 0.0
    for it in range(3):
        grads, _ = OB.make_grads(SCAFFOLD_SIZES, seed=50 + it, offset=3, device=DEV)
        for r, g in zip(ref, grads):
            r.grad = g.clone()
        coef = _torch_clip(ref) if clip else None
        if path == "bpx_sgd_step":
            with torch.no_grad():                                          # torch's step starts from this side's state
                for r, p, m in zip(ref, ps, ms):
                    r.copy_(p)
                    opt.state[r]["momentum_buffer"].copy_(m)
            before = [(p.cpu(), m.cpu()) for p, m in zip(ps, ms)]
            opt.step()
            _sgd(ps, grads, ms, cfg, gscale_d=coef)
            torch.cuda.synchronize()
            for r, p, m, g, (pb, mb) in zip(ref, ps, ms, grads, before):
                bp, bb = SB.sgd_bound(pb, g.cpu(), mb, first=False, **cfg)
                worst = max(worst, SB.worst_ratio(p, r.detach().cpu().double(), 2.0 * bp),
                            SB.worst_ratio(m, opt.state[r]["momentum_buffer"].cpu().double(), 2.0 * bb))
        else:
            opt.step()
            for i, (p, g, m, v, st) in enumerate(zip(ps, grads, ms, vs, steps)):
                arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].step, arr[i].numel = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                                                                    st.data_ptr(), p.numel())
            if clip:
                L.check(L.lib.bpx_adam_step_dev(len(ps), arr, None, 1e-2, beta1_d.data_ptr(), 0.5, 0.999, 1e-8, 1e-2, 1, coef.data_ptr(), L.stream_ptr()))
            else:
                L.check(L.lib.bpx_adam_step(len(ps), arr, None, 1e-2, beta1, 0.999, 1e-8, 1e-2, 1, L.stream_ptr()))
            torch.cuda.synchronize()
        if clip:
            assert float(coef) < 1.0
            assert _same(grads, [r.grad for r in ref]), "p.grad after the step is not what clip_grad_norm_ leaves"
    if path == "bpx_sgd_step":
        print(f"{path}: worst err / (2 bound) {worst:.3f}, bar 1")
        assert worst <= 1.0
        state = (ps, ms)
    else:
        errs = {"p": 0.0, "m": 0.0, "v": 0.0}
        for r, p, m, v in zip(ref, ps, ms, vs):
            errs["p"] = max(errs["p"], relerr(p, r))
            errs["m"] = max(errs["m"], relerr(m, opt.state[r]["exp_avg"]))
            errs["v"] = max(errs["v"], relerr(v, opt.state[r]["exp_avg_sq"]))
        print(f"{path}: " + ", ".join(f"{k} {e:.3e} / bound 2e-6" for k, e in errs.items()))
        assert all(e <= 2e-6 for e in errs.values()), errs
        assert all(float(st) == 3.0 for st in steps) and all(float(opt.state[r]["step"]) == 3.0 for r in ref)
        state = (ps, ms, vs)
    for ts, init in zip(state, (p0, b0 if path == "bpx_sgd_step" else [torch.zeros_like(p) for p in p0], [torch.zeros_like(p) for p in p0])):
        assert not any(torch.equal(t.cpu(), i) for t, i in zip(ts, init)), "a tensor was left at its initial value"


@pytest.mark.parametrize("name", ["nesterov_wd", "wd"])
def test_optim_step_against_torch_over_four_steps(name):
    """optim.step against torch's SGD, lr a device scalar scaled between the steps (as kernel_checks.check_fused_adam does for Adam): the package
    takes every step but the one that creates the momentum buffers; p and the buffer within that check's 2e-6."""
    from kernel_checks import relerr

    from biapy_amd import optim as O

    cfg = SB.CONFIGS[name]
    p0, _ = _base(False)
    pa = [torch.nn.Parameter(p) for p in _dev(p0)]
    pb = [torch.nn.Parameter(p) for p in _dev(p0)]
    oa = SB.torch_sgd(pa, dict(cfg, lr=torch.tensor(cfg["lr"], device=DEV)))
    ob = SB.torch_sgd(pb, dict(cfg, lr=torch.tensor(cfg["lr"], device=DEV)))
    used = []
    for it in range(4):
        grads, _ = OB.make_grads(OB.ADAM_SIZES, seed=40 + it, offset=3 * (it % 2), device=DEV)
        for a, b, g in zip(pa, pb, grads):
            a.grad, b.grad = g.clone(), g
        oa.step()
        used.append(O.step(ob))
        for o in (oa, ob):
            o.param_groups[0]["lr"].mul_(0.7)
    torch.cuda.synchronize()
    mom = cfg["momentum"] != 0
    assert used == ([False, True, True, True] if mom else [True] * 4), used
    worst = {"p": 0.0, "buf": 0.0}
    for a, b in zip(pa, pb):
        worst["p"] = max(worst["p"], relerr(b, a))
        if mom:
            worst["buf"] = max(worst["buf"], relerr(ob.state[b]["momentum_buffer"], oa.state[a]["momentum_buffer"]))
    print(f"optim.step[SGD {name}]: " + ", ".join(f"{k} {v:.3e} / bound 2e-6" for k, v in worst.items()))
    assert all(v <= 2e-6 for v in worst.values()), worst


# ---- captured steps: a two-level ResUNet at 16^3, fp32 compute -----------------------------------------------------------------------------------------
# The gradient norms of this model on these batches are 2.04, 1.55, 1.14 at the first steps (tests/test_clip_sched_gpu.py); the tests assert that
# CLIP_C clips on every step they run, and NO_CLIP_C is far over the largest.
CLIP_C = 0.25
NO_CLIP_C = 1e3
LR = 1e-2


def _resunet(seed=0):
    from biapy_amd.resunet import ResUNet

    torch.manual_seed(seed)
    return ResUNet(image_shape=(16, 16, 16, 1), activation="elu", feature_maps=[16, 32], drop_values=[0.0, 0.0], normalization="in", yx_down=[2],
                   z_down=[2], isotropy=[True, True], larger_io=False, conv_layers=[2, 2], compute_dtype=torch.float32).cuda().train()


def _batches(n=4, B=2, seed=5, channels_last=False):
    g = torch.Generator().manual_seed(seed)
    shape = (B, 16, 16, 16, 1) if channels_last else (B, 1, 16, 16, 16)
    return [(torch.randn(*shape, generator=g), (torch.rand(*shape, generator=g) > 0.5).float()) for _ in range(n)]


def _sgd_opt(m, **kw):
    """The reference's SGD: momentum 0.9, Nesterov, the weight decay in one of two parameter groups."""
    decay = [p for p in m.parameters() if p.dim() > 1]
    rest = [p for p in m.parameters() if p.dim() <= 1]
    return torch.optim.SGD([dict(params=decay, weight_decay=1e-2), dict(params=rest, weight_decay=0.0)], lr=LR, momentum=0.9, nesterov=True, **kw)


def _zero_state(m, opt, snap=None):
    """The state train_engine._restore leaves after a capture's warm-up: the weights put back, the momentum buffers zero."""
    with torch.no_grad():
        if snap is not None:
            for p, s in zip(m.parameters(), snap):
                p.copy_(s)
        for p in m.parameters():
            st = opt.state[p]
            if "momentum_buffer" in st and st["momentum_buffer"] is not None:
                st["momentum_buffer"].zero_()
            else:
                st["momentum_buffer"] = torch.zeros_like(p)


def _within_bar(a, b):
    worst = 0.0
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        if p.dim() == 5:
            err, bound = (p - q).abs().max().item(), 2e-5 * max(1.0, q.abs().max().item())
            worst = max(worst, err / bound)
            assert err <= bound, (k, err, bound)
    return worst


@pytest.mark.parametrize("clip", [0.0, CLIP_C, NO_CLIP_C], ids=["no_clip", "clip", "inactive_clip"])
def test_graphed_sgd_step_is_the_eager_step(clip):
    """GraphedTrainStep with the reference's SGD: 4 replays == 4 eager optim.step steps from the same weights and (zeroed) momentum buffers, bit for
    bit; against torch's own loop from a fresh optimizer (torch seeds the buffers with the first gradient) within the bar of
    test_clip_sched_gpu.test_graphed_step_clips_like_the_eager_loop.  Under clipping grad_norm is [norm, coefficient] of the last step's gradients."""
    from biapy_amd import optim as O
    from biapy_amd.graphs import GraphedTrainStep
    from biapy_amd.losses import BCEWithLogitsLoss

    data = [(x.cuda(), t.cuda()) for x, t in _batches()]
    loss_fn = BCEWithLogitsLoss()
    m = _resunet()
    opt = _sgd_opt(m)
    snap = [p.detach().clone() for p in m.parameters()]
    gstep = GraphedTrainStep(m, loss_fn, opt, data[0][0], data[0][1], max_grad_norm=clip)
    assert gstep.device_momentum and not gstep.device_betas and gstep._fused
    assert all(torch.is_tensor(g["lr"]) and g["lr"].is_cuda for g in opt.param_groups) and all(type(g["momentum"]) is float for g in opt.param_groups)
    _zero_state(m, opt, snap)
    norms = []
    for x, t in data:
        gstep(x, t)
        if clip:
            norms.append(gstep.grad_norm.cpu().numpy().copy())

    twin = _resunet()
    topt = _sgd_opt(twin)
    _zero_state(twin, topt)
    out = torch.zeros(2, device=DEV)
    kw = dict(max_norm=clip, norm_out=out) if clip else {}
    used, want = [], []
    for x, t in data:
        topt.zero_grad(set_to_none=True)
        loss_fn(twin(x), t).backward()
        if clip:
            want.append(OB.clip_reference([p.grad for p in twin.parameters()], clip)[:2])
        used.append(O.step(topt, **kw))
    torch.cuda.synchronize()
    assert used == [True] * 4
    for (k, p), (_, q) in zip(m.named_parameters(), twin.named_parameters()):
        assert torch.equal(p, q), k
        assert torch.equal(opt.state[p]["momentum_buffer"], topt.state[q]["momentum_buffer"]), k
    for got, (wn, wc) in zip(norms, want):                               # 1 ulp each: the bound test_clip_sched_gpu holds bpx_grad_norm to
        assert OB.ulps(got[0], wn) <= 1 and OB.ulps(got[1], wc) <= 1, (got, wn, wc)
        assert (got[1] < 1.0) == (clip == CLIP_C) and (clip == CLIP_C) == (got[0] > clip)

    ref = _resunet()
    ropt = _sgd_opt(ref)
    for x, t in data:
        ropt.zero_grad(set_to_none=True)
        loss_fn(ref(x), t).backward()
        if clip:
            clip_grad_norm_(list(ref.parameters()), max_norm=clip)
        ropt.step()
    torch.cuda.synchronize()
    worst = _within_bar(m, ref)
    print(f"graphed SGD (clip {clip}) vs torch's eager loop: worst err / bound = {worst:.3f}; [norm, coef] {[n.tolist() for n in norms]}")


def test_graphed_sgd_step_refuses_before_capture_what_it_cannot_take():
    """A fresh SGD with momentum and one warm-up step: that step is torch's (it creates the buffers), so the package did not take the last warm-up
    step - ValueError before any capture, never torch's step inside one.  The process stays usable."""
    from biapy_amd.graphs import GraphedTrainStep
    from biapy_amd.losses import BCEWithLogitsLoss

    x, t = [(a.cuda(), b.cuda()) for a, b in _batches(1)][0]
    m = _resunet()
    with pytest.raises(ValueError, match="cannot be captured"):
        GraphedTrainStep(m, BCEWithLogitsLoss(), _sgd_opt(m), x, t, warmup=1)
    assert not torch.cuda.is_current_stream_capturing()
    with pytest.raises(ValueError, match="capturable=True"):
        GraphedTrainStep(m, BCEWithLogitsLoss(), _sgd_opt(m, maximize=True), x, t)
    assert float(torch.ones(4, device=DEV).sum()) == 4.0


def _cfg(clip, sched):
    return types.SimpleNamespace(DATA=types.SimpleNamespace(PATCH_SIZE=(16, 16, 16, 1)),
                                 TRAIN=types.SimpleNamespace(GRADIENT_CLIP_NORM=clip, LR_SCHEDULER=types.SimpleNamespace(NAME=sched), VERBOSE=False))


def _epochs(graph, data, n_epochs=2):
    from biapy_amd import train_engine as TE
    from biapy_amd.losses import BCEWithLogitsLoss

    m = _resunet()
    opt = _sgd_opt(m)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=LR, total_steps=n_epochs * len(data))
    assert sched.cycle_momentum and sched.use_beta1 is False
    loss_fn = BCEWithLogitsLoss()
    stats = []
    for ep in range(n_epochs):
        s, _ = TE.train_one_epoch(_cfg(CLIP_C, "onecycle"), m, None, loss_fn, None, None, data, [opt], torch.device("cuda"), ep, lr_scheduler=[sched],
                                  loss_names=["loss"], graph=graph)
        stats.append(s)
    torch.cuda.synchronize()
    return m, opt, sched, stats


def _onecycle_momenta(steps):
    """The doubles a OneCycleLR of `steps` steps assigns to an SGD's group['momentum'] (they do not depend on the learning rate)."""
    p = [torch.nn.Parameter(torch.zeros(2))]
    p[0].grad = torch.zeros(2)
    opt = torch.optim.SGD(p, lr=LR, momentum=0.9, nesterov=True)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=LR, total_steps=steps)
    out = {opt.param_groups[0]["momentum"]}
    for _ in range(steps - 1):
        opt.step()
        sched.step()
        out.add(opt.param_groups[0]["momentum"])
    return out


@pytest.mark.parametrize("ragged", [False, True], ids=["even", "ragged"])
def test_train_one_epoch_replays_sgd_under_clipping_and_onecycle(ragged):
    """GRADIENT_CLIP_NORM + OneCycleLR (lr AND group['momentum'] move every step) with SGD on the replayed step - a ValueError before this
    feature - against graph="off", compared as test_clip_sched_gpu.test_train_one_epoch_replays_under_clipping_and_onecycle compares AdamW."""
    data = _batches(3, channels_last=True)
    if ragged:
        data = data + _batches(1, B=1, seed=9, channels_last=True)
    on, opt_on, sched_on, st_on = _epochs("on", data)
    off, opt_off, sched_off, st_off = _epochs("off", data)
    gstep = on._bpx_graph_step[1]
    assert gstep.device_momentum and gstep.max_grad_norm == CLIP_C and not hasattr(off, "_bpx_graph_step")
    norm, coef = gstep.grad_norm.tolist()
    assert norm > CLIP_C and 0 < coef < 1
    assert sched_on.last_epoch == sched_off.last_epoch == 2 * len(data)
    for g_on, g_off, dev_mom in zip(opt_on.param_groups, opt_off.param_groups, gstep._lr.momenta):
        assert type(g_on["momentum"]) is float and g_on["momentum"] == g_off["momentum"] != 0.9
        assert abs(float(g_on["lr"]) - float(g_off["lr"])) <= 1e-6 * float(g_off["lr"])
        # the device double is one of the schedule's host doubles (the one the last replay read)
        assert float(dev_mom) in _onecycle_momenta(2 * len(data))
    for a, b in zip(st_on, st_off):
        assert abs(a["lr"] - b["lr"]) <= 1e-6 * b["lr"], (a["lr"], b["lr"])
        assert abs(a["loss"] - b["loss"]) <= 1e-4 * abs(b["loss"]), (a["loss"], b["loss"])
    worst = _within_bar(on, off)
    print(f"train_one_epoch SGD clip+onecycle ragged={ragged}: worst err / bound = {worst:.3f}; lr meters {[s['lr'] for s in st_on]}")


def test_data_parallel_step_replays_sgd():
    """DataParallelTrainStep(graph=True, warmup=1) with SGD at world size 1 against its graph=False form, as
    test_gpu_parity.test_data_parallel_step_adopts_the_engine_gradient_slab compares AdamW."""
    from biapy_amd.graphs import DataParallelTrainStep
    from biapy_amd.losses import BCEWithLogitsLoss

    data = [(x.cuda(), t.cuda()) for x, t in _batches(3)]
    nets = []
    for graph in (False, True):
        m = _resunet()
        opt = _sgd_opt(m)
        if graph:
            snap = [p.detach().clone() for p in m.parameters()]
            step = DataParallelTrainStep(m, BCEWithLogitsLoss(), opt, data[0][0], data[0][1], graph=True, warmup=1)
            assert step.adopted and step._sgd
            _zero_state(m, opt, snap)
        else:
            step = DataParallelTrainStep(m, BCEWithLogitsLoss(), opt, data[0][0], data[0][1], graph=False)
        for x, t in data:
            step(x, t)
        torch.cuda.synchronize()
        nets.append(m)
    _within_bar(nets[1], nets[0])

"""Gradient clipping and per-step schedules on the graphed train step, on the device: the norm kernel against the fp64 statement of optim_bounds,
the Adam kernel with device hyper-parameters against bpx_adam_step and torch's fused capturable Adam(W), GraphedTrainStep(max_grad_norm=...) against
an eager twin, and train_one_epoch(graph="on") under TRAIN.GRADIENT_CLIP_NORM with the one-cycle and warm-up schedules."""
import math
import types

import numpy as np
import pytest
import torch
from torch.nn.utils import clip_grad_norm_

import optim_bounds as OB

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _L():
    from biapy_amd import _lib as L

    return L


def _tensor_array(ps, gs, ms, vs, steps):
    L = _L()
    arr = (L.AdamTensor * len(gs))()
    for i, g in enumerate(gs):
        arr[i].g, arr[i].numel = g.data_ptr(), g.numel()
        if ps is not None:
            arr[i].p, arr[i].m, arr[i].v, arr[i].step = ps[i].data_ptr(), ms[i].data_ptr(), vs[i].data_ptr(), steps[i].data_ptr()
    return arr


def _grad_norm(grads, max_norm):
    """bpx_grad_norm over `grads`: the two output floats as numpy float32."""
    L = _L()
    arr = _tensor_array(None, grads, None, None, None)
    nbytes = L.lib.bpx_grad_norm_workspace(len(grads), arr)
    assert nbytes == 8 * sum(-(-g.numel() // 4096) for g in grads)
    ws = torch.full((nbytes // 8 + 8,), float("nan"), dtype=torch.float64, device=DEV)     # 8 guard doubles behind the workspace
    out = torch.full((2,), -7.0, dtype=torch.float32, device=DEV)
    L.check(L.lib.bpx_grad_norm(len(grads), arr, float(max_norm), ws.data_ptr(), nbytes, out.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.isnan(ws[nbytes // 8:]).all(), "the partials kernel wrote past its workspace"
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def norm_cases():
    """{offset: (device gradient views, slab, fp64 norm)} - computed once."""
    out = {}
    for offset in (0, 3):
        grads, slab = OB.make_grads(OB.MANY_SIZES, seed=1, offset=offset, device=DEV)
        true = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
        out[offset] = (grads, slab, true)
    return out


# ---- 4. the norm kernel --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 3], ids=["aligned", "slab+3"])
@pytest.mark.parametrize("scale", [0.5, 2.0], ids=["below", "above"])
def test_grad_norm_kernel_against_fp64(norm_cases, offset, scale):
    """67 tensors of 1 ... 1.77 M elements (two launches of the partials kernel), views of one slab at offsets 0 and 3.  Both sides sum in fp64: the
    order moves the sum by ~n 2^-53 relative, which can only move the final rounding - 1 float32 ulp for the norm, 1 for the coefficient against
    min(1, float32(max_norm / (float64(norm) + 1e-6))).  Two runs agree bit for bit."""
    grads, _, true = norm_cases[offset]
    assert len(grads) > 64
    max_norm = scale * true
    want_norm, want_coef, _ = OB.clip_reference(grads, max_norm)
    got = _grad_norm(grads, max_norm)
    again = _grad_norm(grads, max_norm)
    un, uc = OB.ulps(got[0], want_norm), OB.ulps(got[1], want_coef)
    print(f"grad_norm[offset={offset} scale={scale}]: norm {got[0]!r} vs {want_norm!r} ({un} ulp / bound 1), coef {got[1]!r} vs {want_coef!r} ({uc} ulp / bound 1)")
    assert got.tobytes() == again.tobytes()
    assert un <= 1 and uc <= 1
    assert (got[1] == np.float32(1.0)) == (scale > 1)


def test_grad_norm_kernel_zero_and_nan(norm_cases):
    grads, slab, _ = norm_cases[3]
    keep = slab.clone()
    try:
        slab.zero_()
        got = _grad_norm(grads, 0.5)
        assert got[0] == 0.0 and got[1] == np.float32(1.0)
        slab.copy_(keep)
        grads[3].view(-1)[1_000_003] = float("nan")                        # inside the 1.77 M-element tensor, far from either end
        got = _grad_norm(grads, 0.5)
        assert np.isnan(got[0]) and np.isnan(got[1])
    finally:
        slab.copy_(keep)                                                  # the fixture is shared: leave it as it was
        torch.cuda.synchronize()


# ---- 5. the Adam kernel with device hyper-parameters ---------------------------------------------------------------------------------------------------
def _adam_state(seed=0):
    gen = torch.Generator().manual_seed(seed)
    base = [torch.randn(*s, generator=gen) for s in OB.ADAM_SIZES]
    mk = lambda: [b.clone().to(DEV) for b in base]                        # noqa: E731
    ps = mk()
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    steps = [torch.zeros((), dtype=torch.float32, device=DEV) for _ in ps]
    return ps, ms, vs, steps


HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)


def _adam(ps, gs, ms, vs, steps, wd, decoupled, *, dev=False, beta1_d=None, gscale_d=None, beta1_h=None):
    L = _L()
    arr = _tensor_array(ps, gs, ms, vs, steps)
    h = dict(HYPER, beta1=HYPER["beta1"] if beta1_h is None else beta1_h)
    if dev:
        L.check(L.lib.bpx_adam_step_dev(len(ps), arr, None, h["lr"], None if beta1_d is None else beta1_d.data_ptr(), h["beta1"], h["beta2"], h["eps"],
                                        wd, decoupled, None if gscale_d is None else gscale_d.data_ptr(), L.stream_ptr()))
    else:
        L.check(L.lib.bpx_adam_step(len(ps), arr, None, h["lr"], h["beta1"], h["beta2"], h["eps"], wd, decoupled, L.stream_ptr()))


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("wd,decoupled", [(1e-2, 1), (1e-3, 0)], ids=["adamw", "adam"])
def test_adam_dev_without_scale_is_bpx_adam_step(wd, decoupled):
    """5a: gscale_d NULL, beta1_d holding the host value (the host argument deliberately wrong): p, m, v bit-identical to bpx_adam_step over 3 steps."""
    A, B = _adam_state(), _adam_state()
    b1 = torch.tensor(HYPER["beta1"], dtype=torch.float64, device=DEV)
    for it in range(3):
        grads, _ = OB.make_grads(OB.ADAM_SIZES, seed=20 + it, offset=3 * (it % 2), device=DEV)
        keep = [g.clone() for g in grads]
        _adam(A[0], grads, A[1], A[2], A[3], wd, decoupled)
        _adam(B[0], grads, B[1], B[2], B[3], wd, decoupled, dev=True, beta1_d=b1, beta1_h=0.5)
        torch.cuda.synchronize()
        assert _same(grads, keep)                                         # no scale: .g is not written
    for k in range(4):
        assert _same(A[k], B[k]), ("p", "m", "v", "step")[k]
    assert float(A[3][0]) == 3.0


@pytest.mark.parametrize("wd,decoupled", [(1e-2, 1), (1e-3, 0)], ids=["adamw", "adam"])
def test_adam_dev_scale_is_mul_then_bpx_adam_step(wd, decoupled):
    """5b: with the coefficient the norm kernel left on the device: bit-identical to bpx_adam_step on g.mul_(c), and .g afterwards is g * c."""
    A, B = _adam_state(), _adam_state()
    L = _L()
    for it in range(3):
        ga, _ = OB.make_grads(OB.ADAM_SIZES, seed=30 + it, offset=3 * (it % 2), device=DEV)
        gb, _ = OB.make_grads(OB.ADAM_SIZES, seed=30 + it, offset=3 * (it % 2), device=DEV)
        arr = _tensor_array(None, gb, None, None, None)
        nbytes = L.lib.bpx_grad_norm_workspace(len(gb), arr)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
        out = torch.zeros(2, dtype=torch.float32, device=DEV)
        L.check(L.lib.bpx_grad_norm(len(gb), arr, 100.0, ws.data_ptr(), nbytes, out.data_ptr(), L.stream_ptr()))
        c = float(out[1])
        assert 0.0 < c < 1.0                                              # ||g|| ~ sqrt(1.77 M) = 1330 > 100
        for g in ga:
            g.mul_(c)
        _adam(A[0], ga, A[1], A[2], A[3], wd, decoupled)
        _adam(B[0], gb, B[1], B[2], B[3], wd, decoupled, dev=True, gscale_d=out[1:])
        torch.cuda.synchronize()
        assert _same(ga, gb), "p.grad after the step is not g * c"
    for k in range(4):
        assert _same(A[k], B[k]), ("p", "m", "v", "step")[k]


@pytest.mark.parametrize("cls,wd", [(torch.optim.AdamW, 1e-2), (torch.optim.Adam, 1e-3)], ids=["adamw", "adam"])
def test_fused_step_with_a_moving_beta1_against_torch(cls, wd):
    """5c: beta1 from a real OneCycleLR, new at every step, against torch's fused capturable Adam / AdamW given the same floats: parameters and
    moments within 2e-6 relative (kernel_checks.relerr - the bar of check_fused_adam)."""
    from kernel_checks import relerr

    from biapy_amd import optim as O

    betas = OB.onecycle_beta1(steps=6)
    gen = torch.Generator().manual_seed(0)
    base = [torch.randn(*s, generator=gen) for s in OB.ADAM_SIZES]
    pa = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    pb = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    oa = cls(pa, lr=torch.tensor(1e-2, device=DEV), weight_decay=wd, fused=True, capturable=True)
    ob = cls(pb, lr=torch.tensor(1e-2, device=DEV), weight_decay=wd, fused=True, capturable=True)
    b1_d = [torch.zeros((), dtype=torch.float64, device=DEV)]
    used = []
    for it, b1 in enumerate(betas):
        grads, _ = OB.make_grads(OB.ADAM_SIZES, seed=40 + it, offset=3 * (it % 2), device=DEV)
        for a, b, g in zip(pa, pb, grads):
            a.grad, b.grad = g.clone(), g
        for o in (oa, ob):
            o.param_groups[0]["betas"] = (b1, 0.999)
        b1_d[0].fill_(b1)
        oa.step()
        used.append(O.step(ob, beta1_d=b1_d))
    torch.cuda.synchronize()
    assert used == [False] + [True] * (len(betas) - 1)                    # the first step creates the state: torch's own
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for a, b in zip(pa, pb):
        sa, sb = oa.state[a], ob.state[b]
        worst["p"] = max(worst["p"], relerr(b, a))
        worst["m"] = max(worst["m"], relerr(sb["exp_avg"], sa["exp_avg"]))
        worst["v"] = max(worst["v"], relerr(sb["exp_avg_sq"], sa["exp_avg_sq"]))
        assert float(sa["step"]) == float(sb["step"]) == len(betas)
    print(f"fused_step[{cls.__name__}, moving beta1]: " + ", ".join(f"{k} {v:.3e} / bound 2e-6" for k, v in worst.items()))
    assert all(v <= 2e-6 for v in worst.values()), worst


# ---- 6. GraphedTrainStep(max_grad_norm=c) --------------------------------------------------------------------------------------------------------------
# The 16^3 two-level fp32 ResUNet (seed 0) trained on the three batches of _batches() with AdamW (lr 1e-3) and clipping has the global gradient norms
# 2.04, 1.55, 1.14 at its first three steps and 1.05, 0.71, 0.95 at the next three (a second epoch), computed beforehand on the CPU with
# oracle/net_oracle.py (resunet_forward + bce_with_logits on the model's state dict).  CLIP_C sits under the smallest by a factor of 2.8 - the tests
# assert that it clips on every step - and NO_CLIP_C far over the largest.
CLIP_C = 0.25
NO_CLIP_C = 1e3


def _resunet(seed=0):
    from biapy_amd.resunet import ResUNet

    torch.manual_seed(seed)
    return ResUNet(image_shape=(16, 16, 16, 1), activation="elu", feature_maps=[16, 32], drop_values=[0.0, 0.0], normalization="in", yx_down=[2],
                   z_down=[2], isotropy=[True, True], larger_io=False, conv_layers=[2, 2], compute_dtype=torch.float32).cuda().train()


def _batches(n=3, B=2, seed=5, channels_last=False):
    g = torch.Generator().manual_seed(seed)
    shape = (B, 16, 16, 16, 1) if channels_last else (B, 1, 16, 16, 16)
    return [(torch.randn(*shape, generator=g), (torch.rand(*shape, generator=g) > 0.5).float()) for _ in range(n)]


def _undo_warmup(m, opt, snap):
    with torch.no_grad():
        for p, s in zip(m.parameters(), snap):
            p.copy_(s)
        for st in opt.state.values():
            for v in st.values():
                if torch.is_tensor(v):
                    v.zero_()


def _graphed_run(max_grad_norm, data):
    from biapy_amd.graphs import GraphedTrainStep
    from biapy_amd.losses import BCEWithLogitsLoss

    m = _resunet()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, capturable=True)
    snap = [p.detach().clone() for p in m.parameters()]
    step = GraphedTrainStep(m, BCEWithLogitsLoss(), opt, data[0][0].cuda(), data[0][1].cuda(), max_grad_norm=max_grad_norm)
    _undo_warmup(m, opt, snap)
    norms = []
    for x, t in data:
        step(x.cuda(), t.cuda())
        if step.grad_norm is not None:
            norms.append(step.grad_norm.cpu().numpy().copy())
    torch.cuda.synchronize()
    return m, norms


def test_graphed_step_clips_like_the_eager_loop():
    from biapy_amd.losses import BCEWithLogitsLoss

    data = _batches()
    m, norms = _graphed_run(CLIP_C, data)
    twin = _resunet()
    opt = torch.optim.AdamW(twin.parameters(), lr=1e-3, capturable=True)
    loss_fn = BCEWithLogitsLoss()
    twin_norms = []
    for x, t in data:
        opt.zero_grad(set_to_none=True)
        loss_fn(twin(x.cuda()), t.cuda()).backward()
        twin_norms.append(float(clip_grad_norm_(list(twin.parameters()), max_norm=CLIP_C)))
        opt.step()
    torch.cuda.synchronize()
    print("eager norms", twin_norms, "graph [norm, coef]", [n.tolist() for n in norms])
    assert all(n > CLIP_C for n in twin_norms), twin_norms                  # clipping is active on every step
    for (gn, gc), tn in zip(norms, twin_norms):
        assert abs(gn - tn) <= 1e-3 * tn and abs(gc - CLIP_C / tn) <= 1e-3 * gc
    worst = 0.0
    for (k, p), (_, q) in zip(m.named_parameters(), twin.named_parameters()):
        if p.dim() == 5:
            err, bound = (p - q).abs().max().item(), 2e-5 * max(1.0, q.abs().max().item())
            worst = max(worst, err / bound)
            assert err <= bound, (k, err, bound)
    print(f"graphed clip vs eager: worst err / bound = {worst:.3f}")


def test_graphed_step_with_an_inactive_clip_is_the_unclipped_step():
    data = _batches()
    a, norms = _graphed_run(NO_CLIP_C, data)
    b, none = _graphed_run(0.0, data)
    assert none == [] and all(float(n[1]) == 1.0 and 0 < float(n[0]) < NO_CLIP_C for n in norms)
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p, q), k


def test_capture_keeps_the_garbage_collector_out():
    """graphs._capture: unreachable cycles are collected before the capture begins and no collection pass runs inside it (a dead step object holds
    a HIP graph and its pool; tearing those down while another capture is open aborts the process); the collector is back on afterwards."""
    import gc
    import weakref

    from biapy_amd.graphs import _capture

    class Node:
        pass

    a, b = Node(), Node()
    a.other, b.other = b, a                                               # a dead cycle, as a dropped GraphedTrainStep is
    a.payload = torch.zeros(8, device=DEV)
    alive = weakref.ref(a)
    del a, b
    x = torch.zeros(4, device=DEV)
    g = torch.cuda.CUDAGraph()
    assert gc.isenabled()
    with _capture(g):
        assert alive() is None and not gc.isenabled()
        y = x + 1
    assert gc.isenabled()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, torch.ones(4, device=DEV))


# ---- 7, 8. train_one_epoch(graph="on") -----------------------------------------------------------------------------------------------------------------
def _cfg(clip, sched):
    return types.SimpleNamespace(DATA=types.SimpleNamespace(PATCH_SIZE=(16, 16, 16, 1)),
                                 TRAIN=types.SimpleNamespace(GRADIENT_CLIP_NORM=clip, LR_SCHEDULER=types.SimpleNamespace(NAME=sched), VERBOSE=False))


class _WarmupCosine:
    """Stand-in for the reference's WarmUpCosineDecayScheduler: per-iteration, ASSIGNS a float to group['lr']."""

    def __init__(self, lr=1e-3, min_lr=1e-5, warmup_epochs=1, epochs=2):
        self.lr, self.min_lr, self.warmup_epochs, self.epochs = lr, min_lr, warmup_epochs, epochs

    def adjust_learning_rate(self, optimizer, epoch):
        if epoch < self.warmup_epochs:
            lr = self.lr * epoch / self.warmup_epochs
        else:
            lr = self.min_lr + (self.lr - self.min_lr) * 0.5 * (1.0 + math.cos(math.pi * (epoch - self.warmup_epochs) / (self.epochs - self.warmup_epochs)))
        for g in optimizer.param_groups:
            g["lr"] = lr
        return lr


def _epochs(graph, clip, sched_name, data, n_epochs=2):
    from biapy_amd import train_engine as TE
    from biapy_amd.losses import BCEWithLogitsLoss

    m = _resunet()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, capturable=True)
    if sched_name == "onecycle":
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, total_steps=n_epochs * len(data))
    else:
        sched = _WarmupCosine(epochs=n_epochs)
    loss_fn = BCEWithLogitsLoss()
    stats = []
    for ep in range(n_epochs):
        s, _ = TE.train_one_epoch(_cfg(clip, sched_name), m, None, loss_fn, None, None, data, [opt], torch.device("cuda"), ep, lr_scheduler=[sched],
                                  loss_names=["loss"], graph=graph)
        stats.append(s)
    torch.cuda.synchronize()
    return m, opt, sched, stats


def _assert_same_training(on, off):
    worst = 0.0
    for (k, p), (_, q) in zip(on.named_parameters(), off.named_parameters()):
        if p.dim() == 5:
            err, bound = (p - q).abs().max().item(), 2e-5 * max(1.0, q.abs().max().item())
            worst = max(worst, err / bound)
            assert err <= bound, (k, err, bound)
    return worst


@pytest.mark.parametrize("ragged", [False, True], ids=["even", "ragged"])
def test_train_one_epoch_replays_under_clipping_and_onecycle(ragged):
    """7: GRADIENT_CLIP_NORM + OneCycleLR (lr AND beta1 move every step) on the replayed step - a ValueError before this feature."""
    data = _batches(3, channels_last=True)
    if ragged:
        data = data + _batches(1, B=1, seed=9, channels_last=True)
    on, opt_on, sched_on, st_on = _epochs("on", CLIP_C, "onecycle", data)
    off, opt_off, sched_off, st_off = _epochs("off", CLIP_C, "onecycle", data)
    gstep = on._bpx_graph_step[1]
    assert gstep.max_grad_norm == CLIP_C and gstep.device_betas and not hasattr(off, "_bpx_graph_step")
    norm, coef = gstep.grad_norm.tolist()
    assert norm > CLIP_C and 0 < coef < 1
    assert sched_on.last_epoch == sched_off.last_epoch == 2 * len(data)
    assert all(type(b) is float for b in opt_on.param_groups[0]["betas"])
    assert opt_on.param_groups[0]["betas"] == opt_off.param_groups[0]["betas"]
    assert float(gstep._lr.beta1s[0]) in set(OB.onecycle_beta1(steps=2 * len(data)))         # the device double is one of the schedule's host doubles
    for a, b in zip(st_on, st_off):
        assert abs(a["lr"] - b["lr"]) <= 1e-6 * b["lr"], (a["lr"], b["lr"])
        assert abs(a["loss"] - b["loss"]) <= 1e-4 * abs(b["loss"]), (a["loss"], b["loss"])
    worst = _assert_same_training(on, off)
    print(f"train_one_epoch clip+onecycle ragged={ragged}: worst err / bound = {worst:.3f}; lr meters {[s['lr'] for s in st_on]}")


def test_train_one_epoch_replays_under_a_warmup_schedule():
    """8: a per-iteration schedule that assigns group['lr'] = float before every step; with clipping as well."""
    data = _batches(3, channels_last=True)
    on, opt_on, _, st_on = _epochs("on", CLIP_C, "warmupcosine", data)
    off, _, _, st_off = _epochs("off", CLIP_C, "warmupcosine", data)
    assert on._bpx_graph_step[1].max_grad_norm == CLIP_C
    for a, b in zip(st_on, st_off):
        assert abs(a["lr"] - b["lr"]) <= 1e-6 * b["lr"], (a["lr"], b["lr"])
    assert st_on[0]["lr"] != st_on[1]["lr"]
    worst = _assert_same_training(on, off)
    print(f"train_one_epoch clip+warmupcosine: worst err / bound = {worst:.3f}")


def test_onecycle_falls_back_where_the_captured_step_cannot_follow_beta1():
    """A momentum-cycling one-cycle schedule needs the package's Adam step (beta1 on the device).  An optimizer it does not reproduce (amsgrad) is
    refused before anything is captured; one whose tensors optim.fused_step declines at capture (here a parameter that never gets a gradient)
    raises under graph="on" and trains eagerly under graph="auto" - never a RuntimeError in the middle of an epoch."""
    from biapy_amd import train_engine as TE
    from biapy_amd.losses import BCEWithLogitsLoss

    data = _batches(3, channels_last=True)

    def run(graph, **opt_kw):
        m = _resunet()
        extra = [] if opt_kw else [torch.nn.Parameter(torch.zeros(4, device=DEV))]       # in the optimizer, not in the model: p.grad stays None
        opt = torch.optim.AdamW(list(m.parameters()) + extra, lr=1e-3, capturable=True, **opt_kw)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, total_steps=len(data))
        TE.train_one_epoch(_cfg(CLIP_C, "onecycle"), m, None, BCEWithLogitsLoss(), None, None, data, [opt], torch.device("cuda"), 0,
                           lr_scheduler=[sched], loss_names=["loss"], graph=graph)
        torch.cuda.synchronize()
        return m, sched

    with pytest.raises(ValueError, match=r"^graph='on'"):
        run("on", amsgrad=True)
    with pytest.raises(ValueError, match=r"^graph='on'"):
        run("on")
    auto, sched = run("auto")
    off, _ = run("off")
    assert sched.last_epoch == len(data)
    _assert_same_training(auto, off)

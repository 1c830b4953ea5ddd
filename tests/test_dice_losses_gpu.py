"""The multi-channel Dice / Dice + CE losses on the device (biapy_amd/losses.py, bpx_dice_*): the loss, every gradient element and the sums within
the bounds tests/loss_bounds.py derives from the kernels' operations around the fp64 reference; the degenerate batches; run-to-run bit equality;
3- and 8-class ResUNets trained with DiceCELoss against the fp32 oracle network; graph replay against the eager step."""
import copy

import pytest
import torch

import loss_bounds as LB
from test_class_heads_gpu import CURVE_TOL, _blob_batches, _labels, _record_diag, _small

pytestmark = pytest.mark.gpu

DEV = "cuda"
WEIGHTS = {2: [0.3, 1.7], 3: [0.2, 0.5, 0.3], 5: [1.0, 2.0, 0.5, 0.25, 4.0], 8: [1.0, 2.0, 0.5, 0.25, 4.0, 1.0, 3.0, 0.1]}
MIXES = ((0.0, 1.0), (1.0, 0.0), (0.5, 2.0))          # (w_ce, w_dice): pure Dice, pure CE weight, mixed
G_UP = 1.7                                            # the upstream gradient the backward reads on the device


def _check(rows):
    for r in rows:
        _record_diag(f"dice_losses[{r['name']}] err/bound = {r['err']:.3e} {r['extra']}")
    bad = [r for r in rows if not r["ok"]]
    assert not bad, bad


def _blocks(vox):
    from biapy_amd import _lib as L
    return L.lib.bpx_dice_blocks(vox)


def _loss_module(C, w_ce, w_dice, batch_dice, weight):
    from biapy_amd import losses as Ls
    if w_ce == 0.0 and w_dice == 1.0 and weight is None:
        return Ls.DiceLoss(batch_dice)
    kw = dict(class_rebalance="manual", class_weights=weight) if weight is not None else {}
    return Ls.DiceCELoss(w_ce, w_dice, num_classes=C, batch_dice=batch_dice, **kw)


def _device_run(lf, z, t):
    from biapy_amd import losses as Ls
    zd = z.to(DEV).requires_grad_(True)
    loss = lf(zd, t.to(DEV))
    sums = Ls._last_dice_sums.clone()
    (loss * G_UP).backward()
    torch.cuda.synchronize()
    return loss.detach(), zd.grad.detach(), sums


def _run_case(name, z, t, class_mode, batch_dice, weight, w_ce, w_dice, shape=None):
    """One loss call on the device, twice: bit-identical, and within the bounds around the fp64 reference (evaluated on the device in float64)."""
    lf = _loss_module(z.shape[1], w_ce, w_dice, batch_dice, weight)
    zs, ts = (z, t) if shape is None else (z.reshape(z.shape[:2] + shape), t.reshape(t.shape[:2] + shape))
    loss, grad, sums = _device_run(lf, zs, ts)
    loss2, grad2, sums2 = _device_run(lf, zs, ts)
    assert torch.equal(loss.view(1).view(torch.int32), loss2.view(1).view(torch.int32)) and torch.equal(grad.view(torch.int32), grad2.view(torch.int32)) \
        and torch.equal(sums, sums2), f"{name}: two runs differ"
    ref = LB.reference(z.to(DEV), t.to(DEV), w_ce=w_ce, w_dice=w_dice, batch_dice=batch_dice, weight=weight, g=G_UP)
    bnd = LB.bounds(ref, _blocks(z.shape[2]))
    _check(LB.check(name, loss, grad.reshape(z.shape), sums, ref, bnd))
    return loss


@pytest.mark.parametrize("V", [350003, 350000], ids=["ragged", "aligned"])
@pytest.mark.parametrize("batch_dice", [True, False], ids=["batch", "per-sample"])
@pytest.mark.parametrize("C", [2, 3, 5, 8])
def test_class_mode_within_derived_bounds(C, batch_dice, V):
    """N = 3 samples of 350003 voxels (the grid wraps, dword loads) and of 350000 (16-byte loads); 10 % ignored voxels, 2 % labels out of range;
    with and without class weights; pure Dice, pure CE weight and mixed."""
    from biapy_amd import losses as Ls
    z, lab = LB.class_fixture(torch.Generator().manual_seed(100 + C), 3, C, V, ignored=0.1, out_of_range=0.02)
    share, present = LB.fixture_condition(lab, C)
    assert share >= 0.85 and present, (share, present)
    for weight in (None, WEIGHTS[C]):
        for w_ce, w_dice in MIXES:
            if weight is not None and w_ce == 0.0:
                continue                                         # class weights act on the CE term only: nothing new without it
            tag = f"class C{C} {'batch' if batch_dice else 'per-sample'} V{V} w_ce{w_ce:g} w_dice{w_dice:g}{' weighted' if weight else ''}"
            _run_case(tag, z, lab, True, batch_dice, weight, w_ce, w_dice)
    assert Ls.last_label_faults() == int(((lab != -100) & ((lab < 0) | (lab >= C))).sum().item()) > 0
    lf = Ls.DiceLoss(batch_dice)
    lf(z.to(DEV), lab.to(DEV))
    Ls.soft_dice_per_class(z.to(DEV), torch.zeros_like(lab).to(DEV))          # another call in between does not change the object's own count
    assert Ls.last_label_faults() == 0 and Ls.last_label_faults(lf) == int(((lab != -100) & ((lab < 0) | (lab >= C))).sum().item())


@pytest.mark.parametrize("V", [350003, 350000], ids=["ragged", "aligned"])
@pytest.mark.parametrize("batch_dice", [True, False], ids=["batch", "per-sample"])
@pytest.mark.parametrize("C", [2, 3, 5, 8])
def test_channel_mode_within_derived_bounds(C, batch_dice, V):
    z, t = LB.channel_fixture(torch.Generator().manual_seed(200 + C), 3, C, V)
    for w_ce, w_dice in MIXES:
        tag = f"channel C{C} {'batch' if batch_dice else 'per-sample'} V{V} w_ce{w_ce:g} w_dice{w_dice:g}"
        _run_case(tag, z, t, False, batch_dice, None, w_ce, w_dice)


def test_channel_mode_equals_the_pinned_oracle():
    """DiceLoss / DiceCELoss on a 4-channel sigmoid head against oracle.loss_oracle.dice / dice_ce themselves (fp32 on the CPU), 5-d shapes."""
    from biapy_amd import losses as Ls
    from oracle import loss_oracle as LO
    z, t = LB.channel_fixture(torch.Generator().manual_seed(7), 2, 4, 12 * 20 * 24)
    z, t = z.reshape(2, 4, 12, 20, 24), t.reshape(2, 4, 12, 20, 24)
    for lf, ref in ((Ls.DiceLoss(), lambda a: LO.dice(a, t)), (Ls.DiceLoss(False), lambda a: LO.dice(a, t, batch_dice=False)),
                    (Ls.DiceCELoss(0.7, 1.3), lambda a: LO.dice_ce(a, t, 0.7, 1.3))):
        zc = z.clone().requires_grad_(True)
        lr = ref(zc)
        lr.backward()
        zd = z.to(DEV).requires_grad_(True)
        ld = lf(zd, t.to(DEV))
        ld.backward()
        assert abs(ld.item() - lr.item()) < 2e-6 * max(1.0, abs(lr.item()))
        assert (zd.grad.cpu() - zc.grad).abs().max().item() < 2e-6 * zc.grad.abs().max().item() + 1e-12


@pytest.mark.parametrize("batch_dice", [True, False], ids=["batch", "per-sample"])
def test_degenerate_batches(batch_dice):
    """An all-ignored sample inside a batch, an absent class (it contributes s / (P + s)), and the all-ignored batch: finite with w_ce = 0 (every
    dice term is s / s, the loss 0 and the gradient 0), NaN with a CE term as torch's mean reduction gives."""
    from biapy_amd import losses as Ls
    g = torch.Generator().manual_seed(300)
    V = 350003
    z, lab = LB.class_fixture(g, 3, 5, V, dead_sample=1)
    for w_ce, w_dice in MIXES:
        _run_case(f"dead sample {'batch' if batch_dice else 'per-sample'} w_ce{w_ce:g} w_dice{w_dice:g}", z, lab, True, batch_dice, None, w_ce, w_dice)
    z, lab = LB.class_fixture(g, 3, 5, V, absent=2)
    assert not bool((lab == 2).any())
    for w_ce, w_dice in MIXES:
        _run_case(f"absent class {'batch' if batch_dice else 'per-sample'} w_ce{w_ce:g} w_dice{w_dice:g}", z, lab, True, batch_dice, WEIGHTS[5] if w_ce else None, w_ce, w_dice)
    z, lab = LB.class_fixture(g, 3, 5, V, all_ignored=True)
    loss = _run_case(f"all ignored {'batch' if batch_dice else 'per-sample'} w_ce0", z, lab, True, batch_dice, None, 0.0, 1.0)
    assert torch.isfinite(loss).item()
    zd = z.to(DEV).requires_grad_(True)
    ln = Ls.DiceCELoss(1.0, 1.0, num_classes=5, batch_dice=batch_dice)(zd, lab.to(DEV))
    assert torch.isnan(ln).item()


def test_label_maps_without_a_channel_axis_dicts_and_logging():
    from biapy_amd import losses as Ls
    g = torch.Generator().manual_seed(400)
    z, lab = LB.class_fixture(g, 2, 3, 16 * 16 * 16, ignore_index=255, ignored=0.1)
    z5, l5 = z.reshape(2, 3, 16, 16, 16).to(DEV), lab.reshape(2, 1, 16, 16, 16).to(DEV)
    lf = Ls.DiceCELoss(1.0, 1.0, num_classes=3, ignore_index=255)
    a, b, c = lf(z5, l5), lf({"pred": z5}, l5), lf(z5, l5[:, 0])
    assert torch.equal(a, b) and torch.equal(a, c)
    ref = LB.reference(z.to(DEV), lab.to(DEV), w_ce=1.0, w_dice=1.0, ignore_index=255)
    assert abs(a.item() - ref["loss"].item()) < 1e-5
    d = Ls.soft_dice_per_class(z5, l5, ignore_index=255)
    assert d.shape == (3,) and d.is_cuda and (d.double() - ref["dice"][0]).abs().max().item() < 1e-5
    assert Ls.last_label_faults() == 0
    with pytest.raises(NotImplementedError):
        lf([z5, z5], l5)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [3, 8])
def test_mixed_training_with_dice_ce_follows_the_fp32_oracle_loss_curve(classes):
    """The default training mode (fp16 forward, bf16 gradients) of a ResUNet (fm 16-32-64) at 2 x 32^3 with DiceCELoss(num_classes) on its softmax
    head: 30 AdamW steps on the device and as the fp32 oracle network with loss_bounds.autograd_loss (checked against the fp64 reference on the
    CPU) from the same weights on the same batches; the worst relative loss gap stays under the existing curve bar."""
    from biapy_amd.losses import DiceCELoss
    from biapy_amd.resunet import ResUNet
    from oracle import net_oracle

    fm, S, steps = [16, 32, 64], 32, 30
    torch.manual_seed(21 + classes)
    m = ResUNet(**_small(fm, S=S, output_channels=[classes], head_activations=["ce_softmax"], compute_dtype=torch.float16)).to(DEV).train()
    cpu_p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.named_parameters()}
    batches = _blob_batches(torch.Generator().manual_seed(22 + classes), 3, 2, S, classes)
    lf = DiceCELoss(1.0, 1.0, num_classes=classes, ndim=3)
    opt_d = torch.optim.AdamW(m.parameters(), lr=1e-3)
    opt_c = torch.optim.AdamW(list(cpu_p.values()), lr=1e-3)
    old = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, old)))
    try:
        cd, cc = [], []
        for it in range(steps):
            x, t = batches[it % len(batches)]
            opt_d.zero_grad(set_to_none=True)
            ld = lf(m(x.to(DEV)), t.to(DEV))
            ld.backward()
            opt_d.step()
            opt_c.zero_grad(set_to_none=True)
            lc = LB.autograd_loss(net_oracle.resunet_forward(cpu_p, x, fm), t, w_ce=1.0, w_dice=1.0)
            lc.backward()
            opt_c.step()
            cd.append(ld.item())
            cc.append(lc.item())
    finally:
        torch.set_num_threads(old)
    cd_, cc_ = torch.tensor(cd), torch.tensor(cc)
    rel = ((cd_ - cc_).abs() / cc_).max().item()
    print("mixed-mode Dice+CE loss curve (device):", [round(v, 4) for v in cd])
    print("fp32 oracle loss curve          (cpu):", [round(v, 4) for v in cc])
    _record_diag(f"loss_curve[{classes}-class ResUNet mixed, DiceCELoss vs fp32 oracle, fm 16-32-64, 2x{S}^3, {steps} steps].worst_rel_gap = {rel:.3e} (bar {CURVE_TOL:g})")
    assert cc_[-3:].mean() < cc_[:3].mean() and cd_[-3:].mean() < cd_[:3].mean(), (cc, cd)
    assert rel < CURVE_TOL, (rel, cc, cd)


@pytest.mark.parametrize("batch_dice", [True, False], ids=["batch", "per-sample"])
def test_graphed_train_step_with_dice_ce_equals_the_eager_step(batch_dice):
    """GraphedTrainStep with DiceCELoss(num_classes=8): after several replays a replayed step gives the eager step's loss and gradients bit for bit
    (lr = 0: both models keep the same weights)."""
    from biapy_amd.graphs import GraphedTrainStep
    from biapy_amd.losses import DiceCELoss
    from biapy_amd.resunet import ResUNet

    torch.manual_seed(33)
    m1 = ResUNet(**_small([16, 32, 64], S=32, output_channels=[8], head_activations=["ce_softmax"])).to(DEV).train()
    m2 = copy.deepcopy(m1)
    g = torch.Generator().manual_seed(34)
    x = torch.randn(2, 1, 32, 32, 32, generator=g).to(DEV)
    t = _labels(g, 2, 8, (32, 32, 32)).to(DEV)
    lf = DiceCELoss(1.0, 1.0, num_classes=8, ndim=3, batch_dice=batch_dice, class_rebalance="manual", class_weights=WEIGHTS[8])
    o1 = torch.optim.AdamW(m1.parameters(), lr=0.0, capturable=True)
    o2 = torch.optim.AdamW(m2.parameters(), lr=0.0, capturable=True)
    gs = GraphedTrainStep(m2, lf, o2, x, t, warmup=2)
    for _ in range(4):
        l2 = gs().clone()
    torch.cuda.synchronize()
    o1.zero_grad(set_to_none=True)
    l1 = lf(m1(x), t)
    l1.backward()
    torch.cuda.synchronize()
    assert torch.equal(l1.detach().view(1), l2.view(1)), (l1.item(), l2.item())
    n = 0
    for (k, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        assert p2.grad is not None and torch.equal(p1.grad, p2.grad), k
        n += 1
    assert n == len(list(m1.parameters()))

"""The one-channel BCE / Dice / Dice + CE loss (bpx_seg_loss_*), the per-channel instance losses (bpx_chan_loss_*) and the multi-class cross entropy
(bpx_softmax_ce_*) on the device: the loss, the sums and every gradient element within the bounds tests/plain_loss_bounds.py derives from the kernels'
operations around the fp64 reference (evaluated on the device), the counts exactly, every case twice and bit-identical.  The shapes are the smallest
that reach each code path: a tail only, one partial block and a tail, whole blocks, and a size at which both grid-stride loops wrap."""
import pytest
import torch

import plain_loss_bounds as PB
from test_class_heads_gpu import _record_diag

pytestmark = pytest.mark.gpu

DEV = "cuda"
G_UP = 1.7                                                    # the upstream gradient: the backward reads fp32(1.7) on the device
G32 = PB.f32(G_UP)
SMOOTH = PB.f32(1e-5)
MIXES = ((1.0, 0.0), (0.0, 1.0), (0.7, 1.3))                  # (w_ce, w_dice); the kernels receive them as floats
SEG_N = (3, 1027, 4096, 4 * 1048576 + 1203)
VOXES = (1, 1029, 512 * 1024 + 1029)
CHAN_SETS = {"bcd_mse": (PB.SPEC_BCD_MSE, (1.0, 1.0, 1.0)), "bcd_l1": (PB.SPEC_BCD_L1, (0.5, 0.25, 2.0)), "all8": (PB.SPEC_ALL8, PB.WEIGHTS_ALL8)}


def _check(family, rows):
    for r in rows:
        _record_diag(f"plain_losses[{family}: {r['name']}] err/bound = {r['err']:.3e} {r['extra']}")
    bad = [r for r in rows if not r["ok"]]
    assert not bad, bad


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _twice(run, name):
    a, b = run(), run()
    assert all(_same_bits(x, y) for x, y in zip(a, b)), f"{name}: two runs differ"
    return a


def _lib():
    from biapy_amd import _lib as L
    return L


# ---- binary ---------------------------------------------------------------------------------------------------------------------------------------------
def _seg_module(w_ce, w_dice, batch_dice=True):
    from biapy_amd import losses as Ls
    if w_dice == 0.0:
        return Ls.BCEWithLogitsLoss()
    if w_ce == 0.0:
        return Ls.DiceLoss(batch_dice)
    return Ls.DiceCELoss(w_ce, w_dice)


def _seg_run(lf, z, t, with_sums):
    """(loss, gradient[, the row of six sums]) of one loss call on device tensors z (a leaf or a view of one) and t."""
    from biapy_amd import losses as Ls
    leaf = z if z.is_leaf else z._base
    leaf.grad = None
    loss = lf(z, t)
    (loss * G_UP).backward()
    out = [loss.detach(), leaf.grad.detach().clone()]
    if with_sums:
        out.append(Ls._sums_and_loss(*Ls._prep(z.detach(), t))[0])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n", SEG_N)
def test_binary_loss_within_derived_bounds(n):
    """(1, 1, n) logits with the saturated values planted; BCE, Dice and Dice + CE; the fused passes through the loss modules and the direct
    backward entry bpx_seg_loss_bwd with coefficients formed on the host from the device's sums."""
    L = _lib()
    B = L.lib.bpx_seg_loss_blocks(n)
    z, t = PB.seg_fixture(torch.Generator().manual_seed(PB.seg_seed(n)), n)
    zd, td = z.to(DEV).requires_grad_(True), t.to(DEV)
    for w_ce, w_dice in MIXES:
        name = f"n{n} w_ce{w_ce:g} w_dice{w_dice:g}"
        loss, grad, sums = _twice(lambda: _seg_run(_seg_module(w_ce, w_dice), zd, td, True), name)
        ref = PB.seg_reference(zd.detach(), td, w_ce=PB.f32(w_ce), w_dice=PB.f32(w_dice), smooth=SMOOTH, g=G32)
        bnd = PB.seg_bounds(ref, B)
        _check("seg", PB.seg_check(name, loss, grad, sums, ref, bnd))
        # the direct entry: a, b, c in double on the host from the device's sums, rounded once
        S = sums.cpu().tolist()
        wc, wd = PB.f32(w_ce), PB.f32(w_dice)
        den = S[2] + S[3] + SMOOTH
        coef = torch.tensor([wc * G32 / n, 2.0 * wd * G32 / den, wd * G32 * (2.0 * S[1] + SMOOTH) / (den * den)], dtype=torch.float64).float().to(DEV)

        def direct():
            dz = torch.empty(n, dtype=torch.float32, device=DEV)
            L.check(L.lib.bpx_seg_loss_bwd(zd.data_ptr(), td.data_ptr(), n, coef.data_ptr(), dz.data_ptr(), L.stream_ptr()))
            torch.cuda.synchronize()
            return [dz]

        (dz,) = _twice(direct, name + " direct")
        _check("seg", PB.seg_check(name + " bpx_seg_loss_bwd", None, dz, None, ref, bnd))


def test_the_cheap_log_form_per_element():
    """seg_log1p_unit read back element by element.  With n = 1, t = 0 and z <= 0 the tail thread's term is 0 - (-0) + log2(fl(1 + en)) ln2, and every
    later addition (shuffles, waves, the double sum) adds zeros: the first of the six sums IS the kernel's log(1 + exp(z)) of that element.  It stays
    within the bound derived from its three roundings and expf's error (at most 5.8 u = 3.5e-7 at z = 0), which no sum over many elements can show."""
    import math

    from biapy_amd import losses as Ls
    worst, worst_abs = 0.0, 0.0
    td = torch.zeros(1, 1, 1, device=DEV)
    for z in (-0.0, -2.0 ** -10, -0.01, -0.1, -0.3, -0.5, -0.7, -1.0, -1.5, -2.0, -3.0, -5.0, -8.0, -12.0, -15.0, -16.5, -17.0, -20.0, -30.0, -88.0, -104.0):
        got = Ls._sums_and_loss(torch.full((1, 1, 1), z, device=DEV), td)[0][0].item()
        en = math.exp(z)
        lg = math.log1p(en)
        bound = PB.seg_log_bound(en, lg) + PB.FLOOR
        worst, worst_abs = max(worst, abs(got - lg) / bound), max(worst_abs, abs(got - lg))
        assert abs(got - lg) <= bound, (z, got, lg, bound)
    _record_diag(f"plain_losses[seg: seg_log1p_unit per element] err/bound = {worst:.3e} worst absolute error {worst_abs:.3e}")


@pytest.mark.parametrize("shape", [(3, 1, 5, 7, 9), (3, 1, 6, 10, 12)], ids=["misaligned", "aligned"])
def test_per_sample_dice_on_batch_slices(shape):
    """DiceLoss(batch_dice=False) on a one-channel head runs the fused passes once per sample on the slices z[i:i + 1]: with 5 x 7 x 9 = 315 voxels
    sample 1 starts 1260 bytes into the batch - no multiple of 16 - and the kernels' 16-byte loads need the copy _prep makes (without it the loss, jaccard_index and
    hard_dice raised "BpxError: bpx_seg_loss_sums: logits and target must be 16-byte aligned" on that sample; 6 x 10 x 12 = 720 voxels never did).  The
    IoU and hard-Dice metrics read the same slices."""
    from biapy_amd import losses as Ls
    L = _lib()
    V = shape[2] * shape[3] * shape[4]
    z, t = PB.seg_fixture(torch.Generator().manual_seed(20 + V), V, N=3)
    zd, td = z.reshape(shape).to(DEV).requires_grad_(True), t.reshape(shape).to(DEV)
    assert (zd[1:2].data_ptr() % 16 != 0) == (V % 4 != 0)
    lf = Ls.DiceLoss(batch_dice=False)
    loss, grad = _twice(lambda: _seg_run(lf, zd, td, False), f"per-sample {shape}")
    ref = PB.seg_reference(z.to(DEV), t.to(DEV), w_ce=0.0, w_dice=1.0, smooth=SMOOTH, batch_dice=False, g=G32)
    bnd = PB.seg_bounds(ref, L.lib.bpx_seg_loss_blocks(V), gup_rel=2.0)
    _check("seg", PB.seg_check(f"per-sample V{V}", loss, grad, None, ref, bnd))
    for i in range(3):
        one = PB.seg_reference(z[i:i + 1].to(DEV), t[i:i + 1].to(DEV), w_ce=1.0, w_dice=0.0)
        a, o = one["counts"].tolist()
        assert Ls.jaccard_index(zd.detach()[i:i + 1], td[i:i + 1]).item() == pytest.approx(a / max(o, 1.0), rel=1e-6)
        assert Ls.hard_dice(zd.detach()[i:i + 1], td[i:i + 1]).item() == pytest.approx((2 * a + 1e-5) / (a + o + 1e-5), rel=1e-6)


def test_binary_loss_on_bf16_logits():
    """bf16 logits are widened exactly: the reference is taken on the stored values; the gradient comes back in bf16, so its bound gains that rounding."""
    n = 1027
    z, t = PB.seg_fixture(torch.Generator().manual_seed(30), n)
    zd, td = z.bfloat16().to(DEV).requires_grad_(True), t.to(DEV)
    assert PB.seg_fixture_condition(zd.detach().float().cpu())[0] == 0
    loss, grad = _twice(lambda: _seg_run(_seg_module(0.7, 1.3), zd, td, False), "bf16")
    assert grad.dtype == torch.bfloat16
    ref = PB.seg_reference(zd.detach().float(), td, w_ce=PB.f32(0.7), w_dice=PB.f32(1.3), smooth=SMOOTH, g=G32)
    bnd = PB.seg_bounds(ref, _lib().lib.bpx_seg_loss_blocks(n), grad_unit=PB.BF16)
    _check("seg", PB.seg_check("bf16 logits n1027", loss, grad, None, ref, bnd))


def test_binary_loss_on_a_permuted_view():
    """A non-contiguous view (two axes swapped) of 79 x 13 = 1027 elements: the kernels see its contiguous copy, the gradient returns through the view."""
    n = 1027
    z, t = PB.seg_fixture(torch.Generator().manual_seed(31), n)
    base = z.reshape(1, 1, 79, 13).to(DEV).requires_grad_(True)
    zv, tv = base.permute(0, 1, 3, 2), t.reshape(1, 1, 79, 13).to(DEV).permute(0, 1, 3, 2)
    assert not zv.is_contiguous()
    loss, gbase = _twice(lambda: _seg_run(_seg_module(0.7, 1.3), zv, tv, False), "permuted")
    ref = PB.seg_reference(zv.detach().reshape(1, 1, n), tv.reshape(1, 1, n), w_ce=PB.f32(0.7), w_dice=PB.f32(1.3), smooth=SMOOTH, g=G32)
    bnd = PB.seg_bounds(ref, _lib().lib.bpx_seg_loss_blocks(n))
    _check("seg", PB.seg_check("permuted view n1027", loss, gbase.permute(0, 1, 3, 2).reshape(1, 1, n), None, ref, bnd))


# ---- per-channel losses ----------------------------------------------------------------------------------------------------------------------------------
def _chan_module(spec, weights):
    from biapy_amd.losses import InstanceChannelsLoss
    names = ["B", "C", "D", "F", "P", "T", "Dn", "Dc"][: len(spec)]
    lf = InstanceChannelsLoss(channel_weights=weights, out_channels=names, losses_to_use=[k for k, _ in spec],
                              head_activations=["ce_sigmoid" if k == "bce" else a for k, a in spec]).to(DEV)
    assert lf.codes == PB.chan_codes(spec)
    return lf


@pytest.mark.parametrize("vox", VOXES)
@pytest.mark.parametrize("name", list(CHAN_SETS))
def test_channel_losses_within_derived_bounds(name, vox):
    """N = 2; BCE / MSE / L1 channels behind linear, tanh and sigmoid activations; z = +-20 on the tanh channels and z == t on the linear L1 channel
    planted.  The fused passes through InstanceChannelsLoss, the per-channel sums through bpx_chan_loss_sums, and the direct backward entry
    bpx_chan_loss_bwd with coef[c] = g w_c / (N vox)."""
    L = _lib()
    spec, weights = CHAN_SETS[name]
    N, C = 2, len(spec)
    nb = L.lib.bpx_chan_loss_blocks(vox)
    z, t, planted = PB.chan_fixture(torch.Generator().manual_seed(PB.chan_seed(vox)), N, spec, vox)
    zd, td = z.to(DEV).requires_grad_(True), t.to(DEV)
    lf = _chan_module(spec, weights)

    def run():
        zd.grad = None
        loss = lf(zd, td)
        (loss * G_UP).backward()
        part = torch.empty((N, C, nb), dtype=torch.float32, device=DEV)
        L.check(L.lib.bpx_chan_loss_sums(zd.data_ptr(), td.data_ptr(), N, C, vox, lf.codes, part.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
        return [loss.detach(), zd.grad.detach().clone(), part]

    tag = f"{name} vox{vox}"
    loss, grad, part = _twice(run, tag)
    ref = PB.chan_reference(zd.detach(), td, spec, weights, g=G32)
    bnd = PB.chan_bounds(ref, nb)
    _check("chan", PB.chan_check(tag, loss, grad, part.double().sum((0, 2)), ref, bnd))
    assert bool((grad[planted.to(DEV)] == 0).all())
    coef = (G32 * ref["w"] / (float(N) * float(vox))).float()

    def direct():
        dz = torch.empty_like(zd)
        L.check(L.lib.bpx_chan_loss_bwd(zd.data_ptr(), td.data_ptr(), N, C, vox, lf.codes, coef.data_ptr(), dz.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
        return [dz]

    (dz,) = _twice(direct, tag + " direct")
    _check("chan", PB.chan_check(tag + " bpx_chan_loss_bwd", None, dz, None, ref, PB.chan_bounds(ref, nb, k_units=1.0)))


# ---- softmax cross entropy ---------------------------------------------------------------------------------------------------------------------------------
def _ce_run(z, lab, w, ignore_index):
    from biapy_amd import losses as Ls
    z.grad = None
    loss = Ls._SoftmaxCEFn.apply(z, lab, w, ignore_index)
    (loss * G_UP).backward()
    sums = Ls._softmax_ce_sums(z.detach(), lab, ignore_index, w)[0]
    torch.cuda.synchronize()
    return [loss.detach(), z.grad.detach().clone(), sums]


@pytest.mark.parametrize("ignore_index", [-100, 255])
@pytest.mark.parametrize("C,vox", [(C, v) for C in (2, 3, 5, 8) for v in VOXES if not (C == 8 and v == 1)])
def test_softmax_ce_within_derived_bounds(C, vox, ignore_index):
    """N = 2; 10 % ignored voxels, 2 % labels out of range, the last class absent, exact two- and three-way ties of the maximum; with and without
    class weights.  Loss, S_nll, S_w and every gradient element within bounds; the 3 x C counts exact; the gradient +-0 wherever nothing counts."""
    L = _lib()
    nb = L.lib.bpx_softmax_ce_blocks(vox)
    z, lab, ties = PB.ce_fixture(torch.Generator().manual_seed(PB.ce_seed(C)), 2, C, vox, ignore_index)
    zd, ld = z.to(DEV).requires_grad_(True), lab.to(DEV)
    for weight in (None, PB.CE_WEIGHTS[C]):
        w = None if weight is None else torch.tensor(weight, dtype=torch.float32, device=DEV)
        tag = f"C{C} vox{vox} ignore{ignore_index}{' weighted' if weight else ''}"
        loss, grad, sums = _twice(lambda: _ce_run(zd, ld, w, ignore_index), tag)
        ref = PB.ce_reference(zd.detach(), ld, weight, ignore_index, g=G32)
        _check("ce", PB.ce_check(tag, loss, grad, sums, ref, PB.ce_bounds(ref, nb)))


def test_softmax_ce_through_the_wrapper_and_all_ignored():
    """CrossEntropyLoss_wrapper(num_classes=3) gives the same bits as the function it wraps; an all-ignored batch gives NaN and an all-zero gradient."""
    from biapy_amd import losses as Ls
    z, lab, _ = PB.ce_fixture(torch.Generator().manual_seed(103), 2, 3, 1029, 255)
    zd, ld = z.reshape(2, 3, 3, 7, 49).to(DEV).requires_grad_(True), lab.reshape(2, 1, 3, 7, 49).to(DEV)
    lw = Ls.CrossEntropyLoss_wrapper(num_classes=3, ndim=3, class_rebalance="manual", class_weights=PB.CE_WEIGHTS[3], ignore_index=255)(zd, ld)
    (lw * G_UP).backward()
    gw = zd.grad.clone()
    loss, grad, _ = _ce_run(zd, ld, torch.tensor(PB.CE_WEIGHTS[3], dtype=torch.float32, device=DEV), 255)
    assert _same_bits(lw.detach(), loss) and _same_bits(gw, grad)
    dead = torch.full_like(ld, 255.0)
    loss, grad, sums = _twice(lambda: _ce_run(zd, dead, None, 255), "all ignored")
    assert torch.isnan(loss).item() and bool((grad == 0).all()) and sums[1:].abs().max().item() == 0.0

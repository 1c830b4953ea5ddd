"""The multi-channel Dice / Dice + CE losses (biapy_amd/losses.py, csrc/losses.hip) in float64 - value, closed-form gradient, the sums - and
per-element error bounds of what the device may differ by, derived from the kernels' operations in the manner of tests/norm_bounds.py:

    |got - ref| <= (error of every fp32 term pushed through on absolute values) + chain 2^-24 sum|terms| + 2^-24 |ref| (+ a floor of 2^-126)

Nothing here is fitted to a measured value.  What enters (u = 2^-24, the fp32 unit roundoff):

* expf, logf, log1pf: 2 ulp = 4 u relative (ocml documents 1 ulp for expf / logf and 2 ulp for log1pf); a division: 2.5 ulp = 5 u.
* softmax of a voxel (dice_softmax): d_c = z_c - max rounds once (u |d_c|, which is the relative error it leaves in e_c), e_c = expf(d_c),
  se = sum e_c is C - 1 additions of positive terms, inv = 1 / se, p_c = e_c inv rounds once:
      |dp_c| <= u p_c (|d_c| + 4 + (maxd + 4 + C - 1) + 5 + 1) <= u p_c (2 maxd + C + 13),   maxd = max_c |d_c|.
* sigmoid (dice_sigmoid): en = expf(-|z|) (4 u), 1 + en rounds once, r = 1 / (1 + en) (5 u), p = r or en r (one more rounding and en's error):
      |dp| <= 16 u p.
* a row of sums: a thread adds n_t terms in fp32 - n_t = 4 ceil(voxels / 4 / (256 blocks)) on the 16-byte path (voxels % 4 == 0),
  ceil(voxels / (256 blocks)) on the dword path, with `blocks` = bpx_dice_blocks(voxels) -, then six shuffle levels and two additions across the
  four waves: chain = n_t + 8.  The rows are added in double in the finish kernel: (rows + 16) 2^-53 of the absolute sum.
* the finish kernel forms dice, the loss and the coefficients in double from the device's sums, so their error is the sums' error pushed through
  (as an interval: numerator up, denominator down) plus one rounding to fp32; the backward kernel's operations are counted where its bound is built.
"""
from __future__ import annotations

import torch

from conv_bounds import U32, compare  # noqa: F401

U64 = 2.0 ** -53
FLOOR = 2.0 ** -126
TRANS, DIV = 4.0, 5.0            # expf / logf / log1pf and a division, in units of u
K_SIG = 16.0
from biapy_amd.losses import DICE_ROW as ROW, DR_CE, DR_CNT, DR_FAULT, DR_I, DR_P, DR_T, DR_W  # noqa: E402  (the layout is named once, there)
FAULTS = ("ignored_in_P", "present_classes_only", "no_smooth", "batch_swapped", "no_jacobian_sum", "weights_on_dice")


def chain_length(vox: int, blocks: int) -> int:
    n_t = 4 * -(-(vox // 4) // (256 * blocks)) if vox % 4 == 0 else -(-vox // (256 * blocks))
    return n_t + 8


def _flat(z, t):
    N, C = z.shape[0], z.shape[1]
    z = z.double().reshape(N, C, -1)
    class_mode = t.numel() != z.numel()          # a label map has one value per voxel, a channel target C
    t = t.double().reshape(N, -1, z.shape[2])
    return z, t, class_mode


def _red(x, batch):
    """Sum over the voxels, and over the samples for batch_dice: (N, C, V) -> (N or 1, C)."""
    s = x.sum(2)
    return s.sum(0, keepdim=True) if batch else s


def reference(z, t, *, w_ce, w_dice, smooth=1e-5, batch_dice=True, ignore_index=-100, weight=None, g=1.0, fault=None):
    """The loss in float64 on the fp32 operands as stored.  z (N, C, *space); t of the same shape (channel mode) or a label map (N, 1, *space) /
    (N, *space) (class mode).  Returns a dict: loss, grad (N, C, V), sums (28: the batch totals in the kernels' columns), and the intermediates the
    bounds need.  `fault`: one of FAULTS - a wrong implementation, for the comparator's self-test."""
    assert fault is None or fault in FAULTS
    z, t, class_mode = _flat(z, t)
    N, C, V = z.shape
    dev = z.device
    s = 0.0 if fault == "no_smooth" else float(smooth)
    batch = (not batch_dice) if fault == "batch_swapped" else bool(batch_dice)
    w = torch.ones(C, dtype=torch.float64, device=dev) if weight is None else torch.as_tensor(weight, dtype=torch.float64, device=dev)
    out = dict(class_mode=class_mode, N=N, C=C, V=V, batch=batch)
    if class_mode:
        lab = t[:, 0].long()
        in_range = (lab >= 0) & (lab < C)
        counted = in_range & (lab != ignore_index)
        oh = torch.nn.functional.one_hot(torch.where(counted, lab, torch.zeros_like(lab)), C).permute(0, 2, 1).bool() & counted[:, None]
        p = torch.softmax(z, 1)
        cm = counted[:, None].double()
        pP = p if fault == "ignored_in_P" else p * cm
        ohd = oh.double()
        I, P, T = _red(p * ohd, batch), _red(pP, batch), _red(ohd, batch)
        lse = torch.logsumexp(z, 1)
        nll = lse - (z * ohd).sum(1)
        wy = (w[None, :, None] * ohd).sum(1)
        S_ce, S_w = (wy * nll).sum(), wy.sum()
        ce = S_ce / S_w
        kce = (w_ce / S_w) if w_ce != 0 else torch.zeros((), dtype=torch.float64, device=dev)
        faults = (~in_range & (lab != ignore_index)).double().sum()
        out.update(counted=counted, oh=oh, lse=lse, nll=nll, wy=wy, cnt=counted.double().sum(), faults=faults)
    else:
        p = torch.sigmoid(z)
        I, P, T = _red(p * t, batch), _red(p, batch), _red(t, batch)
        bce = torch.clamp(z, min=0) - z * t + torch.log1p(torch.exp(-z.abs()))
        S_ce, S_w = bce.sum(), torch.zeros((), dtype=torch.float64, device=dev)
        ce = S_ce / float(N * C * V)
        kce = torch.full((), w_ce / float(N * C * V), dtype=torch.float64, device=dev)
        out.update(bce=bce, cnt=torch.zeros((), dtype=torch.float64, device=dev), faults=torch.zeros((), dtype=torch.float64, device=dev))
    U = P + T
    dice = (2 * I + s) / (U + s)
    if fault == "present_classes_only":
        present = (T > 0).double()
        M = float(present.sum().clamp_min(1).item())
        dice_mean = (dice * present).sum() / M
    else:
        present = torch.ones_like(dice)
        M = float(dice.numel())
        dice_mean = dice.sum() / M
    wd = w[None, :] if fault == "weights_on_dice" else torch.ones(1, C, dtype=torch.float64, device=dev)
    if fault == "weights_on_dice":
        dice_mean = (dice * wd).sum() / M
    loss = torch.zeros((), dtype=torch.float64, device=dev)
    if w_dice != 0:
        loss = loss + w_dice * (1 - dice_mean)
    if w_ce != 0:
        loss = loss + w_ce * ce
    a0 = w_dice * (2 * I + s) / (M * (U + s) ** 2) * present * wd
    a1 = a0 - 2 * w_dice / (M * (U + s)) * present * wd
    a0v, a1v = a0[:, :, None], a1[:, :, None]
    if class_mode:
        A = torch.where(oh, a1v, a0v)
        S = torch.zeros_like(p[:, :1]) if fault == "no_jacobian_sum" else (p * A).sum(1, keepdim=True)
        pmask = cm if fault != "ignored_in_P" else torch.ones_like(cm)
        grad = g * (p * (A - S) * pmask + kce * wy[:, None] * (p - ohd) * cm)
    else:
        A = a0v + t * (a1v - a0v)
        grad = g * (A * p * (1 - p) + kce * (p - t))
    sums = torch.zeros(ROW, dtype=torch.float64, device=dev)
    sums[DR_I:DR_I + C], sums[DR_P:DR_P + C], sums[DR_T:DR_T + C] = I.sum(0), P.sum(0), T.sum(0)
    sums[DR_CE], sums[DR_W], sums[DR_FAULT], sums[DR_CNT] = S_ce, S_w, out["faults"], out["cnt"]
    out.update(z=z, t=t, p=p, I=I, P=P, T=T, U=U, dice=dice, M=M, s=s, a0=a0, a1=a1, A=A, kce=kce, loss=loss, grad=grad, sums=sums, S_ce=S_ce, S_w=S_w,
               w=w, w_ce=float(w_ce), w_dice=float(w_dice), g=float(g), ce=ce)
    return out


def autograd_loss(z, lab, *, w_ce, w_dice, smooth=1e-5, batch_dice=True, weight=None, ignore_index=-100):
    """The class mode written with torch's own operators (softmax, one_hot, F.cross_entropy) in the dtype of z, differentiable: independent of
    reference(), which tests/test_dice_losses_cpu.py checks against it in float64; the training tests use it in fp32 as the oracle's loss.
    z (N, C, *space), lab (N, 1, *space)."""
    import torch.nn.functional as F
    C = z.shape[1]
    y = lab[:, 0].long()
    counted = (y != ignore_index) & (y >= 0) & (y < C)
    oh = F.one_hot(torch.where(counted, y, torch.zeros_like(y)), C).movedim(-1, 1).to(z.dtype) * counted[:, None]
    p = torch.softmax(z, 1) * counted[:, None]
    ax = ([0] if batch_dice else []) + list(range(2, z.dim()))
    dice = (2 * (p * oh).sum(ax) + smooth) / (p.sum(ax) + oh.sum(ax) + smooth)
    loss = w_dice * (1 - dice.mean()) if w_dice != 0 else z.new_zeros(())
    if w_ce != 0:
        wt = None if weight is None else torch.as_tensor(weight, dtype=z.dtype, device=z.device)
        loss = loss + w_ce * F.cross_entropy(z, torch.where(counted, y, torch.full_like(y, -100)), weight=wt, ignore_index=-100)
    return loss


def _ratio_bound(num, dnum, den, dden):
    """|(num' / den') - num / den| for |num' - num| <= dnum, |den' - den| <= dden, num >= 0, den > dden >= 0: the interval's ends."""
    r = num / den
    hi = (num + dnum) / (den - dden)
    lo = (num - dnum).clamp_min(0) / (den + dden)
    return torch.maximum(hi - r, r - lo)


def bounds(ref, blocks: int):
    """Bounds of the device's sums (28), loss (0-d) and gradient (N, C, V) around `ref` (a reference() result without a fault)."""
    z, t, p = ref["z"], ref["t"], ref["p"]
    N, C, V, batch, cls = ref["N"], ref["C"], ref["V"], ref["batch"], ref["class_mode"]
    chain = chain_length(V, blocks)
    rows = blocks * (N if batch else 1)
    g, w_ce, w_dice, M, s = abs(ref["g"]), abs(ref["w_ce"]), abs(ref["w_dice"]), ref["M"], ref["s"]

    def sum_bound(term, eterm):            # the error of the reduced sum of non-negative terms with element errors eterm
        return _red(eterm, batch) + (chain * U32 + (rows + 16) * U64) * _red(term.abs() + eterm, batch)

    if cls:
        oh, counted = ref["oh"], ref["counted"]
        ohd, cm = oh.double(), counted[:, None].double()
        maxd = z.max(1).values - z.min(1).values                               # (N, V)
        dp = U32 * (2 * maxd[:, None] + C + 13) * p
        dI, dP, dT = sum_bound(p * ohd, dp * ohd), sum_bound(p * cm, dp * cm), sum_bound(ohd, torch.zeros_like(ohd))
        lse, nll, wy = ref["lse"], ref["nll"], ref["wy"]
        m = z.max(1).values
        k_se = maxd + TRANS + C - 1
        e_nll = U32 * wy * (k_se + TRANS * (lse - m).abs() + lse.abs() + 2 * nll.abs())
        tot = lambda x: x.sum()
        dS_ce = tot(e_nll) + (chain * U32 + (N * blocks + 16) * U64) * tot((wy * nll).abs() + e_nll)
        dS_w = (chain * U32 + (N * blocks + 16) * U64) * tot(wy)
    else:
        dp = K_SIG * U32 * p
        dI, dP, dT = sum_bound(p * t, dp * t.abs() + U32 * (p * t).abs()), sum_bound(p, dp), sum_bound(t, torch.zeros_like(t))
        bce = ref["bce"]
        e_bce = U32 * (2 * z.abs() + 3 * (z * t).abs() + 8)
        dS_ce = e_bce.sum() + (chain * U32 + (N * blocks + 16) * U64) * (bce.abs() + e_bce).sum()
        dS_w = torch.zeros_like(dS_ce)
    I, U = ref["I"], ref["U"]
    dU = dP + dT
    num, den = 2 * I + s, U + s
    ddice = _ratio_bound(num, 2 * dI, den, dU) if s > 0 else torch.zeros_like(I)
    ddice = torch.where(den > dU, ddice, torch.full_like(ddice, float("inf"))) + 8 * U64
    # sums (the batch totals)
    sb = torch.zeros(ROW, dtype=torch.float64, device=z.device)
    sb[DR_I:DR_I + C], sb[DR_P:DR_P + C], sb[DR_T:DR_T + C] = dI.sum(0), dP.sum(0), dT.sum(0)
    sb[DR_CE], sb[DR_W] = dS_ce, dS_w
    sb = sb + FLOOR
    # loss
    S_ce, S_w = ref["S_ce"], ref["S_w"]
    if cls:
        dce = _ratio_bound(S_ce.abs(), dS_ce, S_w, dS_w) if (w_ce != 0 and float(S_w) > 0) else torch.zeros_like(dS_ce)
        kce = ref["kce"].abs()
        dkce = (kce * dS_w / (S_w - dS_w) + U32 * kce) if (w_ce != 0 and float(S_w) > 0) else torch.zeros_like(dS_ce)
    else:
        dce = dS_ce / float(N * C * V)
        kce = ref["kce"].abs()
        dkce = U32 * kce
    loss_b = U32 * ref["loss"].abs() + FLOOR + 16 * U64 * (w_ce * ref["ce"].abs() if w_ce != 0 else 0.0) + 16 * U64 * w_dice
    if w_dice != 0:
        loss_b = loss_b + w_dice * ddice.sum() / M
    if w_ce != 0:
        loss_b = loss_b + w_ce * dce
    # coefficients: a0 = w_dice num / (M den^2), a1 = a0 - 2 w_dice / (M den), each formed in double and rounded to fp32 once
    a0, a1 = ref["a0"].abs(), ref["a1"].abs()
    safe = (den - dU).clamp_min(1e-300)
    da0_x = torch.maximum(w_dice * (num + 2 * dI) / (M * safe ** 2) - a0, a0 - w_dice * (num - 2 * dI).clamp_min(0) / (M * (den + dU) ** 2))
    db = 2 * w_dice / (M * den) * dU / safe
    da0 = (da0_x + U32 * a0)[:, :, None]
    da1 = (da0_x + db + U32 * a1)[:, :, None]
    A = ref["A"]
    if cls:
        # dice_class_bwd_voxel: e_c inv (in dp), s = sum_k p_k A_k (C products, C additions), p_c (A_c - s) (a subtraction, a product),
        # kc = kce w_y (a product), p_c - [c == y] (a subtraction), kc (..) (a product), the sum of the two terms, times g
        dA = torch.where(oh, da1, da0)
        S = (p * A).sum(1, keepdim=True)
        dS = (dp * A.abs() + p * dA).sum(1, keepdim=True) + (C + 1) * U32 * (p * A.abs()).sum(1, keepdim=True)
        AmS = A - S
        t1 = p * AmS
        dt1 = dp * AmS.abs() + p * (dA + dS + U32 * AmS.abs()) + U32 * t1.abs()
        kc = (ref["kce"] * ref["wy"])[:, None]
        dkc = dkce * ref["wy"][:, None] + U32 * kc.abs()
        pm = p - ohd
        t2 = kc * pm
        dt2 = dkc * pm.abs() + kc.abs() * (dp + U32 * pm.abs()) + U32 * t2.abs()
        gb = (g * (dt1 + dt2 + U32 * (t1 + t2).abs()) + U32 * ref["grad"].abs()) * cm + FLOOR
    else:
        # dice_chan_bwd: A = a0 + t (a1 - a0) (a subtraction, a product, an addition), q = p (1 - p), A q, kce (p - t), their sum, times g
        a0v, a1v = ref["a0"][:, :, None], ref["a1"][:, :, None]
        dA = da0 + t.abs() * (da0 + da1) + U32 * (2 * t.abs() * (a1v - a0v).abs() + A.abs())
        q = p * (1 - p)
        dq = dp + 2 * U32 * q
        t1 = A * q
        dt1 = dA * q + A.abs() * dq + U32 * t1.abs()
        pm = p - t
        t2 = ref["kce"] * pm
        dt2 = dkce * pm.abs() + kce * (dp + U32 * pm.abs()) + U32 * t2.abs()
        gb = g * (dt1 + dt2 + U32 * (t1 + t2).abs()) + U32 * ref["grad"].abs() + FLOOR
    return dict(sums=sb, loss=loss_b, grad=gb)


def check(name, got_loss, got_grad, got_sums, ref, bnd):
    """Rows (conv_bounds.compare form) of the loss, every gradient element and the Dice / CE sums against the reference.  The counts (labels out of
    range, counted voxels) are integers below 2^24: compared exactly."""
    C = ref["C"]
    rows = [compare(f"{name}.loss", got_loss.reshape(1), ref["loss"].reshape(1), bnd["loss"].reshape(1), axes="i"),
            compare(f"{name}.grad", got_grad.reshape(ref["grad"].shape), ref["grad"], bnd["grad"], axes="ncv")]
    if got_sums is not None:
        cols = [k + c for k in (DR_I, DR_P, DR_T) for c in range(C)] + ([DR_CE, DR_W] if ref["w_ce"] != 0 else [])
        idx = torch.tensor(cols, device=ref["sums"].device)
        gs = got_sums.double().to(ref["sums"].device)
        rows.append(compare(f"{name}.sums", gs[idx], ref["sums"][idx], bnd["sums"][idx], axes="k"))
        exact = bool((gs[DR_FAULT] == ref["sums"][DR_FAULT]).item()) and (not ref["class_mode"] or bool((gs[DR_CNT] == ref["sums"][DR_CNT]).item()))
        rows.append(dict(name=f"{name}.counts", err=0.0 if exact else float("inf"), tol=0.0, ok=exact,
                         extra=f"faults {gs[DR_FAULT].item():.0f} / {ref['sums'][DR_FAULT].item():.0f}, counted {gs[DR_CNT].item():.0f} / {ref['sums'][DR_CNT].item():.0f}"))
    return rows


# ---- fixtures (tests/test_dice_losses_cpu.py checks what they promise; tests/test_dice_losses_gpu.py runs them) ---------------------------------------
def class_fixture(gen, N, C, V, *, ignore_index=-100, ignored=0.1, out_of_range=0.0, absent=None, dead_sample=None, all_ignored=False, scale=2.0):
    """Logits (N, C, V) and a label map (N, 1, V) as floats.  `ignored`: the share of voxels labelled ignore_index (at most 0.15, so that at least
    85 % count); `absent`: a class that no voxel carries; `dead_sample`: a sample whose every voxel is ignored; `all_ignored`: the whole batch."""
    z = (torch.randn(N, C, V, generator=gen) * scale).float()
    classes = [c for c in range(C) if c != absent]
    lab = torch.tensor(classes)[torch.randint(0, len(classes), (N, 1, V), generator=gen)]
    for n in range(N):                                            # every (other) class occurs in every sample, whatever the draw
        lab[n, 0, : len(classes)] = torch.tensor(classes)
    r = torch.rand(N, 1, V, generator=gen)
    r[:, :, : len(classes)] = 1.0
    lab = torch.where(r < ignored, torch.full_like(lab, ignore_index), lab)
    if out_of_range > 0:
        lab = torch.where((r >= ignored) & (r < ignored + out_of_range), torch.full_like(lab, C + 1), lab)
    if dead_sample is not None:
        lab[dead_sample] = ignore_index
    if all_ignored:
        lab[:] = ignore_index
    return z, lab.float()


def channel_fixture(gen, N, C, V, scale=2.0):
    z = (torch.randn(N, C, V, generator=gen) * scale).float()
    t = (torch.rand(N, C, V, generator=gen) > 0.6).float()
    return z, t


def fixture_condition(lab, C, ignore_index=-100):
    """(share of counted voxels, every class has a counted voxel) of a label map."""
    y = lab.long().reshape(-1)
    counted = (y != ignore_index) & (y >= 0) & (y < C)
    present = torch.bincount(y[counted], minlength=C) > 0
    return counted.double().mean().item(), bool(present.all().item())

"""The one-channel BCE / Dice / Dice + CE loss (bpx_seg_loss_*), the per-channel instance losses (bpx_chan_loss_*) and the multi-class cross entropy
(bpx_softmax_ce_*) of biapy_amd/losses.py and csrc/plain_losses.hip (shared pieces: csrc/loss_parts.h) in float64 - value, closed-form gradient, the sums, the counts - and per-element
bounds of what the device may differ by, derived from the kernels' operations in the manner of tests/loss_bounds.py:

    |got - ref| <= (error of every fp32 term pushed through on absolute values) + chain 2^-24 sum|terms| + 2^-24 |ref| (+ a floor of 2^-126)

Nothing here is fitted to a measured value.  u = 2^-24.  Shared figures (loss_bounds.py): expf / logf / log1pf TRANS = 4 u, a division DIV = 5 u, the
sigmoid K_SIG = 16 u (either form: r = 1 / (1 + en) then en r, or en / (1 + en): 4 + 4 + 1 + 5 units at most); tanhf: conv_bounds' ACT_REL |y| + ACT_ABS
units.  Products of two errors are below 2^-20 of the first-order terms, which the generous constants (2 ulp where ocml documents 1, 2.5 ulp for a
correctly rounded division) cover.  The floor of 2^-126 stands for denormal results (expf(-88), p at z = -88 ... -104), whether kept or flushed.

BINARY (seg_loss_sums_kernel, seg_loss_finish_kernel, seg_loss_bwd[_fused]_kernel)
* the reference is loss_bounds.reference in channel mode with C = 1.  Identity: with M dice terms (1, or N per sample), a0 = w_dice (2I+s) / (M (U+s)^2),
  a1 = a0 - 2 w_dice / (M (U+s)): the kernel's a = kce g, b = -g (a1 - a0), c = g a0 and dz = a (p - t) - p (1 - p) (b t - c) = g (A p (1 - p) + kce (p - t))
  with A = a0 + t (a1 - a0).  seg_closed_form states the a / b / c form on its own; tests/test_plain_losses_cpu.py checks the two against each other.
* BCE term fmaxf(z, 0) - z t + log2(fl(1 + en)) ln2: en = expf(-|z|) (4 u en); fl(1 + en) moves log by (4 u en + u (1 + en)) / (1 + en); v_log_f32 is
  accurate to one ulp of its result (2 u log2), the product with the rounded constant ln2 rounds twice: e_l = u (1 + 4 en / (1 + en)) + 4 u l, at most
  5.8 u = 3.5e-7 at z = 0.  (The kernel's comment says ~1e-7: it leaves out expf's own error.)  z t rounds once, the two additions once each.
* a thread of the sums kernel adds 4 terms per iteration, ceil((n / 4) / (256 B)) iterations, B = bpx_seg_loss_blocks(n); the tail adds one; six
  shuffle levels; three additions across the waves: chain = 4 ceil((n / 4) / (256 B)) + 1 + 9.  The finish kernel adds the B rows in double.
* loss and coefficients are formed in double from the device's sums and rounded once: the sums' bounds pushed through as intervals.
* dz: p - t, a (..), 1 - p, p (..), b t, (..) - c, the product, the difference: counted in seg_bounds.

CHANNEL (chan_loss_sums_kernel, chan_loss_finish_kernel, chan_loss_bwd_kernel): chain = ceil(vox / (256 nb)) + 9, nb = bpx_chan_loss_blocks(vox); the
finish in double over N nb partials per channel.  k = gup w_c inv_count: inv_count rounds once, two products; the direct entry takes k rounded once.
L1: the sign of d = act(z) - t is exact where |d| exceeds d's bound (or d = 0 exactly with no error, the linear channel's z == t); elsewhere the
device's element is one of -k da, 0, k da: it is compared with 0 under the bound |k| |da|.

SOFTMAX CE (softmax_ce_sums_kernel, softmax_ce_finish_kernel, softmax_ce_bwd_kernel): the nll term as loss_bounds counts it; chain =
ceil(vox / (256 nb)) + 8 (six shuffle levels, (r0 + r1) + (r2 + r3)); the finish in double, one division, one rounding.  Backward: k0 = fl(gup / S_w),
k0 w_y, e inv (the softmax element, 2 maxd + C + 13 units), - onehot, the product.
"""
from __future__ import annotations

import torch

import loss_bounds as LB
from conv_bounds import ACT_ABS, ACT_REL, U32, compare
from loss_bounds import DIV, FLOOR, K_SIG, TRANS, U64, _ratio_bound  # noqa: F401

SEG_FAULTS = ("tail_dropped", "wrap_skipped", "dice_c_sign", "ce_mean_over_vox_not_numel", "log1p_as_log")
CHAN_FAULTS = ("tanh_derivative_missing", "mse_factor_two_missing", "weights_unapplied", "mean_over_vox_not_N_vox", "l1_sign_at_zero")
CE_FAULTS = ("ignored_gets_gradient", "mean_over_count_not_weight_sum", "argmax_last_maximum", "out_of_range_label_counted", "weight_in_loss_only")
FAULTS = dict(seg=SEG_FAULTS, chan=CHAN_FAULTS, ce=CE_FAULTS)
BF16 = 2.0 ** -8                     # the unit roundoff of bf16 (8 significand bits): a gradient handed back in bf16


# the seeds of the GPU fixtures: the CPU tests assert the fixtures' conditions on the same draws
def seg_seed(n):
    return 10 + n


def chan_seed(vox):
    return 30 + vox


def ce_seed(C):
    return 100 + C


def f32(x) -> float:
    """x as the device receives it through a float argument or a float32 tensor."""
    return float(torch.tensor(float(x), dtype=torch.float32).item())


def _exact_row(name, got, ref):
    ok = bool(torch.equal(got.double().cpu(), ref.double().cpu()))
    return dict(name=name, err=0.0 if ok else float("inf"), tol=0.0, ok=ok, extra=f"{got.tolist()} / {ref.tolist()}")


# ==== binary ================================================================================================================================================
SEG_PLANTED = (0.0, -0.0, 17.0, -17.0, 30.0, -30.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4)
SEG_ZERO_BAND = 2.0 ** -10


def seg_chain(n: int, blocks: int) -> int:
    return 4 * -(-(n // 4) // (256 * blocks)) + 1 + 9


def seg_log_bound(en, lg):
    """The absolute error of seg_log1p_unit(en) = log2(fl(1 + en)) ln2 around lg = log(1 + en), en carrying expf's error (module docstring)."""
    return U32 * (1 + TRANS * en / (1 + en)) + 4 * U32 * lg


def seg_fixture(gen, n, N=1):
    """Logits (N, 1, n) = 3 randn with the saturated values planted (first, last - the tail - and evenly between), none other inside
    (0, 2^-10); targets in {0, 1} with a few 0.5 and 0.25."""
    z = torch.randn(N, 1, n, generator=gen) * 3
    z = torch.where(z.abs() < SEG_ZERO_BAND, torch.full_like(z, SEG_ZERO_BAND), z)
    t = (torch.rand(N, 1, n, generator=gen) > 0.6).float()
    k = min(n, len(SEG_PLANTED))
    vals = SEG_PLANTED if k == len(SEG_PLANTED) else SEG_PLANTED[1::len(SEG_PLANTED) // k][:k]
    pos = torch.linspace(0, n - 1, k).round().long()
    assert pos.unique().numel() == k
    z[..., pos] = torch.tensor(vals)
    for j, v in ((0, 0.5), (2, 0.5), (5, 0.25), (10, 0.25), (11, 0.5)):
        if j < k:
            t[..., pos[j]] = v
    if n >= 64:
        t[..., n // 3], t[..., n // 2] = 0.5, 0.25
    return z, t


def seg_fixture_condition(z):
    """(number of elements with 0 < |z| < 2^-10, number of exact zeros)."""
    return int(((z != 0) & (z.abs() < SEG_ZERO_BAND)).sum().item()), int((z == 0).sum().item())


def _seg_counts(z64, t64):
    P, T = torch.sigmoid(z64).float() > 0.5, t64 > 0.5
    return torch.stack([(P & T).sum(), (P | T).sum()]).double()


def seg_reference(z, t, *, w_ce, w_dice, smooth=f32(1e-5), batch_dice=True, g=1.0):
    """loss_bounds.reference in channel mode with C = 1, plus the two IoU counts and the kernel's row of six sums (the batch totals)."""
    assert z.shape[1] == 1 and t.shape == z.shape
    ref = LB.reference(z, t, w_ce=w_ce, w_dice=w_dice, smooth=smooth, batch_dice=batch_dice, g=g)
    ref["counts"] = _seg_counts(ref["z"], ref["t"])
    ref["sums6"] = torch.stack([ref["bce"].sum(), ref["I"].sum(), ref["P"].sum(), ref["T"].sum(), ref["counts"][0], ref["counts"][1]])
    return ref


def seg_closed_form(z, t, *, w_ce, w_dice, smooth=f32(1e-5), batch_dice=True, g=1.0, fault=None, blocks=None, bwd_blocks=None):
    """The kernels' own statement in float64: per call (the whole batch, or one sample after another) the six sums, the loss
    w_ce S0 / n + w_dice (1 - (2 S1 + s) / (S2 + S3 + s)), the coefficients a, b, c and dz = a (p - t) - p (1 - p) (b t - c); per sample the calls'
    mean.  `fault`: one of SEG_FAULTS (wrap_skipped needs the block counts of the two passes)."""
    assert fault is None or fault in SEG_FAULTS
    N, V = z.shape[0], z[0].numel()
    R = 1 if batch_dice else N
    zz, tt = z.double().reshape(R, -1), t.double().reshape(R, -1)
    n = zz.shape[1]
    keep_s = torch.ones(n, dtype=torch.bool, device=z.device)
    keep_g = keep_s.clone()
    if fault == "tail_dropped":
        keep_s[n - n % 4:] = False
        keep_g[n - n % 4:] = False
    if fault == "wrap_skipped":
        keep_s[4 * 256 * blocks:] = False
        keep_g[4 * 256 * bwd_blocks:] = False
    ms = keep_s.double()
    p = torch.sigmoid(zz)
    en = torch.exp(-zz.abs())
    bce = torch.clamp(zz, min=0) - zz * tt + (torch.log(en.clamp_min(1e-300)) if fault == "log1p_as_log" else torch.log1p(en))
    S0, S1, S2, S3 = ((x * ms).sum(1, keepdim=True) for x in (bce, p * tt, p, tt))
    n_mean = float(V if fault == "ce_mean_over_vox_not_numel" else n)
    s = float(smooth)
    den = S2 + S3 + s
    loss_r = torch.zeros_like(S0)
    if w_ce != 0:
        loss_r = loss_r + w_ce * S0 / n_mean
    if w_dice != 0:
        loss_r = loss_r + w_dice * (1 - (2 * S1 + s) / den)
    gr = g / R
    a, b, c = w_ce * gr / n_mean, 2 * w_dice * gr / den, w_dice * gr * (2 * S1 + s) / den ** 2
    if fault == "dice_c_sign":
        c = -c
    grad = (a * (p - tt) - p * (1 - p) * (b * tt - c)) * keep_g.double()
    P, T = (p.float() > 0.5) & keep_s, (tt > 0.5) & keep_s
    counts = torch.stack([(P & T).sum(), (P | T).sum()]).double()
    sums6 = torch.stack([S0.sum(), S1.sum(), S2.sum(), S3.sum(), counts[0], counts[1]])
    return dict(loss=loss_r.mean(), grad=grad.reshape(N, 1, V), sums6=sums6, counts=counts, coef=torch.cat([a * torch.ones_like(b), b, c], 1))


def seg_bounds(ref, blocks: int, gup_rel: float = 0.0, grad_unit: float = 0.0):
    """Bounds of the device's six sums (the batch case), loss (0-d) and gradient (N, 1, V) around a seg_reference() result.  `blocks` =
    bpx_seg_loss_blocks of one call's element count.  gup_rel: units of u by which the upstream gradient the kernel reads may differ from g / M
    (per sample the mean's backward forms it in fp32); grad_unit: the rounding of the gradient's own storage type (BF16), 0 for fp32."""
    N, V, batch = ref["N"], ref["V"], ref["batch"]
    R = 1 if batch else N
    n = N * V // R
    z, t, p, bce, grad = (ref[k].reshape(R, n) for k in ("z", "t", "p", "bce", "grad"))
    w_ce, w_dice, g, s = abs(ref["w_ce"]), abs(ref["w_dice"]), abs(ref["g"]), ref["s"]
    red = seg_chain(n, blocks) * U32 + (blocks + 16) * U64

    def sum_bound(term, e):
        return e.sum(1) + red * (term.abs() + e).sum(1)

    en = torch.exp(-z.abs())
    lg = torch.log1p(en)
    dp = K_SIG * U32 * p + FLOOR
    zt, m = z * t, z.clamp_min(0)
    e_l = seg_log_bound(en, lg)
    e_bce = U32 * (zt.abs() + (m - zt).abs() + bce.abs()) + e_l
    dS0, dI, dP, dT = sum_bound(bce, e_bce), sum_bound(p * t, dp * t.abs() + U32 * (p * t).abs()), sum_bound(p, dp), sum_bound(t, torch.zeros_like(t))
    S0, I, U = bce.sum(1), ref["I"].reshape(R), ref["U"].reshape(R)
    dU = dP + dT
    num, den = 2 * I + s, U + s
    inf = torch.full_like(den, float("inf"))
    ddice = torch.where(den > dU, _ratio_bound(num, 2 * dI, den, dU), inf) + 8 * U64
    loss_r = w_ce * S0 / n + w_dice * (1 - num / den)
    lb = U32 * loss_r.abs() + 16 * U64 * (w_ce * S0.abs() / n + w_dice) + FLOOR
    if w_ce != 0:
        lb = lb + w_ce * dS0 / n
    if w_dice != 0:
        lb = lb + w_dice * ddice
    # torch's mean over the per-sample losses: N - 1 additions and a division in fp32
    loss_b = lb[0] if R == 1 else lb.mean() + (N + 1) * U32 * (loss_r.abs() + lb).mean()
    # the coefficients: double arithmetic on the device's sums, one rounding (and the upstream gradient's own error)
    gr = g / R
    ru = (1 + gup_rel) * U32
    safe = (den - dU).clamp_min(1e-300)
    a = torch.full_like(den, w_ce * gr / n)
    b, c = 2 * w_dice * gr / den, w_dice * gr * num / den ** 2
    da = ru * a
    db = b * dU / safe + ru * b
    dc = torch.maximum(w_dice * gr * (num + 2 * dI) / safe ** 2 - c, c - w_dice * gr * (num - 2 * dI).clamp_min(0) / (den + dU) ** 2) + ru * c
    a, b, c, da, db, dc = (x[:, None] for x in (a, b, c, da, db, dc))
    pm = p - t
    t1 = a * pm
    dt1 = da * pm.abs() + a * (dp + U32 * pm.abs()) + U32 * t1.abs()
    q = p * (1 - p)
    dq = dp + 2 * U32 * q
    bt = b * t
    btc = bt - c
    dbtc = db * t.abs() + U32 * bt.abs() + dc + U32 * btc.abs()
    t2 = q * btc
    dt2 = dq * btc.abs() + q * dbtc + dq * dbtc + U32 * t2.abs()
    gb = dt1 + dt2 + U32 * (t1 - t2).abs() + FLOOR
    if grad_unit:
        gb = gb + grad_unit * (grad.abs() + gb)
    sb = torch.stack([dS0.sum(), dI.sum(), dP.sum(), dT.sum()]) + FLOOR
    return dict(sums=sb, loss=loss_b, grad=gb.reshape(N, 1, V), coef=torch.cat([a, b, c], 1), dcoef=torch.cat([da, db, dc], 1))


def seg_check(name, got_loss, got_grad, got_sums6, ref, bnd):
    """Rows (conv_bounds.compare form).  got_sums6: the device's row of six (a batch call), or None.  The two counts are compared exactly."""
    rows = []
    if got_loss is not None:
        rows.append(compare(f"{name}.loss", got_loss.reshape(1), ref["loss"].reshape(1), bnd["loss"].reshape(1), axes="i"))
    if got_grad is not None:
        rows.append(compare(f"{name}.grad", got_grad.reshape(ref["grad"].shape), ref["grad"], bnd["grad"].reshape(ref["grad"].shape), axes="ncv"))
    if got_sums6 is not None:
        gs = got_sums6.double().to(ref["sums6"].device)
        rows.append(compare(f"{name}.sums", gs[:4], ref["sums6"][:4], bnd["sums"], axes="k"))       # the kernel forms all four whatever the weights
        rows.append(_exact_row(f"{name}.counts", gs[4:6], ref["sums6"][4:6]))
    return rows


# ==== per-channel losses ======================================================================================================================================
SPEC_BCD_MSE = (("bce", "linear"), ("bce", "linear"), ("mse", "tanh"))
SPEC_BCD_L1 = (("bce", "linear"), ("bce", "linear"), ("l1", "tanh"))
SPEC_ALL8 = (("bce", "linear"), ("bce", "linear"), ("mse", "linear"), ("mse", "tanh"), ("mse", "sigmoid"), ("l1", "linear"), ("l1", "tanh"), ("l1", "sigmoid"))
WEIGHTS_ALL8 = (1.0, 0.5, 2.0, 0.25, 1.5, 1.0, 0.75, 3.0)          # exact in fp32
CHAN_PLANT_MIN_VOX = 64


def chan_codes(spec) -> int:
    """code[c] = kind | act << 2 as csrc/plain_losses.hip reads it."""
    kind, act = dict(bce=0, mse=1, l1=2), dict(linear=0, tanh=1, sigmoid=2)
    return sum((kind[k] | ((act[a] if k != "bce" else 0) << 2)) << (4 * i) for i, (k, a) in enumerate(spec))


def chan_chain(vox: int, nb: int) -> int:
    return -(-vox // (256 * nb)) + 9


def chan_fixture(gen, N, spec, vox):
    """Logits 2 randn; targets {0, 1} on BCE channels, uniform in (-1, 1) on tanh channels and in (0, 1) on the others.  From 64 voxels on: z = +-20
    on tanh channels (derivative 0), z == t exactly at four places of a linear L1 channel (gradient 0).  Returns (z, t, planted) with planted the
    (N, C, vox) mask of the z == t elements."""
    C = len(spec)
    z = (torch.randn(N, C, vox, generator=gen) * 2).float()
    t = torch.rand(N, C, vox, generator=gen).float()
    planted = torch.zeros(N, C, vox, dtype=torch.bool)
    for c, (kind, act) in enumerate(spec):
        if kind == "bce":
            t[:, c] = (t[:, c] > 0.6).float()
        elif act == "tanh":
            t[:, c] = t[:, c] * 2 - 1
        if vox >= CHAN_PLANT_MIN_VOX:
            if kind != "bce" and act == "tanh":
                z[:, c, 0], z[:, c, vox - 1], z[:, c, vox // 2] = 20.0, -20.0, 20.0
                t[:, c, vox // 2] = 1.0
            if kind == "l1" and act == "linear":
                for pos in (1, vox // 3, vox // 2, vox - 1):
                    t[:, c, pos] = z[:, c, pos]
                    planted[:, c, pos] = True
    return z, t, planted


def _chan_channel(z, t, kind, act, fault=None):
    """(term, dz, and what the bounds need) of one channel in float64."""
    o = dict(kind=kind, act=act)
    if kind == "bce":
        en = torch.exp(-z.abs())
        p = torch.sigmoid(z)
        o.update(term=torch.clamp(z, min=0) - z * t + torch.log1p(en), dz=p - t, p=p, en=en)
        return o
    if act == "tanh":
        a = torch.tanh(z)
        da = torch.ones_like(z) if fault == "tanh_derivative_missing" else 1 - a * a
    elif act == "sigmoid":
        a = torch.sigmoid(z)
        da = a * (1 - a)
    else:
        a, da = z, torch.ones_like(z)
    d = a - t
    if kind == "mse":
        o.update(term=d * d, dz=(1.0 if fault == "mse_factor_two_missing" else 2.0) * d * da)
    else:
        sgn = torch.sign(d)
        if fault == "l1_sign_at_zero":
            sgn = torch.where(d >= 0, torch.ones_like(d), -torch.ones_like(d))
        o.update(term=d.abs(), dz=sgn * da)
    o.update(a=a, da=da, d=d)
    return o


def chan_reference(z, t, spec, weights, g=1.0, fault=None):
    """z, t (N, C, vox).  loss = sum_c w_c mean over N vox of the channel's terms; grad = g w_c / (N vox) d term / d z."""
    assert fault is None or fault in CHAN_FAULTS
    N, C, V = z.shape[0], z.shape[1], z[0, 0].numel()
    zz, tt = z.double().reshape(N, C, V), t.double().reshape(N, C, V)
    w = torch.as_tensor(weights, dtype=torch.float32, device=z.device).double()
    wa = torch.ones_like(w) if fault == "weights_unapplied" else w
    count = float(V if fault == "mean_over_vox_not_N_vox" else N * V)
    ch = [_chan_channel(zz[:, c], tt[:, c], k, a, fault) for c, (k, a) in enumerate(spec)]
    sums = torch.stack([o["term"].sum() for o in ch])
    loss = (wa * sums / count).sum()
    kc = g * wa / count
    grad = torch.stack([kc[c] * o["dz"] for c, o in enumerate(ch)], 1)
    return dict(N=N, C=C, V=V, spec=tuple(spec), w=w, g=float(g), z=zz, t=tt, ch=ch, sums=sums, loss=loss, grad=grad, k=kc, count=count)


def chan_bounds(ref, nb: int, k_units: float = 3.0):
    """Bounds of the per-channel sums (C), the loss and the gradient (N, C, V) around a chan_reference() result; `undecided` marks the L1 elements whose
    sign the bound of d cannot decide (compared with 0 under |k| |da|).  k_units: roundings in k (3 fused: inv_count and two products; 1 direct)."""
    N, C, V, z, t = ref["N"], ref["C"], ref["V"], ref["z"], ref["t"]
    red = chan_chain(V, nb) * U32 + (N * nb + 16) * U64
    dS, gb, und, eff = [], [], [], []
    for c, o in enumerate(ref["ch"]):
        zc, tc, term, dz = z[:, c], t[:, c], o["term"], o["dz"]
        k = ref["k"][c].abs()
        dk = k_units * U32 * k
        undecided = torch.zeros_like(zc, dtype=torch.bool)
        if o["kind"] == "bce":
            en, p = o["en"], o["p"]
            lg = torch.log1p(en)
            zt, m = zc * tc, zc.clamp_min(0)
            e_term = U32 * (zt.abs() + (m - zt).abs() + term.abs()) + TRANS * U32 * (lg + en / (1 + en)) + FLOOR
            e_dz = K_SIG * U32 * p + FLOOR + U32 * dz.abs()
            zero_b = e_dz
        else:
            a, da, d = o["a"], o["da"], o["d"]
            if o["act"] == "tanh":
                ea = U32 * (ACT_REL * a.abs() + ACT_ABS)
                yy = a * a
                eda = 2 * a.abs() * ea + ea * ea + U32 * yy + U32 * da.abs()
            elif o["act"] == "sigmoid":
                ea = K_SIG * U32 * a + FLOOR
                eda = ea + 2 * U32 * da
            else:
                ea, eda = torch.zeros_like(a), torch.zeros_like(a)
            ed = ea + U32 * d.abs()
            if o["kind"] == "mse":
                e_term = 2 * d.abs() * ed + ed * ed + U32 * term
                e_dz = 2 * (ed * da.abs() + d.abs() * eda + ed * eda) + U32 * dz.abs()
            else:
                e_term = ed
                undecided = ~((d.abs() > ed) | ((d == 0) & (ed == 0)))
                e_dz = eda
            zero_b = da.abs() + eda
        dS.append(e_term.sum() + red * (term.abs() + e_term).sum())
        b_dec = k * e_dz + dk * dz.abs() + dk * e_dz + U32 * (k * dz).abs() + FLOOR
        b_und = (k + dk) * zero_b * (1 + U32) + FLOOR
        gb.append(torch.where(undecided, b_und, b_dec))
        und.append(undecided)
        eff.append(torch.where(undecided, torch.zeros_like(dz), ref["grad"][:, c]))
    dS = torch.stack(dS)
    w = ref["w"].abs()
    loss_b = (w * dS).sum() / ref["count"] + U32 * ref["loss"].abs() + 16 * U64 * (w * ref["sums"].abs()).sum() / ref["count"] + FLOOR
    return dict(sums=dS + FLOOR, loss=loss_b, grad=torch.stack(gb, 1), undecided=torch.stack(und, 1), grad_ref=torch.stack(eff, 1))


def chan_check(name, got_loss, got_grad, got_sums, ref, bnd):
    rows = []
    if got_loss is not None:
        rows.append(compare(f"{name}.loss", got_loss.reshape(1), ref["loss"].reshape(1), bnd["loss"].reshape(1), axes="i"))
    if got_grad is not None:
        share = bnd["undecided"].double().mean().item()
        r = compare(f"{name}.grad", got_grad.reshape(ref["grad"].shape), bnd["grad_ref"], bnd["grad"], axes="ncv")
        gg = got_grad.reshape(ref["grad"].shape).double().to(ref["grad"].device)
        dec = torch.where(bnd["undecided"], torch.zeros_like(gg), (gg - ref["grad"]).abs() / bnd["grad"]).max().item()
        r["extra"] += f"; L1 sign undecided {share:.2e}, worst decided element {dec:.3e}"      # an undecided one sits at ~1 by construction
        rows.append(r)
    if got_sums is not None:
        rows.append(compare(f"{name}.sums", got_sums.double().to(ref["sums"].device), ref["sums"], bnd["sums"], axes="c"))
    return rows


# ==== softmax cross entropy =================================================================================================================================
CE_WEIGHTS = {2: [0.3, 1.7], 3: [0.2, 0.5, 0.3], 5: [1.0, 2.0, 0.5, 0.25, 4.0], 8: [1.0, 2.0, 0.5, 0.25, 4.0, 1.0, 3.0, 0.1]}
CE_TIE = 4.25                     # exact in fp32; every other logit of a tied voxel is clamped to 3 at most


def ce_chain(vox: int, nb: int) -> int:
    return -(-vox // (256 * nb)) + 8


def ce_fixture(gen, N, C, V, ignore_index=-100):
    """Logits (N, C, V) = 2 randn, a label map (N, 1, V) as floats: the last class absent, 10 % of the voxels ignore_index, 2 % out of range (C + 1).
    From 4 C voxels on: every other class occurs in every sample, and three voxels hold exact ties of the maximum (classes 0 and 1; 0, 1 and 2 for
    C >= 3; the last two classes), all of them counted.  Returns (z, labels, the tie positions)."""
    absent = C - 1
    z = (torch.randn(N, C, V, generator=gen) * 2).float()
    classes = [c for c in range(C) if c != absent]
    k = len(classes)
    lab = torch.tensor(classes)[torch.randint(0, k, (N, 1, V), generator=gen)]
    r = torch.rand(N, 1, V, generator=gen)
    ties = []
    if V >= 4 * C:
        lab[:, 0, :k] = torch.tensor(classes)
        ties = [k, k + 1, V - 1]
        r[:, :, : k + 2] = 1.0
        r[:, :, V - 1] = 1.0
        for pos, tied in zip(ties, ([0, 1], [0, 1, 2] if C >= 3 else [0, 1], [C - 2, C - 1])):
            z[:, :, pos] = z[:, :, pos].clamp(max=3.0)
            z[:, tied, pos] = CE_TIE
        lab[:, 0, k], lab[:, 0, k + 1], lab[:, 0, V - 1] = 1 if k > 1 else 0, 0, C - 2
    else:
        r[:] = 1.0
    lab = torch.where(r < 0.1, torch.full_like(lab, ignore_index), lab)
    lab = torch.where((r >= 0.1) & (r < 0.12), torch.full_like(lab, C + 1), lab)
    return z, lab.float(), ties


def ce_fixture_condition(z, lab, C, ignore_index, ties):
    """(share of counted voxels, every class but the last present and counted in every sample, the planted ties are exact maxima shared in fp32)."""
    y = lab[:, 0].long()
    counted = (y != ignore_index) & (y >= 0) & (y < C)
    present = all(bool((torch.bincount(y[n][counted[n]], minlength=C)[: C - 1] > 0).all()) for n in range(y.shape[0]))
    exact = all(bool(((z[:, :, p] == z[:, :, p].max(1, keepdim=True).values).sum(1) >= 2).all()) and bool(counted[:, p].all()) for p in ties)
    return counted.double().mean().item(), present, exact


def ce_reference(z, lab, weight=None, ignore_index=-100, g=1.0, fault=None):
    """z (N, C, V), lab (N, 1, V) class ids as floats.  The closed form of oracle.loss_oracle.softmax_ce with labels outside [0, C) left out as the
    ignored ones are; gradient g w_y / S_w (softmax - onehot), exactly 0 where the label is not counted; the counts of the first-maximum prediction."""
    assert fault is None or fault in CE_FAULTS
    N, C, V = z.shape[0], z.shape[1], z[0, 0].numel()
    dev = z.device
    zz = z.double().reshape(N, C, V)
    y = lab.reshape(N, V).long()
    counted = (y != ignore_index) & (y >= 0) & (y < C)
    if fault == "out_of_range_label_counted":
        counted = y != ignore_index
        y = y.clamp(0, C - 1)
    yc = torch.where(counted, y, torch.zeros_like(y))
    w = torch.ones(C, dtype=torch.float64, device=dev) if weight is None else torch.as_tensor(weight, dtype=torch.float32, device=dev).double()
    cm = counted.double()
    wy = w[yc] * cm
    lse = torch.logsumexp(zz, 1)
    nll = (lse - torch.gather(zz, 1, yc[:, None])[:, 0]) * cm
    S_nll = (wy * nll).sum()
    S_w = cm.sum() if fault == "mean_over_count_not_weight_sum" else wy.sum()
    loss = S_nll / S_w
    p = torch.softmax(zz, 1)
    oh = torch.nn.functional.one_hot(yc, C).permute(0, 2, 1).double() * cm[:, None]
    wg = cm if fault == "weight_in_loss_only" else wy
    k = torch.where(counted, g * wg / S_w, torch.zeros_like(wy))
    if fault == "ignored_gets_gradient":
        k = torch.where(counted, k, g / S_w * torch.ones_like(k))
    grad = k[:, None] * (p - oh)
    idx = torch.arange(C, device=dev)[None, :, None]
    eq = zz == zz.max(1, keepdim=True).values
    am = torch.where(eq, idx, torch.full_like(idx, -1)).max(1).values if fault == "argmax_last_maximum" else torch.where(eq, idx, torch.full_like(idx, C)).min(1).values
    cnt = torch.stack([torch.bincount(yc[counted & (am == yc)], minlength=C), torch.bincount(am[counted], minlength=C), torch.bincount(yc[counted], minlength=C)]).double()
    return dict(N=N, C=C, V=V, z=zz, counted=counted, wy=wy, lse=lse, nll=nll, S_nll=S_nll, S_w=S_w, loss=loss, p=p, oh=oh, k=k, grad=grad, counts=cnt, g=float(g))


def ce_bounds(ref, nb: int):
    """Bounds of S_nll, S_w, the loss and the gradient (N, C, V) around a ce_reference() result; nb = bpx_softmax_ce_blocks(V)."""
    N, C, V, z, p, wy, lse, nll = ref["N"], ref["C"], ref["V"], ref["z"], ref["p"], ref["wy"], ref["lse"], ref["nll"]
    cm = ref["counted"].double()
    red = ce_chain(V, nb) * U32 + (N * nb + 16) * U64
    m = z.max(1).values
    maxd = m - z.min(1).values
    k_se = maxd + TRANS + C - 1
    e_nll = U32 * wy * (k_se + TRANS * (lse - m).abs() + lse.abs() + 2 * nll.abs())
    dS_nll = e_nll.sum() + red * ((wy * nll).abs() + e_nll).sum() + FLOOR
    dS_w = red * wy.sum() + FLOOR
    S_nll, S_w, g = ref["S_nll"], ref["S_w"], abs(ref["g"])
    ok = bool((S_w > dS_w).item())
    inf = torch.full_like(S_w, float("inf"))
    loss_b = (_ratio_bound(S_nll.abs(), dS_nll, S_w, dS_w) + (U32 + 16 * U64) * ref["loss"].abs() + FLOOR) if ok else inf
    k0 = g / S_w if ok else inf
    dk0 = (k0 * dS_w / (S_w - dS_w) + U32 * k0) if ok else inf
    k = ref["k"].abs()[:, None]
    dk = (dk0 * wy)[:, None] + U32 * k
    dp = U32 * p * (2 * maxd[:, None] + C + 13) + FLOOR
    v = p - ref["oh"]
    dv = dp + U32 * v.abs()
    gb = (dk * v.abs() + k * dv + dk * dv + U32 * (k * v).abs()) * cm[:, None] + FLOOR
    gb = torch.where(cm[:, None].expand_as(gb) > 0, gb, torch.full_like(gb, FLOOR))      # 0 (inf) = nan where nothing is counted at all
    return dict(S_nll=dS_nll, S_w=dS_w, loss=loss_b, grad=gb)


def ce_check(name, got_loss, got_grad, got_sums, ref, bnd):
    """got_sums: the device's row {S_nll, S_w, tp[8], pred[8], tgt[8]} or None.  Besides the bound, the gradient must be +-0 bit for bit at every
    voxel that is not counted."""
    C = ref["C"]
    rows = []
    if got_loss is not None:
        rows.append(compare(f"{name}.loss", got_loss.reshape(1), ref["loss"].reshape(1), bnd["loss"].reshape(1), axes="i"))
    if got_grad is not None:
        gg = got_grad.reshape(ref["grad"].shape)
        rows.append(compare(f"{name}.grad", gg, ref["grad"], bnd["grad"], axes="ncv"))
        nz = int(((gg != 0) & ~ref["counted"].to(gg.device)[:, None]).sum().item())
        rows.append(dict(name=f"{name}.grad_uncounted_zero", err=float(nz), tol=0.0, ok=nz == 0, extra=f"{nz} non-zero elements at voxels that are not counted"))
    if got_sums is not None:
        gs = got_sums.double().to(ref["S_w"].device)
        rows.append(compare(f"{name}.sums", gs[:2], torch.stack([ref["S_nll"], ref["S_w"]]), torch.stack([bnd["S_nll"], bnd["S_w"]]), axes="k"))
        rows.append(_exact_row(f"{name}.counts", gs[2:].view(3, 8)[:, :C], ref["counts"]))
    return rows

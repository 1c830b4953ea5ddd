"""The one-channel, per-channel and softmax-CE losses without a GPU: the fp64 references of tests/plain_loss_bounds.py against each other, the oracle
and fp64 autograd; an fp32 emulation of each kernel's operation order inside the derived bounds; every simulated fault rejected by the same
comparator; what the fixtures promise; and the 16-byte alignment `_prep` guarantees."""
import math

import pytest
import torch
import torch.nn.functional as F

import plain_loss_bounds as PB
from oracle import loss_oracle as LO

MIXES = ((1.0, 0.0), (0.0, 1.0), (PB.f32(0.7), PB.f32(1.3)))
G_UP = PB.f32(1.7)
SEG_SMALL = (3, 1027, 4096)
SEG_WRAP = 4 * 1048576 + 1203
VOX_SMALL = (1, 1029)
VOX_WRAP = 512 * 1024 + 1029


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _lib():
    from biapy_amd import _lib as L
    return L.lib


def _ok(rows):
    return all(r["ok"] for r in rows)


def _worst(rows):
    return max(r["err"] for r in rows if r["tol"] == 1.0)


# ---- fp32 emulation of the kernels' operation order ------------------------------------------------------------------------------------------------------
def _tree64(x):
    """Six __shfl_xor levels: lane 0 holds the pairwise tree of its wave's 64 values."""
    for _ in range(6):
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def _thread_sums(units, blocks):
    """units (n, lanes) fp32, unit i owned by thread i % (256 blocks) in iteration i // (256 blocks): the threads' running sums (blocks, 256)."""
    n, lanes = units.shape
    per = 256 * blocks
    it = max(1, -(-n // per))
    x = torch.cat([units, torch.zeros(it * per - n, lanes)]).reshape(it, blocks, 256, lanes)
    s = torch.zeros(blocks, 256)
    for i in range(it):
        for e in range(lanes):
            s = s + x[i, :, :, e]
    return s


def _block_reduce(s, pairwise):
    r = _tree64(s.reshape(-1, 4, 64))
    return (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3]) if pairwise else ((r[:, 0] + r[:, 1]) + r[:, 2]) + r[:, 3]


def _sigmoid_div(z):
    en = torch.exp(-z.abs())
    return torch.where(z >= 0, 1.0 / (1.0 + en), en / (1.0 + en)), en


def emulate_seg(z, t, w_ce, w_dice, smooth, g, blocks):
    z, t = z.reshape(-1).float(), t.reshape(-1).float()
    n = z.numel()
    en = torch.exp(-z.abs())
    r = 1.0 / (1.0 + en)
    p = torch.where(z >= 0, r, en * r)
    lg = torch.log2(1.0 + en) * torch.tensor(0.69314718055994531, dtype=torch.float32)
    bce = (z.clamp_min(0) - z * t) + lg
    P, T = p > 0.5, t > 0.5
    n4 = n // 4
    S = []
    for q in (bce, p * t, p, t, (P & T).float(), (P | T).float()):
        s = _thread_sums(q[: 4 * n4].reshape(n4, 4), blocks)
        s[0, : n - 4 * n4] += q[4 * n4:]
        S.append(_block_reduce(s, False).double().sum())
    S = torch.stack(S)
    den = (S[2] + S[3] + smooth).item()
    loss = torch.tensor(w_ce * S[0].item() / n + w_dice * (1.0 - (2.0 * S[1].item() + smooth) / den), dtype=torch.float64).float()
    a, b, c = (torch.tensor(v, dtype=torch.float64).float() for v in (w_ce * g / n, 2.0 * w_dice * g / den, w_dice * g * (2.0 * S[1].item() + smooth) / (den * den)))
    p2, _ = _sigmoid_div(z)
    dz = a * (p2 - t) - p2 * (1.0 - p2) * (b * t - c)
    return loss, dz, S


def _emulate_chan_term(z, t, kind, act):
    if kind == "bce":
        p, en = _sigmoid_div(z)
        return (z.clamp_min(0) - z * t) + torch.log1p(en), p - t
    if act == "tanh":
        a = torch.tanh(z)
        da = 1.0 - a * a
    elif act == "sigmoid":
        a, _ = _sigmoid_div(z)
        da = a * (1.0 - a)
    else:
        a, da = z, torch.ones_like(z)
    d = a - t
    if kind == "mse":
        return d * d, (2.0 * d) * da
    return d.abs(), torch.sign(d) * da


def emulate_chan(z, t, spec, weights, g, nb):
    N, C, V = z.shape
    w32 = torch.tensor(weights, dtype=torch.float32)
    inv = 1.0 / (float(N) * float(V))
    total, sums, grads = 0.0, [], []
    for c, (kind, act) in enumerate(spec):
        term, dz = _emulate_chan_term(z[:, c], t[:, c], kind, act)
        s = sum(_block_reduce(_thread_sums(term[n].reshape(V, 1), nb), False).double().sum() for n in range(N))
        sums.append(s)
        total += s.item() * inv * float(w32[c])
        k = (torch.tensor(g, dtype=torch.float32) * w32[c]) * torch.tensor(inv, dtype=torch.float64).float()
        grads.append(k * dz)
    return torch.tensor(total, dtype=torch.float64).float(), torch.stack(grads, 1), torch.stack(sums)


def emulate_ce(z, lab, weight, ignore_index, g, nb):
    N, C, V = z.shape
    y = lab.reshape(N, V).to(torch.int32).long()
    counted = (y != ignore_index) & (y >= 0) & (y < C)
    yc = torch.where(counted, y, torch.zeros_like(y))
    w = torch.ones(C) if weight is None else torch.tensor(weight, dtype=torch.float32)
    m = z.max(1).values
    e = torch.exp(z - m[:, None])
    se = torch.zeros_like(m)
    for c in range(C):
        se = se + e[:, c]
    lse = m + torch.log(se)
    wy = w[yc] * counted
    term = wy * (lse - torch.gather(z, 1, yc[:, None])[:, 0]) * counted
    S_nll = sum(_block_reduce(_thread_sums(term[n].reshape(V, 1), nb), True).double().sum() for n in range(N))
    S_w = sum(_block_reduce(_thread_sums(wy[n].reshape(V, 1), nb), True).double().sum() for n in range(N))
    loss = (S_nll / S_w).float()
    k0 = (torch.tensor(g, dtype=torch.float64) / S_w).float()
    k = torch.where(counted, k0 * w[yc], torch.zeros(()))
    inv = 1.0 / se
    oh = F.one_hot(yc, C).permute(0, 2, 1).float() * counted[:, None]
    grad = k[:, None] * (e * inv[:, None] - oh)
    return loss, grad, torch.stack([S_nll, S_w])


# ---- the references ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch_dice", [True, False])
@pytest.mark.parametrize("w_ce,w_dice", MIXES)
def test_binary_reference_is_the_kernels_a_b_c_form(w_ce, w_dice, batch_dice):
    """loss_bounds.reference in channel mode with C = 1 against the a / b / c statement of the kernels, N = 3 samples of 5 x 7 x 9."""
    z, t = PB.seg_fixture(_gen(1), 315, N=3)
    ref = PB.seg_reference(z, t, w_ce=w_ce, w_dice=w_dice, batch_dice=batch_dice, g=G_UP)
    cf = PB.seg_closed_form(z, t, w_ce=w_ce, w_dice=w_dice, batch_dice=batch_dice, g=G_UP)
    assert abs(ref["loss"].item() - cf["loss"].item()) < 1e-14
    assert (ref["grad"] - cf["grad"]).abs().max().item() < 1e-15 * max(1.0, ref["grad"].abs().max().item())
    assert torch.equal(ref["counts"], cf["counts"]) and (ref["sums6"] - cf["sums6"]).abs().max().item() < 1e-9
    if w_ce == 0:
        assert abs(ref["loss"].item() - LO.dice(z.double(), t.double(), PB.f32(1e-5), batch_dice).item()) < 1e-14
    elif w_dice == 0:
        assert abs(ref["loss"].item() - F.binary_cross_entropy_with_logits(z.double(), t.double()).item()) < 1e-14


@pytest.mark.parametrize("spec,weights", [(PB.SPEC_BCD_MSE, (1, 1, 1)), (PB.SPEC_BCD_L1, (0.5, 0.25, 2)), (PB.SPEC_ALL8, PB.WEIGHTS_ALL8)])
def test_channel_reference_equals_fp64_autograd_and_the_oracle(spec, weights):
    z, t, planted = PB.chan_fixture(_gen(2), 2, spec, 1029)
    ref = PB.chan_reference(z, t, spec, weights, g=G_UP)
    zz = z.double().requires_grad_(True)
    acts = [a if k != "bce" else "linear" for k, a in spec]
    lo = LO.instance_channels(LO.apply_head_activations(zz, acts), t.double(), [k for k, _ in spec], list(weights))
    # the oracle casts to float32 inside: agreement at fp32 level; the plain formulas in float64 exactly
    assert abs(ref["loss"].item() - lo.item()) < 2e-6 * abs(lo.item())
    total = 0
    for c, (k, a) in enumerate(spec):
        x = zz[:, c]
        x = torch.tanh(x) if (a == "tanh" and k != "bce") else torch.sigmoid(x) if (a == "sigmoid" and k != "bce") else x
        lt = F.binary_cross_entropy_with_logits(x, t[:, c].double(), reduction="none") if k == "bce" else (x - t[:, c].double()) ** 2 if k == "mse" else (x - t[:, c].double()).abs()
        total = total + weights[c] * lt.mean()
    (G_UP * total).backward()
    assert abs(ref["loss"].item() - total.item()) < 1e-13
    assert (ref["grad"] - zz.grad).abs().max().item() < 1e-15
    assert bool((ref["grad"][planted] == 0).all())                      # d |d| / d d = 0 at d = 0, as torch's sign


@pytest.mark.parametrize("C", [2, 3, 5, 8])
@pytest.mark.parametrize("ignore_index", [-100, 255])
def test_ce_reference_equals_the_oracle_and_fp64_autograd(C, ignore_index):
    z, lab, _ = PB.ce_fixture(_gen(3 + C), 2, C, 1029, ignore_index)
    y = lab[:, 0].long()
    counted = (y != ignore_index) & (y >= 0) & (y < C)
    lab_in = torch.where(counted[:, None], lab, torch.full_like(lab, float(ignore_index)))          # the oracle knows ignore_index only
    for weight in (None, PB.CE_WEIGHTS[C]):
        ref = PB.ce_reference(z, lab, weight, ignore_index, g=G_UP)
        w64 = None if weight is None else torch.tensor(weight, dtype=torch.float32).double()
        zz = z.double().requires_grad_(True)
        lo = LO.softmax_ce(zz, lab_in, w64, ignore_index)
        assert abs(ref["loss"].item() - lo.item()) < 1e-13
        la = F.cross_entropy(zz, torch.where(counted, y, torch.full_like(y, -100)), weight=w64, ignore_index=-100)
        (G_UP * la).backward()
        assert abs(ref["loss"].item() - la.item()) < 1e-13
        assert (ref["grad"] - zz.grad).abs().max().item() < 1e-15
        assert bool((ref["grad"][~counted[:, None].expand_as(ref["grad"])] == 0).all())
    assert torch.equal(ref["counts"], LO.confusion_counts(z.double(), lab_in, ignore_index))


def test_ce_all_ignored_reference():
    z, lab, _ = PB.ce_fixture(_gen(9), 2, 3, 1029)
    ref = PB.ce_reference(z, torch.full_like(lab, -100.0), None, -100, g=G_UP)
    assert torch.isnan(ref["loss"]) and ref["grad"].abs().max().item() == 0.0 and ref["counts"].sum().item() == 0


# ---- a correct fp32 evaluation in the kernels' order lies inside the bounds ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SEG_SMALL)
def test_binary_emulation_within_bounds(n):
    lib = _lib()
    B = lib.bpx_seg_loss_blocks(n)
    z, t = PB.seg_fixture(_gen(PB.seg_seed(n)), n)
    worst = 0.0
    for w_ce, w_dice in MIXES:
        ref = PB.seg_reference(z, t, w_ce=w_ce, w_dice=w_dice, g=G_UP)
        bnd = PB.seg_bounds(ref, B)
        assert all(bool(torch.isfinite(v).all()) for v in (bnd["sums"], bnd["loss"], bnd["grad"]))
        loss, dz, S = emulate_seg(z, t, w_ce, w_dice, PB.f32(1e-5), G_UP, B)
        rows = PB.seg_check(f"seg n{n} {w_ce:g}/{w_dice:g}", loss, dz, S, ref, bnd)
        assert _ok(rows), rows
        worst = max(worst, _worst(rows))
        # the same gradient handed back in bf16 lies inside the bound that includes the bf16 rounding - and not always inside the fp32 one
        rows16 = PB.seg_check("bf16", None, dz.bfloat16(), None, ref, PB.seg_bounds(ref, B, grad_unit=PB.BF16))
        assert _ok(rows16), rows16
    print(f"plain_losses_cpu[seg n={n}] worst emulation err/bound = {worst:.3e}")


def test_binary_per_sample_emulation_within_bounds():
    """Per-sample Dice on (3, 1, 5, 7, 9): three calls of 315 elements with the upstream gradient g / 3 formed in fp32."""
    lib = _lib()
    z, t = PB.seg_fixture(_gen(20), 315, N=3)
    ref = PB.seg_reference(z, t, w_ce=0.0, w_dice=1.0, batch_dice=False, g=G_UP)
    bnd = PB.seg_bounds(ref, lib.bpx_seg_loss_blocks(315), gup_rel=2.0)
    g3 = (torch.tensor(G_UP, dtype=torch.float32) / 3).item()
    parts = [emulate_seg(z[i], t[i], 0.0, 1.0, PB.f32(1e-5), g3, lib.bpx_seg_loss_blocks(315)) for i in range(3)]
    loss = torch.stack([p[0] for p in parts]).mean()
    rows = PB.seg_check("per-sample", loss, torch.stack([p[1] for p in parts]), None, ref, bnd)
    assert _ok(rows), rows
    print(f"plain_losses_cpu[seg per-sample] worst emulation err/bound = {_worst(rows):.3e}")


CHAN_SETS = [("bcd_mse", PB.SPEC_BCD_MSE, (1, 1, 1)), ("bcd_l1", PB.SPEC_BCD_L1, (0.5, 0.25, 2)), ("all8", PB.SPEC_ALL8, PB.WEIGHTS_ALL8)]


@pytest.mark.parametrize("vox", VOX_SMALL)
@pytest.mark.parametrize("name,spec,weights", CHAN_SETS)
def test_channel_emulation_within_bounds(name, spec, weights, vox):
    nb = _lib().bpx_chan_loss_blocks(vox)
    z, t, planted = PB.chan_fixture(_gen(PB.chan_seed(vox)), 2, spec, vox)
    ref = PB.chan_reference(z, t, spec, weights, g=G_UP)
    bnd = PB.chan_bounds(ref, nb)
    assert all(bool(torch.isfinite(bnd[k]).all()) for k in ("sums", "loss", "grad"))
    loss, grad, sums = emulate_chan(z, t, spec, weights, G_UP, nb)
    rows = PB.chan_check(f"chan {name} vox{vox}", loss, grad, sums, ref, bnd)
    assert _ok(rows), rows
    assert bool((grad[planted] == 0).all())
    print(f"plain_losses_cpu[chan {name} vox={vox}] worst emulation err/bound = {_worst(rows):.3e}")


@pytest.mark.parametrize("vox", VOX_SMALL)
@pytest.mark.parametrize("C", [2, 3, 5, 8])
def test_ce_emulation_within_bounds(C, vox):
    nb = _lib().bpx_softmax_ce_blocks(vox)
    z, lab, _ = PB.ce_fixture(_gen(PB.ce_seed(C)), 2, C, vox, 255)
    worst = 0.0
    for weight in (None, PB.CE_WEIGHTS[C]):
        ref = PB.ce_reference(z, lab, weight, 255, g=G_UP)
        bnd = PB.ce_bounds(ref, nb)
        assert all(bool(torch.isfinite(bnd[k]).all()) for k in ("S_nll", "S_w", "loss", "grad"))
        loss, grad, sums = emulate_ce(z, lab, weight, 255, G_UP, nb)
        got = torch.cat([sums, torch.nn.functional.pad(ref["counts"], (0, 8 - C)).reshape(-1)])
        rows = PB.ce_check(f"ce C{C} vox{vox}", loss, grad, got, ref, bnd)
        assert _ok(rows), rows
        worst = max(worst, _worst(rows))
    print(f"plain_losses_cpu[ce C={C} vox={vox}] worst emulation err/bound = {worst:.3e}")


# ---- the comparator rejects every simulated fault ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", PB.SEG_FAULTS)
def test_binary_comparator_rejects(fault):
    """Each fault evaluated in float64 (no rounding at all) on a GPU fixture: 1027 (a tail of 3), the wrapping size for wrap_skipped, and the
    (3, 1, 5, 7, 9) batch - summed over the batch - where the element count and the voxel count differ."""
    lib = _lib()
    n, N = (SEG_WRAP, 1) if fault == "wrap_skipped" else (315, 3) if fault == "ce_mean_over_vox_not_numel" else (1027, 1)
    z, t = PB.seg_fixture(_gen(50), n, N=N)
    B = lib.bpx_seg_loss_blocks(n * N)
    kw = dict(w_ce=PB.f32(0.7), w_dice=PB.f32(1.3), g=G_UP)
    ref = PB.seg_reference(z, t, **kw)
    bnd = PB.seg_bounds(ref, B)
    bad = PB.seg_closed_form(z, t, fault=fault, blocks=B, bwd_blocks=min(-(-(n // 4 + 1) // 256), 4096), **kw)
    good = PB.seg_closed_form(z, t, **kw)
    assert _ok(PB.seg_check(fault, good["loss"], good["grad"], good["sums6"], ref, bnd))
    rows = PB.seg_check(fault, bad["loss"], bad["grad"], bad["sums6"], ref, bnd)
    assert not _ok(rows), rows
    if fault != "log1p_as_log":                                         # a fault of the loss value alone
        assert not _ok([r for r in rows if r["name"].endswith(".grad")]), rows


@pytest.mark.parametrize("fault", PB.CHAN_FAULTS)
def test_channel_comparator_rejects(fault):
    nb = _lib().bpx_chan_loss_blocks(1029)
    spec, weights = (PB.SPEC_ALL8, PB.WEIGHTS_ALL8) if fault == "l1_sign_at_zero" else (PB.SPEC_BCD_L1, (0.5, 0.25, 2)) if fault != "mse_factor_two_missing" else (PB.SPEC_BCD_MSE, (1, 1, 1))
    z, t, _ = PB.chan_fixture(_gen(60), 2, spec, 1029)
    ref = PB.chan_reference(z, t, spec, weights, g=G_UP)
    bnd = PB.chan_bounds(ref, nb)
    assert _ok(PB.chan_check(fault, ref["loss"], ref["grad"], ref["sums"], ref, bnd))
    bad = PB.chan_reference(z, t, spec, weights, g=G_UP, fault=fault)
    rows = PB.chan_check(fault, bad["loss"], bad["grad"], bad["sums"], ref, bnd)
    assert not _ok([r for r in rows if r["name"].endswith(".grad")]), rows


@pytest.mark.parametrize("fault", PB.CE_FAULTS)
def test_ce_comparator_rejects(fault):
    C = 5
    nb = _lib().bpx_softmax_ce_blocks(1029)
    z, lab, _ = PB.ce_fixture(_gen(70), 2, C, 1029)
    ref = PB.ce_reference(z, lab, PB.CE_WEIGHTS[C], -100, g=G_UP)
    bnd = PB.ce_bounds(ref, nb)

    def row(r):
        return torch.cat([torch.stack([r["S_nll"], r["S_w"]]), torch.nn.functional.pad(r["counts"], (0, 8 - C)).reshape(-1)])

    assert _ok(PB.ce_check(fault, ref["loss"], ref["grad"], row(ref), ref, bnd))
    bad = PB.ce_reference(z, lab, PB.CE_WEIGHTS[C], -100, g=G_UP, fault=fault)
    rows = PB.ce_check(fault, bad["loss"], bad["grad"], row(bad), ref, bnd)
    assert not _ok(rows), rows
    if fault == "ignored_gets_gradient":
        assert not [r for r in rows if r["name"].endswith("uncounted_zero")][0]["ok"]
    if fault == "argmax_last_maximum":
        assert not [r for r in rows if r["name"].endswith(".counts")][0]["ok"]             # only the planted ties tell the two apart


# ---- what the fixtures promise -----------------------------------------------------------------------------------------------------------------------------
def test_binary_fixtures_keep_their_promise():
    for n in SEG_SMALL + (SEG_WRAP,):
        z, t = PB.seg_fixture(_gen(PB.seg_seed(n)), n)
        near, zeros = PB.seg_fixture_condition(z)
        assert near == 0 and zeros == (2 if n >= 12 else 1), (n, near, zeros)
        assert set(t.unique().tolist()) <= {0.0, 0.25, 0.5, 1.0}
        if n >= 12:
            assert all(bool((z == v).any()) for v in PB.SEG_PLANTED) and bool((t == 0.5).any()) and bool((t == 0.25).any())
            assert float(z[0, 0, -1]) == -1e4                          # a saturated value in the tail
    lib = _lib()
    z, t = PB.seg_fixture(_gen(PB.seg_seed(SEG_WRAP)), SEG_WRAP)                # the wrapping size: no bound infinite or NaN there either
    bnd = PB.seg_bounds(PB.seg_reference(z, t, w_ce=PB.f32(0.7), w_dice=PB.f32(1.3), g=G_UP), lib.bpx_seg_loss_blocks(SEG_WRAP))
    assert all(bool(torch.isfinite(v).all()) for v in (bnd["sums"], bnd["loss"], bnd["grad"]))
    assert SEG_WRAP > 4 * 256 * 4096 and lib.bpx_seg_loss_blocks(SEG_WRAP) == 2048 and SEG_WRAP % 4 == 3
    assert PB.seg_chain(SEG_WRAP, 2048) == 4 * 3 + 10 and PB.seg_chain(3, 1) == 10 and PB.seg_chain(1027, 1) == 14
    assert lib.bpx_seg_loss_blocks(3) == 1 and lib.bpx_seg_loss_blocks(1027) == 1 and lib.bpx_seg_loss_blocks(4096) == 4


def test_ce_fixtures_keep_their_promise():
    for C in (2, 3, 5, 8):
        for ii in (-100, 255):
            for vox in (1029, VOX_WRAP):
                z, lab, ties = PB.ce_fixture(_gen(PB.ce_seed(C)), 2, C, vox, ii)
                share, present, exact = PB.ce_fixture_condition(z, lab, C, ii, ties)
                assert share >= 0.85 and present and exact and len(ties) == 3, (C, ii, vox, share, present, exact)
                assert not bool((lab == C - 1).any()) and bool((lab == C + 1).any()) and bool((lab == ii).any())
                if ii == 255 and C in (2, 8):
                    bnd = PB.ce_bounds(PB.ce_reference(z, lab, PB.CE_WEIGHTS[C], ii, g=G_UP), _lib().bpx_softmax_ce_blocks(vox))
                    assert all(bool(torch.isfinite(bnd[k]).all()) for k in ("S_nll", "S_w", "loss", "grad"))
    lib = _lib()
    assert lib.bpx_softmax_ce_blocks(VOX_WRAP) == 512 == lib.bpx_chan_loss_blocks(VOX_WRAP) and VOX_WRAP > 256 * 1024
    assert PB.ce_chain(VOX_WRAP, 512) == 5 + 8 and PB.chan_chain(1029, 2) == 3 + 9 and PB.chan_chain(1, 1) == 10


@pytest.mark.parametrize("name,spec,weights", CHAN_SETS)
def test_channel_fixtures_keep_their_promise(name, spec, weights):
    """At most 0.1 % of an L1 channel's elements have a sign the bound cannot decide, the planted z == t elements apart (they are decided: both are 0)."""
    for vox in (1029, VOX_WRAP):
        z, t, planted = PB.chan_fixture(_gen(PB.chan_seed(vox)), 2, spec, vox)
        ref = PB.chan_reference(z, t, spec, weights, g=G_UP)
        bnd = PB.chan_bounds(ref, _lib().bpx_chan_loss_blocks(vox))
        assert all(bool(torch.isfinite(bnd[k]).all()) for k in ("sums", "loss", "grad"))
        for c, (kind, act) in enumerate(spec):
            und = bnd["undecided"][:, c]
            assert not bool((und & planted[:, c]).any())
            assert und.double().mean().item() <= 1e-3, (name, c, und.double().mean().item())
            if kind != "bce" and act == "tanh":
                assert bool((ref["ch"][c]["da"][:, 0] < 1e-16).all()) and float(z[0, c, vox - 1]) == -20.0
            if kind == "l1" and act == "linear":
                assert int(planted[:, c].sum()) == 8 and bool((z[:, c][planted[:, c]] == t[:, c][planted[:, c]]).all())


# ---- the host side -------------------------------------------------------------------------------------------------------------------------------------------
def test_prep_hands_the_kernels_16_byte_aligned_tensors():
    """A batch slice of a (3, 1, 5, 7, 9) tensor is contiguous and starts 4 * 315 i bytes into its base: sample 1 is not 16-byte aligned.  _aligned16
    copies exactly those; an aligned tensor passes through untouched."""
    from biapy_amd import losses as Ls
    x = torch.randn(3, 1, 5, 7, 9)
    assert x.data_ptr() % 16 == 0 and x[1:2].is_contiguous() and x[1:2].data_ptr() % 16 != 0
    for i in range(3):
        s = x[i:i + 1]
        a = Ls._aligned16(s)
        assert a.data_ptr() % 16 == 0 and a.is_contiguous() and a.dtype == torch.float32 and torch.equal(a, s)
        assert (a.data_ptr() == s.data_ptr()) == (s.data_ptr() % 16 == 0)
    y = torch.randn(3, 1, 6, 10, 12)
    assert all(Ls._aligned16(y[i:i + 1]).data_ptr() == y[i:i + 1].data_ptr() for i in range(3))
    h = torch.randn(2, 1, 7, 5).bfloat16()
    assert Ls._aligned16(h).dtype == torch.float32 and torch.equal(Ls._aligned16(h), h.float())
    v = torch.randn(1, 1, 8, 12).permute(0, 1, 3, 2)
    assert Ls._aligned16(v).is_contiguous() and torch.equal(Ls._aligned16(v), v)
    with pytest.raises(RuntimeError, match="MI355X only"):
        Ls._prep(x, x)


def test_the_direct_backward_entry_points_are_bound():
    from biapy_amd import _lib as L
    for sym in ("bpx_seg_loss_bwd", "bpx_chan_loss_bwd"):
        assert sym in L.EXPORTS and getattr(L.lib._raw, sym) is not None
    assert L.lib.bpx_seg_loss_bwd(None, None, 4, None, None, None) != 0 and b"null pointer" in L.lib.bpx_last_error()
    assert L.lib.bpx_chan_loss_bwd(None, None, 1, 1, 4, 0, None, None, None) != 0 and b"null pointer" in L.lib.bpx_last_error()
    assert PB.chan_codes(PB.SPEC_BCD_MSE) == 0 | 0 << 4 | (1 | 1 << 2) << 8 and math.isclose(PB.f32(0.7), 0.699999988079071)

"""The bounds of tests/norm_bounds.py on the CPU: an fp64 simulation of a CORRECT kernel (operands rounded where the kernel rounds them, one
final rounding) passes each bound with err > 0 at every storage type, injected kernel faults fail it, three of them are shown to pass the
whole-tensor relerr bars of tests/kernel_checks.py, and the host functions answer what the GPU rows of tests/test_norm_bounds_gpu.py assume
for their shapes.  No GPU: the faults are injected into the simulations, and the host checks return before any launch."""
import pytest
import torch

import conv_bounds as CB
import norm_bounds as NB

MODES = ("f32", "bf16", "mix16")
SIXTEEN = ("bf16", "mix16")
_CACHE = {}


def _relerr(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- the 1x1x1 GEMM with the IN-backward affine -------------------------------------------------------------------------------------------
AFF_B, AFF_V, AFF_K = 2, 1024, 16


def _affine(x, w, g, t, coef):
    return x @ w.t() + coef[:, None, :, 0].double() * g + coef[:, None, :, 1].double() * t + coef[:, None, :, 2].double()


def affine_case(mode):
    """The operands kernel_checks.check_pw_stream draws (coefficient scales 1, 0.3 and 0.03: b and c0 are means over a sample), B 2 x 1024
    voxels, 16 -> 48 columns, split at 32."""
    def make():
        gk, tk = NB.MODES[mode]
        gen = torch.Generator().manual_seed(0)
        C3 = 3 * AFF_K
        x = CB.round_to(torch.randn(AFF_B, AFF_V, AFF_K, generator=gen), gk)
        w = CB.round_to(torch.randn(C3, AFF_K, generator=gen) / AFF_K ** 0.5, gk)
        g = CB.round_to(torch.randn(AFF_B, AFF_V, C3, generator=gen), gk)
        t = CB.round_to(torch.randn(AFF_B, AFF_V, C3, generator=gen) * 2, tk)
        coef = (torch.randn(AFF_B, C3, 4, generator=gen) * torch.tensor([1.0, 0.3, 0.03, 0.0])).float()
        ref, bound = NB.affine_reference(x, w, g, t, coef, out_kind=gk)
        return dict(x=x, w=w, g=g, t=t, coef=coef, ref=ref, bound=bound, kind=gk, good=CB.round_to(_affine(x, w, g, t, coef), gk))
    return _cached(("affine", mode), make)


def aff_neighbour_coef(c):
    """Fault 1: the coefficients of sample n used for the first 128-voxel block of sample n + 1."""
    v = _affine(c["x"], c["w"], c["g"], c["t"], c["coef"])
    v[1, :128] = _affine(c["x"][1:, :128], c["w"], c["g"][1:, :128], c["t"][1:, :128], c["coef"][:1])[0]
    return CB.round_to(v, c["kind"])


def aff_dropped_c0(c):
    """Fault 2: c0 dropped on the first 16-channel chunk of the y_hi part (columns 32..47 of a split at 32) only."""
    v = _affine(c["x"], c["w"], c["g"], c["t"], c["coef"])
    v[:, :, 32:48] -= c["coef"][:, None, 32:48, 2].double()
    return CB.round_to(v, c["kind"])


def aff_stale_stage(c):
    """Fault 3: one 64-voxel block computed from the block that precedes it by the ring depth (4): a stale LDS stage."""
    v = _affine(c["x"], c["w"], c["g"], c["t"], c["coef"])
    s, d = slice(6 * 64, 7 * 64), slice(2 * 64, 3 * 64)
    v[0, s] = _affine(c["x"][:1, d], c["w"], c["g"][:1, d], c["t"][:1, d], c["coef"][:1])[0]
    return CB.round_to(v, c["kind"])


def aff_truncating_store(c):
    """Fault 7: the 16-bit store truncates instead of rounding to nearest even."""
    return NB.trunc_to(_affine(c["x"], c["w"], c["g"], c["t"], c["coef"]), c["kind"])


def aff_unwritten(c):
    """Fault 8: one element never written."""
    v = c["good"].clone()
    v[1, 1023, 47] = float("nan")
    return v


AFF_FAULTS = {"neighbour_sample_coefficients": aff_neighbour_coef, "c0_dropped_on_a_y_hi_chunk": aff_dropped_c0, "stale_lds_stage": aff_stale_stage,
              "unwritten_element": aff_unwritten}


@pytest.mark.parametrize("mode", MODES)
def test_affine_correctly_rounded_result_passes(mode):
    c = affine_case(mode)
    r = NB.compare("correct", c["good"], c["ref"], c["bound"], axes="nvc")
    assert r["ok"] and r["err"] > 0.0, r


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fault", sorted(AFF_FAULTS))
def test_affine_fault_fails(mode, fault):
    c = affine_case(mode)
    assert not NB.compare(fault, AFF_FAULTS[fault](c), c["ref"], c["bound"], axes="nvc")["ok"]


@pytest.mark.parametrize("mode", SIXTEEN)
def test_affine_truncating_store_fails(mode):
    c = affine_case(mode)
    assert not NB.compare("trunc", aff_truncating_store(c), c["ref"], c["bound"], axes="nvc")["ok"]


@pytest.mark.parametrize("fault", [aff_truncating_store, aff_dropped_c0], ids=["truncating_store", "dropped_small_c0"])
def test_affine_fault_passes_the_old_relerr_bar(fault):
    """Why these checks exist: against the whole-tensor bar of kernel_checks.check_pw_stream (relerr <= 1.5e-2 at bf16) a truncating store
    and a c0 dropped on 16 of the 48 columns both pass, while the element-wise bound rejects them."""
    c = affine_case("mix16")
    got = fault(c)
    assert _relerr(got, c["ref"]) < 1.5e-2
    assert NB.compare("old bar", got, c["ref"], c["bound"], axes="nvc")["err"] > 1.0


# ---- S1 / S2 partial sums ----------------------------------------------------------------------------------------------------------------
RED_B, RED_TILES, RED_C = 2, 8, 16


def red_case(mode, weak_channel=None):
    """norm_act_bwd's product g = dy ELU'(scale x + shift) over 8 rows of 256 voxels, gamma != 1 (conv_bounds.norm_recs draws 1 + 0.2 randn).
    The simulated correct kernel rounds every term to fp32 and sums each row exactly.  weak_channel: that channel's dy is 100 x smaller."""
    def make():
        gk, tk = NB.MODES[mode]
        gen = torch.Generator().manual_seed(3)
        V = RED_TILES * 256
        dy = torch.randn(RED_B, V, RED_C, generator=gen)
        if weak_channel is not None:
            dy[..., weak_channel] *= 0.01
        dy = CB.round_to(dy, gk)
        x = CB.round_to(torch.randn(RED_B, V, RED_C, generator=gen), tk)
        rec = CB.norm_recs(RED_B, RED_C, gen)
        _, _, gv, egv = NB.norm_act_bwd_reference(dy, x, rec, 1, None, gk)
        s, bound = NB.red_reference(gv, egv, x, rec, NB.norm_act_bwd_chain(V, RED_C, gk, RED_TILES))
        xh, _ = NB.xhat_terms(x, rec)
        f32 = lambda v: v.float().double()
        rows = torch.stack([f32(gv).reshape(RED_B, RED_TILES, 256, RED_C).sum(2), f32(f32(gv) * f32(xh)).reshape(RED_B, RED_TILES, 256, RED_C).sum(2)], 2)
        return dict(gv=gv, x=x, rec=rec, s=s, bound=bound, rows=rows)
    return _cached(("red", mode, weak_channel), make)


@pytest.mark.parametrize("mode", MODES)
def test_partial_sums_correct_rows_pass_and_faults_fail(mode):
    """Fault 4: one partial row missing from S2 of one channel; S2 formed with `scale` in place of `rstd` (gamma != 1)."""
    c = red_case(mode)
    r = NB.compare("correct", c["rows"].sum(1), c["s"], c["bound"], axes="nkc")
    assert r["ok"] and r["err"] > 0.0, r
    lost = c["rows"].clone()
    lost[1, 5, 1, 7] = 0.0
    assert not NB.compare("lost row", lost.sum(1), c["s"], c["bound"], axes="nkc")["ok"]
    r64 = c["rec"].double()
    wrong = c["s"].clone()
    wrong[:, 1] = (c["gv"] * (c["x"] - r64[:, None, :, 0]) * r64[:, None, :, 2]).sum(1)
    assert not NB.compare("scale for rstd", wrong, c["s"], c["bound"], axes="nkc")["ok"]
    nan = c["rows"].sum(1)
    nan[0, 0, 3] = float("nan")
    assert not NB.compare("unwritten", nan, c["s"], c["bound"], axes="nkc")["ok"]


def test_a_lost_s2_channel_passes_the_old_relerr_bar():
    """One channel's S2 lost entirely, that channel's gradient 100 x smaller than the others': under the whole-tensor bar of the reductions
    (kernel_checks: relerr <= 1e-2) it passes; per (sample, sum, channel) it fails."""
    c = red_case("bf16", weak_channel=5)
    got = c["rows"].sum(1)
    got[:, 1, 5] = 0.0
    assert _relerr(got, c["s"]) < 1e-2
    assert not NB.compare("lost channel", got, c["s"], c["bound"], axes="nkc")["ok"]


# ---- records and coefficients ---------------------------------------------------------------------------------------------------------
def _f32(v):
    return v.float().double()


def rec_case(tiles, cpg, C=16, N=3):
    def make():
        gen = torch.Generator().manual_seed(tiles + cpg)
        part = torch.randn(N, tiles, 2, C, generator=gen) * 4
        part[:, :, 0] += torch.randn(C, generator=gen) * 8           # channel means that differ
        part[:, :, 1] = part[:, :, 1].abs() * 8 + 260.0              # sum x^2 >= (sum x)^2 / n with room: a positive variance
        gamma, beta = 1 + 0.2 * torch.randn(C, generator=gen), 0.2 * torch.randn(C, generator=gen)
        count = 256
        ref, bound, ok = NB.records_reference(part, count * tiles, gamma, beta, 1e-5, cpg)
        return dict(part=part, gamma=gamma, beta=beta, count=count * tiles, ref=ref, bound=bound, ok=ok, cpg=cpg)
    return _cached(("rec", tiles, cpg, C, N), make)


def _simulated_records(c, mean_of=None):
    """The kernel's last lines in fp32 on the fp64 totals.  mean_of(S1, n): the mean that enters `shift` (fault 5)."""
    S = c["part"].double().sum(1)
    cpg, n = c["cpg"], float(c["count"]) * c["cpg"]
    m = NB.group_fold(S[:, 0], cpg) / n
    v = (NB.group_fold(S[:, 1], cpg) / n - m * m).clamp_min(0)
    rstd = _f32((v + 1e-5).rsqrt())
    ga, be = c["gamma"].float().double()[None], c["beta"].float().double()[None]
    scale = _f32(ga * rstd)
    ms = _f32(m) if mean_of is None else mean_of(S[:, 0])
    shift = _f32(be - _f32(_f32(ms * ga) * rstd))
    return torch.stack([_f32(m), rstd, scale, shift], -1)


@pytest.mark.parametrize("tiles,cpg", [(7, 1), (7, 4), (1025, 1), (1025, 16)])
def test_records_correct_pass_and_shift_with_a_channel_mean_fails(tiles, cpg):
    """Fault 5: `shift` of a GroupNorm record formed with the unrounded mean of ANOTHER channel of the same group (that channel's own S1 /
    count instead of the group's total).  For InstanceNorm (cpg 1) the neighbouring channel's mean plays that part."""
    c = rec_case(tiles, cpg)
    assert c["ok"], "the reference must satisfy dv < (v + eps) / 2"
    r = NB.compare("correct", _simulated_records(c), c["ref"], c["bound"], axes="ncf")
    assert r["ok"] and r["err"] > 0.0, r
    other = lambda S1: S1.roll(1, -1) / float(c["count"]) if cpg == 1 else (S1.reshape(S1.shape[0], -1, cpg).roll(1, -1).reshape(S1.shape) / float(c["count"]))
    assert not NB.compare("other mean", _simulated_records(c, other), c["ref"], c["bound"], axes="ncf")["ok"]


def test_compacted_partials_bound_admits_the_float_segment_totals_only_above_1024_tiles():
    """compact_stats writes segment totals back as floats above 1024 tiles: the simulated kernel with that rounding passes at 1025 tiles, and
    the same rounding injected at 1024 tiles (where the kernel does not compact) is rejected."""
    for tiles, admitted in ((1025, True), (1024, False)):
        c = rec_case(tiles, 1)
        p = c["part"].double()
        seg = -(-tiles // 32)
        pad = torch.zeros(p.shape[0], -(-tiles // seg) * seg - tiles, 2, p.shape[-1], dtype=p.dtype)
        S = _f32(torch.cat([p, pad], 1).reshape(p.shape[0], -1, seg, 2, p.shape[-1]).sum(2)).sum(1)
        S0, d = NB.row_totals(c["part"])
        assert bool(((S - S0).abs() <= d).all()) == admitted, tiles


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("cpg", [1, 4])
def test_coefficients_and_parameter_gradients(cpg, deferred):
    """Coefficients from given partials pass when rounded once; a and c0 swapped-sample faults fail; dgamma / dbeta ADD to what the buffers hold:
    an entry that overwrites a non-zero buffer fails."""
    N, T, C = 5, 7, 16
    gen = torch.Generator().manual_seed(9)
    part = torch.randn(N, T, 2, C, generator=gen)
    rec, gamma = CB.norm_recs(N, C, gen), 1 + 0.2 * torch.randn(C, generator=gen)
    S, d = NB.row_totals(part)
    ref, bound = NB.coef_from_totals(S, d, rec, gamma, 4096, cpg)
    good = _f32(ref)
    r = NB.compare("correct", good, ref, bound, axes="nck")
    assert r["ok"] and r["err"] > 0.0, r
    assert not NB.compare("neighbour sample", good.roll(1, 0), ref, bound, axes="nck")["ok"]
    init_g, init_b = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    (dg, bg), (db, bb) = NB.param_grads_from_totals(S, d, init_g, init_b, deferred)
    sim = _f32(init_g.double() + _f32(_f32(S[:, 1]).sum(0)))
    r = NB.compare("dgamma", sim, dg, bg, axes="c")
    assert r["ok"], r
    assert not NB.compare("dgamma overwritten", _f32(_f32(S[:, 1]).sum(0)), dg, bg, axes="c")["ok"]
    assert not NB.compare("dbeta overwritten", _f32(_f32(S[:, 0]).sum(0)), db, bb, axes="c")["ok"]


# ---- norm_bwd_apply, norm_act fwd / bwd -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_apply_and_norm_act_correct_pass_truncated_and_unwritten_fail(mode):
    gk, tk = NB.MODES[mode]
    gen = torch.Generator().manual_seed(5)
    B, V, C = 2, 600, 48
    g = CB.round_to(torch.randn(B, V, C, generator=gen), gk)
    t = CB.round_to(torch.randn(B, V, C, generator=gen) * 2, tk)
    add = CB.round_to(torch.randn(B, V, C, generator=gen), gk)
    coef = (torch.randn(B, C, 4, generator=gen) * torch.tensor([1.0, 0.3, 0.03, 0.0])).float()
    rec = CB.norm_recs(B, C, gen)
    cases = [("apply", NB.apply_reference(g, t, coef, add, gk)[:2])]
    for act in range(9):
        cases.append((f"act_fwd{act}", NB.norm_act_fwd_reference(t, rec, act, tk)))
        cases.append((f"act_bwd{act}", NB.norm_act_bwd_reference(g, t, rec, act, add, gk)[:2]))
    for name, (ref, bound) in cases:
        kind = tk if name.startswith("act_fwd") else gk
        good = CB.round_to(ref, kind)
        r = NB.compare(name, good, ref, bound, axes="nvc")
        assert r["ok"], r
        assert r["err"] > 0.0 or name in ("act_fwd0", "act_fwd2") and kind == "f32" or name.startswith("act_fwd2"), r
        if kind != "f32":
            assert not NB.compare(name + " truncated", NB.trunc_to(ref, kind), ref, bound, axes="nvc")["ok"], name
        bad = good.clone()
        bad[1, 599, 47] = float("nan")
        assert not NB.compare(name + " unwritten", bad, ref, bound, axes="nvc")["ok"], name
    # fault 1 on the apply kernel: the neighbouring sample's coefficients
    ref, bound = NB.apply_reference(g, t, coef, add, gk)
    wrong = CB.round_to(NB.apply_reference(g, t, coef.roll(1, 0), add, gk)[0], gk)
    assert not NB.compare("apply neighbour sample", wrong, ref, bound, axes="nvc")["ok"]


# ---- pooling: bit for bit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sz", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_pooling_reference_ties_and_faults(sz, mode):
    """Fault 6: the last maximum wins a tie; the addend dropped on odd z planes; (MIX16) the gradient routed by the arg-max of the bf16-rounded
    x where x is fp16.  The inputs hold ties in more than half of the windows and every window position wins somewhere."""
    gk, tk = NB.MODES[mode]
    gdt, xdt = CB.TORCH_DT[gk], CB.TORCH_DT[tk]
    gen = torch.Generator().manual_seed(sz)
    x, dy, add = NB.pool_inputs(2, (4, 6, 8), 16, sz, xdt, gdt, gen)
    winners, tied = NB.pool_tie_stats(x, sz)
    assert winners == set(range(4 * sz)) and tied > 0.5, (winners, tied)
    y, am = NB.pool_fwd_reference(x, sz)
    good = NB.pool_bwd_reference(x, dy, add, sz)
    assert NB.exact_row("correct", good.clone(), good)["ok"]
    # the reference agrees with PyTorch's own pooling where PyTorch defines the result (values; -0 / +0 compare equal there)
    yt = torch.nn.functional.max_pool3d(x.float().permute(0, 4, 1, 2, 3), (sz, 2, 2)).permute(0, 2, 3, 4, 1)
    assert torch.equal(yt, y.float())
    last = NB.pool_bwd_reference(x, dy, add, sz, am=NB.pool_argmax(x, sz, last=True))
    assert not NB.exact_row("last maximum wins", last, good)["ok"]
    dropped = NB.pool_bwd_reference(x, dy, None, sz).float()
    dropped[:, 0::2] = good.float()[:, 0::2]
    assert not NB.exact_row("addend dropped on odd z", dropped.to(gdt), good)["ok"]
    unwritten = good.clone()
    unwritten[1, 3, 5, 7, 15] = float("nan")
    assert not NB.exact_row("unwritten", unwritten, good)["ok"]
    if mode == "mix16":
        # fp16 values that differ below bf16 precision: 1.5 and 1.5 + 2^-10 are one bf16 value
        x2 = x.clone()
        x2[:, :, :, 1::2, :] = torch.where(x2[:, :, :, 1::2, :] == 1.5, torch.tensor(1.5 + 2.0 ** -10, dtype=xdt), x2[:, :, :, 1::2, :])
        good2 = NB.pool_bwd_reference(x2, dy, add, sz)
        routed = NB.pool_bwd_reference(x2, dy, add, sz, am=NB.pool_argmax(x2.to(torch.bfloat16), sz))
        assert not NB.exact_row("arg-max of the bf16-rounded x", routed, good2)["ok"]


# ---- host side: the shapes of the GPU rows reach what they name ----------------------------------------------------------------------------
def _lib():
    from biapy_amd import _lib as L

    return L


def test_tile_counts_of_the_gpu_rows():
    L = _lib()
    lib = L.lib
    for vox, want in ((1, 1), (255, 1), (256, 1), (257, 2), (4096 + 77, 17)):
        assert lib.bpx_tensor_stats_tiles(vox) == want
    # norm_act: min(ceil(voxels G / 256), 512) rounded up to a multiple of G's odd part (a thread keeps its channel group)
    for dt, vox, C, want in ((L.BF16, 1, 16, 1), (L.BF16, 100, 48, 3), (L.BF16, 720, 80, 30), (L.F32, 720, 48, 36), (L.BF16, 10 ** 6, 48, 513)):
        assert lib.bpx_norm_act_tiles(dt, vox, C) == want, (dt, vox, C)
    # pooling: items = pooled voxels x channel groups, (256 / G) G threads x 4 items per row
    for dt, S, sz, C, want in ((L.BF16, (2, 2, 2), 2, 16, 1), (L.BF16, (4, 6, 8), 1, 48, 1), (L.BF16, (8, 12, 20), 2, 80, 3), (L.F32, (8, 12, 20), 2, 96, 6)):
        assert lib.bpx_maxpool3d_stats_tiles(dt, *S, sz, C) == want, (S, sz, C)


def test_streaming_rows_reach_the_streaming_kernel_and_tile_rows_do_not():
    """bpx_conv1x1_fwd_split_wgrad_workspace answers the shape classes pw_nbs_kernel takes: every PWS_ROWS shape, at BF16 and MIX16; none of
    the PW_ROWS shapes.  The walks the rows are meant to have follow from their block counts."""
    L = _lib()
    lib = L.lib
    for name, K, B, vps in NB.PWS_ROWS:
        for dt in (L.BF16, L.MIX16):
            assert lib.bpx_conv1x1_fwd_split_wgrad_workspace(dt, B, vps, K) == 256 * 3 * K * K * 4, name
        assert lib.bpx_conv1x1_fwd_split_wgrad_workspace(L.F32, B, vps, K) == 0
    for name, modes, B, vox, Cin, ncols, split, bias, addend, planar in NB.PW_ROWS:
        assert lib.bpx_conv1x1_fwd_split_wgrad_workspace(L.BF16, B, vox, Cin) == 0, name
    nb, bps = NB.pws_blocks(16, 3, 87424)
    assert (nb, bps, nb % 256, bps % 256 != 0) == (2049, 683, 1, True)
    nb, bps = NB.pws_blocks(32, 5, 52480)
    assert (nb, bps, nb % 256, bps % 256 != 0) == (4100, 820, 4, True)
    assert NB.pws_blocks(16, 1, 262144) == (2048, 2048) and NB.pws_blocks(32, 2, 131072) == (4096, 2048)
    assert lib.bpx_conv1x1_fwd_split_wgrad_workspace(L.BF16, 1, 262144 - 128, 16) == 0      # below the smallest admitted volume


@pytest.mark.parametrize("entry", ["bpx_maxpool3d_bwd", "bpx_maxpool3d_bwd_r1"])
@pytest.mark.parametrize("S,sz", [((3, 4, 4), 2), ((4, 5, 4), 2), ((4, 4, 7), 1)])
def test_pooling_backward_refuses_extents_the_window_does_not_divide(entry, S, sz):
    """A host-side check, as in bpx_maxpool3d_fwd: it returns before anything is launched (the pointers below are never dereferenced).  With an
    odd extent the kernel would leave the last plane / row / column of dx unwritten and lose the addend there."""
    L = _lib()
    lib = L.lib
    t = L.Tensor(4096, 16, 16, 0)
    if entry == "bpx_maxpool3d_bwd":
        rc = lib.bpx_maxpool3d_bwd(L.BF16, 1, *S, sz, t, t, t, t, None)
    else:
        rc = lib.bpx_maxpool3d_bwd_r1(L.BF16, 1, *S, sz, t, t, t, t, 4096, 4096, 4096, 1 << 20, None)
    assert rc != 0
    msg = lib.bpx_last_error().decode()
    assert "extents must be divisible by the window" in msg and entry in msg, msg

"""The bounds of tests/gate_bounds.py on the CPU: an fp64 simulation of a CORRECT kernel (operands rounded where the kernel rounds them, one
final rounding) passes each bound with err > 0 at every storage type, injected kernel faults fail it, four of them are shown to pass the
whole-tensor relative-error bar of 4e-3 (the tightest any network golden applies to these paths), the fp16 subnormal share of the gate
multiply stays under its cap for the reference alone, and the host functions answer what the GPU rows of tests/test_gate_bounds_gpu.py assume
for their shapes.  No GPU: the faults are injected into the simulations, and the host checks return before any launch."""
import pytest
import torch

import conv_bounds as CB
import gate_bounds as GB
import norm_bounds as NB

COARSE = 4e-3
NAN = float("nan")


def _relerr(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


def _f32(v):
    return v.float().double()


def _fails(rows):
    return any(not r["ok"] for r in rows)


# ---- channel_affine --------------------------------------------------------------------------------------------------------------------
def affine_case(kind, off_scale=0.3):
    gen = torch.Generator().manual_seed(1)
    B, V, C = 2, 600, 48
    h = CB.round_to(torch.randn(B, V, C, generator=gen), kind)
    x = CB.round_to(torch.randn(B, V, C, generator=gen), kind)
    s = torch.randn(B, C, generator=gen).float()
    off = (off_scale * torch.randn(B, C, generator=gen)).float()
    return h, x, s, off


@pytest.mark.parametrize("variant", ["x_off", "x_null", "off_null", "both_null"])
@pytest.mark.parametrize("kind", GB.ALL)
def test_channel_affine_correct_passes_and_faults_fail(kind, variant):
    h, x, s, off = affine_case(kind)
    x = x if variant in ("x_off", "off_null") else None
    off = off if variant in ("x_off", "x_null") else None
    ref, bound = GB.channel_affine_reference(h, s, off, x, kind)
    r = GB.compare("correct", CB.round_to(ref, kind), ref, bound, axes="nvc")
    assert r["ok"] and r["err"] > 0.0, r
    # sample n's scale used for sample n + 1
    wrong = CB.round_to(GB.channel_affine_reference(h, s.roll(1, 0), off, x, kind)[0], kind)
    assert not GB.compare("neighbour sample's scale", wrong, ref, bound, axes="nvc")["ok"]
    if off is not None:      # off dropped on one channel group (KPL channels)
        k = GB.kpl(kind)
        v = ref.clone()
        v[..., k:2 * k] -= off.double()[:, None, k:2 * k]
        assert not GB.compare("off dropped on a channel group", CB.round_to(v, kind), ref, bound, axes="nvc")["ok"]
    if kind != "f32":
        assert not GB.compare("truncating store", NB.trunc_to(ref, kind), ref, bound, axes="nvc")["ok"]
    bad = CB.round_to(ref, kind)
    bad[1, 599, 47] = NAN
    assert not GB.compare("unwritten", bad, ref, bound, axes="nvc")["ok"]


def test_channel_affine_faults_that_pass_the_coarse_bar():
    """Found to pass relerr <= 4e-3 over the whole tensor while the element-wise bound rejects them: a truncating fp16 store, and an offset of
    the backward's size (d mean / voxels: 0.01) dropped on one channel group at bf16."""
    h, x, s, off = affine_case("f16")
    ref, bound = GB.channel_affine_reference(h, s, off, x, "f16")
    got = NB.trunc_to(ref, "f16")
    assert _relerr(got, ref) < COARSE and not GB.compare("trunc", got, ref, bound, axes="nvc")["ok"]
    h, x, s, off = affine_case("bf16", off_scale=0.01)
    ref, bound = GB.channel_affine_reference(h, s, off, x, "bf16")
    v = ref.clone()
    v[..., 8:16] -= off.double()[:, None, 8:16]
    got = CB.round_to(v, "bf16")
    assert _relerr(got, ref) < COARSE and not GB.compare("off dropped", got, ref, bound, axes="nvc")["ok"]


# ---- dot_stats -----------------------------------------------------------------------------------------------------------------------------
def dot_rows_sim(a, b, kind, tiles, drop_last_of_thread=None, rotate=False):
    """dot_stats_kernel's rows in fp64: item i = voxel x G + channel group belongs to thread i mod (tiles 256), block = thread / 256; the terms
    are rounded to fp32 (exact at 16 bit), each row is summed exactly and rounded to fp32 once.  Faults: the last item of one thread's walk
    dropped; a block whose first item is not a multiple of G credits its sums to the channel groups rotated by one."""
    B, V, C = a.shape
    k = GB.kpl(kind)
    G = C // k
    t = _f32(a * b).reshape(B, V * G, k)
    i = torch.arange(V * G)
    thread = i % (tiles * 256)
    if drop_last_of_thread is not None:
        last = int(i[thread == drop_last_of_thread].max())
        t[:, last] = 0.0
    slot = (thread // 256) * G + i % G
    rows = torch.zeros(B, tiles * G, k, dtype=torch.float64).index_add_(1, slot, t).reshape(B, tiles, G, k)
    if rotate:
        for bx in range(tiles):
            if (bx * 256) % G:
                rows[:, bx] = rows[:, bx].roll(1, 1)
    return _f32(rows.reshape(B, tiles, C))


DOT_CASES = [(r, m) for r in GB.DOT_ROWS for m in r[1]]


@pytest.mark.parametrize("row,mode", DOT_CASES, ids=[f"{r[0]}-{m}" for r, m in DOT_CASES])
def test_dot_stats_correct_rows_pass_and_faults_fail(row, mode):
    name, _, vox, C, _ = row
    ak, bk = GB.MODES[mode]
    gen = torch.Generator().manual_seed(vox + C)
    a, b = CB.round_to(GB.onesign((2, vox, C), gen), ak), CB.round_to(GB.onesign((2, vox, C), gen), bk)
    tiles = GB.na_tiles(vox, C, ak)
    ref, bound = GB.dot_stats_reference(a, b, GB.dot_stats_chain(vox, C, ak, tiles))
    r = GB.compare("correct", dot_rows_sim(a, b, ak, tiles).sum(1), ref, bound, axes="nc")
    assert r["ok"], r
    # a single 16-bit product per row is exact in fp32: no rounding anywhere, err = 0 there and only there
    assert r["err"] > 0.0 or (ak != "f32" and vox == 1), r
    assert not GB.compare("last voxel of a walk dropped", dot_rows_sim(a, b, ak, tiles, drop_last_of_thread=0).sum(1), ref, bound, axes="nc")["ok"]
    G = C // GB.kpl(ak)
    if any((bx * 256) % G for bx in range(tiles)) and vox * G > 256:
        assert not GB.compare("rotated channel groups", dot_rows_sim(a, b, ak, tiles, rotate=True).sum(1), ref, bound, axes="nc")["ok"]
    bad = dot_rows_sim(a, b, ak, tiles)
    bad[1, tiles - 1, C - 1] = NAN
    assert not GB.compare("unwritten row", bad.sum(1), ref, bound, axes="nc")["ok"]


def test_dot_stats_rotation_fault_is_exercised():
    """The rotated-group fault needs a block whose first item is no multiple of G: true for the odd-factor rows (G 6, 10, 12)."""
    hit = [r[0] for r in GB.DOT_ROWS for m in r[1][:1] if any((bx * 256) % (r[3] // GB.kpl(GB.MODES[m][0])) for bx in range(GB.na_tiles(r[2], r[3], GB.MODES[m][0])))]
    assert {"odd_c48_v150", "odd_c80_v257", "cap_odd_c48", "v720_c48_G12"} <= set(hit), hit


# ---- gate multiply ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", GB.ALL)
def test_gate_mul_fwd_reference_and_faults(kind):
    gen = torch.Generator().manual_seed(2)
    V, C = 4099, 48
    a, x, _ = GB.gate_inputs(V, C, gen)
    a, x = CB.round_to(a, kind), CB.round_to(x, kind)
    ref = GB.gate_product(a, x, kind)
    assert not _fails(GB.gate_fwd_rows("correct", ref.clone(), ref, kind))
    if kind != "f32":      # the product of two stored 16-bit values is exact in fp32
        assert torch.equal((a[:, None] * x).float().double(), a[:, None] * x)
    assert _fails(GB.gate_fwd_rows("neighbouring voxel's gate", GB.gate_product(a.roll(1), x, kind), ref, kind))
    if kind != "f32":
        assert _fails(GB.gate_fwd_rows("truncating store", NB.trunc_to(a[:, None] * x, kind).to(ref.dtype), ref, kind))
    bad = ref.clone()
    bad[4098, 47] = NAN
    assert _fails(GB.gate_fwd_rows("unwritten", bad, ref, kind))
    if kind == "f16":      # the floor is half a subnormal spacing: subnormals flushed to zero are rejected, and so is a normal value one ulp off
        sub = ~GB.f16_normal(ref)
        assert bool(sub.any())
        assert _fails(GB.gate_fwd_rows("flushed subnormals", torch.where(sub, torch.zeros_like(ref), ref), ref, kind))
        off = ref.clone()
        off.view(torch.int16)[0, 0] += 1
        assert _fails(GB.gate_fwd_rows("one ulp", off, ref, kind))


GATE_F16 = [r for r in GB.GATE_ROWS if "f16" in r[1]]


@pytest.mark.parametrize("row", GATE_F16, ids=[r[0] for r in GATE_F16])
def test_gate_mul_f16_subnormal_share_of_the_reference_alone(row):
    """A condition, not a measurement: at most 1 % of the reference's elements are fp16 subnormals (compared within the floor instead of bit
    for bit), on the very data of every f16 row of the GPU file."""
    name, _, _, V, C, _, _ = row
    gen = torch.Generator().manual_seed(V + C)
    a, x, _ = GB.gate_inputs(V, C, gen)
    ref = GB.gate_product(CB.round_to(a, "f16"), CB.round_to(x, "f16"), "f16")
    assert (~GB.f16_normal(ref)).double().mean().item() <= 0.01


@pytest.mark.parametrize("mode", GB.BWD_MODES)
def test_gate_mul_bwd_reference_and_faults(mode):
    gk, tk = GB.MODES[mode]
    gen = torch.Generator().manual_seed(3)
    V, C = 1000, 48
    a, x, dy = GB.gate_inputs(V, C, gen)
    a, x, dy = CB.round_to(a, tk), CB.round_to(x, tk), CB.round_to(dy, gk)
    ref, bound = GB.gate_da_reference(dy, x, mode)
    r = GB.compare("correct", CB.round_to(ref, gk), ref, bound, axes="v")
    assert r["ok"] and r["err"] > 0.0, r
    k = GB.kpl(gk)
    short = CB.round_to((dy * x)[:, :C - k].sum(-1), gk)
    assert not GB.compare("da misses the last channel group", short, ref, bound, axes="v")["ok"]
    if gk != "f32":
        assert not GB.compare("truncating store", NB.trunc_to(ref, gk), ref, bound, axes="v")["ok"]
    bad = CB.round_to(ref, gk)
    bad[999] = NAN
    assert not GB.compare("unwritten", bad, ref, bound, axes="v")["ok"]
    dx = GB.gate_product(a, dy, gk)
    assert _fails(GB.gate_fwd_rows("dx with the neighbouring voxel's gate", GB.gate_product(a.roll(-1), dy, gk), dx, gk))
    # a non-zero value in da16 channel 5: passes the coarse bar over the 16-channel tensor, fails the exact zero
    da16 = torch.zeros(V, 16, dtype=CB.TORCH_DT[gk])
    da16[:, 0] = ref.to(CB.TORCH_DT[gk])
    want = da16.clone()
    da16[17, 5] = 1e-3
    assert _relerr(da16, want) < COARSE
    assert not GB.exact_row("da16 channels 1..15", da16[:, 1:], torch.zeros_like(da16[:, 1:]))["ok"]


# ---- 1-channel up-sampling -----------------------------------------------------------------------------------------------------------------
def ups_case(factor, bias=0.37):
    gen = torch.Generator().manual_seed(4)
    img = torch.randn(2, 3, 5, 7, generator=gen).float()
    w = torch.randn(factor[0] * factor[1] * factor[2], generator=gen).float()
    return img, w, torch.tensor([bias])


@pytest.mark.parametrize("factor", GB.UPS_FACTORS, ids=lambda f: "x".join(map(str, f)))
@pytest.mark.parametrize("kind", GB.ALL)
def test_upsample_fwd_correct_passes_and_faults_fail(kind, factor):
    img, w, bias = ups_case(factor)
    ref, bound = GB.upsample_fwd_reference(img, w, bias, factor, kind)
    # the reference against PyTorch's own transposed convolution
    fz, fy, fx = factor
    tc = torch.nn.functional.conv_transpose3d(img.double()[:, None], w.double().reshape(1, 1, fz, fy, fx), bias.double(), stride=factor)[:, 0]
    assert torch.allclose(ref, tc, rtol=1e-12, atol=1e-12)
    r = GB.compare("correct", CB.round_to(ref, kind), ref, bound, axes="nzyx")
    assert r["ok"] and r["err"] > 0.0, r
    if factor == (2, 3, 2):
        wrong = CB.round_to(GB.upsample_fwd_reference(img, w, bias, factor, kind, transposed=True)[0], kind)
        assert not GB.compare("tap index (a fx + c) fy + b", wrong, ref, bound, axes="nzyx")["ok"]
    assert not GB.compare("bias added twice", CB.round_to(ref + 0.37, kind), ref, bound, axes="nzyx")["ok"]
    if kind != "f32":
        assert not GB.compare("truncating store", NB.trunc_to(ref, kind), ref, bound, axes="nzyx")["ok"]
    bad = CB.round_to(ref, kind)
    bad[-1, -1, -1, -1] = NAN
    assert not GB.compare("unwritten", bad, ref, bound, axes="nzyx")["ok"]


def test_upsample_bias_added_twice_passes_the_coarse_bar():
    """Found to pass: a bias of 0.004 added twice, relerr <= 4e-3 over the whole tensor; rejected element-wise at every storage type."""
    for kind in GB.ALL:
        img, w, bias = ups_case((2, 3, 2), bias=0.004)
        ref, bound = GB.upsample_fwd_reference(img, w, bias, (2, 3, 2), kind)
        got = CB.round_to(ref + 0.004, kind)
        assert _relerr(got, ref) < COARSE and not GB.compare("bias twice", got, ref, bound, axes="nzyx")["ok"], kind


def ups_bwd_rows_sim(img, g, factor, blocks, skip_wave=None):
    """upsample_c1_bwd_kernel's rows: input voxel v belongs to thread v mod (blocks 256); the terms rounded to fp32, each wave total summed
    exactly, the four wave totals added and rounded once.  Fault: one wave's total left out."""
    fz, fy, fx = factor
    N, D, H, W = img.shape
    taps = fz * fy * fx
    gt = g.reshape(N, D, fz, H, fy, W, fx).permute(2, 4, 6, 0, 1, 3, 5).reshape(taps, -1)
    t = torch.stack([_f32(img.double().reshape(1, -1) * gt), gt], -1)
    v = torch.arange(gt.shape[1])
    thread = v % (blocks * 256)
    slot = (thread // 256) * 4 + (thread % 256) // 64
    waves = torch.zeros(taps, blocks * 4, 2, dtype=torch.float64).index_add_(1, slot, t).reshape(taps, blocks, 4, 2)
    if skip_wave is not None:
        waves[:, skip_wave[0], skip_wave[1]] = 0.0
    return _f32(waves.sum(2))


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_upsample_bwd_correct_rows_pass_and_faults_fail(kind):
    gen = torch.Generator().manual_seed(5)
    N, S, f = 2, (6, 20, 31), (2, 3, 2)
    img = (2.0 + 0.1 * torch.randn(N, *S, generator=gen)).float()
    g = CB.round_to(3.0 + 0.1 * torch.randn(N, S[0] * f[0], S[1] * f[1], S[2] * f[2], generator=gen), kind)
    blocks = GB.ups_blocks(N * S[0] * S[1] * S[2])
    assert blocks == 4
    ref, bound = GB.upsample_bwd_reference(img, g, f, blocks)
    r = GB.compare("correct", ups_bwd_rows_sim(img, g, f, blocks).sum(1), ref, bound, axes="tk")
    assert r["ok"] and r["err"] > 0.0, r
    assert not GB.compare("a wave's total left out", ups_bwd_rows_sim(img, g, f, blocks, skip_wave=(3, 2)).sum(1), ref, bound, axes="tk")["ok"]
    # the sums of tap t credited to tap (a fx + c) fy + b: g varies by tap, so the rows differ
    perm = torch.arange(12).reshape(f[0], f[2], f[1]).permute(0, 2, 1).reshape(-1)
    g2 = CB.round_to(g * (1 + 0.01 * torch.arange(g.shape[-1]) % 3), kind)
    ref2, bound2 = GB.upsample_bwd_reference(img, g2, f, blocks)
    sim2 = ups_bwd_rows_sim(img, g2, f, blocks).sum(1)
    assert GB.compare("correct", sim2, ref2, bound2, axes="tk")["ok"]
    assert not GB.compare("transposed tap", sim2[perm], ref2, bound2, axes="tk")["ok"]
    bad = ups_bwd_rows_sim(img, g, f, blocks)
    bad[11, 3, 1] = NAN
    assert not GB.compare("unwritten row", bad.sum(1), ref, bound, axes="tk")["ok"]


# ---- the gate MLP --------------------------------------------------------------------------------------------------------------------------
def mlp_case(tiles, C, R, act, N=3, bias=True, data="bigmean"):
    gen = torch.Generator().manual_seed(tiles + C + R + act)
    col = GB.bigmean_rows(N, tiles, C, gen) if data == "bigmean" else torch.randn(N, tiles, C, generator=gen)
    part = torch.stack([col, torch.randn(N, tiles, C, generator=gen)], 2).float()
    w1, w2 = (torch.randn(R, C, generator=gen) * 0.3).float(), (torch.randn(C, R, generator=gen) * 0.3).float()
    b1, b2 = ((torch.randn(R, generator=gen) * 0.1).float(), (torch.randn(C, generator=gen) * 0.1).float()) if bias else (None, None)
    return part, w1, b1, w2, b2


def mlp_fwd_sim(part, vox, w1, b1, w2, b2, act, keep_rows=None):
    """The forward in fp64 with each saved value rounded to fp32 once.  keep_rows: only the first rows enter the column total - the rows past
    the last full 16-deep pass dropped (a fault)."""
    p = part if keep_rows is None else part[:, :keep_rows]
    f = GB.gate_mlp_fwd_reference(p, vox, w1, b1, w2, b2, act)
    return {k: _f32(v[0]) for k, v in f.items()}


@pytest.mark.parametrize("act", range(9))
def test_gate_mlp_fwd_correct_passes_and_dropped_rows_fail(act):
    tiles, C, R = 1000, 64, 6                    # lanes = 4: a 16-deep pass takes 64 rows; 15 full passes = 960 rows, a tail of 40
    part, w1, b1, w2, b2 = mlp_case(tiles, C, R, act)
    f = GB.gate_mlp_fwd_reference(part, tiles, w1, b1, w2, b2, act)
    good = mlp_fwd_sim(part, tiles, w1, b1, w2, b2, act)
    full = tiles // (16 * (256 // C)) * (16 * (256 // C))
    assert full == 960
    lost = mlp_fwd_sim(part, tiles, w1, b1, w2, b2, act, keep_rows=full)
    for k in ("s", "m", "u1", "a1"):
        r = GB.compare(k, good[k], *f[k], axes="nc")
        assert r["ok"], r
        assert r["err"] > 0.0 or (k == "a1" and act in (0, 2, 4)), r          # identity / relu / leaky relu of an fp32 value is that value or exact
    assert not GB.compare("m with the tail rows dropped", lost["m"], *f["m"], axes="nc")["ok"]
    assert not GB.compare("s with the tail rows dropped", lost["s"], *f["s"], axes="nc")["ok"]
    for k in ("s", "m", "u1", "a1"):
        bad = good[k].clone()
        bad[2, -1] = NAN
        assert not GB.compare(k + " unwritten", bad, *f[k], axes="nc")["ok"]


def test_dropped_tail_rows_at_the_shape_of_the_existing_autograd_test():
    """test_gate_mlp_kernels_match_autograd runs 37 tiles of randn rows at C 16 .. 64 (lanes 16 .. 4): the 16-deep loop needs tiles > 15 lanes
    >= 60, so it is never entered there and a fault in it cannot show.  Had the loop been entered once (C 64, 64 rows in the pass) and the
    rows past it dropped, that test's own bars would have been asked to see 1 row of 65 missing from m: found NOT to pass its atol of 1e-7
    on m (the rows are O(1) and voxels = 5000), so the gap of that test is reach, not tolerance - and it does pass the coarse 4e-3 bar on s."""
    for C in (16, 32, 48, 64):
        assert 37 < GB.mlp_loop_entries(C)[1]
    part, w1, b1, w2, b2 = mlp_case(65, 64, 4, 3, data="randn")
    ref = GB.gate_mlp_fwd_reference(part, 5000, w1, b1, w2, b2, 3)
    lost = mlp_fwd_sim(part, 5000, w1, b1, w2, b2, 3, keep_rows=64)
    assert not torch.allclose(lost["m"], ref["m"][0], atol=1e-7, rtol=0)
    assert _relerr(lost["s"], ref["s"][0]) < COARSE
    assert not GB.compare("dropped", lost["m"], *ref["m"], axes="nc")["ok"]


@pytest.mark.parametrize("act", [0, 2, 3, 5])
@pytest.mark.parametrize("bias", [True, False])
def test_gate_mlp_bwd_correct_passes_and_faults_fail(act, bias):
    N, tiles, C, R = 5, 70, 48, 6
    gen = torch.Generator().manual_seed(act)
    dpart = GB.bigmean_rows(N, tiles, C, gen).float()
    s = (0.05 + 0.9 * torch.rand(N, C, generator=gen)).float()
    saved = torch.randn(N, C + 2 * R, generator=gen).float()
    w1, w2 = (torch.randn(R, C, generator=gen) * 0.3).float(), (torch.randn(C, R, generator=gen) * 0.3).float()
    init = dict(dw1=torch.randn(R, C, generator=gen).float(), dw2=torch.randn(C, R, generator=gen).float(),
                db1=torch.randn(R, generator=gen).float() if bias else None, db2=torch.randn(C, generator=gen).float() if bias else None)
    b = GB.gate_mlp_bwd_reference(dpart, 4096, s, saved, w1, w2, act, init)
    flipped = GB.gate_mlp_bwd_reference(dpart, 4096, s, saved, w1, w2, act, init, flip_s=True)
    zero = {k: (None if v is None else torch.zeros_like(v)) for k, v in init.items()}
    fresh = GB.gate_mlp_bwd_reference(dpart, 4096, s, saved, w1, w2, act, zero)
    assert set(b) == {"off", "dw1", "dw2"} | ({"db1", "db2"} if bias else set())
    for k, (ref, bound) in b.items():
        r = GB.compare(k, _f32(ref), ref, bound, axes="ab"[:ref.dim()])
        assert r["ok"] and r["err"] > 0.0, r
        assert not GB.compare(k + " with s for 1 - s", _f32(flipped[k][0]), ref, bound, axes="ab"[:ref.dim()])["ok"], k
        if k != "off":
            assert not GB.compare(k + " overwritten", _f32(fresh[k][0]), ref, bound, axes="ab"[:ref.dim()])["ok"], k
        assert not GB.compare(k + " neighbour sample's s", _f32(GB.gate_mlp_bwd_reference(dpart, 4096, s.roll(1, 0), saved, w1, w2, act, init)[k][0]), ref, bound,
                              axes="ab"[:ref.dim()])["ok"], k
        bad = _f32(ref)
        bad.view(-1)[-1] = NAN
        assert not GB.compare(k + " unwritten", bad, ref, bound, axes="ab"[:ref.dim()])["ok"], k


def test_column_total_orders_agree_on_exact_rows_and_differ_in_general():
    """On rows whose partial sums are exact in fp64 the kernel's stated order, the tail-loop order and the plain sum agree bit for bit (what the
    GPU bit-identity rows require); the host function does follow another order: on randn rows scaled apart it differs from the plain sum."""
    gen = torch.Generator().manual_seed(6)
    for tiles, C in GB.MLP_BITS_ROWS:
        col = GB.exact_rows(1, tiles, C, gen)[0].double()
        a, b = GB.column_total_kernel_order(col, C), GB.column_total_kernel_order(col, C, tail_only=True)
        assert torch.equal(a, b) and torch.equal(a, col.sum(0))
    col = (torch.randn(1024, 64, generator=gen) * torch.exp(8 * torch.randn(1024, 64, generator=gen))).float().double()
    assert not torch.equal(GB.column_total_kernel_order(col, 64), GB.column_total_kernel_order(col, 64, tail_only=True))


# ---- host side: the contract, and the GPU rows reach what they name ----------------------------------------------------------------------------
def _lib():
    from biapy_amd import _lib as L

    return L


def _dtc(L, kind):
    return {"f32": L.F32, "bf16": L.BF16, "f16": L.F16, "mix16": L.MIX16}[kind]


def _refused(rc, L, *words):
    assert rc != 0
    msg = L.lib.bpx_last_error().decode()
    assert all(w in msg for w in words), msg


def test_host_contract_refusals():
    """BPX_CHECK / BPX_FAIL return before any device call (the pointers below are never dereferenced)."""
    L = _lib()
    lib = L.lib
    P = 4096
    t = lambda C, cs=0: L.Tensor(P, C, C, cs)
    for dt in (L.BF16, L.F32, L.F16):
        _refused(lib.bpx_channel_affine(dt, 2, 720, L.NULL_T, t(24), P, None, t(24), None), L, "bpx_channel_affine", "multiple of 16")
    _refused(lib.bpx_dot_stats(L.BF16, 2, 720, t(24), t(24), P, None), L, "bpx_dot_stats", "multiple of 16")
    _refused(lib.bpx_channel_affine(L.MIX16, 2, 720, L.NULL_T, t(16), P, None, t(16), None), L, "bpx_channel_affine", "dtype")
    _refused(lib.bpx_dot_stats(L.F16, 2, 720, t(16), t(16), P, None), L, "bpx_dot_stats", "dtype")
    _refused(lib.bpx_upsample_c1_bwd(L.F16, 1, 2, 2, 2, 1, 1, 1, P, P, P, None), L, "bpx_upsample_c1_bwd", "dtype")
    for C, R in ((16, 17), (128, 65), (257, 4)):
        _refused(lib.bpx_gate_mlp_fwd(P, 2, 4, C, 1024, P, None, P, None, R, 2, P, P, None), L, "bpx_gate_mlp_fwd", f"C={C} R={R}")
        _refused(lib.bpx_gate_mlp_bwd(P, 2, 4, C, 1024, P, P, P, P, R, 2, P, None, P, None, P, None), L, "bpx_gate_mlp_bwd", f"C={C} R={R}")
    _refused(lib.bpx_upsample_c1_fwd(L.BF16, 1, 2, 2, 2, 8, 8, 9, P, P, P, P, None), L, "bpx_upsample_c1_fwd", "bad factors")
    _refused(lib.bpx_upsample_c1_bwd(L.BF16, 1, 2, 2, 2, 8, 8, 9, P, P, P, None), L, "bpx_upsample_c1_bwd", "bad factors")
    pl = t(16, cs=1 << 20)
    _refused(lib.bpx_channel_affine(L.BF16, 1, 64, L.NULL_T, pl, P, None, t(16), None), L, "bpx_channel_affine", "chunk-planar")
    _refused(lib.bpx_dot_stats(L.BF16, 1, 64, t(16), pl, P, None), L, "bpx_dot_stats", "chunk-planar")
    _refused(lib.bpx_gate_mul_fwd(L.BF16, 64, t(16), pl, t(16), None), L, "bpx_gate_mul_fwd", "chunk-planar")
    _refused(lib.bpx_gate_mul_bwd(L.BF16, 64, t(16), t(16), t(16), pl, P, None), L, "bpx_gate_mul_bwd", "chunk-planar")


def test_tile_function_equals_the_library_at_every_dot_stats_and_affine_row():
    L = _lib()
    for name, kinds, vox, C, *_ in GB.DOT_ROWS + GB.AFFINE_ROWS:
        for m in kinds:
            k = GB.MODES[m][0] if m in GB.MODES else m
            assert L.lib.bpx_norm_act_tiles(_dtc(L, k), vox, C) == GB.na_tiles(vox, C, k), (name, m)
    for v in (1, 2047, 2048, 2049, 522240, 522241, 10 ** 7):
        assert L.lib.bpx_upsample_c1_blocks(v) == GB.ups_blocks(v)


def test_gpu_rows_reach_the_branches_they_name():
    rows = {r[0]: r for r in GB.AFFINE_ROWS}
    for name, kinds, vox, C, *_ in GB.AFFINE_ROWS:
        for k in kinds:
            G = C // GB.kpl(k)
            threads = 4 * GB.na_tiles(vox, C, k) * 256
            assert threads % G == 0
            assert (vox * G > threads) == name.startswith("cap"), name                  # a thread walks more than once exactly in the cap rows
            if name.startswith("cap"):
                assert vox * G > 4 * GB.NA_BLOCKS * 256 and GB.na_tiles(vox, C, k) == GB.NA_BLOCKS
    assert rows["v1_c16_below_one_block"][2] * 4 < 256 and rows["v5_c2048_G512_xnull"][3] // 4 == 512
    assert 48 // GB.kpl("bf16") == 6 and 48 // GB.kpl("f32") == 12                          # the G = 6 mapping and an odd factor at f32
    assert {(r[5], r[6]) for r in GB.AFFINE_ROWS} == {(True, True), (False, True), (True, False), (False, False)}
    assert any(r[7] for r in GB.AFFINE_ROWS) and any(r[4] for r in GB.AFFINE_ROWS)
    for name, modes, vox, C, _ in GB.DOT_ROWS:
        for m in modes:
            k = GB.MODES[m][0]
            G, tiles = C // GB.kpl(k), GB.na_tiles(vox, C, k)
            raw = min(GB.cdiv(vox * G, 256), GB.NA_BLOCKS)
            assert (tiles * 256) % G == 0
            if name.startswith("cap"):
                assert vox * G > GB.NA_BLOCKS * 256 and GB.cdiv(vox * G, tiles * 256) >= 2, name
            if name.startswith("odd") or name == "cap_odd_c48":
                assert tiles > raw, name                                                     # rounded up to a multiple of G's odd part
            if name.startswith("odd"):
                assert (tiles - 1) * 256 >= vox * G, name                                    # the last block holds no item: it must write zeros
            if "G512" in name:
                assert G > 256
    for name, fk, bm, V, C, ld, _ in GB.GATE_ROWS:
        assert (name == "fwd_cap_c64") == any(V * (C // GB.kpl(k)) > GB.GRID_CAP * 256 for k in fk), name
        assert (name == "bwd_cap_c16") == (bool(bm) and V > GB.GRID_CAP * 256), name
    assert {r[5] for r in GB.GATE_ROWS} == {1, 16} and {r[4] for r in GB.GATE_ROWS} >= {16, 48, 128}
    for name, fk, bk, N, S, f in GB.UPS_ROWS:
        vin = N * S[0] * S[1] * S[2]
        assert f[0] * f[1] * f[2] <= 512
        assert (name == "fwd_cap") == (bool(fk) and vin * f[0] * f[1] * f[2] > GB.GRID_CAP * 256), name
        assert (name == "bwd_cap") == (bool(bk) and GB.ups_blocks(vin) == GB.UPS_BWD_CAP and GB.cdiv(vin, GB.UPS_BWD_CAP * 256) > 8), name
    assert {r[5] for r in GB.UPS_ROWS} >= set(GB.UPS_FACTORS)
    # gate MLP: both sides of both loop entries for every C, fewer rows than lanes, the production shape, every activation code, N 1 / 3 / 17
    for C in (16, 48, 64, 80, 160, 256):
        e4, e16 = GB.mlp_loop_entries(C)
        have = {r[0] for r in GB.MLP_ROWS if r[1] == C}
        assert {1, 3, e4 - 1, e4, e16 - 1, e16, 1024} <= have, (C, sorted(have))
    assert GB.mlp_loop_entries(64) == (13, 61) and GB.mlp_loop_entries(16) == (49, 241)
    assert {60, 61, 64, 65} <= {r[0] for r in GB.MLP_ROWS if r[1] == 64} and {240, 241, 257} <= {r[0] for r in GB.MLP_ROWS if r[1] == 16}
    assert {r[3] for r in GB.MLP_ROWS} == set(range(9)) and {r[5] for r in GB.MLP_ROWS} == {1, 3, 17}
    assert {r[2] for r in GB.MLP_ROWS} >= {1, 6, 64} and any(r[1] == r[2] == 16 for r in GB.MLP_ROWS)
    assert {r[4] for r in GB.MLP_ROWS} == {True, False}
    assert all(r[2] <= r[1] and r[2] <= 64 and r[1] <= 256 for r in GB.MLP_ROWS)
    for tiles, C in GB.MLP_BITS_ROWS:
        assert tiles >= GB.mlp_loop_entries(C)[1]                                            # every bit-identity row enters the 16-deep loop

"""Element-wise error bounds for the gate and channel-affine kernels of biapy_amd/csrc/elementwise.hip and the 1-channel up-sampling kernels of ends.hip - the hot path
of the RCAN trunk, of ResUNet++'s squeeze-excite and attention blocks and of ResUNet's super-resolution "pre" path - in the form of
tests/conv_bounds.py and tests/norm_bounds.py, whose comparator, rounding helpers, activation terms and partial-sum bound are reused:

    |got - ref| <= u_out |ref| + (1 + u_out) (E + K 2^-24 M) + floor          (conv_bounds.finish)

``ref`` is the operation in float64 on the operands as stored, ``M`` the sum of the absolute terms, ``K`` the number of fp32 roundings a term
passes through, ``E`` the error of operands formed on the device pushed through on absolute values.  Every chain length is read off the kernel
and stated where the bound is built.  The gate multiply is one exact product and one round-to-nearest-even store: it is compared bit for bit.

Nothing here is fitted to a measured value.  NaN / inf fails (conv_bounds.compare), outputs are pre-filled with NaN by the callers, and no
element is left out of a comparison.
"""
from __future__ import annotations

import torch

import conv_bounds as CB
from conv_bounds import ACT_ABS, ACT_LIP, ACT_REL, ACT_U, F16_FLOOR, U32, act64, compare, dact64, finish, round_to  # noqa: F401
from norm_bounds import MODES, U64, exact_row, same_bits, sums_reference, trunc_to  # noqa: F401

ALL = ("f32", "bf16", "f16")
BWD_MODES = ("f32", "bf16", "mix16")
NA_BLOCKS = 512             # elementwise.hip: blocks (= partial-sum slots) per sample, upper bound
GRID_CAP = 256 * 16         # bpx_common.h grid_for: min(cdiv(total, 256), 256 * 16) blocks
UPS_BWD_CAP = 256           # bpx_upsample_c1_blocks: min(max(1, cdiv(voxels_in, 2048)), 256)


def cdiv(a, b):
    return -(-a // b)


def kpl(kind):
    """Elements of one 16-byte lane operand (ElemTraits<T>::KPL)."""
    return 4 if kind == "f32" else 8


def na_tiles(voxels, C, kind):
    """na_blocks of elementwise.hip (what bpx_norm_act_tiles answers): min(ceil(voxels G / 256), 512) rounded up to a multiple of G's odd
    part, so that 256 x blocks is a multiple of G and a thread keeps its channel group.  dot_stats writes this many rows per sample;
    channel_affine launches four times as many blocks."""
    G = C // kpl(kind)
    odd = G
    while odd % 2 == 0 and odd > 1:
        odd //= 2
    return cdiv(min(cdiv(voxels * G, 256), NA_BLOCKS), odd) * odd


def grid_for(total):
    return min(cdiv(total, 256), GRID_CAP)


def ups_blocks(total_in):
    return min(max(1, cdiv(total_in, 2048)), UPS_BWD_CAP)


def _bc(v):
    """(B, C) per-sample channel vector -> (B, 1, C) float64."""
    return v.double()[:, None, :]


# ---- channel_affine ------------------------------------------------------------------------------------------------------------------
def channel_affine_reference(h, s, off, x, kind):
    """channel_affine_kernel: y = [x +] s[n, c] h [+ off[n, c]] on the stored h, x (B, V, C) and the fp32 s, off (B, C).  The line
    `o = ks * hf + ko` is a product and an addition (2 roundings, 1 if it contracts to an fma), `o += xf` one more: K = 3 covers both
    forms; a null x or off only removes a rounding."""
    t = _bc(s).to(h.device) * h
    ref, M = t, t.abs()
    if off is not None:
        o = _bc(off).to(h.device)
        ref, M = ref + o, M + o.abs()
    if x is not None:
        ref, M = ref + x, M + x.abs()
    return ref, finish(ref, M, 0.0, 3, kind)


# ---- dot_stats ---------------------------------------------------------------------------------------------------------------------------
def dot_stats_chain(voxels, C, kind, tiles):
    """Longest fp32 chain of one dot_stats_kernel row.  `s[e] += af[e] * bf[e]` over the thread's walk: the grid holds tiles x 256 threads for
    voxels x G items, ceil(voxels G / (tiles 256)) additions; `acc += dred[t * KPL + e]` for t = lane0, lane0 + G, ..: the ceil(256 / G)
    threads of the channel group in sequence.  One more at f32 for the product (16-bit products are exact in fp32: bf16 x bf16 has 16
    significand bits, bf16 x f16 has 19).  kind: the storage type of `a` (it selects KPL)."""
    G = C // kpl(kind)
    return cdiv(voxels * G, tiles * 256) + cdiv(256, G) + (1 if kind == "f32" else 0)


def dot_stats_reference(a, b, chain):
    """sum_v a b per (sample, channel) of stored a, b (B, V, C): exact terms, only the chain remains (norm_bounds.sums_reference)."""
    t = a * b
    s, bound = sums_reference(t, 0.0, t, 0.0, chain)
    return s[:, 0], bound[:, 0]


# ---- gate multiply: exact ---------------------------------------------------------------------------------------------------------------
def gate_product(a, x, kind):
    """round(a[v] x[v][c]) in the storage type `kind`, bit for bit what gate_mul_fwd_kernel (`f[e] *= av`, pack16) and the dx of
    gate_mul_bwd_kernel (`g[e] *= av`) store: the product of two stored values is exact in fp32 for every 16-bit pairing (at most 11 + 11
    significand bits) and is ONE fp32 rounding at f32; the store rounds to nearest even.  a (V,), x (V, C) float64 of stored values: the
    float64 product is exact (at most 48 bits) and fits fp32 exactly at 16 bit, so the conversion below rounds once."""
    return (a[:, None] * x).to(CB.TORCH_DT[kind])


def f16_normal(ref16):
    """Where an fp16 reference is compared bit for bit: |ref| >= 2^-14 or ref == 0.  Elsewhere (fp16 subnormals) the result is compared within
    F16_FLOOR, half the subnormal spacing as in conv_bounds: a subnormal flushed to zero is outside it."""
    r = ref16.double().abs()
    return (r >= 2.0 ** -14) | (r == 0)


def gate_fwd_rows(tag, got, ref16, kind):
    """Result rows of a gate_mul_fwd / dx comparison: bit for bit (exact_row); at f16 bit for bit on f16_normal and within F16_FLOOR
    everywhere (an exact match satisfies it)."""
    ref16 = ref16.to(got.device)
    if kind != "f16":
        return [exact_row(tag, got, ref16)]
    nrm = f16_normal(ref16)
    floor = torch.full(ref16.shape, F16_FLOOR, dtype=torch.float64, device=got.device)
    return [exact_row(tag + ".normal_bits", torch.where(nrm, got, ref16), ref16), compare(tag + ".subnormal_floor", got, ref16.double(), floor, axes="vc")]


def gate_inputs(V, C, gen):
    """The gate a in [0.05, 1] (a sigmoid output) and x, dy randn, float32 before rounding to a storage type."""
    a = 0.05 + 0.95 * torch.rand(V, generator=gen)
    return a, torch.randn(V, C, generator=gen), torch.randn(V, C, generator=gen)


def gate_da_reference(dy, x, mode):
    """da[v] = sum_c dy[v][c] x[v][c] of gate_mul_bwd_kernel: `dot += g[e] * xv[e]` over the C channels in sequence - C fp32 additions, one
    more at f32 for the product (exact at 16 bit) - and one store rounded to the gradient type."""
    gk = MODES[mode][0]
    t = dy * x
    C = x.shape[-1]
    ref = t.sum(-1)
    return ref, finish(ref, t.abs().sum(-1), 0.0, C + (1 if gk == "f32" else 0), gk)


# ---- 1-channel up-sampling ---------------------------------------------------------------------------------------------------------------
def tap_kernel(w, factor, transposed=False):
    """The (fz, fy, fx) tap weights as upsample_c1_fwd_kernel indexes them: w[(a * fy + b) * fx + c].  transposed: (a * fx + c) * fy + b - a
    fault, for the CPU self-test."""
    fz, fy, fx = factor
    if not transposed:
        return w.double().reshape(fz, fy, fx)
    return w.double().reshape(fz, fx, fy).permute(0, 2, 1)


def upsample_fwd_reference(img, w, bias, factor, kind, transposed=False):
    """out[n, fz z + a, fy y + b, fx x + c] = img[n, z, y, x] w[a][b][c] + bias of the fp32 img (N, D, H, W), w and bias: a product and an
    addition (`img[..] * w[..] + b[0]`: 2 roundings, 1 as an fma), then the store.  Returns (ref (N, Do, Ho, Wo), bound)."""
    fz, fy, fx = factor
    N, D, H, W = img.shape
    k = tap_kernel(w, factor, transposed).to(img.device)
    t = (img.double()[:, :, None, :, None, :, None] * k[None, None, :, None, :, None, :]).reshape(N, D * fz, H * fy, W * fx)
    b = float(bias.double().reshape(-1)[0])
    ref = t + b
    return ref, finish(ref, t.abs() + abs(b), 0.0, 2, kind)


def upsample_bwd_chain(total_in, blocks):
    """upsample_c1_bwd_kernel: `sw += img[v] * g; sg += g` over the thread's walk, ceil(total_in / (blocks 256)); the wave butterfly
    (__shfl_xor over 1 .. 32: 6 levels); `red[0] + red[1] + red[2] + red[3]`: 3 additions of the four wave totals; one for the product."""
    return cdiv(total_in, blocks * 256) + 6 + 3 + 1


def upsample_bwd_reference(img, g, factor, blocks):
    """Per tap t = (a fy + b) fx + c: (sum_v img[v] g[tap voxel of v], sum_v g[..]) over every input voxel, g (N, Do, Ho, Wo) the stored
    channel 0 of dx16.  The partial rows of a tap are summed in fp64 by the caller (resunet.py does: part.to(float64).sum(1)).
    Returns (ref (taps, 2), bound (taps, 2))."""
    fz, fy, fx = factor
    N, D, H, W = img.shape
    gt = g.reshape(N, D, fz, H, fy, W, fx).permute(2, 4, 6, 0, 1, 3, 5).reshape(fz * fy * fx, -1, 1)
    s, b = sums_reference(img.double().reshape(1, -1, 1) * gt, 0.0, gt, 0.0, upsample_bwd_chain(N * D * H * W, blocks))
    return s[..., 0], b[..., 0]


# ---- the gate MLP --------------------------------------------------------------------------------------------------------------------------
def column_total_kernel_order(col, C, tail_only=False):
    """The fp64 column total of gate_column_sum in the kernel's stated order, on the host: col (tiles, C) float64 rows.  lanes = 256 / C lanes
    per channel; lane l takes the rows l, l + lanes, ..: while sixteen rows remain they go to the accumulators a, a1, a2, a3 in turn (four
    rounds), then while four remain likewise, then the rest into a; (a + a1) + (a2 + a3); the lanes are added in order.  tail_only: every
    row through the last loop (one accumulator per lane) - what the kernel's comment claims gives the same bits."""
    tiles = col.shape[0]
    lanes = 256 // C
    tot = torch.zeros(C, dtype=torch.float64)
    for l in range(lanes):
        acc = [torch.zeros(C, dtype=torch.float64) for _ in range(4)]
        t = l
        if not tail_only:
            for deep in (16, 4):
                while t + (deep - 1) * lanes < tiles:
                    for k in range(deep):
                        acc[k % 4] = acc[k % 4] + col[t + k * lanes]
                    t += deep * lanes
        while t < tiles:
            acc[0] = acc[0] + col[t]
            t += lanes
        tot = tot + ((acc[0] + acc[1]) + (acc[2] + acc[3]))
    return tot


def mlp_loop_entries(C):
    """(first tile count that enters the 4-deep loop, first that enters the 16-deep loop) of gate_column_sum for lane 0: t + 3 lanes < tiles
    and t + 15 lanes < tiles at t = 0."""
    lanes = 256 // C
    return 3 * lanes + 1, 15 * lanes + 1


def _column_total(rows):
    """fp64 total over the tiles (N, tiles, C) and what the device's fp64 sum in another order may differ by."""
    p = rows.double()
    return p.sum(1), (p.shape[1] + 16) * U64 * p.abs().sum(1)


def gate_mlp_fwd_reference(part, voxels, w1, b1, w2, b2, act):
    """gate_mlp_fwd_kernel on GIVEN partial rows part (N, tiles, 2, C) fp32 (sum 0 is read), w1 (R, C), w2 (C, R), biases or None:
        m = tot / voxels; u1 = W1 m + b1; a1 = act(u1); s = sigmoid(W2 a1 + b2);  saved = {m, u1, a1}
    pushed through the four stages on absolute values:
    - `m[t] = tot * inv_vox`: tot an fp64 column total cast to float, inv_vox = (float)(1.0 / voxels), one fp32 product: E_m = 3 2^-24 |m|
      (plus the fp64 order term of the total);
    - `u = b1[t]; u += w1[t * C + c] * m[c]` for C channels: chain C + 1 over |W1||m| + |b1|, plus |W1| E_m;
    - `gate_act(u, act)`: ACT_LIP E_u1 + 2^-24 (ACT_REL |a1| + ACT_ABS + ACT_U |u1|) (conv_bounds: the activation terms);
    - `u = b2[t]; u += w2[t * R + r] * a1[r]`: chain R + 1 over |W2||a1| + |b2|, plus |W2| E_a1;
    - `1.f / (1.f + expf(-u))`: the sigmoid's slope is at most 0.25: 0.25 E_u2 + 2^-24 (ACT_REL s + ACT_ABS).
    Returns {name: (ref, bound)} for s, m, u1, a1."""
    C = part.shape[-1]
    R = w1.shape[0]
    tot, dtot = _column_total(part[:, :, 0, :])
    W1, W2 = w1.double().to(part.device), w2.double().to(part.device)
    z1 = torch.zeros(R, dtype=torch.float64, device=part.device) if b1 is None else b1.double().to(part.device)
    z2 = torch.zeros(C, dtype=torch.float64, device=part.device) if b2 is None else b2.double().to(part.device)
    m = tot / voxels
    em = 3 * U32 * m.abs() + dtot / voxels
    u1 = m @ W1.t() + z1
    eu1 = (C + 1) * U32 * (m.abs() @ W1.abs().t() + z1.abs()) + em @ W1.abs().t()
    a1 = act64(u1, act)
    ea1 = ACT_LIP * eu1 + U32 * (ACT_REL * a1.abs() + ACT_ABS + ACT_U * u1.abs())
    u2 = a1 @ W2.t() + z2
    eu2 = (R + 1) * U32 * (a1.abs() @ W2.abs().t() + z2.abs()) + ea1 @ W2.abs().t()
    s = torch.sigmoid(u2)
    es = 0.25 * eu2 + U32 * (ACT_REL * s + ACT_ABS)
    return dict(s=(s, es), m=(m, em), u1=(u1, eu1), a1=(a1, ea1))


def gate_mlp_bwd_reference(dpart, voxels, s, saved, w1, w2, act, init, flip_s=False):
    """gate_mlp_bwd_kernel on GIVEN operands - dpart (N, tiles, C), s (N, C), saved (N, C + 2 R) = {m, u1, a1}, w1 (R, C), w2 (C, R), all
    fp32 as stored, so the reference is an exact function of stored values (nothing is chained from a forward run) - and the initial
    contents init = {dw1, db1, dw2, db2} of the gradient buffers, which are ADDED to.  Per sample n, in the kernel's lines:
    - `ds = gate_column_sum(..)`: an fp64 total cast to float: 1 rounding;
    - `du2[t] = ds * sg * (1.f - sg)`: the difference and two products: 3 roundings - E_du2 = 4 2^-24 |du2| with the cast;
    - `a += du2[c] * w2[c * R + t]` over C channels: chain C over |du2||W2|, plus E_du2 |W2|;
    - `a *= gate_act_bwd(sv[C + t], act)`: the derivative of the STORED u1 formed in fp32, 2^-24 (ACT_REL |d| + ACT_ABS + ACT_U |u1|), and the
      product rounds once: E_du1;
    - `ab1 += a`, `ab2 += d2`: N additions over the samples, then `db[t] += ab`: chain N + 1 over the terms and the initial value;
    - `aw2[r] += d2 * sv[C + R + r]`, `aw1[r] += du1[r] * mc`: the same with one more rounding for the product: N + 2;
    - `dm += du1[r] * w1[r * C + t]` over R rows: chain R; `off = dm * inv_vox`: inv_vox = (float)(1.0 / voxels) and the product: R + 2.
    flip_s: `1 - s` replaced by `s` in du2 - a fault, for the CPU self-test.
    Returns {name: (ref, bound)} for off (N, C), dw1 (R, C), db1 (R,), dw2 (C, R), db2 (C,)."""
    dev = dpart.device
    N, _, C = dpart.shape
    R = w1.shape[0]
    W1, W2 = w1.double().to(dev), w2.double().to(dev)
    sv, sg = saved.double().to(dev), s.double().to(dev)
    m, u1, a1 = sv[:, :C], sv[:, C:C + R], sv[:, C + R:]
    ds, dds = _column_total(dpart)
    du2 = ds * sg * (sg if flip_s else (1 - sg))
    edu2 = 4 * U32 * du2.abs() + dds * (sg * (1 - sg)).abs()
    t1 = du2 @ W2
    et1 = edu2 @ W2.abs() + C * U32 * (du2.abs() @ W2.abs())
    d = dact64(u1, act)
    ed = U32 * (ACT_REL * d.abs() + ACT_ABS + ACT_U * u1.abs())
    du1 = t1 * d
    edu1 = et1 * d.abs() + (t1.abs() + et1) * ed + U32 * du1.abs()
    i = {k: (None if v is None else v.double().to(dev)) for k, v in init.items()}
    out = {}
    dm = du1 @ W1
    out["off"] = (dm / voxels, finish(dm / voxels, (du1.abs() @ W1.abs()) / voxels, (edu1 @ W1.abs()) / voxels, R + 2, "f32"))
    if i["db1"] is not None:
        out["db1"] = (i["db1"] + du1.sum(0), finish(i["db1"] + du1.sum(0), du1.abs().sum(0) + i["db1"].abs(), edu1.sum(0), N + 1, "f32"))
    if i["db2"] is not None:
        out["db2"] = (i["db2"] + du2.sum(0), finish(i["db2"] + du2.sum(0), du2.abs().sum(0) + i["db2"].abs(), edu2.sum(0), N + 1, "f32"))
    r2 = i["dw2"] + du2.t() @ a1
    out["dw2"] = (r2, finish(r2, du2.abs().t() @ a1.abs() + i["dw2"].abs(), edu2.t() @ a1.abs(), N + 2, "f32"))
    r1 = i["dw1"] + du1.t() @ m
    out["dw1"] = (r1, finish(r1, du1.abs().t() @ m.abs() + i["dw1"].abs(), edu1.t() @ m.abs(), N + 2, "f32"))
    return out


def bigmean(shape, gen, mean=3.0, spread=0.1):
    """Values of one sign per channel (mean = 30 x spread, the sign alternating over the channels): a lost term or row shows against
    chain 2^-24 sum|terms|."""
    C = shape[-1]
    return spread * torch.randn(*shape, generator=gen) + mean * (1 - 2 * (torch.arange(C) % 2)).float()


def bigmean_rows(N, tiles, C, gen):
    """Partial rows (N, tiles, C) of one sign per (sample, channel) column, the sign drawn per column: the samples' means differ, so a
    ReLU gate is not dead for every sample at once."""
    sign = (2 * torch.randint(0, 2, (N, 1, C), generator=gen) - 1).float()
    return bigmean((N, tiles, C), gen) * sign


def onesign(shape, gen):
    """Values of one sign per channel (alternating over the channels) whose magnitudes span four binades, 0.25 .. 4.25: a lost term shows
    against chain 2^-24 sum|terms|, and - unlike values near one magnitude, whose 16-bit products are multiples of one power of two and sum
    exactly in fp32 - the fp32 sums of their bf16 / f16 products do round."""
    C = shape[-1]
    return (0.25 + 4.0 * torch.rand(*shape, generator=gen)) * (1 - 2 * (torch.arange(C) % 2)).float()


# ---- GPU row tables (tests/test_gate_bounds_gpu.py runs them; tests/test_gate_bounds_cpu.py checks that they reach what they name) --------
# channel_affine: (name, kinds, voxels, C, sliced, x, off, in place y = x).  grid = 4 na_tiles blocks per sample; "cap": voxels G > 4 x 512 x 256
# = 524288 threads, so a thread walks more than once and vstep matters.  c24 is refused by the host at every type (C % 16 != 0) - the GPU file
# asserts the refusal - so the G = 6 mapping runs at bf16 C 48 and an odd factor at f32 in c48_G12.
AFFINE_ROWS = [
    ("v1_c16_below_one_block", ALL, 1, 16, False, True, True, False),
    ("v100_c48_sliced_xnull", ALL, 100, 48, True, False, True, False),
    ("v257_c80_inplace_offnull", ALL, 257, 80, False, True, False, True),
    ("v720_c48_G12_bothnull", ("f32",), 720, 48, False, False, False, False),
    ("v5_c2048_G512_xnull", ("f32",), 5, 2048, False, False, True, False),
    ("cap_c64_sliced", ("f32",), 32769 + 3, 64, True, True, True, False),
    ("cap_c128_inplace", ("bf16",), 32769 + 3, 128, False, True, True, True),
]
AFFINE_REFUSED = ("v720_c24", ALL, 720, 24)

# dot_stats: (name, modes, voxels, C, sliced).  "cap": voxels G > 512 x 256 = 131072; "odd": the block count is rounded up to a multiple of
# G's odd part and the blocks past the last item must write zeros; G512: blocks that hold no thread of a channel group.
DOT_ROWS = [
    ("v1_c16", BWD_MODES, 1, 16, False),
    ("v100_c48_sliced", BWD_MODES, 100, 48, True),
    ("v257_c80", BWD_MODES, 257, 80, False),
    ("v720_c48_G12", ("f32",), 720, 48, False),
    ("v5_c2048_G512", ("f32",), 5, 2048, False),
    ("cap_c64", ("bf16", "mix16"), 16384 + 5, 64, False),
    ("odd_c48_v150", ("bf16",), 150, 48, False),
    ("odd_c80_v257", ("bf16",), 257, 80, True),
    ("cap_odd_c48", ("bf16",), 22000, 48, False),
]

# gate_mul: (name, forward kinds, backward modes, total voxels, C, a.ld, sliced).  "cap": past grid_for's 4096 blocks - forward voxels G >
# 1048576, backward voxels > 1048576.
GATE_ROWS = [
    ("v1_c16", ALL, BWD_MODES, 1, 16, 16, False),
    ("v255_c48_ald1_sliced", ALL, BWD_MODES, 255, 48, 1, True),
    ("v4099_c128_sliced", ALL, BWD_MODES, 4099, 128, 16, True),
    ("v4099_c16_ald1", ALL, BWD_MODES, 4099, 16, 1, False),
    ("fwd_cap_c64", ("bf16",), (), 131072 + 7, 64, 16, False),
    ("bwd_cap_c16", (), ("bf16",), 1048576 + 7, 16, 1, False),
]

# upsample_c1: (name, forward kinds, backward kinds, N, (D, H, W), factor).  (2, 3, 2) is anisotropic: a transposed tap index shows.
UPS_FACTORS = [(1, 1, 1), (1, 2, 2), (2, 3, 2), (4, 4, 4)]
UPS_ROWS = [(f"n2_357_f{''.join(map(str, f))}", ALL, ("f32", "bf16"), 2, (3, 5, 7), f) for f in UPS_FACTORS] + [
    ("n1_single_voxel", ALL, ("f32", "bf16"), 1, (1, 1, 1), (2, 3, 2)),
    ("fwd_cap", ALL, (), 2, (17, 32, 32), (4, 4, 4)),                      # 2 x 1114112 output voxels > 1048576
    ("bwd_cap", (), ("f32", "bf16"), 2, (4, 257, 256), (1, 1, 2)),         # 526336 input voxels > 524288: 256 blocks, walks of 9
]


# gate_mlp: (tiles, C, R, act, bias, N).  tiles: 1, 3 (fewer rows than lanes at C 16), each side of the 4-deep and 16-deep loop entries of
# gate_column_sum for the C in use (mlp_loop_entries), one full 16-deep pass plus a tail, and 1024 (the engines' cdiv(voxels, 256) at 64^3).
def _mlp_rows():
    rows = []
    for C, R in ((64, 6), (16, 16), (48, 6), (80, 1), (160, 64), (256, 64)):
        e4, e16 = mlp_loop_entries(C)
        lanes = 256 // C
        for k, t in enumerate(sorted({1, 3, e4 - 1, e4, e16 - 1, e16, 16 * lanes, 16 * lanes + 1, 1024})):
            rows.append((t, C, R, 2 + (k % 2), bool(k % 2), 3))
    rows += [(65, 64, 6, a, True, 3) for a in range(9) if a not in (2, 3)]                  # every activation code at one shape
    rows += [(257, 16, 1, 3, True, 1), (1024, 64, 64, 3, False, 17), (76, 48, 6, 2, True, 17), (1024, 64, 6, 3, True, 1), (46, 80, 1, 2, True, 17)]
    return rows


MLP_ROWS = _mlp_rows()
MLP_BITS_ROWS = [(1024, 64), (65, 64), (61, 64), (257, 16), (76, 48), (46, 80), (1024, 256), (17, 160)]      # (tiles, C) of the bit-identity rows


def exact_rows(N, tiles, C, gen):
    """Partial rows whose every partial sum is exact in fp64 (and in any order): multiples of 2^-10 below 8 in magnitude."""
    return (torch.randint(-8191, 8192, (N, tiles, C), generator=gen).double() / 1024).float()

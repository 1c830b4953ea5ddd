"""Element-wise error bounds for the convolution kernels: an fp64 reference of exactly the operands a kernel consumes, and a per-element
bound derived from the operation, so that a small error at a small output (border and halo voxels, channels with small weights) is judged
against that element's own scale instead of the largest output of the tensor.

A check passes when every output element satisfies

    |got - ref| <= u_out |ref| + (1 + u_out) (E + gamma M) + floor

with these terms:

* ``ref``: the operation in float64 on the operands as stored (inputs and weights rounded to the storage type on the host before they are
  uploaded and packed; packing a representable value is exact).  A norm + activation prologue is evaluated in fp64 on the stored input and
  is NOT rounded: the rounding of the operand the device forms is part of ``E``.
* ``u_out``: unit roundoff of the output type, 2^-24 (f32), 2^-11 (f16), 2^-8 (bf16) - the final store rounds once.
* ``M``: the same operator on absolute values, conv(|A|, |W|) + |bias| + |shortcut terms|.  Every term of the fp32 sum is bounded by it.
* ``gamma = K 2^-24``: fp32 accumulation of K terms.  K counts the products (27 Cin, plus the 1x1 shortcut's channels) and the terms the
  epilogue adds (bias, shortcut bias, rank-1 shortcut product).  16-bit products are exact in fp32 (8- or 11-bit significands); an fp32 MFMA
  is a chain of fmaf, one rounding per product-add; the epilogue adds and the rank-1 product round once each.  Whatever the order of the
  sum, each term passes through at most K roundings, so |fl(sum) - sum| <= K 2^-24 sum|terms| to first order.
* ``E``: the error of operands formed on the device, pushed through the operator on absolute values: conv(E_a, |W|).  For a stored operand
  E_a = 0.  For the prologue a = act(scale x + shift):
    - u = scale x + shift in fp32: |du| <= 2^-24 (|scale x| + |u|); the activation moves it by at most L |du| with L = 1.2 >= max|act'|
      over every code (GELU 1.13, SiLU 1.10, the others <= 1);
    - the fp32 activation itself: ELU's exp(u) - 1 (fast exp: 2^-24 (1 + |u|) e^u relative to e^u, at most 2^-24 absolute for u <= 0),
      the divisions of SiLU / sigmoid / tanh, log1p of softplus, GELU's A&S erf (|error| <= 1.5e-7 = 2.5 ulps at 1, times |u| / 2) are each
      a few fp32 ulps: ACT_REL = 8 ulps of |a| plus ACT_ABS = 8 ulps absolute (the cancelling forms e - 1, (1 - e)/(1 + e) near u = 0) plus
      ACT_U = 4 ulps of |scale x| + |shift| (GELU's erf term, which scales with u);
    - the conversion to the 16-bit operand: u_op |a| (and 2^-25 absolute for fp16 subnormals).
  So E_a = u_op |a| + 2^-24 (ACT_REL |a| + ACT_ABS + ACT_U (|scale x| + |shift|) + L (|scale x| + |u|)) [+ 2^-25 for fp16].
  For the input gradient the device forms act'(u) in fp32 and multiplies the fp32 accumulator by it: E_d = 2^-24 (ACT_REL |d| + ACT_ABS +
  ACT_U |u|) (|act''| <= 1 over every code) and the product rounds once more (one more term in K).
* ``floor``: half the spacing of fp16 subnormals, 2^-25, for fp16 outputs; zero otherwise.

Reductions (statistics partials): a partial row is an fp32 sum of fp32 terms; its error is bounded by (sum of the sequential chain lengths of
the reduction levels) 2^-24 sum|terms| plus the element errors of the terms.  The chain lengths are stated where a bound is built.

Nothing here is fitted to a measured value.  NaN / inf anywhere fails a check; the device buffers are pre-filled with NaN so that an element
the kernel never wrote fails too.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
UNIT = {"f32": 2.0 ** -24, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
F16_FLOOR = 2.0 ** -25
ACT_REL, ACT_ABS, ACT_U, ACT_LIP = 8.0, 8.0, 4.0, 1.2
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def norm_recs(B, C, g):
    """InstanceNorm records (mean, rstd, scale, shift) of the form kernel_checks.make_recs draws, fp32 (B, C, 4)."""
    mean = torch.randn(B, C, generator=g) * 0.3
    rstd = 0.5 + torch.rand(B, C, generator=g)
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    scale = gamma[None] * rstd
    return torch.stack([mean, rstd, scale, beta[None] - mean * scale], -1).float().contiguous()


def round_to(t, kind):
    """Round to the storage type and return float64 (what the device holds, exactly)."""
    return t.to(TORCH_DT[kind]).double()


def act64(u, code):
    return {0: lambda v: v, 1: F.elu, 2: F.relu, 3: F.silu, 4: lambda v: F.leaky_relu(v, 0.01), 5: F.gelu, 6: torch.tanh, 7: torch.sigmoid,
            8: F.softplus}[code](u)


def dact64(u, code):
    v = u.detach().clone().requires_grad_(True)
    act64(v, code).sum().backward()
    return v.grad


# ---- operators in float64 on NDHWC tensors (CPU or device; no device convolution: shifted views and matmuls) -------------------------
def conv3_padded(ap, w):
    """Conv3d k = 3 of an already padded (B, D + 2, H + 2, W + 2, Cin) operand with w (Cout, Cin, 3, 3, 3): sum over the 27 taps of a shifted
    slice times the tap's (Cin, Cout) matrix, in the dtype of the operands."""
    B, Dp, Hp, Wp, _ = ap.shape
    D, H, W = Dp - 2, Hp - 2, Wp - 2
    out = torch.zeros(B, D, H, W, w.shape[0], dtype=ap.dtype, device=ap.device)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                out += ap[:, kz:kz + D, ky:ky + H, kx:kx + W, :] @ w[:, :, kz, ky, kx].t()
    return out


def conv3(a, w):
    """Conv3d k = 3, padding 1 on (B, D, H, W, Cin)."""
    return conv3_padded(F.pad(a, (0, 0, 1, 1, 1, 1, 1, 1)), w)


def convT3(dy, w):
    """The input-gradient operator of conv3 (conv_transpose3d, padding 1): conv3 with the weight's taps mirrored and its channels swapped."""
    return conv3(dy, w.flip(2, 3, 4).transpose(0, 1))


def prologue(x, rec, act, op_kind):
    """a = act(scale x + shift) in fp64 from the stored x and the fp32 norm records; E_a per the module docstring.  rec: (B, C, 4) =
    (mean, rstd, scale, shift).  rec None: the stored x itself, E_a = 0."""
    if rec is None:
        return x, torch.zeros_like(x)
    r = rec.double().to(x.device)
    sc, sh = r[:, None, None, None, :, 2], r[:, None, None, None, :, 3]
    sx = x * sc
    a = act64(sx + sh, act)
    ea = UNIT[op_kind] * a.abs() + U32 * (ACT_REL * a.abs() + ACT_ABS + ACT_U * (sx.abs() + sh.abs()) + ACT_LIP * (sx.abs() + (sx + sh).abs()))
    if op_kind == "f16":
        ea = ea + F16_FLOOR
    return a, ea


def finish(ref, M, E, K, out_kind):
    """Per-element bound of a result rounded to out_kind: u_out |ref| + (1 + u_out) (E + K 2^-24 M) + floor."""
    u = UNIT[out_kind]
    return u * ref.abs() + (1 + u) * (E + K * U32 * M) + (F16_FLOOR if out_kind == "f16" else 0.0)


def fwd_reference(x, w, bias, kind, rec=None, act=0, sc=None, wsc=None, bsc=None):
    """bpx_conv3d_fwd in fp64.  x: stored input (B, D, H, W, Cin); w: stored weight (Cout, Cin, 3, 3, 3); bias fp32 (Cout,).  sc: the shortcut
    operand - (B, D, H, W) fp32 image for the rank-1 form (wsc: (Cout,) fp32) or a stored (B, D, H, W, sc_C) tensor (wsc: stored (Cout, sc_C)).
    Returns (ref, bound, pre) where pre is the bound of the fp32 value before the final rounding (what the statistics sum)."""
    a, ea = prologue(x, rec, act, kind)
    wa = w.abs()
    ref = conv3(a, w)
    M = conv3(a.abs(), wa)
    E = conv3(ea, wa) if rec is not None else torch.zeros_like(ref)
    K = 27 * x.shape[-1]
    if bias is not None:
        ref = ref + bias.double()
        M = M + bias.double().abs()
        K += 1
    if sc is not None:
        if sc.dim() == 4:                                  # rank-1: img * w1 rounded once, then added
            t = sc[..., None].double() * wsc.double()
            K += 2
        else:                                              # 1x1 conv of a stored operand: sc_C more products in the same sum
            t = sc @ wsc.t()
            K += sc.shape[-1]
        ref = ref + t
        M = M + (t.abs() if sc.dim() == 4 else sc.abs() @ wsc.abs().t())
        if bsc is not None:
            ref = ref + bsc.double()
            M = M + bsc.double().abs()
            K += 1
    pre = E + K * U32 * M
    return ref, finish(ref, M, E, K, kind), pre


def shuffle_to_fine_grid(t, s):
    """The fused store of bpx_conv3d_fwd_shuffle on a (B, D, H, W, 16 s^3) tensor whose channels are ordered [sub-position][16 channels]:
    channel block (a s + b) s + e of voxel (z, y, x) goes to voxel (s z + a, s y + b, s x + e) of the (B, sD, sH, sW, 16) tensor."""
    B, D, H, W, C = t.shape
    Fc = C // s ** 3
    return t.reshape(B, D, H, W, s, s, s, Fc).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(B, D * s, H * s, W * s, Fc)


def shuffle_reference(x, w_sub, bias_sub, kind, s, rec=None, act=0):
    """bpx_conv3d_fwd_shuffle in fp64: the conv Cin -> 16 s^3 (fwd_reference: the same sum, K = 27 Cin + 1, one rounding at the store) with
    its reference, bound and pre-rounding bound moved together to the fine grid.  w_sub (16 s^3, Cin, 3, 3, 3) and bias_sub (16 s^3,) are in
    the kernels' [sub-position][channel] row order (rcan_engine.rows_to_subposition_major)."""
    ref, bound, pre = fwd_reference(x, w_sub, bias_sub, kind, rec=rec, act=act)
    return tuple(shuffle_to_fine_grid(t, s) for t in (ref, bound, pre))


def dgrad_reference(dy, w, kind, t=None, rec=None, act=0, out_kind=None):
    """bpx_conv3d_dgrad in fp64: g = convT(dy, W) * act'(scale t + shift).  dy, w, t stored values.  The accumulator is exact-operand
    (E = 0); M = convT(|dy|, |W|) |act'|; act' formed in fp32 on the device (E_d, module docstring) scales the accumulator, and the product
    rounds once (K + 1)."""
    c = convT3(dy, w)
    Mc = convT3(dy.abs(), w.abs())
    K = 27 * dy.shape[-1]
    out_kind = out_kind or kind
    if rec is None:
        return c, finish(c, Mc, torch.zeros_like(c), K, out_kind)
    r = rec.double().to(t.device)
    u = t * r[:, None, None, None, :, 2] + r[:, None, None, None, :, 3]
    d = dact64(u, act)
    ed = U32 * (ACT_REL * d.abs() + ACT_ABS + ACT_U * u.abs())
    ref = c * d
    return ref, finish(ref, Mc * d.abs(), Mc * ed, K + 1, out_kind)


def stats_reference(ref, pre, tile_vox):
    """Per-(sample, channel) sums of the statistics partials: (sum v, sum v^2) over every voxel, with their bounds.  The kernels sum the fp32
    value before it is rounded to the storage type (conv3_kernel, conv3_lp_kernel and the z-march kernels: s1 += v, s2 += v * v on the
    accumulator plus bias), so the terms carry the pre-rounding element bound `pre`.  One partial row is one tile: each lane sums its
    tile_vox / 64 voxels in sequence, 16 lanes are summed in 4 butterfly levels and the 4 waves in a chain of 3 - chain tile_vox / 64 + 7;
    the v * v product rounds once more (+1).  The rows are summed here in fp64.
    Power: the element bound `pre` includes the prologue operand's rounding; at bf16 with a prologue (2^-8 per operand) its sum over a
    sample exceeds one tile's contribution, so these sums cannot see a single lost tile there (they do at f32 and f16, and without a
    prologue) - the element rows of the same call catch it, since an unwritten output stays NaN."""
    chain = tile_vox // 64 + 7 + 1
    red = tuple(range(1, ref.dim() - 1))
    av = ref.abs() + pre
    s1 = ref.sum(red)
    s2 = (ref * ref).sum(red)
    b1 = pre.sum(red) + chain * U32 * av.sum(red)
    b2 = (pre * (2 * ref.abs() + pre)).sum(red) + chain * U32 * (av * av).sum(red)
    return torch.stack([s1, s2], 1), torch.stack([b1, b2], 1)


def compare(name, got, ref, bound, axes="nzyxc"):
    """Element-wise check.  Returns a result dict (kernel_checks._res form) with err = max |got - ref| / bound, tol = 1, the worst element's
    position named by `axes`, and the count of non-finite values (any of which fails)."""
    got = got.double().to(ref.device)
    bad = int((~torch.isfinite(got)).sum().item())
    r = (got - ref).abs() / bound
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, math.inf))
    i = int(torch.argmax(r.reshape(-1)).item())
    worst = float(r.reshape(-1)[i].item())
    pos = []
    for s in reversed(ref.shape):
        pos.append(i % s)
        i //= s
    where = ", ".join(f"{k}={v}" for k, v in zip(axes, reversed(pos)))
    ok = bad == 0 and worst <= 1.0
    return dict(name=name, err=worst if bad == 0 else math.inf, tol=1.0, ok=bool(ok), extra=f"worst at ({where}); non-finite {bad}")


# ---- the forward route table ----------------------------------------------------------------------------------------------------------
# Every dispatch route of bpx_conv3d_fwd / bpx_conv3d_fwd_pool (pick_cfg in conv3d_shared.h, launch_conv3 / use_lean in conv3d_igemm.hip,
# launch_conv3_zm in conv3d_zmarch.hip), the lean kernel with more than one output-channel workgroup (blockIdx.y > 0: the *_two_blocks rows)
# included; the third forward entry, bpx_conv3d_fwd_shuffle (the lean kernel's pixel-shuffle store), has its own table, SHUFFLE_ROWS, below.  cfg = the (tz, ty, tx, ns) tile configuration the row reaches; kinds = the storage types it runs at
# (4x8x16 and the lean / z-march / two-K-group kernels are 16-bit only).  Hooks: ws (bpx_debug_set_conv_ws: 4 = double-buffered kernel,
# 5 = lean kernel), kg (bpx_debug_set_conv_kg), zm (bpx_debug_set_conv_zm; the row expects the z-march kernel to run when zm != 0),
# occ (bpx_debug_set_conv_occ: fewer persistent workgroups, so the grid wraps).  sc: 0, 1 (rank-1 image) or the 1x1 shortcut's channels.
# layout: "dense", "planar" (chunk-planar x, sc and y) or "slice" (channel slices of wider buffers).  act: 0 = no prologue.
ALL, W16 = ("f32", "bf16", "f16"), ("bf16", "f16")


def _r(name, kinds, B, S, Cin, Cout, cfg, act=1, sc=0, layout="dense", ws=0, kg=-1, zm=0, occ=0, pool=0):
    return dict(name=name, kinds=kinds, B=B, S=S, Cin=Cin, Cout=Cout, cfg=cfg, act=act, sc=sc, layout=layout, ws=ws, kg=kg, zm=zm, occ=occ,
                pool=pool)


BIG = (17, 33, 65)          # >= 32^3 voxels, one voxel past a 4x8x16 tile on every axis
FWD_ROUTES = [
    # double-buffered kernel, 4x4x8 tiles (<= 16^3 volumes or W <= 8)
    _r("s448_ns1_ragged", ALL, 3, (5, 6, 7), 16, 16, (4, 4, 8, 1)),
    _r("s448_ns2_D2", ALL, 1, (2, 9, 13), 32, 32, (4, 4, 8, 2), sc=16),
    _r("s448_ns3_H3_rank1", ALL, 3, (9, 3, 17), 16, 48, (4, 4, 8, 3), sc=1),
    _r("s448_ns4_kg2", ALL, 3, (9, 10, 11), 64, 64, (4, 4, 8, 4), kg=1),
    _r("s448_ns4_kg1", W16, 3, (9, 10, 11), 64, 64, (4, 4, 8, 4), kg=0),
    _r("s448_ns2_8cube_kg2", ALL, 1, (8, 8, 8), 128, 64, (4, 4, 8, 2), kg=1, act=0),
    _r("s448_ns2_8cube_kg1", W16, 1, (8, 8, 8), 128, 64, (4, 4, 8, 2), kg=0, act=0),
    _r("s448_ns1_W8_slice", ALL, 1, (6, 20, 8), 32, 16, (4, 4, 8, 1), layout="slice"),
    # double-buffered kernel, 4x4x16 tiles
    _r("s4416_ns1_sc16", ALL, 3, (9, 17, 33), 16, 16, (4, 4, 16, 1), sc=16),
    _r("s4416_ns2_planar", ALL, 1, (8, 12, 47), 32, 32, (4, 4, 16, 2), layout="planar", sc=16),
    _r("s4416_ns3_slice", ALL, 3, (5, 13, 65), 16, 48, (4, 4, 16, 3), layout="slice"),
    _r("s4416_ns4_rank1", ALL, 1, (6, 9, 81), 32, 64, (4, 4, 16, 4), sc=1),
    _r("s4416_ns1_big_f32", ("f32",), 1, BIG, 16, 16, (4, 4, 16, 1)),
    # double-buffered kernel, 4x8x16 tiles (16-bit, >= 32^3 voxels)
    _r("s4816_ws4", W16, 1, BIG, 16, 16, (4, 8, 16, 1), ws=4, sc=1),
    # lean persistent kernel
    _r("lean4816", W16, 3, BIG, 16, 16, (4, 8, 16, 1)),
    _r("lean4816_silu_sc16", W16, 1, BIG, 16, 16, (4, 8, 16, 1), act=3, sc=16),
    _r("lean4416_ns1_ws5", W16, 3, (9, 17, 33), 16, 16, (4, 4, 16, 1), ws=5, sc=1),
    _r("lean4416_ns2_ws5_planar", W16, 1, (9, 17, 33), 32, 32, (4, 4, 16, 2), ws=5, layout="planar"),
    _r("lean4416_ns3_ws5_slice", W16, 3, (9, 17, 33), 16, 48, (4, 4, 16, 3), ws=5, layout="slice"),
    _r("lean4416_ns4_ws5", W16, 1, (9, 17, 33), 32, 64, (4, 4, 16, 4), ws=5, sc=32),
    _r("lean4816_wrap", W16, 2, (40, 48, 64), 16, 16, (4, 8, 16, 1), occ=1),
    # lean kernel, two output-channel workgroups per tile (co_base = blockIdx.y * 16 NS > 0: weights, bias, shortcut, store and partials of block 1)
    _r("lean4416_ns4_two_blocks", W16, 1, BIG, 16, 128, (4, 4, 16, 4)),
    _r("lean4416_ns3_two_blocks", W16, 3, BIG, 16, 96, (4, 4, 16, 3), sc=16),
    # z-march kernels (16 output channels of the 4x8x16 tile)
    _r("zm_rolesplit", W16, 3, BIG, 16, 16, (4, 8, 16, 1), zm=2, sc=1),
    _r("zm_onechunk", W16, 1, BIG, 16, 16, (4, 8, 16, 1), zm=6),
    _r("zm_onechunk_sc16_planar", W16, 1, BIG, 16, 16, (4, 8, 16, 1), zm=2, sc=16, layout="planar"),
    _r("zm_threechunks", W16, 3, BIG, 48, 16, (4, 8, 16, 1), zm=2),
    _r("zm_wrap", W16, 2, (40, 48, 64), 16, 16, (4, 8, 16, 1), zm=2 | (64 << 8)),
    # fused pooling (lean and z-march)
    _r("pool_lean_48", W16, 1, (32, 32, 32), 48, 16, (4, 8, 16, 1), pool=2),
    _r("pool_lean_sz1", W16, 3, (32, 32, 32), 16, 16, (4, 8, 16, 1), pool=1),
    _r("pool_zm", W16, 1, (32, 32, 32), 16, 16, (4, 8, 16, 1), pool=2, zm=2),
] + [
    # the plain kernels' activation codes (use_lean refuses 4..8; ACTK = 0 for 2, 3, ACTK = 2 for the rest)
    _r(f"s448_act{a}", ALL, 1, (5, 9, 10), 16, 32, (4, 4, 8, 2), act=a) for a in range(2, 9)
] + [_r("s4816_gelu", W16, 1, BIG, 16, 16, (4, 8, 16, 1), act=5)]

# bpx_conv3d_fwd_shuffle rows: the conv Cin -> 16 s^3 with the 3-D pixel shuffle by s fused into the lean kernel's store (conv3d_lean.hip,
# p.ps > 1).  Cout = 128 (s 2: NS 4, 2 channel workgroups), 432 (s 3: NS 3, 9) or 1024 (s 4: NS 4, 16).  act: 0 = no prologue, else in_norm
# records + that code.  samples: the samples that are compared (None: all of them) - the reference is built for those only.
def _s(name, kinds, B, S, Cin, s, cfg, act=0, samples=None):
    return dict(name=name, kinds=kinds, B=B, S=S, Cin=Cin, s=s, cfg=cfg, act=act, samples=samples)


SHUFFLE_ROWS = [
    _s("x2_ragged", W16, 3, BIG, 16, 2, (4, 4, 16, 4)),                       # edge tiles on every axis; sample 1 alone has the same bits
    _s("x3_ragged", W16, 1, BIG, 16, 3, (4, 4, 16, 3)),                       # s not a power of two in the / and % of ysub
    _s("x4_ragged", W16, 1, BIG, 16, 4, (4, 4, 16, 4)),
    _s("x2_D3", ("bf16",), 1, (3, 100, 112), 16, 2, (4, 4, 16, 4)),           # D smaller than a tile, 33 600 voxels
    _s("x2_silu_prologue", W16, 1, BIG, 16, 2, (4, 4, 16, 4), act=3),         # in_norm records + SiLU: admitted by the entry
    _s("x2_cin32", ("bf16",), 1, BIG, 32, 2, (4, 4, 16, 4)),                  # x.C = 32: admitted by the entry
    # the largest batch the size check admits at 32^3, s 4: 31 * 2^25 output elements (< 2^30), byte offsets up to just under 2^31
    _s("x4_last_sample", ("bf16",), 31, (32, 32, 32), 16, 4, (4, 4, 16, 4), samples=(0, 30)),
]

# bpx_conv3d_bwd_fused rows (dtype, B, S, Ct, Cdy): every instance bpx_conv3d_bwd_fused_supported admits (MIX16 = 4, BF16 = 1)
BWD_FUSED_ROWS = [(4, 3, BIG, 16, 16), (4, 1, BIG, 48, 16), (1, 1, BIG, 16, 16), (4, 1, BIG, 32, 32), (4, 1, BIG, 16, 32)]

# every tile configuration launch_conv3 instantiates (conv3d_igemm.hip): 4x8x16 for 16-bit storage only
LAUNCH_CONV3_CFGS = {k: [(4, 4, 16, n) for n in (1, 2, 3, 4)] + [(4, 4, 8, n) for n in (1, 2, 3, 4)] + ([(4, 8, 16, 1)] if k != "f32" else [])
                     for k in ALL}


def runs_plain_kernel(row, kind):
    """Whether a route row takes conv3_kernel (launch_conv3) rather than the lean or z-march kernels: fp32 always; 16-bit storage below
    32^3 voxels per sample without the lean hook, with the double-buffered hook, or with an activation code use_lean refuses."""
    if kind == "f32":
        return True
    D, H, W = row["S"]
    if row["ws"] == 4 or row["act"] > 3:
        return True
    return row["ws"] != 5 and D * H * W < 32768 or row["cfg"][2] != 16


# ---- weight gradients -------------------------------------------------------------------------------------------------------------
def wgrad_chains(T, G, tile_vox):
    """Sequential chain lengths of bpx_conv3d_wgrad's reductions (wgrad.hip), for T tiles reduced into G partial slabs:
    - inside a slab: a workgroup walks its tiles (tile = group + k G, or with the y-strip walk of the windowed kernel a contiguous range of
      ceil(T / 8) ids split over ceil(G / 8) slots: at most ceil(T / G) + 1 tiles) and accumulates every voxel of them into one accumulator
      per (ci, co, tap): at most one rounding per product, (ceil(T / G) + 1) tile_vox;
    - the k = 1 kernels add the 4 waves' accumulators through LDS: 3;
    - the bias column sums: one partial per thread over the same voxels, then up to 256 partials added in sequence: 256;
    - wgrad_reduce_kernel: each lane sums every GL-th slab in four interleaved accumulators, (s0 + s1) + (s2 + s3), then the GL lanes in
      sequence: at most G + 3.
    Returns (chain of dW, chain of db)."""
    slab = (-(-T // G) + 1) * tile_vox
    return slab + 3 + G + 3, slab + 256 + G + 3


def wgrad_reference(x, dy, k, op_kind, rec=None, act=0, chains=(0, 0)):
    """dW[co][ci][tap] = sum_v a[v + tap][ci] dy[v][co] and db[co] = sum_v dy[v][co] in fp64, with their bounds: the fp32 outputs round once
    (2^-24 |ref|), the prologue operand carries E_a (formed on the device, then rounded to the MFMA operand type op_kind), and the sum carries
    chain 2^-24 sum|terms| with the chain lengths of wgrad_chains."""
    a, ea = prologue(x, rec, act, op_kind)
    B, D, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    g2, ga = dy.reshape(-1, Cout), dy.abs().reshape(-1, Cout)
    r = k // 2
    ap, aa, ee = (F.pad(t, (0, 0) + (r, r) * 3) for t in (a, a.abs(), ea))
    ref = torch.zeros(Cout, Cin, k, k, k, dtype=torch.float64, device=x.device)
    M, E = torch.zeros_like(ref), torch.zeros_like(ref)
    for kz in range(k):
        for ky in range(k):
            for kx in range(k):
                sl = lambda t: t[:, kz:kz + D, ky:ky + H, kx:kx + W, :].reshape(-1, Cin)
                ref[:, :, kz, ky, kx] = (sl(ap).t() @ g2).t()
                M[:, :, kz, ky, kx] = (sl(aa).t() @ ga).t()
                E[:, :, kz, ky, kx] = (sl(ee).t() @ ga).t()
    bound = U32 * ref.abs() + (1 + U32) * (E + chains[0] * U32 * M)
    db = g2.sum(0)
    db_bound = U32 * db.abs() + (1 + U32) * chains[1] * U32 * ga.sum(0)
    return ref, bound, db, db_bound

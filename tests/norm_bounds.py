"""Element-wise error bounds for the kernels BETWEEN the convolutions of a train step - statistics partials, norm records, InstanceNorm /
GroupNorm backward coefficients, the coefficient apply, the materialised norm + activation, the 1x1x1 GEMM with the IN-backward affine and
max pooling - in the form of tests/conv_bounds.py, whose comparator, rounding helpers and activation terms are reused here:

    |got - ref| <= u_out |ref| + (1 + u_out) (E + K 2^-24 M) + floor          (conv_bounds.finish)

``ref`` is the operation in float64 on the operands as stored, ``M`` the sum of the absolute terms, ``K`` the number of fp32 roundings a term
passes through, ``E`` the error of operands formed on the device pushed through on absolute values.  For reductions the bound is the sum
of the element errors of the terms plus ``chain 2^-24 sum|terms|``; every chain length is read off the kernel and stated where the bound is
built.  Pooling is a selection, one fp32 add of two representable values and one round-to-nearest-even store: it is compared bit for bit.

Nothing here is fitted to a measured value.  NaN / inf fails (conv_bounds.compare), outputs are pre-filled with NaN by the callers, and no
element is left out of a comparison.
"""
from __future__ import annotations

import math

import torch

import conv_bounds as CB
from conv_bounds import ACT_ABS, ACT_LIP, ACT_REL, ACT_U, U32, UNIT, act64, compare, dact64, finish, norm_recs, round_to  # noqa: F401

U64 = 2.0 ** -53
KINDS = ("f32", "bf16", "f16")
MODES = {"f32": ("f32", "f32"), "bf16": ("bf16", "bf16"), "mix16": ("bf16", "f16")}   # mode -> (gradient storage, activation storage)


# ---- partial sums -------------------------------------------------------------------------------------------------------------------
def sums_reference(t1, e1, t2, e2, chain):
    """(sum t1, sum t2) over axis 1 of (B, V, C) fp64 terms with element error bounds e1, e2 (tensors or 0.0): per (sample, sum, channel)
    |got - ref| <= sum e + chain 2^-24 sum (|t| + e), the form of conv_bounds.stats_reference.  The partial ROWS are summed in fp64 by the
    caller, so `chain` is the longest sequence of fp32 additions INSIDE one row (plus the roundings of forming a term where e does not
    carry them).
    Power: one lost row is caught where the terms are exact (tensor statistics, pooling: the bound is chain 2^-24 of the absolute sum).  For
    S1 / S2 at bf16 with an activation derivative formed on the device the element errors add up like those of the convolutions' statistics
    (conv_bounds.stats_reference); there the lost row is caught by the coefficient rows downstream and an unwritten row is NaN."""
    z = torch.zeros_like(t1)
    e1, e2 = z + e1, z + e2
    s = torch.stack([t1.sum(1), t2.sum(1)], 1)
    b = torch.stack([e1.sum(1) + chain * U32 * (t1.abs() + e1).sum(1), e2.sum(1) + chain * U32 * (t2.abs() + e2).sum(1)], 1)
    return s, b


def tensor_stats_chain(C, kind, wide):
    """Longest fp32 chain of one bpx_tensor_stats row (256 voxels).  tensor_stats_kernel (one channel per lane): the 256 voxels in sequence,
    256.  tensor_stats_vec_kernel: slots = 256 / (C / VEC) voxel slots walk ceil(256 / slots) voxels each, then the slots are added in
    sequence through LDS: ceil(256 / slots) + slots.  One more for f * f (the product rounds unless it contracts into an fma)."""
    if not wide:
        return 256 + 1
    slots = 256 // (C // (4 if kind == "f32" else 8))
    return -(-256 // slots) + slots + 1


def tensor_stats_reference(x, chain):
    """bpx_tensor_stats: (sum x, sum x^2) per (sample, channel) of the stored x (B, V, C); the terms are exact functions of stored values
    (the kernel converts to fp32 exactly), so the element errors are zero and only the chain remains."""
    return sums_reference(x, 0.0, x * x, 0.0, chain)


def pool_stats_reference(y, C, kind):
    """The statistics rows of maxpool_fwd_kernel: sums of the pooled values m (a selection of stored x: exact), s1 += m, s2 += m * m.
    A thread sums POOL_IPT = 4 items, then one thread per (sum, channel) adds the blockDim / G threads of its channel group in sequence
    (blockDim = (256 / G) G, G = C / KPL): chain 4 + 256 / G, one more for m * m."""
    G = C // (4 if kind == "f32" else 8)
    yy = y.reshape(y.shape[0], -1, C)
    return sums_reference(yy, 0.0, yy * yy, 0.0, 4 + 256 // G + 1)


def xhat_terms(t, rec):
    """xhat = (t - mean) rstd as the backward kernels form it in fp32 from the stored t and the fp32 record: (t - mean) rounds once, the
    product once (conv3_kernel, norm_act_bwd_kernel, bpx_conv3d_bwd_fused); the lean dgrad kernel's ELU instance uses fma(rstd, t, -mean rstd):
    the product mean rstd rounds once and the fma once.  Either way |d xhat| <= 2 2^-24 |rstd| (|t| + |mean|).  t: (B, ..., C)."""
    r = rec.double().to(t.device)
    sh = (r.shape[0],) + (1,) * (t.dim() - 2) + (r.shape[1],)
    mean, rstd = r[..., 0].reshape(sh), r[..., 1].reshape(sh)
    xh = (t - mean) * rstd
    return xh, 2 * U32 * rstd.abs() * (t.abs() + mean.abs())


def red_reference(g, eg, t, rec, chain):
    """(S1 = sum g, S2 = sum g xhat) per (sample, channel).  g: the fp64 gradient (B, ..., C); eg: the bound of the fp32 value the kernel
    sums (every kernel here sums the fp32 product BEFORE it is rounded to the storage type and before an addend joins it); xhat from
    xhat_terms.  Term errors: eg for S1; eg (|xhat| + dxh) + |g| dxh for S2, and one rounding of the product g xhat (in the chain: + 1)."""
    xh, dxh = xhat_terms(t, rec)
    B, C = g.shape[0], g.shape[-1]
    f = lambda v: v.reshape(B, -1, C)
    e2 = eg * (xh.abs() + dxh) + g.abs() * dxh
    return sums_reference(f(g), f(eg), f(g * xh), f(e2), chain + 1)


# ---- records -------------------------------------------------------------------------------------------------------------------------
def row_totals(part):
    """fp64 totals (N, 2, C) of partial rows (N, T, 2, C) as the finalize kernels form them, with the bound of what the device may differ by:
    - the kernels add the rows in fp64 in another order than this sum: (T + 16) 2^-53 sum|rows|;
    - above 1024 rows compact_stats first sums segments of cdiv(T, 32) rows in fp64 and writes each segment total back AS A FLOAT:
      2^-24 sum|segment totals| (only there)."""
    p = part.double()
    N, T, _, C = p.shape
    S = p.sum(1)
    d = (T + 16) * U64 * p.abs().sum(1)
    if T > 1024:
        seg = -(-T // 32)
        nseg = -(-T // seg)
        pad = torch.zeros(N, nseg * seg - T, 2, C, dtype=p.dtype, device=p.device)
        segs = torch.cat([p, pad], 1).reshape(N, nseg, seg, 2, C).sum(2)
        d = d + U32 * segs.abs().sum(1)
    return S, d


def group_fold(v, cpg):
    """Sum over the channels of each group, repeated to every channel of the group: (..., C) -> (..., C)."""
    C = v.shape[-1]
    return v.reshape(*v.shape[:-1], C // cpg, cpg).sum(-1, keepdim=True).expand(*v.shape[:-1], C // cpg, cpg).reshape(v.shape)


def records_from_totals(S, d, count, gamma, beta, eps, cpg):
    """The records (mean, rstd, scale, shift) from per-channel totals S (N, 2, C) known to within d (norm_finalize_kernel, gn_finalize_kernel):
        m = A / n, v = max(B / n - m^2, 0), rstd = 1 / sqrt(v + eps), scale = gamma rstd, shift = beta - m gamma rstd
    with A, B the group's totals and n = count x channels per group, formed in fp64; the last lines round to fp32:
        mean = (float)m                       one rounding
        rstd = (float)(1 / sqrt(v + eps))     one rounding
        scale = ga * rstd                     a second one
        shift = be - (float)m * ga * rstd     (float)m, rstd, two products, one subtraction: 5 roundings over |be| + |m scale|
    and the error of the totals is propagated: dm = d1 / n, dv = d2 / n + 2 |m| dm, d rstd = dv / (2 (v + eps - dv)^(3/2)).
    Returns (ref (N, C, 4), bound (N, C, 4), ok) where ok says dv < (v + eps) / 2 everywhere - a case only counts if it holds.
    Power: a GroupNorm `shift` formed with ONE channel's own mean (S1[q] / count of a channel q of the group) instead of the group's is
    rejected wherever the channel means differ by more than these few ulps; it is invisible only where they coincide."""
    n = float(count) * cpg
    A, Bq = group_fold(S[:, 0], cpg), group_fold(S[:, 1], cpg)
    d1, d2 = group_fold(d[:, 0], cpg), group_fold(d[:, 1], cpg)
    ga, be = gamma.double().to(S.device)[None], beta.double().to(S.device)[None]
    m = A / n
    v = (Bq / n - m * m).clamp_min(0.0)
    dm = d1 / n
    dv = d2 / n + 2 * m.abs() * dm + 4 * U64 * (Bq.abs() / n + m * m)      # (the subtraction B / n - m^2 itself, in fp64)
    ve = v + float(eps)
    ok = bool((dv < ve / 2).all().item())
    rstd = ve.rsqrt()
    drs = dv / (2 * (ve - dv).clamp_min(1e-300) ** 1.5)
    scale = ga * rstd
    shift = be - m * scale
    ref = torch.stack([m.expand_as(rstd), rstd, scale, shift], -1)
    b_mean = dm + U32 * m.abs()
    b_rstd = drs + U32 * rstd
    b_scale = ga.abs() * b_rstd + U32 * scale.abs()
    b_shift = dm * scale.abs() + m.abs() * ga.abs() * drs + 5 * U32 * (be.abs() + (m * scale).abs())
    return ref, torch.stack([b_mean.expand_as(rstd), b_rstd, b_scale, b_shift], -1), ok


def records_reference(part, count, gamma, beta, eps, cpg):
    """bpx_norm_finalize (and bpx_norm_channel_sums + bpx_groupnorm_finalize) from GIVEN partial rows (N, T, 2, C) fp32."""
    S, d = row_totals(part)
    return records_from_totals(S, d, count, gamma, beta, eps, cpg)


def records_from_tensor(x, chain, count, gamma, beta, eps, cpg):
    """The same through bpx_tensor_stats: the partial-sum bound of tensor_stats_reference is the error of the totals (plus the fp64 order
    term of row_totals)."""
    S, d = tensor_stats_reference(x, chain)
    T = -(-x.shape[1] // 256)
    d = d + (T + 16) * U64 * torch.stack([x.abs().sum(1), (x * x).sum(1)], 1)
    return records_from_totals(S, d, count, gamma, beta, eps, cpg)


# ---- backward coefficients -------------------------------------------------------------------------------------------------------------
def coef_from_totals(S, d, rec, gamma, count, cpg):
    """norm_bwd_finalize_kernel / _ps_kernel / gn_bwd_finalize_kernel (the comment above norm_bwd_finalize_kernel): with m1, m2 the group means
    of gamma S1, gamma S2 (fp64),  a = gamma rstd,  b = -rstd^2 m2,  c0 = -rstd m1 + rstd^2 mean m2, each rounded to fp32 ONCE; the error d of
    the totals is propagated and the fp64 cancellation of c0's two terms is counted (4 2^-53 of their absolute sum).
    Returns (ref (N, C, 3), bound (N, C, 3))."""
    n = float(count) * cpg
    r = rec.double().to(S.device)
    ga = gamma.double().to(S.device)[None]
    m1, m2 = group_fold(ga * S[:, 0], cpg) / n, group_fold(ga * S[:, 1], cpg) / n
    e1, e2 = group_fold(ga.abs() * d[:, 0], cpg) / n, group_fold(ga.abs() * d[:, 1], cpg) / n
    mean, rs = r[..., 0], r[..., 1]
    a = ga * rs
    b = -rs * rs * m2
    c0 = -rs * m1 + rs * rs * mean * m2
    ba = U32 * a.abs()
    bb = rs * rs * e2 + U32 * b.abs() + 4 * U64 * b.abs()
    bc = rs.abs() * e1 + rs * rs * mean.abs() * e2 + U32 * c0.abs() + 4 * U64 * ((rs * m1).abs() + (rs * rs * mean * m2).abs())
    return torch.stack([a.expand_as(b), b, c0], -1), torch.stack([ba.expand_as(b), bb, bc], -1)


def param_grads_from_totals(S, d, init_g, init_b, deferred):
    """dgamma[c] = init + sum_n S2[n][c], dbeta[c] = init + sum_n S1[n][c]: every entry ADDS to what the buffers hold.
    Plain and GroupNorm entries: each per-sample total enters as a float ((double)(float)tot: 2^-24 |S_n| each), the sum over the samples is
    fp64, rounds to fp32 once and is added to the buffer in fp32 (one more rounding of the result).
    Deferred entry: the per-sample totals are written as floats over the first partial row (2^-24 |S_n| each) and bpxred::reduce_rows sums
    the N rows in fp32 (wgrad_reduce_kernel: lanes take every GL-th row, (s0 + s1) + (s2 + s3), then the GL lanes in sequence: a chain of at
    most N + 3) before `dst[i] += s`.
    Returns [(dgamma ref, bound), (dbeta ref, bound)]."""
    out = []
    for k, init in ((1, init_g), (0, init_b)):
        tot = S[:, k].sum(0)
        ab = S[:, k].abs().sum(0)
        ref = init.double().to(S.device) + tot
        chain = (S.shape[0] + 3) if deferred else 1
        out.append((ref, d[:, k].sum(0) + U32 * ab + chain * U32 * ab + U32 * ref.abs()))
    return out


# ---- element-wise kernels ------------------------------------------------------------------------------------------------------------
def _bc(coef, nd):
    """(N, C, k) coefficients / records broadcast over the voxel axes of an (N, ..., C) tensor: a tuple of k (N, 1.., C) views."""
    c = coef.double()
    sh = (c.shape[0],) + (1,) * (nd - 2) + (c.shape[1],)
    return tuple(c[..., i].reshape(sh) for i in range(c.shape[-1]))


def apply_reference(g, t, coef, addend, out_kind):
    """bpx_norm_bwd_apply: dx = a g + b t + c0 (+ addend) on the stored g, t, addend and the fp32 coefficients.  The line
    `ka * g + kb * t + kc` is two products and two additions, the addend a third: K = 4 (5 with the addend); contraction to fma only lowers it."""
    a, b, c0 = _bc(coef.to(g.device), g.dim())[:3]
    ref = a * g + b * t + c0
    M = (a * g).abs() + (b * t).abs() + c0.abs()
    K = 4
    if addend is not None:
        ref, M, K = ref + addend, M + addend.abs(), 5
    return ref, finish(ref, M, 0.0, K, out_kind)


def _act_terms(x, rec):
    _, _, sc, sh = _bc(rec.to(x.device), x.dim())
    sx = x * sc
    u = sx + sh
    return sx, sh, u, U32 * (sx.abs() + u.abs())                    # du: u = scale x + shift in fp32 (two roundings, one with fma)


def norm_act_fwd_reference(x, rec, act, kind):
    """bpx_norm_act_fwd: y = act(scale x + shift), the terms of conv_bounds.prologue WITHOUT the operand rounding (the result is stored
    once, u_out |ref|): E = 2^-24 (ACT_REL |y| + ACT_ABS + ACT_U (|scale x| + |shift|) + ACT_LIP (|scale x| + |u|))."""
    sx, sh, u, _ = _act_terms(x, rec)
    y = act64(u, act)
    E = U32 * (ACT_REL * y.abs() + ACT_ABS + ACT_U * (sx.abs() + sh.abs()) + ACT_LIP * (sx.abs() + u.abs()))
    return y, finish(y, 0.0, E, 0, kind)


def norm_act_bwd_reference(dy, x, rec, act, addend, out_kind):
    """bpx_norm_act_bwd: g = dy act'(u) (+ addend).  act'(u) is formed in fp32: E_d of conv_bounds.dgrad_reference, 2^-24 (ACT_REL |d| +
    ACT_ABS + ACT_U |u|), plus the error of u itself through |act''| <= 1 (du), plus - ReLU and leaky ReLU only, whose derivative jumps at
    0 - the whole jump where |u| <= 2 du.  The product rounds once, the addend's addition once more.
    Returns (ref, bound, gv, egv): gv the product term alone with the bound of its fp32 value (what S1 / S2 sum)."""
    sx, sh, u, du = _act_terms(x, rec)
    d = dact64(u, act)
    ed = U32 * (ACT_REL * d.abs() + ACT_ABS + ACT_U * u.abs()) + du
    if act in (2, 4):
        ed = ed + (u.abs() <= 2 * du).double()
    gv = dy * d
    egv = dy.abs() * ed + U32 * gv.abs()
    ref, M, K = gv, gv.abs(), 1
    if addend is not None:
        ref, M, K = gv + addend, M + addend.abs(), 2
    return ref, finish(ref, M, dy.abs() * ed, K, out_kind), gv, egv


def norm_act_bwd_chain(voxels, C, kind, tiles):
    """Chain of one norm_act_bwd_kernel row: a thread walks ceil(voxels G / (tiles 256)) items, then one thread per (sum, channel) adds the
    256 / G threads of its channel group in sequence."""
    G = C // (4 if kind == "f32" else 8)
    return -(-voxels * G // (tiles * 256)) + -(-256 // G)


# ---- 1x1x1 GEMM with the IN-backward affine -----------------------------------------------------------------------------------------------
def affine_reference(x, w, g, t, coef, addend=None, bias=None, out_kind="bf16"):
    """bpx_conv1x1_fwd / _fwd_split (/_wgrad) with the affine: y = x W^T + a g + b t + c0 (+ bias) (+ addend).  x (B, V, Cin), w (Ncols, Cin)
    stored; g, t (B, V, Ncols) stored; coef (B, Ncols, 4) fp32.  Cin exact products accumulate in fp32 (one rounding each), the epilogue
    `val += a g + b t + c0` is two products and three additions (5), bias and addend one each: pw_kernel and pw_nbs_kernel alike."""
    a, b, c0 = _bc(coef.to(x.device), 3)[:3]
    ref = x @ w.t() + a * g + b * t + c0
    M = x.abs() @ w.abs().t() + (a * g).abs() + (b * t).abs() + c0.abs()
    K = x.shape[-1] + 5
    if bias is not None:
        ref, M, K = ref + bias.double(), M + bias.double().abs(), K + 1
    if addend is not None:
        ref, M, K = ref + addend, M + addend.abs(), K + 1
    return ref, finish(ref, M, 0.0, K, out_kind)


def pws_wgrad_reference(t, x, mixed, nblocks, groups=256):
    """dWsc[co][ci] = sum_v t[v][ci] dOut[v][co] of pw_nbs_kernel<.., WG> (returned as (K, 3K) = (co, ci), the layout of dw_d), in the form of
    conv_bounds.wgrad_reference.  Mixed mode: the fp16 t is converted to a bf16 MFMA operand, E = 2^-8 |t| per operand.  Chain: a wave owns
    one 32-voxel chunk of every block of its workgroup's walk (one MFMA step of 32 products each, ceil(nblocks / groups) blocks), the waves'
    sums meet in at most 2 additions, and bpxred::reduce_partials adds the `groups` slabs (at most groups + 3)."""
    B, V, K = x.shape
    tf, xf = t.reshape(B * V, -1), x.reshape(B * V, K)
    ref = xf.t() @ tf
    M = xf.abs().t() @ tf.abs()
    E = (UNIT["bf16"] * M) if mixed else torch.zeros_like(M)
    chain = 32 * -(-nblocks // groups) + 2 + groups + 3
    return ref, U32 * ref.abs() + (1 + U32) * (E + chain * U32 * M)


# ---- pooling: exact -------------------------------------------------------------------------------------------------------------------
def pool_windows(x, sz):
    """(B, D, H, W, C) -> (B, Do, Ho, Wo, 4 sz, C): the window of every output voxel in the kernels' order k = (dz, dy, dx) row-major."""
    B, D, H, W, C = x.shape
    v = x.reshape(B, D // sz, sz, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4, 6, 7)
    return v.reshape(B, D // sz, H // 2, W // 2, 4 * sz, C)


def pool_unwindow(v, sz):
    B, Do, Ho, Wo, _, C = v.shape
    return v.reshape(B, Do, Ho, Wo, sz, 2, 2, C).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(B, Do * sz, Ho * 2, Wo * 2, C)


def pool_argmax(x, sz, last=False):
    """Index of the FIRST maximum of every window under a strict `>` starting from -inf (maxpool_*_kernel; +0 and -0 compare equal, so the
    first of them wins).  last=True: the last maximum (a fault, for the CPU self-test)."""
    w = pool_windows(x, sz).double()
    m = torch.full_like(w[..., 0, :], -math.inf)
    am = torch.zeros_like(m, dtype=torch.long)
    for k in range(w.shape[-2]):
        f = w[..., k, :]
        take = (f >= m) if last else (f > m)
        m = torch.where(take, f, m)
        am = torch.where(take, torch.full_like(am, k), am)
    return am


def pool_fwd_reference(x, sz):
    """y = the window's first maximum, its stored bits (x in its storage dtype).  Returns (y, arg-max)."""
    am = pool_argmax(x, sz)
    return torch.gather(pool_windows(x, sz), -2, am[..., None, :]).squeeze(-2), am


def pool_bwd_reference(x, dy, addend, sz, am=None):
    """dx = round(addend + (v is the first maximum of its window ? dy : 0)) in the kernel's own arithmetic: fp32 values of the stored
    operands, ONE fp32 addition (0 + where no addend is given), one round-to-nearest-even store to dy's dtype.  x may have another storage type
    than dy (MIX16: fp16 x); am overrides the arg-max (faults of the CPU self-test)."""
    am = pool_argmax(x, sz) if am is None else am
    nw = 4 * sz
    hit = torch.arange(nw, device=dy.device)[:, None] == am[..., None, :]
    sel = torch.where(hit, dy.float()[..., None, :], torch.zeros((), dtype=torch.float32, device=dy.device))
    base = pool_windows(addend, sz).float() if addend is not None else torch.zeros_like(sel)
    return pool_unwindow((base + sel).to(dy.dtype), sz)


def pool_r1_reference(dx, img, items, nw, grid):
    """dWsc[co] = sum_v img[v] dx[v][co] over the STORED dx (maxpool_bwd_kernel<.., R1>): a thread's grid-stride walk of fmaf - ceil(items /
    (grid 256)) windows of nw voxels, one rounding per fma -, five shuffle levels, the four waves in two additions, then
    bpxred::reduce_partials over the `grid` rows (at most grid + 3)."""
    C = dx.shape[-1]
    d, im = dx.double().reshape(-1, C), img.double().reshape(-1, 1)
    ref = (im * d).sum(0)
    M = (im.abs() * d.abs()).sum(0)
    chain = -(-items // (grid * 256)) * nw + 5 + 2 + grid + 3
    return ref, U32 * ref.abs() + (1 + U32) * chain * U32 * M


# ---- helpers shared by the CPU self-test and the GPU rows ------------------------------------------------------------------------------
def trunc_to(v, kind):
    """v (fp64) stored to a 16-bit type by TRUNCATION (towards zero) instead of round-to-nearest-even: a fault, for the CPU self-test."""
    r = v.to(CB.TORCH_DT[kind])
    over = r.double().abs() > v.abs()
    bits = r.view(torch.int16) - over.to(torch.int16)            # sign-magnitude: one step towards zero
    return bits.view(CB.TORCH_DT[kind]).double()


def same_bits(a, b):
    """Bit equality of two tensors of one dtype (NaN pre-fill included: an unwritten element differs)."""
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


def exact_row(name, got, ref):
    """A result row (conv_bounds.compare form) of a bit-for-bit comparison: err = the number of differing elements."""
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[ref.element_size()]
    ref = ref.to(got.device)
    bad = got.dtype != ref.dtype or got.shape != ref.shape
    n = -1 if bad else int((got.contiguous().view(it) != ref.contiguous().view(it)).sum().item())
    where = ""
    if n > 0:
        i = int(torch.nonzero((got.contiguous().view(it) != ref.contiguous().view(it)).reshape(-1))[0].item())
        where = f"first at flat index {i} of {tuple(ref.shape)}"
    return dict(name=name, err=float(n), tol=0.0, ok=n == 0, extra=where)


POOL_VALUES = {1: (-0.0, 0.0, 1.5), 2: (-0.0, 0.0, 1.5, -2.0)}      # at most three values for sz 1 (4-voxel windows), four for sz 2


def pool_inputs(B, S, C, sz, xdtype, gdtype, gen):
    """Pooling operands whose windows mostly hold ties: x drawn uniformly from POOL_VALUES[sz] (+0 / -0 among them), with the first window of
    every sample set to one value; dy and the addend randn rounded to the gradient type."""
    D, H, W = S
    vals = torch.tensor(POOL_VALUES[sz], dtype=torch.float32)
    x = vals[torch.randint(0, len(vals), (B, D, H, W, C), generator=gen)]
    x[:, :sz, :2, :2, :] = 1.5
    dy = torch.randn(B, D // sz, H // 2, W // 2, C, generator=gen).to(gdtype)
    add = torch.randn(B, D, H, W, C, generator=gen).to(gdtype)
    return x.to(xdtype), dy, add


def pool_tie_stats(x, sz):
    """(set of window positions that win somewhere, share of windows whose maximum is attained more than once)."""
    w = pool_windows(x, sz).double()
    am = pool_argmax(x, sz)
    tied = ((w == w.max(-2, keepdim=True).values).sum(-2) > 1).double().mean().item()
    return set(am.unique().tolist()), tied


# ---- GPU row tables (tests/test_norm_bounds_gpu.py runs them; tests/test_norm_bounds_cpu.py checks what they assume) --------------------------
# the streaming kernel pw_nbs_kernel<KC, TV, TT, WG>: (name, K, B, voxels per sample).  pws_ok admits >= 262144 voxels with vps % TV == 0
# (TV = 128 at K 16, 64 at K 32) over min(256, blocks) workgroups, so every workgroup walks at least 8 blocks: walks shorter than the
# four-stage ring (fewer than 3 blocks) cannot be reached through the C-ABI and no hook is added for them.
PWS_ROWS = [
    ("k16_B3_2049blocks", 16, 3, 87424),      # 683 blocks per sample: one workgroup walks 9 blocks, the rest 8; sample boundaries inside walks
    ("k16_B1_smallest", 16, 1, 262144),       # 2048 blocks: every walk 8
    ("k32_B5_4100blocks", 32, 5, 52480),      # 820 blocks per sample, 4100 = 16 x 256 + 4: four walks of 17; boundaries inside walks
    ("k32_B2_smallest", 32, 2, 131072),       # 4096 blocks: every walk 16
]


def pws_blocks(K, B, vps):
    tv = 128 if K == 16 else 64
    return (B * vps) // tv, vps // tv


# the tile kernel pw_kernel<T, MS, NS, PW_CONV1>: (name, modes, B, voxels, Cin, Ncols, split (0 = one output), bias, addend, planar t)
PW_ROWS = [
    ("ns1_v1", ("bf16", "f32", "mix16"), 2, 1, 16, 16, 0, False, False, False),
    ("ns2_v127_bias", ("bf16", "f32", "mix16"), 2, 127, 16, 32, 0, True, False, False),
    ("ns3_v128_split16_addend", ("bf16", "f32", "mix16"), 3, 128, 16, 48, 16, False, True, False),
    ("ns3_v129_split32_planar", ("bf16", "mix16"), 2, 129, 16, 48, 32, False, False, True),
    ("ns4_v4099_split48", ("bf16", "f32", "mix16"), 2, 4099, 32, 64, 48, False, False, False),
    ("ns3_k32_v4099_split64_planar", ("bf16", "mix16"), 1, 4099, 32, 96, 64, False, False, True),
    ("ns4_v129_split16_bias_addend", ("bf16", "f32"), 2, 129, 16, 64, 16, True, True, False),
]

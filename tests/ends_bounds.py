"""Element-wise error bounds for the kernels at the two ENDS of a network - the dropout pair (bpx_norm_act_dropout_fwd / _bwd) of
biapy_amd/csrc/elementwise.hip, the output head (bpx_head_fwd / _bwd) and the first layer's weight gradients (bpx_conv3d_c1_wgrad, _nb,
bpx_conv1x1_c1_wgrad) of ends.hip - in the form of tests/conv_bounds.py, tests/norm_bounds.py and tests/gate_bounds.py, whose comparator, rounding helpers,
activation terms and partial-sum bound are reused:

    |got - ref| <= u_out |ref| + (1 + u_out) (E + K 2^-24 M) + floor          (conv_bounds.finish)

``ref`` is the operation in float64 on the operands as stored, ``M`` the sum of the absolute terms, ``K`` the number of fp32 roundings a term
passes through, ``E`` the error of operands formed on the device pushed through on absolute values.  Every chain length is read off the kernel
and stated where the bound is built.  The dropout mask is a function of integers: it is compared bit for bit with a host Philox4x32-10.

Nothing here is fitted to a measured value.  NaN / inf fails (conv_bounds.compare), outputs are pre-filled with NaN by the callers, and no
element is left out of a comparison.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import norm_bounds as NB
from augment_ref import philox4x32_10
from conv_bounds import ACT_ABS, ACT_REL, U32, UNIT, act64, compare, finish, round_to  # noqa: F401
from norm_bounds import MODES, exact_row, same_bits, sums_reference  # noqa: F401

ALL = ("f32", "bf16", "f16")
BWD_MODES = ("f32", "bf16", "mix16")
ACT_LAST = 8                # BPX_ACT_LAST
NA_BLOCKS = 512             # elementwise.hip: blocks (= partial rows) per sample of the norm + activation kernels, upper bound
WG_ROWS = 1024              # workgroup columns (= partial rows) of the head backward, the scalar first-layer kernel and the rank-1 kernel, upper bound
C1_MFMA_WGS = 768           # persistent workgroups of conv_c1_wgrad_mfma_kernel, upper bound
F32_TINY = 2.0 ** -125      # below the smallest normal fp32 an expf result may be flushed
EXACT = 2.0 ** -1000        # the bound of an element that must equal its reference: below every non-zero difference of two fp32 values


def cdiv(a, b):
    return -(-a // b)


def kpl(kind):
    return 4 if kind == "f32" else 8


def drop_tiles(voxels, C, kind):
    """na_blocks of elementwise.hip (what bpx_norm_act_dropout_tiles answers): min(ceil(voxels G / 256), 512) rounded up to a multiple of G's
    odd part."""
    G = C // kpl(kind)
    odd = G
    while odd % 2 == 0 and odd > 1:
        odd //= 2
    return cdiv(min(cdiv(voxels * G, 256), NA_BLOCKS), odd) * odd


# ---- the dropout mask -----------------------------------------------------------------------------------------------------------------------
def drop_threshold(p):
    """drop_args: thr = (uint32) min(2^32 - 1, (double)p 2^32) with p a float."""
    return int(min(4294967295.0, float(np.float32(p)) * 4294967296.0))


def drop_inv(p):
    """`1.f / (1.f - d.p)`: the fp32 difference and the fp32 quotient, as a Python float."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def dropout_keep(seed, counter, site, p, n_elements, elements=None):
    """keep[e] of drop_keep: Philox4x32-10 with key (lo32(seed), hi32(seed)) at counter (lo32(b), hi32(b), site, lo32(ctr) ^ (hi32(ctr)
    0x9E3779B9 mod 2^32)) for the block b = e >> 2, word e & 3, kept where the word >= thr.  e is the linear index into the dense (N, voxels, C)
    tensor, sample offset included.  Returns a bool array over e = 0 .. n_elements - 1, or over `elements` (any uint64 indices) if given."""
    e = np.arange(n_elements, dtype=np.uint64) if elements is None else np.asarray(elements, dtype=np.uint64)
    seed, counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    c3 = (counter & 0xFFFFFFFF) ^ (((counter >> 32) * 0x9E3779B9) & 0xFFFFFFFF)
    if elements is None:                                     # one Philox call per block of four elements
        b = np.arange(cdiv(n_elements, 4), dtype=np.uint64)
    else:
        b = e >> np.uint64(2)
    r = philox4x32_10(b & np.uint64(0xFFFFFFFF), b >> np.uint64(32), site & 0xFFFFFFFF, c3, seed & 0xFFFFFFFF, seed >> 32)
    r = np.stack(r, -1)
    word = r.reshape(-1)[:n_elements] if elements is None else r[np.arange(len(e)), (e & np.uint64(3)).astype(np.int64)]
    return word >= np.uint32(drop_threshold(p))


def keep_tensor(seed, counter, site, p, shape):
    """dropout_keep over a dense (N, voxels, C) tensor as a torch bool tensor."""
    n = int(np.prod(shape))
    return torch.from_numpy(dropout_keep(seed, counter, site, p, n)).reshape(shape)


# ---- dropout forward / backward ---------------------------------------------------------------------------------------------------------------
def dropout_fwd_reference(x, rec, act, kind, p, keep, inv=None):
    """norm_act_drop_fwd_kernel: y = keep ? act(scale x + shift) inv : 0 on the stored x (N, V, C), the fp32 records and inv = the fp32
    quotient 1 / (1 - p).  The activation carries the terms of norm_bounds.norm_act_fwd_reference (E, scaled by inv); `bpx_act_rt(u) * inv` is
    one more fp32 rounding, and one is allowed for the quotient itself (correctly rounded under the build's flags, within 1 ulp otherwise):
    K = 2 over |act| inv.  A dropped element is exactly 0: its bound is EXACT, which only got == 0 meets.  Returns (ref, bound)."""
    inv = drop_inv(p) if inv is None else inv
    sx, sh, u, _ = NB._act_terms(x, rec)
    y = act64(u, act)
    E = U32 * (ACT_REL * y.abs() + ACT_ABS + NB.ACT_U * (sx.abs() + sh.abs()) + NB.ACT_LIP * (sx.abs() + u.abs()))
    k = keep.to(x.device)
    ref = torch.where(k, y * inv, torch.zeros_like(y))
    return ref, torch.where(k, finish(ref, ref.abs(), E * inv, 2, kind), torch.zeros_like(ref)) + EXACT


def dropout_bwd_reference(dy, x, rec, act, mode, p, keep, tiles, inv=None):
    """norm_act_drop_bwd_kernel: g = keep ? dy inv act'(u) : 0, and the S1 = sum g, S2 = sum g xhat rows.  `dv[e] * inv * act'(u)`: two
    products (2 roundings) and the quotient's own (see dropout_fwd_reference): K = 3; act'(u) formed in fp32 carries the element error of
    norm_bounds.norm_act_bwd_reference (ed, here recovered from its egv with dy inv in place of dy).  The rows: the thread mapping and the LDS
    sum are norm_act_bwd_kernel's, so the chain is norm_bounds.norm_act_bwd_chain and the bound norm_bounds.red_reference.
    Returns (g, bound of the stored g, sums (N, 2, C), bound of the sums)."""
    gk = MODES[mode][0]
    inv = drop_inv(p) if inv is None else inv
    k = keep.to(x.device)
    dyi = torch.where(k, dy * inv, torch.zeros_like(dy))
    g, _, _, egv = NB.norm_act_bwd_reference(dyi, x, rec, act, None, gk)     # egv = |dy inv| ed + 2^-24 |g|
    eg = egv + 2 * U32 * g.abs()                                              # three roundings instead of one
    bound = torch.where(k, finish(g, g.abs(), egv - U32 * g.abs(), 3, gk), torch.zeros_like(g)) + EXACT      # a dropped element, or dy = 0: exactly 0
    N, V, C = x.shape
    s, sb = NB.red_reference(g, eg, x, rec, NB.norm_act_bwd_chain(V, C, gk, tiles))
    return g, bound, s, sb + EXACT                            # (a column whose every element is dropped sums to exactly 0)


# ---- the output head ----------------------------------------------------------------------------------------------------------------------
def head_code(codes):
    """One 4-bit code per output channel, channel 0 in the low nibble (0 linear, 1 sigmoid, 2 tanh, 3 softmax)."""
    v = 0
    for i, c in enumerate(codes):
        v |= c << (4 * i)
    return v


def softmax_groups(codes):
    """[(first, last)] of the runs of consecutive softmax channels."""
    out, i = [], 0
    while i < len(codes):
        if codes[i] == 3:
            j = i
            while j + 1 < len(codes) and codes[j + 1] == 3:
                j += 1
            out.append((i, j))
            i = j + 1
        else:
            i += 1
    return out


HEAD_CODE_SETS = ("linear", "sigmoid", "tanh", "softmax", "mixed", "two_groups", "single_group")


def head_codes(name, Cout):
    """The code lists of the GPU rows.  mixed: [sigmoid, softmax, softmax, tanh, ...] repeated; two_groups: softmax groups split by one linear
    channel (at Cout 1, 2 there is room for one group only); single_group: channel 0 a softmax group of its own, the rest linear."""
    if name in ("linear", "sigmoid", "tanh", "softmax"):
        return [("linear", "sigmoid", "tanh", "softmax").index(name)] * Cout
    if name == "mixed":
        return ([1, 3, 3, 2] * 2)[:Cout]
    if name == "two_groups":
        h = max(1, (Cout - 1) // 2)
        return ([3] * h + [0] + [3] * Cout)[:Cout]
    return ([3, 0] + [3] * Cout)[:Cout] if name == "single_group" else None


def head_fwd_reference(x, w, b, codes):
    """head_fwd_kernel on the stored x (N, V, Cin), the fp32 w (Cout, Cin) and b (Cout,) or None: the logit `a = b; a = fmaf(f[c], w[c], a)`
    is a chain of Cin fmas on the bias - K = Cin over M = |b| + sum |x||w| - and stays as it is for code 0.  The activations, with the figures
    conv_bounds takes for its own fp32 activations (ACT_REL = 8 ulps of the result plus ACT_ABS = 8 ulps absolute for expf / tanhf and the
    divisions behind them; conv_bounds' module docstring), the logit error E_a pushed through by the Lipschitz constant:
    - sigmoid `1.f / (1.f + expf(-a))`: slope <= 1/4:  E_a / 4 + 2^-24 (ACT_REL s + ACT_ABS);
    - `tanhf(a)`: slope <= 1:  E_a + 2^-24 (ACT_REL |t| + ACT_ABS);
    - softmax over a group of L channels: m = max (exact), d = a - m (one rounding, and the two logit errors E_k + max E), e = expf(d) (relative
      ACT_REL 2^-24 + expm1 of the error of d; flushed below the smallest normal: F32_TINY), ssum a chain of L additions, one division:
      |dp_k| <= p_k (r_k + max_j r_j + (L + 1) 2^-24) + F32_TINY.  A group of one channel is expf(0) / (0 + 1) = exactly 1: bound EXACT there.
    Returns (ref (N, Cout, V), bound, logit bound)."""
    Cin = x.shape[-1]
    W = w.double().to(x.device)
    a = x @ W.t()
    M = x.abs() @ W.abs().t()
    if b is not None:
        a, M = a + b.double().to(x.device), M + b.double().abs().to(x.device)
    ea = Cin * U32 * M
    ref, E = a.clone(), ea.clone()
    for co, code in enumerate(codes):
        if code == 1:
            ref[..., co] = torch.sigmoid(a[..., co])
            E[..., co] = 0.25 * ea[..., co] + U32 * (ACT_REL * ref[..., co] + ACT_ABS)
        elif code == 2:
            ref[..., co] = torch.tanh(a[..., co])
            E[..., co] = ea[..., co] + U32 * (ACT_REL * ref[..., co].abs() + ACT_ABS)
    for lo, hi in softmax_groups(codes):
        L = hi - lo + 1
        g, eg = a[..., lo:hi + 1], ea[..., lo:hi + 1]
        p = torch.softmax(g, -1)
        ref[..., lo:hi + 1] = p
        if L == 1:
            continue
        d = g - g.max(-1, keepdim=True).values
        r = ACT_REL * U32 + torch.expm1(U32 * d.abs() + eg + eg.max(-1, keepdim=True).values)
        E[..., lo:hi + 1] = p * (r + r.max(-1, keepdim=True).values + (L + 1) * U32) + F32_TINY
    lin = torch.tensor([c == 0 for c in codes], device=x.device)
    bound = torch.where(lin, finish(ref, M, 0.0, Cin, "f32"), finish(ref, 0.0, E, 0, "f32"))
    for lo, hi in softmax_groups(codes):
        if lo == hi:
            bound[..., lo] = EXACT
    return ref.transpose(1, 2), bound.transpose(1, 2), ea.transpose(1, 2)


def softmax_sum_bound(L):
    """|sum_k p_k - 1| of one softmax group as the kernel forms it: ssum differs from the exact sum of the e_k by its chain of L additions,
    each quotient rounds once - (L + 1) 2^-24 to first order, and the second-order factor."""
    return (L + 1) * U32 * (1 + (L + 1) * U32)


def head_bwd_blocks(total, Cout, Cin):
    """bpx_head_bwd: min(ceil(total / 256), 1024) workgroup columns, rounded up to a multiple of 8 for the sliced kernel (Cout > 4 at Cin 32)."""
    blocks = min(cdiv(total, 256), WG_ROWS)
    return (blocks + 7) & ~7 if Cout > 4 and Cin > 16 else blocks


def rows_chain(total, rows):
    """The chain shared by the voxel sums of head_bwd_kernel, head_bwd_slice_kernel and rank1_wgrad_kernel: the thread's grid-stride walk of
    fmas, ceil(total / (rows 256)); the wave butterfly (__shfl_xor over 1 .. 32: 6 levels); `red[0] + red[1] + red[2] + red[3]`: 3; and the row
    combination of bpxred::reduce_partials (wgrad_reduce_block in wgrad.hip: a lane sums every GL-th row in four interleaved accumulators,
    (s0 + s1) + (s2 + s3), then the GL lanes in sequence: at most rows + 3, as norm_bounds has it)."""
    return cdiv(total, rows * 256) + 6 + 3 + rows + 3


def head_bwd_reference(x, w, dout, mode, db_init):
    """head_bwd_kernel / head_bwd_slice_kernel on the stored x (N, V, Cin), the fp32 w (Cout, Cin) and the fp32 dout (N, Cout, V):
    - dx[v][ci] = sum_co dout[co][v] w[co][ci]: `o[c] = fmaf(d, ws[..], o[c])`, a chain of Cout fmas, then the store of the dx type;
    - dW[co][ci] = sum_v dout[co][v] x[v][ci] and db[co] = sum_v dout[co][v]: rows_chain; db is ADDED to db_init (`j.db[..] += s`: one more
      rounding, the initial value among the terms).
    Returns {name: (ref, bound)} for dx (N, V, Cin), dw (Cout, Cin), db (Cout,) (None without db_init)."""
    gk = MODES[mode][0]
    N, V, Cin = x.shape
    Cout = w.shape[0]
    W = w.double().to(x.device)
    dt = dout.double().transpose(1, 2)                       # (N, V, Cout)
    dx = dt @ W
    out = dict(dx=(dx, finish(dx, dt.abs() @ W.abs(), 0.0, Cout, gk)))
    chain = rows_chain(N * V, head_bwd_blocks(N * V, Cout, Cin))
    d2, x2 = dt.reshape(N * V, Cout), x.reshape(N * V, Cin)
    dw = d2.t() @ x2
    out["dw"] = (dw, finish(dw, d2.abs().t() @ x2.abs(), 0.0, chain, "f32"))
    out["db"] = None
    if db_init is not None:
        i = db_init.double().to(x.device)
        db = i + d2.sum(0)
        out["db"] = (db, finish(db, i.abs() + d2.abs().sum(0), 0.0, chain + 1, "f32"))
    return out


# ---- the first layer's weight gradients -----------------------------------------------------------------------------------------------------
def c1_plan(kernel, N, D, H, W, persist=0):
    """(tile extents (tz, ty, tx), tiles, workgroup columns = partial rows) of c1_wgrad_impl (ends.hip): N C1ScalarTile::tiles(D, H, W) over
    min(tiles, 1024) columns, or N C1MfmaTile::tiles(D, H, W) over min(tiles, 768, bpx_debug_set_c1_persist's cap) persistent workgroups."""
    t = (4, 8, 8) if kernel == "scalar" else (4, 4, 16)        # C1ScalarTile, C1MfmaTile
    tiles = N * cdiv(D, t[0]) * cdiv(H, t[1]) * cdiv(W, t[2])
    rows = min(tiles, WG_ROWS) if kernel == "scalar" else min(tiles, C1_MFMA_WGS, persist if persist > 0 else tiles)
    return t, tiles, rows


def c1_chain(kernel, tiles, rows):
    """Longest fp32 chain of one dW element.
    conv_c1_wgrad_kernel: thread (tap, sub) takes the voxels sub, sub + 9, .. of a 256-voxel tile, ceil(256 / 9) = 29 fmas per tile over the
    ceil(tiles / rows) tiles of its workgroup; `s += sred[q][t][c]` over the 9 subs; the row combination (rows + 3).
    conv_c1_wgrad_mfma_kernel: a wave owns two of a tile's eight 32-voxel K-chunks and issues the hi and the lo MFMA on each - 4 MFMAs of 32
    products (at most one rounding per product, as norm_bounds.pws_wgrad_reference counts an MFMA step) per tile; the four waves `sred[0] + .. +
    sred[3]`: 3; the row combination.  db is the same sum through the ones row (MFMA) or `bs += d` (scalar) and is ADDED to the buffer: + 1."""
    per = 29 if kernel == "scalar" else 4 * 32
    mid = 9 if kernel == "scalar" else 3
    return per * cdiv(tiles, rows) + mid + rows + 3


IMG_SPLIT = UNIT["bf16"] ** 2        # |img - hi - lo| <= u_bf16 |img - hi| <= u_bf16^2 |img|: the bound of the f16 split in test_c1_fwd_f16_elementwise


def c1_tap_terms(img, shift_tap=None):
    """The 27 shifted views (zero padding 1) of img (N, D, H, W): yields (tap, the image at voxel + tap as (V,), V the voxels in dy's order).
    shift_tap: that tap reads one voxel further along x - a fault, for the CPU self-test."""
    N, D, H, W = img.shape
    ip = F.pad(img, (2, 2, 1, 1, 1, 1))
    for tap in range(27):
        kz, ky, kx = tap // 9, (tap // 3) % 3, tap % 3
        o = 1 + (1 if tap == shift_tap else 0)
        yield tap, ip[:, kz:kz + D, ky:ky + H, kx + o:kx + o + W].reshape(-1)


def c1_wgrad_reference(img, dy, kernel, rows_info, db_init, edy=None):
    """dW[co][tap] = sum_v img[v + tap] dy[v][co] with zero padding and db = db_init + sum_v dy of the fp32 img (N, D, H, W) and dy (N, D, H, W,
    Cout) float64.  Scalar kernel: the operands are exact in fp32 and every fma rounds once - only the chain.  MFMA kernel: the image enters as
    hi + lo bf16 parts, relative operand error IMG_SPLIT, carried as E = IMG_SPLIT sum |img||dy|.  edy: the element bound of a dy formed on the
    device (the _nb entry; dy is then the UNROUNDED fp64 value) - E += sum (1 + IMG_SPLIT) |img| edy, and for db sum edy.
    rows_info = (tiles, rows) of c1_plan.  Returns {dw: (ref (Cout, 27), bound), db: (ref, bound) or None}."""
    Cout = dy.shape[-1]
    g = dy.reshape(-1, Cout)
    ga = g.abs()
    chain = c1_chain(kernel, *rows_info)
    split = IMG_SPLIT if kernel == "mfma" else 0.0
    ref = torch.zeros(Cout, 27, dtype=torch.float64, device=img.device)
    M, E = torch.zeros_like(ref), torch.zeros_like(ref)
    e2 = None if edy is None else edy.reshape(-1, Cout)
    for tap, iv in c1_tap_terms(img):
        ref[:, tap] = iv @ g
        M[:, tap] = iv.abs() @ ga
        E[:, tap] = split * M[:, tap]
        if e2 is not None:
            E[:, tap] += (1 + split) * (iv.abs() @ e2)
            M[:, tap] += iv.abs() @ e2
    out = dict(dw=(ref, finish(ref, M, E, chain, "f32") + EXACT), db=None)      # (D = 1: the taps above and below the plane see padding only - exactly 0)
    if db_init is not None:
        i = db_init.double().to(img.device)
        db = i + g.sum(0)
        Eb = 0.0 if e2 is None else e2.sum(0)
        out["db"] = (db, finish(db, i.abs() + ga.sum(0) + Eb, Eb, chain + 1, "f32"))
    return out


def rank1_rows(total):
    return min(cdiv(total, 256), WG_ROWS)


def rank1_reference(img, dy):
    """rank1_wgrad_kernel: dW[co] = sum_v img[v] dy[v][co] of the fp32 img (V,) and the stored dy (V, Cout): `acc[c] = fmaf(iv, f[c], acc[c])`
    over the thread's walk - the four-in-flight loop and the tail add in the same order -, then rows_chain's shuffles, waves and rows."""
    ref = img @ dy
    return ref, finish(ref, img.abs() @ dy.abs(), 0.0, rows_chain(img.shape[0], rank1_rows(img.shape[0])), "f32")


def rank1_loops(total):
    """(threads that take at least one four-in-flight iteration, threads that take a tail iteration after one) of rank1_wgrad_kernel."""
    stride = rank1_rows(total) * 256
    four = max(0, min(stride, total - 3 * stride))
    both = 0
    if four:
        v = np.arange(four, dtype=np.int64)
        it = (total - 3 * stride - v + 4 * stride - 1) // (4 * stride)
        both = int(((v + it * 4 * stride) < total).sum())
    return four, both


# ---- GPU row tables (tests/test_ends_bounds_gpu.py runs them; tests/test_ends_bounds_cpu.py checks that they reach what they name) ----------------
# dropout: (name, N, voxels, C, activation codes).  Every code on the first shape, ELU and one other on the rest.
DROP_ROWS = [
    ("partly_filled_block", 2, 77, 16, tuple(range(ACT_LAST + 1))),
    ("odd3_c48", 3, 1031, 48, (1, 3)),
    ("odd5_c80", 1, 4099, 80, (1, 2)),
    ("grid_wrap_c16", 2, 70001, 16, (1, 5)),
    ("G512_c2048", 1, 5, 2048, (1, 8)),
]
DROP_P, DROP_SEED, DROP_SITE = 0.3, 0x123456789ABCDEF, 5
DROP_COUNTERS = (0, 1, 2 ** 32 + 1)

HEAD_N, HEAD_VPS = 3, 1031
HEAD_FWD_WRAP = [(1, 32), (4, 16)]                 # (Cout, Cin) at N 3, vps 350003: past grid_for's 4096 x 256 threads
HEAD_FWD_WRAP_SHAPE = (3, 350003)
HEAD_BWD_WRAP = [(1, 32), (4, 32), (5, 32), (8, 16)]
HEAD_BWD_WRAP_SHAPE = (2, 140001)                  # past 1024 x 256 threads

# first layer: (N, D, H, W, Cout)
C1_SCALAR_ROWS = [((2, 5, 9, 8, 16), ("f32", "bf16")), ((1, 1, 8, 8, 16), ("f32", "bf16")), ((1, 1, 17, 7, 32), ("f32", "bf16")),
                  ((2, 6, 10, 19, 32), ("f32",)), ((1, 8, 64, 520, 16), ("f32",))]
C1_MFMA_ROWS = [((3, 4, 4, 9, 16), 0), ((2, 6, 10, 19, 32), 0), ((1, 1, 17, 19, 16), 0), ((3, 8, 12, 40, 16), 5)]       # (shape, workgroup cap)
RANK1_TOTALS = (1, 255, 3072, 262144 + 77, 4 * 262144 + 1000)

"""The bounds of tests/ends_bounds.py on the CPU: the fp64 references agree with torch autograd in float64, the host dropout mask agrees with a
scalar re-statement of Philox4x32-10 (an element index >= 2^34 and a step counter >= 2^32 among the probes) and keeps the right share, an fp32
emulation of each kernel's arithmetic (operation order, fp32 accumulators, the storage rounding of the kind) passes its bound at the shapes of
tests/test_ends_bounds_gpu.py - reduced where an fp64 pass over the GPU shape would take more than a second - and six seeded defects fail.
The worst |err| / bound of every emulation is recorded, not asserted.  No GPU: the host checks return before any launch."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_bounds as CB
import ends_bounds as EB
import norm_bounds as NB
from test_conv_bounds_gpu import _record_diag

NAN = float("nan")


def _f32(v):
    return v.float().double()


def _fma(a, b, c):
    """fmaf on fp32 tensors: the exact product (48 bits) and the sum in fp64, rounded to fp32."""
    return (a.double() * b.double() + c.double()).float()


def _rec(rows, tag):
    worst = max(r["err"] for r in rows)
    _record_diag(f"ends_bounds_cpu[{tag}] emulation worst err/bound = {worst:.3e}")
    bad = [r for r in rows if not r["ok"]]
    assert not bad, bad
    return worst


def _fails(row):
    return not row["ok"]


# ---- the mask --------------------------------------------------------------------------------------------------------------------------------
def _philox_scalar(c, k):
    """Philox4x32-10 on Python integers (Salmon et al., SC'11): counter words c[0..3], key words k[0..1]."""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def _keep_scalar(seed, ctr, site, p, e):
    b = e >> 2
    c3 = (ctr & 0xFFFFFFFF) ^ (((ctr >> 32) * 0x9E3779B9) & 0xFFFFFFFF)
    r = _philox_scalar([b & 0xFFFFFFFF, b >> 32, site, c3], [seed & 0xFFFFFFFF, seed >> 32])
    thr = min(2 ** 32 - 1, math.floor(float(np.float32(p)) * 2.0 ** 32))
    return r[e & 3] >= thr


def test_dropout_keep_equals_the_scalar_restatement():
    els = [0, 1, 3, 4, 7, 1030, 2 ** 32 - 1, 2 ** 32, 2 ** 34 + 5, 2 ** 40 + 2]
    for seed, ctr, site, p in ((EB.DROP_SEED, 0, 5, 0.3), (7, 1, 0, 0.5), (2 ** 63 + 11, 2 ** 32 + 1, 77, 0.9), (1, 2 ** 32, 3, 0.05), (5, 1, 3, 0.05)):
        got = EB.dropout_keep(seed, ctr, site, p, 0, elements=els)
        assert got.tolist() == [_keep_scalar(seed, ctr, site, p, e) for e in els], (seed, ctr, site, p)
        dense = EB.dropout_keep(seed, ctr, site, p, 1031)
        assert dense.tolist() == [_keep_scalar(seed, ctr, site, p, e) for e in range(1031)]
    # the high words matter: c1 (block index >= 2^32) and the high half of the counter
    a = EB.dropout_keep(3, 0, 0, 0.5, 0, elements=np.arange(4096, dtype=np.uint64) + np.uint64(2 ** 34))
    assert not np.array_equal(a, EB.dropout_keep(3, 0, 0, 0.5, 4096))
    assert not np.array_equal(EB.dropout_keep(3, 1, 0, 0.5, 4096), EB.dropout_keep(3, 2 ** 32 + 1, 0, 0.5, 4096))
    assert EB.drop_threshold(0.0) == 0 and EB.dropout_keep(3, 1, 0, 0.0, 4096).all()
    assert EB.drop_threshold(0.999) == math.floor(float(np.float32(0.999)) * 2.0 ** 32) and EB.drop_inv(0.0) == 1.0


@pytest.mark.parametrize("p", [0.05, 0.1, 0.5, 0.9])
def test_keep_rate_within_five_sigmas(p):
    n = 2 ** 20
    kept = int(EB.dropout_keep(EB.DROP_SEED, 1, EB.DROP_SITE, p, n).sum())
    q = 1.0 - EB.drop_threshold(p) / 2.0 ** 32
    assert abs(kept - n * q) <= 5 * math.sqrt(n * q * (1 - q)), (p, kept / n)


# ---- dropout ---------------------------------------------------------------------------------------------------------------------------------
def drop_operands(N, V, C, act, xk, gk, seed=0):
    gen = torch.Generator().manual_seed(1000 * seed + V + C + act)
    x = CB.round_to(torch.randn(N, V, C, generator=gen), xk)
    dy = CB.round_to(torch.randn(N, V, C, generator=gen), gk)
    return x, dy, CB.norm_recs(N, C, gen)


def _u32(x, rec):
    sc, sh = rec[:, None, :, 2], rec[:, None, :, 3]
    return sc * x.float() + sh                                # `sc[e] * f[e] + sh[e]`: a product and a sum in fp32 (contraction is off)


def drop_fwd_emu(x, rec, act, kind, keep, inv):
    a = CB.act64(_u32(x, rec), act) * torch.tensor(inv, dtype=torch.float32)
    return CB.round_to(torch.where(keep, a, torch.zeros_like(a)), kind)


def drop_bwd_emu(dy, x, rec, act, mode, keep, inv, tiles):
    """g and the partial rows of norm_act_drop_bwd_kernel: item i = voxel G + channel group belongs to thread i mod (tiles 256), block = thread /
    256; the terms are fp32 values, each row is summed exactly and rounded to fp32 once (as test_gate_bounds_cpu.dot_rows_sim does)."""
    gk = EB.MODES[mode][0]
    N, V, C = x.shape
    k = EB.kpl(gk)
    G = C // k
    da = CB.dact64(_u32(x, rec), act)
    gv = dy.float() * torch.tensor(inv, dtype=torch.float32) * da
    gv = torch.where(keep, gv, torch.zeros_like(gv))
    xh = (x.float() - rec[:, None, :, 0]) * rec[:, None, :, 1]
    i = torch.arange(V * G)
    slot = ((i % (tiles * 256)) // 256) * G + i % G
    rows = []
    for t in (gv, gv * xh):
        r = torch.zeros(N, tiles * G, k, dtype=torch.float64).index_add_(1, slot, t.double().reshape(N, V * G, k))
        rows.append(_f32(r.reshape(N, tiles, C)))
    return CB.round_to(gv, gk), torch.stack(rows, 2)


DROP_CASES = [(r, a) for r in EB.DROP_ROWS for a in r[4]]


@pytest.mark.parametrize("row,act", DROP_CASES, ids=[f"{r[0]}-act{a}" for r, a in DROP_CASES])
def test_dropout_emulation_passes_and_defects_fail(row, act):
    name, N, V, C, _ = row
    p, inv = EB.DROP_P, EB.drop_inv(EB.DROP_P)
    keep = EB.keep_tensor(EB.DROP_SEED, 1, EB.DROP_SITE, p, (N, V, C))
    rows = []
    for kind in EB.ALL:
        x, _, rec = drop_operands(N, V, C, act, kind, kind)
        ref, bound = EB.dropout_fwd_reference(x, rec, act, kind, p, keep)
        rows.append(EB.compare(f"fwd {kind}", drop_fwd_emu(x, rec, act, kind, keep, inv), ref, bound, axes="nvc"))
        if kind == "bf16" and act == 1:
            shifted = keep.reshape(-1).roll(1).reshape(keep.shape)
            assert _fails(EB.compare("mask shifted by one element", drop_fwd_emu(x, rec, act, kind, shifted, inv), ref, bound, axes="nvc"))
            if N > 1:
                nooff = keep[:1].expand_as(keep)
                assert not torch.equal(nooff, keep)
                assert _fails(EB.compare("mask without the sample offset", drop_fwd_emu(x, rec, act, kind, nooff, inv), ref, bound, axes="nvc"))
            assert _fails(EB.compare("inv = 1", drop_fwd_emu(x, rec, act, kind, keep, 1.0), ref, bound, axes="nvc"))
            bad = drop_fwd_emu(x, rec, act, kind, keep, inv)
            bad[-1, -1, -1] = NAN
            assert _fails(EB.compare("unwritten", bad, ref, bound, axes="nvc"))
    for mode in EB.BWD_MODES:
        gk, xk = EB.MODES[mode]
        x, dy, rec = drop_operands(N, V, C, act, xk, gk)
        tiles = EB.drop_tiles(V, C, gk)
        g, bound, s, sb = EB.dropout_bwd_reference(dy, x, rec, act, mode, p, keep, tiles)
        ge, part = drop_bwd_emu(dy, x, rec, act, mode, keep, inv, tiles)
        rows += [EB.compare(f"bwd {mode} g", ge, g, bound, axes="nvc"), EB.compare(f"bwd {mode} sums", part.sum(1), s, sb, axes="nkc")]
        if mode == "f32" and act == 1:
            g1, p1 = drop_bwd_emu(dy, x, rec, act, mode, keep, 1.0, tiles)
            assert _fails(EB.compare("inv = 1 in g", g1, g, bound, axes="nvc")) and _fails(EB.compare("inv = 1 in the sums", p1.sum(1), s, sb, axes="nkc"))
            if tiles > 1:
                lost = part.clone()
                lost[:, tiles // 2] = 0
                assert _fails(EB.compare("a partial row lost", lost.sum(1), s, sb, axes="nkc"))
    _rec(rows, f"dropout {name} act{act}")


def test_dropout_reference_is_autograd():
    N, V, C, p = 2, 50, 16, 0.3
    inv = EB.drop_inv(p)
    keep = EB.keep_tensor(3, 1, 2, p, (N, V, C))
    for act in range(EB.ACT_LAST + 1):
        x, dy, rec = drop_operands(N, V, C, act, "f32", "f32")
        u = (x * rec.double()[:, None, :, 2] + rec.double()[:, None, :, 3]).requires_grad_(True)
        y = F.dropout(CB.act64(u, act), 0.0) * keep * inv                      # F.dropout's semantics with the mask made explicit: kept / (1 - p)
        (y * dy).sum().backward()
        ref, _ = EB.dropout_fwd_reference(x, rec, act, "f32", p, keep)
        g, _, s, _ = EB.dropout_bwd_reference(dy, x, rec, act, "f32", p, keep, 1)
        assert torch.allclose(ref, y.detach(), rtol=1e-13, atol=1e-13) and torch.allclose(g, u.grad, rtol=1e-13, atol=1e-13)
        xh = (x - rec.double()[:, None, :, 0]) * rec.double()[:, None, :, 1]
        assert torch.allclose(s, torch.stack([u.grad.sum(1), (u.grad * xh).sum(1)], 1), rtol=1e-12, atol=1e-12)
    z = torch.randn(4, 8, dtype=torch.float64)
    torch.manual_seed(0)
    d = F.dropout(z, p)
    assert torch.allclose(d[d != 0], (z / (1 - p))[d != 0])                    # what "kept / (1 - p), else 0" restates


# ---- the head --------------------------------------------------------------------------------------------------------------------------------
def head_operands(N, V, Cin, Cout, kind, scale=1.0, seed=0):
    gen = torch.Generator().manual_seed(seed + 100 * Cout + Cin)
    x = CB.round_to(scale * torch.randn(N, V, Cin, generator=gen), kind)
    w = (scale * torch.randn(Cout, Cin, generator=gen) / Cin ** 0.5).float()
    b = (0.3 * torch.randn(Cout, generator=gen)).float()
    dout = torch.randn(N, Cout, V, generator=gen).float()
    return x, w, b, dout


def head_fwd_emu(x, w, b, codes, drop_last=False):
    """head_fwd_kernel in fp32: the fma chain on the bias, then the activations channel by channel in the kernel's order.  drop_last: a softmax
    group's sum omits its last channel - a fault."""
    f = x.float()
    Cout, Cin = w.shape
    a = (b if b is not None else torch.zeros(Cout))[None, None, :].expand(*f.shape[:2], Cout).contiguous()
    for c in range(Cin):
        a = _fma(f[..., c:c + 1], w[None, None, :, c], a)
    one = torch.ones((), dtype=torch.float32)
    for co, code in enumerate(codes):
        if code == 1:
            a[..., co] = one / (one + torch.exp(-a[..., co]))
        elif code == 2:
            a[..., co] = torch.tanh(a[..., co])
    for lo, hi in EB.softmax_groups(codes):
        e = torch.exp(a[..., lo:hi + 1] - a[..., lo:hi + 1].max(-1, keepdim=True).values)
        s = torch.zeros_like(e[..., 0])
        for k in range(hi - lo + 1 - (1 if drop_last and hi > lo else 0)):
            s = s + e[..., k]
        a[..., lo:hi + 1] = e / s[..., None]
    return a.transpose(1, 2)


def head_bwd_emu(x, w, dout, mode, db_init, omit_last_row=False):
    gk = EB.MODES[mode][0]
    N, V, Cin = x.shape
    Cout = w.shape[0]
    d = dout.transpose(1, 2).contiguous()
    o = torch.zeros(N, V, Cin)
    for co in range(Cout):
        o = _fma(d[..., co:co + 1], w[co][None, None, :], o)
    blocks = EB.head_bwd_blocks(N * V, Cout, Cin)
    i = torch.arange(N * V)
    slot = (i % (blocks * 256)) // 256
    d2, x2 = d.reshape(N * V, Cout).double(), x.reshape(N * V, Cin)
    terms = (d2[:, :, None] * x2[:, None, :]).reshape(N * V, Cout * Cin)
    rw = _f32(torch.zeros(blocks, Cout * Cin, dtype=torch.float64).index_add_(0, slot, terms)).float()
    rb = _f32(torch.zeros(blocks, Cout, dtype=torch.float64).index_add_(0, slot, d2)).float()
    last = min(blocks, EB.cdiv(N * V, 256)) - 1                # the last row that holds voxels (the sliced kernel's grid may end in empty columns)
    dw, db = torch.zeros(Cout * Cin), torch.zeros(Cout)
    for r in range(blocks):
        if not (omit_last_row and r == last):
            dw, db = dw + rw[r], db + rb[r]
    return CB.round_to(o, gk), dw.reshape(Cout, Cin), None if db_init is None else db_init + db


HEAD_SHAPES = [(co, ci) for co in range(1, 9) for ci in (16, 32)]


@pytest.mark.parametrize("Cout,Cin", HEAD_SHAPES)
def test_head_emulation_passes_and_defects_fail(Cout, Cin):
    N, V = EB.HEAD_N, EB.HEAD_VPS
    rows = []
    for kind in EB.ALL:
        for scale in (1.0, 10.0):                              # 10: |logit| reaches about 100
            x, w, b, _ = head_operands(N, V, Cin, Cout, kind, scale)
            for cs in EB.HEAD_CODE_SETS:
                codes = EB.head_codes(cs, Cout)
                ref, bound, _ = EB.head_fwd_reference(x, w, b, codes)
                got = head_fwd_emu(x, w, b, codes)
                rows.append(EB.compare(f"fwd {kind} x{scale:g} {cs}", got, ref, bound, axes="ncv"))
                for lo, hi in EB.softmax_groups(codes):
                    tot = got[:, lo:hi + 1].double().sum(1)
                    rows.append(EB.compare(f"fwd {kind} x{scale:g} {cs} group{lo} sums to 1", tot, torch.ones_like(tot),
                                           torch.full_like(tot, EB.softmax_sum_bound(hi - lo + 1)), axes="nv"))
                    if hi == lo:
                        assert bool((got[:, lo] == 1.0).all())
                if cs == "softmax" and Cout > 1 and kind == "f32" and scale == 1.0:
                    assert _fails(EB.compare("a softmax group without its last channel", head_fwd_emu(x, w, b, codes, drop_last=True), ref, bound, axes="ncv"))
            if scale == 10.0:
                assert float(EB.head_fwd_reference(x, w, b, [0] * Cout)[0].abs().max()) > 80
    for mode in EB.BWD_MODES:
        gk, xk = EB.MODES[mode]
        x, w, _, dout = head_operands(N, V, Cin, Cout, xk)
        dout = dout + 0.5                                       # db and dW terms of one prevailing sign: a lost row shows
        x = CB.round_to(x + 0.5, xk)
        db0 = torch.arange(1, Cout + 1).float()
        ref = EB.head_bwd_reference(x, w, dout, mode, db0)
        dx, dw, db = head_bwd_emu(x, w, dout, mode, db0)
        rows += [EB.compare(f"bwd {mode} dx", dx, *ref["dx"], axes="nvc"), EB.compare(f"bwd {mode} dw", dw, *ref["dw"], axes="oi"),
                 EB.compare(f"bwd {mode} db", db, *ref["db"], axes="o")]
        if mode == "f32":
            _, dw1, db1 = head_bwd_emu(x, w, dout, mode, db0, omit_last_row=True)
            assert _fails(EB.compare("dW without the last partial row", dw1, *ref["dw"], axes="oi"))
            assert _fails(EB.compare("db without the last partial row", db1, *ref["db"], axes="o"))
            assert _fails(EB.compare("db overwritten, not added to", db - db0, *ref["db"], axes="o"))
    _rec(rows, f"head Cout{Cout} Cin{Cin}")


def test_head_reference_is_autograd():
    N, S, Cin, Cout = 2, (3, 4, 5), 16, 6
    V = S[0] * S[1] * S[2]
    x, w, b, dout = head_operands(N, V, Cin, Cout, "f32")
    codes = [1, 3, 3, 2, 0, 3]
    xt = x.clone().requires_grad_(True)
    wt, bt = w.double().requires_grad_(True), b.double().requires_grad_(True)
    z = F.conv3d(xt.reshape(N, *S, Cin).permute(0, 4, 1, 2, 3), wt[:, :, None, None, None], bt).reshape(N, Cout, V)
    out = torch.stack([torch.sigmoid(z[:, 0]), *torch.softmax(z[:, 1:3], 1).unbind(1), torch.tanh(z[:, 3]), z[:, 4], torch.ones_like(z[:, 5])], 1)
    ref, _, _ = EB.head_fwd_reference(x, w, b, codes)
    assert torch.allclose(ref, out.detach(), rtol=1e-12, atol=1e-12)
    (z * dout.double()).sum().backward()
    r = EB.head_bwd_reference(x, w, dout, "f32", torch.zeros(Cout))
    assert torch.allclose(r["dx"][0], xt.grad, rtol=1e-12, atol=1e-12) and torch.allclose(r["dw"][0], wt.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(r["db"][0], bt.grad, rtol=1e-12, atol=1e-12)


# ---- the first layer -------------------------------------------------------------------------------------------------------------------------
def c1_operands(shape, kind, seed=0):
    N, D, H, W, C = shape
    gen = torch.Generator().manual_seed(seed + D + H + W + C)
    img = (0.5 + torch.randn(N, D, H, W, generator=gen)).float()
    dy = CB.round_to(0.25 + torch.randn(N, D, H, W, C, generator=gen), kind)
    return img, dy


def nb_operands(shape, tk, seed=0):
    """g (bf16), t (tk) and per-sample coefficients that differ strongly between the samples: a = 1, 4, 16, .., b and c0 likewise."""
    N, D, H, W, C = shape
    gen = torch.Generator().manual_seed(seed + 7 + D + H + W + C)
    g = CB.round_to(0.25 + torch.randn(N, D, H, W, C, generator=gen), "bf16")
    t = CB.round_to(torch.randn(N, D, H, W, C, generator=gen), tk)
    coef = torch.randn(N, C, 4, generator=gen).float() * 0.3 + 0.5
    coef = (coef * (4.0 ** torch.arange(N))[:, None, None]).float().contiguous()
    return g, t, coef


def bf16_split(img):
    hi = img.float().to(torch.bfloat16).float()
    return hi.double() + (img.float() - hi).to(torch.bfloat16).double()


def c1_emu(img, dy, kernel, rows, db_init, shift_tap=None):
    """The partial rows of the first-layer kernels: a tile's terms go to row (tile mod rows); a row is summed exactly and rounded to fp32 once,
    the rows are added in sequence in fp32.  MFMA: the image as its hi + lo bf16 parts."""
    N, D, H, W = img.shape
    Cout = dy.shape[-1]
    (tz, ty, tx), tiles, _ = EB.c1_plan(kernel, N, D, H, W)
    n, z, y, x = torch.meshgrid(torch.arange(N), torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")
    tY, tX = EB.cdiv(H, ty), EB.cdiv(W, tx)
    tile = n * (EB.cdiv(D, tz) * tY * tX) + ((z // tz) * tY + y // ty) * tX + x // tx
    slot = (tile % rows).reshape(-1)
    im = bf16_split(img) if kernel == "mfma" else img.double()
    g = dy.reshape(-1, Cout)
    dw = torch.zeros(Cout, 27)
    for tap, iv in EB.c1_tap_terms(im, shift_tap):
        part = _f32(torch.zeros(rows, Cout, dtype=torch.float64).index_add_(0, slot, iv[:, None] * g)).float()
        s = torch.zeros(Cout)
        for r in range(rows):
            s = s + part[r]
        dw[:, tap] = s
    part = _f32(torch.zeros(rows, Cout, dtype=torch.float64).index_add_(0, slot, g)).float()
    s = torch.zeros(Cout)
    for r in range(rows):
        s = s + part[r]
    return dw, None if db_init is None else db_init + s


def _cpu_shape(shape):
    """The GPU shape, or the one reduced shape: (1, 8, 64, 520, 16) - 266,240 voxels - keeps its W (65 tiles along x) at D 4, H 16."""
    return (1, 4, 16, 520, 16) if shape == (1, 8, 64, 520, 16) else shape


C1_SCALAR_CASES = [(s, k) for s, ks in EB.C1_SCALAR_ROWS for k in ks]


@pytest.mark.parametrize("shape,kind", C1_SCALAR_CASES, ids=[f"{'x'.join(map(str, s))}-{k}" for s, k in C1_SCALAR_CASES])
def test_c1_scalar_emulation_passes_and_defects_fail(shape, kind):
    shape = _cpu_shape(shape)
    img, dy = c1_operands(shape, kind)
    _, tiles, rows = EB.c1_plan("scalar", *shape[:4])
    db0 = torch.arange(1, shape[4] + 1).float()
    ref = EB.c1_wgrad_reference(img.double(), dy, "scalar", (tiles, rows), db0)
    dw, db = c1_emu(img, dy, "scalar", rows, db0)
    _rec([EB.compare("dw", dw, *ref["dw"], axes="ot"), EB.compare("db", db, *ref["db"], axes="o")], f"c1_scalar {shape} {kind}")
    for tap in (9, 13, 17):                                    # (the plane of the voxel itself: with D = 1 the other taps see padding only)
        assert _fails(EB.compare(f"tap {tap} one voxel off", c1_emu(img, dy, "scalar", rows, db0, shift_tap=tap)[0], *ref["dw"], axes="ot"))


@pytest.mark.parametrize("shape,cap", EB.C1_MFMA_ROWS, ids=["x".join(map(str, s)) + f"-cap{c}" for s, c in EB.C1_MFMA_ROWS])
def test_c1_mfma_emulation_passes_and_defects_fail(shape, cap):
    img, dy = c1_operands(shape, "bf16")
    _, tiles, rows = EB.c1_plan("mfma", *shape[:4], persist=cap)
    db0 = torch.arange(1, shape[4] + 1).float()
    ref = EB.c1_wgrad_reference(img.double(), dy, "mfma", (tiles, rows), db0)
    dw, db = c1_emu(img, dy, "mfma", rows, db0)
    out = [EB.compare("dw", dw, *ref["dw"], axes="ot"), EB.compare("db", db, *ref["db"], axes="o")]
    assert _fails(EB.compare("tap 14 one voxel off", c1_emu(img, dy, "mfma", rows, db0, shift_tap=14)[0], *ref["dw"], axes="ot"))
    hi_only = img.float().to(torch.bfloat16).float()
    if img.numel() < 3000:      # (random-sign operand errors of 2^-9 grow like sqrt(voxels), the bound's 2^-16 term like voxels: shown at the small shapes)
        assert _fails(EB.compare("the image's lo part dropped", c1_emu(hi_only, dy, "scalar", rows, db0)[0], *ref["dw"], axes="ot"))
    if shape[0] > 1 and shape[3] > 8:
        for mode in ("bf16", "mix16"):
            g, t, coef = nb_operands(shape, EB.MODES[mode][1])
            dref, dbound = NB.apply_reference(g, t, coef, None, "bf16")
            k = coef[:, None, None, None]
            dev = CB.round_to(k[..., 0] * g.float() + k[..., 1] * t.float() + k[..., 2], "bf16")      # `ka * g + kb * t + kc` in fp32, the bf16 store
            rn = EB.c1_wgrad_reference(img.double(), dref, "mfma", (tiles, rows), db0, edy=dbound)
            dwn, dbn = c1_emu(img, dev, "mfma", rows, db0)
            out += [EB.compare(f"nb {mode} dw", dwn, *rn["dw"], axes="ot"), EB.compare(f"nb {mode} db", dbn, *rn["db"], axes="o")]
            kk = coef.roll(1, 0)[:, None, None, None]                                                  # every sample with its predecessor's coefficients
            stale = CB.round_to(kk[..., 0] * g.float() + kk[..., 1] * t.float() + kk[..., 2], "bf16")
            assert _fails(EB.compare("the previous sample's coefficients", c1_emu(img, stale, "mfma", rows, db0)[0], *rn["dw"], axes="ot"))
            kk = torch.cat([coef[:1], coef[:-1]])[:, None, None, None]                                 # only the samples after the first
            stale = CB.round_to(kk[..., 0] * g.float() + kk[..., 1] * t.float() + kk[..., 2], "bf16")
            assert _fails(EB.compare("coefficients kept across a sample boundary", c1_emu(img, stale, "mfma", rows, db0)[0], *rn["dw"], axes="ot"))
    _rec(out, f"c1_mfma {shape} cap{cap}")


def test_c1_reference_is_autograd():
    shape = (2, 3, 5, 6, 16)
    img, dy = c1_operands(shape, "f32")
    w = torch.zeros(16, 1, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(16, dtype=torch.float64, requires_grad=True)
    (F.conv3d(img.double()[:, None], w, b, padding=1).permute(0, 2, 3, 4, 1) * dy).sum().backward()
    ref = EB.c1_wgrad_reference(img.double(), dy, "scalar", (1, 1), torch.zeros(16))
    assert torch.allclose(ref["dw"][0], w.grad.reshape(16, 27), rtol=1e-12, atol=1e-12) and torch.allclose(ref["db"][0], b.grad, rtol=1e-12, atol=1e-12)
    w1 = torch.zeros(16, 1, 1, 1, 1, dtype=torch.float64, requires_grad=True)
    (F.conv3d(img.double()[:, None], w1).permute(0, 2, 3, 4, 1) * dy).sum().backward()
    assert torch.allclose(EB.rank1_reference(img.double().reshape(-1), dy.reshape(-1, 16))[0], w1.grad.reshape(16), rtol=1e-12, atol=1e-12)


def rank1_emu(img, dy, lose=None):
    """The partial rows of rank1_wgrad_kernel: voxel v belongs to thread v mod (rows 256); lose: a range of voxels left out - a fault."""
    total, C = dy.shape
    rows = EB.rank1_rows(total)
    v = torch.arange(total)
    slot = (v % (rows * 256)) // 256
    t = img.double()[:, None] * dy
    if lose is not None:
        t[lose[0]:lose[1]] = 0
    part = _f32(torch.zeros(rows, C, dtype=torch.float64).index_add_(0, slot, t)).float()
    s = torch.zeros(C)
    for r in range(rows):
        s = s + part[r]
    return s


@pytest.mark.parametrize("total", EB.RANK1_TOTALS)
def test_rank1_emulation_passes_and_defects_fail(total):
    rows = []
    stride = EB.rank1_rows(total) * 256
    for kind in ("f32", "bf16"):
        gen = torch.Generator().manual_seed(total % 1000)
        img = (0.5 + torch.randn(total, generator=gen)).float()
        dy = CB.round_to(0.25 + torch.randn(total, 16, generator=gen), kind)
        ref, bound = EB.rank1_reference(img.double(), dy)
        rows.append(EB.compare(f"{kind}", rank1_emu(img, dy), ref, bound, axes="o"))
        if total <= 3072:
            assert _fails(EB.compare("the last voxel lost", rank1_emu(img, dy, lose=(total - 1, total)), ref, bound, axes="o"))
        else:       # the second trip of the tail loop (fourth total) / the tail behind the four-in-flight loop (fifth) lost
            assert _fails(EB.compare("the voxels past the first sweep lost", rank1_emu(img, dy, lose=(total - total % stride, total)), ref, bound, axes="o"))
    _rec(rows, f"rank1 total{total}")


# ---- the rows reach what they name -----------------------------------------------------------------------------------------------------------
def test_gpu_rows_reach_the_paths_they_name():
    rows = {r[0]: r for r in EB.DROP_ROWS}
    assert rows["partly_filled_block"][2] * (16 // 8) < 256 and set(rows["partly_filled_block"][4]) == set(range(EB.ACT_LAST + 1))
    for name, N, V, C, acts in EB.DROP_ROWS:
        assert 1 in acts and len(acts) >= 2
        for kind in EB.ALL:
            assert (EB.drop_tiles(V, C, kind) * 256) % (C // EB.kpl(kind)) == 0
    assert {48 // EB.kpl(k) for k in EB.ALL} == {6, 12}
    assert all(EB.drop_tiles(1031, 48, k) % 3 == 0 and EB.cdiv(1031 * (48 // EB.kpl(k)), 256) % 3 != 0 for k in ("f32", "bf16"))
    assert all(EB.drop_tiles(4099, 80, k) % 5 == 0 for k in EB.ALL)
    assert all(70001 * (16 // EB.kpl(k)) > EB.NA_BLOCKS * 256 for k in EB.ALL)
    assert 2048 // 4 == 512
    assert EB.head_bwd_blocks(EB.HEAD_N * EB.HEAD_VPS, 8, 32) == 16 and EB.cdiv(EB.HEAD_N * EB.HEAD_VPS, 256) == 13
    assert EB.head_bwd_blocks(EB.HEAD_N * EB.HEAD_VPS, 8, 16) == 13 and EB.head_bwd_blocks(EB.HEAD_N * EB.HEAD_VPS, 4, 32) == 13
    assert EB.HEAD_FWD_WRAP_SHAPE[0] * EB.HEAD_FWD_WRAP_SHAPE[1] > 4096 * 256 and EB.HEAD_BWD_WRAP_SHAPE[0] * EB.HEAD_BWD_WRAP_SHAPE[1] > 1024 * 256
    for name in EB.HEAD_CODE_SETS:
        for Cout in range(1, 9):
            assert len(EB.head_codes(name, Cout)) == Cout
    assert EB.softmax_groups(EB.head_codes("two_groups", 8)) == [(0, 2), (4, 7)] and EB.softmax_groups(EB.head_codes("single_group", 4)) == [(0, 0), (2, 3)]
    assert EB.head_codes("mixed", 4) == [1, 3, 3, 2]
    for shape, kinds in EB.C1_SCALAR_ROWS:                     # the scalar kernel runs at f32 always and at bf16 where W <= 8
        assert all(k == "f32" or shape[3] <= 8 for k in kinds)
    assert EB.c1_plan("scalar", 1, 8, 64, 520)[1] > 1024 and EB.c1_plan("scalar", 1, 8, 64, 520)[2] == 1024
    assert all(s[3] > 8 for s, _ in EB.C1_MFMA_ROWS)
    t, tiles, wgs = EB.c1_plan("mfma", 3, 8, 12, 40, persist=5)
    assert (tiles // 3, tiles, wgs) == (18, 54, 5)             # 18 tiles per sample, not a multiple of 5: every workgroup crosses sample boundaries
    for w in range(5):
        assert len({tt // 18 for tt in range(w, 54, 5)}) == 3
    assert {s[1] for s, _ in EB.C1_SCALAR_ROWS + EB.C1_MFMA_ROWS} >= {1} and {s[4] for s, _ in EB.C1_SCALAR_ROWS + EB.C1_MFMA_ROWS} == {16, 32}
    assert [EB.rank1_loops(t) for t in EB.RANK1_TOTALS] == [(0, 0), (0, 0), (0, 0), (0, 0), (262144, 1000)]
    assert EB.rank1_rows(262144 + 77) == 1024 and EB.cdiv(262144 + 77, 1024 * 256) == 2


def test_host_refusals_of_the_dropout_entries():
    """BPX_CHECK returns before any device call: the pointers below are never dereferenced."""
    from biapy_amd import _lib as L

    lib = L.lib
    P = 4096
    t = lambda C, ld=None: L.Tensor(P, C if ld is None else ld, C, 0)

    def fwd(p=0.3, ctr=P, mode=0, mask=None, x=None):
        return lib.bpx_norm_act_dropout_fwd(L.BF16, 1, 64, x or t(16), P, 1, p, 1, ctr, 0, mask, mode, t(16), None)

    def bwd(p=0.3, ctr=P, mode=0, mask=None, x=None):
        return lib.bpx_norm_act_dropout_bwd(L.BF16, 1, 64, t(16), x or t(16), P, 1, p, 1, ctr, 0, mask, mode, t(16), P, None)

    for fn, call in (("bpx_norm_act_dropout_fwd", fwd), ("bpx_norm_act_dropout_bwd", bwd)):
        for kw, words in ((dict(p=1.0), "outside [0, 1)"), (dict(p=-0.1), "outside [0, 1)"), (dict(ctr=None), "step counter is null"),
                          (dict(mode=1), "needs a mask buffer"), (dict(x=t(16, 32)), "dense tensors only")):
            assert call(**kw) != 0
            msg = lib.bpx_last_error().decode()
            assert fn in msg and words in msg, msg

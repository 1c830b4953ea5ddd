"""The gate and channel-affine kernels of elementwise.hip and the 1-channel up-sampling kernels of ends.hip element by element against float64
(tests/gate_bounds.py): bpx_channel_affine, bpx_dot_stats, bpx_gate_mul_fwd / _bwd (bit for bit), bpx_upsample_c1_fwd / _bwd and
bpx_gate_mlp_fwd / _bwd.  Every output is pre-filled with NaN, carries one sentinel voxel or row past its end that must keep its value, sliced buffers are checked for untouched
neighbours, and each row records max(|got - ref| / bound) with the position of its worst element."""
import math

import pytest
import torch

import conv_bounds as CB
import gate_bounds as GB
from test_conv_bounds_gpu import _record_diag
from test_norm_bounds_gpu import Buf, _flag

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _L():
    from biapy_amd import _lib as L

    return L


def _check(rows):
    for r in rows:
        _record_diag(f"gate_bounds[{r['name']}] err/bound = {r['err']:.3e} {r['extra']}")
    bad = [r for r in rows if not r["ok"]]
    assert not bad, bad


def _dtc(mode):
    L = _L()
    return {"f32": L.F32, "bf16": L.BF16, "f16": L.F16, "mix16": L.MIX16}[mode]


class SBuf(Buf):
    """A Buf with one sentinel voxel (every channel 7) past its end."""

    def __init__(self, shape, kind, sliced=False, value=None, pad=16):
        T = CB.TORCH_DT[kind]
        C = shape[-1]
        self.pad = pad if sliced else 0
        self.C = C
        nv = math.prod(shape[:-1])
        self.flat = torch.full((nv + 1, C + 2 * self.pad), 7.0, dtype=T, device=DEV)
        self.buf = self.flat[:nv].view(*shape[:-1], C + 2 * self.pad)
        self.buf[..., self.pad:self.pad + C] = NAN if value is None else value.to(T).to(DEV)

    def untouched(self, tag):
        return super().untouched(tag) + [_flag(tag + ".sentinel_kept", bool((self.flat[-1].float() == 7).all().item()))]


def _rows_out(*shape):
    """An fp32 output of `shape` pre-filled with NaN, and the sentinel row of 7s past its end: (view, flat)."""
    n = math.prod(shape)
    flat = torch.full((n + shape[-1],), NAN, device=DEV)
    flat[n:] = 7.0
    return flat[:n].view(*shape), flat


def _kept(tag, flat, n):
    return _flag(tag + ".sentinel_kept", bool((flat[n:] == 7).all().item()))


# ---- channel_affine ---------------------------------------------------------------------------------------------------------------------
AFFINE_CASES = [(r, k) for r in GB.AFFINE_ROWS for k in r[1]]


@pytest.mark.parametrize("row,kind", AFFINE_CASES, ids=[f"{r[0]}-{k}" for r, k in AFFINE_CASES])
def test_channel_affine_elementwise(row, kind):
    """channel_affine_kernel<T>: y = [x +] s[n, c] h [+ off[n, c]]; in place means y = x, as resunetpp_engine._accum calls it.  B 3: sample 1
    alone gives the same bits."""
    L = _L()
    lib = L.lib
    name, _, vox, C, sliced, with_x, with_off, inplace = row
    B = 3
    gen = torch.Generator().manual_seed(vox + C)
    h = CB.round_to(torch.randn(B, vox, C, generator=gen), kind)
    x = CB.round_to(torch.randn(B, vox, C, generator=gen), kind) if with_x else None
    s = torch.randn(B, C, generator=gen).float()
    off = (0.3 * torch.randn(B, C, generator=gen)).float() if with_off else None

    def run(sel):
        n = h[sel].shape[0]
        hb = SBuf((n, vox, C), kind, sliced, h[sel])
        xb = SBuf((n, vox, C), kind, sliced, x[sel]) if with_x else None
        yb = xb if inplace else SBuf((n, vox, C), kind, sliced)
        sd = s[sel].contiguous().to(DEV)
        od = off[sel].contiguous().to(DEV) if with_off else None
        L.check(lib.bpx_channel_affine(_dtc(kind), n, vox, xb.view() if with_x else L.NULL_T, hb.view(), sd.data_ptr(), L.ptr(od), yb.view(), L.stream_ptr()))
        torch.cuda.synchronize()
        return yb

    yb = run(slice(0, B))
    ref, bound = GB.channel_affine_reference(h.to(DEV), s, off, x.to(DEV) if with_x else None, kind)
    tag = f"channel_affine[{name} {kind}]"
    alone = run(slice(1, 2))
    _check([GB.compare(tag + ".y", yb.read(), ref, bound, axes="nvc"), GB.exact_row(tag + ".sample1_alone_same_bits", alone.read()[0], yb.read()[1])] +
           yb.untouched(tag))


@pytest.mark.parametrize("kind", GB.AFFINE_REFUSED[1])
def test_channel_affine_refuses_c24(kind):
    """The host demands C % 16 == 0 at every storage type (the vector is 4 elements wide at f32, but the launcher does not admit C 24 there
    either): nothing is launched and the output keeps its pre-fill."""
    L = _L()
    _, _, vox, C = GB.AFFINE_REFUSED
    hb, yb = SBuf((2, vox, C), kind), SBuf((2, vox, C), kind)
    sd = torch.ones(2, C, device=DEV)
    assert L.lib.bpx_channel_affine(_dtc(kind), 2, vox, L.NULL_T, hb.view(), sd.data_ptr(), None, yb.view(), L.stream_ptr()) != 0
    assert "multiple of 16" in L.lib.bpx_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(yb.read().float()).all().item())


# ---- dot_stats ----------------------------------------------------------------------------------------------------------------------------
DOT_CASES = [(r, m) for r in GB.DOT_ROWS for m in r[1]]


@pytest.mark.parametrize("row,mode", DOT_CASES, ids=[f"{r[0]}-{m}" for r, m in DOT_CASES])
def test_dot_stats_elementwise(row, mode):
    """dot_stats_kernel<T, TB>: part[n][block][c] = sum over the block's items of a b, the rows summed here in fp64.  Data of one sign per
    channel, so a lost term or row shows against chain 2^-24 sum|terms|; every row written and finite; B 3: sample 1 alone gives the same rows."""
    L = _L()
    lib = L.lib
    name, _, vox, C, sliced = row
    ak, bk = GB.MODES[mode]
    B = 3
    gen = torch.Generator().manual_seed(vox + C)
    a = CB.round_to(GB.onesign((B, vox, C), gen), ak)
    b = CB.round_to(GB.onesign((B, vox, C), gen), bk)
    tiles = lib.bpx_norm_act_tiles(_dtc(ak), vox, C)
    assert tiles == GB.na_tiles(vox, C, ak)

    def run(sel):
        n = a[sel].shape[0]
        ab, bb = Buf((n, vox, C), ak, sliced, a[sel]), Buf((n, vox, C), bk, sliced, b[sel])
        part, flat = _rows_out(n, tiles, C)
        L.check(lib.bpx_dot_stats(_dtc(mode), n, vox, ab.view(), bb.view(), part.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
        return part, flat

    part, flat = run(slice(0, B))
    ref, bound = GB.dot_stats_reference(a.to(DEV), b.to(DEV), GB.dot_stats_chain(vox, C, ak, tiles))
    tag = f"dot_stats[{name} {mode} tiles{tiles}]"
    alone, _ = run(slice(1, 2))
    _check([GB.compare(tag + ".sums", part.double().sum(1), ref, bound, axes="nc"), _flag(tag + ".every_row_finite", bool(torch.isfinite(part).all().item())),
            GB.exact_row(tag + ".sample1_alone_same_rows", alone[0], part[1]), _kept(tag, flat, part.numel())])


# ---- gate multiply: bit for bit ---------------------------------------------------------------------------------------------------------
def _gate_a(a, kind, ld):
    """The gate as the engines hand it over: channel 3 of a 16-channel tensor (ld 16) or a dense 1-channel tensor (ld 1); the other channels 7."""
    L = _L()
    buf = torch.full((a.shape[0], ld), 7.0, dtype=CB.TORCH_DT[kind], device=DEV)
    c0 = 3 if ld == 16 else 0
    buf[:, c0] = a.to(CB.TORCH_DT[kind]).to(DEV)
    return buf, L.tview(buf, c0, 1)


GATE_FWD_CASES = [(r, k) for r in GB.GATE_ROWS for k in r[1]]


@pytest.mark.parametrize("row,kind", GATE_FWD_CASES, ids=[f"{r[0]}-{k}" for r, k in GATE_FWD_CASES])
def test_gate_mul_fwd_bit_for_bit(row, kind):
    """gate_mul_fwd_kernel<T>: y = a[v] x[v][c], one exact product and one round-to-nearest-even store."""
    L = _L()
    name, _, _, V, C, ld, sliced = row
    gen = torch.Generator().manual_seed(V + C)
    a, x, _ = GB.gate_inputs(V, C, gen)
    a, x = CB.round_to(a, kind), CB.round_to(x, kind)
    abuf, av = _gate_a(a, kind, ld)
    xb, yb = SBuf((V, C), kind, sliced, x), SBuf((V, C), kind, sliced)
    L.check(L.lib.bpx_gate_mul_fwd(_dtc(kind), V, av, xb.view(), yb.view(), L.stream_ptr()))
    torch.cuda.synchronize()
    tag = f"gate_mul_fwd[{name} {kind}]"
    _check(GB.gate_fwd_rows(tag + ".y", yb.read(), GB.gate_product(a.to(DEV), x.to(DEV), kind), kind) + yb.untouched(tag + ".y"))


GATE_BWD_CASES = [(r, m) for r in GB.GATE_ROWS for m in r[2]]


@pytest.mark.parametrize("row,mode", GATE_BWD_CASES, ids=[f"{r[0]}-{m}" for r, m in GATE_BWD_CASES])
def test_gate_mul_bwd_elementwise(row, mode):
    """gate_mul_bwd_kernel<T, TT>: dx = dy a bit for bit; da = sum_c dy x in channel 0 of a 16-channel tensor against its bound, channels
    1..15 exactly 0."""
    L = _L()
    name, _, _, V, C, ld, sliced = row
    gk, tk = GB.MODES[mode]
    gen = torch.Generator().manual_seed(V + C + 1)
    a, x, dy = GB.gate_inputs(V, C, gen)
    a, x, dy = CB.round_to(a, tk), CB.round_to(x, tk), CB.round_to(dy, gk)
    abuf, av = _gate_a(a, tk, ld)
    xb, dyb, dxb = Buf((V, C), tk, sliced, x), Buf((V, C), gk, sliced, dy), SBuf((V, C), gk, sliced)
    da = SBuf((V, 16), gk)
    L.check(L.lib.bpx_gate_mul_bwd(_dtc(mode), V, dyb.view(), av, xb.view(), dxb.view(), da.buf.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    tag = f"gate_mul_bwd[{name} {mode}]"
    ref, bound = GB.gate_da_reference(dy.to(DEV), x.to(DEV), mode)
    got = da.read()
    _check(GB.gate_fwd_rows(tag + ".dx", dxb.read(), GB.gate_product(a.to(DEV), dy.to(DEV), gk), gk) + dxb.untouched(tag + ".dx") +
           [GB.compare(tag + ".da", got[:, 0], ref, bound, axes="v"), GB.exact_row(tag + ".da16_channels_1_15_zero", got[:, 1:], torch.zeros_like(got[:, 1:]))] +
           da.untouched(tag + ".da16"))


# ---- 1-channel up-sampling ----------------------------------------------------------------------------------------------------------------
def _ups_operands(N, S, factor, gen):
    img = torch.randn(N, *S, generator=gen).float()
    w = torch.randn(factor[0] * factor[1] * factor[2], generator=gen).float()        # a distinct weight per tap
    bias = torch.tensor([0.37])
    return img, w, bias


UPS_FWD_CASES = [(r, k) for r in GB.UPS_ROWS for k in r[1]]


@pytest.mark.parametrize("row,kind", UPS_FWD_CASES, ids=[f"{r[0]}-{k}" for r, k in UPS_FWD_CASES])
def test_upsample_c1_fwd_elementwise(row, kind):
    """upsample_c1_fwd_kernel<T>: channel 0 = img w[a][b][c] + bias, channels 1..15 exactly 0."""
    L = _L()
    name, _, _, N, S, f = row
    gen = torch.Generator().manual_seed(sum(S) + sum(f))
    img, w, bias = _ups_operands(N, S, f, gen)
    imgd, wd, bd = img.to(DEV), w.to(DEV), bias.to(DEV)
    out = SBuf((N, S[0] * f[0], S[1] * f[1], S[2] * f[2], 16), kind)
    L.check(L.lib.bpx_upsample_c1_fwd(_dtc(kind), N, *S, *f, imgd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.buf.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    ref, bound = GB.upsample_fwd_reference(imgd, w, bias, f, kind)
    tag = f"upsample_c1_fwd[{name} {kind}]"
    rest = out.buf[..., 1:]
    _check([GB.compare(tag + ".channel0", out.buf[..., 0], ref, bound, axes="nzyx"),
            _flag(tag + ".channels_1_15_zero", bool((rest.view(torch.int32 if kind == "f32" else torch.int16) == 0).all().item()))] + out.untouched(tag))


UPS_BWD_CASES = [(r, k) for r in GB.UPS_ROWS for k in r[2]]


@pytest.mark.parametrize("row,kind", UPS_BWD_CASES, ids=[f"{r[0]}-{k}" for r, k in UPS_BWD_CASES])
def test_upsample_c1_bwd_elementwise(row, kind):
    """upsample_c1_bwd_kernel<T>: per tap (sum img g, sum g) with g the stored channel 0 of dx16; the partial rows of a tap are summed in fp64
    as resunet.py does.  g of one sign, img of one sign: a lost wave total or row shows."""
    L = _L()
    name, _, _, N, S, f = row
    taps = f[0] * f[1] * f[2]
    gen = torch.Generator().manual_seed(sum(S) + sum(f) + 1)
    img = (2.0 + 0.1 * torch.randn(N, *S, generator=gen)).float()
    So = (S[0] * f[0], S[1] * f[1], S[2] * f[2])
    g = CB.round_to(3.0 + 0.1 * torch.randn(N, *So, generator=gen), kind)
    dx16 = torch.full((N, *So, 16), 7.0, dtype=CB.TORCH_DT[kind], device=DEV)      # channels 1..15 are not read
    dx16[..., 0] = g.to(CB.TORCH_DT[kind]).to(DEV)
    total_in = N * S[0] * S[1] * S[2]
    blocks = L.lib.bpx_upsample_c1_blocks(total_in)
    assert blocks == GB.ups_blocks(total_in)
    part, flat = _rows_out(taps, blocks, 2)
    imgd = img.to(DEV)
    L.check(L.lib.bpx_upsample_c1_bwd(_dtc(kind), N, *S, *f, imgd.data_ptr(), dx16.data_ptr(), part.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    ref, bound = GB.upsample_bwd_reference(imgd, g.to(DEV), f, blocks)
    tag = f"upsample_c1_bwd[{name} {kind} blocks{blocks}]"
    _check([GB.compare(tag + ".sums", part.double().sum(1), ref, bound, axes="tk"), _flag(tag + ".every_row_finite", bool(torch.isfinite(part).all().item())),
            _kept(tag, flat, part.numel())])


# ---- the gate MLP -------------------------------------------------------------------------------------------------------------------------
def _mlp_weights(C, R, bias, gen):
    w1, w2 = (torch.randn(R, C, generator=gen) * 0.3).float(), (torch.randn(C, R, generator=gen) * 0.3).float()
    b1 = (torch.randn(R, generator=gen) * 0.1).float() if bias else None
    b2 = (torch.randn(C, generator=gen) * 0.1).float() if bias else None
    return w1, b1, w2, b2


def _run_mlp_fwd(part, vox, w1, b1, w2, b2, act):
    L = _L()
    N, tiles, _, C = part.shape
    R = w1.shape[0]
    d = lambda t: None if t is None else t.to(DEV)
    pd, w1d, b1d, w2d, b2d = d(part), d(w1), d(b1), d(w2), d(b2)
    s, sflat = _rows_out(N, C)
    sv, svflat = _rows_out(N, C + 2 * R)
    L.check(L.lib.bpx_gate_mlp_fwd(pd.data_ptr(), N, tiles, C, vox, w1d.data_ptr(), L.ptr(b1d), w2d.data_ptr(), L.ptr(b2d), R, act, s.data_ptr(), sv.data_ptr(),
                                   L.stream_ptr()))
    torch.cuda.synchronize()
    return s, sflat, sv, svflat


@pytest.mark.parametrize("tiles,C,R,act,bias,N", GB.MLP_ROWS, ids=[f"t{t}-C{c}-R{r}-act{a}-b{int(b)}-N{n}" for t, c, r, a, b, n in GB.MLP_ROWS])
def test_gate_mlp_fwd_bwd_elementwise(tiles, C, R, act, bias, N):
    """gate_mlp_fwd_kernel (s and the three parts of saved, each against its own bound; partial rows of one sign per channel, so a lost row
    shows in m) and gate_mlp_bwd_kernel on operands supplied here (off, dW1, db1, dW2, db2 ADDED to non-zero buffers; with null db1 / db2
    nothing else is touched); sample 1 alone gives the bits of s and saved."""
    L = _L()
    gen = torch.Generator().manual_seed(tiles + C + R + act + N)
    vox = 5 * tiles
    part = torch.stack([GB.bigmean_rows(N, tiles, C, gen), torch.randn(N, tiles, C, generator=gen)], 2).float().contiguous()
    w1, b1, w2, b2 = _mlp_weights(C, R, bias, gen)
    s, sflat, sv, svflat = _run_mlp_fwd(part, vox, w1, b1, w2, b2, act)
    tag = f"gate_mlp[t{tiles} C{C} R{R} act{act} bias{int(bias)} N{N}]"
    f = GB.gate_mlp_fwd_reference(part.to(DEV), vox, w1, b1, w2, b2, act)
    if not bool((f["a1"][0] != 0).any().item()):
        _record_diag(f"gate_bounds[{tag}] every unit of the hidden layer is off for every sample: a1 = 0 and s = sigmoid(b2) carry no rounding (err 0 is exact)")
    rows = [GB.compare(tag + ".s", s, *f["s"], axes="nc"), GB.compare(tag + ".saved.m", sv[:, :C], *f["m"], axes="nc"),
            GB.compare(tag + ".saved.u1", sv[:, C:C + R], *f["u1"], axes="nr"), GB.compare(tag + ".saved.a1", sv[:, C + R:], *f["a1"], axes="nr"),
            _kept(tag + ".s", sflat, s.numel()), _kept(tag + ".saved", svflat, sv.numel())]
    if N > 1:
        s1, _, sv1, _ = _run_mlp_fwd(part[1:2], vox, w1, b1, w2, b2, act)
        rows += [GB.exact_row(tag + ".s.sample1_alone_same_bits", s1[0], s[1]), GB.exact_row(tag + ".saved.sample1_alone_same_bits", sv1[0], sv[1])]
    # backward on its own operands
    btiles = max(1, tiles // 2 + 1)
    dpart = GB.bigmean_rows(N, btiles, C, gen).float()
    s_in = (0.05 + 0.9 * torch.rand(N, C, generator=gen)).float()
    saved = torch.cat([torch.randn(N, C, generator=gen), torch.randn(N, R, generator=gen), torch.randn(N, R, generator=gen)], 1).float()
    saved[0, C:C + R] = saved[0, C:C + R].abs()             # sample 0's hidden units are on: a ReLU backward is never dead for every sample
    init = dict(dw1=torch.randn(R, C, generator=gen).float(), dw2=torch.randn(C, R, generator=gen).float(),
                db1=torch.randn(R, generator=gen).float() if bias else None, db2=torch.randn(C, generator=gen).float() if bias else None)
    dev ={k: (None if v is None else _with_sentinel(v)) for k, v in init.items()}
    off, offflat = _rows_out(N, C)
    dpd, sd, svd, w1d, w2d = dpart.to(DEV), s_in.to(DEV), saved.to(DEV), w1.to(DEV), w2.to(DEV)
    p = lambda k: None if dev[k] is None else dev[k][0].data_ptr()
    L.check(L.lib.bpx_gate_mlp_bwd(dpd.data_ptr(), N, btiles, C, vox, sd.data_ptr(), svd.data_ptr(), w1d.data_ptr(), w2d.data_ptr(), R, act, p("dw1"), p("db1"), p("dw2"),
                                   p("db2"), off.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    b = GB.gate_mlp_bwd_reference(dpd, vox, s_in, saved, w1, w2, act, init)
    rows += [GB.compare(tag + ".bwd.off", off, *b["off"], axes="nc"), _kept(tag + ".bwd.off", offflat, off.numel())]
    for k, axes in (("dw1", "rc"), ("dw2", "cr"), ("db1", "r"), ("db2", "c")):
        if dev[k] is not None:
            rows += [GB.compare(tag + f".bwd.{k}_added", dev[k][0], *b[k], axes=axes), _kept(tag + f".bwd.{k}", dev[k][1], dev[k][0].numel())]
    rows.append(_flag(tag + ".bwd.operands_unchanged", torch.equal(sd.cpu(), s_in) and torch.equal(svd.cpu(), saved) and torch.equal(dpd.cpu(), dpart)))
    _check(rows)


def _with_sentinel(v):
    n = v.numel()
    flat = torch.full((n + v.shape[-1],), 7.0, device=DEV)
    flat[:n] = v.reshape(-1).to(DEV)
    return flat[:n].view(v.shape), flat


@pytest.mark.parametrize("tiles,C", GB.MLP_BITS_ROWS, ids=[f"t{t}-C{c}" for t, c in GB.MLP_BITS_ROWS])
def test_gate_column_sum_same_bits_in_every_loop(tiles, C):
    """The claim in gate_column_sum that its 16-deep and 4-deep loops "keep the order of the 4-row loop: same bits".  The device cannot be told
    to skip its loops, so the total is formed on the host in fp64 in the kernel's stated order and with every row through the tail loop alone, on
    rows whose partial sums are exact in fp64 (gate_bounds.exact_rows): the two must agree, and saved[:, :C] must equal float(total) * inv_vox
    bit for bit."""
    N, R, vox = 2, 1, 3 * tiles + 1
    gen = torch.Generator().manual_seed(tiles + C)
    col = GB.exact_rows(N, tiles, C, gen)
    part = torch.stack([col, torch.randn(N, tiles, C, generator=gen)], 2).float().contiguous()
    w1, b1, w2, b2 = _mlp_weights(C, R, False, gen)
    s, _, sv, _ = _run_mlp_fwd(part, vox, w1, b1, w2, b2, 2)
    tag = f"gate_column_sum[t{tiles} C{C}]"
    rows = []
    want = []
    for n in range(N):
        tot = GB.column_total_kernel_order(col[n].double(), C)
        tail = GB.column_total_kernel_order(col[n].double(), C, tail_only=True)
        rows.append(_flag(tag + f".n{n}.stated_order_equals_tail_loop_order", torch.equal(tot, tail) and torch.equal(tot, col[n].double().sum(0))))
        want.append(tot.float() * torch.tensor(1.0 / vox, dtype=torch.float64).float())
    rows.append(GB.exact_row(tag + ".saved_m_bits", sv[:, :C], torch.stack(want)))
    _check(rows)

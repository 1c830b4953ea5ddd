"""The dropout pair of elementwise.hip, the output head and the first layer's weight gradients of ends.hip element by element against float64
(tests/ends_bounds.py): bpx_norm_act_dropout_fwd / _bwd (the mask bit for bit against a host Philox4x32-10), bpx_head_fwd / _bwd, bpx_conv3d_c1_wgrad,
bpx_conv3d_c1_wgrad_nb and bpx_conv1x1_c1_wgrad.  Every output is pre-filled with NaN, the padding of every input row and output stride holds NaN
or a sentinel that must keep its value, every backward runs twice and must give the same bits, and each row records max(|got - ref| / bound)
with the position of its worst element."""
import functools

import pytest
import torch

import conv_bounds as CB
import ends_bounds as EB
import norm_bounds as NB
from test_conv_bounds_gpu import _record_diag
from test_gate_bounds_gpu import SBuf, _kept, _rows_out
from test_norm_bounds_gpu import _flag

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _L():
    from biapy_amd import _lib as L

    return L


def _check(rows):
    for r in rows:
        _record_diag(f"ends_bounds[{r['name']}] err/bound = {r['err']:.3e} {r['extra']}")
    bad = [r for r in rows if not r["ok"]]
    assert not bad, bad


def _dtc(mode):
    L = _L()
    return {"f32": L.F32, "bf16": L.BF16, "f16": L.F16, "mix16": L.MIX16}[mode]


def _sync():
    torch.cuda.synchronize()


class PBuf:
    """An operand or output whose rows carry `extra` more channels BEHIND the C in use (the base stays 16-byte aligned): NaN there for an operand -
    a kernel that read them would show it -, 7 for an output, which must keep it; one more row of 7s past the end."""

    def __init__(self, shape, kind, value=None, extra=16):
        T = CB.TORCH_DT[kind]
        C = shape[-1]
        self.C, self.out = C, value is None
        n = 1
        for s in shape[:-1]:
            n *= s
        self.flat = torch.full((n + 1, C + extra), 7.0 if self.out else NAN, dtype=T, device=DEV)
        self.flat[-1] = 7.0
        self.buf = self.flat[:n].view(*shape[:-1], C + extra)
        self.buf[..., :C] = NAN if value is None else value.to(T).to(DEV)

    def view(self):
        return _L().tview(self.buf, 0, self.C)

    def read(self):
        return self.buf[..., :self.C].clone()

    def untouched(self, tag):
        ok = bool((self.flat[-1].float() == 7).all().item()) and (not self.out or bool((self.buf[..., self.C:].float() == 7).all().item()))
        return [_flag(tag + ".padding_and_sentinel_kept", ok)]


class Work:
    """Exactly `nbytes` of workspace (NaN: a partial row that is read but was never written shows) inside a larger buffer whose tail holds 7."""

    def __init__(self, nbytes):
        assert nbytes % 4 == 0
        self.n = nbytes // 4
        self.flat = torch.full((self.n + 256,), 7.0, device=DEV)
        self.flat[:self.n] = NAN
        self.bytes = nbytes

    def ptr(self):
        return self.flat.data_ptr()

    def kept(self, tag):
        return _flag(tag + ".workspace_tail_kept", bool((self.flat[self.n:] == 7).all().item()))


def _vec(v):
    """An fp32 vector on the device with one sentinel row of its own length behind it: (view, flat)."""
    n = v.numel()
    flat = torch.full((2 * n,), 7.0, device=DEV)
    flat[:n] = v.reshape(-1).float().to(DEV)
    return flat[:n].view(v.shape), flat


# ---- dropout ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _keep(shape, seed, ctr, site, p):
    return EB.keep_tensor(seed, ctr, site, p, shape).to(DEV)


def _drop_operands(N, V, C, act, xk, gk):
    gen = torch.Generator().manual_seed(V + C + act)
    x = CB.round_to(torch.randn(N, V, C, generator=gen), xk)
    dy = CB.round_to(torch.randn(N, V, C, generator=gen), gk)
    return x, dy, CB.norm_recs(N, C, gen)


def _counter(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def _flags(n, value=None):
    """n keep flags and 64 sentinel bytes (7) behind them; unwritten flags hold 0xAA."""
    flat = torch.full((n + 64,), 7, dtype=torch.uint8, device=DEV)
    flat[:n] = 0xAA if value is None else value.reshape(-1)
    return flat


def _drop_fwd(kind, x, recd, act, p, seed, ctr, site, flags, mode):
    L = _L()
    N, V, C = x.shape
    xb, yb = SBuf((N, V, C), kind, value=x), SBuf((N, V, C), kind)
    L.check(L.lib.bpx_norm_act_dropout_fwd(_dtc(kind), N, V, xb.view(), recd.data_ptr(), act, p, seed, ctr.data_ptr(), site, L.ptr(flags), mode, yb.view(),
                                           L.stream_ptr()))
    _sync()
    return yb


def _drop_bwd(mode, dy, x, recd, act, p, seed, ctr, site, flags, mmode, tiles):
    L = _L()
    gk, xk = EB.MODES[mode]
    N, V, C = x.shape
    dyb, xb, gb = SBuf((N, V, C), gk, value=dy), SBuf((N, V, C), xk, value=x), SBuf((N, V, C), gk)
    part, pflat = _rows_out(N, tiles, 2, C)
    L.check(L.lib.bpx_norm_act_dropout_bwd(_dtc(mode), N, V, dyb.view(), xb.view(), recd.data_ptr(), act, p, seed, ctr.data_ptr(), site, L.ptr(flags), mmode,
                                           gb.view(), part.data_ptr(), L.stream_ptr()))
    _sync()
    return gb, part, pflat


PAIRS = (("f32", "f32"), ("bf16", "bf16"), ("f16", "mix16"))          # (forward kind, backward mode): the activation tensor has the forward's type
DROP_CASES = [(r, a, pr) for r in EB.DROP_ROWS for a in r[4] for pr in PAIRS]


@pytest.mark.parametrize("row,act,pair", DROP_CASES, ids=[f"{r[0]}-act{a}-{pr[0]}" for r, a, pr in DROP_CASES])
def test_dropout_mask_fwd_bwd_elementwise(row, act, pair):
    """Checks 1 - 4 of a shape: the flags of mode 2 are the host mask whatever the type, y is 0 where dropped and within its bound where kept,
    modes 0 and 1 (flags 255 for keep) give the bits of mode 2; the backward in modes 0 and 1 has g within its bound, zeros where dropped, the
    S1 / S2 rows - bpx_norm_act_dropout_tiles of them - within their chain bound, and the same bits when run again."""
    L = _L()
    name, N, V, C, _ = row
    kind, mode = pair
    p, seed, site, ctrv = EB.DROP_P, EB.DROP_SEED, EB.DROP_SITE, 1
    keep = _keep((N, V, C), seed, ctrv, site, p)
    x, _, rec = _drop_operands(N, V, C, act, kind, kind)
    recd, ctr = rec.to(DEV), _counter(ctrv)
    n = N * V * C
    tag = f"dropout[{name} act{act} {kind}]"
    fl = _flags(n)
    y2 = _drop_fwd(kind, x, recd, act, p, seed, ctr, site, fl, 2)
    ref, bound = EB.dropout_fwd_reference(x.to(DEV), rec, act, kind, p, keep)
    rows = [EB.exact_row(tag + ".flags_equal_host_mask", fl[:n].view(N, V, C), keep.to(torch.uint8)), _flag(tag + ".flags.sentinel_kept", bool((fl[n:] == 7).all().item())),
            EB.compare(tag + ".y", y2.read(), ref, bound, axes="nvc")] + y2.untouched(tag + ".y")
    y0 = _drop_fwd(kind, x, recd, act, p, seed, ctr, site, None, 0)
    rows.append(EB.exact_row(tag + ".mode0_bits_of_mode2", y0.read(), y2.read()))
    fl255 = _flags(n, keep.to(torch.uint8) * 255)
    y1 = _drop_fwd(kind, x, recd, act, p, seed, ctr, site, fl255, 1)
    rows += [EB.exact_row(tag + ".mode1_bits_of_mode2", y1.read(), y2.read()), _flag(tag + ".mode1_flags_unchanged", torch.equal(fl255[:n].view(N, V, C), keep.to(torch.uint8) * 255))]
    # backward
    gk, xk = EB.MODES[mode]
    x, dy, rec = _drop_operands(N, V, C, act, xk, gk)
    tiles = L.lib.bpx_norm_act_dropout_tiles(_dtc(mode), V, C)
    assert tiles == EB.drop_tiles(V, C, gk)
    g, gb, s, sb = EB.dropout_bwd_reference(dy.to(DEV), x.to(DEV), rec, act, mode, p, keep, tiles)
    tag = f"dropout_bwd[{name} act{act} {mode} tiles{tiles}]"
    first = None
    for mm, flg in ((0, None), (1, fl255), (0, None)):
        got, part, pflat = _drop_bwd(mode, dy, x, recd, act, p, seed, ctr, site, flg, mm, tiles)
        if first is None:
            first = (got.read(), part.clone())
            rows += [EB.compare(tag + ".g", got.read(), g, gb, axes="nvc"), EB.compare(tag + ".S1S2", part.double().sum(1), s, sb, axes="nkc"),
                     _flag(tag + ".every_row_finite", bool(torch.isfinite(part).all().item())), _kept(tag + ".rows", pflat, part.numel())] + got.untouched(tag + ".g")
        else:
            t2 = tag + (".mode1" if mm == 1 else ".again")
            rows += [EB.exact_row(t2 + ".g_same_bits", got.read(), first[0]), EB.exact_row(t2 + ".rows_same_bits", part, first[1])]
    _check(rows)


@pytest.mark.parametrize("row", EB.DROP_ROWS, ids=[r[0] for r in EB.DROP_ROWS])
def test_dropout_mask_follows_counter_site_and_seed(row):
    """Check 5: the device counter (0, 1, 2^32 + 1), the site and either half of the seed each change the mask, and every mask is the host's."""
    name, N, V, C, _ = row
    p, seed, site = EB.DROP_P, EB.DROP_SEED, EB.DROP_SITE
    x, _, rec = _drop_operands(N, V, C, 1, "bf16", "bf16")
    recd = rec.to(DEV)
    n = N * V * C
    rows, seen = [], []
    variants = [(seed, c, site) for c in EB.DROP_COUNTERS] + [(seed, 1, site + 1), (seed ^ 1, 1, site), (seed ^ (1 << 32), 1, site)]
    for sd, c, st in variants:
        fl = _flags(n)
        _drop_fwd("bf16", x, recd, 1, p, sd, _counter(c), st, fl, 2)
        host = EB.keep_tensor(sd, c, st, p, (N, V, C)).to(DEV)
        rows.append(EB.exact_row(f"dropout_mask[{name} seed{sd:#x} ctr{c} site{st}].equals_host", fl[:n].view(N, V, C), host.to(torch.uint8)))
        for k, other in enumerate(seen):
            rows.append(_flag(f"dropout_mask[{name} seed{sd:#x} ctr{c} site{st}].differs_from_variant{k}", not torch.equal(other, fl[:n])))
        seen.append(fl[:n].clone())
    _check(rows)


@pytest.mark.parametrize("row", EB.DROP_ROWS, ids=[r[0] for r in EB.DROP_ROWS])
def test_dropout_at_p0_and_p0999(row):
    """Checks 6 and 7.  p = 0: thr = 0 keeps everything and inv = 1.f / (1.f - 0.f) = 1, so `act * inv` and `dv * inv * act'` are the values of
    norm_act_fwd_kernel and norm_act_bwd_kernel (x * 1.f is exact) in the same thread mapping and the same LDS sum - no operation-order
    difference: y, g and the partial rows are compared bit for bit with bpx_norm_act_fwd / _bwd (null addend).  One exception, in the compiled
    f16 forward: there the multiply by inv and the conversion are one instruction, v_fma_mixlo_f16 (a, inv, +0), and (-0) 1 + (+0) = +0, where
    norm_act_fwd_kernel's v_cvt_pk_f16_f32 keeps -0 (GELU of a very negative u is -0).  At f16 the zeros of both are therefore compared as
    +0, every other element bit for bit.  p = 0.999: inv is about 1000; outputs finite and within bound."""
    L = _L()
    lib = L.lib
    name, N, V, C, acts = row
    act = acts[1]
    rows = []
    for kind, mode in PAIRS:
        gk, xk = EB.MODES[mode]
        x, dy, rec = _drop_operands(N, V, C, act, xk, gk)
        recd, ctr = rec.to(DEV), _counter(3)
        tiles = lib.bpx_norm_act_dropout_tiles(_dtc(mode), V, C)
        assert tiles == lib.bpx_norm_act_tiles(_dtc(mode), V, C)
        tag = f"dropout_p0[{name} act{act} {kind}/{mode}]"
        y = _drop_fwd(kind, x, recd, act, 0.0, 9, ctr, 1, None, 0)
        xb, yb = SBuf((N, V, C), kind, value=x), SBuf((N, V, C), kind)
        L.check(lib.bpx_norm_act_fwd(_dtc(kind), N, V, xb.view(), recd.data_ptr(), act, yb.view(), L.stream_ptr()))
        g, part, _ = _drop_bwd(mode, dy, x, recd, act, 0.0, 9, ctr, 1, None, 0, tiles)
        dyb, xb2, gb = SBuf((N, V, C), gk, value=dy), SBuf((N, V, C), xk, value=x), SBuf((N, V, C), gk)
        part0, _ = _rows_out(N, tiles, 2, C)
        L.check(lib.bpx_norm_act_bwd(_dtc(mode), N, V, dyb.view(), xb2.view(), recd.data_ptr(), act, L.NULL_T, gb.view(), part0.data_ptr(), L.stream_ptr()))
        _sync()
        unsign = (lambda t: torch.where(t == 0, torch.zeros_like(t), t)) if kind == "f16" else (lambda t: t)
        rows += [EB.exact_row(tag + ".y_bits_of_norm_act_fwd", unsign(y.read()), unsign(yb.read())), EB.exact_row(tag + ".g_bits_of_norm_act_bwd", g.read(), gb.read()),
                 EB.exact_row(tag + ".rows_bits_of_norm_act_bwd", part, part0)]
        p = 0.999
        keep = EB.keep_tensor(9, 3, 1, p, (N, V, C)).to(DEV)
        tag = f"dropout_p0999[{name} act{act} {kind}/{mode}]"
        y = _drop_fwd(kind, x, recd, act, p, 9, ctr, 1, None, 0)
        ref, bound = EB.dropout_fwd_reference(x.to(DEV), rec, act, kind, p, keep)
        g, part, _ = _drop_bwd(mode, dy, x, recd, act, p, 9, ctr, 1, None, 0, tiles)
        gr, gbnd, s, sb = EB.dropout_bwd_reference(dy.to(DEV), x.to(DEV), rec, act, mode, p, keep, tiles)
        rows += [EB.compare(tag + ".y", y.read(), ref, bound, axes="nvc"), EB.compare(tag + ".g", g.read(), gr, gbnd, axes="nvc"),
                 EB.compare(tag + ".S1S2", part.double().sum(1), s, sb, axes="nkc")]
    _check(rows)


def test_dropout_refusals():
    """Check 8: p = 1, p < 0, a null counter, mode 1 without a buffer and a padded tensor are refused with the entry's message."""
    L = _L()
    lib = L.lib
    N, V, C = 1, 64, 16
    x, dy, rec = _drop_operands(N, V, C, 1, "bf16", "bf16")
    recd, ctr = rec.to(DEV), _counter(1)
    xb, yb, dyb = SBuf((N, V, C), "bf16", value=x), SBuf((N, V, C), "bf16"), SBuf((N, V, C), "bf16", value=dy)
    wide = SBuf((N, V, C), "bf16", sliced=True, value=x)
    part, _ = _rows_out(N, 1, 2, C)

    def fwd(p=0.3, c=ctr.data_ptr(), mode=0, xv=None):
        return lib.bpx_norm_act_dropout_fwd(L.BF16, N, V, xv or xb.view(), recd.data_ptr(), 1, p, 1, c, 0, None, mode, yb.view(), L.stream_ptr())

    def bwd(p=0.3, c=ctr.data_ptr(), mode=0, xv=None):
        return lib.bpx_norm_act_dropout_bwd(L.BF16, N, V, dyb.view(), xv or xb.view(), recd.data_ptr(), 1, p, 1, c, 0, None, mode, yb.view(), part.data_ptr(), L.stream_ptr())

    for fn, call in (("bpx_norm_act_dropout_fwd", fwd), ("bpx_norm_act_dropout_bwd", bwd)):
        for kw, words in ((dict(p=1.0), "outside [0, 1)"), (dict(p=-0.1), "outside [0, 1)"), (dict(c=None), "step counter is null"),
                          (dict(mode=1), "needs a mask buffer"), (dict(xv=wide.view()), "dense tensors only")):
            assert call(**kw) != 0
            msg = lib.bpx_last_error().decode()
            assert fn in msg and words in msg, msg
    _sync()
    assert bool(torch.isnan(yb.read().float()).all().item()) and bool(torch.isnan(part).all().item())


# ---- the head --------------------------------------------------------------------------------------------------------------------------------
def _head_operands(N, V, Cin, Cout, kind, scale=1.0):
    gen = torch.Generator().manual_seed(100 * Cout + Cin)
    x = CB.round_to(scale * torch.randn(N, V, Cin, generator=gen), kind)
    w = (scale * torch.randn(Cout, Cin, generator=gen) / Cin ** 0.5).float()
    b = (0.3 * torch.randn(Cout, generator=gen)).float()
    dout = (0.5 + torch.randn(N, Cout, V, generator=gen)).float()
    return x, w, b, dout


class Planes:
    """(N, Cout, V) fp32 channel planes with strides sc = V + 5 and sn = Cout sc + 11: the gaps hold `gap` (7 for an output, NaN for an operand)."""

    def __init__(self, N, Cout, V, value=None):
        self.sc, self.sn = V + 5, Cout * (V + 5) + 11
        self.out = value is None
        self.flat = torch.full((N * self.sn + 16,), 7.0 if self.out else NAN, device=DEV)
        self.idx = (torch.arange(N, device=DEV)[:, None, None] * self.sn + torch.arange(Cout, device=DEV)[None, :, None] * self.sc + torch.arange(V, device=DEV)[None, None, :])
        self.flat[self.idx] = NAN if value is None else value.to(DEV)

    def read(self):
        return self.flat[self.idx]

    def gaps_kept(self, tag):
        m = torch.ones_like(self.flat, dtype=torch.bool)
        m[self.idx.reshape(-1)] = False
        return _flag(tag + ".stride_gaps_kept", bool((self.flat[m] == 7).all().item()))


def _head_fwd(kind, x, w, b, codes, N, V):
    L = _L()
    Cout, Cin = w.shape
    xb = PBuf((N, V, Cin), kind, value=x, extra=8)
    out = Planes(N, Cout, V)
    wd, bd = w.to(DEV), None if b is None else b.to(DEV)
    L.check(L.lib.bpx_head_fwd(_dtc(kind), V, N, xb.view(), wd.data_ptr(), L.ptr(bd), Cout, EB.head_code(codes), out.flat.data_ptr(), out.sn, out.sc, L.stream_ptr()))
    _sync()
    return out


def _head_fwd_rows(tag, out, x, w, b, codes, saturated):
    ref, bound, _ = EB.head_fwd_reference(x.to(DEV), w, b, codes)
    got = out.read()
    rows = [EB.compare(tag + ".out", got, ref, bound, axes="ncv"), out.gaps_kept(tag)]
    for lo, hi in EB.softmax_groups(codes):
        tot = got[:, lo:hi + 1].double().sum(1)
        rows.append(EB.compare(tag + f".group{lo}_sums_to_1", tot, torch.ones_like(tot), torch.full_like(tot, EB.softmax_sum_bound(hi - lo + 1)), axes="nv"))
    if saturated:
        sq = torch.tensor([c in (1, 3) for c in codes], device=DEV)
        g = got[:, sq]
        rows.append(_flag(tag + ".sigmoid_softmax_finite_in_0_1", bool((torch.isfinite(g) & (g >= 0) & (g <= 1)).all().item())))
    return rows


HEAD_CASES = [(co, ci, k) for co in range(1, 9) for ci in (16, 32) for k in EB.ALL]


@pytest.mark.parametrize("Cout,Cin,kind", HEAD_CASES, ids=[f"co{a}-ci{b}-{k}" for a, b, k in HEAD_CASES])
def test_head_fwd_elementwise(Cout, Cin, kind):
    """head_fwd_kernel<T, CIN, COUT> under every code set, each element against the bound of its code; a softmax group of one channel is exactly
    1; then with x and w scaled by 10 (|logit| reaches about 100): sigmoid and softmax outputs finite and in [0, 1], every group sums to 1."""
    N, V = EB.HEAD_N, EB.HEAD_VPS
    rows = []
    for scale in (1.0, 10.0):
        x, w, b, _ = _head_operands(N, V, Cin, Cout, kind, scale)
        if scale == 10.0:
            assert float(EB.head_fwd_reference(x, w, b, [0] * Cout)[0].abs().max()) > 80
        for cs in EB.HEAD_CODE_SETS:
            codes = EB.head_codes(cs, Cout)
            out = _head_fwd(kind, x, w, b if cs != "tanh" else None, codes, N, V)
            rows += _head_fwd_rows(f"head_fwd[co{Cout} ci{Cin} {kind} x{scale:g} {cs}]", out, x, w, b if cs != "tanh" else None, codes, scale == 10.0)
    _check(rows)


HEAD_WRAP_CASES = [(co, ci, k) for co, ci in EB.HEAD_FWD_WRAP for k in EB.ALL]


@pytest.mark.parametrize("Cout,Cin,kind", HEAD_WRAP_CASES, ids=[f"co{a}-ci{b}-{k}" for a, b, k in HEAD_WRAP_CASES])
def test_head_fwd_grid_wrap(Cout, Cin, kind):
    N, V = EB.HEAD_FWD_WRAP_SHAPE
    x, w, b, _ = _head_operands(N, V, Cin, Cout, kind)
    codes = EB.head_codes("mixed", Cout)
    _check(_head_fwd_rows(f"head_fwd_wrap[co{Cout} ci{Cin} {kind}]", _head_fwd(kind, x, w, b, codes, N, V), x, w, b, codes, False))


def _head_bwd(mode, x, w, dout, db0, N, V):
    """One bpx_head_bwd call: dW pre-filled with 5, db with db0 (None: a null db), dx NaN with sentinel padding channels."""
    L = _L()
    gk, xk = EB.MODES[mode]
    Cout, Cin = w.shape
    xb, dxb = PBuf((N, V, Cin), xk, value=x, extra=8), PBuf((N, V, Cin), gk, extra=8)
    do = Planes(N, Cout, V, value=dout)
    wd = w.to(DEV)
    dw, dwflat = _vec(torch.full((Cout, Cin), 5.0))
    db, dbflat = _vec(db0) if db0 is not None else (None, None)
    ws = Work(L.lib.bpx_head_bwd_workspace(Cin, Cout))
    L.check(L.lib.bpx_head_bwd(_dtc(mode), V, N, xb.view(), wd.data_ptr(), Cout, do.flat.data_ptr(), do.sn, do.sc, dxb.view(), dw.data_ptr(), L.ptr(db), ws.ptr(), ws.bytes,
                               L.stream_ptr()))
    _sync()
    return dxb, dw, dwflat, db, dbflat, ws


def _head_bwd_rows(tag, mode, Cout, Cin, N, V):
    gk, xk = EB.MODES[mode]
    x, w, _, dout = _head_operands(N, V, Cin, Cout, xk)
    x = CB.round_to(x + 0.5, xk)                                # terms of one prevailing sign: a lost row or column shows
    db0 = torch.arange(1, Cout + 1).float() * 3
    ref = EB.head_bwd_reference(x.to(DEV), w, dout.to(DEV), mode, db0)
    dxb, dw, dwflat, db, dbflat, ws = _head_bwd(mode, x, w, dout, db0, N, V)
    rows = [EB.compare(tag + ".dx", dxb.read(), *ref["dx"], axes="nvc"), EB.compare(tag + ".dw_overwritten", dw, *ref["dw"], axes="oi"),
            EB.compare(tag + ".db_added", db, *ref["db"], axes="o"), _kept(tag + ".dw", dwflat, dw.numel()), _kept(tag + ".db", dbflat, db.numel()), ws.kept(tag)]
    rows += dxb.untouched(tag + ".dx")
    dx2, dw2, _, db2, _, _ = _head_bwd(mode, x, w, dout, db0, N, V)
    rows += [EB.exact_row(tag + ".again.dx_same_bits", dx2.read(), dxb.read()), EB.exact_row(tag + ".again.dw_same_bits", dw2, dw), EB.exact_row(tag + ".again.db_same_bits", db2, db)]
    dx3, dw3, _, _, _, ws3 = _head_bwd(mode, x, w, dout, None, N, V)
    rows += [EB.exact_row(tag + ".null_db.dx_same_bits", dx3.read(), dxb.read()), EB.exact_row(tag + ".null_db.dw_same_bits", dw3, dw), ws3.kept(tag + ".null_db")]
    return rows


HEAD_BWD_CASES = [(co, ci, m) for co in range(1, 9) for ci in (16, 32) for m in EB.BWD_MODES]


@pytest.mark.parametrize("Cout,Cin,mode", HEAD_BWD_CASES, ids=[f"co{a}-ci{b}-{m}" for a, b, m in HEAD_BWD_CASES])
def test_head_bwd_elementwise(Cout, Cin, mode):
    """head_bwd_kernel<T, CIN, 1..4, TX> and head_bwd_slice_kernel<T, 5..8, TX>: dx per element with its padding channels untouched, dW
    overwritten (pre-fill 5), db added to a non-zero vector, a null db accepted, exactly bpx_head_bwd_workspace bytes used.  13 blocks of voxels:
    the sliced kernel at Cin 32 launches 16 columns, three of them empty - their rows must hold zeros (the workspace is pre-filled with NaN)."""
    _check(_head_bwd_rows(f"head_bwd[co{Cout} ci{Cin} {mode}]", mode, Cout, Cin, EB.HEAD_N, EB.HEAD_VPS))


HEAD_BWD_WRAP_CASES = [(co, ci, m) for co, ci in EB.HEAD_BWD_WRAP for m in EB.BWD_MODES]


@pytest.mark.parametrize("Cout,Cin,mode", HEAD_BWD_WRAP_CASES, ids=[f"co{a}-ci{b}-{m}" for a, b, m in HEAD_BWD_WRAP_CASES])
def test_head_bwd_grid_wrap(Cout, Cin, mode):
    _check(_head_bwd_rows(f"head_bwd_wrap[co{Cout} ci{Cin} {mode}]", mode, Cout, Cin, *EB.HEAD_BWD_WRAP_SHAPE))


# ---- the first layer -------------------------------------------------------------------------------------------------------------------------
class _Persist:
    """bpx_debug_set_c1_persist for the duration of a call, restored to its default (2048 workgroups, buffer-addressed) after it."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        _L().lib.bpx_debug_set_c1_persist(self.value)

    def __exit__(self, *a):
        _L().lib.bpx_debug_set_c1_persist(2048)


def _c1_operands(shape, kind):
    N, D, H, W, C = shape
    gen = torch.Generator().manual_seed(D + H + W + C)
    img = (0.5 + torch.randn(N, D, H, W, generator=gen)).float()
    dy = CB.round_to(0.25 + torch.randn(N, D, H, W, C, generator=gen), kind)
    return img, dy


def _c1_call(kind, shape, img, dy, db0, hook=2048, nb=None, defer=False):
    """One bpx_conv3d_c1_wgrad (nb = (mode, t, coef): bpx_conv3d_c1_wgrad_nb with dy = g) call: dW pre-filled with NaN, db with db0 (None: null)."""
    L = _L()
    lib = L.lib
    N, D, H, W, C = shape
    imgd = torch.cat([img.reshape(-1), torch.full((64,), NAN)]).to(DEV)
    dyb = PBuf(shape, kind, value=dy)
    dw, dwflat = _rows_out(C, 27)
    db, dbflat = _vec(db0) if db0 is not None else (None, None)
    ws = Work(lib.bpx_conv3d_c1_wgrad_workspace(C))
    keep = []
    with _Persist(hook):
        if defer:
            L.check(lib.bpx_wgrad_defer_begin())
        try:
            if nb is None:
                L.check(lib.bpx_conv3d_c1_wgrad(_dtc(kind), N, D, H, W, imgd.data_ptr(), dyb.view(), dw.data_ptr(), L.ptr(db), ws.ptr(), ws.bytes, L.stream_ptr()))
            else:
                mode, t, coef = nb
                tb, cd = PBuf(shape, EB.MODES[mode][1], value=t), coef.to(DEV)
                keep += [tb, cd]
                L.check(lib.bpx_conv3d_c1_wgrad_nb(_dtc(mode), N, D, H, W, imgd.data_ptr(), dyb.view(), tb.view(), cd.data_ptr(), dw.data_ptr(), L.ptr(db), ws.ptr(), ws.bytes,
                                                   L.stream_ptr()))
        finally:
            if defer:
                L.check(lib.bpx_wgrad_defer_flush(L.stream_ptr()))
        _sync()
    return dw, dwflat, db, dbflat, ws


def _c1_rows(tag, kind, kernel, shape, cap=0, nb_mode=None, defer_case=False):
    N, D, H, W, C = shape
    hook = cap if cap else 2048
    _, tiles, wgs = EB.c1_plan(kernel, N, D, H, W, persist=hook)
    db0 = torch.arange(1, C + 1).float()
    img, dy = _c1_operands(shape, kind)
    nb = None
    if nb_mode is None:
        ref = EB.c1_wgrad_reference(img.double().to(DEV), dy.to(DEV), kernel, (tiles, wgs), db0)
    else:
        gen = torch.Generator().manual_seed(7 + D + H + W + C)
        t = CB.round_to(torch.randn(N, D, H, W, C, generator=gen), EB.MODES[nb_mode][1])
        coef = torch.randn(N, C, 4, generator=gen).float() * 0.3 + 0.5
        coef = (coef * (4.0 ** torch.arange(N))[:, None, None]).float().contiguous()      # the samples' coefficients differ by factors of 4
        nb = (nb_mode, t, coef)
        dref, dbound = NB.apply_reference(dy.to(DEV), t.to(DEV), coef, None, "bf16")
        ref = EB.c1_wgrad_reference(img.double().to(DEV), dref, kernel, (tiles, wgs), db0, edy=dbound)
    dw, dwflat, db, dbflat, ws = _c1_call(kind, shape, img, dy, db0, hook, nb)
    rows = [EB.compare(tag + ".dw_overwritten", dw, *ref["dw"], axes="ot"), EB.compare(tag + ".db_added", db, *ref["db"], axes="o"), _kept(tag + ".dw", dwflat, dw.numel()),
            _kept(tag + ".db", dbflat, db.numel()), ws.kept(tag)]
    dw2, _, db2, _, _ = _c1_call(kind, shape, img, dy, db0, hook, nb)
    rows += [EB.exact_row(tag + ".again.dw_same_bits", dw2, dw), EB.exact_row(tag + ".again.db_same_bits", db2, db)]
    dw3, _, _, _, ws3 = _c1_call(kind, shape, img, dy, None, hook, nb)
    rows += [EB.exact_row(tag + ".null_db.dw_same_bits", dw3, dw), ws3.kept(tag + ".null_db")]
    if kernel == "mfma":
        dw4, _, db4, _, _ = _c1_call(kind, shape, img, dy, db0, hook | (1 << 30), nb)
        rows += [EB.exact_row(tag + ".pointer_addressed.dw_same_bits", dw4, dw), EB.exact_row(tag + ".pointer_addressed.db_same_bits", db4, db)]
    if defer_case:
        dw5, _, db5, _, _ = _c1_call(kind, shape, img, dy, db0, hook, nb, defer=True)
        rows += [EB.exact_row(tag + ".deferred.dw_same_bits", dw5, dw), EB.exact_row(tag + ".deferred.db_same_bits", db5, db)]
    return rows


C1_SCALAR_CASES = [(s, k) for s, ks in EB.C1_SCALAR_ROWS for k in ks]


@pytest.mark.parametrize("shape,kind", C1_SCALAR_CASES, ids=[f"{'x'.join(map(str, s))}-{k}" for s, k in C1_SCALAR_CASES])
def test_c1_wgrad_scalar_elementwise(shape, kind):
    """conv_c1_wgrad_kernel<T>: f32 always, bf16 where W <= 8.  D = 1, Cout 32 (blockIdx.y = 1), the 1024-column wrap, a null db; the first
    shape also inside a bpx_wgrad_defer_begin / _flush window."""
    _check(_c1_rows(f"c1_wgrad_scalar[{shape} {kind}]", kind, "scalar", shape, defer_case=shape == EB.C1_SCALAR_ROWS[0][0]))


@pytest.mark.parametrize("shape,cap", EB.C1_MFMA_ROWS, ids=["x".join(map(str, s)) + f"-cap{c}" for s, c in EB.C1_MFMA_ROWS])
def test_c1_wgrad_mfma_elementwise(shape, cap):
    """conv_c1_wgrad_mfma_kernel<uint16_t, false, BUF> at bf16, buffer- and pointer-addressed (same bits); cap 5: 54 tiles over 5 persistent
    workgroups, each crossing sample boundaries while it stages two tiles ahead."""
    _check(_c1_rows(f"c1_wgrad_mfma[{shape} cap{cap}]", "bf16", "mfma", shape, cap=cap, defer_case=cap == 5))


C1_NB_CASES = [(s, c, m) for s, c in EB.C1_MFMA_ROWS[1:] for m in ("bf16", "mix16")]


@pytest.mark.parametrize("shape,cap,mode", C1_NB_CASES, ids=["x".join(map(str, s)) + f"-cap{c}-{m}" for s, c, m in C1_NB_CASES])
def test_c1_wgrad_nb_elementwise(shape, cap, mode):
    """conv_c1_wgrad_mfma_kernel<TT, true, BUF>: dy = round_bf16(a g + b t + c0) formed on the device with per-sample coefficients that differ by
    factors of 4 - a workgroup that kept the previous sample's coefficients past a sample boundary falls outside the bound."""
    _check(_c1_rows(f"c1_wgrad_nb[{shape} cap{cap} {mode}]", "bf16", "mfma", shape, cap=cap, nb_mode=mode))


RANK1_CASES = [(t, c, k) for t in EB.RANK1_TOTALS for c in (16, 48) for k in ("f32", "bf16")]


@pytest.mark.parametrize("total,Cout,kind", RANK1_CASES, ids=[f"v{t}-c{c}-{k}" for t, c, k in RANK1_CASES])
def test_rank1_wgrad_elementwise(total, Cout, kind):
    """rank1_wgrad_kernel<T>: one voxel, one partly filled block, 12 blocks, the tail loop alone under the grid cap (262144 + 77 voxels), and one
    four-in-flight iteration followed by the tail (4 x 262144 + 1000)."""
    L = _L()
    lib = L.lib
    gen = torch.Generator().manual_seed(total % 1000 + Cout)
    img = (0.5 + torch.randn(total, generator=gen)).float()
    dy = CB.round_to(0.25 + torch.randn(total, Cout, generator=gen), kind)
    imgd = torch.cat([img, torch.full((64,), NAN)]).to(DEV)
    ref, bound = EB.rank1_reference(img.double().to(DEV), dy.to(DEV))
    tag = f"rank1_wgrad[v{total} c{Cout} {kind}]"

    def run():
        dyb = PBuf((total, Cout), kind, value=dy)
        dw, flat = _rows_out(Cout)
        ws = Work(lib.bpx_conv1x1_c1_wgrad_workspace(Cout))
        L.check(lib.bpx_conv1x1_c1_wgrad(_dtc(kind), total, imgd.data_ptr(), dyb.view(), dw.data_ptr(), ws.ptr(), ws.bytes, L.stream_ptr()))
        _sync()
        return dw, flat, ws

    dw, flat, ws = run()
    dw2, _, _ = run()
    _check([EB.compare(tag + ".dw", dw, ref, bound, axes="o"), _kept(tag, flat, dw.numel()), ws.kept(tag), EB.exact_row(tag + ".again.same_bits", dw2, dw)])

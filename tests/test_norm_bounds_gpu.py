"""The kernels between the convolutions element by element against float64 (tests/norm_bounds.py): statistics partials and the records they
give, InstanceNorm / GroupNorm backward coefficients and parameter gradients, norm_bwd_apply, the materialised norm + activation, the 1x1x1
GEMM with the IN-backward affine (tile kernel and the streaming kernel, bits equal between them) and max pooling (bit for bit).  Each row
names the kernel instance it is meant to reach and records max(|got - ref| / bound) with the position of its worst element."""
import pytest
import torch

import conv_bounds as CB
import norm_bounds as NB
from test_conv_bounds_gpu import _pack, _record_diag

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _L():
    from biapy_amd import _lib as L

    return L


def _check(rows):
    for r in rows:
        _record_diag(f"norm_bounds[{r['name']}] err/bound = {r['err']:.3e} {r['extra']}")
    bad = [r for r in rows if not r["ok"]]
    assert not bad, bad


def _flag(name, ok, extra=""):
    return dict(name=name, err=float(not ok), tol=0.0, ok=bool(ok), extra=extra)


def _dtc(mode):
    L = _L()
    return {"f32": L.F32, "bf16": L.BF16, "f16": L.F16, "mix16": L.MIX16}[mode]


class Buf:
    """An operand or output on the device: dense, or the channels [pad, pad + C) of a wider buffer whose other channels hold 7."""

    def __init__(self, shape, kind, sliced=False, value=None, pad=16):
        T = CB.TORCH_DT[kind]
        C = shape[-1]
        self.pad = pad if sliced else 0
        self.C = C
        self.buf = torch.full((*shape[:-1], C + 2 * self.pad), 7.0, dtype=T, device=DEV)
        self.buf[..., self.pad:self.pad + C] = NAN if value is None else value.to(T).to(DEV)

    def view(self):
        return _L().tview(self.buf, self.pad, self.C)

    def read(self):
        return self.buf[..., self.pad:self.pad + self.C].clone()

    def untouched(self, tag):
        if not self.pad:
            return []
        nb = torch.cat([self.buf[..., :self.pad], self.buf[..., self.pad + self.C:]], -1)
        return [_flag(tag + ".neighbours_untouched", bool((nb.float() == 7).all().item()))]


# ---- statistics partials and the records they give ----------------------------------------------------------------------------------------
# (name, kinds, voxels, ld, c0, C, fallback kinds, data).  Kernel: tensor_stats_vec_kernel where C and ld are multiples of the 16-byte vector (8
# elements at 16 bit, 4 at fp32) and the base is 16-byte aligned, else tensor_stats_kernel (one channel per lane) - `fallback` names the kinds
# that take the latter.  Data: "randn"; "bigmean" - mean = 30 x spread per channel with channel-dependent sign (it bites at f32 and f16: bf16
# values near one magnitude are multiples of one power of two and 256 of them, and their squares, sum exactly in fp32 - no evidence there);
# "const" - channel 1 constant 0.125 (v = 0 exactly: rstd is bounded through eps alone; 0.125 and its square are powers of two, so the sums
# are exact and the reference's own dv stays below (v + eps) / 2).
STATS_ROWS = [
    ("vec_dense_257", NB.KINDS, 257, 32, 0, 32, (), "randn"),
    ("vec_slice_ragged_4173", NB.KINDS, 4173, 48, 16, 16, (), "randn"),
    ("vec_c24_255", NB.KINDS, 255, 24, 0, 24, (), "randn"),
    ("vec_c40_256", NB.KINDS, 256, 40, 0, 40, (), "randn"),
    ("vec_c80_1", NB.KINDS, 1, 80, 0, 80, (), "randn"),
    ("fallback_c5", NB.KINDS, 1576, 32, 3, 5, NB.KINDS, "randn"),
    ("fallback_ld36", NB.KINDS, 300, 36, 0, 16, ("bf16", "f16"), "randn"),
    ("fallback_base_8_bytes_off", ("bf16", "f16"), 513, 32, 4, 16, ("bf16", "f16"), "randn"),
    ("vec_bigmean_1024", NB.KINDS, 1024, 32, 0, 32, (), "bigmean"),
    ("fallback_bigmean_512", NB.KINDS, 512, 32, 3, 5, NB.KINDS, "bigmean"),
    ("vec_const_channel_768", NB.KINDS, 768, 32, 0, 32, (), "const"),
    ("fallback_const_channel_768", NB.KINDS, 768, 32, 3, 5, NB.KINDS, "const"),
]
STATS_CASES = [(r, k) for r in STATS_ROWS for k in r[1]]


@pytest.mark.parametrize("row,kind", STATS_CASES, ids=[f"{r[0]}-{k}" for r, k in STATS_CASES])
def test_tensor_stats_and_records_elementwise(row, kind):
    L = _L()
    lib = L.lib
    name, _, vox, ld, c0, C, fallback, data = row
    B = 2
    es = 4 if kind == "f32" else 2
    vec = 16 // es
    wide = C % vec == 0 and ld % vec == 0 and (c0 * es) % 16 == 0
    assert wide == (kind not in fallback), "the row must reach the kernel it names"
    gen = torch.Generator().manual_seed(len(name))
    x = torch.randn(B, vox, C, generator=gen)
    if data == "bigmean":
        x = 0.1 * x + 3.0 * (1 - 2 * (torch.arange(C) % 2)).float()
    elif data == "const":
        x[..., 1] = 0.125
    x = CB.round_to(x, kind)
    buf = torch.full((B, vox, ld), 7.0, dtype=CB.TORCH_DT[kind], device=DEV)
    buf[..., c0:c0 + C] = x.to(CB.TORCH_DT[kind]).to(DEV)
    tiles = lib.bpx_tensor_stats_tiles(vox)
    part = torch.full((B, tiles, 2, C), NAN, device=DEV)
    L.check(lib.bpx_tensor_stats(_dtc(kind), B, vox, L.tview(buf, c0, C), part.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    chain = NB.tensor_stats_chain(C, kind, wide)
    xd = x.to(DEV)
    s, sb = NB.tensor_stats_reference(xd, chain)
    tag = f"tensor_stats[{name} {kind} v{vox} ld{ld} c{c0}+{C} {'vec' if wide else 'lane'}]"
    rows = [NB.compare(tag + ".sums", part.double().sum(1), s, sb, axes="nkc")]
    if vox >= 256:
        gamma, beta = 1 + 0.2 * torch.randn(C, generator=gen), 0.2 * torch.randn(C, generator=gen)
        ref, bound, ok = NB.records_from_tensor(xd, chain, vox, gamma, beta, 1e-5, 1)
        assert ok, "the reference alone must satisfy dv < (v + eps) / 2"
        gd, bd = gamma.to(DEV), beta.to(DEV)
        rec = torch.full((B, C, 4), NAN, device=DEV)
        L.check(lib.bpx_norm_finalize(part.data_ptr(), B, tiles, C, vox, gd.data_ptr(), bd.data_ptr(), 1e-5, C, rec.data_ptr(), C, 0, L.stream_ptr()))
        torch.cuda.synchronize()
        rows.append(NB.compare(tag + ".records", rec, ref, bound, axes="ncf"))
    _check(rows)


# ---- records, coefficients and parameter gradients from synthetic partials ---------------------------------------------------------------------
# (tiles, N, C, channels per group).  Tile counts: one row, fewer rows than the 64 tile lanes, each side of tile_sums' 4-row and 8-row unrolled
# loops at 64 lanes (255 / 256 / 257, 511 / 512 / 513), the benched levels (768, 1024), each side of compact_stats' 1024 threshold (1025: 32
# segments of 33 with a last one of 2) and a ragged last segment (4097).  N: NB, the samples per pass of norm_bwd_finalize_impl, is 1, 2 or 4
# depending on N and the channel block - passes with idle sample slots and N not a multiple of NB.
FIN_ROWS = ([(t, 3, 48, 1) for t in (1, 7, 255, 256, 257, 511, 512, 513, 768, 1024, 1025, 4097)] +
            [(7, n, 16, 1) for n in (1, 2, 4, 5, 17)] + [(1025, 5, 16, g) for g in (2, 4, 8, 16)] + [(257, 2, 48, g) for g in (2, 4, 8, 16)] +
            [(7, 3, 80, g) for g in (1, 2, 4, 8, 16)] + [(513, 2, 256, g) for g in (1, 32, 64)] + [(1025, 17, 256, 64)])


def _partials(N, tiles, C, gen, positive):
    p = torch.randn(N, tiles, 2, C, generator=gen)
    if positive:     # statistics rows: sum x^2 comfortably above (sum x)^2 / n, channel means that differ
        p[:, :, 0] = p[:, :, 0] * 4 + torch.randn(C, generator=gen) * 8
        p[:, :, 1] = p[:, :, 1].abs() * 8 + 260.0
    return p.float()


@pytest.mark.parametrize("tiles,N,C,cpg", FIN_ROWS, ids=[f"t{t}-N{n}-C{c}-cpg{g}" for t, n, c, g in FIN_ROWS])
def test_norm_finalize_and_bwd_finalize_elementwise(tiles, N, C, cpg):
    L = _L()
    lib = L.lib
    gen = torch.Generator().manual_seed(tiles + N + C + cpg)
    count = 256 * tiles
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=gen), 0.2 * torch.randn(C, generator=gen)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    tag = f"finalize[t{tiles} N{N} C{C} cpg{cpg}]"
    rows = []
    # forward records, into columns [16, 16 + C) of a wider record row
    part = _partials(N, tiles, C, gen, True)
    ref, bound, ok = NB.records_reference(part.to(DEV), count, gamma, beta, 1e-5, cpg)
    assert ok, "the reference alone must satisfy dv < (v + eps) / 2"
    ld = C + 32
    rec = torch.full((N, ld, 4), 7.0, device=DEV)
    rec[:, 16:16 + C] = NAN
    pd = part.to(DEV).clone()
    L.check(lib.bpx_norm_finalize(pd.data_ptr(), N, tiles, C, count, gd.data_ptr(), bd.data_ptr(), 1e-5, C // cpg, rec.data_ptr(), ld, 16, L.stream_ptr()))
    torch.cuda.synchronize()
    rows.append(NB.compare(tag + ".records", rec[:, 16:16 + C], ref, bound, axes="ncf"))
    rows.append(_flag(tag + ".records.neighbours_untouched", bool((torch.cat([rec[:, :16], rec[:, 16 + C:]], 1) == 7).all().item())))
    # backward: coefficients, dgamma / dbeta on top of a non-zero buffer
    red = _partials(N, tiles, C, gen, False)
    recs = CB.norm_recs(N, C, gen)
    recd = recs.to(DEV)
    S, d = NB.row_totals(red.to(DEV))
    cref, cbound = NB.coef_from_totals(S, d, recs, gamma, count, cpg)
    init = torch.randn(2 * C, generator=gen)

    def run(fn, window, form):
        rd = red.to(DEV).clone()
        slab = init.to(DEV).clone()                      # [dgamma | dbeta], adjacent as in the engine's gradient slab
        apart = init.to(DEV).clone()
        coef = torch.full((N, C, 4), NAN, device=DEV)
        dg, db = {"adjacent": (slab.data_ptr(), slab[C:].data_ptr()), "apart": (slab.data_ptr(), apart[C:].data_ptr()),
                  "no_dbeta": (slab.data_ptr(), None), "no_dgamma": (None, slab[C:].data_ptr())}[form]
        if window:
            L.check(lib.bpx_wgrad_defer_begin())
        try:
            L.check(fn(rd.data_ptr(), N, tiles, C, count, recd.data_ptr(), gd.data_ptr(), dg, db, C // cpg, coef.data_ptr(), L.stream_ptr()))
        finally:
            if window:
                L.check(lib.bpx_wgrad_defer_flush(L.stream_ptr()))
        torch.cuda.synchronize()
        dgam = slab[:C] if dg else None
        dbet = (slab[C:] if form != "apart" else apart[C:]) if db else None
        return coef, dgam, dbet, slab, apart

    def grad_rows(t, res, deferred, form):
        coef, dgam, dbet, slab, apart = res
        out = [NB.compare(t + ".coef", coef[..., :3], cref, cbound, axes="nck"), _flag(t + ".coef.pad_is_zero", bool((coef[..., 3] == 0).all().item()))]
        (dgr, dgb), (dbr, dbb) = NB.param_grads_from_totals(S, d, init[:C], init[C:], deferred)
        if dgam is not None:
            out.append(NB.compare(t + ".dgamma_added", dgam, dgr, dgb, axes="c"))
        else:
            out.append(_flag(t + ".dgamma_untouched", torch.equal(slab[:C].cpu(), init[:C])))
        if dbet is not None:
            out.append(NB.compare(t + ".dbeta_added", dbet, dbr, dbb, axes="c"))
        else:
            out.append(_flag(t + ".dbeta_untouched", torch.equal(slab[C:].cpu(), init[C:])))
        return out

    rows += grad_rows(tag + ".bwd", run(lib.bpx_norm_bwd_finalize, False, "adjacent"), False, "adjacent")
    if N > 1:
        for form in ("adjacent", "apart", "no_dbeta", "no_dgamma"):
            rows += grad_rows(tag + f".bwd_deferred[{form}]", run(lib.bpx_norm_bwd_finalize_deferred, True, form), True, form)
    _check(rows)


@pytest.mark.parametrize("tiles,N", [(7, 2), (1025, 3)])
def test_groupnorm_over_two_producers_elementwise(tiles, N):
    """The decoder's first GroupNorm: 8 groups over 48 = 16 + 32 channels from two producers (bpx_norm_channel_sums twice into one (N, 48, 2)
    array, then bpx_groupnorm_finalize / _bwd_finalize): groups of 6 channels, one of which straddles the two producers' columns."""
    L = _L()
    lib = L.lib
    C, cpg, count = 48, 6, 256 * tiles
    gen = torch.Generator().manual_seed(tiles)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=gen), 0.2 * torch.randn(C, generator=gen)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    tag = f"groupnorm_straddle[t{tiles} N{N}]"
    rows = []
    for positive in (True, False):
        part = _partials(N, tiles, C, gen, positive)
        sums = torch.full((N, C, 2), NAN, dtype=torch.float64, device=DEV)
        pa, pb = part[..., :16].contiguous().to(DEV), part[..., 16:].contiguous().to(DEV)
        L.check(lib.bpx_norm_channel_sums(pa.data_ptr(), N, tiles, 16, sums.data_ptr(), C, 0, L.stream_ptr()))
        L.check(lib.bpx_norm_channel_sums(pb.data_ptr(), N, tiles, 32, sums.data_ptr(), C, 16, L.stream_ptr()))
        S, d = NB.row_totals(part.to(DEV))
        if positive:
            ref, bound, ok = NB.records_from_totals(S, d, count, gamma, beta, 1e-5, cpg)
            assert ok
            rec = torch.full((N, C, 4), NAN, device=DEV)
            L.check(lib.bpx_groupnorm_finalize(sums.data_ptr(), N, C, count, gd.data_ptr(), bd.data_ptr(), 1e-5, C // cpg, rec.data_ptr(), L.stream_ptr()))
            torch.cuda.synchronize()
            rows.append(NB.compare(tag + ".channel_sums", sums.permute(0, 2, 1), S, d + NB.U64 * S.abs(), axes="nkc"))
            rows.append(NB.compare(tag + ".records", rec, ref, bound, axes="ncf"))
        else:
            recs = CB.norm_recs(N, C, gen)
            recd = recs.to(DEV)
            cref, cbound = NB.coef_from_totals(S, d, recs, gamma, count, cpg)
            init = torch.randn(2 * C, generator=gen)
            slab = init.to(DEV).clone()
            coef = torch.full((N, C, 4), NAN, device=DEV)
            L.check(lib.bpx_groupnorm_bwd_finalize(sums.data_ptr(), N, C, count, recd.data_ptr(), gd.data_ptr(), slab.data_ptr(), slab[C:].data_ptr(), C // cpg,
                                                   coef.data_ptr(), L.stream_ptr()))
            torch.cuda.synchronize()
            (dgr, dgb), (dbr, dbb) = NB.param_grads_from_totals(S, d, init[:C], init[C:], False)
            rows += [NB.compare(tag + ".coef", coef[..., :3], cref, cbound, axes="nck"), NB.compare(tag + ".dgamma_added", slab[:C], dgr, dgb, axes="c"),
                     NB.compare(tag + ".dbeta_added", slab[C:], dbr, dbb, axes="c")]
    _check(rows)


# ---- norm_bwd_apply, norm_act fwd / bwd ----------------------------------------------------------------------------------------------------
# (voxels, C, sliced operands, addend, in place)
EW_ROWS = [(1, 16, False, False, False), (100, 48, True, True, False), (720, 80, False, True, True), (720, 48, True, False, True), (100, 16, False, True, False)]
EW_CASES = [(r, m) for r in EW_ROWS for m in ("bf16", "f32", "mix16")]


def _coefs(B, C, gen):
    return (torch.randn(B, C, 4, generator=gen) * torch.tensor([1.0, 0.3, 0.03, 0.0])).float().contiguous()


@pytest.mark.parametrize("row,mode", EW_CASES, ids=[f"v{r[0]}-c{r[1]}-s{int(r[2])}a{int(r[3])}i{int(r[4])}-{m}" for r, m in EW_CASES])
def test_norm_bwd_apply_elementwise(row, mode):
    """norm_bwd_apply_kernel<T, TT>: dx = a g + b t + c0 (+ addend); in place means dx = g, as the engines call it.  B 3: sample 1 alone gives
    the same bits (the sample groups of a large batch rely on it)."""
    L = _L()
    lib = L.lib
    vox, C, sliced, addend, inplace = row
    gk, tk = NB.MODES[mode]
    B = 3
    gen = torch.Generator().manual_seed(vox + C)
    g = CB.round_to(torch.randn(B, vox, C, generator=gen), gk)
    t = CB.round_to(torch.randn(B, vox, C, generator=gen) * 2, tk)
    a = CB.round_to(torch.randn(B, vox, C, generator=gen), gk) if addend else None
    coef = _coefs(B, C, gen)

    def run(sel):
        n = g[sel].shape[0]
        gb, tb = Buf((n, vox, C), gk, sliced, g[sel]), Buf((n, vox, C), tk, sliced, t[sel])
        ab = Buf((n, vox, C), gk, sliced, a[sel]) if addend else None
        ob = gb if inplace else Buf((n, vox, C), gk, sliced)
        cd = coef[sel].contiguous().to(DEV)
        L.check(lib.bpx_norm_bwd_apply(_dtc(mode), n, vox, gb.view(), tb.view(), cd.data_ptr(), ab.view() if addend else L.NULL_T, ob.view(), L.stream_ptr()))
        torch.cuda.synchronize()
        return ob

    ob = run(slice(0, B))
    ref, bound = NB.apply_reference(g.to(DEV), t.to(DEV), coef, a.to(DEV) if addend else None, gk)
    tag = f"norm_bwd_apply[{mode} v{vox} C{C} sliced{int(sliced)} addend{int(addend)} inplace{int(inplace)}]"
    alone = run(slice(1, 2))
    _check([NB.compare(tag + ".dx", ob.read(), ref, bound, axes="nvc"), NB.exact_row(tag + ".sample1_alone_same_bits", alone.read()[0], ob.read()[1])] +
           ob.untouched(tag))


ACT_CASES = [(r, m, act) for r in EW_ROWS[:4] for m in ("bf16", "f32", "mix16") for act in range(9) if act in (1, 2, 5) or r[0] == 100]


@pytest.mark.parametrize("row,mode,act", ACT_CASES, ids=[f"v{r[0]}-c{r[1]}-{m}-act{a}" for r, m, a in ACT_CASES])
def test_norm_act_fwd_bwd_elementwise(row, mode, act):
    """norm_act_fwd_kernel (y = act(scale x + shift); storage f16 in the mixed mode's forward) and norm_act_bwd_kernel (g = dy act'(u) (+ addend),
    with its S1 / S2 rows: the sums of the fp32 product before the addend joins and before the store); in place means g = dy."""
    L = _L()
    lib = L.lib
    vox, C, sliced, addend, inplace = row
    gk, tk = NB.MODES[mode]
    B = 2
    gen = torch.Generator().manual_seed(vox + C + act)
    x = CB.round_to(torch.randn(B, vox, C, generator=gen), tk)
    dy = CB.round_to(torch.randn(B, vox, C, generator=gen), gk)
    a = CB.round_to(torch.randn(B, vox, C, generator=gen), gk) if addend else None
    rec = CB.norm_recs(B, C, gen)
    recd = rec.to(DEV)
    tag = f"norm_act[{mode} v{vox} C{C} act{act} sliced{int(sliced)} addend{int(addend)} inplace{int(inplace)}]"
    xb, yb = Buf((B, vox, C), tk, sliced, x), Buf((B, vox, C), tk, sliced)
    L.check(lib.bpx_norm_act_fwd(_dtc(tk), B, vox, xb.view(), recd.data_ptr(), act, yb.view(), L.stream_ptr()))
    torch.cuda.synchronize()
    yref, ybound = NB.norm_act_fwd_reference(x.to(DEV), rec, act, tk)
    rows = [NB.compare(tag + ".y", yb.read(), yref, ybound, axes="nvc")] + yb.untouched(tag + ".y")
    dyb = Buf((B, vox, C), gk, sliced, dy)
    ab = Buf((B, vox, C), gk, sliced, a) if addend else None
    gb = dyb if inplace else Buf((B, vox, C), gk, sliced)
    tiles = lib.bpx_norm_act_tiles(_dtc(gk), vox, C)
    red = torch.full((B, tiles, 2, C), NAN, device=DEV)
    L.check(lib.bpx_norm_act_bwd(_dtc(mode), B, vox, dyb.view(), xb.view(), recd.data_ptr(), act, ab.view() if addend else L.NULL_T, gb.view(), red.data_ptr(),
                                 L.stream_ptr()))
    torch.cuda.synchronize()
    gref, gbound, gv, egv = NB.norm_act_bwd_reference(dy.to(DEV), x.to(DEV), rec, act, a.to(DEV) if addend else None, gk)
    s, sb = NB.red_reference(gv, egv, x.to(DEV), rec, NB.norm_act_bwd_chain(vox, C, gk, tiles))
    rows += [NB.compare(tag + ".g", gb.read(), gref, gbound, axes="nvc"), NB.compare(tag + ".S1S2", red.double().sum(1), s, sb, axes="nkc")] + gb.untouched(tag + ".g")
    _check(rows)


# ---- the 1x1x1 GEMM with the IN-backward affine ---------------------------------------------------------------------------------------------
def _affine_operands(mode, B, vox, Cin, ncols, gen, bias, addend):
    gk, tk = NB.MODES[mode]
    o = dict(x=CB.round_to(torch.randn(B, vox, Cin, generator=gen), gk), w=CB.round_to(torch.randn(ncols, Cin, generator=gen) / Cin ** 0.5, gk),
             g=CB.round_to(torch.randn(B, vox, ncols, generator=gen), gk), t=CB.round_to(torch.randn(B, vox, ncols, generator=gen) * 2, tk),
             coef=_coefs(B, ncols, gen), bias=(torch.randn(ncols, generator=gen) * 0.1).float() if bias else None,
             addend=CB.round_to(torch.randn(B, vox, ncols, generator=gen), gk) if addend else None)
    return o


def _run_affine(mode, o, B, vox, S, split, planar, wgrad=False, sel=None):
    """One bpx_conv1x1_fwd / _fwd_split / _fwd_split_wgrad call; returns (y (B, vox, ncols), dw or None)."""
    L = _L()
    lib = L.lib
    gk, tk = NB.MODES[mode]
    sel = slice(0, B) if sel is None else sel
    T, TT = CB.TORCH_DT[gk], CB.TORCH_DT[tk]
    ncols, Cin = o["w"].shape
    n = o["x"][sel].shape[0]
    xd, gd = o["x"][sel].to(T).to(DEV).contiguous(), o["g"][sel].to(T).to(DEV).contiguous()
    td = o["t"][sel].to(TT).to(DEV).contiguous()
    tp = L.Planar(n, S, ncols, TT, DEV).copy_from_dense(td.view(n, *S, ncols)) if planar else None
    tv = L.tview(tp) if planar else L.tview(td)
    cd = o["coef"][sel].contiguous().to(DEV)
    bd = o["bias"].to(DEV) if o["bias"] is not None else None
    ad = o["addend"][sel].to(T).to(DEV).contiguous() if o["addend"] is not None else None
    wp = _pack(o["w"].view(ncols, Cin, 1, 1, 1), L.PK_DENSE, Cin, ncols, gk)
    dw = None
    if not split:
        y = torch.full((n, vox, ncols), NAN, dtype=T, device=DEV)
        L.check(lib.bpx_conv1x1_fwd(_dtc(mode), n, vox, L.tview(xd), wp.data_ptr(), L.ptr(bd), L.tview(gd), tv, cd.data_ptr(), L.tview(ad), L.tview(y), L.stream_ptr()))
        torch.cuda.synchronize()
        return y, None
    lo = torch.full((n, vox, split), NAN, dtype=T, device=DEV)
    hi = torch.full((n, vox, ncols - split), NAN, dtype=T, device=DEV)
    if wgrad:
        need = int(lib.bpx_conv1x1_fwd_split_wgrad_workspace(_dtc(mode), n, vox, Cin))
        assert need > 0
        dw = torch.full((Cin, ncols), NAN, device=DEV)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        L.check(lib.bpx_conv1x1_fwd_split_wgrad(_dtc(mode), n, vox, L.tview(xd), wp.data_ptr(), L.tview(gd), tv, cd.data_ptr(), L.tview(lo), L.tview(hi), dw.data_ptr(),
                                                ws.data_ptr(), ws.numel(), L.stream_ptr()))
    else:
        L.check(lib.bpx_conv1x1_fwd_split(_dtc(mode), n, vox, L.tview(xd), wp.data_ptr(), L.ptr(bd), L.tview(gd), tv, cd.data_ptr(), L.tview(ad), L.tview(lo), L.tview(hi),
                                          L.stream_ptr()))
    torch.cuda.synchronize()
    return torch.cat([lo, hi], -1), dw


def _affine_ref(o, gk):
    d = lambda v: None if v is None else v.to(DEV)
    return NB.affine_reference(d(o["x"]), d(o["w"]), d(o["g"]), d(o["t"]), o["coef"], addend=d(o["addend"]), bias=d(o["bias"]), out_kind=gk)


PW_CASES = [(r, m) for r in NB.PW_ROWS for m in r[1]]


@pytest.mark.parametrize("row,mode", PW_CASES, ids=[f"{r[0]}-{m}" for r, m in PW_CASES])
def test_conv1x1_affine_tile_kernel_elementwise(row, mode):
    """pw_kernel<T, MS, NS, PW_CONV1, PL, TT> with the affine: NS 1 .. 4 (16 .. 64 columns per workgroup), voxel counts around the 128-voxel block,
    bias, addend, the split at 16 / 32 / 48 / 64 columns, chunk-planar t."""
    name, _, B, vox, Cin, ncols, split, bias, addend, planar = row
    gk, _ = NB.MODES[mode]
    gen = torch.Generator().manual_seed(len(name) + vox)
    o = _affine_operands(mode, B, vox, Cin, ncols, gen, bias, addend)
    y, _ = _run_affine(mode, o, B, vox, (1, 1, vox), split, planar)
    ref, bound = _affine_ref(o, gk)
    tag = f"conv1x1_affine[{name} {mode} B{B} v{vox} {Cin}->{ncols} split{split} bias{int(bias)} addend{int(addend)} planar{int(planar)}]"
    rows = [NB.compare(tag + ".y", y, ref, bound, axes="nvc")]
    if B > 1:
        alone, _ = _run_affine(mode, o, B, vox, (1, 1, vox), split, planar, sel=slice(1, 2))
        rows.append(NB.exact_row(tag + ".sample1_alone_same_bits", alone[0], y[1]))
    _check(rows)


PWS_CASES = [(r, m, p) for r in NB.PWS_ROWS for m in ("bf16", "mix16") for p in (False, True)]


@pytest.mark.parametrize("row,mode,planar", PWS_CASES, ids=[f"{r[0]}-{m}-planar{int(p)}" for r, m, p in PWS_CASES])
def test_conv1x1_affine_streaming_kernel_elementwise(row, mode, planar):
    """pw_nbs_kernel<KC, TV, TT, WG> (NB.PWS_ROWS: walks of unequal length, sample boundaries inside walks, the smallest admitted volume, B 1
    and B 5) against the fp64 expression element by element; bits equal to the tile kernel (bpx_debug_set_pw_stream(0)); with the shortcut weight
    gradient riding along (WG) the outputs keep their bits and dWsc meets its own bound."""
    L = _L()
    lib = L.lib
    name, K, B, vps = row
    gk, _ = NB.MODES[mode]
    gen = torch.Generator().manual_seed(K + B)
    o = _affine_operands(mode, B, vps, K, 3 * K, gen, False, False)
    S = (vps // 64, 8, 8)
    split = 2 * K
    y, _ = _run_affine(mode, o, B, vps, S, split, planar)
    lib.bpx_debug_set_pw_stream(0)
    try:
        ytile, _ = _run_affine(mode, o, B, vps, S, split, planar)
    finally:
        lib.bpx_debug_set_pw_stream(1)
    ywg, dw = _run_affine(mode, o, B, vps, S, split, planar, wgrad=True)
    ref, bound = _affine_ref(o, gk)
    nblocks, _ = NB.pws_blocks(K, B, vps)
    dref, dbound = NB.pws_wgrad_reference(o["t"].to(DEV), o["x"].to(DEV), mode == "mix16", nblocks)
    tag = f"conv1x1_affine_stream[{name} {mode} planar{int(planar)}]"
    _check([NB.compare(tag + ".y", y, ref, bound, axes="nvc"), NB.exact_row(tag + ".same_bits_as_tile_kernel", y, ytile),
            NB.exact_row(tag + ".wgrad_form_same_output_bits", ywg, y), NB.compare(tag + ".dWsc", dw, dref, dbound, axes="oi")])


# ---- pooling: bit for bit --------------------------------------------------------------------------------------------------------------------
# (sz, mode, C, S, x layout, sliced dy / addend / dx, in place).  x layouts: dense, planar (chunk-planar), slice (channels [16, 16 + C) of a wider dense
# buffer), planar_slice (the same of a chunk-planar buffer: the engines pass tview(cat[i], Cup, fm[i])).  In place: addend and dx are one buffer, as
# every engine calls it.  (2, 2, 2) / (1, 2, 2): the smallest volume; (4, 6, 10) at C 48 / 80: an item count that is not a multiple of the block.
POOL_ROWS = [(2, "bf16", 16, (2, 2, 2), "dense", False, True), (1, "bf16", 16, (1, 2, 2), "dense", False, False),
             (2, "mix16", 48, (4, 6, 10), "planar", True, True), (1, "mix16", 80, (4, 6, 10), "slice", True, False),
             (2, "f32", 96, (4, 6, 10), "dense", False, True), (1, "f32", 48, (3, 6, 10), "slice", True, True),
             (2, "bf16", 80, (8, 12, 20), "planar_slice", False, True), (1, "bf16", 96, (4, 6, 10), "planar", True, True),
             (2, "mix16", 16, (8, 12, 20), "planar_slice", True, True), (1, "mix16", 32, (5, 8, 8), "dense", False, False)]


def _place_x(x, layout):
    L = _L()
    B, D, H, W, C = x.shape
    if layout.startswith("planar"):
        off = 16 if layout == "planar_slice" else 0
        p = L.Planar(B, (D, H, W), C + off, x.dtype, DEV)
        p._flat.fill_(7.0)
        full = torch.full((B, D, H, W, C + off), 7.0, dtype=x.dtype, device=DEV)
        full[..., off:] = x.to(DEV)
        p.copy_from_dense(full)
        return L.tview(p, off, C), p
    off = 16 if layout == "slice" else 0
    buf = torch.full((B, D, H, W, C + 2 * off), 7.0, dtype=x.dtype, device=DEV)
    buf[..., off:off + C] = x.to(DEV)
    return L.tview(buf, off, C), buf


@pytest.mark.parametrize("row", POOL_ROWS, ids=[f"sz{r[0]}-{r[1]}-c{r[2]}-{'x'.join(map(str, r[3]))}-{r[4]}-s{int(r[5])}i{int(r[6])}" for r in POOL_ROWS])
def test_maxpool_fwd_bwd_bit_for_bit(row):
    """maxpool_fwd_kernel<T> (storage f16 in the mixed mode's forward) and maxpool_bwd_kernel<T, TX, SZ, ADD>: exactly specified operations, compared
    bit for bit; the statistics rows of the forward against their own bound."""
    L = _L()
    lib = L.lib
    sz, mode, C, S, layout, sliced, inplace = row
    gk, tk = NB.MODES[mode]
    B = 2
    D, H, W = S
    gen = torch.Generator().manual_seed(C + sz)
    x, dy, add = NB.pool_inputs(B, S, C, sz, CB.TORCH_DT[tk], CB.TORCH_DT[gk], gen)
    winners, tied = NB.pool_tie_stats(x, sz)
    if D * H * W >= 64:
        assert winners == set(range(4 * sz)) and tied > 0.5, (winners, tied)
    tag = f"maxpool[sz{sz} {mode} C{C} {S} x={layout} sliced{int(sliced)} inplace{int(inplace)}]"
    xv, xkeep = _place_x(x, layout)
    Do, Ho, Wo = D // sz, H // 2, W // 2
    yb = Buf((B, Do, Ho, Wo, C), tk, sliced)
    tiles = lib.bpx_maxpool3d_stats_tiles(_dtc(tk), D, H, W, sz, C)
    part = torch.full((B, tiles, 2, C), NAN, device=DEV)
    L.check(lib.bpx_maxpool3d_fwd(_dtc(tk), B, D, H, W, sz, xv, yb.view(), part.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    yref, _ = NB.pool_fwd_reference(x, sz)
    s, sb = NB.pool_stats_reference(yref.double().to(DEV), C, tk)
    rows = [NB.exact_row(tag + ".y", yb.read(), yref), NB.compare(tag + ".stats", part.double().sum(1), s, sb, axes="nkc")] + yb.untouched(tag + ".y")
    for with_add in (True, False):
        dyb = Buf((B, Do, Ho, Wo, C), gk, sliced, dy)
        ab = Buf((B, D, H, W, C), gk, sliced, add) if with_add else None
        ob = ab if (inplace and with_add) else Buf((B, D, H, W, C), gk, sliced)
        L.check(lib.bpx_maxpool3d_bwd(_dtc(mode), B, D, H, W, sz, xv, dyb.view(), ab.view() if with_add else L.NULL_T, ob.view(), L.stream_ptr()))
        torch.cuda.synchronize()
        ref = NB.pool_bwd_reference(x, dy, add if with_add else None, sz)
        rows += [NB.exact_row(tag + f".dx[addend{int(with_add)}]", ob.read(), ref)] + ob.untouched(tag + f".dx[addend{int(with_add)}]")
    _check(rows)


@pytest.mark.parametrize("sz,mode,S", [(2, "bf16", (64, 64, 64)), (1, "mix16", (32, 64, 64))])
def test_maxpool_bwd_r1_same_bits_and_rank1_gradient(sz, mode, S):
    """maxpool_bwd_kernel<.., R1> at its admitted shapes (C 16, >= 65536 items): the dx bits of bpx_maxpool3d_bwd, in place, and dWsc[co] =
    sum_v img[v] dx[v][co] over the stored dx against its bound."""
    L = _L()
    lib = L.lib
    gk, tk = NB.MODES[mode]
    B, C = 1, 16
    D, H, W = S
    gen = torch.Generator().manual_seed(sz)
    x, dy, add = NB.pool_inputs(B, S, C, sz, CB.TORCH_DT[tk], CB.TORCH_DT[gk], gen)
    img = torch.randn(B, D, H, W, generator=gen)
    need = int(lib.bpx_maxpool3d_bwd_r1_workspace(_dtc(mode), B, D, H, W, sz, C))
    assert need > 0
    xd, dyd, imgd = x.to(DEV), dy.to(DEV), img.to(DEV)
    ab = Buf((B, D, H, W, C), gk, False, add)
    dw = torch.full((C,), NAN, device=DEV)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    L.check(lib.bpx_maxpool3d_bwd_r1(_dtc(mode), B, D, H, W, sz, L.tview(xd), L.tview(dyd), ab.view(), ab.view(), imgd.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws.numel(),
                                     L.stream_ptr()))
    torch.cuda.synchronize()
    ref = NB.pool_bwd_reference(x, dy, add, sz)
    items = B * (D // sz) * (H // 2) * (W // 2) * 2
    grid = need // 64
    wref, wbound = NB.pool_r1_reference(ref.to(DEV), imgd, items, 4 * sz, grid)
    tag = f"maxpool_bwd_r1[sz{sz} {mode} {S}]"
    _check([NB.exact_row(tag + ".dx", ab.read(), ref), NB.compare(tag + ".dWsc", dw, wref, wbound, axes="o")])

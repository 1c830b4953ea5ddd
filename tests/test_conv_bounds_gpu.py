"""The conv kernels element by element against float64 (tests/conv_bounds.py): every forward route of bpx_conv3d_fwd / _fwd_pool at f32, bf16
and f16 (the lean kernel with several output-channel workgroups included), batch independence of a sample's bits, bpx_conv3d_fwd_shuffle (the
RCAN up-scaling stage: the lean kernel's pixel-shuffle store, inside guard bands, against the unfused launch, and what the entry refuses), the
first-layer / 1x1 / transposed-conv forwards at f16, the input gradient at f32, bf16 and MIX16 with its S1 / S2 rows, the weight gradients (the
up-scaling stage's 128- and 48-channel shapes of both included), and the fused backward's g, S1 / S2 rows, dW and db.  Each row records max(|got - ref| / bound) and the position of its worst element."""
import pytest
import torch

import conv_bounds as CB
import kernel_checks
import norm_bounds as NB

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {"f32": 0, "bf16": 1, "f16": 2}


def _record_diag(line):
    """Measured values, recorded beside those of the other parity tests by their own recorder (test_gpu_parity._record_diag)."""
    print(line)
    try:
        from test_gpu_parity import _record_diag as record
    except ImportError:
        return
    record(line)


def _check(rows):
    for r in rows:
        _record_diag(f"conv_bounds[{r['name']}] err/bound = {r['err']:.3e} {r['extra']}")
    bad = [r for r in rows if not r["ok"]]
    assert not bad, bad


def _L():
    from biapy_amd import _lib as L

    return L


def _pack(w, mode, cin, cout, kind):
    L = _L()
    dt = DT[kind]
    n = L.lib.bpx_packed_weight_elems(mode, cin, cout, dt)
    out = torch.empty(n, dtype=CB.TORCH_DT[kind], device=DEV)
    wd = w.float().contiguous().to(DEV)
    L.check(L.lib.bpx_pack_weight(mode, wd.data_ptr(), cin, cout, dt, out.data_ptr(), L.stream_ptr()))
    return out


_recs = CB.norm_recs


def _nan(shape, kind):
    return torch.full(shape, float("nan"), dtype=CB.TORCH_DT[kind], device=DEV)


class _Hooks:
    """Route hooks of a table row, set for the duration of a call and restored to their defaults after it."""

    def __init__(self, row):
        self.row = row

    def __enter__(self):
        lib = _L().lib
        lib.bpx_debug_set_conv_ws(self.row["ws"])
        lib.bpx_debug_set_conv_kg(self.row["kg"])
        lib.bpx_debug_set_conv_zm(self.row["zm"])
        lib.bpx_debug_set_conv_occ(self.row["occ"])
        return self

    def __exit__(self, *a):
        lib = _L().lib
        lib.bpx_debug_set_conv_ws(0)
        lib.bpx_debug_set_conv_kg(-1)
        lib.bpx_debug_set_conv_zm(-1)
        lib.bpx_debug_set_conv_occ(0)


def _operands(row, kind, seed):
    B, (D, H, W), Cin, Cout = row["B"], row["S"], row["Cin"], row["Cout"]
    g = torch.Generator().manual_seed(seed)
    o = dict(x=CB.round_to(torch.randn(B, D, H, W, Cin, generator=g), kind),
             w=CB.round_to(torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5, kind),
             b=(torch.randn(Cout, generator=g) * 0.1).float(), rec=_recs(B, Cin, g) if row["act"] else None, sc=None, wsc=None, bsc=None)
    if row["sc"] == 1:
        o.update(sc=torch.randn(B, D, H, W, generator=g).double(), wsc=torch.randn(Cout, generator=g).double(), bsc=torch.randn(Cout, generator=g) * 0.1)
    elif row["sc"]:
        o.update(sc=CB.round_to(torch.randn(B, D, H, W, row["sc"], generator=g), kind),
                 wsc=CB.round_to(torch.randn(Cout, row["sc"], generator=g) / row["sc"] ** 0.5, kind), bsc=torch.randn(Cout, generator=g) * 0.1)
    return o


def _place(t, kind, layout, extra=16):
    """A stored operand on the device in the row's layout; returns (bpx_tensor, keep-alive, reader of the C channels as dense NDHWC)."""
    L = _L()
    T = CB.TORCH_DT[kind]
    C = t.shape[-1]
    if layout == "planar":
        p = L.Planar(t.shape[0], t.shape[1:4], C, T, DEV).copy_from_dense(t.to(T).to(DEV))
        return L.tview(p), p, p.dense
    if layout == "slice":
        buf = torch.zeros(*t.shape[:-1], C + 2 * extra, dtype=T, device=DEV)
        buf[..., extra:extra + C] = t.to(T).to(DEV)
        return L.tview(buf, extra, C), buf, lambda: buf[..., extra:extra + C]
    d = t.to(T).to(DEV).contiguous()
    return L.tview(d), d, lambda: d


def _out(shape, kind, layout, extra=16):
    """A NaN-filled output in the row's layout: (bpx_tensor, keep-alive, dense reader, reader of the neighbouring channels or None)."""
    L = _L()
    T = CB.TORCH_DT[kind]
    C = shape[-1]
    if layout == "planar":
        p = L.Planar(shape[0], shape[1:4], C, T, DEV)
        p._flat.fill_(float("nan"))
        return L.tview(p), p, p.dense, None
    if layout == "slice":
        buf = torch.full((*shape[:-1], C + 2 * extra), 7.0, dtype=T, device=DEV)
        buf[..., extra:extra + C] = float("nan")
        return L.tview(buf, extra, C), buf, lambda: buf[..., extra:extra + C], lambda: torch.cat([buf[..., :extra], buf[..., extra + C:]], -1)
    d = _nan(shape, kind)
    return L.tview(d), d, lambda: d, None


def _run_fwd(row, kind, o, B):
    """One bpx_conv3d_fwd(_pool) call of the row on the first B samples of the operands; returns the dense outputs."""
    L = _L()
    lib, dt = L.lib, DT[kind]
    D, H, W = row["S"]
    Cout = row["Cout"]
    xv, xk, _ = _place(o["x"][:B], kind, row["layout"])
    yv, yk, yread, nb = _out((B, D, H, W, Cout), kind, row["layout"])
    wp = _pack(o["w"], L.PK_K3, row["Cin"], Cout, kind)
    recd = o["rec"][:B].contiguous().to(DEV) if o["rec"] is not None else None
    bd = o["b"].to(DEV)
    sct, wscp, bscd, keep = L.NULL_T, None, None, []
    if row["sc"] == 1:
        img = o["sc"][:B].float().contiguous().to(DEV)
        w1 = o["wsc"].float().contiguous().to(DEV)
        sct, wscp, keep = L.Tensor(img.data_ptr(), 1, 1), w1.data_ptr(), [img, w1]
    elif row["sc"]:
        sct, sk, _ = _place(o["sc"][:B], kind, row["layout"] if row["layout"] == "planar" else "dense")
        wk = _pack(o["wsc"].view(Cout, row["sc"], 1, 1, 1), L.PK_K1, row["sc"], Cout, kind)
        wscp, keep = wk.data_ptr(), [sk, wk]
    if o["bsc"] is not None:
        bscd = o["bsc"].float().to(DEV)
    tiles = lib.bpx_conv3d_stats_tiles(dt, B, D, H, W, Cout)
    part = torch.full((B, tiles, 2, Cout), float("nan"), device=DEV)
    act = row["act"]
    with _Hooks(row):
        n0 = lib.bpx_debug_conv_zm_launches()
        if row["pool"]:
            sz = row["pool"]
            pooled = _nan((B, D // sz, H // 2, W // 2, Cout), kind)
            ppart = torch.full((B, tiles, 2, Cout), float("nan"), device=DEV)
            L.check(lib.bpx_conv3d_fwd_pool(dt, B, D, H, W, xv, L.ptr(recd), act, wp.data_ptr(), bd.data_ptr(), sct, wscp, L.ptr(bscd), yv,
                                            part.data_ptr(), sz, L.tview(pooled), ppart.data_ptr(), L.stream_ptr()))
        else:
            pooled = None
            L.check(lib.bpx_conv3d_fwd(dt, B, D, H, W, xv, L.ptr(recd), act, wp.data_ptr(), bd.data_ptr(), sct, wscp, L.ptr(bscd), yv, part.data_ptr(),
                                       L.stream_ptr()))
        torch.cuda.synchronize()
        zm_ran = lib.bpx_debug_conv_zm_launches() - n0
    return dict(y=yread().clone(), part=part, pooled=pooled, zm_ran=zm_ran, neighbours=nb() if nb else None)


def _row_id(row, kind):
    return f"{row['name']} {kind} B{row['B']} {row['S']} {row['Cin']}->{row['Cout']} act{row['act']} sc{row['sc']} {row['layout']}"


FWD_CASES = [(r, k) for r in CB.FWD_ROUTES for k in r["kinds"]]


@pytest.mark.parametrize("row,kind", FWD_CASES, ids=[f"{r['name']}-{k}" for r, k in FWD_CASES])
def test_conv3d_fwd_elementwise(row, kind):
    o = _operands(row, kind, seed=len(row["name"]) + DT[kind])
    tile_vox = row["cfg"][0] * row["cfg"][1] * row["cfg"][2]
    got = _run_fwd(row, kind, o, row["B"])
    dev = lambda t: None if t is None else t.to(DEV)
    ref, bound, pre = CB.fwd_reference(o["x"].to(DEV), o["w"].to(DEV), o["b"].to(DEV), kind, rec=dev(o["rec"]), act=row["act"], sc=dev(o["sc"]),
                                       wsc=dev(o["wsc"]), bsc=dev(o["bsc"]))
    tag = _row_id(row, kind)
    rows = [CB.compare(tag + ".y", got["y"], ref, bound)]
    s, sb = CB.stats_reference(ref, pre, tile_vox)
    rows.append(CB.compare(tag + ".stats", got["part"].double().sum(1), s, sb, axes="nkc"))
    if row["pool"]:
        sz = row["pool"]
        mp = lambda t: torch.nn.functional.max_pool3d(t.permute(0, 4, 1, 2, 3), (sz, 2, 2)).permute(0, 2, 3, 4, 1)
        pb = mp(bound)      # |max a - max b| <= max |a - b| over the window
        rows.append(CB.compare(tag + ".pooled", got["pooled"], mp(ref), pb))
        same = torch.equal(got["pooled"].double(), mp(got["y"].double()))
        rows.append(dict(name=tag + ".pooled_is_max_of_stored_y", err=0.0 if same else 1.0, tol=0.0, ok=same, extra=""))
    if row["zm"]:
        rows.append(dict(name=tag + ".zmarch_kernel_ran", err=float(got["zm_ran"] != 1), tol=0.0, ok=got["zm_ran"] == 1, extra=f"launches {got['zm_ran']}"))
    if got["neighbours"] is not None:
        ok = bool((got["neighbours"].float() == 7).all().item())
        rows.append(dict(name=tag + ".neighbours_untouched", err=float(not ok), tol=0.0, ok=ok, extra=""))
    if row["B"] == 3:   # a sample's bits must not depend on the batch it travels in (use_lean; the sharded sliding window relies on it)
        one = {k: (v[1:2] if v is not None and k in ("x", "sc") else v) for k, v in o.items()}
        if one["rec"] is not None:
            one["rec"] = o["rec"][1:2]
        alone = _run_fwd(row, kind, one, 1)
        same = torch.equal(alone["y"][0].contiguous().view(torch.uint8), got["y"][1].contiguous().view(torch.uint8))
        rows.append(dict(name=tag + ".sample1_alone_same_bits", err=float(not same), tol=0.0, ok=same, extra=""))
    _check(rows)


# ---- the fused conv + 3-D pixel shuffle: bpx_conv3d_fwd_shuffle ----------------------------------------------------------------------------------
SENTINEL = 0x7FC1      # a NaN of bf16 and of f16 alike, with a payload no kernel produces: an element never written fails as non-finite
GUARD = 4096           # elements of the guard band in front of and behind an output (8 KB: the view's base keeps the allocation's alignment)


def _guarded(nbytes):
    """An output of nbytes inside a larger sentinel-filled allocation: (whole int16 buffer, int16 view of the output)."""
    n = nbytes // 2
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
    y = buf[GUARD:GUARD + n]
    assert y.data_ptr() % 16 == 0
    return buf, y


def _guards_untouched(buf):
    return bool((buf[:GUARD] == SENTINEL).all().item() and (buf[-GUARD:] == SENTINEL).all().item())


def _shuffle_operands(row, kind):
    """Stored operands of a SHUFFLE_ROWS row: the weight and bias are drawn in PyTorch's [channel][sub-position] order and re-ordered the way
    RCANEngine does it."""
    from biapy_amd.rcan_engine import rows_to_subposition_major

    B, (D, H, W), Cin, s3 = row["B"], row["S"], row["Cin"], row["s"] ** 3
    g = torch.Generator().manual_seed(100 + len(row["name"]) + DT[kind])
    x = CB.round_to(torch.randn(B, D, H, W, Cin, generator=g), kind)
    w = CB.round_to(torch.randn(16 * s3, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5, kind)
    b = (torch.randn(16 * s3, generator=g) * 0.1).float()
    wu, bu = rows_to_subposition_major(w, b, 16, s3)
    return dict(x=x, wu=wu, bu=bu, rec=_recs(B, Cin, g) if row["act"] else None)


def _run_shuffle(row, kind, o, lo, hi, unfused):
    """bpx_conv3d_fwd_shuffle on samples lo..hi-1 of the operands, into a guarded view; with `unfused` also bpx_conv3d_fwd of the same operands
    (Cout = 16 s^3, same packed weight) whose stored tensor, permuted here, must hold the same bits."""
    L = _L()
    lib, dt, T = L.lib, DT[kind], CB.TORCH_DT[kind]
    (D, H, W), Cin, s = row["S"], row["Cin"], row["s"]
    B, Cout = hi - lo, 16 * s ** 3
    xd = o["x"][lo:hi].to(T).to(DEV).contiguous()
    wp = _pack(o["wu"], L.PK_K3, Cin, Cout, kind)
    bd = o["bu"].to(DEV)
    recd = o["rec"][lo:hi].contiguous().to(DEV) if o["rec"] is not None else None
    buf, y = _guarded(B * D * H * W * Cout * 2)
    L.check(lib.bpx_conv3d_fwd_shuffle(dt, B, D, H, W, L.tview(xd), L.ptr(recd), row["act"], wp.data_ptr(), bd.data_ptr(), s, L.Tensor(y.data_ptr(), 16, 16, 0),
                                       L.stream_ptr()))
    torch.cuda.synchronize()
    out = dict(y=y.view(T).view(B, D * s, H * s, W * s, 16), guards=_guards_untouched(buf), keep=buf)
    if unfused:
        yu = _nan((B, D, H, W, Cout), kind)
        L.check(lib.bpx_conv3d_fwd(dt, B, D, H, W, L.tview(xd), L.ptr(recd), row["act"], wp.data_ptr(), bd.data_ptr(), L.NULL_T, None, None, L.tview(yu), None,
                                   L.stream_ptr()))
        torch.cuda.synchronize()
        out["same_as_unfused"] = torch.equal(CB.shuffle_to_fine_grid(yu, s).contiguous().view(torch.int16), out["y"].view(torch.int16))
    return out


SHUFFLE_CASES = [(r, k) for r in CB.SHUFFLE_ROWS for k in r["kinds"]]


@pytest.mark.parametrize("row,kind", SHUFFLE_CASES, ids=[f"{r['name']}-{k}" for r, k in SHUFFLE_CASES])
def test_conv3d_fwd_shuffle_elementwise(row, kind):
    """The RCAN up-scaling stage's forward at its own entry: every element of the (B, sD, sH, sW, 16) output against the fp64 conv moved to the
    fine grid (conv_bounds.shuffle_reference), on volumes with edge tiles on every axis, B > 1, a prologue, 32 input channels and byte offsets
    up to 2^31; nothing outside the output written; the same bits as the unfused lean launch, and as the sample run alone."""
    o = _shuffle_operands(row, kind)
    B, sel = row["B"], row["samples"]
    got = _run_shuffle(row, kind, o, 0, B, unfused=sel is None)
    idx = list(range(B)) if sel is None else list(sel)
    pick = lambda t: None if t is None else t[idx].to(DEV)
    ref, bound, _ = CB.shuffle_reference(pick(o["x"]), o["wu"].to(DEV), o["bu"].to(DEV), kind, row["s"], rec=pick(o["rec"]), act=row["act"])
    tag = f"shuffle[{row['name']} {kind} B{B} {row['S']} {row['Cin']}->16 x{row['s']} act{row['act']}]"
    rows = [CB.compare(tag + ".y", got["y"][idx], ref, bound)]
    if sel is not None:      # the samples that are not compared element by element: at least written, every element
        left = int((got["y"].view(torch.int16) == SENTINEL).sum().item())
        rows.append(dict(name=tag + ".every_sample_written", err=float(left), tol=0.0, ok=left == 0, extra=f"elements still holding the pre-fill {left}"))
    rows.append(dict(name=tag + ".guards_untouched", err=float(not got["guards"]), tol=0.0, ok=got["guards"], extra=""))
    if sel is None:
        same = got["same_as_unfused"]
        rows.append(dict(name=tag + ".is_permutation_of_unfused", err=float(not same), tol=0.0, ok=same, extra=""))
    if row["name"] == "x2_ragged":
        alone = _run_shuffle(row, kind, o, 1, 2, unfused=False)
        same = torch.equal(alone["y"][0].view(torch.int16), got["y"][1].view(torch.int16))
        rows.append(dict(name=tag + ".sample1_alone_same_bits", err=float(not same), tol=0.0, ok=same, extra=""))
    _check(rows)


# (name, dtype code, N, S, Cin, s, y.C = y.ld): what bpx_conv3d_fwd_shuffle must refuse.  Every buffer has the size the call would need if it
# were accepted (x, the packed weight and bias of 16 s^3 rows, y with its guard bands), so a missing check shows as a written y or a zero return
# code and never as an access outside an allocation.
SHUFFLE_REFUSALS = [("s1", 1, 1, (32, 32, 32), 16, 1, 16), ("s5", 1, 1, (32, 32, 32), 16, 5, 16), ("f32", 0, 1, (32, 32, 32), 16, 2, 16),
                    ("yC32", 1, 1, (32, 32, 32), 16, 2, 32), ("W8", 1, 1, (64, 64, 8), 16, 2, 16), ("vol_16x32x32", 1, 1, (16, 32, 32), 16, 2, 16),
                    ("out_2pow30", 1, 32, (32, 32, 32), 16, 4, 16)]


@pytest.mark.parametrize("case", SHUFFLE_REFUSALS, ids=[c[0] for c in SHUFFLE_REFUSALS])
def test_conv3d_fwd_shuffle_refuses(case):
    L = _L()
    lib = L.lib
    _, dt, N, (D, H, W), Cin, s, yC = case
    es = 4 if dt == L.F32 else 2
    T = torch.float32 if dt == L.F32 else torch.bfloat16
    Cout = 16 * s ** 3
    x = torch.zeros((N, D, H, W, Cin), dtype=T, device=DEV)
    wp = torch.zeros(max(int(lib.bpx_packed_weight_elems(L.PK_K3, Cin, Cout, dt)), (Cin // 16) * 56 * 8 * Cout), dtype=T, device=DEV)
    bias = torch.zeros(Cout, device=DEV)
    buf, y = _guarded(N * D * H * W * s ** 3 * yC * es)
    rc = lib.bpx_conv3d_fwd_shuffle(dt, N, D, H, W, L.tview(x), None, 0, wp.data_ptr(), bias.data_ptr(), s, L.Tensor(y.data_ptr(), yC, yC, 0), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0, "accepted"
    assert bool((buf == SENTINEL).all().item()), "y or its guard bands were written"


# ---- input gradient ------------------------------------------------------------------------------------------------------------------
# (name, B, S, Cdy, Cg, ws, norm): the dgrad routes - 4x4x8 / 4x4x16 double-buffered, the lean kernel (hook and default size), NS 1..4
# (name, B, S, Cdy, Cg, ws, norm, act, planar t): the dgrad routes - 4x4x8 (two K groups at >= 4 even dy chunks), 4x4x16 and 4x8x16 double-buffered,
# the lean kernel (hook and default size), NS 1..4, the act' epilogue instances (ELU, run-time codes 0-3, codes 4-8), a chunk-planar t, D and H
# smaller than a tile
DGRAD_ROWS = [("s448_ns1", 3, (5, 6, 7), 16, 16, 0, True, 1, False), ("s448_ns4", 1, (9, 10, 11), 32, 64, 0, True, 1, False),
              ("s448_kg2_ns4_relu", 1, (9, 10, 11), 64, 64, 0, True, 2, False), ("s448_kg2_ns2_D2H3_gelu", 3, (2, 3, 13), 64, 32, 0, True, 5, False),
              ("s4416_ns3", 3, (5, 13, 65), 16, 48, 0, True, 1, False), ("s4416_ns2_plain", 1, (9, 17, 33), 32, 32, 0, False, 1, False),
              ("s4416_ws4_silu_planar", 1, (9, 17, 33), 16, 16, 4, True, 3, True), ("lean4416_ws5_ns2", 1, (9, 17, 33), 16, 32, 5, True, 1, False),
              ("s4816_ws4_tanh", 1, CB.BIG, 16, 16, 4, True, 6, False), ("lean4816", 3, CB.BIG, 16, 16, 0, True, 1, False),
              ("lean4816_planar", 1, CB.BIG, 32, 16, 0, True, 1, True), ("lean4416_ns3", 1, CB.BIG, 16, 48, 0, True, 1, False),
              # the RCAN up-scaling stage's backward (rcan_engine: blocks of 8 or 3 sub-positions = 128- / 48-channel dy into 16 channels, 8 and 3
              # K chunks per tap, no t operand).  bf16 and mix16 (no t: the same instance) reach conv3_lp_kernel<4, 8, 16, 1, EPI_DGRAD, 0>, f32
              # conv3_kernel<float, 4, 4, 16, 1, EPI_DGRAD, 0>
              ("lean4816_dy128_plain", 1, CB.BIG, 128, 16, 0, False, 1, False), ("lean4816_dy48_plain", 3, CB.BIG, 48, 16, 0, False, 1, False)]
DGRAD_CASES = [(r, m) for r in DGRAD_ROWS for m in ("f32", "bf16", "mix16")]


@pytest.mark.parametrize("row,mode", DGRAD_CASES, ids=[f"{r[0]}-{m}" for r, m in DGRAD_CASES])
def test_conv3d_dgrad_elementwise(row, mode):
    L = _L()
    lib = L.lib
    name, B, (D, H, W), Cdy, Cg, ws, norm, act, planar = row
    gk = "f32" if mode == "f32" else "bf16"        # dy, weights, g
    tk = {"f32": "f32", "bf16": "bf16", "mix16": "f16"}[mode]    # t (the forward's activation)
    dtc = {"f32": L.F32, "bf16": L.BF16, "mix16": L.MIX16}[mode]
    g = torch.Generator().manual_seed(7 + Cg)
    dy = CB.round_to(torch.randn(B, D, H, W, Cdy, generator=g), gk)
    w = CB.round_to(torch.randn(Cdy, Cg, 3, 3, 3, generator=g) / (27 * Cdy) ** 0.5, gk)
    t = CB.round_to(torch.randn(B, D, H, W, Cg, generator=g), tk)
    rec = _recs(B, Cg, g)
    dyd = dy.to(CB.TORCH_DT[gk]).to(DEV).contiguous()
    td = t.to(CB.TORCH_DT[tk]).to(DEV).contiguous()
    if planar:
        td = L.Planar(B, (D, H, W), Cg, CB.TORCH_DT[tk], DEV).copy_from_dense(td)
    wp = _pack(w, L.PK_K3_T, Cg, Cdy, gk)
    out = _nan((B, D, H, W, Cg), gk)
    tiles = lib.bpx_conv3d_stats_tiles(DT[gk], B, D, H, W, Cg)
    red = torch.full((B, tiles, 2, Cg), float("nan"), device=DEV)
    recd = rec.to(DEV)
    lib.bpx_debug_set_conv_ws(ws)
    try:
        if norm:
            L.check(lib.bpx_conv3d_dgrad(dtc, B, D, H, W, L.tview(dyd), wp.data_ptr(), L.tview(td), recd.data_ptr(), act, L.tview(out), red.data_ptr(),
                                         L.stream_ptr()))
        else:
            L.check(lib.bpx_conv3d_dgrad(dtc, B, D, H, W, L.tview(dyd), wp.data_ptr(), L.NULL_T, None, 0, L.tview(out), None, L.stream_ptr()))
        torch.cuda.synchronize()
    finally:
        lib.bpx_debug_set_conv_ws(0)
    ref, bound = CB.dgrad_reference(dy.to(DEV), w.to(DEV), gk, t=t.to(DEV) if norm else None, rec=rec.to(DEV) if norm else None, act=act)
    tag = f"dgrad[{name} {mode} B{B} {(D, H, W)} dy{Cdy}->g{Cg} norm{int(norm)} act{act} planar{int(planar)}]"
    rows = [CB.compare(tag + ".g", out, ref, bound)]
    if norm:
        # S1 = sum g, S2 = sum g xhat: the kernels sum the fp32 product acc * act'(u) BEFORE it is rounded to the storage type (conv3_kernel,
        # conv3_lean_kernel: s1 += v, s2 += v * xh), so the terms carry the bound of the fp32 value - dgrad_reference with an fp32 store; xhat is
        # (t - mean) rstd in fp32 from the stored t (norm_bounds.xhat_terms).  One row per tile: a lane sums its tile_vox / 64 <= 8 voxels, 16
        # lanes in 4 butterfly levels, the 4 waves in a chain of 3: 8 + 7.  The rows are summed here in fp64.
        _, pre = CB.dgrad_reference(dy.to(DEV), w.to(DEV), gk, t=t.to(DEV), rec=rec.to(DEV), act=act, out_kind="f32")
        s, sb = NB.red_reference(ref, pre, t.to(DEV), rec, 8 + 7)
        rows.append(CB.compare(tag + ".red", red.double().sum(1), s, sb, axes="nkc"))
    _check(rows)


# ---- fused backward: g, the S1 / S2 rows, dW and db --------------------------------------------------------------------------------------------
# (dtype, B, S, Ct, Cdy) - every instance bpx_conv3d_bwd_fused_supported admits, each serial and role-split where that form exists
BWD_CASES = [(r, rs) for r in CB.BWD_FUSED_ROWS for rs in ((0, 3) if r[4] == 16 else (0,))]


@pytest.mark.parametrize("row,rs", BWD_CASES, ids=[f"dt{r[0]}-t{r[3]}-dy{r[4]}-B{r[1]}-rs{rs}" for r, rs in BWD_CASES])
def test_conv3d_bwd_fused_g_elementwise(row, rs):
    L = _L()
    lib = L.lib
    dtc, B, (D, H, W), Ct, Cdy = row
    tk = "f16" if dtc == L.MIX16 else "bf16"
    g = torch.Generator().manual_seed(11 + Ct + Cdy)
    dy = CB.round_to(torch.randn(B, D, H, W, Cdy, generator=g), "bf16")
    w = CB.round_to(torch.randn(Cdy, Ct, 3, 3, 3, generator=g) / (27 * Cdy) ** 0.5, "bf16")
    t = CB.round_to(torch.randn(B, D, H, W, Ct, generator=g), tk)
    rec = _recs(B, Ct, g)
    lib.bpx_debug_set_bwd_rs(rs)
    try:
        dyd = dy.to(torch.bfloat16).to(DEV).contiguous()
        td = t.to(CB.TORCH_DT[tk]).to(DEV).contiguous()
        wp = _pack(w, L.PK_K3_T, Ct, Cdy, "bf16")
        out = _nan((B, D, H, W, Ct), "bf16")
        ft = lib.bpx_conv3d_bwd_fused_stats_tiles(B, D, H, W, Ct, Cdy)
        red = torch.full((B, ft, 2, Ct), float("nan"), device=DEV)
        dw = torch.full((Cdy, Ct, 3, 3, 3), float("nan"), device=DEV)
        db = torch.zeros(Cdy, device=DEV)
        ws = torch.empty(max(1, lib.bpx_conv3d_bwd_fused_workspace(B, D, H, W, Ct, Cdy)), dtype=torch.uint8, device=DEV)
        recd = rec.to(DEV)
        L.check(lib.bpx_conv3d_bwd_fused(dtc, B, D, H, W, L.tview(dyd), wp.data_ptr(), L.tview(td), recd.data_ptr(), 1, L.tview(out), red.data_ptr(),
                                         dw.data_ptr(), db.data_ptr(), None, ws.data_ptr(), ws.numel(), L.stream_ptr()))
        torch.cuda.synchronize()
    finally:
        lib.bpx_debug_set_bwd_rs(kernel_checks.RS_DEFAULT)
    ref, bound = CB.dgrad_reference(dy.to(DEV), w.to(DEV), "bf16", t=t.to(DEV), rec=rec.to(DEV), act=1)
    tag = f"bwd_fused[dt{dtc} B{B} {(D, H, W)} dy{Cdy}->t{Ct} rs{rs}]"
    rows = [CB.compare(tag + ".g", out, ref, bound)]
    # S1 / S2 as in the input-gradient test (the fp32 product is summed, xhat in fp32).  One row per workgroup (or per D wave, or per tile): a lane
    # keeps its sums over the tiles of a sample its workgroup walks - at most every 4x4x16 tile of the sample, 4 voxels per lane each - then 4
    # butterfly levels and a chain of 3 over the waves.
    tps = -(-D // 4) * -(-H // 4) * -(-W // 16)
    _, pre = CB.dgrad_reference(dy.to(DEV), w.to(DEV), "bf16", t=t.to(DEV), rec=rec.to(DEV), act=1, out_kind="f32")
    s, sb = NB.red_reference(ref, pre, t.to(DEV), rec, 4 * tps + 7)
    rows.append(CB.compare(tag + ".red", red.double().sum(1), s, sb, axes="nkc"))
    # dW[co][ci][tap] = sum_v a[v + tap][ci] dy[v][co], a = ELU(scale t + shift) rounded to a bf16 MFMA operand, and db = sum_v dy: one partial slab
    # per workgroup column (G of them: the workspace holds G (27 Ct + 1) Cdy floats).  A workgroup walks a contiguous share of its XCD's
    # ceil(T / 8) tiles, at most ceil(ceil(T / 8) / (G / 8)) + 1 of them, 256 voxels each, one rounding per product; the waves' accumulators meet in
    # at most 7 additions (8 waves in the role-split form); db sums one partial per thread and up to 512 of them in sequence; the reduction over
    # the slabs is wgrad_reduce_kernel's G + 3 (conv_bounds.wgrad_chains).
    G = ws.numel() // ((27 * Ct + 1) * Cdy * 4)
    T = B * tps
    slab = (-(-(-(-T // 8)) // max(1, G // 8)) + 1) * 256
    wref, wbound, dbr, dbb = CB.wgrad_reference(t.to(DEV), dy.to(DEV), 3, "bf16", rec=rec.to(DEV), act=1, chains=(slab + 7 + G + 3, slab + 512 + G + 3))
    rows += [CB.compare(tag + ".dw", dw, wref, wbound, axes="oikyx"), CB.compare(tag + ".db", db, dbr, dbb, axes="o")]
    _check(rows)


# ---- other forward entry points at f16 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B,persist", [((9, 17, 33), 3, 2048), ((40, 48, 64), 1, 64)])
def test_c1_fwd_f16_elementwise(S, B, persist):
    """bpx_conv3d_c1_fwd (first layer: one fp32 input channel) at f16.  The kernel rounds the fp32 weights to f16 like every 16-bit layer (here
    rounded on the host first, so that rounding is exact) and splits the fp32 image into hi + lo f16 parts, two MFMAs: the operand error is
    |img - hi - lo| <= u_f16 |img - hi| <= u_f16^2 |img|, plus 2^-25 where lo is an fp16 subnormal.  54 exact products and the bias in fp32,
    then the f16 store.  persist 64: the persistent workgroups wrap around the volume."""
    L = _L()
    lib = L.lib
    D, H, W = S
    Cout = 16
    g = torch.Generator().manual_seed(3)
    img = torch.randn(B, D, H, W, generator=g)
    w1 = CB.round_to(torch.randn(Cout, 1, 3, 3, 3, generator=g) * 0.2, "f16").float()
    b1 = (torch.randn(Cout, generator=g) * 0.1).float()
    imgd, wd, bd = img.to(DEV).contiguous(), w1.to(DEV).contiguous(), b1.to(DEV)
    y = _nan((B, D, H, W, Cout), "f16")
    tiles = lib.bpx_conv3d_c1_stats_tiles(D, H, W)
    part = torch.full((B, tiles, 2, Cout), float("nan"), device=DEV)
    lib.bpx_debug_set_c1_persist(persist)
    try:
        L.check(lib.bpx_conv3d_c1_fwd(L.F16, B, D, H, W, imgd.data_ptr(), wd.data_ptr(), bd.data_ptr(), L.tview(y), part.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
    finally:
        lib.bpx_debug_set_c1_persist(2048)
    x64, w64 = imgd.double()[..., None], wd.double()
    ref = CB.conv3(x64, w64) + bd.double()
    M = CB.conv3(x64.abs(), w64.abs()) + bd.double().abs()
    ea = CB.UNIT["f16"] ** 2 * x64.abs() + CB.F16_FLOOR
    bound = CB.finish(ref, M, CB.conv3(ea, w64.abs()), 2 * 27 + 1, "f16")
    _check([CB.compare(f"c1_fwd[f16 B{B} {S} wgs{persist}].y", y, ref, bound)])


@pytest.mark.parametrize("vox,Cin,Cout", [(4099, 48, 16), (1000, 16, 64)])
def test_conv1x1_fwd_f16_elementwise(vox, Cin, Cout):
    """bpx_conv1x1_fwd at f16: y = x W + bias (Cin products and the bias in fp32)."""
    L = _L()
    lib = L.lib
    B = 3
    g = torch.Generator().manual_seed(5)
    x = CB.round_to(torch.randn(B, vox, Cin, generator=g), "f16")
    w = CB.round_to(torch.randn(Cout, Cin, generator=g) / Cin ** 0.5, "f16")
    b = (torch.randn(Cout, generator=g) * 0.1).float()
    wp = _pack(w.view(Cout, Cin, 1, 1, 1), L.PK_DENSE, Cin, Cout, "f16")
    xd, bd = x.half().to(DEV).contiguous(), b.to(DEV)
    y = _nan((B, vox, Cout), "f16")
    L.check(lib.bpx_conv1x1_fwd(L.F16, B, vox, L.tview(xd), wp.data_ptr(), bd.data_ptr(), L.NULL_T, L.NULL_T, None, L.NULL_T, L.tview(y),
                                L.stream_ptr()))
    torch.cuda.synchronize()
    x64, w64 = x.to(DEV), w.to(DEV)
    ref = x64 @ w64.t() + bd.double()
    M = x64.abs() @ w64.abs().t() + bd.double().abs()
    bound = CB.finish(ref, M, torch.zeros_like(ref), Cin + 1, "f16")
    _check([CB.compare(f"conv1x1_fwd[f16 B{B} v{vox} {Cin}->{Cout}].y", y, ref, bound, axes="nvc")])


@pytest.mark.parametrize("k1", [0, 1])
@pytest.mark.parametrize("S,Cin,Cout,planar", [((5, 7, 16), 32, 16, True), ((3, 6, 9), 64, 32, False)])
def test_convT_fwd_f16_elementwise(k1, S, Cin, Cout, planar):
    """bpx_convT3d_k2s2_fwd at f16: y[2z+a, 2y+b, 2x+e] = x[z, y, x] W[:, :, a, b, e] + bias (Cin products and the bias).  k1 = 1 takes the
    one-K-step buffer-addressed kernel (convt_k1) where it applies (W % 16 == 0, Cin <= 32, chunk-planar output), 0 the general kernel."""
    L = _L()
    lib = L.lib
    B, (D, H, W) = 3, S
    g = torch.Generator().manual_seed(9)
    x = CB.round_to(torch.randn(B, D, H, W, Cin, generator=g), "f16")
    w = CB.round_to(torch.randn(Cin, Cout, 2, 2, 2, generator=g) / Cin ** 0.5, "f16")
    b = (torch.randn(Cout, generator=g) * 0.1).float()
    wp = _pack(w, L.PK_CT, Cin, Cout, "f16")
    xd, bd = x.half().to(DEV).contiguous(), b.to(DEV)
    S2 = (2 * D, 2 * H, 2 * W)
    tiles = lib.bpx_convT3d_stats_tiles(D, H, W, 2)
    part = torch.full((B, tiles, 2, Cout), float("nan"), device=DEV)
    if planar:
        cat = L.Planar(B, S2, Cout + 16, torch.float16, DEV)
        cat._flat.fill_(float("nan"))
        yv, read = L.tview(cat, 0, Cout), lambda: cat.dense()[..., :Cout]
    else:
        yb = _nan((B, *S2, Cout), "f16")
        yv, read = L.tview(yb), lambda: yb
    lib.bpx_debug_set_convt_k1(k1)
    try:
        L.check(lib.bpx_convT3d_k2s2_fwd(L.F16, B, D, H, W, 2, L.tview(xd), wp.data_ptr(), bd.data_ptr(), yv, part.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
    finally:
        lib.bpx_debug_set_convt_k1(-1)
    x64, w64 = x.to(DEV), w.to(DEV)
    ref = torch.einsum("nzyxi,ioabe->nzaybxeo", x64, w64).reshape(B, *S2, Cout) + bd.double()
    M = torch.einsum("nzyxi,ioabe->nzaybxeo", x64.abs(), w64.abs()).reshape(B, *S2, Cout) + bd.double().abs()
    bound = CB.finish(ref, M, torch.zeros_like(ref), Cin + 1, "f16")
    _check([CB.compare(f"convT_fwd[f16 B{B} {S} {Cin}->{Cout} planar{int(planar)} k1={k1}].y", read(), ref, bound)])


# ---- weight gradients ------------------------------------------------------------------------------------------------------------
# (name, mode, k, Cin, Cout, use_tr, act): the k = 3 tile kernel (use_tr 1 | 2: never the shift-dy kernels), the windowed shift-dy kernel
# (use_tr 1 | 4 = 5: wgrad_sdm_kernel at 16 -> 16, wgrad_sd_kernel NS 2 at 32 -> 32), MIX16 (fp16 x staged as bf16), fp32, the k = 1 tile kernel.
# B 2 x 9 x 17 x 33: T = 90 4x4x16 tiles, below every schedule's group target (tile kernel 2048 / (chunks x co blocks), k = 1 768 / .., windowed
# kernel 256 x occupancy / units) and, with the slab cap raised (bpx_debug_set_wgrad_cap), below the cap: G = T partial slabs, one tile each
# (conv_bounds.wgrad_chains).  The k = 1 streaming kernel needs >= 65536 voxels and is not reached here.
WGRAD_S, WGRAD_B = (9, 17, 33), 2
WGRAD_ROWS = [("k3_tile_f32", "f32", 3, 16, 16, 1, 1), ("k3_tile_bf16", "bf16", 3, 16, 16, 3, 1), ("k3_sdm_bf16", "bf16", 3, 16, 16, 5, 1),
              ("k3_sd_ns2_bf16", "bf16", 3, 32, 32, 5, 3), ("k3_mix16", "mix16", 3, 16, 16, 5, 1), ("k3_tile_bf16_gelu", "bf16", 3, 16, 32, 3, 5),
              ("k1_tile_bf16", "bf16", 1, 48, 16, 1, 0), ("k1_tile_f32", "f32", 1, 16, 32, 1, 1),
              # the RCAN up-scaling stage's weight gradients, 16 -> 128 and 16 -> 48 (blocks of 8 and 3 sub-positions), no prologue.  pick_wcfg
              # splits 16 -> 128 down to NS 1 (90 groups x 1 chunk x 8 co blocks = 720 >= 512 only there) and 48 is NS 1 anyway; its group count is
              # min(T, cap, 2048 / (chunks x co blocks)) = min(90, 11574, 256 | 683) = 90.  use_tr 5: launch_wgrad_sd with ns 1 and sdm_plan mc 1
              # (one input chunk) - wgrad_sdm_kernel<1, 0> (bf16) / <1, 0, true> (mix16), groups min(8-aligned 1024 / (8 | 3 units) = 128 | 344,
              # cap, T) = 90.  use_tr 3: wgrad_kernel<uint16_t, 4, 4, 16, 1, 27, true, 0>, 90 groups.  G = T = 90 in every row.
              ("k3_sdm_bf16_c128", "bf16", 3, 16, 128, 5, 0), ("k3_sdm_mix16_c128", "mix16", 3, 16, 128, 5, 0),
              ("k3_sdm_bf16_c48", "bf16", 3, 16, 48, 5, 0), ("k3_tile_bf16_c128", "bf16", 3, 16, 128, 3, 0)]


@pytest.mark.parametrize("row", WGRAD_ROWS, ids=[r[0] for r in WGRAD_ROWS])
def test_conv3d_wgrad_elementwise(row):
    L = _L()
    lib = L.lib
    name, mode, k, Cin, Cout, use_tr, act = row
    B, (D, H, W) = WGRAD_B, WGRAD_S
    xk = {"f32": "f32", "bf16": "bf16", "mix16": "f16"}[mode]
    gk = "f32" if mode == "f32" else "bf16"
    dtc = {"f32": L.F32, "bf16": L.BF16, "mix16": L.MIX16}[mode]
    g = torch.Generator().manual_seed(21 + Cin + Cout + k)
    x = CB.round_to(torch.randn(B, D, H, W, Cin, generator=g), xk)
    dy = CB.round_to(torch.randn(B, D, H, W, Cout, generator=g), gk)
    rec = _recs(B, Cin, g) if act else None
    xd = x.to(CB.TORCH_DT[xk]).to(DEV).contiguous()
    dyd = dy.to(CB.TORCH_DT[gk]).to(DEV).contiguous()
    recd = rec.to(DEV) if rec is not None else None
    dw = torch.full((Cout, Cin, k, k, k), float("nan"), device=DEV)
    db = torch.zeros(Cout, device=DEV)
    lib.bpx_debug_set_wgrad_tr(use_tr)
    lib.bpx_debug_set_wgrad_cap(10000)
    try:
        ws = torch.empty(max(1, lib.bpx_conv3d_wgrad_workspace(B, D, H, W, Cin, Cout, k)), dtype=torch.uint8, device=DEV)
        L.check(lib.bpx_conv3d_wgrad(dtc, B, D, H, W, L.tview(xd), L.ptr(recd), act, L.tview(dyd), k, dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                     ws.numel(), L.stream_ptr()))
        torch.cuda.synchronize()
    finally:
        lib.bpx_debug_set_wgrad_tr(1)
        lib.bpx_debug_set_wgrad_cap(100)
    T = B * -(-D // 4) * -(-H // 4) * -(-W // 16)
    if k == 3:   # the workspace holds max(pick_wcfg groups, sdm_plan groups) slabs of (27 Cin + 1) Cout floats: G = T, as the chains below assume
        assert ws.numel() == T * (27 * Cin + 1) * Cout * 4, (ws.numel(), T)
    chains = CB.wgrad_chains(T, T, 256)
    if mode == "mix16" and rec is None:
        # MIX16 stages the fp16 x as the bf16 MFMA operand (WgradParams.x_f16: v_cvt_pk_bf16_f32, round to nearest even).  Behind a prologue that
        # conversion is the u_op |a| term of E_a; without one the operand is exactly the stored x rounded to bf16, which the host reproduces:
        # the reference takes that operand and E stays 0 (the stored fp16 x itself as the operand misses by up to 2^-9 |x| per product)
        x = CB.round_to(x, "bf16")
    ref, bound, dbr, dbb = CB.wgrad_reference(x.to(DEV), dy.to(DEV), k, "f32" if mode == "f32" else "bf16", rec=recd, act=act, chains=chains)
    tag = f"wgrad[{name} {mode} B{B} {WGRAD_S} {Cin}->{Cout} k{k} tr{use_tr} act{act}]"
    _check([CB.compare(tag + ".dw", dw, ref, bound, axes="oikyx"), CB.compare(tag + ".db", db, dbr, dbb, axes="o")])

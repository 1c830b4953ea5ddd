"""The small-tile conv kernel with WN of a K group's four waves across the output channels (conv3_kernel<..., WN>, bpx_debug_set_conv_wn): WN = 2 and
WN = 4 against WN = 1, bit for bit, on the output AND on the statistics partial rows - forward (with and without the norm + ELU prologue, no / 16- /
48-channel / rank-1 shortcut, fp16 and bf16) and input gradient (ELU' epilogue with both sums; t in bf16 and, mixed mode, fp16), one and two K groups,
whole and partial tiles, one to four channel blocks; one forward and one dgrad row per WN element by element against fp64 (tests/conv_bounds.py);
one train step of a four-level net whatever the hook says.

A (shape, WN) pair without an instance is skipped by asking the library (bpx_conv3d_wn_supported); only WN = 4 at NS = 2 may be."""
import functools

import pytest
import torch

import conv_bounds as CB
import norm_bounds as NB
import test_conv_bounds_gpu as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = 2                                            # a sample boundary falls between workgroups
VOLUMES = [(8, 8, 8), (6, 10, 12)]               # whole tiles; partial 4x4x8 tiles on all three axes
CINS = [32, 48, 64]                              # two chunks (one K group), an odd chunk count (one K group), four chunks (two K groups)
COUTS = [32, 64, 128]                            # NS 2, NS 4 (NS 2 at 8^3), two or more channel blocks
PROLOGUES = [0, 1]                               # none, norm + ELU
SHORTCUTS = [0, 16, 48, 1]                       # none, 1x1 conv of 16 / 48 channels, rank-1 image
WNS = [2, 4]


def _lib():
    return G._L().lib


def _bytes_equal(a, b):
    """torch.equal on the stored bits (so that a NaN the kernels never wrote in both runs does not hide behind NaN != NaN: it fails _written)."""
    return a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _written(*ts):
    return all(bool(torch.isfinite(t.float()).all().item()) for t in ts)


def _need_instance(dt, S, Cout, wn):
    if not _lib().bpx_conv3d_wn_supported(dt, S[0], S[1], S[2], Cout, wn):
        assert wn == 4, "every WN = 2 row must run"
        assert _lib().bpx_conv3d_wn_supported(dt, S[0], S[1], S[2], Cout, 2), "only the NS 2 instances lack WN = 4"
        pytest.skip("no WN = 4 instance at NS = 2")


class _Wn:
    def __init__(self, wn):
        self.wn = wn

    def __enter__(self):
        _lib().bpx_debug_set_conv_wn(self.wn)

    def __exit__(self, *a):
        _lib().bpx_debug_set_conv_wn(-1)


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
def _fwd_row(S, Cin, Cout, act, sc):
    return CB._r(f"wn_{S}_{Cin}_{Cout}_a{act}_sc{sc}", CB.W16, B, S, Cin, Cout, (4, 4, 8, 0), act=act, sc=sc)


@functools.lru_cache(maxsize=None)
def _fwd_operands(S, Cin, Cout, act, sc, kind):
    return G._operands(_fwd_row(S, Cin, Cout, act, sc), kind, seed=Cin + Cout + sc + act + S[0])


@functools.lru_cache(maxsize=None)
def _fwd(S, Cin, Cout, act, sc, kind, wn):
    with _Wn(wn):
        return G._run_fwd(_fwd_row(S, Cin, Cout, act, sc), kind, _fwd_operands(S, Cin, Cout, act, sc, kind), B)


@pytest.mark.parametrize("wn", WNS)
@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("Cout", COUTS)
@pytest.mark.parametrize("Cin", CINS)
@pytest.mark.parametrize("S", VOLUMES, ids=["8x8x8", "6x10x12"])
def test_fwd_same_bits_as_wn1(S, Cin, Cout, kind, wn):
    _need_instance(G.DT[kind], S, Cout, wn)
    bad = []
    for act in PROLOGUES:
        for sc in SHORTCUTS:
            one, got = _fwd(S, Cin, Cout, act, sc, kind, 1), _fwd(S, Cin, Cout, act, sc, kind, wn)
            assert _written(one["y"], one["part"]), (act, sc)
            if not _bytes_equal(got["y"], one["y"]):
                bad.append((act, sc, "y", int((got["y"] != one["y"]).sum().item())))
            if not _bytes_equal(got["part"], one["part"]):
                bad.append((act, sc, "part", int((got["part"] != one["part"]).sum().item())))
    assert not bad, bad


# ---- input gradient --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dgrad_operands(S, Cdy, Cg, mode):
    tk = "f16" if mode == "mix16" else "bf16"
    g = torch.Generator().manual_seed(7 + Cg + Cdy + S[0])
    D, H, W = S
    dy = CB.round_to(torch.randn(B, D, H, W, Cdy, generator=g), "bf16")
    w = CB.round_to(torch.randn(Cdy, Cg, 3, 3, 3, generator=g) / (27 * Cdy) ** 0.5, "bf16")
    t = CB.round_to(torch.randn(B, D, H, W, Cg, generator=g), tk)
    return dict(dy=dy, w=w, t=t, rec=G._recs(B, Cg, g), tk=tk)


@functools.lru_cache(maxsize=None)
def _dgrad(S, Cdy, Cg, mode, wn):
    """bpx_conv3d_dgrad with the ELU' epilogue and both sums: bf16 gradients, t in bf16 or (mix16) fp16."""
    L = G._L()
    lib = L.lib
    D, H, W = S
    o = _dgrad_operands(S, Cdy, Cg, mode)
    dyd = o["dy"].to(torch.bfloat16).to(DEV).contiguous()
    td = o["t"].to(CB.TORCH_DT[o["tk"]]).to(DEV).contiguous()
    wp = G._pack(o["w"], L.PK_K3_T, Cg, Cdy, "bf16")
    out = G._nan((B, D, H, W, Cg), "bf16")
    tiles = lib.bpx_conv3d_stats_tiles(G.DT["bf16"], B, D, H, W, Cg)
    red = torch.full((B, tiles, 2, Cg), float("nan"), device=DEV)
    recd = o["rec"].to(DEV)
    with _Wn(wn):
        L.check(lib.bpx_conv3d_dgrad(L.MIX16 if mode == "mix16" else L.BF16, B, D, H, W, L.tview(dyd), wp.data_ptr(), L.tview(td), recd.data_ptr(), 1,
                                     L.tview(out), red.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
    return dict(g=out, red=red)


@pytest.mark.parametrize("wn", WNS)
@pytest.mark.parametrize("mode", ["bf16", "mix16"])
@pytest.mark.parametrize("Cg", COUTS)
@pytest.mark.parametrize("Cdy", CINS)
@pytest.mark.parametrize("S", VOLUMES, ids=["8x8x8", "6x10x12"])
def test_dgrad_same_bits_as_wn1(S, Cdy, Cg, mode, wn):
    L = G._L()
    _need_instance(L.MIX16 if mode == "mix16" else L.BF16, S, Cg, wn)
    one, got = _dgrad(S, Cdy, Cg, mode, 1), _dgrad(S, Cdy, Cg, mode, wn)
    assert _written(one["g"], one["red"])
    assert _bytes_equal(got["g"], one["g"]), int((got["g"] != one["g"]).sum().item())
    assert _bytes_equal(got["red"], one["red"]), int((got["red"] != one["red"]).sum().item())


# ---- element by element against fp64 ---------------------------------------------------------------------------------------------------
# the partial-tile volume, four input chunks (two K groups), 64 output channels (NS 4: both WN have an instance)
BOUND_S, BOUND_CIN, BOUND_COUT = (6, 10, 12), 64, 64


@pytest.mark.parametrize("wn", WNS)
def test_fwd_elementwise_against_fp64(wn):
    kind, act, sc = "f16", 1, 48
    _need_instance(G.DT[kind], BOUND_S, BOUND_COUT, wn)
    o = _fwd_operands(BOUND_S, BOUND_CIN, BOUND_COUT, act, sc, kind)
    got = _fwd(BOUND_S, BOUND_CIN, BOUND_COUT, act, sc, kind, wn)
    dev = lambda t: None if t is None else t.to(DEV)
    ref, bound, pre = CB.fwd_reference(o["x"].to(DEV), o["w"].to(DEV), o["b"].to(DEV), kind, rec=dev(o["rec"]), act=act, sc=dev(o["sc"]), wsc=dev(o["wsc"]),
                                       bsc=dev(o["bsc"]))
    tag = f"conv_wn[fwd {kind} wn{wn} B{B} {BOUND_S} {BOUND_CIN}->{BOUND_COUT} act{act} sc{sc}]"
    s, sb = CB.stats_reference(ref, pre, 128)
    G._check([CB.compare(tag + ".y", got["y"], ref, bound), CB.compare(tag + ".stats", got["part"].double().sum(1), s, sb, axes="nkc")])


@pytest.mark.parametrize("wn", WNS)
def test_dgrad_elementwise_against_fp64(wn):
    L = G._L()
    mode = "mix16"
    _need_instance(L.MIX16, BOUND_S, BOUND_COUT, wn)
    o = _dgrad_operands(BOUND_S, BOUND_CIN, BOUND_COUT, mode)
    got = _dgrad(BOUND_S, BOUND_CIN, BOUND_COUT, mode, wn)
    args = (o["dy"].to(DEV), o["w"].to(DEV), "bf16")
    ref, bound = CB.dgrad_reference(*args, t=o["t"].to(DEV), rec=o["rec"].to(DEV), act=1)
    _, pre = CB.dgrad_reference(*args, t=o["t"].to(DEV), rec=o["rec"].to(DEV), act=1, out_kind="f32")
    # one row per tile: a lane sums its 128 / 64 = 2 voxels, 16 lanes in 4 butterfly levels, the 4 z-slices in a chain of 3 - inside the 8 + 7 of
    # test_conv3d_dgrad_elementwise, which is kept
    s, sb = NB.red_reference(ref, pre, o["t"].to(DEV), o["rec"], 8 + 7)
    tag = f"conv_wn[dgrad {mode} wn{wn} B{B} {BOUND_S} dy{BOUND_CIN}->g{BOUND_COUT}]"
    G._check([CB.compare(tag + ".g", got["g"], ref, bound), CB.compare(tag + ".red", got["red"].double().sum(1), s, sb, axes="nkc")])


# ---- one train step ----------------------------------------------------------------------------------------------------------------------
def test_train_step_same_bits_whatever_wn():
    """A four-level cfg-2-shaped net (fm 16-32-64-128) at 32^3, B = 2, mixed mode (fp16 forward, bf16 gradients): its 16^3, 8^3 and 4^3 levels take
    conv3_kernel's 4x4x8 instances.  One train step with the launcher's choice (0), with WN = 1 and with WN forced to 2 and 4: loss, logits and
    every gradient the same bits."""
    import torch.nn.functional as F_

    from biapy_amd.resunet import ResUNet

    fm, S = [16, 32, 64, 128], 32
    torch.manual_seed(11)
    m = ResUNet(image_shape=(S, S, S, 1), activation="elu", feature_maps=fm, drop_values=[0.0] * 4, normalization="in", yx_down=[2] * 3, z_down=[2] * 3,
                isotropy=[True] * 4, larger_io=False, conv_layers=[2] * 4, compute_dtype=torch.float16).cuda().train()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 1, S, S, S, generator=g).cuda()
    t = (torch.rand(B, 1, S, S, S, generator=g) > 0.5).float().cuda()

    def step(wn):
        with _Wn(wn):
            m.zero_grad(set_to_none=True)
            logits = m(x)
            loss = F_.binary_cross_entropy_with_logits(logits, t)
            loss.backward()
            torch.cuda.synchronize()
        return loss.detach().clone(), logits.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}

    loss1, logits1, grads1 = step(1)
    assert _written(loss1, logits1, *grads1.values())
    for wn in (0, 2, 4):
        loss, logits, grads = step(wn)
        assert _bytes_equal(loss, loss1) and _bytes_equal(logits, logits1), wn
        bad = [k for k in grads1 if not _bytes_equal(grads[k], grads1[k])]
        assert not bad, (wn, bad)

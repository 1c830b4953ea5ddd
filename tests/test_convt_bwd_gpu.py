"""bpx_convT3d_k2s2_bwd on the MI355X: both gradients of the transposed conv from one call, against the two separate entries
(bpx_convT3d_k2s2_wgrad, bpx_convT3d_k2s2_dgrad) BIT FOR BIT.

The one-pass instances (wgrad_ct_kernel<2, 2, 2, DG>: 32 -> 32 channels, sz = 2, >= 262144 input voxels; wgrad_ct_dma_kernel<4, 4, 32, .., DG>:
64 -> 64 channels, sz = 2, W % 32 == 0, >= 65536 input voxels; bf16 / MIX16) keep the weight-gradient phase of their kernel as it is and form dx
with the operands, the K order and ONE accumulator chain per element as pw_kernel<.., PW_CONVTD> does, so dW, db and dx must be equal, not close.  Every other shape runs the two kernels inside the entry and is equal by construction; the test pins that no
such shape is refused.  Output buffers start as NaN: a voxel the one-pass kernel forgets to store shows.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _operands(dt, B, S, Cin, Cout, sz, seed, dy_extra=0):
    """Seeded x (fp16 for MIX16), dy (bf16, optionally a channel slice of a wider buffer), the weight and its dgrad pack."""
    import kernel_checks as KC
    from biapy_amd import _lib as L

    D, H, W = S
    g = torch.Generator(device=DEV).manual_seed(seed)
    f32 = dt == L.F32
    gT = torch.float32 if f32 else torch.bfloat16
    xT = torch.float16 if dt == L.MIX16 else gT
    x = torch.randn((B, D, H, W, Cin), generator=g, device=DEV).to(xT)
    dyb = torch.randn((B, sz * D, 2 * H, 2 * W, Cout + dy_extra), generator=g, device=DEV).to(gT)
    w = torch.randn((Cin, Cout, sz, 2, 2), generator=g, device=DEV) / Cin ** 0.5
    wt = KC.pack(w.cpu(), L.PK_CT_T if sz == 2 else L.PK_CT4_T, Cin, Cout, L.F32 if f32 else L.BF16)
    return x, dyb, w, wt


def _separate(dt, B, S, sz, x, dyv, wt, Cin, Cout, dx_extra=0):
    from biapy_amd import _lib as L

    lib = L.lib
    D, H, W = S
    gT = torch.float32 if dt == L.F32 else torch.bfloat16
    dw = torch.full((Cin, Cout, sz, 2, 2), float("nan"), device=DEV)
    db = torch.zeros(Cout, device=DEV)                                    # accumulated into
    dx = torch.full((B, D, H, W, Cin + dx_extra), float("nan"), dtype=gT, device=DEV)
    ws = torch.empty(max(1, lib.bpx_convT3d_k2s2_wgrad_workspace(B, D, H, W, sz, Cin, Cout)), dtype=torch.uint8, device=DEV)
    L.check(lib.bpx_convT3d_k2s2_wgrad(dt, B, D, H, W, sz, L.tview(x), dyv, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr()))
    L.check(lib.bpx_convT3d_k2s2_dgrad(L.BF16 if dt == L.MIX16 else dt, B, D, H, W, sz, dyv, wt.data_ptr(), L.tview(dx, 0, Cin), L.stream_ptr()))
    torch.cuda.synchronize()
    return dw, db, dx


def _one_call(dt, B, S, sz, x, dyv, wt, Cin, Cout, dx_extra=0):
    from biapy_amd import _lib as L

    lib = L.lib
    D, H, W = S
    gT = torch.float32 if dt == L.F32 else torch.bfloat16
    dw = torch.full((Cin, Cout, sz, 2, 2), float("nan"), device=DEV)
    db = torch.zeros(Cout, device=DEV)
    dx = torch.full((B, D, H, W, Cin + dx_extra), float("nan"), dtype=gT, device=DEV)
    ws = torch.empty(max(1, lib.bpx_convT3d_k2s2_wgrad_workspace(B, D, H, W, sz, Cin, Cout)), dtype=torch.uint8, device=DEV)
    n0 = lib.bpx_debug_convt_bwd_launches()
    L.check(lib.bpx_convT3d_k2s2_bwd(dt, B, D, H, W, sz, L.tview(x), dyv, wt.data_ptr(), L.tview(dx, 0, Cin), dw.data_ptr(), db.data_ptr(),
                                     ws.data_ptr(), ws.numel(), L.stream_ptr()))
    torch.cuda.synchronize()
    return dw, db, dx, lib.bpx_debug_convt_bwd_launches() - n0


def _compare(dt, B, S, Cin, Cout, sz, one_pass, seed=0, dy_extra=0, dx_extra=0):
    from biapy_amd import _lib as L

    x, dyb, w, wt = _operands(dt, B, S, Cin, Cout, sz, seed, dy_extra)
    dyv = L.tview(dyb, 0, Cout)
    dw0, db0, dx0 = _separate(dt, B, S, sz, x, dyv, wt, Cin, Cout, dx_extra)
    assert not torch.isnan(dx0[..., :Cin].float()).any() and not torch.isnan(dw0).any()
    dw1, db1, dx1, launches = _one_call(dt, B, S, sz, x, dyv, wt, Cin, Cout, dx_extra)
    assert launches == (1 if one_pass else 0), f"one-pass launches: {launches}"
    assert torch.equal(dw1, dw0), f"dW differs: max |d| = {(dw1 - dw0).abs().max().item():.3e}"
    assert torch.equal(db1, db0), f"db differs: max |d| = {(db1 - db0).abs().max().item():.3e}"
    a, b = dx1[..., :Cin], dx0[..., :Cin]
    assert not torch.isnan(a.float()).any(), f"{int(torch.isnan(a.float()).sum())} dx elements were never stored"
    assert torch.equal(a, b), f"dx differs in {int((a != b).sum())} of {a.numel()} elements, max |d| = {(a.float() - b.float()).abs().max().item():.3e}"
    if dx_extra:
        assert torch.isnan(dx1[..., Cin:].float()).all(), "channels beside the dx slice were written"
    return x, dyb, w, dx1


def _dts():
    from biapy_amd import _lib as L

    return {"bf16": L.BF16, "mix16": L.MIX16, "f32": L.F32}


@pytest.mark.parametrize("mode", ["bf16", "mix16"])
@pytest.mark.parametrize("B, S, C, one_pass", [
    (4, (64, 64, 64), 32, True),        # level 0 of the benched step
    (4, (32, 32, 32), 64, True),        # level 1 of the benched step (the streaming kernel's instance)
    (2, (50, 52, 80), 32, True),        # >= 262144 voxels, no extent a multiple of the 2x4x16 tile: edge tiles in z (50 = 25 x 2 fits), y and x
    (1, (65, 67, 61), 32, True),        # odd extents on every axis
    (3, (23, 31, 32), 64, True),        # the streaming kernel: 2139 blocks of 32 voxels over 256 workgroups, the last walk ragged
    (1, (16, 33, 128), 64, True),       # ... and a last block (67584 voxels = 2112 blocks) with rows of 4 blocks: every voxel of a block on one x row
    (2, (40, 41, 40), 64, False),       # W % 32 != 0: the 64 -> 64 layer runs the tile kernel, which has no one-pass instance
], ids=["4x64^3x32", "4x32^3x64", "2x50x52x80x32", "1x65x67x61x32", "3x23x31x32x64", "1x16x33x128x64", "2x40x41x40x64"])
def test_bwd_equals_the_two_entries_bit_for_bit(mode, B, S, C, one_pass):
    _compare(_dts()[mode], B, S, C, C, 2, one_pass, seed=B * 100 + C)


@pytest.mark.parametrize("case, mode, B, S, Cin, Cout, sz", [
    ("small_volume", "bf16", 2, (10, 12, 48), 32, 32, 2),
    ("cin48", "bf16", 2, (64, 64, 32), 48, 48, 2),
    ("cout64", "mix16", 2, (64, 64, 32), 32, 64, 2),
    ("sz1", "bf16", 2, (64, 64, 32), 32, 32, 1),
    ("fp32", "f32", 2, (64, 64, 32), 32, 32, 2),
])
def test_shapes_without_an_instance_run_the_two_kernels(case, mode, B, S, Cin, Cout, sz):
    _compare(_dts()[mode], B, S, Cin, Cout, sz, False, seed=7)


def test_switch_off_runs_the_two_kernels():
    from biapy_amd import _lib as L

    L.lib.bpx_debug_set_convt_bwd(0)
    try:
        _compare(L.MIX16, 2, (64, 64, 32), 32, 32, 2, False, seed=3)
    finally:
        L.lib.bpx_debug_set_convt_bwd(1)


@pytest.mark.parametrize("dy_extra, dx_extra", [(16, 0), (0, 16), (32, 8)])
def test_pitched_operands(dy_extra, dx_extra):
    """ld > C: dy as a channel slice of a wider buffer (the ResUNet++ decoder passes one), dx into a slice.  The one-pass kernel addresses both
    through their pitches, so it stays on; the channels beside the dx slice keep their fill."""
    from biapy_amd import _lib as L

    _compare(L.BF16, 2, (64, 64, 32), 32, 32, 2, True, seed=11, dy_extra=dy_extra, dx_extra=dx_extra)


def test_misaligned_dx_falls_back_like_the_dgrad_entry():
    """A dx slice that starts 8 bytes into a voxel row: bpx_convT3d_k2s2_dgrad refuses it (16-byte alignment), and so does the one call - with
    an error, not a fault: the one-pass kernel is never launched on it."""
    from biapy_amd import _lib as L

    lib = L.lib
    B, S, C = 2, (64, 64, 32), 32
    x, dyb, w, wt = _operands(L.BF16, B, S, C, C, 2, 5)
    dxb = torch.zeros((B,) + S + (C + 16,), dtype=torch.bfloat16, device=DEV)
    dw, db = torch.zeros((C, C, 2, 2, 2), device=DEV), torch.zeros(C, device=DEV)
    ws = torch.empty(max(1, lib.bpx_convT3d_k2s2_wgrad_workspace(B, *S, 2, C, C)), dtype=torch.uint8, device=DEV)
    n0 = lib.bpx_debug_convt_bwd_launches()
    rc_sep = lib.bpx_convT3d_k2s2_dgrad(L.BF16, B, *S, 2, L.tview(dyb), wt.data_ptr(), L.tview(dxb, 4, C), L.stream_ptr())
    rc_one = lib.bpx_convT3d_k2s2_bwd(L.BF16, B, *S, 2, L.tview(x), L.tview(dyb), wt.data_ptr(), L.tview(dxb, 4, C), dw.data_ptr(), db.data_ptr(),
                                      ws.data_ptr(), ws.numel(), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc_sep != 0 and rc_one != 0 and lib.bpx_debug_convt_bwd_launches() == n0


@pytest.mark.parametrize("B, S, C", [(2, (50, 52, 80), 32), (3, (23, 31, 32), 64)], ids=["32ch", "64ch"])
def test_dx_against_fp64_per_element(B, S, C):
    """The one-pass dx against an fp64 transposed-conv backward on the bf16-rounded operands, every element, with the bound of tests/conv_bounds.py
    (u_out = 2^-8, gamma = K 2^-24 with K = 8 Cout, E = 0; derived there, not fitted): the bit-equality above rests on today's dgrad, this stands
    on its own.  (_compare has already required that today's dgrad gives the same bits on these operands.)"""
    import conv_bounds as CB
    from biapy_amd import _lib as L

    x, dyb, w, dx = _compare(L.BF16, B, S, C, C, 2, True, seed=21)
    wr = w.to(torch.bfloat16).double()                                   # (Cin, Cout, 2, 2, 2)
    D, H, W = S
    dy64 = dyb.double().view(B, D, 2, H, 2, W, 2, C)                     # dx[v][ci] = sum_{co, sub} dy[2v + sub][co] W[ci][co][sub]
    ref = torch.einsum("bdahpwqo,ioapq->bdhwi", dy64, wr)
    mag = torch.einsum("bdahpwqo,ioapq->bdhwi", dy64.abs(), wr.abs())
    bound = CB.finish(ref, mag, 0.0, 8 * C, "bf16")
    r = CB.compare(f"convT_bwd[bf16 B{B} {S} {C}->{C}].dx", dx, ref, bound)
    print(f"{r['name']}: worst error / bound = {r['err']:.3f} {r['extra']}")
    assert r["ok"], r


def test_train_step_gradients_do_not_depend_on_the_switch():
    """One cfg-2-shaped mixed-mode train step whose level-0 and level-1 transposed convs take the one-pass kernels (2 x 128^3: 524288 and
    65536 input voxels):
    every parameter gradient with the switch on equals the one with it off, bit for bit (every instance is bit-identical above)."""
    from biapy_amd import _lib as L
    from biapy_amd.engine import NetConfig, ResUNetEngine
    from oracle import net_oracle

    fm = [16, 32, 64, 128, 256]
    sd = net_oracle.init_state_dict(1, fm, seed=0)
    g = torch.Generator().manual_seed(9)
    P3 = (128, 128, 128)
    x = torch.randn(2, 1, *P3, generator=g)
    tgt = (torch.rand(2, 1, *P3, generator=g) > 0.5).float()

    def step():
        eng = ResUNetEngine(NetConfig(in_ch=1, feature_maps=fm), torch.float16)
        P = {k: v.cuda() for k, v in sd.items()}
        logits, ctx = eng.forward(P, x.cuda(), head_act=0, save=True)
        lg = logits.detach().clone().requires_grad_(True)
        F.binary_cross_entropy_with_logits(lg, tgt.cuda()).backward()
        n0 = L.lib.bpx_debug_convt_bwd_launches()
        G = eng.backward(P, ctx, lg.grad)
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in G.items()}, L.lib.bpx_debug_convt_bwd_launches() - n0

    G1, n1 = step()
    L.lib.bpx_debug_set_convt_bwd(0)
    try:
        G0, n0 = step()
    finally:
        L.lib.bpx_debug_set_convt_bwd(1)
    assert n1 == 2 and n0 == 0, (n1, n0)
    assert set(G1) == set(G0)
    diff = [k for k in G1 if not torch.equal(G1[k], G0[k])]
    assert not diff, f"gradients differ with the switch: {diff[:5]}"

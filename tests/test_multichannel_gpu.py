"""Images of 2 to 15 channels on the device: the pack kernel bit for bit, the zero-padded engine against the 16-channel path bit for bit, the
modules against the fp32 oracle, the sliding-window predictor and graph replay (tests/multichannel_checks.py)."""
import pytest
import torch

import multichannel_checks as MC

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]


def _assert_all(rows):
    for r in rows:
        print(f"{'ok  ' if r['ok'] else 'FAIL'} {r['name']}: {r['err']:.3e} (bar {r['tol']:.3e}) {r['extra']}")
    bad = [r for r in rows if not r["ok"]]
    assert not bad, "\n".join(f"{r['name']}: {r['err']:.3e} > {r['tol']:.3e} {r['extra']}" for r in bad)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("layout", ["planar", "channels_last", "2d"])
@pytest.mark.parametrize("C", [2, 3, 4, 5, 15])
def test_image_pack16_bit_for_bit(C, layout, dtype):
    """bpx_image_pack16 equals bpx_cast of the zero-filled NDHWC tensor; the padding channels are written, the sentinel tail is not."""
    _assert_all(MC.check_image_pack16(C, layout, dtype))


def test_engine_picks_the_layout_from_the_strides():
    """Planar, the channels-last view and a stride pattern that is neither (made contiguous on the host) give the same padded tensor."""
    from biapy_amd import _lib as L
    from biapy_amd.engine import NetConfig, ResUNetEngine

    eng = ResUNetEngine(NetConfig(in_ch=3, feature_maps=[16, 32]), torch.float32)
    x = torch.randn(2, 3, 4, 6, 10, device="cuda")
    want = MC.zero_filled(x).permute(0, 2, 3, 4, 1).contiguous()
    odd = torch.randn(2, 3, 4, 6, 20, device="cuda")[..., ::2]
    for xin, ref in ((x, want), (MC.channels_last_view(x), want), (odd, MC.zero_filled(odd).permute(0, 2, 3, 4, 1).contiguous())):
        got = eng._pack_image16(xin, L.stream_ptr())
        torch.cuda.synchronize()
        assert got.shape == ref.shape and torch.equal(got, ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "mixed"])
@pytest.mark.parametrize("norm,C", [("in", 3), ("gn", 2), ("bn", 15)])
def test_same_bits_as_the_16_channel_path(norm, C, dtype):
    """fm [16, 32, 64], patch (16, 32, 32), B = 2: logits and every gradient equal those of the in_ch = 16 engine on padded operands."""
    _assert_all(MC.check_same_bits_as_16_channels(C, [16, 32, 64], (16, 32, 32), 2, dtype, norm=norm))


def test_same_bits_as_the_16_channel_path_through_the_large_level_kernels():
    """fm [16, 32], patch 64^3, B = 1, mixed mode: the first block runs through the >= 64^3 kernels (lean, z-march, fused pool)."""
    _assert_all(MC.check_same_bits_as_16_channels(4, [16, 32], (64, 64, 64), 1, torch.float16))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "mixed"])
def test_same_bits_as_the_16_channel_path_2d(dtype):
    """The 2-D engine ((B, C, Y, X) tensors, Conv2d-shaped parameters) in the 16-bit modes, whose oracle bars are the 3-D network's: bit equality
    with the 16-channel path instead."""
    _assert_all(MC.check_same_bits_as_16_channels(3, [16, 32, 64], (64, 64), 2, dtype, ndim=2))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "mixed"])
@pytest.mark.parametrize("C", [2, 3, 4])
def test_resunet_module_matches_the_oracle(C, dtype):
    """ResUNet(image_shape=(16, 32, 32, C)) in train mode on a planar input and on a channels-last view: logits, BCE loss and every parameter
    gradient within LOGITS_TOL / LOSS_TOL / GRAD_TOL / GRAD_TOL_LEVEL_16 of kernel_checks.py; gradient shapes are the parameters'; eval logits."""
    _assert_all(MC.check_module_3d(C, dtype))


@pytest.mark.parametrize("kind", ["resunet", "unet"])
def test_2d_rgb_modules_match_the_oracle(kind):
    """A 2-D RGB ResUNet / U_Net at (64, 64, 3) against net_oracle.resunet_forward / unet_oracle.unet_forward driven by the module's own state
    dict, at the same bars.  In fp32, where the bars follow from the number format: the 16-bit bars of kernel_checks.py (per-level gradient bars,
    logits 4e-3 in the mixed mode) were set on 3-D ResUNets - the repository's own 2-D checks (check_unet) carry wider ones - so the 16-bit modes
    of the 2-D path are held to bit equality with the 16-channel path above instead of to an oracle bar that was not made for them."""
    _assert_all(MC.check_module_2d(kind, torch.float32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_sliding_window_on_a_3_channel_volume(dtype):
    """Volume (48, 40, 56, 3), patch 32^3, overlap (0.5, 0.25, 0.5), padding (0, 4, 0), batch 5 against the oracle pipeline: probabilities within
    2e-5 (f32) / 4e-3 (fp16), labels equal outside the mode's band."""
    _assert_all(MC.check_sliding_window(dtype))


def test_graph_replay_of_a_3_channel_model():
    """capture_graphs on a 3-channel model: two replayed training calls equal the eager calls bit for bit."""
    _assert_all(MC.check_graph_replay())

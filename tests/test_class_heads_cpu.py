"""Output heads of 5..8 channels (multi-class segmentation, instance channels beside a class head) - the host side, no GPU.

The head kernels take up to eight channels (one 4-bit activation code per channel in a C int); the engines, models and the compiled kernels are
checked here: construction of every model family at 5..8 channels, parameter names and shapes against the oracle / the reference's keyword sets,
the refusal above eight, the 8-channel activation code, and no scratch in any head-kernel instance.
"""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
HIPCC_DERIVED_WITH = "7.2"        # as tests/test_isa_cpu.py: another compiler release is skipped, not failed

SMALL = dict(image_shape=(16, 16, 16, 1), activation="elu", feature_maps=[16, 32], drop_values=[0.0] * 2, normalization="in", yx_down=[2], z_down=[2],
             isotropy=[True] * 2, larger_io=False, conv_layers=[2] * 2)


def _kwargs(name):
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "build_model_kwargs.json")))
    return {k: (tuple(v) if k in ("image_shape", "upsampling_factor") else v) for k, v in rec[name].items()}


def _shapes(sd):
    return {k: tuple(v.shape) for k, v in sd.items()}


def _assert_like_oracle(m, fm, out_channels):
    from oracle import net_oracle

    ref = net_oracle.init_state_dict(1, fm, out_channels=tuple(out_channels), z_down=m.cfg.z_down)
    assert _shapes(m.state_dict()) == _shapes(ref)


def test_resunet_eight_class_softmax_head_constructs():
    from biapy_amd.resunet import ResUNet

    m = ResUNet(output_channels=[8], head_activations=["ce_softmax"], **SMALL)
    assert sum(m.output_channels) == 8 and tuple(m.heads[0].weight.shape) == (8, 16, 1, 1, 1)
    _assert_like_oracle(m, [16, 32], [8])


def test_resunet_instance_channels_with_a_class_head_construct():
    from biapy_amd.resunet import ResUNet

    m = ResUNet(output_channels=[3, 5], output_channel_info=["BCD", "class"], head_activations=["ce_sigmoid", "ce_sigmoid", "tanh", "ce_softmax"], **SMALL)
    assert m.return_class and m._class_channels == [3, 4, 5, 6, 7] and m._pred_channels == [0, 1, 2]
    _assert_like_oracle(m, [16, 32], [3, 5])


def test_resunet_ovarian_widths_six_channels_construct():
    """The GEMM-fed wide head (first level 48): the reference's Ovarian-Reserve keyword set with six output channels."""
    from biapy_amd.resunet import ResUNet

    kw = _kwargs("ovarian_reserve_resunet")
    kw.update(output_channels=[6], head_activations=["ce_softmax"], output_channel_info=["F"])
    m = ResUNet(**kw)
    assert m.cfg.true_feature_maps is None and list(m.cfg.feature_maps) == [48, 64, 80, 96]
    _assert_like_oracle(m, [48, 64, 80, 96], [6])


def test_resunet_cartocell_widths_seven_channels_construct():
    """Zero-padded widths (52-68-84 run as 64-80-96 inside the engine); parameters stay in the reference's shapes."""
    from biapy_amd.resunet import ResUNet

    kw = _kwargs("cartocell_resunet")
    kw.update(output_channels=[7], head_activations=["ce_softmax"], output_channel_info=["F"])
    m = ResUNet(**kw)
    assert list(m.cfg.feature_maps) == [64, 80, 96]
    _assert_like_oracle(m, [52, 68, 84], [7])


@pytest.mark.parametrize("n", [6, 7, 8])
def test_unet_with_six_to_eight_channels_constructs(n):
    from biapy_amd.unet import U_Net

    g = np.load(os.path.join(ROOT, "tests", "golden", "unet_golden.npz"))
    ref = {k[len("3d/sd/"):]: tuple(g[k].shape) for k in g.files if k.startswith("3d/sd/")}
    fm = [int(v) for v in g["3d/feature_maps"]]
    m = U_Net(image_shape=(16, 16, 16, 1), activation="elu", feature_maps=fm, drop_values=[0.0] * len(fm), normalization="in", yx_down=[2] * (len(fm) - 1),
              z_down=[int(v) for v in g["3d/z_down"]], output_channels=[n], isotropy=[True] * len(fm), larger_io=False, conv_layers=[2] * len(fm))
    got = _shapes(m.state_dict())
    ref["heads.0.weight"], ref["heads.0.bias"] = (n,) + ref["heads.0.weight"][1:], (n,)
    assert got == ref


@pytest.mark.parametrize("n", [6, 8])
def test_resunetpp_with_six_to_eight_channels_constructs(n):
    from biapy_amd.resunetpp import ResUNetPlusPlus

    kw = _kwargs("cfg4_resunet++")
    kw.update(output_channels=[n], output_channel_info=["F"], head_activations=["ce_softmax"])
    m = ResUNetPlusPlus(**kw)
    ref = ResUNetPlusPlus(**_kwargs("cfg4_resunet++"))                      # the reference's keyword set, three channels
    want = _shapes(ref.state_dict())
    want["heads.0.weight"], want["heads.0.bias"] = (n,) + want["heads.0.weight"][1:], (n,)
    assert _shapes(m.state_dict()) == want


def test_nine_channels_are_refused():
    from biapy_amd.resunet import ResUNet
    from biapy_amd.resunetpp import ResUNetPlusPlus
    from biapy_amd.unet import U_Net

    with pytest.raises(NotImplementedError, match="<= 8 channels"):
        ResUNet(output_channels=[9], head_activations=["ce_softmax"], **SMALL)
    with pytest.raises(NotImplementedError, match="<= 8 channels"):
        ResUNet(output_channels=[3, 6], output_channel_info=["BCD", "class"], head_activations=["ce_sigmoid", "ce_sigmoid", "tanh", "ce_softmax"], **SMALL)
    with pytest.raises(NotImplementedError, match="<= 8 channels"):
        U_Net(image_shape=(16, 16, 16, 1), activation="elu", feature_maps=[16, 32], drop_values=[0.0] * 2, normalization="in", yx_down=[2], z_down=[2],
              output_channels=[9], isotropy=[True] * 2, larger_io=False, conv_layers=[2] * 2)
    kw = _kwargs("cfg4_resunet++")
    kw.update(output_channels=[9], output_channel_info=["F"], head_activations=["ce_softmax"])
    with pytest.raises(NotImplementedError, match="<= 8 channels"):
        ResUNetPlusPlus(**kw)


def test_eight_channel_head_activation_codes():
    from biapy_amd.resunet import ResUNet

    m = ResUNet(output_channels=[8], head_activations=["ce_softmax"], **SMALL)
    assert m.head_activation_code() == 0x33333333
    assert m.head_activation_code(["sigmoid", "sigmoid", "tanh"] + ["softmax"] * 5) == 0x33333211
    assert m.head_activation_code(["softmax"] * 3 + ["linear"] + ["softmax"] * 4) == 0x33330333


def _hipcc_version() -> str:
    if not os.path.exists(HIPCC):
        return ""
    out = subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout
    m = re.search(r"HIP version:\s*(\d+\.\d+)", out)
    return m.group(1) if m else ""


def _isa(src: str, tmp_path_factory) -> str:
    # the helper of tests/test_isa_cpu.py, with the Makefile's flags
    out = str(tmp_path_factory.mktemp("isa") / (src + ".s"))
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-result", "-S", "--cuda-device-only",
           os.path.join(ROOT, "biapy_amd", "csrc", src + ".hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)} failed:\n{r.stderr[-3000:]}"
    return open(out).read()


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.skipif(_hipcc_version() != HIPCC_DERIVED_WITH, reason=f"resource figures read off hipcc {HIPCC_DERIVED_WITH}")
def test_head_kernels_use_no_scratch(tmp_path_factory):
    """Every instance of the head kernels (forward: 3 types x 2 widths x Cout 1..8; backward: the Cout <= 4 kernel and the channel-sliced Cout 5..8
    kernel) keeps its accumulators in registers."""
    text = _isa("ends", tmp_path_factory)
    found = {}
    for m in re.finditer(r"^\s+\.name:\s+(\S+)\s*\n\s+\.private_segment_fixed_size:\s+(\d+)", text, re.M):
        if re.search(r"head_(fwd|bwd|bwd_slice)_kernel", m.group(1)):
            found[m.group(1)] = int(m.group(2))
    fwd = [k for k in found if "head_fwd_kernel" in k]
    sliced = [k for k in found if "head_bwd_slice_kernel" in k]
    assert len(fwd) == 3 * 2 * 8, sorted(fwd)
    assert len(sliced) == 3 * 4, sorted(sliced)                     # F32, BF16, MIX16 x Cout 5..8
    assert sum("head_bwd_kernel" in k for k in found) == 3 * 2 * 4
    assert all(v == 0 for v in found.values()), {k: v for k, v in found.items() if v}

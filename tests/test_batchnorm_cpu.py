"""BatchNorm ("bn") normalisation of the ResUNet drop-in - the host side, no GPU.

Construction of the cfg-2 network with BatchNorm3d layers, its state_dict against the reference key list with the running buffers inserted,
strict loading both ways against a module tree built with nn.BatchNorm3d, the configurations refused up front, the exported entry points and
no scratch in the BatchNorm kernels.
"""
import ast
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
HIPCC_DERIVED_WITH = "7.2"        # as tests/test_isa_cpu.py: another compiler release is skipped, not failed
BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def _cfg2_kwargs(**kw):
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "build_model_kwargs.json")))["cfg2_resunet"]
    out = {k: (tuple(v) if k == "image_shape" else v) for k, v in rec.items()}
    out.update(normalization="bn")
    out.update(kw)
    return out


def _bn_tree_from_in(**kw):
    """The same network with every InstanceNorm3d replaced by a plain nn.BatchNorm3d (what other PyTorch code builds for 'bn')."""
    from biapy_amd.resunet import ResUNet

    m = ResUNet(**_cfg2_kwargs(normalization="in", **kw))
    for name, mod in list(m.named_modules()):
        for cname, child in list(mod.named_children()):
            if isinstance(child, nn.InstanceNorm3d):
                setattr(mod, cname, nn.BatchNorm3d(child.num_features))
    return m


def test_cfg2_bn_state_dict_is_the_reference_keys_with_running_buffers(resunet_golden):
    from biapy_amd.engine import bn_layers
    from biapy_amd.resunet import ResUNet

    m = ResUNet(**_cfg2_kwargs())
    layers = set(bn_layers(m.cfg))
    keys, shapes = [str(k) for k in resunet_golden["cfg2/keys"]], [tuple(ast.literal_eval(str(s))) for s in resunet_golden["cfg2/shapes"]]
    want = []
    for k, s in zip(keys, shapes):
        want.append((k, s))
        if k.endswith(".bias") and k[:-len(".bias")] in layers:
            c = s[0]
            want += [(k[:-len("bias")] + "running_mean", (c,)), (k[:-len("bias")] + "running_var", (c,)), (k[:-len("bias")] + "num_batches_tracked", ())]
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == want
    assert len(layers) == 17
    norms = [mod for mod in m.modules() if isinstance(mod, (nn.BatchNorm3d, nn.InstanceNorm3d, nn.GroupNorm))]
    assert len(norms) == 17 and all(type(n) is nn.BatchNorm3d for n in norms)
    assert all(n.eps == 1e-5 and n.momentum == 0.1 and n.affine and n.track_running_stats for n in norms)


def test_bn_load_state_dict_strict_both_ways():
    from biapy_amd.resunet import ResUNet

    m = ResUNet(**_cfg2_kwargs())
    ref = _bn_tree_from_in()
    assert list(ref.state_dict()) == list(m.state_dict())
    g = torch.Generator().manual_seed(0)
    sd = {k: (torch.randint(0, 100, v.shape, generator=g) if v.dtype == torch.int64 else torch.rand(v.shape, generator=g) + 0.5)
          for k, v in ref.state_dict().items()}
    ref.load_state_dict(sd, strict=True)
    m.load_state_dict(ref.state_dict(), strict=True)
    back = _bn_tree_from_in()
    back.load_state_dict(m.state_dict(), strict=True)
    for k, v in sd.items():
        assert torch.equal(m.state_dict()[k], v) and torch.equal(back.state_dict()[k], v), k


@pytest.mark.parametrize("case, kw", [
    ("2d", dict(image_shape=(64, 64, 1), z_down=[1] * 4)),
    ("width", dict(feature_maps=[24, 32, 64, 128, 256])),
    ("sr_pre", dict(upsampling_factor=(2, 2, 2), upsampling_position="pre")),
    ("sr_post", dict(upsampling_factor=(2, 2, 2), upsampling_position="post")),
    ("dropout", dict(drop_values=[0.1, 0.1, 0.1, 0.1, 0.1])),
])
def test_bn_refusals_at_construction(case, kw):
    from biapy_amd.resunet import ResUNet

    with pytest.raises(NotImplementedError, match="bn"):
        ResUNet(**_cfg2_kwargs(**kw))


def test_bn_refusals_of_other_normalisations_and_models():
    from biapy_amd.engine import NetConfig
    from biapy_amd.resunet import ResUNet
    from biapy_amd.resunetpp import ResUNetPlusPlus
    from biapy_amd.unet import U_Net

    with pytest.raises(NotImplementedError, match="sync_bn"):
        ResUNet(**_cfg2_kwargs(normalization="sync_bn"))
    with pytest.raises(NotImplementedError, match="bn"):
        NetConfig(in_ch=1, feature_maps=[16, 32], normalization="bn", ndim=2)
    unet_kw = dict(image_shape=(32, 32, 32, 1), activation="elu", feature_maps=[16, 32, 64], drop_values=[0.0] * 3, normalization="bn",
                   yx_down=[2, 2], z_down=[2, 2], isotropy=True, larger_io=False, conv_layers=[2] * 3)
    with pytest.raises(NotImplementedError, match="bn"):
        U_Net(**unet_kw)
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "build_model_kwargs.json")))["cfg4_resunet++"]
    kw = {k: (tuple(v) if k == "image_shape" else v) for k, v in rec.items()}
    kw["normalization"] = "bn"
    with pytest.raises(NotImplementedError, match="bn"):
        ResUNetPlusPlus(**kw)


def test_bn_momentum_none_is_refused():
    from biapy_amd.resunet import ResUNet

    m = ResUNet(**_cfg2_kwargs())
    m.engine()                                                       # 0.1 everywhere: fine
    m.down_path[1].block[0].momentum = None
    with pytest.raises(NotImplementedError, match="momentum=None"):
        m.engine()


def test_bn_data_parallel_step_is_refused():
    from biapy_amd.graphs import DataParallelTrainStep
    from biapy_amd.resunet import ResUNet

    m = ResUNet(**_cfg2_kwargs(image_shape=(32, 32, 32, 1)))
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    x = torch.zeros(1, 1, 32, 32, 32)
    with pytest.raises(NotImplementedError, match="bn"):
        DataParallelTrainStep(m, torch.nn.functional.mse_loss, opt, x, x, graph=False)


def test_bn_engine_flags_follow_the_module():
    from biapy_amd.resunet import ResUNet

    m = ResUNet(**_cfg2_kwargs(image_shape=(32, 32, 32, 1)))
    m.up_paths[0][1].conv_block.block[0].eps = 1e-3
    eng = m.train().engine()
    assert eng.bn and eng.bn_training and eng.bn_hparams["up_paths.0.1.conv_block.block.0"] == (1e-3, 0.1)
    assert m.eval().engine().bn_training is False
    assert set(m._bn_buffers()) == {k for k in m.state_dict() if k.endswith(BUFFERS)}
    assert ResUNet(**_cfg2_kwargs(normalization="in"))._bn_buffers() == {}


def test_bn_entry_points_are_exported():
    from biapy_amd import _lib as L

    for name in ("bpx_batchnorm_finalize", "bpx_batchnorm_bwd_finalize", "bpx_batchnorm_eval_records"):
        assert name in L.EXPORTS
        assert callable(getattr(L.lib, name))
    assert "bpx_batchnorm_eval_records" in open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    assert L.BnEvalJob.C.offset == 40 and ctypes.sizeof(L.BnEvalJob) == 48    # bpx_bn_eval_job: five pointers, int32 C, float eps


def _hipcc_version() -> str:
    if not os.path.exists(HIPCC):
        return ""
    out = subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout
    m = re.search(r"HIP version:\s*(\d+\.\d+)", out)
    return m.group(1) if m else ""


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.skipif(_hipcc_version() != HIPCC_DERIVED_WITH, reason=f"resource figures read off hipcc {HIPCC_DERIVED_WITH}")
def test_bn_kernels_use_no_scratch(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "elementwise.s")
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-result", "-S", "--cuda-device-only",
           os.path.join(ROOT, "biapy_amd", "csrc", "elementwise.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    found = {}
    for m in re.finditer(r"^\s+\.name:\s+(\S+)\s*\n\s+\.private_segment_fixed_size:\s+(\d+)", open(out).read(), re.M):
        if re.search(r"bn_(finalize|bwd_finalize|eval_records)_kernel", m.group(1)):
            found[m.group(1)] = int(m.group(2))
    assert len(found) == 3, sorted(found)
    assert all(v == 0 for v in found.values()), found

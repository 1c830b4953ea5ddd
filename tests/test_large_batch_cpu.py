"""Batches whose whole-batch operands pass the kernels' 2^31 span (engine.batch_groups): host-side checks, no GPU needed."""
import hashlib
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
HIPCC_DERIVED_WITH = "7.2"        # as tests/test_isa_cpu.py: another compiler release is skipped, not failed

CFG2 = [16, 32, 64, 128, 256]
FM32 = [32, 64, 128, 256]
P128 = (128, 128, 128)


def _cfg(fm):
    from biapy_amd.engine import NetConfig

    return NetConfig(in_ch=1, feature_maps=fm)


def _covers(groups, B):
    return groups[0][0] == 0 and groups[-1][1] == B and all(a < b for a, b in groups) and all(groups[q][1] == groups[q + 1][0] for q in range(len(groups) - 1))


@pytest.mark.parametrize("fm", [CFG2, FM32], ids=["fm16", "fm32"])
@pytest.mark.parametrize("B", [6, 8, 12, 16])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["mixed", "bf16", "f32"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "infer"])
def test_large_batches_are_accepted(fm, B, dtype, training):
    from biapy_amd.engine import SPAN_LIMIT, SPAN_MARGIN, _plane_pad, batch_groups, sample_span

    groups = batch_groups(_cfg(fm), dtype, B, P128, training)
    assert _covers(groups, B), groups
    per, _ = sample_span(_cfg(fm), dtype, P128, training)
    sizes = [b - a for a, b in groups]
    margin = SPAN_MARGIN + _plane_pad(_cfg(fm), False)
    assert all(n * per + margin <= SPAN_LIMIT for n in sizes), (sizes, per)
    assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
    if len(groups) > 1:            # the fewest groups: one fewer would put a group over the span
        assert -(-B // (len(groups) - 1)) * per + margin > SPAN_LIMIT


def test_group_plans_of_the_issue_shapes():
    from biapy_amd.engine import batch_groups

    # the benched cfg-2 step and every shape that ran before: one group, i.e. the launches they always ran
    assert batch_groups(_cfg(CFG2), torch.float16, 4, P128, True) == [(0, 4)]
    assert batch_groups(_cfg(CFG2), torch.float32, 4, P128, True) == [(0, 4)]
    assert batch_groups(_cfg(CFG2), torch.float16, 10, P128, True) == [(0, 10)]        # 48 ch x 2 B x 20.97 M voxels < 2 GiB
    assert batch_groups(_cfg(CFG2), torch.float16, 16, P128, False) == [(0, 16)]       # 1.6 G elements: the predictor's batch of 16
    assert batch_groups(_cfg(FM32), torch.float16, 5, P128, True) == [(0, 5)]
    # beyond: the fewest equal groups
    assert batch_groups(_cfg(FM32), torch.float16, 6, P128, True) == [(0, 3), (3, 6)]
    assert batch_groups(_cfg(FM32), torch.float16, 8, P128, True) == [(0, 4), (4, 8)]
    assert batch_groups(_cfg(CFG2), torch.float16, 11, P128, True) == [(0, 6), (6, 11)]
    assert batch_groups(_cfg(CFG2), torch.float16, 12, P128, True) == [(0, 6), (6, 12)]
    assert batch_groups(_cfg(FM32), torch.float16, 16, P128, False) == [(0, 8), (8, 16)]
    # fp32 training: the fp32 kernels address with 64-bit pointers and bound element counts, so the bound is 2^31 elements there
    assert batch_groups(_cfg(FM32), torch.float32, 4, P128, True) == [(0, 4)]
    assert batch_groups(_cfg(CFG2), torch.float32, 6, P128, True) == [(0, 6)]
    assert batch_groups(_cfg(FM32), torch.float32, 8, P128, True) == [(0, 8)]
    assert batch_groups(_cfg(FM32), torch.float32, 12, P128, True) == [(0, 6), (6, 12)]
    assert batch_groups(_cfg(FM32), torch.float32, 1, (192, 192, 192), True) == [(0, 1)]
    # the U-Net engine's decoder input is [up (fm0) | skip (fm0)]: 64 channels at fm0 = 32, batch 7 still fits (the ResUNet's 96 do not)
    assert batch_groups(_cfg(FM32), torch.float16, 7, P128, True, unet=True) == [(0, 7)]
    assert batch_groups(_cfg(FM32), torch.float16, 7, P128, True) == [(0, 4), (4, 7)]
    assert batch_groups(_cfg(FM32), torch.float16, 12, P128, True, unet=True) == [(0, 6), (6, 12)]


def test_plane_padding_counts_against_the_span(monkeypatch):
    """With the BPX_PLANE_PAD hook every 16-channel plane of a chunk-planar decoder input adds a pad to its span: counted for the widest one
    (384 channels = 24 planes at fm = [32, 64, 128, 256]; the U-Net's 256 = 16)."""
    from biapy_amd import _lib as L
    from biapy_amd.engine import _plane_pad, batch_groups

    patch = (128, 232, 376)              # one sample: 2^31 - 1.6 MiB bytes in the mixed mode
    assert batch_groups(_cfg(FM32), torch.float16, 1, patch, True) == [(0, 1)]
    monkeypatch.setattr(L, "PLANE_PAD_BYTES", 1 << 20)
    assert _plane_pad(_cfg(FM32), False) == 24 << 20 and _plane_pad(_cfg(FM32), True) == 16 << 20
    with pytest.raises(NotImplementedError, match="per-sample limit"):
        batch_groups(_cfg(FM32), torch.float16, 1, patch, True)


def test_unet_engine_plans_with_its_own_layout():
    from biapy_amd.unet_engine import UNetEngine

    eng = UNetEngine(_cfg(FM32), 3, torch.float16)
    assert eng._groups_for(7, P128, True) == [(0, 7)]
    assert eng._groups_for(12, P128, True) == [(0, 6), (6, 12)]


def test_one_sample_beyond_the_limit_raises_on_the_host():
    from biapy_amd.engine import ResUNetEngine, batch_groups

    with pytest.raises(NotImplementedError, match=r"patch 384x384x384: .*level-0 decoder input \(96 channels\).*per-sample limit of 2\^31 bytes"):
        batch_groups(_cfg(FM32), torch.float16, 1, (384, 384, 384), True)
    with pytest.raises(NotImplementedError, match=r"2\^31 elements"):
        batch_groups(_cfg(FM32), torch.float16, 1, (640, 640, 640), False)
    # the engine asks the same question before its first launch: no tensor is needed, no device is touched
    eng = ResUNetEngine(_cfg(FM32), torch.float16)
    with pytest.raises(NotImplementedError, match="per-sample limit"):
        eng._groups_for(2, (384, 384, 384), True)
    assert eng._groups_for(8, P128, True) == [(0, 4), (4, 8)]
    # BatchNorm couples the samples: a large batch keeps running as one (and keeps the refusals its own tests pin)
    from biapy_amd.engine import NetConfig

    bn = ResUNetEngine(NetConfig(in_ch=1, feature_maps=FM32, normalization="bn"), torch.float16)
    assert bn._groups_for(8, P128, True) == [(0, 8)]


def test_split_wgrad_query_refuses_what_the_kernel_refuses():
    """bpx_conv1x1_fwd_split_wgrad_query: the streaming kernel's own predicate (ADVICE r6 'medium'); pure host code, fake pointers."""
    from biapy_amd import _lib as L

    lib = L.lib
    base = 1 << 40

    def T(ptr, ld, C, cs=0):
        return L.Tensor(ptr, ld, C, cs)

    def query(N, vps, K=32, dt=L.MIX16, align=0, t_cs=None):
        vox = N * vps
        cs = t_cs if t_cs is not None else vox * 16
        x = T(base + align, K, K)
        g = T(None, 3 * K, 3 * K)
        t = T(base + (1 << 36), 16, 3 * K, cs)
        y_lo, y_hi = T(base + (2 << 36), 3 * K, 2 * K), T(base + (2 << 36) + 4 * K, 3 * K, K)
        return int(lib.bpx_conv1x1_fwd_split_wgrad_query(dt, N, vps, x, g, t, None, y_lo, y_hi))

    vps = 128 ** 3
    assert query(4, vps) == int(lib.bpx_conv1x1_fwd_split_wgrad_workspace(L.MIX16, 4, vps, 32)) > 0
    assert query(4, vps, K=16) > 0
    # past the 2^31-byte span: batch 6 at 128^3 with 32 channels (t: 96 channels x 2 B); the shape-only answer says yes there
    assert int(lib.bpx_conv1x1_fwd_split_wgrad_workspace(L.MIX16, 6, vps, 32)) > 0
    assert query(6, vps) == 0
    assert query(12, vps, K=16) == 0
    assert query(4, vps, align=8) == 0                  # misaligned operand
    assert query(4, vps, dt=L.F32) == 0
    assert query(1, 32 ** 3) == 0                       # below the streaming kernel's size


def _hipcc_version() -> str:
    if not os.path.exists(HIPCC):
        return ""
    out = subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout
    m = re.search(r"HIP version:\s*(\d+\.\d+)", out)
    return m.group(1) if m else ""


def kernel_digests(listing: str):
    """{kernel symbol: sha256[:16] of its function body} of a `hipcc -S --cuda-device-only` listing."""
    out = {}
    for m in re.finditer(r"^(\S+):\s+; @\1\n(.*?)^\.Lfunc_end\d+:", listing, re.M | re.S):
        out[m.group(1)] = hashlib.sha256(m.group(2).encode()).hexdigest()[:16]
    return out


# The kernels of pointwise.hip - the one kernel file whose host code this change touches - as listed from the tree before it.
POINTWISE_ISA = {
    "_ZN12_GLOBAL__N_113pw_nbs_kernelILi1ELi128EDF16_Lb0EEEvNS_9PwsParamsE": "59eaa985703315e6",
    "_ZN12_GLOBAL__N_113pw_nbs_kernelILi1ELi128EDF16_Lb1EEEvNS_9PwsParamsE": "5eafef6d25e4c70c",
    "_ZN12_GLOBAL__N_113pw_nbs_kernelILi1ELi128EtLb0EEEvNS_9PwsParamsE": "b942b2696b864aa3",
    "_ZN12_GLOBAL__N_113pw_nbs_kernelILi1ELi128EtLb1EEEvNS_9PwsParamsE": "e1b99fb246ebba8e",
    "_ZN12_GLOBAL__N_113pw_nbs_kernelILi2ELi64EDF16_Lb0EEEvNS_9PwsParamsE": "6fd852e48cedcc5c",
    "_ZN12_GLOBAL__N_113pw_nbs_kernelILi2ELi64EDF16_Lb1EEEvNS_9PwsParamsE": "c0a221b87016262e",
    "_ZN12_GLOBAL__N_113pw_nbs_kernelILi2ELi64EtLb0EEEvNS_9PwsParamsE": "f91a20e5459b3c33",
    "_ZN12_GLOBAL__N_113pw_nbs_kernelILi2ELi64EtLb1EEEvNS_9PwsParamsE": "1136b4776fad7f4a",
    "_ZN12_GLOBAL__N_115convt_k1_kernelIDF16_EEvNS_8PwParamsE": "28290654b46ca184",
    "_ZN12_GLOBAL__N_115convt_k1_kernelItEEvNS_8PwParamsE": "7d7ee4f8aaa0698c",
    "_ZN12_GLOBAL__N_19pw_kernelIDF16_Li2ELi1ELi0ELb0EDF16_Lb0EEEvNS_8PwParamsE": "555eda7876052c13",
    "_ZN12_GLOBAL__N_19pw_kernelIDF16_Li2ELi1ELi0ELb1EDF16_Lb0EEEvNS_8PwParamsE": "b06b7c98a26b6abc",
    "_ZN12_GLOBAL__N_19pw_kernelIDF16_Li2ELi1ELi1ELb0EDF16_Lb0EEEvNS_8PwParamsE": "befba91e78db6ad6",
    "_ZN12_GLOBAL__N_19pw_kernelIDF16_Li2ELi1ELi1ELb1EDF16_Lb0EEEvNS_8PwParamsE": "f066c9131940b9d4",
    "_ZN12_GLOBAL__N_19pw_kernelIDF16_Li2ELi2ELi0ELb0EDF16_Lb0EEEvNS_8PwParamsE": "dc29e9df272ab7dc",
    "_ZN12_GLOBAL__N_19pw_kernelIDF16_Li2ELi2ELi0ELb1EDF16_Lb0EEEvNS_8PwParamsE": "8a735b76c4caa3d0",
    "_ZN12_GLOBAL__N_19pw_kernelIDF16_Li2ELi2ELi1ELb0EDF16_Lb0EEEvNS_8PwParamsE": "b5c0402cf6aa901c",
    "_ZN12_GLOBAL__N_19pw_kernelIDF16_Li2ELi2ELi1ELb1EDF16_Lb0EEEvNS_8PwParamsE": "ba9b7bef90460eac",
    "_ZN12_GLOBAL__N_19pw_kernelIDF16_Li2ELi3ELi0ELb0EDF16_Lb0EEEvNS_8PwParamsE": "04b8ec3368ebea4c",
    "_ZN12_GLOBAL__N_19pw_kernelIDF16_Li2ELi3ELi0ELb1EDF16_Lb0EEEvNS_8PwParamsE": "4d7b2bf2efe5e24b",
    "_ZN12_GLOBAL__N_19pw_kernelIDF16_Li2ELi3ELi1ELb0EDF16_Lb0EEEvNS_8PwParamsE": "195185a72f6c6733",
    "_ZN12_GLOBAL__N_19pw_kernelIDF16_Li2ELi3ELi1ELb1EDF16_Lb0EEEvNS_8PwParamsE": "b7f1c47c6bc0fe3c",
    "_ZN12_GLOBAL__N_19pw_kernelIDF16_Li2ELi4ELi0ELb0EDF16_Lb0EEEvNS_8PwParamsE": "ea5c5f5442ae4018",
    "_ZN12_GLOBAL__N_19pw_kernelIDF16_Li2ELi4ELi0ELb1EDF16_Lb0EEEvNS_8PwParamsE": "0e79b86845eab1dc",
    "_ZN12_GLOBAL__N_19pw_kernelIDF16_Li2ELi4ELi1ELb0EDF16_Lb0EEEvNS_8PwParamsE": "1a1fb3a4b93c3140",
    "_ZN12_GLOBAL__N_19pw_kernelIDF16_Li2ELi4ELi1ELb1EDF16_Lb0EEEvNS_8PwParamsE": "0670abb47a2beb6e",
    "_ZN12_GLOBAL__N_19pw_kernelIDF16_Li2ELi4ELi1ELb1EDF16_Lb1EEEvNS_8PwParamsE": "f53271b9a39d101c",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi1ELi0ELb0EfLb0EEEvNS_8PwParamsE": "122736f04defd026",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi1ELi0ELb1EfLb0EEEvNS_8PwParamsE": "06c2706c72bd268a",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi1ELi1ELb0EfLb0EEEvNS_8PwParamsE": "38b4167cc4adb523",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi1ELi1ELb1EfLb0EEEvNS_8PwParamsE": "7dc5927d39fd1c2e",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi1ELi2ELb0EfLb0EEEvNS_8PwParamsE": "6f4f488042393b04",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi2ELi0ELb0EfLb0EEEvNS_8PwParamsE": "d18e0e7419fb894a",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi2ELi0ELb1EfLb0EEEvNS_8PwParamsE": "be4429d61ed970eb",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi2ELi1ELb0EfLb0EEEvNS_8PwParamsE": "f2cf9dcbcc4c9517",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi2ELi1ELb1EfLb0EEEvNS_8PwParamsE": "245753343c47e444",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi2ELi2ELb0EfLb0EEEvNS_8PwParamsE": "ef111226f14ad833",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi3ELi0ELb0EfLb0EEEvNS_8PwParamsE": "44bf5073d2a45e02",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi3ELi0ELb1EfLb0EEEvNS_8PwParamsE": "9cb93166eba12222",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi3ELi1ELb0EfLb0EEEvNS_8PwParamsE": "7be9d5c999500ef1",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi3ELi1ELb1EfLb0EEEvNS_8PwParamsE": "8baefe2cba1ab23b",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi3ELi2ELb0EfLb0EEEvNS_8PwParamsE": "b34921baccb67604",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi4ELi0ELb0EfLb0EEEvNS_8PwParamsE": "8725cfbb783b20f7",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi4ELi0ELb1EfLb0EEEvNS_8PwParamsE": "957b6167c6f6a4f2",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi4ELi1ELb0EfLb0EEEvNS_8PwParamsE": "284795b1735ee20a",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi4ELi1ELb1EfLb0EEEvNS_8PwParamsE": "3119520cc170ce47",
    "_ZN12_GLOBAL__N_19pw_kernelIfLi2ELi4ELi2ELb0EfLb0EEEvNS_8PwParamsE": "abe8082de6899a32",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi1ELi0ELb0EDF16_Lb0EEEvNS_8PwParamsE": "40fa7d7f20811cd9",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi1ELi0ELb0EtLb0EEEvNS_8PwParamsE": "97ea357d17f1ce48",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi1ELi0ELb1EDF16_Lb0EEEvNS_8PwParamsE": "d8dfa675c9574967",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi1ELi0ELb1EtLb0EEEvNS_8PwParamsE": "7e256e4ae45ccaca",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi1ELi1ELb0EtLb0EEEvNS_8PwParamsE": "429c21a9fe5ebab6",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi1ELi1ELb1EtLb0EEEvNS_8PwParamsE": "d9c40776a4476926",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi1ELi2ELb0EtLb0EEEvNS_8PwParamsE": "8b6b75c4eee2c0ea",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi2ELi0ELb0EDF16_Lb0EEEvNS_8PwParamsE": "e7d2cc0cef63dd0f",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi2ELi0ELb0EtLb0EEEvNS_8PwParamsE": "375bf79d7242c9f1",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi2ELi0ELb1EDF16_Lb0EEEvNS_8PwParamsE": "dc0797fc6b82064c",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi2ELi0ELb1EtLb0EEEvNS_8PwParamsE": "5297710353135064",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi2ELi1ELb0EtLb0EEEvNS_8PwParamsE": "784a9977379ff096",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi2ELi1ELb1EtLb0EEEvNS_8PwParamsE": "4d2dca819be85ee6",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi2ELi2ELb0EtLb0EEEvNS_8PwParamsE": "3afd47caa2cebc50",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi3ELi0ELb0EDF16_Lb0EEEvNS_8PwParamsE": "83a257d8d5b0eaa4",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi3ELi0ELb0EtLb0EEEvNS_8PwParamsE": "6ea0f835ed686996",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi3ELi0ELb1EDF16_Lb0EEEvNS_8PwParamsE": "e124050a653dc4d4",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi3ELi0ELb1EtLb0EEEvNS_8PwParamsE": "a84663338ad04221",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi3ELi1ELb0EtLb0EEEvNS_8PwParamsE": "01cd112f59157fd1",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi3ELi1ELb1EtLb0EEEvNS_8PwParamsE": "289ed4a2c288213c",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi3ELi2ELb0EtLb0EEEvNS_8PwParamsE": "71827c7e44ea8b12",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi4ELi0ELb0EDF16_Lb0EEEvNS_8PwParamsE": "3ab2ae8f2d3ad06d",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi4ELi0ELb0EtLb0EEEvNS_8PwParamsE": "0db7d6d49d8d1420",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi4ELi0ELb1EDF16_Lb0EEEvNS_8PwParamsE": "0bed766a2618f23a",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi4ELi0ELb1EtLb0EEEvNS_8PwParamsE": "d1266f942e64e4ce",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi4ELi1ELb0EtLb0EEEvNS_8PwParamsE": "fc3674e12f4ba577",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi4ELi1ELb1EtLb0EEEvNS_8PwParamsE": "8ede4dbe173ae298",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi4ELi1ELb1EtLb1EEEvNS_8PwParamsE": "ef13598531ee60c9",
    "_ZN12_GLOBAL__N_19pw_kernelItLi2ELi4ELi2ELb0EtLb0EEEvNS_8PwParamsE": "7f73627b1e61fdda",
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.skipif(_hipcc_version() != HIPCC_DERIVED_WITH, reason=f"digests read off hipcc {HIPCC_DERIVED_WITH}")
def test_pointwise_kernels_compile_to_the_same_isa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "pointwise.s")
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-result", "-S", "--cuda-device-only",
           os.path.join(ROOT, "biapy_amd", "csrc", "pointwise.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = kernel_digests(open(out).read())
    assert got == POINTWISE_ISA, sorted(set(got.items()) ^ set(POINTWISE_ISA.items()))[:6]

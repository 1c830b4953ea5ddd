"""bpx_convT3d_k2s2_bwd without a GPU: the C-ABI is declared, exported and bound; the compiled one-pass kernel (wgrad_ct_kernel<2, 2, 2, DG = true>,
hipcc cross-compiles gfx950 here) uses no scratch and leaves room for the two workgroups per CU its launch plan (pick_ct) counts on; the streaming
64 -> 64 instance (wgrad_ct_dma_kernel<4, 4, 32, .., DG = true>) uses no scratch and keeps its ring."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FUSED = r"wgrad_ct_kernelILi2ELi2ELi2ELb1EE"       # <NS = 2, SZ = 2, MC = 2, DG = true>
PLAIN = r"wgrad_ct_kernelILi2ELi2ELi2ELb0EE"
FUSED_STREAM = r"wgrad_ct_dma_kernelILi4ELi4ELi32ELb[01]ELb1EE"      # <MC = 4, NS = 4, TV = 32, XF16, DG = true>
PLAIN_STREAM = r"wgrad_ct_dma_kernelILi4ELi4ELi32ELb[01]ELb0EE"


def test_entry_is_declared_exported_and_bound():
    from biapy_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    m = re.search(r"int\s+bpx_convT3d_k2s2_bwd\s*\(([^;]*)\)\s*;", hdr)
    assert m, "bpx_convT3d_k2s2_bwd is not declared in include/biapy_amd.h"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert len(params) == 15, params
    assert [p.split()[-1].lstrip("*") for p in params] == ["dtype", "N", "D", "H", "W", "sz", "x", "dy", "w_packed_T_d", "dx", "dw_d", "db_d", "ws_d",
                                                           "ws_bytes", "stream"]
    for name in ("bpx_convT3d_k2s2_bwd", "bpx_debug_set_convt_bwd", "bpx_debug_convt_bwd_launches",
                 "bpx_convT3d_k2s2_wgrad", "bpx_convT3d_k2s2_dgrad", "bpx_convT3d_k2s2_wgrad_workspace"):     # the two separate entries stay
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
    argtypes, restype = _lib._SIGS["bpx_convT3d_k2s2_bwd"]
    assert len(argtypes) == 15 and [i for i, a in enumerate(argtypes) if a is _lib.Tensor] == [6, 7, 9]
    assert _lib.lib.bpx_debug_convt_bwd_launches() == 0


def test_engines_call_the_one_entry():
    """Both engines run the transposed conv's backward through ResUNetEngine._convT_bwd, the one caller of the entry; neither calls the separate dgrad."""
    src = {f: open(os.path.join(ROOT, "biapy_amd", f)).read() for f in ("engine.py", "unet_engine.py")}
    helper = src["engine.py"].split("    def _convT_bwd(", 1)[1].split("\n    def ", 1)[0]
    assert "bpx_convT3d_k2s2_bwd(" in helper
    for f, text in src.items():
        assert "self._convT_bwd(" in text and "bpx_convT3d_k2s2_dgrad(" not in text and "bpx_convT3d_k2s2_wgrad(" not in text, f


@pytest.fixture(scope="module")
def wgrad_resources():
    """{mangled kernel name: {VGPRs, AGPRs, ScratchSize, Occupancy, LDS Size}} of wgrad.hip from hipcc's kernel-resource-usage remarks."""
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc to cross-compile the kernels")
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-result", "--cuda-device-only", "-c",   # the Makefile's flags
           "-Rpass-analysis=kernel-resource-usage", os.path.join(ROOT, "biapy_amd", "csrc", "wgrad.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)} failed:\n{r.stderr[-3000:]}"
    out, cur = {}, None
    for line in r.stderr.split("\n"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def _one(res, pattern):
    hits = [(k, v) for k, v in res.items() if re.search(pattern, k)]
    assert len(hits) == 1, f"{pattern}: {[k for k, _ in hits]}"
    return hits[0][1]


def test_one_pass_kernel_has_no_scratch_and_two_workgroups_per_cu(wgrad_resources):
    r = _one(wgrad_resources, FUSED)
    assert r["ScratchSize"] == 0, r
    assert r["Occupancy"] >= 2, r                       # 256 threads = one wave per SIMD and workgroup: two workgroups per CU
    assert 2 * r["LDS Size"] <= 160 * 1024, r           # both fit the CU's 160 KB
    assert r["VGPRs"] + r["AGPRs"] <= 256, r


def test_streaming_one_pass_kernels_have_no_scratch_and_keep_the_ring(wgrad_resources):
    """64 -> 64: both element types of x; one workgroup per CU as before (512 registers per lane), the three-stage ring of the plain instance."""
    hits = [(k, v) for k, v in wgrad_resources.items() if re.search(FUSED_STREAM, k)]
    plain = [v for k, v in wgrad_resources.items() if re.search(PLAIN_STREAM, k)]
    assert len(hits) == 2 and len(plain) == 2, [k for k, _ in hits]
    for k, r in hits:
        assert r["ScratchSize"] == 0 and r["Occupancy"] >= 1 and r["VGPRs"] + r["AGPRs"] <= 512, (k, r)
        assert r["LDS Size"] == plain[0]["LDS Size"] and r["LDS Size"] <= 160 * 1024, (k, r)


def test_plain_instance_kept_its_registers(wgrad_resources):
    """The dgrad phase is compiled into its own instance: the tile kernel every other caller launches is the one it was (126 VGPRs recorded in
    profiles/kernel_resources.txt; the bar is the occupancy it is launched for, not that figure)."""
    r = _one(wgrad_resources, PLAIN)
    assert r["ScratchSize"] == 0 and r["Occupancy"] >= 2 and r["LDS Size"] == _one(wgrad_resources, FUSED)["LDS Size"], r

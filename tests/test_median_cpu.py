"""Median filter - what can be checked without a GPU: ``bpx_median_filter`` is declared, exported and bound; every host-side refusal names its
cause, in the order of the argument list, before anything is launched; ``prepost.median_filter`` / ``median_filter_axes`` refuse bad arguments
and CPU tensors in the house order; the NumPy twin the GPU tests hold the device against (tests/median_ref.py) is
``scipy.ndimage.median_filter`` as values on every NaN-free input of those tests and gives the hand-made cases of the definition; and no
instance of the compiled kernel spills."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import median_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
A = 4096                                   # any non-null, aligned "device" address: nothing is launched
F32, U8 = 0, 3
REFLECT, NEAREST, CONSTANT = 0, 1, 2


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_entry_point_is_declared_exported_and_bound():
    from biapy_amd import _lib as L
    from biapy_amd import prepost

    header, source, core = _read("include", "biapy_amd.h"), _read("biapy_amd", "csrc", "median.hip"), _read("biapy_amd", "csrc", "median_core.h")
    assert re.findall(r'extern "C" \w+ (\w+)\(', source) == ["bpx_median_filter"]
    assert re.search(r"^int bpx_median_filter\(const void\* in_d, int dtype, int Z, int Y, int X, int sz, int sy, int sx, int mode, double cval, "
                     r"void\* out_d,\s+bpx_stream_t stream\);", header, re.M)
    vp, i, d = L.C.c_void_p, L.C.c_int, L.C.c_double
    assert "bpx_median_filter" in L.EXPORTS and L._SIGS["bpx_median_filter"] == ([vp, i, i, i, i, i, i, i, i, d, vp, vp], i)
    assert (L.F32, L.U8) == (F32, U8)
    make = _read("biapy_amd", "csrc", "Makefile")
    assert "median.hip" in make and re.search(r"^median\.o:.*median_core\.h.*peaks_core\.h", make, re.M)
    # the shared steps, not a copy: the kernel file defines no MEDIAN_HD function and calls the core's; the core takes the float key from peaks_core.h
    assert '#include "median_core.h"' in source and not re.search(r"\bMEDIAN_HD\b", source)
    for call in ("median_stage(", "median_lane<", "median_plan(", "median_instance(", "median_cval_key("):
        assert call in source, call
    assert '#include "peaks_core.h"' in core and "peaks_okey(" in core and "peaks_unokey(" in core and "0x80000000" not in core.split("#pragma once")[1]
    for fn in ("median_key", "median_unkey", "median_cval_key", "median_load_key", "median_store_key", "median_src", "median_plan", "median_instance",
               "median_stage", "median_walk", "median_next", "median_cx", "median_ends", "median_shrink", "median_select", "median_lane"):
        assert re.search(r"MEDIAN_HD \w+ %s\(" % fn, core), fn
    check = _read("scripts", "median_cpu_check.cpp")
    assert '#include "median_core.h"' in check and "int main()" in check and "-fsanitize=address,undefined" in check
    for call in ("median_select<", "median_src(", "median_plan(", "median_stage(", "median_lane<", "median_instance(", "std::nth_element"):
        assert call in check, call
    assert not re.search(r"\bMEDIAN_HD\b", check)
    assert callable(prepost.median_filter) and callable(prepost.median_filter_axes)
    assert prepost._MEDIAN_MAX_WINDOW == int(re.search(r"MEDIAN_MAX_WINDOW = (\d+);", core).group(1)) == 125
    assert prepost._MEDIAN_MAX_SIZE == int(re.search(r"MEDIAN_MAX_SIZE = (\d+);", core).group(1)) == 15
    modes = dict(re.findall(r"MEDIAN_(REFLECT|NEAREST|CONSTANT) = (\d)", core))
    assert {k.lower(): int(v) for k, v in modes.items()} == prepost._MEDIAN_MODES == {"reflect": REFLECT, "nearest": NEAREST, "constant": CONSTANT}
    instances = [int(v) for v in re.search(r"MEDIAN_INSTANCES\[MEDIAN_NUM_INSTANCES\] = \{([\d, ]+)\}", core).group(1).split(",")]
    assert instances == sorted(instances) and instances[-1] == 125 and all(f"median_launch<{w}>" in source for w in instances)
    assert 45 not in instances and 21 not in instances                      # the padded sizes of the device tests stay padded


def test_host_checks_answer_without_a_device():
    from biapy_amd import _lib as L

    lib = L.lib

    def err():
        return lib.bpx_last_error().decode()

    def med(in_d=A, dtype=F32, Z=4, Y=5, X=6, sz=3, sy=3, sx=3, mode=REFLECT, cval=0.0, out_d=2 * A):
        return lib.bpx_median_filter(in_d, dtype, Z, Y, X, sz, sy, sx, mode, cval, out_d, None)

    for kw in (dict(in_d=None), dict(out_d=None), dict(in_d=None, out_d=None)):
        assert med(**kw) != 0 and "null pointer" in err(), kw
    for kw in (dict(Z=0), dict(Y=0), dict(X=0), dict(Z=-1), dict(X=-7)):
        assert med(**kw) != 0 and "extents must be at least 1" in err(), kw
    for shape in ((2048, 1024, 1024), (1, 65536, 32768), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert med(Z=shape[0], Y=shape[1], X=shape[2]) != 0 and "2^31 voxels or more" in err(), shape
    for dtype in (1, 2, 4, 5, 6, 7, -1):                                                    # int32 (6) among them
        assert med(dtype=dtype) != 0 and "dtype must be float32 or uint8" in err(), dtype
    for kw in (dict(sz=0), dict(sy=2), dict(sx=4), dict(sx=17), dict(sz=-3), dict(sy=16), dict(sz=1, sy=1, sx=14)):
        assert med(**kw) != 0 and "sizes must be odd and in 1..15" in err(), kw
    for kw in (dict(sz=5, sy=5, sx=7), dict(sz=1, sy=9, sx=15), dict(sz=15, sy=15, sx=15), dict(sz=3, sy=3, sx=15)):
        assert med(**kw) != 0 and "at most 125 are supported" in err(), kw
    for mode in (-1, 3, 4, 100):
        assert med(mode=mode) != 0 and "unknown mode" in err(), mode
    for cval in (float("nan"), float("inf"), -float("inf"), 1e39):
        assert med(cval=cval) != 0 and "cval must be finite" in err(), cval
        assert med(cval=cval, mode=CONSTANT) != 0 and "cval must be finite" in err(), cval
    for cval in (0.5, -1.0, 256.0, float("nan"), float("inf"), 1e10):
        assert med(dtype=U8, cval=cval) != 0 and "integer in 0..255" in err(), cval
    assert med(out_d=A) != 0 and "out_d must not be in_d" in err()
    for kw in (dict(in_d=A + 2), dict(out_d=2 * A + 1), dict(in_d=A + 3, out_d=2 * A + 3)):
        assert med(**kw) != 0 and "4-byte aligned" in err(), kw
    # the order: each call fails every later check too and names the earlier one
    assert med(in_d=None, Z=0) != 0 and "null pointer" in err()
    assert med(Z=0, dtype=6, sz=2) != 0 and "extents" in err()
    assert med(Z=2048, Y=1024, X=1024, dtype=6, sz=2) != 0 and "2^31" in err()
    assert med(dtype=6, sz=2, mode=9) != 0 and "dtype" in err()
    assert med(sz=2, sy=15, sx=15, mode=9) != 0 and "sizes must be odd" in err()
    assert med(sz=5, sy=5, sx=7, mode=9, cval=float("nan")) != 0 and "at most 125" in err()
    assert med(mode=9, cval=float("nan"), out_d=A) != 0 and "unknown mode" in err()
    assert med(cval=float("nan"), out_d=A + 2, in_d=A + 2) != 0 and "cval" in err()
    assert med(out_d=A + 2, in_d=A + 2) != 0 and "out_d must not be in_d" in err()
    assert med(in_d=A + 2) != 0 and "4-byte aligned" in err()
    # what is allowed up to the last check made here: the largest volume, the largest window, uint8 at any byte (it fails on out_d == in_d only)
    assert med(Z=1, Y=1, X=2 ** 31 - 1, sz=1, sy=1, sx=15, mode=CONSTANT, cval=-3.0e38, out_d=A) != 0 and "out_d must not be" in err()
    assert med(dtype=U8, in_d=A + 1, out_d=A + 1, sz=5, sy=5, sx=5, mode=NEAREST, cval=255.0) != 0 and "out_d must not be" in err()


def test_prepost_refuses_in_the_house_order():
    from biapy_amd import prepost as P

    x = torch.rand(4, 5, 6)
    for t in (x, x[0], (x * 255).to(torch.uint8), x > 0.5):
        with pytest.raises(RuntimeError, match="no CPU path"):
            P.median_filter(t)
        with pytest.raises(RuntimeError, match="no CPU path"):
            P.median_filter(t, 5, "constant", 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.median_filter(x, (1, 1, 15), "nearest")
    for dt in (torch.int32, torch.int64, torch.float16, torch.float64, torch.int8):
        with pytest.raises(NotImplementedError, match="works on float32, uint8 or bool"):
            P.median_filter(x.to(dt))
    for bad in (x.view(-1), x[None], x[0, 0, 0]):
        with pytest.raises(ValueError, match="2-D .* or 3-D"):
            P.median_filter(bad)
    with pytest.raises(NotImplementedError, match="empty axis"):
        P.median_filter(torch.zeros(4, 0, 6))
    for size, t in (((3, 3), x), ((3, 3, 3), x[0]), ((3,), x), ([1, 3, 3, 3], x)):
        with pytest.raises(ValueError, match="size must be an int or one int per axis"):
            P.median_filter(t, size)
    for size in (0, -3, (3, 0, 3)):
        with pytest.raises(ValueError, match="size must be at least 1"):
            P.median_filter(x, size)
    for size in (2, 4, (3, 3, 2), (1, 14, 1)):
        with pytest.raises(NotImplementedError, match="size must be odd"):
            P.median_filter(x, size)
    for size in (17, (1, 1, 17), (21, 1, 1)):
        with pytest.raises(NotImplementedError, match="at most 15"):
            P.median_filter(x, size)
    for size in (7, (5, 5, 7), (1, 9, 15), (3, 3, 15)):
        with pytest.raises(NotImplementedError, match="at most 125 are supported"):
            P.median_filter(x, size)
    for mode in ("mirror", "wrap"):
        with pytest.raises(NotImplementedError, match="is not offered"):
            P.median_filter(x, 3, mode)
    for mode in ("grid-wrap", "symmetric", "", None):
        with pytest.raises(ValueError, match="mode must be"):
            P.median_filter(x, 3, mode)
    for cval in (float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="cval must be finite"):
            P.median_filter(x, 3, "constant", cval)
    for cval in (0.5, -1, 256, float("nan")):
        for t in ((x * 255).to(torch.uint8), x > 0.5):
            with pytest.raises(ValueError, match="integer in 0..255"):
                P.median_filter(t, 3, "constant", cval)
    # the order: dtype, rank, empty axis, size, mode, cval, and the device last
    with pytest.raises(NotImplementedError, match="works on"):
        P.median_filter(x[None].to(torch.float64), 2, "wrap", float("nan"))
    with pytest.raises(ValueError, match="2-D .* or 3-D"):
        P.median_filter(x[None], 2, "wrap", float("nan"))
    with pytest.raises(NotImplementedError, match="empty axis"):
        P.median_filter(torch.zeros(4, 0, 6), 2, "wrap", float("nan"))
    with pytest.raises(NotImplementedError, match="size must be odd"):
        P.median_filter(x, 2, "wrap", float("nan"))
    with pytest.raises(NotImplementedError, match="is not offered"):
        P.median_filter(x, 3, "wrap", float("nan"))
    with pytest.raises(ValueError, match="cval"):
        P.median_filter(x, 3, "reflect", float("nan"))
    for name in ("footprint", "origin", "output", "axes"):                                    # not offered
        with pytest.raises(TypeError):
            P.median_filter(x, 3, **{name: None})
    # median_filter_axes: its own refusals first, then median_filter's for every step, the device last
    for axes in ("xy", "yx", "yz", "zy", "zx", "xz", "z", "y", "x", "xyz"):
        with pytest.raises(RuntimeError, match="no CPU path"):
            P.median_filter_axes(x, axes, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.median_filter_axes(x, ["xy", "z"], [5, 3])
    for axes in ("xx", "zyx", "w", "", "XY"):
        with pytest.raises(ValueError, match="axes must be one of"):
            P.median_filter_axes(x, axes, 3)
    for axes, size in ((["xy", "z"], 3), (["xy", "z"], [3]), (["xy"], [3, 3])):
        with pytest.raises(ValueError, match="one size each"):
            P.median_filter_axes(x, axes, size)
    with pytest.raises(ValueError, match="takes a 3-D"):
        P.median_filter_axes(x[0], "xy", 3)
    with pytest.raises(NotImplementedError, match="works on"):
        P.median_filter_axes(x.to(torch.float64), "xy", 3)
    with pytest.raises(NotImplementedError, match="size must be odd"):
        P.median_filter_axes(x, ["xy", "z"], [3, 4])                                          # the second step is refused before the first is launched
    with pytest.raises(NotImplementedError, match="at most 125"):
        P.median_filter_axes(x, "xyz", 7)
    doc = P.median_filter.__doc__
    for phrase in ("rank ``W // 2``", "``-0.0`` sorts", "product-defined", "majority vote", "captured in a graph"):
        assert phrase in doc, phrase


# ---- the twin against SciPy --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", (np.float32, np.uint8), ids=("float32", "uint8"))
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_twin_equals_scipy_on_every_device_input_without_nan(shape, dtype):
    n = 0
    for x, kind, size, mode, cval in R.cases(shape, dtype):
        if R.has_nan(x):
            continue
        got = R.median_ref(x, size, mode, cval)
        assert got.dtype == x.dtype and got.shape == x.shape
        np.testing.assert_array_equal(got, R.scipy_median(x, size, mode, cval), err_msg=str((kind, shape, size, mode, cval)))
        n += 1
    kinds = len(R.F32_KINDS) - 1 if dtype == np.float32 else len(R.U8_KINDS)
    modes = len(R.F32_MODES) if dtype == np.float32 else len(R.U8_MODES)
    sizes = sum(R.per_axis(s, len(shape)) is not None for s in R.SIZES)
    assert n == kinds * modes * sizes and sizes == (10 if len(shape) == 2 else len(R.SIZES))


def test_twin_on_a_larger_volume_and_the_axes_form():
    p = R.probability((12, 40, 44))
    for size in ((1, 5, 5), (3, 3, 3), (5, 1, 1)):
        np.testing.assert_array_equal(R.median_ref(p, size), R.scipy_median(p, size, "reflect", 0.0))
    np.testing.assert_array_equal(R.median_axes_ref(p, "xy", 5), R.median_ref(p, (1, 5, 5)))
    np.testing.assert_array_equal(R.median_axes_ref(p, "zx", 3), R.median_ref(p, (3, 1, 3)))
    np.testing.assert_array_equal(R.median_axes_ref(p, ["xy", "z"], [5, 3]), R.median_ref(R.median_ref(p, (1, 5, 5)), (3, 1, 1)))
    b = p > 0.5
    got = R.median_ref(b, 3)
    assert got.dtype == np.bool_
    np.testing.assert_array_equal(got, R.scipy_median(b.view(np.uint8), 3, "reflect", 0).astype(bool))


def test_twin_hand_made_cases():
    const = np.full((3, 4, 5), 0.75, np.float32)
    for mode in ("reflect", "nearest"):
        np.testing.assert_array_equal(R.median_ref(const, 3, mode), const)
    np.testing.assert_array_equal(R.median_ref(const, 3, "constant", 0.75), const)
    assert R.median_ref(const, 3, "constant", 0.0)[0, 0, 0] == 0.0 and R.median_ref(const, 3, "constant", 0.0)[1, 1, 1] == 0.75     # 19 of a corner's 27 are cval
    # a single voxel: itself under reflect / nearest whatever the window, cval under constant as soon as the window holds more than the voxel
    one = np.array([[[0.3]]], np.float32)
    for size in (1, 3, 5, (1, 1, 15), (1, 11, 11)):
        assert R.median_ref(one, size, "reflect")[0, 0, 0] == R.median_ref(one, size, "nearest")[0, 0, 0] == np.float32(0.3)
        assert R.median_ref(one, size, "constant", 0.25)[0, 0, 0] == (np.float32(0.3) if size == 1 else np.float32(0.25))
    # one outlier goes, a step edge stays where it is
    img = np.zeros((9, 9), np.float32)
    img[:, 5:] = 1.0
    spoiled = img.copy()
    spoiled[4, 2] = 50.0
    np.testing.assert_array_equal(R.median_ref(spoiled, 3), img)
    np.testing.assert_array_equal(R.median_ref(img, 5), img)
    # -0.0 sorts below +0.0: the median of (-0.0, -0.0, +0.0) is -0.0, of (-0.0, +0.0, +0.0) it is +0.0 - equal as values either way
    z = np.array([[-0.0, -0.0, -0.0, 0.0, 0.0, 0.0]], np.float32)
    got = R.median_ref(z, (1, 3), "nearest")
    assert np.signbit(got).tolist() == [[True, True, True, False, False, False]]
    z2 = np.array([[-0.0, 0.0, -0.0, 0.0, 0.0]], np.float32)
    assert np.signbit(R.median_ref(z2, (1, 3), "nearest")).tolist() == [[True, True, False, False, False]]
    # NaNs at the ends: a negative-sign NaN below -inf, a positive-sign NaN above +inf, so one of each in a window of three leaves the third
    row = np.array([[0xFFC00002, 0xFF800000, 0x7FC00001, 0x40000000, 0xFFC00002, 0x7F800000, 0x7FC00001]], np.uint32).view(np.float32)
    got = R.median_ref(row, (1, 3), "nearest")
    assert R.bits(got).tolist() == [[0xFFC00002, 0xFF800000, 0x40000000, 0x40000000, 0x40000000, 0x7F800000, 0x7FC00001]]
    # denormals and uint8 come back as they went in
    d = np.array([[1, 2, 3, 0x80000001, 0x80000002]], np.uint32).view(np.float32)
    assert R.bits(R.median_ref(d, (1, 3), "nearest")).tolist() == [[1, 2, 2, 0x80000001, 0x80000002]]
    u = np.array([[0, 255, 255, 3, 0, 0]], np.uint8)
    assert R.median_ref(u, (1, 3), "constant", 255).tolist() == [[255, 255, 255, 3, 0, 0]]
    assert R.median_ref(u, (1, 3), "reflect").tolist() == [[0, 255, 255, 3, 0, 0]]


# ---- the compiled kernel -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc to cross-compile the kernel to ISA")
def test_no_instance_of_the_kernel_spills(tmp_path):
    out = str(tmp_path / "median.s")
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-result", "-S", "--cuda-device-only",     # the Makefile's flags
           os.path.join(ROOT, "biapy_amd", "csrc", "median.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)} failed:\n{r.stderr[-3000:]}"
    text = open(out).read()
    kernels = re.findall(r"\.name:\s+(_Z\w*median_kernel\w*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    core = _read("biapy_amd", "csrc", "median_core.h")
    instances = re.search(r"MEDIAN_INSTANCES\[MEDIAN_NUM_INSTANCES\] = \{([\d, ]+)\}", core).group(1).split(",")
    assert len(kernels) == len(instances) == 10, kernels
    for name, private in kernels:
        assert int(private) == 0, f"{name} keeps {private} bytes of scratch per lane"

"""Separable / Gaussian filter - what can be checked without a GPU: ``bpx_sepfilter`` and ``bpx_sepfilter_workspace`` are declared, exported and
bound; every host-side refusal names its cause, in the stated order, before anything is launched; ``prepost.separable_filter`` /
``gaussian_filter`` / ``gaussian_laplace`` refuse bad arguments and CPU tensors in the house order; the restated Gaussian weights are SciPy's
bit for bit; the NumPy twin the GPU tests hold the device against (tests/gauss_ref.py) stays within the derived bound of SciPy's float64
result on every input of those tests; and no instance of the compiled kernels spills."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import gauss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
A = 1 << 30                                # any non-null, aligned "device" address: nothing is launched
REFLECT, MIRROR, NEAREST, CONSTANT = 0, 1, 2, 3


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_entry_points_are_declared_exported_and_bound():
    from biapy_amd import _lib as L
    from biapy_amd import prepost

    header, source, core = _read("include", "biapy_amd.h"), _read("biapy_amd", "csrc", "sepfilter.hip"), _read("biapy_amd", "csrc", "sepfilter_core.h")
    assert re.findall(r'extern "C" \w+ (\w+)\(', source) == ["bpx_sepfilter_workspace", "bpx_sepfilter"]
    assert re.search(r"^int64_t bpx_sepfilter_workspace\(int Z, int Y, int X, int rz, int ry, int rx\);", header, re.M)
    assert re.search(r"^int bpx_sepfilter\(const void\* in_d, int Z, int Y, int X, const float\* wz, int rz, const float\* wy, int ry, const float\* wx, "
                     r"int rx, int mode,\s+double cval, void\* out_d, void\* ws_d, int64_t ws_bytes, bpx_stream_t stream\);", header, re.M)
    vp, i, i64, d = C.c_void_p, C.c_int, C.c_int64, C.c_double
    assert L._SIGS["bpx_sepfilter_workspace"] == ([i, i, i, i, i, i], i64)
    assert L._SIGS["bpx_sepfilter"] == ([vp, i, i, i, vp, i, vp, i, vp, i, i, d, vp, vp, i64, vp], i)
    assert {"bpx_sepfilter", "bpx_sepfilter_workspace"} <= set(L.EXPORTS)
    make = _read("biapy_amd", "csrc", "Makefile")
    assert "sepfilter.hip" in make and re.search(r"^sepfilter\.o:.*sepfilter_core\.h", make, re.M) and "-ffp-contract=off" in make
    # the shared steps, not a copy: the kernel file defines no SEPFILTER_HD function and calls the core's; no fused multiply-add is asked for
    assert '#include "sepfilter_core.h"' in source and not re.search(r"\bSEPFILTER_HD\b", source)
    for call in ("sepfilter_stage_lanes(", "sepfilter_lane(", "sepfilter_stage_rows(", "sepfilter_row(", "sepfilter_plan("):
        assert call in source, call
    for fn in ("sepfilter_fold", "sepfilter_plan", "sepfilter_window", "sepfilter_stage_lanes", "sepfilter_lane", "sepfilter_stage_rows", "sepfilter_row"):
        assert re.search(r"SEPFILTER_HD \w+ %s\(" % fn, core), fn
    assert "fmaf(" not in source and "fmaf(" not in core.split("#pragma once")[1] and not re.search(r"atomic\w*\(", source + core)
    check = _read("scripts", "sepfilter_cpu_check.cpp")
    assert '#include "sepfilter_core.h"' in check and "int main()" in check and "-fsanitize=address,undefined" in check
    for call in ("sepfilter_fold(", "sepfilter_plan(", "sepfilter_window<", "sepfilter_stage_lanes(", "sepfilter_lane(", "sepfilter_stage_rows(", "sepfilter_row("):
        assert call in check, call
    assert not re.search(r"\bSEPFILTER_HD\b", check)
    for f in (prepost.separable_filter, prepost.gaussian_filter, prepost.gaussian_laplace):
        assert callable(f)
    assert prepost._SEPFILTER_MAX_RADIUS == int(re.search(r"SEPFILTER_MAX_RADIUS = (\d+);", core).group(1)) == R.MAX_RADIUS == 32
    modes = re.search(r"SEPFILTER_REFLECT = (\d), SEPFILTER_MIRROR = (\d), SEPFILTER_NEAREST = (\d), SEPFILTER_CONSTANT = (\d)", core).groups()
    assert dict(zip(("reflect", "mirror", "nearest", "constant"), map(int, modes))) == prepost._SEPFILTER_MODES
    assert prepost._SEPFILTER_MODES == {"reflect": REFLECT, "mirror": MIRROR, "nearest": NEAREST, "constant": CONSTANT}
    assert "_gaussian_kernel1d" not in _read("biapy_amd", "prepost.py")                      # restated, not imported


def _weights(r, fill=0.5):
    return (C.c_float * (2 * r + 1))(*([fill] * (2 * r + 1)))


def test_host_checks_answer_without_a_device():
    from biapy_amd import _lib as L

    lib = L.lib
    n = 4 * 5 * 6 * 4
    w1, w32, w0 = _weights(1), _weights(32), _weights(0)

    def err():
        return lib.bpx_last_error().decode()

    def sep(in_d=A, Z=4, Y=5, X=6, wz=w1, rz=1, wy=w1, ry=1, wx=w1, rx=1, mode=REFLECT, cval=0.0, out_d=2 * A, ws_d=3 * A, ws_bytes=n):
        p = [None if w is None else C.cast(w, C.c_void_p).value for w in (wz, wy, wx)]
        return lib.bpx_sepfilter(in_d, Z, Y, X, p[0], rz, p[1], ry, p[2], rx, mode, cval, out_d, ws_d, ws_bytes, None)

    for kw in (dict(in_d=None), dict(out_d=None), dict(wz=None), dict(wy=None, ry=0), dict(wx=None, rx=32), dict(wx=None, rx=40)):
        assert sep(**kw) != 0 and "null pointer" in err(), kw
    for kw in (dict(Z=0), dict(Y=0), dict(X=0), dict(Z=-1), dict(X=-7)):
        assert sep(**kw) != 0 and "extents must be at least 1" in err(), kw
    for shape in ((2048, 1024, 1024), (1, 65536, 32768), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert sep(Z=shape[0], Y=shape[1], X=shape[2]) != 0 and "2^31 voxels or more" in err(), shape
    for kw in (dict(rz=33), dict(ry=-1), dict(rx=100), dict(wz=w32, rz=64), dict(rx=-5)):
        assert sep(**kw) != 0 and "must be in 0..32" in err(), kw
    for bad in (float("nan"), float("inf"), -float("inf")):
        w = _weights(1)
        w[2] = bad
        for kw in (dict(wz=w), dict(wy=w), dict(wx=w)):
            assert sep(**kw) != 0 and "a weight is not finite" in err(), (bad, kw)
    for mode in (-1, 4, 5, 100):
        assert sep(mode=mode) != 0 and "unknown mode" in err(), mode
    for cval in (float("nan"), float("inf"), -float("inf"), 1e39):
        assert sep(cval=cval) != 0 and "cval must be finite" in err(), cval
        assert sep(cval=cval, mode=CONSTANT) != 0 and "cval must be finite" in err(), cval
    for kw in (dict(ws_bytes=n - 1), dict(ws_bytes=0), dict(ws_d=None), dict(ws_bytes=-8), dict(wz=None, rz=-1, ws_bytes=n - 4)):
        assert sep(**kw) != 0 and "workspace too small" in err(), kw
    for kw in (dict(out_d=A), dict(out_d=A + 16), dict(out_d=A - n + 4)):
        assert sep(**kw) != 0 and "out_d must not be in_d" in err(), kw
    for kw in (dict(ws_d=A), dict(ws_d=2 * A), dict(ws_d=2 * A + n - 4), dict(ws_d=A - 8)):
        assert sep(**kw) != 0 and "ws_d must not be" in err(), kw
    for kw in (dict(in_d=A + 2), dict(out_d=2 * A + 1), dict(ws_d=3 * A + 3)):
        assert sep(**kw) != 0 and "4-byte aligned" in err(), kw
    # the order: each call fails every later check too and names the earlier one
    assert sep(in_d=None, Z=0) != 0 and "null pointer" in err()
    assert sep(wx=None, Z=0) != 0 and "null pointer" in err()
    assert sep(Z=0, rz=40, mode=9) != 0 and "extents" in err()
    assert sep(Z=2048, Y=1024, X=1024, rz=40, mode=9) != 0 and "2^31" in err()
    bad = _weights(1, float("nan"))
    assert sep(rz=40, wy=bad, mode=9) != 0 and "must be in 0..32" in err()
    assert sep(wy=bad, mode=9, cval=float("nan")) != 0 and "not finite" in err() and "weight" in err()
    assert sep(mode=9, cval=float("nan"), ws_bytes=0) != 0 and "unknown mode" in err()
    assert sep(cval=float("nan"), ws_bytes=0, out_d=A) != 0 and "cval" in err()
    assert sep(ws_bytes=0, out_d=A) != 0 and "workspace too small" in err()
    assert sep(out_d=A, ws_d=A, in_d=A + 2) != 0 and "out_d must not be in_d" in err()
    assert sep(out_d=A + 4, ws_d=A + 4) != 0 and "out_d must not be in_d" in err()
    assert sep(ws_d=2 * A, in_d=A + 2) != 0 and "ws_d must not be" in err()
    # what is allowed up to the last check made here: one axis needs no workspace, the largest radius, a radius of 0 (alignment is the last check)
    assert sep(wz=None, rz=-1, wy=None, ry=-3, wx=w32, rx=32, ws_d=None, ws_bytes=0, in_d=A + 2) != 0 and "4-byte aligned" in err()
    assert sep(wz=w0, rz=0, wy=None, ry=-1, wx=None, rx=-1, ws_d=None, ws_bytes=0, mode=CONSTANT, cval=-3.0e38, out_d=2 * A + 1) != 0 and "4-byte aligned" in err()
    assert sep(wz=None, rz=-1, wy=None, ry=-1, wx=None, rx=-1, ws_d=None, ws_bytes=0, in_d=A + 1) != 0 and "4-byte aligned" in err()


def test_workspace_formula():
    from biapy_amd import _lib as L

    ws = L.lib.bpx_sepfilter_workspace
    for Z, Y, X in ((4, 5, 6), (1, 17, 70), (1, 1, 1), (1024, 1024, 1024), (1, 1, 2 ** 31 - 1)):
        n = Z * Y * X
        for radii, active in (((-1, -1, -1), 0), ((0, -1, -1), 1), ((-1, 32, -1), 1), ((-1, -7, 4), 1), ((1, 2, -1), 2), ((-1, 0, 0), 2), ((32, -1, 32), 2),
                              ((0, 0, 0), 3), ((4, 4, 4), 3), ((32, 32, 32), 3)):
            assert ws(Z, Y, X, *radii) == (4 * n if active >= 2 else 0), (Z, Y, X, radii)
    for bad in ((0, 5, 6, 1, 1, 1), (4, -1, 6, 1, 1, 1), (4, 5, 0, 1, 1, 1), (2048, 1024, 1024, 1, 1, 1), (4, 5, 6, 33, 1, 1), (4, 5, 6, -1, -1, 33),
                (4, 5, 6, 1, 1000, 1)):
        assert ws(*bad) == -1, bad


def test_prepost_refuses_in_the_house_order():
    from biapy_amd import prepost as P

    x = torch.rand(4, 5, 6)
    for t in (x, x[0]):
        with pytest.raises(RuntimeError, match="no CPU path"):
            P.gaussian_filter(t, 1.0)
        with pytest.raises(RuntimeError, match="no CPU path"):
            P.gaussian_filter(t, 2, 1, "constant", 1.0, 2.0, 3)
        with pytest.raises(RuntimeError, match="no CPU path"):
            P.gaussian_laplace(t, 1.0)
        with pytest.raises(RuntimeError, match="no CPU path"):
            P.separable_filter(t, [None] * t.dim())
        with pytest.raises(RuntimeError, match="no CPU path"):
            P.separable_filter(t, [[1.0, 2.0, 3.0]] + [None] * (t.dim() - 1), "mirror")
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.gaussian_filter(x, (0, 8, 0.5), (0, 2, 1), radius=(None, 32, 1))
    calls = (lambda t, **k: P.gaussian_filter(t, 1.0, **k), lambda t, **k: P.gaussian_laplace(t, 1.0, **k),
             lambda t, **k: P.separable_filter(t, [[0.25, 0.5, 0.25]] * t.dim(), **k))
    for call in calls:
        for dt in (torch.int32, torch.uint8, torch.float16, torch.float64, torch.bool):
            with pytest.raises(NotImplementedError, match=r"works on float32 tensors .*\.float\(\)"):
                call(x.to(dt))
        for bad in (x.view(-1), x[None], x[0, 0, 0]):
            with pytest.raises(ValueError, match="2-D .* or 3-D"):
                call(bad)
        with pytest.raises(NotImplementedError, match="empty axis"):
            call(torch.zeros(4, 0, 6))
        with pytest.raises(NotImplementedError, match="'wrap' is not offered"):
            call(x, mode="wrap")
        for mode in ("grid-wrap", "symmetric", "", None):
            with pytest.raises(ValueError, match="mode must be"):
                call(x, mode=mode)
        for cval in (float("nan"), float("inf"), 1e39):
            with pytest.raises(ValueError, match="cval must be finite"):
                call(x, cval=cval)
    for sigma, t in (((1, 1), x), ((1, 1, 1), x[0]), ((1,), x), ([1, 1, 1, 1], x)):
        with pytest.raises(ValueError, match="sigma must be a scalar or one value per axis"):
            P.gaussian_filter(t, sigma)
    with pytest.raises(ValueError, match="order must be a scalar or one value per axis"):
        P.gaussian_filter(x, 1.0, (0, 1))
    with pytest.raises(ValueError, match="radius must be a scalar or one value per axis"):
        P.gaussian_filter(x, 1.0, radius=(1, 2))
    for sigma in (-1.0, (1, -0.5, 1), float("nan")):
        with pytest.raises(ValueError, match="sigma must not be negative"):
            P.gaussian_filter(x, sigma)
    for order in (3, -1, (0, 0, 4), 1.5):
        with pytest.raises(ValueError, match="order must be 0, 1 or 2"):
            P.gaussian_filter(x, 1.0, order)
    with pytest.raises(ValueError, match="truncate"):
        P.gaussian_filter(x, 1.0, truncate=-1.0)
    for radius in (-1, (1, -2, 1), 1.5):
        with pytest.raises(ValueError, match="radius must be None or a non-negative integer"):
            P.gaussian_filter(x, 1.0, radius=radius)
    with pytest.raises(NotImplementedError, match=r"sigma 9 with truncate 4 needs a radius of 36 voxels; at most 32"):
        P.gaussian_filter(x, 9.0)
    with pytest.raises(NotImplementedError, match=r"sigma 8.2 .* radius of 33"):
        P.gaussian_filter(x, (1.0, 8.2, 1.0))
    with pytest.raises(NotImplementedError, match=r"radius=33 \(sigma 2\)"):
        P.gaussian_filter(x, 2.0, radius=33)
    with pytest.raises(NotImplementedError, match="sigma 9"):
        P.gaussian_laplace(x, 9.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.gaussian_filter(x, (0.0, 100.0, 8.0), truncate=0.3)                                 # radii 0 (skipped), 30, 2
    for weights in (None, [None, None], [[1.0]] * 4, 3.0):
        with pytest.raises(ValueError, match="one entry .* per axis"):
            P.separable_filter(x, weights)
    for w in ([1.0, 2.0], [], [[1.0, 2.0, 3.0]], 2.0):
        with pytest.raises(ValueError, match="1-D sequence of odd length"):
            P.separable_filter(x, [None, w, None])
    for w in ([1.0, float("nan"), 1.0], [float("inf")], [1e39, 0.0, 0.0]):
        with pytest.raises(ValueError, match="finite as float32"):
            P.separable_filter(x, [w, None, None])
    with pytest.raises(NotImplementedError, match="67 taps .* at most 65"):
        P.separable_filter(x, [None, None, [0.0] * 67])
    # the order: dtype, rank, empty axis, the parameters, the radius, the mode, cval, and the device last
    with pytest.raises(NotImplementedError, match="works on"):
        P.gaussian_filter(x[None].double(), -1.0, 5, "wrap", float("nan"))
    with pytest.raises(ValueError, match="2-D .* or 3-D"):
        P.gaussian_filter(x[None], -1.0, 5, "wrap", float("nan"))
    with pytest.raises(NotImplementedError, match="empty axis"):
        P.gaussian_filter(torch.zeros(4, 0, 6), -1.0, 5, "wrap", float("nan"))
    with pytest.raises(ValueError, match="sigma must not be negative"):
        P.gaussian_filter(x, -1.0, 5, "wrap", float("nan"))
    with pytest.raises(ValueError, match="order must be"):
        P.gaussian_filter(x, 9.0, 5, "wrap", float("nan"))
    with pytest.raises(NotImplementedError, match="at most 32"):
        P.gaussian_filter(x, 9.0, 2, "wrap", float("nan"))
    with pytest.raises(NotImplementedError, match="is not offered"):
        P.gaussian_filter(x, 1.0, 2, "wrap", float("nan"))
    with pytest.raises(ValueError, match="mode must be"):
        P.gaussian_filter(x, 1.0, 2, "periodic", float("nan"))
    with pytest.raises(ValueError, match="cval"):
        P.gaussian_filter(x, 1.0, 2, "reflect", float("nan"))
    with pytest.raises(ValueError, match="odd length"):
        P.separable_filter(x, [[1.0, 2.0], [0.0] * 67, None], "wrap", float("nan"))
    with pytest.raises(NotImplementedError, match="67 taps"):
        P.separable_filter(x, [[1.0], [0.0] * 67, None], "wrap", float("nan"))
    with pytest.raises(NotImplementedError, match="is not offered"):
        P.separable_filter(x, [[1.0], None, None], "wrap", float("nan"))
    for name in ("output", "axes", "origin"):                                                  # not offered
        with pytest.raises(TypeError):
            P.gaussian_filter(x, 1.0, **{name: None})
    for f, phrases in ((P.separable_filter, ("product-defined", "no FMA", "captured in a graph", "in that order")),
                       (P.gaussian_filter, ("product-defined", "sigma <= 1e-15", "captured in a graph", "int(truncate * sigma + 0.5)")),
                       (P.gaussian_laplace, ("blob_log", "axis order z, y, x"))):
        for phrase in phrases:
            assert phrase in f.__doc__, phrase


# ---- the weights ------------------------------------------------------------------------------------------------------------------------------------------

def test_restated_weights_are_scipys_bit_for_bit():
    from scipy.ndimage._filters import _gaussian_kernel1d

    from biapy_amd import prepost as P

    n = 0
    for sigma in (0.5, 0.7, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.5, 8.0):
        for order in (0, 1, 2):
            for radius in (int(4.0 * sigma + 0.5), int(2.0 * sigma + 0.5), 1, 32):
                want = _gaussian_kernel1d(float(sigma), order, radius)[::-1]
                for got in (R.gaussian_weights(float(sigma), order, radius), P._gaussian_weights(float(sigma), order, radius)):
                    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), (sigma, order, radius)
                n += 1
    assert n == 120
    ws, m, c = P._gaussian_check(torch.zeros(3, 4, 5), "gaussian_filter", (0.0, 1.0, 8.0), (0, 1, 2), "mirror", 0.25, 4.0, (None, None, 7))
    assert ws[0] is None and (m, c) == (MIRROR, 0.25) and [w.dtype for w in ws[1:]] == [np.float32] * 2 and [w.size for w in ws[1:]] == [9, 15]
    assert np.array_equal(ws[1], _gaussian_kernel1d(1.0, 1, 4)[::-1].astype(np.float32))
    assert np.array_equal(ws[2], _gaussian_kernel1d(8.0, 2, 7)[::-1].astype(np.float32))


# ---- the twin ----------------------------------------------------------------------------------------------------------------------------------------------

def test_fold_equals_numpy_pad_over_several_periods():
    for n in (1, 2, 3, 5, 8):
        base = np.arange(n)
        for r in (1, 4, 8, 32):
            at = np.arange(-r, n + r)
            for mode, np_mode in (("reflect", "symmetric"), ("mirror", "reflect"), ("nearest", "edge")):
                np.testing.assert_array_equal(R.fold(mode, at, n), np.pad(base, r, mode=np_mode), err_msg=str((n, r, mode)))
            want = np.pad(base, r, mode="constant", constant_values=-1)
            np.testing.assert_array_equal(R.fold("constant", at, n), want)


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_twin_is_within_the_bound_of_scipy_on_every_device_input(shape):
    import scipy.ndimage as ndi

    worst, n = 0.0, 0
    for s, kind, mode, cval, kw in R.gaussian_cases():
        if s != shape:
            continue
        x = R.volume(kind, shape)
        ws = R.gaussian_axes(len(shape), kw["sigma"], kw.get("order", 0), kw.get("truncate", 4.0), kw.get("radius"))
        got = R.gaussian_ref(x, mode=mode, cval=cval, **kw)
        ref, bound = R.reference_and_bound(x, ws, mode, cval)
        if kind != "infinities":                                                              # the chained correlate1d is gaussian_filter itself
            np.testing.assert_array_equal(ref, ndi.gaussian_filter(x.astype(np.float64), mode=mode, cval=cval, **kw))
        ratio = R.check_within(got, ref, bound, (shape, kind, mode, cval, kw))
        worst, n = max(worst, ratio), n + 1
    assert n >= 53 and 0 < worst <= 1.0
    print(f"{shape}: {n} cases, largest err / bound {worst:.3f}")


def test_impulse_response_is_the_reversed_weights():
    x = np.zeros((9, 11, 13), np.float32)
    x[4, 5, 6] = 1.0
    wz, wy, wx = [1.0, 2.0, 3.0], [5.0, 7.0, 11.0, 13.0, 17.0], [0.5, 0.25, 0.125]
    got = R.separable_ref(x, [wz, None, None])
    assert got[3:6, 5, 6].tolist() == wz[::-1] and got.sum() == 6.0                           # out[i] = sum_j w[j] x[i + j - r]: w[j] lands at i = c + r - j
    got = R.separable_ref(x, [None, wy, None])
    assert got[4, 3:8, 6].tolist() == wy[::-1]
    got = R.separable_ref(x, [wz, wy, wx])
    np.testing.assert_array_equal(got[3:6, 3:8, 5:8], np.einsum("i,j,k->ijk", wz[::-1], wy[::-1], wx[::-1]).astype(np.float32))
    for order in (0, 1, 2):
        w = R.gaussian_weights(1.5, order, 6)
        line = np.zeros(31, np.float32)
        line[15] = 1.0
        np.testing.assert_array_equal(R.gaussian_ref(line[None], (0.0, 1.5), order)[0, 9:22], w[::-1].astype(np.float32))
    # the first tap is a product alone: -0.0 times a positive weight stays -0.0
    z = np.full((1, 4), -0.0, np.float32)
    assert np.signbit(R.separable_ref(z, [None, [1.0]])).all() and np.signbit(R.separable_ref(z, [None, [0.5, 0.25, 0.25]])).all()


def test_constant_volume_stays_constant_within_the_bound():
    for shape in R.SHAPES:
        x = R.volume("constant", shape)
        for mode in ("reflect", "mirror", "nearest"):
            for sigma in (1.0, 3.0, 8.0):
                ws = R.gaussian_axes(len(shape), sigma)
                got = R.gaussian_ref(x, sigma, mode=mode)
                ref, bound = R.reference_and_bound(x, ws, mode)
                np.testing.assert_allclose(ref, 0.75, rtol=0, atol=1e-14)
                R.check_within(got, ref, bound, (shape, mode, sigma))
                assert (np.abs(got.astype(np.float64) - 0.75) <= bound + 1e-14).all()


def test_laplace_twin_against_scipy_within_the_summed_bound():
    import scipy.ndimage as ndi

    for shape in ((5, 9, 70), (17, 70), (8, 16, 128)):
        x = R.volume("normal", shape)
        for sigma, mode, cval in ((1.0, "reflect", 0.0), (2.0, "constant", 0.25), (1.5, "mirror", 0.0)):
            got = R.laplace_ref(x, sigma, mode, cval)
            ref, bound = 0.0, 0.0
            for ws in R.laplace_axes(len(shape), sigma):
                v, b = R.reference_and_bound(x, ws, mode, cval)
                # the float32 add of a term: one more rounding of the partial sum (at most |sum so far| + |term|, with their own errors)
                ref, bound = ref + v, bound + b
            bound = bound + len(shape) * R.U * (np.abs(ref) + sum(np.abs(R.reference_and_bound(x, ws, mode, cval)[0]) for ws in R.laplace_axes(len(shape), sigma)))
            np.testing.assert_allclose(ref, ndi.gaussian_laplace(x.astype(np.float64), sigma, mode=mode, cval=cval), rtol=1e-12, atol=1e-13)
            assert (np.abs(got - ref) <= bound).all(), (shape, sigma, mode)


# ---- the compiled kernels ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc to cross-compile the kernels to ISA")
def test_no_instance_of_the_kernels_spills_and_denormals_are_kept(tmp_path):
    out = str(tmp_path / "sepfilter.s")
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-result", "-S", "--cuda-device-only",   # the Makefile's flags
           os.path.join(ROOT, "biapy_amd", "csrc", "sepfilter.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)} failed:\n{r.stderr[-3000:]}"
    text = open(out).read()
    kernels = re.findall(r"\.name:\s+(_Z\w*sepfilter_\w*kernel\w*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(kernels) == 2, kernels
    for name, private in kernels:
        assert int(private) == 0, f"{name} keeps {private} bytes of scratch per lane"
    assert re.findall(r"\.amdhsa_float_denorm_mode_32 (\d)", text) == ["3", "3"]              # gradual underflow, as the twin's

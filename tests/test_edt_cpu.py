"""Euclidean distance transform - what can be checked without a GPU: the entry points are declared, exported and bound; every host-side
refusal names its cause before anything is launched; the workspace is bounded by the threads in flight and refused with the shape; the
NumPy statement of the separable rule (tests/edt_ref.py) equals SciPy bit for bit on the masks the device tests use, equals the brute force
on tiny label volumes and equals per-label SciPy on the label inputs; ``prepost``'s own refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import edt_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bpx_edt_workspace", "bpx_edt")
A = 4096                                   # any non-null, aligned "device" address: nothing is launched
U8, I32 = 3, 6


def test_entry_points_are_declared_exported_and_bound():
    from biapy_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    source = open(os.path.join(ROOT, "biapy_amd", "csrc", "edt.hip")).read()
    assert set(re.findall(r'extern "C" \w+ (bpx_[a-z0-9_]+)\(', source)) == set(NAMES)          # the prefix bpx_edt_ / bpx_edt only
    for name in NAMES:
        assert re.search(r"^(int|int64_t) %s\(" % name, header, re.M), name
        assert name in L.EXPORTS and getattr(L.lib._raw, name) is not None, name
    assert re.search(r"BPX_I32 = 6", header) and L.I32 == I32 and L.U8 == U8
    make = open(os.path.join(ROOT, "biapy_amd", "csrc", "Makefile")).read()
    assert "edt.hip" in make and "edt_core.h" in make
    assert L.lib._raw.bpx_edt_workspace.restype is L.C.c_int64
    assert "edt" not in open(os.path.join(ROOT, "biapy_amd", "csrc", "label.hip")).read()


def test_both_forms_share_one_kernel_set():
    csrc = os.path.join(ROOT, "biapy_amd", "csrc")
    for name in ("edt.hip", "edt_index.hip"):                         # entry points only: the shared kernels, not a copy
        source = open(os.path.join(csrc, name)).read()
        assert '#include "edt_kernels.h"' in source and "__global__" not in source, name
    kernels = open(os.path.join(csrc, "edt_kernels.h")).read()
    assert re.findall(r"^template <[^>]*>\n?\s*__global__ void __launch_bounds__\(\d+\) (\w+)\(", kernels, re.M) == ["edt_row_kernel", "edt_column_kernel"]
    assert kernels.count("__global__") == 2
    core = open(os.path.join(csrc, "edt_core.h")).read()
    assert len(re.findall(r"\bEDT_HD void edt_column\(", core)) == 1 and "edt_column(" in kernels
    assert "edt_column_sites" not in core and "flush_site" not in core


def test_host_checks_answer_without_a_device():
    from biapy_amd import _lib as L

    lib = L.lib

    def err():
        return lib.bpx_last_error().decode()

    def samp(*v):
        return (ctypes.c_double * 3)(*v)

    def edt(key=A, dtype=U8, label_mode=0, Z=9, Y=21, X=37, sampling=None, squared=0, out=A, ws=A, ws_bytes=None):
        need = lib.bpx_edt_workspace(9, 21, 37, 0 if sampling is None else 1) if ws_bytes is None else ws_bytes
        return lib.bpx_edt(key, dtype, label_mode, Z, Y, X, sampling, squared, out, ws, need, None)

    for kw in (dict(key=None), dict(out=None), dict(ws=None)):
        assert edt(**kw) != 0 and "null pointer" in err(), kw
    for dt in (0, 1, 2, 4, 5, 7):
        assert edt(dtype=dt) != 0 and "BPX_U8 or BPX_I32" in err(), dt
    for kw in (dict(Z=0), dict(Y=0), dict(X=-1)):
        assert edt(**kw) != 0 and "extents must be at least 1" in err(), kw
    assert edt(Z=2048, Y=1024, X=1024, ws_bytes=1 << 50) != 0 and "2^31 voxels or more" in err()
    assert edt(Z=2048, Y=1024, X=1024, sampling=samp(1, 1, 1), ws_bytes=1 << 50) != 0 and "2^31 voxels or more" in err()
    assert edt(Z=1, Y=1, X=46341, ws_bytes=1 << 40) != 0 and "Z^2 + Y^2 + X^2" in err()
    assert edt(Z=1, Y=32768, X=32768, ws_bytes=1 << 50) != 0 and "Z^2 + Y^2 + X^2" in err()     # 2^30 voxels, a sum of 2^31 + 1
    assert edt(Z=1, Y=1, X=46340, ws_bytes=0) != 0 and "workspace too small" in err()            # 46340^2 + 2 < 2^31 - 1: admitted
    assert edt(Z=1, Y=1, X=46341, sampling=samp(1, 1, 1), ws_bytes=0) != 0 and "workspace too small" in err()   # the fp64 path has no such limit
    for bad in (samp(0, 1, 1), samp(1, -2, 1), samp(1, 1, float("inf")), samp(float("nan"), 1, 1)):
        assert edt(sampling=bad, ws_bytes=1 << 40) != 0 and "sampling must be positive and finite" in err(), list(bad)
    assert edt(ws_bytes=lib.bpx_edt_workspace(9, 21, 37, 0) - 1) != 0 and "workspace too small" in err()
    assert edt(sampling=samp(2, 1, 0.5), ws_bytes=lib.bpx_edt_workspace(9, 21, 37, 1) - 1) != 0 and "workspace too small" in err()
    assert edt(ws_bytes=0) != 0 and "workspace too small" in err()
    assert edt(out=A + 2) != 0 and "4-byte aligned" in err()
    assert edt(ws=A + 4) != 0 and "8-byte aligned" in err()
    assert edt(key=A + 2, dtype=I32, label_mode=1) != 0 and "4-byte aligned" in err()


def test_workspace_is_bounded_by_the_threads_in_flight():
    from biapy_amd import _lib as L

    ws = L.lib.bpx_edt_workspace

    def threads(cols):
        return min(131072, -(-(-(-cols // 4)) // 64) * 64)

    def entries(Z, Y, X):                                             # stacks of the Y pass (Z * X columns of Y), of the Z pass (Y * X columns of Z)
        return max(threads(Z * X) * Y, threads(Y * X) * Z)

    for Z, Y, X in ((1, 1, 1), (9, 21, 37), (20, 43, 150), (1, 33, 70), (5000, 2, 3), (1, 30000, 3), (256, 256, 256), (512, 512, 512), (1024, 1024, 1024)):
        assert ws(Z, Y, X, 0) == 8 * entries(Z, Y, X), (Z, Y, X)
        assert ws(Z, Y, X, 1) == 8 * Z * Y * X + 16 * entries(Z, Y, X), (Z, Y, X)
    assert ws(1, 1, 1, 0) == 8 * 64 and ws(1, 1, 40000, 0) == 8 * 10048 and ws(1, 30000, 3, 0) == 8 * 64 * 30000
    # the integer path never takes a second voxel-sized array: at most half the int32 output's bytes once a quarter of the columns fills whole
    # waves, and a fixed 131072 stacks beyond - a quarter of the output at 1024^3
    for s in (256, 512, 1024):
        assert ws(s, s, s, 0) <= 4 * s ** 3 // 2
    assert ws(1024, 1024, 1024, 0) == 2 ** 30 == 4 * 1024 ** 3 // 4
    assert ws(2048, 1024, 1024, 0) < 0 and ws(2048, 1024, 1024, 1) < 0 and ws(1300, 1300, 1300, 1) < 0       # 2^31 voxels and beyond
    assert ws(0, 4, 4, 0) < 0 and ws(4, -1, 4, 1) < 0
    assert ws(1, 1, 46341, 0) < 0 and ws(1, 1, 46340, 0) > 0 and ws(1, 1, 46341, 1) > 0                       # the sentinel limit: integer path only
    assert ws(1, 32768, 32768, 0) < 0 and ws(1, 32767, 32767, 0) > 0 and ws(1, 32768, 32768, 1) > 0          # 2^31 + 1 against 2^31 - 131069


@pytest.mark.parametrize("shape", E.SHAPES, ids=str)
def test_separable_rule_equals_scipy_on_the_random_masks(shape):
    for p, mask in E.random_masks(shape).items():
        assert mask.dtype == np.uint8 and not mask.all()
        sq = E.separable_sq(E.keys_of(mask, False))
        assert sq.dtype == np.int32
        np.testing.assert_array_equal(sq, E.scipy_sq(mask), err_msg=str(p))
        assert E.sqrt_f32(sq).view(np.int32).tolist() == E.scipy_f32(mask).view(np.int32).tolist()           # float32(sqrt(float64(sq))) IS SciPy's, rounded
    if np.prod(shape) > 1000:
        assert E.scipy_sq(E.random_masks(shape)[0.999]).max() > E.scipy_sq(E.random_masks(shape)[0.5]).max()  # sparse zeros: long distances


@pytest.mark.parametrize("name", [n for n in E.STRUCTURED if n != "zero"])
def test_separable_rule_equals_scipy_on_the_structured_masks(name):
    mask = E.structured(name)
    sq = E.separable_sq(E.keys_of(mask, False))
    np.testing.assert_array_equal(sq, E.scipy_sq(mask))
    assert np.array_equal(E.sqrt_f32(sq).view(np.int32), E.scipy_f32(mask).view(np.int32))


def test_all_zero_and_all_one():
    assert not E.separable_sq(E.keys_of(E.structured("zero"), False)).any()
    ones = np.ones((3, 4, 5), np.uint8)
    assert (E.separable_sq(ones) == E.INF).all() and (E.brute_sq(ones) == E.INF).all()
    assert np.isinf(E.sqrt_f32(E.separable_sq(ones))).all()
    from scipy import ndimage

    assert np.isfinite(ndimage.distance_transform_edt(ones)).all()                                           # SciPy: a fictitious point - not a reference


@pytest.mark.parametrize("name", list(E.LONG))
def test_long_axes_closed_form_is_scipys(name):
    mask, sq = E.long_axis(name)
    np.testing.assert_array_equal(sq, E.scipy_sq(mask))
    assert 0 < int(sq.max()) < E.INF
    if name == "x":
        assert int(sq.max()) == 39999 ** 2 and np.array_equal(E.separable_sq(E.keys_of(mask, False)), sq)


def test_separable_rule_equals_the_brute_force_on_tiny_label_volumes():
    rng = np.random.default_rng(2)
    for shape in ((3, 4, 5), (2, 7, 9), (1, 6, 11), (6, 11), (4, 1, 13), (5, 5, 5)):
        for hi in (2, 4, 9):
            lab = rng.integers(0, hi, size=shape)
            np.testing.assert_array_equal(E.separable_sq(lab), E.brute_sq(lab), err_msg=f"{shape} {hi}")
        blocks = np.kron(rng.integers(0, 3, size=tuple(-(-s // 2) for s in shape)), np.ones((2,) * len(shape), np.int64))[tuple(slice(0, s) for s in shape)]
        np.testing.assert_array_equal(E.separable_sq(blocks), E.brute_sq(blocks))
        lone = np.full(shape, 7)
        lone[tuple(s // 2 for s in shape)] = 3
        np.testing.assert_array_equal(E.separable_sq(lone), E.brute_sq(lone))
        np.testing.assert_array_equal(E.separable_sq(lone != 0), np.full(shape, E.INF))                       # as a mask: no background at all


@pytest.mark.parametrize("name", list(E.LABELS))
def test_separable_rule_equals_per_label_scipy(name):
    lab = E.labels(name)
    assert lab.dtype == np.int32 and len(np.unique(lab)) > 1
    np.testing.assert_array_equal(E.separable_sq(E.keys_of(lab, True)), E.label_ref_sq(lab))
    if name == "large_ids":
        assert lab.max() > 2 ** 30


def test_prepost_refusals():
    from biapy_amd import prepost as P

    with pytest.raises(RuntimeError, match="no CPU path"):
        P.distance_transform_edt(torch.zeros(4, 5, 6, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.distance_transform_edt(torch.zeros(5, 6, dtype=torch.bool), sampling=(1.0, 2.0), squared=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.label_distance(torch.zeros(4, 5, 6, dtype=torch.int32))
    for dt in (torch.float32, torch.int32, torch.int64, torch.float16):
        with pytest.raises(NotImplementedError, match="uint8 or bool"):
            P.distance_transform_edt(torch.zeros(4, 5, 6, dtype=dt))
    for dt in (torch.uint8, torch.bool, torch.int64, torch.float32):
        with pytest.raises(NotImplementedError, match="int32 labels"):
            P.label_distance(torch.zeros(4, 5, 6, dtype=dt))
    for shape in ((7,), (2, 3, 4, 5), ()):                            # rank and sampling are judged before the device is asked for
        with pytest.raises(ValueError, match="2-D .* or 3-D"):
            P.distance_transform_edt(torch.zeros(shape, dtype=torch.uint8))
        with pytest.raises(ValueError, match="2-D .* or 3-D"):
            P.label_distance(torch.zeros(shape, dtype=torch.int32), squared=True)
    m3, m2 = torch.zeros(4, 5, 6, dtype=torch.uint8), torch.zeros(5, 6, dtype=torch.int32)
    for bad in ((1.0, 2.0), (1.0, 2.0, 3.0, 4.0), (1.0, 0.0, 1.0), (1.0, -1.0, 1.0), (1.0, float("inf"), 1.0), (float("nan"), 1.0, 1.0), 2.0, "abc"):
        with pytest.raises(ValueError, match="sampling"):
            P.distance_transform_edt(m3, sampling=bad)
    for bad in ((1.0,), (1.0, 2.0, 3.0), (0.0, 1.0)):
        with pytest.raises(ValueError, match="sampling"):
            P.label_distance(m2, sampling=bad)
    with pytest.raises(RuntimeError, match="no CPU path"):           # a valid sampling: the next thing judged is the device
        P.label_distance(m2, sampling=(1, 2))

"""Local maxima - what can be checked without a GPU: ``bpx_peaks_workspace`` and ``bpx_peak_local_max`` are declared, exported and bound; every
host-side refusal names its cause before anything is launched; the ``prepost`` calls refuse bad arguments and CPU tensors in the stated order;
and the NumPy twin the GPU tests hold the device against (tests/peaks_ref.py) is scikit-image's mask on tie-free images, a strict subset of it
on ties, and gives the hand-made cases of the definition."""
import math
import os
import re

import numpy as np
import pytest
import torch

import peaks_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 4096                                   # any non-null, aligned "device" address: nothing is launched
I32, F32 = 6, 0


def test_entry_points_are_declared_exported_and_bound():
    from biapy_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    source = open(os.path.join(ROOT, "biapy_amd", "csrc", "peaks.hip")).read()
    assert set(re.findall(r'extern "C" \w+ (\w+)\(', source)) == {"bpx_peaks_workspace", "bpx_peak_local_max"}
    assert re.search(r"^int64_t bpx_peaks_workspace\(int Z, int Y, int X\);", header, re.M)
    assert re.search(r"^int bpx_peak_local_max\(const void\* img_d, int dtype, int Z, int Y, int X, int rz, int ry, int rx, double threshold, "
                     r"int bz, int by, int bx,\s+void\* mask_d, void\* keys_d, int max_peaks, int\* num_d, void\* ws_d, int64_t ws_bytes, "
                     r"bpx_stream_t stream\);", header, re.M)
    vp, i, i64, d = L.C.c_void_p, L.C.c_int, L.C.c_int64, L.C.c_double
    for name in ("bpx_peaks_workspace", "bpx_peak_local_max"):
        assert name in L.EXPORTS, name
    assert L._SIGS["bpx_peaks_workspace"] == ([i, i, i], i64) and L.lib._raw.bpx_peaks_workspace.restype is i64
    assert L._SIGS["bpx_peak_local_max"] == ([vp, i, i, i, i, i, i, i, d, i, i, i, vp, vp, i, vp, vp, i64, vp], i)
    assert (L.I32, L.F32) == (I32, F32)
    make = open(os.path.join(ROOT, "biapy_amd", "csrc", "Makefile")).read()
    assert "peaks.hip" in make and re.search(r"^peaks\.o:.*peaks_core\.h", make, re.M)
    core = open(os.path.join(ROOT, "biapy_amd", "csrc", "peaks_core.h")).read()
    assert '#include "peaks_core.h"' in source and "peaks_lane<" in source and "peaks_plan(" in source       # the shared steps, not a copy
    assert not re.search(r"\bPEAKS_HD \w+ peaks_\w+\(", source)
    for fn in ("peaks_okey", "peaks_key", "peaks_decode", "peaks_plan", "peaks_load_bits", "peaks_load_keys", "peaks_store_keys", "peaks_window_max",
               "peaks_column_max", "peaks_test", "peaks_lane"):
        assert re.search(r"PEAKS_HD \w+ %s\(" % fn, core), fn
    check = open(os.path.join(ROOT, "scripts", "peaks_cpu_check.cpp")).read()
    assert '#include "peaks_core.h"' in check and "int main()" in check and "-fsanitize=address,undefined" in check
    assert "peaks_lane<" in check and "peaks_plan(" in check and "peaks_decode(" in check
    from biapy_amd import prepost
    assert callable(prepost.peak_local_max) and callable(prepost.peak_mask)
    assert prepost._PEAKS_MAX_RADIUS == int(re.search(r"PEAKS_MAX_RADIUS = (\d+);", core).group(1)) == 64


def test_workspace_is_two_key_volumes_at_most():
    from biapy_amd import _lib as L

    lib = L.lib
    assert lib.bpx_peaks_workspace(1, 1, 1) == 16 and lib.bpx_peaks_workspace(9, 21, 37) == 16 * 9 * 21 * 37
    assert lib.bpx_peaks_workspace(1024, 1024, 1024) == 16 * 2 ** 30
    for shape in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (2048, 1024, 1024), (1, 65536, 32768)):
        assert lib.bpx_peaks_workspace(*shape) == -1, shape
    assert lib.bpx_peaks_workspace(1, 1, 2 ** 31 - 1) == 16 * (2 ** 31 - 1)


def test_host_checks_answer_without_a_device():
    from biapy_amd import _lib as L

    lib = L.lib

    def err():
        return lib.bpx_last_error().decode()

    def peaks(img_d=A, dtype=F32, Z=4, Y=5, X=6, rz=1, ry=1, rx=1, threshold=0.5, bz=0, by=0, bx=0, mask_d=2 * A, keys_d=3 * A, max_peaks=7,
              num_d=4 * A, ws_d=5 * A, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = max(int(lib.bpx_peaks_workspace(Z, Y, X)), 0)
        return lib.bpx_peak_local_max(img_d, dtype, Z, Y, X, rz, ry, rx, threshold, bz, by, bx, mask_d, keys_d, max_peaks, num_d, ws_d, ws_bytes, None)

    for kw in (dict(img_d=None), dict(num_d=None), dict(ws_d=None)):
        assert peaks(**kw) != 0 and "null pointer" in err(), kw
    assert peaks(mask_d=None, keys_d=None) != 0 and "mask_d and keys_d are both null" in err()
    for kw in (dict(Z=0), dict(Y=0), dict(X=0), dict(Z=-1), dict(X=-7)):
        assert peaks(**kw) != 0 and "extents must be at least 1" in err(), kw
    for shape in ((2048, 1024, 1024), (1, 65536, 32768), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert peaks(Z=shape[0], Y=shape[1], X=shape[2]) != 0 and "2^31 voxels or more" in err(), shape
    for dtype in (1, 2, 3, 4, 5, 7, -1):                                                    # uint8 (3) among them
        assert peaks(dtype=dtype) != 0 and "dtype must be float32 or int32" in err(), dtype
    for kw in (dict(rz=-1), dict(ry=65), dict(rx=-3), dict(rx=65), dict(rz=1000)):
        assert peaks(**kw) != 0 and "radii must be in 0..64" in err(), kw
    for kw in (dict(bz=-1), dict(by=-1), dict(bx=-2 ** 31)):
        assert peaks(**kw) != 0 and "border margin must not be negative" in err(), kw
    assert peaks(threshold=float("nan")) != 0 and "threshold is NaN" in err()
    for mp in (0, -1):
        assert peaks(max_peaks=mp) != 0 and "max_peaks must be at least 1" in err(), mp
    for wb in (0, 16 * 120 - 1, -5):
        assert peaks(ws_bytes=wb) != 0 and "workspace too small" in err(), wb
    for kw in (dict(img_d=A + 2), dict(img_d=A + 1), dict(dtype=I32, img_d=A + 3)):
        assert peaks(**kw) != 0 and "image must be 4-byte aligned" in err(), kw
    for kw in (dict(ws_d=5 * A + 4), dict(keys_d=3 * A + 4)):
        assert peaks(**kw) != 0 and "8-byte aligned" in err(), kw
    assert peaks(mask_d=A) != 0 and "mask_d must not be img_d" in err()
    # the order: each call fails every later check too and names the earlier one
    assert peaks(img_d=None, mask_d=None, keys_d=None, Z=0) != 0 and "null pointer" in err()
    assert peaks(mask_d=None, keys_d=None, Z=0) != 0 and "both null" in err()
    assert peaks(Z=0, dtype=3, rz=-1) != 0 and "extents" in err()
    assert peaks(dtype=3, rz=-1, bz=-1) != 0 and "dtype" in err()
    assert peaks(rz=-1, bz=-1, threshold=float("nan")) != 0 and "radii" in err()
    assert peaks(bz=-1, threshold=float("nan"), max_peaks=0) != 0 and "border margin" in err()
    assert peaks(threshold=float("nan"), max_peaks=0, ws_bytes=0) != 0 and "threshold is NaN" in err()
    assert peaks(max_peaks=0, ws_bytes=0, img_d=A + 2) != 0 and "max_peaks" in err()
    assert peaks(ws_bytes=0, img_d=A + 2, mask_d=A + 2) != 0 and "workspace too small" in err()
    assert peaks(img_d=A + 2, mask_d=A + 2) != 0 and "4-byte aligned" in err()
    # what is allowed: max_peaks is not looked at without a key array - the largest volume passes every check but the last one made here
    assert peaks(Z=1, Y=1, X=2 ** 31 - 1, keys_d=None, max_peaks=0, rx=64, threshold=-math.inf, bx=2 ** 31 - 1, mask_d=A) != 0 and "mask_d must not be" in err()


def test_prepost_refuses_in_the_stated_order():
    from biapy_amd import prepost as P

    x = torch.rand(4, 5, 6)
    for fn in (P.peak_local_max, P.peak_mask):
        for t in (x, x[0], x.to(torch.int32)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                fn(t, 1, 0.5)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(x, (1, 2, 3), 0.5, (0, 1, 2))
        for bad in (x.view(-1), x[None], x[0, 0, 0]):
            with pytest.raises(ValueError, match="2-D .* or 3-D"):
                fn(bad, 1, 0.5)
        for md, t in (((1, 2), x), ((1, 2, 3), x[0]), ((1,), x), ([1, 2, 3, 4], x)):
            with pytest.raises(ValueError, match="min_distance must be an int or one int per axis"):
                fn(t, md, 0.5)
        for md in (-1, 65, (1, 1, 65), (0, -2, 0)):
            with pytest.raises(ValueError, match=r"min_distance must be in 0\.\.64"):
                fn(x, md, 0.5)
        for eb in ((1, 2), (0,)):
            with pytest.raises(ValueError, match="exclude_border must be an int or one int per axis"):
                fn(x, 1, 0.5, eb)
        for eb in (-1, (0, 0, -1)):
            with pytest.raises(ValueError, match="exclude_border must not be negative"):
                fn(x, 1, 0.5, eb)
        with pytest.raises(ValueError, match="threshold_abs must not be NaN"):
            fn(x, 1, float("nan"))
        for dt in (torch.uint8, torch.int64, torch.float16, torch.float64, torch.bool):
            with pytest.raises(NotImplementedError, match="works on float32 or int32"):
                fn(x.to(dt), 1, 0.5)
        with pytest.raises(NotImplementedError, match="empty axis"):
            fn(torch.zeros(4, 0, 6), 1, 0.5)
        # the order: ValueError before NotImplementedError before RuntimeError
        with pytest.raises(ValueError, match="2-D .* or 3-D"):
            fn(x[None].to(torch.float64), 1, 0.5)
        with pytest.raises(ValueError, match="min_distance"):
            fn(x.to(torch.float64), 65, 0.5)
        with pytest.raises(NotImplementedError, match="works on"):
            fn(x.to(torch.float64), 1, 0.5)
        for name in ("threshold_rel", "labels", "footprint", "p_norm"):                     # not offered
            with pytest.raises(TypeError):
                fn(x, 1, 0.5, **{name: None})
    for kw in (dict(max_peaks=0), dict(max_peaks=-3), dict(num_peaks=0), dict(num_peaks=-1)):
        with pytest.raises(ValueError, match="must be at least 1"):
            P.peak_local_max(x, 1, 0.5, **kw)
        with pytest.raises(ValueError, match="must be at least 1"):
            P.peak_local_max(x.to(torch.float64), 1, 0.5, **kw)
    doc = P.peak_local_max.__doc__
    for phrase in ("each other's box", "SUBSET", "raster-first", "READS ONE SCALAR BACK","ensure_spacing"):
        assert phrase in doc, phrase


# ---- the twin against scikit-image's mask --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", R.RADII, ids=str)
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_twin_equals_scipy_on_tie_free_images(shape, r):
    img = R.tie_free(shape)
    radii = R.per_axis(r, img.ndim)
    total = 0
    for border in (0, radii):
        got = R.peak_mask_ref(img, radii, 0.5, border)
        np.testing.assert_array_equal(got, R.scipy_mask(img, radii, 0.5, border))
        assert got.dtype == np.uint8 and R.no_two_in_a_box(got, radii)
        total += int(got.sum())
    free = R.peak_mask_ref(img, radii, -np.inf, 0)
    assert free.sum() >= 1 and free.reshape(-1)[np.argmax(img)] == 1                         # the global maximum is always a peak
    if shape in ((9, 21, 37), (3, 70, 130), (37, 41)):
        assert total > 0, "a comparison of two empty masks shows nothing"


@pytest.mark.parametrize("shape", ((9, 21, 37), (37, 41)), ids=str)
def test_twin_is_a_strict_subset_on_ties(shape):
    img = R.quantised(shape)
    assert np.unique(img).size <= 40
    for r in (1, 2):
        got, sk = R.peak_mask_ref(img, r, 0.5, 0), R.scipy_mask(img, r, 0.5, 0)
        assert ((got == 1) <= (sk == 1)).all() and 0 < got.sum() < sk.sum(), (r, got.sum(), sk.sum())
        assert R.no_two_in_a_box(got, r) and not R.no_two_in_a_box(sk, r)


def test_hand_made_cases():
    row = R.plateau_row()
    coords, values = R.peak_list_ref(row, (0, 2), 0.5, 0)
    assert coords.tolist() == [[0, 3]] and values.tolist() == [1.0]
    assert R.scipy_mask(row, (0, 2), 0.5, 0).sum() == 12
    # a constant volume: the raster-first voxel, or none under the threshold or inside the margin
    const = np.full((4, 5, 6), 2.0, np.float32)
    assert R.peak_list_ref(const, 8, 1.0, 0)[0].tolist() == [[0, 0, 0]]
    assert R.peak_list_ref(const, 8, 2.0, 0)[0].shape == (0, 3) and R.peak_list_ref(const, 8, None, 0)[0].shape == (0, 3)
    assert R.peak_mask_ref(const, 8, 1.0, 1).sum() == 0                                      # the only candidate lies on the border
    # -0.0 < +0.0; a plateau yields its raster-first voxel only (x = 5 beats x = 6 in the box of 6 without being a peak itself); the order of
    # the list is value descending, then index ascending
    z = np.zeros((1, 9), np.float32)
    z[0, :4] = -0.0
    assert R.peak_list_ref(z, (0, 1), -1.0, 0)[0].tolist() == [[0, 4], [0, 0]]
    assert R.peak_list_ref(z, (0, 0), -1.0, 0)[0].tolist() == [[0, 4], [0, 5], [0, 6], [0, 7], [0, 8], [0, 0], [0, 1], [0, 2], [0, 3]]
    # exclude_border beyond half an extent: no voxel on that axis
    img = R.tie_free((5, 6, 7))
    assert R.peak_mask_ref(img, 1, -np.inf, (0, 3, 0)).sum() == 0 and R.peak_mask_ref(img, 1, -np.inf, (2, 2, 3)).sum() <= 2
    # int32 at both ends of its range
    i = np.array([[np.iinfo(np.int32).min, np.iinfo(np.int32).min, np.iinfo(np.int32).max, 5, np.iinfo(np.int32).min]], np.int32)
    assert R.peak_list_ref(i, (0, 1), -np.inf, 0)[0].tolist() == [[0, 2], [0, 0]]
    assert R.peak_list_ref(i, (0, 1), None, 0)[0].tolist() == [[0, 2]]                       # image.min() itself is no peak

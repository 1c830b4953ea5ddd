"""Nearest-source indices of the distance transform - what can be checked without a GPU: the entry points are declared, exported and bound;
every host-side refusal names its cause before anything is launched; the workspace formula of the index-in-the-stack design is pinned and
refused with the shape; the NumPy statement of the separable passes (tests/edt_index_ref.py) equals the brute-force rule on tiny volumes and
names, on the masks the device tests use, a source at exactly SciPy's distance; the ``expand_labels`` / ``voronoi_on_mask`` twins against
per-label SciPy; ``prepost``'s own refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import edt_index_ref as R
import edt_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bpx_edt_index_workspace", "bpx_edt_index")
A = 4096                                   # any non-null, aligned "device" address: nothing is launched
U8, I32 = 3, 6


def test_entry_points_are_declared_exported_and_bound():
    from biapy_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    source = open(os.path.join(ROOT, "biapy_amd", "csrc", "edt_index.hip")).read()
    assert set(re.findall(r'extern "C" \w+ (bpx_[a-z0-9_]+)\(', source)) == set(NAMES)
    for name in NAMES:
        assert re.search(r"^(int|int64_t) %s\(" % name, header, re.M), name
        assert name in L.EXPORTS and getattr(L.lib._raw, name) is not None, name
    make = open(os.path.join(ROOT, "biapy_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bedt_index\.hip\b", make, re.M) and re.search(r"^edt_index\.o: .*edt_core\.h", make, re.M)
    assert L.lib._raw.bpx_edt_index_workspace.restype is L.C.c_int64
    assert "address_space(3)" in open(os.path.join(ROOT, "biapy_amd", "csrc", "edt_kernels.h")).read()     # the LDS part of the stack stays typed as LDS


def test_host_checks_answer_without_a_device():
    from biapy_amd import _lib as L

    lib = L.lib

    def err():
        return lib.bpx_last_error().decode()

    def samp(*v):
        return (ctypes.c_double * 3)(*v)

    def edt(key=A, dtype=U8, invert=0, Z=9, Y=21, X=37, sampling=None, squared=0, dist=A, index=A, ws=A, ws_bytes=None):
        need = lib.bpx_edt_index_workspace(9, 21, 37, 0 if sampling is None else 1) if ws_bytes is None else ws_bytes
        return lib.bpx_edt_index(key, dtype, invert, Z, Y, X, sampling, squared, dist, index, ws, need, None)

    for kw in (dict(key=None), dict(index=None), dict(ws=None)):
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
    need_i, need_f = lib.bpx_edt_index_workspace(9, 21, 37, 0), lib.bpx_edt_index_workspace(9, 21, 37, 1)
    assert edt(ws_bytes=need_i - 1) != 0 and "workspace too small" in err()
    assert edt(sampling=samp(2, 1, 0.5), ws_bytes=need_f - 1) != 0 and "workspace too small" in err()
    assert edt(sampling=samp(2, 1, 0.5), dist=None, ws_bytes=need_f - 1) != 0 and "workspace too small" in err()
    # without dist_d the integer path keeps its values in the workspace: 4 more bytes per voxel, and the message says so
    assert edt(dist=None, ws_bytes=need_i + 4 * 9 * 21 * 37 - 1) != 0 and "workspace too small" in err() and "4 bytes per voxel" in err()
    assert edt(ws_bytes=0) != 0 and "workspace too small" in err()
    assert edt(dist=A + 2) != 0 and "4-byte aligned" in err()
    assert edt(index=A + 2) != 0 and "4-byte aligned" in err()
    assert edt(ws=A + 4) != 0 and "8-byte aligned" in err()
    assert edt(key=A + 2, dtype=I32, invert=1) != 0 and "4-byte aligned" in err()


def test_workspace_is_that_of_the_index_in_the_stack_entry():
    """12 (fp64: 20) bytes per stack entry - position | first winning position, height, index - for the threads in flight of a column pass, at
    most 98304 (6 waves per CU at 24 KiB of LDS per wave); no second index volume."""
    from biapy_amd import _lib as L

    ws = L.lib.bpx_edt_index_workspace

    def threads(cols):
        return min(98304, -(-(-(-cols // 4)) // 64) * 64)

    def entries(Z, Y, X):                                             # stacks of the Y pass (Z * X columns of Y), of the Z pass (Y * X columns of Z)
        return max(threads(Z * X) * Y, threads(Y * X) * Z)

    for Z, Y, X in ((1, 1, 1), (9, 21, 37), (20, 43, 150), (1, 33, 70), (5000, 2, 3), (1, 30000, 3), (256, 256, 256), (512, 512, 512), (1024, 1024, 1024)):
        assert ws(Z, Y, X, 0) == 12 * entries(Z, Y, X), (Z, Y, X)
        assert ws(Z, Y, X, 1) == 8 * Z * Y * X + 20 * entries(Z, Y, X), (Z, Y, X)
    assert ws(1, 1, 1, 0) == 12 * 64 and ws(1, 1, 40000, 0) == 12 * 10048 and ws(1, 30000, 3, 0) == 12 * 64 * 30000
    assert ws(1024, 1024, 1024, 0) == 12 * 98304 * 1024 == 9 * 2 ** 27                           # 1.125 GiB beside 8 GiB of distances and indices
    for s in (256, 512, 1024):
        assert ws(s, s, s, 0) <= 3 * 4 * s ** 3 // 4                                             # at most 3 bytes per voxel, where a ping-pong index volume alone takes 4
    assert ws(2048, 1024, 1024, 0) < 0 and ws(2048, 1024, 1024, 1) < 0 and ws(1300, 1300, 1300, 1) < 0       # 2^31 voxels and beyond
    assert ws(0, 4, 4, 0) < 0 and ws(4, -1, 4, 1) < 0
    assert ws(1, 1, 46341, 0) < 0 and ws(1, 1, 46340, 0) > 0 and ws(1, 1, 46341, 1) > 0                       # the sentinel limit: integer path only
    assert ws(1, 32768, 32768, 0) < 0 and ws(1, 32767, 32767, 0) > 0 and ws(1, 32768, 32768, 1) > 0


def test_separable_passes_equal_the_brute_force_rule_on_tiny_volumes():
    rng = np.random.default_rng(5)
    for shape in ((3, 4, 5), (2, 7, 9), (6, 11), (5, 5, 5), (4, 1, 13), (7, 8, 9)):
        for p in (0.5, 0.9, 0.97):
            key = (rng.random(shape) < p).astype(np.uint8)
            for invert in (False, True):
                np.testing.assert_array_equal(R.separable_index(key, invert), R.brute_index(key, invert), err_msg=f"{shape} {p} {invert}")
        lone = np.ones(shape, np.uint8)
        at = tuple(int(rng.integers(0, s)) for s in shape)
        lone[at] = 0
        want = int(np.ravel_multi_index(at, shape))
        assert (R.separable_index(lone) == want).all() and (R.brute_index(lone) == want).all()               # a single source: its index everywhere
        assert (R.separable_index(lone, True)[lone != 0] == np.flatnonzero(lone)).all()                       # inverted: every source names itself
        none = np.ones(shape, np.uint8)
        assert (R.separable_index(none) == -1).all() and (R.brute_index(none) == -1).all()                   # no source
        sq, _ = R.separable(none)
        assert (sq == R.INF).all()
        assert np.array_equal(R.separable_index(np.zeros(shape, np.uint8)), np.arange(np.prod(shape)).reshape(shape))


def test_the_rule_is_not_scipys_tie_choice():
    """SciPy's return_indices names another of several nearest zeros on the checkerboard: the distance is the reference, not the voxel."""
    from scipy import ndimage

    mask = np.ascontiguousarray(E.structured("checkerboard")[:6, :7, :9])
    ind = ndimage.distance_transform_edt(mask, return_distances=False, return_indices=True)
    idx = R.separable_index(mask)
    assert (np.ravel_multi_index(tuple(ind), mask.shape) != idx).any()
    np.testing.assert_array_equal(R.sq_of(idx, mask.shape), ((ind - np.indices(mask.shape)) ** 2).sum(axis=0))
    np.testing.assert_array_equal(idx, R.brute_index(mask))


def _check_twin(mask):
    sq, idx = R.twin(mask)
    assert idx.dtype == np.int32 and idx.shape == mask.shape and idx.min() >= 0
    assert not mask.reshape(-1)[idx].any()                                                                   # points at a source
    np.testing.assert_array_equal(R.sq_of(idx, mask.shape), E.scipy_sq(mask))                                # ... at exactly SciPy's distance
    np.testing.assert_array_equal(sq, E.scipy_sq(mask))
    assert (idx[mask == 0] == np.flatnonzero(mask.reshape(-1) == 0)).all()                                   # a source's index is its own


@pytest.mark.parametrize("shape", E.SHAPES, ids=str)
def test_twin_names_a_source_at_scipys_distance_on_the_random_masks(shape):
    for mask in E.random_masks(shape).values():
        _check_twin(mask)


@pytest.mark.parametrize("name", [n for n in E.STRUCTURED if n != "zero"])
def test_twin_names_a_source_at_scipys_distance_on_the_structured_masks(name):
    _check_twin(E.structured(name))


@pytest.mark.parametrize("name", list(E.LONG))
def test_twin_equals_the_closed_form_on_the_long_axes(name):
    """A single zero: its index everywhere, over 40000, 30000 and 5000 positions."""
    mask, sq = E.long_axis(name)
    got_sq, idx = R.twin(mask)
    assert (idx == long_index(name)).all()
    np.testing.assert_array_equal(got_sq, sq)


def long_index(name):
    shape, at = E.LONG[name]
    return int(np.ravel_multi_index(at, shape))


@pytest.mark.parametrize("distance", [0, 1, 2.5, 1000, 1e200])
def test_expand_twin_against_per_label_scipy(distance):
    from scipy import ndimage

    lab = E.labels("blocks")
    out = R.expand_ref(lab, distance)
    to_any = ndimage.distance_transform_edt(lab == 0)
    assert np.array_equal(out[lab != 0], lab[lab != 0])                                                      # labelled voxels keep theirs
    np.testing.assert_array_equal(out != 0, to_any ** 2 <= np.floor(min(float(distance), 1e6) ** 2) + 0.5)             # integers: the squares are exact
    for l in np.unique(out[out != 0]):
        to_l = ndimage.distance_transform_edt(lab != l)
        np.testing.assert_array_equal(to_l[out == l], to_any[out == l])                                      # the label given is a nearest one
    if distance == 0:
        assert np.array_equal(out, lab)
    if distance >= 1000:
        assert (out != 0).all()                                                                              # 1e200: its square is no float, the test is still an integer one


def test_voronoi_twin_against_per_label_scipy():
    from scipy import ndimage

    lab = E.labels("blocks")
    mask = E.random_masks(lab.shape)[0.5]
    out = R.voronoi_ref(lab, mask)
    assert not out[mask == 0].any() and (out[mask != 0] != 0).all()
    assert np.array_equal(out[(mask != 0) & (lab != 0)], lab[(mask != 0) & (lab != 0)])
    to_any = ndimage.distance_transform_edt(lab == 0)
    for l in np.unique(out[out != 0]):
        np.testing.assert_array_equal(ndimage.distance_transform_edt(lab != l)[out == l], to_any[out == l])
    assert not R.voronoi_ref(np.zeros_like(lab), mask).any()                                                 # no label at all
    assert not R.expand_ref(np.zeros_like(lab), 3).any()


def test_prepost_refusals():
    from biapy_amd import prepost as P

    m3, l3 = torch.zeros(4, 5, 6, dtype=torch.uint8), torch.zeros(4, 5, 6, dtype=torch.int32)
    with pytest.raises(ValueError, match="return_distances"):
        P.distance_transform_edt(m3, return_distances=False)
    for bad in ("coords", 2, None, "LINEAR"):
        with pytest.raises(ValueError, match="return_indices"):
            P.distance_transform_edt(m3, return_indices=bad)
    for kw in (dict(return_indices=True), dict(return_indices="linear"), dict(return_indices="linear", return_distances=False)):
        with pytest.raises(NotImplementedError, match="uint8 or bool"):
            P.distance_transform_edt(l3, **kw)
        with pytest.raises(ValueError, match="2-D .* or 3-D"):
            P.distance_transform_edt(torch.zeros(7, dtype=torch.uint8), **kw)
        with pytest.raises(ValueError, match="sampling"):
            P.distance_transform_edt(m3, sampling=(1.0, 2.0), **kw)
    for dt in (torch.uint8, torch.bool, torch.int64, torch.float32):
        with pytest.raises(NotImplementedError, match="int32 labels"):
            P.expand_labels(torch.zeros(4, 5, 6, dtype=dt))
        with pytest.raises(NotImplementedError, match="int32 labels"):
            P.voronoi_on_mask(torch.zeros(4, 5, 6, dtype=dt), m3)
    for bad in (-1, -0.001, float("nan"), float("inf"), "far"):
        with pytest.raises(ValueError, match="distance"):
            P.expand_labels(l3, bad)
    with pytest.raises(ValueError, match="2-D .* or 3-D"):
        P.expand_labels(torch.zeros(2, 3, 4, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match="sampling"):
        P.expand_labels(l3, 2, sampling=(1.0, 0.0, 1.0))
    for dt in (torch.int32, torch.float32):
        with pytest.raises(NotImplementedError, match="uint8 or bool"):
            P.voronoi_on_mask(l3, torch.zeros(4, 5, 6, dtype=dt))
    with pytest.raises(ValueError, match="differ in shape"):
        P.voronoi_on_mask(l3, torch.zeros(4, 5, 7, dtype=torch.uint8))
    # every argument valid: the last thing judged is the device
    for call in (lambda: P.distance_transform_edt(m3, return_indices=True), lambda: P.distance_transform_edt(m3, return_indices="linear", return_distances=False),
                 lambda: P.distance_transform_edt(torch.zeros(5, 6, dtype=torch.bool), sampling=(1.0, 2.0), return_indices="linear"),
                 lambda: P.expand_labels(l3), lambda: P.expand_labels(l3, 2.5, sampling=(2, 1, 1)), lambda: P.voronoi_on_mask(l3, m3),
                 lambda: P.voronoi_on_mask(l3, m3.bool())):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()

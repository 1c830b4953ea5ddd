"""Morphology - what can be checked without a GPU: ``bpx_morph`` is declared, exported and bound; every host-side refusal names its cause before
anything is launched; the ``prepost`` calls refuse on CPU tensors; and the NumPy statement the GPU tests hold the device against
(tests/morph_ref.py) agrees with SciPy bit for bit on every input those tests use, and with hand-made cases."""
import os
import re

import numpy as np
import pytest
import torch

import morph_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 4096                                   # any non-null, aligned "device" address: nothing is launched
U8, I32, F32 = 3, 6, 0


def _structure(ndim, c):
    from scipy import ndimage

    return ndimage.generate_binary_structure(ndim, c)


def test_entry_point_is_declared_exported_and_bound():
    from biapy_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    source = open(os.path.join(ROOT, "biapy_amd", "csrc", "morph.hip")).read()
    assert set(re.findall(r'extern "C" \w+ (\w+)\(', source)) == {"bpx_morph"}
    assert re.search(r"^int bpx_morph\(const void\* in_d, int dtype, int Z, int Y, int X, int ndim, int connectivity, int op, int flags, "
                     r"int background, void\* out_d,\s+bpx_stream_t stream\);", header, re.M)
    assert "bpx_morph" in L.EXPORTS and L.lib._raw.bpx_morph.restype is L.C.c_int
    vp, i = L.C.c_void_p, L.C.c_int
    assert L._SIGS["bpx_morph"][0] == [vp, i, i, i, i, i, i, i, i, i, vp, vp]
    assert (L.U8, L.I32, L.F32) == (U8, I32, F32)
    make = open(os.path.join(ROOT, "biapy_amd", "csrc", "Makefile")).read()
    assert "morph.hip" in make and re.search(r"^morph\.o:.*morph_core\.h", make, re.M)
    core = open(os.path.join(ROOT, "biapy_amd", "csrc", "morph_core.h")).read()
    assert '#include "morph_core.h"' in source and "morph_lane<" in source                  # the shared steps, not a copy
    assert not re.search(r"\bMORPH_HD \w+ morph_\w+\(", source)
    for fn in ("morph_row_in", "morph_row_wide", "morph_fill", "morph_norm01", "morph_left", "morph_right", "morph_pick", "morph_load", "morph_store",
               "morph_lane"):
        assert re.search(r"MORPH_HD \w+ %s\(" % fn, core), fn
    check = open(os.path.join(ROOT, "scripts", "morph_cpu_check.cpp")).read()
    assert '#include "morph_core.h"' in check and "int main()" in check and "-fsanitize=address,undefined" in check and "morph_lane<" in check
    from biapy_amd import prepost
    for name in ("binary_erosion", "binary_dilation", "binary_opening", "binary_closing", "erosion", "dilation", "find_boundaries",
                 "binary_fill_holes", "clear_border"):
        assert callable(getattr(prepost, name)), name


def test_host_checks_answer_without_a_device():
    from biapy_amd import _lib as L

    lib = L.lib

    def err():
        return lib.bpx_last_error().decode()

    def morph(in_d=A, dtype=U8, Z=4, Y=5, X=6, ndim=3, connectivity=1, op=0, flags=0, background=0, out_d=2 * A):
        return lib.bpx_morph(in_d, dtype, Z, Y, X, ndim, connectivity, op, flags, background, out_d, None)

    for kw in (dict(in_d=None), dict(out_d=None)):
        assert morph(**kw) != 0 and "null pointer" in err(), kw
    for kw in (dict(Z=0), dict(Y=0), dict(X=0), dict(Z=-1), dict(X=-7)):
        assert morph(**kw) != 0 and "extents must be at least 1" in err(), kw
    for shape in ((2048, 1024, 1024), (1, 65536, 32768), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert morph(Z=shape[0], Y=shape[1], X=shape[2]) != 0 and "2^31 voxels or more" in err(), shape
    for kw in (dict(ndim=1), dict(ndim=4), dict(ndim=2), dict(ndim=0)):                     # ndim 2 with Z = 4
        assert morph(**kw) != 0 and "ndim must be 3, or 2 with Z = 1" in err(), kw
    for kw in (dict(connectivity=0), dict(connectivity=4), dict(connectivity=-1), dict(connectivity=3, ndim=2, Z=1)):
        assert morph(**kw) != 0 and "connectivity must be in 1.." in err(), kw
    for dtype in (1, 2, 4, 5, 7, -1):
        assert morph(dtype=dtype) != 0 and "dtype must be uint8, int32 or float32" in err(), dtype
    for op in (-1, 3, 99):
        assert morph(op=op) != 0 and "unknown op" in err(), op
    for flags in (8, 16, -1):
        assert morph(flags=flags) != 0 and "unknown flags" in err(), flags
    for kw in (dict(flags=1, dtype=I32), dict(flags=1, dtype=F32), dict(flags=1, op=2), dict(flags=3, dtype=I32)):
        assert morph(**kw) != 0 and "binary flag takes a uint8 input and erode or dilate" in err(), kw
    for kw in (dict(flags=2), dict(flags=2, dtype=I32), dict(flags=2, op=2)):
        assert morph(**kw) != 0 and "absorbing border is offered on the binary path only" in err(), kw
    for kw in (dict(flags=4), dict(flags=4, op=1), dict(flags=5)):
        assert morph(**kw) != 0 and "inner flag belongs to the boundary op" in err(), kw
    assert morph(out_d=A) != 0 and "out_d must not be in_d" in err()
    for kw in (dict(dtype=I32, in_d=A + 2), dict(dtype=F32, in_d=A + 1), dict(dtype=I32, out_d=A + 6), dict(dtype=F32, op=1, out_d=A + 3),
               dict(dtype=I32, op=2, in_d=A + 2)):
        assert morph(**kw) != 0 and "4-byte aligned" in err(), kw
    # the largest volume admitted passes every check but the last one made here
    assert morph(Z=1, Y=1, X=2 ** 31 - 1, dtype=I32, in_d=A + 2) != 0 and "4-byte aligned" in err()


def test_prepost_refuses_before_any_launch():
    from biapy_amd import prepost as P

    m = torch.ones(4, 5, 6, dtype=torch.uint8)
    lab = torch.ones(4, 5, 6, dtype=torch.int32)
    binary = (P.binary_erosion, P.binary_dilation, P.binary_opening, P.binary_closing, P.binary_fill_holes)
    for fn in binary + (P.erosion, P.dilation, P.find_boundaries):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(m)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(m[0])
        for bad in (m.view(-1), m[None], m[0, 0, 0]):
            with pytest.raises(ValueError, match="2-D .* or 3-D"):
                fn(bad)
        for dt in (torch.int64, torch.int16, torch.float16, torch.float64):
            with pytest.raises(NotImplementedError, match="works on"):
                fn(m.to(dt))
    for fn in binary:
        for dt in (torch.int32, torch.float32):
            with pytest.raises(NotImplementedError, match="uint8 or bool"):
                fn(m.to(dt))
    for fn in (P.erosion, P.dilation):
        with pytest.raises(NotImplementedError, match="uint8, int32 or float32"):
            fn(m.bool())
    for fn in binary[:4] + (P.erosion, P.dilation, P.find_boundaries):
        for c, t in ((0, m), (4, m), (-1, m), (3, m[0])):
            with pytest.raises(ValueError, match="connectivity must be in 1.."):
                fn(t, c)
    for fn in binary[:4]:
        for k in (0, -1):
            with pytest.raises(NotImplementedError, match="iterations must be >= 1"):
                fn(m, 1, k)
        for bv in (2, -1, 0.5):
            with pytest.raises(ValueError, match="border_value must be 0 or 1"):
                fn(m, 1, 1, bv)
    with pytest.raises(NotImplementedError, match="border_value=1 only"):
        P.binary_erosion(m, radius=2)                                                          # the default border_value=0
    with pytest.raises(NotImplementedError, match="border_value=0 only"):
        P.binary_dilation(m, border_value=1, radius=2)
    for fn, bv in ((P.binary_erosion, 1), (P.binary_dilation, 0)):
        for kw in (dict(connectivity=2), dict(iterations=2)):
            with pytest.raises(ValueError, match="INSTEAD of connectivity / iterations"):
                fn(m, border_value=bv, radius=2, **kw)
        for r in (-1, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="radius must be a finite number >= 0"):
                fn(m, border_value=bv, radius=r)
    for mode in ("outer", "subpixel"):
        with pytest.raises(NotImplementedError, match="offers the modes 'thick' and 'inner'"):
            P.find_boundaries(lab, mode=mode)
    with pytest.raises(ValueError, match="mode must be"):
        P.find_boundaries(lab, mode="thin")
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.clear_border(lab, 3)
    with pytest.raises(NotImplementedError, match="int32 labels"):
        P.clear_border(m, 3)
    with pytest.raises(ValueError, match="2-D .* or 3-D"):
        P.clear_border(lab[None], 3)
    for fn in (P.clear_border, P.binary_fill_holes):
        with pytest.raises(ValueError, match="num must not be negative"):
            fn(lab if fn is P.clear_border else m, -1)


# ---- the statement against SciPy ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.binary_cases()), ids=str)
def test_binary_statement_equals_scipy(name):
    from scipy import ndimage

    mask, c, dilate, random = R.binary_cases()[name]
    fn = ndimage.binary_dilation if dilate else ndimage.binary_erosion
    for bv in (0, 1):
        got = R.binary_ref(mask, dilate, c, 1, bv)
        np.testing.assert_array_equal(got, fn(mask, _structure(mask.ndim, c), 1, border_value=bv).astype(np.uint8))
        if random:          # an all-zero erosion or an all-one dilation would let a broken kernel pass
            assert 0.01 <= got.mean() <= 0.99, (name, bv, got.mean())
    assert got.dtype == np.uint8


@pytest.mark.parametrize("c", (1, 2, 3))
def test_iterations_opening_and_closing_equal_scipy(c):
    from scipy import ndimage

    m = R.ball_volume()
    s = _structure(3, c)
    for bv in (0, 1):
        for k in (1, 2, 3, 7):
            np.testing.assert_array_equal(R.binary_erosion_ref(m, c, k, bv), ndimage.binary_erosion(m, s, k, border_value=bv))
            np.testing.assert_array_equal(R.binary_dilation_ref(m, c, k, bv), ndimage.binary_dilation(m, s, k, border_value=bv))
        for k in (1, 2):
            np.testing.assert_array_equal(R.binary_opening_ref(m, c, k, bv), ndimage.binary_opening(m, s, k, border_value=bv))
            np.testing.assert_array_equal(R.binary_closing_ref(m, c, k, bv), ndimage.binary_closing(m, s, k, border_value=bv))
    small = np.zeros_like(m)
    small[:14, :14, :14] = m[:14, :14, :14]                                                # the ball of radius 5 alone
    assert small.sum() > 0 and R.binary_erosion_ref(small, 1, 3, 1).any() and not R.binary_erosion_ref(small, 1, 7, 1).any()
    assert 0.01 <= R.binary_erosion_ref(m, 1, 3, 1).mean() and R.binary_dilation_ref(m, 1, 3, 0).mean() <= 0.99


@pytest.mark.parametrize("name", list(R.grey_cases()), ids=str)
def test_grey_statement_equals_scipy(name):
    from scipy import ndimage

    x = R.grey_cases()[name]
    for c in range(1, x.ndim + 1):
        s = _structure(x.ndim, c)
        np.testing.assert_array_equal(R.erosion_ref(x, c), ndimage.grey_erosion(x, footprint=s))
        np.testing.assert_array_equal(R.dilation_ref(x, c), ndimage.grey_dilation(x, footprint=s))
        assert R.erosion_ref(x, c).dtype == x.dtype


@pytest.mark.parametrize("key", list(R.span_cases()), ids=str)
def test_span_inputs_differ_across_every_lane_and_row_edge(key):
    from scipy import ndimage

    x = R.span_cases()[key]
    lane = R.LANE[x.dtype.type]
    rows_, X = x.shape
    fg = x > 0
    for k in range(1, (X - 1) // lane + 1):
        assert (fg[:, k * lane - 1] != fg[:, k * lane]).all(), k
    for y in range(rows_ - 1):
        assert fg[y, X - 1] != fg[y + 1, 0], y
    for c in (1, 2):
        s = _structure(2, c)
        np.testing.assert_array_equal(R.erosion_ref(x, c), ndimage.grey_erosion(x, footprint=s))
        np.testing.assert_array_equal(R.dilation_ref(x, c), ndimage.grey_dilation(x, footprint=s))
        if x.dtype == np.uint8:
            for bv in (0, 1):
                np.testing.assert_array_equal(R.binary_erosion_ref(x, c, 1, bv), ndimage.binary_erosion(x, s, border_value=bv))
                np.testing.assert_array_equal(R.binary_dilation_ref(x, c, 1, bv), ndimage.binary_dilation(x, s, border_value=bv))


@pytest.mark.parametrize("r", (1, 2, 3, 5))
def test_the_ball_identity(r):
    """The ball statement, SciPy with the ball footprint, and the threshold of SciPy's squared distance transform are one thing."""
    from scipy import ndimage

    m = R.ball_volume()
    g = np.indices((2 * r + 1,) * 3) - r
    ball = (g ** 2).sum(0) <= r * r
    dil, ero = R.ball_ref(m, r, True), R.ball_ref(m, r, False)
    np.testing.assert_array_equal(dil, ndimage.binary_dilation(m, ball, border_value=0))
    np.testing.assert_array_equal(ero, ndimage.binary_erosion(m, ball, border_value=1))
    d2 = lambda a: np.rint(ndimage.distance_transform_edt(a) ** 2).astype(np.int64)         # noqa: E731
    np.testing.assert_array_equal(dil, d2(m == 0) <= r * r)
    np.testing.assert_array_equal(ero, d2(m) > r * r)
    # the sentinel: without a zero (a one) the transform answers "farther than any r", which erodes (dilates) nothing
    ones, zeros = np.ones((6, 7, 8), np.uint8), np.zeros((6, 7, 8), np.uint8)
    assert R.ball_ref(ones, r, False).all() and not R.ball_ref(zeros, r, True).any()


def test_fill_holes_statement_equals_scipy_and_the_hand_made_cases():
    from scipy import ndimage

    for name, (mask, filled) in R.hand_cases().items():
        np.testing.assert_array_equal(R.fill_holes_ref(mask), filled, err_msg=name)
        np.testing.assert_array_equal(R.fill_holes_ref(mask), ndimage.binary_fill_holes(mask), err_msg=name)
    for m in (R.holes_volume(), R.ball_volume(), R.random_mask((33, 37, 41), 0.7, 3), R.random_mask((37, 41), 0.6, 4)):
        got = R.fill_holes_ref(m)
        np.testing.assert_array_equal(got, ndimage.binary_fill_holes(m))
        # the route the device takes: the background's components at connectivity 1 that touch no face
        lab, n = ndimage.label(m == 0)
        holes = np.isin(lab, [l for l in range(1, n + 1) if l not in R.border_ids(lab, n)])
        np.testing.assert_array_equal(got, (holes | (m != 0)))
    h = R.holes_volume()
    assert R.fill_holes_ref(h).sum() - h.sum() >= 20                                           # holes there are


def test_single_voxel_in_each_corner():
    from scipy import ndimage

    for corner, m in R.corner_cases().items():
        for c in (1, 2, 3):
            s = _structure(3, c)
            d = R.binary_dilation_ref(m, c)
            np.testing.assert_array_equal(d, ndimage.binary_dilation(m, s))
            assert d.sum() == {1: 4, 2: 7, 3: 8}[c], (corner, c)                               # the part of the element inside the volume
            assert not R.binary_erosion_ref(m, c, 1, 1).any()
            np.testing.assert_array_equal(R.binary_dilation_ref(m, c, 1, 1), ndimage.binary_dilation(m, s, border_value=1))
            b = R.find_boundaries_ref(m.astype(np.int32), c)
            np.testing.assert_array_equal(b, d)                                                # thick: the voxel and its neighbours
            assert R.find_boundaries_ref(m.astype(np.int32), c, "inner").sum() == 1


def test_boundaries_of_two_labels_that_touch():
    lab = R.touching_labels()
    thick, inner = R.find_boundaries_ref(lab, 1), R.find_boundaries_ref(lab, 1, "inner")
    assert thick[2, 3] == 1 and thick[2, 4] == 1                                               # both sides of the line where 1 meets 2
    assert thick[2, 2] == 0 and inner[2, 2] == 0                                               # inside label 1
    assert thick[2, 0] == 1 and inner[2, 0] == 0                                               # background next to label 1
    assert thick[0, 6] == 1 and inner[0, 7] == 1 and inner[0, 6] == 0
    np.testing.assert_array_equal(inner, thick & (lab != 0))
    np.testing.assert_array_equal(R.find_boundaries_ref(lab, 1, "inner", background=2), thick & (lab != 2))
    np.testing.assert_array_equal(R.find_boundaries_ref(-lab, 2), R.find_boundaries_ref(lab, 2))   # negative labels are ordinary values
    assert R.dilation_ref(lab, 1)[2, 3] == 2 and R.dilation_ref(lab, 1)[2, 0] == 1             # the largest neighbouring id wins


def test_a_label_on_each_face_is_cleared():
    lab = R.face_labels()
    assert R.border_ids(lab, 8) == {1, 2, 3, 4, 5, 6}
    out, left = R.clear_border_ref(lab, 8)
    assert left == 2 and set(np.unique(out)) == {0, 7}                                         # 7 survives, 8 is absent and counts, 9 > n_max goes
    out, left = R.clear_border_ref(lab, 8, relabel=True)
    assert left == 2 and set(np.unique(out)) == {0, 1}
    out, left = R.clear_border_ref(lab, 9)
    assert left == 3 and set(np.unique(out)) == {0, 7, 9}
    two = R.touching_labels()
    assert R.border_ids(two, 3) == {3}
    assert set(np.unique(R.clear_border_ref(two, 3)[0])) == {0, 1, 2}

"""Local maxima on the MI355X (biapy_amd/prepost.py: peak_mask, peak_local_max; csrc/peaks.hip) against the NumPy twin of their definition
(tests/peaks_ref.py, itself held against scikit-image's mask by test_peaks_cpu.py).  Every comparison is bit for bit: the search is integer
arithmetic on keys.  Every test but the one about ``max_peaks`` uses the default ``max_peaks``, which these shapes (n <= 27 300) cannot
exceed.  Inputs and references are built once per process."""
import numpy as np
import pytest
import torch

import peaks_ref as R

pytestmark = pytest.mark.gpu


def _P():
    from biapy_amd import prepost

    return prepost


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                                  # a copy: the shared inputs are read-only


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(img, r, thr, border, what=""):
    """peak_mask and peak_local_max of `img` on the device against the twin; returns the number of peaks."""
    P = _P()
    what = (what, img.shape, r, thr, border)
    d = _dev(img)
    want_mask = R.peak_mask_ref(img, r, thr, border)
    want_coords, want_values = R.peak_list_ref(img, r, thr, border)
    K = len(want_coords)
    mask = P.peak_mask(d, r, thr, border)
    assert mask.is_cuda and mask.dtype == torch.uint8 and tuple(mask.shape) == img.shape, what
    np.testing.assert_array_equal(mask.cpu().numpy(), want_mask, err_msg=str(what))
    coords, values, num = P.peak_local_max(d, r, thr, border, return_values=True)
    mp = min(img.size, 2 ** 20)
    assert coords.is_cuda and coords.dtype == torch.int32 and tuple(coords.shape) == (mp, img.ndim), what
    assert values.dtype == d.dtype and tuple(values.shape) == (mp,) and num.is_cuda and num.dtype == torch.int32 and num.dim() == 0, what
    assert int(num) == K, (what, int(num), K)
    np.testing.assert_array_equal(coords[:K].cpu().numpy(), want_coords, err_msg=str(what))
    np.testing.assert_array_equal(_bits(values[:K].cpu().numpy()), _bits(want_values), err_msg=str(what))     # -0.0 is not +0.0 here
    assert (coords[K:] == -1).all() and (_bits(values[K:].cpu().numpy()) == 0).all(), what
    only, n2 = P.peak_local_max(d, r, thr, border)
    assert torch.equal(only, coords) and int(n2) == K, what
    np.testing.assert_array_equal(_bits(d.cpu().numpy()), _bits(img), err_msg="the input is left alone")
    return K


def _radii(r, ndim):
    return R.per_axis(r, ndim) if isinstance(r, tuple) else r


# ---- tie-free and quantised inputs ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_tie_free_and_quantised_images(shape):
    total = 0
    for r in R.RADII:
        r = _radii(r, len(shape))
        for border in (False, True):
            total += _check(R.tie_free(shape), r, 0.5, border, "tie-free")
            total += _check(R.quantised(shape), r, 0.5, border, "quantised")
    _check(R.tie_free(shape), 1, None, True, "threshold_abs=None")
    _check(R.tie_free(shape), 1, -np.inf, 0, "no threshold")
    assert total > 0


def test_box_larger_than_the_volume_and_single_axis_radii():
    for img in (R.tie_free((2, 3, 5)), R.quantised((2, 3, 5), 3)):
        assert _check(img, 8, -np.inf, 0) == 1                                              # the volume's raster-first maximum
        _check(img, (8, 0, 8), -np.inf, 0)
    row = R.tie_free((1, 1, 300))
    for r in ((0, 0, 3), (3, 0, 0), (0, 0, 0), 64, (0, 0, 64), (64, 64, 0)):
        _check(row, r, 0.25, 0)
        _check(R.quantised((1, 1, 300), 12), r, 0.25, 0)
    assert _check(row, (3, 0, 0), 0.25, 0) == _check(row, 0, 0.25, 0) == int((row > 0.25).sum())       # radii along axes of one voxel change nothing
    for r in ((0, 0, 5), (0, 5, 0), (5, 0, 0), (0, 2, 3), (3, 2, 0), (3, 0, 2), 0):
        _check(R.tie_free((9, 21, 37)), r, 0.5, 0)
        _check(R.quantised((9, 21, 37)), r, 0.5, (1, 0, 2))


# ---- dtypes and special values ------------------------------------------------------------------------------------------------------------------------

def test_int32_images():
    edt = R.squared_edt((9, 21, 37))
    assert edt.dtype == np.int32 and edt.max() >= 4
    for r in (1, 2, (1, 2, 3)):
        assert _check(edt, r, 0, False, "squared EDT") > 0
        _check(edt, r, None, True, "squared EDT")
        _check(-edt, r, -3, False, "negative values")
    rng = np.random.default_rng(5)
    lim = np.iinfo(np.int32)
    ends = rng.choice(np.array([lim.min, lim.min + 1, -1, 0, 1, lim.max - 1, lim.max], np.int32), (5, 6, 7))
    for thr in (-np.inf, None, 0, lim.max - 1, lim.max):
        _check(ends, 1, thr, False, "INT32_MIN / INT32_MAX")
    _check(R.squared_edt((37, 41)), 2, 1, True, "2-D int32")


def test_infinities_and_signed_zeros():
    rng = np.random.default_rng(6)
    inf = rng.choice(np.array([-np.inf, -1.0, 0.0, 1.0, np.inf], np.float32), (5, 6, 7))
    for thr in (-np.inf, None, 0.0, np.inf, 3.0e38):
        _check(inf, 1, thr, False, "infinities")
    zeros = np.zeros((9, 21, 37), np.float32)
    zeros.reshape(-1)[rng.choice(zeros.size, 40, replace=False)] = -0.0
    zeros[0, 0, :3] = -0.0                                                                   # so that index 0 does not win everything
    assert np.signbit(zeros).sum() >= 40
    for r in (1, 3, 0):
        K = _check(zeros, r, -1.0, False, "signed zeros")
        assert K >= 1
    _check(zeros, 1, None, False, "signed zeros, threshold -0.0")                            # image.min() is -0.0 == +0.0: nothing is above it
    _check(-zeros, 1, -1.0, False, "mostly -0.0")


# ---- degenerate volumes -------------------------------------------------------------------------------------------------------------------------------

def test_constant_volume_and_single_voxel():
    P = _P()
    for shape in ((6, 7, 19), (7, 19)):
        const = np.full(shape, 2.0, np.float32)
        for r in (1, 4, 64):
            assert _check(const, r, 1.0, False) == 1
            coords, _ = P.peak_local_max(_dev(const), r, 1.0, False)
            assert coords[0].tolist() == [0] * len(shape)                                     # index 0
            assert _check(const, r, 2.0, False) == 0 and _check(const, r, None, False) == 0 and _check(const, r, 1.0, True) == 0
        _check(const.astype(np.int32), 2, 1, False)
    one = np.array([[[0.75]]], np.float32)
    assert _check(one, 1, 0.5, False) == 1 and _check(one, 0, 0.5, False) == 1 and _check(one, 64, 0.5, 0) == 1
    assert _check(one, 1, 0.75, False) == 0 and _check(one, 1, 0.5, True) == 0 and _check(one, 1, None, False) == 0
    assert _check(one[0], 1, 0.5, False) == 1


# ---- borders and alignment ------------------------------------------------------------------------------------------------------------------------------

def test_exclude_border_beyond_half_an_extent():
    img = R.tie_free((5, 6, 7))
    assert _check(img, 1, -np.inf, (0, 3, 0)) == 0 and _check(img, 1, -np.inf, (3, 0, 0)) == 0 and _check(img, 1, -np.inf, 100) == 0
    _check(img, 1, -np.inf, (2, 2, 3))
    _check(img, 0, -np.inf, (2, 2, 3))
    for b in (1, 2, (0, 1, 3), (4, 0, 0)):
        _check(R.tie_free((9, 21, 37)), 2, 0.5, b)
        _check(R.quantised((37, 41)), 2, 0.5, b[1:] if isinstance(b, tuple) else b)


def test_unaligned_view_of_a_batch():
    P = _P()
    rng = np.random.default_rng(7)
    for dtype in (np.float32, np.int32):
        stack = np.floor(rng.random((2, 5, 6, 7)) * 50).astype(dtype)
        d = _dev(stack)
        view = d[1]
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        for r in (1, 2, (1, 0, 3)):
            want = R.peak_mask_ref(stack[1], r, 10, False)
            np.testing.assert_array_equal(P.peak_mask(view, r, 10, False).cpu().numpy(), want)
            coords, values, num = P.peak_local_max(view, r, 10, False, return_values=True)
            wc, wv = R.peak_list_ref(stack[1], r, 10, False)
            assert int(num) == len(wc) > 0
            np.testing.assert_array_equal(coords[:len(wc)].cpu().numpy(), wc)
            np.testing.assert_array_equal(_bits(values[:len(wc)].cpu().numpy()), _bits(wv))
            assert torch.equal(P.peak_mask(view.clone(), r, 10, False), P.peak_mask(view, r, 10, False))       # aligned copy: the same bits
        assert torch.equal(d.cpu(), torch.from_numpy(stack))


def test_2d_call_equals_the_one_plane_volume():
    P = _P()
    for img in (R.tie_free((37, 41)), R.quantised((37, 41))):
        d = _dev(img)
        for r, b in ((1, True), (2, False), ((2, 3), (1, 0))):
            r3 = (0,) + r if isinstance(r, tuple) else (0, r, r)
            b3 = (0,) + b if isinstance(b, tuple) else ((0, r, r) if b else 0)
            assert torch.equal(P.peak_mask(d, r, 0.5, b)[None], P.peak_mask(d[None], r3, 0.5, b3))
            c2, v2, n2 = P.peak_local_max(d, r, 0.5, b, return_values=True)
            c3, v3, n3 = P.peak_local_max(d[None], r3, 0.5, b3, return_values=True)
            K = int(n2)
            assert K == int(n3) > 0 and torch.equal(c2[:K], c3[:K, 1:]) and (c3[:K, 0] == 0).all() and torch.equal(v2, v3)


# ---- outputs ------------------------------------------------------------------------------------------------------------------------------------------

def test_num_peaks_and_max_peaks():
    P = _P()
    img = R.tie_free((9, 21, 37))
    d = _dev(img)
    wc, wv = R.peak_list_ref(img, 2, 0.5, False)
    K = len(wc)
    assert K >= 8
    for k in (1, 3, K, K + 5):
        coords, values, num = P.peak_local_max(d, 2, 0.5, False, num_peaks=k, return_values=True)
        assert tuple(coords.shape) == (k, 3) and tuple(values.shape) == (k,) and int(num) == min(K, k)
        m = min(K, k)
        np.testing.assert_array_equal(coords[:m].cpu().numpy(), wc[:m])                       # the k largest
        np.testing.assert_array_equal(values[:m].cpu().numpy(), wv[:m])
        assert (coords[m:] == -1).all() and (values[m:] == 0).all()
    for mp in (K, K + 1, 4 * K):                                                              # enough room: the whole list
        coords, num = P.peak_local_max(d, 2, 0.5, False, max_peaks=mp)
        assert tuple(coords.shape) == (mp, 3) and int(num) == K
        np.testing.assert_array_equal(coords[:K].cpu().numpy(), wc)
        assert (coords[K:] == -1).all()
    for mp in (1, K // 2, K - 1):                                                             # not enough: num says so
        coords, num = P.peak_local_max(d, 2, 0.5, False, max_peaks=mp)
        assert tuple(coords.shape) == (mp, 3) and int(num) == -1
        coords, num = P.peak_local_max(d, 2, 0.5, False, max_peaks=mp, num_peaks=3)
        assert tuple(coords.shape) == (min(mp, 3), 3) and int(num) == -1
    coords, num = P.peak_local_max(d, 2, 0.5, False, max_peaks=K + 2, num_peaks=K + 7)
    assert tuple(coords.shape) == (K + 2, 3) and int(num) == K


def test_no_two_peaks_share_a_box():
    P = _P()
    for img, r in ((R.quantised((9, 21, 37)), 1), (R.quantised((9, 21, 37)), (1, 2, 3)), (R.squared_edt((9, 21, 37)), 2)):
        thr = 0.5 if img.dtype == np.float32 else 0
        mask = P.peak_mask(_dev(img), r, thr, False).cpu().numpy()
        assert mask.sum() > 1 and R.no_two_in_a_box(mask, r)
        if img.dtype == np.float32:
            sk = R.scipy_mask(img, r, thr, 0)
            assert ((mask == 1) <= (sk == 1)).all() and mask.sum() < sk.sum()                # a strict subset of scikit-image's mask on ties
    row = R.plateau_row()
    coords, num = P.peak_local_max(_dev(row), (0, 2), 0.5, False)
    assert int(num) == 1 and coords[0].tolist() == [0, 3]


# ---- runtime behaviour ----------------------------------------------------------------------------------------------------------------------------------

def test_two_runs_give_the_same_bits():
    P = _P()
    d = _dev(R.quantised((3, 70, 130)))
    first = P.peak_local_max(d, 2, 0.5, False, return_values=True)
    for _ in range(3):
        again = P.peak_local_max(d, 2, 0.5, False, return_values=True)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert int(first[2]) > 10
    assert torch.equal(P.peak_mask(d, 2, 0.5, False), P.peak_mask(d, 2, 0.5, False))


def test_capture_in_a_graph_and_replay_on_new_contents():
    P = _P()
    a, b = R.tie_free((9, 21, 37)), R.quantised((9, 21, 37), 40, 1)
    buf = _dev(a)
    P.peak_local_max(buf, (1, 2, 3), 0.5, True, return_values=True)                          # warm-up outside the capture
    P.peak_mask(buf, (1, 2, 3), 0.5, True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        coords, values, num = P.peak_local_max(buf, (1, 2, 3), 0.5, True, return_values=True)
        mask = P.peak_mask(buf, (1, 2, 3), 0.5, True)
    for img in (b, a, b):
        buf.copy_(torch.from_numpy(np.array(img)))
        g.replay()
        torch.cuda.synchronize()
        wc, wv = R.peak_list_ref(img, (1, 2, 3), 0.5, True)
        K = len(wc)
        assert int(num) == K > 0
        np.testing.assert_array_equal(coords[:K].cpu().numpy(), wc)
        np.testing.assert_array_equal(values[:K].cpu().numpy(), wv)
        assert (coords[K:] == -1).all()
        np.testing.assert_array_equal(mask.cpu().numpy(), R.peak_mask_ref(img, (1, 2, 3), 0.5, True))


# ---- the recipe -----------------------------------------------------------------------------------------------------------------------------------------

def test_marker_recipe_splits_two_overlapping_balls():
    P = _P()
    fg = _dev(R.two_balls())
    assert int(P.label(fg, return_num=True)[1]) == 1                                          # one component before
    edt = P.distance_transform_edt(fg, squared=True)
    markers, n = P.label(P.peak_mask(edt, 4, 0, False), return_num=True)
    assert int(n) == 2
    inst = P.watershed(-edt, markers, mask=fg)
    got = inst.cpu().numpy()
    assert set(np.unique(got)) == {0, 1, 2} and ((got > 0) == (R.two_balls() > 0)).all()
    assert got[10, 10, 10] != got[10, 10, 20] and min((got == 1).sum(), (got == 2).sum()) > 500

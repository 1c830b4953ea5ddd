"""The scans either side of the network on the MI355X (biapy_amd/prepost.py, csrc/prepost.hip) at their edges: negative values, ties,
signed zeros, denormals, infinities, n < 4 and n % 4 != 0, more elements than the capped grid covers in one sweep, both LDS layouts of the
histogram, values exactly on a bin edge, views that are contiguous but not 16-byte aligned, NaN.  Order statistics, percentiles, min / max,
histogram counts, masks and the arg-max are compared exactly; mean / std within a bound derived from the arithmetic (test_mean_std).
Inputs and references: tests/prepost_ref.py, computed once per process."""
import math

import numpy as np
import pytest
import torch

import prepost_ref as R
from oracle import prepost_oracle as PO

pytestmark = pytest.mark.gpu


def _P():
    from biapy_amd import prepost

    return prepost


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()           # a copy: the references are read-only, torch wants a writable array


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int32)


# ---- order statistics ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", R.CLASSES)
def test_kth_values(cls):
    """x_sorted[k] at {0, 1, n//3, n//2, n-2, n-1} and, for the tied classes, at both ends of the tie run around the median; every size.
    Compared with ``==``: -0.0 and +0.0 tie in ``np.sort`` and may come back as either."""
    P = _P()
    for n in R.SIZES:
        ks, s = R.ranks(cls, n), R.sorted_sample(cls, n)
        got = P.kth_values(_dev(R.sample(cls, n)), ks)
        want = [float(s[k]) for k in ks]
        assert got == want, (cls, n, ks, got, want)


@pytest.mark.parametrize("cls", ["signed", "u8", "sigmoid"])
def test_percentile(cls):
    P = _P()
    for n in R.SIZES:
        x = _dev(R.sample(cls, n))
        for q in R.QS:
            assert P.percentile(x, q) == R.percentile_ref(cls, n, q), (cls, n, q)


@pytest.mark.parametrize("cls", ["signed", "u8", "sigmoid"])
def test_percentile_clip(cls):
    """Bounds equal to ``float(np.percentile(x, q))`` and the clipped tensor bit-identical to ``np.clip``; a sample that happens to hold only
    0 / 1 (small n) takes the early return on both sides."""
    P = _P()
    for n in R.SIZES:
        x = R.sample(cls, n)
        xd = _dev(x)
        for lo, hi in ((0.1, 99.9), (1, 99), (5, 50), (33.3, 99)):
            want, wlo, whi = PO.percentile_clip(x, lo, hi)
            got, glo, ghi = P.percentile_clip(xd, lo, hi)
            assert (glo, ghi) == (wlo, whi), (cls, n, lo, hi)
            if PO.is_binary_channel(x):
                assert got is xd and (glo, ghi) == (0.0, 1.0)
            else:
                assert (glo, ghi) == (R.percentile_ref(cls, n, lo), R.percentile_ref(cls, n, hi))
                assert got.dtype == torch.float32 and want.dtype == np.float32
                np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=f"{cls} {n} {lo} {hi}")


@pytest.mark.parametrize("case", R.binary_like(), ids=lambda c: c[0])
def test_binary_channels_are_left_alone_where_the_reference_leaves_them(case):
    """norm.py:38-42: a channel of 0 / 1 only is returned as it is with bounds (0, 1); {0.25, 0.75}, a 0.5, a denormal, -1e-40 or 1 + ulp
    among the 0 / 1 end that."""
    P = _P()
    name, a, binary = case
    ad = _dev(a)
    assert P._is_binary(ad) == binary
    got, lo, hi = P.percentile_clip(ad, 1, 99)
    want, wlo, whi = PO.percentile_clip(a, 1, 99)
    assert (got is ad) == binary and (lo, hi) == (wlo, whi)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    got, mean, std = P.zero_mean_unit_variance_normalization(ad)
    assert (got is ad) == binary and ((mean, std) == (0.0, 1.0)) == binary


# ---- min / max, moments, normalisation ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", R.CLASSES)
def test_minmax(cls):
    P = _P()
    for n in R.SIZES:
        x = R.sample(cls, n)
        assert P.minmax(_dev(x)) == (float(x.min()), float(x.max())), (cls, n)


@pytest.mark.parametrize("n,where", [(1025, 0), (1025, 512), (1025, 1024), (1025, 301), (4099, 2500), (4099, 4098), (3, 1)])
def test_minmax_returns_nan_for_a_single_nan(n, where):
    """``ndarray.min()`` / ``.max()`` of data with one NaN are NaN - through the thread loop, the wave shuffles, the block reduce and the
    reduction of the partials, whatever follows the NaN.  n = 1025: first, middle and last position (the last one is the tail element), and
    one that is neither the first element of its thread nor in the first lane or wave.  n = 4099: five blocks, the NaN in the share of the
    third (so the other blocks' partials are numbers) and at the very end."""
    P = _P()
    for cls in ("signed", "extreme"):
        x = R.sample(cls, n).copy()
        x[where] = np.nan
        assert np.isnan(x.min()) and np.isnan(x.max())
        mn, mx = P.minmax(_dev(x))
        assert math.isnan(mn) and math.isnan(mx), (cls, where, mn, mx)
        assert not P._is_binary(_dev(x))
    b = (np.arange(n) % 2).astype(np.float32)                                   # 0 / 1 and one NaN: not a binary channel
    b[where] = np.nan
    assert not P._is_binary(_dev(b)) and not PO.is_binary_channel(b)


@pytest.mark.parametrize("cls", ["signed", "u8", "two", "zeros", "sigmoid"])
def test_mean_std(cls):
    """Against ``np.mean`` / ``np.std`` with ``dtype=float64``.  The bound is derived, not measured.  Every term (x - c) or (x - c)^2 is formed
    in double from a float32 x: relative error at most 2^-53 each (the difference of a float32 and a double, then one product).  A sum of n
    such terms in ANY order - the thread's running sum, the shuffle tree, the block partials, the final reduction - is off by at most
    (n - 1) 2^-53 sum|term| to first order, and the reference's own pairwise sum by less; the factor 2 covers both and the tree.  Hence
        |mean - ref| <= 2 n 2^-53 mean|x|,
    and, the terms of the variance being non-negative (sum|term| = the sum itself), a relative error of 2 n 2^-53 on each side of the
    comparison, 4 n 2^-53 for the std to be safe (the square root halves it; the device mean in place of the exact one changes the sum of
    squares by n (mean - ref)^2, second order).  At n = 4099 these are 9e-13 relative - a float32 accumulation would miss them by orders of
    magnitude.  n = 1: the mean is x itself and the std exactly 0."""
    P = _P()
    for n in R.SIZES:
        x = R.sample(cls, n)
        mref, sref = R.mean_std_ref(x)
        dm, ds = R.mean_std_bounds(x)
        mean, std = P.mean_std(_dev(x))
        print(f"mean_std {cls} n={n}: |mean - ref| {abs(mean - mref):.3e} (allowed {dm:.3e}), std rel {abs(std - sref) / sref if sref else abs(std):.3e} (allowed {ds:.3e})")
        assert abs(mean - mref) <= dm, (cls, n, mean, mref)
        assert abs(std - sref) <= ds * sref, (cls, n, std, sref)


@pytest.mark.parametrize("v", R.CONSTANTS + (255.0, 1e-40))
def test_mean_std_of_a_constant_volume(v):
    """n v is exact in double for a float32 v and n = 315, and so is its quotient by n: the mean is v itself, the std at most 2^-50 |v|."""
    P = _P()
    x = torch.full(R.CONSTANT_SHAPE, v, dtype=torch.float32, device="cuda")
    mean, std = P.mean_std(x)
    assert mean == float(np.float32(v)) and 0.0 <= std <= 2.0 ** -50 * abs(v), (v, mean, std)


@pytest.mark.parametrize("cls", ["signed", "u8", "two", "sigmoid"])
def test_zero_mean_unit_variance_normalization_is_the_float32_statement(cls):
    """The output is ``(x - float32(mean)) / float32(max(std, eps))`` in float32 operations, with the mean and std the call returned, bit
    for bit: one subtraction and one IEEE division, no contraction, no reciprocal."""
    P = _P()
    for n in R.SIZES:
        x = R.sample(cls, n)[None]
        xd = _dev(x)
        got, mean, std = P.zero_mean_unit_variance_normalization(xd)
        if PO.is_binary_channel(x):
            assert got is xd and (mean, std) == (0.0, 1.0)
            continue
        assert (mean, std) == P.mean_std(xd) and got.shape == x.shape and got.dtype == torch.float32
        np.testing.assert_array_equal(_bits(got), _bits(R.znorm_ref(x, mean, std)), err_msg=f"{cls} {n}")
    x = R.sample(cls, 4099)[None]                                                    # given statistics, and a std below eps
    for mean, std in ((12.5, 3.0), (0.1, 1e-9), (-7.0, 0.0)):
        got, m, s = P.zero_mean_unit_variance_normalization(_dev(x), mean=mean, std=std)
        assert (m, s) == (mean, std)
        np.testing.assert_array_equal(_bits(got), _bits(R.znorm_ref(x, mean, std)))


# ---- histogram, Otsu, binarisation --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nbins", R.NBINS)
@pytest.mark.parametrize("cls", R.HIST_CLASSES)
def test_histogram_on_the_edges(cls, nbins):
    """Inputs ON every edge and one ulp either side of it; 1024 / 1025 bins are the last size with one LDS copy of the counts per wave and
    the first with a single copy.  Counts and edges are ``np.histogram``'s."""
    x, mn, mx, _ = R.hist_input(cls, nbins)
    counts, edges = _P().histogram(_dev(x), nbins)
    want, wedges = R.hist_ref(cls, nbins)
    assert counts.dtype == np.int64 and edges.dtype == np.float32
    np.testing.assert_array_equal(_bits(edges), _bits(wedges))
    np.testing.assert_array_equal(counts, want)


@pytest.mark.parametrize("case", R.refused_inputs(), ids=lambda c: c[0])
def test_histogram_refuses_what_numpy_refuses(case):
    """A NaN, a +inf, and max = nextafter(min) at 1025 bins: ``ValueError`` on both sides, nothing counted into duplicate edges."""
    P = _P()
    name, x, nbins = case
    with pytest.raises(ValueError):
        np.histogram(x, bins=nbins, range=(x.min(), x.max()))
    with pytest.raises(ValueError, match="Too many bins" if name == "narrow" else "not finite"):
        P.histogram(_dev(x), nbins)
    if name != "narrow":
        with pytest.raises(ValueError, match="not finite"):
            P.threshold_otsu(_dev(x))
    else:
        counts, _ = P.histogram(_dev(x), 1)                                          # one bin is no problem
        assert counts.tolist() == [1025]


@pytest.mark.parametrize("cls", ["sigmoid", "u8", "two"])
def test_threshold_otsu_and_binarize(cls):
    """Threshold and mask equal to the oracle's; n = 1, 3, 5, 4099 end in the byte tail of the packed store.  A sample that happens to be
    constant (n = 1, or all equal) gives the value itself and an empty mask on both sides."""
    P = _P()
    for n in R.SIZES:
        x = R.sample(cls, n)
        xd = _dev(x)
        assert P.threshold_otsu(xd) == PO.threshold_otsu(x), (cls, n)
        got = P.binarize(xd)
        assert got.dtype == torch.uint8 and got.shape == x.shape
        np.testing.assert_array_equal(got.cpu().numpy(), PO.binarize(x), err_msg=f"{cls} {n}")
        for th in (float(x.min()), float(np.sort(x)[n // 2]), float(x.max())):      # a threshold ON values of the data: strictly greater
            np.testing.assert_array_equal(P.binarize(xd, threshold=th).cpu().numpy(), (x > np.float32(th)).astype(np.uint8))


@pytest.mark.parametrize("v", R.CONSTANTS)
def test_constant_volume_gives_its_value_and_an_empty_mask(v):
    """A blank tile (a saturated sigmoid): skimage's ``threshold_otsu`` returns the value, so ``pred > th`` is empty - not all foreground."""
    P = _P()
    x = np.full(R.CONSTANT_SHAPE, v, np.float32)
    xd = _dev(x)
    assert PO.threshold_otsu(x) == float(np.float32(v)) and not PO.binarize(x).any()
    assert P.threshold_otsu(xd) == float(np.float32(v))
    mask = P.binarize(xd)
    assert mask.shape == R.CONSTANT_SHAPE and mask.dtype == torch.uint8 and int(mask.sum()) == 0
    counts, edges = P.histogram(xd, 256)                                             # the histogram itself still widens the range, as NumPy
    want, wedges = np.histogram(x, bins=256, range=(x.min(), x.max()))
    np.testing.assert_array_equal(counts, want)
    np.testing.assert_array_equal(_bits(edges), _bits(wedges))


# ---- views that are contiguous but not 16-byte aligned ------------------------------------------------------------------------------------

def _misaligned_views():
    base = _dev(R.sample("signed", 4100))
    stack = _dev(np.stack([R.sample(c, 315).reshape(R.CONSTANT_SHAPE) for c in ("u8", "sigmoid", "signed")]))
    tied = _dev(R.sample("u8", 4100))
    return [("base[1:]", base[1:]), ("stack[1]", stack[1]), ("stack[2]", stack[2]), ("u8[3:]", tied[3:])]


def test_misaligned_views_give_what_their_aligned_copies_give():
    """``base[1:]`` of an aligned flat tensor and ``stack[k]`` of a (3, 5, 7, 9) tensor (315 elements per item: 12 and 8 bytes past a 16-byte
    boundary) are contiguous and only 4-byte aligned.  Every scan returns EXACTLY what it returns on ``.clone()``: a thread owns the same four
    elements either way, so even the double sums of mean / std are formed in the same order."""
    P = _P()
    for name, view in _misaligned_views():
        copy = view.clone()
        assert view.is_contiguous() and view.data_ptr() % 16 != 0 and view.data_ptr() % 4 == 0 and copy.data_ptr() % 16 == 0, name
        n = view.numel()
        ks = [0, 1, n // 3, n // 2, n - 2, n - 1]
        host = view.cpu().numpy().reshape(-1)
        assert P.kth_values(view, ks) == P.kth_values(copy, ks) == [float(np.sort(host)[k]) for k in ks], name
        a, alo, ahi = P.percentile_clip(view, 0.1, 99.9)
        b, blo, bhi = P.percentile_clip(copy, 0.1, 99.9)
        assert (alo, ahi) == (blo, bhi) == (float(np.percentile(host, 0.1)), float(np.percentile(host, 99.9))), name
        assert a.shape == view.shape and np.array_equal(_bits(a), _bits(b)), name
        assert P.minmax(view) == P.minmax(copy) == (float(host.min()), float(host.max())), name
        assert P.mean_std(view) == P.mean_std(copy), name
        for nbins in (256, 1025):
            (ca, ea), (cb, eb) = P.histogram(view, nbins), P.histogram(copy, nbins)
            assert np.array_equal(ca, cb) and np.array_equal(_bits(ea), _bits(eb)), name
            assert np.array_equal(ca, np.histogram(host, bins=nbins, range=(host.min(), host.max()))[0]), name
        assert P.threshold_otsu(view) == P.threshold_otsu(copy) == PO.threshold_otsu(host), name
        ma, mb = P.binarize(view), P.binarize(copy)
        assert ma.shape == view.shape and torch.equal(ma, mb) and np.array_equal(ma.cpu().numpy().reshape(-1), PO.binarize(host)), name
        za, zb = P.zero_mean_unit_variance_normalization(view[None]), P.zero_mean_unit_variance_normalization(copy[None])
        assert za[1:] == zb[1:] and np.array_equal(_bits(za[0]), _bits(zb[0])), name
        # the mask of binarize() is always a fresh, aligned tensor; the entry point also takes one that is not (bytes instead of packed words)
        from biapy_amd import _lib as L

        room = torch.full((n + 8,), 7, dtype=torch.uint8, device="cuda")
        for src in (view, copy):
            for off in (1, 2, 3):
                room.fill_(7)
                L.check(L.lib.bpx_threshold_u8(src.data_ptr(), n, 0.25, room.data_ptr() + off, L.stream_ptr()))
                got = room.cpu().numpy()
                assert np.array_equal(got[off:off + n], (host > np.float32(0.25)).astype(np.uint8)) and (got[:off] == 7).all() and (got[off + n:] == 7).all(), (name, off)


# ---- more elements than the capped grid covers in one sweep -------------------------------------------------------------------------------

def test_large_volume_past_the_grid_cap():
    """n = 2^24 + 4099 (67 MB), ``signed``: the float4 loops of the select, the moments, the histogram and the threshold run on 4096 blocks and
    wrap, n - 1 is no float32 any more, and three elements are left for the tail."""
    P = _P()
    x = R.large()
    xd = _dev(x)
    stats = R.large_order_stats()
    ks = [0, 1, R.LARGE // 3, R.LARGE // 2, R.LARGE - 2, R.LARGE - 1]
    assert P.kth_values(xd, ks) == [stats[k] for k in ks]
    for q in (0.1, 33.3, 99.9):
        assert P.percentile(xd, q) == R.percentile_ref("signed", R.LARGE, q), q
    assert P.minmax(xd) == (stats[0], stats[R.LARGE - 1])
    mref, sref = R.mean_std_ref(x)
    dm, ds = R.mean_std_bounds(x)
    mean, std = P.mean_std(xd)
    print(f"mean_std large: |mean - ref| {abs(mean - mref):.3e} (allowed {dm:.3e}), std rel {abs(std - sref) / sref:.3e} (allowed {ds:.3e})")
    assert abs(mean - mref) <= dm and abs(std - sref) <= ds * sref
    counts, edges = P.histogram(xd, 256)
    want, wedges = np.histogram(x, bins=256, range=(x.min(), x.max()))
    np.testing.assert_array_equal(counts, want)
    np.testing.assert_array_equal(_bits(edges), _bits(wedges))
    th = stats[R.LARGE // 3]
    mask = P.binarize(xd, threshold=th).cpu().numpy()
    np.testing.assert_array_equal(mask, (x > np.float32(th)).astype(np.uint8))


# ---- class arg-max ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vox", R.ARGMAX_VOXELS)
@pytest.mark.parametrize("C,k", R.ARGMAX_CK)
def test_class_argmax_first_maximum_wins(vox, C, k):
    """Values from {0, 0.25, 0.5, 1}: tied maxima in more than a third of the voxels.  The leading C - k channels pass through bit for bit, the
    last channel is ``np.argmax`` over the class channels - the FIRST maximum."""
    from biapy_amd import _lib as L

    a = R.argmax_input(vox, C)
    ad = _dev(a)
    out = torch.full((vox, C - k + 1), -7.0, dtype=torch.float32, device="cuda")
    L.check(L.lib.bpx_class_argmax(ad.data_ptr(), vox, C, k, out.data_ptr(), L.stream_ptr()))
    np.testing.assert_array_equal(_bits(out), _bits(R.argmax_ref(a, k)))
    np.testing.assert_array_equal(_bits(ad), _bits(a))                               # the input is left alone

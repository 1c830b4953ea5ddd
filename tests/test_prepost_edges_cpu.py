"""The scans of ``biapy_amd.prepost`` at their edges - what can be checked without a GPU: that the generators of tests/prepost_ref.py make
what the device tests rely on (signs, ties that straddle the chosen ranks, inputs sitting exactly on bin edges, tied class maxima), and the
host arithmetic of the product: ``percentile``'s interpolation driven by ``np.partition`` order statistics against ``np.percentile``, the
float32 bin-edge table against ``np.histogram``'s, and its two refusals."""
import numpy as np
import pytest

import prepost_ref as R

A = 4096                                   # any non-null, aligned "device" address: nothing is launched


def _P():
    from biapy_amd import prepost

    return prepost


def test_classes_are_what_they_claim():
    n = 4099
    s = R.sample("signed", n)
    assert (s < 0).sum() > n // 3 and (s > 0).sum() > n // 3 and len(np.unique(s)) > n - 10
    u = R.sample("u8", n)
    assert np.array_equal(u, np.round(u)) and u.min() == 0 and u.max() == 255 and len(np.unique(u)) == 256
    assert set(np.unique(R.sample("two", n)).tolist()) == {0.25, 0.75}
    z = R.sample("zeros", n)
    zero = z[z == 0]
    assert np.signbit(zero).any() and not np.signbit(zero).all()                     # -0.0 and +0.0
    assert ((z != 0) & (np.abs(z) < np.finfo(np.float32).tiny)).sum() > n // 6       # denormals of both signs
    assert (z == np.float32(1e-40)).any() and (z == np.float32(-1e-40)).any()
    e = R.sample("extreme", n)
    for v in (np.inf, -np.inf, np.finfo(np.float32).max, -np.finfo(np.float32).max, np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny, 0.5):
        assert (e == np.float32(v)).any(), v
    g = R.sample("sigmoid", n)
    assert g.min() == 0.0 and g.max() == 1.0 and (g == 0).sum() >= 2 and (g == 1).sum() >= 2      # saturated on both sides, exactly
    assert ((g > 0) & (g < 1)).sum() > n // 2 and len(np.unique(g)) < n                            # and ties next to the ends
    for cls in R.CLASSES:
        for m in R.SIZES:
            x = R.sample(cls, m)
            assert x.dtype == np.float32 and x.shape == (m,) and not x.flags.writeable and not np.isnan(x).any()
            assert np.array_equal(x.view(np.int32), R.sample(cls, m).view(np.int32))             # seeded: the same bits every time
    assert R.LARGE > 2 ** 24 + 4096 and R.LARGE % 4 == 3 and R.LARGE // 4 > 4096 * 1024


@pytest.mark.parametrize("cls", ["u8", "two"])
def test_tie_runs_straddle_the_chosen_ranks(cls):
    """The tied classes are asked for the first and the last index of the tie run around the median: ranks whose left neighbour, right
    neighbour or both hold the same value - a select that breaks ties wrongly lands on another value at one of them."""
    for n in R.SIZES:
        s, ks = R.sorted_sample(cls, n), R.ranks(cls, n)
        assert ks == sorted(set(ks)) and all(0 <= k < n for k in ks)
        assert {0, n - 1, n // 2, n // 3} <= set(ks)
        first, last = R.tie_run(s, n // 2)
        assert first in ks and last in ks and first <= n // 2 <= last and s[first] == s[last] == s[n // 2]
        assert first == 0 or s[first - 1] < s[first]
        assert last == n - 1 or s[last + 1] > s[last]
        if n >= (1023 if cls == "u8" else 7):
            assert last > first, (cls, n)                                           # a real run
            assert any(k > 0 and s[k - 1] == s[k] for k in ks) and any(k < n - 1 and s[k + 1] == s[k] for k in ks)
    for cls_plain in ("signed", "zeros", "extreme", "sigmoid"):
        for n in R.SIZES:
            assert set(R.ranks(cls_plain, n)) == {min(max(k, 0), n - 1) for k in (0, 1, n // 3, n // 2, n - 2, n - 1)}


@pytest.mark.parametrize("cls", ["signed", "u8", "sigmoid"])
def test_percentile_host_arithmetic_equals_numpy(cls):
    """``prepost.percentile`` is two order statistics and NumPy's float32 interpolation repeated on the host: fed the order statistics of
    ``np.partition`` it must return ``float(np.percentile(x, q))``, every size x every q."""
    P = _P()
    for n in R.SIZES:
        x = R.sample(cls, n)
        for q in R.QS:
            seen = []

            def kth(ks):
                seen.extend(ks)
                return [float(np.partition(x, k)[k]) for k in ks]

            assert P._percentile_of(n, q, kth) == R.percentile_ref(cls, n, q), (cls, n, q)
            assert len(seen) == 2 and 0 <= seen[0] <= seen[1] <= n - 1 and seen[1] - seen[0] <= 1


def test_percentile_host_arithmetic_above_float32_integer_exactness():
    """n = 2^24 + 4099: ``(n - 1) * q / 100`` is formed in float32, as NumPy forms it, where float32 no longer holds every integer (n itself
    is none) and the virtual index is a multiple of 1 or 2 at best."""
    P, stats = _P(), R.large_order_stats()
    assert int(np.float32(R.LARGE)) != R.LARGE
    for q in R.QS:
        assert P._percentile_of(R.LARGE, q, lambda ks: [stats[k] for k in ks]) == R.percentile_ref("signed", R.LARGE, q), q


@pytest.mark.parametrize("nbins", R.NBINS)
def test_histogram_inputs_sit_on_the_edges(nbins):
    """At least ``nbins`` inputs equal an edge exactly (so a mis-built table cannot hide), their one-ulp neighbours are there too, min / max are
    the sample's, the length is no multiple of 4 - and the edge table of the product is ``np.histogram``'s."""
    P = _P()
    for cls in R.HIST_CLASSES:
        x, mn, mx, edges = R.hist_input(cls, nbins)
        assert x.dtype == np.float32 and x.size % 4 != 0 and x.min() == mn and x.max() == mx and mn < mx
        assert edges.dtype == np.float32 and edges.shape == (nbins + 1,) and edges[0] == mn and edges[-1] == mx
        assert np.all(edges[:-1] < edges[1:])
        assert int(np.isin(x, edges).sum()) >= nbins + 1
        inner = edges[1:-1]
        assert np.isin(np.nextafter(inner, np.float32(-np.inf)), x).all() and np.isin(np.nextafter(inner, np.float32(np.inf)), x).all()
        counts, ref_edges = R.hist_ref(cls, nbins)
        assert ref_edges.dtype == np.float32 and np.array_equal(ref_edges.view(np.int32), edges.view(np.int32))
        assert counts.sum() == x.size and counts.shape == (nbins,)
        mine = P._bin_edges(float(mn), float(mx), nbins)
        assert mine.dtype == np.float32 and np.array_equal(mine.view(np.int32), ref_edges.view(np.int32))
    one = P._bin_edges(0.37, 0.37, nbins)                                          # an empty range is widened by +-0.5, as NumPy does
    assert np.array_equal(one, np.histogram(np.full(3, 0.37, np.float32), bins=nbins)[1])


@pytest.mark.parametrize("case", R.refused_inputs(), ids=lambda c: c[0])
def test_histogram_refusals_are_numpys(case):
    name, x, nbins = case
    with pytest.raises(ValueError):
        np.histogram(x, bins=nbins, range=(x.min(), x.max()))
    with pytest.raises(ValueError, match="not finite" if name != "narrow" else "Too many bins"):
        _P()._bin_edges(float(x.min()), float(x.max()), nbins)
    if name == "narrow":                                                            # two adjacent floats: one bin is all they can carry
        assert len(np.unique(x)) == 2 and len(_P()._bin_edges(float(x.min()), float(x.max()), 1)) == 2
        with pytest.raises(ValueError, match="Too many bins"):
            _P()._bin_edges(float(x.min()), float(x.max()), 2)


def test_class_argmax_inputs_hold_tied_maxima():
    for vox in R.ARGMAX_VOXELS:
        for C, k in R.ARGMAX_CK:
            a = R.argmax_input(vox, C)
            assert a.shape == (vox, C) and a.dtype == np.float32 and set(np.unique(a).tolist()) <= set(R.ARGMAX_VALUES.tolist())
            ref = R.argmax_ref(a, k)
            assert ref.shape == (vox, C - k + 1) and ref.dtype == np.float32
            if k >= 2 and vox >= 1025:
                assert R.tied_share(a, k) >= 1 / 3, (vox, C, k)
                cls = a[:, C - k:]
                later = (cls == cls.max(axis=1, keepdims=True))[:, ::-1].argmax(axis=1)        # distance of the LAST maximum from the end
                assert ((k - 1 - later) != ref[:, -1]).mean() >= 1 / 3                          # "last maximum wins" would differ there
            if k == 1:
                assert not ref[:, -1].any()


def test_binary_like_inputs_are_on_both_sides_of_the_reference_test():
    from oracle import prepost_oracle as PO

    flags = []
    for name, a, flag in R.binary_like():
        assert a.ndim == 2 and a.dtype == np.float32 and PO.is_binary_channel(a) == flag, name
        flags.append(flag)
    assert any(flags) and not all(flags)


def test_select_and_threshold_take_any_float_pointer():
    """Nothing is launched: the refusals that remain are a pointer that is no float pointer and a workspace that is not 8-byte aligned."""
    from biapy_amd import _lib as L

    lib = L.lib
    assert lib.bpx_select_kth_f32(A + 2, 10, 3, A, A, None) != 0 and b"4-byte aligned" in lib.bpx_last_error()
    assert lib.bpx_select_kth_f32(A + 4, 10, 3, A, A + 4, None) != 0 and b"8-byte aligned" in lib.bpx_last_error()
    assert lib.bpx_select_kth_f32(A + 4, 10, 10, A, A, None) != 0 and b"rank" in lib.bpx_last_error()
    assert lib.bpx_threshold_u8(None, 10, 0.5, A, None) != 0 and b"bad arguments" in lib.bpx_last_error()

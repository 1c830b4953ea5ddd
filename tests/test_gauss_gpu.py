"""Separable / Gaussian filter on the MI355X (biapy_amd/prepost.py: separable_filter, gaussian_filter, gaussian_laplace; csrc/sepfilter.hip)
against the NumPy twin of its stated float32 arithmetic (tests/gauss_ref.py, itself held within a derived bound of SciPy's float64 result by
test_gauss_cpu.py).  Every comparison with the twin is bit for bit through the integer view - signed zeros, denormals and infinities count;
where the twin holds a NaN (inf - inf under derivative weights) the device holds a NaN.  The shapes are the smallest at which the kernels can
go wrong (two and three tiles along x, ragged ends on every axis, axes of one voxel and axes shorter than the halo); inputs are built once
per process."""
import os

import numpy as np
import pytest
import torch

import gauss_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _P():
    from biapy_amd import prepost

    return prepost


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                                  # a copy: the shared inputs are read-only


def _same(got, want, what):
    R.same_bits(got.cpu().numpy(), want, what)


# ---- every shape, value kind, mode and parameter set --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_every_kind_mode_and_parameter_set(shape):
    """sigma 1 on every kind and mode; per-axis sigma (0, 1, 3) and (2, 0, 0); orders 1 and 2; radius= given; truncate=2; sigma 8 (r = 32) on
    the shapes whose axes are shorter than the halo.  The denormal kind holds the device to the twin's gradual underflow."""
    P = _P()
    on_device, n, seen = {}, 0, set()
    for s, kind, mode, cval, kw in R.gaussian_cases():
        if s != shape:
            continue
        x = R.volume(kind, shape)
        if kind not in on_device:
            on_device[kind] = _dev(x)
        d = on_device[kind]
        out = P.gaussian_filter(d, mode=mode, cval=cval, **kw)
        assert out.is_cuda and out.dtype == torch.float32 and out.shape == d.shape and out.data_ptr() != d.data_ptr()
        _same(out, R.gaussian_ref(x, mode=mode, cval=cval, **kw), (shape, kind, mode, cval, kw))
        n += 1
        seen.add(tuple(sorted(kw)))
    for kind, d in on_device.items():                                                        # the input is left unchanged
        _same(d, R.volume(kind, shape), ("input", kind))
    assert set(on_device) == set(R.KINDS) and n == (63 if shape in R.SHORT_SHAPES else 53) and len(seen) == 4


def test_denormal_results_are_not_flushed():
    P = _P()
    x = R.volume("denormal", (5, 9, 70))
    want = R.gaussian_ref(x, 1.0)
    tiny = np.abs(want) < np.float32(1.1754944e-38)
    assert tiny.all() and (want != 0).mean() > 0.99                                          # every result is a denormal, almost none is zero
    _same(P.gaussian_filter(_dev(x), 1.0), want, "denormals")


def test_separable_filter_pins_the_tap_direction_and_the_axis_order():
    P = _P()
    w = [1.0, 2.0, 4.0, 8.0, 16.0]                                                           # asymmetric: out[i] = sum_j w[j] x[i + j - r]
    for shape in ((5, 9, 70), (3, 6, 131), (8, 16, 128)):
        x = R.volume("normal", shape)
        d = _dev(x)
        for axis in range(3):
            weights = [w if a == axis else None for a in range(3)]
            for mode, cval in (("reflect", 0.0), ("constant", 0.25)):
                _same(P.separable_filter(d, weights, mode, cval), R.separable_ref(x, weights, mode, cval), (shape, axis, mode))
        imp = R.volume("impulse", shape)
        c = np.unravel_index(int(np.prod(shape)) // 2, shape)
        for axis in range(3):
            weights = [w if a == axis else None for a in range(3)]
            got = P.separable_filter(_dev(imp), weights, "constant").cpu().numpy()
            line = np.moveaxis(got, axis, 0)[(slice(None),) + tuple(v for a, v in enumerate(c) if a != axis)]
            for j, wj in enumerate(w):                                                       # w[j] lands at c + r - j: the weights reversed
                at = c[axis] + 2 - j
                if 0 <= at < shape[axis]:
                    assert line[at] == wj, (shape, axis, j)
            assert got.sum() == sum(wj for j, wj in enumerate(w) if 0 <= c[axis] + 2 - j < shape[axis])
        # three different kernels: the passes run z, then y, then x, each on the float32 result of the one before
        weights = [[0.3, 0.5, 0.2], [0.1, 0.2, 0.3, 0.25, 0.15], [1.0 / 3, 1.0 / 7, 1.0 / 11]]
        _same(P.separable_filter(d, weights, "mirror"), R.separable_ref(x, weights, "mirror"), (shape, "zyx"))
        swapped = R.separable_ref(R.separable_ref(R.separable_ref(x, [None, None, weights[2]], "mirror"), [None, weights[1], None], "mirror"),
                                  [weights[0], None, None], "mirror")
        assert not np.array_equal(R.bits(swapped), R.bits(R.separable_ref(x, weights, "mirror")))     # the order is visible in the bits
        _same(P.separable_filter(d, [[0.5], None, [2.0]]), R.separable_ref(x, [[0.5], None, [2.0]]), "radius 0")
        _same(d, x, "the input is left unchanged")


def test_all_skipped_call_is_a_copy_of_the_bits():
    P = _P()
    raw = np.array([0x7FC00001, 0xFFC00002, 0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x3F800000, 0x80000003] * 9, np.uint32).view(np.float32)
    for x in (raw.reshape(3, 4, 6), raw.reshape(8, 9), R.volume("denormal", (3, 6, 131))):
        d = _dev(x)
        for out in (P.gaussian_filter(d, 0.0), P.gaussian_filter(d, [0.0] * x.ndim, order=1, mode="constant", cval=3.0), P.separable_filter(d, [None] * x.ndim)):
            assert out.data_ptr() != d.data_ptr() and out.dtype == torch.float32
            np.testing.assert_array_equal(R.bits(out.cpu().numpy()), R.bits(x))             # NaN payloads and all


def test_2d_call_equals_the_one_plane_volume():
    P = _P()
    for kind in ("normal", "infinities", "denormal"):
        x = R.volume(kind, (17, 70))
        d = _dev(x)
        for kw in (dict(sigma=1.0), dict(sigma=(2.0, 0.5), order=(1, 0)), dict(sigma=8.0, mode="mirror"), dict(sigma=1.5, mode="constant", cval=0.25)):
            flat = P.gaussian_filter(d, **kw)
            kw3 = {k: ((0,) + tuple(v) if isinstance(v, tuple) else v) for k, v in kw.items()}
            kw3["sigma"] = (0.0,) + (tuple(kw["sigma"]) if isinstance(kw["sigma"], tuple) else (kw["sigma"],) * 2)
            vol = P.gaussian_filter(d[None], **kw3)
            _same(flat, R.gaussian_ref(x, **kw), (kind, kw))
            _same(vol[0], R.gaussian_ref(x, **kw), (kind, kw, "as a volume"))


# ---- addresses and views ----------------------------------------------------------------------------------------------------------------------------------

def test_non_contiguous_view_and_a_view_4_bytes_past_alignment():
    P = _P()
    rng = np.random.default_rng(23)
    stack = rng.standard_normal((2, 5, 9, 72)).astype(np.float32)
    d = _dev(stack)
    t = d[0].permute(2, 0, 1)                                                                 # (72, 5, 9), strides that are not a volume's
    assert not t.is_contiguous()
    _same(P.gaussian_filter(t, 1.0), R.gaussian_ref(np.ascontiguousarray(stack[0].transpose(2, 0, 1)), 1.0), "non-contiguous")
    _same(P.gaussian_filter(d[0, :, ::2, 3:], (1.0, 0.0, 2.0)), R.gaussian_ref(np.ascontiguousarray(stack[0, :, ::2, 3:]), (1.0, 0.0, 2.0)), "strided")
    for shape in ((5, 9, 72), (3, 6, 131), (8, 16, 128)):                                     # rows of a multiple of 4 elements and not
        x = R.volume("normal", shape)
        n = x.size
        pad = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
        assert pad.data_ptr() % 16 == 0
        pad[1:1 + n] = _dev(x).flatten()
        view = pad.flatten()[1:1 + n].view(shape)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        for kw in (dict(sigma=1.0), dict(sigma=(0.0, 0.0, 2.0)), dict(sigma=(0.0, 1.0, 0.0), mode="nearest"), dict(sigma=8.0, mode="mirror")):
            out = P.gaussian_filter(view, **kw)
            _same(out, R.gaussian_ref(x, **kw), (shape, kw, "4 bytes past alignment"))
            assert torch.equal(out.view(torch.int32), P.gaussian_filter(view.clone(), **kw).view(torch.int32))    # an aligned copy: the same bits
        assert float(pad[0]) == 0.0 and float(pad[1 + n:].abs().sum()) == 0.0
    assert torch.equal(d.cpu(), torch.from_numpy(stack))                                     # the input is left unchanged


def test_two_calls_give_the_same_bits():
    P = _P()
    for x, kw in ((R.volume("normal", (3, 6, 131)), dict(sigma=2.0)), (R.volume("infinities", (5, 9, 70)), dict(sigma=1.5, order=2)),
                  (R.volume("denormal", (8, 16, 128)), dict(sigma=8.0))):
        d = _dev(x)
        first = P.gaussian_filter(d, **kw)
        for _ in range(3):
            assert torch.equal(first.view(torch.int32), P.gaussian_filter(d, **kw).view(torch.int32))


# ---- the Laplacian of Gaussian -------------------------------------------------------------------------------------------------------------------------------

def test_gaussian_laplace_against_its_twin():
    P = _P()
    for shape in ((5, 9, 70), (17, 70), (8, 16, 128), (2, 3, 1)):
        for kind in ("normal", "impulse"):
            x = R.volume(kind, shape)
            d = _dev(x)
            for sigma, mode, cval in ((1.0, "reflect", 0.0), (2.0, "constant", 0.25), (1.5, "mirror", 0.0)):
                _same(P.gaussian_laplace(d, sigma, mode, cval), R.laplace_ref(x, sigma, mode, cval), (shape, kind, sigma, mode))
            _same(P.gaussian_laplace(d, 3.0, truncate=2.0), R.laplace_ref(x, 3.0, truncate=2.0), (shape, kind, "truncate"))
            _same(d, x, "the input is left unchanged")


# ---- against SciPy's float64 result -------------------------------------------------------------------------------------------------------------------------

def test_64_cubed_against_scipy_within_the_bound():
    """Device against scipy.ndimage.gaussian_filter of the float64 image, per element within the bound of tests/gauss_ref.py; the largest
    err / bound of every case goes to profiles/gauss_values.txt."""
    import scipy.ndimage as ndi

    P = _P()
    x = R.blobs((64, 64, 64))
    d = _dev(x)
    lines = ["# device gaussian_filter vs scipy.ndimage.gaussian_filter (float64) on a 64^3 probability map: largest |err| / bound (tests/gauss_ref.py)"]
    for kw in (dict(sigma=2.0), dict(sigma=8.0, mode="mirror"), dict(sigma=(1.0, 2.0, 3.0), order=(0, 1, 2), mode="constant", cval=0.25), dict(sigma=1.0, mode="nearest")):
        mode, cval = kw.get("mode", "reflect"), kw.get("cval", 0.0)
        ws = R.gaussian_axes(3, kw["sigma"], kw.get("order", 0))
        ref, bound = R.reference_and_bound(x, ws, mode, cval)
        np.testing.assert_array_equal(ref, ndi.gaussian_filter(x.astype(np.float64), **kw))
        got = P.gaussian_filter(d, **kw).cpu().numpy()
        err = np.abs(got.astype(np.float64) - ref)
        ratio = float(np.max(err / bound))
        print(f"{kw}: largest err / bound {ratio:.4f}, largest err {err.max():.3e}")
        lines.append(f"{kw}: max err/bound {ratio:.4f}  max err {err.max():.3e}  max |ref| {np.abs(ref).max():.3e}")
        assert (err <= bound).all() and ratio > 0, kw
        _same(torch.from_numpy(got), R.gaussian_ref(x, **kw), kw)
    try:
        with open(os.path.join(ROOT, "profiles", "gauss_values.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass                                                                                  # a read-only checkout: the figures were printed


# ---- runtime behaviour ----------------------------------------------------------------------------------------------------------------------------------------

def _two_points(shape, seed):
    rng = np.random.default_rng(seed)
    a = np.zeros(shape, np.float32)
    pts = [tuple(int(rng.integers(6, s // 2 - 6)) for s in shape), tuple(int(rng.integers(s // 2 + 6, s - 6)) for s in shape)]
    for p in pts:
        a[p] = 1.0
    return a, sorted(pts)


def test_capture_in_a_graph_and_replay_on_new_contents():
    P = _P()
    import scipy.ndimage as ndi

    shape = (32, 40, 72)
    (a, _), (b, _) = _two_points(shape, 1), _two_points(shape, 2)
    a, b = a + R.blobs(shape, 8) * np.float32(0.01), b + R.blobs(shape, 9) * np.float32(0.01)
    buf = _dev(a)
    P.label(P.peak_mask(P.gaussian_filter(buf, 2.0), 3, 0.004), return_num=True)             # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        smooth = P.gaussian_filter(buf, 2.0)
        peaks = P.peak_mask(smooth, 3, 0.004)
        lab, num = P.label(peaks, return_num=True)
    for img in (b, a, b):
        buf.copy_(torch.from_numpy(np.array(img)))
        g.replay()
        torch.cuda.synchronize()
        want = R.gaussian_ref(img, 2.0)
        _same(smooth, want, "replayed")
        want_peaks = P.peak_mask(_dev(want), 3, 0.004)
        assert torch.equal(peaks, want_peaks) and int(peaks.sum()) >= 2
        wl, wn = ndi.label(want_peaks.cpu().numpy(), ndi.generate_binary_structure(3, 3))
        assert int(num) == wn
        np.testing.assert_array_equal(lab.cpu().numpy(), wl)


def test_pipeline_median_gaussian_peaks_finds_both_points():
    P = _P()
    shape = (32, 40, 72)
    pts_img, pts = _two_points(shape, 4)
    import scipy.ndimage as ndi

    blurred = ndi.gaussian_filter(pts_img.astype(np.float64), 2.0).astype(np.float32)        # two blurred points ...
    rng = np.random.default_rng(6)
    salt = rng.random(shape) < 0.01
    noisy = blurred.copy()
    noisy[salt] = 1.0                                                                          # ... under salt noise that would each be a peak
    d = _dev(noisy)
    smooth = P.gaussian_filter(P.median_filter(d, 3), 1.5)
    coords, num = P.peak_local_max(smooth, min_distance=4, threshold_abs=float(blurred.max()) * 0.25)
    found = sorted(tuple(int(v) for v in row) for row in coords[:int(num)].cpu().numpy())
    assert len(found) == 2 and all(max(abs(f - p) for f, p in zip(fp, pp)) <= 1 for fp, pp in zip(found, pts)), (found, pts)
    import median_ref

    _same(smooth, R.gaussian_ref(median_ref.median_ref(noisy, 3), 1.5), "the pipeline's smoothing")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals_on_device_tensors():
    P = _P()
    x = _dev(R.volume("normal", (5, 9, 70)))
    with pytest.raises(NotImplementedError, match="works on float32"):
        P.gaussian_filter(x.double(), 1.0)
    with pytest.raises(ValueError, match="2-D .* or 3-D"):
        P.gaussian_filter(x[None], 1.0)
    with pytest.raises(NotImplementedError, match="empty axis"):
        P.gaussian_filter(x[:, :0], 1.0)
    with pytest.raises(ValueError, match="sigma must"):
        P.gaussian_filter(x, (1.0, 1.0))
    with pytest.raises(NotImplementedError, match="at most 32"):
        P.gaussian_filter(x, 8.2)
    with pytest.raises(NotImplementedError, match="is not offered"):
        P.gaussian_laplace(x, 1.0, "wrap")
    with pytest.raises(ValueError, match="cval must be finite"):
        P.separable_filter(x, [None, None, [1.0]], "constant", float("inf"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.gaussian_filter(x.cpu(), 1.0)
    from biapy_amd import _lib as L                                                           # the C entry refuses in-place filtering on real pointers too
    w = np.ones(3, np.float32)
    assert L.lib.bpx_sepfilter(x.data_ptr(), 5, 9, 70, None, -1, None, -1, w.ctypes.data, 1, 0, 0.0, x.data_ptr(), None, 0, L.stream_ptr()) != 0
    assert "out_d must not be in_d" in L.lib.bpx_last_error().decode()
    _same(x, R.volume("normal", (5, 9, 70)), "nothing was launched")

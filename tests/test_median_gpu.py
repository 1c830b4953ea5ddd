"""Median filter on the MI355X (biapy_amd/prepost.py: median_filter, median_filter_axes; csrc/median.hip) against the NumPy twin of its
definition (tests/median_ref.py, itself held against scipy.ndimage.median_filter by test_median_cpu.py).  Every comparison is bit for bit -
float32 through its integer view, so signed zeros and NaN payloads count: the filter selects, it does not compute.  The shapes are the
smallest at which the kernel can go wrong (two and three tiles along x, ragged last tiles on every axis, axes of one voxel and axes shorter
than the halo); inputs are built once per process."""
import numpy as np
import pytest
import torch

import median_ref as R

pytestmark = pytest.mark.gpu


def _P():
    from biapy_amd import prepost

    return prepost


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                                  # a copy: the shared inputs are read-only


def _same_bits(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_array_equal(R.bits(got), R.bits(want), err_msg=str(what))


# ---- every shape, dtype, value kind, size and mode --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", (np.float32, np.uint8), ids=("float32", "uint8"))
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_every_size_mode_and_value_kind(shape, dtype):
    P = _P()
    on_device, n = {}, 0
    for x, kind, size, mode, cval in R.cases(shape, dtype):
        if kind not in on_device:
            on_device[kind] = _dev(x)
        d = on_device[kind]
        given = R.per_axis(size, x.ndim) if isinstance(size, tuple) else size                 # a (1, sy, sx) triple is (sy, sx) on a 2-D input
        out = P.median_filter(d, given, mode, cval)
        assert out.is_cuda and out.dtype == d.dtype and out.data_ptr() != d.data_ptr()
        _same_bits(out, R.median_ref(x, size, mode, cval), (kind, shape, size, mode, cval))
        n += 1
    for kind, d in on_device.items():                                                        # the input is left alone
        _same_bits(d, R.f32_input(kind, shape) if dtype == np.float32 else R.u8_input(kind, shape), ("input", kind))
    f32 = dtype == np.float32
    sizes = sum(R.per_axis(s, len(shape)) is not None for s in R.SIZES)
    assert set(on_device) == set(R.F32_KINDS if f32 else R.U8_KINDS) and n == len(on_device) * sizes * len(R.F32_MODES if f32 else R.U8_MODES)


def test_window_of_one_voxel_is_a_copy():
    P = _P()
    for x in (R.f32_input("nans", (5, 9, 70)), R.u8_input("full_range", (3, 6, 131)), R.f32_input("denormals", (17, 70))):
        d = _dev(x)
        for mode, cval in (("reflect", 0), ("constant", 1)):
            out = P.median_filter(d, 1, mode, cval)
            assert out.data_ptr() != d.data_ptr()
            _same_bits(out, x, "copy")
            _same_bits(P.median_filter(d, (1,) * x.ndim, mode, cval), x, "copy")


def test_2d_call_equals_the_one_plane_volume():
    P = _P()
    for x in (R.f32_input("tie_free", (17, 70)), R.f32_input("quantised", (17, 70)), R.f32_input("nans", (17, 70)), R.u8_input("full_range", (17, 70))):
        d = _dev(x)
        for size in ((3, 3), (5, 5), (1, 7), (7, 7), (1, 15), (11, 11), (3, 7)):
            for mode, cval in (("reflect", 0), ("nearest", 0), ("constant", 1)):
                flat, vol = P.median_filter(d, size, mode, cval), P.median_filter(d[None], (1,) + size, mode, cval)
                assert torch.equal(flat.view(torch.uint8), vol[0].view(torch.uint8)), (size, mode)
                _same_bits(flat, R.median_ref(x, size, mode, cval), (size, mode))


def test_bool_masks_come_back_as_bool():
    P = _P()
    for shape in ((5, 9, 70), (17, 70), (2, 3, 1)):
        for kind in ("binary_0.1", "binary_0.5", "binary_0.9"):
            x = R.u8_input(kind, shape).astype(bool)
            d = _dev(x)
            for size in (3, 5):
                for mode, cval in (("reflect", 0), ("constant", 1), ("constant", 0)):
                    out = P.median_filter(d, size, mode, cval)
                    assert out.dtype == torch.bool and out.is_cuda
                    want = R.median_ref(x, size, mode, cval)
                    np.testing.assert_array_equal(out.cpu().numpy(), want)
                    # the majority vote, counted: more than half of the window's voxels are set
                    half = size // 2
                    padded = np.pad(x, half, mode="symmetric") if mode == "reflect" else np.pad(x, half, mode="constant", constant_values=bool(cval))
                    votes = np.lib.stride_tricks.sliding_window_view(padded, (size,) * x.ndim).reshape(x.shape + (-1,)).sum(-1)
                    np.testing.assert_array_equal(want, votes > size ** x.ndim // 2)


# ---- addresses and views ----------------------------------------------------------------------------------------------------------------------------------

def test_unaligned_view_of_a_batch_and_a_non_contiguous_view():
    P = _P()
    rng = np.random.default_rng(17)
    for dtype in (np.float32, np.uint8):
        stack = np.floor(rng.random((2, 5, 9, 71)) * 50).astype(dtype)                        # an odd element count per item
        d = _dev(stack)
        view = d[1]
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        for size, mode in ((3, "reflect"), ((1, 5, 5), "nearest"), ((3, 1, 5), "constant")):
            out = P.median_filter(view, size, mode, 1)
            _same_bits(out, R.median_ref(stack[1], size, mode, 1), (dtype, size, mode))
            assert torch.equal(out, P.median_filter(view.clone(), size, mode, 1))            # an aligned copy: the same bits
        t = d[0].permute(2, 0, 1)                                                             # (71, 5, 9), strides that are not a volume's
        assert not t.is_contiguous()
        _same_bits(P.median_filter(t, (3, 3, 5)), R.median_ref(np.ascontiguousarray(stack[0].transpose(2, 0, 1)), (3, 3, 5)), "non-contiguous")
        _same_bits(P.median_filter(d[0, :, ::2, 3:]), R.median_ref(np.ascontiguousarray(stack[0, :, ::2, 3:])), "strided")
        assert torch.equal(d.cpu(), torch.from_numpy(stack))                                 # the input is left alone


def test_two_calls_give_the_same_bits():
    P = _P()
    for x, size in ((R.f32_input("quantised", (3, 6, 131)), (3, 3, 3)), (R.f32_input("nans", (5, 9, 70)), 5), (R.u8_input("binary_0.5", (5, 9, 70)), (1, 7, 7))):
        d = _dev(x)
        first = P.median_filter(d, size)
        for _ in range(3):
            assert torch.equal(first.view(torch.uint8), P.median_filter(d, size).view(torch.uint8))


# ---- the reference's call shape -------------------------------------------------------------------------------------------------------------------------------

def test_median_filter_axes():
    P = _P()
    x = R.f32_input("quantised", (5, 9, 70))
    d = _dev(x)
    for axes, size in (("xy", 5), ("yx", 3), ("z", 3), ("z", 5), ("zx", 3), ("yz", 3), ("x", 7), ("y", 5), ("xyz", 3), ("xyz", 5)):
        _same_bits(P.median_filter_axes(d, axes, size), R.median_axes_ref(x, axes, size), (axes, size))
    assert torch.equal(P.median_filter_axes(d, "xy", 5), P.median_filter(d, (1, 5, 5)))
    for axes, size in ((["xy", "z"], [5, 3]), (["z", "xy", "zx"], [3, 3, 5]), (["xy"], [7])):
        got = P.median_filter_axes(d, axes, size)
        _same_bits(got, R.median_axes_ref(x, axes, size), (axes, size))
    assert torch.equal(P.median_filter_axes(d, ["xy", "z"], [5, 3]), P.median_filter(P.median_filter(d, (1, 5, 5)), (3, 1, 1)))
    m = _dev(R.u8_input("binary_0.5", (5, 9, 70)))
    _same_bits(P.median_filter_axes(m, "xy", 3), R.median_axes_ref(R.u8_input("binary_0.5", (5, 9, 70)), "xy", 3), "uint8")
    _same_bits(d, x, "the input is left alone")


# ---- runtime behaviour ----------------------------------------------------------------------------------------------------------------------------------------

def test_capture_in_a_graph_and_replay_on_new_contents():
    P = _P()
    import scipy.ndimage as ndi

    a, b = R.probability((6, 20, 70), 3), R.probability((6, 20, 70), 4)
    buf = _dev(a)
    P.label(P.binarize(P.median_filter(buf, (1, 5, 5)), 0.5), return_num=True)              # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        smooth = P.median_filter(buf, (1, 5, 5))
        lab, num = P.label(P.binarize(smooth, 0.5), return_num=True)
    for img in (b, a, b):
        buf.copy_(torch.from_numpy(np.array(img)))
        g.replay()
        torch.cuda.synchronize()
        want = R.median_ref(img, (1, 5, 5))
        _same_bits(smooth, want, "replayed")
        wl, wn = ndi.label(want > 0.5, ndi.generate_binary_structure(3, 3))
        assert int(num) == wn > 0
        np.testing.assert_array_equal(lab.cpu().numpy(), wl)


# ---- against SciPy directly -------------------------------------------------------------------------------------------------------------------------------------

def test_64_cubed_against_scipy():
    P = _P()
    x = R.probability((64, 64, 64))
    d = _dev(x)
    for size, mode in (((1, 5, 5), "reflect"), ((3, 3, 3), "nearest")):
        np.testing.assert_array_equal(P.median_filter(d, size, mode).cpu().numpy(), R.scipy_median(x, size, mode, 0.0))
    m = (x > 0.5).astype(np.uint8)
    np.testing.assert_array_equal(P.median_filter(_dev(m), 3).cpu().numpy(), R.scipy_median(m, 3, "reflect", 0))


def test_pipeline_median_binarize_label_region_props():
    P = _P()
    import scipy.ndimage as ndi

    prob = R.probability((12, 40, 44))
    raw_n = ndi.label(prob > 0.5, ndi.generate_binary_structure(3, 3))[1]
    smooth = P.median_filter(_dev(prob), (1, 5, 5))
    lab, num = P.label(P.binarize(smooth, 0.5), return_num=True)
    props = P.region_props(lab, num)
    want_smooth = R.scipy_median(prob, (1, 5, 5), "reflect", 0.0)
    wl, wn = ndi.label(want_smooth > 0.5, ndi.generate_binary_structure(3, 3))
    assert int(num) == wn and 0 < wn < raw_n                                                  # the filter removed the salt's speckle
    np.testing.assert_array_equal(lab.cpu().numpy(), wl)
    np.testing.assert_array_equal(props.area.cpu().numpy()[1:], np.bincount(wl.ravel())[1:])
    boxes = ndi.find_objects(wl)
    np.testing.assert_array_equal(props.bbox.cpu().numpy()[1:], np.array([[s.start for s in b] + [s.stop for s in b] for b in boxes]))
    com = np.array(ndi.center_of_mass(wl > 0, wl, range(1, wn + 1)))
    np.testing.assert_allclose(props.centroid.cpu().numpy()[1:], com, rtol=0, atol=1e-9)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals_on_device_tensors():
    P = _P()
    x = _dev(R.f32_input("tie_free", (5, 9, 70)))
    with pytest.raises(NotImplementedError, match="works on"):
        P.median_filter(x.to(torch.int32))
    with pytest.raises(NotImplementedError, match="works on"):
        P.median_filter(x.double())
    with pytest.raises(ValueError, match="2-D .* or 3-D"):
        P.median_filter(x[None])
    with pytest.raises(NotImplementedError, match="empty axis"):
        P.median_filter(x[:, :0])
    for size in (2, (3, 3, 4)):
        with pytest.raises(NotImplementedError, match="size must be odd"):
            P.median_filter(x, size)
    with pytest.raises(NotImplementedError, match="at most 15"):
        P.median_filter(x, (1, 1, 17))
    with pytest.raises(NotImplementedError, match="at most 125"):
        P.median_filter(x, 7)
    with pytest.raises(ValueError, match="size must be"):
        P.median_filter(x, (3, 3))
    for mode in ("mirror", "wrap"):
        with pytest.raises(NotImplementedError, match="is not offered"):
            P.median_filter(x, 3, mode)
    with pytest.raises(ValueError, match="mode must be"):
        P.median_filter(x, 3, "periodic")
    with pytest.raises(ValueError, match="cval must be finite"):
        P.median_filter(x, 3, "constant", float("inf"))
    with pytest.raises(ValueError, match="integer in 0..255"):
        P.median_filter((x > 0).to(torch.uint8), 3, "constant", 0.25)
    with pytest.raises(ValueError, match="axes must be one of"):
        P.median_filter_axes(x, "xw", 3)
    with pytest.raises(NotImplementedError, match="size must be odd"):
        P.median_filter_axes(x, ["xy", "z"], [3, 2])
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.median_filter(x.cpu())
    from biapy_amd import _lib as L                                                           # the C entry refuses in place filtering on real pointers too
    assert L.lib.bpx_median_filter(x.data_ptr(), L.F32, 5, 9, 70, 3, 3, 3, 0, 0.0, x.data_ptr(), L.stream_ptr()) != 0
    assert "out_d must not be in_d" in L.lib.bpx_last_error().decode()
    _same_bits(x, R.f32_input("tie_free", (5, 9, 70)), "nothing was launched")

"""Intensity properties on the device against the big-integer twin (tests/intensityprops_ref.py): every field bit for bit - the limbs, the sum
rounded once, min / max with the bits of the winning voxel, the non-finite counters - and ``mean`` within 1 float64 ulp of the twin's division
(0 expected).  The worst ulp distance seen goes to profiles/intensityprops_values.txt."""
import os

import numpy as np
import pytest
import torch

import intensityprops_ref as R
import regionprops_ref as RP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = os.path.join(ROOT, "profiles", "intensityprops_values.txt")
_ulps = {}


def _P():
    from biapy_amd import prepost

    return prepost


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                                  # a copy: the shared inputs are read-only


def _check(p, want, what):
    """The device's IntensityProps == the twin: types, shapes, every field but mean as bits, mean within 1 ulp; absent rows hold zeros."""
    n = want["area"].shape[0]
    assert type(p).__name__ == "IntensityProps" and p._fields == R.FIELDS
    got = {f: getattr(p, f).cpu().numpy() for f in R.FIELDS}
    assert all(getattr(p, f).is_cuda and getattr(p, f).shape[0] == n for f in R.FIELDS), what
    for f in ("area", "min", "max", "sum", "sum_limbs", "nonfinite"):
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f, got[f].dtype, got[f].shape)
        if not R.same_bits(got[f], want[f]):
            bad = np.flatnonzero((got[f].reshape(n, -1).view(np.uint8) != want[f].reshape(n, -1).view(np.uint8)).any(1))
            raise AssertionError(f"{what}: {f} differs in rows {bad[:8]}: got {got[f][bad[:4]]}, want {want[f][bad[:4]]}")
    assert got["mean"].dtype == np.float64 and got["mean"].shape == (n,), what
    d = R.ulp_distance(got["mean"], want["mean"])
    _ulps[what] = max(_ulps.get(what, 0), d)
    assert d <= 1, (what, d)
    absent = want["area"] == 0
    assert absent[0] and np.isnan(got["mean"][absent]).all(), what
    for f in ("area", "min", "max", "sum", "sum_limbs", "nonfinite"):
        assert not got[f][absent].view(np.uint8).any(), f"{what}: {f} of an absent label"


def _run_case(name, num="int"):
    labels, image, n_max = R.cases()[name]
    given = n_max if num == "int" else torch.tensor(n_max, dtype=torch.int32, device="cuda")
    p = _P().intensity_props(_dev(labels), _dev(image), given)
    _check(p, R.ref(name), name)
    return p


@pytest.mark.parametrize("name", list(R.cases()), ids=str)
def test_every_shared_case_bit_for_bit(name):
    _run_case(name)


def test_the_worst_mean_distance_is_recorded():
    """After the cases above (file order): 0 ulp expected, 1 allowed."""
    for name in ("uniform (16, 32, 64) L40", "exponents (16, 32, 64) L40", "u16 (16, 32, 64) L40"):
        _run_case(name)
    worst = max(_ulps.values())
    try:
        with open(VALUES, "w") as f:
            f.write("prepost.intensity_props against tests/intensityprops_ref.py on the device: every field but mean equal as bits;\n")
            f.write(f"mean: largest distance {worst} float64 ulp over {len(_ulps)} comparisons (bound 1)\n")
            for k in sorted(_ulps):
                f.write(f"{_ulps[k]:3d}  {k}\n")
    except OSError:
        pass
    assert worst <= 1


def test_2d_input_equals_its_3d_form():
    P = _P()
    labels, image, n_max = R.cases()[R.named("(37, 41) L7")]
    two, three = P.intensity_props(_dev(labels), _dev(image), n_max), P.intensity_props(_dev(labels[None]), _dev(image[None]), n_max)
    _check(two, R.intensity_props_ref(labels, image, n_max), "2-D (37, 41)")
    for a, b in zip(two, three):
        assert R.same_bits(a.cpu().numpy(), b.cpu().numpy())


def test_num_as_int_tensor_and_none():
    P = _P()
    name = "exponents (16, 32, 64) L40"
    labels, image, n_max = R.cases()[name]
    _run_case(name, "tensor")
    top = int(labels.max())
    _check(P.intensity_props(_dev(labels), _dev(image)), R.intensity_props_ref(labels, image, top), name + ", num=None")
    _check(P.intensity_props(_dev(labels), _dev(image), n_max + 30), R.intensity_props_ref(labels, image, n_max + 30), name + ", an upper bound")
    _check(P.intensity_props(_dev(labels), _dev(image), 0), R.intensity_props_ref(labels, image, 0), name + ", num=0")
    zeros = np.zeros_like(labels)
    _check(P.intensity_props(_dev(zeros), _dev(image)), R.intensity_props_ref(zeros, image, 0), "all background, num=None")


def _views(a, off):
    """`a` on the device `off` elements past a 16-byte boundary; as a transposed view; as every second plane of a taller tensor.  Built on the
    host and uploaded, so that no device operation but the call's own .contiguous() touches them."""
    n = a.size
    flat = np.zeros(n + 16, a.dtype)
    flat[off:off + n] = a.ravel()
    buf = torch.from_numpy(flat).cuda()
    assert buf.data_ptr() % 16 == 0                                                          # the allocator's blocks are aligned to more than that
    shifted = buf[off:off + n].view(a.shape)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == (off * a.itemsize) % 16
    perm = torch.from_numpy(np.ascontiguousarray(np.swapaxes(a, 0, 1))).cuda().transpose(0, 1)
    tall = np.zeros((2 * a.shape[0],) + a.shape[1:], a.dtype)
    tall[::2] = a
    every_second = torch.from_numpy(tall).cuda()[::2]
    assert not perm.is_contiguous() and not every_second.is_contiguous()
    return shifted, perm, every_second


def test_unaligned_and_non_contiguous_views_of_both_operands():
    P = _P()
    for name in ("boundaries (16, 32, 64) L40", "u8 (16, 32, 64) L40", "u16 (16, 32, 64) L40", R.named("(3, 37, 41) L1000")):
        labels, image, n_max = R.cases()[name]
        lab, img = _dev(labels), _dev(image)
        for off_bytes in (4, 8, 12):
            lviews, iviews = _views(labels, off_bytes // 4), _views(image, off_bytes // image.itemsize)
            assert lviews[0].data_ptr() % 16 == off_bytes and iviews[0].data_ptr() % 16 == off_bytes
            _check(P.intensity_props(lviews[0], img, n_max), R.ref(name), f"{name}: labels at {off_bytes} bytes")
            _check(P.intensity_props(lab, iviews[0], n_max), R.ref(name), f"{name}: image at {off_bytes} bytes")
            _check(P.intensity_props(lviews[0], iviews[0], n_max), R.ref(name), f"{name}: both at {off_bytes} bytes")
        if image.itemsize < 4:                                                               # an odd element offset of the narrow images
            _check(P.intensity_props(lab, _views(image, 1)[0], n_max), R.ref(name), f"{name}: image at {image.itemsize} bytes")
        lviews, iviews = _views(labels, 0), _views(image, 0)
        for k in (1, 2):
            _check(P.intensity_props(lviews[k], img, n_max), R.ref(name), f"{name}: labels as non-contiguous view {k}")
            _check(P.intensity_props(lab, iviews[k], n_max), R.ref(name), f"{name}: image as non-contiguous view {k}")
            _check(P.intensity_props(lviews[k], iviews[3 - k], n_max), R.ref(name), f"{name}: both non-contiguous {k}")


FORM_CASES = ("uniform (16, 32, 64) L40", "exponents (3, 37, 41) one label", "boundaries (3, 37, 41) one label", "nonfinite (3, 37, 41) one label",
              "zeros (3, 37, 41) one label", "cancelling (3, 37, 41) one label", "one label 1 x 1 x 70000", "one label 1 x 1 x 70000 u16",
              "two rows of 8193 one label", "two rows of 257 one label", "FLT_MAX in 2^20 voxels", "FLT_MAX cancelling in 2^21 voxels",
              "uint16 65535 in 2^20 voxels", "4096 voxels each its own label", "the non-finite table")


def test_both_kernel_forms_give_the_same_bits():
    from biapy_amd import _lib as L

    P = _P()
    try:
        for name in FORM_CASES:
            labels, image, n_max = R.cases()[name]
            lab, img = _dev(labels), _dev(image)
            out = []
            for form in (0, 1):
                L.lib.bpx_debug_set_intensityprops_wave(form)
                out.append(P.intensity_props(lab, img, n_max))
                _check(out[-1], R.ref(name), f"{name}, form {'ab'[form]}")
            for a, b in zip(*out):
                assert R.same_bits(a.cpu().numpy(), b.cpu().numpy()), name
    finally:
        L.lib.bpx_debug_set_intensityprops_wave(-1)                                         # negative: the library's default


def test_two_calls_give_the_same_bits():
    P = _P()
    for name in ("exponents (16, 32, 64) L40", "cancelling (16, 32, 64) L40", "4096 voxels each its own label", "one label 1 x 1 x 70000"):
        labels, image, n_max = R.cases()[name]
        lab, img = _dev(labels), _dev(image)
        first, second = P.intensity_props(lab, img, n_max), P.intensity_props(lab, img, n_max)
        for a, b in zip(first, second):
            assert R.same_bits(a.cpu().numpy(), b.cpu().numpy()), name


def test_area_equals_region_props_and_the_other_props_are_unchanged():
    import shapeprops_ref as SR

    P = _P()
    for name in ("exponents (16, 32, 64) L40", "4096 voxels each its own label", "negative labels", "labels above num"):
        labels, image, n_max = R.cases()[name]
        lab = _dev(labels)
        r = P.region_props(lab, n_max)
        ip = P.intensity_props(lab, _dev(image), n_max)
        assert torch.equal(ip.area, r.area) and ip.area.dtype == r.area.dtype, name
        after = P.region_props(lab, n_max)
        want = RP.region_props_ref(labels, n_max)
        for got in (r, after):
            np.testing.assert_array_equal(got.area.cpu().numpy(), want[0])
            np.testing.assert_array_equal(got.coord_sum.cpu().numpy(), want[1])
            np.testing.assert_array_equal(got.bbox.cpu().numpy(), want[2])
        s, sw = P.shape_props(lab, n_max), SR.shape_props_ref(labels, n_max)
        for f in ("area", "bbox", "coord_sum", "moments", "faces"):
            np.testing.assert_array_equal(getattr(s, f).cpu().numpy(), sw[f], err_msg=f"{name}: {f}")
        assert R.same_bits(s.covariance.cpu().numpy(), sw["covariance"])


def _prediction(shape, seed, fill=0.3):
    rng = np.random.default_rng(seed)
    return (0.35 * rng.random(shape) + 0.6 * RP.balls(shape, fill=fill, seed=seed, rmin=2, rmax=5)).astype(np.float32)


def _confidence_filter(P, pred, bound, t):
    lab = P.label(P.binarize(pred, 0.5), connectivity=1)
    ip = P.intensity_props(lab, pred, bound)
    keep = ip.mean >= t
    return lab, ip, keep, P.select_objects(lab, keep, relabel=True, return_num=True)


def test_binarize_label_intensity_props_select_objects_chain():
    P = _P()
    host = _prediction((24, 48, 64), 5)
    pred = _dev(host)
    lab, num = P.label(P.binarize(pred, 0.5), connectivity=1, return_num=True)
    n, hl = int(num), lab.cpu().numpy()
    assert n > 5
    ip = P.intensity_props(lab, pred, n)
    want = R.intensity_props_ref(hl, host, n)
    _check(ip, want, "the chain's instances")
    means = np.sort(want["mean"][1:])
    t = float((means[n // 2 - 1] + means[n // 2]) / 2)                                      # between two objects' means: no tie for the filter to break
    keep = np.nan_to_num(want["mean"], nan=-np.inf) >= t
    assert 0 < keep[1:].sum() < n
    got, left = P.select_objects(lab, ip.mean >= t, return_num=True)
    np.testing.assert_array_equal(got.cpu().numpy(), np.where(keep[hl], hl, 0))
    assert int(left) == int(keep[1:].sum())


def test_graph_capture_of_the_confidence_filter():
    """Captured once with an upper bound for num, replayed after the prediction was overwritten in place (an all-background one among them)."""
    P = _P()
    shape, bound, t = (12, 40, 56), 400, 0.78
    preds = [_prediction(shape, 1), _prediction(shape, 2, 0.15), np.zeros(shape, np.float32), _prediction(shape, 1)]
    pred = _dev(preds[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _confidence_filter(P, pred, bound, t)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lab, ip, keep, (kept, left) = _confidence_filter(P, pred, bound, t)
    for k, host in enumerate(preds):
        pred.copy_(_dev(host))
        g.replay()
        torch.cuda.synchronize()
        elab = P.label(P.binarize(_dev(host), 0.5), connectivity=1)
        assert torch.equal(lab, elab)
        want = R.intensity_props_ref(elab.cpu().numpy(), host, bound)
        _check(ip, want, f"replay {k}")
        ekeep = np.nan_to_num(want["mean"], nan=-np.inf) >= t
        np.testing.assert_array_equal(keep.cpu().numpy(), ekeep)
        ekept, eleft = P.select_objects(elab, _dev(ekeep), relabel=True, return_num=True)
        assert torch.equal(kept, ekept) and int(left) == int(eleft)
        if k == 0:
            assert 0 < int(left) < int(elab.max())
        if not host.any():
            assert not ip.area.any() and not ip.sum_limbs.any() and not kept.any()


def test_refusals_on_device_tensors():
    P = _P()
    a = torch.zeros(4, 5, 6, dtype=torch.int32, device="cuda")
    x = torch.zeros(4, 5, 6, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="2-D .* or 3-D"):
        P.intensity_props(a.view(-1), x.view(-1), 2)
    with pytest.raises(ValueError, match="num must not be negative"):
        P.intensity_props(a, x, -1)
    with pytest.raises(ValueError, match="must have the labels' shape"):
        P.intensity_props(a, x[:3], 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.intensity_props(a, x.cpu(), 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.intensity_props(a.cpu(), x, 2)
    with pytest.raises(NotImplementedError, match="int32 labels"):
        P.intensity_props(a.long(), x, 2)
    for dt in (torch.float64, torch.float16, torch.bfloat16, torch.int32, torch.int16, torch.bool):
        with pytest.raises(NotImplementedError, match="float32, uint8 or uint16 images"):
            P.intensity_props(a, x.to(dt), 2)
    with pytest.raises(NotImplementedError, match="empty"):
        P.intensity_props(a[:0], x[:0], 2)

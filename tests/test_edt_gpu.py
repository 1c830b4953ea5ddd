"""Exact Euclidean distance transform on the MI355X (biapy_amd/prepost.py: distance_transform_edt, label_distance; csrc/edt.hip).  On the unit
grid every comparison is bit for bit: the int32 squared distance against SciPy's (rebuilt from ``return_indices``), the float32 distance
against ``scipy(...).astype(float32)``, label mode against per-label SciPy.  With ``sampling`` the float32 result is held to 1 fp32 ulp of
``float32(scipy float64)``: both sides are fp64 evaluations of a real candidate distance, each within a few 2^-53 of the true minimum, and
rounding to fp32 can split two such values by one ulp at most.  All-foreground inputs give the sentinel (INT32_MAX / +inf) and are not
compared with SciPy, which measures to a fictitious point there.  Inputs and references: tests/edt_ref.py, computed once per process."""
import os

import numpy as np
import pytest
import torch

import edt_ref as E
import label_ref as LR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _P():
    from biapy_amd import prepost

    return prepost


def _dev(a):
    return torch.from_numpy(np.asarray(a)).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _check_binary(mask, sq_want):
    """distance_transform_edt of the mask: the int32 squared result and the float32 result, both bit for bit."""
    P, m = _P(), _dev(mask)
    sq = P.distance_transform_edt(m, squared=True)
    assert sq.dtype == torch.int32 and sq.shape == tuple(mask.shape) and sq.is_cuda and sq.is_contiguous()
    np.testing.assert_array_equal(sq.cpu().numpy(), sq_want)
    d = P.distance_transform_edt(m)
    assert d.dtype == torch.float32 and d.shape == tuple(mask.shape)
    np.testing.assert_array_equal(_bits(d), E.sqrt_f32(sq_want).view(np.int32))
    return d


def _check_labels(lab):
    P, l = _P(), _dev(lab)
    want = E.label_ref_sq(lab)
    sq = P.label_distance(l, squared=True)
    assert sq.dtype == torch.int32 and sq.shape == tuple(lab.shape)
    np.testing.assert_array_equal(sq.cpu().numpy(), want)
    d = P.label_distance(l)
    assert d.dtype == torch.float32
    np.testing.assert_array_equal(_bits(d), E.sqrt_f32(want).view(np.int32))


@pytest.mark.parametrize("shape", E.SHAPES, ids=str)
def test_random_masks_bit_for_bit(shape):
    """Foreground densities 0.5 ... 0.999 (sparse zeros: long distances, deep envelopes) on shapes unaligned everywhere, aligned, with rows
    of several chunks, 2-D in both spellings and with axes of one voxel."""
    for p in E.DENSITIES:
        mask = E.random_masks(shape)[p]
        d = _check_binary(mask, E.scipy_sq(mask))
        np.testing.assert_array_equal(_bits(d), E.scipy_f32(mask).view(np.int32))        # SciPy's own float64 result, rounded


@pytest.mark.parametrize("name", [n for n in E.STRUCTURED if n != "zero"])
def test_structured_masks_bit_for_bit(name):
    """20 x 43 x 150: a single zero at each corner and at the centre, a zero plane on each axis, a diagonal zero plane, the checkerboard, balls."""
    mask = E.structured(name)
    d = _check_binary(mask, E.scipy_sq(mask))
    np.testing.assert_array_equal(_bits(d), E.scipy_f32(mask).view(np.int32))


def test_all_zero_gives_zeros_and_all_one_gives_the_sentinel():
    P = _P()
    zero = _dev(E.structured("zero"))
    for kw in (dict(squared=True), dict(), dict(sampling=(2.0, 1.0, 0.5)), dict(sampling=(2.0, 1.0, 0.5), squared=True)):
        assert not P.distance_transform_edt(zero, **kw).any()
    for shape in (E.BIG, (33, 70), (1, 1, 300), (5, 1, 1)):
        one = torch.ones(shape, dtype=torch.uint8, device="cuda")
        assert (P.distance_transform_edt(one, squared=True) == 2 ** 31 - 1).all()        # not SciPy's fictitious point
        for kw in (dict(), dict(sampling=(1.0,) * len(shape)), dict(sampling=(1.0,) * len(shape), squared=True)):
            out = P.distance_transform_edt(one, **kw)
            assert out.dtype == torch.float32 and torch.isinf(out).all() and (out > 0).all()
        lab = torch.full(shape, 5, dtype=torch.int32, device="cuda")                     # a label filling the whole volume
        assert (P.label_distance(lab, squared=True) == 2 ** 31 - 1).all() and torch.isinf(P.label_distance(lab)).all()


@pytest.mark.parametrize("name", list(E.LONG))
def test_long_axes(name):
    """(1,1,40000), (1,30000,3), (5000,2,3) with a single zero at a corner: chunk carries over 625 chunks, envelopes 30000 deep, squared
    values up to 39999^2 (64-bit intermediates)."""
    mask, sq = E.long_axis(name)
    _check_binary(mask, sq)
    lab = np.where(mask != 0, 2 ** 30 + 3, 7).astype(np.int32)                           # the same geometry as two labels: the lone voxel measures 1
    got = _P().label_distance(_dev(lab), squared=True).cpu().numpy()
    want = sq.copy()
    want[mask == 0] = 1
    np.testing.assert_array_equal(got, want)


def test_refusals_before_any_launch():
    P = _P()
    with pytest.raises(NotImplementedError, match="2\\^31 - 1"):
        P.distance_transform_edt(torch.ones(1, 1, 46341, dtype=torch.uint8, device="cuda"))
    with pytest.raises(NotImplementedError, match="2\\^31 - 1"):
        P.label_distance(torch.ones(46341, 1, dtype=torch.int32, device="cuda"), squared=True)
    ok = P.distance_transform_edt(torch.ones(1, 1, 46341, dtype=torch.uint8, device="cuda"), sampling=(1, 1, 1))   # the fp64 path has no such limit
    assert torch.isinf(ok).all()
    big = torch.empty(2 ** 31, dtype=torch.uint8, device="cuda").view(2048, 1024, 1024)
    with pytest.raises(NotImplementedError, match="2\\^31 voxels"):
        P.distance_transform_edt(big)
    with pytest.raises(NotImplementedError, match="2\\^31 voxels"):
        P.distance_transform_edt(big, sampling=(1, 1, 1))
    del big
    with pytest.raises(NotImplementedError, match="empty axis"):
        P.distance_transform_edt(torch.ones(3, 0, 5, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="2-D .* or 3-D"):
        P.distance_transform_edt(torch.ones(2, 3, 4, 5, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="sampling"):
        P.distance_transform_edt(torch.ones(3, 4, 5, dtype=torch.uint8, device="cuda"), sampling=(1.0, 2.0))
    with pytest.raises(NotImplementedError, match="uint8 or bool"):
        P.distance_transform_edt(torch.ones(3, 4, 5, dtype=torch.int32, device="cuda"))
    with pytest.raises(NotImplementedError, match="int32 labels"):
        P.label_distance(torch.ones(3, 4, 5, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("name", list(E.LABELS))
def test_label_mode_against_per_label_scipy(name):
    """label(balls), touching 4 x 4 x 4 blocks of labels 0..3, one label but for one foreign voxel (a label, or background), ids 2^30 + k."""
    _check_labels(E.labels(name))


def test_label_of_balls_on_the_device_then_its_distance():
    P = _P()
    lab = P.label(_dev(LR.balls(E.BIG)))
    np.testing.assert_array_equal(lab.cpu().numpy(), E.labels("balls"))
    np.testing.assert_array_equal(P.label_distance(lab, squared=True).cpu().numpy(), E.label_ref_sq(E.labels("balls")))


def test_binary_and_label_mode_agree():
    P = _P()
    for mask in (E.random_masks((9, 21, 37))[0.9], E.random_masks((33, 70))[0.99], E.structured("diagonal"), E.structured("balls")):
        m = _dev(mask)
        as_labels = (m != 0).to(torch.int32)
        for kw in (dict(squared=True), dict(), dict(sampling=(1.5,) * mask.ndim)):
            assert torch.equal(P.distance_transform_edt(m, **kw), P.label_distance(as_labels, **kw))


def test_input_forms():
    """Every nonzero byte is the same foreground; bool inputs; non-contiguous views; the 2-D spellings (33,70) and (1,33,70)."""
    P = _P()
    base = E.random_masks((9, 21, 37))[0.9]
    want = E.scipy_sq(base)
    vals = np.random.default_rng(1).choice(np.array([1, 2, 255], np.uint8), size=base.shape)
    for m in (_dev(base * vals), _dev(base.astype(bool))):
        np.testing.assert_array_equal(P.distance_transform_edt(m, squared=True).cpu().numpy(), want)
    perm = _dev(np.ascontiguousarray(base.transpose(1, 0, 2))).permute(1, 0, 2)
    tall = torch.zeros(18, 21, 37, dtype=torch.uint8, device="cuda")
    tall[::2] = _dev(base)
    for view in (perm, tall[::2], tall.bool()[::2]):
        assert not view.is_contiguous()
        out = P.distance_transform_edt(view, squared=True)
        assert out.is_contiguous() and np.array_equal(out.cpu().numpy(), want)
    lab = E.labels("blocks")
    lperm = _dev(np.ascontiguousarray(lab.transpose(2, 1, 0))).permute(2, 1, 0)
    assert not lperm.is_contiguous()
    np.testing.assert_array_equal(P.label_distance(lperm, squared=True).cpu().numpy(), E.label_ref_sq(lab))
    flat = E.random_masks((33, 70))[0.99]
    for kw in (dict(squared=True), dict()):
        a, b = P.distance_transform_edt(_dev(flat), **kw), P.distance_transform_edt(_dev(flat[None]), **kw)
        assert a.shape == (33, 70) and b.shape == (1, 33, 70) and torch.equal(a, b[0])
    a = P.distance_transform_edt(_dev(flat), sampling=E.SAMPLING_2D)
    b = P.distance_transform_edt(_dev(flat[None]), sampling=(9.0,) + E.SAMPLING_2D)
    assert torch.equal(a, b[0])


def _ulps(got, want):
    """Largest distance in fp32 ulps and the number of elements that differ (finite, non-negative floats: the bit patterns are ordered)."""
    g, w = got.view(np.int32).astype(np.int64), want.view(np.int32).astype(np.int64)
    diff = np.abs(g - w)
    return int(diff.max()), int((diff != 0).sum())


def _sampling_cases():
    cases = []
    for s in E.SAMPLINGS:
        for shape in ((9, 21, 37), (17, 16, 200), (20, 43, 150)):
            cases += [(E.random_masks(shape)[p], s, f"random {shape} p={p}") for p in (0.5, 0.99, 0.999)]
        cases += [(E.structured(n), s, n) for n in ("corner000", "centre", "plane_y", "diagonal", "checkerboard", "balls")]
    cases += [(E.random_masks((33, 70))[p], E.SAMPLING_2D, f"random (33, 70) p={p}") for p in E.DENSITIES]
    return cases


def test_sampling_within_one_fp32_ulp_of_scipy():
    """sampling (2, 1, 0.5), (40, 4, 4) and a 2-D pair on the same masks: the float32 distance within 1 fp32 ulp of float32(scipy float64),
    the float32 square within 1 ulp of SciPy's square computed in fp64.  What was seen is appended to profiles/edt_values.txt."""
    P = _P()
    worst = dict(dist=(0, 0), sq=(0, 0))
    voxels = 0
    for mask, s, name in _sampling_cases():
        ref = E.scipy_f64(mask, s)
        d = P.distance_transform_edt(_dev(mask), sampling=s)
        q = P.distance_transform_edt(_dev(mask), sampling=s, squared=True)
        assert d.dtype == torch.float32 and q.dtype == torch.float32
        for key, got, want in (("dist", d, ref.astype(np.float32)), ("sq", q, (ref * ref).astype(np.float32))):
            u, cnt = _ulps(got.cpu().numpy(), want)
            print(f"edt sampling {s} {name} {key}: largest difference {u} ulp, {cnt} of {mask.size} voxels differ")
            worst[key] = (max(worst[key][0], u), worst[key][1] + cnt)
            assert u <= 1, (name, s, key, u)
        voxels += mask.size
    line = (f"tests/test_edt_gpu.py sampling path against float32(scipy float64), {voxels} voxels: distance largest {worst['dist'][0]} ulp, "
            f"{worst['dist'][1]} voxels differ; square largest {worst['sq'][0]} ulp, {worst['sq'][1]} voxels differ")
    print(line)
    try:
        with open(os.path.join(ROOT, "profiles", "edt_values.txt"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass                                                                             # a read-only checkout: the figures are in the output


def test_sampling_in_label_mode_and_the_unit_sampling():
    P = _P()
    lab = E.labels("blocks_big")
    s = E.SAMPLINGS[0]
    u, _ = _ulps(P.label_distance(_dev(lab), sampling=s).cpu().numpy(), E.label_ref_f64(lab, s).astype(np.float32))
    assert u <= 1
    mask = E.structured("balls")                                                         # sampling (1, 1, 1) takes the fp64 path too: float32 either way
    q = P.distance_transform_edt(_dev(mask), sampling=(1, 1, 1), squared=True)
    assert q.dtype == torch.float32 and np.array_equal(q.cpu().numpy(), E.scipy_sq(mask).astype(np.float32))   # integers below 2^24: exact in fp64 and fp32
    np.testing.assert_array_equal(_bits(P.distance_transform_edt(_dev(mask), sampling=(1, 1, 1))), E.scipy_f32(mask).view(np.int32))


def test_two_calls_give_the_same_bits():
    P = _P()
    for mask in (E.random_masks((17, 16, 200))[0.99], E.structured("checkerboard"), E.structured("balls")):
        m = _dev(mask)
        for kw in (dict(squared=True), dict(), dict(sampling=(2.0, 1.0, 0.5))):
            assert torch.equal(P.distance_transform_edt(m, **kw), P.distance_transform_edt(m, **kw))
    l = _dev(E.labels("balls"))
    assert torch.equal(P.label_distance(l), P.label_distance(l))


def test_graph_capture_of_label_and_label_distance():
    """Captured once, replayed after the mask was overwritten in place: labels and distances are the references' for the NEW mask."""
    P = _P()
    shape = (17, 16, 200)
    first, second = LR.random_masks(shape)[3, 0.25], E.random_masks(shape)[0.9]
    m = _dev(first).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        P.label_distance(P.label(m, 3), squared=True)
        P.label_distance(P.label(m, 3), sampling=(2.0, 1.0, 0.5))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lab = P.label(m, 3)
        sq = P.label_distance(lab, squared=True)
        ds = P.label_distance(lab, sampling=(2.0, 1.0, 0.5))
    for mask in (first, second, np.zeros(shape, np.uint8), first):
        m.copy_(_dev(mask))
        g.replay()
        want_lab = np.ascontiguousarray(LR.scipy_label(mask, 3)[0])
        np.testing.assert_array_equal(lab.cpu().numpy(), want_lab)
        ref_sq, ref_d = E._label_ref(want_lab, (2.0, 1.0, 0.5))
        ref_unit = E._label_ref(want_lab, None)[0]
        np.testing.assert_array_equal(sq.cpu().numpy(), ref_unit.astype(np.int32))
        assert _ulps(ds.cpu().numpy(), ref_d.astype(np.float32))[0] <= 1


def test_binarize_label_label_distance_end_to_end():
    P = _P()
    rng = np.random.default_rng(3)
    blobs = LR.balls((12, 40, 72), fill=0.15, rmin=2, rmax=4)                            # a bimodal prediction: blobs near 0.8 on a floor near 0.1
    pred = torch.from_numpy((0.2 * rng.random((12, 40, 72)) + 0.7 * blobs).astype(np.float32)).cuda()
    mask = P.binarize(pred)
    lab, num = P.label(mask, return_num=True)
    dist = P.label_distance(lab)
    cpu = mask.cpu().numpy()
    want_lab, n = LR.scipy_label(cpu, 3)
    assert 0 < cpu.mean() < 1 and n > 1 and int(num) == n
    want = E._label_ref(np.ascontiguousarray(want_lab), None)[0]
    np.testing.assert_array_equal(_bits(dist), E.sqrt_f32(want).view(np.int32))
    inside = P.distance_transform_edt(mask)                                              # per instance never farther than the mask's own distance to background
    assert (dist <= inside).all() and (dist[lab == 0] == 0).all()

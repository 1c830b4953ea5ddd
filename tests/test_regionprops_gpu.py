"""Region properties on the MI355X (biapy_amd/prepost.py: region_props, centroids, select_objects; csrc/regionprops.hip) against their statement
(tests/regionprops_ref.py, itself held against SciPy by test_regionprops_cpu.py): ``area``, ``coord_sum`` and ``bbox`` bit for bit; ``centroid``
within 1 fp64 ulp (``np.spacing``) of NumPy's ``coord_sum / area`` - both sides do one division of the same exact integers, and the one ulp is
there because the rounding of the device's fp64 division cannot be checked without the device.  The largest ulp distance seen goes to
profiles/regionprops_values.txt.  Inputs and references are built once per process."""
import os

import numpy as np
import pytest
import torch

import regionprops_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = os.path.join(ROOT, "profiles", "regionprops_values.txt")
_rows = {}
_REFS = {}


def _P():
    from biapy_amd import prepost

    return prepost


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                                  # a copy: the shared inputs are read-only


def _record(key, text):
    """profiles/regionprops_values.txt: one row per measured case, rewritten whole so that a partial run leaves a readable file."""
    _rows[key] = text
    try:
        with open(VALUES, "w") as f:
            f.write("biapy_amd.prepost.region_props on the device: what tests/test_regionprops_gpu.py measured (bound: 1 ulp of fp64)\n")
            for k in sorted(_rows):
                f.write(_rows[k] + "\n")
    except OSError:
        pass


def _ref(name):
    if name not in _REFS:
        labels, n_max = R.cases()[name]
        _REFS[name] = R.region_props_ref(labels, n_max)
    return _REFS[name]


def _check(p, want, ndim, what):
    """The device's RegionProps == the reference (area, coord_sum, bbox), the types, and the centroid within 1 ulp.  Returns the worst ulp distance."""
    area, sums, bbox = want
    n = area.shape[0]
    assert p.area.dtype == torch.int32 and tuple(p.area.shape) == (n,) and p.area.is_cuda, what
    assert p.bbox.dtype == torch.int32 and tuple(p.bbox.shape) == (n, 2 * ndim) and p.bbox.is_cuda, what
    assert p.coord_sum.dtype == torch.int64 and tuple(p.coord_sum.shape) == (n, ndim) and p.coord_sum.is_cuda, what
    assert p.centroid.dtype == torch.float64 and tuple(p.centroid.shape) == (n, ndim) and p.centroid.is_cuda, what
    np.testing.assert_array_equal(p.area.cpu().numpy(), area, err_msg=what)
    np.testing.assert_array_equal(p.coord_sum.cpu().numpy(), sums, err_msg=what)
    np.testing.assert_array_equal(p.bbox.cpu().numpy(), bbox, err_msg=what)
    got, c = p.centroid.cpu().numpy(), R.centroid_ref(area, sums)
    assert np.array_equal(np.isnan(got), np.isnan(c)) and np.isnan(got[0]).all(), what
    ok = area > 0
    ulps = float((np.abs(got[ok] - c[ok]) / np.spacing(np.abs(c[ok]))).max()) if ok.any() else 0.0
    print(f"{what}: centroid worst ulp distance {ulps}")
    assert ulps <= 1.0, what
    return ulps


def _run_case(name, num="int"):
    labels, n_max = R.cases()[name]
    d = _dev(labels)
    given = n_max if num == "int" else torch.tensor(n_max, dtype=torch.int32, device="cuda")
    return _check(_P().region_props(d, given), _ref(name), labels.ndim, name)


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_random_runs_bit_for_bit(shape):
    """Shapes unaligned everywhere, aligned, 2-D and 3-D, with axes of one voxel (every voxel a row start), with 0, 1, 7 and 1000 labels - 1000
    overflow the block's table."""
    worst = max(_run_case(f"runs {shape} L{k}") for k in R.LABEL_COUNTS)
    _record(f"runs {shape}", f"runs {shape}, 0 / 1 / 7 / 1000 labels: centroid worst ulp distance {worst}")


@pytest.mark.parametrize("x", R.ROW_LENGTHS, ids=str)
def test_rows_one_below_at_and_above_the_lane_trip_and_span_lengths(x):
    """Two rows of X voxels: a run must break at the row start even when the label continues."""
    worst = max(_run_case(f"one label 2 x {x}"), _run_case(f"runs 2 x {x}"))
    p = _P().region_props(_dev(R.cases()[f"one label 2 x {x}"][0]), 3)
    assert p.area.tolist() == [0, 0, 0, 2 * x] and p.bbox[3].tolist() == [0, 0, 2, x] and p.coord_sum[3].tolist() == [x, x * (x - 1)]
    _record(f"rows of {x:5d}", f"2 rows of {x}: centroid worst ulp distance {worst}")


def test_one_label_over_long_rows():
    """(2, 1 100 000): runs cut at span ends with x0 about 10^6, so L x0 passes 2^32; (3, 3, 70 000): the sum of x passes 2^32."""
    worst = max(_run_case("one label 2 x 1100000"), _run_case("one label 3 x 3 x 70000"))
    x = 1_100_000
    p = _P().region_props(_dev(R.cases()["one label 2 x 1100000"][0]), 2)
    assert p.coord_sum[2].tolist() == [x, x * (x - 1)] and x * (x - 1) > 2 ** 32 and p.centroid[2].tolist() == [0.5, (x - 1) / 2]
    _record("long rows", f"one label over rows of 1 100 000 and 70 000: centroid worst ulp distance {worst}")


def test_every_voxel_its_own_label():
    worst = _run_case("8192 voxels, each its own label")
    p = _P().region_props(_dev(R.cases()["8192 voxels, each its own label"][0]), 8192)
    assert (p.area[1:] == 1).all() and ((p.bbox[1:, 3:] - p.bbox[1:, :3]) == 1).all()
    assert torch.equal(p.centroid[1:], p.coord_sum[1:].double())
    _record("own labels", f"8192 voxels, each its own label: centroid worst ulp distance {worst}")


def test_n_max_zero_all_background_and_ignored_labels():
    P = _P()
    _run_case("n_max 0 under labels")
    p = P.region_props(_dev(R.cases()["n_max 0 under labels"][0]), 0)
    assert p.area.tolist() == [0] and p.bbox.tolist() == [[0] * 6] and p.coord_sum.tolist() == [[0] * 3]
    _run_case("all background")
    p = P.region_props(_dev(R.cases()["all background"][0]))                                # num = None: max() = 0
    assert p.area.tolist() == [0] and torch.isnan(p.centroid).all()
    _run_case("labels above num, negative labels")
    labels, _ = R.cases()["labels above num, negative labels"]
    assert (labels > 4).any() and (labels < 0).any()
    p = P.region_props(_dev(np.full((3, 4), -5, np.int32)))                                  # num = None under negative labels only
    assert p.area.tolist() == [0]


def test_num_as_int_as_tensor_and_as_none():
    P = _P()
    name = "runs (9, 21, 37) L7"
    labels, _ = R.cases()[name]
    _run_case(name, "int")
    _run_case(name, "tensor")
    top = int(labels.max())
    _check(P.region_props(_dev(labels)), R.region_props_ref(labels, top), 3, "num = None")
    _check(P.region_props(_dev(labels), 50), R.region_props_ref(labels, 50), 3, "num = an upper bound")
    lab, num = P.label(_dev((labels > 0).astype(np.uint8)), return_num=True)
    _check(P.region_props(lab, num), R.region_props_ref(lab.cpu().numpy(), int(num)), 3, "num = the tensor of label()")


def test_unaligned_and_non_contiguous_views():
    P = _P()
    for name in ("runs (9, 21, 37) L7", "runs (9, 21, 37) L1000"):
        labels, n_max = R.cases()[name]
        n = labels.size
        for off in (1, 2, 3):                                                                # 4, 8, 12 bytes past a 16-byte boundary
            buf = torch.zeros(n + 8, dtype=torch.int32, device="cuda")
            view = buf[off:off + n].view(labels.shape)
            view.copy_(_dev(labels))
            assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
            _check(P.region_props(view, n_max), _ref(name), 3, f"{name} at {4 * off} bytes")
        perm = _dev(labels.transpose(1, 0, 2)).permute(1, 0, 2)
        tall = torch.zeros((18,) + labels.shape[1:], dtype=torch.int32, device="cuda")
        tall[::2] = _dev(labels)
        for view in (perm, tall[::2]):
            assert not view.is_contiguous()
            _check(P.region_props(view, n_max), _ref(name), 3, f"{name}, a non-contiguous view")


def test_two_calls_give_the_same_bits():
    P = _P()
    for name in ("runs (9, 21, 37) L1000", "runs 2 x 8193", "one label 3 x 3 x 70000"):
        labels, n_max = R.cases()[name]
        d = _dev(labels)
        first, second = P.region_props(d, n_max), P.region_props(d, n_max)
        for a, b in zip(first[:3], second[:3]):
            assert torch.equal(a, b), name
        assert torch.equal(first.centroid.view(torch.int64), second.centroid.view(torch.int64)), name


def test_both_forms_give_the_same_bits():
    """Form (a), every run straight to the per-label arrays, against form (b), the block's table in LDS first."""
    from biapy_amd import _lib as L

    P = _P()
    try:
        for name in ("runs (9, 21, 37) L1000", "runs (8, 16, 64) L7", "runs 2 x 8193", "one label 2 x 1100000", "8192 voxels, each its own label"):
            labels, n_max = R.cases()[name]
            d = _dev(labels)
            got = []
            for form in (0, 1):
                L.lib.bpx_debug_set_regionprops_local(form)
                got.append(P.region_props(d, n_max))
                _check(got[-1], _ref(name), labels.ndim, f"{name}, form {'ab'[form]}")
            for a, b in zip(got[0][:3], got[1][:3]):
                assert torch.equal(a, b), name
    finally:
        L.lib.bpx_debug_set_regionprops_local(int(os.environ.get("BPX_REGIONPROPS_LOCAL", "-1")))      # negative: the library's default


def test_2d_input_equals_its_3d_form():
    P = _P()
    labels, n_max = R.cases()["runs (33, 70) L7"]
    two, three = P.region_props(_dev(labels), n_max), P.region_props(_dev(labels[None]), n_max)
    assert torch.equal(two.area, three.area)
    assert torch.equal(two.bbox, three.bbox[:, [1, 2, 4, 5]]) and torch.equal(two.coord_sum, three.coord_sum[:, 1:])
    assert (three.bbox[:, 0] == 0).all() and torch.equal(three.bbox[:, 3], (three.area > 0).to(torch.int32)) and (three.coord_sum[:, 0] == 0).all()
    assert torch.equal(torch.isnan(two.centroid), torch.isnan(three.centroid[:, 1:]))
    ok = two.area > 0
    assert torch.equal(two.centroid[ok], three.centroid[ok][:, 1:]) and (three.centroid[ok][:, 0] == 0).all()


_E2E = {}


def _instances():
    """binarize -> label of a prediction of overlapping balls at 64^3, once per process: (labels on the device, its host copy, N)."""
    if not _E2E:
        P = _P()
        shape = (64, 64, 64)
        rng = np.random.default_rng(3)
        pred = (0.2 * rng.random(shape) + 0.7 * R.balls(shape, fill=0.3, seed=3)).astype(np.float32)
        lab, num = P.label(P.binarize(_dev(pred)), connectivity=1, return_num=True)
        _E2E["v"] = (lab, lab.cpu().numpy(), int(num))
    return _E2E["v"]


def test_binarize_to_label_to_region_props_end_to_end_against_scipy():
    from scipy import ndimage

    P = _P()
    lab, host, n = _instances()
    assert n > 5
    p = P.region_props(lab, n)
    worst = _check(p, R.region_props_ref(host, n), 3, "64^3 balls")
    ids = np.arange(1, n + 1)
    np.testing.assert_array_equal(p.area.cpu().numpy()[1:], np.bincount(host.ravel(), minlength=n + 1)[1:])
    boxes = [[s.start for s in sl] + [s.stop for s in sl] for sl in ndimage.find_objects(host, max_label=n)]
    np.testing.assert_array_equal(p.bbox.cpu().numpy()[1:], np.asarray(boxes))
    com = np.asarray(ndimage.center_of_mass((host > 0).astype(np.float64), host, ids))
    np.testing.assert_allclose(p.centroid.cpu().numpy()[1:], com, rtol=1e-12, atol=0)
    assert torch.equal(p.area[1:], P.component_sizes(lab, n)[1:])
    _record("e2e", f"binarize -> label -> region_props, 64^3 balls, {n} labels: centroid worst ulp distance {worst}")


def test_centroids_is_the_centroid_without_the_background_row():
    P = _P()
    lab, _, n = _instances()
    c, p = P.centroids(lab, n), P.region_props(lab, n)
    assert tuple(c.shape) == (n, 3) and c.dtype == torch.float64 and torch.equal(c, p.centroid[1:]) and not torch.isnan(c).any()
    two = _dev(R.cases()["runs (33, 70) L7"][0])
    assert torch.equal(P.centroids(two, 7).view(torch.int64), P.region_props(two, 7).centroid[1:].view(torch.int64))


def test_select_objects_by_area_equals_remove_small_objects():
    P = _P()
    lab, _, n = _instances()
    p = P.region_props(lab, n)
    sizes = sorted(set(p.area[1:].tolist()))
    for m in (1, sizes[len(sizes) // 2], sizes[-1], sizes[-1] + 1, 64):
        for relabel in (False, True):
            want, want_n = P.remove_small_objects(lab, m, relabel=relabel, num=n, return_num=True)
            for keep in (p.area >= m, (p.area >= m).to(torch.uint8)):
                got, got_n = P.select_objects(lab, keep, relabel=relabel, return_num=True)
                assert got.dtype == torch.int32 and got.shape == lab.shape and got.data_ptr() != lab.data_ptr()
                assert torch.equal(got, want) and int(got_n) == int(want_n), (m, relabel)
    labels, _ = R.cases()["labels above num, negative labels"]                              # labels above len(keep) - 1 and negative ones become 0
    d = _dev(labels)
    p4 = P.region_props(d, 4)
    assert torch.equal(P.select_objects(d, p4.area >= 3), P.remove_small_objects(d, 3, num=4))
    assert torch.equal(P.select_objects(d.permute(1, 0, 2), p4.area >= 3), P.select_objects(d, p4.area >= 3).permute(1, 0, 2))


def test_select_objects_border_filter_all_and_none():
    P = _P()
    lab, host, n = _instances()
    p = P.region_props(lab, n)
    shape = torch.tensor(lab.shape, device="cuda")
    inside = (p.bbox[:, :3] > 0).all(1) & (p.bbox[:, 3:] < shape).all(1)
    touching = np.unique(np.concatenate([f.ravel() for f in (host[0], host[-1], host[:, 0], host[:, -1], host[:, :, 0], host[:, :, -1])]))
    keep_np = np.ones(n + 1, bool)
    keep_np[touching] = False
    assert 0 < keep_np[1:].sum() < n
    np.testing.assert_array_equal(inside.cpu().numpy()[1:], keep_np[1:])
    got, left = P.select_objects(lab, inside, return_num=True)
    np.testing.assert_array_equal(got.cpu().numpy(), np.where(keep_np[host], host, 0))
    assert int(left) == int(keep_np[1:].sum())
    renum, left = P.select_objects(lab, inside, relabel=True, return_num=True)
    new_id = np.where(keep_np, np.cumsum(keep_np & (np.arange(n + 1) > 0)), 0)
    np.testing.assert_array_equal(renum.cpu().numpy(), new_id[host])
    assert int(left) == int(renum.max())
    everything = torch.ones(n + 1, dtype=torch.bool, device="cuda")
    for relabel in (False, True):
        got, left = P.select_objects(lab, everything, relabel=relabel, return_num=True)
        assert torch.equal(got, lab) and int(left) == n
        got, left = P.select_objects(lab, ~everything, relabel=relabel, return_num=True)
        assert not got.any() and int(left) == 0
    everything[0] = False                                                                   # entry 0 is ignored either way
    assert torch.equal(P.select_objects(lab, everything), lab)


def test_graph_capture_of_label_region_props_select_objects():
    """Captured once with an upper bound for num, replayed after the mask was overwritten in place (an all-background one among them): every
    replay gives what the eager calls give on the mask of that moment."""
    P = _P()
    shape, bound, m = (12, 40, 56), 400, 20
    masks = [R.balls(shape, fill=f, seed=s, rmin=2, rmax=4) for f, s in ((0.3, 1), (0.15, 2))] + [np.zeros(shape, np.uint8), R.balls(shape, 0.3, 1, 2, 4)]
    mask = _dev(masks[0])

    def pipeline():
        lab = P.label(mask, connectivity=1)
        p = P.region_props(lab, bound)
        return lab, p, P.select_objects(lab, p.area >= m, relabel=True, return_num=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pipeline()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lab, p, (kept, left) = pipeline()
    for k, mk in enumerate(masks):
        mask.copy_(_dev(mk))
        g.replay()
        torch.cuda.synchronize()
        elab, n = P.label(_dev(mk), connectivity=1, return_num=True)
        assert int(n) <= bound and torch.equal(lab, elab)
        _check(p, R.region_props_ref(elab.cpu().numpy(), bound), 3, f"replay {k}")
        ekept, eleft = P.remove_small_objects(elab, m, relabel=True, num=int(n), return_num=True)
        assert torch.equal(kept, ekept) and int(left) == int(eleft)
        if not mk.any():
            assert not p.area.any() and not p.bbox.any() and int(left) == 0


def test_refusals_on_device_tensors():
    P = _P()
    a = torch.zeros(4, 5, 6, dtype=torch.int32, device="cuda")
    keep = torch.ones(3, dtype=torch.bool, device="cuda")
    for fn in (P.region_props, P.centroids):
        with pytest.raises(NotImplementedError, match="int32 labels"):
            fn(a.long(), 2)
        with pytest.raises(ValueError, match="2-D .* or 3-D"):
            fn(a.view(-1), 2)
        with pytest.raises(ValueError, match="2-D .* or 3-D"):
            fn(a[None], 2)
        with pytest.raises(NotImplementedError, match="empty"):
            fn(a[:0], 2)
        with pytest.raises(ValueError, match="num must not be negative"):
            fn(a, -1)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(a.cpu(), 2)
    with pytest.raises(NotImplementedError, match="int32 labels"):
        P.select_objects(a.long(), keep)
    with pytest.raises(NotImplementedError, match="keep must be a bool or uint8"):
        P.select_objects(a, keep.long())
    with pytest.raises(RuntimeError, match="keep must be on the device"):
        P.select_objects(a, keep.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.select_objects(a.cpu(), keep)
    with pytest.raises(NotImplementedError, match="empty"):
        P.select_objects(a[:0], keep)
    big = torch.empty((2, 2 ** 15, 2 ** 15), dtype=torch.int32, device="cuda")               # 2^31 voxels: nothing is launched
    with pytest.raises(NotImplementedError, match="2\\^31"):
        P.region_props(big, 1)

"""Shape properties on the MI355X (biapy_amd/prepost.py: shape_props and the derived measures; csrc/shapeprops.hip) against their statement
(tests/shapeprops_ref.py, itself held against independent statements by test_shapeprops_cpu.py): ``moments``, ``faces`` and
``perimeter_classes`` bit for bit, and so the four fields of ``region_props``; ``covariance`` bit for bit as well - both sides form the exact
numerator and then do the same correctly rounded float64 operations (conversions, one multiplication by 2^64, one addition, two divisions).  The
derived measures within the bounds stated at ``_check_derived``.  Inputs and references are built once per process."""
import numpy as np
import pytest
import torch

import regionprops_ref as RP
import shapeprops_ref as R

pytestmark = pytest.mark.gpu

_INT_FIELDS = ("area", "bbox", "coord_sum", "moments", "faces")


def _P():
    from biapy_amd import prepost

    return prepost


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                                  # a copy: the shared inputs are read-only


def _check(p, want, ndim, what):
    """The device's ShapeProps == the twin: every integer field and the covariance bit for bit, the types and shapes, the centroid within 1 ulp."""
    n = want["area"].shape[0]
    assert type(p).__name__ == "ShapeProps" and p._fields == ("area", "bbox", "coord_sum", "centroid", "moments", "covariance", "faces", "perimeter_classes")
    assert p.moments.dtype == torch.int64 and tuple(p.moments.shape) == (n, 6 if ndim == 3 else 3) and p.moments.is_cuda, what
    assert p.faces.dtype == torch.int64 and tuple(p.faces.shape) == (n, ndim) and p.faces.is_cuda, what
    assert p.covariance.dtype == torch.float64 and tuple(p.covariance.shape) == (n, ndim, ndim) and p.covariance.is_cuda, what
    assert p.area.dtype == torch.int32 and p.bbox.dtype == torch.int32 and p.coord_sum.dtype == torch.int64 and p.centroid.dtype == torch.float64
    for f in _INT_FIELDS:
        np.testing.assert_array_equal(getattr(p, f).cpu().numpy(), want[f], err_msg=f"{what}: {f}")
    if ndim == 2:
        assert p.perimeter_classes.dtype == torch.int32 and tuple(p.perimeter_classes.shape) == (n, 3) and p.perimeter_classes.is_cuda, what
        np.testing.assert_array_equal(p.perimeter_classes.cpu().numpy(), want["perimeter_classes"], err_msg=f"{what}: perimeter_classes")
    else:
        assert p.perimeter_classes is None, what
    np.testing.assert_array_equal(p.covariance.cpu().numpy().view(np.int64), want["covariance"].view(np.int64), err_msg=f"{what}: covariance")
    got, c = p.centroid.cpu().numpy(), want["centroid"]
    assert np.array_equal(np.isnan(got), np.isnan(c)), what
    ok = want["area"] > 0
    assert not ok.any() or float((np.abs(got[ok] - c[ok]) / np.spacing(np.abs(c[ok]))).max()) <= 1.0, what
    for f in ("moments", "faces", "covariance"):
        assert not getattr(p, f)[0].any(), f"{what}: row 0 of {f}"
        assert not getattr(p, f)[torch.from_numpy(~ok).cuda()].any(), f"{what}: {f} of an absent label"


def _run_case(name, num="int"):
    labels, n_max = R.cases()[name]
    given = n_max if num == "int" else torch.tensor(n_max, dtype=torch.int32, device="cuda")
    p = _P().shape_props(_dev(labels), given)
    _check(p, R.ref(name), labels.ndim, name)
    return p


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_random_runs_bit_for_bit(shape):
    """Shapes unaligned everywhere, aligned (X a multiple of 4: the 16-byte neighbour loads) and 2-D, with 0, 1, 7 and 1000 labels - 1000 labels
    overflow a block's 256-slot table."""
    for k in R.LABEL_COUNTS:
        _run_case(f"runs {shape} L{k}")


def test_an_axis_of_one_voxel_on_each_position():
    for shape in R.ONE_VOXEL_AXES:
        _run_case(f"runs {shape} L7")


@pytest.mark.parametrize("x", R.ROW_LENGTHS)
def test_rows_around_the_lane_and_trip_sizes(x):
    p = _run_case(f"one label 2 x {x}")
    assert p.faces[3].tolist() == [2 * x, 4] and p.area[3] == 2 * x                          # the hull of the 2 x X rectangle
    _run_case(f"runs 2 x 3 x {x}", num="tensor")


def test_compact_objects_2d_and_3d():
    for shape in ((37, 41), (64, 64), (5, 3), (1, 9), (6, 10, 14)):
        _run_case(f"blocks {shape}")


def test_one_run_across_trip_and_span_boundaries_has_two_x_faces():
    p = _run_case("one label 1 x 1 x 70000")
    assert p.faces[1].tolist() == [140000, 140000, 2]


def test_large_sums():
    """A row of 1 100 000 voxels of one label: sum xx passes 2^53.  The longest row the moments bound admits (computed from the rule): the closed
    form's largest intermediate lies just below 2^64; one voxel more is refused before anything is launched."""
    P = _P()
    p = _run_case("one label 1 x 1 x 1100000")
    n = 1_100_000
    assert int(p.moments[2, 2]) == (n - 1) * n * (2 * n - 1) // 6 > 2 ** 53
    E = R.longest_row()
    assert E * (E - 1) ** 2 < 2 ** 63 <= (E + 1) * E ** 2
    p = _run_case("the longest row the moments bound admits")
    assert int(p.moments[1, 2]) == (E - 1) * E * (2 * E - 1) // 6 and p.faces[1].tolist() == [2 * E, 2 * E, 2]
    too_long = torch.empty((1, 1, E + 1), dtype=torch.int32, device="cuda")                  # never read: refused with no launch
    with pytest.raises(NotImplementedError, match=r"n \* \(Emax - 1\)\^2 >= 2\^63"):
        P.shape_props(too_long, 1)
    from biapy_amd import _lib as L

    mom = torch.full((2, 6), -7, dtype=torch.int64, device="cuda")
    rc = L.lib.bpx_region_moments(too_long.data_ptr(), 1, 1, E + 1, 1, None, None, mom.data_ptr(), None, L.stream_ptr())
    assert rc != 0 and "must stay below 2^63" in L.lib.bpx_last_error().decode()
    torch.cuda.synchronize()
    assert (mom == -7).all()                                                                # no launch: not even the zero pass


def test_moments_without_covariance_form_the_sums_only():
    """cov_d = NULL: the sums alone, the same bits; area_d and sums_d are not asked for."""
    from biapy_amd import _lib as L

    for name in ("runs (9, 21, 37) L1000", "runs (37, 41) L7"):
        labels, n_max = R.cases()[name]
        d = _dev(labels)
        Z, Y, X = (1,) + labels.shape if labels.ndim == 2 else labels.shape
        mom = torch.full((n_max + 1, 6), -7, dtype=torch.int64, device="cuda")
        L.check(L.lib.bpx_region_moments(d.data_ptr(), Z, Y, X, n_max, None, None, mom.data_ptr(), None, L.stream_ptr()))
        want = R.ref(name)["moments"]
        np.testing.assert_array_equal(mom.cpu().numpy()[:, [1, 2, 5]] if labels.ndim == 2 else mom.cpu().numpy(), want)


def test_every_voxel_its_own_label_overflows_the_block_table():
    p = _run_case("8192 voxels, each its own label")
    assert (p.area[1:] == 1).all() and (p.faces[1:] == 2).all() and not p.covariance.any()


def test_label_range():
    P = _P()
    _run_case("labels above num, negative labels")
    _run_case("n_max 0 under labels")
    p = _run_case("all background")
    assert not p.moments.any() and not p.faces.any()
    p = P.shape_props(_dev(np.full((3, 4), -5, np.int32)))                                   # num = None under negative labels only: max() < 0
    assert tuple(p.moments.shape) == (1, 3) and tuple(p.perimeter_classes.shape) == (1, 3) and not p.faces.any()
    labels, _ = R.cases()["runs (9, 21, 37) L7"]
    top = int(labels.max())
    _check(P.shape_props(_dev(labels)), R.shape_props_ref(labels, top), 3, "num = None")


def test_unaligned_and_non_contiguous_views():
    P = _P()
    for name in ("runs (8, 16, 64) L7", "runs (9, 21, 37) L1000", "blocks (64, 64)"):
        labels, n_max = R.cases()[name]
        n = labels.size
        for off in (1, 2, 3):                                                                # 4, 8, 12 bytes past a 16-byte boundary
            buf = torch.zeros(n + 8, dtype=torch.int32, device="cuda")
            view = buf[off:off + n].view(labels.shape)
            view.copy_(_dev(labels))
            assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
            _check(P.shape_props(view, n_max), R.ref(name), labels.ndim, f"{name} at {4 * off} bytes")
        perm = _dev(np.swapaxes(labels, 0, 1)).transpose(0, 1)
        tall = torch.zeros((2 * labels.shape[0],) + labels.shape[1:], dtype=torch.int32, device="cuda")
        tall[::2] = _dev(labels)
        for view in (perm, tall[::2]):
            assert not view.is_contiguous()
            _check(P.shape_props(view, n_max), R.ref(name), labels.ndim, f"{name}, a non-contiguous view")


def test_two_calls_give_the_same_bits():
    P = _P()
    for name in ("runs (9, 21, 37) L1000", "runs (37, 41) L1000", "one label 1 x 1 x 70000"):
        labels, n_max = R.cases()[name]
        d = _dev(labels)
        first, second = P.shape_props(d, n_max), P.shape_props(d, n_max)
        for a, b in zip(first, second):
            assert (a is None and b is None) or torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                                                            b.view(torch.int64) if b.dtype == torch.float64 else b), name


def test_2d_input_equals_its_3d_form():
    P = _P()
    labels, n_max = R.cases()["runs (37, 41) L7"]
    two, three = P.shape_props(_dev(labels), n_max), P.shape_props(_dev(labels[None]), n_max)
    assert torch.equal(two.moments, three.moments[:, [1, 2, 5]]) and not three.moments[:, [0, 3, 4]].any()
    assert torch.equal(two.faces, three.faces[:, 1:]) and torch.equal(three.faces[:, 0], 2 * three.area.long())
    assert torch.equal(two.covariance, three.covariance[:, 1:, 1:]) and not three.covariance[:, 0].any() and not three.covariance[:, :, 0].any()
    assert three.perimeter_classes is None and torch.equal(two.area, three.area)


def test_perimeter_cases_and_their_hand_counts():
    P = _P()
    for name in ("touching labels 20 x 70", "labels on the image edge 18 x 67", "one-pixel lines 17 x 70", "checkerboard of two labels 17 x 70"):
        _run_case(name)
    square = np.zeros((9, 9), np.int32)
    square[2:7, 2:7] = 1                                                                      # a 5 x 5 square: 12 edge pixels of code 5 (weight 1), 4 corners of code 5
    p = P.shape_props(_dev(square), 1)
    assert p.perimeter_classes[1].tolist() == [16, 0, 0] and float(P.perimeter(p)[1]) == 16.0 and p.faces[1].tolist() == [10, 10]
    assert float(P.circularity(p)[1]) == 4 * np.pi * 25 / 256


def test_region_props_is_unchanged_in_both_forms():
    from biapy_amd import _lib as L

    P = _P()
    try:
        for name in ("runs (9, 21, 37) L1000", "runs (8, 16, 64) L7", "runs (37, 41) L7"):
            labels, n_max = R.cases()[name]
            d = _dev(labels)
            want = RP.region_props_ref(labels, n_max)
            for form in (0, 1):
                L.lib.bpx_debug_set_regionprops_local(form)
                r, s = P.region_props(d, n_max), P.shape_props(d, n_max)
                for got in (r, s):
                    np.testing.assert_array_equal(got.area.cpu().numpy(), want[0])
                    np.testing.assert_array_equal(got.coord_sum.cpu().numpy(), want[1])
                    np.testing.assert_array_equal(got.bbox.cpu().numpy(), want[2])
                assert torch.equal(r.centroid.view(torch.int64), s.centroid.view(torch.int64)) and type(r).__name__ == "RegionProps"
    finally:
        L.lib.bpx_debug_set_regionprops_local(-1)                                           # negative: the library's default


def _check_derived(P, p, want, ndim, what, sampling=None):
    """principal_moments against numpy.linalg.eigvalsh and against the closed form in NumPy within R.EIG_BOUND units of 2^-52 * trace (measured on
    the CPU, shapeprops_ref's docstring).  The other measures are at most four correctly rounded float64 operations (sqrt, *, /) or a pow of a few
    ulp on the device's own fields and eigenvalues: 8 ulp relative against the same expression in NumPy, NaN and inf in the same places."""
    lam = P.principal_moments(p).cpu().numpy()
    cov = want["covariance"]
    assert lam.shape == (len(cov), ndim) and (lam >= 0).all() and (np.diff(lam, axis=1) <= 0).all(), what
    dev = R.eig_deviation(cov, lam)
    twin = R.principal_moments_ref(cov)
    trace = np.trace(cov, axis1=1, axis2=2)
    print(f"{what}: eigenvalues {dev:.3f} units of 2^-52 trace from eigvalsh")
    assert dev <= R.EIG_BOUND, what
    assert (np.abs(lam - twin).max(1) <= R.EIG_BOUND * 2.0 ** -52 * trace).all(), what
    fields = R.derived_ref(want["area"], lam, want["faces"], want["perimeter_classes"], sampling)
    got = dict(axis_lengths=P.axis_lengths(p), elongation=P.elongation(p), surface_area=P.surface_area(p, sampling))
    if ndim == 2:
        got.update(perimeter=P.perimeter(p), circularity=P.circularity(p))
    else:
        got.update(sphericity=P.sphericity(p, sampling))
    assert set(got) == set(fields)
    for k, v in got.items():
        g, w = v.cpu().numpy(), fields[k]
        assert v.dtype == torch.float64 and g.shape == w.shape, (what, k)
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isinf(g), np.isinf(w)), (what, k)
        ok = np.isfinite(w)
        assert (np.abs(g[ok] - w[ok]) <= 8 * np.spacing(np.abs(w[ok]))).all(), (what, k)


def test_derived_measures():
    P = _P()
    for name in ("blocks (6, 10, 14)", "blocks (64, 64)", "runs (9, 21, 37) L7", "runs (37, 41) L7", "full cube 7", "8192 voxels, each its own label",
                 "one label 1 x 1 x 70000", "touching labels 20 x 70"):
        labels, n_max = R.cases()[name]
        p = P.shape_props(_dev(labels), n_max)
        _check_derived(P, p, R.ref(name), labels.ndim, name)
        _check_derived(P, p, R.ref(name), labels.ndim, name + ", anisotropic", sampling=(2.0, 0.5, 1.5)[:labels.ndim])
    cube = P.shape_props(_dev(np.ones((7, 7, 7), np.int32)), 1)
    assert cube.covariance[1].tolist() == [[4.0, 0, 0], [0, 4.0, 0], [0, 0, 4.0]] and cube.faces[1].tolist() == [98, 98, 98]
    assert float(P.elongation(cube)[1]) == 1.0 and abs(float(P.sphericity(cube)[1]) - (np.pi / 6) ** (1 / 3)) < 1e-14
    rod = P.shape_props(_dev(np.ones((1, 1, 30), np.int32)), 1)
    assert torch.isinf(P.elongation(rod)[1]) and torch.isnan(P.elongation(rod)[0])
    one = P.shape_props(_dev(np.ones((1, 1, 1), np.int32)), 1)
    assert torch.isnan(P.elongation(one)[1]) and one.faces[1].tolist() == [2, 2, 2]
    with pytest.raises(ValueError, match="2-D labels only"):
        P.perimeter(cube)
    with pytest.raises(ValueError, match="3-D labels only"):
        P.sphericity(P.shape_props(_dev(np.ones((3, 3), np.int32)), 1))


_E2E = {}


def _instances():
    """binarize -> label of a prediction of overlapping balls at 64^3, once per process: (labels on the device, its host copy, N)."""
    if not _E2E:
        P = _P()
        shape = (64, 64, 64)
        rng = np.random.default_rng(3)
        pred = (0.2 * rng.random(shape) + 0.7 * RP.balls(shape, fill=0.3, seed=3)).astype(np.float32)
        lab, num = P.label(P.binarize(_dev(pred)), connectivity=1, return_num=True)
        _E2E["v"] = (lab, lab.cpu().numpy(), int(num))
    return _E2E["v"]


def test_binarize_label_shape_props_select_objects_chain():
    P = _P()
    lab, host, n = _instances()
    assert n > 5
    p = P.shape_props(lab, n)
    want = R.shape_props_ref(host, n)
    _check(p, want, 3, "64^3 balls")
    _check_derived(P, p, want, 3, "64^3 balls")
    lam = R.principal_moments_ref(want["covariance"])
    with np.errstate(invalid="ignore", divide="ignore"):
        el = np.sqrt(lam[:, 0] / lam[:, 2])
    finite = np.sort(el[np.isfinite(el)])
    assert len(finite) > 4
    t = float((finite[len(finite) // 2 - 1] + finite[len(finite) // 2]) / 2)                 # between two objects' values: no tie for the filter to break
    keep = np.nan_to_num(el, nan=np.inf) < t
    assert 0 < keep[1:].sum() < n
    got, left = P.select_objects(lab, P.elongation(p) < t, return_num=True)
    np.testing.assert_array_equal(got.cpu().numpy(), np.where(keep[host], host, 0))
    assert int(left) == int(keep[1:].sum())


@pytest.mark.parametrize("ndim", (3, 2))
def test_graph_capture_of_label_shape_props_select_objects(ndim):
    """Captured once with an upper bound for num, replayed after the mask was overwritten in place (an all-background one among them)."""
    P = _P()
    shape, bound = (12, 40, 56), 400
    masks = [RP.balls(shape, fill=f, seed=s, rmin=2, rmax=4) for f, s in ((0.3, 1), (0.15, 2))] + [np.zeros(shape, np.uint8), RP.balls(shape, 0.3, 1, 2, 4)]
    if ndim == 2:
        masks = [m[5] for m in masks]
    mask = _dev(masks[0])

    def keep_of(p):
        if ndim == 2:
            return (P.circularity(p) > 0.5) & (P.elongation(p) < 2.5) & (P.surface_area(p, (2.0, 1.0)) > 20)
        return (P.sphericity(p, (2.0, 1.0, 1.0)) > 0.6) & (P.elongation(p) < 2.5) & (P.axis_lengths(p)[:, 0] > 4)

    def pipeline():
        lab = P.label(mask, connectivity=1)
        p = P.shape_props(lab, bound)
        keep = keep_of(p)
        return lab, p, keep, P.select_objects(lab, keep, relabel=True, return_num=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pipeline()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lab, p, keep, (kept, left) = pipeline()
    for k, mk in enumerate(masks):
        mask.copy_(_dev(mk))
        g.replay()
        torch.cuda.synchronize()
        elab = P.label(_dev(mk), connectivity=1)
        assert torch.equal(lab, elab)
        _check(p, R.shape_props_ref(elab.cpu().numpy(), bound), ndim, f"replay {k}")
        ekeep = keep_of(P.shape_props(elab, bound))
        ekept, eleft = P.select_objects(elab, ekeep, relabel=True, return_num=True)
        assert torch.equal(keep, ekeep) and torch.equal(kept, ekept) and int(left) == int(eleft)
        if k == 0:
            assert 0 < int(left) < int(elab.max())
        if not mk.any():
            assert not p.moments.any() and not p.faces.any() and not p.covariance.any() and not kept.any()


def test_refusals_on_device_tensors():
    P = _P()
    a = torch.zeros(4, 5, 6, dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError, match="int32 labels"):
        P.shape_props(a.long(), 2)
    with pytest.raises(ValueError, match="2-D .* or 3-D"):
        P.shape_props(a.view(-1), 2)
    with pytest.raises(NotImplementedError, match="empty"):
        P.shape_props(a[:0], 2)
    with pytest.raises(ValueError, match="num must not be negative"):
        P.shape_props(a, -1)
    with pytest.raises(TypeError, match="takes the ShapeProps"):
        P.elongation(P.region_props(a, 2))
    with pytest.raises(ValueError, match="sampling must be 3 finite positive numbers"):
        P.surface_area(P.shape_props(a, 2), (1.0, 2.0))

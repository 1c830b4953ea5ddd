"""Nearest-source indices of the distance transform on the MI355X (biapy_amd/prepost.py: distance_transform_edt(return_indices=...),
expand_labels, voronoi_on_mask; csrc/edt_index.hip).  On the unit grid every comparison is bit for bit against the host twin
(tests/edt_index_ref.py: the nearest zero, the raster-first among equally near ones), and the distances returned beside the indices against
the plain call.  With ``sampling`` the index must name a zero voxel whose distance - evaluated on the host in fp64 and rounded to float32 -
lies within 1 fp32 ulp of ``float32(scipy float64)``, the bound tests/test_edt_gpu.py holds that path's distances to, for the same reason:
both are fp64 evaluations of a real candidate distance within a few 2^-53 of the true minimum.  Inputs: tests/edt_ref.py."""
import os

import numpy as np
import pytest
import torch

import edt_index_ref as R
import edt_ref as E
import label_ref as LR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _P():
    from biapy_amd import prepost

    return prepost


def _dev(a):
    return torch.from_numpy(np.asarray(a)).cuda()


def _check(mask):
    """Linear indices against the twin, and the distances beside them against the plain call, both bit for bit."""
    P, m = _P(), _dev(mask)
    want_sq, want = R.twin(mask)
    sq, idx = P.distance_transform_edt(m, squared=True, return_indices="linear")
    assert idx.dtype == torch.int32 and idx.shape == tuple(mask.shape) and idx.is_cuda and idx.is_contiguous()
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    assert sq.dtype == torch.int32 and torch.equal(sq, P.distance_transform_edt(m, squared=True))
    np.testing.assert_array_equal(sq.cpu().numpy(), want_sq)
    d, idx2 = P.distance_transform_edt(m, return_indices="linear")
    assert d.dtype == torch.float32 and torch.equal(d.view(torch.int32), P.distance_transform_edt(m).view(torch.int32)) and torch.equal(idx2, idx)
    only = P.distance_transform_edt(m, return_distances=False, return_indices="linear")                      # the values then live in the workspace
    assert torch.equal(only, idx)
    return idx


@pytest.mark.parametrize("shape", E.SHAPES, ids=str)
def test_random_masks_bit_for_bit(shape):
    """Densities 0.5 ... 0.999 on every shape of edt_ref: rows of several 64-lane chunks ((1, 1, 300), (17, 16, 200): the run start and end carry
    across chunks and the left / right tie is met), 2-D in both spellings, unit axes, ties on every axis at density 0.5."""
    for p in E.DENSITIES:
        _check(E.random_masks(shape)[p])


@pytest.mark.parametrize("name", [n for n in E.STRUCTURED if n != "zero"])
def test_structured_masks_bit_for_bit(name):
    """20 x 43 x 150.  plane_x: every row's g is equal along Y, so all 43 sites survive in the envelope - deeper than the 32 entries a thread
    keeps in LDS, the spill to the workspace slab carries indices.  checkerboard: ties on every axis.  The corner zeros: one index everywhere."""
    mask = E.structured(name)
    idx = _check(mask)
    if name.startswith("corner") or name == "centre":
        assert (idx == int(np.flatnonzero(mask.reshape(-1) == 0)[0])).all()


def test_all_zero_names_itself_and_all_one_gives_minus_one():
    P = _P()
    zero = _dev(E.structured("zero"))
    own = torch.arange(zero.numel(), dtype=torch.int32, device="cuda").view(zero.shape)
    for kw in (dict(), dict(squared=True), dict(sampling=(2.0, 1.0, 0.5))):
        d, idx = P.distance_transform_edt(zero, return_indices="linear", **kw)
        assert torch.equal(idx, own) and not d.any()
    for shape in (E.BIG, (33, 70), (1, 1, 300), (5, 1, 1)):
        one = torch.ones(shape, dtype=torch.uint8, device="cuda")
        sq, idx = P.distance_transform_edt(one, squared=True, return_indices="linear")
        assert (idx == -1).all() and (sq == 2 ** 31 - 1).all()
        for kw in (dict(), dict(sampling=(1.0,) * len(shape))):
            d, idx = P.distance_transform_edt(one, return_indices=True, **kw)
            assert idx.shape == (len(shape),) + tuple(shape) and (idx == -1).all() and torch.isinf(d).all() and (d > 0).all()
        assert (P.distance_transform_edt(one, return_distances=False, return_indices="linear") == -1).all()


@pytest.mark.parametrize("name", list(E.LONG))
def test_long_axes(name):
    """(1,1,40000), (1,30000,3), (5000,2,3) with a single zero at a corner: its index everywhere, the distances the closed form."""
    mask, sq = E.long_axis(name)
    shape, at = E.LONG[name]
    got, idx = _P().distance_transform_edt(_dev(mask), squared=True, return_indices="linear")
    assert (idx == int(np.ravel_multi_index(at, shape))).all()
    np.testing.assert_array_equal(got.cpu().numpy(), sq)


def test_input_forms():
    """bool inputs, every nonzero byte the same foreground, non-contiguous views, the 2-D spellings, and SciPy's coordinate form."""
    P = _P()
    base = E.random_masks((9, 21, 37))[0.9]
    want = R.twin(base)[1]
    vals = np.random.default_rng(1).choice(np.array([1, 2, 255], np.uint8), size=base.shape)
    for m in (_dev(base * vals), _dev(base.astype(bool))):
        np.testing.assert_array_equal(P.distance_transform_edt(m, return_distances=False, return_indices="linear").cpu().numpy(), want)
    perm = _dev(np.ascontiguousarray(base.transpose(1, 0, 2))).permute(1, 0, 2)
    tall = torch.zeros(18, 21, 37, dtype=torch.uint8, device="cuda")
    tall[::2] = _dev(base)
    for view in (perm, tall[::2], tall.bool()[::2]):
        assert not view.is_contiguous()
        d, idx = P.distance_transform_edt(view, return_indices="linear")
        assert idx.is_contiguous() and d.is_contiguous() and np.array_equal(idx.cpu().numpy(), want)
    d, co = P.distance_transform_edt(_dev(base), return_indices=True)                                        # (distances, indices), SciPy's order and form
    assert co.dtype == torch.int32 and co.shape == (3,) + base.shape and d.shape == base.shape and d.dtype == torch.float32
    np.testing.assert_array_equal(co.cpu().numpy(), R.unravel(want, base.shape))
    np.testing.assert_array_equal(P.distance_transform_edt(_dev(base), return_distances=False, return_indices=True).cpu().numpy(), R.unravel(want, base.shape))
    flat = E.random_masks((33, 70))[0.99]
    a, b = (P.distance_transform_edt(_dev(f), return_distances=False, return_indices="linear") for f in (flat, flat[None]))
    assert a.shape == (33, 70) and b.shape == (1, 33, 70) and torch.equal(a, b[0])
    co2 = P.distance_transform_edt(_dev(flat), return_distances=False, return_indices=True)
    assert co2.shape == (2, 33, 70) and np.array_equal(co2.cpu().numpy(), R.unravel(R.twin(flat)[1], flat.shape))


def test_default_call_is_unchanged():
    """No keyword, and the keywords at their defaults, return today's tensor: SciPy bit for bit."""
    P = _P()
    for mask in (E.random_masks((17, 16, 200))[0.9], E.structured("balls")):
        m = _dev(mask)
        for kw in (dict(), dict(squared=True), dict(sampling=(2.0, 1.0, 0.5))):
            a, b = P.distance_transform_edt(m, **kw), P.distance_transform_edt(m, return_distances=True, return_indices=False, **kw)
            assert isinstance(a, torch.Tensor) and torch.equal(a, b)
        np.testing.assert_array_equal(P.distance_transform_edt(m, squared=True).cpu().numpy(), E.scipy_sq(mask))


def _ulps(got, want):
    g, w = got.view(np.int32).astype(np.int64), want.view(np.int32).astype(np.int64)
    diff = np.abs(g - w)
    return int(diff.max()), int((diff != 0).sum())


def _sampling_cases():
    cases = []
    for s in E.SAMPLINGS:
        cases += [(E.random_masks(shape)[p], s, f"random {shape} p={p}") for shape in ((9, 21, 37), (17, 16, 200)) for p in (0.5, 0.99)]
        cases += [(E.structured(n), s, n) for n in ("corner000", "plane_x", "checkerboard", "balls")]
    cases += [(E.random_masks((33, 70))[p], E.SAMPLING_2D, f"random (33, 70) p={p}") for p in E.DENSITIES]
    return cases


def test_sampling_index_within_one_fp32_ulp_of_scipy():
    """sampling (2, 1, 0.5), (40, 4, 4) and a 2-D pair: the index names a zero voxel, and float32(sqrt(sum((w * delta)^2))) - evaluated on the host
    in fp64 from the index - is within 1 fp32 ulp of float32(scipy float64); the distances beside the indices are the plain call's bits.  What
    was seen is appended to profiles/edt_values.txt."""
    P = _P()
    worst, differ, voxels = 0, 0, 0
    for mask, s, name in _sampling_cases():
        m = _dev(mask)
        d, idx = P.distance_transform_edt(m, sampling=s, return_indices="linear")
        assert torch.equal(d.view(torch.int32), P.distance_transform_edt(m, sampling=s).view(torch.int32)), (name, s)
        i = idx.cpu().numpy()
        assert i.min() >= 0 and not mask.reshape(-1)[i].any(), (name, s)                                     # points at a source
        got = np.sqrt(R.sq_of(i, mask.shape, s)).astype(np.float32)
        u, cnt = _ulps(got, E.scipy_f32(mask, s))
        print(f"edt index sampling {s} {name}: largest difference {u} ulp, {cnt} of {mask.size} voxels differ")
        worst, differ, voxels = max(worst, u), differ + cnt, voxels + mask.size
        assert u <= 1, (name, s, u)
    line = (f"tests/test_edt_index_gpu.py sampling path, distance of the returned index against float32(scipy float64), {voxels} voxels: "
            f"largest {worst} ulp, {differ} voxels differ")
    print(line)
    try:
        with open(os.path.join(ROOT, "profiles", "edt_values.txt"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass                                                                             # a read-only checkout: the figures are in the output


@pytest.mark.parametrize("name", ["blocks", "balls"])
def test_expand_labels_and_voronoi_on_mask_against_their_twins(name):
    P = _P()
    lab = E.labels(name)
    l = _dev(lab)
    for distance in (0, 1, 2.5, 1000, 1e200):
        out = P.expand_labels(l, distance)
        assert out.dtype == torch.int32 and out.shape == l.shape and out.data_ptr() != l.data_ptr()
        np.testing.assert_array_equal(out.cpu().numpy(), R.expand_ref(lab, distance), err_msg=str(distance))
    np.testing.assert_array_equal(l.cpu().numpy(), lab)                                                      # the input is left alone
    mask = E.random_masks(lab.shape)[0.5]
    for m in (_dev(mask), _dev(mask.astype(bool))):
        np.testing.assert_array_equal(P.voronoi_on_mask(l, m).cpu().numpy(), R.voronoi_ref(lab, mask))
    lperm = _dev(np.ascontiguousarray(lab.transpose(2, 1, 0))).permute(2, 1, 0)                              # int32 labels, inverted, non-contiguous
    assert not lperm.is_contiguous()
    np.testing.assert_array_equal(P.expand_labels(lperm, 2).cpu().numpy(), R.expand_ref(lab, 2))
    none = torch.zeros_like(l)
    assert not P.expand_labels(none, 5).any() and not P.voronoi_on_mask(none, _dev(mask)).any()
    unit = P.expand_labels(l, 2.5, sampling=(1, 1, 1))                                                       # the fp64 path on the unit grid: the same voxels grow
    assert torch.equal(unit != 0, P.expand_labels(l, 2.5) != 0)
    assert torch.equal(P.expand_labels(l, 1e200, sampling=(2, 1, 0.5)) != 0, torch.ones_like(l, dtype=torch.bool))   # beyond float32: still finite
    assert not P.expand_labels(none, 1e200, sampling=(2, 1, 0.5)).any()
    with pytest.raises(RuntimeError, match="no CPU path"):                                                  # a CPU mask beside device labels: refused before any launch
        P.voronoi_on_mask(l, torch.from_numpy(np.asarray(mask).copy()))


def test_two_calls_give_the_same_bits():
    P = _P()
    for mask in (E.random_masks((17, 16, 200))[0.5], E.structured("checkerboard"), E.structured("plane_x")):
        m = _dev(mask)
        for kw in (dict(squared=True), dict(), dict(sampling=(2.0, 1.0, 0.5))):
            (d1, i1), (d2, i2) = (P.distance_transform_edt(m, return_indices="linear", **kw) for _ in range(2))
            assert torch.equal(i1, i2) and torch.equal(d1.view(torch.int32), d2.view(torch.int32))
    l = _dev(E.labels("balls"))
    assert torch.equal(P.expand_labels(l, 3), P.expand_labels(l, 3))


def test_graph_capture_of_expand_labels():
    """Captured once, replayed after the labels were overwritten in place: the eager result for the NEW labels."""
    P = _P()
    first, second = E.labels("blocks"), np.ascontiguousarray(E.labels("blocks")[::-1])
    l = _dev(first).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        P.expand_labels(l, 2)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = P.expand_labels(l, 2)
    for lab in (first, second, np.zeros_like(first), first):
        l.copy_(_dev(lab))
        g.replay()
        assert torch.equal(out, P.expand_labels(_dev(lab), 2))
        np.testing.assert_array_equal(out.cpu().numpy(), R.expand_ref(lab, 2))


def test_binarize_label_expand_labels_region_props_end_to_end():
    P = _P()
    rng = np.random.default_rng(3)
    blobs = LR.balls((12, 40, 72), fill=0.15, rmin=2, rmax=4)                            # a bimodal prediction: blobs near 0.8 on a floor near 0.1
    pred = torch.from_numpy((0.2 * rng.random((12, 40, 72)) + 0.7 * blobs).astype(np.float32)).cuda()
    lab, num = P.label(P.binarize(pred), return_num=True)
    grown = P.expand_labels(lab, 2)
    n = int(num)
    assert n > 1
    np.testing.assert_array_equal(grown.cpu().numpy(), R.expand_ref(lab.cpu().numpy(), 2))
    before, after = P.region_props(lab, n), P.region_props(grown, n)
    assert (after.area >= before.area).all() and int(after.area.sum()) > int(before.area.sum())              # no instance shrinks, some grow
    assert torch.equal(torch.unique(grown), torch.unique(lab))                                               # the ids remain the original set
    assert torch.equal(grown[lab != 0], lab[lab != 0])                                                       # nothing is relabelled: no two instances merge
    assert int(P.label(grown != 0, return_num=True)[1]) <= n                                                 # though their foregrounds may touch

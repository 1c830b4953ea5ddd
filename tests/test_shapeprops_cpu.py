"""Shape properties - what can be checked without a GPU: the entry points are declared, exported and bound; every host-side refusal of the three
entries names its cause, in the stated order, before anything is launched; ``prepost.shape_props`` and the derived calls refuse on CPU tensors;
the NumPy twins the GPU tests hold the device against (tests/shapeprops_ref.py) agree with independent statements - ``np.bincount`` with integer
weights, shifted-array comparisons on padded volumes, the SciPy restatement of scikit-image's perimeter per label - on every input those tests
use; the twin's covariance lies within its derived bound of the exact ``fractions.Fraction`` value; the closed-form eigenvalues lie within 4 x
their measured deviation from ``numpy.linalg.eigvalsh``; hand-made cases; and the comparators catch three seeded defects."""
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import shapeprops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NAMES = ("bpx_region_moments", "bpx_region_faces", "bpx_region_perimeter2d")
VALUES = os.path.join(ROOT, "profiles", "shapeprops_values.txt")
A = 4096                                   # any non-null, aligned "device" address: nothing is launched


def test_entry_points_are_declared_exported_and_bound():
    from biapy_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    source = open(os.path.join(ROOT, "biapy_amd", "csrc", "shapeprops.hip")).read()
    assert set(re.findall(r'extern "C" \w+ (\w+)\(', source)) == set(NAMES)
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in L.EXPORTS and getattr(L.lib._raw, name) is not None, name
        assert getattr(L.lib._raw, name).restype is L.C.c_int
    vp, i = L.C.c_void_p, L.C.c_int
    assert L._SIGS["bpx_region_moments"][0] == [vp, i, i, i, i, vp, vp, vp, vp, vp]
    assert L._SIGS["bpx_region_faces"][0] == [vp, i, i, i, i, vp, vp]
    assert L._SIGS["bpx_region_perimeter2d"][0] == [vp, i, i, i, vp, vp]
    make = open(os.path.join(ROOT, "biapy_amd", "csrc", "Makefile")).read()
    assert "shapeprops.hip" in make and re.search(r"^shapeprops\.o:.*shapeprops_core\.h.*regionprops_core\.h.*label_walk\.h", make, re.M)
    core = open(os.path.join(ROOT, "biapy_amd", "csrc", "shapeprops_core.h")).read()
    assert '#include "shapeprops_core.h"' in source and not re.search(r"\bSP_HD \w+ sp_\w+\(", source)      # the shared steps, not a copy
    for fn in ("sp_moments_fit", "sp_apply_moments", "sp_cov_numerator", "sp_cov_entry", "sp_finish_row", "sp_face", "sp_lane_faces", "sp_count_step",
               "sp_merge_counts", "sp_is_border", "sp_perimeter_class", "sp_pixel_class"):
        assert re.search(r"SP_HD \w+ %s\(" % fn, core) and fn + "(" in source + core, fn
    check = open(os.path.join(ROOT, "scripts", "shapeprops_cpu_check.cpp")).read()
    assert '#include "shapeprops_core.h"' in check and "int main()" in check and "-fsanitize=address,undefined" in check


def test_host_checks_answer_without_a_device_in_the_stated_order():
    from biapy_amd import _lib as L

    lib = L.lib

    def err():
        return lib.bpx_last_error().decode()

    def moments(labels=A, Z=4, Y=5, X=6, n_max=3, area=A, sums=A, mom=A, cov=A):
        return lib.bpx_region_moments(labels, Z, Y, X, n_max, area, sums, mom, cov, None)

    def faces(labels=A, Z=4, Y=5, X=6, n_max=3, faces=A):
        return lib.bpx_region_faces(labels, Z, Y, X, n_max, faces, None)

    def perimeter(labels=A, Z=1, Y=5, X=6, n_max=3, classes=A):
        assert Z == 1
        return lib.bpx_region_perimeter2d(labels, Y, X, n_max, classes, None)

    for fn, nulls in ((moments, (dict(labels=None), dict(mom=None), dict(area=None), dict(sums=None))), (faces, (dict(labels=None), dict(faces=None))),
                      (perimeter, (dict(labels=None), dict(classes=None)))):
        for kw in nulls:
            assert fn(**kw) != 0 and "null pointer" in err(), (fn.__name__, kw)
            assert fn(Y=0, n_max=-1, **kw) != 0 and "null pointer" in err(), (fn.__name__, kw)       # the first refusal wins
        for kw in (dict(Y=0), dict(X=0), dict(X=-7), dict(Y=-1)):
            assert fn(n_max=-1, **kw) != 0 and "extents must be at least 1" in err(), (fn.__name__, kw)
        for Y, X in ((65536, 32768), (2 ** 31 - 1, 2 ** 31 - 1)):
            assert fn(Y=Y, X=X, n_max=-1) != 0 and "2^31 voxels or more" in err(), (fn.__name__, Y, X)
        for n_max in (-1, -2 ** 31, 2 ** 31 - 1):
            assert fn(n_max=n_max, labels=A + 2) != 0 and "n_max must be in [0, 2^31 - 1)" in err(), (fn.__name__, n_max)
        assert fn(labels=A + 2) != 0 and "aligned" in err(), fn.__name__
    for kw in (dict(Z=0), dict(Z=-1)):
        assert moments(**kw) != 0 and "extents must be at least 1" in err() and faces(**kw) != 0 and "extents must be at least 1" in err()
    assert moments(Z=2048, Y=1024, X=1024) != 0 and "2^31 voxels or more" in err()
    assert moments(cov=None, area=None, sums=None, Z=0) != 0 and "extents" in err()             # without cov the area and the sums are not asked for
    for kw in (dict(area=A + 1), dict(sums=A + 4), dict(mom=A + 4), dict(cov=A + 2)):
        assert moments(**kw) != 0 and "aligned" in err(), kw
    assert faces(faces=A + 4) != 0 and "aligned" in err() and perimeter(classes=A + 2) != 0 and "aligned" in err()
    # the moments bound comes last: an unaligned pointer is named before it, and an aligned call at the bound is refused by it
    E = R.longest_row()
    assert E == 2 ** 21
    assert moments(Z=1, Y=1, X=E + 1, mom=A + 4) != 0 and "aligned" in err()
    for shape in ((1, 1, E + 1), (E + 1, 1, 1), (1, 16384, 131071), (2, 1024, 1048575)):
        n, emax = math.prod(shape), max(shape)
        assert n * (emax - 1) ** 2 >= 2 ** 63 and n < 2 ** 31
        assert moments(Z=shape[0], Y=shape[1], X=shape[2]) != 0 and "must stay below 2^63" in err(), shape
    # faces and the perimeter classes have no such bound: the largest row passes every check but the last one made here
    assert faces(Z=1, Y=1, X=2 ** 31 - 1, n_max=2 ** 31 - 2, faces=A + 4) != 0 and "aligned" in err()
    assert perimeter(Y=1, X=2 ** 31 - 1, n_max=2 ** 31 - 2, classes=A + 2) != 0 and "aligned" in err()


def test_prepost_refuses_before_any_launch():
    from biapy_amd import prepost

    a = torch.zeros(4, 5, 6, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        prepost.shape_props(a)
    with pytest.raises(RuntimeError, match="no CPU path"):
        prepost.shape_props(a[0], 3)
    for dt in (torch.int64, torch.uint8, torch.float32, torch.int16):
        with pytest.raises(NotImplementedError, match="int32 labels"):
            prepost.shape_props(a.to(dt), 3)
    for bad in (a.view(-1), a[None], a[0, 0, 0]):
        with pytest.raises(ValueError, match="2-D .* or 3-D"):
            prepost.shape_props(bad, 3)
    for num in (-1, -100, torch.tensor(-2)):
        with pytest.raises(ValueError, match="num must not be negative"):
            prepost.shape_props(a.view(-1), num)                                           # the first refusal wins
    E = R.longest_row()
    row = torch.zeros((1, 1, E + 1), dtype=torch.int64)                                      # the bound is named before the dtype and the device
    for bad in (row, row.view(E + 1, 1, 1), row.view(1, E + 1)):
        with pytest.raises(NotImplementedError, match=r"n \* \(Emax - 1\)\^2 >= 2\^63"):
            prepost.shape_props(bad, 1)
    with pytest.raises(NotImplementedError, match="int32 labels"):
        prepost.shape_props(row[:, :, :E], 1)                                              # admitted by the bound
    assert prepost.moments_fit((1, 1, E)) and not prepost.moments_fit((1, 1, E + 1)) and prepost.moments_fit((1290, 1290, 1290))
    assert prepost.moments_fit((2 ** 15 - 1, 2 ** 16)) and not prepost.moments_fit((2 ** 14, 2 ** 17 - 1)) and prepost.moments_fit((0, 5, 6))
    assert prepost.ShapeProps._fields == ("area", "bbox", "coord_sum", "centroid", "moments", "covariance", "faces", "perimeter_classes")
    assert prepost.ShapeProps._fields[:4] == prepost.RegionProps._fields


def _props(nd, n=3):
    """A ShapeProps of CPU tensors: the derived calls are torch expressions and run anywhere."""
    from biapy_amd import prepost

    z = torch.zeros
    return prepost.ShapeProps(z(n, dtype=torch.int32), z(n, 2 * nd, dtype=torch.int32), z(n, nd, dtype=torch.int64), z(n, nd, dtype=torch.float64),
                              z(n, 6 if nd == 3 else 3, dtype=torch.int64), z(n, nd, nd, dtype=torch.float64), z(n, nd, dtype=torch.int64),
                              z(n, 3, dtype=torch.int32) if nd == 2 else None)


def test_the_derived_calls_refuse():
    from biapy_amd import prepost

    rp = prepost.RegionProps(*_props(3)[:4])
    for fn in (prepost.principal_moments, prepost.axis_lengths, prepost.elongation, prepost.surface_area, prepost.perimeter, prepost.circularity,
               prepost.sphericity):
        for bad in (rp, None, torch.zeros(3)):
            with pytest.raises(TypeError, match="takes the ShapeProps of shape_props"):
                fn(bad)
    for fn in (prepost.perimeter, prepost.circularity):
        with pytest.raises(ValueError, match="2-D labels only"):
            fn(_props(3))
    with pytest.raises(ValueError, match="3-D labels only"):
        prepost.sphericity(_props(2))
    for fn, nd in ((prepost.surface_area, 2), (prepost.surface_area, 3), (prepost.sphericity, 3)):
        for bad in ((1.0,) * (nd + 1), (1.0,) * (nd - 1), (0.0,) * nd, (-1.0,) + (1.0,) * (nd - 1), (float("nan"),) * nd, (float("inf"),) * nd):
            with pytest.raises(ValueError, match=f"sampling must be {nd} finite positive numbers"):
                fn(_props(nd), bad)


# ---- the twins against independent statements ---------------------------------------------------------------------------------------------------------

def _bincount_exact(ids, w, rows):
    """sum of the non-negative int64 weights per id through np.bincount, whose weights are float64: the weights are split at 2^21, so that every
    partial sum of at most 2^22 terms below 2^21 (or 2^42 / 2^21) stays below 2^53 and is exact."""
    assert len(ids) <= 2 ** 22 and (w >= 0).all() and (w < 2 ** 42).all()
    lo = np.bincount(ids, weights=(w & (2 ** 21 - 1)).astype(np.float64), minlength=rows)[:rows]
    hi = np.bincount(ids, weights=(w >> 21).astype(np.float64), minlength=rows)[:rows]
    return hi.astype(np.int64) * 2 ** 21 + lo.astype(np.int64)


def moments_by_bincount(labels, n_max):
    c = R.clean(labels, n_max).ravel()
    grids = [g.ravel() for g in np.indices(labels.shape)]
    pairs = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)] if labels.ndim == 3 else [(0, 0), (1, 1), (0, 1)]
    out = np.stack([_bincount_exact(c, grids[a].astype(np.int64) * grids[b], n_max + 1) for a, b in pairs], 1)
    out[0] = 0
    return out


def faces_by_shifts(labels, n_max, split_at=None):
    """Shifted-array comparisons on the volume padded with -1.  ``split_at``: the seeded defect - a cut of every row after x = split_at counts as a
    face on both sides, as an implementation that took the ends of its runs for faces would."""
    c = R.clean(labels, n_max)
    p = np.pad(c, 1, constant_values=-1)
    inner = tuple(slice(1, -1) for _ in range(c.ndim))
    out = np.zeros((n_max + 1, c.ndim), np.int64)
    for k in range(c.ndim):
        before = tuple(slice(0, -2) if j == k else slice(1, -1) for j in range(c.ndim))
        after = tuple(slice(2, None) if j == k else slice(1, -1) for j in range(c.ndim))
        count = (p[before] != p[inner]).astype(np.int64) + (p[after] != p[inner])
        if split_at is not None and k == c.ndim - 1 and c.shape[-1] > split_at + 1:
            same = c[..., split_at] == c[..., split_at + 1]
            count[..., split_at] += same
            count[..., split_at + 1] += same
        out[:, k] = np.bincount(c.ravel(), weights=count.ravel(), minlength=n_max + 1)[:n_max + 1]
    out[0] = 0
    return out


def perimeter_classes_by_scipy(labels, n_max):
    """scikit-image's perimeter(neighborhood=4) restated with SciPy, per label: the border is the image minus its erosion by the 4-neighbourhood
    (border_value 0), the code image its convolution with [[10, 2, 10], [2, 1, 2], [10, 2, 10]] (constant 0 outside), the histogram of the codes
    split into the three weight classes."""
    from scipy import ndimage

    c = R.clean(labels, n_max)
    out = np.zeros((n_max + 1, 3), np.int32)
    cross = ndimage.generate_binary_structure(2, 1)
    kernel = np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]])
    for l in np.unique(c[c > 0]):
        image = (c == l).astype(np.uint8)
        border = image - ndimage.binary_erosion(image, cross, border_value=0).astype(np.uint8)
        hist = np.bincount(ndimage.convolve(border, kernel, mode="constant", cval=0).ravel(), minlength=50)
        out[l] = [hist[[5, 7, 15, 17, 25, 27]].sum(), hist[[21, 33]].sum(), hist[[13, 23]].sum()]
    return out


@pytest.mark.parametrize("name", list(R.cases()), ids=str)
def test_the_twins_agree_with_independent_statements_on_every_gpu_input(name):
    labels, n_max = R.cases()[name]
    want = R.ref(name)
    np.testing.assert_array_equal(want["moments"], moments_by_bincount(labels, n_max))
    np.testing.assert_array_equal(want["faces"], faces_by_shifts(labels, n_max))
    if labels.ndim == 2:
        np.testing.assert_array_equal(want["perimeter_classes"], perimeter_classes_by_scipy(labels, n_max))
        assert want["perimeter_classes"].dtype == np.int32
    else:
        assert want["perimeter_classes"] is None
    assert want["moments"].dtype == np.int64 and want["faces"].dtype == np.int64 and want["covariance"].dtype == np.float64
    absent = want["area"] == 0
    assert not want["moments"][absent].any() and not want["faces"][absent].any() and not want["covariance"][absent].any()


@pytest.mark.parametrize("name", list(R.cases()), ids=str)
def test_the_covariance_twin_lies_within_its_bound_of_the_exact_value(name):
    want = R.ref(name)
    cov = want["covariance"]
    for l in np.flatnonzero(want["area"])[:300]:                                             # 300 labels a case: Fractions are slow
        for (a, b), exact in R.covariance_exact(want["area"], want["coord_sum"], want["moments"], l).items():
            got = Fraction(float(cov[l, a, b]))
            assert abs(got - exact) <= R.COV_BOUND * abs(exact), (name, l, a, b)
            assert cov[l, a, b] == cov[l, b, a] and (a != b or cov[l, a, a] >= 0)


def test_the_numerator_needs_more_than_64_bits_and_the_sequence_survives_it():
    """The longest admitted row: A = 2^21, sum xx about 2^62.6, so A * S_xx is about 2^83.6; the exact variance is (E^2 - 1) / 12."""
    E = R.longest_row()
    A, S, Sxx = E, E * (E - 1) // 2, (E - 1) * E * (2 * E - 1) // 6
    assert R.numerator(A, Sxx, S, S) == E * E * (E * E - 1) // 12 > 2 ** 80
    assert abs(Fraction(R.cov_entry(A, Sxx, S, S)) - Fraction(E * E - 1, 12)) <= R.COV_BOUND * Fraction(E * E - 1, 12)
    assert R.cov_entry(3, 12, 6, 6) == 0.0 and R.cov_entry(0, 0, 0, 0) == 0.0 and R.cov_entry(2, 0, 1, 1) == -0.25      # a negative numerator keeps its sign


_eig_rows = {}


def test_closed_form_eigenvalues_against_eigvalsh_on_every_gpu_input():
    """The largest deviation in units of 2^-52 * trace goes to profiles/shapeprops_values.txt; the bound is 4 x the value measured when the twin
    was written (R.EIG_MEASURED)."""
    worst, where = 0.0, ""
    for name in R.cases():
        cov = R.ref(name)["covariance"]
        lam = R.principal_moments_ref(cov)
        assert (lam >= 0).all() and (np.diff(lam, axis=1) <= 0).all(), name
        _eig_rows[name] = R.eig_deviation(cov, lam)
        if _eig_rows[name] > worst:
            worst, where = _eig_rows[name], name
    print(f"closed-form eigenvalues: worst {worst:.3f} units of 2^-52 trace on {where!r}")
    try:
        with open(VALUES, "w") as f:
            f.write("tests/shapeprops_ref.principal_moments_ref against numpy.linalg.eigvalsh on the CPU: largest deviation in units of 2^-52 * trace\n")
            f.write(f"worst {worst:.3f} on {where!r}; EIG_MEASURED {R.EIG_MEASURED}, test bound 4 x that = {R.EIG_BOUND}\n")
            for k in sorted(_eig_rows):
                f.write(f"{_eig_rows[k]:9.3f}  {k}\n")
    except OSError:
        pass
    assert worst <= R.EIG_BOUND, (worst, where)


# ---- hand-made cases -------------------------------------------------------------------------------------------------------------------------------------

def test_a_single_voxel_a_rod_and_a_full_cube():
    one = np.zeros((3, 4, 5), np.int32)
    one[1, 2, 3] = 1
    r = R.shape_props_ref(one, 1)
    assert r["moments"][1].tolist() == [1, 4, 9, 2, 3, 6] and r["faces"][1].tolist() == [2, 2, 2] and not r["covariance"].any()
    lam = R.principal_moments_ref(r["covariance"])
    assert not lam.any() and np.isnan(R.derived_ref(r["area"], lam, r["faces"])["elongation"]).all()
    L = 30
    rod = np.ones((1, 1, L), np.int32)
    r = R.shape_props_ref(rod, 1)
    assert r["moments"][1].tolist() == [0, 0, (L - 1) * L * (2 * L - 1) // 6, 0, 0, 0] and r["faces"][1].tolist() == [2 * L, 2 * L, 2]
    assert r["covariance"][1].tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, (L * L - 1) / 12]]
    lam = R.principal_moments_ref(r["covariance"])
    d = R.derived_ref(r["area"], lam, r["faces"])
    assert abs(lam[1, 0] - (L * L - 1) / 12) <= R.EIG_BOUND * 2.0 ** -52 * (L * L - 1) / 12 and lam[1, 1:].tolist() == [0, 0]
    assert np.isinf(d["elongation"][1]) and d["surface_area"][1] == 4 * L + 2 and np.isclose(d["axis_lengths"][1, 0], np.sqrt(20 * (L * L - 1) / 12), rtol=1e-14)
    flat = R.shape_props_ref(np.ones((1, L)), 1)                                              # the same rod as a 2-D image
    assert flat["moments"][1].tolist() == [0, (L - 1) * L * (2 * L - 1) // 6, 0] and flat["faces"][1].tolist() == [2 * L, 2]
    assert np.isinf(R.derived_ref(flat["area"], R.principal_moments_ref(flat["covariance"]), flat["faces"], flat["perimeter_classes"])["elongation"][1])
    for E in (2, 7, 12):
        r = R.shape_props_ref(np.ones((E, E, E), np.int32), 1)
        assert r["covariance"][1].tolist() == [[(E * E - 1) / 12 if a == b else 0 for b in range(3)] for a in range(3)]
        assert r["faces"][1].tolist() == [2 * E * E] * 3
        d = R.derived_ref(r["area"], R.principal_moments_ref(r["covariance"]), r["faces"])
        assert abs(d["elongation"][1] - 1.0) < 1e-14 and abs(d["sphericity"][1] - (math.pi / 6) ** (1 / 3)) < 1e-15
        assert R.derived_ref(r["area"], R.principal_moments_ref(r["covariance"]), r["faces"], sampling=(2, 3, 5))["surface_area"][1] == 2 * E * E * 31


def test_two_labels_sharing_a_face_and_a_label_touching_every_border():
    v = np.zeros((2, 3, 6), np.int32)
    v[:, :, :3], v[:, :, 3:] = 1, 2                                                           # two 2 x 3 x 3 blocks that share a 2 x 3 face: it counts for both
    r = R.shape_props_ref(v, 2)
    assert r["faces"].tolist() == [[0, 0, 0], [18, 12, 12], [18, 12, 12]]
    assert r["faces"][1:].sum() == R.shape_props_ref((v > 0).astype(np.int32), 1)["faces"][1].sum() + 2 * 6
    frame = np.zeros((5, 6, 7), np.int32)
    frame[0], frame[-1], frame[:, 0], frame[:, -1], frame[:, :, 0], frame[:, :, -1] = 1, 1, 1, 1, 1, 1      # a hollow box on every border
    r = R.shape_props_ref(frame, 1)
    np.testing.assert_array_equal(r["faces"], faces_by_shifts(frame, 1))
    assert r["faces"][1].tolist() == [2 * 6 * 7 + 2 * 4 * 5, 2 * 5 * 7 + 2 * 3 * 5, 2 * 5 * 6 + 2 * 3 * 4]                 # outside and the cavity's walls
    assert r["bbox"][1].tolist() == [0, 0, 0, 5, 6, 7]
    ring = np.zeros((6, 7), np.int32)
    ring[0], ring[-1], ring[:, 0], ring[:, -1] = 1, 1, 1, 1
    np.testing.assert_array_equal(R.perimeter_classes_ref(ring, 1), perimeter_classes_by_scipy(ring, 1))
    assert R.perimeter_classes_ref(ring, 1)[1].sum() == 22                                   # every pixel of the ring is a border pixel with two neighbours in it


# ---- seeded defects the comparators must catch --------------------------------------------------------------------------------------------------------

def _differs(a, b):
    return not np.array_equal(a, b)


def test_the_comparators_catch_seeded_defects():
    labels, n_max = R.cases()["runs (9, 21, 37) L7"]
    want = R.ref("runs (9, 21, 37) L7")
    # a run split counted as a face: rows cut after x = 15, as a lane or trip end would cut them
    assert _differs(want["faces"], faces_by_shifts(labels, n_max, split_at=15))
    one, _ = R.cases()["one label 1 x 1 x 70000"]
    assert faces_by_shifts(one, 1, split_at=255)[1].tolist() == [140000, 140000, 4] and R.ref("one label 1 x 1 x 70000")["faces"][1, 2] == 2
    # a dropped x0 * L * (L - 1) term of the closed form: sum xx from runs, with and without it
    def sum_xx_by_runs(drop):
        out = np.zeros(n_max + 1, np.int64)
        c = R.clean(labels, n_max)
        for row in c.reshape(-1, c.shape[-1]):
            edges = np.flatnonzero(np.diff(row)) + 1
            for x0, x1 in zip(np.r_[0, edges], np.r_[edges, len(row)]):
                L = int(x1 - x0)
                out[row[x0]] += L * x0 * x0 + (0 if drop else x0 * L * (L - 1)) + (L - 1) * L * (2 * L - 1) // 6
        out[0] = 0
        return out
    np.testing.assert_array_equal(sum_xx_by_runs(False), want["moments"][:, 2])
    assert _differs(sum_xx_by_runs(True), want["moments"][:, 2])
    # swapped zy and zx
    swapped = want["moments"][:, [0, 1, 2, 4, 3, 5]]
    assert _differs(swapped, moments_by_bincount(labels, n_max))
    assert _differs(R.covariance_ref(want["area"], want["coord_sum"], swapped).view(np.int64), want["covariance"].view(np.int64))


# ---- the compiled kernels ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc to cross-compile the kernels to ISA")
def test_no_kernel_uses_scratch(tmp_path):
    out = str(tmp_path / "shapeprops.s")
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-result", "-S", "--cuda-device-only",   # the Makefile's flags
           os.path.join(ROOT, "biapy_amd", "csrc", "shapeprops.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)} failed:\n{r.stderr[-3000:]}"
    kernels = re.findall(r"\.name:\s+(_Z\w*sp_\w*kernel\w*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", open(out).read())
    assert sorted(re.search(r"sp_\w+?_kernel", k).group(0) for k, _ in kernels) == ["sp_faces_kernel", "sp_finish_kernel", "sp_moments_kernel",
                                                                                   "sp_perimeter_kernel", "sp_zero_kernel"], kernels
    for name, private in kernels:
        assert int(private) == 0, f"{name} keeps {private} bytes of scratch per lane"

"""The statement of ``bpx_region_moments`` / ``bpx_region_faces`` / ``bpx_region_perimeter2d`` (include/biapy_amd.h) and of the derived measures
of ``prepost.shape_props`` in NumPy, written from the header's text: one visit per voxel, ``np.add.at`` into integer arrays.  Shared by
test_shapeprops_cpu.py (which holds it against ``np.bincount``, shifted-array comparisons and the SciPy restatement of scikit-image's perimeter)
and test_shapeprops_gpu.py (which holds the device against it bit for bit); also the inputs both files use.

THE COVARIANCE BOUND.  ``covariance_ref`` repeats csrc/shapeprops_core.h's sequence: the numerator ``N = A * S_ab - S_a * S_b`` as a Python int
(exact), ``|N| = hi * 2^64 + lo``, ``d = float(hi) * 2.0**64 + float(lo)``, the sign, ``(d / float(A)) / float(A)``.  ``hi < 2^30`` so
``float(hi)`` and its product with 2^64 are exact; ``float(lo)`` rounds once (relative error <= u = 2^-53 of ``lo <= |N|``), the sum rounds once,
each division rounds once, ``float(A)`` is exact (A < 2^31); nothing underflows (a nonzero ``|N| / A^2 >= 2^-62``).  Four roundings:
``|cov - N / A^2| <= ((1 + u)^4 - 1) * |N / A^2|`` = COV_BOUND, held as an exact Fraction against the exact ``Fraction(N, A * A)``.

THE EIGENVALUE BOUND.  ``principal_moments_ref`` is the closed form ``prepost.principal_moments`` uses; its largest deviation from
``numpy.linalg.eigvalsh`` over every input of the tests, in units of ``2^-52 * trace``, was measured on the CPU (EIG_MEASURED, recorded in
profiles/shapeprops_values.txt by test_shapeprops_cpu.py); the tests allow 4 x that, since the trigonometric form loses accuracy for near-equal
eigenvalues.  The measured value is large, 4.1e-9 * trace: the 1000-label inputs hold many objects of two or three voxels on a slanted line,
whose two zero eigenvalues the arc cosine near 1 resolves only to the square root of the rounding error.  Objects whose eigenvalues are
well apart, and objects flat along an axis (reduced to the 2 x 2 form), come out to a few units."""
import math
from fractions import Fraction

import numpy as np

import regionprops_ref as RP

U = Fraction(1, 2 ** 53)
COV_BOUND = (1 + U) ** 4 - 1
EIG_MEASURED = 18264718.688              # units of 2^-52 * trace (4.1e-9 * trace), on 'runs (3, 70, 130) L1000'; profiles/shapeprops_values.txt
EIG_BOUND = 4 * EIG_MEASURED
PERIMETER_WEIGHTS = (1.0, math.sqrt(2.0), (1.0 + math.sqrt(2.0)) / 2.0)
CLASS_OF_CODE = np.full(50, -1, np.int64)
CLASS_OF_CODE[[5, 7, 15, 17, 25, 27]] = 0
CLASS_OF_CODE[[21, 33]] = 1
CLASS_OF_CODE[[13, 23]] = 2


def clean(labels, n_max):
    """The label every voxel counts for: itself inside 1..n_max, else background 0."""
    labels = np.asarray(labels).astype(np.int64)
    return np.where((labels > 0) & (labels <= n_max), labels, 0)


def moments_ref(labels, n_max):
    """int64 (N+1, 6): the sums of zz, yy, xx, zy, zx, yx per label; (N+1, 3) for a 2-D array: yy, xx, yx."""
    c = clean(labels, n_max)
    nd = c.ndim
    take = c.ravel() > 0
    ids = c.ravel()[take]
    co = [g.ravel()[take].astype(np.int64) for g in np.indices(c.shape)]
    pairs = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)] if nd == 3 else [(0, 0), (1, 1), (0, 1)]
    out = np.zeros((n_max + 1, len(pairs)), np.int64)
    for k, (a, b) in enumerate(pairs):
        np.add.at(out[:, k], ids, co[a] * co[b])
    return out


def faces_ref(labels, n_max):
    """int64 (N+1, ndim): per axis the (voxel, direction) pairs of each label whose neighbour is outside the array or carries another label."""
    c = clean(labels, n_max)
    out = np.zeros((n_max + 1, c.ndim), np.int64)
    take = c > 0
    for k in range(c.ndim):
        m = np.moveaxis(c, k, 0)
        count = np.full(m.shape, 2, np.int64)                     # both neighbours differ until shown equal
        same = m[1:] == m[:-1]
        count[1:] -= same                                         # the neighbour before
        count[:-1] -= same                                        # the neighbour after
        count = np.moveaxis(count, 0, k)
        np.add.at(out[:, k], c[take], count[take])
    return out


def perimeter_classes_ref(labels, n_max):
    """int32 (N+1, 3) of a 2-D array: the border pixels of each label in the three weight classes of scikit-image's perimeter(neighborhood=4)."""
    c = clean(labels, n_max)
    assert c.ndim == 2
    Y, X = c.shape
    p = np.pad(c, 2)                                              # background around the image
    mid = p[1:-1, 1:-1]                                           # the image with one ring
    border = (mid > 0) & ((p[:-2, 1:-1] != mid) | (p[2:, 1:-1] != mid) | (p[1:-1, :-2] != mid) | (p[1:-1, 2:] != mid))
    code = np.ones((Y, X), np.int64)
    centre = mid[1:-1, 1:-1]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            nb = (slice(1 + dy, 1 + dy + Y), slice(1 + dx, 1 + dx + X))
            code += np.where(border[nb] & (mid[nb] == centre), 2 if dy == 0 or dx == 0 else 10, 0)
    cls = np.where(border[1:-1, 1:-1], CLASS_OF_CODE[np.minimum(code, 49)], -1)
    out = np.zeros((n_max + 1, 3), np.int64)
    np.add.at(out, (c[cls >= 0], cls[cls >= 0]), 1)
    return out.astype(np.int32)


def numerator(A, Sab, Sa, Sb):
    return int(A) * int(Sab) - int(Sa) * int(Sb)


def cov_entry(A, Sab, Sa, Sb):
    """One entry of the covariance by the float sequence of csrc/shapeprops_core.h."""
    if A == 0:
        return 0.0
    N = numerator(A, Sab, Sa, Sb)
    mag = abs(N)
    d = float(mag >> 64) * 18446744073709551616.0 + float(mag & (2 ** 64 - 1))
    if N < 0:
        d = -d
    return d / float(A) / float(A)


def _pair_columns(nd):
    """{(a, b): column of the moments} for a <= b."""
    return {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (0, 2): 4, (1, 2): 5} if nd == 3 else {(0, 0): 0, (1, 1): 1, (0, 1): 2}


def covariance_ref(area, sums, moments):
    """float64 (N+1, ndim, ndim) from the integer fields; zeros where the area is 0."""
    nd = sums.shape[1]
    col = _pair_columns(nd)
    out = np.zeros((len(area), nd, nd))
    for l in np.flatnonzero(area):
        for (a, b), k in col.items():
            out[l, a, b] = out[l, b, a] = cov_entry(area[l], moments[l, k], sums[l, a], sums[l, b])
    return out


def covariance_exact(area, sums, moments, l):
    """{(a, b): Fraction} of label l (area > 0)."""
    A = int(area[l])
    return {ab: Fraction(numerator(A, moments[l, k], sums[l, ab[0]], sums[l, ab[1]]), A * A) for ab, k in _pair_columns(sums.shape[1]).items()}


def _eig2(a, d, b):
    mid, half = (a + d) / 2, np.sqrt(((a - d) / 2) ** 2 + b * b)
    return mid + half, mid - half


def principal_moments_ref(cov):
    """The closed-form eigenvalues of symmetric 2 x 2 / 3 x 3 matrices, descending, never negative: prepost.principal_moments in NumPy, the
    reduction to 2 x 2 where an axis has no variance included."""
    c = np.asarray(cov, np.float64)
    if c.shape[1] == 2:
        return np.maximum(np.stack(_eig2(c[:, 0, 0], c[:, 1, 1], c[:, 0, 1]), 1), 0)
    a, d, f = c[:, 0, 0], c[:, 1, 1], c[:, 2, 2]
    b, e, g = c[:, 0, 1], c[:, 0, 2], c[:, 1, 2]
    q = (a + d + f) / 3
    p1 = b * b + e * e + g * g
    a0, d0, f0 = a - q, d - q, f - q
    s = np.sqrt((a0 * a0 + d0 * d0 + f0 * f0 + 2 * p1) / 6)
    det = a0 * (d0 * f0 - g * g) - b * (b * f0 - g * e) + e * (b * g - d0 * e)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.clip(np.where(s > 0, det / (2 * s * s * s), 0.0), -1, 1)
    phi = np.arccos(r) / 3
    hi = q + 2 * s * np.cos(phi)
    lo = q + 2 * s * np.cos(phi + 2 * math.pi / 3)
    lam = np.stack((hi, 3 * q - hi - lo, lo), 1)
    zero = np.zeros_like(q)
    for flat, (u, v, w) in ((a == 0, (d, f, g)), (d == 0, (a, f, e)), (f == 0, (a, d, b))):
        lam = np.where(flat[:, None], np.stack(_eig2(u, v, w) + (zero,), 1), lam)
    return -np.sort(-np.maximum(lam, 0), axis=1)


def eig_deviation(cov, lam):
    """The largest |lam - eigvalsh(cov)| over the rows in units of 2^-52 * trace (rows of trace 0 must agree exactly: they count as 0 or inf)."""
    want = np.linalg.eigvalsh(cov)[:, ::-1]
    trace = np.trace(cov, axis1=1, axis2=2)
    dev = np.abs(lam - np.maximum(want, 0)).max(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        units = np.where(trace > 0, dev / (trace * 2.0 ** -52), np.where(dev == 0, 0.0, np.inf))
    return float(units.max()) if len(units) else 0.0


def derived_ref(area, lam, faces, classes=None, sampling=None):
    """The derived measures from the fields in NumPy: a dict of float64 (N+1,) arrays (axis_lengths (N+1, ndim))."""
    nd = faces.shape[1]
    s = (1.0,) * nd if sampling is None else tuple(float(v) for v in sampling)
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        out["axis_lengths"] = 4 * np.sqrt(lam) if nd == 2 else np.sqrt(20 * lam)
        out["elongation"] = np.sqrt(lam[:, 0] / lam[:, -1])
        surface = sum(faces[:, k].astype(np.float64) * math.prod(s[j] for j in range(nd) if j != k) for k in range(nd))
        out["surface_area"] = surface
        if nd == 2:
            c = classes.astype(np.float64)
            per = c[:, 0] * PERIMETER_WEIGHTS[0] + c[:, 1] * PERIMETER_WEIGHTS[1] + c[:, 2] * PERIMETER_WEIGHTS[2]
            out["perimeter"] = per
            out["circularity"] = 4 * math.pi * area.astype(np.float64) / per ** 2
        else:
            v = area.astype(np.float64) * math.prod(s)
            out["sphericity"] = math.pi ** (1.0 / 3.0) * (6 * v) ** (2.0 / 3.0) / surface
    return out


def shape_props_ref(labels, n_max):
    """Every field of ShapeProps for the labels 1..n_max as NumPy arrays: a dict."""
    labels = np.asarray(labels)
    area, sums, bbox = RP.region_props_ref(labels, n_max)
    mom = moments_ref(labels, n_max)
    return dict(area=area, bbox=bbox, coord_sum=sums, centroid=RP.centroid_ref(area, sums), moments=mom, covariance=covariance_ref(area, sums, mom),
                faces=faces_ref(labels, n_max), perimeter_classes=perimeter_classes_ref(labels, n_max) if labels.ndim == 2 else None)


def longest_row():
    """The longest 1 x 1 x E row the moments bound admits: the largest E with E * (E - 1)**2 < 2**63, found from the rule by bisection."""
    lo, hi = 1, 2 ** 31
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if mid * (mid - 1) ** 2 < 2 ** 63 else (lo, mid)
    return lo


def blocks(shape, n_labels, cell, seed):
    """Compact objects: every cell x cell (x cell) block of the array draws one label of 0..n_labels, about a third background."""
    rng = np.random.default_rng(seed)
    small = tuple(-(-s // cell) for s in shape)
    ids = np.where(rng.random(small) < 0.35, 0, rng.integers(1, max(n_labels, 1) + 1, size=small))
    for k in range(len(shape)):
        ids = np.repeat(ids, cell, axis=k)
    return np.ascontiguousarray(ids[tuple(slice(0, s) for s in shape)]).astype(np.int32)


SHAPES = [(9, 21, 37), (3, 70, 130), (8, 16, 64), (37, 41)]
LABEL_COUNTS = (0, 1, 7, 1000)                      # 1000 labels overflow a block's 256-slot table
ONE_VOXEL_AXES = [(1, 12, 20), (12, 1, 20), (12, 20, 1), (1, 1, 40), (1, 40, 1), (40, 1, 1), (1, 40), (40, 1)]
ROW_LENGTHS = (63, 64, 65, 255, 256, 257)

_CASES = {}


def cases():
    """{name: (labels, n_max)}: every input the GPU tests hold against the twin, built once per process and never written to."""
    if _CASES:
        return _CASES
    for shape in SHAPES:
        for k in LABEL_COUNTS:
            _CASES[f"runs {shape} L{k}"] = (RP.run_labels(shape, k, 17 * k + len(shape)), k)
    for shape in ONE_VOXEL_AXES:
        _CASES[f"runs {shape} L7"] = (RP.run_labels(shape, 7, sum(shape)), 7)
    for x in ROW_LENGTHS:
        _CASES[f"one label 2 x {x}"] = (np.full((2, x), 3, np.int32), 3)
        _CASES[f"runs 2 x 3 x {x}"] = (RP.run_labels((2, 3, x), 7, x), 7)
    for shape in ((37, 41), (64, 64), (5, 3), (1, 9), (6, 10, 14)):
        _CASES[f"blocks {shape}"] = (blocks(shape, 9, 3, sum(shape)), 9)
    _CASES["one label 1 x 1 x 70000"] = (np.full((1, 1, 70_000), 1, np.int32), 1)
    _CASES["one label 1 x 1 x 1100000"] = (np.full((1, 1, 1_100_000), 2, np.int32), 2)
    _CASES["the longest row the moments bound admits"] = (np.full((1, 1, longest_row()), 1, np.int32), 1)
    _CASES["8192 voxels, each its own label"] = ((8192 - np.arange(8192, dtype=np.int32)).reshape(4, 32, 64), 8192)
    _CASES["n_max 0 under labels"] = (RP.run_labels((9, 21, 37), 7, 5), 0)
    _CASES["all background"] = (np.zeros((9, 21, 37), np.int32), 5)
    _CASES["labels above num, negative labels"] = (RP.run_labels((9, 21, 37), 7, 6), 4)
    _CASES["full cube 7"] = (np.ones((7, 7, 7), np.int32), 1)
    # the perimeter's own: touching labels, labels on the image edge, one-pixel lines, a checkerboard of two labels
    t = np.zeros((20, 70), np.int32)
    t[2:12, 3:30], t[2:12, 30:50], t[12:18, 10:40] = 1, 2, 3
    _CASES["touching labels 20 x 70"] = (t, 3)
    e = np.zeros((18, 67), np.int32)
    e[:5, :9], e[13:, 60:], e[:, 30:33], e[8:11, :] = 1, 2, 3, 4
    _CASES["labels on the image edge 18 x 67"] = (e, 4)
    y, x = np.indices((17, 70))
    _CASES["one-pixel lines 17 x 70"] = (np.where(y % 3 == 0, 1, np.where(x % 5 == 0, 2, 0)).astype(np.int32), 2)
    _CASES["checkerboard of two labels 17 x 70"] = ((1 + ((x + y) & 1)).astype(np.int32), 2)
    for v in _CASES.values():
        v[0].setflags(write=False)
    return _CASES


_REFS = {}


def ref(name):
    """shape_props_ref of cases()[name], computed once per process."""
    if name not in _REFS:
        _REFS[name] = shape_props_ref(*cases()[name])
    return _REFS[name]

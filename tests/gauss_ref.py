"""The NumPy twin of ``prepost.separable_filter`` / ``gaussian_filter`` / ``gaussian_laplace`` (the rule in their docstrings, nothing of the
device's tiles or windows), the fp64 reference with its per-element bound, and the inputs the CPU and the GPU tests share.

THE TWIN.  Along an axis of ``n`` voxels with ``2 r + 1`` ``float32`` weights: ``acc = w[0] * v[f(i - r)]``, then ``acc = acc + w[j] * v[f(i + j
- r)]`` for ``j = 1 .. 2 r`` in that order - a Python loop over the taps whose products and sums are NumPy ``float32`` array operations (one IEEE
operation per element each, round to nearest, denormals kept).  ``f`` is the border fold in integer arithmetic: ``reflect`` ``d c b a | a b c
d`` (period ``2 n``), ``mirror`` ``d c b | a b c d`` (period ``2 n - 2``, ``n = 1`` maps to 0), ``nearest`` clamps, ``constant`` takes
``float32(cval)``.  The ``float32`` result of one axis is the input of the next, in axis order.

THE REFERENCE is ``scipy.ndimage.correlate1d`` chained in ``float64`` with the ``float64`` weights (for Gaussian weights:
``scipy.ndimage.gaussian_filter`` of the ``float64`` image).

THE BOUND on |twin - reference| per element, to first order in ``u = 2^-24``.  One pass computes, with ``n_a = 2 r_a + 1`` taps, the float32
weight ``w~_j = w_j (1 + d_j)``, ``|d_j| <= u`` (the weight's rounding), each product ``w~_j x~_j (1 + e_j)``, ``|e_j| <= u`` (one rounding),
and ``n_a - 1`` adds, each a factor ``(1 + g)``, ``|g| <= u``; a product passes through at most ``n_a - 1`` adds.  With ``x~ = v + b`` the
float32 input, ``v`` the fp64 intermediate and ``|b| <= B`` the error carried in, the output's error is at most

    sum_j |w_j| B_j  +  (1 + 1 + (n_a - 1)) u sum_j |w_j| |v_j|   <=   |w| (*) B  +  (n_a + 2) u (|w| (*) |v|)

(the derivation needs ``n_a + 1``; the statement keeps the ``n_a + 2`` it was given with, and the spare ``u`` absorbs the second-order terms) where ``(*)``
is the correlation in the same border mode, ``|cval|`` standing in for the constant of ``|v|`` and 0 for that of ``B`` (the test ``cval`` s are
float32 numbers).  A product that underflows loses up to one smallest denormal ``2^-149`` instead of a relative ``u``: one such term per tap
is added.  The bound is carried from pass to pass: ``B <- |w| (*) B + (n_a + 2) u (|w| (*) |v|) + n_a 2^-149``.  Derived, not tuned."""
import functools

import numpy as np

SHAPES = ((5, 9, 70), (3, 6, 131), (17, 70), (2, 3, 1), (1, 1, 200), (8, 16, 128))
SHORT_SHAPES = ((5, 9, 70), (3, 6, 131), (17, 70), (2, 3, 1))          # axes shorter than the halo of r = 32
KINDS = ("normal", "denormal", "impulse", "infinities", "constant")
MODES = (("reflect", 0.0), ("mirror", 0.0), ("nearest", 0.0), ("constant", 0.0), ("constant", 0.25))
U = 2.0 ** -24
TINY = 2.0 ** -149
MAX_RADIUS = 32


# ---- the weights: SciPy's _gaussian_kernel1d(sigma, order, radius)[::-1], restated -------------------------------------------------------------------

def gaussian_weights(sigma, order, radius):
    exponent_range = np.arange(order + 1)
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    phi_x = phi_x / phi_x.sum()
    if order == 0:
        return phi_x[::-1]
    q = np.zeros(order + 1)
    q[0] = 1
    D = np.diag(exponent_range[1:], 1)
    P = np.diag(np.ones(order) / -sigma2, -1)
    Q_deriv = D + P
    for _ in range(order):
        q = Q_deriv.dot(q)
    q = (x[:, None] ** exponent_range).dot(q)
    return (q * phi_x)[::-1]


def per_axis(value, ndim):
    return list(value) if isinstance(value, (tuple, list)) else [value] * ndim


def gaussian_axes(ndim, sigma, order=0, truncate=4.0, radius=None):
    """One float64 weight vector per axis, or None where SciPy skips the axis (sigma <= 1e-15)."""
    out = []
    for sd, o, r in zip(per_axis(sigma, ndim), per_axis(order, ndim), per_axis(radius, ndim)):
        sd = float(sd)
        if sd <= 1e-15:
            out.append(None)
            continue
        lw = int(truncate * sd + 0.5) if r is None else int(r)
        out.append(gaussian_weights(sd, int(o), lw))
    return out


# ---- the border ---------------------------------------------------------------------------------------------------------------------------------------

def fold(mode, i, n):
    """Source index of every entry of the integer array ``i`` on an axis of ``n`` voxels; -1 is the constant."""
    i = np.asarray(i, dtype=np.int64)
    inside = (i >= 0) & (i < n)
    if mode == "constant":
        return np.where(inside, i, -1)
    if mode == "nearest" or n == 1:
        return np.clip(i, 0, n - 1)
    if mode == "reflect":
        period = 2 * n
        r = np.mod(i, period)
        return np.where(r < n, r, period - 1 - r)
    assert mode == "mirror", mode
    period = 2 * n - 2
    r = np.mod(i, period)
    return np.where(r < n, r, period - r)


def _taps(v, axis, w, mode, cval, dtype):
    """The terms w[j] * v[f(i + j - r)] of every output along ``axis``, tap by tap, in ``dtype`` arithmetic."""
    n = v.shape[axis]
    r = (len(w) - 1) // 2
    const = np.asarray(cval, dtype=dtype)
    for j in range(len(w)):
        src = fold(mode, np.arange(n) + j - r, n)
        taken = np.take(v, np.where(src < 0, 0, src), axis=axis)
        if mode == "constant":
            shape = [1] * v.ndim
            shape[axis] = n
            taken = np.where((src < 0).reshape(shape), const, taken)
        yield dtype(w[j]) * taken


def correlate_axis(v, axis, w, mode, cval, dtype=np.float32):
    """One pass of the rule: the first tap is a product alone, the others are added in tap order."""
    w = np.asarray(w, dtype=dtype)
    acc = None
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for term in _taps(np.asarray(v, dtype=dtype), axis, w, mode, cval, dtype):
            acc = term if acc is None else acc + term
    assert acc.dtype == dtype
    return acc


def separable_ref(x, weights, mode="reflect", cval=0.0):
    """The twin of ``prepost.separable_filter``: ``weights`` one entry per axis (None, or the weights, rounded to float32 here)."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and len(weights) == x.ndim
    out = x.copy()
    for axis, w in enumerate(weights):
        if w is not None:
            out = correlate_axis(out, axis, np.asarray(w, dtype=np.float64).astype(np.float32), mode, np.float32(cval))
    return out


def gaussian_ref(x, sigma, order=0, mode="reflect", cval=0.0, truncate=4.0, radius=None):
    return separable_ref(x, gaussian_axes(np.asarray(x).ndim, sigma, order, truncate, radius), mode, cval)


def laplace_axes(ndim, sigma, truncate=4.0):
    return [gaussian_axes(ndim, sigma, [2 if a == axis else 0 for a in range(ndim)], truncate) for axis in range(ndim)]


def laplace_ref(x, sigma, mode="reflect", cval=0.0, truncate=4.0):
    """The twin of ``prepost.gaussian_laplace``: the terms added as float32 in axis order."""
    out = None
    with np.errstate(invalid="ignore", over="ignore"):
        for ws in laplace_axes(np.asarray(x).ndim, sigma, truncate):
            g = separable_ref(x, ws, mode, cval)
            out = g if out is None else out + g
    return out


# ---- the fp64 reference and the bound ---------------------------------------------------------------------------------------------------------------------

def reference_and_bound(x, weights, mode="reflect", cval=0.0):
    """(scipy.ndimage.correlate1d chained in float64 with the float64 ``weights``, the per-element bound of the module's docstring)."""
    import scipy.ndimage as ndi

    v = np.asarray(x, dtype=np.float64)
    B = np.zeros_like(v)
    with np.errstate(invalid="ignore", over="ignore"):
        for axis, w in enumerate(weights):
            if w is None:
                continue
            w = np.asarray(w, dtype=np.float64)
            n_a = len(w)
            aw = np.abs(w)
            B = (ndi.correlate1d(B, aw, axis, mode=mode, cval=0.0) + (n_a + 2) * U * ndi.correlate1d(np.abs(v), aw, axis, mode=mode, cval=abs(cval))
                 + n_a * TINY)
            v = ndi.correlate1d(v, w, axis, mode=mode, cval=cval)
    return v, B


def check_within(got, ref, bound, what=""):
    """``got`` (float32) within ``bound`` of ``ref`` wherever the bound is finite; elsewhere (an infinity went in) the same infinity, or NaN where
    the reference holds NaN.  Returns the largest error / bound over the finite part."""
    got = np.asarray(got, dtype=np.float64)
    ok = np.isfinite(bound) & np.isfinite(ref)
    err = np.abs(got[ok] - ref[ok])
    assert np.isfinite(got[ok]).all() and (err <= bound[ok]).all(), (what, float(np.max(err / bound[ok])) if ok.any() else None)
    rest_got, rest_ref = got[~ok], ref[~ok]
    nan = np.isnan(rest_ref)
    assert np.isnan(rest_got[nan]).all() and np.array_equal(rest_got[~nan], rest_ref[~nan]), (what, "non-finite part")
    return float(np.max(err / bound[ok])) if ok.any() else 0.0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, want, what=""):
    """Bit for bit through the integer view; where the twin holds a NaN the device holds a NaN (payloads are not compared)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), (what, "NaN expected")
    np.testing.assert_array_equal(bits(got)[~nan], bits(want)[~nan], err_msg=str(what))


# ---- inputs: built once per process, read-only --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def volume(kind, shape):
    rng = np.random.default_rng([7 + KINDS.index(kind), len(shape)] + list(shape))
    n = int(np.prod(shape))
    if kind == "normal":
        a = rng.standard_normal(n).astype(np.float32)
    elif kind == "denormal":                                                               # products with the weights are denormal
        a = (rng.standard_normal(n) * 1e-40).astype(np.float32)
    elif kind == "impulse":                                                                # the response is the weights themselves, reversed
        a = np.zeros(n, np.float32)
        a[n // 2] = 1.0
    elif kind == "infinities":
        a = rng.standard_normal(n).astype(np.float32)
        at = rng.permutation(n)[:max(2, n // 40)]
        a[at] = np.where(np.arange(at.size) % 2 == 0, np.inf, -np.inf).astype(np.float32)
    else:
        a = np.full(n, 0.75, np.float32)
    a = np.ascontiguousarray(a.reshape(shape))
    a.setflags(write=False)
    return a


# the parameter sets of the device tests: (name, shapes, keyword arguments of gaussian_filter)
def _fit(value, ndim):
    return tuple(value[3 - ndim:]) if isinstance(value, tuple) else value


def gaussian_cases():
    """(shape, kind, mode, cval, kwargs) of every device comparison of gaussian_filter with the twin."""
    for shape in SHAPES:
        nd = len(shape)
        for kind in KINDS:
            for mode, cval in MODES:
                yield shape, kind, mode, cval, dict(sigma=1.0)
        for kind in ("normal", "infinities"):
            for mode, cval in (("reflect", 0.0), ("constant", 0.25)):
                yield shape, kind, mode, cval, dict(sigma=_fit((0.0, 1.0, 3.0), nd))
                yield shape, kind, mode, cval, dict(sigma=_fit((2.0, 0.0, 0.0), nd) if nd == 3 else (2.0, 0.0))
                yield shape, kind, mode, cval, dict(sigma=1.5, order=1)
                yield shape, kind, mode, cval, dict(sigma=1.5, order=_fit((0, 2, 1), nd))
                yield shape, kind, mode, cval, dict(sigma=2.0, radius=3)
                yield shape, kind, mode, cval, dict(sigma=2.0, radius=_fit((1, 5, 2), nd))
                yield shape, kind, mode, cval, dict(sigma=3.0, truncate=2.0)
    for shape in SHORT_SHAPES:
        for kind in ("normal", "impulse"):
            for mode, cval in MODES:
                yield shape, kind, mode, cval, dict(sigma=8.0)


@functools.lru_cache(maxsize=None)
def blobs(shape, seed=5):
    """A smooth probability map with noise: what the 64^3 case and the pipelines filter."""
    import scipy.ndimage as ndi

    rng = np.random.default_rng(seed)
    a = ndi.gaussian_filter(rng.random(shape), 2.0)
    a = (a - a.min()) / (a.max() - a.min()) + 0.05 * rng.standard_normal(shape)
    a = a.astype(np.float32)
    a.setflags(write=False)
    return a

"""The host twin of ``prepost.intensity_props`` and the inputs the CPU and the GPU tests share.

The twin restates the product-defined semantics with NumPy integers and Python big integers, not with the device's code: a ``float32`` is an
integer ``m < 2^24`` times ``2^(q - 149)``; its two pieces go to the ``int64`` limbs ``q >> 5`` and ``(q >> 5) + 1``; the limbs of a label are
summed with integer adds (sort + ``np.add.reduceat``: exact); ``sum`` is ``V / 2**149`` with ``V = sum_j limbs[j] << 32 j`` a Python int, whose
true division rounds correctly (to nearest even) - the value ``math.fsum`` returns; ``mean`` is NumPy's float64 division.  ``min`` / ``max`` are
the extremes of the order-preserving ``uint32`` key over the voxels that are not NaN."""
import math
from fractions import Fraction

import numpy as np

NL_F32, NL_INT = 9, 1
FLT_MAX = np.float32(3.4028234663852886e38)
F32_NAN_BITS = 0x7FC00000


def clean(labels, n_max):
    c = np.asarray(labels).astype(np.int64)
    return np.where((c > 0) & (c <= n_max), c, 0)


def bits_of(image):
    return np.ascontiguousarray(image, dtype=np.float32).view(np.uint32).ravel()


def pieces(bits, drop_high=False):
    """(limb, lo, hi, cls) of float32 words: cls 0 finite, 1 NaN, 2 +inf, 3 -inf; limb -1 and no pieces unless finite.  ``drop_high``: the seeded
    defect - the piece for limb + 1 is forgotten."""
    bits = np.asarray(bits, dtype=np.uint32).astype(np.int64)
    E, f, neg = (bits >> 23) & 255, bits & 0x7FFFFF, (bits >> 31) != 0
    m = np.where(E == 0, f, f | 0x800000)
    q = np.where(E == 0, 0, E - 1)
    w = m << (q & 31)                                       # below 2^55
    lo, hi = w & 0xFFFFFFFF, w >> 32
    if drop_high:
        hi = np.zeros_like(hi)
    lo, hi = np.where(neg, -lo, lo), np.where(neg, -hi, hi)
    finite = E != 255
    cls = np.where(finite, 0, np.where(f != 0, 1, np.where(neg, 3, 2)))
    return np.where(finite, q >> 5, -1), np.where(finite, lo, 0), np.where(finite, hi, 0), cls


def okey(bits):
    bits = np.asarray(bits, dtype=np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def unokey(key):
    key = np.asarray(key, dtype=np.uint32)
    return np.where(key & np.uint32(0x80000000), key ^ np.uint32(0x80000000), ~key).astype(np.uint32)


def _by_label(c, values, rows, op, empty):
    """op.reduce of ``values`` over the voxels of every label 0..rows - 1 (``empty`` where there is none): a stable sort and ``reduceat``."""
    order = np.argsort(c, kind="stable")
    cs, vs = c[order], values[order]
    out = np.full(rows, empty, dtype=values.dtype)
    if cs.size:
        starts = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]])
        out[cs[starts]] = op.reduceat(vs, starts)
    return out


def limbs_value(limbs, unit=-149):
    """The exact value of a row of limbs as a Fraction."""
    v = sum(int(x) << (32 * j) for j, x in enumerate(limbs))
    return Fraction(v) * Fraction(2) ** unit


def round_limbs(limbs, unit=-149, truncate=False):
    """The float64 nearest (ties to even) to the limbs' exact value: Python's int / int division is correctly rounded.  ``truncate``: the
    seeded defect - the bits below the 53rd are cut off."""
    v = sum(int(x) << (32 * j) for j, x in enumerate(limbs))
    if truncate and v:
        a = abs(v)
        cut = max(a.bit_length() - 53, 0)
        v = (a >> cut << cut) * (1 if v > 0 else -1)
    return v / (1 << -unit) if unit < 0 else float(v << unit)


def sum_rule(rounded, nan, pinf, ninf):
    if nan or (pinf and ninf):
        return math.nan
    return math.inf if pinf else -math.inf if ninf else rounded


def intensity_props_ref(labels, image, n_max, drop_high=False, truncate=False, nan_in_min=False):
    """The twin: a dict of NumPy arrays with the fields of ``IntensityProps``.  The keyword arguments seed the three defects the comparisons of
    tests/test_intensityprops_cpu.py must catch."""
    image = np.asarray(image)
    c = clean(labels, n_max).ravel()
    rows = n_max + 1
    inside = c > 0
    c = c[inside]
    area = np.bincount(c, minlength=rows)[:rows].astype(np.int32)
    if image.dtype == np.float32:
        bits = bits_of(image)[inside]
        limb, lo, hi, cls = pieces(bits, drop_high)
        limbs = np.zeros((rows, NL_F32), np.int64)
        for j in range(NL_F32):
            limbs[:, j] = _by_label(c, np.where(limb == j, lo, 0) + np.where(limb + 1 == j, hi, 0), rows, np.add, 0)
        nonfinite = np.stack([np.bincount(c[cls == k], minlength=rows)[:rows] for k in (1, 2, 3)], 1).astype(np.int32)
        take = np.ones_like(cls, bool) if nan_in_min else cls != 1
        key = okey(bits)
        kmin = _by_label(c[take], key[take], rows, np.minimum, np.uint32(0xFFFFFFFF))
        kmax = _by_label(c[take], key[take], rows, np.maximum, np.uint32(0))
        seen = np.bincount(c[take], minlength=rows)[:rows] > 0
        lo_bits = np.where(seen, unokey(kmin), np.where(area > 0, F32_NAN_BITS, 0)).astype(np.uint32)
        hi_bits = np.where(seen, unokey(kmax), np.where(area > 0, F32_NAN_BITS, 0)).astype(np.uint32)
        vmin, vmax, unit = lo_bits.view(np.float32), hi_bits.view(np.float32), -149
    else:
        assert image.dtype in (np.uint8, np.uint16), image.dtype
        val = image.ravel().astype(np.int64)[inside]
        limbs = _by_label(c, val, rows, np.add, 0).reshape(rows, NL_INT)
        nonfinite = np.zeros((rows, 3), np.int32)
        vmin = np.where(area > 0, _by_label(c, val, rows, np.minimum, 0), 0).astype(np.int32)
        vmax = np.where(area > 0, _by_label(c, val, rows, np.maximum, 0), 0).astype(np.int32)
        unit = 0
    total = np.array([sum_rule(round_limbs(limbs[l], unit, truncate), *nonfinite[l]) if area[l] else 0.0 for l in range(rows)], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(area > 0, total / np.maximum(area, 1).astype(np.float64), np.nan)
    return dict(area=area, min=vmin, max=vmax, sum=total, mean=mean, sum_limbs=limbs, nonfinite=nonfinite)


FIELDS = ("area", "min", "max", "sum", "mean", "sum_limbs", "nonfinite")


def same_bits(a, b):
    """Equal as bit patterns (NaN payloads and the sign of zero included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def ulp_distance(a, b):
    """The largest distance in float64 ulps between the entries of a and b; NaN must meet NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)

    def line(x):                                            # the float64 line as ordered integers
        i = x.view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i)
    return int(np.abs(line(a[ok]) - line(b[ok])).max()) if ok.any() else 0


# ---- the shared inputs ---------------------------------------------------------------------------------------------------------------------------------

def blocks(shape, n_labels, cell, seed):
    """Labels 0..n_labels in cells of `cell` voxels along x (ragged against the 4 voxels of a lane and the 256 of a trip), shuffled."""
    rng = np.random.default_rng(seed)
    n = math.prod(shape)
    if n_labels == 0:
        return np.zeros(shape, np.int32)
    ids = rng.integers(0, n_labels + 1, size=n // cell + 1)
    return np.repeat(ids, cell)[:n].reshape(shape).astype(np.int32)


def from_bits(E, f, neg):
    return ((neg.astype(np.uint32) << 31) | (E.astype(np.uint32) << 23) | f.astype(np.uint32)).view(np.float32)


def image_of(kind, shape, seed):
    rng = np.random.default_rng(seed)
    n = math.prod(shape)
    if kind == "uniform":
        x = rng.random(n, dtype=np.float32)
    elif kind == "exponents":                               # the whole range: every exponent field 0..254, either sign
        x = from_bits(rng.integers(0, 255, n), rng.integers(0, 1 << 23, n), rng.integers(0, 2, n))
    elif kind == "boundaries":                              # q & 31 at 0, 8, 9, 30, 31: pieces that end at, straddle and start at a limb boundary
        q = rng.choice([31, 32, 40, 41, 62, 63, 64, 95, 96, 127, 128, 159, 160, 223, 224, 253], n)
        f = rng.choice([0, 1, 0x7FFFFF, 0x400000, 0x7FFFFE], n)
        x = from_bits(q + 1, f, rng.integers(0, 2, n))
    elif kind == "denormals":
        x = from_bits(np.zeros(n, np.int64), rng.integers(0, 1 << 23, n), rng.integers(0, 2, n))
    elif kind == "cancelling":                              # x and -x in shuffled places, over the whole range: exact zeros and near-zeros
        h = from_bits(rng.integers(0, 255, n), rng.integers(0, 1 << 23, n), np.zeros(n, np.int64))
        x = np.where(np.arange(n) % 2 == 0, h, -np.roll(h, 1))
    elif kind == "zeros":                                   # signed zeros, a few ones between them
        x = rng.choice(np.array([0.0, -0.0, -0.0, 0.0, 1.0], np.float32), n)
    elif kind == "nonfinite":                               # mixed into finite values
        x = rng.random(n, dtype=np.float32) - np.float32(0.5)
        r = rng.random(n)
        x[r < 0.02] = np.nan
        x[(r >= 0.02) & (r < 0.04)] = np.inf
        x[(r >= 0.04) & (r < 0.06)] = -np.inf
        x[(r >= 0.06) & (r < 0.07)] = from_bits(np.full(n, 255), np.full(n, 1), np.ones(n, np.int64))[(r >= 0.06) & (r < 0.07)]     # a signalling, negative NaN
    elif kind == "u8":
        return rng.integers(0, 256, n).astype(np.uint8).reshape(shape)
    elif kind == "u16":
        return rng.integers(0, 65536, n).astype(np.uint16).reshape(shape)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(x, dtype=np.float32).reshape(shape)


SHAPES = [(5, 7, 9), (3, 37, 41), (16, 32, 64), (37, 41)]
LABEL_COUNTS = (0, 1, 7, 1000)                      # 1000 labels overflow a block's 256-slot table
ONE_VOXEL_AXES = [(1, 12, 20), (12, 1, 20), (12, 20, 1), (1, 1, 40), (40, 1, 1), (1, 40), (40, 1)]
ROW_LENGTHS = (255, 256, 257, 8191, 8192, 8193)
KINDS = ("uniform", "exponents", "boundaries", "denormals", "cancelling", "zeros", "nonfinite", "u8", "u16")
BIG = 1 << 20

_CASES = {}


def cases():
    """name -> (labels, image, n_max)"""
    if _CASES:
        return _CASES
    seed = 0
    for shape in SHAPES:
        for k, n_labels in enumerate(LABEL_COUNTS):
            seed += 1
            kind = KINDS[seed % len(KINDS)]
            _CASES[f"{kind} {shape} L{n_labels}"] = (blocks(shape, n_labels, 3 if n_labels == 1000 else 11, seed), image_of(kind, shape, seed), n_labels)
    for kind in KINDS:                                  # every image kind on the shape with several blocks
        seed += 1
        _CASES[f"{kind} (16, 32, 64) L40"] = (blocks((16, 32, 64), 40, 7, seed), image_of(kind, (16, 32, 64), seed), 40)
        _CASES[f"{kind} (3, 37, 41) one label"] = (np.ones((3, 37, 41), np.int32), image_of(kind, (3, 37, 41), seed + 100), 1)
    for shape in ONE_VOXEL_AXES:
        seed += 1
        _CASES[f"one-voxel axes {shape}"] = (blocks(shape, 5, 3, seed), image_of("exponents", shape, seed), 5)
    for L in ROW_LENGTHS:
        seed += 1
        _CASES[f"two rows of {L}"] = (blocks((2, L), 3, 300, seed), image_of("boundaries", (2, L), seed), 3)
        _CASES[f"two rows of {L} one label"] = (np.ones((2, L), np.int32), image_of("uniform", (2, L), seed), 1)
    seed += 1
    _CASES["one label 1 x 1 x 70000"] = (np.ones((1, 1, 70000), np.int32), image_of("uniform", (1, 1, 70000), seed), 1)
    _CASES["one label 1 x 1 x 70000 u16"] = (np.ones((1, 1, 70000), np.int32), image_of("u16", (1, 1, 70000), seed), 1)
    own = np.arange(1, 4097, dtype=np.int32).reshape(1, 64, 64)
    _CASES["4096 voxels each its own label"] = (own, image_of("exponents", own.shape, seed), 4096)
    _CASES["all background"] = (np.zeros((3, 37, 41), np.int32), image_of("uniform", (3, 37, 41), seed), 6)
    lab = blocks((3, 37, 41), 9, 5, seed)
    _CASES["labels above num"] = (lab, image_of("exponents", lab.shape, seed), 4)
    neg = lab.copy()
    neg[::2, ::3] = -neg[::2, ::3] - 1
    neg[0, 0, 0] = -2 ** 31
    _CASES["negative labels"] = (neg, image_of("exponents", lab.shape, seed), 9)
    # +-FLT_MAX filling a label of 2^20 voxels each: 2^20 * FLT_MAX is past float32's range, a limb takes 2^20 pieces of almost 2^32
    two = np.repeat(np.array([1, 2], np.int32), BIG).reshape(2, 1024, 1024)
    _CASES["FLT_MAX in 2^20 voxels"] = (two, np.where(two == 1, FLT_MAX, -FLT_MAX).astype(np.float32), 2)
    _CASES["FLT_MAX cancelling in 2^21 voxels"] = (np.ones_like(two), np.where(two == 1, FLT_MAX, -FLT_MAX).astype(np.float32), 1)
    _CASES["uint16 65535 in 2^20 voxels"] = (two, np.where(two == 1, 65535, 7).astype(np.uint16), 2)
    # the non-finite table, one label per row of 300 voxels: (NaN), (+inf), (-inf), (+inf, -inf), (NaN, +inf), every voxel NaN, every voxel +inf, finite
    t = np.repeat(np.arange(1, 9, dtype=np.int32), 300).reshape(8, 300)
    x = image_of("uniform", t.shape, seed)
    x[0, 7], x[1, 255], x[2, 256], x[3, 0], x[3, 299], x[4, 1], x[4, 2] = np.nan, np.inf, -np.inf, np.inf, -np.inf, np.nan, np.inf
    x[5], x[6] = np.nan, np.inf
    _CASES["the non-finite table"] = (t, x, 8)
    return _CASES


def named(suffix):
    """The one case whose name ends with `suffix`."""
    (name,) = [k for k in cases() if k.endswith(suffix)]
    return name


_REFS = {}


def ref(name):
    if name not in _REFS:
        _REFS[name] = intensity_props_ref(*cases()[name])
    return _REFS[name]

"""The NumPy twin of ``prepost.median_filter`` (the definition in its docstring, nothing of the device's tiles or networks) and the inputs the
CPU and the GPU tests share.

The twin: pad the volume by half a window per axis (``np.pad`` with ``symmetric`` for "reflect", ``edge`` for "nearest", ``constant``), take
every window with ``sliding_window_view``, turn the values into their order-preserving ``uint32`` keys, ``np.partition`` the keys at ``W // 2``
and turn that key back into a value.  Bits in, bits out: ``-0.0`` sorts below ``+0.0`` and NaNs sort by their bits."""
import functools

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

SHAPES = ((5, 9, 70), (3, 6, 131), (8, 8, 64), (1, 17, 70), (17, 70), (6, 1, 66), (2, 3, 1), (1, 1, 1))
# W = 45 (3, 3, 5) and W = 21 (1, 3, 7) have no network of their own and run padded on the next larger one; so do 1, 121 and 35 ... of the rest
SIZES = (3, 5, (1, 3, 3), (1, 5, 5), (3, 3, 3), (5, 1, 1), (5, 5, 1), (1, 1, 7), (1, 7, 7), (3, 1, 5), (5, 5, 5), (1, 1, 15), (1, 11, 11), (3, 3, 5),
         (1, 3, 7), 1)
F32_MODES = (("reflect", 0.0), ("nearest", 0.0), ("constant", 0.0), ("constant", 0.25))
U8_MODES = (("reflect", 0), ("nearest", 0), ("constant", 0), ("constant", 1), ("constant", 255))
F32_KINDS = ("tie_free", "quantised", "signed_zeros", "infinities", "denormals", "nans", "constant")
U8_KINDS = ("full_range", "binary_0.1", "binary_0.5", "binary_0.9")
NP_MODE = {"reflect": "symmetric", "nearest": "edge", "constant": "constant"}


def per_axis(size, ndim):
    """``size`` for an ``ndim``-D input, or None when a (z, y, x) triple does not fit a 2-D one (its z entry is not 1)."""
    if isinstance(size, (tuple, list)):
        size = tuple(int(s) for s in size)
        if len(size) == ndim:
            return size
        return size[1:] if len(size) == ndim + 1 and size[0] == 1 else None
    return (int(size),) * ndim


def keys_of(a):
    """The order-preserving uint32 key of every element: float32 ``bits | 0x80000000`` for a clear sign bit, ``~bits`` otherwise; uint8 the value."""
    if a.dtype == np.uint8:
        return a.astype(np.uint32)
    assert a.dtype == np.float32
    bits = np.ascontiguousarray(a).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def values_of(keys, dtype):
    if dtype == np.uint8:
        return keys.astype(np.uint8)
    bits = np.where(keys & np.uint32(0x80000000), keys ^ np.uint32(0x80000000), ~keys).astype(np.uint32)
    return bits.view(np.float32)


def median_ref(x, size=3, mode="reflect", cval=0.0):
    x = np.asarray(x)
    if x.dtype == np.bool_:
        return median_ref(x.view(np.uint8), size, mode, cval).view(np.bool_)
    sizes = per_axis(size, x.ndim)
    assert sizes is not None and all(s % 2 == 1 for s in sizes)
    pad = [(s // 2, s // 2) for s in sizes]
    padded = np.pad(x, pad, mode="constant", constant_values=x.dtype.type(cval)) if mode == "constant" else np.pad(x, pad, mode=NP_MODE[mode])
    W = int(np.prod(sizes))
    windows = sliding_window_view(padded, sizes).reshape(x.shape + (W,))
    keys = np.partition(keys_of(windows), W // 2, axis=-1)[..., W // 2]
    return values_of(np.ascontiguousarray(keys), x.dtype).reshape(x.shape)


def median_axes_ref(x, axes, size):
    """``prepost.median_filter_axes``: ``size`` along the named axes of a (Z, Y, X) volume and 1 along the others; a list is applied in sequence."""
    if isinstance(axes, str):
        axes, size = [axes], [size]
    for a, s in zip(axes, size):
        x = median_ref(x, tuple(int(s) if ax in a else 1 for ax in "zyx"))
    return x


def scipy_median(x, size, mode, cval):
    import scipy.ndimage as ndi

    return ndi.median_filter(x, size=per_axis(size, x.ndim), mode=mode, cval=cval)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8)


# ---- inputs: built once per process, read-only --------------------------------------------------------------------------------------------------------

def _seed(shape, salt):
    return [salt, len(shape)] + list(shape)


@functools.lru_cache(maxsize=None)
def f32_input(kind, shape):
    rng = np.random.default_rng(_seed(shape, 11 + F32_KINDS.index(kind)))
    n = int(np.prod(shape))
    if kind == "tie_free":                                                                 # normals of both signs, no two equal
        a = (rng.permutation(n).astype(np.float32) - n // 2) / np.float32(7.0)
    elif kind == "quantised":                                                              # 8 levels: most windows hold ties
        a = np.floor(rng.random(n) * 8).astype(np.float32) / np.float32(8.0)
    elif kind == "signed_zeros":
        a = rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 0.5, -0.5], np.float32), n)
    elif kind == "infinities":
        a = rng.choice(np.array([-np.inf, -1.0, 0.0, 1.0, np.inf], np.float32), n)
    elif kind == "denormals":                                                              # below the smallest normal, both signs, with zeros
        a = (rng.integers(0, 6, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))).view(np.float32)
    elif kind == "nans":                                                                   # NaNs of both signs and several payloads among normals
        pool = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF, 0xFF800000, 0x7F800000], np.uint32).view(np.float32)
        a = rng.random(n).astype(np.float32) - np.float32(0.5)
        at = rng.random(n) < 0.3
        at[0] = True                                                                       # also the volume of one voxel holds a NaN
        a[at] = rng.choice(pool, int(at.sum()))
    else:
        a = np.full(n, 0.75, np.float32)
    a = np.ascontiguousarray(a.reshape(shape))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def u8_input(kind, shape):
    rng = np.random.default_rng(_seed(shape, 31 + U8_KINDS.index(kind)))
    if kind == "full_range":
        a = rng.integers(0, 256, shape, dtype=np.uint8)
    else:
        a = (rng.random(shape) < float(kind.split("_")[1])).astype(np.uint8)
    a.setflags(write=False)
    return a


def has_nan(a):
    return a.dtype == np.float32 and bool(np.isnan(a).any())


def cases(shape, dtype):
    """(input, kind, size, mode, cval) of every device comparison on `shape` with `dtype` (np.float32 or np.uint8)."""
    f32 = dtype == np.float32
    for kind in (F32_KINDS if f32 else U8_KINDS):
        x = f32_input(kind, shape) if f32 else u8_input(kind, shape)
        for size in SIZES:
            if per_axis(size, len(shape)) is None:
                continue
            for mode, cval in (F32_MODES if f32 else U8_MODES):
                yield x, kind, size, mode, cval


@functools.lru_cache(maxsize=None)
def probability(shape, seed=3):
    """A smooth map in 0..1 with salt noise: what the pipeline tests filter, threshold and label."""
    import scipy.ndimage as ndi

    rng = np.random.default_rng(seed)
    a = ndi.gaussian_filter(rng.random(shape), 2.0)
    a = (a - a.min()) / (a.max() - a.min())
    salt = rng.random(shape) < 0.05
    a[salt] = rng.random(int(salt.sum()))
    a = a.astype(np.float32)
    a.setflags(write=False)
    return a

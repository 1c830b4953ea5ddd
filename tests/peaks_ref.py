"""The NumPy twin of ``prepost.peak_local_max`` / ``peak_mask`` (the definition in their docstrings, nothing of the device's passes or lanes),
and the inputs the CPU and the GPU tests share.

The keys are ``uint64`` and their box maximum is taken by integer shifts with ``np.maximum``.  ``scipy.ndimage``'s filters are NOT used on the
keys: they work in float64, which drops the index bits below bit 11 - a twin written that way finds no peak at all."""
import functools

import numpy as np

SHAPES = ((9, 21, 37), (5, 6, 7), (37, 41), (1, 1, 300), (3, 70, 130))
RADII = (1, 2, (1, 2, 3), 4)


def per_axis(v, ndim):
    if isinstance(v, (tuple, list)):
        v = tuple(int(a) for a in v)
        return v[len(v) - ndim:] if len(v) >= ndim else (0,) * (ndim - len(v)) + v      # (rz, ry, rx) on a 2-D image: (ry, rx)
    return (int(v),) * ndim


def okey(img):
    """The order-preserving uint32 image of the values: int32 v + 2^31; float32 the sign-flip map."""
    bits = np.ascontiguousarray(img).view(np.uint32)
    if img.dtype == np.int32:
        return bits ^ np.uint32(0x80000000)
    assert img.dtype == np.float32
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def keys_of(img):
    index = np.arange(img.size, dtype=np.uint64).reshape(img.shape)
    return (okey(img).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - index)


def box_max(keys, radii):
    """The maximum of the keys over the box clipped to the volume: one axis at a time, one shift at a time."""
    out = keys
    for axis, r in enumerate(radii):
        src, out = out, out.copy()
        for s in range(1, min(r, src.shape[axis] - 1) + 1):
            lo = [slice(None)] * src.ndim
            hi = [slice(None)] * src.ndim
            lo[axis], hi[axis] = slice(None, -s), slice(s, None)
            lo, hi = tuple(lo), tuple(hi)
            out[lo] = np.maximum(out[lo], src[hi])                  # the voxel s further on
            out[hi] = np.maximum(out[hi], src[lo])                  # and the one s before
    return out


def border_ok(shape, border):
    ok = np.ones(shape, bool)
    for axis, b in enumerate(border):
        i = np.arange(shape[axis])
        keep = (i >= b) & (i < shape[axis] - b)
        ok &= keep.reshape([-1 if a == axis else 1 for a in range(len(shape))])
    return ok


def resolve(img, min_distance, threshold_abs, exclude_border):
    radii = per_axis(min_distance, img.ndim)
    if exclude_border is True:
        border = radii
    elif exclude_border is False:
        border = (0,) * img.ndim
    else:
        border = per_axis(exclude_border, img.ndim)
    thr = float(img.min()) if threshold_abs is None else float(threshold_abs)
    return radii, border, thr


def peak_mask_ref(img, min_distance=1, threshold_abs=None, exclude_border=True):
    radii, border, thr = resolve(img, min_distance, threshold_abs, exclude_border)
    keys = keys_of(img)
    above = np.ones(img.shape, bool) if thr == -np.inf else img.astype(np.float64) > thr
    return ((box_max(keys, radii) == keys) & above & border_ok(img.shape, border)).astype(np.uint8)


def peak_list_ref(img, min_distance=1, threshold_abs=None, exclude_border=True):
    """(coords int32 (K, ndim), values) sorted by value descending, then by linear index ascending: the keys, descending."""
    mask = peak_mask_ref(img, min_distance, threshold_abs, exclude_border)
    keys = np.sort(keys_of(img)[mask != 0])[::-1]
    index = (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
    coords = np.stack(np.unravel_index(index, img.shape), axis=1).astype(np.int32).reshape(-1, img.ndim)
    return coords, img.reshape(-1)[index]


def scipy_mask(img, min_distance, threshold, border):
    """scikit-image's candidate mask: equal to the maximum filter, above the threshold, the border cleared."""
    from scipy import ndimage

    radii = per_axis(min_distance, img.ndim)
    size = tuple(2 * r + 1 for r in radii)
    m = (img == ndimage.maximum_filter(img, size=size, mode="nearest")) & (img > threshold)
    return (m & border_ok(img.shape, per_axis(border, img.ndim))).astype(np.uint8)


def no_two_in_a_box(mask, min_distance):
    """No peak has another peak in its box."""
    radii = per_axis(min_distance, mask.ndim)
    pts = np.argwhere(mask != 0)
    if len(pts) < 2:
        return True
    d = np.abs(pts[:, None, :] - pts[None, :, :])
    close = (d <= np.array(radii)[None, None, :]).all(-1)
    return int(close.sum()) == len(pts)                              # each point and itself only


# ---- the shared inputs (built once per process; treat as read-only) -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tie_free(shape, seed=0):
    """A smooth image without two equal values: the ranks of a smoothed random field, scaled into [0, 1)."""
    from scipy import ndimage

    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    smooth = ndimage.gaussian_filter(rng.random(shape), 1)
    img = (np.argsort(np.argsort(smooth.ravel(), kind="stable"), kind="stable").astype(np.float32) / np.float32(n)).reshape(shape)
    assert n < 2 ** 24 and np.unique(img).size == img.size
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def quantised(shape, levels=40, seed=0):
    """The same field on `levels` values: ties everywhere."""
    img = (np.floor(tie_free(shape, seed) * levels) / np.float32(levels)).astype(np.float32)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def squared_edt(shape, seed=3):
    """An int32 image with plateaus and ridges: the squared distance transform of a random mask."""
    from scipy import ndimage

    mask = np.random.default_rng(seed).random(shape) < 0.93
    d = np.rint(ndimage.distance_transform_edt(mask) ** 2).astype(np.int32)
    d.setflags(write=False)
    return d


def plateau_row():
    row = np.zeros((1, 21), np.float32)
    row[0, 3:15] = 1.0
    return row


def two_balls():
    """Two overlapping balls of radius 7 whose centres are 10 apart: one component, two instances."""
    z, y, x = np.indices((20, 20, 32))
    a = (z - 10) ** 2 + (y - 10) ** 2 + (x - 10) ** 2 <= 49
    b = (z - 10) ** 2 + (y - 10) ** 2 + (x - 20) ** 2 <= 49
    return (a | b).astype(np.uint8)

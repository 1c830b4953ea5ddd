"""The statement of the morphology calls of ``biapy_amd.prepost`` (``bpx_morph``, include/biapy_amd.h) in NumPy, written from the header's text:
shifted slices of the padded volume combined by the row rule.  Shared by test_morph_cpu.py (which holds it against SciPy) and test_morph_gpu.py
(which holds the device against it); also the inputs both files use, built once per process and never written to."""
import functools

import numpy as np

# ---- the statement ---------------------------------------------------------------------------------------------------------------------------------


def rows(ndim, connectivity):
    """The rows (dz, dy) of the element with their x offsets: k = |dz| + |dy| <= connectivity (2-D: dz = 0 only); x - 1, x, x + 1 when
    k + 1 <= connectivity, x alone otherwise."""
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            k = abs(dz) + abs(dy)
            if k <= connectivity and (ndim == 3 or dz == 0):
                out.append((dz, dy, (-1, 0, 1) if k + 1 <= connectivity else (0,)))
    return out


def _identity(dtype, is_max):
    if np.issubdtype(dtype, np.floating):
        return -np.inf if is_max else np.inf
    info = np.iinfo(dtype)
    return info.min if is_max else info.max


def extreme(x, connectivity, is_max, outside=None):
    """The maximum (``is_max``) or minimum over the element; an out-of-volume neighbour counts as ``outside``, or is ignored (``None``)."""
    v = x if x.ndim == 3 else x[None]
    Z, Y, X = v.shape
    p = np.pad(v, 1, constant_values=_identity(v.dtype, is_max) if outside is None else outside)
    acc = None
    for dz, dy, dxs in rows(x.ndim, connectivity):
        for dx in dxs:
            s = p[1 + dz:1 + dz + Z, 1 + dy:1 + dy + Y, 1 + dx:1 + dx + X]
            acc = s.copy() if acc is None else (np.maximum if is_max else np.minimum)(acc, s)
    return acc.reshape(x.shape)


def binary_ref(mask, dilate, connectivity=1, iterations=1, border_value=0):
    m = (np.asarray(mask) != 0).astype(np.uint8)
    for _ in range(iterations):
        m = extreme(m, connectivity, dilate, outside=border_value)
    return m


def binary_erosion_ref(mask, connectivity=1, iterations=1, border_value=0):
    return binary_ref(mask, False, connectivity, iterations, border_value)


def binary_dilation_ref(mask, connectivity=1, iterations=1, border_value=0):
    return binary_ref(mask, True, connectivity, iterations, border_value)


def binary_opening_ref(mask, connectivity=1, iterations=1, border_value=0):
    return binary_ref(binary_ref(mask, False, connectivity, iterations, border_value), True, connectivity, iterations, border_value)


def binary_closing_ref(mask, connectivity=1, iterations=1, border_value=0):
    return binary_ref(binary_ref(mask, True, connectivity, iterations, border_value), False, connectivity, iterations, border_value)


def erosion_ref(x, connectivity=1):
    return extreme(x, connectivity, False)


def dilation_ref(x, connectivity=1):
    return extreme(x, connectivity, True)


def find_boundaries_ref(labels, connectivity=1, mode="thick", background=0):
    x = np.asarray(labels)
    x = x.view(np.uint8) if x.dtype == np.bool_ else x
    edge = extreme(x, connectivity, True) != extreme(x, connectivity, False)
    if mode == "inner":
        edge &= x != background
    return edge.astype(np.uint8)


def ball_ref(mask, radius, dilate):
    """Erosion (out-of-volume ignored: border_value=1) or dilation (border_value=0) by the Euclidean ball dz^2 + dy^2 + dx^2 <= radius^2."""
    m = (np.asarray(mask) != 0)
    v = m if m.ndim == 3 else m[None]
    Z, Y, X = v.shape
    r = int(np.floor(radius))
    rz = r if m.ndim == 3 else 0
    p = np.pad(v, ((rz, rz), (r, r), (r, r)), constant_values=not dilate)
    acc = np.full(v.shape, not dilate)
    for dz in range(-rz, rz + 1):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dz * dz + dy * dy + dx * dx <= radius * radius:
                    s = p[rz + dz:rz + dz + Z, r + dy:r + dy + Y, r + dx:r + dx + X]
                    acc = (acc | s) if dilate else (acc & s)
    return acc.reshape(m.shape).astype(np.uint8)


def fill_holes_ref(mask):
    """The background reached from outside the volume at connectivity 1 stays background; everything else is 1."""
    fg = np.asarray(mask) != 0
    bg = (~fg).astype(np.uint8)
    reached = np.zeros_like(bg)
    while True:
        grown = extreme(reached, 1, True, outside=1) & bg
        if np.array_equal(grown, reached):
            return (reached == 0).astype(np.uint8)
        reached = grown


def border_ids(labels, n_max):
    lab = np.asarray(labels)
    ids = set()
    for axis in range(lab.ndim):
        for side in (0, lab.shape[axis] - 1):
            ids.update(int(v) for v in np.unique(np.take(lab, side, axis=axis)) if 0 < v <= n_max)
    return ids


def clear_border_ref(labels, n_max, relabel=False):
    """(result, survivors): labels on the border and labels outside 1..n_max are 0; the survivors are the ids 1..n_max not on the border."""
    lab = np.asarray(labels)
    gone = border_ids(lab, n_max)
    keep = np.array([False] + [l not in gone for l in range(1, n_max + 1)])
    clean = np.where((lab > 0) & (lab <= n_max), lab, 0)
    out = np.where(keep[clean], clean, 0).astype(np.int32)
    if relabel:
        out = (np.cumsum(keep)[out] * (out > 0)).astype(np.int32)
    return out, int(keep.sum())


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------------------
DENSITY = {1: 0.9, 2: 0.97, 3: 0.97}           # of the erosion inputs per connectivity (the eroded foreground stays near a half); dilation takes the complement
RANDOM_SHAPES = ((5, 7, 9), (33, 37, 41), (16, 32, 64), (37, 41))
THIN_SHAPES = ((1, 37, 41), (33, 1, 41), (33, 37, 1), (1, 1, 41), (1, 9, 1), (7, 1, 1), (1, 1, 1), (1, 41), (9, 1), (1, 1))
SPANS = {np.uint8: (15, 16, 17, 1023, 1024, 1025), np.int32: (3, 4, 5, 255, 256, 257), np.float32: (3, 4, 5, 255, 256, 257)}
LANE = {np.uint8: 16, np.int32: 4, np.float32: 4}


def random_mask(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


@functools.lru_cache(None)
def binary_cases():
    """{name: (mask, connectivity, dilate, random)}: ``random`` marks the cases whose result must hold both values in 1 % of its voxels."""
    out = {}
    for si, shape in enumerate(RANDOM_SHAPES + THIN_SHAPES):
        for c in range(1, len(shape) + 1):
            for dilate in (False, True):
                d = 1 - DENSITY[c] if dilate else DENSITY[c]
                out[f"{'dilate' if dilate else 'erode'} {shape} c{c}"] = (random_mask(shape, d, 100 * si + 10 * c + dilate), c, dilate,
                                                                           shape in RANDOM_SHAPES)
    return out


def span_mask(rows_, X, lane, seed):
    """A 2-D mask of ``rows_`` rows that differs on both sides of every lane edge (x = k lane - 1 | k lane) and of every row edge."""
    m = random_mask((rows_, X), 0.8, seed)
    for k in range(1, (X - 1) // lane + 1):
        m[0::2, k * lane - 1], m[0::2, k * lane] = 1, 0
        m[1::2, k * lane - 1], m[1::2, k * lane] = 0, 1
    for y in range(rows_ - 1):
        m[y + 1, 0] = 1 - m[y, X - 1]
    return m


def _values(mask, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return np.where(mask != 0, rng.integers(1, 256, mask.shape), 0).astype(np.uint8)
    if dtype == np.int32:
        return np.where(mask != 0, rng.integers(1, 6, mask.shape), -rng.integers(0, 2, mask.shape) * 7).astype(np.int32)
    return np.where(mask != 0, np.round(rng.random(mask.shape) * 8, 1) + 0.5, -np.round(rng.random(mask.shape), 1)).astype(np.float32)


@functools.lru_cache(None)
def span_cases():
    """{(dtype name, rows, X): array}: two and three rows with X one below, at and one above the lane and wave spans of each dtype."""
    out = {}
    for dt, xs in SPANS.items():
        for r in (2, 3):
            for X in xs:
                m = span_mask(r, X, LANE[dt], 1000 * r + X)
                out[(np.dtype(dt).name, r, X)] = _values(m, dt, X + r)
    return out


@functools.lru_cache(None)
def grey_cases():
    """{name: array}: uint8, int32 and float32 volumes with ties and, for int32, negative values."""
    out = {}
    for si, shape in enumerate(RANDOM_SHAPES + THIN_SHAPES):
        for dt in (np.uint8, np.int32, np.float32):
            out[f"{np.dtype(dt).name} {shape}"] = _values(random_mask(shape, 0.6, 7 * si + 1), dt, 7 * si + 2)
    return out


def balls(shape, count, rmin, rmax, seed):
    """A uint8 mask of ``count`` random balls."""
    rng = np.random.default_rng(seed)
    grid = np.indices(shape)
    m = np.zeros(shape, np.uint8)
    for _ in range(count):
        centre = [rng.integers(0, s) for s in shape]
        r = rng.integers(rmin, rmax + 1)
        m |= (sum((g - c) ** 2 for g, c in zip(grid, centre)) <= r * r).astype(np.uint8)
    return m


@functools.lru_cache(None)
def ball_volume():
    """40^3 with one ball of radius 5 well inside (erased by 7 erosions at connectivity 1, not by 3) and others up to radius 9."""
    m = balls((40, 40, 40), 6, 6, 9, 5)
    m[:14, :14, :14] = 0
    g = np.indices((13, 13, 13))
    m[:13, :13, :13] = (sum((a - 6) ** 2 for a in g) <= 25).astype(np.uint8)
    return m


@functools.lru_cache(None)
def holes_volume():
    """64^3 balls with punched holes: closed ones, one open to a ball's outside, and balls cut by the volume's faces."""
    m = balls((64, 64, 64), 14, 6, 12, 11)
    rng = np.random.default_rng(12)
    inside = np.argwhere(extreme(m, 1, False, outside=0) != 0)
    for z, y, x in inside[rng.choice(len(inside), 40, replace=False)]:
        m[z, y, x] = 0
        if rng.random() < 0.5:
            m[z, y, min(x + 1, 63)] = 0
    return m


def hand_cases():
    """{name: (mask, filled)}: the hand-made hole-filling cases with their expected results."""
    out = {}
    solid = np.ones((5, 5, 5), np.uint8)
    a = solid.copy(); a[2, 2, 2] = 0
    out["a one-voxel hole"] = (a, solid)
    b = solid.copy(); b[2, 2, 2] = 0; b[2, 2, 3] = 0; b[2, 2, 4] = 0
    out["a hole open to the border through one voxel"] = (b, b)
    c = np.ones((5, 5), np.uint8); c[2, 2] = 0; c[1, 1] = 0; c[0, 0] = 0
    out["a hole open only through a diagonal stays a hole at connectivity 1"] = (c, np.where(np.arange(25).reshape(5, 5) == 0, 0, 1).astype(np.uint8))
    d = np.zeros((4, 6), np.uint8)
    out["all background"] = (d, d)
    out["all foreground"] = (np.ones((3, 4, 5), np.uint8), np.ones((3, 4, 5), np.uint8))
    return out


def corner_cases():
    """A single voxel in each corner of a (4, 5, 6) volume."""
    out = {}
    for z in (0, 3):
        for y in (0, 4):
            for x in (0, 5):
                m = np.zeros((4, 5, 6), np.uint8)
                m[z, y, x] = 1
                out[(z, y, x)] = m
    return out


def touching_labels():
    """Two labels that touch, a third apart, on background: (6, 8) int32."""
    lab = np.zeros((6, 8), np.int32)
    lab[1:5, 1:4], lab[1:5, 4:6], lab[0, 7] = 1, 2, 3
    return lab


def face_labels():
    """(5, 6, 7) int32: labels 1..6 on one face each, 7 in the middle touching none, 8 absent, 9 above n_max = 8 in use."""
    lab = np.zeros((5, 6, 7), np.int32)
    lab[0, 2, 2], lab[4, 2, 2], lab[2, 0, 2], lab[2, 5, 2], lab[2, 2, 0], lab[2, 2, 6] = 1, 2, 3, 4, 5, 6
    lab[2, 2:4, 2:5] = 7
    lab[1, 1, 1] = 9
    return lab

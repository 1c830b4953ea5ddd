"""Reference statement of ``biapy_amd.prepost.label`` and the masks its tests share (test infrastructure, pure NumPy).

``label_ref(mask, c)`` states the rule in code: foreground is every nonzero element; two foreground voxels are joined when they differ by at
most one step on at most ``c`` axes (``generate_structure``); background is 0 and the components are numbered ``1..N`` IN RASTER ORDER OF EACH
COMPONENT'S FIRST VOXEL; the labels are ``int32``.  That is what ``scipy.ndimage.label(mask, structure=generate_structure(mask.ndim, c))``
returns, and ``tests/test_label_cpu.py`` holds the two equal bit for bit.  The masks are built once per process and handed out read-only."""
import numpy as np

SHAPE = (20, 43, 150)          # two full 8 x 8 x 64 tiles of csrc/label.hip and a partial one on every axis (also of a 4 x 8 x 64 tile)
DENSITIES = (0.1, 0.25, 0.32, 0.5, 0.9)
_cache = {}


def generate_structure(ndim, c):
    """``scipy.ndimage.generate_binary_structure(ndim, c)``: the 3^ndim neighbourhood, True where at most ``c`` axes are off centre."""
    off = np.abs(np.indices((3,) * ndim) - 1).sum(axis=0)
    return off <= c


def _offsets(ndim, c):
    s = generate_structure(ndim, c)
    return [tuple(int(v) - 1 for v in idx) for idx in np.argwhere(s) if any(v != 1 for v in idx)]


def _shifted_pairs(shape, off):
    """Slices (a, b) with ``x[b]`` the neighbour at offset ``off`` of ``x[a]``, for the voxels whose neighbour lies inside the volume."""
    a = tuple(slice(max(0, -o), min(s, s - o)) for o, s in zip(off, shape))
    b = tuple(slice(max(0, o), min(s, s + o)) for o, s in zip(off, shape))
    return a, b


def label_ref(mask, c):
    """(labels int32, N).  A union-find over raster indices, run on whole arrays: every foreground voxel starts as its own root; a round
    takes for every voxel the smallest root among its neighbours (``generate_structure``), hangs the voxel's root under it (a smaller index
    only ever replaces a larger one) and then shortens every path to its end; rounds repeat until nothing moves.  A component's root then is
    its smallest raster index, i.e. ITS FIRST VOXEL IN RASTER ORDER, and component k is the one whose root is the k-th smallest."""
    fg = np.asarray(mask) != 0
    shape, n = fg.shape, fg.size
    parent = np.where(fg, np.arange(n, dtype=np.int64).reshape(shape), n)          # n: background, larger than every index
    where = np.flatnonzero(fg)
    offs = _offsets(fg.ndim, c)
    while where.size:
        best = parent.copy()
        for off in offs:
            a, b = _shifted_pairs(shape, off)
            np.minimum(best[a], parent[b], out=best[a])
        flat, bflat = parent.reshape(-1), best.reshape(-1)
        before = flat[where].copy()
        np.minimum.at(flat, before, bflat[where])                                  # union: the voxel's root goes under the smaller root
        while True:                                                                # find, for everybody: parent = parent[parent] to the end
            nxt = flat[flat[where]]
            if np.array_equal(nxt, flat[where]):
                break
            flat[where] = nxt
        if np.array_equal(flat[where], before):
            break
    roots = np.unique(parent[fg])                                                  # ascending = raster order of the first voxels
    lab = np.zeros(shape, np.int32)
    lab[fg] = np.searchsorted(roots, parent[fg]) + 1
    return lab, int(roots.size)


def _ro(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    a.setflags(write=False)
    return a


REF_COUNTS = {1: (526, 615, 513, 78, 1), 3: (151, 11, 7, 1, 1)}       # N of random_masks((9, 21, 37)) by connectivity, per density (SciPy)


def random_masks(shape, seed=0):
    """{(c, p): mask} for every connectivity c of the shape's dimension and every density p: ``rng.random(shape) < p`` drawn from ONE
    ``np.random.default_rng(seed)``, connectivity in the outer loop and density in the inner one."""
    key = ("random", tuple(shape), seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        _cache[key] = {(c, p): _ro(rng.random(tuple(shape)) < p) for c in range(1, len(shape) + 1) for p in DENSITIES}
    return _cache[key]


def many_components():
    """64 x 128 x 128 at p = 0.1: about 7e4 components at connectivity 1, in every chunk of the numbering."""
    if "many" not in _cache:
        _cache["many"] = _ro(np.random.default_rng(5).random((64, 128, 128)) < 0.1)
    return _cache["many"]


def snake(shape):
    """A one-voxel-wide path through the whole volume: boustrophedon rows in the even planes, the planes joined at alternating ends - one
    component at connectivity 1 with the deepest trees a union-find can be handed."""
    Z, Y, X = shape
    m = np.zeros(shape, np.uint8)
    R = (Y - 1) // 2
    for z in range(0, Z, 2):
        for r in range(R + 1):
            m[z, 2 * r, :] = 1
            if r < R:
                m[z, 2 * r + 1, X - 1 if r % 2 == 0 else 0] = 1
        if z + 2 < Z:
            if (z // 2) % 2 == 0:
                m[z + 1, 2 * R, X - 1 if R % 2 == 0 else 0] = 1
            else:
                m[z + 1, 0, 0] = 1
    return m


def combs(shape):
    """Two interleaved combs, spines on opposite sides, teeth two voxels apart: they never touch."""
    Z, Y, X = shape
    m = np.zeros(shape, np.uint8)
    m[:, 0, :] = 1
    m[:, Y - 1, :] = 1
    m[:, 0:Y - 2, 0::4] = 1
    m[:, 2:Y, 2::4] = 1
    return m


EDGE_PAIRS = [((7, 7, 10), (8, 8, 10)), ((15, 3, 63), (16, 3, 64)), ((15, 30, 64), (16, 30, 63)), ((8, 24, 5), (9, 23, 5)),
              ((3, 15, 100), (3, 16, 101)), ((3, 7, 127), (4, 8, 127)), ((11, 20, 63), (11, 21, 64))]
CORNER_PAIRS = [((7, 15, 63), (8, 16, 64)), ((7, 32, 64), (8, 31, 63)), ((15, 39, 127), (16, 40, 128)), ((3, 23, 63), (4, 24, 64))]


def pairs(shape):
    """Pairs of voxels that touch only by an edge (EDGE_PAIRS) or only by a corner (CORNER_PAIRS), each placed exactly across a border of the
    8 x 8 x 64 tile (the z borders 3|4, 7|8, 11|12 and 15|16 cover a tile 4 deep too): 22 components at connectivity 1, 15 at 2, 11 at 3."""
    m = np.zeros(shape, np.uint8)
    for a, b in EDGE_PAIRS + CORNER_PAIRS:
        m[a] = 1
        m[b] = 1
    return m


def structured(name):
    """The structured masks at SHAPE: zero, one, last, checkerboard, snake, combs, pairs."""
    key = ("structured", name)
    if key not in _cache:
        Z, Y, X = SHAPE
        if name == "zero":
            m = np.zeros(SHAPE, np.uint8)
        elif name == "one":
            m = np.ones(SHAPE, np.uint8)
        elif name == "last":
            m = np.zeros(SHAPE, np.uint8)
            m[-1, -1, -1] = 1
        elif name == "checkerboard":
            m = (np.indices(SHAPE).sum(axis=0) & 1).astype(np.uint8)
        elif name == "snake":
            m = snake(SHAPE)
        elif name == "combs":
            m = combs(SHAPE)
        elif name == "pairs":
            m = pairs(SHAPE)
        else:
            raise KeyError(name)
        _cache[key] = _ro(m)
    return _cache[key]


STRUCTURED = ("zero", "one", "last", "checkerboard", "snake", "combs", "pairs")
# N at connectivity 1, 2, 3 - by construction, not from the code under test
STRUCTURED_COUNTS = {"zero": (0, 0, 0), "one": (1, 1, 1), "last": (1, 1, 1), "checkerboard": (20 * 43 * 150 // 2, 1, 1), "snake": (1, 1, 1),
                     "combs": (2, 2, 2), "pairs": (22, 15, 11)}


def balls(shape, fill=0.3, seed=0, rmin=3, rmax=9):
    """Random balls until about ``fill`` of the volume is set: the realistic mask (blobs that touch and merge)."""
    key = ("balls", tuple(shape), fill, seed, rmin, rmax)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        m = np.zeros(shape, bool)
        Z, Y, X = shape
        vol = np.mean([4.19 * r ** 3 for r in range(rmin, rmax + 1)])
        count = int(-np.log(1 - fill) * Z * Y * X / vol)                     # Boolean model: fill = 1 - exp(-balls per voxel * mean ball volume)
        for _ in range(max(count, 1)):
            r = int(rng.integers(rmin, rmax + 1))
            c = [int(rng.integers(0, s)) for s in shape]
            lo = [max(0, ci - r) for ci in c]
            hi = [min(s, ci + r + 1) for ci, s in zip(c, shape)]
            g = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
            m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= (g[0] - c[0]) ** 2 + (g[1] - c[1]) ** 2 + (g[2] - c[2]) ** 2 <= r * r
        _cache[key] = _ro(m)
    return _cache[key]


def scipy_label(mask, c):
    """(labels int32, N) from scipy.ndimage.label with the matching structure; cached per mask object and connectivity."""
    from scipy import ndimage

    key = ("scipy", id(mask), c)
    if key not in _cache:
        lab, n = ndimage.label(np.asarray(mask), structure=generate_structure(np.asarray(mask).ndim, c))
        lab = _ro_i32(lab)
        _cache[key] = (mask, lab, int(n))                   # the mask is kept so that its id stays its own
    return _cache[key][1], _cache[key][2]


def _ro_i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    a.setflags(write=False)
    return a

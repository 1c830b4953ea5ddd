"""The statement of ``bpx_region_props`` (include/biapy_amd.h) in NumPy, written from the header's text: one visit per voxel, ``np.add.at`` into
int64 arrays and ``np.minimum.at`` / ``np.maximum.at`` for the boxes.  Shared by test_regionprops_cpu.py (which holds it against SciPy) and
test_regionprops_gpu.py (which holds the device against it); also the inputs both files use."""
import numpy as np


def region_props_ref(labels, n_max):
    """(area int32 (N+1,), coord_sum int64 (N+1, ndim), bbox int32 (N+1, 2 ndim)) of a 2-D / 3-D integer label array for the labels 1..n_max:
    row 0 and the rows of absent labels all zeros, voxels with a label <= 0 or > n_max ignored, boxes half-open."""
    labels = np.asarray(labels)
    nd = labels.ndim
    flat = labels.ravel().astype(np.int64)
    take = (flat > 0) & (flat <= n_max)
    ids = flat[take]
    coords = [c.ravel()[take].astype(np.int64) for c in np.indices(labels.shape, sparse=False)]
    area = np.zeros(n_max + 1, np.int64)
    np.add.at(area, ids, 1)
    sums = np.zeros((n_max + 1, nd), np.int64)
    lo = np.full((n_max + 1, nd), np.iinfo(np.int32).max, np.int64)
    hi = np.full((n_max + 1, nd), -1, np.int64)
    for k in range(nd):
        np.add.at(sums[:, k], ids, coords[k])
        np.minimum.at(lo[:, k], ids, coords[k])
        np.maximum.at(hi[:, k], ids, coords[k])
    bbox = np.concatenate((lo, hi + 1), axis=1)
    bbox[area == 0] = 0
    assert area[0] == 0 and not sums[0].any()
    return area.astype(np.int32), sums, bbox.astype(np.int32)


def centroid_ref(area, sums):
    """coord_sum / area in float64, NaN where area == 0: one division of two exactly represented integers per entry."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return sums.astype(np.float64) / area.astype(np.float64)[:, None]


def run_labels(shape, n_labels, seed):
    """Labels in runs along the flattened volume that do NOT stop at row ends (a run must be cut there), ids 1..n_labels, about 40 % background,
    some negative - generated like test_overlap_gpu._labels."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    starts = rng.random(n) < 0.15
    starts[0] = True
    ids = np.where(rng.random(n) < 0.4, np.where(rng.random(n) < 0.2, -2, 0), rng.integers(1, max(n_labels, 1) + 1, size=n) if n_labels else 0)
    return ids[np.maximum.accumulate(np.where(starts, np.arange(n), 0))].astype(np.int32).reshape(shape)


def balls(shape, fill=0.3, seed=0, rmin=3, rmax=6):
    """A uint8 mask of random overlapping balls."""
    rng = np.random.default_rng(seed)
    m = np.zeros(shape, bool)
    vol = np.mean([4.19 * r ** 3 for r in range(rmin, rmax + 1)])
    for _ in range(int(-np.log(1 - fill) * np.prod(shape) / vol)):
        r = int(rng.integers(rmin, rmax + 1))
        c = [int(rng.integers(0, s)) for s in shape]
        lo, hi = [max(0, v - r) for v in c], [min(s, v + r + 1) for v, s in zip(c, shape)]
        g = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= (g[0] - c[0]) ** 2 + (g[1] - c[1]) ** 2 + (g[2] - c[2]) ** 2 <= r * r
    return m.view(np.uint8)


SHAPES = [(9, 21, 37), (8, 16, 64), (1, 33, 70), (33, 70), (5, 1, 1), (300, 1), (1, 1, 300)]
LABEL_COUNTS = (0, 1, 7, 1000)                      # 1000 labels overflow a block's 256-slot table
ROW_LENGTHS = (63, 64, 65, 255, 256, 257, 8191, 8192, 8193)

_CASES = {}


def cases():
    """{name: (labels, n_max)}: every input the GPU tests hold against region_props_ref, built once per process and never written to."""
    if _CASES:
        return _CASES
    for shape in SHAPES:
        for k in LABEL_COUNTS:
            _CASES[f"runs {shape} L{k}"] = (run_labels(shape, k, 17 * k + len(shape)), k)
    for x in ROW_LENGTHS:                           # one label through both rows, and runs that cross the row end
        _CASES[f"one label 2 x {x}"] = (np.full((2, x), 3, np.int32), 3)
        _CASES[f"runs 2 x {x}"] = (run_labels((2, x), 7, x), 7)
    _CASES["one label 2 x 1100000"] = (np.full((2, 1_100_000), 2, np.int32), 2)
    _CASES["one label 3 x 3 x 70000"] = (np.full((3, 3, 70_000), 1, np.int32), 1)
    _CASES["8192 voxels, each its own label"] = ((8192 - np.arange(8192, dtype=np.int32)).reshape(4, 32, 64), 8192)
    _CASES["n_max 0 under labels"] = (run_labels((9, 21, 37), 7, 5), 0)
    _CASES["all background"] = (np.zeros((9, 21, 37), np.int32), 5)
    _CASES["labels above num, negative labels"] = (run_labels((9, 21, 37), 7, 6), 4)
    for v in _CASES.values():
        v[0].setflags(write=False)
    return _CASES

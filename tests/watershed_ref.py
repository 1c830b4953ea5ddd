"""Reference statement of ``biapy_amd.prepost.watershed`` and the volumes its tests share (test infrastructure, NumPy and plain Python).

The contract: nodes are the voxels inside the mask; edges join neighbours at the connectivity; the weight of an edge is ``max(okey(u), okey(v))``;
the edges are in the strict total order (weight, raster-first endpoint ``u``, rank of the offset among ``u``'s forward offsets in (dz, dy, dx)
lexicographic order); a voxel with ``markers > 0`` inside the mask is seeded.  ``watershed_ref`` is KRUSKAL over the edges in that order, joining
two trees unless they are the same or both hold a seed; every voxel takes its tree's label.  ``boruvka_ref`` states the same forest the way the
device builds it - synchronous rounds in which every unseeded tree takes its first outgoing edge of the sorted list - and counts the rounds.
``minimax_heights`` gives, by a heap, the lowest pass height over which a set of seeds reaches every voxel: the property a watershed must have
whatever its tie-breaking.  Volumes and references are built once per process and handed out read-only."""
import heapq

import numpy as np

_cache = {}
UNREACHED = np.iinfo(np.int64).max


def rounds_bound(n):
    """R = ceil(log2(max(n, 2))) + 1: the rounds the device launches, computed here from n and never asked of the library."""
    return int(max(n, 2) - 1).bit_length() + 1


def okey(a):
    """The order-preserving uint32 image of int32 / float32 values: ``v + 2^31``, and the sign-flip map of the float's bits (-0.0 < +0.0)."""
    a = np.ascontiguousarray(a)
    bits = a.view(np.uint32)
    if a.dtype == np.int32:
        return bits ^ np.uint32(0x80000000)
    assert a.dtype == np.float32, a.dtype
    return np.where(bits & np.uint32(0x80000000) != 0, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def forward_offsets(connectivity):
    """The forward half of the 3-D neighbourhood in (dz, dy, dx) lexicographic order: 3 / 9 / 13 offsets."""
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dz, dy, dx) > (0, 0, 0) and (dz != 0) + (dy != 0) + (dx != 0) <= connectivity]


def _vol(a):
    a = np.asarray(a)
    return a[None] if a.ndim == 2 else a


def sorted_edges(image, mask=None, connectivity=1):
    """(u, v, weight) of every edge, in the strict order; u is the raster-first endpoint."""
    key = okey(_vol(image))
    shape = key.shape
    inside = np.ones(shape, bool) if mask is None else _vol(mask) != 0
    idx = np.arange(key.size, dtype=np.int64).reshape(shape)
    us, vs, ws, rs = [], [], [], []
    for rank, off in enumerate(forward_offsets(connectivity)):
        a = tuple(slice(max(0, -o), min(s, s - o)) for o, s in zip(off, shape))
        b = tuple(slice(max(0, o), min(s, s + o)) for o, s in zip(off, shape))
        ok = inside[a] & inside[b]
        us.append(idx[a][ok])
        vs.append(idx[b][ok])
        ws.append(np.maximum(key[a], key[b])[ok])
        rs.append(np.full(int(ok.sum()), rank, np.int64))
    u, v, w, r = (np.concatenate(x) for x in (us, vs, ws, rs))
    order = np.lexsort((r, u, w))
    return u[order], v[order], w[order]


def _seed_labels(markers, mask):
    mk = _vol(markers).astype(np.int64).ravel()
    inside = np.ones(mk.size, bool) if mask is None else (_vol(mask) != 0).ravel()
    return np.where(inside & (mk > 0), mk, 0), inside


def _find(parent, i):
    r = i
    while parent[r] != r:
        r = parent[r]
    while parent[i] != r:
        parent[i], i = r, parent[i]
    return r


def watershed_ref(image, markers, mask=None, connectivity=1):
    """The labels (int32, the image's shape) by Kruskal's algorithm on the sorted edges."""
    u, v, _ = sorted_edges(image, mask, connectivity)
    seeds, inside = _seed_labels(markers, mask)
    parent, lab = list(range(seeds.size)), seeds.tolist()
    for a, b in zip(u.tolist(), v.tolist()):
        a, b = _find(parent, a), _find(parent, b)
        if a == b or (lab[a] and lab[b]):
            continue
        parent[a] = b
        if lab[a]:
            lab[b] = lab[a]
    out = np.array([lab[_find(parent, i)] if inside[i] else 0 for i in range(seeds.size)], np.int32)
    return out.reshape(np.asarray(image).shape)


def boruvka_ref(image, markers, mask=None, connectivity=1):
    """(labels, rounds): synchronous rounds.  In a round every tree without a seed takes the FIRST edge of the sorted list that leaves it - all
    at once, on the trees as they stood when the round began - and the trees so linked are joined.  ``rounds`` counts the rounds that joined
    anything; without a seed in the volume there is nothing to do and it is 0."""
    u, v, _ = sorted_edges(image, mask, connectivity)
    seeds, inside = _seed_labels(markers, mask)
    n = seeds.size
    root, lab = np.arange(n), seeds.copy()                        # root[i]: the tree of voxel i; lab[r]: the label of the tree with root r
    pos = np.arange(u.size, dtype=np.int64)
    rounds = 0
    while seeds.any():
        ru, rv = root[u], root[v]
        leaves = ru != rv
        first = np.full(n, u.size, np.int64)
        for side in (ru, rv):
            pick = leaves & (lab[side] == 0)
            np.minimum.at(first, side[pick], pos[pick])
        picked = np.flatnonzero(first < u.size)
        if picked.size == 0:
            break
        rounds += 1
        parent = list(range(n))
        for e in first[picked].tolist():
            a, b = _find(parent, int(ru[e])), _find(parent, int(rv[e]))
            if a != b:
                parent[a] = b
        new_root = np.array([_find(parent, i) for i in range(n)])
        carried = np.zeros(n, np.int64)
        np.maximum.at(carried, new_root, lab)                     # a joined group holds at most one seeded tree: its label, or 0
        held = np.zeros(n, np.int64)
        np.add.at(held, new_root, lab > 0)
        assert held.max() <= 1
        lab = carried
        root = new_root[root]
    out = np.where(inside, lab[root], 0).astype(np.int32)
    return out.reshape(np.asarray(image).shape), rounds


def minimax_heights(image, seed_mask, mask=None, connectivity=1):
    """int64 array: for every voxel inside the mask the least, over all paths from a voxel of ``seed_mask`` (inside the mask), of the largest edge
    weight on the path; -1 on the seeds themselves, ``UNREACHED`` where no path leads and outside the mask."""
    key = okey(_vol(image)).astype(np.int64)
    shape = key.shape
    inside = np.ones(shape, bool) if mask is None else _vol(mask) != 0
    h = np.full(shape, UNREACHED, np.int64)
    heap = []
    for p in map(tuple, np.argwhere(_vol(seed_mask).astype(bool) & inside)):
        h[p] = -1
        heap.append((-1, p))
    heapq.heapify(heap)
    offs = forward_offsets(connectivity)
    offs = offs + [tuple(-o for o in off) for off in offs]
    while heap:
        d, p = heapq.heappop(heap)
        if d > h[p]:
            continue
        for off in offs:
            q = tuple(a + b for a, b in zip(p, off))
            if any(c < 0 or c >= s for c, s in zip(q, shape)) or not inside[q]:
                continue
            nd = max(d, int(max(key[p], key[q])))
            if nd < h[q]:
                h[q] = nd
                heapq.heappush(heap, (nd, q))
    return h.reshape(np.asarray(image).shape)


def check_pass_heights(image, markers, mask, connectivity, labels):
    """Every labelled voxel is reached by ITS label's seeds over the lowest pass height any seed reaches it over; a masked voxel no seed reaches
    is 0, as is every voxel outside the mask.  Returns the number of reachable voxels checked."""
    image, markers, labels = np.asarray(image), np.asarray(markers), np.asarray(labels)
    inside = np.ones(image.shape, bool) if mask is None else np.asarray(mask) != 0
    seeded = inside & (markers > 0)
    per = {int(l): minimax_heights(image, seeded & (markers == l), mask, connectivity) for l in np.unique(markers[seeded])}
    lowest = np.minimum.reduce(list(per.values())) if per else np.full(image.shape, UNREACHED, np.int64)
    reach = lowest != UNREACHED
    assert not labels[~reach].any()
    assert (labels[reach] > 0).all()
    for l, h in per.items():
        sel = reach & (labels == l)
        assert np.array_equal(h[sel], lowest[sel]), l
    assert set(np.unique(labels[reach]).tolist()) <= set(per)
    return int(reach.sum())


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def random_case(shape, levels, dtype, keep, seeds, seed=0):
    """(image, markers, mask or None): ``levels`` image levels around 0 (one level: every weight ties and the index order alone decides), a mask
    keeping ``keep`` of the voxels (1.0: ``None``), markers 1..5 - repeated labels - on ``seeds`` of the voxels and a few negative ones."""
    key = ("random", tuple(shape), levels, np.dtype(dtype).name, keep, seeds, seed)
    if key not in _cache:
        rng = np.random.default_rng([seed, levels, int(keep * 100), int(seeds * 1000)] + list(shape))
        q = rng.integers(0, levels, size=shape) - levels // 2
        image = (q * 0.25).astype(np.float32) if np.dtype(dtype) == np.float32 else q.astype(np.int32)
        mask = None if keep >= 1.0 else _ro((rng.random(shape) < keep).astype(np.uint8))
        draw = rng.random(shape)
        markers = np.where(draw < seeds, rng.integers(1, 6, size=shape), np.where(draw > 0.98, -3, 0)).astype(np.int32)
        _cache[key] = (_ro(image), _ro(markers), mask)
    return _cache[key]


def reference(image, markers, mask, connectivity):
    """``watershed_ref`` cached per (objects, connectivity): the arrays are kept so that their ids stay their own."""
    key = ("ref", id(image), id(markers), id(mask), connectivity)
    if key not in _cache:
        _cache[key] = (image, markers, mask, _ro(watershed_ref(image, markers, mask, connectivity)))
    return _cache[key][3]


def snake_path(Y, X):
    """(mask (Y, X) uint8, the path's voxels in order as (y, x) pairs): a one-voxel-wide boustrophedon path through the plane."""
    mask, order = np.zeros((Y, X), np.uint8), []
    rows = (Y - 1) // 2
    for r in range(rows + 1):
        order += [(2 * r, x if r % 2 == 0 else X - 1 - x) for x in range(X)]
        if r < rows:
            order.append((2 * r + 1, X - 1 if r % 2 == 0 else 0))
    for p in order:
        mask[p] = 1
    return mask, order


def balls(shape, fill=0.3, seed=0, rmin=3, rmax=9):
    """Random balls until about ``fill`` of the volume is set: blobs that touch and overlap (as tests/label_ref.py)."""
    rng = np.random.default_rng(seed)
    m = np.zeros(shape, bool)
    vol = np.mean([4.19 * r ** 3 for r in range(rmin, rmax + 1)])
    for _ in range(max(int(-np.log(1 - fill) * np.prod(shape) / vol), 1)):
        r = int(rng.integers(rmin, rmax + 1))
        c = [int(rng.integers(0, s)) for s in shape]
        lo, hi = [max(0, ci - r) for ci in c], [min(s, ci + r + 1) for ci, s in zip(c, shape)]
        g = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= (g[0] - c[0]) ** 2 + (g[1] - c[1]) ** 2 + (g[2] - c[2]) ** 2 <= r * r
    return m.view(np.uint8)


def plateau_recipe(q, markers):
    """The documented recipe for saturated maps: int32 ``(q << 15) | min(d, 32767)``, d the squared Euclidean distance to the nearest marker."""
    from scipy import ndimage

    d = ndimage.distance_transform_edt(np.asarray(markers) <= 0) ** 2
    return ((np.asarray(q).astype(np.int64) << 15) | np.minimum(np.rint(d).astype(np.int64), 32767)).astype(np.int32)

"""NumPy twin of the label stitching of ``biapy_amd/csrc/stitch_core.h`` (``prepost.LabelStitcher``) and the inputs of its tests.

``stitch_ref(blocks, nums, shape, block_shape, connectivity, rule, min_contact, max_labels)`` takes the per-block ``int32`` labels in raster order
of the grid and returns the renumbered blocks and ``M``: global ids ``off_b + l``; unions over the cross-block backward neighbours (``"touch"``)
or over the face planes by the contact ratio (``"contact"``); the merged objects numbered ``1..M`` in raster order of each object's first voxel
in the whole volume.  ``M = -1`` and the blocks unchanged when the ids pass ``max_labels``.  Written for clarity, not for speed."""
import functools
import itertools

import numpy as np
from scipy import ndimage

SHAPE, BLOCK = (13, 21, 70), (5, 8, 33)            # a ragged 3 x 3 x 3 grid
BLOCKS = (BLOCK, (1, 8, 33), (4, 21, 70), SHAPE)
DENSITIES = (0.2, 0.32, 0.5, 0.7)


def grid_of(shape, block):
    return tuple(-(-s // b) for s, b in zip(shape, block))


def block_slices(shape, block):
    """The slices of every block, in raster order of (i, j, k)."""
    return [tuple(slice(i * b, min((i + 1) * b, s)) for i, b, s in zip(idx, block, shape)) for idx in itertools.product(*(range(g) for g in grid_of(shape, block)))]


def structure(ndim, connectivity):
    return ndimage.generate_binary_structure(ndim, connectivity)


def scipy_label(mask, connectivity):
    lab, n = ndimage.label(mask, structure=structure(mask.ndim, connectivity))
    return lab.astype(np.int32), int(n)


def label_per_block(mask, block, connectivity):
    """``scipy.ndimage.label`` of every block on its own: (list of int32 blocks, list of counts)."""
    out = [scipy_label(mask[s], connectivity) for s in block_slices(mask.shape, block)]
    return [np.ascontiguousarray(a) for a, _ in out], [n for _, n in out]


def backward_offsets(connectivity):
    """The 3 / 9 / 13 offsets that come before the centre in raster order."""
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if d < (0, 0, 0) and sum(v != 0 for v in d) <= connectivity]


class _Sets:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, a):
        while self.p[a] != a:
            self.p[a] = self.p[self.p[a]]
            a = self.p[a]
        return a

    def unite(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.p[max(a, b)] = min(a, b)


def _global_ids(blocks, nums, shape, block):
    G = np.zeros(shape, np.int64)
    B = np.zeros(shape, np.int64)
    off = 0
    for b, (s, lab, n) in enumerate(zip(block_slices(shape, block), blocks, nums)):
        n = max(int(n), 0)
        G[s] = np.where((lab > 0) & (lab <= n), lab.astype(np.int64) + off, 0)
        B[s] = b
        off += n
    return G, B, off


def contact_pairs(G, shape, block):
    """Every (a, b, c, s_A, s_B) over the face planes of the grid: a in the low block's last plane, b in the high block's first plane."""
    out = []
    for axis in range(3):
        for f in range(1, grid_of(shape, block)[axis]):
            pa, pb = np.take(G, f * block[axis] - 1, axis), np.take(G, f * block[axis], axis)
            sa, sb = np.bincount(pa.ravel()), np.bincount(pb.ravel())
            both = (pa > 0) & (pb > 0)
            pairs, counts = np.unique(np.stack((pa[both], pb[both]), 1), axis=0, return_counts=True) if both.any() else (np.zeros((0, 2), np.int64), [])
            out += [(int(a), int(b), int(c), int(sa[a]), int(sb[b])) for (a, b), c in zip(pairs, counts)]
    return out


def stitch_ref(blocks, nums, shape, block, connectivity=1, rule="touch", min_contact=(1, 2), max_labels=None):
    if len(shape) == 2:
        out, M = stitch_ref([b[None] for b in blocks], nums, (1,) + tuple(shape), (1,) + tuple(block), connectivity, rule, min_contact, max_labels)
        return [o[0] for o in out], M
    shape, block = tuple(shape), tuple(min(b, s) for b, s in zip(block, shape))
    G, B, T = _global_ids(blocks, nums, shape, block)
    if max_labels is not None and T > max_labels:
        return [b.copy() for b in blocks], -1
    sets = _Sets(T + 1)
    if rule == "touch":
        for d in backward_offsets(connectivity):
            v = tuple(slice(max(0, -k), s - max(0, k)) for k, s in zip(d, shape))        # voxels whose neighbour at d exists
            u = tuple(slice(max(0, k), s + min(0, k)) for k, s in zip(d, shape))         # that neighbour
            sel = (G[v] > 0) & (G[u] > 0) & (B[v] != B[u])
            for a, b in set(zip(G[v][sel].tolist(), G[u][sel].tolist())):
                sets.unite(a, b)
    else:
        p, q = min_contact
        for a, b, c, sa, sb in contact_pairs(G, shape, block):
            if c * q >= p * min(sa, sb):
                sets.unite(a, b)
    ids, first = np.unique(G.ravel(), return_index=True)            # the smallest global linear index of every id that a voxel carries
    key = {}
    for g, f in zip(ids.tolist(), first.tolist()):
        if g:
            r = sets.find(g)
            key[r] = min(key.get(r, f), f)
    number = {r: k + 1 for k, r in enumerate(sorted(key, key=key.get))}
    table = np.zeros(T + 1, np.int32)
    for g in ids.tolist():
        if g:
            table[g] = number[sets.find(g)]
    whole = table[G]
    return [np.ascontiguousarray(whole[s]) for s in block_slices(shape, block)], len(number)


def assemble(blocks, shape, block):
    shape3, block3 = ((1,) + tuple(shape), (1,) + tuple(block)) if len(shape) == 2 else (tuple(shape), tuple(block))
    out = np.zeros(shape3, np.int32)
    for s, b in zip(block_slices(shape3, tuple(min(a, c) for a, c in zip(block3, shape3))), blocks):
        out[s] = b.reshape(out[s].shape)
    return out.reshape(shape)


def contact_brute(blocks, nums, shape, block, min_contact):
    """The contact rule position by position and block pair by block pair: the set of united (block, label) pairs."""
    p, q = min_contact
    grid = grid_of(shape, block)
    index = {idx: b for b, idx in enumerate(itertools.product(*(range(g) for g in grid)))}
    joined = set()
    for idx, b in index.items():
        for axis in range(3):
            nxt = tuple(v + (k == axis) for k, v in enumerate(idx))
            if nxt not in index:
                continue
            A, Bk = np.take(blocks[b], -1, axis), np.take(blocks[index[nxt]], 0, axis)
            c, sa, sb = {}, {}, {}
            for la, lb in zip(A.ravel().tolist(), Bk.ravel().tolist()):
                la = la if 0 < la <= nums[b] else 0
                lb = lb if 0 < lb <= nums[index[nxt]] else 0
                if la:
                    sa[la] = sa.get(la, 0) + 1
                if lb:
                    sb[lb] = sb.get(lb, 0) + 1
                if la and lb:
                    c[la, lb] = c.get((la, lb), 0) + 1
            joined |= {((b, la), (index[nxt], lb)) for (la, lb), n in c.items() if n * q >= p * min(sa[la], sb[lb])}
    return joined


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------

def random_mask(shape, density, seed=0):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def snake(Z, Y, X):
    """A one-voxel-wide path through the whole volume: boustrophedon rows in the even planes, joined at alternating ends."""
    v = np.zeros((Z, Y, X), np.uint8)
    R = (Y - 1) // 2
    for z in range(0, Z, 2):
        for r in range(R + 1):
            v[z, 2 * r, :] = 1
            if r < R:
                v[z, 2 * r + 1, X - 1 if r % 2 == 0 else 0] = 1
        if z + 2 < Z:
            if (z // 2) % 2 == 0:
                v[z + 1, 2 * R, X - 1 if R % 2 == 0 else 0] = 1
            else:
                v[z + 1, 0, 0] = 1
    return v


def balls(shape, fill=0.3, seed=0, rmin=3, rmax=9):
    rng = np.random.default_rng(seed)
    m = np.zeros(shape, bool)
    vol = np.mean([4.19 * r ** 3 for r in range(rmin, rmax + 1)])
    for _ in range(int(-np.log(1 - fill) * np.prod(shape) / vol)):
        r = int(rng.integers(rmin, rmax + 1))
        c = [int(rng.integers(0, n)) for n in shape]
        lo, hi = [max(0, v - r) for v in c], [min(n, v + r + 1) for v, n in zip(c, shape)]
        g = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= (g[0] - c[0]) ** 2 + (g[1] - c[1]) ** 2 + (g[2] - c[2]) ** 2 <= r * r
    return m.view(np.uint8)


def _points(*pts):
    m = np.zeros(SHAPE, np.uint8)
    for p in pts:
        m[p] = 1
    return m


@functools.lru_cache(maxsize=None)
def structured():
    """name -> mask, all of SHAPE, to be cut by BLOCK."""
    z, y, x = np.indices(SHAPE)
    gap = random_mask(SHAPE, 0.4, 7)
    gap[:, :, 33:66] = 0                                           # the middle column of blocks holds no label
    later = _points((0, 0, 0), (0, 8, 5), (0, 8, 30), (0, 8, 31), (0, 8, 32), (0, 8, 33), (1, 8, 33), (1, 7, 33), (0, 9, 0), (0, 20, 5), (1, 0, 50))
    return {
        "all zero": np.zeros(SHAPE, np.uint8),
        "all one": np.ones(SHAPE, np.uint8),
        "checkerboard": ((z + y + x) & 1).astype(np.uint8),
        "corner pair": _points((4, 7, 32), (5, 8, 33)),              # touch only across a block corner
        "edge pair": _points((4, 7, 10), (5, 8, 10)),                # only across a block edge (z, y)
        "edge pair high x": _points((3, 7, 33), (3, 8, 32)),         # backward neighbour (0, -1, +1) leaves through the HIGH x face
        "boustrophedon": snake(*SHAPE),
        "empty blocks between": gap,
        "first voxel in a later block": later,                       # the object through (0, 8, 30) .. (1, 7, 33): smallest id in block 1, first voxel in block 3
    }


@functools.lru_cache(maxsize=None)
def all_masks():
    """Every mask of the GPU tests: name -> (mask, block shapes)."""
    out = {f"random {d}": (random_mask(SHAPE, d, int(d * 100)), BLOCKS) for d in DENSITIES}
    out.update({name: (m, (BLOCK,)) for name, m in structured().items()})
    out["lanes"] = (random_mask((3, 70, 300), 0.4, 3), ((2, 33, 130),))
    out["2-D"] = (random_mask((33, 70), 0.45, 4), ((8, 33),))
    out["balls 64"] = (balls((64, 64, 64)), ((16, 64, 64),))
    return out


def contact_cases():
    """name -> (blocks, nums, shape, block shape, min_contact, expected M): hand-made per-block instance labels."""
    out = {}
    g = np.ogrid[0:12, 0:12, 0:24]
    ball = ((g[0] - 6) ** 2 + (g[1] - 6) ** 2 + (g[2] - 11.5) ** 2 <= 16).astype(np.int32)
    out["ball cut by a face"] = ([np.ascontiguousarray(ball[:, :, :12]), np.ascontiguousarray(ball[:, :, 12:])], [1, 1], (12, 12, 24), (12, 12, 12), (1, 2), 1)
    a, b = np.zeros((1, 19, 2), np.int32), np.zeros((1, 19, 2), np.int32)
    a[0, 0:10, :], b[0, 9:19, :] = 1, 1
    out["1 of 10 positions"] = ([a, b], [1, 1], (1, 19, 4), (1, 19, 2), (1, 2), 2)
    a, b, c = (np.zeros((1, 20, 2), np.int32) for _ in range(3))
    a[0, 0:6, :] = 1
    b[0, 0:6, 0], b[0, 10:16, 1] = 1, 1
    b[0, 6:10, :] = 1                                              # b's one label: holds a's rows on its low face, c's rows on its high face
    c[0, 10:16, :] = 1
    out["chain of three"] = ([a, b, c], [1, 1, 1], (1, 20, 6), (1, 20, 2), (1, 2), 1)
    a, b = np.zeros((1, 30, 2), np.int32), np.zeros((1, 30, 2), np.int32)
    a[0, 0:10, :], b[0, 5:15, :] = 1, 1                            # c = 5, s = 10 and 10: exactly 1 / 2
    a[0, 16:26, :], b[0, 22:30, :] = 2, 2                          # c = 4, s = 10 and 8: 4 / 8 = 1 / 2 exactly, too
    out["ratio on p / q"] = ([a, b], [2, 2], (1, 30, 4), (1, 30, 2), (1, 2), 2)
    a, b = a.copy(), b.copy()
    b[0, 5, :] = 0                                                 # c = 4 of min(10, 9): below 1 / 2
    out["ratio below p / q"] = ([a, b], [2, 2], (1, 30, 4), (1, 30, 2), (1, 2), 3)
    out["ratio 1 / 3"] = ([a, b], [2, 2], (1, 30, 4), (1, 30, 2), (1, 3), 2)
    return out


# ---- a mask whose labels are a closed-form function of (y, x): z-aligned rods on a 4 x 4 lattice plus full y = 16 s + 2 slabs ------------------
# Rods stand at y % 4 == 0 and x % 4 == 0, slabs at y % 16 == 2: no two of them are neighbours at any connectivity, every one spans all z, so
# the components in raster order of their first voxel (all in plane z = 0) are, row after row, the rods of a rod row and the slab of a slab row.

def rods_mask(shape, device):
    import torch

    Z, Y, X = shape
    y, x = torch.arange(Y, device=device)[:, None], torch.arange(X, device=device)[None, :]
    plane = (((y % 4 == 0) & (x % 4 == 0)) | (y % 16 == 2)).to(torch.uint8)
    return plane[None].expand(Z, Y, X).contiguous()


def rods_expected(shape, device):
    """(the expected labels of one plane as int32 (Y, X), the expected count)."""
    import torch

    _, Y, X = shape
    y, x = torch.arange(Y, device=device)[:, None], torch.arange(X, device=device)[None, :]
    nx = (X + 3) // 4
    rod = (y // 4) * nx + (y + 13) // 16 + x // 4 + 1               # rod rows before + slabs before (16 s + 2 < y) + place in the row
    slab = ((y + 2) // 4) * nx + y // 16 + 1 + 0 * x                # rod rows before (4 r < y) + slabs before + 1
    plane = torch.where(y % 16 == 2, slab, torch.where((y % 4 == 0) & (x % 4 == 0), rod, 0 * rod)).to(torch.int32)
    return plane, ((Y + 3) // 4) * nx + (Y + 13) // 16


def rods_check(labels, shape):
    """True when ``labels`` (device int32) is the closed form, compared plane group by plane group with no host copy of the volume."""
    plane, _ = rods_expected(shape, labels.device)
    return all(bool((labels[z:z + 64] == plane[None]).all()) for z in range(0, shape[0], 64))

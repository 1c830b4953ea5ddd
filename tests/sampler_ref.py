"""The statement of ``biapy_amd.sampler`` on the host (helper of test_sampler_cpu.py / test_sampler_gpu.py, no test itself): ``draw`` gives the
origins of a call in NumPy / Python integers, written from the statement in include/biapy_amd.h (not from the kernel), and ``gather`` the batch of
given origins by torch slicing on the CPU.  Philox4x32-10 is tests/augment_ref.py's."""
import numpy as np
import torch

from augment_ref import philox4x32_10

# the seeds of the frequency tests: test_sampler_cpu checks that the twin alone meets the five-sigma bounds with them
FREQ_SEED_UNIFORM = 1001
FREQ_SEED_CLASS = 2002
FREQ_B, FREQ_CALLS = 4096, 4


def class_cum(class_probs):
    """Running fp32 sum of the normalised probabilities in index order; the last entry - and every entry from the last class of positive
    probability on, which the draw can then never pass - is 1.0."""
    total = float(sum(class_probs))
    acc, out = np.float32(0), []
    for p in class_probs:
        acc = np.float32(acc + np.float32(p / total))
        out.append(np.float32(min(acc, np.float32(1))))
    last = max(i for i, p in enumerate(class_probs) if p > 0)
    return [np.float32(1) if i >= last else c for i, c in enumerate(out)]


def row_tables(maps, K):
    """rowcum[c] (R + 1 Python-exact int64 prefix over all (v, z, y) rows) and the first row of every volume."""
    counts = []
    for c in range(K):
        per = [(np.asarray(m).reshape(-1, m.shape[-1]) == c).sum(axis=1).astype(np.int64) for m in maps]
        counts.append(np.concatenate([[0], np.cumsum(np.concatenate(per))]).astype(np.int64))
    row0 = np.concatenate([[0], np.cumsum([int(np.prod(m.shape[:-1])) for m in maps])]).astype(np.int64)
    return counts, row0


def draw(seed, counter, B, extents, patch, class_maps=None, class_probs=None, centres=False):
    """origins (B, 4) int32 = (v, z0, y0, x0) of the call that draws with ``counter``.  extents: [(Z, Y, X)] per volume; patch (Pz, Py, Px);
    class mode: class_maps = uint8 arrays (Z, Y, X) and the probabilities.  centres=True: also the (B, 4) centres (v, z, y, x) of the class mode."""
    Pz, Py, Px = patch
    r = philox4x32_10(np.arange(B, dtype=np.uint64), 0, counter & 0xFFFFFFFF, (counter >> 32) & 0xFFFFFFFF, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out, cen = np.zeros((B, 4), np.int32), np.zeros((B, 4), np.int32)
    if class_maps is None:
        n = [(Z - Pz + 1) * (Y - Py + 1) * (X - Px + 1) for Z, Y, X in extents]
        cum = [0]
        for a in n:
            cum.append(cum[-1] + a)
    else:
        K = len(class_probs)
        cc = class_cum(class_probs)
        rowcum, row0 = row_tables([np.asarray(m).reshape(e) for m, e in zip(class_maps, extents)], K)
    for b in range(B):
        r64 = (int(r[0][b]) << 32) | int(r[1][b])
        if class_maps is None:
            k = (r64 * cum[-1]) >> 64
            v = max(i for i in range(len(n)) if cum[i] <= k)
            Z, Y, X = extents[v]
            rest = k - cum[v]
            nx, ny = X - Px + 1, Y - Py + 1
            out[b] = (v, rest // (nx * ny), (rest // nx) % ny, rest % nx)
            continue
        u = np.float32(int(r[2][b]) >> 8) * np.float32(2.0 ** -24)
        c = next(i for i in range(K) if u < cc[i])
        k = (r64 * int(rowcum[c][-1])) >> 64
        row = int(np.searchsorted(rowcum[c], k, side="right")) - 1         # rowcum[row] <= k < rowcum[row + 1]
        j = k - int(rowcum[c][row])
        v = int(np.searchsorted(row0, row, side="right")) - 1
        Z, Y, X = extents[v]
        rin = row - int(row0[v])
        z, y = rin // Y, rin % Y
        x = int(np.flatnonzero(np.asarray(class_maps[v]).reshape(Z, Y, X)[z, y] == c)[j])
        cen[b] = (v, z, y, x)
        out[b] = (v, min(max(z - Pz // 2, 0), Z - Pz), min(max(y - Py // 2, 0), Y - Py), min(max(x - Px // 2, 0), X - Px))
    return (out, cen) if centres else out


def gather(images, targets, origins, patch, scale=None):
    """(x, t) of CPU tensors by slicing: images / targets are lists of (Z, Y, X, C) tensors, origins (B, 4), patch (Pz, Py, Px)."""
    Pz, Py, Px = patch
    xs, ts = [], []
    for v, z0, y0, x0 in np.asarray(origins).tolist():
        w = images[v][z0:z0 + Pz, y0:y0 + Py, x0:x0 + Px].to(torch.float32)
        xs.append(w * torch.tensor(scale, dtype=torch.float32) if scale is not None else w)
        ts.append(targets[v][z0:z0 + Pz, y0:y0 + Py, x0:x0 + Px])
    return torch.stack(xs), torch.stack(ts)


def uniform_cells(extents, patch):
    """{(v, z0, y0, x0): probability} of the uniform mode."""
    Pz, Py, Px = patch
    cells = [(v, z, y, x) for v, (Z, Y, X) in enumerate(extents) for z in range(Z - Pz + 1) for y in range(Y - Py + 1) for x in range(X - Px + 1)]
    return {c: 1.0 / len(cells) for c in cells}


def class_cells(extents, patch, class_maps, class_probs):
    """{origin: probability} of the class mode: every voxel of class c carries class_probs[c] / sum / count_c to the origin its patch gets."""
    Pz, Py, Px = patch
    total = float(sum(class_probs))
    counts = [sum(int((np.asarray(m) == c).sum()) for m in class_maps) for c in range(len(class_probs))]
    cells = {}
    for v, ((Z, Y, X), m) in enumerate(zip(extents, class_maps)):
        m = np.asarray(m).reshape(Z, Y, X)
        for z in range(Z):
            for y in range(Y):
                for x in range(X):
                    c = int(m[z, y, x])
                    if class_probs[c] > 0:
                        o = (v, min(max(z - Pz // 2, 0), Z - Pz), min(max(y - Py // 2, 0), Y - Py), min(max(x - Px // 2, 0), X - Px))
                        cells[o] = cells.get(o, 0.0) + class_probs[c] / total / counts[c]
    return cells


def check_frequencies(origins, cells):
    """Five sigma per cell: |count - N p| <= 5 sqrt(N p (1 - p)) for every cell, and no draw outside the cells.  Returns the worst ratio."""
    origins = np.asarray(origins).reshape(-1, 4)
    N = len(origins)
    seen = {}
    for o in map(tuple, origins.tolist()):
        seen[o] = seen.get(o, 0) + 1
    assert set(seen) <= set(cells), sorted(set(seen) - set(cells))[:5]
    worst = 0.0
    for o, p in cells.items():
        dev, bound = abs(seen.get(o, 0) - N * p), 5 * np.sqrt(N * p * (1 - p))
        assert dev <= bound, (o, seen.get(o, 0), N * p, bound)
        worst = max(worst, dev / bound)
    return worst


# ---- the cases both test files draw -------------------------------------------------------------------------------------------------------------
FREQ_UNIFORM = dict(extents=[(3, 4, 5), (2, 3, 6)], patch=(2, 2, 3))                    # 18 + 8 origins


def freq_class_case():
    """One volume (4, 6, 10), three classes with probabilities (0.2, 0.5, 0.3), patch (2, 3, 4): the clamp folds centres near a face onto one origin."""
    g = np.random.RandomState(7)
    m = g.randint(0, 3, size=(4, 6, 10)).astype(np.uint8)
    return dict(extents=[(4, 6, 10)], patch=(2, 3, 4), class_maps=[m], class_probs=(0.2, 0.5, 0.3))


def hard_class_case():
    """Two volumes for the class mode: class 2 present in a single voxel, rows of 200 voxels (no multiple of 64) whose class-1 voxels lie past
    position 128, and classes 1 and 2 absent from the whole second volume."""
    a = np.zeros((2, 3, 200), np.uint8)
    a[:, :, 130:190:3] = 1
    a[1, 2, 199] = 2
    b = np.zeros((3, 4, 9), np.uint8)
    return [a, b], [(2, 3, 200), (3, 4, 9)]


def thin_class_case():
    """X = 1 rows: two volumes one voxel wide, two classes."""
    g = np.random.RandomState(3)
    maps = [g.randint(0, 2, size=(5, 7, 1)).astype(np.uint8), g.randint(0, 2, size=(3, 4, 1)).astype(np.uint8)]
    return maps, [(5, 7, 1), (3, 4, 1)]

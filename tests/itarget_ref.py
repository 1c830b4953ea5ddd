"""The NumPy twin of ``biapy_amd.targets.InstanceTargets`` / ``prepost.instance_targets`` (test infrastructure): every rule of the module's
docstring in the stated fp64 / fp32 arithmetic, an independent SciPy statement of the same channels, the comparator, and the inputs the CPU and
GPU tests share - built once per process and never written to.

NumPy evaluates ``a * a + b * b`` as separate correctly rounded operations (no FMA), float64 ``sqrt`` and ``/`` are correctly rounded, and
``astype(float32)`` rounds to nearest even - the arithmetic the kernels are built for (``-ffp-contract=off``)."""
import numpy as np

import edt_ref as ER

CHANNELS = ("F", "C", "D", "Dc", "H", "V", "Z")
ALL7 = CHANNELS
ALL2D = ("F", "C", "D", "Dc", "H", "V")
DEFECTS = ("box_exclusive", "dmax_other_sample", "contour_ignores_background")


# ---- the rules ------------------------------------------------------------------------------------------------------------------------------

def sanitise(t, n_max):
    """``(int32 ids, faults)``: a value that is no integer in ``0..n_max`` (NaN and +-inf among them) is background and one fault."""
    t = np.asarray(t)
    if t.dtype.kind == "f":
        with np.errstate(invalid="ignore"):
            ok = (t >= 0) & (t <= np.float32(n_max)) & (t == np.trunc(t))
        ids = np.where(ok, np.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0), 0).astype(np.int32)
    else:
        ok = (t >= 0) & (t <= n_max)
        ids = np.where(ok, t, 0).astype(np.int32)
    return ids, int((~ok).sum())


def edge(ids, connectivity, ignore_background=False):
    """bool: some in-volume neighbour within ``generate_binary_structure(ndim, connectivity)`` carries another id (2-D: no z neighbours)."""
    v = ids if ids.ndim == 3 else ids[None]
    Z, Y, X = v.shape
    out = np.zeros(v.shape, bool)
    for dz in ((-1, 0, 1) if ids.ndim == 3 else (0,)):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k = (dz != 0) + (dy != 0) + (dx != 0)
                if k == 0 or k > connectivity:
                    continue
                dst = tuple(slice(max(0, -d), n - max(0, d)) for d, n in zip((dz, dy, dx), (Z, Y, X)))
                src = tuple(slice(max(0, d), n - max(0, -d)) for d, n in zip((dz, dy, dx), (Z, Y, X)))
                diff = v[dst] != v[src]
                if ignore_background:                                   # the seeded defect: a background voxel is never marked
                    diff &= v[dst] > 0
                out[dst] |= diff
    return out.reshape(ids.shape)


def distance(ids):
    """The float32 distance of ``prepost.label_distance`` on the unit grid: ``float32(sqrt(float64(squared)))``, ``+inf`` at the sentinel."""
    return ER.sqrt_f32(ER.separable_sq(ids))


def records(ids, n_max):
    """``(area int64 [n_max + 1], sums int64 [n_max + 1, 3], lo, hi int64 [n_max + 1, 3] inclusive)`` over z, y, x; rows without voxels: lo > hi."""
    v = ids if ids.ndim == 3 else ids[None]
    co = np.indices(v.shape).reshape(3, -1)
    flat = v.reshape(-1)
    keep = flat > 0
    lab, co = flat[keep], co[:, keep]
    area = np.bincount(lab, minlength=n_max + 1).astype(np.int64)
    sums = np.zeros((n_max + 1, 3), np.int64)
    lo = np.full((n_max + 1, 3), np.iinfo(np.int32).max, np.int64)
    hi = np.full((n_max + 1, 3), -1, np.int64)
    for a in range(3):
        np.add.at(sums[:, a], lab, co[a])
        np.minimum.at(lo[:, a], lab, co[a])
        np.maximum.at(hi[:, a], lab, co[a])
    return area, sums, lo, hi


def _scale(sampling, ndim):
    s = [1.0] * 3 if sampling is None else [1.0] * (3 - ndim) + [float(x) for x in sampling]
    return np.array(s, np.float64)


def sample_targets(ids, channels, n_max, *, contour_mode="thick", contour_connectivity=1, f_excludes_contour=False, d_norm="instance", d_clip=None,
                   sampling=None, d=None, dmax_from=None, defect=None):
    """The ``(Ct, *ids.shape)`` float32 target of ONE sample of sanitised int32 ids.  ``d``: the float32 distances (default: the unit-grid twin;
    with ``sampling`` the caller passes ``prepost.label_distance``'s own result).  ``dmax_from``: the distances the per-instance maximum is taken
    from, for the seeded defect that uses another sample's."""
    ids = np.asarray(ids, np.int32)
    v = ids if ids.ndim == 3 else ids[None]
    l = v.reshape(-1).astype(np.int64)
    fg = l > 0
    e = edge(ids, contour_connectivity, ignore_background=defect == "contour_ignores_background").reshape(-1)
    contour = e if contour_mode == "thick" else e & fg
    if d is None and sampling is not None:
        raise ValueError("with sampling the distances are the caller's")
    d = (distance(ids) if d is None else np.asarray(d, np.float32)).reshape(-1)
    area, sums, lo, hi = records(ids, n_max)
    if defect == "box_exclusive":
        hi = hi + 1
    with np.errstate(invalid="ignore", divide="ignore"):
        cen = sums.astype(np.float64) / area.astype(np.float64)[:, None]            # c_a = double(S_a) / double(A)
    p = np.indices(v.shape).reshape(3, -1).astype(np.float64)
    s = _scale(sampling, ids.ndim)
    out = []
    for c in channels:
        if c == "C":
            out.append(contour.astype(np.float32))
            continue
        val = np.zeros(l.shape, np.float32)
        if c == "F":
            val[fg] = 1.0
            if f_excludes_contour:
                val[contour] = 0.0
        elif c == "D":
            bits = np.zeros(n_max + 1, np.uint32)
            src = d if dmax_from is None else np.asarray(dmax_from, np.float32).reshape(-1)
            np.maximum.at(bits, l[fg], src[fg].view(np.uint32))                      # the order of non-negative floats is their bits' order
            dmax = bits.view(np.float32)
            if d_norm == "none":
                val[fg] = d[fg] if d_clip is None else np.minimum(d[fg], np.float32(d_clip))
            else:
                with np.errstate(invalid="ignore", divide="ignore"):
                    q = d[fg] / dmax[l[fg]]                                          # one fp32 division
                val[fg] = np.where(np.isinf(d[fg]), np.float32(1.0), q)
        elif c == "Dc":
            cz, cy, cx = (cen[l[fg], a] for a in range(3))
            dz, dy, dx = (p[0][fg] - cz) * s[0], (p[1][fg] - cy) * s[1], (p[2][fg] - cx) * s[2]
            rc = np.sqrt((dz * dz + dy * dy) + dx * dx).astype(np.float32)
            bits = np.zeros(n_max + 1, np.uint32)
            np.maximum.at(bits, l[fg], rc.view(np.uint32))
            rcmax = bits.view(np.float32)[l[fg]]
            with np.errstate(invalid="ignore", divide="ignore"):
                val[fg] = np.where(rcmax == 0, np.float32(1.0), np.float32(1.0) - rc / rcmax)      # two fp32 operations
        elif c in ("H", "V", "Z"):
            a = {"Z": 0, "V": 1, "H": 2}[c]
            if c == "Z" and ids.ndim == 2:
                raise ValueError("channel 'Z' needs 3-D samples")
            ca = cen[l[fg], a]
            o = p[a][fg] - ca
            ext = np.where(o >= 0, hi[l[fg], a].astype(np.float64) - ca, ca - lo[l[fg], a].astype(np.float64))
            with np.errstate(invalid="ignore", divide="ignore"):
                val[fg] = np.where(ext == 0, np.float32(0.0), (o / ext).astype(np.float32))
        else:
            raise ValueError(c)
        out.append(val)
    return np.stack(out).reshape((len(channels),) + ids.shape)


def batch_targets(t, channels, n_max, d=None, defect=None, **options):
    """``(target (B, Ct, *sample) float32, faults)`` of a batch ``t`` of shape ``(B, *sample)`` of any accepted dtype; ``d``: ``(B, *sample)``."""
    ids, faults = sanitise(t, n_max)
    B = ids.shape[0]
    out = []
    for b in range(B):
        other = None
        if defect == "dmax_other_sample":
            other = distance(ids[(b + 1) % B]) if d is None else d[(b + 1) % B]
        out.append(sample_targets(ids[b], channels, n_max, d=None if d is None else d[b], dmax_from=other, defect=defect, **options))
    return np.stack(out), faults


# ---- the independent statement: SciPy, label by label -----------------------------------------------------------------------------------------

def scipy_targets(ids, channels, n_max, contour_mode="thick", contour_connectivity=1):
    """The same channels of one sample (unit grid, ``d_norm="instance"``) from ``scipy.ndimage``: per-label ``distance_transform_edt``,
    ``center_of_mass``, ``find_objects`` and ``grey_dilation != grey_erosion``; float64 until the last step of each rule."""
    from scipy import ndimage

    ids = np.asarray(ids, np.int32)
    nd = ids.ndim
    fg = ids > 0
    fp = ndimage.generate_binary_structure(nd, contour_connectivity)
    e = ndimage.grey_dilation(ids, footprint=fp) != ndimage.grey_erosion(ids, footprint=fp)
    contour = e if contour_mode == "thick" else e & fg
    present = [int(l) for l in np.unique(ids) if l > 0]
    boxes = ndimage.find_objects(ids, max_label=n_max)
    grid = np.indices(ids.shape).astype(np.float64)
    vals = {c: np.zeros(ids.shape, np.float32) for c in channels}
    if "F" in vals:
        vals["F"][fg] = 1.0
    if "C" in vals:
        vals["C"] = contour.astype(np.float32)
    for l in present:
        m = ids == l
        if "D" in vals:
            if m.all():
                vals["D"][m] = 1.0
            else:
                d32 = ndimage.distance_transform_edt(m).astype(np.float32)
                vals["D"][m] = (d32 / d32.max())[m]
        com = ndimage.center_of_mass(m)
        box = boxes[l - 1]
        if "Dc" in vals:
            r = np.sqrt(sum((grid[a] - com[a]) ** 2 for a in range(nd)))
            rc = r.astype(np.float32)
            rmax = rc[m].max()
            vals["Dc"][m] = 1.0 if rmax == 0 else (np.float32(1.0) - rc / rmax)[m]
        for c, a in (("Z", nd - 3), ("V", nd - 2), ("H", nd - 1)):
            if c in vals:
                o = grid[a] - com[a]
                ext = np.where(o >= 0, (box[a].stop - 1) - com[a], com[a] - box[a].start)
                with np.errstate(invalid="ignore", divide="ignore"):
                    vals[c][m] = np.where(ext == 0, 0.0, o / ext).astype(np.float32)[m]
    return np.stack([vals[c] for c in channels])


# ---- the comparator -----------------------------------------------------------------------------------------------------------------------------

def ulp_distance(a, b):
    """The largest distance in float32 ulps between two arrays without NaNs (infinities equal to themselves)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0

    def key(x):                                                          # a monotone map of the floats onto the integers; -0.0 and 0.0 meet
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    return int(np.abs(key(a) - key(b)).max())


def mismatch(got, want, channels, ulps=None, axis=1):
    """``None`` when ``got`` equals ``want`` - bit for bit, or within ``ulps[channel]`` float32 ulps for the channels named there - else a text
    that names the first offending channel.  ``axis``: where the channels lie, 1 for a batch ``(B, Ct, ...)``, 0 for one sample."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != np.float32 or got.shape[axis] != len(channels):
        return f"shape / dtype: {got.shape} {got.dtype} against {want.shape}"
    for i, c in enumerate(channels):
        g, w = np.take(got, i, axis=axis), np.take(want, i, axis=axis)
        if np.isnan(g).any() or np.isnan(w).any():
            return f"channel {c}: NaN"
        tol = (ulps or {}).get(c, 0)
        if tol == 0:
            bad = g.view(np.uint32) != w.view(np.uint32)
            if bad.any():
                at = tuple(int(k) for k in np.argwhere(bad)[0])
                return f"channel {c}: {int(bad.sum())} voxels differ, first at {at}: {g[at]!r} against {w[at]!r}"
        else:
            u = ulp_distance(g, w)
            if u > tol:
                return f"channel {c}: {u} ulps apart (allowed {tol})"
    return None


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------------------

def blobs(shape, count, seed, rmin=2, rmax=6):
    """int32 ids 1..count: balls around random centres, a voxel going to the nearest centre whose ball holds it - instances touch where balls
    overlap, and balls are cut by every face."""
    rng = np.random.default_rng(seed)
    dims = (1,) * (3 - len(shape)) + tuple(shape)
    g = np.indices(dims).astype(np.float64)
    best = np.full(dims, np.inf)
    out = np.zeros(dims, np.int32)
    for i in range(1, count + 1):
        c = [rng.integers(0, n) for n in dims]
        r = rng.integers(rmin, rmax + 1)
        d2 = sum((g[a] - c[a]) ** 2 for a in range(3))
        take = (d2 <= r * r) & (d2 < best)
        out[take] = i
        best[take] = d2[take]
    return out.reshape(shape)


_CASES = {}
PIECES = "ids in two and three pieces, 3 x 6x10x40"


def cases():
    """{name: (t, n_max)}: ``t`` is ``(B, *sample)``, float32 unless named otherwise; ids reused across the samples of a batch on purpose."""
    if _CASES:
        return _CASES
    c = _CASES
    a = blobs((13, 22, 37), 9, 1) * 3                                     # ids with gaps: 3, 6 .. 27; 27 = n_max
    b3 = np.stack([a, blobs((13, 22, 37), 9, 2) * 3, np.where(a == 6, 3, a)])           # sample 2: ids 3 and 6 merged - the two blobs touch, so ONE larger piece
    c["blobs 3 x 13x22x37, gaps, n_max = an id"] = (b3.astype(np.float32), 27)
    c["blobs 1 x 13x22x37 uint8"] = (b3[:1].astype(np.uint8), 27)
    c["blobs 2 x 13x22x37 int32, ids above n_max"] = (b3[:2].astype(np.int32), 20)
    c["2-D 3 x 45x50"] = (np.stack([blobs((45, 50), 7, s, 3, 9) for s in (3, 4, 5)]).astype(np.float32), 7)
    c["2-D as Z = 1, 1 x 1x45x50"] = (blobs((1, 45, 50), 7, 3, 3, 9)[None].astype(np.float32), 7)
    c["tiny 3 x 3x5x7"] = (np.stack([blobs((3, 5, 7), 3, s, 1, 3) for s in (6, 7, 8)]).astype(np.float32), 3)
    c["8^3, every voxel its own id"] = ((1 + np.arange(512, dtype=np.int32)).reshape(1, 8, 8, 8).astype(np.float32), 512)
    c["8^3 blobs"] = (blobs((8, 8, 8), 4, 9, 2, 4)[None].astype(np.float32), 4)
    c["64^3 blobs"] = (blobs((64, 64, 64), 40, 10, 5, 14)[None].astype(np.float32), 40)
    for x in (63, 64, 65, 255, 256, 257):
        rows = blobs((2, 3, x), 5, x, 2, 12)
        rows[0, 1, :] = 5                                                 # one id through a whole row
        c[f"rows 1 x 2x3x{x}"] = (rows[None].astype(np.float32), 5)
    c["all background"] = (np.zeros((2, 4, 6, 10), np.float32), 5)
    full = np.full((2, 3, 5, 7), 2, np.float32)
    full[1, 0, 0, 0] = 0
    c["an instance filling its sample"] = (full, 2)
    c["n_max = 0 under ids"] = (b3[:1].astype(np.float32), 0)
    bad = b3.astype(np.float32).copy()
    bad[0, 0, 0, :6] = (28.0, -1.0, 2.5, np.nan, np.inf, -np.inf)         # n_max + 1, negative, a fraction, NaN, +-inf
    bad[1, 5, 5, 5] = 2.5
    bad[2, 12, 21, 36] = np.nan
    c["values that are no id"] = (bad, 27)
    two = np.zeros((1, 4, 9, 12), np.float32)
    two[0, :, 2:7, 1:6] = 1
    two[0, :, 2:7, 6:11] = 2                                              # two touching boxes
    c["two touching instances"] = (two, 2)
    pieces = np.zeros((3, 6, 10, 40), np.float32)                         # PIECES: ids whose voxels form two or three pieces that do not touch
    pieces[0, 1:5, 2:8, 2:9] = pieces[0, 0:3, 4:10, 27:38] = 1            # sample 0: id 1 in two boxes far apart along x, id 2 between them
    pieces[0, 2:6, 0:5, 14:20] = 2
    pieces[1, 0:2, :, 5:30] = pieces[1, 4:6, 3:9, 10:36] = 2              # sample 1: id 2 in two slabs apart along z, id 1 in three
    pieces[1, 3, 0, 0] = pieces[1, 3, 9, 39] = pieces[1, 2:4, 4:6, 0:3] = 1
    pieces[2, :, :, 0:3] = pieces[2, :, :, 37:40] = 3                     # sample 2: id 3 on two opposite faces, id 1 one voxel off a corner of id 2
    pieces[2, 2:4, 2:5, 10:20] = 2
    pieces[2, 4, 5, 20] = 1
    c[PIECES] = (pieces, 3)
    for v in c.values():
        v[0].setflags(write=False)
    return c


"""The statement of ``biapy_amd.augment`` in NumPy / torch on the CPU (helper of test_augment_cpu.py / test_augment_gpu.py, no test itself):
a Philox4x32-10 host twin, ``draw`` (the records of a call, bit for bit what ``bpx_aug_draw`` writes), ``apply`` (the output of given records in
torch fp32 operations, in the stated order, without the noise term) and the fp64 mean.  Stream ids and keying: the head of csrc/augment.hip."""
import numpy as np
import torch

REC = 32
F_ZFLIP, F_VFLIP, F_HFLIP, K_SHIFT, F_CONTRAST, F_BRIGHTNESS, F_NOISE, NBOX_SHIFT = 1, 2, 4, 3, 0x20, 0x40, 0x80, 8
W_FLAGS, W_A, W_B, W_S, W_M, W_CTR, W_BOX = 0, 1, 2, 3, 4, 5, 8
EN_ROT90, EN_ZFLIP, EN_VFLIP, EN_HFLIP, EN_CONTRAST, EN_BRIGHTNESS, EN_NOISE, EN_CUTOUT = (1 << i for i in range(8))
EN_ALL = 0xFF
NOISE_KEY_XOR = 0x4E4F4953
_M32 = np.uint64(0xFFFFFFFF)
_2M24 = np.float32(2.0 ** -24)

# the seed of the noise statistics (test_augment_gpu case 5); test_augment_cpu checks that a correct generator meets the five-sigma conditions with it
NOISE_SEED = 20240607
NOISE_SHAPE = (3, 5, 72, 72, 3)          # S1 with C = 3: 233,280 elements


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counter words (arrays or scalars, broadcast) and key words (scalars) -> four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3)))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                      # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _M32, p1 >> np.uint64(32), p1 & _M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def _uniform(r, lo, hi):
    lo, hi = np.float32(lo), np.float32(hi)
    u = (r >> np.uint32(8)).astype(np.float32) * _2M24
    return np.minimum(lo + u * np.float32(hi - lo), hi).astype(np.float32)


def _below(r, n):
    return ((r.astype(np.uint64) * np.asarray(n, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)


def _extent(r, lo, hi, dim):
    e = np.floor(_uniform(r, lo, hi) * np.float32(dim)).astype(np.int64)
    return np.clip(e, 1, dim)


def draw(seed, counter, B, shape, config):
    """records (B, 32) int32 of the call that draws with ``counter``; shape = (Z, Y, X); config = ``DeviceAugmenter.config()``."""
    Z, Y, X = shape
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    cl, ch = counter & 0xFFFFFFFF, (counter >> 32) & 0xFFFFFFFF
    en, thr = config["enable"], np.uint64(config["thr"])
    b = np.arange(B, dtype=np.uint64)

    def stream(i):
        return philox4x32_10(b, i, cl, ch, k0, k1)

    def fires(r, bit):
        return (r.astype(np.uint64) < thr) & bool(en & bit)

    w = np.zeros((B, REC), dtype=np.uint32)
    r, q = stream(0), stream(1)
    flags = np.zeros(B, dtype=np.uint32)
    flags |= np.where(fires(r[0], EN_ROT90), (q[0] >> np.uint32(30)) << np.uint32(K_SHIFT), 0).astype(np.uint32)
    if Z > 1:
        flags |= np.where(fires(r[1], EN_ZFLIP), F_ZFLIP, 0).astype(np.uint32)
    flags |= np.where(fires(r[2], EN_VFLIP), F_VFLIP, 0).astype(np.uint32)
    flags |= np.where(fires(r[3], EN_HFLIP), F_HFLIP, 0).astype(np.uint32)
    flags |= np.where(fires(q[1], EN_CONTRAST), F_CONTRAST, 0).astype(np.uint32)
    flags |= np.where(fires(q[2], EN_BRIGHTNESS), F_BRIGHTNESS, 0).astype(np.uint32)
    flags |= np.where(fires(q[3], EN_NOISE), F_NOISE, 0).astype(np.uint32)
    r = stream(2)
    if en & EN_CONTRAST:
        w[:, W_A] = (np.float32(1) + _uniform(r[0], *config["contrast"])).astype(np.float32).view(np.uint32)
    if en & EN_BRIGHTNESS:
        w[:, W_B] = _uniform(r[1], *config["brightness"]).view(np.uint32)
    if en & EN_NOISE:
        w[:, W_S] = _uniform(r[2], *config["noise"]).view(np.uint32)
    cut = fires(r[3], EN_CUTOUT)
    n_lo, n_hi = config["box"]
    nb = np.where(cut, n_lo + _below(stream(3)[0], n_hi - n_lo + 1), 0)
    flags |= (nb.astype(np.uint32) << np.uint32(NBOX_SHIFT))
    f_lo, f_hi = config["size"]
    for i in range(4):
        r, q = stream(4 + i), stream(8 + i)
        on = i < nb
        ext = [_extent(r[a], f_lo, f_hi, d) for a, d in enumerate((Z, Y, X))]
        org = [_below(q[a], d - e + 1) for a, (d, e) in enumerate(zip((Z, Y, X), ext))]
        for a in range(3):
            w[:, W_BOX + 6 * i + a] = np.where(on, org[a], 0).astype(np.uint32)
            w[:, W_BOX + 6 * i + 3 + a] = np.where(on, ext[a], 0).astype(np.uint32)
    w[:, W_FLAGS] = flags
    w[:, W_CTR], w[:, W_CTR + 1] = cl, ch
    return w.view(np.int32)


def make_record(k=0, zflip=False, vflip=False, hflip=False, a=None, b=None, s=None, boxes=(), counter=0):
    """One record (32 int32) with the given draws; a / b / s not None set their 'fired' bits."""
    w = np.zeros(REC, dtype=np.uint32)
    flags = (k << K_SHIFT) | (F_ZFLIP if zflip else 0) | (F_VFLIP if vflip else 0) | (F_HFLIP if hflip else 0) | (len(boxes) << NBOX_SHIFT)
    for v, bit, word in ((a, F_CONTRAST, W_A), (b, F_BRIGHTNESS, W_B), (s, F_NOISE, W_S)):
        if v is not None:
            flags |= bit
            w[word] = np.float32(v).view(np.uint32)
    w[W_FLAGS] = flags
    w[W_CTR], w[W_CTR + 1] = counter & 0xFFFFFFFF, (counter >> 32) & 0xFFFFFFFF
    for i, box in enumerate(boxes):
        w[W_BOX + 6 * i:W_BOX + 6 * i + 6] = np.asarray(box, dtype=np.uint32)
    return w.view(np.int32)


def parse(rec):
    """A record -> dict of its fields."""
    w = np.asarray(rec, dtype=np.int32).view(np.uint32)
    f = int(w[W_FLAGS])
    nb = (f >> NBOX_SHIFT) & 7
    fl = w[1:5].view(np.float32)
    return dict(zflip=bool(f & F_ZFLIP), vflip=bool(f & F_VFLIP), hflip=bool(f & F_HFLIP), k=(f >> K_SHIFT) & 3, contrast=bool(f & F_CONTRAST),
                brightness=bool(f & F_BRIGHTNESS), noise=bool(f & F_NOISE), nbox=nb, a=fl[0], b=fl[1], s=fl[2], m=fl[3],
                counter=int(w[W_CTR]) | (int(w[W_CTR + 1]) << 32), reserved=int(w[7]),
                boxes=[tuple(int(v) for v in w[W_BOX + 6 * i:W_BOX + 6 * i + 6].view(np.int32)) for i in range(nb)])


def geometry(v, rec):
    """rot90 over (Y, X) then the flips, of one sample (Z, Y, X, C)."""
    p = rec if isinstance(rec, dict) else parse(rec)
    v = torch.rot90(v, p["k"], dims=(1, 2))
    dims = [d for d, on in ((0, p["zflip"]), (1, p["vflip"]), (2, p["hflip"])) if on]
    return torch.flip(v, dims) if dims else v


def mean32(x):
    """float32 rounding of the fp64 mean of every sample of x (B, ...) -> float32 array (B,)."""
    return x.reshape(x.shape[0], -1).to(torch.float64).mean(dim=1).to(torch.float32).numpy()


def apply(x, t, records, m, cval=0.0, apply_to_mask=False):
    """(x', t') of CPU tensors x (B,Z,Y,X,C) float32 and t (B,Z,Y,X,Ct) under ``records`` with the sample means ``m`` (float32, (B,)), in torch
    fp32 operations in the stated order.  The noise term is NOT added (its samples are the device's own): compare such samples outside of it."""
    xo, to = torch.empty_like(x), torch.empty_like(t)
    for b in range(x.shape[0]):
        p = parse(records[b])
        v, u = geometry(x[b], p).clone(), geometry(t[b], p).clone()
        if p["contrast"]:
            mm = torch.tensor(m[b], dtype=torch.float32)
            v = (v - mm) * torch.tensor(p["a"], dtype=torch.float32) + mm
        if p["brightness"]:
            v = v + torch.tensor(p["b"], dtype=torch.float32)
        for z0, y0, x0, dz, dy, dx in p["boxes"]:
            v[z0:z0 + dz, y0:y0 + dy, x0:x0 + dx] = cval
            if apply_to_mask:
                u[z0:z0 + dz, y0:y0 + dy, x0:x0 + dx] = 0
        xo[b], to[b] = v, u
    return xo, to


def box_mask(records, shape):
    """bool (B, Z, Y, X): the voxels inside a cutout box."""
    B = len(records)
    mask = torch.zeros((B,) + tuple(shape), dtype=torch.bool)
    for b in range(B):
        for z0, y0, x0, dz, dy, dx in parse(records[b])["boxes"]:
            mask[b, z0:z0 + dz, y0:y0 + dy, x0:x0 + dx] = True
    return mask


def noise_normals(seed, counter, sample, n):
    """The N(0, 1) values of output elements 0 .. n-1 of ``sample`` (float64, NumPy's Box-Muller on the twin's uniform stream)."""
    blk = np.arange((n + 3) // 4, dtype=np.uint64)
    r = philox4x32_10(blk & _M32, (blk >> np.uint64(32)) ^ np.uint64((sample << 8) & 0xFFFFFFFF), counter & 0xFFFFFFFF, (counter >> 32) & 0xFFFFFFFF,
                      (seed & 0xFFFFFFFF) ^ NOISE_KEY_XOR, (seed >> 32) & 0xFFFFFFFF)
    out = np.empty((len(blk), 4), dtype=np.float64)
    for p in range(2):
        u1 = ((r[2 * p] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (r[2 * p + 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        rad = np.sqrt(-2.0 * np.log(u1))
        out[:, 2 * p], out[:, 2 * p + 1] = rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2)
    return out.reshape(-1)[:n]


def noise_stats(d):
    """The five figures of the noise test from d (B, Z, Y, X, C) float64: mean, variance, lag-1 autocorrelation along X, correlation of samples
    0 and 1, max |d|."""
    n = d.size
    mean, var = d.mean(), d.var()
    c = d - mean
    lag = (c[:, :, :, 1:] * c[:, :, :, :-1]).mean() / var
    cross = (c[0] * c[1]).mean() / var
    return dict(n=n, mean=float(mean), var=float(var), lag1=float(lag), cross=float(cross), max=float(np.abs(d).max()))


def noise_bounds(n):
    return dict(mean=5 / np.sqrt(n), var=5 * np.sqrt(2 / n), lag1=5 / np.sqrt(n), cross=5 / np.sqrt(n), max=np.sqrt(48 * np.log(2)) + 1e-3)

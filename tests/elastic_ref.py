"""The statement of the elastic deformation of ``biapy_amd.augment`` (step 0b) in NumPy on the CPU (helper of test_elastic_cpu.py /
test_elastic_gpu.py, no test itself): ``draw`` (the elastic records of a call, bit for bit what ``bpx_elastic_draw`` writes), ``noise`` (the
uniform field ``bpx_elastic_noise`` fills, Philox through augment_ref's host twin), ``smooth`` (tests/gauss_ref.py's bit-for-bit twin of
``bpx_sepfilter`` on the field seen as a (2B, Y, X) volume) and ``apply`` (the deformed pair of given records and a given smoothed field, every
coordinate and every interpolation step one fp32 operation in the stated association, the border rule warp_ref.tap_index - bit for bit what
``bpx_elastic_apply`` writes).

THE BOUND of ``apply`` against a float64 evaluation of the same taps at the same fp32 field (``image_bound``, counted from the twin's own
operations, u = 2^-24 per fp32 operation, first order, nothing fitted):

    coordinate   f = fl(y + fl(alpha s)): the product's rounding u |alpha s| and the sum's u |f|:  e_f = u (|alpha s| + |f|)
    weights      w = f - floor(f) is exact in fp32 when floor(f) is the floor of the exact coordinate too (Sterbenz / same binade); it carries
                 the coordinate's error e_f.  1 - w adds one rounding: e_u = e_f + u
    top / bot    v00 (1-w) + v01 w: the taps are exact; each product rounds (u |v| |weight|), the sum rounds (u |top|), and the weights' errors
                 enter as (|v00| + |v01|) e_wx:  e_top = (|v00| + |v01|) (e_wx + u) + 2 u (|v00| + |v01|)   [generous: |weight| <= 1]
    out          top (1-wy) + bot wy: likewise  e_out = e_top + e_bot + (|top| + |bot|) (e_wy + u) + 2 u (|top| + |bot|)

A voxel whose coordinate lies within e_f of an integer may take other taps than the float64 reference (bilinear interpolation is continuous
there, so the value error stays of the order of e_f times the local slope and the bound's weight terms cover it); for the nearest-voxel target
a coordinate whose f + 0.5 lies within e_f + u |f + 0.5| of an integer may round to the other voxel: ``near_tie`` marks those."""
import numpy as np
import torch

import augment_ref as AR
import gauss_ref as GR
import warp_ref as WR

REC = 8
F_FIRED = 1
W_FLAGS, W_ALPHA, W_CTR = 0, 1, 2
STREAM, KEY_XOR = 24, 0x454C4153
LIM = WR.LIM
U32 = 2.0 ** -24
_F1, _H = np.float32(1), np.float32(0.5)


# ---- draws ----------------------------------------------------------------------------------------------------------------------------------
def draw(seed, counter, B, config):
    """records (B, 8) int32 of the call that draws with ``counter``; config = ``DeviceAugmenter.elastic_config()``."""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    cl, ch = counter & 0xFFFFFFFF, (counter >> 32) & 0xFFFFFFFF
    r = AR.philox4x32_10(np.arange(B, dtype=np.uint64), STREAM, cl, ch, k0, k1)
    fired = r[0].astype(np.uint64) < np.uint64(config["thr"])
    alpha = np.where(fired, AR._uniform(r[1], *config["alpha"]), np.float32(0)).astype(np.float32)
    w = np.zeros((B, REC), dtype=np.uint32)
    w[:, W_FLAGS] = np.where(fired, F_FIRED, 0)
    w[:, W_ALPHA] = alpha.view(np.uint32)
    w[:, W_CTR], w[:, W_CTR + 1] = cl, ch
    return w.view(np.int32)


def make_records(alphas, fired=None, counter=0):
    """(B, 8) int32 with the given alphas (any floats, rounded to fp32); ``fired``: per-sample flags (default: all 1)."""
    alphas = np.asarray(alphas, dtype=np.float32)
    w = np.zeros((len(alphas), REC), dtype=np.uint32)
    w[:, W_FLAGS] = 1 if fired is None else np.asarray(fired, dtype=np.uint32)
    w[:, W_ALPHA] = alphas.view(np.uint32)
    w[:, W_CTR], w[:, W_CTR + 1] = counter & 0xFFFFFFFF, (counter >> 32) & 0xFFFFFFFF
    return w.view(np.int32)


# ---- the field ------------------------------------------------------------------------------------------------------------------------------
def noise(seed, counter, B, Y, X):
    """float32 (B, 2, Y, X): element e of sample b is u * 2 - 1, u = (r >> 8) * 2^-24, r word e % 4 of the block q = e // 4."""
    n = 2 * Y * X
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    out = np.empty((B, n), dtype=np.float32)
    for b in range(B):
        r = AR.philox4x32_10(q & AR._M32, (q >> np.uint64(32)) ^ np.uint64((b << 8) & 0xFFFFFFFF), counter & 0xFFFFFFFF, (counter >> 32) & 0xFFFFFFFF,
                             (seed & 0xFFFFFFFF) ^ KEY_XOR, (seed >> 32) & 0xFFFFFFFF)
        u = (np.stack(r, axis=1).reshape(-1)[:n] >> np.uint32(8)).astype(np.float32) * AR._2M24
        out[b] = u * np.float32(2) - _F1
    return out.reshape(B, 2, Y, X)


def smooth(field, sigma):
    """The smoothed field: gauss_ref's twin of bpx_sepfilter on (2B, Y, X), z skipped, y and x with the Gaussian weights of radius
    int(4 sigma + 0.5), mode reflect."""
    B, _, Y, X = field.shape
    w = GR.gaussian_weights(float(sigma), 0, int(4.0 * float(sigma) + 0.5))
    return GR.separable_ref(np.ascontiguousarray(field, dtype=np.float32).reshape(2 * B, Y, X), [None, w, w], "reflect").reshape(B, 2, Y, X)


# ---- the apply ------------------------------------------------------------------------------------------------------------------------------
def source_coords(alpha, s):
    """(fy, fx) float32 (Y, X) of the fp32 alpha and the smoothed field s (2, Y, X) of one sample."""
    alpha = np.float32(alpha)
    s = np.asarray(s, dtype=np.float32)
    Y, X = s.shape[1:]
    with np.errstate(all="ignore"):
        fy = np.arange(Y, dtype=np.float32)[:, None] + alpha * s[0]
        fx = np.arange(X, dtype=np.float32)[None, :] + alpha * s[1]
    return np.fmin(np.fmax(fy, -LIM), LIM).astype(np.float32), np.fmin(np.fmax(fx, -LIM), LIM).astype(np.float32)


def apply(x, t, records, field, mode="constant", cval=0.0):
    """(x', t') of CPU tensors x (B,Z,Y,X,C) float32 and t (B,Z,Y,X,Ct) float32 / uint8 under elastic ``records`` (B, 8) and the smoothed
    ``field`` (B, 2, Y, X)."""
    xn, tn = x.numpy(), t.numpy()
    field = np.asarray(field, dtype=np.float32)
    xo, to = np.empty_like(xn), np.empty_like(tn)
    Y, X = xn.shape[2], xn.shape[3]
    cv = np.float32(cval)
    for b in range(xn.shape[0]):
        w = np.asarray(records[b], dtype=np.int32).view(np.uint32)
        if w[W_FLAGS] == 0:
            xo[b], to[b] = xn[b], tn[b]
            continue
        fy, fx = source_coords(w[W_ALPHA:W_ALPHA + 1].view(np.float32)[0], field[b])
        y0, x0 = np.floor(fy), np.floor(fx)
        wy, wx = (fy - y0)[None, :, :, None], (fx - x0)[None, :, :, None]
        (ya, iy0), (yb, iy1) = WR.tap_index(y0.astype(np.int64), Y, mode), WR.tap_index(y0.astype(np.int64) + 1, Y, mode)
        (xa, ix0), (xb, ix1) = WR.tap_index(x0.astype(np.int64), X, mode), WR.tap_index(x0.astype(np.int64) + 1, X, mode)

        def tap(yi, xi, inside):
            return np.where(inside[None, :, :, None], xn[b][:, yi, xi, :], cv)

        with np.errstate(all="ignore"):
            ux, uy = _F1 - wx, _F1 - wy
            top = tap(ya, xa, iy0 & ix0) * ux + tap(ya, xb, iy0 & ix1) * wx
            bot = tap(yb, xa, iy1 & ix0) * ux + tap(yb, xb, iy1 & ix1) * wx
            xo[b] = top * uy + bot * wy
        yn, iy = WR.tap_index(np.floor(fy + _H).astype(np.int64), Y, mode)
        xv, ix = WR.tap_index(np.floor(fx + _H).astype(np.int64), X, mode)
        to[b] = np.where((iy & ix)[None, :, :, None], tn[b][:, yn, xv, :], tn.dtype.type(0))
    return torch.from_numpy(xo), torch.from_numpy(to)


# ---- the float64 statement on one plane and the counted bound ---------------------------------------------------------------------------------
def coords64(alpha, s):
    """The exact coordinates of the fp32 alpha and field, float64 (no rounding: a 24-bit by 24-bit product and a sum of this size are exact)."""
    s = np.asarray(s, dtype=np.float64)
    Y, X = s.shape[1:]
    a = float(np.float32(alpha))
    return np.arange(Y, dtype=np.float64)[:, None] + a * s[0], np.arange(X, dtype=np.float64)[None, :] + a * s[1]


def coord_error(alpha, s):
    """(e_fy, e_fx): the bound on |fp32 coordinate - exact coordinate|, float64 (Y, X): the module docstring."""
    fy, fx = coords64(alpha, s)
    a = abs(float(np.float32(alpha)))
    s = np.abs(np.asarray(s, dtype=np.float64))
    return U32 * (a * s[0] + np.abs(fy)), U32 * (a * s[1] + np.abs(fx))


def image_bound(plane, alpha, s, mode, cval=0.0):
    """Bound on |twin - float64 bilinear interpolation at the exact coordinates| per voxel of one (Y, X) plane, float64: the module docstring.
    The taps' magnitudes are taken at the exact coordinates' cells, the largest of the four taps standing in for each."""
    plane = np.asarray(plane, dtype=np.float64)
    Y, X = plane.shape
    fy, fx = coords64(alpha, s)
    e_y, e_x = coord_error(alpha, s)
    y0, x0 = np.floor(fy).astype(np.int64), np.floor(fx).astype(np.int64)
    mags = []
    for dy in (-1, 0, 1, 2):                                                # the cell and its neighbours: a coordinate within e_f of an integer
        for dx in (-1, 0, 1, 2):                                            # may take the next cell's taps
            (yi, iy), (xi, ix) = WR.tap_index(y0 + dy, Y, mode), WR.tap_index(x0 + dx, X, mode)
            mags.append(np.where(iy & ix, np.abs(plane[yi, xi]), abs(float(cval))))
    v = np.max(mags, axis=0)                                                # every tap, top and bot are at most v in magnitude
    e_wx, e_wy = e_x + U32, e_y + U32
    e_top = 2 * v * (e_wx + U32) + 2 * U32 * 2 * v
    return 2 * e_top + 2 * v * (e_wy + U32) + 2 * U32 * 2 * v


def near_tie(alpha, s):
    """bool (Y, X): f + 0.5 lies within the counted coordinate error (plus the rounding of that sum) of an integer on either axis."""
    fy, fx = coords64(alpha, s)
    e_y, e_x = coord_error(alpha, s)
    out = np.zeros(fy.shape, dtype=bool)
    for f, e in ((fy, e_y), (fx, e_x)):
        g = f + 0.5
        out |= np.abs(g - np.round(g)) <= e + U32 * np.abs(g)
    return out

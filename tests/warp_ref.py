"""The statement of the affine warp of ``biapy_amd.augment`` (step 0) in NumPy on the CPU (helper of test_warp_cpu.py / test_warp_gpu.py, no test
itself): ``draw`` (flags and the drawn parameters of a call, bit for bit what ``bpx_warp_draw`` writes into words 0 and 8-12), ``apply`` (the warped
pair of given warp records, every coordinate and every interpolation step as one fp32 operation in the stated association - bit for bit what
``bpx_warp_apply`` writes), and the fp64 statement of the matrix with the bound on its fp32 evaluation.  Philox and the uniform map: augment_ref.

The bound on words 1-6 (``matrix_bound``), first order on absolute values, u = 2^-24 per fp32 operation:

    arguments   ra = fl(theta * fl(pi/180)): the constant's rounding and the product's are 2u |ra| < |theta| u (theta in DEGREES; the issue's
                figure, generous by a factor of 28), likewise rp from phi
    c, s, t     |c - cos| <= |theta| u |sin| + T ulp(c) with ulp(v) <= 2u |v|; likewise s; |t - tan| <= |phi| u sec^2 + T 2u |tan|.
                T = TRIG_ULP = 4: OCML's documentation of the ulp error of sinf / cosf / tanf is not on the build machine, so the issue's
                fallback of 4 ulp each is used.
    iz = 1/z    u |iz|
    products and sums: e(ab) = |a| e_b + |b| e_a + u |ab|,  e(a + b) = e_a + e_b + u |a + b|
    m00 = iz (c + s t)    m01 = iz s    m10 = iz (c t - s)    m11 = iz c
    m02 = cy - ty Y: cy, ty, Y carry no error (ty is the fp32 word 11 itself): u |ty Y| + u |m02|; likewise m12

evaluated at the fp64 magnitudes; SAFETY = 1.25 (as tests/sgd_bounds.py) covers the second-order terms, FLOOR = 2^-126 the denormal range."""
import numpy as np
import torch

import augment_ref as AR

REC = 16
F_ROT, F_ZOOM, F_SHEAR, F_SHIFT = 1, 2, 4, 8
W_FLAGS, W_M, W_P = 0, 1, 8
MODES = {"constant": 0, "reflect": 1, "edge": 2}
LIM = np.float32(2.0 ** 30)
U32 = 2.0 ** -24
TRIG_ULP = 4.0
SAFETY = 1.25
FLOOR = 2.0 ** -126
_F1, _H = np.float32(1), np.float32(0.5)


# ---- draws ----------------------------------------------------------------------------------------------------------------------------------
def draw(seed, counter, B, config):
    """(flags uint32 (B,), params float32 (B, 5) = theta, z, phi, ty, tx) of the call that draws with ``counter``; config = ``warp_config()``."""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    cl, ch = counter & 0xFFFFFFFF, (counter >> 32) & 0xFFFFFFFF
    en, thr = config["enable"], np.uint64(config["thr"])
    b = np.arange(B, dtype=np.uint64)
    f, u, v = (AR.philox4x32_10(b, s, cl, ch, k0, k1) for s in (16, 17, 18))
    fire = [(f[i].astype(np.uint64) < thr) & bool(en & bit) for i, bit in enumerate((F_ROT, F_ZOOM, F_SHEAR, F_SHIFT))]
    flags = np.zeros(B, dtype=np.uint32)
    for on, bit in zip(fire, (F_ROT, F_ZOOM, F_SHEAR, F_SHIFT)):
        flags |= np.where(on, bit, 0).astype(np.uint32)
    p = np.empty((B, 5), dtype=np.float32)
    p[:, 0] = np.where(fire[0], AR._uniform(u[0], *config["rotation"]), np.float32(0))
    p[:, 1] = np.where(fire[1], AR._uniform(u[1], *config["zoom"]), np.float32(1))
    p[:, 2] = np.where(fire[2], AR._uniform(u[2], *config["shear"]), np.float32(0))
    p[:, 3] = np.where(fire[3], AR._uniform(v[0], *config["shift"]), np.float32(0))
    p[:, 4] = np.where(fire[3], AR._uniform(v[1], *config["shift"]), np.float32(0))
    return flags, p


def matrix64(params, Y, X):
    """The fp64 statement of words 1-6 from the fp32 parameters (B, 5) -> float64 (B, 6)."""
    th, z, ph, ty, tx = (np.asarray(params, dtype=np.float64)[:, i] for i in range(5))
    c, s, t = np.cos(np.deg2rad(th)), np.sin(np.deg2rad(th)), np.tan(np.deg2rad(ph))
    return np.stack([(c + s * t) / z, s / z, (Y - 1) / 2 - ty * Y, (c * t - s) / z, c / z, (X - 1) / 2 - tx * X], axis=1)


def matrix_bound(params, Y, X):
    """Bound on |fp32 word - matrix64| per word, float64 (B, 6): the module docstring."""
    th, z, ph, ty, tx = (np.asarray(params, dtype=np.float64)[:, i] for i in range(5))
    u, T = U32, TRIG_ULP
    c, s, t = np.cos(np.deg2rad(th)), np.sin(np.deg2rad(th)), np.tan(np.deg2rad(ph))
    e_c = np.abs(th) * u * np.abs(s) + T * 2 * u * np.abs(c)
    e_s = np.abs(th) * u * np.abs(c) + T * 2 * u * np.abs(s)
    e_t = np.abs(ph) * u * (1 + t * t) + T * 2 * u * np.abs(t)
    iz = 1 / z
    e_iz = u * np.abs(iz)

    def mul(a, ea, b, eb):
        return np.abs(a) * eb + np.abs(b) * ea + u * np.abs(a * b)

    e_q0 = e_c + mul(s, e_s, t, e_t) + u * np.abs(c + s * t)
    e_q1 = mul(c, e_c, t, e_t) + e_s + u * np.abs(c * t - s)
    e = np.stack([mul(iz, e_iz, c + s * t, e_q0), mul(iz, e_iz, s, e_s), u * np.abs(ty * Y) + u * np.abs((Y - 1) / 2 - ty * Y),
                  mul(iz, e_iz, c * t - s, e_q1), mul(iz, e_iz, c, e_c), u * np.abs(tx * X) + u * np.abs((X - 1) / 2 - tx * X)], axis=1)
    return SAFETY * e + FLOOR


def make_record(m=None, flags=F_ROT, params=(0, 1, 0, 0, 0), plane=None):
    """One warp record (16 int32).  ``m``: the six matrix words, or a 2x2 ``A`` with ``plane = (Y, X)`` for the centred m02 = cy, m12 = cx."""
    w = np.zeros(REC, dtype=np.uint32)
    w[W_FLAGS] = flags
    m = np.asarray(m, dtype=np.float32)
    if m.shape == (2, 2):
        Y, X = plane
        m = np.array([m[0, 0], m[0, 1], (Y - 1) / 2, m[1, 0], m[1, 1], (X - 1) / 2], dtype=np.float32)
    w[W_M:W_M + 6] = m.view(np.uint32)
    w[W_P:W_P + 5] = np.asarray(params, dtype=np.float32).view(np.uint32)
    return w.view(np.int32)


def records_from(flags, params, matrix):
    """(B, 16) int32 of drawn flags, parameters and matrix words (any float array, rounded to fp32)."""
    B = len(flags)
    w = np.zeros((B, REC), dtype=np.uint32)
    w[:, W_FLAGS] = flags
    w[:, W_M:W_M + 6] = np.asarray(matrix, dtype=np.float32).view(np.uint32)
    w[:, W_P:W_P + 5] = np.asarray(params, dtype=np.float32).view(np.uint32)
    return w.view(np.int32)


# ---- the apply ------------------------------------------------------------------------------------------------------------------------------
def tap_index(i, n, mode):
    """(source index, inside) of integer tap indices i on an axis of n voxels; ``inside`` is False only where a constant-mode tap is cval."""
    i = np.asarray(i, dtype=np.int64)
    if mode == "reflect":
        if n == 1:
            return np.zeros_like(i), np.ones(i.shape, dtype=bool)
        p = 2 * n - 2
        r = np.mod(i, p)                                               # non-negative
        return np.where(r < n, r, p - r), np.ones(i.shape, dtype=bool)
    inside = (i >= 0) & (i < n) if mode == "constant" else np.ones(i.shape, dtype=bool)
    return np.clip(i, 0, n - 1), inside


def source_coords(m, Y, X):
    """(fy, fx) float32 (Y, X) of the six fp32 matrix words, one fp32 operation per written operation."""
    m = np.asarray(m, dtype=np.float32)
    cy, cx = np.float32(Y - 1) * _H, np.float32(X - 1) * _H
    dy = (np.arange(Y, dtype=np.float32) - cy)[:, None]
    dx = (np.arange(X, dtype=np.float32) - cx)[None, :]
    with np.errstate(all="ignore"):
        fy = (m[0] * dy + m[1] * dx) + m[2]
        fx = (m[3] * dy + m[4] * dx) + m[5]
    return np.fmin(np.fmax(fy, -LIM), LIM).astype(np.float32), np.fmin(np.fmax(fx, -LIM), LIM).astype(np.float32)


def apply(x, t, warp_records, mode="constant", cval=0.0):
    """(x', t') of CPU tensors x (B,Z,Y,X,C) float32 and t (B,Z,Y,X,Ct) float32 / uint8 under ``warp_records`` (B, 16)."""
    xn, tn = x.numpy(), t.numpy()
    xo, to = np.empty_like(xn), np.empty_like(tn)
    Y, X = xn.shape[2], xn.shape[3]
    cv = np.float32(cval)
    for b in range(xn.shape[0]):
        w = np.asarray(warp_records[b], dtype=np.int32).view(np.uint32)
        if w[W_FLAGS] == 0:
            xo[b], to[b] = xn[b], tn[b]
            continue
        fy, fx = source_coords(w[W_M:W_M + 6].view(np.float32), Y, X)
        y0, x0 = np.floor(fy), np.floor(fx)
        wy, wx = (fy - y0)[None, :, :, None], (fx - x0)[None, :, :, None]
        (ya, iy0), (yb, iy1) = tap_index(y0.astype(np.int64), Y, mode), tap_index(y0.astype(np.int64) + 1, Y, mode)
        (xa, ix0), (xb, ix1) = tap_index(x0.astype(np.int64), X, mode), tap_index(x0.astype(np.int64) + 1, X, mode)

        def tap(yi, xi, inside):
            return np.where(inside[None, :, :, None], xn[b][:, yi, xi, :], cv)

        with np.errstate(all="ignore"):
            ux, uy = _F1 - wx, _F1 - wy
            top = tap(ya, xa, iy0 & ix0) * ux + tap(ya, xb, iy0 & ix1) * wx
            bot = tap(yb, xa, iy1 & ix0) * ux + tap(yb, xb, iy1 & ix1) * wx
            xo[b] = top * uy + bot * wy
        yn, iy = tap_index(np.floor(fy + _H).astype(np.int64), Y, mode)
        xv, ix = tap_index(np.floor(fx + _H).astype(np.int64), X, mode)
        to[b] = np.where((iy & ix)[None, :, :, None], tn[b][:, yn, xv, :], tn.dtype.type(0))
    return torch.from_numpy(xo), torch.from_numpy(to)

"""Training-time augmentation on the device: flips, rot90, brightness, contrast, Gaussian noise and cutout of a batch and its target
in one gather pass (``csrc/augment.hip``).

The reference augments on the CPU inside its data generators (``biapy/data/generators/augmentors.py``); a loader cannot do that to 33 MB of
patches every 8 ms.  ``DeviceAugmenter`` covers the transforms that are a permutation or a per-element map.  The semantics below are the
PRODUCT'S OWN - **parity-unpinned**: the reference's draws are random, and its exact conventions could not be compared on the build machine.

Per sample every enabled transform fires independently with probability ``da_prob``; the output is defined in this order:

0. affine warp in the (Y, X) plane, identically for every z and channel, when ``rotation`` / ``zoom`` / ``shear`` / ``shift`` are given (the
   section "The affine warp" below); image bilinear, target nearest;
0b. elastic deformation in the (Y, X) plane, identically for every z and channel, when ``elastic`` is given (the section "The elastic
   deformation" below); image bilinear, target nearest;
1. geometry, image and target alike: ``v = torch.rot90(src, k, dims=(Y, X))`` with ``k`` uniform in {0, 1, 2, 3} when ``rot90`` fires (else 0),
   then ``torch.flip`` over Z (``zflip``), Y (``vflip``) and X (``hflip``) for the flips that fired - bit for bit a permutation;
2. contrast, image only: ``v = (v - m) * a + m``, ``a = 1 + c`` with ``c`` uniform in ``contrast``, ``m`` the fp32 rounding of the sample's
   mean over all voxels and channels (summed in fp64 in a fixed order);
3. brightness, image only: ``v = v + b``, ``b`` uniform in ``brightness``;
4. Gaussian noise, image only: ``v = v + s * n``, ``s`` uniform in ``gaussian_noise`` per sample, ``n`` ~ N(0, 1) per output element
   (Box-Muller on Philox words, the logarithm's argument is ``((r >> 8) + 1) * 2^-24``);
5. cutout: ``n`` boxes (at most 4) in output coordinates, each extent ``max(1, floor(f * dim))`` with ``f`` uniform in ``size`` per axis, the
   origin uniform over the positions that keep the box inside; the image becomes ``cval`` there, the target 0 only with ``apply_to_mask``.

fp32 throughout, one IEEE operation per written operation, and a step that did not fire is SKIPPED (``(v - m) * 1 + m`` is not ``v``): with
nothing fired the output is bit for bit the input.

The draws of a call are one 32-word record per sample (layout: ``include/biapy_amd.h``), filled on the device from Philox4x32-10 keyed by
``seed`` with the augmenter's own device counter, which advances by one per call.  Nothing is read back, so a call can be captured in a HIP
graph and every replay draws anew.  ``last_records`` / ``records=`` / ``counter`` are the inspection hooks.

The affine warp (step 0; product-defined and parity-unpinned like the rest)
---------------------------------------------------------------------------
``rotation=(lo, hi)`` (degrees), ``zoom=(lo, hi)``, ``shear=(lo, hi)`` (degrees) and ``shift=(lo, hi)`` (fractions of Y and X, ``ty`` and ``tx``
drawn independently) each fire with ``da_prob``; a sample's draw is a WARP RECORD of 16 words (layout: ``include/biapy_amd.h``): word 0 the flags
(bit 0 rotation, 1 zoom, 2 shear, 3 shift), words 1-6 ``m00 m01 m02 m10 m11 m12`` (fp32), words 8-12 the drawn ``theta, z, phi, ty, tx`` with the
neutral 0, 1, 0, 0, 0 where a transform did not fire, the other words 0.  A sample with flags 0 is copied bit for bit (the step is skipped).

Output voxel (y, x) reads the source at, all in fp32 with one IEEE operation per written operation and in exactly this association,
``cy = (Y-1)/2``, ``cx = (X-1)/2``, ``dy = y - cy``, ``dx = x - cx``, ``fy = (m00 dy + m01 dx) + m02``, ``fx = (m10 dy + m11 dx) + m12``, each
clamped to ``[-2^30, 2^30]`` (a NaN becomes a bound).  Image: ``y0 = floor(fy)``, ``wy = fy - y0``, likewise ``x0``, ``wx``; taps ``v00 v01 v10
v11`` at ``(y0, x0) (y0, x0+1) (y0+1, x0) (y0+1, x0+1)``; ``top = v00 (1-wx) + v01 wx``, ``bot = v10 (1-wx) + v11 wx``, ``out = top (1-wy) + bot wy``.
Target: the voxel ``(floor(fy + 0.5), floor(fx + 0.5))``.  The border rule ``affine_mode`` acts on every integer tap index on its own, for an axis
of ``n`` voxels: ``"constant"`` - a tap outside ``[0, n)`` is ``affine_cval`` for the image and 0 for the target; ``"edge"`` - the index is clamped;
``"reflect"`` - ``numpy.pad``'s: index 0 for ``n == 1``, else ``p = 2n - 2``, ``r = i mod p`` (non-negative), the index ``r`` if ``r < n`` else ``p - r``.

The matrix of the drawn parameters, computed in fp32 by the draw kernel:
``A = (1/z) [[cos t, sin t], [-sin t, cos t]] [[1, 0], [tan p, 1]]``, ``m00 m01 m10 m11 = A``, ``m02 = cy - ty Y``, ``m12 = cx - tx X``: zoom > 1
magnifies, and the exact matrix ``[[0, 1], [-1, 0]]`` on a square plane is ``torch.rot90(src, 1, dims=(Y, X))``.  Draws: the key and counter words
of the other draws (the call's counter value is read from words 5-6 of the sample's record), streams 16 (fires), 17 (theta, z, phi) and 18
(ty, tx).  The contrast mean ``m`` stays the mean of the INPUT sample.  With any affine option on, the call launches ``bpx_aug_draw``,
``bpx_warp_draw``, ``bpx_aug_mean`` (contrast only), ``bpx_warp_apply`` into scratch tensors the augmenter owns and ``bpx_aug_apply`` from those
into the output - a second pass over the batch that leaves the gather pass as it is; with none on, exactly the launches listed above.
``last_warp_records`` / ``warp_records=`` are the inspection hooks.

The elastic deformation (step 0b; product-defined and parity-unpinned like the rest)
------------------------------------------------------------------------------------
``elastic=dict(alpha=(12, 16), sigma=4.0, mode="constant", cval=0.0)`` (every key optional): a smooth random displacement field per sample,
scaled by ``alpha`` voxels, ``0 <= lo <= hi <= 1024``; ``sigma`` in ``(0, 8]`` is the Gaussian's (the tap radius ``int(4 sigma + 0.5)`` must not
exceed the 32 ``bpx_sepfilter`` takes); ``mode`` is one of ``AFFINE_MODES`` and ``cval`` the image's value outside in ``"constant"`` mode.  The
step runs after the affine warp, if any, and before the gather pass; a sample fires with ``da_prob``, independently of every other transform.  A
sample's draw is an ELASTIC RECORD of 8 words (layout: ``include/biapy_amd.h``): word 0 the flags (bit 0 fired), word 1 ``alpha`` (fp32, 0 when
the sample did not fire), words 2-3 the call's counter value, the other words 0.  Draws: the key and counter words of the other draws (the
counter value is read from words 5-6 of the sample's record), stream 24: ``r0`` fires, ``r1`` is ``alpha``'s uniform.

The field of a call is a float32 tensor ``(B, 2, Y, X)``, plane 0 ``dy`` and plane 1 ``dx``, fewer than 2^31 elements (``ValueError`` otherwise,
before anything is launched).  Noise: element ``e`` (the linear ``(plane, y, x)`` index within the sample's field) is ``n = u * 2 - 1`` with
``u = (r >> 8) * 2^-24``, ``r`` word ``e mod 4`` of the Philox block with the key ``(seed low ^ 0x454C4153, seed high)`` and the counter words
``(q low, q high ^ (sample << 8), c low, c high)``, ``q = e // 4``: a function of (seed, counter value, sample, element) only.  Smoothing:
``bpx_sepfilter`` on the field seen as a ``(2B, Y, X)`` volume, the z axis skipped, y and x with ``prepost._gaussian_weights(sigma, 0, radius)``
rounded to fp32, mode ``"reflect"`` - the arithmetic ``prepost.separable_filter`` states.  The smoothed field ``s`` is NOT rescaled.

Output voxel (y, x) reads the source at ``fy = y + alpha s[0][y][x]``, ``fx = x + alpha s[1][y][x]`` - fp32, one multiply and one add each, no
FMA - each clamped to ``[-2^30, 2^30]`` (a NaN becomes the lower bound).  From there exactly the warp's rules above: the four bilinear taps and
their association for the image, the voxel ``(floor(fy + 0.5), floor(fx + 0.5))`` for the target, the border rule per integer tap index,
``cval`` for the image and 0 for the target in ``"constant"`` mode.  A sample whose flags are 0 is copied bit for bit; whatever the field holds,
every load stays inside the sample's plane.

With ``elastic`` given the call launches, everything on: ``bpx_aug_draw``, ``bpx_warp_draw``, ``bpx_elastic_draw``, ``bpx_aug_mean``,
``bpx_warp_apply``, ``bpx_elastic_noise``, ``bpx_sepfilter``, ``bpx_elastic_apply``, ``bpx_aug_apply``; the field, its smoothing workspace and
the deformed pair are scratch the augmenter owns and keeps until the shape changes.  The contrast mean ``m`` stays the mean of the INPUT sample.
``last_elastic_records`` / ``last_elastic_field`` (the smoothed, unscaled field of the last call) inspect; ``elastic_records=`` (skips the
draw) and ``elastic_field=`` (skips noise and smoothing) inject.  With ``elastic=None`` nothing of this exists and a call launches what it
launched before.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import _lib as L

lib = L.lib

REC_WORDS = 32
MAX_BOXES = 4
# record word 0 (include/biapy_amd.h)
F_ZFLIP, F_VFLIP, F_HFLIP, K_SHIFT, F_CONTRAST, F_BRIGHTNESS, F_NOISE, NBOX_SHIFT = 1, 2, 4, 3, 0x20, 0x40, 0x80, 8
W_FLAGS, W_A, W_B, W_S, W_M, W_CTR, W_BOX = 0, 1, 2, 3, 4, 5, 8
EN_ROT90, EN_ZFLIP, EN_VFLIP, EN_HFLIP, EN_CONTRAST, EN_BRIGHTNESS, EN_NOISE, EN_CUTOUT = (1 << i for i in range(8))

WARP_REC_WORDS = 16
WF_ROT, WF_ZOOM, WF_SHEAR, WF_SHIFT = 1, 2, 4, 8                 # warp record word 0, and bpx_warp_cfg.enable
WW_FLAGS, WW_M, WW_P = 0, 1, 8
AFFINE_MODES = {"constant": 0, "reflect": 1, "edge": 2}          # BPX_WARP_CONSTANT / _REFLECT / _EDGE
WARP_M_MAX = 2.0 ** 20                                            # |matrix word| accepted through warp_records=

ELASTIC_REC_WORDS = 8
EF_FIRED = 1                                                      # elastic record word 0
EW_FLAGS, EW_ALPHA, EW_CTR = 0, 1, 2
ELASTIC_STREAM, ELASTIC_KEY_XOR = 24, 0x454C4153                  # BPX_ELASTIC_STREAM / _KEY_XOR
ELASTIC_ALPHA_MAX, ELASTIC_SIGMA_MAX, ELASTIC_RADIUS_MAX = 1024.0, 8.0, 32      # the radius limit is bpx_sepfilter's
ELASTIC_FIELD_MAX = 2 ** 31                                       # elements of a call's field: bpx_sepfilter's int32 indices
_ELASTIC_DEFAULTS = dict(alpha=(12.0, 16.0), sigma=4.0, mode="constant", cval=0.0)

_CUTOUT_DEFAULTS = dict(n=(1, 3), size=(0.05, 0.3), cval=0.0, apply_to_mask=False)


def _range(name: str, v) -> Optional[Tuple[float, float]]:
    if v is None:
        return None
    try:
        lo, hi = (float(a) for a in v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a (lo, hi) pair of numbers, got {v!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi:
        raise ValueError(f"{name} must be a finite (lo, hi) range with lo <= hi, got {v!r}")
    return lo, hi


def _bounded(name: str, v, lo: float, hi: float) -> Optional[Tuple[float, float]]:
    r = _range(name, v)
    if r is not None and not (lo <= r[0] and r[1] <= hi):
        raise ValueError(f"{name} must lie within [{lo:g}, {hi:g}], got {v!r}")
    return r


def _contig_strides(shape: Sequence[int]):
    st, acc = [], 1
    for n in reversed(shape):
        st.append(acc)
        acc *= n
    return st[::-1]


def _layout(t: torch.Tensor, name: str):
    """``(memory view (B, [Z,] Y, X, C), channels_first)`` of a batch that is (B,[Z,]Y,X,C)-contiguous or the (B,C,[Z,]Y,X) permuted view of
    such memory.  Strides are compared on the dimensions longer than 1; where both readings fit (only with one channel) the permuted view is
    recognised by its channel stride of 1."""
    nd = t.dim()
    if nd not in (4, 5):
        raise ValueError(f"{name} must have 4 or 5 dimensions, got shape {tuple(t.shape)}")
    perm = (0, *range(2, nd), 1)

    def match(strides):
        return all(s == e for n, s, e in zip(t.shape, t.stride(), strides) if n > 1)

    last = match(_contig_strides(t.shape))
    pst = _contig_strides([t.shape[i] for i in perm])
    first_strides = [0] * nd
    for j, i in enumerate(perm):
        first_strides[i] = pst[j]
    first = match(first_strides)
    if first and last:
        first = t.stride(1) == 1
    if first:
        return t.permute(*perm), True
    if last:
        return t, False
    raise ValueError(f"{name} must be (B,[Z,]Y,X,C)-contiguous or the (B,C,[Z,]Y,X) permuted view of such memory; got shape "
                     f"{tuple(t.shape)} with strides {tuple(t.stride())}")


def _span(t: torch.Tensor):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


class DeviceAugmenter:
    """See the module docstring.  ``aug(x, t, out=None, records=None, warp_records=None, elastic_records=None, elastic_field=None) ->
    (x_out, t_out)``."""

    def __init__(self, *, da_prob: float = 0.5, rot90: bool = False, zflip: bool = False, vflip: bool = False, hflip: bool = False,
                 brightness=None, contrast=None, gaussian_noise=None, cutout=None, seed: Optional[int] = None, rotation=None, zoom=None,
                 shear=None, shift=None, affine_mode: str = "constant", affine_cval: float = 0.0, elastic=None):
        da_prob = float(da_prob)
        if not (0.0 <= da_prob <= 1.0):
            raise ValueError(f"da_prob must lie in [0, 1], got {da_prob}")
        self.da_prob = da_prob
        self.rot90, self.zflip, self.vflip, self.hflip = bool(rot90), bool(zflip), bool(vflip), bool(hflip)
        self.brightness = _range("brightness", brightness)
        self.contrast = _range("contrast", contrast)
        self.gaussian_noise = _range("gaussian_noise", gaussian_noise)
        if self.gaussian_noise is not None and self.gaussian_noise[0] < 0:
            raise ValueError(f"gaussian_noise is a standard-deviation range and cannot be negative, got {gaussian_noise!r}")
        self.cutout = None
        if cutout is not None:
            if not isinstance(cutout, dict):
                raise ValueError(f"cutout must be a dict with the keys {sorted(_CUTOUT_DEFAULTS)}, got {cutout!r}")
            unknown = set(cutout) - set(_CUTOUT_DEFAULTS)
            if unknown:
                raise ValueError(f"cutout has unknown keys {sorted(unknown)}")
            c = {**_CUTOUT_DEFAULTS, **cutout}
            try:
                n_lo, n_hi = (int(v) for v in c["n"])
            except (TypeError, ValueError):
                raise ValueError(f"cutout['n'] must be a (lo, hi) pair of integers, got {c['n']!r}") from None
            if not (1 <= n_lo <= n_hi <= MAX_BOXES):
                raise ValueError(f"cutout['n'] must satisfy 1 <= lo <= hi <= {MAX_BOXES} (at most {MAX_BOXES} boxes), got {c['n']!r}")
            size = _range("cutout['size']", c["size"])
            if not (0.0 < size[0] and size[1] <= 1.0):
                raise ValueError(f"cutout['size'] fractions must lie in (0, 1], got {c['size']!r}")
            cval = float(c["cval"])
            if not math.isfinite(cval):
                raise ValueError(f"cutout['cval'] must be finite, got {c['cval']!r}")
            self.cutout = dict(n=(n_lo, n_hi), size=size, cval=cval, apply_to_mask=bool(c["apply_to_mask"]))
        self.rotation = _bounded("rotation", rotation, -360.0, 360.0)
        self.zoom = _bounded("zoom", zoom, 0.1, 10.0)
        self.shear = _bounded("shear", shear, -60.0, 60.0)
        self.shift = _bounded("shift", shift, -1.0, 1.0)
        if affine_mode not in AFFINE_MODES:
            raise ValueError(f"affine_mode must be one of {sorted(AFFINE_MODES)}, got {affine_mode!r}")
        self.affine_mode = affine_mode
        try:
            self.affine_cval = float(affine_cval)
        except (TypeError, ValueError):
            raise ValueError(f"affine_cval must be a number, got {affine_cval!r}") from None
        if not math.isfinite(self.affine_cval):
            raise ValueError(f"affine_cval must be finite, got {affine_cval!r}")
        self.elastic = None
        if elastic is not None:
            if not isinstance(elastic, dict):
                raise ValueError(f"elastic must be a dict with the keys {sorted(_ELASTIC_DEFAULTS)}, got {elastic!r}")
            unknown = set(elastic) - set(_ELASTIC_DEFAULTS)
            if unknown:
                raise ValueError(f"elastic has unknown keys {sorted(unknown)}")
            e = {**_ELASTIC_DEFAULTS, **elastic}
            alpha = _bounded("elastic['alpha']", e["alpha"], 0.0, ELASTIC_ALPHA_MAX)
            if alpha is None:
                raise ValueError("elastic['alpha'] must be a (lo, hi) pair of numbers, got None")
            try:
                sigma = float(e["sigma"])
            except (TypeError, ValueError):
                raise ValueError(f"elastic['sigma'] must be a number, got {e['sigma']!r}") from None
            if not (math.isfinite(sigma) and 0.0 < sigma <= ELASTIC_SIGMA_MAX):
                raise ValueError(f"elastic['sigma'] must satisfy 0 < sigma <= {ELASTIC_SIGMA_MAX:g}: the tap radius int(4 sigma + 0.5) must not exceed the "
                                 f"{ELASTIC_RADIUS_MAX} voxels bpx_sepfilter takes, got {e['sigma']!r}")
            if e["mode"] not in AFFINE_MODES:
                raise ValueError(f"elastic['mode'] must be one of {sorted(AFFINE_MODES)}, got {e['mode']!r}")
            try:
                ecval = float(e["cval"])
            except (TypeError, ValueError):
                raise ValueError(f"elastic['cval'] must be a number, got {e['cval']!r}") from None
            if not math.isfinite(ecval):
                raise ValueError(f"elastic['cval'] must be finite, got {e['cval']!r}")
            self.elastic = dict(alpha=alpha, sigma=sigma, mode=e["mode"], cval=ecval)
            radius = int(4.0 * sigma + 0.5)
            from .prepost import _gaussian_weights

            self._ew = np.ascontiguousarray(_gaussian_weights(sigma, 0, radius).astype(np.float32))   # y and x alike, computed once
        if seed is None:
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
            seed = torch.initial_seed() + rank                        # ranks draw differently
        try:
            self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        except (TypeError, ValueError):
            raise ValueError(f"seed must be an integer, got {seed!r}") from None
        self._state = None            # int64[2] on the device: [counter, ticket of the draw kernel]
        self._records = None
        self._ws = None
        self._warp = None             # int32 (B, 16): the warp records
        self._wx = self._wt = None    # the warped pair, input of the gather pass
        self._erec = None             # int32 (B, 8): the elastic records
        self._efield = None           # float32 (B, 2, Y, X): the smoothed field
        self._ews = None              # float32 (2, B, 2, Y, X): the noise, then bpx_sepfilter's workspace
        self._ex = self._et = None    # the deformed pair, input of the gather pass

    # ---- configuration --------------------------------------------------------------------------------------------------------
    @property
    def enable_mask(self) -> int:
        m = 0
        for on, bit in ((self.rot90, EN_ROT90), (self.zflip, EN_ZFLIP), (self.vflip, EN_VFLIP), (self.hflip, EN_HFLIP),
                        (self.contrast is not None, EN_CONTRAST), (self.brightness is not None, EN_BRIGHTNESS),
                        (self.gaussian_noise is not None, EN_NOISE), (self.cutout is not None, EN_CUTOUT)):
            if on:
                m |= bit
        return m

    def config(self) -> dict:
        """The draw parameters as plain numbers (what ``bpx_aug_cfg`` carries; ``tests/augment_ref.draw`` takes the same dict)."""
        cut = self.cutout or dict(n=(1, 1), size=(1.0, 1.0), cval=0.0, apply_to_mask=False)
        return dict(seed=self.seed, thr=int(math.floor(self.da_prob * 2.0 ** 32)), enable=self.enable_mask, box=cut["n"],
                    contrast=self.contrast or (0.0, 0.0), brightness=self.brightness or (0.0, 0.0), noise=self.gaussian_noise or (0.0, 0.0),
                    size=cut["size"])

    @property
    def warp_enable_mask(self) -> int:
        return sum(bit for on, bit in ((self.rotation, WF_ROT), (self.zoom, WF_ZOOM), (self.shear, WF_SHEAR), (self.shift, WF_SHIFT)) if on is not None)

    def warp_config(self) -> dict:
        """The warp's draw parameters as plain numbers (what ``bpx_warp_cfg`` carries; ``tests/warp_ref.draw`` takes the same dict)."""
        return dict(seed=self.seed, thr=int(math.floor(self.da_prob * 2.0 ** 32)), enable=self.warp_enable_mask, rotation=self.rotation or (0.0, 0.0),
                    zoom=self.zoom or (1.0, 1.0), shear=self.shear or (0.0, 0.0), shift=self.shift or (0.0, 0.0))

    def _warp_cfg_struct(self) -> "L.WarpCfg":
        c = self.warp_config()
        return L.WarpCfg(c["seed"], c["thr"], c["enable"], 0, *c["rotation"], *c["zoom"], *c["shear"], *c["shift"])

    def elastic_config(self) -> Optional[dict]:
        """The elastic step's parameters as plain numbers (``tests/elastic_ref.draw`` takes the same dict); ``None`` without ``elastic=``."""
        if self.elastic is None:
            return None
        return dict(seed=self.seed, thr=int(math.floor(self.da_prob * 2.0 ** 32)), alpha=self.elastic["alpha"], sigma=self.elastic["sigma"],
                    radius=(len(self._ew) - 1) // 2, mode=self.elastic["mode"], cval=self.elastic["cval"])

    def _cfg_struct(self) -> "L.AugCfg":
        c = self.config()
        return L.AugCfg(c["seed"], c["thr"], c["enable"], c["box"][0], c["box"][1], *c["contrast"], *c["brightness"], *c["noise"], *c["size"])

    @classmethod
    def from_cfg(cls, cfg, seed: Optional[int] = None, *, affine: bool = False, elastic: bool = False) -> Optional["DeviceAugmenter"]:
        """The augmenter a reference configuration asks for, ``None`` when ``AUGMENTOR.ENABLE`` is false.

        Mapped ``AUGMENTOR`` keys: ``DA_PROB``; ``ROT90``, ``ZFLIP``, ``VFLIP``, ``HFLIP``; ``BRIGHTNESS`` + ``BRIGHTNESS_FACTOR``; ``CONTRAST`` +
        ``CONTRAST_FACTOR``; ``GAUSSIAN_NOISE`` + ``GAUSSIAN_NOISE_STD`` (a range; this package's own key) or the reference's scalar
        ``GAUSSIAN_NOISE_VAR`` (the fixed deviation ``sqrt(var)``); ``CUTOUT`` + ``COUT_NB_ITERATIONS``, ``COUT_SIZE``, ``COUT_CVAL``,
        ``COUT_APPLY_TO_MASK``.  Any OTHER switch of the node that is ``True`` (``RANDOM_ROT``, ``ELASTIC``, ``ZOOM``, ``SHEAR``, ``G_BLUR``,
        ``GAMMA_CONTRAST``, ...) raises ``NotImplementedError`` naming it: a run never silently trains with less augmentation than configured.

        ``affine=True`` also maps the affine family onto step 0: ``RANDOM_ROT`` + ``RANDOM_ROT_RANGE`` (degrees), ``ZOOM`` + ``ZOOM_RANGE``
        (``ZOOM_IN_Z`` is refused: the warp acts in the (Y, X) plane), ``SHEAR`` + ``SHEAR_RANGE`` (degrees), ``SHIFT`` + ``SHIFT_RANGE`` (fractions)
        and ``AFFINE_MODE`` (``constant`` / ``reflect`` / ``edge``; ``wrap`` and ``symmetric`` are refused by name; ``reflect`` when the key is
        absent, as the reference's tree is remembered).  It is opt-in because these semantics are this package's own: the default keeps refusing them.

        ``elastic=True`` also maps ``ELASTIC`` onto step 0b: ``E_ALPHA`` (a range), ``E_SIGMA`` (a scalar, used as it is; a range is refused by
        name) and ``E_MODE`` (``constant`` / ``reflect`` / ``edge``; any other is refused by name).  Opt-in for the same reason: the default, and
        ``affine=True`` alone, keep refusing ``ELASTIC``.

        The key names are written from memory of the reference's configuration tree and could not be verified against it on the build machine;
        the semantics of every transform are this package's own (parity-unpinned, see the module docstring)."""
        from .train_engine import _cfg_get

        def get(key, default=None):
            return _cfg_get(cfg, "AUGMENTOR." + key, default)

        if not get("ENABLE", False):
            return None
        node = _cfg_get(cfg, "AUGMENTOR", None)
        if isinstance(node, dict):
            items = dict(node)
        else:
            items = {k: getattr(node, k) for k in dir(node) if k.isupper()}
        for k in _UNSUPPORTED_SWITCHES + (("ZOOM_IN_Z",) if affine else ()):   # also those a node that cannot be listed still answers for
            if k not in items and get(k, False) is True:
                items[k] = True
        for k in sorted(items):
            if items[k] is True and k not in _MAPPED_SWITCHES and k not in _NEUTRAL_SWITCHES and not (affine and k in _AFFINE_SWITCHES) and not (elastic and k == "ELASTIC"):
                raise NotImplementedError(f"AUGMENTOR.{k} is enabled but biapy_amd.augment.DeviceAugmenter does not implement it (supported: "
                                          f"{', '.join(sorted(_MAPPED_SWITCHES - {'ENABLE'}))}); keep this transform in the loader or switch it off")
        kw = dict(da_prob=get("DA_PROB", 0.5), rot90=bool(get("ROT90", False)), zflip=bool(get("ZFLIP", False)),
                  vflip=bool(get("VFLIP", False)), hflip=bool(get("HFLIP", False)), seed=seed)
        if get("BRIGHTNESS", False):
            kw["brightness"] = tuple(get("BRIGHTNESS_FACTOR", (-0.1, 0.1)))
        if get("CONTRAST", False):
            kw["contrast"] = tuple(get("CONTRAST_FACTOR", (-0.1, 0.1)))
        if get("GAUSSIAN_NOISE", False):
            if float(get("GAUSSIAN_NOISE_MEAN", 0.0) or 0.0) != 0.0:
                raise NotImplementedError("AUGMENTOR.GAUSSIAN_NOISE_MEAN other than 0 is not implemented by biapy_amd.augment.DeviceAugmenter")
            std = get("GAUSSIAN_NOISE_STD", None)
            if std is None:
                sd = math.sqrt(float(get("GAUSSIAN_NOISE_VAR", 0.05)))
                std = (sd, sd)
            kw["gaussian_noise"] = tuple(std)
        if get("CUTOUT", False):
            kw["cutout"] = dict(n=tuple(get("COUT_NB_ITERATIONS", (1, 3))), size=tuple(get("COUT_SIZE", (0.05, 0.3))),
                                cval=get("COUT_CVAL", 0.0), apply_to_mask=bool(get("COUT_APPLY_TO_MASK", False)))
        if affine:
            for switch, key, name, default in (("RANDOM_ROT", "RANDOM_ROT_RANGE", "rotation", (-180.0, 180.0)), ("ZOOM", "ZOOM_RANGE", "zoom", (0.8, 1.2)),
                                               ("SHEAR", "SHEAR_RANGE", "shear", (-20.0, 20.0)), ("SHIFT", "SHIFT_RANGE", "shift", (0.1, 0.2))):
                if get(switch, False):
                    kw[name] = tuple(get(key, default))
            mode = str(get("AFFINE_MODE", "reflect"))
            if mode not in AFFINE_MODES:
                raise NotImplementedError(f"AUGMENTOR.AFFINE_MODE = {mode!r} is not implemented by biapy_amd.augment.DeviceAugmenter (supported: "
                                          f"{', '.join(sorted(AFFINE_MODES))})")
            kw["affine_mode"] = mode
        if elastic and get("ELASTIC", False):
            sigma = get("E_SIGMA", _ELASTIC_DEFAULTS["sigma"])
            if isinstance(sigma, (tuple, list)) or hasattr(sigma, "__len__"):
                raise NotImplementedError(f"AUGMENTOR.E_SIGMA = {sigma!r} is a range; biapy_amd.augment.DeviceAugmenter takes one sigma per augmenter "
                                          f"(its weights are computed once): give a scalar")
            emode = str(get("E_MODE", _ELASTIC_DEFAULTS["mode"]))
            if emode not in AFFINE_MODES:
                raise NotImplementedError(f"AUGMENTOR.E_MODE = {emode!r} is not implemented by biapy_amd.augment.DeviceAugmenter (supported: "
                                          f"{', '.join(sorted(AFFINE_MODES))})")
            kw["elastic"] = dict(alpha=tuple(get("E_ALPHA", _ELASTIC_DEFAULTS["alpha"])), sigma=sigma, mode=emode)
        return cls(**kw)

    # ---- state ----------------------------------------------------------------------------------------------------------------
    def _ensure(self, device, B: int) -> None:
        if self._state is None or self._state.device != device:
            self._state = torch.zeros(2, dtype=torch.int64, device=device)
            self._records = None
            self._ws = None
        if self._records is None or self._records.shape[0] != B:
            self._records = torch.zeros((B, REC_WORDS), dtype=torch.int32, device=device)

    @property
    def counter(self) -> torch.Tensor:
        """The device counter (int64 scalar view): the value the NEXT call draws with."""
        if self._state is None:
            self._state = torch.zeros(2, dtype=torch.int64, device=torch.device("cuda", torch.cuda.current_device()))
        return self._state[0]

    @property
    def last_warp_records(self) -> Optional[torch.Tensor]:
        """The ``(B, 16)`` int32 device tensor of the last call's warp records (``None`` before the first call that warps)."""
        return self._warp

    @property
    def last_elastic_records(self) -> Optional[torch.Tensor]:
        """The ``(B, 8)`` int32 device tensor of the last call's elastic records (``None`` before the first call that deforms)."""
        return self._erec

    @property
    def last_elastic_field(self) -> Optional[torch.Tensor]:
        """The ``(B, 2, Y, X)`` float32 device tensor of the last call's smoothed, unscaled field (``None`` before the first call that deforms)."""
        return self._efield

    @property
    def last_records(self) -> Optional[torch.Tensor]:
        """The ``(B, 32)`` int32 device tensor of the last call's records (the augmenter's own buffer, overwritten by the next call)."""
        return self._records

    # ---- the call -------------------------------------------------------------------------------------------------------------
    def __call__(self, x: torch.Tensor, t: torch.Tensor, out=None, *, records: Optional[torch.Tensor] = None,
                 warp_records: Optional[torch.Tensor] = None, elastic_records: Optional[torch.Tensor] = None,
                 elastic_field: Optional[torch.Tensor] = None):
        for name, v in (("x", x), ("t", t)):
            if not torch.is_tensor(v) or not v.is_cuda:
                raise ValueError(f"{name} must be a CUDA/HIP tensor: biapy_amd.augment runs on the device only, there is no CPU path")
        if x.dtype != torch.float32:
            raise ValueError(f"x must be float32, got {x.dtype}")
        if t.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"t must be float32 or uint8, got {t.dtype}")
        if t.device != x.device:
            raise ValueError("x and t must live on the same device")
        xm, x_first = _layout(x, "x")
        tm, t_first = _layout(t, "t")
        if xm.dim() != tm.dim() or tuple(xm.shape[:-1]) != tuple(tm.shape[:-1]):
            raise ValueError(f"x and t must cover the same (B,[Z,]Y,X): {tuple(xm.shape[:-1])} vs {tuple(tm.shape[:-1])}")
        B, C, Ct = xm.shape[0], xm.shape[-1], tm.shape[-1]
        Z, Y, X = (1, *xm.shape[1:-1]) if xm.dim() == 4 else tuple(xm.shape[1:-1])
        if not 1 <= C <= 16:
            raise ValueError(f"x must have 1 to 16 channels, got {C}")
        if not 1 <= Ct <= 8:
            raise ValueError(f"t must have 1 to 8 channels, got {Ct}")
        if min(B, Z, Y, X) < 1:
            raise ValueError(f"empty batch: x has shape {tuple(x.shape)}")
        if self.rot90 and Y != X:
            raise ValueError(f"rot90=True needs square (Y, X) planes, got Y = {Y}, X = {X}")
        if out is None:
            xo, to = torch.empty_like(xm, memory_format=torch.contiguous_format), torch.empty_like(tm, memory_format=torch.contiguous_format)
            x_out = xo.permute(0, xo.dim() - 1, *range(1, xo.dim() - 1)) if x_first else xo
            t_out = to.permute(0, to.dim() - 1, *range(1, to.dim() - 1)) if t_first else to
        else:
            try:
                x_out, t_out = out
            except (TypeError, ValueError):
                raise ValueError("out must be a pair (x_out, t_out)") from None
            for name, o, i in (("out[0]", x_out, x), ("out[1]", t_out, t)):
                if (not torch.is_tensor(o) or o.device != i.device or o.dtype != i.dtype or tuple(o.shape) != tuple(i.shape)
                        or any(a != b for n, a, b in zip(i.shape, o.stride(), i.stride()) if n > 1)):
                    raise ValueError(f"{name} must have the shape, dtype, strides and device of its input")
            xo, to = _layout(x_out, "out[0]")[0], _layout(t_out, "out[1]")[0]
        spans_in, spans_out = [_span(x), _span(t)], [_span(x_out), _span(t_out)]
        for a0, a1 in spans_out:
            for b0, b1 in spans_in:
                if a0 < b1 and b0 < a1:
                    raise ValueError("out overlaps an input: the augmentation is a gather pass and cannot run in place")
        if spans_out[0][0] < spans_out[1][1] and spans_out[1][0] < spans_out[0][1]:
            raise ValueError("out[0] and out[1] overlap")
        if records is not None:
            if (not torch.is_tensor(records) or records.device != x.device or records.dtype != torch.int32
                    or tuple(records.shape) != (B, REC_WORDS) or not records.is_contiguous()):
                raise ValueError(f"records must be a contiguous ({B}, {REC_WORDS}) int32 tensor on the device of x")
        warp = warp_records is not None or self.warp_enable_mask != 0
        if warp_records is not None:                                   # checked on the host: the hook may read back
            if (not torch.is_tensor(warp_records) or warp_records.device != x.device or warp_records.dtype != torch.int32
                    or tuple(warp_records.shape) != (B, WARP_REC_WORDS) or not warp_records.is_contiguous()):
                raise ValueError(f"warp_records must be a contiguous ({B}, {WARP_REC_WORDS}) int32 tensor on the device of x")
            m = warp_records[:, WW_M:WW_M + 6].contiguous().view(torch.float32)
            if not bool((torch.isfinite(m) & (m.abs() <= WARP_M_MAX)).all()):
                raise ValueError(f"warp_records words 1-6 (the matrix) must be finite with |m| <= 2^20, got {m.cpu().tolist()}")

        elastic = self.elastic is not None
        if (elastic_records is not None or elastic_field is not None) and not elastic:
            raise ValueError("elastic_records= and elastic_field= need an augmenter built with elastic=: mode and cval are its")
        if elastic:                                                    # checked on the host, before anything is launched or allocated
            if 2 * B * Y * X >= ELASTIC_FIELD_MAX:
                raise ValueError(f"the elastic field of this batch has 2 * {B} * {Y} * {X} = {2 * B * Y * X} elements; 2^31 or more are not supported")
            if elastic_records is not None and (not torch.is_tensor(elastic_records) or elastic_records.device != x.device
                                                or elastic_records.dtype != torch.int32 or tuple(elastic_records.shape) != (B, ELASTIC_REC_WORDS)
                                                or not elastic_records.is_contiguous()):
                raise ValueError(f"elastic_records must be a contiguous ({B}, {ELASTIC_REC_WORDS}) int32 tensor on the device of x")
            if elastic_field is not None and (not torch.is_tensor(elastic_field) or elastic_field.device != x.device
                                              or elastic_field.dtype != torch.float32 or tuple(elastic_field.shape) != (B, 2, Y, X)
                                              or not elastic_field.is_contiguous()):
                raise ValueError(f"elastic_field must be a contiguous ({B}, 2, {Y}, {X}) float32 tensor on the device of x")

        self._ensure(x.device, B)
        if elastic:
            if self._erec is None or self._erec.shape[0] != B or self._erec.device != x.device:
                self._erec = torch.zeros((B, ELASTIC_REC_WORDS), dtype=torch.int32, device=x.device)
            if self._efield is None or tuple(self._efield.shape) != (B, 2, Y, X) or self._efield.device != x.device:
                self._efield = torch.empty((B, 2, Y, X), dtype=torch.float32, device=x.device)
                self._ews = torch.empty((2, B, 2, Y, X), dtype=torch.float32, device=x.device)
            for name, like in (("_ex", xm), ("_et", tm)):
                buf = getattr(self, name)
                if buf is None or buf.shape != like.shape or buf.dtype != like.dtype or buf.device != like.device:
                    setattr(self, name, torch.empty(like.shape, dtype=like.dtype, device=like.device))
        if warp:
            if self._warp is None or self._warp.shape[0] != B or self._warp.device != x.device:
                self._warp = torch.zeros((B, WARP_REC_WORDS), dtype=torch.int32, device=x.device)
            for name, like in (("_wx", xm), ("_wt", tm)):
                buf = getattr(self, name)
                if buf is None or buf.shape != like.shape or buf.dtype != like.dtype or buf.device != like.device:
                    setattr(self, name, torch.empty(like.shape, dtype=like.dtype, device=like.device))
        s = L.stream_ptr()
        rec = self._records
        if records is None:
            import ctypes

            cfg = self._cfg_struct()
            L.check(lib.bpx_aug_draw(ctypes.addressof(cfg), B, Z, Y, X, self._state.data_ptr(), rec.data_ptr(), s))
        else:
            rec.copy_(records)
        if warp_records is not None:
            self._warp.copy_(warp_records)
        elif warp:
            import ctypes

            wcfg = self._warp_cfg_struct()
            L.check(lib.bpx_warp_draw(ctypes.addressof(wcfg), B, Y, X, rec.data_ptr(), self._warp.data_ptr(), s))
        if elastic_records is not None:
            self._erec.copy_(elastic_records)
        elif elastic:
            ec = self.elastic_config()
            L.check(lib.bpx_elastic_draw(ec["seed"], ec["thr"], ec["alpha"][0], ec["alpha"][1], B, rec.data_ptr(), self._erec.data_ptr(), s))
        if records is not None or self.contrast is not None:           # m is only ever used by the contrast step
            n = Z * Y * X * C
            need = B * int(lib.bpx_aug_mean_blocks(n))
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.float64, device=x.device)
            L.check(lib.bpx_aug_mean(xm.data_ptr(), B, n, self._ws.data_ptr(), rec.data_ptr(), s))
        if warp:                                                       # step 0 into the scratch pair, the gather pass then reads that
            L.check(lib.bpx_warp_apply(xm.data_ptr(), tm.data_ptr(), L.dt_of(t), B, Z, Y, X, C, Ct, self._warp.data_ptr(), AFFINE_MODES[self.affine_mode],
                                       self.affine_cval, self._wx.data_ptr(), self._wt.data_ptr(), s))
            xm, tm = self._wx, self._wt
        if elastic:                                                    # step 0b into its own scratch pair
            if elastic_field is not None:
                self._efield.copy_(elastic_field)
            else:
                r = (len(self._ew) - 1) // 2
                L.check(lib.bpx_elastic_noise(self.seed, B, Y, X, self._erec.data_ptr(), self._ews[0].data_ptr(), s))
                L.check(lib.bpx_sepfilter(self._ews[0].data_ptr(), 2 * B, Y, X, None, -1, self._ew.ctypes.data, r, self._ew.ctypes.data, r, 0, 0.0,
                                          self._efield.data_ptr(), self._ews[1].data_ptr(), self._efield.numel() * 4, s))
            L.check(lib.bpx_elastic_apply(xm.data_ptr(), tm.data_ptr(), L.dt_of(t), B, Z, Y, X, C, Ct, self._erec.data_ptr(), self._efield.data_ptr(),
                                          AFFINE_MODES[self.elastic["mode"]], self.elastic["cval"], self._ex.data_ptr(), self._et.data_ptr(), s))
            xm, tm = self._ex, self._et
        cut = self.cutout or _CUTOUT_DEFAULTS
        L.check(lib.bpx_aug_apply(xm.data_ptr(), tm.data_ptr(), L.dt_of(t), B, Z, Y, X, C, Ct, rec.data_ptr(), self.seed, float(cut["cval"]),
                                  int(bool(cut["apply_to_mask"])), xo.data_ptr(), to.data_ptr(), s))
        return x_out, t_out


# AUGMENTOR switches from_cfg maps, switches that select no transform, and the transforms it refuses by name (from memory of the reference's tree)
_MAPPED_SWITCHES = {"ENABLE", "ROT90", "ZFLIP", "VFLIP", "HFLIP", "BRIGHTNESS", "CONTRAST", "GAUSSIAN_NOISE", "CUTOUT", "COUT_APPLY_TO_MASK"}
_AFFINE_SWITCHES = {"RANDOM_ROT", "ZOOM", "SHEAR", "SHIFT"}         # mapped by from_cfg(affine=True) only
_NEUTRAL_SWITCHES = {"DRAW_GRID", "AUG_SAMPLES", "SHUFFLE_TRAIN_DATA_EACH_EPOCH", "SHUFFLE_VAL_DATA_EACH_EPOCH"}
_UNSUPPORTED_SWITCHES = ("RANDOM_ROT", "ELASTIC", "ZOOM", "SHEAR", "SHIFT", "AFFINE", "G_BLUR", "MEDIAN_BLUR", "MOTION_BLUR", "GAMMA_CONTRAST",
                         "BRIGHTNESS_EM", "CONTRAST_EM", "DROPOUT", "CUTBLUR", "CUTMIX", "CUTNOISE", "MISALIGNMENT", "MISSING_SECTIONS",
                         "GRAYSCALE", "CHANNEL_SHUFFLE", "GRIDMASK", "POISSON_NOISE", "SALT", "PEPPER", "SALT_AND_PEPPER")

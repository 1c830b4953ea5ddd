"""Training-time augmentation on the device: flips, rot90, brightness, contrast, Gaussian noise and cutout of a batch and its target
in one gather pass (``csrc/augment.hip``).

The reference augments on the CPU inside its data generators (``biapy/data/generators/augmentors.py``); a loader cannot do that to 33 MB of
patches every 8 ms.  ``DeviceAugmenter`` covers the transforms that are a permutation or a per-element map.  The semantics below are the
PRODUCT'S OWN - **parity-unpinned**: the reference's draws are random, and its exact conventions could not be compared on the build machine.

Per sample every enabled transform fires independently with probability ``da_prob``; the output is defined in this order:

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
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

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
    """See the module docstring.  ``aug(x, t, out=None, records=None) -> (x_out, t_out)``."""

    def __init__(self, *, da_prob: float = 0.5, rot90: bool = False, zflip: bool = False, vflip: bool = False, hflip: bool = False,
                 brightness=None, contrast=None, gaussian_noise=None, cutout=None, seed: Optional[int] = None):
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

    def _cfg_struct(self) -> "L.AugCfg":
        c = self.config()
        return L.AugCfg(c["seed"], c["thr"], c["enable"], c["box"][0], c["box"][1], *c["contrast"], *c["brightness"], *c["noise"], *c["size"])

    @classmethod
    def from_cfg(cls, cfg, seed: Optional[int] = None) -> Optional["DeviceAugmenter"]:
        """The augmenter a reference configuration asks for, ``None`` when ``AUGMENTOR.ENABLE`` is false.

        Mapped ``AUGMENTOR`` keys: ``DA_PROB``; ``ROT90``, ``ZFLIP``, ``VFLIP``, ``HFLIP``; ``BRIGHTNESS`` + ``BRIGHTNESS_FACTOR``; ``CONTRAST`` +
        ``CONTRAST_FACTOR``; ``GAUSSIAN_NOISE`` + ``GAUSSIAN_NOISE_STD`` (a range; this package's own key) or the reference's scalar
        ``GAUSSIAN_NOISE_VAR`` (the fixed deviation ``sqrt(var)``); ``CUTOUT`` + ``COUT_NB_ITERATIONS``, ``COUT_SIZE``, ``COUT_CVAL``,
        ``COUT_APPLY_TO_MASK``.  Any OTHER switch of the node that is ``True`` (``RANDOM_ROT``, ``ELASTIC``, ``ZOOM``, ``SHEAR``, ``G_BLUR``,
        ``GAMMA_CONTRAST``, ...) raises ``NotImplementedError`` naming it: a run never silently trains with less augmentation than configured.

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
        for k in _UNSUPPORTED_SWITCHES:                                # also those a node that cannot be listed still answers for
            if k not in items and get(k, False) is True:
                items[k] = True
        for k in sorted(items):
            if items[k] is True and k not in _MAPPED_SWITCHES and k not in _NEUTRAL_SWITCHES:
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
    def last_records(self) -> Optional[torch.Tensor]:
        """The ``(B, 32)`` int32 device tensor of the last call's records (the augmenter's own buffer, overwritten by the next call)."""
        return self._records

    # ---- the call -------------------------------------------------------------------------------------------------------------
    def __call__(self, x: torch.Tensor, t: torch.Tensor, out=None, *, records: Optional[torch.Tensor] = None):
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

        self._ensure(x.device, B)
        s = L.stream_ptr()
        rec = self._records
        if records is None:
            import ctypes

            cfg = self._cfg_struct()
            L.check(lib.bpx_aug_draw(ctypes.addressof(cfg), B, Z, Y, X, self._state.data_ptr(), rec.data_ptr(), s))
        else:
            rec.copy_(records)
        if records is not None or self.contrast is not None:           # m is only ever used by the contrast step
            n = Z * Y * X * C
            need = B * int(lib.bpx_aug_mean_blocks(n))
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.float64, device=x.device)
            L.check(lib.bpx_aug_mean(xm.data_ptr(), B, n, self._ws.data_ptr(), rec.data_ptr(), s))
        cut = self.cutout or _CUTOUT_DEFAULTS
        L.check(lib.bpx_aug_apply(xm.data_ptr(), tm.data_ptr(), L.dt_of(t), B, Z, Y, X, C, Ct, rec.data_ptr(), self.seed, float(cut["cval"]),
                                  int(bool(cut["apply_to_mask"])), xo.data_ptr(), to.data_ptr(), s))
        return x_out, t_out


# AUGMENTOR switches from_cfg maps, switches that select no transform, and the transforms it refuses by name (from memory of the reference's tree)
_MAPPED_SWITCHES = {"ENABLE", "ROT90", "ZFLIP", "VFLIP", "HFLIP", "BRIGHTNESS", "CONTRAST", "GAUSSIAN_NOISE", "CUTOUT", "COUT_APPLY_TO_MASK"}
_NEUTRAL_SWITCHES = {"DRAW_GRID", "AUG_SAMPLES", "SHUFFLE_TRAIN_DATA_EACH_EPOCH", "SHUFFLE_VAL_DATA_EACH_EPOCH"}
_UNSUPPORTED_SWITCHES = ("RANDOM_ROT", "ELASTIC", "ZOOM", "SHEAR", "SHIFT", "AFFINE", "G_BLUR", "MEDIAN_BLUR", "MOTION_BLUR", "GAMMA_CONTRAST",
                         "BRIGHTNESS_EM", "CONTRAST_EM", "DROPOUT", "CUTBLUR", "CUTMIX", "CUTNOISE", "MISALIGNMENT", "MISSING_SECTIONS",
                         "GRAYSCALE", "CHANNEL_SHUFFLE", "GRIDMASK", "POISSON_NOISE", "SALT", "PEPPER", "SALT_AND_PEPPER")

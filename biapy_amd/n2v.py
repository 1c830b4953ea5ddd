"""Noise2Void on the device: the blind-spot manipulation of a training batch and the target its masked loss reads (``csrc/n2v.hip``,
``csrc/n2v_core.h``; the loss is ``biapy_amd.losses.N2VLoss``).

The reference manipulates the batch on the CPU inside its data generator; with ``DevicePatchSampler`` and ``DeviceAugmenter`` in front, a denoising
run would be the only one that still leaves the device every step.  The semantics below are the PRODUCT'S OWN - **parity-unpinned**: the
reference's sources are not on the build machine, its draws are random, and the rules here are stated exactly and checked bit for bit against a
host twin (``tests/n2v_ref.py``).

``masker(x, t=None, out=None) -> (x_masked, target)``

* ``x``: float32 ``(B,[Z,]Y,X,C)``-contiguous or the ``(B,C,[Z,]Y,X)`` permuted view of such memory (``augment._layout``'s rule), ``1 <= C <= 8``,
  ``B < 2^24``, fewer than 2^31 voxels per sample; 2-D data is ``Z = 1``.
* ``x_masked`` has ``x``'s shape and strides and equals ``x`` bit for bit everywhere except at the masked voxels.
* ``target`` is always a contiguous channel-first float32 ``(B, 2C, [Z,] Y, X)``: ``target[b, c]`` holds ``x``'s ORIGINAL value at the masked voxels
  of channel ``c`` and 0 elsewhere, ``target[b, C + c]`` is 1 there and 0 elsewhere - what ``N2VLoss`` reads without a copy.
* ``t`` is accepted and ignored: the call obeys the ``augment=`` protocol of ``train_one_epoch``, ``(batch, targets) -> (batch, targets)``.
* With ``augment=`` a ``DeviceAugmenter``, that augmenter runs first on ``x`` with a one-channel uint8 scratch target the masker owns.
* The masking reads the input and cannot run in place: ``out = (x_out, target_out)`` overlapping ``x`` (or each other) is refused.

The grid.  ``box = (sz, sy, sx)`` is an int or one per axis, each ``1 <= s <= 64``; an axis of extent 1 always gets ``s = 1``.  ``box=None`` derives
the isotropic ``s = max(1, floor((100 / perc_pix) ** (1 / d) + 0.5))`` over the ``d`` axes of extent above 1 (8 in 3-D and 22 in 2-D at the
default 0.198); ``perc_pix`` lies in ``(0, 100]``.  Boxes per axis ``n_a = ceil(dim_a / s_a)``, box index ``i = (iz n_y + iy) n_x + ix``, fewer than
2^31 boxes per sample.

The draw.  Every (sample ``b``, channel ``c``, box ``i``) draws on its own, a pure function of (seed, the masker's device counter value ``q``, ``b``,
``c``, ``i``); the counter advances by one per call.  Nothing is read back, so a call can be captured in a HIP graph and every replay draws anew.
Philox4x32-10, key ``(seed_lo ^ 0x4E32564D, seed_hi)``, counter words ``(i, (b << 4) | c | (stream << 28), q_lo, q_hi)``; ``mulhi(r, n) = (r * n) >> 32``.

* Stream 0, the position: ``p_a = i_a s_a + mulhi(r_a, s_a)`` for ``a = z, y, x`` from words 0, 1, 2.  If any ``p_a >= dim_a`` the box masks nothing
  (the ragged last boxes).
* Stream 1, the replacement: ``radius`` is an int or one per axis, ``0..15``, and 0 on an axis of extent 1; the window is
  ``[max(0, p_a - R_a), min(dim_a, p_a + R_a + 1))`` per axis, ``w_a`` its widths, ``n = w_z w_y w_x``, ``cen`` the raster index of ``p`` inside it.

Manipulators: ``"uniform_withCP"``: ``k = mulhi(r0, n)``; ``"uniform_withoutCP"``: ``k = mulhi(r0, n - 1)``, then ``k += (k >= cen)``, and a window of
one voxel masks nothing.  For both, the new value is ``x`` at the window's voxel of raster index ``k``, read from the INPUT: a masked neighbour is
never seen.  ``"identity"``: the value stays and the mask is set.  ``"normal_additive"``: ``x[p] + sigma * n``, one fp32 multiply and one add, ``n``
from Box-Muller on ``r0``, ``r1`` exactly as ``augment.hip``'s ``noise4`` forms its cosine element (``u1 = ((r0 >> 8) + 1) 2^-24``,
``u2 = (r1 >> 8) 2^-24``).  Every other name is refused by name: ``normal_withoutCP``, ``normal_fitted``, ``mean``, ``median`` and the structN2V mask.

Inspection hooks: ``last_coords`` / ``last_sources``, int32 ``(B, C, boxes)`` written by the kernel: the linear ``(z, y, x)`` index of the masked
voxel within the sample and of its source (the voxel itself for ``identity`` and ``normal_additive``), -1 and -1 where a box masks nothing;
``counter`` (the value the NEXT call draws with) and ``config()`` as the augmenter's.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch
import torch.distributed as dist

from . import _lib as L
from .augment import DeviceAugmenter, _layout, _span

lib = L.lib

MANIPULATORS = {"uniform_withCP": 0, "uniform_withoutCP": 1, "identity": 2, "normal_additive": 3}      # BPX_N2V_*
UNSUPPORTED_MANIPULATORS = ("normal_withoutCP", "normal_fitted", "mean", "median")
KEY_XOR = 0x4E32564D
MAX_BOX, MAX_RADIUS, MAX_CHANNELS = 64, 15, 8


def _per_axis(name: str, v, lo: int, hi: int):
    try:
        vals = (int(v),) * 3 if not hasattr(v, "__len__") else tuple(int(a) for a in v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be an integer or one per axis (z, y, x), got {v!r}") from None
    if len(vals) == 2:
        vals = (1 if name == "box" else 0,) + vals                 # 2-D spelling: (y, x)
    if len(vals) != 3:
        raise ValueError(f"{name} must be an integer or one per axis (z, y, x), got {v!r}")
    if not all(lo <= a <= hi for a in vals):
        raise ValueError(f"{name} entries must lie in {lo}..{hi}, got {v!r}")
    return vals


def derived_box(perc_pix: float, dims) -> int:
    """The isotropic box edge of ``box=None``: ``max(1, floor((100 / perc_pix) ** (1 / d) + 0.5))`` over the ``d`` axes of extent above 1."""
    d = max(1, sum(1 for n in dims if n > 1))
    return max(1, int(math.floor((100.0 / perc_pix) ** (1.0 / d) + 0.5)))


class N2VMasker:
    """See the module docstring.  ``masker(x, t=None, out=None) -> (x_masked, target)``."""

    def __init__(self, *, box=None, perc_pix: float = 0.198, radius=5, manipulator: str = "uniform_withCP", sigma: float = 1.0,
                 augment: Optional[DeviceAugmenter] = None, seed: Optional[int] = None):
        if manipulator not in MANIPULATORS:
            if manipulator in UNSUPPORTED_MANIPULATORS or "struct" in str(manipulator).lower():
                raise NotImplementedError(f"manipulator {manipulator!r} is not implemented by biapy_amd.n2v.N2VMasker (supported: "
                                          f"{', '.join(MANIPULATORS)}); the neighbourhood-statistics manipulators and the structN2V mask are out of scope")
            raise ValueError(f"manipulator must be one of {', '.join(MANIPULATORS)}, got {manipulator!r}")
        self.manipulator = manipulator
        try:
            perc_pix = float(perc_pix)
        except (TypeError, ValueError):
            raise ValueError(f"perc_pix must be a number, got {perc_pix!r}") from None
        if not (0.0 < perc_pix <= 100.0):
            raise ValueError(f"perc_pix must lie in (0, 100], got {perc_pix!r}")
        self.perc_pix = perc_pix
        self.box = None if box is None else _per_axis("box", box, 1, MAX_BOX)
        self.radius = _per_axis("radius", radius, 0, MAX_RADIUS)
        try:
            self.sigma = float(sigma)
        except (TypeError, ValueError):
            raise ValueError(f"sigma must be a number, got {sigma!r}") from None
        if not math.isfinite(self.sigma):
            raise ValueError(f"sigma must be finite, got {sigma!r}")
        if augment is not None and not isinstance(augment, DeviceAugmenter):
            raise ValueError(f"augment must be a biapy_amd.augment.DeviceAugmenter or None, got {type(augment).__name__}")
        self.augment = augment
        if seed is None:
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
            seed = torch.initial_seed() + rank                        # ranks draw differently
        try:
            self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        except (TypeError, ValueError):
            raise ValueError(f"seed must be an integer, got {seed!r}") from None
        self._state = None            # int64[2] on the device: [counter, the value the last call drew with]
        self._coords = self._sources = None
        self._dummy = self._ax = None  # the inner augmenter's scratch target and output

    # ---- configuration --------------------------------------------------------------------------------------------------------
    def grid(self, Z: int, Y: int, X: int):
        """``(box, radius)`` per axis as they apply to a ``(Z, Y, X)`` sample: 1 and 0 on an axis of extent 1, the derived edge with ``box=None``."""
        dims = (Z, Y, X)
        if self.box is None:
            s = derived_box(self.perc_pix, dims)
            if s > MAX_BOX:
                raise ValueError(f"perc_pix = {self.perc_pix!r} derives a box edge of {s} on a sample of shape {dims}; at most {MAX_BOX}")
            box = (s, s, s)
        else:
            box = self.box
        return (tuple(1 if n == 1 else b for n, b in zip(dims, box)), tuple(0 if n == 1 else r for n, r in zip(dims, self.radius)))

    def config(self, shape=None) -> dict:
        """The draw parameters as plain numbers (``tests/n2v_ref.mask`` takes the same dict); with ``shape = (Z, Y, X)`` box and radius as they
        apply to such a sample."""
        box, radius = (self.box, self.radius) if shape is None else self.grid(*shape)
        return dict(seed=self.seed, box=box, radius=radius, manipulator=self.manipulator, sigma=self.sigma, perc_pix=self.perc_pix)

    def _cfg_struct(self, Z, Y, X) -> "L.N2VCfg":
        box, radius = self.grid(Z, Y, X)
        return L.N2VCfg(self.seed, (ctypes.c_int32 * 3)(*box), (ctypes.c_int32 * 3)(*radius), MANIPULATORS[self.manipulator], self.sigma)

    @classmethod
    def from_cfg(cls, cfg, seed: Optional[int] = None, augment: Optional[DeviceAugmenter] = None) -> Optional["N2VMasker"]:
        """The masker a reference configuration asks for, ``None`` when ``PROBLEM.TYPE`` is not ``DENOISING``.

        Mapped ``PROBLEM.DENOISING`` keys: ``N2V_PERC_PIX`` (0.198), ``N2V_MANIPULATOR`` (``uniform_withCP``), ``N2V_NEIGHBORHOOD_RADIUS`` (5) and
        ``N2V_STRUCTMASK`` (refused when true).  An unsupported manipulator is refused by name.  The key names and defaults are written from
        memory of the reference's configuration tree and could not be verified against it on the build machine; the semantics are this package's
        own (parity-unpinned, see the module docstring)."""
        from .train_engine import _cfg_get

        if str(_cfg_get(cfg, "PROBLEM.TYPE", "")).upper() != "DENOISING":
            return None
        if _cfg_get(cfg, "PROBLEM.DENOISING.N2V_STRUCTMASK", False):
            raise NotImplementedError("PROBLEM.DENOISING.N2V_STRUCTMASK is enabled but biapy_amd.n2v.N2VMasker does not implement the structN2V mask")
        manip = str(_cfg_get(cfg, "PROBLEM.DENOISING.N2V_MANIPULATOR", "uniform_withCP"))
        if manip not in MANIPULATORS:
            raise NotImplementedError(f"PROBLEM.DENOISING.N2V_MANIPULATOR = {manip!r} is not implemented by biapy_amd.n2v.N2VMasker (supported: "
                                      f"{', '.join(MANIPULATORS)})")
        return cls(perc_pix=_cfg_get(cfg, "PROBLEM.DENOISING.N2V_PERC_PIX", 0.198), manipulator=manip,
                   radius=_cfg_get(cfg, "PROBLEM.DENOISING.N2V_NEIGHBORHOOD_RADIUS", 5), seed=seed, augment=augment)

    # ---- state ----------------------------------------------------------------------------------------------------------------
    @property
    def counter(self) -> torch.Tensor:
        """The device counter (int64 scalar view): the value the NEXT call draws with."""
        if self._state is None:
            self._state = torch.zeros(2, dtype=torch.int64, device=torch.device("cuda", torch.cuda.current_device()))
        return self._state[0]

    @property
    def last_coords(self) -> Optional[torch.Tensor]:
        """int32 ``(B, C, boxes)``: the masked voxel of every box of the last call, -1 where it masks nothing (the masker's own buffer)."""
        return self._coords

    @property
    def last_sources(self) -> Optional[torch.Tensor]:
        """int32 ``(B, C, boxes)``: the source voxel of every box of the last call, -1 where it masks nothing (the masker's own buffer)."""
        return self._sources

    # ---- the call -------------------------------------------------------------------------------------------------------------
    def __call__(self, x: torch.Tensor, t=None, out=None):
        if not torch.is_tensor(x) or not x.is_cuda:
            raise ValueError("x must be a CUDA/HIP tensor: biapy_amd.n2v runs on the device only, there is no CPU path")
        if x.dtype != torch.float32:
            raise ValueError(f"x must be float32, got {x.dtype}")
        xm, x_first = _layout(x, "x")
        nd = xm.dim()
        B, C = xm.shape[0], xm.shape[-1]
        Z, Y, X = (1, *xm.shape[1:-1]) if nd == 4 else tuple(xm.shape[1:-1])
        if not 1 <= C <= MAX_CHANNELS:
            raise ValueError(f"x must have 1 to {MAX_CHANNELS} channels, got {C}")
        if min(B, Z, Y, X) < 1:
            raise ValueError(f"empty batch: x has shape {tuple(x.shape)}")
        if B >= 2 ** 24:
            raise ValueError(f"a batch of {B} samples; 2^24 or more are not supported")
        if Z * Y * X >= 2 ** 31:
            raise ValueError(f"a sample of {Z * Y * X} voxels; 2^31 or more are not supported")
        cfg = self._cfg_struct(Z, Y, X)
        boxes = int(lib.bpx_n2v_boxes(ctypes.addressof(cfg), Z, Y, X))
        if boxes < 0:
            raise ValueError(lib.bpx_last_error().decode())
        t_shape = (B, 2 * C) + tuple(xm.shape[1:-1])
        if out is None:
            xo = torch.empty_like(xm, memory_format=torch.contiguous_format)
            x_out = xo.permute(0, nd - 1, *range(1, nd - 1)) if x_first else xo
            target = torch.empty(t_shape, dtype=torch.float32, device=x.device)
        else:
            try:
                x_out, target = out
            except (TypeError, ValueError):
                raise ValueError("out must be a pair (x_out, target_out)") from None
            if (not torch.is_tensor(x_out) or x_out.device != x.device or x_out.dtype != x.dtype or tuple(x_out.shape) != tuple(x.shape)
                    or any(a != b for n, a, b in zip(x.shape, x_out.stride(), x.stride()) if n > 1)):
                raise ValueError("out[0] must have the shape, dtype, strides and device of x")
            if (not torch.is_tensor(target) or target.device != x.device or target.dtype != torch.float32 or tuple(target.shape) != t_shape
                    or not target.is_contiguous()):
                raise ValueError(f"out[1] must be a contiguous float32 tensor of shape {t_shape} on the device of x")
            xo = _layout(x_out, "out[0]")[0]
            (a0, a1), (b0, b1), (c0, c1) = _span(x), _span(x_out), _span(target)
            if (b0 < a1 and a0 < b1) or (c0 < a1 and a0 < c1):
                raise ValueError("out overlaps the input: the masking reads the input and cannot run in place")
            if b0 < c1 and c0 < b1:
                raise ValueError("out[0] and out[1] overlap")
        if self._state is None or self._state.device != x.device:
            self._state = torch.zeros(2, dtype=torch.int64, device=x.device)
        if self._coords is None or tuple(self._coords.shape) != (B, C, boxes) or self._coords.device != x.device:
            self._coords = torch.empty((B, C, boxes), dtype=torch.int32, device=x.device)
            self._sources = torch.empty((B, C, boxes), dtype=torch.int32, device=x.device)
        src = xm
        if self.augment is not None:
            d_shape = tuple(xm.shape[:-1]) + (1,)
            if self._dummy is None or tuple(self._dummy.shape) != d_shape or self._dummy.device != x.device:
                self._dummy = torch.zeros(d_shape, dtype=torch.uint8, device=x.device)
                self._ax = (torch.empty_like(xm, memory_format=torch.contiguous_format), torch.empty_like(self._dummy))
            src = self.augment(xm, self._dummy, out=self._ax)[0]
        L.check(lib.bpx_n2v_mask(src.data_ptr(), B, Z, Y, X, C, ctypes.addressof(cfg), self._state.data_ptr(), xo.data_ptr(), target.data_ptr(),
                                 self._coords.data_ptr(), self._sources.data_ptr(), L.stream_ptr()))
        return x_out, target

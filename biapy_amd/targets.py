"""Instance-segmentation training targets on the device: from a batch of instance-id patches the channel targets the heads are trained on
(``csrc/itarget.hip``, ``csrc/itarget_core.h``; the loss is ``biapy_amd.losses.InstanceChannelsLoss``).

The reference builds these channels on the host with SciPy before training.  Here the ids go through sampling and augmentation exactly (a
``float32`` id is exact to 2^24 and the target path of ``DeviceAugmenter`` interpolates to the nearest voxel), and the channels are computed from
the AUGMENTED ids, once per step, on the device.  The semantics below are the PRODUCT'S OWN - **parity-unpinned**: the reference's sources are not
on the build machine, the mapping to its channel letters is written from memory and unverified, and every rule here is stated exactly and checked
bit for bit against a host twin (``tests/itarget_ref.py``).

``it(x, t, out=None) -> (x, target)``

* ``t``, the ids: one sample is ``([Z,] Y, X)`` with fewer than 2^31 voxels, 2-D is ``Z = 1``.  ``float32`` or ``uint8`` ``(B,[Z,]Y,X,1)``-contiguous
  or the ``(B,1,[Z,]Y,X)`` permuted view of such memory (``augment._layout``'s rule), or ``int32`` ``(B,[Z,]Y,X)``.
* Id sanitising: a value that is not an integer, is negative, is above ``n_max``, or is NaN or infinite counts as background, and is counted in
  the device counter ``last_faults`` (int32, the count of the last call; nothing is read back by the call).  ``0 <= n_max < 2^24``.
* ``x`` is returned as it came.  With ``augment=`` a ``DeviceAugmenter``, that runs first on ``(x, t)`` and its outputs are what is returned and
  what the channels are computed from.
* ``target`` is contiguous channel-first ``float32`` ``(B, Ct, [Z,] Y, X)``, ``Ct = len(channels) <= 8`` - what ``InstanceChannelsLoss`` reads
  without a copy.  ``out=`` is accepted; an ``out`` that overlaps ``t`` or ``x`` is refused.
* Everything is PER SAMPLE: the same id in two samples is two instances.  The same id in two disconnected pieces of one sample is ONE instance
  (one centroid, one box, one ``dmax``) - ids are taken as given, nothing is relabelled.
* Nothing is read back and every launch is fixed by the shapes and the options: the call can be captured in a graph.

Channels; ``l`` is the voxel's sanitised id, and every channel is 0 on the background unless stated otherwise.

* ``"F"``: 1 where ``l > 0``; with ``f_excludes_contour`` 0 also where ``C`` is 1.
* ``"C"``: 1 where ``prepost.find_boundaries(ids, contour_connectivity, contour_mode)`` is 1, bit for bit.  ``"thick"``: some in-volume neighbour
  within ``generate_binary_structure(ndim, connectivity)`` carries another id - background voxels next to an instance included; ``"inner"``: that
  and ``l > 0``.  ``"outer"`` and ``"subpixel"`` are refused by name.
* ``"D"``: ``d`` is the ``float32`` distance of ``prepost.label_distance(ids, sampling)`` with the same bits.  ``d_norm="instance"``: ``d / dmax[l]``,
  one fp32 division, ``dmax[l]`` the largest ``d`` over the instance; 1.0 where ``d`` is the ``+inf`` sentinel (an instance that fills its sample).
  ``d_norm="none"``: ``d``, or ``min(d, d_clip)`` with ``d_clip``; WITHOUT A CLIP THE SENTINEL STAYS ``+inf``.
* ``"Dc"``: the centroid is ``c_a = double(S_a) / double(A)`` (coordinate sums over area); ``r = sqrt(((dz sz)^2 + (dy sy)^2) + (dx sx)^2)`` in fp64,
  in that order, without FMA; ``rc = float32(r)``, ``rcmax[l]`` its maximum over the instance; the value is ``1.0f - rc / rcmax[l]`` in two fp32
  operations, 1.0 when ``rcmax == 0``.
* ``"H"``, ``"V"``, ``"Z"``: the offsets from the centroid along x, y and z.  ``o = double(p_a) - c_a``; ``e = double(hi_a) - c_a`` when ``o >= 0`` else
  ``c_a - double(lo_a)``, ``lo`` / ``hi`` the instance's inclusive box; the value is ``float32(o / e)``, 0 when ``e == 0``; the range is [-1, 1].
  ``"Z"`` on 2-D input is refused.
* Refused by name with ``NotImplementedError``: ``B``, ``P``, ``T``, ``Db``, ``Dn``, ``R``, ``A``, ``E_*``, ``We``, ``M`` - rays, affinities, embeddings,
  weight maps and skeleton-based centres are follow-ups.

``sampling`` is the voxel size per axis (``(sz, sy, sx)``, ``(sy, sx)`` in 2-D) for ``D`` and ``Dc``; ``None`` is the unit grid, where ``D`` takes
the exact integer path of the distance transform.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from . import _lib as L
from .augment import DeviceAugmenter, _layout, _span

lib = L.lib

CHANNELS = {"F": 1, "C": 2, "D": 3, "Dc": 4, "H": 5, "V": 6, "Z": 7}                     # BPX_ITARGET_*
UNSUPPORTED_CHANNELS = ("B", "P", "T", "Db", "Dn", "R", "A", "We", "M")                  # and every E_*
CONTOUR_MODES = {"thick": 0, "inner": 1}
FLAG_F_EXCLUDES_C, FLAG_D_RAW, FLAG_D_CLIP = 1, 2, 4
MAX_CHANNELS, ID_LIMIT = 8, 1 << 24


def _check_channels(channels, where: str = "channels"):
    if isinstance(channels, str) or not hasattr(channels, "__iter__"):
        raise ValueError(f"{where} must be a sequence of channel letters, got {channels!r}")
    chans = tuple(channels)
    for c in chans:
        if c in CHANNELS:
            continue
        if c in UNSUPPORTED_CHANNELS or str(c).startswith("E_"):
            raise NotImplementedError(f"channel {c!r} is not implemented by biapy_amd.targets.InstanceTargets (supported: {', '.join(CHANNELS)}); rays, "
                                      "affinities, embeddings, weight maps and skeleton-based centres are follow-ups")
        raise ValueError(f"unknown channel {c!r} in {where} (supported: {', '.join(CHANNELS)})")
    if not 1 <= len(chans) <= MAX_CHANNELS:
        raise ValueError(f"{where} must name 1 to {MAX_CHANNELS} channels, got {len(chans)}")
    return chans


class InstanceTargets:
    """See the module docstring.  ``it(x, t, out=None) -> (x, target)``."""

    def __init__(self, channels=("F", "C", "D"), *, n_max: int, contour_mode: str = "thick", contour_connectivity: int = 1,
                 f_excludes_contour: bool = False, d_norm: str = "instance", d_clip: Optional[float] = None, sampling=None,
                 augment: Optional[DeviceAugmenter] = None):
        self.channels = _check_channels(channels)
        try:
            self.n_max = int(n_max)
        except (TypeError, ValueError):
            raise ValueError(f"n_max must be an integer, got {n_max!r}") from None
        if not 0 <= self.n_max < ID_LIMIT:
            raise ValueError(f"n_max must lie in [0, 2^24) - a float32 holds every such id exactly - got {n_max!r}")
        if contour_mode not in CONTOUR_MODES:
            if contour_mode in ("outer", "subpixel"):
                raise NotImplementedError(f"contour_mode {contour_mode!r} is not implemented (supported: {', '.join(CONTOUR_MODES)})")
            raise ValueError(f"contour_mode must be one of {', '.join(CONTOUR_MODES)}, got {contour_mode!r}")
        self.contour_mode = contour_mode
        try:
            self.contour_connectivity = int(contour_connectivity)
        except (TypeError, ValueError):
            raise ValueError(f"contour_connectivity must be an integer, got {contour_connectivity!r}") from None
        if not 1 <= self.contour_connectivity <= 3:
            raise ValueError(f"contour_connectivity must lie in 1..3 (1..2 for 2-D samples), got {contour_connectivity!r}")
        self.f_excludes_contour = bool(f_excludes_contour)
        if d_norm not in ("instance", "none"):
            raise ValueError(f"d_norm must be 'instance' or 'none', got {d_norm!r}")
        self.d_norm = d_norm
        if d_clip is not None:
            if d_norm != "none":
                raise ValueError("d_clip applies to d_norm='none' only")
            try:
                d_clip = float(d_clip)
            except (TypeError, ValueError):
                raise ValueError(f"d_clip must be a number, got {d_clip!r}") from None
            if not d_clip >= 0.0:
                raise ValueError(f"d_clip must be a number >= 0, got {d_clip!r}")
        self.d_clip = d_clip
        if sampling is not None:
            try:
                sampling = tuple(float(v) for v in sampling)
            except (TypeError, ValueError):
                sampling = ()
            if len(sampling) not in (2, 3) or not all(math.isfinite(v) and v > 0.0 for v in sampling):
                raise ValueError("sampling must be 2 or 3 positive finite numbers, one per axis")
        self.sampling = sampling
        if augment is not None and not isinstance(augment, DeviceAugmenter):
            raise ValueError(f"augment must be a biapy_amd.augment.DeviceAugmenter or None, got {type(augment).__name__}")
        self.augment = augment
        self.codes = 0
        for i, c in enumerate(self.channels):
            self.codes |= CHANNELS[c] << (4 * i)
        self.flags = ((FLAG_F_EXCLUDES_C if self.f_excludes_contour else 0) | (FLAG_D_RAW if d_norm == "none" else 0)
                      | (FLAG_D_CLIP if d_clip is not None else 0))
        self._faults = None
        self._key = None               # what the scratch below was sized for
        self._ids = self._dist = self._rec = self._ws = None

    @classmethod
    def from_cfg(cls, cfg, n_max: int, augment: Optional[DeviceAugmenter] = None) -> Optional["InstanceTargets"]:
        """The target generator a reference configuration asks for, ``None`` when ``PROBLEM.TYPE`` is not ``INSTANCE_SEG``.

        Mapped: ``PROBLEM.INSTANCE_SEG.DATA_CHANNELS`` (a list of letters, or one string such as ``"FCD"`` cut into the known letters), default
        ``("F", "C", "D")``.  An unsupported or unknown letter is refused by name.  The key names are written from memory of the reference's
        configuration tree and could not be verified against it on the build machine; the semantics are this package's own (parity-unpinned,
        see the module docstring)."""
        from .train_engine import _cfg_get

        if str(_cfg_get(cfg, "PROBLEM.TYPE", "")).upper() != "INSTANCE_SEG":
            return None
        chans = _cfg_get(cfg, "PROBLEM.INSTANCE_SEG.DATA_CHANNELS", ("F", "C", "D"))
        if isinstance(chans, str):
            chans = _split_letters(chans)
        return cls(_check_channels(chans, "PROBLEM.INSTANCE_SEG.DATA_CHANNELS"), n_max=n_max, augment=augment)

    @property
    def last_faults(self) -> Optional[torch.Tensor]:
        """int32 scalar on the device: how many values of the last call's ``t`` were no id (and counted as background); ``None`` before a call."""
        return self._faults

    @property
    def last_ids(self) -> Optional[torch.Tensor]:
        """int32 ``(B, Z, Y, X)``: the sanitised ids the last call's channels were computed from - with ``augment=`` the augmented ones (the
        generator's own buffer, overwritten by the next call); ``None`` before a call."""
        return self._ids

    # ---- the call ---------------------------------------------------------------------------------------------------------------------------
    def _ids_view(self, t: torch.Tensor):
        """``(flat memory of the ids, sample shape)`` of an accepted ``t``."""
        if t.dtype == torch.int32:
            if t.dim() not in (3, 4):
                raise ValueError(f"int32 ids must be (B,[Z,]Y,X), got shape {tuple(t.shape)}")
            if not t.is_contiguous():
                raise ValueError("int32 ids must be contiguous")
            return t, tuple(t.shape[1:])
        if t.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"t must be float32, uint8 or int32, got {t.dtype}")
        tm, _ = _layout(t, "t")
        if tm.shape[-1] != 1:
            raise ValueError(f"t must have one id channel, got {tm.shape[-1]}")
        return tm, tuple(tm.shape[1:-1])

    def __call__(self, x, t, out=None):
        # dtype, rank and the options against the sample's rank first, the device last: every refusal names the first thing that is wrong
        if not torch.is_tensor(t):
            raise ValueError(f"t must be a tensor, got {type(t).__name__}")
        tm, sample = self._ids_view(t)
        ndim = len(sample)
        B = tm.shape[0]
        Z, Y, X = (1, *sample) if ndim == 2 else sample
        if min(B, Z, Y, X) < 1:
            raise ValueError(f"empty batch: t has shape {tuple(t.shape)}")
        if Z * Y * X >= 2 ** 31:
            raise ValueError(f"a sample of {Z * Y * X} voxels; 2^31 or more are not supported")
        if ndim == 2 and "Z" in self.channels:
            raise ValueError("channel 'Z' needs 3-D samples")
        if self.contour_connectivity > ndim:
            raise ValueError(f"contour_connectivity must lie in 1..{ndim} for {ndim}-D samples, got {self.contour_connectivity}")
        samp = None
        if self.sampling is not None:
            if len(self.sampling) != ndim:
                raise ValueError(f"sampling has {len(self.sampling)} entries for {ndim}-D samples")
            samp = (ctypes.c_double * 3)(*([1.0] * (3 - ndim) + list(self.sampling)))
        if not t.is_cuda:
            raise ValueError("t must be a CUDA/HIP tensor: biapy_amd.targets runs on the device only, there is no CPU path")
        if x is not None and (not torch.is_tensor(x) or x.device != t.device):
            raise ValueError("x must be a tensor on the device of t (or None)")
        if self.augment is not None:
            if x is None:
                raise ValueError("augment= needs the batch x beside the ids")
            if t.dtype == torch.int32:
                raise ValueError("augment= takes float32 or uint8 ids (B,[Z,]Y,X,1): the augmenter has no int32 target path")
        Ct, V = len(self.channels), Z * Y * X
        t_shape = (B, Ct) + sample
        if out is None:
            target = torch.empty(t_shape, dtype=torch.float32, device=t.device)
        else:
            target = out
            if (not torch.is_tensor(target) or target.device != t.device or target.dtype != torch.float32 or tuple(target.shape) != t_shape
                    or not target.is_contiguous()):
                raise ValueError(f"out must be a contiguous float32 tensor of shape {t_shape} on the device of t")
            c0, c1 = _span(target)                                  # against the caller's tensors: the augmenter's outputs are its own, fresh ones
            for name, other in (("t", t), ("x", x)):
                if other is not None:
                    a0, a1 = _span(other)
                    if c0 < a1 and a0 < c1:
                        raise ValueError(f"out overlaps {name}")
        need_rec = int(lib.bpx_itarget_records_bytes(B, self.n_max))
        need_ws = int(lib.bpx_edt_workspace(Z, Y, X, 0 if samp is None else 1))
        if need_rec < 0:
            raise ValueError(lib.bpx_last_error().decode())
        if need_ws < 0:
            raise NotImplementedError(f"a {sample} sample is refused by the exact integer path of the distance transform: Z^2 + Y^2 + X^2 must stay "
                                      "below 2^31 - 1")
        if self.augment is not None:                                   # every refusal of this call is behind: the augmenter draws and advances its counter now
            x, t = self.augment(x, t)                                  # same shape, dtype and layout
            tm = self._ids_view(t)[0]
        key = (B, Z, Y, X, samp is None, t.device)
        if self._key != key:
            self._ids = torch.empty((B, Z, Y, X), dtype=torch.int32, device=t.device)
            self._dist = torch.empty((B, Z, Y, X), dtype=torch.float32, device=t.device)
            self._rec = torch.empty((need_rec + 7) // 8, dtype=torch.int64, device=t.device)
            self._ws = torch.empty(max(need_ws, 8), dtype=torch.uint8, device=t.device)       # shared by the samples: they run one after the other
            self._key = key
        if self._faults is None or self._faults.device != t.device:
            self._faults = torch.zeros((), dtype=torch.int32, device=t.device)
        s = L.stream_ptr()
        self._faults.zero_()
        dt = {torch.float32: L.F32, torch.uint8: L.U8, torch.int32: L.I32}[tm.dtype]
        L.check(lib.bpx_itarget_ids(tm.data_ptr(), dt, B * V, self.n_max, self._ids.data_ptr(), self._faults.data_ptr(), s))
        for b in range(B):           # 3 launches per sample
            L.check(lib.bpx_edt(self._ids.data_ptr() + 4 * b * V, L.I32, 1, Z, Y, X, samp, 0, self._dist.data_ptr() + 4 * b * V, self._ws.data_ptr(),
                                need_ws, s))
        L.check(lib.bpx_itarget_stats(self._ids.data_ptr(), self._dist.data_ptr(), B, Z, Y, X, self.n_max, samp, 1 if "Dc" in self.channels else 0,
                                      self._rec.data_ptr(), s))
        L.check(lib.bpx_itarget_pack(self._ids.data_ptr(), self._dist.data_ptr(), self._rec.data_ptr(), B, Z, Y, X, self.n_max, self.codes, Ct, ndim,
                                     self.contour_connectivity, CONTOUR_MODES[self.contour_mode], self.flags,
                                     0.0 if self.d_clip is None else self.d_clip, samp, target.data_ptr(), s))
        return x, target


def _split_letters(s: str):
    """``"FCDc"`` -> ``["F", "C", "Dc"]``: the longest known or refused letter first; what is neither is handed on for the refusal by name."""
    names = sorted(list(CHANNELS) + list(UNSUPPORTED_CHANNELS), key=len, reverse=True)
    out, i = [], 0
    while i < len(s):
        for n in names:
            if s.startswith(n, i):
                out.append(n)
                i += len(n)
                break
        else:
            out.append(s[i:])
            break
    return out

"""Random training patches drawn on the device from device-resident volumes (``csrc/sampler.hip``).

The reference's common 3-D setting is a few large volumes and a random crop per sample and step (``DATA.EXTRACT_RANDOM_PATCH``, optionally with a
foreground-weighted probability map).  A host loader that crops, collates and copies 33 MB every 8 ms is pure overhead when the volumes fit the
device's memory many times over: ``DevicePatchSampler`` keeps them there and a call is two launches - draw the origins, copy the windows.
``DevicePatchLoader`` makes it a ``data_loader`` of ``train_engine.train_one_epoch``: sampler -> ``DeviceAugmenter`` -> replayed step, with nothing
crossing the host per step.  The semantics below are the PRODUCT'S OWN - **parity-unpinned**: the reference's draws are random, and its exact
probability-map rule could not be compared on the build machine.

A call draws, per sample ``b``, the record ``(v, z0, y0, x0)`` and returns

    ``x[b] = float32(images[v][z0:z0+Pz, y0:y0+Py, x0:x0+Px, :])`` (times ``scale`` when given: one fp32 multiply), ``t[b]`` = the same window
    of ``targets[v]``, bit for bit.

uint8 / uint16 images convert exactly; a float32 image without ``scale`` moves bit for bit.  Two draw modes (``include/biapy_amd.h`` has the
arithmetic, every step of it in integers but one fp32 compare, so ``tests/sampler_ref.py`` reproduces every origin):

* uniform (no ``class_maps``): every valid origin of every volume is equally likely - a volume is drawn in proportion to its number of origins;
* class (``class_maps`` + ``class_probs``): class ``c`` is drawn with probability ``class_probs[c] / sum``, then one voxel uniformly among ALL voxels
  of that class in all volumes; the patch is centred on it (``origin = centre - P // 2``) and moved inside the volume where it sticks out.

The draws come from Philox4x32-10 keyed by ``seed`` with the sampler's own device counter, which advances by one per call.  Nothing is read back,
so a call can be captured in a HIP graph and every replay draws anew.  ``last_origins`` / ``origins=`` / ``counter`` are the inspection hooks.

Not offered: crops that reach outside a volume and are padded, validation crops, host-resident or Zarr volumes, float
probability maps.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import _lib as L

lib = L.lib

MAX_CLASSES = 8
_IMG_DTYPES = {torch.float32: L.F32, torch.uint8: L.U8}
if hasattr(torch, "uint16"):
    _IMG_DTYPES[torch.uint16] = L.U16
_TGT_DTYPES = {torch.float32: L.F32, torch.uint8: L.U8}


def _as_list(v, name: str) -> List[torch.Tensor]:
    vs = [v] if torch.is_tensor(v) else list(v) if isinstance(v, (list, tuple)) else None
    if not vs or not all(torch.is_tensor(a) for a in vs):
        raise ValueError(f"{name} must be a tensor or a non-empty list of tensors")
    return vs


def _span(t: torch.Tensor) -> Tuple[int, int]:
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


def class_cum(class_probs: Sequence[float]) -> List[float]:
    """The running fp32 sum the draw compares ``u`` with: ``class_probs`` (already normalised) added in index order in float32; the entries from
    the last class of positive probability on are 1.0, so a class without probability is never drawn."""
    acc, out = np.float32(0.0), []
    for p in class_probs:
        acc = np.float32(acc + np.float32(p))
        out.append(float(min(acc, np.float32(1.0))))
    last = max(i for i, p in enumerate(class_probs) if p > 0)
    return [1.0 if i >= last else c for i, c in enumerate(out)]


class DevicePatchSampler:
    """See the module docstring.  ``sampler(out=None, *, origins=None) -> (x, t)``.

    ``images`` / ``targets``: a device tensor or a list of them, ``(Z,Y,X,C)`` or ``(Y,X,C)`` each, contiguous; volumes may differ in extents, not in
    channel counts or dtypes (image float32 / uint8 / uint16 with 1 to 16 channels, target uint8 / float32 with 1 to 8).  ``patch_size``: ``(Pz,Py,Px)``,
    ``(Py,Px)`` for 2-D data; a trailing channel entry as in ``DATA.PATCH_SIZE`` is accepted when it equals ``C``.  ``class_maps``: one uint8
    ``(Z,Y,X)`` / ``(Y,X)`` device tensor per volume with values below ``len(class_probs)`` (at most 8 classes)."""

    def __init__(self, images, targets, patch_size, *, batch_size: int, class_maps=None, class_probs=None, scale: Optional[float] = None,
                 seed: Optional[int] = None):
        imgs, tgts = _as_list(images, "images"), _as_list(targets, "targets")
        if len(imgs) != len(tgts):
            raise ValueError(f"images and targets must pair up: {len(imgs)} images, {len(tgts)} targets")
        try:
            self.batch_size = int(batch_size)
        except (TypeError, ValueError):
            raise ValueError(f"batch_size must be an integer, got {batch_size!r}") from None
        if self.batch_size < 1:
            raise ValueError(f"batch_size must be at least 1, got {batch_size!r}")
        # ---- class probabilities: plain numbers, checked before any tensor ----
        if (class_maps is None) != (class_probs is None):
            raise ValueError("class_maps and class_probs go together: give both (class mode) or neither (uniform mode)")
        self.class_probs = None
        if class_probs is not None:
            try:
                probs = [float(p) for p in class_probs]
            except (TypeError, ValueError):
                raise ValueError(f"class_probs must be a sequence of numbers, got {class_probs!r}") from None
            if not 1 <= len(probs) <= MAX_CLASSES:
                raise ValueError(f"class_probs must name 1 to {MAX_CLASSES} classes, got {len(probs)}")
            if any(not np.isfinite(p) or p < 0 for p in probs):
                raise ValueError(f"class_probs must be finite and not negative, got {class_probs!r}")
            if sum(probs) <= 0:
                raise ValueError(f"class_probs sum to 0: no class can be drawn, got {class_probs!r}")
            self.class_probs = [p / sum(probs) for p in probs]
        # ---- the volumes: structure first, the device last ----
        self.ndim = imgs[0].dim() - 1
        if self.ndim not in (2, 3):
            raise ValueError(f"a volume is (Z,Y,X,C) or (Y,X,C), got shape {tuple(imgs[0].shape)}")
        self.C, self.Ct = int(imgs[0].shape[-1]), int(tgts[0].shape[-1]) if tgts[0].dim() else 0
        self.img_dtype, self.tgt_dtype = imgs[0].dtype, tgts[0].dtype
        if self.img_dtype not in _IMG_DTYPES:
            raise ValueError(f"images must be float32, uint8 or uint16, got {self.img_dtype}")
        if self.tgt_dtype not in _TGT_DTYPES:
            raise ValueError(f"targets must be uint8 or float32, got {self.tgt_dtype}")
        if not 1 <= self.C <= 16:
            raise ValueError(f"images must have 1 to 16 channels, got {self.C}")
        if not 1 <= self.Ct <= 8:
            raise ValueError(f"targets must have 1 to 8 channels, got {self.Ct}")
        try:
            patch = tuple(int(p) for p in patch_size)
        except (TypeError, ValueError):
            raise ValueError(f"patch_size must be a sequence of integers, got {patch_size!r}") from None
        if len(patch) == self.ndim + 1:
            if patch[-1] != self.C:
                raise ValueError(f"patch_size {patch} ends with {patch[-1]} channels, the images have {self.C}")
            patch = patch[:-1]
        if len(patch) != self.ndim or min(patch) < 1:
            raise ValueError(f"patch_size must hold {self.ndim} positive extents for these volumes, got {patch_size!r}")
        self.patch = patch
        Pz, Py, Px = (1, *patch) if self.ndim == 2 else patch
        maps = None if class_maps is None else _as_list(class_maps, "class_maps")
        if maps is not None and len(maps) != len(imgs):
            raise ValueError(f"class_maps must hold one map per volume: {len(maps)} maps, {len(imgs)} volumes")
        self.extents = []
        for v, (im, tg) in enumerate(zip(imgs, tgts)):
            for name, a, ch, dt in (("images", im, self.C, self.img_dtype), ("targets", tg, self.Ct, self.tgt_dtype)):
                if a.dim() != self.ndim + 1 or a.shape[-1] != ch or a.dtype != dt:
                    raise ValueError(f"{name}[{v}] has shape {tuple(a.shape)} and dtype {a.dtype}: every volume must have {self.ndim + 1} dimensions, "
                                     f"{ch} channels and dtype {dt} like the first")
                if not a.is_contiguous():
                    raise ValueError(f"{name}[{v}] is non-contiguous (strides {tuple(a.stride())}): a resident volume must be contiguous")
            if tuple(im.shape[:-1]) != tuple(tg.shape[:-1]):
                raise ValueError(f"mismatched extents: images[{v}] covers {tuple(im.shape[:-1])}, targets[{v}] {tuple(tg.shape[:-1])}")
            ext = (1, *im.shape[:-1]) if self.ndim == 2 else tuple(im.shape[:-1])
            if min(ext) < 1 or max(ext) >= 2 ** 31:
                raise ValueError(f"images[{v}] has extents {tuple(im.shape[:-1])}: each must lie in 1 .. 2^31 - 1")
            if Pz > ext[0] or Py > ext[1] or Px > ext[2]:
                raise ValueError(f"volume {v} with extents {tuple(im.shape[:-1])} is smaller than the patch {patch}")
            if maps is not None:
                m = maps[v]
                if m.dtype != torch.uint8 or tuple(m.shape) != tuple(im.shape[:-1]):
                    raise ValueError(f"class_maps[{v}] must be uint8 with the extents {tuple(im.shape[:-1])} of its volume, got {m.dtype} "
                                     f"{tuple(m.shape)}")
                if not m.is_contiguous():
                    raise ValueError(f"class_maps[{v}] is non-contiguous: a class map must be contiguous")
            self.extents.append(tuple(int(e) for e in ext))
        every = imgs + tgts + (maps or [])
        for a in every:
            if not a.is_cuda:
                raise ValueError("volumes must be CUDA/HIP tensors: biapy_amd.sampler draws and copies on the device only, there is no CPU path")
        self.device = imgs[0].device
        if any(a.device != self.device for a in every):
            raise ValueError("all volumes, targets and class maps must live on one device")
        if scale is not None:
            scale = float(scale)
            if not np.isfinite(scale):
                raise ValueError(f"scale must be finite, got {scale!r}")
        self.scale = scale
        if seed is None:
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
            seed = torch.initial_seed() + rank                        # ranks draw differently
        try:
            self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        except (TypeError, ValueError):
            raise ValueError(f"seed must be an integer, got {seed!r}") from None
        self.images, self.targets, self.class_maps = imgs, tgts, maps

        # ---- the tables of the draw, built once ----
        V = len(imgs)
        self._vols_h = (L.PatchVol * V)()
        row0 = 0
        for v, (Z, Y, X) in enumerate(self.extents):
            self._vols_h[v] = L.PatchVol(imgs[v].data_ptr(), tgts[v].data_ptr(), maps[v].data_ptr() if maps else None, Z, Y, X, 0, row0)
            row0 += Z * Y
        self._rows = row0
        self._vols_d = torch.frombuffer(bytearray(bytes(self._vols_h)), dtype=torch.uint8).to(self.device)
        self._cum = self._rowcum = None
        if maps is None:
            n = [(Z - Pz + 1) * (Y - Py + 1) * (X - Px + 1) for Z, Y, X in self.extents]
            cum = [0]
            for a in n:
                cum.append(cum[-1] + a)
            if cum[-1] >= 2 ** 63:
                raise ValueError("the volumes hold 2^63 or more patch origins")
            self._cum = torch.tensor(cum, dtype=torch.int64).to(self.device)
        else:
            K = len(self.class_probs)
            if max(int(m.max()) for m in maps) >= K:
                raise ValueError(f"class_maps hold a value of {max(int(m.max()) for m in maps)}: every value must be below the {K} classes of class_probs")
            rowcum = torch.zeros((K, self._rows + 1), dtype=torch.int64, device=self.device)
            for c in range(K):                                         # integer sums on the device: exact in any order
                counts = torch.cat([(m == c).sum(dim=-1, dtype=torch.int64).reshape(-1) for m in maps])
                torch.cumsum(counts, 0, out=rowcum[c, 1:])
            totals = rowcum[:, -1].tolist()
            for c, (p, n_c) in enumerate(zip(self.class_probs, totals)):
                if p > 0 and n_c == 0:
                    raise ValueError(f"class {c} has probability {p:g} but no voxel in any class map")
            self._rowcum = rowcum
            self.class_counts = totals
        self._state = torch.zeros(2, dtype=torch.int64, device=self.device)          # [counter, ticket of the draw kernel]
        self._origins = torch.zeros((self.batch_size, 4), dtype=torch.int32, device=self.device)
        c = self.config()
        cum = c["class_cum"] or []
        self._cfg = L.PatchCfg(self.seed, V, Pz, Py, Px, len(cum), (ctypes.c_float * 8)(*cum))

    # ---- configuration --------------------------------------------------------------------------------------------------------
    def config(self) -> dict:
        """The draw parameters as plain numbers (``tests/sampler_ref.draw`` takes the same dict)."""
        return dict(seed=self.seed, batch_size=self.batch_size, patch=(1, *self.patch) if self.ndim == 2 else tuple(self.patch),
                    extents=list(self.extents), class_probs=None if self.class_probs is None else list(self.class_probs),
                    class_cum=None if self.class_probs is None else class_cum(self.class_probs), scale=self.scale)

    @staticmethod
    def foreground_map(target: torch.Tensor) -> torch.Tensor:
        """The two-class map of a target ``([Z,]Y,X,Ct)``: uint8, 1 where channel 0 is non-zero, else 0."""
        return (target[..., 0] != 0).to(torch.uint8).contiguous()

    @classmethod
    def from_cfg(cls, cfg, images, targets, seed: Optional[int] = None) -> "DevicePatchSampler":
        """The sampler a reference configuration asks for: ``DATA.PATCH_SIZE`` (its trailing channel entry must match the images) and
        ``TRAIN.BATCH_SIZE``; with ``DATA.PROBABILITY_MAP`` true the class mode over ``foreground_map`` of every target with the probabilities
        ``(DATA.W_BACKGROUND, DATA.W_FOREGROUND)``, else the uniform mode.

        The key names are written from memory of the reference's configuration tree and could not be verified against it on the build machine;
        the semantics of the draw are this package's own (parity-unpinned, see the module docstring)."""
        from .train_engine import _cfg_get

        patch = _cfg_get(cfg, "DATA.PATCH_SIZE", None)
        if not patch:
            raise ValueError("DATA.PATCH_SIZE is missing from the configuration")
        batch = _cfg_get(cfg, "TRAIN.BATCH_SIZE", None)
        if batch is None:
            raise ValueError("TRAIN.BATCH_SIZE is missing from the configuration")
        kw = {}
        if _cfg_get(cfg, "DATA.PROBABILITY_MAP", False):
            kw["class_maps"] = [cls.foreground_map(t) for t in _as_list(targets, "targets")]
            kw["class_probs"] = (_cfg_get(cfg, "DATA.W_BACKGROUND", 0.06), _cfg_get(cfg, "DATA.W_FOREGROUND", 0.94))
        return cls(images, targets, tuple(patch), batch_size=batch, seed=seed, **kw)

    # ---- state ----------------------------------------------------------------------------------------------------------------
    @property
    def counter(self) -> torch.Tensor:
        """The device counter (int64 scalar view): the value the NEXT call draws with."""
        return self._state[0]

    @property
    def last_origins(self) -> torch.Tensor:
        """The ``(B, 4)`` int32 device tensor ``(v, z0, y0, x0)`` of the last call (the sampler's own buffer, overwritten by the next call)."""
        return self._origins

    def _out_shapes(self):
        B = self.batch_size
        return (B, *self.patch, self.C), (B, *self.patch, self.Ct)

    # ---- the call -------------------------------------------------------------------------------------------------------------
    def __call__(self, out=None, *, origins: Optional[torch.Tensor] = None):
        xs, ts = self._out_shapes()
        if out is None:
            x_out = torch.empty(xs, dtype=torch.float32, device=self.device)
            t_out = torch.empty(ts, dtype=self.tgt_dtype, device=self.device)
        else:
            try:
                x_out, t_out = out
            except (TypeError, ValueError):
                raise ValueError("out must be a pair (x_out, t_out)") from None
            for name, o, shape, dt in (("out[0]", x_out, xs, torch.float32), ("out[1]", t_out, ts, self.tgt_dtype)):
                if not torch.is_tensor(o) or o.device != self.device or o.dtype != dt or tuple(o.shape) != shape or not o.is_contiguous():
                    raise ValueError(f"{name} must be a contiguous {dt} tensor of shape {shape} on {self.device}")
            so = [_span(x_out), _span(t_out)]
            if so[0][0] < so[1][1] and so[1][0] < so[0][1]:
                raise ValueError("out[0] and out[1] overlap")
            for a0, a1 in so:
                for src in self.images + self.targets + (self.class_maps or []) + [self._origins]:
                    b0, b1 = _span(src)
                    if a0 < b1 and b0 < a1:
                        raise ValueError("out overlaps a resident volume: the copy is a gather pass and cannot write what it reads")
        if origins is not None:
            B = self.batch_size
            if (not torch.is_tensor(origins) or origins.device != self.device or origins.dtype != torch.int32 or tuple(origins.shape) != (B, 4)
                    or not origins.is_contiguous()):
                raise ValueError(f"origins must be a contiguous ({B}, 4) int32 tensor on {self.device}")
            o = origins.cpu().tolist()                                 # the inspection hook reads back: given origins are checked on the host
            Pz, Py, Px = self.config()["patch"]
            for b, (v, z0, y0, x0) in enumerate(o):
                if not 0 <= v < len(self.extents):
                    raise ValueError(f"origins[{b}] names volume {v}: there are {len(self.extents)}")
                Z, Y, X = self.extents[v]
                if not (0 <= z0 <= Z - Pz and 0 <= y0 <= Y - Py and 0 <= x0 <= X - Px):
                    raise ValueError(f"origins[{b}] = {(z0, y0, x0)} puts the patch outside volume {v} with extents {(Z, Y, X)}")
        s = L.stream_ptr()
        c = self._cfg
        if origins is None:
            L.check(lib.bpx_patch_draw(ctypes.addressof(c), ctypes.addressof(self._vols_h), self._vols_d.data_ptr(), L.ptr(self._cum),
                                       L.ptr(self._rowcum), self._rows, self.batch_size, self._state.data_ptr(), self._origins.data_ptr(), s))
        else:
            self._origins.copy_(origins)
        L.check(lib.bpx_patch_gather(ctypes.addressof(self._vols_h), self._vols_d.data_ptr(), c.V, _IMG_DTYPES[self.img_dtype], self.C,
                                     _TGT_DTYPES[self.tgt_dtype], self.Ct, c.Pz, c.Py, c.Px, self._origins.data_ptr(), self.batch_size,
                                     int(self.scale is not None), float(self.scale or 0.0), x_out.data_ptr(), t_out.data_ptr(), s))
        return x_out, t_out


class DevicePatchLoader:
    """``steps_per_epoch`` calls of a ``DevicePatchSampler`` as an iterable of ``(batch, targets)``, fresh tensors each: a ``data_loader`` of
    ``train_engine.train_one_epoch(..., augment=...)``."""

    def __init__(self, sampler: DevicePatchSampler, steps_per_epoch: int):
        if not isinstance(sampler, DevicePatchSampler):
            raise ValueError(f"sampler must be a DevicePatchSampler, got {type(sampler).__name__}")
        self.sampler = sampler
        self.steps_per_epoch = int(steps_per_epoch)
        if self.steps_per_epoch < 1:
            raise ValueError(f"steps_per_epoch must be at least 1, got {steps_per_epoch!r}")

    def __len__(self) -> int:
        return self.steps_per_epoch

    def __iter__(self):
        for _ in range(self.steps_per_epoch):
            yield self.sampler()

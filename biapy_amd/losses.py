"""Segmentation losses / metrics on the device: the binary (1-channel) head, and heads of 2..8 channels.

Mirrors ``biapy/engine/metrics.py``: ``CrossEntropyLoss_wrapper`` (:493-586; the default ``LOSS.TYPE = "CE"`` on one output
channel is ``BCEWithLogitsLoss``), ``DiceLoss`` (:726-762, ``batch_dice=True``, smooth 1e-5), ``DiceCELoss`` (:764-973,
binary case: ``w_ce * BCE + w_dice * (1 - Dice)``) and ``jaccard_index`` (:138-232, threshold 0.5).  One streaming HIP kernel
produces every sum the four need (``bpx_seg_loss_sums``); the backward is one more pass (``bpx_seg_loss_bwd``).  Round 6: the multi-class
case of ``CrossEntropyLoss_wrapper`` (``num_classes > 2``: softmax cross entropy over 3..8 class channels with ``ignore_index`` and the "manual"
class weights) and the confusion counts of the multi-class IoU run on the device too (``bpx_softmax_ce_*``).  These two and the per-channel losses
(``bpx_chan_loss_*``) are csrc/plain_losses.hip; the pieces every loss kernel shares are csrc/loss_parts.h.

Dice and Dice + CE on heads of 2..8 channels (``bpx_dice_*``, csrc/losses.hip: sums, finish, backward - three launches per loss call whatever N,
``batch_dice`` or the CE weight are, no host read-back).  Logits are ``(N, C, *space)`` fp32; ``C = 1`` keeps the one-channel path above, more than
8 channels raise ``NotImplementedError``.  The target's shape chooses the mode:

* CHANNEL mode, ``target.shape == logits.shape``: ``p = sigmoid(z)`` per channel, ``I[n,c] = sum_v p t``, ``P = sum_v p``, ``T = sum_v t``
  (``batch_dice=True`` sums them over ``n`` as well), ``dice = (2 I + s) / (P + T + s)``, ``loss = 1 - mean(dice)`` over ``c`` and - per sample - over
  ``n``.  This is ``oracle.loss_oracle.dice``, which is PINNED to the reference's ``DiceLoss``.  ``DiceCELoss`` here is
  ``w_ce * BCEWithLogits(mean over all elements) + w_dice * dice`` = ``oracle.loss_oracle.dice_ce``.
* CLASS mode, the target is a label map ``(N, 1, *space)`` or ``(N, *space)`` of class ids as floats: ``p = softmax_c(z)``, ``t = one-hot(label)``.
  A voxel counts if its label is not ``ignore_index`` and lies in ``[0, C)``; uncounted voxels leave all of ``I``, ``P``, ``T`` and the CE sums.  The
  same Dice formula over all ``C`` classes (a class absent from the labels contributes ``s / (P + s)``); the CE term is the softmax cross entropy of
  ``CrossEntropyLoss_wrapper`` (``class_weights`` on the CE term only, ``ignore_index = -1`` meaning -100);
  ``loss = w_ce * CE + w_dice * (1 - mean dice)``.  A term whose weight is 0 is not formed: an all-ignored batch with ``w_ce = 0`` gives a finite
  value, with ``w_ce != 0`` NaN as torch does.  PRODUCT-DEFINED, PARITY-UNPINNED: ``oracle/`` restates only the sigmoid ``DiceLoss``, so this mode
  is checked against its own fp64 statement (tests/loss_bounds.py) and fp64 autograd, not against the reference's values.

Gradient, with ``U = P + T``, ``M`` the number of dice terms averaged (``C``, or ``N C`` per sample), ``a0[c] = (2 I_c + s) / (M (U_c + s)^2)`` and
``a1[c] = a0[c] - 2 / (M (U_c + s))``: class mode ``dz[v,c] = w_dice g p_c (a[c; t_vc] - sum_k p_k a[k; t_vk])`` on counted voxels
(``a[c; t] = a1[c]`` where ``t = 1``, ``a0[c]`` where ``t = 0``) plus the CE gradient, 0 on uncounted voxels; channel mode
``dz = g (w_dice a p (1 - p) + w_ce (p - t) / numel)`` with ``a = a0 + t (a1 - a0)``.
"""
from __future__ import annotations

import torch

from . import _lib as L

lib = L.lib


def _sums_and_loss(logits: torch.Tensor, target: torch.Tensor, w_ce: float = 1.0, w_dice: float = 0.0, smooth: float = 1e-5):
    """({sum bce, sum p*t, sum p, sum t, |P&T|, |P|T|} as a float64 device tensor, the loss as a 0-d float32 device tensor): one streaming
    pass + one single-block kernel that sums the partial rows in a fixed order in double and forms the loss (no host sync, no PyTorch
    element-wise launches: round 2's profile showed ~25 of them per training step)."""
    n = logits.numel()
    nb = lib.bpx_seg_loss_blocks(n)
    part = torch.empty((nb, 6), dtype=torch.float32, device=logits.device)
    L.check(lib.bpx_seg_loss_sums(logits.data_ptr(), target.data_ptr(), n, part.data_ptr(), L.stream_ptr()))
    sums = torch.empty(6, dtype=torch.float64, device=logits.device)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    L.check(lib.bpx_seg_loss_finish(part.data_ptr(), nb, n, w_ce, w_dice, smooth, sums.data_ptr(), loss.data_ptr(), L.stream_ptr()))
    return sums, loss


def _sums(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return _sums_and_loss(logits, target)[0]


def _aligned16(x: torch.Tensor) -> torch.Tensor:
    """x as a contiguous float32 tensor whose storage starts on a 16-byte boundary, which the 16-byte loads of bpx_seg_loss_sums / _bwd_fused
    require.  A batch slice ``x[i:i + 1]`` is contiguous as it stands and starts 4 i V bytes into its base: it is copied when that is no multiple
    of 16 (a fresh allocation is aligned)."""
    x = x.contiguous().to(torch.float32)
    return x.clone() if x.data_ptr() % 16 else x


def _prep(logits: torch.Tensor, target: torch.Tensor):
    if not logits.is_cuda:
        raise RuntimeError("biapy_amd.losses run on the MI355X only (logits are on %s); there is no CPU path" % logits.device)
    if logits.dim() < 3 or logits.shape[1] != 1:
        raise NotImplementedError("biapy_amd.losses implement the 1-channel (binary) head; use the reference losses for multi-class outputs")
    if target.shape != logits.shape:
        raise ValueError(f"target shape {tuple(target.shape)} != logits shape {tuple(logits.shape)}")
    return _aligned16(logits), _aligned16(target)


class _SegLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, w_ce, w_dice, smooth):
        z, t = _prep(logits, target)
        s, loss = _sums_and_loss(z, t, w_ce, w_dice, smooth)
        ctx.save_for_backward(z, t, s)
        ctx.cfg = (w_ce, w_dice, smooth, z.numel())
        return loss

    @staticmethod
    def backward(ctx, g):
        z, t, s = ctx.saved_tensors
        w_ce, w_dice, smooth, n = ctx.cfg
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.to(torch.float32).contiguous()
        dz = torch.empty_like(z)
        # the three coefficients a = w_ce g / n, b = 2 w_dice g / (U + s), c = w_dice g (2 I + s) / (U + s)^2 are formed inside the kernel
        L.check(lib.bpx_seg_loss_bwd_fused(z.data_ptr(), t.data_ptr(), n, s.data_ptr(), g.data_ptr(), w_ce, w_dice, smooth, dz.data_ptr(), L.stream_ptr()))
        return dz, None, None, None, None


class BCEWithLogitsLoss(torch.nn.Module):
    """``CrossEntropyLoss_wrapper`` on a 1-channel head (metrics.py:543-544)."""

    def forward(self, logits, target):
        return _SegLossFn.apply(logits, target, 1.0, 0.0, 1e-5)


class DiceLoss(torch.nn.Module):
    """metrics.py:726-762: ``batch_dice=True`` (sums over batch and space) and ``batch_dice=False`` (Dice per sample, then the mean).  One channel:
    the binary passes; 2..8 channels: the multi-channel passes (module docstring: channel mode for a target of the logits' shape, class mode for a
    label map, where ``ignore_index = -1`` means -100)."""

    def __init__(self, batch_dice: bool = True, smooth: float = 1e-5, *, ignore_index: int = -1):
        super().__init__()
        self.batch_dice, self.smooth = bool(batch_dice), smooth
        self.ignore_index = ignore_index if ignore_index != -1 else -100

    def forward(self, logits, target):
        logits = _single_pred(logits, "DiceLoss")
        if _multi_channel(logits):
            loss = _DiceFn.apply(logits, target, None, 0.0, 1.0, float(self.smooth), self.batch_dice, self.ignore_index)
            self._dice_sums_d = _last_dice_sums            # last_label_faults(self)
            return loss
        if self.batch_dice:
            return _SegLossFn.apply(logits, target, 0.0, 1.0, self.smooth)
        # batch_dice=False (:749-751): the sums stay per sample, the loss is 1 - mean_n dice_n = mean_n (1 - dice_n): the same fused passes once per
        # sample (contiguous slices of the one-channel logits), averaged
        return torch.stack([_SegLossFn.apply(logits[i:i + 1], target[i:i + 1], 0.0, 1.0, self.smooth) for i in range(logits.shape[0])]).mean()


class DiceCELoss(torch.nn.Module):
    """metrics.py:764-973.  One channel: ``w_ce * BCEWithLogits + w_dice * DiceLoss`` (the binary passes; ``batch_dice`` must stay True there).
    2..8 channels: the multi-channel passes (module docstring) - ``class_rebalance="manual"`` passes ``class_weights`` to the class mode's CE term.
    A dict prediction is read at ``"pred"``; a list of predictions (deep supervision) is refused."""

    def __init__(self, w_ce: float = 1.0, w_dice: float = 1.0, smooth: float = 1e-5, *, num_classes: int = 2, ndim: int = 3, batch_dice: bool = True,
                 class_rebalance: str = "none", class_weights=(), ignore_index: int = -1):
        super().__init__()
        self.w_ce, self.w_dice, self.smooth = float(w_ce), float(w_dice), float(smooth)
        self.num_classes, self.ndim, self.batch_dice, self.class_rebalance = int(num_classes), ndim, bool(batch_dice), class_rebalance
        self.ignore_index = ignore_index if ignore_index != -1 else -100
        if class_rebalance not in ("none", "manual"):
            raise NotImplementedError(f"biapy_amd.losses.DiceCELoss: class_rebalance={class_rebalance!r} is not built ('none' or 'manual' with class_weights)")
        self.class_weights = torch.tensor(list(class_weights), dtype=torch.float32) if class_rebalance == "manual" else None

    def forward(self, logits, target):
        logits = _single_pred(logits, "DiceCELoss")
        if not _multi_channel(logits):
            if not self.batch_dice or self.class_weights is not None:
                raise NotImplementedError("biapy_amd.losses.DiceCELoss: the one-channel case sums Dice over the batch and takes no class weights")
            return _SegLossFn.apply(logits, target, self.w_ce, self.w_dice, self.smooth)
        if target.shape != logits.shape and self.num_classes > 2 and self.num_classes != logits.shape[1] <= DICE_MAXC:
            raise ValueError(f"DiceCELoss(num_classes={self.num_classes}) got logits of {logits.shape[1]} class channels")
        w = self.class_weights
        if w is not None:
            if target.shape == logits.shape:
                raise NotImplementedError("biapy_amd.losses.DiceCELoss: class weights belong to the class mode (label-map target)")
            if w.numel() != logits.shape[1]:
                raise ValueError(f"{w.numel()} class weights for {logits.shape[1]} class channels")
            if w.device != logits.device and logits.is_cuda:
                w = self.class_weights = w.to(logits.device)
        loss = _DiceFn.apply(logits, target, w, self.w_ce, self.w_dice, self.smooth, self.batch_dice, self.ignore_index)
        self._dice_sums_d = _last_dice_sums                # last_label_faults(self)
        return loss


@torch.no_grad()
def _jaccard_binary(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    z, t = _prep(logits, target)
    s = _sums(z, t)
    return (s[4] / torch.clamp(s[5], min=1.0)).to(torch.float32)


class jaccard_index:
    """``biapy.engine.metrics.jaccard_index`` (metrics.py:138-232): the reference builds the metric once - ``jaccard_index(num_classes=, device=, t=,
    model_source=, ndim=, ignore_index=)`` - and calls it with ``(y_pred, y_true)`` per batch; the same here, on the fused device passes.
    ``num_classes <= 2``: IoU of ``sigmoid(logits) > 0.5`` against ``target > 0.5`` on the one-channel head (thresholds other than 0.5 and an
    ignore value are refused: the reference leaves them to torchmetrics); ``num_classes > 2``: ``jaccard_index_multiclass`` (parity-unpinned, see
    there).  A dict prediction is read at ``"pred"``, a list of predictions is averaged with the target rescaled by nearest-neighbour interpolation
    (:219-231).  ``jaccard_index(logits, target)`` with two tensors keeps the functional form of rounds 2-5 (binary IoU, 0-d device tensor)."""

    def __new__(cls, *args, **kwargs):
        if len(args) >= 2 and isinstance(args[0], torch.Tensor):
            return _jaccard_binary(args[0], args[1])
        return super().__new__(cls)

    def __init__(self, num_classes: int, device=None, t: float = 0.5, model_source: str = "biapy", ndim: int = 2, ignore_index: int = -1):
        self.num_classes, self.device, self.t, self.model_source, self.ndim = int(num_classes), device, float(t), model_source, ndim
        self.ignore_index = ignore_index if ignore_index != -1 else None
        if self.num_classes <= 2 and (self.t != 0.5 or self.ignore_index is not None):
            raise NotImplementedError("biapy_amd.losses.jaccard_index: the binary IoU kernel thresholds at 0.5 and has no ignore value; use the reference metric")
        if model_source != "biapy":
            raise NotImplementedError("biapy_amd.losses.jaccard_index: only model_source='biapy' (one-channel binary head / class channels)")

    @torch.no_grad()
    def __call__(self, y_pred, y_true):
        pds = y_pred["pred"] if isinstance(y_pred, dict) and "pred" in y_pred else y_pred
        if not isinstance(pds, list):
            pds = [pds]
        iou = 0
        for pd in pds:
            yt = y_true
            if pd.shape[-self.ndim:] != y_true.shape[-self.ndim:]:
                yt = torch.nn.functional.interpolate(y_true.clone().float(), size=pd.shape[-self.ndim:], mode="nearest")
            if self.num_classes > 2:
                iou = iou + jaccard_index_multiclass(pd, yt, -100 if self.ignore_index is None else self.ignore_index)
            else:
                iou = iou + _jaccard_binary(pd, yt)
        return iou / len(pds)


@torch.no_grad()
def hard_dice(logits: torch.Tensor, target: torch.Tensor, smooth: float = 1e-5) -> torch.Tensor:
    """Dice of the binarised prediction (the parity metric of BASELINE.json): 2|P&T| / (|P| + |T|)."""
    z, t = _prep(logits, target)
    s = _sums(z, t)
    return ((2.0 * s[4] + smooth) / (s[4] + s[5] + smooth)).to(torch.float32)   # |P| + |T| = |P&T| + |P|T|


# ---------------------------------------------------------------------------------------------------------------------------
# multi-class semantic segmentation (MODEL.N_CLASSES > 2): softmax cross entropy + per-class confusion counts
# ---------------------------------------------------------------------------------------------------------------------------
def _prep_classes(logits: torch.Tensor, target: torch.Tensor):
    if logits.dim() < 3 or not 2 <= logits.shape[1] <= 8:
        raise NotImplementedError("biapy_amd.losses: the multi-class cross entropy takes 2..8 class channels; use the reference loss beyond that")
    if not logits.is_cuda:
        raise RuntimeError("biapy_amd.losses run on the MI355X only (logits are on %s); there is no CPU path" % logits.device)
    if target.dim() == logits.dim() - 1:
        target = target.unsqueeze(1)
    if target.shape[0] != logits.shape[0] or target.shape[1] != 1 or target.shape[2:] != logits.shape[2:]:
        raise ValueError(f"target shape {tuple(target.shape)} does not match logits {tuple(logits.shape)} (one label channel expected)")
    return logits.contiguous().to(torch.float32), target.contiguous().to(torch.float32)      # class ids as floats (exact below 2^24)


def _softmax_ce_sums(z: torch.Tensor, t: torch.Tensor, ignore_index: int, weight):
    N, C = z.shape[0], z.shape[1]
    vox = z.numel() // (N * C)
    nb, row = lib.bpx_softmax_ce_blocks(vox), lib.bpx_softmax_ce_row()
    part = torch.empty((N * nb, row), dtype=torch.float32, device=z.device)
    L.check(lib.bpx_softmax_ce_sums(z.data_ptr(), t.data_ptr(), N, C, vox, ignore_index, L.ptr(weight), part.data_ptr(), L.stream_ptr()))
    sums = torch.empty(row, dtype=torch.float64, device=z.device)
    loss = torch.empty((), dtype=torch.float32, device=z.device)
    L.check(lib.bpx_softmax_ce_finish(part.data_ptr(), N, vox, sums.data_ptr(), loss.data_ptr(), L.stream_ptr()))
    return sums, loss


class _SoftmaxCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index):
        z, t = _prep_classes(logits, target)
        s, loss = _softmax_ce_sums(z, t, ignore_index, weight)
        ctx.save_for_backward(z, t, s, weight if weight is not None else z.new_empty(0))
        ctx.cfg = (ignore_index, weight is not None, logits.dtype)
        return loss

    @staticmethod
    def backward(ctx, g):
        z, t, s, w = ctx.saved_tensors
        ignore_index, has_w, dtype = ctx.cfg
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.to(torch.float32).contiguous()
        N, C = z.shape[0], z.shape[1]
        dz = torch.empty_like(z)
        L.check(lib.bpx_softmax_ce_bwd(z.data_ptr(), t.data_ptr(), N, C, z.numel() // (N * C), ignore_index, w.data_ptr() if has_w else None,
                                       s.data_ptr(), g.data_ptr(), dz.data_ptr(), L.stream_ptr()))
        return dz.to(dtype), None, None, None


# ---------------------------------------------------------------------------------------------------------------------------
# Dice / Dice + CE on 2..8 channels (module docstring): bpx_dice_sums -> bpx_dice_finish -> bpx_dice_bwd
# ---------------------------------------------------------------------------------------------------------------------------
def _single_pred(y_pred, who: str):
    pd = y_pred["pred"] if isinstance(y_pred, dict) and "pred" in y_pred else y_pred
    if isinstance(pd, (list, tuple)):
        raise NotImplementedError(f"biapy_amd.losses.{who}: a list of predictions (deep supervision) is not built; use the reference loss")
    return pd


def _multi_channel(logits: torch.Tensor) -> bool:
    return logits.dim() >= 3 and logits.shape[1] != 1


def _prep_dice(logits: torch.Tensor, target: torch.Tensor):
    """(z, t, class_mode): channel mode for a target of the logits' shape, class mode for a label map."""
    if logits.dim() < 3 or not 2 <= logits.shape[1] <= 8:
        raise NotImplementedError("biapy_amd.losses: the multi-channel Dice losses take 2..8 channels; use the reference loss beyond that")
    class_mode = target.shape != logits.shape
    if class_mode:
        if target.dim() == logits.dim() - 1:
            target = target.unsqueeze(1)
        if target.dim() != logits.dim() or target.shape[0] != logits.shape[0] or target.shape[1] != 1 or target.shape[2:] != logits.shape[2:]:
            raise ValueError(f"target shape {tuple(target.shape)} matches neither the logits {tuple(logits.shape)} (channel mode) nor their label map (class mode)")
    if not logits.is_cuda:
        raise RuntimeError("biapy_amd.losses run on the MI355X only (logits are on %s); there is no CPU path" % logits.device)
    return logits.contiguous().to(torch.float32), target.contiguous().to(torch.float32), class_mode      # class ids as floats (exact below 2^24)


# the layout csrc/losses.hip writes (DICE_MAXC, DR_*, DICE_COEF_* there; tests/test_dice_losses_cpu.py compares the two files): a row of sums is
# {I[8], P[8], T[8], CE sum, weight sum, labels out of range, counted voxels}, the coefficients are a head of 8 floats and 16 per group
DICE_MAXC = 8
DR_I, DR_P, DR_T, DR_CE, DR_W, DR_FAULT, DR_CNT = 0, DICE_MAXC, 2 * DICE_MAXC, 3 * DICE_MAXC, 3 * DICE_MAXC + 1, 3 * DICE_MAXC + 2, 3 * DICE_MAXC + 3
DICE_ROW, DICE_COEF_HEAD, DICE_COEF_GROUP = 3 * DICE_MAXC + 4, 8, 2 * DICE_MAXC
assert lib.bpx_dice_row() == DICE_ROW, "biapy_amd.losses and csrc/losses.hip disagree about the row of Dice sums"

_last_dice_sums = None     # the sums of the latest multi-channel Dice call of any loss object (device tensor; read only when asked)


def _dice_sums(z, t, class_mode, weight, w_ce, w_dice, smooth, batch_dice, ignore_index):
    """(batch totals as a float64 device tensor of bpx_dice_row() columns, the backward's coefficients, the loss as a 0-d float32 device tensor)."""
    global _last_dice_sums
    N, C = z.shape[0], z.shape[1]
    vox = z.numel() // (N * C)
    nb, row = lib.bpx_dice_blocks(vox), lib.bpx_dice_row()
    part = torch.empty((N * nb, row), dtype=torch.float32, device=z.device)
    L.check(lib.bpx_dice_sums(z.data_ptr(), t.data_ptr(), N, C, vox, int(class_mode), ignore_index, L.ptr(weight), int(w_ce != 0.0), part.data_ptr(),
                              L.stream_ptr()))
    sums = torch.empty(row, dtype=torch.float64, device=z.device)
    coef = torch.empty(DICE_COEF_HEAD + DICE_COEF_GROUP * (1 if batch_dice else N), dtype=torch.float32, device=z.device)
    loss = torch.empty((), dtype=torch.float32, device=z.device)
    L.check(lib.bpx_dice_finish(part.data_ptr(), N, C, vox, int(class_mode), int(batch_dice), w_ce, w_dice, smooth, sums.data_ptr(), coef.data_ptr(),
                                loss.data_ptr(), L.stream_ptr()))
    _last_dice_sums = sums
    return sums, coef, loss


class _DiceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, weight, w_ce, w_dice, smooth, batch_dice, ignore_index):
        z, t, class_mode = _prep_dice(logits, target)
        if weight is not None and not class_mode:
            raise NotImplementedError("biapy_amd.losses: class weights belong to the class mode (label-map target)")
        _, coef, loss = _dice_sums(z, t, class_mode, weight, w_ce, w_dice, smooth, batch_dice, ignore_index)
        ctx.save_for_backward(z, t, coef, weight if weight is not None else z.new_empty(0))
        ctx.cfg = (class_mode, batch_dice, ignore_index, weight is not None, logits.dtype)
        return loss

    @staticmethod
    def backward(ctx, g):
        z, t, coef, w = ctx.saved_tensors
        class_mode, batch_dice, ignore_index, has_w, dtype = ctx.cfg
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.to(torch.float32).contiguous()
        N, C = z.shape[0], z.shape[1]
        dz = torch.empty_like(z)
        L.check(lib.bpx_dice_bwd(z.data_ptr(), t.data_ptr(), N, C, z.numel() // (N * C), int(class_mode), int(batch_dice), ignore_index,
                                 w.data_ptr() if has_w else None, coef.data_ptr(), g.data_ptr(), dz.data_ptr(), L.stream_ptr()))
        return dz.to(dtype), None, None, None, None, None, None, None


@torch.no_grad()
def soft_dice_per_class(logits: torch.Tensor, target: torch.Tensor, ignore_index: int = -100) -> torch.Tensor:
    """``(C,)`` float32 device tensor of the soft Dice per class / channel over the batch, ``(2 I + 1e-5) / (P + T + 1e-5)``, from the sums pass of
    the multi-channel Dice losses (either mode) - for logging; nothing is read back."""
    z, t, class_mode = _prep_dice(_single_pred(logits, "soft_dice_per_class"), target)
    s, _, _ = _dice_sums(z, t, class_mode, None, 0.0, 1.0, 1e-5, True, ignore_index)
    C = z.shape[1]
    return ((2.0 * s[DR_I:DR_I + C] + 1e-5) / (s[DR_P:DR_P + C] + s[DR_T:DR_T + C] + 1e-5)).to(torch.float32)


def last_label_faults(loss_module=None) -> int:
    """Labels outside ``[0, C)`` other than ``ignore_index`` that a multi-channel Dice call met (they are left out of every sum, like ignored voxels;
    channel mode: none).  ``loss_module``: a ``DiceLoss`` / ``DiceCELoss`` object - ITS latest call; without it the latest call of any of them,
    ``soft_dice_per_class`` included.  The count rides with the sums on the device; THIS call reads it back (one sync) - the train step never does."""
    sums = _last_dice_sums if loss_module is None else getattr(loss_module, "_dice_sums_d", None)
    return 0 if sums is None else int(sums[DR_FAULT].item())


class CrossEntropyLoss_wrapper(torch.nn.Module):
    """``biapy.engine.metrics.CrossEntropyLoss_wrapper`` (metrics.py:493-586), same constructor: ``num_classes <= 2`` is ``BCEWithLogitsLoss`` on the
    one-channel head, ``num_classes > 2`` is ``torch.nn.CrossEntropyLoss(ignore_index, weight)`` on the class channels against the label map
    ``y_true[:, 0]`` - both as fused device passes.  ``class_rebalance="manual"`` passes ``class_weights``; ``ignore_index=-1`` means torch's
    default -100 (:535).  A dict prediction is read at ``"pred"``; a LIST of predictions (deep supervision, :566-583) is weighted by 0.5^i / sum
    with the target rescaled by nearest-neighbour interpolation, as the reference does."""

    def __init__(self, num_classes: int, ndim: int = 2, class_rebalance: str = "none", class_weights=(), ignore_index: int = -1, device=None):
        super().__init__()
        self.ndim, self.num_classes, self.class_rebalance = ndim, int(num_classes), class_rebalance
        self.ignore_index = ignore_index if ignore_index != -1 else -100
        self.gamma = 0.5
        self.class_weights = None
        if class_rebalance == "manual":
            self.class_weights = torch.tensor(list(class_weights), dtype=torch.float32, device=device)
        if self.num_classes <= 2 and self.class_weights is not None:
            raise NotImplementedError("biapy_amd.losses: class weights of the binary (BCEWithLogits) case are not built; use the reference loss")

    def _one(self, pd, y_true):
        if self.num_classes <= 2:
            return _SegLossFn.apply(pd, y_true, 1.0, 0.0, 1e-5)
        w = self.class_weights
        if w is not None:
            if w.numel() != pd.shape[1]:
                raise ValueError(f"{w.numel()} class weights for {pd.shape[1]} class channels")
            if w.device != pd.device:
                w = self.class_weights = w.to(pd.device)
        return _SoftmaxCEFn.apply(pd, y_true[:, 0:1], w, self.ignore_index)

    def forward(self, y_pred, y_true):
        pds = y_pred["pred"] if isinstance(y_pred, dict) and "pred" in y_pred else y_pred
        if not isinstance(pds, list):
            pds, ws = [pds], [1.0]
        else:
            ws = [self.gamma ** i for i in range(len(pds))]
            ws = [x / sum(ws) for x in ws]
        loss = 0
        for pd, wj in zip(pds, ws):
            yt = y_true
            if pd.shape[-self.ndim:] != y_true.shape[-self.ndim:]:
                yt = torch.nn.functional.interpolate(y_true.clone().float(), size=pd.shape[-self.ndim:], mode="nearest")     # scale_target, metrics.py:437-455
            loss = loss + self._one(pd, yt) * wj
        return loss


@torch.no_grad()
def class_confusion_counts(logits: torch.Tensor, target: torch.Tensor, ignore_index: int = -100) -> torch.Tensor:
    """(3, C) float64 device tensor {|P_c & T_c|, |P_c|, |T_c|} of the argmax prediction against the label map, labels equal to ``ignore_index``
    left out - the confusion counts behind the multi-class ``jaccard_index`` (metrics.py:170-176)."""
    z, t = _prep_classes(logits, target)
    s, _ = _softmax_ce_sums(z, t, ignore_index, None)
    return s[2:].view(3, 8)[:, : z.shape[1]]


@torch.no_grad()
def jaccard_index_multiclass(logits: torch.Tensor, target: torch.Tensor, ignore_index: int = -100) -> torch.Tensor:
    """Macro-averaged IoU over the classes that occur in the prediction or the labels: mean_c tp_c / (|P_c| + |T_c| - tp_c).  The reference hands this
    to ``torchmetrics.JaccardIndex(task="multiclass")`` (metrics.py:170-173), which is not installed in this image: the definition is torchmetrics'
    documented macro average and is PARITY-UNPINNED (the counts themselves are checked against a confusion matrix in the tests)."""
    c = class_confusion_counts(logits, target, ignore_index)
    union = c[1] + c[2] - c[0]
    seen = union > 0
    return ((c[0] / torch.clamp(union, min=1.0)) * seen).sum().div(torch.clamp(seen.sum(), min=1)).to(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# multi-channel heads (row X / cfg 4: instance segmentation with B, C, D channels)
# ---------------------------------------------------------------------------------------------------------------------------
_KIND = {"bce": 0, "mse": 1, "l1": 2, "mae": 2}
_ACT = {"linear": 0, "ce_sigmoid": 0, "ce_softmax": 0, "tanh": 1, "sigmoid": 2}


class _ChanLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, codes, weights):
        if not logits.is_cuda:
            raise RuntimeError("biapy_amd.losses run on the MI355X only (logits are on %s); there is no CPU path" % logits.device)
        z, t = logits.contiguous().to(torch.float32), target.contiguous().to(torch.float32)
        N, Cc = z.shape[:2]
        vox = z[0, 0].numel()
        nb = lib.bpx_chan_loss_blocks(vox)
        part = torch.empty((N, Cc, nb), dtype=torch.float32, device=z.device)
        L.check(lib.bpx_chan_loss_sums(z.data_ptr(), t.data_ptr(), N, Cc, vox, codes, part.data_ptr(), L.stream_ptr()))
        # mean of every channel's terms (metrics.py:1784-1788), weighted and summed, by one single-block kernel (fixed-order double sums)
        w32 = weights if (weights.dtype == torch.float32 and weights.is_contiguous()) else weights.to(torch.float32).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        L.check(lib.bpx_chan_loss_finish(part.data_ptr(), N, Cc, vox, w32.data_ptr(), loss.data_ptr(), L.stream_ptr()))
        ctx.save_for_backward(z, t, w32)
        ctx.cfg = (codes, N, Cc, vox)
        return loss

    @staticmethod
    def backward(ctx, g):
        z, t, weights = ctx.saved_tensors
        codes, N, Cc, vox = ctx.cfg
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.to(torch.float32).contiguous()
        dz = torch.empty_like(z)
        L.check(lib.bpx_chan_loss_bwd_fused(z.data_ptr(), t.data_ptr(), N, Cc, vox, codes, weights.data_ptr(), g.data_ptr(), dz.data_ptr(), L.stream_ptr()))
        return dz, None, None, None


class InstanceChannelsLoss(torch.nn.Module):
    """``instance_segmentation_loss`` (biapy/engine/metrics.py:1418-1810) for plain channels - e.g. ``out_channels=["B","C","D"]``,
    ``losses_to_use=["bce","bce","mse"]`` - as one fused pass each way, taking the model's RAW logits: the head activation the
    workflow applies before the loss in training (``head_activations``, base_workflow.py:1403-1457; 'D' -> tanh,
    instance_seg.py:405-409) is part of the kernel.  Masks (``mask_values``), class re-balancing, border weights ('We'),
    multi-width channels ('R', 'A', discretised 'Db') and the separate class head stay on the reference implementation."""

    def __init__(self, channel_weights=(1, 1), out_channels=("F", "C"), losses_to_use=(), head_activations=None, channel_extra_opts=None,
                 class_rebalance_within_channels: bool = False, separated_class_channel: bool = False, ignore_index: int = -1, **_unused):
        super().__init__()
        chans = [c for c in out_channels if c not in ("We", "I")]
        if len(chans) != len(out_channels) or separated_class_channel or class_rebalance_within_channels or ignore_index != -1:
            raise NotImplementedError("InstanceChannelsLoss: border weights, class heads, re-balancing and ignore_index stay on the reference loss")
        if any(c in ("R", "A", "E_offset", "E_sigma", "E_seediness") for c in chans) or any((channel_extra_opts or {}).get(c, {}).get("mask_values") for c in chans):
            raise NotImplementedError("InstanceChannelsLoss: multi-width channels and masked channels stay on the reference loss")
        if any(c in ("Gv", "Gh", "Gz") for c in chans):
            # the reference multiplies the flow TARGET by flow_target_scale (5 for cellpose / omnipose fields, metrics.py:235-246, :1700-1705)
            raise NotImplementedError("InstanceChannelsLoss: flow channels (Gv / Gh / Gz: scaled targets) stay on the reference loss")
        if "Db" in chans and (channel_extra_opts or {}).get("Db", {}).get("val_type", "norm") == "discretize":
            # 11 prediction channels against one index channel, cross-entropy (metrics.py:1679-1688)
            raise NotImplementedError("InstanceChannelsLoss: a discretised 'Db' channel stays on the reference loss")
        if len(losses_to_use) != len(chans) or len(channel_weights) != len(chans) or len(chans) > 8:
            raise ValueError("one loss and one weight per output channel (at most 8 channels)")
        acts = list(head_activations) if head_activations is not None else ["tanh" if c == "D" else "ce_sigmoid" for c in chans]
        codes = 0
        for i, (name, a) in enumerate(zip(losses_to_use, acts)):
            if name not in _KIND or a.lower() not in _ACT:
                raise NotImplementedError(f"loss {name!r} / head activation {a!r} is not implemented on the MI355X path")
            kind = _KIND[name]
            act = _ACT[a.lower()] if kind != 0 else 0
            if kind == 0 and a.lower() not in ("ce_sigmoid", "linear"):
                raise NotImplementedError("a BCE channel takes logits (head activation ce_sigmoid)")
            codes |= (kind | (act << 2)) << (4 * i)
        self.codes = codes
        self.fused_head_activations = [a.lower() for a in acts]          # train_engine: the graph path hands this loss the raw logits
        self.register_buffer("weights", torch.tensor([float(w) for w in channel_weights], dtype=torch.float32))

    def forward(self, logits, target):
        logits = logits["pred"] if isinstance(logits, dict) else logits
        if logits.shape != target.shape or logits.shape[1] != self.weights.numel():
            raise ValueError(f"logits {tuple(logits.shape)} / target {tuple(target.shape)} do not match the {self.weights.numel()} configured channels")
        return _ChanLossFn.apply(logits, target, self.codes, self.weights.to(logits.device))


# ---------------------------------------------------------------------------------------------------------------------------
# denoising (Noise2Void): the masked MSE on the target biapy_amd.n2v.N2VMasker writes
# ---------------------------------------------------------------------------------------------------------------------------
class _N2VLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        if not pred.is_cuda or not target.is_cuda:
            raise RuntimeError("biapy_amd.losses run on the MI355X only (pred is on %s, target on %s); there is no CPU path" % (pred.device, target.device))
        z, t = pred.contiguous().to(torch.float32), target.contiguous().to(torch.float32)
        N, Cc = z.shape[:2]
        vox = z[0, 0].numel()
        nb = lib.bpx_n2v_loss_blocks(vox)
        part = torch.empty((2, N, Cc, nb), dtype=torch.float32, device=z.device)
        L.check(lib.bpx_n2v_loss_sums(z.data_ptr(), t.data_ptr(), N, Cc, vox, part.data_ptr(), L.stream_ptr()))
        out = torch.empty(2, dtype=torch.float32, device=z.device)           # [the loss, 1 / sum m]
        L.check(lib.bpx_n2v_loss_finish(part.data_ptr(), N, Cc, vox, out.data_ptr(), L.stream_ptr()))
        ctx.save_for_backward(z, t, out)
        ctx.cfg = (N, Cc, vox)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        z, t, out = ctx.saved_tensors
        N, Cc, vox = ctx.cfg
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.to(torch.float32).contiguous()
        dz = torch.empty_like(z)
        L.check(lib.bpx_n2v_loss_bwd(z.data_ptr(), t.data_ptr(), N, Cc, vox, out.data_ptr(), g.data_ptr(), dz.data_ptr(), L.stream_ptr()))
        return dz, None


class N2VLoss(torch.nn.Module):
    """The masked MSE of Noise2Void (the reference's ``n2v_loss_mse``, written from memory of it) on a LINEAR head: ``pred (B, C, ...)`` against the
    ``target (B, 2C, ...)`` of ``biapy_amd.n2v.N2VMasker``, ``v = target[:, :C]`` the original values at the masked voxels, ``m = target[:, C:]`` the
    mask; ``e = v - pred m``, ``loss = sum e^2 / sum m`` over the whole batch, ``d pred = g (-2 m e) / sum m``.  One stated difference: ``sum m = 0``
    gives loss 0 and a zero gradient where the reference gives 0 / 0.  One fused pass each way (``bpx_n2v_loss_*``): per-block fp32 partials of
    both sums in a fixed order, a one-block finish in double that also leaves ``1 / sum m`` for the backward; deterministic, no host read-back,
    capturable.  The head stays linear: the loss sets no ``fused_head_activations``."""

    def forward(self, pred, target):
        pred = pred["pred"] if isinstance(pred, dict) else pred
        if pred.dim() < 3 or target.dim() != pred.dim() or target.shape[0] != pred.shape[0] or target.shape[1] != 2 * pred.shape[1] \
                or target.shape[2:] != pred.shape[2:]:
            raise ValueError(f"pred {tuple(pred.shape)} needs a target of twice its channels (values, then masks), got {tuple(target.shape)}")
        if not 1 <= pred.shape[1] <= 8:
            raise NotImplementedError(f"N2VLoss takes 1 to 8 channels, got {pred.shape[1]}")
        return _N2VLossFn.apply(pred, target)

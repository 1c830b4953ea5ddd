"""``optimizer.step()`` of the training loop (reference: biapy/engine/train_engine.py:173-177) for ``torch.optim.Adam`` / ``AdamW`` through
``bpx_adam_step``: the same update, in the arithmetic order of torch's fused kernel, written into the optimizer's OWN state tensors
(``exp_avg``, ``exp_avg_sq``, ``step``) - ``state_dict()`` / ``load_state_dict()``, schedulers and a later plain ``optimizer.step()`` see
nothing unusual.  torch's multi-tensor launch gives one 64 K-element chunk to a block: the 6.7 M parameters of cfg 2 are ~200 blocks on 256 CUs
and three launches of 45 us; ``bpx_adam_step`` uses 4096-element blocks (two launches plus the step increment).

``fused_step(optimizer)`` returns False - and does nothing - for anything it does not reproduce exactly (another optimizer class, amsgrad,
maximize, host-side ``step`` counters, tensor-valued betas / eps / weight decay, registered step hooks, state not yet initialised, non-fp32 or
non-contiguous tensors, sparse gradients, a missing gradient) - decided for every group before the first launch, so a step is never half done:
the caller then runs ``optimizer.step()`` itself.

Two things a captured step may not hold as host constants go through ``csrc/optim.hip`` (``max_norm`` / ``beta1_d``, both off by default, in which
case nothing above changes): gradient clipping - ``bpx_grad_norm`` over ALL groups leaves ``[total_norm, coefficient]`` on the device, every group's
``bpx_adam_step_dev`` launch multiplies its gradients by that coefficient and stores the product, so ``p.grad`` afterwards is what
``clip_grad_norm_`` leaves - and a ``beta1`` that a scheduler moves every step (``OneCycleLR``, ``cycle_momentum``), read as a device double.

``torch.optim.SGD`` (the reference's ``TRAIN.OPTIMIZER = "SGD"``: momentum 0.9, Nesterov) goes through ``fused_sgd_step`` / ``bpx_sgd_step``: torch's
``_multi_tensor_sgd`` in one pass over parameter, gradient and ``momentum_buffer``, with ``lr``, the momentum (``momentum_d``: OneCycleLR cycles
``group["momentum"]`` on an SGD) and the clip coefficient read from device memory - torch's own SGD step reads a tensor ``lr`` back to the host and
cannot be captured.  It declines the first step of a fresh optimizer with momentum (no ``momentum_buffer`` yet: torch seeds it with the gradient).
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import torch
from torch.nn.utils import clip_grad_norm_

from . import _lib as L

lib = L.lib

_ENABLED = os.environ.get("BPX_FUSED_ADAM", "1") != "0"


def _group_ok(opt, g) -> bool:
    if g.get("amsgrad", False) or g.get("maximize", False) or g.get("differentiable", False):
        return False
    if not g.get("capturable", False):       # host-side step counters: torch's own path
        return False
    if any(torch.is_tensor(v) for v in (*g["betas"], g["eps"], g["weight_decay"])):
        return False
    lr = g["lr"]
    if torch.is_tensor(lr) and lr.is_cuda and (lr.dtype != torch.float32 or lr.numel() != 1):
        return False
    for p in g["params"]:
        if p.grad is None:
            return False
        st = opt.state.get(p)
        if not st or "exp_avg" not in st or "exp_avg_sq" not in st or not torch.is_tensor(st.get("step")):
            return False
        ts = (p, p.grad, st["exp_avg"], st["exp_avg_sq"])
        if any((not t.is_cuda) or t.dtype != torch.float32 or not t.is_contiguous() or t.is_sparse for t in ts):
            return False
        if st["step"].dtype != torch.float32 or not st["step"].is_cuda or st["step"].numel() != 1:
            return False
        if any(t.numel() != p.numel() for t in ts):
            return False
    return True


def _has_step_hooks(opt) -> bool:
    import torch.optim.optimizer as O

    return bool(getattr(opt, "_optimizer_step_pre_hooks", None) or getattr(opt, "_optimizer_step_post_hooks", None)
                or getattr(O, "_global_optimizer_pre_hooks", None) or getattr(O, "_global_optimizer_post_hooks", None))


def supports(optimizer) -> bool:
    """What can be told before any state exists: an Adam / AdamW without amsgrad / maximize / step hooks is what ``fused_step`` reproduces."""
    if not _ENABLED or type(optimizer) not in (torch.optim.Adam, torch.optim.AdamW) or _has_step_hooks(optimizer):
        return False
    return not any(g.get("amsgrad", False) or g.get("maximize", False) or g.get("differentiable", False) for g in optimizer.param_groups)


def supports_sgd(optimizer) -> bool:
    """What can be told before any state exists: exactly ``torch.optim.SGD`` without maximize / differentiable / step hooks and with Python-number
    momentum, dampening and weight decay is what ``fused_sgd_step`` reproduces."""
    if not _ENABLED or type(optimizer) is not torch.optim.SGD or _has_step_hooks(optimizer):
        return False
    for g in optimizer.param_groups:
        if g.get("maximize", False) or g.get("differentiable", False):
            return False
        if any(torch.is_tensor(g.get(k)) for k in ("momentum", "dampening", "weight_decay")):
            return False
    return True


def _sgd_group_ok(opt, g) -> bool:
    lr = g["lr"]
    if torch.is_tensor(lr) and lr.is_cuda and (lr.dtype != torch.float32 or lr.numel() != 1):
        return False
    if g["nesterov"] and (g["momentum"] <= 0 or g["dampening"] != 0):       # torch's constructor refuses it; a later assignment could still make it
        return False
    for p in g["params"]:
        if p.grad is None:
            return False
        ts = [p, p.grad]
        if g["momentum"] != 0:
            buf = opt.state.get(p, {}).get("momentum_buffer")
            if buf is None:                      # the first step of a fresh optimizer: torch seeds the buffer with the gradient
                return False
            ts.append(buf)
        if any((not t.is_cuda) or t.dtype != torch.float32 or t.is_sparse or not t.is_contiguous() or t.numel() != p.numel() for t in ts):
            return False
    return True


def sgd_ready(optimizer) -> bool:
    """Would ``fused_sgd_step`` take the optimizer's next step as its tensors stand now (gradients present, momentum buffers created)?"""
    return supports_sgd(optimizer) and all(_sgd_group_ok(optimizer, g) for g in optimizer.param_groups)


def _sgd_tensor_list(optimizer, ps, with_buf):
    arr = (L.AdamTensor * len(ps))()
    for i, p in enumerate(ps):
        arr[i].p, arr[i].g, arr[i].numel = p.data_ptr(), p.grad.data_ptr(), p.numel()
        if with_buf:
            arr[i].m = optimizer.state[p]["momentum_buffer"].data_ptr()
    return arr


@torch.no_grad()
def fused_sgd_step(optimizer: torch.optim.Optimizer, *, max_norm: Optional[float] = None, momentum_d: Optional[Sequence[Optional[torch.Tensor]]] = None,
                   norm_out: Optional[torch.Tensor] = None) -> bool:
    """One ``torch.optim.SGD`` step through ``bpx_sgd_step``; False (nothing done) when the optimizer or its tensors are not what the kernel
    reproduces.  ``max_norm`` / ``norm_out`` as in ``fused_step``.  ``momentum_d``: per param group a 0-d float64 device tensor the kernel reads in
    place of ``group["momentum"]``, or None for a group without momentum."""
    if not supports_sgd(optimizer):
        return False
    groups = optimizer.param_groups
    if not all(_sgd_group_ok(optimizer, g) for g in groups):     # every refusal is decided BEFORE the first launch: no partial step
        return False
    clip = max_norm is not None
    if momentum_d is not None:
        momentum_d = list(momentum_d)
        if len(momentum_d) != len(groups):
            return False
        for g, m in zip(groups, momentum_d):
            if m is None:
                continue
            if g["momentum"] == 0 or not (torch.is_tensor(m) and m.is_cuda and m.dtype == torch.float64 and m.numel() == 1):
                return False
    if clip and norm_out is not None and not (norm_out.is_cuda and norm_out.dtype == torch.float32 and norm_out.numel() == 2 and norm_out.is_contiguous()):
        return False
    st = L.stream_ptr()
    if clip:
        every = [p for g in groups for p in g["params"]]
        if not every:
            return False
        arr = _sgd_tensor_list(optimizer, every, False)
        nbytes = lib.bpx_grad_norm_workspace(len(every), arr)
        if nbytes < 0:
            raise L.BpxError("bpx_grad_norm_workspace: bad tensor list")
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=every[0].device)
        if norm_out is None:
            norm_out = torch.empty(2, dtype=torch.float32, device=every[0].device)
        L.check(lib.bpx_grad_norm(len(every), arr, float(max_norm), ws.data_ptr(), nbytes, norm_out.data_ptr(), st))
    for k, g in enumerate(groups):
        ps = list(g["params"])
        if not ps:
            continue
        mom = float(g["momentum"])
        arr = _sgd_tensor_list(optimizer, ps, mom != 0)
        lr = g["lr"]
        lr_d, lr_h = (lr.data_ptr(), 0.0) if torch.is_tensor(lr) and lr.is_cuda else (None, float(lr))
        mom_d = momentum_d[k].data_ptr() if momentum_d is not None and momentum_d[k] is not None else None
        L.check(lib.bpx_sgd_step(len(ps), arr, lr_d, lr_h, mom_d, mom, float(g["dampening"]), float(g["weight_decay"]), 1 if g["nesterov"] else 0,
                                 norm_out.data_ptr() + 4 if clip else None, st))
    optimizer._opt_called = True
    return True


def _tensor_list(optimizer, ps):
    arr = (L.AdamTensor * len(ps))()
    for i, p in enumerate(ps):
        s = optimizer.state[p]
        arr[i].p, arr[i].g, arr[i].m, arr[i].v = p.data_ptr(), p.grad.data_ptr(), s["exp_avg"].data_ptr(), s["exp_avg_sq"].data_ptr()
        arr[i].step, arr[i].numel = s["step"].data_ptr(), p.numel()
    return arr


@torch.no_grad()
def fused_step(optimizer: torch.optim.Optimizer, *, max_norm: Optional[float] = None, beta1_d: Optional[Sequence[torch.Tensor]] = None,
               norm_out: Optional[torch.Tensor] = None) -> bool:
    """One optimizer step through ``bpx_adam_step``; False (nothing done) when the optimizer is not an Adam(W) this kernel reproduces.

    ``max_norm``: ``clip_grad_norm_(all parameters, max_norm)`` first (one norm over all groups, every group's launch reads the same
    coefficient); ``norm_out`` (2 device floats, optional) receives ``[total_norm, coefficient]``.  ``beta1_d``: one 0-d float64 device tensor
    per param group, read by the kernel in place of ``group["betas"][0]``."""
    if not _ENABLED or type(optimizer) not in (torch.optim.Adam, torch.optim.AdamW):
        return False
    if _has_step_hooks(optimizer):            # hooks hang on optimizer.step(): torch's own path runs them
        return False
    groups = optimizer.param_groups
    if not all(_group_ok(optimizer, g) for g in groups):     # every refusal is decided BEFORE the first launch: no partial step
        return False
    clip = max_norm is not None
    if beta1_d is not None:
        beta1_d = list(beta1_d)
        if len(beta1_d) != len(groups) or any(not (torch.is_tensor(b) and b.is_cuda and b.dtype == torch.float64 and b.numel() == 1) for b in beta1_d):
            return False
    if clip and norm_out is not None and not (norm_out.is_cuda and norm_out.dtype == torch.float32 and norm_out.numel() == 2 and norm_out.is_contiguous()):
        return False
    st = L.stream_ptr()
    if clip:
        every = [p for g in groups for p in g["params"]]
        if not every:
            return False
        arr = _tensor_list(optimizer, every)
        nbytes = lib.bpx_grad_norm_workspace(len(every), arr)
        if nbytes < 0:
            raise L.BpxError("bpx_grad_norm_workspace: bad tensor list")
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=every[0].device)
        if norm_out is None:
            norm_out = torch.empty(2, dtype=torch.float32, device=every[0].device)
        L.check(lib.bpx_grad_norm(len(every), arr, float(max_norm), ws.data_ptr(), nbytes, norm_out.data_ptr(), st))
    for k, g in enumerate(groups):
        decoupled = 1 if isinstance(optimizer, torch.optim.AdamW) or g.get("decoupled_weight_decay", False) else 0
        ps = [p for p in g["params"]]
        if not ps:
            continue
        arr = _tensor_list(optimizer, ps)
        lr = g["lr"]
        lr_d, lr_h = (lr.data_ptr(), 0.0) if torch.is_tensor(lr) and lr.is_cuda else (None, float(lr))
        b1, b2 = g["betas"]
        if clip or beta1_d is not None:
            L.check(lib.bpx_adam_step_dev(len(ps), arr, lr_d, lr_h, None if beta1_d is None else beta1_d[k].data_ptr(), float(b1), float(b2),
                                          float(g["eps"]), float(g["weight_decay"]), decoupled, norm_out.data_ptr() + 4 if clip else None, st))
        else:
            L.check(lib.bpx_adam_step(len(ps), arr, lr_d, lr_h, float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]), decoupled, st))
    optimizer._opt_called = True             # what lr_scheduler's wrapper of optimizer.step() records (its "scheduler before optimizer" warning reads it)
    return True


def step(optimizer: torch.optim.Optimizer, *, max_norm: Optional[float] = None, beta1_d: Optional[Sequence[torch.Tensor]] = None,
         norm_out: Optional[torch.Tensor] = None, momentum_d: Optional[Sequence[Optional[torch.Tensor]]] = None) -> bool:
    """[``clip_grad_norm_(parameters, max_norm)`` ->] ``optimizer.step()``, through the HIP kernels where they apply (True); torch's own otherwise
    (False: the first step of a fresh optimizer, for one - its state does not exist yet)."""
    if fused_step(optimizer, max_norm=max_norm, beta1_d=beta1_d, norm_out=norm_out):
        return True
    if fused_sgd_step(optimizer, max_norm=max_norm, momentum_d=momentum_d, norm_out=norm_out):
        return True
    if max_norm is not None:
        total = clip_grad_norm_([p for g in optimizer.param_groups for p in g["params"]], max_norm=max_norm)
        if norm_out is not None:
            norm_out[0].copy_(total)
            norm_out[1].copy_(torch.clamp(max_norm / (total + 1e-6), max=1.0))
    optimizer.step()
    return False

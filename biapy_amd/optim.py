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


def _tensors_ok(p, ts) -> bool:
    """What every kernel of csrc/optim.hip walks: fp32, contiguous, dense CUDA tensors of the parameter's size."""
    return not any((not t.is_cuda) or t.dtype != torch.float32 or not t.is_contiguous() or t.is_sparse or t.numel() != p.numel() for t in ts)


def _lr_ok(lr) -> bool:
    """A Python number, a host tensor (read here) or ONE device float (read by the kernel)."""
    return not (torch.is_tensor(lr) and lr.is_cuda and (lr.dtype != torch.float32 or lr.numel() != 1))


def _lr_split(lr):
    """``(lr_d, lr_h)`` of the entry points: the device float's address, or None and the host value."""
    return (lr.data_ptr(), 0.0) if torch.is_tensor(lr) and lr.is_cuda else (None, float(lr))


def _is_device_double(t) -> bool:
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.numel() == 1


def _clip_ok(groups, max_norm, norm_out) -> bool:
    """``max_norm`` needs a parameter to clip and, where given, a ``norm_out`` of two contiguous device floats."""
    if max_norm is None:
        return True
    if not any(g["params"] for g in groups):
        return False
    return norm_out is None or (norm_out.is_cuda and norm_out.dtype == torch.float32 and norm_out.numel() == 2 and norm_out.is_contiguous())


def _tensor_list(optimizer, ps, **state_keys):
    """The ``bpx_adam_tensor`` list of ``ps``: p, g and numel, and each field named in ``state_keys`` from that entry of the optimizer's state."""
    arr = (L.AdamTensor * len(ps))()
    for i, p in enumerate(ps):
        arr[i].p, arr[i].g, arr[i].numel = p.data_ptr(), p.grad.data_ptr(), p.numel()
        for field, key in state_keys.items():
            setattr(arr[i], field, optimizer.state[p][key].data_ptr())
    return arr


def _clip_coefficient(optimizer, max_norm, norm_out, st) -> Optional[int]:
    """``clip_grad_norm_`` over ALL groups up to the scaling itself: ``bpx_grad_norm`` leaves ``[total_norm, coefficient]`` on the device and every
    group's update launch multiplies its gradients by that coefficient.  Returns the coefficient's device address; None without ``max_norm``."""
    if max_norm is None:
        return None
    every = [p for g in optimizer.param_groups for p in g["params"]]
    arr = _tensor_list(optimizer, every)
    nbytes = lib.bpx_grad_norm_workspace(len(every), arr)
    if nbytes < 0:
        raise L.BpxError("bpx_grad_norm_workspace: bad tensor list")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=every[0].device)
    if norm_out is None:
        norm_out = torch.empty(2, dtype=torch.float32, device=every[0].device)
    L.check(lib.bpx_grad_norm(len(every), arr, float(max_norm), ws.data_ptr(), nbytes, norm_out.data_ptr(), st))
    return norm_out.data_ptr() + 4


def _group_ok(opt, g) -> bool:
    if not g.get("capturable", False):       # host-side step counters: torch's own path
        return False
    if any(torch.is_tensor(v) for v in (*g["betas"], g["eps"], g["weight_decay"])):
        return False
    if not _lr_ok(g["lr"]):
        return False
    for p in g["params"]:
        if p.grad is None:
            return False
        st = opt.state.get(p)
        if not st or "exp_avg" not in st or "exp_avg_sq" not in st or not torch.is_tensor(st.get("step")):
            return False
        if not _tensors_ok(p, (p, p.grad, st["exp_avg"], st["exp_avg_sq"])):
            return False
        if st["step"].dtype != torch.float32 or not st["step"].is_cuda or st["step"].numel() != 1:
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
    if not _lr_ok(g["lr"]):
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
        if not _tensors_ok(p, ts):
            return False
    return True


def sgd_ready(optimizer) -> bool:
    """Would ``fused_sgd_step`` take the optimizer's next step as its tensors stand now (gradients present, momentum buffers created)?"""
    return supports_sgd(optimizer) and all(_sgd_group_ok(optimizer, g) for g in optimizer.param_groups)


@torch.no_grad()
def fused_sgd_step(optimizer: torch.optim.Optimizer, *, max_norm: Optional[float] = None, momentum_d: Optional[Sequence[Optional[torch.Tensor]]] = None,
                   norm_out: Optional[torch.Tensor] = None) -> bool:
    """One ``torch.optim.SGD`` step through ``bpx_sgd_step``; False (nothing done) when the optimizer or its tensors are not what the kernel
    reproduces.  ``max_norm`` / ``norm_out`` as in ``fused_step``.  ``momentum_d``: per param group a 0-d float64 device tensor the kernel reads in
    place of ``group["momentum"]``, or None for a group without momentum."""
    groups = optimizer.param_groups
    if not sgd_ready(optimizer) or not _clip_ok(groups, max_norm, norm_out):     # every refusal is decided BEFORE the first launch: no partial step
        return False
    momentum_d = [None] * len(groups) if momentum_d is None else list(momentum_d)
    if len(momentum_d) != len(groups) or any(m is not None and (g["momentum"] == 0 or not _is_device_double(m)) for g, m in zip(groups, momentum_d)):
        return False
    st = L.stream_ptr()
    coef = _clip_coefficient(optimizer, max_norm, norm_out, st)
    for g, m in zip(groups, momentum_d):
        ps = list(g["params"])
        if not ps:
            continue
        mom = float(g["momentum"])
        arr = _tensor_list(optimizer, ps, **(dict(m="momentum_buffer") if mom != 0 else {}))
        L.check(lib.bpx_sgd_step(len(ps), arr, *_lr_split(g["lr"]), None if m is None else m.data_ptr(), mom, float(g["dampening"]),
                                 float(g["weight_decay"]), 1 if g["nesterov"] else 0, coef, st))
    optimizer._opt_called = True             # what lr_scheduler's wrapper of optimizer.step() records (its "scheduler before optimizer" warning reads it)
    return True


@torch.no_grad()
def fused_step(optimizer: torch.optim.Optimizer, *, max_norm: Optional[float] = None, beta1_d: Optional[Sequence[torch.Tensor]] = None,
               norm_out: Optional[torch.Tensor] = None) -> bool:
    """One optimizer step through ``bpx_adam_step``; False (nothing done) when the optimizer is not an Adam(W) this kernel reproduces.

    ``max_norm``: ``clip_grad_norm_(all parameters, max_norm)`` first (one norm over all groups, every group's launch reads the same
    coefficient); ``norm_out`` (2 device floats, optional) receives ``[total_norm, coefficient]``.  ``beta1_d``: one 0-d float64 device tensor
    per param group, read by the kernel in place of ``group["betas"][0]``."""
    groups = optimizer.param_groups
    if not supports(optimizer) or not all(_group_ok(optimizer, g) for g in groups) or not _clip_ok(groups, max_norm, norm_out):
        return False                         # every refusal is decided BEFORE the first launch: no partial step
    if beta1_d is not None:
        beta1_d = list(beta1_d)
        if len(beta1_d) != len(groups) or not all(_is_device_double(b) for b in beta1_d):
            return False
    st = L.stream_ptr()
    coef = _clip_coefficient(optimizer, max_norm, norm_out, st)
    for k, g in enumerate(groups):
        ps = list(g["params"])
        if not ps:
            continue
        decoupled = 1 if isinstance(optimizer, torch.optim.AdamW) or g.get("decoupled_weight_decay", False) else 0
        arr = _tensor_list(optimizer, ps, m="exp_avg", v="exp_avg_sq", step="step")
        b1, b2 = g["betas"]
        hyper = (float(b2), float(g["eps"]), float(g["weight_decay"]), decoupled)
        if coef is not None or beta1_d is not None:
            L.check(lib.bpx_adam_step_dev(len(ps), arr, *_lr_split(g["lr"]), None if beta1_d is None else beta1_d[k].data_ptr(), float(b1), *hyper,
                                          coef, st))
        else:
            L.check(lib.bpx_adam_step(len(ps), arr, *_lr_split(g["lr"]), float(b1), *hyper, st))
    optimizer._opt_called = True             # what lr_scheduler's wrapper of optimizer.step() records (its "scheduler before optimizer" warning reads it)
    return True


def step(optimizer: torch.optim.Optimizer, *, max_norm: Optional[float] = None, beta1_d: Optional[Sequence[torch.Tensor]] = None,
         norm_out: Optional[torch.Tensor] = None, momentum_d: Optional[Sequence[Optional[torch.Tensor]]] = None) -> bool:
    """[``clip_grad_norm_(parameters, max_norm)`` ->] ``optimizer.step()``, through the HIP kernels where they apply (True); torch's own otherwise
    (False: the first step of a fresh optimizer, for one - its state does not exist yet)."""
    if type(optimizer) is torch.optim.SGD:
        fused = fused_sgd_step(optimizer, max_norm=max_norm, momentum_d=momentum_d, norm_out=norm_out)
    else:
        fused = fused_step(optimizer, max_norm=max_norm, beta1_d=beta1_d, norm_out=norm_out)
    if fused:
        return True
    if max_norm is not None:
        total = clip_grad_norm_([p for g in optimizer.param_groups for p in g["params"]], max_norm=max_norm)
        if norm_out is not None:
            norm_out[0].copy_(total)
            norm_out[1].copy_(torch.clamp(max_norm / (total + 1e-6), max=1.0))
    optimizer.step()
    return False

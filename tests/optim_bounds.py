"""fp64 statement of what ``bpx_grad_norm`` / the ``gscale_d`` product of ``bpx_adam_step_dev`` compute (torch's ``clip_grad_norm_``, norm_type 2,
error_if_nonfinite False), and the float32 yardsticks the clipping tests measure with.  Pure numpy / torch on the CPU."""
import numpy as np
import torch

# the tensor list of kernel_checks.check_fused_adam (1 ... 1.77 M elements, (4099,) = one 4096-element chunk + 3) ...
ADAM_SIZES = [(16,), (1,), (16, 1, 3, 3, 3), (256, 256, 3, 3, 3), (5, 7), (48, 16, 1, 1, 1), (4099,)]
# ... and enough 16-element tensors to cross the 64-tensor launch batch (67 tensors: two launches of the partials kernel, the second one short)
MANY_SIZES = ADAM_SIZES + [(16,)] * 60


def clip_reference(grads, max_norm):
    """(total_norm, coefficient, clipped gradients): the sum of squares in fp64, the norm rounded to float32, the coefficient
    ``min(1, float32(max_norm / (float64(norm) + 1e-6)))``, the clipped gradients as ONE float32 product per element.  A NaN gradient gives NaN
    for everything (the comparison below keeps it, as torch's clamp(max=1) does)."""
    total = 0.0
    for g in grads:
        total += float((g.detach().cpu().double() ** 2).sum())
    with np.errstate(invalid="ignore"):
        norm = np.float32(np.sqrt(np.float64(total)))
        c = np.float32(np.float64(max_norm) / (np.float64(norm) + 1e-6))
    coef = np.float32(1.0) if c > np.float32(1.0) else c
    clipped = [(g.detach().cpu().float() * float(coef)) for g in grads]
    return norm, coef, clipped


def ulps(a, b) -> int:
    """Distance of two float32 values in units in the last place (0 for two NaNs, a huge number for one)."""
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) or np.isnan(b):
        return 0 if (np.isnan(a) and np.isnan(b)) else 1 << 31

    def key(v):
        i = int(np.array(v, dtype=np.float32).view(np.int32))
        return i if i >= 0 else -(i & 0x7FFFFFFF)

    return abs(key(a) - key(b))


def make_grads(sizes, seed=0, offset=0, device="cpu"):
    """Gradients as consecutive views of ONE slab starting ``offset`` elements in (offset 3: every view but those that happen to land on a 16-byte
    boundary is unaligned), as the engine hands them to the optimizer.  Returns (views, slab)."""
    gen = torch.Generator().manual_seed(seed)
    n = sum(int(np.prod(s)) for s in sizes)
    slab = torch.zeros(n + offset + 1, dtype=torch.float32)
    slab[offset:offset + n] = torch.randn(n, generator=gen)
    slab = slab.to(device)
    views, off = [], offset
    for s in sizes:
        k = int(np.prod(s))
        views.append(slab[off:off + k].view(*s))
        off += k
    return views, slab


def onecycle_beta1(steps=10, max_lr=1e-3):
    """The beta1 values a real OneCycleLR (cycle_momentum, torch's default) assigns over ``steps`` steps, the initial one first: host doubles such
    as 0.8999999999999999 that no float32 holds."""
    p = [torch.nn.Parameter(torch.zeros(2))]
    p[0].grad = torch.zeros(2)
    opt = torch.optim.AdamW(p, lr=1e-3)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=max_lr, total_steps=steps)
    out = [opt.param_groups[0]["betas"][0]]
    for _ in range(steps - 1):
        opt.step()
        sched.step()
        out.append(opt.param_groups[0]["betas"][0])
    return out

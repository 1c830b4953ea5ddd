"""The masked MSE of Noise2Void (bpx_n2v_loss_* of csrc/n2v.hip, biapy_amd.losses.N2VLoss) in float64 - value and closed-form gradient - and the
bounds of what the device may differ by, derived from the kernels' counted operations in the manner of tests/plain_loss_bounds.py (helper of
test_n2v_cpu.py / test_n2v_gpu.py, no test itself).  Nothing here is fitted to a measured value.  u = 2^-24.

    pred (N, C, V), target (N, 2C, V): v = target[:, :C], m = target[:, C:], e = v - pred m, loss = sum e^2 / sum m, d pred = g (-2 m e) / sum m,
    both 0 when sum m = 0.

FORWARD (n2v_loss_sums_kernel): pm = fl(pred m) (u |pm|), e = fl(v - pm) (u |e| more), the term fl(e e) (2 |e| de + de^2, and u of the result).  A
thread adds ceil(V / (256 nb)) terms, nb = bpx_n2v_loss_blocks(V); six shuffle levels; three additions across the waves:
chain = ceil(V / (256 nb)) + 9 for either sum.  m enters its sum as it is.
FINISH (n2v_loss_finish_kernel): both sums over the N C nb partials in double, (N C nb + 16) 2^-53 of the absolute sum; the quotient in double,
rounded to fp32 once; 1 / sum m likewise.  A zero sum of m gives exactly 0 for both.
BACKWARD (n2v_loss_bwd_kernel): k = fl(g inv), inv carrying the error of the device's sum of m and its own rounding; pm and e as above; fl(m e); the
factor -2 is exact; the product with k rounds once.
"""
from __future__ import annotations

import torch

from conv_bounds import U32, compare

U64 = 2.0 ** -53
FLOOR = 2.0 ** -126
FAULTS = ("mask_not_applied_to_pred", "factor_two_missing", "mean_over_voxels_not_sum_m", "tail_dropped")
VOXELS = (1, 255, 256, 257, 1023, 1024, 1025, 1024 * 512 + 1)     # the last one wraps the grid-stride loop of the 512 blocks


def f32(x) -> float:
    return float(torch.tensor(float(x), dtype=torch.float32).item())


def seed_of(vox, C):
    return 7000 + 11 * (vox % 100003) + C


def fixture(gen, N, C, V, kind="sparse", scale=1.0):
    """pred = scale randn; v uniform in (-1, 1) scaled alike; the mask by kind: "sparse" (about one voxel in eight, at least one), "ones",
    "zeros", "fraction" (non-binary values in [0, 1)).  v is 0 where m is 0, as the masker writes it, except for "fraction"."""
    pred = (torch.randn(N, C, V, generator=gen) * scale).float()
    v = ((torch.rand(N, C, V, generator=gen) * 2 - 1) * scale).float()
    if kind == "sparse":
        m = (torch.rand(N, C, V, generator=gen) < 0.125).float()
        m[0, 0, V - 1] = 1.0
    elif kind == "ones":
        m = torch.ones(N, C, V)
    elif kind == "zeros":
        m = torch.zeros(N, C, V)
    else:
        m = torch.rand(N, C, V, generator=gen).float()
    if kind != "fraction":
        v = v * m
    return pred, torch.cat([v, m], 1).contiguous()


def reference(pred, target, g=1.0, fault=None):
    assert fault is None or fault in FAULTS
    N, C = pred.shape[0], pred.shape[1]
    p = pred.double().reshape(N, C, -1)
    V = p.shape[2]
    t = target.double().reshape(N, 2 * C, V)
    v, m = t[:, :C], t[:, C:]
    keep = torch.ones(V, dtype=torch.float64, device=p.device)
    if fault == "tail_dropped":
        keep[V - 1:] = 0
    e = v - (p if fault == "mask_not_applied_to_pred" else p * m)
    Se, Sm = (e * e * keep).sum(), (m * keep).sum()
    den = torch.tensor(float(N * C * V), dtype=torch.float64, device=p.device) if fault == "mean_over_voxels_not_sum_m" else Sm
    some = bool(den > 0)
    loss = Se / den if some else torch.zeros_like(Se)
    two = 1.0 if fault == "factor_two_missing" else 2.0
    grad = (g * (-two * m * e) / den) * keep if some else torch.zeros_like(e)
    return dict(N=N, C=C, V=V, p=p, v=v, m=m, e=e, Se=Se, Sm=Sm, loss=loss, grad=grad, g=float(g), some=some)


def chain(vox: int, nb: int) -> int:
    return -(-vox // (256 * nb)) + 9


def bounds(ref, nb: int):
    """Bounds of the loss (0-d) and of the gradient (N, C, V) around a reference() result without a fault; nb = bpx_n2v_loss_blocks(V).  With
    sum m = 0 both are 0: the device's values are exact zeros."""
    N, C, V, p, m, e = ref["N"], ref["C"], ref["V"], ref["p"], ref["m"], ref["e"]
    if not ref["some"]:
        return dict(loss=torch.zeros_like(ref["loss"]), grad=torch.zeros_like(ref["grad"]), exact=True)
    red = chain(V, nb) * U32 + (N * C * nb + 16) * U64
    pm = (p * m).abs()
    de = U32 * pm + U32 * e.abs()
    term = e * e
    dterm = (1 + U32) * (2 * e.abs() * de + de * de) + U32 * term + FLOOR
    Se, Sm = ref["Se"], ref["Sm"]
    dSe = dterm.sum() + red * (term + dterm).sum()
    dSm = red * m.abs().sum()
    assert bool(Sm > dSm)
    lo, hi = (Se - dSe).clamp_min(0) / (Sm + dSm), (Se + dSe) / (Sm - dSm)
    loss = ref["loss"]
    loss_b = torch.maximum(hi - loss, loss - lo) + (U32 + 4 * U64) * hi + FLOOR
    inv = 1.0 / Sm
    dinv = inv * dSm / (Sm - dSm) + (U32 + 4 * U64) * inv
    g = abs(ref["g"])
    k = g * inv
    dk = g * dinv * (1 + U32) + U32 * k
    me = (m * e).abs()
    dme = (1 + U32) * m.abs() * de + U32 * me
    y, dy = 2 * me, 2 * dme
    grad_b = (1 + U32) * (dk * y + k * dy + dk * dy) + U32 * k * y + FLOOR
    return dict(loss=loss_b, grad=grad_b, exact=False)


def _exact(name, got, ref):
    ok = bool((got.double().cpu() == 0).all()) and bool((ref.double().cpu() == 0).all())
    return dict(name=name, err=0.0 if ok else float("inf"), tol=0.0, ok=ok, extra="exact zeros expected")


def check(name, got_loss, got_grad, ref, bnd):
    """Rows in conv_bounds.compare's form; with sum m = 0 the device's loss and gradient must be exact zeros."""
    rows = []
    if bnd["exact"]:
        if got_loss is not None:
            rows.append(_exact(f"{name}.loss", got_loss.reshape(1), ref["loss"].reshape(1)))
        if got_grad is not None:
            rows.append(_exact(f"{name}.grad", got_grad.reshape(ref["grad"].shape), ref["grad"]))
        return rows
    if got_loss is not None:
        rows.append(compare(f"{name}.loss", got_loss.reshape(1), ref["loss"].reshape(1), bnd["loss"].reshape(1), axes="i"))
    if got_grad is not None:
        rows.append(compare(f"{name}.grad", got_grad.reshape(ref["grad"].shape), ref["grad"], bnd["grad"], axes="ncv"))
    return rows

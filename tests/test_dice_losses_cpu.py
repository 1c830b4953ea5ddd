"""The multi-channel Dice / Dice + CE losses without a GPU: the fp64 reference of tests/loss_bounds.py against the pinned oracle (channel mode) and
against fp64 autograd (class mode), the comparator's power against simulated faults, the host-side refusals, the C-ABI's five symbols and the
compiled kernels' scratch use."""
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import loss_bounds as LB
from oracle import loss_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ("bpx_dice_blocks", "bpx_dice_row", "bpx_dice_sums", "bpx_dice_finish", "bpx_dice_bwd")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _blocks(vox):
    from biapy_amd import _lib as L
    return L.lib.bpx_dice_blocks(vox)


# ---- the reference --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3, 8])
@pytest.mark.parametrize("batch_dice", [True, False])
def test_channel_mode_reference_is_the_pinned_oracle_dice(C, batch_dice):
    z, t = LB.channel_fixture(_gen(C), 3, C, 6 * 7 * 5)
    z5, t5 = z.reshape(3, C, 6, 7, 5), t.reshape(3, C, 6, 7, 5)
    zz = z5.double().requires_grad_(True)
    lo = LO.dice(zz, t5.double(), 1e-5, batch_dice)
    lo.backward()
    ref = LB.reference(z5, t5, w_ce=0.0, w_dice=1.0, batch_dice=batch_dice)
    assert abs(ref["loss"].item() - lo.item()) < 1e-14
    assert (ref["grad"].reshape(zz.shape) - zz.grad).abs().max().item() < 1e-16


@pytest.mark.parametrize("C", [2, 5])
def test_channel_mode_reference_is_the_pinned_oracle_dice_ce(C):
    z, t = LB.channel_fixture(_gen(10 + C), 2, C, 333)
    zz = z.double().requires_grad_(True)
    lo = LO.dice_ce(zz, t.double(), 0.7, 1.3, 1e-5)
    (2.5 * lo).backward()
    ref = LB.reference(z, t, w_ce=0.7, w_dice=1.3, g=2.5)
    # the oracle's bce casts the target to float32, which makes torch evaluate the BCE term in float32 whatever the logits' type: fp32 agreement
    assert abs(ref["loss"].item() - lo.item()) < 1e-6 * abs(lo.item())
    assert (ref["grad"] - zz.grad).abs().max().item() < 1e-6 * zz.grad.abs().max().item()
    bce64 = F.binary_cross_entropy_with_logits(z.double(), t.double())
    assert abs(ref["loss"].item() - (0.7 * bce64 + 1.3 * LO.dice(z.double(), t.double())).item()) < 1e-14


@pytest.mark.parametrize("C,batch_dice,weight,w_ce,w_dice", [(3, True, None, 1.0, 1.0), (3, False, [0.2, 0.5, 0.3], 0.5, 2.0), (8, True, [1, 2, .5, .25, 4, 1, 3, .1], 1.0, 1.0),
                                                            (5, False, None, 0.0, 1.0), (2, True, None, 1.0, 0.0)])
def test_class_mode_reference_equals_fp64_autograd(C, batch_dice, weight, w_ce, w_dice):
    z, lab = LB.class_fixture(_gen(20 + C), 3, C, 401, ignored=0.1, out_of_range=0.03, dead_sample=1 if not batch_dice else None, absent=C - 1 if C > 2 else None)
    zz = z.double().requires_grad_(True)
    la = LB.autograd_loss(zz, lab, w_ce=w_ce, w_dice=w_dice, batch_dice=batch_dice, weight=weight)
    (1.7 * la).backward()
    ref = LB.reference(z, lab, w_ce=w_ce, w_dice=w_dice, batch_dice=batch_dice, weight=weight, g=1.7)
    assert abs(ref["loss"].item() - la.item()) < 1e-13
    assert (ref["grad"] - zz.grad).abs().max().item() < 1e-15
    assert ref["sums"][LB.DR_FAULT].item() > 0 and ref["sums"][LB.DR_CNT].item() == ((lab >= 0) & (lab < C)).sum().item()


def test_all_ignored_batch():
    z, lab = LB.class_fixture(_gen(31), 2, 3, 200, all_ignored=True)
    ref = LB.reference(z, lab, w_ce=0.0, w_dice=1.0)
    assert ref["loss"].item() == 0.0 and ref["grad"].abs().max().item() == 0.0          # every dice term is s / s
    assert torch.isnan(LB.reference(z, lab, w_ce=1.0, w_dice=1.0)["loss"])


# ---- the comparator ---------------------------------------------------------------------------------------------------------------------------------
def _fp32_evaluation(z, t, class_mode, C, w_ce, w_dice, batch_dice, weight):
    """The loss and its gradient by fp32 autograd on the CPU: a correct implementation with fp32 rounding, which the bounds must admit."""
    zz = z.clone().requires_grad_(True)
    if class_mode:
        y = t[:, 0].long()
        counted = (y != -100) & (y >= 0) & (y < C)
        oh = F.one_hot(torch.where(counted, y, torch.zeros_like(y)), C).permute(0, 2, 1).float() * counted[:, None]
        p = torch.softmax(zz, 1) * counted[:, None]
        ce = F.cross_entropy(zz, torch.where(counted, y, torch.full_like(y, -100)), weight=None if weight is None else torch.tensor(weight), ignore_index=-100)
    else:
        oh, p = t, torch.sigmoid(zz)
        ce = F.binary_cross_entropy_with_logits(zz, t)
    ax = [0, 2] if batch_dice else [2]
    loss = w_ce * ce + w_dice * (1 - ((2 * (p * oh).sum(ax) + 1e-5) / (p.sum(ax) + oh.sum(ax) + 1e-5)).mean())
    loss.backward()
    return loss.detach(), zz.grad


CASES = [("class3", True, 3, True, [0.2, 0.5, 0.3]), ("class8_per_sample", True, 8, False, None), ("chan5", False, 5, True, None), ("chan2_per_sample", False, 2, False, None)]


@pytest.mark.parametrize("name,class_mode,C,batch_dice,weight", CASES)
def test_bounds_admit_a_correct_fp32_evaluation(name, class_mode, C, batch_dice, weight):
    N, V = 3, 20003
    z, t = LB.class_fixture(_gen(40 + C), N, C, V) if class_mode else LB.channel_fixture(_gen(40 + C), N, C, V)
    ref = LB.reference(z, t, w_ce=1.0, w_dice=1.0, batch_dice=batch_dice, weight=weight)
    bnd = LB.bounds(ref, _blocks(V))
    loss, grad = _fp32_evaluation(z, t, class_mode, C, 1.0, 1.0, batch_dice, weight)
    rows = LB.check(name, loss, grad, None, ref, bnd)
    assert all(r["ok"] for r in rows), rows
    assert all(r["err"] < 1.0 for r in rows)


@pytest.mark.parametrize("fault", LB.FAULTS)
def test_comparator_rejects_a_simulated_fault(fault):
    """Each fault is a plausible wrong implementation evaluated in fp64 (no rounding at all): the loss or a gradient element must leave its bound."""
    N, C, V = 3, 4, 20003
    kw = dict(w_ce=1.0, w_dice=1.0, batch_dice=True, weight=[0.2, 1.5, 0.7, 1.0])
    z, lab = LB.class_fixture(_gen(50), N, C, V, ignored=0.1, absent=3 if fault == "present_classes_only" else None,
                              dead_sample=1 if fault == "no_smooth" else None)
    if fault == "no_jacobian_sum":
        kw.update(w_ce=0.0)
    if fault == "no_smooth":          # 1e-5 beside sums of 1e4 is far below fp32 resolution: the fault shows where a sample has no counted voxel (0 / 0)
        kw.update(batch_dice=False)
    ref = LB.reference(z, lab, **kw)
    bnd = LB.bounds(ref, _blocks(V))
    bad = LB.reference(z, lab, fault=fault, **kw)
    rows = LB.check(fault, bad["loss"], bad["grad"], bad["sums"], ref, bnd)
    assert not all(r["ok"] for r in rows), rows
    if fault in ("no_jacobian_sum", "weights_on_dice", "batch_swapped", "present_classes_only", "no_smooth"):
        loss_or_grad = [r for r in rows if r["name"].endswith((".loss", ".grad"))]
        assert not all(r["ok"] for r in loss_or_grad), rows                      # caught without the help of the sums
    good = LB.check(fault, ref["loss"], ref["grad"], ref["sums"], ref, bnd)
    assert all(r["ok"] for r in good), good


def test_smooth_only_matters_where_nothing_is_counted():
    """An absent class moves the loss by s / (P + s) ~ 1e-9 with or without `smooth` (invisible in fp32); a sample without counted voxels is 0 / 0."""
    z, lab = LB.class_fixture(_gen(51), 2, 3, 5001, absent=2)
    a, b = (LB.reference(z, lab, w_ce=0.0, w_dice=1.0, batch_dice=False, fault=f)["loss"].item() for f in (None, "no_smooth"))
    assert abs(a - b) < 1e-8
    z2, lab2 = LB.class_fixture(_gen(51), 2, 3, 5001, dead_sample=1)
    assert torch.isfinite(LB.reference(z2, lab2, w_ce=0.0, w_dice=1.0, batch_dice=False)["loss"])
    assert not torch.isfinite(LB.reference(z2, lab2, w_ce=0.0, w_dice=1.0, batch_dice=False, fault="no_smooth")["loss"])


def test_fixtures_keep_their_promise():
    for C in (2, 3, 5, 8):
        z, lab = LB.class_fixture(_gen(60 + C), 3, C, 20003, ignored=0.1, out_of_range=0.02)
        share, present = LB.fixture_condition(lab, C)
        assert share >= 0.85 and present, (C, share, present)
    assert LB.chain_length(350003, 342) == -(-350003 // (256 * 342)) + 8 and LB.chain_length(262144, 256) == 4 * 1 + 8


# ---- host side --------------------------------------------------------------------------------------------------------------------------------------
def test_host_refusals():
    from biapy_amd import losses as Ls
    z3, lab = torch.zeros(2, 3, 4, 4, 4), torch.zeros(2, 1, 4, 4, 4)
    for lf in (Ls.DiceLoss(), Ls.DiceLoss(False), Ls.DiceCELoss(num_classes=3)):
        with pytest.raises(RuntimeError, match="MI355X only"):
            lf(z3, lab)
        with pytest.raises(RuntimeError, match="MI355X only"):
            lf(z3, torch.zeros_like(z3))
        with pytest.raises(NotImplementedError):
            lf(torch.zeros(2, 9, 4, 4, 4), lab)
        with pytest.raises(ValueError):
            lf(z3, torch.zeros(2, 1, 4, 4, 5))
        with pytest.raises(ValueError):
            lf(z3, torch.zeros(2, 2, 4, 4, 4))
        with pytest.raises(ValueError):
            lf(z3, torch.zeros(1, 4, 4, 4))
        with pytest.raises(NotImplementedError, match="list"):
            lf([z3, z3], lab)
    with pytest.raises(RuntimeError, match="MI355X only"):
        Ls.soft_dice_per_class(z3, lab)
    with pytest.raises(ValueError):
        Ls.DiceCELoss(num_classes=3, class_rebalance="manual", class_weights=[1.0, 2.0])({"pred": z3}, lab)
    with pytest.raises(ValueError, match="num_classes=5"):
        Ls.DiceCELoss(num_classes=5)(z3, lab)
    with pytest.raises(NotImplementedError, match="class_rebalance"):
        Ls.DiceCELoss(class_rebalance="auto")
    assert Ls.last_label_faults(Ls.DiceLoss()) == 0                    # an object that has not run yet has met none


def test_constructors_keep_their_positional_arguments():
    from biapy_amd import losses as Ls
    d = Ls.DiceLoss(False, 1e-3)
    assert (d.batch_dice, d.smooth, d.ignore_index) == (False, 1e-3, -100)
    m = Ls.DiceCELoss(0.3, 0.7, 1e-4)
    assert (m.w_ce, m.w_dice, m.smooth, m.num_classes, m.batch_dice, m.ignore_index, m.class_weights) == (0.3, 0.7, 1e-4, 2, True, -100, None)
    assert Ls.DiceCELoss(ignore_index=255).ignore_index == 255


def test_graph_step_admits_softmax_heads_with_the_dice_losses():
    """train_one_epoch(graph="on") asks _graphable_model: a drop-in with ce_softmax heads passes with the new losses as it does with the cross entropy."""
    from biapy_amd import losses as Ls
    from biapy_amd.train_engine import _graphable_model

    class M:
        _bpx_dropin = True
        head_activations = ["ce_softmax"] * 5

    for lf in (Ls.DiceLoss(), Ls.DiceCELoss(num_classes=5)):
        assert _graphable_model(M(), lf)


# ---- the C-ABI and the compiled kernels ----------------------------------------------------------------------------------------------------------------
def test_the_five_entry_points_are_declared_bound_and_exported():
    from biapy_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"^int %s\(" % sym, header, re.M), f"{sym} is not declared in include/biapy_amd.h"
        assert sym in L.EXPORTS, f"{sym} is missing from _lib's signature table"
        assert getattr(L.lib._raw, sym) is not None
    assert L.lib.bpx_dice_row() == LB.ROW
    assert L.lib.bpx_dice_blocks(1) == 1 and L.lib.bpx_dice_blocks(350003) == 342 and L.lib.bpx_dice_blocks(128 ** 3) == 512
    assert L.lib.bpx_dice_sums(None, None, 1, 3, 8, 1, -100, None, 1, None, None) != 0 and b"null pointer" in L.lib.bpx_last_error()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc to cross-compile the kernels")
def test_loss_kernels_compile_for_gfx950_without_scratch(tmp_path):
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-result", "--cuda-device-only", "-c",
           "-Rpass-analysis=kernel-resource-usage", os.path.join(ROOT, "biapy_amd", "csrc", "losses.hip"), "-o", str(tmp_path / "losses.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == 2 * 7 * 4 + 1, (len(names), len(scratch))       # sums and bwd: C 2..8 x mode x load width; finish
    assert all(v == 0 for v in scratch), [(n, v) for n, v in zip(names, scratch) if v]
    table = open(os.path.join(ROOT, "profiles", "kernel_resources.txt")).read()
    assert all(n in table for n in names), [n for n in names if n not in table]


def test_python_and_kernel_file_name_the_same_layout():
    """biapy_amd/losses.py names the columns of a row of sums and the coefficient layout once; csrc/losses.hip must say the same."""
    from biapy_amd import losses as Ls
    src = open(os.path.join(ROOT, "biapy_amd", "csrc", "losses.hip")).read()
    env = {}
    for decl in re.findall(r"^constexpr int ([^;]+);", src, re.M):
        for part in decl.split(", "):
            name, expr = part.split(" = ")
            env[name.strip()] = eval(expr, {}, env)
    for k in ("DICE_MAXC", "DICE_ROW", "DR_I", "DR_P", "DR_T", "DR_CE", "DR_W", "DR_FAULT", "DR_CNT", "DICE_COEF_HEAD", "DICE_COEF_GROUP"):
        assert env[k] == getattr(Ls, k), (k, env[k], getattr(Ls, k))

"""Batches whose whole-batch operands pass the kernels' 2^31 span, on the MI355X: the engine runs them as sample groups
(engine.batch_groups).  Bars fixed before the first run."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

CFG2 = [16, 32, 64, 128, 256]
FM32 = [32, 64, 128, 256]
P128 = (128, 128, 128)


def _data(B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, *P128, generator=g)
    tgt = (torch.rand(B, 1, *P128, generator=g) > 0.5).float()
    return x, tgt


def _step(fm, dtype, sd, x, tgt, make=None):
    """One engine train step (BCE with logits, mean): (engine, logits, loss, gradients).  make: engine factory (default: the ResUNet engine)."""
    from biapy_amd.engine import NetConfig, ResUNetEngine

    eng = make() if make is not None else ResUNetEngine(NetConfig(in_ch=1, feature_maps=fm), dtype)
    P = {k: v.cuda() for k, v in sd.items()}
    logits, ctx = eng.forward(P, x.cuda(), head_act=0, save=True)
    lg = logits.detach().clone().requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(lg, tgt.cuda())
    loss.backward()
    G = eng.backward(P, ctx, lg.grad)
    torch.cuda.synchronize()
    return eng, logits.detach(), loss.detach(), {k: v.detach().clone() for k, v in G.items()}


def test_fm32_batch8_mixed_train_step_vs_oracle():
    """feature_maps [32, 64, 128, 256], mixed mode, 8 x 128^3 (the decoder input of level 0 alone is 3.2 GB): logits, loss and every
    parameter gradient against the fp32 oracle run on the GPU, at the bars of kernel_checks."""
    import kernel_checks as KC
    from oracle import net_oracle

    sd = net_oracle.init_state_dict(1, FM32, seed=0)
    x, tgt = _data(8, 11)
    eng, logits, loss, G = _step(FM32, torch.float16, sd, x, tgt)
    assert eng.last_groups == [(0, 4), (4, 8)]
    with torch.backends.cudnn.flags(enabled=False):
        loss_ref, lo_ref, grads_ref = net_oracle.train_step_grads({k: v.cuda() for k, v in sd.items()}, x.cuda(), tgt.cuda(), feature_maps=FM32)
    lo_ref = lo_ref.cpu()
    grads_ref = {k: v.cpu() for k, v in grads_ref.items()}
    tag = "large_batch[f16 fm32 8x128^3]"
    rows = [KC._res(tag + ".logits_rel", (logits.cpu() - lo_ref).abs().max().item() / lo_ref.abs().max().item(), KC.LOGITS_TOL["f16"]),
            KC._res(tag + ".loss", abs(loss.item() - loss_ref.item()), KC.LOSS_TOL["f16"])]
    rows += KC.parity_rows(tag, logits.cpu(), lo_ref, tgt, torch.float16)
    rows += KC.grad_rows(tag, G, grads_ref, "f16", len(FM32) - 1)
    bad = [r for r in rows if not r["ok"]]
    assert not bad, bad


def _halves_match(fm, dtype, B, gtol, sd=None, make=None, grouped=True, scale_of="tensor"):
    from oracle import net_oracle

    sd = sd if sd is not None else net_oracle.init_state_dict(1, fm, seed=3)
    x, tgt = _data(B, 5)
    h = B // 2
    e_all, lo_all, _, G_all = _step(fm, dtype, sd, x, tgt, make)
    e_a, lo_a, _, G_a = _step(fm, dtype, sd, x[:h], tgt[:h], make)
    e_b, lo_b, _, G_b = _step(fm, dtype, sd, x[h:], tgt[h:], make)
    if grouped:       # the same launches: the whole batch runs as groups of the half batch's own plan
        assert e_all.last_groups == [(0, h), (h, B)] and e_a.last_groups == [(0, h)], (e_all.last_groups, e_a.last_groups)
    else:             # under the span: one launch sequence, as before this change
        assert e_all.last_groups == [(0, B)]
    assert torch.equal(lo_all[:h], lo_a) and torch.equal(lo_all[h:], lo_b), "per-sample logits are not bit-identical"
    worst, name = 0.0, ""
    net_max = max(g.abs().max().item() for g in G_all.values())
    for k, g in G_all.items():
        scale = g.abs().max().item() if scale_of == "tensor" else net_max
        if scale == 0.0:
            continue
        e = (g - 0.5 * (G_a[k] + G_b[k])).abs().max().item() / scale
        if e > worst:
            worst, name = e, k
    assert worst <= gtol, (worst, name)


def test_fm32_batch8_mixed_equals_two_batches_of_4():
    _halves_match(FM32, torch.float16, 8, 1e-4)


def test_cfg2_batch12_mixed_equals_two_batches_of_6():
    _halves_match(CFG2, torch.float16, 12, 1e-4)


def test_unet_fm32_batch8_mixed_equals_two_batches_of_4():
    """The U-Net engine's grouped forward and backward (its decoder input is [up (32) | skip (32)]: 2^31 bytes at batch 8)."""
    from biapy_amd.unet import U_Net
    from biapy_amd.unet_engine import UNetEngine

    torch.manual_seed(0)
    m = U_Net(image_shape=P128 + (1,), activation="elu", feature_maps=FM32, drop_values=[0.0] * 4, normalization="in", yx_down=[2] * 3,
              z_down=[2] * 3, isotropy=[True] * 4, larger_io=False, conv_layers=[2] * 4)
    sd = {n: p.detach().clone() for n, p in m.named_parameters()}
    _halves_match(FM32, torch.float16, 8, 1e-4, sd=sd, make=lambda: UNetEngine(m.cfg, 3, torch.float16))


def _release():
    """Drop a test's captured graphs now, not in some later test's capture."""
    import gc

    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _resunet_fm32():
    from oracle import net_oracle

    from biapy_amd.resunet import ResUNet

    m = ResUNet(image_shape=P128 + (1,), activation="elu", feature_maps=FM32, drop_values=[0.0] * 4, normalization="in", yx_down=[2] * 3,
                z_down=[2] * 3, isotropy=[True] * 4, larger_io=False, conv_layers=[2] * 4, compute_dtype=torch.float16)
    m.load_state_dict(net_oracle.init_state_dict(1, FM32, seed=0), strict=True)
    return m.cuda().train()


def test_graphed_train_step_at_batch8_replays_the_eager_step_bit_for_bit():
    """GraphedTrainStep with test 1's model and batch: the captured step runs the two sample groups; one replay and one eager step from the
    same weights give the same logits, loss and parameter gradients, bit for bit."""
    from biapy_amd.graphs import GraphedTrainStep

    m = _resunet_fm32()
    x, t = (v.cuda() for v in _data(8, 11))
    params = list(m.parameters())
    snap = [p.detach().clone() for p in params]

    def restore():
        with torch.no_grad():
            for p, s_ in zip(params, snap):
                p.copy_(s_)

    opt = torch.optim.AdamW(params, lr=1e-3, capturable=True)
    gs = GraphedTrainStep(m, F.binary_cross_entropy_with_logits, opt, x, t, warmup=1)
    assert m.engine().last_groups == [(0, 4), (4, 8)]
    restore()
    loss_r = gs().clone()
    torch.cuda.synchronize()
    out_r = gs.outputs.clone()
    grads_r = [p.grad.detach().clone() for p in params]
    restore()
    opt.zero_grad(set_to_none=True)
    out_e = m(gs.x)
    loss_e = F.binary_cross_entropy_with_logits(out_e, gs.target)
    loss_e.backward()
    torch.cuda.synchronize()
    assert torch.equal(out_e.detach(), out_r)
    assert torch.equal(loss_e.detach(), loss_r), (loss_e.item(), loss_r.item())
    bad = [n for (n, p), g in zip(m.named_parameters(), grads_r) if not torch.equal(p.grad, g)]
    del gs, opt, m, params
    _release()
    assert not bad, bad[:5]


def test_data_parallel_graph_step_at_batch8_equals_its_eager_form():
    """DataParallelTrainStep(graph=True) at a grouped shape: its overlapped capture splits the backward at on_last_block, which the grouped
    backward calls once, after the last group; the replayed gradient slab equals the eager form's bit for bit."""
    from biapy_amd.graphs import DataParallelTrainStep
    from biapy_amd.losses import BCEWithLogitsLoss

    m = _resunet_fm32()
    x, t = (v.cuda() for v in _data(8, 11))
    params = list(m.parameters())
    snap = [p.detach().clone() for p in params]

    def restore():
        with torch.no_grad():
            for p, s_ in zip(params, snap):
                p.copy_(s_)

    opt = torch.optim.AdamW(params, lr=1e-3, capturable=True)
    step = DataParallelTrainStep(m, BCEWithLogitsLoss(), opt, x, t, graph=True, warmup=1)
    assert step.overlapped
    assert m.engine().last_groups == [(0, 4), (4, 8)]
    restore()
    step(x, t)
    torch.cuda.synchronize()
    g_graph = step.flat_grad.clone()
    restore()
    eager = DataParallelTrainStep(m, BCEWithLogitsLoss(), opt, x, t, graph=False)
    eager(x, t)
    torch.cuda.synchronize()
    same = torch.equal(eager.flat_grad, g_graph)
    del step, eager, opt, m, params
    _release()
    assert same


@pytest.mark.parametrize("fm", [CFG2, FM32], ids=["fm16", "fm32"])
def test_sliding_window_batch16_matches_batch4(fm):
    """SlidingWindowPredictor with cfg 3's patch (128^3, 50 % overlap, fp16 inference) on a 256^3 volume (27 patches): batch size 16 merges
    the same bits as batch size 4."""
    from oracle import net_oracle

    from biapy_amd.resunet import ResUNet
    from biapy_amd.workflow import SlidingWindowPredictor

    n = len(fm)
    m = ResUNet(image_shape=P128 + (1,), activation="elu", feature_maps=fm, drop_values=[0.0] * n, normalization="in", yx_down=[2] * (n - 1),
                z_down=[2] * (n - 1), isotropy=[True] * n, larger_io=False, conv_layers=[2] * n, compute_dtype=torch.bfloat16)
    m.load_state_dict(net_oracle.init_state_dict(1, fm, seed=9), strict=True)
    m = m.cuda().eval()
    vol = torch.randn(256, 256, 256, 1, generator=torch.Generator().manual_seed(4)).cuda()
    out = {}
    for bs in (4, 16):
        sw = SlidingWindowPredictor(m, P128, (0.5, 0.5, 0.5), (0, 0, 0), batch_size=bs, compute_dtype=torch.float16)
        out[bs] = sw.predict(vol).clone()
        torch.cuda.synchronize()
    assert torch.isfinite(out[4]).all()
    assert torch.equal(out[4], out[16])


# fp32 last: the fp32 bound counts elements (its kernels address with 64-bit pointers), so batch 8 at fm = 32 runs as one launch sequence
# (6.4 GB operands, as before this change) and batch 12 as two groups of 6
def test_fm32_f32_batch8_equals_two_batches_of_4_in_one_group():
    # one launch sequence for 8 samples and one for 4 lay out the weight-gradient partial sums differently, so the biases in front of an
    # InstanceNorm (true gradient exactly zero) hold different rounding noise: gradients are compared at the network's largest gradient here
    _halves_match(FM32, torch.float32, 8, 1e-5, grouped=False, scale_of="network")


def test_fm32_f32_batch12_equals_two_batches_of_6():
    _halves_match(FM32, torch.float32, 12, 1e-5)

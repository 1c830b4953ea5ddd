"""Output heads of 5..8 channels on the device: the head kernels' entry points against fp64, the networks that feed a multi-class loss
against the oracle graphs, the mixed training mode's loss curve, graph replay and the sliding-window arg-max."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
CURVE_TOL = 1e-2          # the cfg-4 loss-curve bar


def _record_diag(line):
    """Measured values, recorded beside those of the other parity tests by their own recorder (test_gpu_parity._record_diag).  Recording is a
    record, not a check: without the recorder the line is only printed."""
    print(line)
    try:
        from test_gpu_parity import _record_diag as record
    except ImportError:
        return
    record(line)


def _relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _acts64(z, code, cout):
    """apply_model_activations in fp64 on (N, C, V) logits: 4-bit codes, consecutive softmax channels are one group."""
    codes = [(code >> (4 * c)) & 15 for c in range(cout)]
    out = z.clone()
    c = 0
    while c < cout:
        if codes[c] == 1:
            out[:, c] = torch.sigmoid(z[:, c])
        elif codes[c] == 2:
            out[:, c] = torch.tanh(z[:, c])
        elif codes[c] == 3:
            e = c
            while e + 1 < cout and codes[e + 1] == 3:
                e += 1
            out[:, c:e + 1] = torch.softmax(z[:, c:e + 1], dim=1)
            c = e
        c += 1
    return out


# 8 softmax channels; [sigmoid, sigmoid, tanh, softmax x 5]; two softmax groups split by a linear channel (low nibble = channel 0)
CODES = (0x33333333, 0x33333211, 0x33330333)


@pytest.mark.parametrize("cin", [16, 32])
@pytest.mark.parametrize("cout", [5, 6, 7, 8])
@pytest.mark.parametrize("fdt,bdt", [("F32", "F32"), ("BF16", "BF16"), ("F16", "MIX16")])
def test_head_entry_points_five_to_eight_channels(cout, cin, fdt, bdt):
    """bpx_head_fwd / bpx_head_bwd at Cout 5..8 against fp64 F.conv3d / autograd on the dtype-rounded inputs: N = 3 samples of a ragged voxel count
    (3 x 350003 > 4096 x 256 threads of the forward and 1024 x 256 of the backward: both grid-stride loops wrap), padded x / dx rows, padded output
    strides (the padding of dout holds NaN: a read of it would show), two backward runs bit-identical."""
    from biapy_amd import _lib as L

    lib = L.lib
    fd, bd = getattr(L, fdt), getattr(L, bdt)
    xt = {"F32": torch.float32, "BF16": torch.bfloat16, "F16": torch.float16}[fdt]
    dxt = {"F32": torch.float32, "BF16": torch.bfloat16, "MIX16": torch.bfloat16}[bdt]
    N, vps, ld = 3, 350003, cin + 8
    sc = vps + 5
    sn = cout * sc + 11
    g = torch.Generator().manual_seed(1000 * cout + cin)
    xs = torch.randn(N * vps, ld, generator=g).to(xt)
    x64 = xs[:, :cin].double()
    w = torch.randn(cout, cin, generator=g) * 0.3
    b = torch.randn(cout, generator=g) * 0.1
    x_d, w_d, b_d = xs.to(DEV), w.to(DEV), b.to(DEV)
    z64 = (x64 @ w.double().t() + b.double()).view(N, vps, cout).permute(0, 2, 1)          # (N, C, V)
    out = torch.full((N * sn,), float("nan"), dtype=torch.float32, device=DEV)
    for code in (0,) + CODES:
        code &= (1 << (4 * cout)) - 1
        L.check(lib.bpx_head_fwd(fd, vps, N, L.tview(x_d, 0, cin), w_d.data_ptr(), b_d.data_ptr(), cout, code, out.data_ptr(), sn, sc, L.stream_ptr()))
        torch.cuda.synchronize()
        got = out.as_strided((N, cout, vps), (sn, sc, 1))
        err = _relerr(got, _acts64(z64, code, cout))
        assert err < 1e-5, (hex(code), err)
    # backward
    dout = torch.randn(N, cout, vps, generator=g)
    dbuf = torch.full((N * sn,), float("nan"), dtype=torch.float32)
    dbuf.as_strided((N, cout, vps), (sn, sc, 1)).copy_(dout)
    dbuf = dbuf.to(DEV)
    d64 = dout.double().permute(0, 2, 1).reshape(N * vps, cout)
    dx_ref, dw_ref, db_ref = d64 @ w.double(), d64.t() @ x64, d64.sum(0)
    ws = torch.empty(lib.bpx_head_bwd_workspace(cin, cout), dtype=torch.uint8, device=DEV)
    runs = []
    for _ in range(2):
        dx = torch.full((N * vps, ld), 7.0, dtype=dxt, device=DEV)
        dw = torch.full((cout, cin), 5.0, dtype=torch.float32, device=DEV)        # overwritten
        db = torch.zeros(cout, dtype=torch.float32, device=DEV)                   # accumulated: the caller zeroes it
        L.check(lib.bpx_head_bwd(bd, vps, N, L.tview(x_d, 0, cin), w_d.data_ptr(), cout, dbuf.data_ptr(), sn, sc, L.tview(dx, 0, cin), dw.data_ptr(),
                                 db.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr()))
        torch.cuda.synchronize()
        runs.append((dx.cpu(), dw.cpu(), db.cpu()))
    dx, dw, db = runs[0]
    assert bool((dx[:, cin:] == 7.0).all()), "dx written outside its channels"
    assert _relerr(dx[:, :cin], dx_ref) < (2e-5 if bdt == "F32" else 1.5e-2)      # tests/kernel_checks.py tol_for (bf16 dx in both 16-bit modes)
    assert _relerr(dw, dw_ref) < 1e-4
    assert _relerr(db, db_ref) < 1e-4
    for a, b_ in zip(runs[0], runs[1]):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                           b_.view(torch.int16) if b_.dtype == torch.bfloat16 else b_.view(torch.int32))


# ---- networks in f32 against the oracle graphs ----------------------------------------------------------------------------------------------------
def _small(fm, S=16, **kw):
    d = len(fm)
    base = dict(image_shape=(S, S, S, 1), activation="elu", feature_maps=fm, drop_values=[0.0] * d, normalization="in", yx_down=[2] * (d - 1),
                z_down=[2] * (d - 1), isotropy=[True] * d, larger_io=False, conv_layers=[2] * d, compute_dtype=torch.float32)
    base.update(kw)
    return base


def _labels(g, B, n, S):
    return torch.randint(0, n, (B, 1) + S, generator=g).float()


def _check_grads(m, P, tag, full_tol=2e-3, norm_min=0.0):
    """Every gradient norm (of the parameters whose gradient norm exceeds norm_min of the largest) within 2e-3 relative, every full gradient
    within full_tol; floor of both: 1e-3 of the largest norm."""
    refs = {k: v.grad for k, v in P.items() if v.grad is not None}
    gmax = max(v.norm().item() for v in refs.values())
    named = dict(m.named_parameters())
    worst_n = worst_f = 0.0
    for k, ref in refs.items():
        got = named[k].grad.detach().cpu()
        den = max(ref.norm().item(), 1e-3 * gmax)
        en, ef = abs(got.norm().item() - ref.norm().item()) / den, (got - ref).norm().item() / den
        if ref.norm().item() <= norm_min * gmax:
            en = 0.0
        worst_n, worst_f = max(worst_n, en), max(worst_f, ef)
        assert en <= 2e-3 and ef <= full_tol, (k, en, ef)
    _record_diag(f"class_heads[{tag}].grads worst_rel norm = {worst_n:.3e} (bar 2e-3), full = {worst_f:.3e} (bar {full_tol:g})")


def _oracle_params(m):
    return {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("fm", [[16, 32, 64], [48, 64]], ids=["fm16", "wide-head-fm48"])
def test_eight_class_resunet_with_cross_entropy_matches_oracle(fm):
    """ResUNet(output_channels=[8], ce_softmax) + CrossEntropyLoss_wrapper(num_classes=8): logits, loss and every gradient against the oracle
    graph; fm48 = the GEMM-fed wide head (first level other than 16 / 32) at 8 channels."""
    from biapy_amd.losses import CrossEntropyLoss_wrapper
    from biapy_amd.resunet import ResUNet
    from oracle import net_oracle

    torch.manual_seed(3)
    m = ResUNet(**_small(fm, output_channels=[8], head_activations=["ce_softmax"])).to(DEV).train()
    P = _oracle_params(m)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 1, 16, 16, 16, generator=g)
    t = _labels(g, 2, 8, (16, 16, 16))
    lo_ref = net_oracle.resunet_forward(P, x, fm)
    loss_ref = F.cross_entropy(lo_ref, t[:, 0].long())
    loss_ref.backward()
    lf = CrossEntropyLoss_wrapper(num_classes=8, ndim=3)
    lo = m(x.to(DEV))
    loss = lf(lo, t.to(DEV))
    loss.backward()
    assert lo.shape == (2, 8, 16, 16, 16)
    assert (lo.detach().cpu() - lo_ref.detach()).abs().max().item() < 5e-5
    assert abs(loss.item() - loss_ref.item()) < 2e-5
    _check_grads(m, P, f"resunet 8-class fm{fm[0]}")
    with torch.no_grad():
        pr = m.eval().predict_proba(x.to(DEV)).cpu()
    assert (pr - torch.softmax(lo_ref.detach(), 1)).abs().max().item() < 2e-5


def test_instance_channels_with_a_five_class_head_match_oracle():
    """output_channels [3, 5] with output_channel_info ["BCD", "class"]: out["pred"] / out["class"], a loss over both, every gradient; then the
    return_one_tensor form (pred + arg-max class)."""
    from biapy_amd.resunet import ResUNet
    from oracle import net_oracle

    fm = [16, 32, 64]
    kw = _small(fm, output_channels=[3, 5], output_channel_info=["BCD", "class"], head_activations=["ce_sigmoid", "ce_sigmoid", "tanh", "ce_softmax"])
    torch.manual_seed(5)
    m = ResUNet(**kw).to(DEV).train()
    P = _oracle_params(m)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 1, 16, 16, 16, generator=g)
    tgt = (torch.rand(2, 3, 16, 16, 16, generator=g) > 0.5).float()
    cls_t = _labels(g, 2, 5, (16, 16, 16))[:, 0].long()
    lo_ref = net_oracle.resunet_forward(P, x, fm, n_heads=2)
    loss_ref = F.binary_cross_entropy_with_logits(lo_ref[:, :3], tgt) + F.cross_entropy(lo_ref[:, 3:], cls_t)
    loss_ref.backward()
    o = m(x.to(DEV))
    assert isinstance(o, dict) and set(o) == {"pred", "class"} and o["class"].shape[1] == 5
    assert (o["pred"].detach().cpu() - lo_ref[:, :3].detach()).abs().max().item() < 5e-5
    assert (o["class"].detach().cpu() - lo_ref[:, 3:].detach()).abs().max().item() < 5e-5
    loss = F.binary_cross_entropy_with_logits(o["pred"], tgt.to(DEV)) + F.cross_entropy(o["class"], cls_t.to(DEV))
    loss.backward()
    assert abs(loss.item() - loss_ref.item()) < 2e-5
    _check_grads(m, P, "resunet [3, 5] BCD + class")
    m1 = ResUNet(return_one_tensor=True, **kw).to(DEV).eval()
    m1.load_state_dict(m.state_dict())
    with torch.no_grad():
        one = m1(x.to(DEV)).cpu()
    assert one.shape == (2, 4, 16, 16, 16) and (one[:, :3] - lo_ref[:, :3].detach()).abs().max().item() < 5e-5
    assert (one[:, 3] != lo_ref[:, 3:].detach().argmax(1)).float().mean().item() < 1e-3      # ties at fp32 rounding aside


def test_eight_class_unet_matches_oracle():
    from biapy_amd.losses import CrossEntropyLoss_wrapper
    from biapy_amd.unet import U_Net
    from oracle import unet_oracle

    fm = [16, 32, 64]
    torch.manual_seed(7)
    m = U_Net(**_small(fm, output_channels=[8])).to(DEV).train()
    P = _oracle_params(m)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 1, 16, 16, 16, generator=g)
    t = _labels(g, 2, 8, (16, 16, 16))
    lo_ref = unet_oracle.unet_forward(P, x, fm)
    loss_ref = F.cross_entropy(lo_ref, t[:, 0].long())
    loss_ref.backward()
    lo = m(x.to(DEV))
    loss = CrossEntropyLoss_wrapper(num_classes=8, ndim=3)(lo, t.to(DEV))
    loss.backward()
    assert (lo.detach().cpu() - lo_ref.detach()).abs().max().item() < 5e-5
    assert abs(loss.item() - loss_ref.item()) < 2e-5
    _check_grads(m, P, "unet 8-class")


def test_eight_class_resunetpp_matches_oracle():
    """ResUNet++'s own f32 bars (tests/kernel_checks.py check_resunetpp_cfg4_shape: its squeeze-excite products and attention gates amplify fp32
    rounding - 3e-3 measured at the first conv and at an attention-gate bias here): full gradients within 2e-2, the norms within 2e-3 for the
    parameters that carry more than 5 % of the largest gradient norm."""
    from biapy_amd.losses import CrossEntropyLoss_wrapper
    from biapy_amd.resunetpp import ResUNetPlusPlus
    from oracle import resunetpp_oracle

    fm = [16, 32, 64]
    torch.manual_seed(9)
    m = ResUNetPlusPlus(image_shape=(16, 32, 32, 1), activation="elu", feature_maps=fm, drop_values=[0.0] * 3, normalization="in", yx_down=[2, 2],
                        z_down=[2, 2], output_channels=[8], output_channel_info=["F"], head_activations=["ce_softmax"], isotropy=[True] * 3,
                        larger_io=False, conv_layers=[2] * 3, compute_dtype=torch.float32).to(DEV).train()
    P = _oracle_params(m)
    g = torch.Generator().manual_seed(10)
    x = torch.randn(2, 1, 16, 32, 32, generator=g)
    t = _labels(g, 2, 8, (16, 32, 32))
    lo_ref = resunetpp_oracle.resunetpp_forward(P, x, fm)
    loss_ref = F.cross_entropy(lo_ref, t[:, 0].long())
    loss_ref.backward()
    lo = m(x.to(DEV))
    loss = CrossEntropyLoss_wrapper(num_classes=8, ndim=3)(lo, t.to(DEV))
    loss.backward()
    assert (lo.detach().cpu() - lo_ref.detach()).abs().max().item() < 5e-5
    assert abs(loss.item() - loss_ref.item()) < 2e-5
    _check_grads(m, P, "resunet++ 8-class", full_tol=2e-2, norm_min=0.05)


# ---- training ---------------------------------------------------------------------------------------------------------------------------------------
def _blob_batches(g, n, B, S, classes):
    out = []
    for _ in range(n):
        field = F.avg_pool3d(torch.randn(B, classes, S, S, S, generator=g), 7, stride=1, padding=3)
        lab = field.argmax(1, keepdim=True)
        x = lab.float() / (classes - 1) * 2 - 1 + 0.5 * torch.randn(B, 1, S, S, S, generator=g)
        out.append((x, lab.float()))
    return out


def test_eight_class_mixed_training_follows_the_fp32_oracle_loss_curve():
    """The default training mode (fp16 forward, bf16 gradients) of the 8-class ResUNet at 2 x 32^3: 20 AdamW steps on the device and as the fp32
    oracle graph from the same weights on the same batches; the loss curves agree step by step."""
    from biapy_amd.losses import CrossEntropyLoss_wrapper
    from biapy_amd.resunet import ResUNet
    from oracle import net_oracle

    fm, S, steps = [16, 32, 64], 32, 20
    torch.manual_seed(11)
    m = ResUNet(**_small(fm, S=S, output_channels=[8], head_activations=["ce_softmax"], compute_dtype=torch.float16)).to(DEV).train()
    cpu_p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.named_parameters()}
    batches = _blob_batches(torch.Generator().manual_seed(12), 3, 2, S, 8)
    lf = CrossEntropyLoss_wrapper(num_classes=8, ndim=3)
    opt_d = torch.optim.AdamW(m.parameters(), lr=1e-3)
    opt_c = torch.optim.AdamW(list(cpu_p.values()), lr=1e-3)
    old = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, old)))
    try:
        cd, cc = [], []
        for it in range(steps):
            x, t = batches[it % len(batches)]
            opt_d.zero_grad(set_to_none=True)
            ld = lf(m(x.to(DEV)), t.to(DEV))
            ld.backward()
            opt_d.step()
            opt_c.zero_grad(set_to_none=True)
            lc = F.cross_entropy(net_oracle.resunet_forward(cpu_p, x, fm), t[:, 0].long())
            lc.backward()
            opt_c.step()
            cd.append(ld.item())
            cc.append(lc.item())
    finally:
        torch.set_num_threads(old)
    cd_, cc_ = torch.tensor(cd), torch.tensor(cc)
    rel = ((cd_ - cc_).abs() / cc_).max().item()
    print("mixed-mode 8-class loss curve (device):", [round(v, 4) for v in cd])
    print("fp32 oracle loss curve          (cpu):", [round(v, 4) for v in cc])
    _record_diag(f"loss_curve[8-class ResUNet mixed vs fp32 oracle, fm 16-32-64, 2x{S}^3, {steps} steps].worst_rel_gap = {rel:.3e} (bar {CURVE_TOL:g})")
    assert cc_[-3:].mean() < cc_[:3].mean() and cd_[-3:].mean() < cd_[:3].mean(), (cc, cd)
    assert rel < CURVE_TOL, (rel, cc, cd)


def test_eight_class_graphed_train_step_equals_the_eager_step():
    """GraphedTrainStep with CrossEntropyLoss_wrapper(num_classes=8): a replayed step gives the eager step's loss and gradients bit for bit
    (lr = 0: both models keep the same weights)."""
    from biapy_amd.graphs import GraphedTrainStep
    from biapy_amd.losses import CrossEntropyLoss_wrapper
    from biapy_amd.resunet import ResUNet

    torch.manual_seed(13)
    m1 = ResUNet(**_small([16, 32, 64], S=32, output_channels=[8], head_activations=["ce_softmax"])).to(DEV).train()
    m2 = copy.deepcopy(m1)
    g = torch.Generator().manual_seed(14)
    x = torch.randn(2, 1, 32, 32, 32, generator=g).to(DEV)
    t = _labels(g, 2, 8, (32, 32, 32)).to(DEV)
    lf = CrossEntropyLoss_wrapper(num_classes=8, ndim=3)
    o1 = torch.optim.AdamW(m1.parameters(), lr=0.0, capturable=True)
    o2 = torch.optim.AdamW(m2.parameters(), lr=0.0, capturable=True)
    gs = GraphedTrainStep(m2, lf, o2, x, t, warmup=2)
    l2 = gs().clone()
    torch.cuda.synchronize()
    o1.zero_grad(set_to_none=True)
    l1 = lf(m1(x), t)
    l1.backward()
    torch.cuda.synchronize()
    assert torch.equal(l1.detach().view(1), l2.view(1)), (l1.item(), l2.item())
    n = 0
    for (k, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        assert p2.grad is not None and torch.equal(p1.grad, p2.grad), k
        n += 1
    assert n == len(list(m1.parameters()))


# ---- sliding window ---------------------------------------------------------------------------------------------------------------------------------
def test_eight_class_sliding_window_and_class_argmax():
    """An 8-class net on a 96^3 volume through SlidingWindowPredictor.process_test_sample: the blended probabilities equal the oracle's crop / merge
    of the same per-patch predictions; with class_channels=8 the result is the arg-max of those probabilities (fp32 ties aside)."""
    from biapy_amd.resunet import ResUNet
    from biapy_amd.workflow import SlidingWindowPredictor
    from oracle import tiling_oracle

    torch.manual_seed(15)
    m = ResUNet(**_small([16, 32, 64], S=32, output_channels=[8], head_activations=["ce_softmax"])).to(DEV).eval()
    vol = np.random.RandomState(16).rand(96, 96, 96, 1).astype(np.float32)
    patch, ov = (32, 32, 32), (0.5, 0.5, 0.5)
    sw = SlidingWindowPredictor(m, patch, ov, (0, 0, 0), batch_size=4)
    vd = torch.from_numpy(vol).to(DEV)
    probs = sw.process_test_sample(vd).cpu().numpy()
    labels = sw.process_test_sample(vd, class_channels=8).cpu().numpy()
    pr, _ = tiling_oracle.crop(vol, patch + (1,), ov)
    with torch.no_grad():
        outs = [m.predict_proba(torch.from_numpy(pr[i:i + 4]).permute(0, 4, 1, 2, 3).contiguous().to(DEV)).permute(0, 2, 3, 4, 1).cpu().numpy()
                for i in range(0, len(pr), 4)]
    ref = tiling_oracle.merge(np.concatenate(outs, 0), (96, 96, 96, 8), overlap=ov)
    assert probs.shape == (96, 96, 96, 8) and labels.shape == (96, 96, 96, 1)
    assert np.abs(probs - ref).max() < 1e-5
    s = np.sort(ref, axis=-1)
    want = ref.argmax(-1)
    diff = labels[..., 0] != want
    assert np.all(s[..., -1][diff] - s[..., -2][diff] < 1e-5), "arg-max differs away from a tie"
    assert diff.mean() < 1e-4 and len(np.unique(want)) > 1

"""Checks of networks whose image has 2 to 15 channels (NetConfig.true_in_ch: the image and the first block's input weights run zero-padded to
16 channels; bpx_image_pack16 writes the padded tensor).  The host helpers at the top need no GPU (tests/test_multichannel_cpu.py); every
``check_*`` returns result rows ``{name, err, tol, ok}`` as tests/kernel_checks.py does, with that file's bars."""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

from biapy_amd.engine import NetConfig, bn_layers, pad_input_channels
from oracle import net_oracle

DEV = "cuda"


# ---- host helpers ------------------------------------------------------------------------------------------------------------------------
def module_kwargs(fm, zd=None):
    """Constructor arguments of the drop-in modules for a plain configuration of widths ``fm``."""
    n = len(fm)
    return dict(activation="elu", feature_maps=list(fm), drop_values=[0.0] * n, normalization="in", yx_down=[2] * (n - 1),
                z_down=list(zd) if zd is not None else [2] * (n - 1), isotropy=[True] * n, larger_io=False, conv_layers=[2] * n)


def state_dict_2d(sd):
    """The 2-D network's state dict of a 3-D one built with z_down = 1: the centre z-tap of every kernel (3 -> tap 1, 1 -> tap 0)."""
    return {k: (v[:, :, v.shape[2] // 2].contiguous() if v.dim() == 5 else v) for k, v in sd.items()}


def perturbed_state_dict(C, fm, seed, zd=None):
    """net_oracle.init_state_dict with every vector (norm affine parameters, biases) moved off its initial value."""
    sd = net_oracle.init_state_dict(C, list(fm), z_down=zd, seed=seed)
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        for v in sd.values():
            if v.dim() == 1:
                v.add_(0.1 * (torch.rand(v.shape, generator=g) * 2 - 1))
    return sd


def zero_filled(x, cin=16):
    """(B, C, ...) -> (B, cin, ...) with zeros in the added channels."""
    return torch.cat([x, x.new_zeros((x.shape[0], cin - x.shape[1]) + tuple(x.shape[2:]))], 1)


def channels_last_view(x):
    """The (B, C, ...) view of a dense (B, ..., C) tensor: what to_pytorch_format and the sliding-window predictor hand to forward."""
    n = x.dim()
    return x.permute(0, *range(2, n), 1).contiguous().permute(0, n - 1, *range(1, n - 1))


# ---- the pack kernel ---------------------------------------------------------------------------------------------------------------------
PACK_SHAPES = ((1, (3, 5, 7)), (2, (4, 6, 33)), (3, (8, 8, 8)))        # less than one block; odd extents, two samples; more than one sample


def check_image_pack16(C, layout, dtype):
    """bpx_image_pack16 bit for bit against bpx_cast of the torch-built zero-filled NDHWC fp32 tensor.  The output is pre-filled with NaN (an
    unwritten padding channel would show) and carries a 256-element tail that must come back untouched."""
    from biapy_amd import _lib as L
    from kernel_checks import _res

    lib = L.lib
    dt = L.dt_of(torch.empty((), dtype=dtype))
    ibits = torch.int32 if dtype == torch.float32 else torch.int16
    rows = []
    for B, S in PACK_SHAPES:
        shape = S[1:] if layout == "2d" else S
        vox = int(np.prod(shape))
        g = torch.Generator().manual_seed(100 * C + B)
        x = (torch.randn((B, C) + tuple(shape), generator=g) * 3).to(DEV)
        if layout == "channels_last":
            x = channels_last_view(x)
            assert not x.is_contiguous() or vox == 1
            sv, sc = C, 1
        else:
            sv, sc = 1, vox
        ref32 = zero_filled(x).reshape(B, 16, vox).permute(0, 2, 1).contiguous()
        want = torch.empty(ref32.shape, dtype=dtype, device=DEV)
        if dtype == torch.float32:
            want.copy_(ref32)
        else:
            L.check(lib.bpx_cast(L.F32, ref32.data_ptr(), dt, want.data_ptr(), ref32.numel(), L.stream_ptr()))
        n = B * vox * 16
        out = torch.full((n + 256,), float("nan"), dtype=dtype, device=DEV)
        before = out.view(ibits).clone()
        L.check(lib.bpx_image_pack16(dt, B, vox, C, x.data_ptr(), C * vox, sv, sc, out.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
        got = out.view(ibits)
        tag = f"image_pack16[C={C} {layout} {str(dtype)[6:]} B={B} {shape}]"
        rows.append(_res(tag + ".bits_differ", int((got[:n] != want.view(ibits).reshape(-1)).sum()), 0))
        rows.append(_res(tag + ".tail_touched", int((got[n:] != before[n:]).sum()), 0))
    return rows


# ---- engine: the same bits as the 16-channel path ------------------------------------------------------------------------------------------
def _engine_sd(C, fm, norm, seed):
    sd = perturbed_state_dict(C, fm, seed)
    if norm == "bn":
        for n in bn_layers(NetConfig(in_ch=1, feature_maps=list(fm), normalization="bn")):
            c = sd[n + ".weight"].numel()
            sd[n + ".running_mean"], sd[n + ".running_var"] = torch.zeros(c), torch.ones(c)
            sd[n + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)
    return sd


def check_same_bits_as_16_channels(C, fm, patch, B, dtype, norm="in", seed=3, ndim=3):
    """The C-channel engine on true-shaped parameters and a C-channel image against the in_ch = 16 engine on the zero-padded parameters and the
    zero-filled image: logits and every gradient (the two padded ones sliced) must be equal bit for bit - they are the same launches on the
    same operands.  ndim = 2: (B, C, Y, X) tensors and 2-D parameters."""
    from biapy_amd.engine import ResUNetEngine
    from kernel_checks import _res

    fm = list(fm)
    zd = None if ndim == 3 else [1] * (len(fm) - 1)
    sd = _engine_sd(C, fm, norm, seed) if ndim == 3 else state_dict_2d(perturbed_state_dict(C, fm, seed, zd=zd))
    g = torch.Generator().manual_seed(seed + 11)
    x = torch.randn((B, C) + tuple(patch), generator=g).to(DEV)
    out = {}
    for tag, cin in (("C", C), ("16", 16)):
        eng = ResUNetEngine(NetConfig(in_ch=cin, feature_maps=fm, normalization=norm, z_down=zd, ndim=ndim), dtype)
        P = {k: v.clone().to(DEV) for k, v in sd.items()}
        xin = x
        if cin == 16:
            P, xin = pad_input_channels(P, 16), zero_filled(x)
        logits, ctx = eng.forward(P, xin, save=True)
        dl = torch.sin(torch.arange(logits.numel(), device=DEV, dtype=torch.float32)).reshape(logits.shape) / logits.numel()
        G = eng.backward(P, ctx, dl)
        torch.cuda.synchronize()
        out[tag] = (logits, G, {k: tuple(v.shape) for k, v in P.items()})
    (la, Ga, _), (lb, Gb, _) = out["C"], out["16"]
    name = f"same_bits[C={C} {norm} {str(dtype)[6:]} fm={fm} {tuple(x.shape)}]"
    rows = [_res(name + ".logits_differ", 0.0 if torch.equal(la, lb) else 1.0, 0),
            _res(name + ".logits_finite", 0.0 if bool(torch.isfinite(la).all()) and float(la.abs().max()) > 0 else 1.0, 0)]
    bad, shapes_ok = [], True
    for k, p in sd.items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            continue
        gb = Gb[k][:, :C] if Gb[k].shape != Ga[k].shape else Gb[k]
        shapes_ok &= tuple(Ga[k].shape) == tuple(p.shape)
        if not torch.equal(Ga[k], gb):
            bad.append(k)
    rows.append(_res(name + ".gradients_differ", len(bad), 0, extra=", ".join(bad[:4])))
    rows.append(_res(name + ".grad_shapes_are_the_parameters", 0.0 if shapes_ok else 1.0, 0))
    return rows


# ---- modules against the fp32 oracle -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_step_3d(C, fm, patch, B, seed):
    """(state dict, x, target, oracle logits, loss, gradients) of one BCE step of the C-channel ResUNet: computed once, shared, never modified."""
    sd = perturbed_state_dict(C, fm, seed)
    g = torch.Generator().manual_seed(seed + 17)
    x = torch.randn((B, C) + tuple(patch), generator=g)
    tgt = (torch.rand((B, 1) + tuple(patch), generator=g) > 0.5).float()
    loss, lo, grads = net_oracle.train_step_grads(sd, x, tgt, feature_maps=list(fm))
    return sd, x, tgt, lo, loss, grads


def _module_rows(tag, m, x, tgt, lo_ref, loss_ref, grads_ref, dtype, depth):
    """One training step and one eval forward of a module on x against the oracle's figures, with kernel_checks' bars."""
    import kernel_checks as K

    tagd = K._mode(dtype)[0]
    m.zero_grad(set_to_none=True)
    logits = m.train()(x)
    loss = F.binary_cross_entropy_with_logits(logits, tgt.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    scale = lo_ref.abs().max().item()
    rows = [K._res(tag + ".logits_rel", (logits.detach().cpu() - lo_ref).abs().max().item() / scale, K.LOGITS_TOL[tagd]),
            K._res(tag + ".loss", abs(loss.item() - float(loss_ref)), K.LOSS_TOL[tagd])]
    G = {k: p.grad for k, p in m.named_parameters()}
    shapes_ok = all(G[k] is not None and G[k].shape == p.shape for k, p in m.named_parameters())
    rows.append(K._res(tag + ".grad_shapes_are_the_parameters", 0.0 if shapes_ok else 1.0, 0))
    rows += K.grad_rows(tag, G, grads_ref, tagd, depth)
    with torch.no_grad():
        pr = m.eval()(x)
    rows.append(K._res(tag + ".eval_logits_rel", (pr.cpu() - lo_ref).abs().max().item() / scale, K.LOGITS_TOL[tagd]))
    m.train()
    return rows


def check_module_3d(C, dtype, fm=(16, 32, 64), patch=(16, 32, 32), B=2, seed=5):
    """ResUNet(image_shape = patch + (C,)) through the module (strict load of the reference-shaped state dict, autograd backward) against the
    fp32 oracle on the C-channel network: planar input and channels-last view."""
    from biapy_amd.resunet import ResUNet
    import kernel_checks as K

    sd, x, tgt, lo, loss, grads = _oracle_step_3d(C, tuple(fm), tuple(patch), B, seed)
    m = ResUNet(image_shape=tuple(patch) + (C,), compute_dtype=dtype, **module_kwargs(fm))
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    rows = []
    for layout, xin in (("planar", x.to(DEV)), ("channels_last", channels_last_view(x.to(DEV)))):
        tag = f"multichannel_resunet[C={C} {K._mode(dtype)[0]} {layout} fm={list(fm)} {tuple(x.shape)}]"
        rows += _module_rows(tag, m, xin, tgt, lo, loss, grads, dtype, len(fm) - 1)
    return rows


def check_module_2d(kind, dtype, C=3, fm=(16, 32, 64), patch=(64, 64), B=2, seed=9):
    """A 2-D RGB ResUNet / U_Net through the module against the oracle driven by the module's own state dict."""
    from biapy_amd.resunet import ResUNet
    from biapy_amd.unet import U_Net
    from oracle import unet_oracle
    import kernel_checks as K

    torch.manual_seed(seed)
    cls, fwd = (ResUNet, net_oracle.resunet_forward) if kind == "resunet" else (U_Net, unet_oracle.unet_forward)
    m = cls(image_shape=tuple(patch) + (C,), compute_dtype=dtype, **module_kwargs(fm))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.1 * (torch.rand(p.shape, generator=g) * 2 - 1))
    x = torch.randn((B, C) + tuple(patch), generator=g)
    tgt = (torch.rand((B, 1) + tuple(patch), generator=g) > 0.5).float()
    ref = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    lo = fwd(ref, x, list(fm))
    loss = F.binary_cross_entropy_with_logits(lo, tgt)
    names = [k for k, _ in m.named_parameters()]
    grads = dict(zip(names, torch.autograd.grad(loss, [ref[k] for k in names])))
    m = m.to(DEV)
    tag = f"multichannel_{kind}_2d[C={C} {K._mode(dtype)[0]} fm={list(fm)} {tuple(x.shape)}]"
    rows = _module_rows(tag + "[planar]", m, x.to(DEV), tgt, lo.detach(), loss.detach(), grads, dtype, len(fm) - 1)
    rows += _module_rows(tag + "[channels_last]", m, channels_last_view(x.to(DEV)), tgt, lo.detach(), loss.detach(), grads, dtype, len(fm) - 1)
    return rows


def check_sliding_window(dtype, C=3):
    """crop -> forward -> merge of a C-channel volume on the device against the same pipeline built from the oracle pieces on the CPU (the shapes of
    kernel_checks.check_sliding_window)."""
    from biapy_amd.resunet import ResUNet
    from biapy_amd.workflow import SlidingWindowPredictor
    from oracle import tiling_oracle as TO
    import kernel_checks as K

    fm = [16, 32]
    sd = net_oracle.init_state_dict(C, fm, seed=5)
    m = ResUNet(image_shape=(32, 32, 32, C), compute_dtype=dtype, **module_kwargs(fm))
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    vol = np.random.RandomState(2).randn(48, 40, 56, C).astype(np.float32)
    ov, pad, patch = (0.5, 0.25, 0.5), (0, 4, 0), (32, 32, 32)
    p, _ = TO.crop(vol, patch + (C,), ov, pad)
    with torch.no_grad():
        pr = torch.sigmoid(net_oracle.resunet_forward(sd, torch.from_numpy(p).permute(0, 4, 1, 2, 3), fm)).permute(0, 2, 3, 4, 1).contiguous().numpy()
    ref = TO.merge(pr, vol.shape[:3] + (1,), overlap=ov, padding=pad)
    if dtype == torch.float16:
        m.compute_dtype = torch.bfloat16
        sw = SlidingWindowPredictor(m, patch, ov, pad, batch_size=5, compute_dtype=torch.float16)
    else:
        sw = SlidingWindowPredictor(m, patch, ov, pad, batch_size=5)
    got = sw.predict(torch.from_numpy(vol).cuda()).cpu().numpy()
    tagd, band, _ = K._mode(dtype)
    rows = [K._res(f"multichannel_sliding_window_prob[C={C} {tagd}]", np.abs(got - ref).max(), {"f32": 2e-5, "f16": 4e-3}[tagd])]
    lab_ref, lab_got = (ref > 0.5), (got > 0.5)
    near = np.abs(ref - 0.5) < band
    rows.append(K._res(f"multichannel_sliding_window_labels_away_from_threshold[C={C} {tagd}]", int(((lab_ref != lab_got) & ~near).sum()), 0,
                       extra=f"undecidable voxels: {int(near.sum())} of {near.size}"))
    return rows


def check_graph_replay(dtype=torch.float16, C=3, fm=(16, 32), patch=(16, 32, 32), B=2, seed=13):
    """capture_graphs on a C-channel model: two replayed training calls equal the eager calls bit for bit (logits and all gradients)."""
    from biapy_amd.resunet import ResUNet
    from kernel_checks import _res

    sd = perturbed_state_dict(C, fm, seed)
    m = ResUNet(image_shape=tuple(patch) + (C,), compute_dtype=dtype, **module_kwargs(fm))
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train()
    g = torch.Generator().manual_seed(seed + 1)
    xs = [torch.randn((B, C) + tuple(patch), generator=g).to(DEV) for _ in range(2)]
    tgt = (torch.rand((B, 1) + tuple(patch), generator=g) > 0.5).float().to(DEV)

    def step(x):
        m.zero_grad(set_to_none=True)
        lo = m(x)
        F.binary_cross_entropy_with_logits(lo, tgt).backward()
        torch.cuda.synchronize()
        return lo.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}

    eager = [step(x) for x in xs]
    m.capture_graphs(xs[0])
    replayed = [step(x) for x in xs]
    used = getattr(m, "_graphs", None) is not None
    m.release_graphs()
    rows = [_res("multichannel_graph_replay.graphs_captured", 0.0 if used else 1.0, 0)]
    for i, ((le, Ge), (lr, Gr)) in enumerate(zip(eager, replayed)):
        rows.append(_res(f"multichannel_graph_replay.call{i}.logits_differ", 0.0 if torch.equal(le, lr) else 1.0, 0))
        bad = [k for k in Ge if not torch.equal(Ge[k], Gr[k])]
        rows.append(_res(f"multichannel_graph_replay.call{i}.gradients_differ", len(bad), 0, extra=", ".join(bad[:4])))
    return rows

"""BatchNorm ("bn") normalisation on the MI355X: the finalize kernels against fp64, the network against a BatchNorm oracle, running buffers,
eval mode, graph replay and the launch set of a training step.

The network oracle is oracle.net_oracle with its _norm swapped for F.batch_norm (monkeypatch, this module only): training mode uses the batch
statistics and updates the running buffers of the state dict in place, eval mode reads them.
"""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kernel_checks import GRAD_TOL, LOGITS_TOL, LOSS_TOL, _mode, parity_rows

pytestmark = pytest.mark.gpu

DEV = "cuda"
BUFS = (".running_mean", ".running_var", ".num_batches_tracked")
MODES = [torch.float32, torch.bfloat16, torch.float16]


# ------------------------------------------------------------------------------------------------------------------------------------------
# finalize kernels on synthetic partials
# ------------------------------------------------------------------------------------------------------------------------------------------
def _fwd_ref(part, count, gamma, beta, eps, mom, rm, rv):
    p = part.double()
    S1, S2 = p[:, :, 0].sum((0, 1)), p[:, :, 1].sum((0, 1))
    n = part.shape[0] * count
    m = S1 / n
    v = (S2 / n - m * m).clamp_min(0)
    rstd = 1 / torch.sqrt(v + eps)
    rec = torch.stack([m, rstd, gamma.double() * rstd, beta.double() - m * gamma.double() * rstd], 1)
    return rec, (1 - mom) * rm.double() + mom * m, (1 - mom) * rv.double() + mom * v * n / (n - 1)


@pytest.mark.parametrize("N, tiles, C, count", [(2, 7, 16, 400), (4, 1500, 48, 64 ** 3), (3, 33, 20, 1000), (1, 1, 16, 2), (5, 1024, 256, 4096)])
def test_batchnorm_finalize_against_fp64(N, tiles, C, count):
    from biapy_amd import _lib as L

    g = torch.Generator().manual_seed(N * 1000 + C)
    vps = count / tiles
    mean = torch.randn(C, generator=g)
    x1 = (mean + 0.1 * torch.randn(N, tiles, C, generator=g)) * vps
    x2 = (mean * mean + 1 + 0.1 * torch.rand(N, tiles, C, generator=g)) * vps
    part = torch.stack([x1, x2], 2).float().contiguous()                # [N][tiles][2][C]
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    ref, rm_ref, rv_ref = _fwd_ref(part, count, gamma, beta, 1e-5, 0.1, rm0, rv0)
    off, ld = 8, C + 24                                                   # column range [8, 8 + C) of wider records
    gd, bd = gamma.to(DEV), beta.to(DEV)                                  # (held: a pointer to a freed temporary could be handed out again)
    outs = []
    for _ in range(2):
        pd = part.to(DEV)                                                 # consumed: a fresh copy per call
        rm, rv = torch.cat([torch.zeros(off), rm0]).to(DEV), torch.cat([torch.zeros(off), rv0]).to(DEV)
        nbt = torch.tensor(5, dtype=torch.int64, device=DEV)
        rec = torch.full((N, ld, 4), -7.0, device=DEV)
        L.check(L.lib.bpx_batchnorm_finalize(pd.data_ptr(), N, tiles, C, count, gd.data_ptr(), bd.data_ptr(), 1e-5, 0.1,
                                             rm[off:].data_ptr(), rv[off:].data_ptr(), nbt.data_ptr(), rec.data_ptr(), ld, off, L.stream_ptr()))
        torch.cuda.synchronize()
        outs.append((rec.cpu(), rm.cpu(), rv.cpu(), int(nbt)))
    rec, rm, rv, nbt = outs[0]
    assert nbt == 6
    assert (rec[:, :off] == -7).all() and (rec[:, off + C:] == -7).all() and (rm[:off] == 0).all()
    for n in range(N):
        e = (rec[n, off:off + C].double() - ref).abs() / ref.abs().max(0).values
        assert e.max() < 2e-6, (n, e.max())
    assert ((rm[off:].double() - rm_ref).abs() <= 2e-6 * rm_ref.abs().clamp_min(1)).all()
    assert ((rv[off:].double() - rv_ref).abs() <= 2e-6 * rv_ref.abs().clamp_min(1)).all()
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, b)                                          # bit-identical


@pytest.mark.parametrize("running", [0, 1], ids=["batch_stats", "running_stats"])
@pytest.mark.parametrize("N, tiles, C, count", [(2, 7, 16, 400), (4, 1500, 48, 64 ** 3), (1, 1, 16, 3), (3, 900, 96, 8000)])
def test_batchnorm_bwd_finalize_against_fp64(N, tiles, C, count, running):
    from biapy_amd import _lib as L

    g = torch.Generator().manual_seed(7 * N + C)
    part = torch.randn(N, tiles, 2, C, generator=g).contiguous()
    rec = torch.zeros(N, C, 4)
    rec[:, :, 0] = torch.randn(C, generator=g)
    rec[:, :, 1] = torch.rand(C, generator=g) + 0.5
    gamma = 1 + 0.3 * torch.randn(C, generator=g)
    p = part.double()
    S1, S2 = p[:, :, 0].sum((0, 1)), p[:, :, 1].sum((0, 1))
    inv = 0.0 if running else 1.0 / (N * count)                         # running statistics: constants, no mean / variance terms
    ga, rs, mu = gamma.double(), rec[0, :, 1].double(), rec[0, :, 0].double()
    m1, m2 = ga * S1 * inv, ga * S2 * inv
    ref = torch.stack([ga * rs, -rs * rs * m2, -rs * m1 + rs * rs * mu * m2], 1)
    recd, gd = rec.to(DEV), gamma.to(DEV)
    outs = []
    for _ in range(2):
        dg, db = torch.full((C,), 0.5, device=DEV), torch.full((C,), -0.25, device=DEV)
        coef = torch.empty(N, C, 4, device=DEV)
        pd = part.to(DEV)                                                 # consumed: a fresh copy per call
        L.check(L.lib.bpx_batchnorm_bwd_finalize(pd.data_ptr(), N, tiles, C, count, recd.data_ptr(), gd.data_ptr(),
                                                 dg.data_ptr(), db.data_ptr(), running, coef.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
        outs.append((coef.cpu(), dg.cpu(), db.cpu()))
    coef, dg, db = outs[0]
    for n in range(N):
        e = (coef[n, :, :3].double() - ref).abs() / ref.abs().max(0).values.clamp_min(1e-30)
        assert e.max() < 2e-6, (n, e.max())
        if running:
            assert (coef[n, :, 1:3] == 0).all()
    scale = (S1.abs().max() + S2.abs().max()).item()
    assert ((dg.double() - (S2 + 0.5)).abs().max() / scale) < 1e-6
    assert ((db.double() - (S1 - 0.25)).abs().max() / scale) < 1e-6
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)


def test_batchnorm_eval_records_one_launch():
    from biapy_amd import _lib as L

    g = torch.Generator().manual_seed(3)
    N, Cs, eps = 3, [16, 48, 256], [1e-5, 1e-3, 1e-5]
    ts, jobs, outs = [], (L.BnEvalJob * 3)(), []
    for q, c in enumerate(Cs):
        t = [1 + 0.3 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g), torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.1]
        td = [v.to(DEV) for v in t]
        o = torch.empty(N, c, 4, device=DEV)
        jobs[q] = L.BnEvalJob(*(v.data_ptr() for v in td), o.data_ptr(), c, eps[q])
        ts.append((t, td))
        outs.append(o)
    import ctypes
    L.check(L.lib.bpx_batchnorm_eval_records(3, ctypes.cast(jobs, ctypes.c_void_p), N, L.stream_ptr()))
    torch.cuda.synchronize()
    for (t, _), o, e in zip(ts, outs, eps):
        ga, be, rm, rv = (v.double() for v in t)
        rstd = 1 / torch.sqrt(rv + e)
        ref = torch.stack([rm, rstd, ga * rstd, be - rm * ga * rstd], 1)
        for n in range(N):
            assert ((o[n].cpu().double() - ref).abs() / ref.abs().max(0).values).max() < 2e-6


# ------------------------------------------------------------------------------------------------------------------------------------------
# network against the BatchNorm oracle
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def bn_oracle(monkeypatch):
    from oracle import net_oracle

    state = {"training": True}
    orig = net_oracle._norm

    def _norm(x, sd, key, kind, groups=8):
        if kind != "bn":
            return orig(x, sd, key, kind, groups)
        y = F.batch_norm(x, sd[key + ".running_mean"], sd[key + ".running_var"], sd[key + ".weight"], sd[key + ".bias"], state["training"], 0.1, 1e-5)
        if state["training"]:
            sd[key + ".num_batches_tracked"].add_(1)
        return y

    monkeypatch.setattr(net_oracle, "_norm", _norm)

    def step(sd, x, tgt, fm, z_down, training=True):
        """(loss, logits, {param: grad}) - logits only without a target; the buffers of sd are updated in place in training mode."""
        state["training"] = training
        params = {k: v.detach().clone().requires_grad_(tgt is not None) for k, v in sd.items() if not k.endswith(BUFS)}
        full = dict(params)
        full.update({k: v for k, v in sd.items() if k.endswith(BUFS)})
        logits = net_oracle.resunet_forward(full, x, fm, z_down=z_down, normalization="bn")
        if tgt is None:
            return None, logits.detach(), None
        loss = F.binary_cross_entropy_with_logits(logits, tgt)
        grads = torch.autograd.grad(loss, list(params.values()))
        return loss.detach(), logits.detach(), dict(zip(params, grads))

    return step


def _bn_sd(fm, z_down, seed, random_buffers=False):
    from biapy_amd.engine import NetConfig, bn_layers
    from oracle import net_oracle

    sd = net_oracle.init_state_dict(1, fm, seed=seed, z_down=z_down)
    g = torch.Generator().manual_seed(seed + 99)
    for n in bn_layers(NetConfig(in_ch=1, feature_maps=fm, z_down=z_down, normalization="bn")):
        c = sd[n + ".weight"].numel()
        sd[n + ".weight"] = sd[n + ".weight"] + 0.2 * torch.randn(c, generator=g)    # non-trivial affine parameters
        sd[n + ".bias"] = sd[n + ".bias"] + 0.2 * torch.randn(c, generator=g)
        sd[n + ".running_mean"] = 0.2 * torch.randn(c, generator=g) if random_buffers else torch.zeros(c)
        sd[n + ".running_var"] = 0.5 + torch.rand(c, generator=g) if random_buffers else torch.ones(c)
        sd[n + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)
    return sd


def _grad_check(tag, G, grads_ref, tagd):
    """Relative L2 error of every gradient; parameters whose exact gradient is zero (conv biases whose output only reaches a BatchNorm) are held
    against the LARGEST gradient norm of the network instead of their own noise."""
    gmax = max(v.norm().item() for v in grads_ref.values())
    zero_bar = {"f32": 1e-5, "bf16": 2e-2, "f16": 1e-2}[tagd]
    bad = []
    for k, gr in grads_ref.items():
        gg = G[k].cpu()
        if gr.norm().item() < 1e-6 * gmax:
            e = gg.norm().item() / gmax
            if e > zero_bar:
                bad.append((k, "zero", e))
        else:
            e = (gg - gr).norm().item() / gr.norm().item()
            if e > GRAD_TOL[tagd]:
                bad.append((k, "rel", e))
    assert not bad, (tag, bad[:5])


NETS = {"cfg2_32": ([16, 32, 64, 128, 256], [2, 2, 2, 2], (32, 32, 32), 2), "ragged3": ([16, 32, 64], [1, 2], (12, 40, 16), 3)}


@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("dtype", MODES, ids=["f32", "bf16", "mixed"])
def test_bn_network_training_against_oracle(bn_oracle, net, dtype):
    from biapy_amd.engine import NetConfig, ResUNetEngine

    fm, zd, patch, B = NETS[net]
    tagd = _mode(dtype)[0]
    sd = _bn_sd(fm, zd, seed=11)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(B, 1, *patch, generator=g)
    tgt = (torch.rand(B, 1, *patch, generator=g) > 0.5).float()
    eng = ResUNetEngine(NetConfig(in_ch=1, feature_maps=fm, z_down=zd, normalization="bn"), dtype)
    P = {k: v.to(DEV) for k, v in sd.items()}
    logits, ctx = eng.forward(P, x.to(DEV), save=True)
    lg = logits.detach().clone().requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(lg, tgt.to(DEV))
    loss.backward()
    G = eng.backward(P, ctx, lg.grad)
    torch.cuda.synchronize()
    ref_sd = {k: v.clone() for k, v in sd.items()}
    loss_ref, lo_ref, grads_ref = bn_oracle(ref_sd, x, tgt, fm, zd)
    tag = f"bn[{tagd} {net}]"
    err = (logits.cpu() - lo_ref).abs().max().item() / lo_ref.abs().max().item()
    assert err < LOGITS_TOL[tagd], (tag, err)
    assert abs(loss.item() - loss_ref.item()) < LOSS_TOL[tagd]
    rows = parity_rows(tag, logits.cpu(), lo_ref, tgt, dtype)
    assert all(r["ok"] for r in rows), rows
    _grad_check(tag, G, grads_ref, tagd)
    assert not any(k.endswith(BUFS) for k in G)
    for k in sd:
        if k.endswith(".num_batches_tracked"):
            assert int(P[k]) == 1 and int(ref_sd[k]) == 1


@pytest.mark.parametrize("dtype", MODES, ids=["f32", "bf16", "mixed"])
def test_bn_running_buffers_after_three_steps(bn_oracle, dtype):
    """Three training forwards of fixed parameters on three batches: the device buffers follow the oracle's."""
    from biapy_amd.engine import NetConfig, ResUNetEngine

    fm, zd, patch, B = NETS["ragged3"]
    tagd = _mode(dtype)[0]
    sd = _bn_sd(fm, zd, seed=21, random_buffers=True)
    eng = ResUNetEngine(NetConfig(in_ch=1, feature_maps=fm, z_down=zd, normalization="bn"), dtype)
    P = {k: v.to(DEV) for k, v in sd.items()}
    ref_sd = {k: v.clone() for k, v in sd.items()}
    g = torch.Generator().manual_seed(22)
    for _ in range(3):
        x = torch.randn(B, 1, *patch, generator=g) * 2 + 0.5
        tgt = (torch.rand(B, 1, *patch, generator=g) > 0.5).float()
        lo, ctx = eng.forward(P, x.to(DEV), save=True)
        eng.backward(P, ctx, torch.ones_like(lo) / lo.numel())
        bn_oracle(ref_sd, x, tgt, fm, zd)
    torch.cuda.synchronize()
    tol = 1e-5 if tagd == "f32" else LOGITS_TOL[tagd]
    for k in sd:
        if k.endswith(".num_batches_tracked"):
            assert int(P[k]) == 3 and int(ref_sd[k]) == 3
        elif k.endswith((".running_mean", ".running_var")):
            e = (P[k].cpu() - ref_sd[k]).abs().max().item() / ref_sd[k].abs().max().item()
            assert e <= tol, (k, e)


def _model(fm, zd, S, dtype, **kw):
    from biapy_amd.resunet import ResUNet

    d = len(fm)
    return ResUNet(image_shape=(S, S, S, 1), activation="elu", feature_maps=fm, drop_values=[0.0] * d, normalization="bn", yx_down=[2] * (d - 1),
                   z_down=zd, isotropy=[True] * d, larger_io=False, conv_layers=[2] * d, compute_dtype=dtype, **kw)


@pytest.mark.parametrize("dtype", MODES, ids=["f32", "bf16", "f16"])
def test_bn_eval_mode(bn_oracle, dtype):
    fm, zd = [16, 32, 64], [2, 2]
    tagd = _mode(dtype)[0]
    sd = _bn_sd(fm, zd, seed=31, random_buffers=True)
    m = _model(fm, zd, 32, dtype)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(32)
    x = torch.randn(3, 1, 32, 32, 32, generator=g)
    with torch.no_grad():
        lo = m(x.to(DEV)).cpu()
        singles = [m(x[i:i + 1].to(DEV)).cpu() for i in range(3)]
    _, lo_ref, _ = bn_oracle({k: v.clone() for k, v in sd.items()}, x, None, fm, zd, training=False)
    err = (lo - lo_ref).abs().max().item() / lo_ref.abs().max().item()
    assert err < LOGITS_TOL[tagd], err
    for i in range(3):
        assert torch.equal(lo[i:i + 1], singles[i])                      # running statistics: samples are independent
    assert all(int(v) == 0 for k, v in m.state_dict().items() if k.endswith(".num_batches_tracked"))
    # new buffers through load_state_dict (in-place copies): the cached eval records must follow
    sd2 = {k: v.clone() for k, v in sd.items()}
    for k in sd2:
        if k.endswith(".running_mean"):
            sd2[k] += 1.0
    m.load_state_dict(sd2, strict=True)
    with torch.no_grad():
        lo2 = m(x.to(DEV)).cpu()
    _, lo2_ref, _ = bn_oracle({k: v.clone() for k, v in sd2.items()}, x, None, fm, zd, training=False)
    moved = (lo2_ref - lo_ref).abs().max().item()
    assert moved > 5 * LOGITS_TOL[tagd] * lo_ref.abs().max().item() and (lo2 - lo).abs().max().item() > 0.5 * moved
    assert (lo2 - lo2_ref).abs().max().item() / lo2_ref.abs().max().item() < LOGITS_TOL[tagd]


@pytest.mark.parametrize("dtype", MODES, ids=["f32", "bf16", "mixed"])
def test_bn_eval_mode_gradients_against_oracle(bn_oracle, dtype):
    """Backward of an eval-mode forward (running statistics are constants: dx = gamma * rstd * g) against F.batch_norm(training=False)."""
    from biapy_amd.engine import NetConfig, ResUNetEngine

    fm, zd, patch, B = NETS["ragged3"]
    tagd = _mode(dtype)[0]
    sd = _bn_sd(fm, zd, seed=61, random_buffers=True)
    g = torch.Generator().manual_seed(62)
    x = torch.randn(B, 1, *patch, generator=g)
    tgt = (torch.rand(B, 1, *patch, generator=g) > 0.5).float()
    eng = ResUNetEngine(NetConfig(in_ch=1, feature_maps=fm, z_down=zd, normalization="bn"), dtype)
    eng.bn_training = False
    P = {k: v.to(DEV) for k, v in sd.items()}
    logits, ctx = eng.forward(P, x.to(DEV), save=True)
    lg = logits.detach().clone().requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(lg, tgt.to(DEV))
    loss.backward()
    G = eng.backward(P, ctx, lg.grad)
    torch.cuda.synchronize()
    loss_ref, lo_ref, grads_ref = bn_oracle({k: v.clone() for k, v in sd.items()}, x, tgt, fm, zd, training=False)
    assert (logits.cpu() - lo_ref).abs().max().item() / lo_ref.abs().max().item() < LOGITS_TOL[tagd]
    assert abs(loss.item() - loss_ref.item()) < LOSS_TOL[tagd]
    _grad_check(f"bn_eval[{tagd}]", G, grads_ref, tagd)
    for k in sd:
        if k.endswith(BUFS):
            assert torch.equal(P[k].cpu(), sd[k]), k                   # eval mode leaves the buffers alone


def test_bn_eval_forward_with_grad_enabled():
    """model.eval(); y = model(x) with gradients enabled (no torch.no_grad()): the running statistics, the same bits as without gradients, and a
    backward that works."""
    fm, zd = [16, 32, 64], [2, 2]
    sd = _bn_sd(fm, zd, seed=71, random_buffers=True)
    m = _model(fm, zd, 32, torch.float16)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    x = torch.randn(2, 1, 32, 32, 32, generator=torch.Generator().manual_seed(72)).to(DEV)
    with torch.no_grad():
        y0 = m(x)
    y = m(x)
    assert y.requires_grad and torch.equal(y.detach(), y0)
    y.square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    assert m.down_path[1].block[0].weight.grad.abs().max() > 0
    for k, v in m.state_dict().items():
        if k.endswith(BUFS):
            assert torch.equal(v.cpu(), sd[k]), k


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_bn_eval_mode_at_64_cubed(bn_oracle, dtype):
    """The 64^3 level runs the fused conv + pool kernel: in eval mode it gets null statistics pointers, like every other producer."""
    fm, zd = [16, 32, 64], [2, 2]
    tagd = _mode(dtype)[0]
    sd = _bn_sd(fm, zd, seed=81, random_buffers=True)
    m = _model(fm, zd, 64, dtype)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    x = torch.randn(2, 1, 64, 64, 64, generator=torch.Generator().manual_seed(82))
    with torch.no_grad():
        lo = m(x.to(DEV)).cpu()
    _, lo_ref, _ = bn_oracle({k: v.clone() for k, v in sd.items()}, x, None, fm, zd, training=False)
    assert (lo - lo_ref).abs().max().item() / lo_ref.abs().max().item() < LOGITS_TOL[tagd]


def test_bn_eval_records_follow_eps():
    fm, zd = [16, 32], [2]
    m = _model(fm, zd, 16, torch.float32)
    m.load_state_dict(_bn_sd(fm, zd, seed=91, random_buffers=True), strict=True)
    m = m.to(DEV).eval()
    x = torch.randn(2, 1, 16, 16, 16, device=DEV)
    with torch.no_grad():
        y1 = m(x)
        m.bottleneck.block[0].eps = 0.5                                  # no train() / eval() switch in between
        y2 = m(x)
        m.train().eval()                                                  # drops every cache
        y3 = m(x)
    assert not torch.equal(y1, y2) and torch.equal(y2, y3)


def test_bn_capture_graphs_leaves_buffers_and_replays_in_its_mode_only():
    fm, zd, S = [16, 32, 64], [2, 2], 32
    torch.manual_seed(101)
    m = _model(fm, zd, S, torch.float16)
    m.load_state_dict(_bn_sd(fm, zd, seed=101, random_buffers=True), strict=True)
    m = m.to(DEV).train()
    g = torch.Generator().manual_seed(102)
    x = torch.randn(2, 1, S, S, S, generator=g).to(DEV)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    m.capture_graphs(x)
    torch.cuda.synchronize()
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k                               # capturing is not training
    m.eval()
    y_eval = m(x)                                                         # grad enabled, captured shape: must NOT replay the training graph
    with torch.no_grad():
        y_ref = m(x)
    assert torch.equal(y_eval.detach(), y_ref)
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    m.train()
    m(x).sum().backward()                                                 # replayed: one training forward's buffer update
    torch.cuda.synchronize()
    assert all(int(v) == int(before[k]) + 1 for k, v in m.state_dict().items() if k.endswith(".num_batches_tracked"))
    assert any(not torch.equal(v, before[k]) for k, v in m.state_dict().items() if k.endswith(".running_mean"))
    m.release_graphs()


def test_bn_eval_sliding_window(bn_oracle):
    from biapy_amd.workflow import SlidingWindowPredictor
    from oracle import tiling_oracle

    fm, zd = [16, 32], [2]
    sd = _bn_sd(fm, zd, seed=41, random_buffers=True)
    m = _model(fm, zd, 16, torch.float32)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    vol = np.random.RandomState(4).randn(24, 16, 28, 1).astype(np.float32)
    ov, pad, patch = (0.25, 0.0, 0.5), (0, 0, 0), (16, 16, 16)
    p, _ = tiling_oracle.crop(vol, patch + (1,), ov, padding=pad)
    pt = torch.from_numpy(p).permute(0, 4, 1, 2, 3).contiguous()
    _, lo, _ = bn_oracle({k: v.clone() for k, v in sd.items()}, pt, None, fm, zd, training=False)
    pr = torch.sigmoid(lo).permute(0, 2, 3, 4, 1).numpy()
    ref = tiling_oracle.merge(pr, vol.shape, overlap=ov, padding=pad)
    got = SlidingWindowPredictor(m, patch, ov, pad, batch_size=5).predict(torch.from_numpy(vol).cuda()).cpu().numpy()
    assert np.abs(got - ref).max() < 2e-5


def test_bn_training_needs_more_than_one_value_per_channel():
    from biapy_amd.engine import NetConfig, ResUNetEngine

    fm, zd = [16, 32], [2]
    eng = ResUNetEngine(NetConfig(in_ch=1, feature_maps=fm, z_down=zd, normalization="bn"), torch.float32)
    P = {k: v.to(DEV) for k, v in _bn_sd(fm, zd, seed=1).items()}
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        eng.forward(P, torch.randn(1, 1, 2, 2, 2, device=DEV), save=True)
    assert all(int(v) == 0 for k, v in P.items() if k.endswith(".num_batches_tracked"))


# ------------------------------------------------------------------------------------------------------------------------------------------
# graphs and the launch set
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_bn_graphed_train_step_matches_eager_bit_for_bit():
    """N replays of GraphedTrainStep == N eager steps (the same step function: forward, loss, backward, the package's AdamW step): parameters and
    running buffers bit for bit."""
    from biapy_amd.graphs import GraphedInference, GraphedTrainStep, _LrTensors, _opt_step
    from biapy_amd.losses import BCEWithLogitsLoss

    fm, zd, S, B = [16, 32, 64], [2, 2], 32, 2
    g = torch.Generator().manual_seed(51)
    xs = [torch.randn(B, 1, S, S, S, generator=g).to(DEV) for _ in range(4)]
    ts = [(torch.rand(B, 1, S, S, S, generator=g) > 0.5).float().to(DEV) for _ in range(4)]
    torch.manual_seed(52)
    init = {k: v.clone() for k, v in _model(fm, zd, S, torch.float16).to(DEV).state_dict().items()}
    loss_fn = BCEWithLogitsLoss()

    def reset(m, opt):                                                    # undo warm-up steps: initial weights, buffers and optimizer state
        m.load_state_dict(init)
        for st in opt.state.values():
            for v in st.values():
                if torch.is_tensor(v):
                    v.zero_()

    runs = []
    for graphed in (False, True):
        m = _model(fm, zd, S, torch.float16).to(DEV).train()
        m.load_state_dict(init)
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, fused=True, capturable=True)
        if graphed:
            step = GraphedTrainStep(m, loss_fn, opt, xs[0], ts[0], warmup=1)
            reset(m, opt)
            for x, t in zip(xs, ts):
                step(x, t)
        else:
            lr = _LrTensors(opt, DEV)

            def eager(x, t):
                lr.sync()
                opt.zero_grad(set_to_none=True)
                loss = loss_fn(m(x), t)
                loss.backward()
                _opt_step(opt)

            eager(xs[0], ts[0])
            reset(m, opt)
            for x, t in zip(xs, ts):
                eager(x, t)
        torch.cuda.synchronize()
        runs.append({k: v.detach().clone() for k, v in m.state_dict().items()})
    eager, replayed = runs
    for k in eager:
        assert torch.equal(eager[k], replayed[k]), k
    assert all(int(v) == 4 for k, v in replayed.items() if k.endswith(".num_batches_tracked"))

    # a replayed inference reads the buffers of its time, not those of the capture
    m.eval()
    xe = xs[0]
    gi = GraphedInference(lambda v: m.predict_proba(v), xe)
    y0 = gi().clone()
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k.endswith(".running_mean"):
                v.add_(0.25)
    y1 = gi().clone()
    with torch.no_grad():
        y_eager = m.predict_proba(xe)
    assert not torch.equal(y0, y1)
    assert torch.equal(y1, y_eager)


def _launches(normalization):
    from biapy_amd import _lib as L
    from biapy_amd.resunet import ResUNet

    d = 5
    m = ResUNet(image_shape=(64, 64, 64, 1), activation="elu", feature_maps=[16, 32, 64, 128, 256], drop_values=[0.0] * d, normalization=normalization,
                yx_down=[2] * 4, z_down=[2] * 4, isotropy=[True] * d, larger_io=False, conv_layers=[2] * d, compute_dtype=torch.float16).to(DEV).train()
    x = torch.randn(4, 1, 64, 64, 64, device=DEV)
    m(x).sum().backward()                                                  # warm-up
    torch.cuda.synchronize()
    prof = L.Profile()
    L.lib.prof = prof
    try:
        m(x).sum().backward()
        torch.cuda.synchronize()
    finally:
        L.lib.prof = None
    return collections.Counter(r[0] for r in prof.records)


def test_bn_train_step_keeps_the_fast_path():
    fin = {"bpx_norm_finalize", "bpx_norm_bwd_finalize", "bpx_norm_bwd_finalize_deferred", "bpx_batchnorm_finalize", "bpx_batchnorm_bwd_finalize"}
    a, b = _launches("in"), _launches("bn")
    assert {k: v for k, v in a.items() if k not in fin} == {k: v for k, v in b.items() if k not in fin}
    assert b["bpx_batchnorm_finalize"] > 0 and b["bpx_batchnorm_bwd_finalize"] > 0
    assert not any(k in b for k in ("bpx_norm_finalize", "bpx_norm_bwd_finalize", "bpx_norm_bwd_finalize_deferred"))

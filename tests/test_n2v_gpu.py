"""Noise2Void on the device against its host twin (tests/n2v_ref.py), bit for bit: ``x_masked``, ``target``, ``last_coords`` and ``last_sources`` over
the shapes of the known-answer table, both views of ``x``, a misaligned ``x``, 2-D in both spellings, consecutive calls, the counter across 2^32, the four
manipulators, ``out=``, graph capture, an inner augmenter and a batch past 2 GiB; ``N2VLoss`` against its fp64 statement within the derived bounds
of tests/n2v_bounds.py; and ``train_one_epoch(augment=masker)``.  Measured figures go to profiles/n2v_values.txt."""
import os
import types

import numpy as np
import pytest
import torch

import augment_ref as AR
import n2v_bounds as NB
import n2v_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = os.path.join(ROOT, "profiles", "n2v_values.txt")
_rows = {}

# the known-answer table of tests/test_n2v_cpu.py: shape, box, radius
TABLE = (((13, 22, 37), 4, 2), ((1, 45, 50), (1, 22, 22), (0, 5, 5)), ((3, 5, 7), 8, 3), ((8, 8, 8), 1, 1), ((64, 64, 64), 4, 2))


def _record(key, text):
    """profiles/n2v_values.txt: one row per measured case, rewritten whole so that a partial run leaves a readable file."""
    _rows[key] = text
    try:
        with open(VALUES, "w") as f:
            f.write("biapy_amd.n2v / losses.N2VLoss on the device: what tests/test_n2v_gpu.py measured (bounds: tests/n2v_bounds.py)\n")
            for k in sorted(_rows):
                f.write(_rows[k] + "\n")
    except OSError:
        pass


def _masker(**kw):
    from biapy_amd.n2v import N2VMasker

    return N2VMasker(**kw)


def _host(shape5, seed):
    return np.random.default_rng(seed).standard_normal(shape5).astype(np.float32)


def _device(x_np, first=False, misalign=False):
    """The batch on the device: channel-last memory, optionally starting 4 bytes past a 16-byte boundary, optionally as its (B,C,...) view."""
    n = x_np.size
    buf = torch.empty(n + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    mem = buf[1:n + 1] if misalign else buf[:n]
    mem = mem.view(x_np.shape)
    mem.copy_(torch.from_numpy(x_np))
    nd = mem.dim()
    return mem.permute(0, nd - 1, *range(1, nd - 1)) if first else mem


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(dev, host):
    host = torch.from_numpy(np.ascontiguousarray(host))
    return dev.shape == host.shape and torch.equal(_bits(dev).cpu(), host.view(torch.int32))


def _check(m, x, x_np5, counter, out=None, normal=False, **ref_kw):
    """One call of masker ``m`` on ``x`` (any layout) against the twin at ``counter``; x_np5 is the batch as (B,Z,Y,X,C)."""
    from biapy_amd.augment import _layout

    xo, t = m(x, None, out=out)
    want_x, want_t, coords, sources = R.mask(x_np5, m.seed, counter, **ref_kw)
    assert xo.shape == x.shape and all(a == b for n, a, b in zip(x.shape, xo.stride(), x.stride()) if n > 1)
    B, Z, Y, X, C = x_np5.shape
    assert t.is_contiguous() and t.dtype == torch.float32 and t.shape[:2] == (B, 2 * C) and t.numel() == 2 * x.numel()
    assert torch.equal(m.last_coords.cpu(), torch.from_numpy(coords.astype(np.int32)))
    assert torch.equal(m.last_sources.cpu(), torch.from_numpy(sources.astype(np.int32)))
    assert _same(t.reshape(B, 2 * C, Z, Y, X), want_t)
    assert _layout(xo, "x_masked")[1] == _layout(x, "x")[1]
    got = _layout(xo, "x_masked")[0].reshape(B, Z, Y, X, C)
    if not normal:
        assert _same(got, want_x)
    else:                                              # the masked values are the device's own transcendental functions: everything else bit for bit
        on = torch.from_numpy(want_t[:, C:].transpose(0, 2, 3, 4, 1) > 0)
        assert torch.equal(_bits(got).cpu()[~on], torch.from_numpy(x_np5).view(torch.int32)[~on])
    return xo, t, got


# ---- 1. masking ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(TABLE)))
@pytest.mark.parametrize("manip", ["uniform_withCP", "uniform_withoutCP"])
def test_table_shapes_channels_batches_views_and_alignment(case, manip):
    shape, box, radius = TABLE[case]
    combos = [(B, C, first, misalign) for B in (1, 5) for C in (1, 3, 8) for first in (False, True) for misalign in (False, True)]
    if case == 4:                                                              # 64^3: the twin's share of the time
        combos = [(1, 1, False, False), (5, 3, True, True), (1, 8, True, False), (5, 1, False, True)]
    for B, C, first, misalign in combos:
        x_np = _host((B,) + shape + (C,), seed=B * 10 + C)
        x = _device(x_np, first, misalign)
        assert (x.data_ptr() % 16 == 4) == misalign
        m = _masker(seed=31, box=box, radius=radius, manipulator=manip)
        _check(m, x, x_np, 0, box=box, radius=radius, manipulator=manip)
        if (B, C) == (1, 1):
            assert (x_np.size % 4 != 0) == (case in (0, 1, 2))                 # 10582, 2250 and 105 elements: the scalar tail of the streaming pass
            n_masked = int((m.last_coords >= 0).sum())
            assert n_masked == {0: 167, 1: 5, 2: 0, 3: 512, 4: 4096}[case]     # the known answers of the rule (seed 31, counter 0)


def test_2d_in_both_spellings_and_the_derived_box():
    x_np = _host((3, 1, 45, 50, 2), seed=4)
    m5, m4 = _masker(seed=8), _masker(seed=8)
    _, t5, g5 = _check(m5, _device(x_np), x_np, 0)
    xo4, t4 = m4(_device(x_np[:, 0]))
    assert xo4.shape == (3, 45, 50, 2) and t4.shape == (3, 4, 45, 50) and t5.shape == (3, 4, 1, 45, 50)
    assert torch.equal(_bits(xo4), _bits(g5[:, 0])) and torch.equal(_bits(t4), _bits(t5[:, :, 0]))
    assert m5.config((1, 45, 50))["box"] == (1, 22, 22) and m5.last_coords.shape == (3, 2, 9)
    xo4f, t4f = _masker(seed=8)(_device(x_np[:, 0], first=True))
    assert xo4f.shape == (3, 2, 45, 50) and torch.equal(_bits(xo4f.permute(0, 2, 3, 1)), _bits(xo4)) and torch.equal(t4f, t4)
    m3 = _masker(seed=8)                                                      # 3-D: the derived edge is 8
    x3 = _host((1, 16, 16, 24, 1), seed=5)
    _check(m3, _device(x3), x3, 0)
    assert m3.last_coords.shape == (1, 1, 12)


def test_consecutive_calls_and_the_counter_across_2_32():
    shape, box, radius = TABLE[0]
    x_np = _host((2,) + shape + (3,), seed=6)
    x = _device(x_np)
    m = _masker(seed=1234567890123456789, box=box, radius=radius)
    seen = []
    for q in range(3):
        assert int(m.counter) == q
        seen.append(_check(m, x, x_np, q, box=box, radius=radius)[2].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    m.counter.fill_(2 ** 32 - 1)
    for q in (2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1):
        assert int(m.counter) == q
        _check(m, x, x_np, q, box=box, radius=radius)


@pytest.mark.parametrize("i", range(len(R.CORNER_CASES)))
def test_manipulators_on_the_corner_cases(i):
    """The (6, 7, 9) sample with box 2: across these cases every corner of the sample is masked (tests/test_n2v_cpu.py::test_corner_seeds)."""
    case = R.CORNER_CASES[i]
    kw = dict(box=case["box"], radius=case["radius"], manipulator=case["manipulator"])
    x_np = _host((2,) + R.CORNER_SHAPE + (2,), seed=i)
    m = _masker(seed=case["seed"], sigma=0.75, **kw)
    xo, t, got = _check(m, _device(x_np), x_np, 0, normal=case["manipulator"] == "normal_additive", sigma=0.75, **kw)
    if case["manipulator"] == "identity":
        assert torch.equal(_bits(got).cpu(), torch.from_numpy(x_np).view(torch.int32)) and float(t[:, 2:].sum()) == float((m.last_coords >= 0).sum())


def test_normal_additive_statistics():
    """(x_masked - x) / sigma at the masked voxels is N(0, 1): five-sigma bands of mean and variance (augment_ref.noise_bounds), and it follows the
    float64 Box-Muller of the same Philox words within fp32 rounding of the transcendental functions."""
    shape, sigma = (32, 32, 32), 0.5
    x_np = np.zeros((4,) + shape + (2,), np.float32)                          # x = 0: the difference is sigma n exactly
    m = _masker(seed=99, box=1, radius=0, manipulator="normal_additive", sigma=sigma)
    xo, t, got = _check(m, _device(x_np), x_np, 0, normal=True, box=1, radius=0, manipulator="normal_additive", sigma=sigma)
    d = (got.double().cpu().numpy() / sigma).reshape(-1)
    n = d.size
    assert n == 4 * 32 ** 3 * 2 and float(t[:, 2:].sum()) == n
    b = AR.noise_bounds(n)
    _record("1_normal", f"normal_additive, {n} masked voxels: mean {d.mean():+.3e} (band {b['mean']:.3e}), variance - 1 {d.var() - 1:+.3e} (band {b['var']:.3e}), "
            f"max |n| {np.abs(d).max():.3f} (limit {b['max']:.3f})")
    assert abs(d.mean()) <= b["mean"] and abs(d.var() - 1) <= b["var"] and np.abs(d).max() <= b["max"]
    _, _, r0, r1 = R.draw(99, 0, 4, 2, shape, 1, 0, "normal_additive")
    want = R.normals(r0, r1).reshape(4, 2, -1).transpose(0, 2, 1).reshape(-1)
    assert np.abs(d - want).max() <= 1e-4


# ---- 2. call protocol and capture ---------------------------------------------------------------------------------------------------------------------
def test_out_and_the_overlap_refusals():
    shape, box, radius = TABLE[0]
    x_np = _host((2,) + shape + (3,), seed=7)
    for first in (False, True):
        x = _device(x_np, first)
        xo, to = torch.empty_like(x), torch.empty((2, 6) + shape, device="cuda")
        m = _masker(seed=5, box=box, radius=radius)
        got = _check(m, x, x_np, 0, out=(xo, to), box=box, radius=radius)
        assert got[0].data_ptr() == xo.data_ptr() and got[1].data_ptr() == to.data_ptr()
    x = _device(x_np)
    xo, to = torch.empty_like(x), torch.empty((2, 6) + shape, device="cuda")
    fresh = _masker(seed=5, box=box, radius=radius)
    big = torch.zeros(3 * x.numel() + 8, device="cuda")
    with pytest.raises(ValueError, match="overlap"):
        fresh(x, None, out=(x, to))
    with pytest.raises(ValueError, match="overlap"):                       # a shifted alias of the input's memory
        fresh(big[:x.numel()].view(x.shape), None, out=(big[8:x.numel() + 8].view(x.shape), to))
    with pytest.raises(ValueError, match="overlap"):
        fresh(big[:x.numel()].view(x.shape), None, out=(xo, big[8:2 * x.numel() + 8].view(to.shape)))
    with pytest.raises(ValueError, match="out\\[0\\] and out\\[1\\] overlap"):
        fresh(x, None, out=(big[:x.numel()].view(x.shape), big[8:2 * x.numel() + 8].view(to.shape)))
    for out, word in (((xo.double(), to), "out\\[0\\]"), ((xo, to[:, :3]), "out\\[1\\]"), ((xo.permute(0, 4, 1, 2, 3), to), "out\\[0\\]"), ((xo,), "pair")):
        with pytest.raises(ValueError, match=word):
            fresh(x, None, out=out)
    assert int(fresh.counter) == 0                                         # refused before any launch
    assert fresh(x, torch.zeros(1, device="cuda"))[0].shape == x.shape     # t is accepted and ignored


def test_captured_call_draws_anew_at_every_replay():
    shape, box, radius = TABLE[0]
    x_np = _host((2,) + shape + (3,), seed=9)
    x = _device(x_np)
    xo, to = torch.empty_like(x), torch.empty((2, 6) + shape, device="cuda")
    a = _masker(seed=77, box=box, radius=radius, manipulator="uniform_withoutCP")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a(x, None, out=(xo, to))                                           # the first call creates the masker's state: outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a(x, None, out=(xo, to))
    assert int(a.counter) == 1                                             # capturing ran nothing
    seen = []
    for i in range(3):
        g.replay()
        want_x, want_t, coords, sources = R.mask(x_np, 77, 1 + i, box=box, radius=radius, manipulator="uniform_withoutCP")
        assert _same(xo, want_x) and _same(to, want_t)
        assert torch.equal(a.last_coords.cpu(), torch.from_numpy(coords.astype(np.int32))) and torch.equal(a.last_sources.cpu(), torch.from_numpy(sources.astype(np.int32)))
        seen.append(a.last_coords.clone())
        assert int(a.counter) == i + 2
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def test_inner_augmenter_runs_first():
    from biapy_amd.augment import DeviceAugmenter

    kw = dict(vflip=True, hflip=True, zflip=True, brightness=(-0.1, 0.3), cutout=dict(n=(1, 2), size=(0.1, 0.3), cval=0.5), da_prob=0.7)
    x_np = _host((3, 6, 24, 40, 2), seed=11)
    x = _device(x_np)
    inner, alone = DeviceAugmenter(seed=41, **kw), DeviceAugmenter(seed=41, **kw)
    m = _masker(seed=42, box=4, radius=2, augment=inner)
    dummy = torch.zeros(3, 6, 24, 40, 1, dtype=torch.uint8, device="cuda")
    for q in range(2):
        xo, t = m(x)
        ax, _ = alone(x, dummy)
        assert torch.equal(inner.last_records, alone.last_records) and int(inner.counter) == int(alone.counter) == q + 1
        want_x, want_t, coords, sources = R.mask(ax.cpu().numpy(), 42, q, box=4, radius=2)
        assert _same(xo, want_x) and _same(t, want_t) and torch.equal(m.last_coords.cpu(), torch.from_numpy(coords.astype(np.int32)))


# ---- 3. past 2 GiB ------------------------------------------------------------------------------------------------------------------------------------
def test_batch_past_2gib():
    """33 x 128^3 x 8 fp32 = 2.2 GB in, 2.2 GB out and a 4.4 GB target: byte offsets past 2^31 and element offsets past 2^30, compared on the device."""
    B, N, C, box, radius = 33, 128, 8, (7, 9, 11), 3
    try:
        x = torch.empty(B, N, N, N, C, device="cuda")
        for b in range(B):
            x[b].normal_(generator=torch.Generator(device="cuda").manual_seed(b))
        assert x.numel() * 4 > 2 ** 31
        m = _masker(seed=3, box=box, radius=radius)
        xo, t = m(x)
        coords, _, _, _ = R.draw(3, 0, B, C, (N, N, N), box, radius)
        co, so = m.last_coords.long(), m.last_sources.long()
        on = co >= 0
        assert torch.equal(on.sum((1, 2)).cpu(), torch.from_numpy((coords >= 0).sum((1, 2))))            # the per-sample count is the twin's
        assert torch.equal(co[:, :, ::97].cpu(), torch.from_numpy(coords[:, :, ::97]))
        V = N ** 3
        xf, of = x.view(B, V, C), xo.view(B, V, C)
        bi = torch.arange(B, device="cuda")[:, None, None].expand_as(co)
        ci = torch.arange(C, device="cuda")[None, :, None].expand_as(co)
        flat_c, flat_s = ((bi * V + co) * C + ci)[on], ((bi * V + so) * C + ci)[on]
        assert torch.equal(xo.view(-1)[flat_c].view(torch.int32), x.view(-1)[flat_s].view(torch.int32))   # gathers at coords = gathers of x at sources
        tv = t.view(B, 2 * C, V)
        t_idx = ((bi * 2 * C + ci) * V + co)[on]
        assert torch.equal(t.view(-1)[t_idx].view(torch.int32), x.view(-1)[flat_c].view(torch.int32)) and bool((t.view(-1)[t_idx + C * V] == 1).all())
        assert int((tv[:, C:] != 0).sum()) == int(on.sum()) and int((tv[:, :C] != 0).sum()) <= int(on.sum())
        diff = xf.view(torch.int32) != of.view(torch.int32)
        assert int(diff.sum()) <= int(on.sum())
        diff.view(-1)[flat_c] = False
        assert not bool(diff.any())                                                                       # x_masked equals x off the coordinates
        del diff, bi, ci, flat_c, flat_s, t_idx
    finally:
        x = xo = t = xf = of = tv = m = None
        torch.cuda.empty_cache()


# ---- 4. the loss --------------------------------------------------------------------------------------------------------------------------------------
G_UP = NB.f32(1.7)


def _loss_run(pred, target, g=G_UP):
    from biapy_amd.losses import N2VLoss

    p = pred.clone().requires_grad_(True)
    loss = N2VLoss()(p, target)
    (loss * g).backward()
    return loss.detach(), p.grad


def _loss_case(name, pred, target, g=G_UP):
    from biapy_amd import _lib as L

    pred, target = pred.cuda(), target.cuda()
    (l1, g1), (l2, g2) = _loss_run(pred, target, g), _loss_run(pred, target, g)
    assert torch.equal(_bits(l1.reshape(1)), _bits(l2.reshape(1))) and torch.equal(_bits(g1), _bits(g2)), f"{name}: two calls differ"
    ref = NB.reference(pred, target, g)
    V = ref["V"]
    rows = NB.check(name, l1, g1, ref, NB.bounds(ref, L.lib.bpx_n2v_loss_blocks(V)))
    for r in rows:
        print(f"n2v_loss[{r['name']}] err/bound = {r['err']:.3e} {r['extra']}")
        _record("4_" + r["name"], f"N2VLoss {r['name']}: err / bound = {r['err']:.3e} ({r['extra']})")
    bad = [r for r in rows if not r["ok"]]
    assert not bad, bad
    return l1, g1


@pytest.mark.parametrize("C", [1, 3, 8])
@pytest.mark.parametrize("V", NB.VOXELS)
def test_loss_within_the_derived_bounds(V, C):
    gen = torch.Generator().manual_seed(NB.seed_of(V, C))
    N = 2 if V > 1024 * 512 else 3
    pred, target = NB.fixture(gen, N, C, V, "sparse")
    _loss_case(f"V{V}_C{C}", pred, target)


@pytest.mark.parametrize("kind,scale,g", [("ones", 1.0, G_UP), ("zeros", 1.0, G_UP), ("fraction", 1.0, G_UP), ("sparse", 1e4, G_UP), ("ones", 1e4, 1.0),
                                          ("sparse", 1.0, NB.f32(-0.003))])
def test_loss_dense_masks_large_predictions_and_upstream_gradients(kind, scale, g):
    gen = torch.Generator().manual_seed(17)
    pred, target = NB.fixture(gen, 2, 3, 5 * 7 * 37, kind, scale)
    loss, grad = _loss_case(f"{kind}_x{scale:g}_g{g:g}", pred.view(2, 3, 5, 7, 37), target.view(2, 6, 5, 7, 37), g)
    if kind == "zeros":
        assert float(loss) == 0 and not bool(grad.any()) and grad.shape == (2, 3, 5, 7, 37)


def test_loss_on_the_maskers_target():
    shape, box, radius = TABLE[0]
    x_np = _host((2,) + shape + (3,), seed=21)
    x = _device(x_np, first=True)
    xo, t = _masker(seed=2, box=box, radius=radius)(x)
    pred = torch.randn(2, 3, *shape, generator=torch.Generator().manual_seed(3))
    _loss_case("masker_target", pred, t)
    xo0, t0 = _masker(seed=2, box=8, radius=1)(_device(_host((1, 3, 5, 7, 1), seed=1)))          # the all-unmasked sample
    loss, grad = _loss_case("masker_nothing_masked", torch.randn(1, 1, 3, 5, 7), t0)
    assert float(t0.abs().sum()) == 0 and float(loss) == 0 and not bool(grad.any())


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------------------------
def _resunet():
    from biapy_amd.resunet import ResUNet

    torch.manual_seed(0)
    return ResUNet(image_shape=(32, 32, 32, 1), activation="elu", feature_maps=[16, 32], drop_values=[0.0, 0.0], normalization="in", yx_down=[2],
                   z_down=[2], isotropy=[True, True], larger_io=False, conv_layers=[2, 2], compute_dtype=torch.float32,
                   head_activations=["linear"]).cuda().train()


def _cfg():
    return types.SimpleNamespace(DATA=types.SimpleNamespace(PATCH_SIZE=(32, 32, 32, 1)),
                                 TRAIN=types.SimpleNamespace(GRADIENT_CLIP_NORM=0.0, LR_SCHEDULER=types.SimpleNamespace(NAME=""), VERBOSE=False))


def _train(graph, masked):
    from biapy_amd import train_engine as TE
    from biapy_amd.losses import InstanceChannelsLoss, N2VLoss

    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(2, 32, 32, 32, 1, generator=g), torch.rand(2, 32, 32, 32, 1, generator=g)) for _ in range(4)]
    m = _resunet()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, capturable=True)
    seen = []

    def metric(outputs, targets, metric_logger=None):
        seen.append(targets.detach().clone())

    masker = _masker(seed=31, box=4, radius=2) if masked else None
    loss = N2VLoss() if masked else InstanceChannelsLoss(channel_weights=(1,), out_channels=("F",), losses_to_use=["mse"], head_activations=["linear"]).cuda()
    TE.train_one_epoch(_cfg(), m, None, loss, metric, None, data, [opt], torch.device("cuda"), 0, loss_names=["loss"], graph=graph, augment=masker)
    torch.cuda.synchronize()
    assert hasattr(m, "_bpx_graph_step") == (graph == "on")
    return [p.detach().clone() for p in m.parameters()], seen, data, masker


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(graph, masked):
        if (graph, masked) not in cache:
            cache[(graph, masked)] = _train(graph, masked)
        return cache[(graph, masked)]

    return get


def _max_diff(a, b):
    return max((p - q).abs().max().item() for p, q in zip(a, b))


def test_train_one_epoch_trains_on_the_masked_batch(runs):
    """Four steps with graph='on' and four with graph='off', N2VLoss and maskers of one seed: both ways see the same targets (``metric_function``'s
    view), the twin's, and end with parameters as close as the same pair of runs does without the masker under a fixed MSE
    (``InstanceChannelsLoss(losses_to_use=["mse"])``), within a factor of 2 - the margin and baseline of the augmenter's own test."""
    p_on, seen_on, data, m_on = runs("on", True)
    p_off, seen_off, _, m_off = runs("off", True)
    assert int(m_on.counter) == int(m_off.counter) == 4 and len(seen_on) == len(seen_off) == 4
    for step, (s_on, s_off, (img, _)) in enumerate(zip(seen_on, seen_off, data)):
        assert torch.equal(s_on, s_off) and s_on.shape == (2, 2, 32, 32, 32)
        assert _same(s_on, R.mask(img.numpy(), 31, step, box=4, radius=2)[1])
    base = _max_diff(runs("on", False)[0], runs("off", False)[0])
    with_n2v = _max_diff(p_on, p_off)
    print(f"max |graph on - graph off| over all parameters after 4 steps: {base:.3e} under the plain MSE, {with_n2v:.3e} with masker and N2VLoss")
    _record("5_train", f"train_one_epoch, 32^3 batch 2, 4 steps: max |graph on - off| = {base:.3e} under the plain MSE, {with_n2v:.3e} with masker and N2VLoss "
            f"(allowed: 2 x the former)")
    assert with_n2v <= 2 * base


def test_forty_eager_steps_denoise_a_smooth_signal():
    """A sanity condition, not a threshold: on a smooth signal plus Gaussian noise the mean loss of the last 5 of 40 eager steps is below that of the
    first 5."""
    from biapy_amd import train_engine as TE
    from biapy_amd.losses import N2VLoss

    g = torch.Generator().manual_seed(8)
    z, y, x = torch.meshgrid(*(torch.linspace(0, 3.14159, 32),) * 3, indexing="ij")
    clean = (torch.sin(2 * z) * torch.cos(3 * y) + torch.sin(x))[None, ..., None]
    data = [(clean.expand(2, -1, -1, -1, -1) + 0.3 * torch.randn(2, 32, 32, 32, 1, generator=g), torch.zeros(2, 32, 32, 32, 1)) for _ in range(40)]
    m = _resunet()
    opt = torch.optim.AdamW(m.parameters(), lr=2e-3, capturable=True)
    losses = []
    crit = N2VLoss()

    def loss_fn(out, tgt):
        v = crit(out, tgt)
        losses.append(v.detach())
        return v

    TE.train_one_epoch(_cfg(), m, None, loss_fn, None, None, data, [opt], torch.device("cuda"), 0, loss_names=["loss"], graph="off",
                       augment=_masker(seed=1, box=4, radius=2))
    vals = torch.stack(losses).cpu()
    first, last = float(vals[:5].mean()), float(vals[-5:].mean())
    print(f"mean N2V loss of steps 0-4: {first:.4f}, of steps 35-39: {last:.4f}")
    _record("5_denoise", f"40 eager steps on a smooth signal + N(0, 0.3^2): mean loss of the first 5 steps {first:.4f}, of the last 5 {last:.4f}")
    assert len(vals) == 40 and last < first

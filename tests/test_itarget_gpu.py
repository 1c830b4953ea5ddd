"""``biapy_amd.targets.InstanceTargets`` / ``prepost.instance_targets`` on the MI355X, bit for bit against the NumPy twin (tests/itarget_ref.py) on the
inputs tests/test_itarget_cpu.py holds the twin against SciPy on: shapes, id inputs, views, options, the cross-checks against
``prepost.find_boundaries`` / ``label_distance`` on the device, repeatability, ``out=``, graph capture, the inner augmenter, a target past 2^31 bytes
and ``train_one_epoch(augment=InstanceTargets(...))``.  Measured figures go to profiles/itarget_values.txt."""
import os
import types

import numpy as np
import pytest
import torch

import itarget_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = os.path.join(ROOT, "profiles", "itarget_values.txt")
_rows = {}
NAMES = list(R.cases())
BLOBS, BLOBS2D, TINY = NAMES[0], "2-D 3 x 45x50", "tiny 3 x 3x5x7"


def _record(key, text):
    """profiles/itarget_values.txt: one row per measured case, rewritten whole so that a partial run leaves a readable file."""
    _rows[key] = text
    try:
        with open(VALUES, "w") as f:
            f.write("biapy_amd.targets.InstanceTargets on the device: what tests/test_itarget_gpu.py measured (twin and SciPy statement: tests/itarget_ref.py)\n")
            for k in sorted(_rows):
                f.write(_rows[k] + "\n")
    except OSError:
        pass


def _gen(channels=("F", "C", "D"), **kw):
    from biapy_amd.targets import InstanceTargets

    return InstanceTargets(channels, **kw)


def _device(t_np, first=False, misalign=False):
    """The ids on the device.  float32 / uint8: (B,*sample,1) memory, optionally starting 4 bytes (float32) past a 16-byte boundary, optionally as
    its (B,1,*sample) view; int32: (B,*sample)."""
    dt = {np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32}[t_np.dtype]
    n = t_np.size
    buf = torch.empty(n + 4, dtype=dt, device="cuda")
    assert buf.data_ptr() % 16 == 0
    mem = buf[1:n + 1] if misalign else buf[:n]
    if dt == torch.int32:
        mem = mem.view(t_np.shape)
        mem.copy_(torch.from_numpy(np.ascontiguousarray(t_np)))
        return mem
    mem = mem.view(t_np.shape + (1,))
    mem.copy_(torch.from_numpy(np.ascontiguousarray(t_np))[..., None])
    nd = mem.dim()
    return mem.permute(0, nd - 1, *range(1, nd - 1)) if first else mem


def _all(t_np):
    return R.ALL7 if t_np.ndim == 4 else R.ALL2D


def _hold(target, want, channels):
    bad = R.mismatch(target.cpu().numpy(), want, channels)
    assert bad is None, bad


# ---- 1. every input, every channel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(NAMES)))
def test_every_input_with_every_channel(i):
    t_np, n_max = R.cases()[NAMES[i]]
    ch = _all(t_np)
    it = _gen(ch, n_max=n_max)
    t = _device(t_np, first=i % 2 == 1)
    x = torch.zeros(1, device="cuda")
    xr, target = it(x, t)
    want, faults = R.batch_targets(t_np, ch, n_max)
    assert xr is x and target.shape == (t_np.shape[0], len(ch)) + t_np.shape[1:] and target.is_contiguous() and target.dtype == torch.float32
    _hold(target, want, ch)
    assert it.last_faults.dtype == torch.int32 and int(it.last_faults) == faults
    assert torch.equal(it.last_ids.cpu().view(t_np.shape), torch.from_numpy(R.sanitise(t_np, n_max)[0]))
    _record(f"1_{i:02d}", f"{NAMES[i]}: {len(ch)} channels bit for bit, faults {faults}")


def test_the_device_against_the_scipy_statement():
    """The device's channels against per-label SciPy on every input: F, C and D bit for bit, Dc, H, V and Z within 1 float32 ulp; the largest
    distances seen are recorded."""
    worst, count = {c: 0 for c in ("Dc", "H", "V", "Z")}, 0
    for name, (t_np, n_max) in R.cases().items():
        ch = _all(t_np)
        got = _gen(ch, n_max=n_max)(None, _device(t_np))[1].cpu().numpy()
        ids = R.sanitise(t_np, n_max)[0]
        want = np.stack([R.scipy_targets(ids[b], ch, n_max) for b in range(len(ids))])
        bad = R.mismatch(got, want, ch, ulps={c: 1 for c in worst})
        assert bad is None, f"{name}: {bad}"
        for k, c in enumerate(ch):
            if c in worst:
                worst[c] = max(worst[c], R.ulp_distance(got[:, k], want[:, k]))
        count += len(ids)
    _record("0_scipy", f"against per-label SciPy on {len(R.cases())} inputs ({count} samples): F, C, D bit for bit; largest ulp distance "
            + ", ".join(f"{c} {u}" for c, u in worst.items()) + " (allowed 1)")


@pytest.mark.parametrize("channels", [(c,) for c in R.CHANNELS] + [("F", "C", "D"), ("D", "Z", "F", "H", "C", "V", "Dc", "D")])
def test_single_channels_the_default_and_eight(channels):
    t_np, n_max = R.cases()[BLOBS]
    it = _gen(channels, n_max=n_max) if channels != ("F", "C", "D") else _gen(n_max=n_max)
    _hold(it(None, _device(t_np))[1], R.batch_targets(t_np, channels, n_max)[0], channels)


# ---- 2. options ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,conn", [(BLOBS, 1), (BLOBS, 2), (BLOBS, 3), (BLOBS2D, 1), (BLOBS2D, 2), ("two touching instances", 1), ("two touching instances", 3), (R.PIECES, 1), (R.PIECES, 3)])
@pytest.mark.parametrize("mode", ["thick", "inner"])
def test_contour_modes_and_connectivity_against_find_boundaries(name, conn, mode):
    from biapy_amd import prepost

    t_np, n_max = R.cases()[name]
    ch = ("C", "F")
    it = _gen(ch, n_max=n_max, contour_mode=mode, contour_connectivity=conn, f_excludes_contour=True)
    target = it(None, _device(t_np))[1]
    _hold(target, R.batch_targets(t_np, ch, n_max, contour_mode=mode, contour_connectivity=conn, f_excludes_contour=True)[0], ch)
    ids = it.last_ids.view(t_np.shape)
    for b in range(t_np.shape[0]):                                         # the same ids through prepost.find_boundaries on the device
        assert torch.equal(target[b, 0], prepost.find_boundaries(ids[b], conn, mode).float())
    assert not bool((target[:, 0] * target[:, 1]).any())                   # F leaves the contour out


def test_3d_connectivity_on_2d_samples_is_refused():
    t_np, n_max = R.cases()[BLOBS2D]
    with pytest.raises(ValueError, match="contour_connectivity"):
        _gen(("C",), n_max=n_max, contour_connectivity=3)(None, _device(t_np))
    with pytest.raises(ValueError, match="'Z' needs 3-D"):
        _gen(("Z",), n_max=n_max)(None, _device(t_np))


@pytest.mark.parametrize("name", [BLOBS, BLOBS2D, "an instance filling its sample", R.PIECES])
def test_unnormalised_distance_against_label_distance_with_and_without_a_clip(name):
    from biapy_amd import prepost

    t_np, n_max = R.cases()[name]
    ch = ("D", "F")
    for clip in (None, 2.5, 0.75):
        it = _gen(ch, n_max=n_max, d_norm="none", d_clip=clip)
        target = it(None, _device(t_np))[1]
        _hold(target, R.batch_targets(t_np, ch, n_max, d_norm="none", d_clip=clip)[0], ch)
        ids = it.last_ids.view(t_np.shape)
        for b in range(t_np.shape[0]):
            d = prepost.label_distance(ids[b])
            assert torch.equal(target[b, 0].view(torch.int32), (d if clip is None else d.clamp(max=clip)).view(torch.int32))
    if name == "an instance filling its sample":
        assert bool(torch.isinf(_gen(ch, n_max=n_max, d_norm="none")(None, _device(t_np))[1][0, 0]).all())      # without a clip the sentinel stays


@pytest.mark.parametrize("name,sampling", [(BLOBS, (2.0, 1.0, 1.0)), (BLOBS2D, (2.0, 1.0)), ("64^3 blobs", (2.0, 1.0, 1.0)), (R.PIECES, (2.0, 1.0, 1.0))])
def test_sampling_with_label_distances_own_bits(name, sampling):
    from biapy_amd import prepost

    t_np, n_max = R.cases()[name]
    ch = _all(t_np)
    it = _gen(ch, n_max=n_max, sampling=sampling)
    target = it(None, _device(t_np))[1]
    ids = it.last_ids.view(t_np.shape)
    d = np.stack([prepost.label_distance(ids[b], sampling=sampling).cpu().numpy() for b in range(t_np.shape[0])])
    _hold(target, R.batch_targets(t_np, ch, n_max, d=d, sampling=sampling)[0], ch)


# ---- 3. views ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.uint8, np.int32])
@pytest.mark.parametrize("name", [BLOBS, TINY, BLOBS2D])               # 10 582, 105 and 2 250 voxels: none a multiple of 4
def test_dtypes_layouts_and_a_misaligned_base(name, dtype):
    t_src, n_max = R.cases()[name]
    t_np = t_src.astype(dtype)
    ch = _all(t_np)
    want, faults = R.batch_targets(t_np, ch, n_max)
    it = _gen(ch, n_max=n_max)
    for first in ((False,) if dtype == np.int32 else (False, True)):
        for misalign in (False, True):
            t = _device(t_np, first=first, misalign=misalign)
            assert t.data_ptr() % 16 == (t.element_size() if misalign else 0)          # 4 bytes past a 16-byte boundary (1 for uint8)
            out_buf = torch.empty(want.size + 4, device="cuda")
            out = (out_buf[1:want.size + 1] if misalign else out_buf[:want.size]).view(want.shape)
            assert it(None, t, out=out)[1] is out
            _hold(out, want, ch)
            assert int(it.last_faults) == faults


def test_prepost_instance_targets_is_the_batch_of_one():
    from biapy_amd import prepost

    for name in (BLOBS, BLOBS2D, "8^3, every voxel its own id"):
        t_np, n_max = R.cases()[name]
        ch = _all(t_np)
        lab = torch.from_numpy(t_np[0].astype(np.int32)).cuda()
        one = _gen(ch, n_max=n_max, contour_mode="inner")(None, lab[None])[1][0]
        got = prepost.instance_targets(lab, ch, num=n_max, contour_mode="inner")
        assert got.shape == (len(ch),) + lab.shape and torch.equal(got.view(torch.int32), one.view(torch.int32))
        assert torch.equal(prepost.instance_targets(lab, ch, contour_mode="inner").view(torch.int32), one.view(torch.int32))     # num=None: labels.max()
        want = R.sample_targets(R.sanitise(t_np[0], n_max)[0], ch, n_max, contour_mode="inner")
        bad = R.mismatch(got.cpu().numpy(), want, ch, axis=0)
        assert bad is None, bad
    lab2 = torch.from_numpy(R.cases()["2-D as Z = 1, 1 x 1x45x50"][0][0, 0].astype(np.int32)).cuda()          # (45, 50): the 2-D spelling
    as3d = prepost.instance_targets(lab2[None], R.ALL2D, num=7, contour_connectivity=2)
    as2d = prepost.instance_targets(lab2, R.ALL2D, num=7, contour_connectivity=2)
    assert torch.equal(as2d.view(torch.int32), as3d[:, 0].view(torch.int32))                                # no z neighbours either way at Z = 1


# ---- 4. repeatability, out=, capture ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_out_is_checked():
    t_np, n_max = R.cases()["8^3, every voxel its own id"]
    it = _gen(R.ALL7, n_max=n_max)
    t = _device(t_np)
    a = it(None, t)[1].clone()
    b = it(None, t)[1]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    big, n_big = R.cases()["64^3 blobs"]
    it2, t2 = _gen(R.ALL7, n_max=n_big), _device(big)
    a2 = it2(None, t2)[1].clone()
    assert torch.equal(a2.view(torch.int32), it2(None, t2)[1].view(torch.int32))
    x = torch.zeros(1, 8, 8, 8, 1, device="cuda")
    shape = (1, 7, 8, 8, 8)
    for bad in (torch.empty(shape, device="cuda", dtype=torch.float64), torch.empty((1, 6, 8, 8, 8), device="cuda"), torch.empty(shape),
                torch.empty((1, 8, 8, 8, 7), device="cuda").permute(0, 4, 1, 2, 3)):
        with pytest.raises(ValueError, match="out must be a contiguous float32"):
            it(x, t, out=bad)
    pool = torch.zeros(7 * 512 + 512, device="cuda")
    pool[:512] = torch.from_numpy(t_np.reshape(-1))
    t_in = pool[:512].view(1, 8, 8, 8, 1)
    with pytest.raises(ValueError, match="out overlaps t"):
        it(None, t_in, out=pool[256:256 + 7 * 512].view(shape))
    xin = pool[512:1024].view(1, 8, 8, 8, 1)
    with pytest.raises(ValueError, match="out overlaps x"):
        it(xin, t, out=pool[512:].view(shape))
    assert it(xin, t_in, out=torch.empty(shape, device="cuda"))[0] is xin


def test_a_captured_call_replays_on_overwritten_ids():
    t_np, n_max = R.cases()[BLOBS]
    ch = R.ALL7
    it = _gen(ch, n_max=n_max)
    t = _device(t_np)
    out = torch.empty((3, 7) + t_np.shape[1:], device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        it(None, t, out=out)                                               # the first call sizes the generator's scratch: outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        it(None, t, out=out)
    feeds = [R.cases()["values that are no id"][0], np.zeros_like(t_np), np.ascontiguousarray(t_np[::-1])]
    for feed in feeds:
        t.copy_(torch.from_numpy(feed)[..., None])
        out.fill_(-3.0)
        g.replay()
        want, faults = R.batch_targets(feed, ch, n_max)
        _hold(out, want, ch)
        assert int(it.last_faults) == faults


# ---- 5. composition -------------------------------------------------------------------------------------------------------------------------------------------
def test_the_inner_augmenter_runs_first_and_its_ids_are_the_twins_input():
    from biapy_amd.augment import DeviceAugmenter

    kw = dict(vflip=True, hflip=True, zflip=True, rot90=True, rotation=(-30, 30), zoom=(0.8, 1.2), da_prob=0.8)
    ids_np = np.stack([R.blobs((12, 40, 40), 9, s, 3, 8) for s in (21, 22, 23)]).astype(np.float32)
    t = _device(ids_np)
    x = torch.randn(3, 12, 40, 40, 2, device="cuda")
    inner, alone = DeviceAugmenter(seed=41, **kw), DeviceAugmenter(seed=41, **kw)
    ch = R.ALL7
    it = _gen(ch, n_max=9, augment=inner)
    pool = torch.empty(3 * 7 * 12 * 40 * 40, device="cuda")
    t_in = pool[:t.numel()].view(t.shape).copy_(t)                            # ids that lie inside the would-be target
    for ids, bad in ((t, torch.empty(1, device="cuda")), (t_in, pool.view(3, 7, 12, 40, 40))):      # a refused call: nothing is drawn
        with pytest.raises(ValueError, match="out must be|out overlaps t"):
            it(x, ids, out=bad)
    assert int(inner.counter) == 0
    changed = 0
    for q in range(2):
        xo, target = it(x, t)
        ax, at = alone(x, t)
        assert torch.equal(inner.last_records, alone.last_records) and int(inner.counter) == int(alone.counter) == q + 1
        assert torch.equal(xo, ax)
        at_np = at.cpu().numpy()[..., 0]
        want, faults = R.batch_targets(at_np, ch, 9)
        _hold(target, want, ch)
        assert faults == 0 and int(it.last_faults) == 0                    # nearest-voxel interpolation: ids stay ids
        changed += int((at_np != ids_np).sum())
    assert changed > 0


# ---- 6. past 2^31 bytes -----------------------------------------------------------------------------------------------------------------------------------------
def test_a_target_past_2_31_bytes_equals_the_per_sample_calls():
    """37 x 7 x 128^3 fp32 = 2.17 GB: byte offsets past 2^31 and element offsets past 2^29, compared on the device sample by sample."""
    B, N, ch = 37, 128, R.ALL7
    try:
        base = torch.from_numpy(R.cases()["64^3 blobs"][0][0]).cuda().repeat_interleave(2, 0).repeat_interleave(2, 1).repeat_interleave(2, 2)
        t = torch.stack([torch.roll(base, (3 * b, 5 * b, 7 * b), (0, 1, 2)) for b in range(B)])[..., None].contiguous()
        it = _gen(ch, n_max=40)
        target = it(None, t)[1]
        assert target.numel() * 4 > 2 ** 31
        one = _gen(ch, n_max=40)
        for b in range(B):
            assert torch.equal(one(None, t[b:b + 1])[1][0].view(torch.int32), target[b].view(torch.int32)), b
        assert float(target[-1, 0].sum()) > 0
    finally:
        t = target = it = one = base = None
        torch.cuda.empty_cache()


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------------------------------------
def _resunet():
    from biapy_amd.resunet import ResUNet

    torch.manual_seed(0)
    return ResUNet(image_shape=(32, 32, 32, 1), activation="elu", feature_maps=[16, 32], drop_values=[0.0, 0.0], normalization="in", yx_down=[2],
                   z_down=[2], isotropy=[True, True], larger_io=False, conv_layers=[2, 2], compute_dtype=torch.float32, output_channels=[3],
                   head_activations=["linear"]).cuda().train()


def _cfg():
    return types.SimpleNamespace(DATA=types.SimpleNamespace(PATCH_SIZE=(32, 32, 32, 1)),
                                 TRAIN=types.SimpleNamespace(GRADIENT_CLIP_NORM=0.0, LR_SCHEDULER=types.SimpleNamespace(NAME=""), VERBOSE=False))


def _blob_batches(count, fixed):
    """(image, ids) batches of 2 x 32^3: the image is the foreground plus noise, so the channels can be learnt from it."""
    g = torch.Generator().manual_seed(5)
    data = []
    for k in range(count):
        ids = np.stack([R.blobs((32, 32, 32), 6, 100 + (0 if fixed else 2 * k) + b, 4, 9) for b in range(2)]).astype(np.float32)
        ids_t = torch.from_numpy(ids)[..., None]
        data.append(((ids_t > 0).float() + 0.1 * torch.randn(2, 32, 32, 32, 1, generator=g), ids_t))
    return data


def _loss():
    from biapy_amd.losses import InstanceChannelsLoss

    return InstanceChannelsLoss(channel_weights=(1, 1, 1), out_channels=["F", "C", "D"], losses_to_use=["bce", "bce", "mse"]).cuda()


def _train(graph, on_device):
    """Four steps on (image, ids) batches.  ``on_device``: the targets come from ``augment=InstanceTargets``; otherwise the same targets, computed
    beforehand, come through the loader as (B,Z,Y,X,3) tensors and nothing sits between the loader and the step."""
    from biapy_amd import train_engine as TE

    data = _blob_batches(4, fixed=False)
    it = _gen(("F", "C", "D"), n_max=6)
    if not on_device:
        data = [(img, it(None, ids.cuda())[1].permute(0, 2, 3, 4, 1).contiguous().cpu()) for img, ids in data]
    m = _resunet()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, capturable=True)
    seen = []

    def metric(outputs, targets, metric_logger=None):
        seen.append(targets.detach().clone())

    TE.train_one_epoch(_cfg(), m, None, _loss(), metric, None, data, [opt], torch.device("cuda"), 0, loss_names=["loss"], graph=graph,
                       augment=it if on_device else None)
    torch.cuda.synchronize()
    assert hasattr(m, "_bpx_graph_step") == (graph == "on")
    return [p.detach().clone() for p in m.parameters()], seen


def _max_diff(a, b):
    return max((p - q).abs().max().item() for p, q in zip(a, b))


def test_train_one_epoch_graph_replay_against_eager():
    """Four steps with graph='on' and four with graph='off', each with ``augment=InstanceTargets(("F", "C", "D"))`` and with the same targets
    computed beforehand and fed through the loader.  Bit for bit: the targets both ways train on (``metric_function``'s view) - each other's, the
    precomputed ones' and the twin's - and, within either way, the parameters after the four steps with the generator in the loop against those
    with precomputed targets: the generator changes nothing the step computes.  The replayed and the eager step themselves are two
    implementations of the step (``graphs.GraphedTrainStep`` against model call, ``backward()`` and ``optimizer.step()``) and do not end on the same parameter bits with or without the
    generator; measured on an MI355X: max |graph on - off| 1.5e-3 after 4 steps of this net either way.  That difference is held to the
    precomputed pair's, within the factor 2 that the augmenter's and the Noise2Void masker's tests use - which, after the two equalities above,
    adds nothing: with equal parameters in either mode the two differences are the same number.  It is kept as the statement of what replay
    against eager is held to."""
    ids = [b[1] for b in _blob_batches(4, fixed=False)]
    p_on, seen_on = _train("on", True)
    p_off, seen_off = _train("off", True)
    q_on, fixed_on = _train("on", False)
    q_off, fixed_off = _train("off", False)
    assert len(seen_on) == len(seen_off) == len(fixed_on) == len(fixed_off) == 4
    for s_on, s_off, f_on, f_off, t in zip(seen_on, seen_off, fixed_on, fixed_off, ids):
        assert s_on.shape == (2, 3, 32, 32, 32)
        for other in (s_off, f_on, f_off):
            assert torch.equal(s_on.view(torch.int32), other.contiguous().view(torch.int32))
        _hold(s_on, R.batch_targets(t.numpy()[..., 0], ("F", "C", "D"), 6)[0], ("F", "C", "D"))
    with_it, base = _max_diff(p_on, p_off), _max_diff(q_on, q_off)
    same_on, same_off = _max_diff(p_on, q_on), _max_diff(p_off, q_off)
    print(f"max |graph on - graph off| over all parameters after 4 steps: {with_it:.3e} with InstanceTargets, {base:.3e} with precomputed targets; "
          f"max |with - precomputed|: {same_on:.3e} replayed, {same_off:.3e} eager")
    _record("7_train", f"train_one_epoch(augment=InstanceTargets(F, C, D)), 32^3 batch 2, 4 steps: max |graph on - off| over the parameters = {with_it:.3e}, "
            f"{base:.3e} with the same targets precomputed (allowed: 2 x the latter); max |with - precomputed| {same_on:.3e} replayed, {same_off:.3e} eager (allowed: 0)")
    assert same_on == 0 and same_off == 0
    assert with_it <= 2 * base


def test_thirty_eager_steps_on_fixed_blobs_lower_the_loss():
    from biapy_amd import train_engine as TE

    data = _blob_batches(30, fixed=True)
    m = _resunet()
    opt = torch.optim.AdamW(m.parameters(), lr=2e-3, capturable=True)
    crit, losses = _loss(), []

    def loss_fn(out, tgt):
        v = crit(out, tgt)
        losses.append(v.detach())
        return v

    TE.train_one_epoch(_cfg(), m, None, loss_fn, None, None, data, [opt], torch.device("cuda"), 0, loss_names=["loss"], graph="off",
                       augment=_gen(("F", "C", "D"), n_max=6))
    vals = torch.stack(losses).cpu()
    print(f"loss of step 0: {float(vals[0]):.4f}, of step 29: {float(vals[-1]):.4f}")
    _record("7_steps", f"30 eager steps on fixed synthetic blobs, BCE + BCE + MSE on (F, C, D): loss {float(vals[0]):.4f} -> {float(vals[-1]):.4f}")
    assert len(vals) == 30 and float(vals[-1]) < float(vals[0])

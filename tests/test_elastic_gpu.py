"""The elastic deformation of the device augmenter on the MI355X (biapy_amd/augment.py step 0b, csrc/elastic.hip) against its statement, bit for
bit against the host twin (tests/elastic_ref.py) throughout: the noise, the smoothed field, ``bpx_elastic_apply`` for injected records and
fields, the drawn records, the full call against the twins composed, the unchanged launch list without ``elastic=``, refusals, scratch, graph
capture, a batch past 2 GiB and ``train_one_epoch(augment=...)``."""
import types

import numpy as np
import pytest
import torch

import augment_ref as AR
import elastic_ref as ER
import warp_ref as WR

pytestmark = pytest.mark.gpu

MODES = ["constant", "reflect", "edge"]
AFFINE = dict(rotation=(-30, 45), zoom=(0.8, 1.25), shear=(-10, 12), shift=(-0.1, 0.2))
# everything of the existing augmenter but the noise (its samples are the device's own; tests/test_augment_gpu.py covers them)
REST = dict(rot90=True, zflip=True, vflip=True, hflip=True, brightness=(-0.1, 0.3), contrast=(-0.2, 0.2), cutout=dict(n=(1, 4), size=(0.05, 0.3), cval=0.5))
PLANES = [(24, 20), (37, 41), (5, 3)]          # the issue's; not a multiple of the 32 x 32 tile (2 x 2 tiles); smaller than a tile


def _aug(**kw):
    from biapy_amd.augment import DeviceAugmenter

    return DeviceAugmenter(**kw)


def _first(mem):
    return mem.permute(0, mem.dim() - 1, *range(1, mem.dim() - 1))


def _mem(v, first):
    return v.permute(0, *range(2, v.dim()), 1) if first else v


def _pair(shape, C, Ct, tdtype, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(*shape, C, generator=g, device="cuda")
    t = torch.randint(0, 256, (*shape, Ct), generator=g, device="cuda").to(tdtype)
    return x, t


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the noise, bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, Y, X", [(3, 24, 20), (1, 7, 9), (2, 7, 9), (1500, 8, 8)])
def test_noise_bit_for_bit(B, Y, X):
    """(3, 24, 20): whole Philox blocks; 7 x 9: 126 elements a sample - a tail, and with B = 2 a sample that starts off a 16-byte boundary; B = 1500:
    the ``sample << 8`` counter word.  Also into a field that starts 4 bytes past a 16-byte boundary."""
    from biapy_amd import _lib as L

    seed, counter = 0x1234567887654321, (5 << 32) | 77
    rec = _dev(ER.make_records(np.ones(B), counter=counter))
    want = ER.noise(seed, counter, B, Y, X)
    for shift in (0, 1):
        buf = torch.full((B * 2 * Y * X + 8,), 9.0, device="cuda")
        L.check(L.lib.bpx_elastic_noise(seed, B, Y, X, rec.data_ptr(), buf[shift:].data_ptr(), L.stream_ptr()))
        got = buf.cpu().numpy()
        assert np.array_equal(_bits(got[shift:shift + want.size]), _bits(want.reshape(-1))), (B, Y, X, shift)
        assert (got[:shift] == 9).all() and (got[shift + want.size:] == 9).all()            # nothing written around the field


# ---- 2. the smoothed field, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [4.0, 0.5])
def test_smoothed_field_bit_for_bit(sigma):
    """(2, 24, 20) with sigma 4: radius 16 folds more than once on X = 20; sigma 0.5: radius 2."""
    x, t = _pair((2, 3, 24, 20), 1, 1, torch.uint8)
    aug = _aug(seed=41, da_prob=1.0, elastic=dict(sigma=sigma))
    for call in range(2):
        aug(x, t)
        got = aug.last_elastic_field.cpu().numpy()
        want = ER.smooth(ER.noise(41, call, 2, 24, 20), sigma)
        assert got.shape == (2, 2, 24, 20) and np.array_equal(_bits(got), _bits(want)), call


# ---- 3. the apply, bit for bit ----------------------------------------------------------------------------------------------------------------
def _fields(Y, X, seed):
    """Four (alpha, field (2, Y, X)) of a plane: a smooth field moving voxels by several voxels; displacements beyond three extents; +-1e30, +-inf
    and NaN entries in a moderate field; exact half-integers."""
    rng = np.random.default_rng([seed, Y, X])
    smooth = ER.smooth(ER.noise(seed, 0, 1, Y, X), 2.0)[0]
    far = rng.uniform(-3.5, 3.5, (2, Y, X)).astype(np.float32) * np.float32([Y, X])[:, None, None]
    wild = rng.uniform(-2, 2, (2, Y, X)).astype(np.float32)
    flat = wild.reshape(-1)
    at = rng.permutation(flat.size)[:min(flat.size, 10)]
    flat[at] = np.resize(np.float32([1e30, -1e30, np.inf, -np.inf, np.nan]), at.size)
    half = (rng.integers(-6, 7, (2, Y, X)) + 0.5).astype(np.float32)
    return [(25.0, smooth), (1.0, far), (2.0, wild), (1.0, half)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("first", [False, True], ids=["channels_last", "permuted_view"])
@pytest.mark.parametrize("tdtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("C, Ct", [(1, 1), (3, 2), (16, 8)])
def test_apply_bit_for_bit(C, Ct, tdtype, first, mode):
    """B = 2, Z = 3, every plane of PLANES, every field of ``_fields``, injected records and fields: torch.equal on the bits of every element of
    image and target against elastic_ref.apply.  The twin reproduces every coordinate in fp32: no tie band, nothing excluded."""
    aug = _aug(elastic=dict(mode=mode, cval=0.75))
    for pi, (Y, X) in enumerate(PLANES):
        x, t = _pair((2, 3, Y, X), C, Ct, tdtype, seed=pi)
        xin, tin = (_first(x), _first(t)) if first else (x, t)
        cases = _fields(Y, X, pi)
        for i in range(0, len(cases), 2):
            rec = ER.make_records([a for a, _ in cases[i:i + 2]])
            field = np.stack([f for _, f in cases[i:i + 2]])
            xo, to = aug(xin, tin, elastic_records=_dev(rec), elastic_field=_dev(field))
            assert xo.shape == xin.shape and xo.stride() == xin.stride() and to.dtype == tdtype
            want_x, want_t = ER.apply(x.cpu(), t.cpu(), rec, field, mode, cval=0.75)
            assert torch.equal(_mem(xo, first).cpu().view(torch.int32), want_x.view(torch.int32)), (Y, X, i)
            assert torch.equal(_mem(to, first).cpu(), want_t), (Y, X, i)
            assert torch.isfinite(xo).all()                                  # whatever the field holds, the taps are the plane's or cval
    assert int(aug.counter) == 2 * len(PLANES)


def test_flags_zero_is_the_input_bit_for_bit():
    """Z = 11: two runs of z planes per tile, the second partial.  Flags 0 copies the bits whatever alpha and the field hold; in a mixed batch
    only the sample that fired moves."""
    x, t = _pair((3, 11, 37, 41), 3, 2, torch.uint8)
    x[0, 0, 0, 0, 0], x[2, 10, 36, 40, 2], x[0, 5, 3, 4, 1] = float("nan"), float("inf"), -0.0
    field = np.random.default_rng(3).uniform(-40, 40, (3, 2, 37, 41)).astype(np.float32)
    for mode in MODES:
        aug = _aug(elastic=dict(mode=mode, cval=5.0))
        xo, to = aug(x, t, elastic_records=_dev(ER.make_records([3.0, 7.0, np.nan], fired=[0, 0, 0])), elastic_field=_dev(field))
        assert torch.equal(xo.view(torch.int32), x.view(torch.int32)) and torch.equal(to, t) and xo.data_ptr() != x.data_ptr()
        rec = ER.make_records([3.0, 1.5, 7.0], fired=[0, 1, 0])
        xo, to = aug(x, t, elastic_records=_dev(rec), elastic_field=_dev(field))
        assert torch.equal(xo[0].view(torch.int32), x[0].view(torch.int32)) and torch.equal(xo[2].view(torch.int32), x[2].view(torch.int32))
        assert torch.equal(to[0], t[0]) and torch.equal(to[2], t[2]) and not torch.equal(to[1], t[1])
        want_x, want_t = ER.apply(x.cpu(), t.cpu(), rec, field, mode, cval=5.0)
        assert torch.equal(xo[1].cpu().view(torch.int32), want_x[1].view(torch.int32)) and torch.equal(to.cpu(), want_t)
    aug = _aug(da_prob=0.0, elastic={}, **AFFINE, **REST)                    # nothing fires: warp, elastic and gather all copy
    xo, to = aug(x[:, :, :37, :37].contiguous(), t[:, :, :37, :37].contiguous())
    assert torch.equal(xo.view(torch.int32), x[:, :, :37, :37].contiguous().view(torch.int32)) and torch.equal(to, t[:, :, :37, :37])
    assert not aug.last_elastic_records[:, :2].any() and int(aug.counter) == 1


# ---- 4. draws ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 24, 24), (1500, 8, 8)], ids=["B3", "B1500"])
def test_draws_are_the_host_twins(shape):
    """8 consecutive calls with everything on: the elastic records equal elastic_ref.draw bit for bit; the augmentation records and the warp's
    flags and parameters are what their twins give - the existing streams did not move."""
    x, t = _pair(shape, 1, 1, torch.uint8)
    aug = _aug(seed=0x1234567887654321, elastic=dict(alpha=(3, 9), sigma=1.0), **AFFINE, **REST)
    B = shape[0]
    zyx = (1, *shape[1:]) if len(shape) == 3 else shape[1:]
    fired = 0
    for call in range(8):
        aug(x, t)
        got = aug.last_elastic_records.cpu().numpy()
        assert got.shape == (B, 8) and got.dtype == np.int32
        assert np.array_equal(got, ER.draw(aug.seed, call, B, aug.elastic_config())), call
        fired += int(got[:, 0].sum())
        flags, params = WR.draw(aug.seed, call, B, aug.warp_config())
        wrec = aug.last_warp_records.cpu().numpy()
        assert np.array_equal(wrec[:, 0].view(np.uint32), flags) and np.array_equal(wrec[:, 8:13], params.view(np.int32))
        want = AR.draw(aug.seed, call, B, zyx, _aug(seed=aug.seed, **REST).config())
        keep = [w for w in range(32) if w != AR.W_M]
        assert np.array_equal(aug.last_records.cpu().numpy()[:, keep], want[:, keep]), call
        assert int(aug.counter) == call + 1
    assert 0 < fired < 8 * B
    for p, flag in ((0.0, 0), (1.0, 1)):
        a = _aug(seed=5, da_prob=p, elastic={})
        a(x, t)
        rec = a.last_elastic_records.cpu().numpy()
        assert (rec[:, 0] == flag).all() and np.array_equal(rec, ER.draw(5, 0, B, a.elastic_config()))


# ---- 5. the full call -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_full_call_is_the_twins_composed(mode):
    """Warp, elastic deformation, rot90 / flips, contrast, brightness and cutout from drawn records: warp_ref.apply, then elastic_ref.apply with
    the TWIN's records and field (which the device's equal bit for bit), then augment_ref.apply with the device's own m - the mean of the INPUT."""
    shape = (3, 3, 40, 40)
    x, t = _pair(shape, 3, 2, torch.uint8, seed=11)
    x = x + 0.5
    aug = _aug(seed=122, da_prob=0.7, affine_mode="reflect", affine_cval=-1.0, elastic=dict(alpha=(6, 10), sigma=2.0, mode=mode, cval=0.25), **AFFINE, **REST)
    deformed = 0
    for call in range(3):
        xo, to = aug(x, t)
        recs, wrec = aug.last_records.cpu().numpy(), aug.last_warp_records.cpu().numpy()
        erec = ER.draw(122, call, 3, aug.elastic_config())
        field = ER.smooth(ER.noise(122, call, 3, 40, 40), 2.0)
        assert np.array_equal(aug.last_elastic_records.cpu().numpy(), erec) and np.array_equal(_bits(aug.last_elastic_field.cpu().numpy()), _bits(field))
        m = recs[:, AR.W_M].copy().view(np.float32)
        wx, wt = WR.apply(x.cpu(), t.cpu(), wrec, "reflect", cval=-1.0)
        ex, et = ER.apply(wx, wt, erec, field, mode, cval=0.25)
        want_x, want_t = AR.apply(ex, et, recs, m, cval=0.5)
        assert torch.equal(xo.cpu().view(torch.int32), want_x.view(torch.int32)), call
        assert torch.equal(to.cpu(), want_t), call
        for b in range(3):
            mean = x[b].double().mean().item()
            bound = float(np.spacing(np.float32(abs(mean)))) + x[b].numel() * 2.0 ** -53 * x[b].double().abs().mean().item()
            assert abs(float(m[b]) - mean) <= bound                           # m is the input's mean
            deformed += int(erec[b, 0])
    assert deformed


def test_launch_list_and_outputs_are_unchanged_without_elastic(monkeypatch):
    from biapy_amd import augment as A

    calls = []

    class Trace:
        def __getattr__(self, name):
            fn = getattr(A.L.lib, name)

            def call(*a):
                calls.append(name)
                return fn(*a)
            return call

    monkeypatch.setattr(A, "lib", Trace())
    x, t = _pair((2, 3, 24, 24), 2, 1, torch.uint8, seed=4)
    kw = dict(seed=9, da_prob=0.8, **AFFINE, **REST)
    outs = []
    for extra in (dict(), dict(elastic=None)):
        a = _aug(**kw, **extra)
        calls.clear()
        xo, to = a(x, t)
        assert calls == ["bpx_aug_draw", "bpx_warp_draw", "bpx_aug_mean_blocks", "bpx_aug_mean", "bpx_warp_apply", "bpx_aug_apply"], calls
        assert a.last_elastic_records is None and a.last_elastic_field is None and a._ex is None and a._ews is None
        outs.append((xo, to, a.last_records.clone(), a.last_warp_records.clone()))
    assert all(torch.equal(p, q) for p, q in zip(*outs))
    calls.clear()
    plain = _aug(seed=9, hflip=True)
    plain(x, t)
    assert calls == ["bpx_aug_draw", "bpx_aug_apply"]
    calls.clear()
    full = _aug(**kw, elastic={})
    xe, te = full(x, t)
    assert calls == ["bpx_aug_draw", "bpx_warp_draw", "bpx_elastic_draw", "bpx_aug_mean_blocks", "bpx_aug_mean", "bpx_warp_apply", "bpx_elastic_noise",
                     "bpx_sepfilter", "bpx_elastic_apply", "bpx_aug_apply"], calls
    assert torch.equal(full.last_records, outs[0][2]) and torch.equal(full.last_warp_records, outs[0][3])      # the other draws did not move
    calls.clear()
    full(x, t, elastic_records=full.last_elastic_records.clone(), elastic_field=full.last_elastic_field.clone())
    assert "bpx_elastic_draw" not in calls and "bpx_elastic_noise" not in calls and "bpx_sepfilter" not in calls and "bpx_elastic_apply" in calls


# ---- 6. refusals, scratch ---------------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    from biapy_amd import augment as A

    x, t = _pair((3, 2, 20, 24), 3, 1, torch.float32, seed=8)
    xo, to = torch.empty_like(x), torch.empty_like(t)
    fresh = _aug(elastic={})
    for out in ((x, to), (xo, t), (x, t)):
        with pytest.raises(ValueError, match="overlap"):
            fresh(x, t, out=out)
    rec, field = _dev(ER.make_records([1, 2, 3])), torch.zeros(3, 2, 20, 24, device="cuda")
    for bad in (rec[:2], rec.to(torch.int64), rec.cpu(), torch.zeros(3, 16, dtype=torch.int32, device="cuda"), torch.zeros(3, 16, dtype=torch.int32, device="cuda")[:, ::2]):
        with pytest.raises(ValueError, match="elastic_records"):
            fresh(x, t, elastic_records=bad)
    for bad in (field[:2], field.double(), field.cpu(), torch.zeros(3, 2, 24, 20, device="cuda"), torch.zeros(3, 20, 24, device="cuda"),
                torch.zeros(3, 2, 20, 48, device="cuda")[..., ::2]):
        with pytest.raises(ValueError, match="elastic_field"):
            fresh(x, t, elastic_field=bad)
    with pytest.raises(ValueError, match="built with elastic="):
        _aug(hflip=True)(x, t, elastic_field=field)
    monkeypatch.setattr(A, "ELASTIC_FIELD_MAX", 2 * 3 * 20 * 24)             # a mocked limit: this batch's field has exactly that many elements
    with pytest.raises(ValueError, match="2\\^31 or more"):
        fresh(x, t)
    assert int(fresh.counter) == 0 and fresh.last_elastic_records is None and fresh.last_elastic_field is None    # refused before any launch and any allocation
    monkeypatch.setattr(A, "ELASTIC_FIELD_MAX", 2 * 3 * 20 * 24 + 1)
    fresh(x, t)
    assert int(fresh.counter) == 1


def test_scratch_is_kept_until_the_shape_changes():
    x, t = _pair((2, 2, 20, 24), 1, 1, torch.uint8)
    aug = _aug(elastic={}, seed=1)
    aug(x, t)
    ptrs = lambda: tuple(b.data_ptr() for b in (aug._efield, aug._ews, aug._ex, aug._et, aug._erec))      # noqa: E731
    first = ptrs()
    aug(x, t)
    assert ptrs() == first and aug._ews.shape == (2, 2, 2, 20, 24) and aug._wx is None
    aug(x, t.float())
    assert ptrs()[:3] == first[:3] and aug._et.dtype == torch.float32
    x2, t2 = _pair((2, 2, 24, 20), 1, 1, torch.uint8)
    aug(x2, t2)
    assert aug._efield.shape == (2, 2, 24, 20) and aug._ex.shape == x2.shape and aug._et.dtype == torch.uint8
    plain = _aug(rotation=(-10, 10), seed=1)                                 # no elastic option: no elastic state at all
    plain(x, t)
    assert plain._efield is None and plain._ews is None and plain._ex is None and plain._et is None and plain.last_elastic_records is None


# ---- 7. graph ---------------------------------------------------------------------------------------------------------------------------------
def test_captured_call_draws_anew_at_every_replay():
    shape = (3, 3, 40, 40)
    x, t = _pair(shape, 3, 2, torch.uint8, seed=9)
    xo, to = torch.empty_like(x), torch.empty_like(t)
    a = _aug(seed=77, da_prob=0.8, affine_mode="reflect", elastic=dict(alpha=(6, 10), sigma=2.0, mode="edge"), **AFFINE, **REST)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a(x, t, out=(xo, to))                                              # the first call creates state and scratch: outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a(x, t, out=(xo, to))
    assert int(a.counter) == 1                                             # capturing ran nothing
    outs = []
    for i in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert int(a.counter) == i + 2
        recs, wrec = a.last_records.cpu().numpy(), a.last_warp_records.cpu().numpy()
        erec, field = ER.draw(77, i + 1, 3, a.elastic_config()), ER.smooth(ER.noise(77, i + 1, 3, 40, 40), 2.0)      # the twins for this replay's counter
        assert np.array_equal(a.last_elastic_records.cpu().numpy(), erec) and np.array_equal(_bits(a.last_elastic_field.cpu().numpy()), _bits(field))
        wx, wt = WR.apply(x.cpu(), t.cpu(), wrec, "reflect")
        ex, et = ER.apply(wx, wt, erec, field, "edge")
        want_x, want_t = AR.apply(ex, et, recs, recs[:, AR.W_M].copy().view(np.float32), cval=0.5)
        assert torch.equal(xo.cpu().view(torch.int32), want_x.view(torch.int32)) and torch.equal(to.cpu(), want_t)
        outs.append((xo.clone(), field))
    assert not torch.equal(outs[0][0], outs[1][0]) and not np.array_equal(outs[0][1], outs[1][1])
    eager = _aug(seed=77, da_prob=0.8, affine_mode="reflect", elastic=dict(alpha=(6, 10), sigma=2.0, mode="edge"), **AFFINE, **REST)
    eager.counter.fill_(2)                                                 # the eager call with the second replay's counter value
    ex, _ = eager(x, t)
    assert torch.equal(ex.view(torch.int32), outs[1][0].view(torch.int32))


# ---- 8. past 2 GiB ----------------------------------------------------------------------------------------------------------------------------
def test_batch_past_2gib():
    """17 x 128^3 x 16 fp32 = 2.28 GB in, in the scratch and out (the shape of test_warp_gpu.test_batch_past_2gib): the last sample's byte offsets
    lie past 2^31.  The last sample against the twin, bit for bit."""
    B, N, C = 17, 128, 16
    try:
        x = torch.empty(B, N, N, N, C, device="cuda")
        for b in range(B):
            x[b].normal_(generator=torch.Generator(device="cuda").manual_seed(b))
        t = torch.randint(0, 256, (B, N, N, N, 1), device="cuda", dtype=torch.uint8)
        last = ER.smooth(ER.noise(3, 0, 1, N, N), 4.0)
        field = torch.zeros(B, 2, N, N, device="cuda")
        field[B - 1] = _dev(last[0])
        field[0] = _dev(last[0, ::-1])
        rec = ER.make_records([60.0] * B)
        xo, to = _aug(elastic=dict(mode="reflect"))(x, t, elastic_records=_dev(rec), elastic_field=field)
        assert x.numel() * 4 > 2 ** 31
        want_x, want_t = ER.apply(x[B - 1:].cpu(), t[B - 1:].cpu(), rec[B - 1:], last, "reflect")
        assert torch.equal(xo[B - 1:].cpu().view(torch.int32), want_x.view(torch.int32))
        assert torch.equal(to[B - 1:].cpu(), want_t)
        assert not torch.equal(xo[B - 1], x[B - 1]) and not torch.equal(xo[0], xo[B - 1])        # deformed, and the samples' own data
    finally:
        x = t = xo = to = field = None
        torch.cuda.empty_cache()


# ---- 9. train_one_epoch -----------------------------------------------------------------------------------------------------------------------
def test_train_one_epoch_trains_on_the_deformed_pair():
    """Four replayed steps with ``augment=DeviceAugmenter(elastic=...)``: ``metric_function`` sees, step by step, the targets elastic_ref.apply gives
    for the loader's targets under the twin's records and field for counter = step, which the device's equal; the parameters end up elsewhere
    than without the augmenter."""
    from biapy_amd import train_engine as TE
    from biapy_amd.losses import BCEWithLogitsLoss
    from biapy_amd.resunet import ResUNet

    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(2, 32, 32, 32, 1, generator=g), (torch.rand(2, 32, 32, 32, 1, generator=g) > 0.5).float()) for _ in range(4)]
    cfg = types.SimpleNamespace(DATA=types.SimpleNamespace(PATCH_SIZE=(32, 32, 32, 1)),
                                TRAIN=types.SimpleNamespace(GRADIENT_CLIP_NORM=0.0, LR_SCHEDULER=types.SimpleNamespace(NAME=""), VERBOSE=False))

    def run(aug):
        torch.manual_seed(0)
        m = ResUNet(image_shape=(32, 32, 32, 1), activation="elu", feature_maps=[16, 32], drop_values=[0.0, 0.0], normalization="in", yx_down=[2],
                    z_down=[2], isotropy=[True, True], larger_io=False, conv_layers=[2, 2], compute_dtype=torch.float32).cuda().train()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, capturable=True)
        seen = []

        def metric(outputs, targets, metric_logger=None):
            seen.append((targets.detach().clone(), None if aug is None else (aug.last_elastic_records.clone(), aug.last_elastic_field.clone())))

        TE.train_one_epoch(cfg, m, None, BCEWithLogitsLoss(), metric, None, data, [opt], torch.device("cuda"), 0, loss_names=["loss"], graph="on", augment=aug)
        torch.cuda.synchronize()
        assert hasattr(m, "_bpx_graph_step")
        return [p.detach().clone() for p in m.parameters()], seen

    aug = _aug(seed=31, da_prob=0.75, elastic=dict(alpha=(8, 12), sigma=3.0, mode="reflect"))
    p_aug, seen = run(aug)
    p_plain, _ = run(None)
    assert int(aug.counter) == 4 and len(seen) == 4
    fired = 0
    for step, ((tgt_seen, (erec, field)), (_, tgt)) in enumerate(zip(seen, data)):
        want_rec, want_field = ER.draw(31, step, 2, aug.elastic_config()), ER.smooth(ER.noise(31, step, 2, 32, 32), 3.0)
        assert np.array_equal(erec.cpu().numpy(), want_rec) and np.array_equal(_bits(field.cpu().numpy()), _bits(want_field))
        fired += int(want_rec[:, 0].sum())
        want = ER.apply(tgt, tgt, want_rec, want_field, "reflect")[1]
        assert tgt_seen.shape == (2, 1, 32, 32, 32) and torch.equal(_mem(tgt_seen, True).cpu(), want), step
    assert fired > 0
    assert max((p - q).abs().max().item() for p, q in zip(p_aug, p_plain)) > 0

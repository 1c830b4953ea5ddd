"""Device augmentation on the MI355X (biapy_amd/augment.py, csrc/augment.hip) against its statement: geometry bit for bit against torch.rot90 /
torch.flip, the drawn records bit for bit against the host twin (tests/augment_ref.py), the fp64 mean, the intensity steps bit for bit against torch
fp32 operations on the CPU, the noise statistics, ``out=``, graph capture, a batch past 2 GiB and ``train_one_epoch(augment=...)``.
Measured figures of the mean, noise and training cases go to profiles/augment_values.txt."""
import os
import types

import numpy as np
import pytest
import torch

import augment_ref as AR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = os.path.join(ROOT, "profiles", "augment_values.txt")
_rows = {}

S1 = (3, 5, 72, 72)          # 72 crosses the 16-, 32- and 64-wide tiles with a remainder; odd Z; B no power of two
S2 = (2, 6, 24, 40)          # non-square: no rot90
S3 = (2, 40, 40)             # 2-D
S4 = (2, 3, 18, 18)          # rows of 18 voxels: no multiple of 4 elements at 1 or 3 channels, so the kernel takes its element-wise accesses
ALL_ON = dict(rot90=True, zflip=True, vflip=True, hflip=True, brightness=(-0.1, 0.3), contrast=(-0.2, 0.2), gaussian_noise=(0.01, 0.05),
              cutout=dict(n=(1, 4), size=(0.05, 0.3), cval=0.5))


def _record(key, text):
    """profiles/augment_values.txt: one row per measured case, rewritten whole so that a partial run leaves a readable file."""
    _rows[key] = text
    try:
        with open(VALUES, "w") as f:
            f.write("biapy_amd.augment on the device: what tests/test_augment_gpu.py measured (bounds: the test's docstrings, tests/augment_ref.py)\n")
            for k in sorted(_rows):
                f.write(_rows[k] + "\n")
    except OSError:
        pass


def _aug(**kw):
    from biapy_amd.augment import DeviceAugmenter

    return DeviceAugmenter(**kw)


def _first(mem):
    """The (B,C,[Z,]Y,X) permuted view of (B,[Z,]Y,X,C) memory - what train_engine.to_pytorch_format produces."""
    return mem.permute(0, mem.dim() - 1, *range(1, mem.dim() - 1))


def _mem(v, first):
    return v.permute(0, *range(2, v.dim()), 1) if first else v


def _pair(shape, C, Ct, tdtype, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(*shape, C, generator=g, device="cuda")
    t = torch.randint(0, 256, (*shape, Ct), generator=g, device="cuda").to(tdtype)
    return x, t


def _records(rows):
    return torch.from_numpy(np.stack(rows)).cuda()


def _geometry_ref(mem, recs):
    """torch.rot90 / torch.flip on the device, sample by sample (2-D batches as Z = 1)."""
    v = mem.unsqueeze(1) if mem.dim() == 4 else mem
    out = torch.stack([AR.geometry(v[b], recs[b]) for b in range(v.shape[0])])
    return out.squeeze(1) if mem.dim() == 4 else out


# ---- 1. geometry --------------------------------------------------------------------------------------------------------------------------------------
COMBOS = [dict(k=k, zflip=bool(f & 1), vflip=bool(f & 2), hflip=bool(f & 4)) for k in range(4) for f in range(8)]


@pytest.mark.parametrize("first", [False, True], ids=["channels_last", "permuted_view"])
@pytest.mark.parametrize("tdtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("C, Ct", [(1, 1), (1, 2), (3, 2), (16, 1)])
def test_geometry_bit_for_bit_s1(C, Ct, tdtype, first):
    """All 32 combinations of k and the three flips through ``records=``: torch.equal against torch.rot90 / torch.flip on the device."""
    x, t = _pair(S1, C, Ct, tdtype)
    xin, tin = (_first(x), _first(t)) if first else (x, t)
    aug = _aug()
    combos = COMBOS + [COMBOS[0]]                                         # 33 = 11 batches of 3
    for i in range(0, len(combos), 3):
        recs = [AR.make_record(**c) for c in combos[i:i + 3]]
        xo, to = aug(xin, tin, records=_records(recs))
        assert xo.shape == xin.shape and to.shape == tin.shape and xo.stride() == xin.stride() and to.dtype == tdtype
        assert torch.equal(_mem(xo, first), _geometry_ref(x, recs)), combos[i:i + 3]
        assert torch.equal(_mem(to, first), _geometry_ref(t, recs)), combos[i:i + 3]
    assert int(aug.counter) == 0                                           # given records: nothing is drawn, the counter stays


@pytest.mark.parametrize("tdtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("C, Ct", [(1, 1), (3, 2), (16, 1)])
def test_geometry_bit_for_bit_nonsquare_and_2d(C, Ct, tdtype):
    x, t = _pair(S2, C, Ct, tdtype, seed=1)
    aug = _aug()
    flips = [c for c in COMBOS if c["k"] == 0]
    for i in range(0, 8, 2):
        recs = [AR.make_record(**c) for c in flips[i:i + 2]]
        xo, to = aug(_first(x), t, records=_records(recs))                # mixed views: each output comes back in the view of its input
        assert torch.equal(_mem(xo, True), _geometry_ref(x, recs)) and torch.equal(to, _geometry_ref(t, recs))
    # an odd k cannot apply to a non-square plane: such a record is applied with that bit cleared (include/biapy_amd.h)
    xo, to = aug(x, t, records=_records([AR.make_record(k=1, hflip=True), AR.make_record(k=3)]))
    want = [AR.make_record(k=0, hflip=True), AR.make_record(k=2)]
    assert torch.equal(xo, _geometry_ref(x, want)) and torch.equal(to, _geometry_ref(t, want))
    with pytest.raises(ValueError, match="rot90"):
        _aug(rot90=True)(x, t)
    x, t = _pair(S3, C, Ct, tdtype, seed=2)
    flat = [c for c in COMBOS if not c["zflip"]]
    for i in range(0, 16, 2):
        recs = [AR.make_record(**c) for c in flat[i:i + 2]]
        xo, to = aug(x, _first(t), records=_records(recs))
        assert xo.shape == x.shape and torch.equal(xo, _geometry_ref(x, recs)) and torch.equal(_mem(to, True), _geometry_ref(t, recs))


@pytest.mark.parametrize("tdtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("C, Ct", [(1, 1), (3, 2), (2, 1)])
def test_geometry_bit_for_bit_unaligned_rows(C, Ct, tdtype):
    """S4: image and target rows that are no multiple of 4 elements ((1, 1)), only the image's ((3, 2)), only the target's ((2, 1))."""
    x, t = _pair(S4, C, Ct, tdtype, seed=3)
    aug = _aug()
    for i in range(0, 32, 2):
        recs = [AR.make_record(**c) for c in COMBOS[i:i + 2]]
        xo, to = aug(x, t, records=_records(recs))
        assert torch.equal(xo, _geometry_ref(x, recs)) and torch.equal(to, _geometry_ref(t, recs)), COMBOS[i:i + 2]


def test_nothing_fired_is_the_input_bit_for_bit():
    x, t = _pair(S1, 3, 2, torch.uint8)
    x[0, 0, 0, 0, 0], x[1, 2, 3, 4, 1], x[2, 4, 71, 71, 2] = float("nan"), float("inf"), -0.0       # a permutation of bits, whatever they are
    for aug in (_aug(da_prob=0.0, **ALL_ON), _aug()):
        xo, to = aug(x, t)
        assert torch.equal(xo.view(torch.int32), x.view(torch.int32)) and torch.equal(to, t)
        assert xo.data_ptr() != x.data_ptr() and int(aug.counter) == 1


def test_layouts_that_are_refused():
    x, t = _pair(S1, 3, 1, torch.float32)
    aug = _aug(hflip=True)
    for bad in (x[:, :, ::2], x.permute(0, 2, 1, 3, 4), x[..., :2]):
        with pytest.raises(ValueError, match="permuted view"):
            aug(bad, t)
    for bad_x, bad_t, word in ((x.double(), t, "float32"), (x, t.half(), "float32 or uint8"), (x, t[:2], "same"), (x, t[:, :, :40].contiguous(), "same"),
                               (torch.zeros(1, 4, 8, 8, 17, device="cuda"), torch.zeros(1, 4, 8, 8, 1, device="cuda"), "1 to 16"),
                               (torch.zeros(1, 4, 8, 8, 1, device="cuda"), torch.zeros(1, 4, 8, 8, 9, device="cuda"), "1 to 8")):
        with pytest.raises(ValueError, match=word):
            aug(bad_x, bad_t)
    with pytest.raises(ValueError, match="records"):
        aug(x, t, records=torch.zeros(2, 32, dtype=torch.int32, device="cuda"))
    assert int(aug.counter) == 0                                           # every refusal came before any launch


# ---- 2. draws -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [S1, (1500, 8, 8)], ids=["S1", "B1500"])
def test_draws_are_the_host_twins(shape):
    """``last_records`` of three consecutive calls, everything enabled, against augment_ref.draw with the same seed and counter - every word but
    the mean (word 4, the statistics pass).  B = 1500 takes more than one workgroup of the draw kernel."""
    x, t = _pair(shape, 1, 1, torch.uint8)
    aug = _aug(seed=0x1234567887654321, **ALL_ON)
    zyx = (1, *shape[1:]) if len(shape) == 3 else shape[1:]
    assert int(aug.counter) == 0
    for call in range(3):
        aug(x, t)
        got = aug.last_records.cpu().numpy()
        want = AR.draw(aug.seed, call, shape[0], zyx, aug.config())
        keep = [w for w in range(32) if w != AR.W_M]
        assert got.shape == (shape[0], 32) and got.dtype == np.int32
        assert np.array_equal(got[:, keep], want[:, keep]), np.argwhere(got[:, keep] != want[:, keep])[:5]
        assert int(aug.counter) == call + 1                                # exactly one per call
    assert int(aug._state[1]) == 0                                         # the draw kernel's ticket is back at zero


# ---- 3. mean ------------------------------------------------------------------------------------------------------------------------------------------
def test_sample_mean_in_record_word_4():
    """m = fp32(S / n) with S the fp64 sum of the n elements of a sample.  Any order of n - 1 fp64 additions leaves |S - sum| <= (n - 1) 2^-53 sum|x|
    to first order, the division adds half an fp64 ulp, so the fp64 quotient is within n 2^-53 mean|x| of the true mean; rounding it to fp32 moves it
    by at most half an fp32 ulp, and the fp64 torch mean it is compared with carries the same kind of error, far below the other half ulp.  Hence
    |m - mean64| <= ulp32(mean) + n 2^-53 mean|x|.  The summation order is fixed: two calls give the same bits."""
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(*S1, 3, generator=g, device="cuda") * 2 + torch.tensor([0.7, -130.0, 1e-3], device="cuda").view(3, 1, 1, 1, 1)
    t = torch.zeros(*S1, 1, dtype=torch.uint8, device="cuda")
    aug = _aug(contrast=(-0.2, 0.2), seed=4)
    aug(x, t)
    m1 = aug.last_records[:, AR.W_M].clone().view(torch.float32).cpu().numpy()
    aug(x, t)
    m2 = aug.last_records[:, AR.W_M].clone().view(torch.float32).cpu().numpy()
    assert np.array_equal(m1.view(np.int32), m2.view(np.int32))
    n = x[0].numel()
    worst = 0.0
    for b in range(S1[0]):
        mean = x[b].double().mean().item()
        bound = float(np.spacing(np.float32(abs(mean)))) + n * 2.0 ** -53 * x[b].double().abs().mean().item()
        err = abs(float(m1[b]) - mean)
        worst = max(worst, err / bound)
        print(f"sample {b}: m = {m1[b]!r}, fp64 mean = {mean!r}, err = {err:.3e}, bound = {bound:.3e}")
        assert err <= bound
    _record("3_mean", f"case 3 mean: S1 C=3, n = {n} per sample: worst |m - fp64 mean| / (ulp32 + n 2^-53 mean|x|) = {worst:.4f}")
    # no contrast: the statistics pass does not run and word 4 stays 0
    quiet = _aug(brightness=(0.1, 0.1), seed=4)
    quiet(x, t)
    assert not quiet.last_records[:, AR.W_M].any()


# ---- 4. intensity and cutout --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("apply_to_mask", [False, True], ids=["image_only", "mask_too"])
def test_intensity_and_cutout_bit_for_bit(apply_to_mask):
    """Drawn records, everything on (seed 122: its first two calls hold samples with contrast alone, contrast + brightness + a box, an odd k, and
    noise with boxes - asserted below).  Where noise did not fire the image is augment_ref.apply, evaluated with torch fp32 operations on the CPU and
    the device's own m, bit for bit; where it fired the cutout voxels are cval; the target is bit for bit everywhere."""
    x, t = _pair(S1, 3, 2, torch.uint8, seed=6)
    cut = dict(ALL_ON["cutout"], apply_to_mask=apply_to_mask)
    aug = _aug(seed=122, **dict(ALL_ON, cutout=cut))
    seen = []
    for call in range(2):
        xo, to = aug(x, t)
        recs = aug.last_records.cpu().numpy()
        assert np.array_equal(np.delete(recs, AR.W_M, 1), np.delete(AR.draw(122, call, S1[0], S1[1:], aug.config()), AR.W_M, 1))
        m = recs[:, AR.W_M].copy().view(np.float32)
        want_x, want_t = AR.apply(x.cpu(), t.cpu(), recs, m, cval=0.5, apply_to_mask=apply_to_mask)
        inside = AR.box_mask(recs, S1[1:])
        xo, to = xo.cpu(), to.cpu()
        assert torch.equal(to, want_t)
        if not apply_to_mask:
            assert torch.equal(to, _geometry_ref(t, recs).cpu())            # the target only moved
        for b in range(S1[0]):
            p = AR.parse(recs[b])
            seen.append(p)
            assert (xo[b][inside[b]] == 0.5).all()
            if apply_to_mask:
                assert not to[b][inside[b]].any()
            if not p["noise"]:
                assert torch.equal(xo[b], want_x[b]), (call, b, p)
            else:                                                          # noise: |n| <= sqrt(48 ln 2) bounds the distance outside the boxes
                d = (xo[b] - want_x[b])[~inside[b]].abs().max().item()
                assert 0 < d <= float(p["s"]) * 5.77 + 1e-5
    quiet = [p for p in seen if not p["noise"]]
    assert any(p["contrast"] and p["brightness"] and p["nbox"] for p in quiet) and any(p["contrast"] and not p["brightness"] for p in quiet)
    assert any(p["k"] % 2 for p in quiet) and any(p["noise"] and p["nbox"] for p in seen)


def test_fired_steps_are_applied_and_skipped_steps_are_not():
    """(v - m) * 1 + m is not v: a contrast that fired with a = 1 changes bits, one that did not fire leaves them."""
    x, t = _pair(S1, 1, 1, torch.float32, seed=7)
    aug = _aug()
    recs = [AR.make_record(a=1.0), AR.make_record(), AR.make_record(b=0.0)]
    xo, _ = aug(x, t, records=_records(recs))
    m = aug.last_records[:, AR.W_M].cpu().numpy().view(np.float32)
    want, _ = AR.apply(x.cpu(), t.cpu(), np.stack(recs), m)
    assert torch.equal(xo.cpu(), want) and torch.equal(xo[1], x[1]) and torch.equal(xo[2], x[2]) and not torch.equal(xo[0], x[0])


# ---- 5. noise -----------------------------------------------------------------------------------------------------------------------------------------
def test_noise_statistics_and_determinism():
    """Zeros image, noise only, da_prob = 1, s = 0.25 (lo == hi), S1 with C = 3: d = out / s is exact.  Five-sigma conditions of n = 233,280 standard
    normals on a fixed seed (tests/augment_ref.noise_bounds; test_augment_cpu checks that a correct generator meets them with this seed), and
    max |d| <= sqrt(48 ln 2) + 1e-3, the Box-Muller ceiling of a 24-bit uniform."""
    x = torch.zeros(*AR.NOISE_SHAPE, device="cuda")
    t = torch.zeros(*AR.NOISE_SHAPE[:-1], 1, dtype=torch.uint8, device="cuda")
    aug = _aug(da_prob=1.0, gaussian_noise=(0.25, 0.25), seed=AR.NOISE_SEED)
    xo, _ = aug(x, t)
    first = xo.clone()
    assert all(AR.parse(r)["noise"] and AR.parse(r)["s"] == 0.25 for r in aug.last_records.cpu().numpy())
    d = (first.double() / 0.25).cpu().numpy()
    st, bd = AR.noise_stats(d), AR.noise_bounds(d.size)
    print("device noise statistics:", st, "bounds:", bd)
    _record("5_noise", "case 5 noise: n = {n}: mean {mean:.3e} (<= {bm:.3e}), var - 1 {v:.3e} (<= {bv:.3e}), lag-1 {lag1:.3e}, samples 0/1 {cross:.3e} "
            "(<= {bl:.3e}), max |d| {max:.4f} (<= {bx:.4f})".format(bm=bd["mean"], v=st["var"] - 1, bv=bd["var"], bl=bd["lag1"], bx=bd["max"], **st))
    assert st["n"] == 233280 and np.isfinite(d).all()
    assert abs(st["mean"]) <= bd["mean"]
    assert abs(st["var"] - 1) <= bd["var"]
    assert abs(st["lag1"]) <= bd["lag1"] and abs(st["cross"]) <= bd["cross"]
    assert st["max"] <= bd["max"]
    # the keying is (seed, counter, sample, output element): the host twin's stream through NumPy's Box-Muller gives the same values up to the
    # device's fp32 log / sqrt / sin / cos (a few ulp of values below 6: 1e-4 is far above that and far below the spacing of distinct draws)
    per = int(np.prod(AR.NOISE_SHAPE[1:]))
    host = np.stack([AR.noise_normals(AR.NOISE_SEED, 0, b, per) for b in range(AR.NOISE_SHAPE[0])]).reshape(AR.NOISE_SHAPE)
    assert np.abs(d - host).max() <= 1e-4
    # rows of 18 elements: the element-wise path picks its value out of the same Philox blocks
    xs, ts = torch.zeros(*S4, 1, device="cuda"), torch.zeros(*S4, 1, dtype=torch.uint8, device="cuda")
    small, _ = _aug(da_prob=1.0, gaussian_noise=(0.25, 0.25), seed=AR.NOISE_SEED)(xs, ts)
    host = np.stack([AR.noise_normals(AR.NOISE_SEED, 0, b, xs[0].numel()) for b in range(S4[0])]).reshape(xs.shape)
    assert np.abs((small.double() / 0.25).cpu().numpy() - host).max() <= 1e-4
    xo2, _ = aug(x, t)                                                     # the next call: counter 1
    assert not torch.equal(xo2, first)
    twin = _aug(da_prob=1.0, gaussian_noise=(0.25, 0.25), seed=AR.NOISE_SEED)
    xo3, _ = twin(x, t)                                                    # same seed and counter: the same bits
    assert torch.equal(xo3, first)


# ---- 6. out= ------------------------------------------------------------------------------------------------------------------------------------------
def test_out_tensors_and_overlap():
    x, t = _pair(S1, 3, 1, torch.float32, seed=8)
    recs = _records([AR.make_record(k=1, b=0.5), AR.make_record(hflip=True, boxes=[(1, 2, 3, 2, 30, 40)]), AR.make_record(k=2, zflip=True)])
    aug = _aug()
    want_x, want_t = aug(_first(x), _first(t), records=recs)
    xo, to = torch.empty_like(x), torch.empty_like(t)
    got = aug(_first(x), _first(t), out=(_first(xo), _first(to)), records=recs)
    assert got[0].data_ptr() == xo.data_ptr() and got[1].data_ptr() == to.data_ptr() and got[0].shape == _first(x).shape
    assert torch.equal(_first(xo), want_x) and torch.equal(_first(to), want_t)
    fresh = _aug(hflip=True)
    for out in ((x, to), (xo, t), (x, t)):
        with pytest.raises(ValueError, match="overlap"):
            fresh(x, t, out=out)
    big = torch.zeros(x.numel() + 8, device="cuda")
    with pytest.raises(ValueError, match="overlap"):                      # a shifted alias of the input's memory
        fresh(big[:x.numel()].view(x.shape), t, out=(big[8:].view(x.shape), to))
    for out, word in (((xo.double(), to), "out\\[0\\]"), ((xo, to[:2]), "out\\[1\\]"), ((_first(xo), to), "out\\[0\\]"), (xo, "pair")):
        with pytest.raises(ValueError, match=word):
            fresh(x, t, out=out)
    assert int(fresh.counter) == 0                                         # refused before any launch


# ---- 7. graph -----------------------------------------------------------------------------------------------------------------------------------------
def test_captured_call_draws_anew_at_every_replay():
    x, t = _pair(S1, 3, 2, torch.uint8, seed=9)
    xo, to = torch.empty_like(x), torch.empty_like(t)
    a, b = _aug(seed=77, **ALL_ON), _aug(seed=77, **ALL_ON)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a(x, t, out=(xo, to))                                              # the first call creates the augmenter's state: outside the capture
    torch.cuda.current_stream().wait_stream(side)
    b(x, t)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a(x, t, out=(xo, to))
    assert int(a.counter) == 1                                             # capturing ran nothing
    seen = []
    for i in range(3):
        g.replay()
        ex, et = b(x, t)
        assert torch.equal(a.last_records, b.last_records)
        assert torch.equal(xo.view(torch.int32), ex.view(torch.int32)) and torch.equal(to, et)
        seen.append(a.last_records.clone())
        assert int(a.counter) == i + 2
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ---- 8. past 2 GiB ------------------------------------------------------------------------------------------------------------------------------------
def test_batch_past_2gib():
    """17 x 128^3 x 16 fp32 = 2.28 GB in and out: byte offsets past 2^31 (and element offsets past 2^29) in image and target."""
    B, N, C = 17, 128, 16
    try:
        x = torch.empty(B, N, N, N, C, device="cuda")
        for b in range(B):
            x[b].normal_(generator=torch.Generator(device="cuda").manual_seed(b))
        t = torch.randint(0, 256, (B, N, N, N, 1), device="cuda", dtype=torch.uint8)
        recs = [AR.make_record(k=b % 4, zflip=bool(b & 4), vflip=bool(b & 8), hflip=bool(b & 16)) for b in range(B)]
        xo, to = _aug()(x, t, records=_records(recs))
        assert x.numel() * 4 > 2 ** 31
        for b in range(B):
            assert torch.equal(xo[b], AR.geometry(x[b], recs[b])), b
            assert torch.equal(to[b], AR.geometry(t[b], recs[b])), b
    finally:
        x = t = xo = to = None
        torch.cuda.empty_cache()


# ---- 9. train_one_epoch -------------------------------------------------------------------------------------------------------------------------------
def _resunet():
    from biapy_amd.resunet import ResUNet

    torch.manual_seed(0)
    return ResUNet(image_shape=(32, 32, 32, 1), activation="elu", feature_maps=[16, 32], drop_values=[0.0, 0.0], normalization="in", yx_down=[2],
                   z_down=[2], isotropy=[True, True], larger_io=False, conv_layers=[2, 2], compute_dtype=torch.float32).cuda().train()


def _train(graph, augment, pass_kw=True):
    from biapy_amd import train_engine as TE
    from biapy_amd.losses import BCEWithLogitsLoss

    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(2, 32, 32, 32, 1, generator=g), (torch.rand(2, 32, 32, 32, 1, generator=g) > 0.5).float()) for _ in range(4)]
    cfg = types.SimpleNamespace(DATA=types.SimpleNamespace(PATCH_SIZE=(32, 32, 32, 1)),
                                TRAIN=types.SimpleNamespace(GRADIENT_CLIP_NORM=0.0, LR_SCHEDULER=types.SimpleNamespace(NAME=""), VERBOSE=False))
    m = _resunet()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, capturable=True)
    seen = []

    def metric(outputs, targets, metric_logger=None):
        seen.append(targets.detach().clone())

    kw = dict(augment=_aug(seed=31, **ALL_ON) if augment else None) if pass_kw else {}
    TE.train_one_epoch(cfg, m, None, BCEWithLogitsLoss(), metric, None, data, [opt], torch.device("cuda"), 0, loss_names=["loss"], graph=graph, **kw)
    torch.cuda.synchronize()
    assert hasattr(m, "_bpx_graph_step") == (graph == "on")
    return [p.detach().clone() for p in m.parameters()], seen, data, kw.get("augment")


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(graph, augment, pass_kw=True):
        key = (graph, augment, pass_kw)
        if key not in cache:
            cache[key] = _train(graph, augment, pass_kw)
        return cache[key]

    return get


def _max_diff(a, b):
    return max((p - q).abs().max().item() for p, q in zip(a, b))


def test_train_one_epoch_augment_none_is_todays_step(runs):
    for graph in ("on", "off"):
        a, b = runs(graph, False)[0], runs(graph, False, pass_kw=False)[0]
        assert all(torch.equal(p, q) for p, q in zip(a, b)), graph


def test_train_one_epoch_trains_on_the_augmented_pair(runs):
    """Four steps with graph='on' and four with graph='off', augmenters of one seed: both ways see the same augmented targets (``metric_function``'s
    view, the host twin's geometry of the loader's targets), and end with parameters as close as the SAME runs without augmentation do on this
    device, within a factor of 2."""
    p_on, seen_on, data, aug_on = runs("on", True)
    p_off, seen_off, _, aug_off = runs("off", True)
    assert int(aug_on.counter) == int(aug_off.counter) == 4 and len(seen_on) == len(seen_off) == 4
    for step, (s_on, s_off, (_, tgt)) in enumerate(zip(seen_on, seen_off, data)):
        assert torch.equal(s_on, s_off)
        recs = AR.draw(31, step, 2, (32, 32, 32), aug_on.config())
        assert s_on.shape == (2, 1, 32, 32, 32) and torch.equal(_mem(s_on, True).cpu(), AR.apply(tgt, tgt, recs, np.zeros(2, np.float32))[1])
    base = _max_diff(runs("on", False)[0], runs("off", False)[0])
    with_aug = _max_diff(p_on, p_off)
    moved = _max_diff(p_on, runs("on", False)[0])
    print(f"max |graph on - graph off| over all parameters after 4 steps: {base:.3e} without augmentation, {with_aug:.3e} with; "
          f"augmented vs plain run: {moved:.3e}")
    _record("9_train", f"case 9 train_one_epoch, 32^3 batch 2, 4 steps: max |graph on - off| = {base:.3e} without augmentation, {with_aug:.3e} with "
            f"(allowed: 2 x the former); augmented vs plain parameters differ by {moved:.3e}")
    assert moved > 0 and _max_diff(p_off, runs("off", False)[0]) > 0
    assert with_aug <= 2 * base

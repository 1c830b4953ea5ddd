"""The affine warp of the device augmenter on the MI355X (biapy_amd/augment.py step 0, csrc/augment.hip) against its statement: ``bpx_warp_apply``
bit for bit against the host twin (tests/warp_ref.py) for given warp records, the drawn flags and parameters bit for bit and the matrix words within
the derived bound of the fp64 statement, the full call against the two twins composed, ``out=``, graph capture, a batch past 2 GiB and
``train_one_epoch(augment=...)``.  Err / bound of the drawn matrices goes to profiles/warp_values.txt."""
import os
import types

import numpy as np
import pytest
import torch

import augment_ref as AR
import warp_ref as WR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = os.path.join(ROOT, "profiles", "warp_values.txt")
_rows = {}

MODES = ["constant", "reflect", "edge"]
AFFINE = dict(rotation=(-30, 45), zoom=(0.8, 1.25), shear=(-10, 12), shift=(-0.1, 0.2))
# everything of the existing augmenter but the noise (its samples are the device's own; tests/test_augment_gpu.py covers them)
REST = dict(rot90=True, zflip=True, vflip=True, hflip=True, brightness=(-0.1, 0.3), contrast=(-0.2, 0.2), cutout=dict(n=(1, 4), size=(0.05, 0.3), cval=0.5))
# (B, Z, Y, X): the issue's shape; one voxel along Y, along X (2-D batches); rows of an odd number of elements at 1 and 3 channels on a square
# plane; 2 x 3 tiles of 32 with a partial tile in Y and in X; the same on a square plane (the quarter turn against torch.rot90)
SHAPES = [(3, 2, 20, 24), (2, 1, 1, 37), (2, 1, 37, 1), (2, 2, 11, 11), (1, 1, 40, 70), (1, 1, 40, 40)]


def _record(key, text):
    """profiles/warp_values.txt: one row per measured case, rewritten whole so that a partial run leaves a readable file."""
    _rows[key] = text
    try:
        with open(VALUES, "w") as f:
            f.write("biapy_amd.augment, the affine warp on the device: what tests/test_warp_gpu.py measured (bound: tests/warp_ref.py)\n")
            for k in sorted(_rows):
                f.write(_rows[k] + "\n")
    except OSError:
        pass


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


def _matrices(Y, X):
    """The five matrices of the issue as warp records for a (Y, X) plane: a 33 degree rotation, a zoom-out x0.15 shifted by 3 extents (its taps lie
    several reflect periods away), a 20 degree shear, the identity and the quarter turn [[0, 1], [-1, 0]]."""
    rot = WR.matrix64(np.float32([[33, 1, 0, 0, 0]]), Y, X)[0]
    far = WR.matrix64(np.float32([[0, 0.15, 0, 3, -3]]), Y, X)[0]
    shear = WR.matrix64(np.float32([[0, 1, 20, 0, 0]]), Y, X)[0]
    return [WR.make_record(rot, WR.F_ROT, (33, 1, 0, 0, 0)), WR.make_record(far, WR.F_ZOOM | WR.F_SHIFT, (0, 0.15, 0, 3, -3)),
            WR.make_record(shear, WR.F_SHEAR, (0, 1, 20, 0, 0)), WR.make_record([[1, 0], [0, 1]], plane=(Y, X)),
            WR.make_record([[0, 1], [-1, 0]], plane=(Y, X), params=(90, 1, 0, 0, 0))]


def _dev(rows):
    return torch.from_numpy(np.stack(rows)).cuda()


# ---- 1. the apply, bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("first", [False, True], ids=["channels_last", "permuted_view"])
@pytest.mark.parametrize("tdtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("C, Ct", [(1, 1), (3, 2), (16, 8)])
def test_apply_bit_for_bit(C, Ct, tdtype, first, mode):
    """Every element of image and target, every shape of SHAPES (2-D ones as 4-D batches), every matrix of ``_matrices``: torch.equal on the bits
    against warp_ref.apply.  The twin reproduces every coordinate in fp32, so there is no tie band and nothing is excluded."""
    aug = _aug(affine_mode=mode, affine_cval=0.75)
    for si, shape in enumerate(SHAPES):
        B, Z, Y, X = shape
        x, t = _pair(shape, C, Ct, tdtype, seed=si)
        flat = Z == 1 and min(Y, X) > 1                                    # a 2-D batch (B, Y, X, C); an axis of one voxel keeps its Z = 1 (with one
        if flat:                                                           # channel too, a 4-D (B, n, 1, 1) would read as n channels)
            xin, tin = x[:, 0], t[:, 0]
        else:
            xin, tin = x, t
        if first:
            xin, tin = _first(xin), _first(tin)
        mats = _matrices(Y, X)
        mats += mats[:(-len(mats)) % B]                                    # whole batches
        for i in range(0, len(mats), B):
            recs = mats[i:i + B]
            xo, to = aug(xin, tin, warp_records=_dev(recs))
            assert xo.shape == xin.shape and xo.stride() == xin.stride() and to.dtype == tdtype
            xo, to = _mem(xo, first), _mem(to, first)
            if flat:
                xo, to = xo.unsqueeze(1), to.unsqueeze(1)
            want_x, want_t = WR.apply(x.cpu(), t.cpu(), np.stack(recs), mode, cval=0.75)
            assert torch.equal(xo.cpu().view(torch.int32), want_x.view(torch.int32)), (shape, i)
            assert torch.equal(to.cpu(), want_t), (shape, i)
            for b, r in enumerate(recs):
                if Y == X and r is mats[4]:                                # the exact quarter turn is torch.rot90, in every mode
                    assert torch.equal(xo[b], torch.rot90(x[b], 1, dims=(1, 2))) and torch.equal(to[b], torch.rot90(t[b], 1, dims=(1, 2)))
                if r is mats[3]:
                    assert torch.equal(xo[b], x[b]) and torch.equal(to[b], t[b])
    assert int(aug.counter) == 2 + 3 * 3 + 2 * 5                          # one draw of the (empty) augmentation record per call, no more


def test_flags_zero_is_the_input_bit_for_bit():
    x, t = _pair((3, 2, 40, 40), 3, 2, torch.uint8)
    x[0, 0, 0, 0, 0], x[1, 1, 3, 4, 1], x[2, 1, 39, 39, 2] = float("nan"), float("inf"), -0.0     # a copy of bits, whatever they are
    wild = [WR.make_record([7, -3, 1e5, 0.1, 9, -1e5], flags=0) for _ in range(3)]                # flags 0: the matrix words are not looked at
    for mode in MODES:
        xo, to = _aug(affine_mode=mode, affine_cval=5.0)(x, t, warp_records=_dev(wild))
        assert torch.equal(xo.view(torch.int32), x.view(torch.int32)) and torch.equal(to, t) and xo.data_ptr() != x.data_ptr()
    aug = _aug(da_prob=0.0, **AFFINE, **REST)                              # nothing fires: warp and gather both copy
    xo, to = aug(x, t)
    assert torch.equal(xo.view(torch.int32), x.view(torch.int32)) and torch.equal(to, t)
    assert not aug.last_warp_records[:, 0].any() and int(aug.counter) == 1


# ---- 2. draws ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 24, 24), (1500, 8, 8)], ids=["B3", "B1500"])
def test_draws_are_the_host_twins(shape):
    """8 consecutive calls with everything on.  Warp records: flags and words 8-12 equal warp_ref.draw bit for bit, words 7 and 13-15 are 0, words
    1-6 lie within warp_ref.matrix_bound of the fp64 statement (err / bound goes to profiles/warp_values.txt).  The augmentation records of the same
    calls are what augment_ref.draw gives for an augmenter without the affine options: the existing streams did not move."""
    x, t = _pair(shape, 1, 1, torch.uint8)
    aug = _aug(seed=0x1234567887654321, **AFFINE, **REST)
    B = shape[0]
    zyx = (1, *shape[1:]) if len(shape) == 3 else shape[1:]
    worst = np.zeros(6)
    fired = np.zeros(4, dtype=np.int64)
    for call in range(8):
        aug(x, t)
        got = aug.last_warp_records.cpu().numpy()
        assert got.shape == (B, 16) and got.dtype == np.int32
        flags, params = WR.draw(aug.seed, call, B, aug.warp_config())
        assert np.array_equal(got[:, 0].view(np.uint32), flags), call
        assert np.array_equal(got[:, 8:13], params.view(np.int32)), np.argwhere(got[:, 8:13] != params.view(np.int32))[:5]
        assert not got[:, 7].any() and not got[:, 13:].any()
        m = got[:, 1:7].copy().view(np.float32).astype(np.float64)
        ratio = np.abs(m - WR.matrix64(params, zyx[1], zyx[2])) / WR.matrix_bound(params, zyx[1], zyx[2])
        worst = np.maximum(worst, ratio.max(axis=0))
        print(f"call {call}: max err / bound per matrix word = {np.round(ratio.max(axis=0), 4).tolist()}")
        assert np.isfinite(ratio).all() and ratio.max() <= 1.0, (call, ratio.max())
        fired += [(flags & bit != 0).sum() for bit in (1, 2, 4, 8)]
        rec = aug.last_records.cpu().numpy()
        want = AR.draw(aug.seed, call, B, zyx, _aug(seed=aug.seed, **REST).config())
        keep = [w for w in range(32) if w != AR.W_M]
        assert np.array_equal(rec[:, keep], want[:, keep]), call
        assert int(aug.counter) == call + 1
    assert fired.min() > 0                                                  # every transform fired in the 8 calls, also at B = 3
    _record("draw_B%d" % B, f"draws, B = {B}, plane {zyx[1]} x {zyx[2]}, 8 calls: worst |word - fp64 statement| / bound of m00 m01 m02 m10 m11 m12 = "
            + " ".join(f"{v:.4f}" for v in worst) + f" (bound: 4 ulp assumed for sinf / cosf / tanf, safety {WR.SAFETY})")


# ---- 3. the full call -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_full_call_is_the_twins_composed(mode):
    """Warp, then rot90 / flips, then contrast, brightness and cutout, from drawn records of both kinds: warp_ref.apply followed by augment_ref.apply
    (with the device's own m), bit for bit.  m is the mean of the INPUT sample (bound: test_augment_gpu.test_sample_mean_in_record_word_4)."""
    shape = (3, 3, 40, 40)
    x, t = _pair(shape, 3, 2, torch.uint8, seed=11)
    x = x + 0.5
    aug = _aug(seed=122, da_prob=0.7, affine_mode=mode, affine_cval=-1.0, **AFFINE, **REST)
    warped, plain, moved = 0, 0, 0.0
    for call in range(3):
        xo, to = aug(x, t)
        recs, wrec = aug.last_records.cpu().numpy(), aug.last_warp_records.cpu().numpy()
        m = recs[:, AR.W_M].copy().view(np.float32)
        wx, wt = WR.apply(x.cpu(), t.cpu(), wrec, mode, cval=-1.0)
        want_x, want_t = AR.apply(wx, wt, recs, m, cval=0.5)
        assert torch.equal(xo.cpu().view(torch.int32), want_x.view(torch.int32)), call
        assert torch.equal(to.cpu(), want_t), call
        n = x[0].numel()
        for b in range(shape[0]):
            mean = x[b].double().mean().item()
            bound = float(np.spacing(np.float32(abs(mean)))) + n * 2.0 ** -53 * x[b].double().abs().mean().item()
            assert abs(float(m[b]) - mean) <= bound
            if wrec[b, 0]:
                warped += 1
                moved = max(moved, abs(wx[b].double().mean().item() - mean) / bound)
            else:
                plain += 1
    assert warped and moved > 10                                            # the warped sample's mean is another number: m is not taken from it
    print(f"{warped} warped samples, {plain} copied; the warped mean differs from m by up to {moved:.0f} bounds")


# ---- 4. out=, refusals ------------------------------------------------------------------------------------------------------------------------
def test_out_tensors_overlap_and_warp_records_refusals():
    shape = (3, 2, 20, 24)
    x, t = _pair(shape, 3, 1, torch.float32, seed=8)
    wrec = _dev(_matrices(20, 24)[:3])
    recs = _dev([AR.make_record(hflip=True, b=0.5), AR.make_record(zflip=True, boxes=[(0, 2, 3, 2, 10, 12)]), AR.make_record(k=2)])
    aug = _aug(affine_mode="reflect")
    want_x, want_t = aug(_first(x), _first(t), records=recs, warp_records=wrec)
    xo, to = torch.empty_like(x), torch.empty_like(t)
    got = aug(_first(x), _first(t), out=(_first(xo), _first(to)), records=recs, warp_records=wrec)
    assert got[0].data_ptr() == xo.data_ptr() and got[1].data_ptr() == to.data_ptr()
    assert torch.equal(_first(xo), want_x) and torch.equal(_first(to), want_t)
    wx, wt = WR.apply(x.cpu(), t.cpu(), wrec.cpu().numpy(), "reflect")
    tx, tt = AR.apply(wx, wt, recs.cpu().numpy(), aug.last_records[:, AR.W_M].cpu().numpy().view(np.float32))
    assert torch.equal(xo.cpu(), tx) and torch.equal(to.cpu(), tt)
    fresh = _aug(rotation=(-10, 10))
    for out in ((x, to), (xo, t), (x, t)):
        with pytest.raises(ValueError, match="overlap"):
            fresh(x, t, out=out)
    for bad, word in ((wrec[:2], "warp_records"), (wrec.to(torch.int64), "warp_records"), (wrec.cpu(), "warp_records"),
                      (torch.zeros(3, 32, dtype=torch.int32, device="cuda"), "warp_records")):
        with pytest.raises(ValueError, match=word):
            fresh(x, t, warp_records=bad)
    for value in (float("inf"), float("nan"), 2.0 ** 20 + 1, -1e9):
        rows = _matrices(20, 24)[:3]
        rows[1] = rows[1].copy()
        rows[1][1 + 2] = np.float32(value).view(np.int32)
        with pytest.raises(ValueError, match="words 1-6"):
            fresh(x, t, warp_records=_dev(rows))
    assert int(fresh.counter) == 0 and fresh.last_warp_records is None     # refused before any launch and any allocation


def test_scratch_is_kept_until_the_shape_changes():
    x, t = _pair((2, 2, 20, 24), 1, 1, torch.uint8)
    aug = _aug(rotation=(-10, 10), seed=1)
    aug(x, t)
    a, b, w = aug._wx.data_ptr(), aug._wt.data_ptr(), aug.last_warp_records.data_ptr()
    aug(x, t)
    assert (aug._wx.data_ptr(), aug._wt.data_ptr(), aug.last_warp_records.data_ptr()) == (a, b, w)
    aug(x, t.float())
    assert aug._wx.data_ptr() == a and aug._wt.dtype == torch.float32
    x2, t2 = _pair((2, 2, 24, 20), 1, 1, torch.uint8)
    aug(x2, t2)
    assert aug._wx.shape == x2.shape and aug._wt.dtype == torch.uint8
    plain = _aug(hflip=True, seed=1)                                        # no affine option: no warp state at all
    plain(x, t)
    assert plain._wx is None and plain._wt is None and plain.last_warp_records is None


# ---- 5. graph ---------------------------------------------------------------------------------------------------------------------------------
def test_captured_call_draws_anew_at_every_replay():
    shape = (3, 3, 40, 40)
    x, t = _pair(shape, 3, 2, torch.uint8, seed=9)
    xo, to = torch.empty_like(x), torch.empty_like(t)
    a = _aug(seed=77, da_prob=0.8, affine_mode="reflect", **AFFINE, **REST)
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
        flags, params = WR.draw(77, i + 1, shape[0], a.warp_config())      # the twin for this replay's counter value
        assert np.array_equal(wrec[:, 0].view(np.uint32), flags) and np.array_equal(wrec[:, 8:13], params.view(np.int32))
        keep = [w for w in range(32) if w != AR.W_M]
        assert np.array_equal(recs[:, keep], AR.draw(77, i + 1, shape[0], shape[1:], a.config())[:, keep])
        wx, wt = WR.apply(x.cpu(), t.cpu(), wrec, "reflect")
        want_x, want_t = AR.apply(wx, wt, recs, recs[:, AR.W_M].copy().view(np.float32), cval=0.5)
        assert torch.equal(xo.cpu().view(torch.int32), want_x.view(torch.int32)) and torch.equal(to.cpu(), want_t)
        outs.append((xo.clone(), wrec))
    assert not torch.equal(outs[0][0], outs[1][0]) and not np.array_equal(outs[0][1], outs[1][1])


# ---- 6. past 2 GiB ----------------------------------------------------------------------------------------------------------------------------
def test_batch_past_2gib():
    """17 x 128^3 x 16 fp32 = 2.28 GB in, in the scratch and out (the shape of test_augment_gpu.test_batch_past_2gib): the last sample's byte
    offsets lie past 2^31 (its element offsets past 2^29).  The last sample against the twin, bit for bit."""
    B, N, C = 17, 128, 16
    try:
        x = torch.empty(B, N, N, N, C, device="cuda")
        for b in range(B):
            x[b].normal_(generator=torch.Generator(device="cuda").manual_seed(b))
        t = torch.randint(0, 256, (B, N, N, N, 1), device="cuda", dtype=torch.uint8)
        rot = WR.matrix64(np.float32([[33, 1.1, 5, 0.05, -0.02]]), N, N)[0]
        recs = [WR.make_record(rot, 0xF, (33, 1.1, 5, 0.05, -0.02))] * B
        xo, to = _aug(affine_mode="reflect")(x, t, warp_records=_dev(recs))
        assert x.numel() * 4 > 2 ** 31
        want_x, want_t = WR.apply(x[B - 1:].cpu(), t[B - 1:].cpu(), recs[B - 1:], "reflect")
        assert torch.equal(xo[B - 1:].cpu().view(torch.int32), want_x.view(torch.int32))
        assert torch.equal(to[B - 1:].cpu(), want_t)
        assert not torch.equal(xo[0], xo[B - 1])                            # the samples' own data, not one sample's
    finally:
        x = t = xo = to = None
        torch.cuda.empty_cache()


# ---- 7. train_one_epoch -----------------------------------------------------------------------------------------------------------------------
def test_train_one_epoch_trains_on_the_warped_pair():
    """Four replayed steps with ``augment=DeviceAugmenter(rotation=...)``: ``metric_function`` sees, step by step, the targets warp_ref.apply gives
    for the loader's targets under the step's warp records, whose flags and angle are warp_ref.draw's for counter = step; the parameters end up
    elsewhere than without the augmenter."""
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
            seen.append((targets.detach().clone(), None if aug is None else aug.last_warp_records.clone()))

        TE.train_one_epoch(cfg, m, None, BCEWithLogitsLoss(), metric, None, data, [opt], torch.device("cuda"), 0, loss_names=["loss"], graph="on", augment=aug)
        torch.cuda.synchronize()
        assert hasattr(m, "_bpx_graph_step")
        return [p.detach().clone() for p in m.parameters()], seen

    aug = _aug(seed=31, da_prob=0.75, rotation=(-45, 45), affine_mode="reflect")
    p_aug, seen = run(aug)
    p_plain, _ = run(None)
    assert int(aug.counter) == 4 and len(seen) == 4
    fired = 0
    for step, ((tgt_seen, wrec), (_, tgt)) in enumerate(zip(seen, data)):
        wrec = wrec.cpu().numpy()
        flags, params = WR.draw(31, step, 2, aug.warp_config())
        assert np.array_equal(wrec[:, 0].view(np.uint32), flags) and np.array_equal(wrec[:, 8:13], params.view(np.int32))
        fired += int((flags != 0).sum())
        want = WR.apply(tgt, tgt, wrec, "reflect")[1]
        assert tgt_seen.shape == (2, 1, 32, 32, 32) and torch.equal(_mem(tgt_seen, True).cpu(), want), step
    assert fired > 0
    assert max((p - q).abs().max().item() for p, q in zip(p_aug, p_plain)) > 0

"""Device augmentation - what can be checked without a GPU: the entry points are declared, exported and bound; the constructor and ``from_cfg``
validate and map; the host twin's Philox4x32-10 reproduces Random123's known answers; ``augment_ref.draw`` keeps the record layout and its draws have
the stated properties; ``augment_ref.apply`` is a permutation for geometry-only records and the identity for clear ones; the noise seed of the
device test meets its five-sigma conditions under a correct generator."""
import os
import re
import types

import numpy as np
import pytest
import torch

import augment_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bpx_aug_draw", "bpx_aug_mean_blocks", "bpx_aug_mean", "bpx_aug_apply")


def test_entry_points_are_declared_exported_and_bound():
    from biapy_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    source = open(os.path.join(ROOT, "biapy_amd", "csrc", "augment.hip")).read()
    assert set(re.findall(r"\bbpx_aug_[a-z_]+(?=\()", source)) == set(NAMES)          # every bpx_aug_* entry of the source is one of these
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in L.EXPORTS and getattr(L.lib._raw, name) is not None, name
    assert "augment.hip" in open(os.path.join(ROOT, "biapy_amd", "csrc", "Makefile")).read()
    # the host-side argument checks answer without a device
    assert L.lib.bpx_aug_draw(None, 1, 1, 8, 8, None, None, None) != 0 and b"null pointer" in L.lib.bpx_last_error()
    assert L.lib.bpx_aug_mean(None, 1, 64, None, None, None) != 0 and b"null pointer" in L.lib.bpx_last_error()
    assert L.lib.bpx_aug_apply(16, 32, L.F32, 1, 1, 8, 8, 17, 1, 48, 0, 0.0, 0, 64, 80, None) != 0 and b"1..16 image channels" in L.lib.bpx_last_error()
    assert L.lib.bpx_aug_apply(16, 32, L.BF16, 1, 1, 8, 8, 1, 1, 48, 0, 0.0, 0, 64, 80, None) != 0 and b"float32 or uint8" in L.lib.bpx_last_error()
    assert L.lib.bpx_aug_apply(16, 32, L.F32, 1, 1, 8, 8, 1, 1, 48, 0, 0.0, 0, 16, 80, None) != 0 and b"in place" in L.lib.bpx_last_error()
    assert L.lib.bpx_aug_mean_blocks(1) == 1 and 1 <= L.lib.bpx_aug_mean_blocks(4 * 128 ** 3) <= 256
    # the record layout of the header is the one the module and the host twin use
    from biapy_amd import augment as A

    for macro, value in (("REC_WORDS", 32), ("MAX_BOXES", 4), ("F_ZFLIP", "0x1u"), ("F_VFLIP", "0x2u"), ("F_HFLIP", "0x4u"), ("K_SHIFT", 3),
                         ("F_CONTRAST", "0x20u"), ("F_BRIGHTNESS", "0x40u"), ("F_NOISE", "0x80u"), ("NBOX_SHIFT", 8), ("W_M", 4), ("W_CTR", 5), ("W_BOX", 8)):
        assert re.search(r"^#define BPX_AUG_%s %s$" % (macro, value), header, re.M), macro
    assert (A.W_FLAGS, A.W_A, A.W_B, A.W_S, A.W_M, A.W_CTR, A.W_BOX) == (AR.W_FLAGS, AR.W_A, AR.W_B, AR.W_S, AR.W_M, AR.W_CTR, AR.W_BOX) == (0, 1, 2, 3, 4, 5, 8)


@pytest.mark.parametrize("kw, word", [
    (dict(da_prob=-0.1), "da_prob"), (dict(da_prob=1.5), "da_prob"),
    (dict(brightness=(0.2, 0.1)), "brightness"), (dict(contrast=(0.2, 0.1)), "contrast"), (dict(gaussian_noise=(0.2, 0.1)), "gaussian_noise"),
    (dict(gaussian_noise=(-0.1, 0.1)), "gaussian_noise"), (dict(brightness=0.3), "brightness"),
    (dict(cutout=dict(n=(1, 5))), "cutout['n']"), (dict(cutout=dict(n=(0, 2))), "cutout['n']"), (dict(cutout=dict(n=(3, 2))), "cutout['n']"),
    (dict(cutout=dict(size=(0.0, 0.3))), "cutout['size']"), (dict(cutout=dict(size=(0.1, 1.5))), "cutout['size']"),
    (dict(cutout=dict(size=(0.4, 0.3))), "cutout['size']"), (dict(cutout=dict(boxes=2)), "cutout"), (dict(seed="x"), "seed"),
])
def test_constructor_validation(kw, word):
    from biapy_amd.augment import DeviceAugmenter

    with pytest.raises(ValueError) as e:
        DeviceAugmenter(**kw)
    assert word in str(e.value)


def test_constructor_is_keyword_only_and_defaults_are_off():
    from biapy_amd.augment import DeviceAugmenter

    with pytest.raises(TypeError):
        DeviceAugmenter(0.5)
    a = DeviceAugmenter(seed=3)
    assert a.enable_mask == 0 and a.da_prob == 0.5 and a.seed == 3
    assert DeviceAugmenter().seed == torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
    c = DeviceAugmenter(cutout={}).cutout
    assert c == dict(n=(1, 3), size=(0.05, 0.3), cval=0.0, apply_to_mask=False)
    assert DeviceAugmenter(da_prob=1.0).config()["thr"] == 2 ** 32 and DeviceAugmenter(da_prob=0.0).config()["thr"] == 0


def _cfg(**aug):
    return types.SimpleNamespace(AUGMENTOR=types.SimpleNamespace(**aug))


def test_from_cfg():
    from biapy_amd.augment import DeviceAugmenter

    assert DeviceAugmenter.from_cfg(_cfg(ENABLE=False, ELASTIC=True)) is None
    assert DeviceAugmenter.from_cfg({"AUGMENTOR": {"ENABLE": False}}) is None
    a = DeviceAugmenter.from_cfg(_cfg(ENABLE=True, DA_PROB=0.25, ROT90=True, ZFLIP=True, VFLIP=True, HFLIP=True, BRIGHTNESS=True,
                                      BRIGHTNESS_FACTOR=(-0.2, 0.3), CONTRAST=True, CONTRAST_FACTOR=(-0.4, 0.5), GAUSSIAN_NOISE=True,
                                      GAUSSIAN_NOISE_STD=(0.01, 0.02), CUTOUT=True, COUT_NB_ITERATIONS=(2, 4), COUT_SIZE=(0.1, 0.2), COUT_CVAL=0.5,
                                      COUT_APPLY_TO_MASK=True, ELASTIC=False, DRAW_GRID=True, SHUFFLE_TRAIN_DATA_EACH_EPOCH=True), seed=11)
    assert (a.da_prob, a.rot90, a.zflip, a.vflip, a.hflip, a.seed) == (0.25, True, True, True, True, 11)
    assert a.brightness == (-0.2, 0.3) and a.contrast == (-0.4, 0.5) and a.gaussian_noise == (0.01, 0.02)
    assert a.cutout == dict(n=(2, 4), size=(0.1, 0.2), cval=0.5, apply_to_mask=True)
    b = DeviceAugmenter.from_cfg({"AUGMENTOR": {"ENABLE": True, "HFLIP": True, "BRIGHTNESS": False, "BRIGHTNESS_FACTOR": (-1, 1),
                                                "GAUSSIAN_NOISE": True, "GAUSSIAN_NOISE_VAR": 0.04}})
    assert (b.rot90, b.zflip, b.vflip, b.hflip, b.brightness, b.contrast, b.cutout, b.da_prob) == (False, False, False, True, None, None, None, 0.5)
    assert b.gaussian_noise == pytest.approx((0.2, 0.2))
    for key in ("RANDOM_ROT", "ELASTIC", "ZOOM", "SHEAR", "G_BLUR", "GAMMA_CONTRAST", "SOME_FUTURE_SWITCH"):
        with pytest.raises(NotImplementedError) as e:
            DeviceAugmenter.from_cfg(_cfg(ENABLE=True, HFLIP=True, **{key: True}))
        assert "AUGMENTOR." + key in str(e.value)
    with pytest.raises(NotImplementedError):
        DeviceAugmenter.from_cfg({"AUGMENTOR": {"ENABLE": True, "CUTMIX": True}})
    with pytest.raises(ValueError):
        DeviceAugmenter.from_cfg(_cfg(ENABLE=True, DA_PROB=2.0))


def test_call_refuses_cpu_tensors():
    from biapy_amd.augment import DeviceAugmenter

    with pytest.raises(ValueError) as e:
        DeviceAugmenter(hflip=True)(torch.zeros(1, 2, 8, 8, 1), torch.zeros(1, 2, 8, 8, 1))
    assert "no CPU path" in str(e.value)


def test_train_one_epoch_takes_augment_after_sync_every():
    import inspect

    from biapy_amd import train_engine as TE

    ps = list(inspect.signature(TE.train_one_epoch).parameters.values())
    assert [p.name for p in ps[-3:]] == ["graph", "sync_every", "augment"]
    assert ps[-1].default is None and ps[-1].kind is inspect.Parameter.KEYWORD_ONLY
    assert "augment" not in inspect.signature(TE.evaluate).parameters


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds: counter and key all zero, all ones, and the digits of pi."""
    def hexes(words):
        return ["%08x" % int(w) for w in words]

    assert hexes(AR.philox4x32_10(0, 0, 0, 0, 0, 0)) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = 0xFFFFFFFF
    assert hexes(AR.philox4x32_10(f, f, f, f, f, f)) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert hexes(AR.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]
    r = AR.philox4x32_10(np.arange(5), 1, 2, 3, 4, 5)                    # arrays broadcast, element by element the scalar result
    for i in range(5):
        assert [int(w[i]) for w in r] == [int(w) for w in AR.philox4x32_10(i, 1, 2, 3, 4, 5)]


def _config(**kw):
    from biapy_amd.augment import DeviceAugmenter

    return DeviceAugmenter(**kw).config()


ALL_ON = dict(rot90=True, zflip=True, vflip=True, hflip=True, brightness=(-0.1, 0.3), contrast=(-0.2, 0.2), gaussian_noise=(0.01, 0.05),
              cutout=dict(n=(1, 4), size=(0.05, 0.3)))


def test_draw_layout_and_properties():
    B, shape = 4096, (5, 72, 72)
    rec = AR.draw(1234, 7, B, shape, _config(seed=1234, **ALL_ON))
    assert rec.shape == (B, 32) and rec.dtype == np.int32
    ps = [AR.parse(r) for r in rec]
    assert {p["k"] for p in ps} == {0, 1, 2, 3}
    assert all(p["counter"] == 7 and p["reserved"] == 0 and p["m"] == 0 for p in ps)
    for name in ("zflip", "vflip", "hflip", "contrast", "brightness", "noise"):
        frac = np.mean([p[name] for p in ps])
        assert abs(frac - 0.5) <= 5 * 0.5 / np.sqrt(B), (name, frac)        # five sigma of a fair coin over 4096 samples
    assert {p["nbox"] for p in ps} == {0, 1, 2, 3, 4}
    for p in ps:
        assert -0.1 <= p["b"] <= np.float32(0.3) and np.float32(0.8) <= p["a"] <= np.float32(1.2) and np.float32(0.01) <= p["s"] <= np.float32(0.05)
        for (z0, y0, x0, dz, dy, dx) in p["boxes"]:
            for o, d, n in ((z0, dz, shape[0]), (y0, dy, shape[1]), (x0, dx, shape[2])):
                assert 1 <= d <= max(1, int(0.3 * n) + 1) and 0 <= o and o + d <= n
    # boxes beyond the count stay zero
    for r, p in zip(rec, ps):
        assert not r[8 + 6 * p["nbox"]:].any()
    # round trip of the layout
    p = AR.parse(AR.make_record(k=3, zflip=True, hflip=True, a=1.25, s=0.5, boxes=[(1, 2, 3, 4, 5, 6)], counter=(5 << 32) | 9))
    assert (p["k"], p["zflip"], p["vflip"], p["hflip"], p["contrast"], p["brightness"], p["noise"]) == (3, True, False, True, True, False, True)
    assert p["a"] == 1.25 and p["s"] == 0.5 and p["boxes"] == [(1, 2, 3, 4, 5, 6)] and p["counter"] == (5 << 32) | 9
    # another counter or seed: other draws
    assert (AR.draw(1234, 8, B, shape, _config(seed=1234, **ALL_ON)) != rec).any()


def test_draw_probability_extremes_and_degenerate_ranges():
    B, shape = 4096, (5, 72, 72)
    none = AR.draw(5, 0, B, shape, _config(seed=5, da_prob=0.0, **ALL_ON))
    assert not (none[:, 0]).any() and not none[:, 8:].any()
    kw = dict(ALL_ON, brightness=(0.125, 0.125), contrast=(0.1, 0.1), gaussian_noise=(0.3, 0.3), cutout=dict(n=(2, 2), size=(0.1, 0.1)))
    every = [AR.parse(r) for r in AR.draw(5, 0, B, shape, _config(seed=5, da_prob=1.0, **kw))]
    for p in every:
        assert p["zflip"] and p["vflip"] and p["hflip"] and p["contrast"] and p["brightness"] and p["noise"] and p["nbox"] == 2
        assert p["b"] == np.float32(0.125) and p["a"] == np.float32(1) + np.float32(0.1) and p["s"] == np.float32(0.3)       # lo == hi: exactly lo
        assert all(b[3:] == (1, 7, 7) for b in p["boxes"])                    # max(1, floor(0.1 * 5)) = 1, floor(float32(0.1) * 72) = 7
    assert {p["k"] for p in every} == {0, 1, 2, 3}
    # disabled transforms never fire, whatever da_prob is; 2-D (Z = 1) never flips Z
    only = [AR.parse(r) for r in AR.draw(5, 0, 256, shape, _config(seed=5, da_prob=1.0, hflip=True))]
    assert all(p["hflip"] and not (p["zflip"] or p["vflip"] or p["k"] or p["contrast"] or p["brightness"] or p["noise"] or p["nbox"]) for p in only)
    flat = [AR.parse(r) for r in AR.draw(5, 0, 256, (1, 40, 40), _config(seed=5, da_prob=1.0, **ALL_ON))]
    assert not any(p["zflip"] for p in flat) and all(p["vflip"] for p in flat)


def _sample_pair(B=2, Z=3, Y=6, X=6, C=2, Ct=1):
    n = B * Z * Y * X
    x = torch.arange(n * C, dtype=torch.float32).reshape(B, Z, Y, X, C) * 0.5 - 7
    t = (torch.arange(n * Ct).reshape(B, Z, Y, X, Ct) % 251).to(torch.uint8)
    return x, t


def test_reference_apply_is_a_permutation_for_geometry():
    x, t = _sample_pair()
    pos = torch.arange(x[..., :1].numel(), dtype=torch.float32).reshape(x[..., :1].shape)     # the voxel's own index travels with it
    for k in range(4):
        for flips in range(8):
            rec = np.stack([AR.make_record(k=k, zflip=bool(flips & 1), vflip=bool(flips & 2), hflip=bool(flips & 4)),
                            AR.make_record(k=(k + 1) % 4, zflip=bool(flips & 4), vflip=bool(flips & 1), hflip=bool(flips & 2))])
            xo, to = AR.apply(x, t, rec, np.zeros(2, np.float32))
            po, _ = AR.apply(pos, t, rec, np.zeros(2, np.float32))
            for b in range(2):
                assert torch.equal(xo[b].reshape(-1, 2).sort(0).values, x[b].reshape(-1, 2).sort(0).values)
                src = po[b].reshape(-1).long() - b * pos[0].numel()
                assert torch.equal(xo[b].reshape(-1, 2), x[b].reshape(-1, 2)[src])         # image and target moved by the same permutation
                assert torch.equal(to[b].reshape(-1), t[b].reshape(-1)[src])
                assert sorted(src.tolist()) == list(range(pos[0].numel()))
    # the stated convention: k = 1 is torch.rot90 over (Y, X), vflip is Y, hflip is X
    xo, _ = AR.apply(x, t, np.stack([AR.make_record(k=1), AR.make_record(vflip=True)]), np.zeros(2, np.float32))
    assert torch.equal(xo[0], torch.rot90(x[0], 1, dims=(1, 2))) and torch.equal(xo[1], torch.flip(x[1], (1,)))


def test_reference_apply_identity_order_and_cutout():
    x, t = _sample_pair()
    clear = np.stack([AR.make_record(), AR.make_record(counter=99)])
    xo, to = AR.apply(x, t, clear, np.array([3.0, 4.0], np.float32))
    assert torch.equal(xo, x) and torch.equal(to, t)
    m = AR.mean32(x)
    assert m.dtype == np.float32 and m[0] == np.float32(x[0].double().mean().item())
    rec = np.stack([AR.make_record(a=1.5, b=0.25, boxes=[(0, 1, 2, 2, 3, 4)]), AR.make_record(a=1.0)])
    xo, to = AR.apply(x, t, rec, m, cval=-1.0)
    want = (x[0] - torch.tensor(m[0])) * 1.5 + torch.tensor(m[0]) + 0.25
    want[0:2, 1:4, 2:6] = -1.0
    assert torch.equal(xo[0], want) and torch.equal(to, t)
    assert torch.equal(xo[1], (x[1] - torch.tensor(m[1])) * 1.0 + torch.tensor(m[1]))     # a fired step is applied even with a neutral factor
    _, to = AR.apply(x, t, rec, m, cval=-1.0, apply_to_mask=True)
    assert not to[0, 0:2, 1:4, 2:6].any() and torch.equal(to[1], t[1]) and to[0].sum() < t[0].sum()
    assert torch.equal(AR.box_mask(rec, (3, 6, 6))[0].nonzero()[:, 0].unique(), torch.tensor([0, 1]))


def test_noise_seed_meets_the_five_sigma_conditions_under_a_correct_generator():
    """The device test's conditions (test_augment_gpu case 5) hold for NumPy's Box-Muller on the host twin's uniform stream with the seed, counter
    and shape that test uses - so a failure there is the device generator's, not the seed's."""
    B = AR.NOISE_SHAPE[0]
    per = int(np.prod(AR.NOISE_SHAPE[1:]))
    d = np.stack([AR.noise_normals(AR.NOISE_SEED, 0, b, per) for b in range(B)]).reshape(AR.NOISE_SHAPE)
    st, bd = AR.noise_stats(d), AR.noise_bounds(d.size)
    print("host noise statistics:", st, "bounds:", bd)
    assert st["n"] == 233280 and np.isfinite(d).all()
    assert abs(st["mean"]) <= bd["mean"] and abs(st["var"] - 1) <= bd["var"] and abs(st["lag1"]) <= bd["lag1"] and abs(st["cross"]) <= bd["cross"]
    assert st["max"] <= bd["max"]
    d1 = AR.noise_normals(AR.NOISE_SEED, 1, 0, per)
    assert not np.array_equal(d1, d[0].reshape(-1))                          # the next call's counter gives other values

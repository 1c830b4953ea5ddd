"""The affine warp of the device augmenter - what can be checked without a GPU: the entry points are declared, exported and bound and refuse bad
arguments on the host; the record macros of the header are the module's; the constructor and ``from_cfg(affine=True)`` validate and map; and the
host twin (tests/warp_ref.py) keeps the stated conventions: [[0, 1], [-1, 0]] is np.rot90, the identity is bit for bit, the reflect rule is
numpy.pad's over several periods, and the fires have the stated frequency."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import warp_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bpx_warp_draw", "bpx_warp_apply")


def test_entry_points_are_declared_exported_and_bound():
    from biapy_amd import _lib as L
    from biapy_amd import augment as A

    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    source = open(os.path.join(ROOT, "biapy_amd", "csrc", "augment.hip")).read()
    assert set(re.findall(r"\bbpx_warp_[a-z_]+(?=\()", source)) == set(NAMES)
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in L.EXPORTS and getattr(L.lib._raw, name) is not None, name
    for macro, value, mine in (("REC_WORDS", "16", A.WARP_REC_WORDS), ("F_ROT", "0x1u", A.WF_ROT), ("F_ZOOM", "0x2u", A.WF_ZOOM),
                               ("F_SHEAR", "0x4u", A.WF_SHEAR), ("F_SHIFT", "0x8u", A.WF_SHIFT), ("W_FLAGS", "0", A.WW_FLAGS), ("W_M", "1", A.WW_M),
                               ("W_P", "8", A.WW_P), ("CONSTANT", "0", A.AFFINE_MODES["constant"]), ("REFLECT", "1", A.AFFINE_MODES["reflect"]),
                               ("EDGE", "2", A.AFFINE_MODES["edge"])):
        assert re.search(r"^#define BPX_WARP_%s %s\b" % (macro, value), header, re.M), macro
        assert int(value.rstrip("u"), 0) == mine, macro
    assert (WR.REC, WR.F_ROT, WR.F_ZOOM, WR.F_SHEAR, WR.F_SHIFT, WR.W_FLAGS, WR.W_M, WR.W_P) == (16, 1, 2, 4, 8, 0, 1, 8) and WR.MODES == A.AFFINE_MODES
    assert ctypes.sizeof(L.WarpCfg) == 56                                 # two uint64, two uint32, eight floats: the header's struct


def test_host_side_argument_checks():
    from biapy_amd import _lib as L

    def err():
        return L.lib.bpx_last_error()

    cfg = L.WarpCfg(1, 1 << 31, 0xF, 0, -10, 10, 0.5, 2, -5, 5, -0.1, 0.1)
    p = ctypes.addressof(cfg)
    assert L.lib.bpx_warp_draw(None, 1, 8, 8, None, None, None) != 0 and b"null pointer" in err()
    assert L.lib.bpx_warp_draw(p, 0, 8, 8, 64, 128, None) != 0 and b"bad extents" in err()
    assert L.lib.bpx_warp_draw(p, 1, 8, 8, 64, 132, None) != 0 and b"16-byte aligned" in err()
    bad = L.WarpCfg(1, (1 << 32) + 1, 0xF, 0, -10, 10, 0.5, 2, -5, 5, -0.1, 0.1)
    assert L.lib.bpx_warp_draw(ctypes.addressof(bad), 1, 8, 8, 64, 128, None) != 0 and b"thr above 2^32" in err()
    bad = L.WarpCfg(1, 1, 0xF, 0, -10, 10, 0.0, 2, -5, 5, -0.1, 0.1)
    assert L.lib.bpx_warp_draw(ctypes.addressof(bad), 1, 8, 8, 64, 128, None) != 0 and b"zoom range" in err()
    bad = L.WarpCfg(1, 1, 0xF, 0, 10, -10, 0.5, 2, -5, 5, -0.1, 0.1)
    assert L.lib.bpx_warp_draw(ctypes.addressof(bad), 1, 8, 8, 64, 128, None) != 0 and b"lo > hi" in err()
    # bpx_warp_apply: the checks of bpx_aug_apply - null pointers, channel ranges, dtype, in place - and the mode
    assert L.lib.bpx_warp_apply(None, 32, L.F32, 1, 1, 8, 8, 1, 1, 48, 0, 0.0, 64, 80, None) != 0 and b"null pointer" in err()
    assert L.lib.bpx_warp_apply(16, 32, L.F32, 1, 1, 8, 8, 17, 1, 48, 0, 0.0, 64, 80, None) != 0 and b"1..16 image channels" in err()
    assert L.lib.bpx_warp_apply(16, 32, L.F32, 1, 1, 8, 8, 1, 9, 48, 0, 0.0, 64, 80, None) != 0 and b"1..8 target channels" in err()
    assert L.lib.bpx_warp_apply(16, 32, L.BF16, 1, 1, 8, 8, 1, 1, 48, 0, 0.0, 64, 80, None) != 0 and b"float32 or uint8" in err()
    assert L.lib.bpx_warp_apply(16, 32, L.F32, 1, 1, 8, 8, 1, 1, 48, 0, 0.0, 16, 80, None) != 0 and b"in place" in err()
    assert L.lib.bpx_warp_apply(16, 32, L.U8, 1, 1, 8, 8, 1, 1, 48, 0, 0.0, 64, 32, None) != 0 and b"in place" in err()
    assert L.lib.bpx_warp_apply(16, 32, L.F32, 1, 1, 8, 8, 1, 1, 48, 3, 0.0, 64, 80, None) != 0 and b"border mode" in err()
    assert L.lib.bpx_warp_apply(16, 32, L.F32, 1, 0, 8, 8, 1, 1, 48, 0, 0.0, 64, 80, None) != 0 and b"bad extents" in err()


@pytest.mark.parametrize("kw, word", [
    (dict(rotation=(-400, 0)), "rotation"), (dict(rotation=(10, -10)), "rotation"), (dict(rotation=(0, 361)), "rotation"), (dict(rotation=30), "rotation"),
    (dict(zoom=(0.05, 1)), "zoom"), (dict(zoom=(1, 11)), "zoom"), (dict(zoom=(2, 1)), "zoom"), (dict(zoom=(float("nan"), 1)), "zoom"),
    (dict(shear=(-61, 0)), "shear"), (dict(shear=(0, 60.5)), "shear"), (dict(shift=(-1.5, 0)), "shift"), (dict(shift=(0, 1.01)), "shift"),
    (dict(shift=("a", "b")), "shift"), (dict(affine_mode="wrap"), "affine_mode"), (dict(affine_mode=None), "affine_mode"),
    (dict(affine_cval=float("inf")), "affine_cval"), (dict(affine_cval="x"), "affine_cval"),
])
def test_constructor_validation(kw, word):
    from biapy_amd.augment import DeviceAugmenter

    with pytest.raises(ValueError) as e:
        DeviceAugmenter(**kw)
    assert word in str(e.value)


def test_constructor_defaults_and_config():
    from biapy_amd.augment import DeviceAugmenter

    a = DeviceAugmenter(seed=3)
    assert (a.rotation, a.zoom, a.shear, a.shift, a.affine_mode, a.affine_cval) == (None, None, None, None, "constant", 0.0)
    assert a.warp_enable_mask == 0 and a.enable_mask == 0 and a.last_warp_records is None
    b = DeviceAugmenter(seed=3, da_prob=0.25, rotation=(-360, 360), zoom=(0.1, 10), shear=(-60, 60), shift=(-1, 1), affine_mode="reflect", affine_cval=2)
    assert b.warp_config() == dict(seed=3, thr=1 << 30, enable=0xF, rotation=(-360.0, 360.0), zoom=(0.1, 10.0), shear=(-60.0, 60.0), shift=(-1.0, 1.0))
    assert b.enable_mask == 0                                             # bpx_aug_cfg.enable does not know the warp
    assert DeviceAugmenter(zoom=(1, 2)).warp_enable_mask == WR.F_ZOOM and DeviceAugmenter(shift=(0, 0)).warp_enable_mask == WR.F_SHIFT
    assert DeviceAugmenter(rotation=(0, 90), rot90=True).config()["enable"] == 1        # the existing record configuration is untouched
    with pytest.raises(ValueError) as e:                                  # the device-only refusal comes first, warp or not
        DeviceAugmenter(rotation=(0, 90))(torch.zeros(1, 2, 8, 8, 1), torch.zeros(1, 2, 8, 8, 1))
    assert "no CPU path" in str(e.value)


def _cfg(**aug):
    return types.SimpleNamespace(AUGMENTOR=types.SimpleNamespace(**aug))


def test_from_cfg_affine():
    from biapy_amd.augment import DeviceAugmenter

    for key in ("RANDOM_ROT", "ZOOM", "SHEAR", "SHIFT"):                  # the default keeps refusing the family by name
        with pytest.raises(NotImplementedError) as e:
            DeviceAugmenter.from_cfg(_cfg(ENABLE=True, HFLIP=True, **{key: True}))
        assert "AUGMENTOR." + key in str(e.value)
    a = DeviceAugmenter.from_cfg(_cfg(ENABLE=True, DA_PROB=0.25, HFLIP=True, RANDOM_ROT=True, RANDOM_ROT_RANGE=(-30, 45), ZOOM=True, ZOOM_RANGE=(0.9, 1.5),
                                      ZOOM_IN_Z=False, SHEAR=True, SHEAR_RANGE=(-10, 12), SHIFT=True, SHIFT_RANGE=(0.05, 0.1), AFFINE_MODE="edge",
                                      ELASTIC=False), seed=5, affine=True)
    assert (a.rotation, a.zoom, a.shear, a.shift, a.affine_mode, a.hflip, a.da_prob, a.seed) == ((-30.0, 45.0), (0.9, 1.5), (-10.0, 12.0), (0.05, 0.1), "edge",
                                                                                                  True, 0.25, 5)
    b = DeviceAugmenter.from_cfg({"AUGMENTOR": {"ENABLE": True, "RANDOM_ROT": True, "ZOOM": False, "ZOOM_RANGE": (0.5, 2), "AFFINE_MODE": "constant"}}, affine=True)
    assert b.rotation == (-180.0, 180.0) and b.zoom is None and b.shear is None and b.shift is None and b.affine_mode == "constant"
    assert DeviceAugmenter.from_cfg(_cfg(ENABLE=True, VFLIP=True), affine=True).warp_enable_mask == 0
    assert DeviceAugmenter.from_cfg(_cfg(ENABLE=False, RANDOM_ROT=True), affine=True) is None
    for extra, word in ((dict(ELASTIC=True), "AUGMENTOR.ELASTIC"), (dict(ZOOM=True, ZOOM_IN_Z=True), "AUGMENTOR.ZOOM_IN_Z"),
                        (dict(AFFINE_MODE="wrap"), "wrap"), (dict(AFFINE_MODE="symmetric"), "symmetric"), (dict(G_BLUR=True), "AUGMENTOR.G_BLUR"),
                        (dict(AFFINE=True), "AUGMENTOR.AFFINE")):
        with pytest.raises(NotImplementedError) as e:
            DeviceAugmenter.from_cfg(_cfg(ENABLE=True, RANDOM_ROT=True, **extra), affine=True)
        assert word in str(e.value), extra
    with pytest.raises(ValueError, match="zoom"):
        DeviceAugmenter.from_cfg(_cfg(ENABLE=True, ZOOM=True, ZOOM_RANGE=(0.0, 1.0)), affine=True)


# ---- the twin's own conventions ---------------------------------------------------------------------------------------------------------------
def _pair(B=2, Z=2, Y=7, X=7, C=2, Ct=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, Z, Y, X, C, generator=g), torch.randint(0, 256, (B, Z, Y, X, Ct), generator=g).to(torch.uint8)


@pytest.mark.parametrize("mode", ["constant", "reflect", "edge"])
def test_twin_quarter_turn_is_rot90_and_identity_is_bit_for_bit(mode):
    x, t = _pair()
    rec = np.stack([WR.make_record([[0, 1], [-1, 0]], plane=(7, 7)), WR.make_record([[1, 0], [0, 1]], plane=(7, 7))])
    xo, to = WR.apply(x, t, rec, mode, cval=9.0)
    assert np.array_equal(xo[0].numpy(), np.rot90(x[0].numpy(), 1, axes=(1, 2))) and np.array_equal(to[0].numpy(), np.rot90(t[0].numpy(), 1, axes=(1, 2)))
    assert torch.equal(xo[0], torch.rot90(x[0], 1, dims=(1, 2)))
    assert torch.equal(xo[1].view(torch.int32), x[1].view(torch.int32)) and torch.equal(to[1], t[1])
    # a non-square plane, the identity again; flags 0 copies whatever the matrix words hold
    x, t = _pair(Y=5, X=8, seed=1)
    rec = np.stack([WR.make_record([[1, 0], [0, 1]], plane=(5, 8)), WR.make_record([[3, 1], [2, 5]], flags=0, plane=(5, 8))])
    xo, to = WR.apply(x, t, rec, mode)
    assert torch.equal(xo.view(torch.int32), x.view(torch.int32)) and torch.equal(to, t)


def test_twin_half_voxel_shift_interpolates_and_constant_fills():
    x, t = _pair(B=1, Z=1, Y=4, X=6, C=1)
    rec = [WR.make_record([1, 0, 1.5, 0, 1, 3.0], flags=WR.F_SHIFT)]     # fy = y, fx = x + 0.5: the mean of two neighbours along X
    xo, to = WR.apply(x, t, rec, "constant", cval=2.0)
    v = x[0, 0, :, :, 0]
    assert torch.equal(xo[0, 0, :, :5, 0], v[:, :5] * 0.5 + v[:, 1:] * 0.5)
    assert torch.equal(xo[0, 0, :, 5, 0], v[:, 5] * 0.5 + 2.0 * 0.5)                    # the tap past the edge is cval
    assert torch.equal(to[0, 0, :, :5, 0], t[0, 0, :, 1:, 0]) and not to[0, 0, :, 5, 0].any()   # floor(x + 1): the right neighbour, 0 past the edge
    xe, te = WR.apply(x, t, rec, "edge")
    assert torch.equal(xe[0, 0, :, 5, 0], v[:, 5] * 0.5 + v[:, 5] * 0.5) and torch.equal(te[0, 0, :, 5, 0], t[0, 0, :, 5, 0])


@pytest.mark.parametrize("n", [1, 2, 5])
def test_twin_reflect_is_numpy_pad_over_several_periods(n):
    pad = 4 * max(2 * n - 2, 1) + 3
    base = np.arange(n)
    if n == 1:
        want = np.zeros(2 * pad + 1, dtype=np.int64)                       # numpy.pad cannot reflect one voxel: the stated rule is index 0
    else:
        want = np.pad(base, pad, mode="reflect")
    got, inside = WR.tap_index(np.arange(-pad, n + pad), n, "reflect")
    assert np.array_equal(got, want) and inside.all() and got.min() >= 0 and got.max() <= n - 1
    e, ie = WR.tap_index(np.arange(-pad, n + pad), n, "edge")
    assert np.array_equal(e, np.pad(base, pad, mode="edge")) and ie.all()
    c, ic = WR.tap_index(np.arange(-pad, n + pad), n, "constant")
    assert np.array_equal(ic, np.pad(np.ones(n, bool), pad)) and c.min() >= 0 and c.max() <= n - 1


def test_twin_draw_frequencies_ranges_and_neutral_values():
    from biapy_amd.augment import DeviceAugmenter

    B = 12000
    aug = DeviceAugmenter(seed=99, da_prob=0.5, rotation=(-30, 45), zoom=(0.8, 1.25), shear=(-10, 12), shift=(-0.1, 0.2))
    flags, p = WR.draw(99, 3, B, aug.warp_config())
    for bit in (WR.F_ROT, WR.F_ZOOM, WR.F_SHEAR, WR.F_SHIFT):
        frac = np.mean((flags & bit) != 0)
        assert abs(frac - 0.5) <= 5 * 0.5 / np.sqrt(B), (bit, frac)      # five sigma of a fair coin over 12,000 samples
    both = np.mean((flags & 3) == 3)
    assert abs(both - 0.25) <= 5 * np.sqrt(0.25 * 0.75 / B)               # the fires are independent words
    for i, (bit, lo, hi, neutral) in enumerate(((1, -30, 45, 0), (2, 0.8, 1.25, 1), (4, -10, 12, 0), (8, -0.1, 0.2, 0), (8, -0.1, 0.2, 0))):
        on = (flags & bit) != 0
        assert (p[~on, i] == neutral).all() and (p[on, i] >= np.float32(lo)).all() and (p[on, i] <= np.float32(hi)).all()
        assert p[on, i].max() - p[on, i].min() > 0.9 * (hi - lo)
    assert abs(np.corrcoef(p[(flags & 8) != 0, 3], p[(flags & 8) != 0, 4])[0, 1]) <= 5 / np.sqrt(B / 2 - 400)     # ty and tx are separate words
    f2, p2 = WR.draw(99, 4, B, aug.warp_config())
    assert (f2 != flags).any() and (p2 != p).any()
    none, pn = WR.draw(99, 3, 64, DeviceAugmenter(seed=99, da_prob=0.0, rotation=(-30, 45), zoom=(0.8, 1.25)).warp_config())
    assert not none.any() and (pn == np.float32([0, 1, 0, 0, 0])).all()
    only, po = WR.draw(99, 3, 64, DeviceAugmenter(seed=99, da_prob=1.0, zoom=(2, 2)).warp_config())
    assert (only == WR.F_ZOOM).all() and (po == np.float32([0, 2, 0, 0, 0])).all()


def test_matrix_statement_and_bound():
    p = np.float32([[90, 1, 0, 0, 0], [0, 2, 0, 0.25, -0.5], [0, 1, 45, 0, 0], [0, 1, 0, 0, 0]])
    m = WR.matrix64(p, 9, 5)
    assert np.allclose(m[0], [0, 1, 4, -1, 0, 2], atol=1e-15)             # the quarter turn of the issue's sign convention
    assert np.allclose(m[1], [0.5, 0, 4 - 2.25, 0, 0.5, 2 + 2.5]) and np.allclose(m[2], [1, 0, 4, 1, 1, 2]) and np.array_equal(m[3], [1, 0, 4, 0, 1, 2])
    bd = WR.matrix_bound(p, 9, 5)
    assert bd.shape == (4, 6) and (bd > 0).all() and (bd < 1e-4).all()
    # numpy's own fp32 evaluation in the kernel's association lies inside the bound (its sin / cos / tan are within the assumed 4 ulp)
    rng = np.random.default_rng(0)
    q = np.stack([rng.uniform(-360, 360, 500), rng.uniform(0.1, 10, 500), rng.uniform(-60, 60, 500), rng.uniform(-1, 1, 500), rng.uniform(-1, 1, 500)], 1).astype(np.float32)
    d2r = np.float32(0.017453292519943295)
    c, s, t, iz = np.cos(q[:, 0] * d2r), np.sin(q[:, 0] * d2r), np.tan(q[:, 2] * d2r), np.float32(1) / q[:, 1]
    Y, X = 300, 77
    got = np.stack([iz * (c + s * t), iz * s, np.float32((Y - 1) / 2) - q[:, 3] * np.float32(Y), iz * (c * t - s), iz * c, np.float32((X - 1) / 2) - q[:, 4] * np.float32(X)], 1)
    assert got.dtype == np.float32
    ratio = np.abs(got.astype(np.float64) - WR.matrix64(q, Y, X)) / WR.matrix_bound(q, Y, X)
    assert ratio.max() <= 1.0, ratio.max()

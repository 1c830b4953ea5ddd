"""The elastic deformation of the device augmenter - what can be checked without a GPU: the entry points are declared, exported and bound and
refuse bad arguments on the host; the record macros of the header are the module's; the constructor and ``from_cfg(elastic=True)`` validate and
map while the default and ``affine=True`` keep refusing ``ELASTIC``; and the host twin (tests/elastic_ref.py) keeps the stated conventions:
alpha 0 and flags 0 give the input's bits, a constant integer field is an exact shift in every mode, and on a smooth random field it lies
within the counted bound of ``scipy.ndimage.map_coordinates`` in float64."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import elastic_ref as ER
import warp_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bpx_elastic_draw", "bpx_elastic_noise", "bpx_elastic_apply")
MODES = ["constant", "reflect", "edge"]


def test_entry_points_are_declared_exported_and_bound():
    from biapy_amd import _lib as L
    from biapy_amd import augment as A

    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    source = open(os.path.join(ROOT, "biapy_amd", "csrc", "elastic.hip")).read()
    assert set(re.findall(r'extern "C" \w+ (\w+)\(', source)) == set(NAMES)
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in L.EXPORTS and getattr(L.lib._raw, name) is not None, name
    for macro, value, mine in (("REC_WORDS", "8", A.ELASTIC_REC_WORDS), ("F_FIRED", "0x1u", A.EF_FIRED), ("W_FLAGS", "0", A.EW_FLAGS),
                               ("W_ALPHA", "1", A.EW_ALPHA), ("W_CTR", "2", A.EW_CTR), ("STREAM", "24", A.ELASTIC_STREAM),
                               ("KEY_XOR", "0x454C4153u", A.ELASTIC_KEY_XOR)):
        assert re.search(r"^#define BPX_ELASTIC_%s %s\b" % (macro, value), header, re.M), macro
        assert int(value.rstrip("u"), 0) == mine, macro
    assert re.search(r"^#define BPX_ELASTIC_ALPHA_MAX 1024\.0f", header, re.M) and A.ELASTIC_ALPHA_MAX == 1024.0
    assert (ER.REC, ER.F_FIRED, ER.W_FLAGS, ER.W_ALPHA, ER.W_CTR, ER.STREAM, ER.KEY_XOR) == (8, 1, 0, 1, 2, 24, 0x454C4153)
    make = open(os.path.join(ROOT, "biapy_amd", "csrc", "Makefile")).read()
    assert "elastic.hip" in make and re.search(r"^elastic\.o:.*augment_core\.h", make, re.M) and re.search(r"^augment\.o:.*augment_core\.h", make, re.M)
    core = open(os.path.join(ROOT, "biapy_amd", "csrc", "augment_core.h")).read()
    check = open(os.path.join(ROOT, "scripts", "elastic_cpu_check.cpp")).read()
    assert "elastic_voxel<" in source and "elastic_voxel<" in check and '#include "augment_core.h"' in check    # one text for device and host
    assert "ElasticTaps elastic_voxel(" in core and "fmaf" not in core.split("#pragma once")[1]
    assert A.ELASTIC_RADIUS_MAX == 32 and int(4 * A.ELASTIC_SIGMA_MAX + 0.5) == A.ELASTIC_RADIUS_MAX and A.ELASTIC_FIELD_MAX == 2 ** 31


def test_host_side_argument_checks():
    from biapy_amd import _lib as L

    def err():
        return L.lib.bpx_last_error()

    thr = 1 << 31
    assert L.lib.bpx_elastic_draw(1, thr, 12.0, 16.0, 1, None, 128, None) != 0 and b"null pointer" in err()
    assert L.lib.bpx_elastic_draw(1, thr, 12.0, 16.0, 1, 64, None, None) != 0 and b"null pointer" in err()
    assert L.lib.bpx_elastic_draw(1, thr, 12.0, 16.0, 0, 64, 128, None) != 0 and b"bad extents" in err()
    assert L.lib.bpx_elastic_draw(1, thr, 12.0, 16.0, 1, 64, 132, None) != 0 and b"16-byte aligned" in err()
    assert L.lib.bpx_elastic_draw(1, (1 << 32) + 1, 12.0, 16.0, 1, 64, 128, None) != 0 and b"thr above 2^32" in err()
    for lo, hi in ((-1.0, 2.0), (3.0, 2.0), (0.0, 1025.0), (float("nan"), 1.0)):
        assert L.lib.bpx_elastic_draw(1, thr, lo, hi, 1, 64, 128, None) != 0 and b"alpha range" in err(), (lo, hi)
    assert L.lib.bpx_elastic_noise(1, 1, 8, 8, None, 256, None) != 0 and b"null pointer" in err()
    assert L.lib.bpx_elastic_noise(1, 1, 8, 8, 128, None, None) != 0 and b"null pointer" in err()
    assert L.lib.bpx_elastic_noise(1, 1, 0, 8, 128, 256, None) != 0 and b"bad extents" in err()
    assert L.lib.bpx_elastic_noise(1, 4, 16384, 16384, 128, 256, None) != 0 and b"2^31 or more" in err()      # 2 * 4 * 2^28 elements: the limit itself
    assert L.lib.bpx_elastic_noise(1, 1, 8, 8, 128, 258, None) != 0 and b"4-byte aligned" in err()
    # bpx_elastic_apply(x, t, dtype, B, Z, Y, X, C, Ct, records, field, mode, cval, x_out, t_out, stream); 1 x 1 x 8 x 8 x 1: 256 bytes a tensor
    x, t, rec, fld, xo, to = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000

    def call(x=x, t=t, dt=L.F32, B=1, Z=1, Y=8, X=8, C=1, Ct=1, rec=rec, fld=fld, mode=0, cval=0.0, xo=xo, to=to):
        return L.lib.bpx_elastic_apply(x, t, dt, B, Z, Y, X, C, Ct, rec, fld, mode, cval, xo, to, None)

    for kw in (dict(x=None), dict(t=None), dict(rec=None), dict(fld=None), dict(xo=None), dict(to=None)):
        assert call(**kw) != 0 and b"null pointer" in err(), kw
    for kw in (dict(B=0), dict(Z=0), dict(Y=0), dict(X=-1)):
        assert call(**kw) != 0 and b"bad extents" in err(), kw
    assert call(B=4, Y=16384, X=16384) != 0 and b"2^31 or more" in err()
    assert call(C=17) != 0 and b"1..16 image channels" in err() and call(C=0) != 0 and b"1..16 image channels" in err()
    assert call(Ct=9) != 0 and b"1..8 target channels" in err() and call(Ct=0) != 0 and b"1..8 target channels" in err()
    assert call(dt=L.BF16) != 0 and b"float32 or uint8" in err()
    assert call(mode=3) != 0 and b"border mode" in err() and call(mode=-1) != 0 and b"border mode" in err()
    assert call(cval=float("inf")) != 0 and b"cval must be finite" in err() and call(cval=float("nan")) != 0 and b"cval must be finite" in err()
    for kw in (dict(xo=x), dict(to=t), dict(xo=x + 252), dict(xo=t - 4), dict(to=fld + 8), dict(xo=fld - 252), dict(to=rec + 28), dict(xo=rec)):
        assert call(**kw) != 0 and b"out overlaps an input" in err(), kw
    assert call(to=xo + 128) != 0 and b"outputs overlap" in err()
    assert call(dt=L.U8, to=t + 63) != 0 and b"out overlaps an input" in err()                  # a uint8 target is 64 bytes


@pytest.mark.parametrize("kw, word", [
    (dict(alpha=(-1, 2)), "alpha"), (dict(alpha=(3, 2)), "alpha"), (dict(alpha=(0, 1025)), "alpha"), (dict(alpha=(float("nan"), 1)), "alpha"),
    (dict(alpha=(0, float("inf"))), "alpha"), (dict(alpha=5), "alpha"), (dict(alpha=None), "alpha"),
    (dict(sigma=0), "sigma"), (dict(sigma=-1), "sigma"), (dict(sigma=8.01), "32"), (dict(sigma=float("nan")), "sigma"), (dict(sigma=float("inf")), "sigma"),
    (dict(sigma="x"), "sigma"), (dict(sigma=(1, 2)), "sigma"),
    (dict(mode="wrap"), "mode"), (dict(mode=None), "mode"), (dict(cval=float("inf")), "cval"), (dict(cval=float("nan")), "cval"), (dict(cval="x"), "cval"),
    (dict(alfa=(1, 2)), "unknown keys"),
])
def test_constructor_validation(kw, word):
    from biapy_amd.augment import DeviceAugmenter

    with pytest.raises(ValueError) as e:
        DeviceAugmenter(elastic=kw)
    assert word in str(e.value)


def test_constructor_defaults_and_config():
    from biapy_amd import prepost as P
    from biapy_amd.augment import DeviceAugmenter

    with pytest.raises(ValueError, match="dict"):
        DeviceAugmenter(elastic=True)
    a = DeviceAugmenter(seed=3)
    assert a.elastic is None and a.elastic_config() is None and a.last_elastic_records is None and a.last_elastic_field is None
    b = DeviceAugmenter(seed=3, da_prob=0.25, elastic={})
    assert b.elastic == dict(alpha=(12.0, 16.0), sigma=4.0, mode="constant", cval=0.0)
    assert b.elastic_config() == dict(seed=3, thr=1 << 30, alpha=(12.0, 16.0), sigma=4.0, radius=16, mode="constant", cval=0.0)
    assert b.enable_mask == 0 and b.warp_enable_mask == 0                   # the other draws do not know the elastic step
    assert b._ew.dtype == np.float32 and np.array_equal(b._ew, P._gaussian_weights(4.0, 0, 16).astype(np.float32))      # computed once, at construction
    c = DeviceAugmenter(elastic=dict(alpha=(0, 1024), sigma=8, mode="reflect", cval=-2))
    assert c.elastic == dict(alpha=(0.0, 1024.0), sigma=8.0, mode="reflect", cval=-2.0) and len(c._ew) == 65
    assert len(DeviceAugmenter(elastic=dict(sigma=0.1))._ew) == 1           # radius 0: the field is the noise
    with pytest.raises(ValueError) as e:                                  # the device-only refusal comes first
        DeviceAugmenter(elastic={})(torch.zeros(1, 2, 8, 8, 1), torch.zeros(1, 2, 8, 8, 1))
    assert "no CPU path" in str(e.value)


def _cfg(**aug):
    return types.SimpleNamespace(AUGMENTOR=types.SimpleNamespace(**aug))


def test_from_cfg_elastic():
    from biapy_amd.augment import DeviceAugmenter

    for kw in (dict(), dict(affine=True)):                                # the default and affine=True alone keep refusing ELASTIC by name
        with pytest.raises(NotImplementedError) as e:
            DeviceAugmenter.from_cfg(_cfg(ENABLE=True, HFLIP=True, ELASTIC=True), **kw)
        assert "AUGMENTOR.ELASTIC" in str(e.value)
    a = DeviceAugmenter.from_cfg(_cfg(ENABLE=True, DA_PROB=0.25, HFLIP=True, ELASTIC=True, E_ALPHA=(10, 20), E_SIGMA=3, E_MODE="reflect"), seed=5, elastic=True)
    assert a.elastic == dict(alpha=(10.0, 20.0), sigma=3.0, mode="reflect", cval=0.0) and a.hflip and a.da_prob == 0.25 and a.seed == 5
    b = DeviceAugmenter.from_cfg({"AUGMENTOR": {"ENABLE": True, "ELASTIC": True}}, elastic=True)
    assert b.elastic == dict(alpha=(12.0, 16.0), sigma=4.0, mode="constant", cval=0.0)
    assert DeviceAugmenter.from_cfg(_cfg(ENABLE=True, VFLIP=True, ELASTIC=False, E_SIGMA=(1, 2)), elastic=True).elastic is None
    assert DeviceAugmenter.from_cfg(_cfg(ENABLE=False, ELASTIC=True), elastic=True) is None
    both = DeviceAugmenter.from_cfg(_cfg(ENABLE=True, ELASTIC=True, RANDOM_ROT=True, AFFINE_MODE="edge"), affine=True, elastic=True)
    assert both.elastic is not None and both.rotation == (-180.0, 180.0) and both.affine_mode == "edge"
    for extra, word in ((dict(E_SIGMA=(3, 5)), "E_SIGMA"), (dict(E_SIGMA=[4]), "E_SIGMA"), (dict(E_MODE="wrap"), "wrap"), (dict(E_MODE="symmetric"), "symmetric"),
                        (dict(G_BLUR=True), "AUGMENTOR.G_BLUR"), (dict(RANDOM_ROT=True), "AUGMENTOR.RANDOM_ROT")):
        with pytest.raises(NotImplementedError) as e:
            DeviceAugmenter.from_cfg(_cfg(ENABLE=True, ELASTIC=True, **extra), elastic=True)
        assert word in str(e.value), extra
    with pytest.raises(ValueError, match="sigma"):
        DeviceAugmenter.from_cfg(_cfg(ENABLE=True, ELASTIC=True, E_SIGMA=9), elastic=True)
    with pytest.raises(ValueError, match="alpha"):
        DeviceAugmenter.from_cfg(_cfg(ENABLE=True, ELASTIC=True, E_ALPHA=(0, 2000)), elastic=True)


# ---- the twin's own conventions ---------------------------------------------------------------------------------------------------------------
def _pair(B=2, Z=2, Y=7, X=9, C=2, Ct=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, Z, Y, X, C, generator=g), torch.randint(0, 256, (B, Z, Y, X, Ct), generator=g).to(torch.uint8)


@pytest.mark.parametrize("mode", MODES)
def test_twin_alpha_zero_and_flags_zero_give_the_inputs_bits(mode):
    x, t = _pair()
    field = np.random.default_rng(1).standard_normal((2, 2, 7, 9)).astype(np.float32) * 50
    xo, to = ER.apply(x, t, ER.make_records([0.0, 0.0]), field, mode, cval=9.0)                       # alpha 0: f = y + 0 s = y exactly
    assert torch.equal(xo.view(torch.int32), x.view(torch.int32)) and torch.equal(to, t)
    x[1, 0, 0, 0, 0], x[1, 1, 3, 4, 1] = float("nan"), -0.0                                            # flags 0 copies whatever the bits are
    xo, to = ER.apply(x, t, ER.make_records([5.0, 7.0], fired=[1, 0]), field, mode, cval=9.0)
    assert torch.equal(xo[1].view(torch.int32), x[1].view(torch.int32)) and torch.equal(to[1], t[1])
    assert not torch.equal(xo[0], x[0])


@pytest.mark.parametrize("mode", MODES)
def test_twin_constant_integer_field_is_an_exact_shift(mode):
    x, t = _pair(B=1, Z=2, Y=7, X=9, C=2)
    for dy, dx in ((2, -3), (-1, 0), (0, 4), (30, -40)):                  # the last: several reflect periods away
        field = np.empty((1, 2, 7, 9), dtype=np.float32)
        field[0, 0], field[0, 1] = dy / 4, dx / 4                         # alpha 4: exact products
        xo, to = ER.apply(x, t, ER.make_records([4.0]), field, mode, cval=0.5)
        (yi, iy), (xi, ix) = WR.tap_index(np.arange(7) + dy, 7, mode), WR.tap_index(np.arange(9) + dx, 9, mode)
        inside = (iy[:, None] & ix[None, :])[None, :, :, None]
        want_x = np.where(inside, x[0].numpy()[:, yi][:, :, xi], np.float32(0.5))
        want_t = np.where(inside, t[0].numpy()[:, yi][:, :, xi], np.uint8(0))
        assert np.array_equal(xo[0].numpy(), want_x) and np.array_equal(to[0].numpy(), want_t), (dy, dx)


def test_twin_noise_and_draw_statistics():
    from biapy_amd.augment import DeviceAugmenter

    n = ER.noise(77, 5, 3, 24, 20)
    assert n.shape == (3, 2, 24, 20) and n.dtype == np.float32 and n.min() >= -1 and n.max() < 1
    assert abs(n.mean()) <= 5 / np.sqrt(3 * n.size) and abs(n.var() - 1 / 3) <= 5 * np.sqrt(4 / 45 / n.size)      # uniform on [-1, 1): five sigma
    assert not np.array_equal(n[0], n[1]) and not np.array_equal(n, ER.noise(77, 6, 3, 24, 20)) and not np.array_equal(n, ER.noise(78, 5, 3, 24, 20))
    assert np.array_equal(ER.noise(77, 5, 2, 7, 9), ER.noise(77, 5, 3, 7, 9)[:2])             # a function of (seed, counter, sample, element) only
    assert np.array_equal(ER.noise(77, 5, 1, 2, 3).reshape(-1), ER.noise(77, 5, 1, 6, 5).reshape(-1)[:12])     # element e whatever the plane
    B = 12000
    aug = DeviceAugmenter(seed=99, da_prob=0.5, elastic=dict(alpha=(12, 16)))
    rec = ER.draw(99, 3, B, aug.elastic_config()).view(np.uint32)
    on = rec[:, 0] == 1
    alpha = rec[:, 1].copy().view(np.float32)
    assert set(np.unique(rec[:, 0])) == {0, 1} and abs(on.mean() - 0.5) <= 5 * 0.5 / np.sqrt(B)
    assert (alpha[~on] == 0).all() and (alpha[on] >= 12).all() and (alpha[on] <= 16).all() and alpha[on].max() - alpha[on].min() > 0.9 * 4
    assert (rec[:, 2] == 3).all() and not rec[:, 3:].any()
    assert not ER.draw(99, 3, 64, DeviceAugmenter(seed=99, da_prob=0.0, elastic={}).elastic_config())[:, :2].any()
    one = ER.draw(99, 3, 64, DeviceAugmenter(seed=99, da_prob=1.0, elastic=dict(alpha=(7, 7))).elastic_config()).view(np.uint32)
    assert (one[:, 0] == 1).all() and (one[:, 1].copy().view(np.float32) == 7).all()


FIELD_SEED = 4          # chosen so that the reference alone keeps the excluded target voxels within the cap (asserted below)


@pytest.mark.parametrize("mode, scipy_mode", [("constant", "grid-constant"), ("reflect", "mirror"), ("edge", "nearest")])
def test_twin_against_scipy_map_coordinates(mode, scipy_mode):
    """A smooth random field on a 24 x 20 plane (the twin's own noise, smoothed with sigma 4, alpha 40: displacements of several voxels that leave
    the plane at the border).  Image: scipy.ndimage.map_coordinates(order=1) in float64 at the exact coordinates, per element within
    elastic_ref.image_bound.  Target: order=0, equal outside the near ties, which are at most 1 % of the voxels."""
    from scipy import ndimage

    Y, X, alpha, cval = 24, 20, np.float32(40.0), 0.75
    s = ER.smooth(ER.noise(FIELD_SEED, 0, 1, Y, X), 4.0)
    assert np.abs(alpha * s).max() > 3                                     # the field moves voxels by several voxels
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 1, Y, X, 1, generator=g)
    t = torch.randint(0, 256, (1, 1, Y, X, 1), generator=g).to(torch.uint8)
    xo, to = ER.apply(x, t, ER.make_records([alpha]), s, mode, cval=cval)
    fy, fx = ER.coords64(alpha, s[0])
    plane = x[0, 0, :, :, 0].numpy().astype(np.float64)
    ref = ndimage.map_coordinates(plane, [fy, fx], order=1, mode=scipy_mode, cval=cval)
    bound = ER.image_bound(plane, alpha, s[0], mode, cval)
    err = np.abs(xo[0, 0, :, :, 0].numpy().astype(np.float64) - ref)
    print(f"{mode}: max err / bound = {float((err / bound).max()):.4f}, max bound = {float(bound.max()):.3e}")
    assert (bound < 1e-4).all() and (err <= bound).all(), float((err / bound).max())
    tie = ER.near_tie(alpha, s[0])
    assert tie.mean() <= 0.01, tie.mean()                                  # the cap on what may be left out
    ref_t = ndimage.map_coordinates(t[0, 0, :, :, 0].numpy().astype(np.float64), [fy, fx], order=0, mode=scipy_mode, cval=0.0)
    assert np.array_equal(to[0, 0, :, :, 0].numpy()[~tie].astype(np.float64), ref_t[~tie])
    assert (to[0, 0, :, :, 0].numpy() != t[0, 0, :, :, 0].numpy()).mean() > 0.3        # the target really moved

"""Device patch sampler - what can be checked without a GPU: the entry points are declared, exported and bound and their host-side checks name
the cause; the constructor and ``from_cfg`` validate; the host twin (tests/sampler_ref.py) keeps every origin in range, centres its class-mode
patches, and meets the five-sigma frequency bounds with the seeds the device tests use."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import sampler_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bpx_patch_draw", "bpx_patch_gather")


def _vols(L, extents, img=16, tgt=32, cls=None):
    arr = (L.PatchVol * len(extents))()
    row0 = 0
    for i, (Z, Y, X) in enumerate(extents):
        arr[i] = L.PatchVol(img, tgt, cls, Z, Y, X, 0, row0)
        row0 += Z * Y
    return arr, row0


def test_entry_points_are_declared_exported_and_bound():
    from biapy_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    source = open(os.path.join(ROOT, "biapy_amd", "csrc", "sampler.hip")).read()
    assert set(re.findall(r"\bbpx_patch_[a-z_]+(?=\()", source)) == set(NAMES)
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in L.EXPORTS and getattr(L.lib._raw, name) is not None, name
    assert "sampler.hip" in open(os.path.join(ROOT, "biapy_amd", "csrc", "Makefile")).read()
    assert re.search(r"BPX_U16 = %d\b" % L.U16, header)
    assert ctypes.sizeof(L.PatchVol) == 48 and ctypes.sizeof(L.PatchCfg) == 64          # the structs of the header, field for field


def test_host_checks_answer_without_a_device():
    from biapy_amd import _lib as L

    lib = L.lib
    vols, R = _vols(L, [(9, 21, 37), (12, 16, 40)])
    V, A = ctypes.addressof(vols), 4096                                   # A: any non-null, aligned "device" address - nothing is launched

    def err():
        return lib.bpx_last_error().decode()

    cfg = L.PatchCfg(1, 2, 4, 8, 16, 0, (ctypes.c_float * 8)())
    c = ctypes.addressof(cfg)
    assert lib.bpx_patch_draw(None, V, A, A, None, 0, 4, A, A, None) != 0 and "null pointer" in err()
    assert lib.bpx_patch_draw(c, V, A, None, None, 0, 4, A, A, None) != 0 and "null pointer (cum_d" in err()
    assert lib.bpx_patch_draw(c, V, A, A, None, 0, 0, A, A, None) != 0 and "B must be at least 1" in err()
    big = L.PatchCfg(1, 2, 4, 8, 41, 0, (ctypes.c_float * 8)())
    assert lib.bpx_patch_draw(ctypes.addressof(big), V, A, A, None, 0, 4, A, A, None) != 0 and "larger than volume 0" in err()
    cls = L.PatchCfg(1, 2, 4, 8, 16, 2, (ctypes.c_float * 8)(0.5, 1.0))
    assert lib.bpx_patch_draw(ctypes.addressof(cls), V, A, None, A, R, 4, A, A, None) != 0 and "class map of volume 0" in err()
    nine = L.PatchCfg(1, 2, 4, 8, 16, 9, (ctypes.c_float * 8)())
    assert lib.bpx_patch_draw(ctypes.addressof(nine), V, A, A, A, R, 4, A, A, None) != 0 and "1..8 classes" in err()

    def gather(vols_p=V, img=L.F32, C=1, tgt=L.U8, Ct=1, P=(4, 8, 16), B=4, x=A, t=A):
        return lib.bpx_patch_gather(vols_p, A, 2, img, C, tgt, Ct, *P, A, B, 0, 0.0, x, t, None)

    assert gather(x=None) != 0 and "null pointer" in err()
    assert gather(vols_p=ctypes.addressof(_vols(L, [(9, 21, 37), (12, 16, 40)], img=None)[0])) != 0 and "null pointer (volume 0)" in err()
    assert gather(C=17) != 0 and "1..16 image channels" in err()
    assert gather(Ct=9) != 0 and "1..8 target channels" in err()
    assert gather(Ct=0) != 0 and "1..8 target channels" in err()
    assert gather(img=L.BF16) != 0 and "float32, uint8 or uint16" in err()
    assert gather(tgt=L.U16) != 0 and "float32 or uint8" in err()
    assert gather(B=0) != 0 and "B must be at least 1" in err()
    assert gather(P=(4, 8, 38)) != 0 and "larger than volume 0" in err()
    assert gather(P=(10, 8, 16)) != 0 and "larger than volume 0" in err()
    assert gather(P=(4, 17, 16)) != 0 and "larger than volume 1" in err()


def _pair(shape=(6, 8, 10), C=1, Ct=1, idt=torch.float32, tdt=torch.uint8):
    return torch.zeros(*shape, C, dtype=idt), torch.zeros(*shape, Ct, dtype=tdt)


def test_constructor_validation():
    from biapy_amd.sampler import DevicePatchSampler as S

    x, t = _pair()
    m = torch.zeros(6, 8, 10, dtype=torch.uint8)
    cases = [
        (dict(images=x, targets=t, patch_size=(4, 4, 4), batch_size=2), "no CPU path"),
        (dict(images=[x, x], targets=[t, t], patch_size=(4, 4, 4, 1), batch_size=2), "no CPU path"),
        (dict(images=x.transpose(0, 1), targets=t.transpose(0, 1), patch_size=(4, 4, 4), batch_size=2), "non-contiguous"),
        (dict(images=x, targets=t[:, :, ::2], patch_size=(4, 4, 4), batch_size=2), "non-contiguous"),
        (dict(images=x, targets=t, patch_size=(7, 4, 4), batch_size=2), "smaller than the patch"),
        (dict(images=x, targets=t, patch_size=(4, 4, 11), batch_size=2), "smaller than the patch"),
        (dict(images=[x, _pair((3, 8, 10))[0]], targets=[t, _pair((3, 8, 10))[1]], patch_size=(4, 4, 4), batch_size=2), "volume 1"),
        (dict(images=x, targets=_pair((6, 8, 9))[1], patch_size=(4, 4, 4), batch_size=2), "mismatched extents"),
        (dict(images=x, targets=t, patch_size=(4, 4, 4), batch_size=0), "batch_size"),
        (dict(images=x, targets=t, patch_size=(4, 4), batch_size=2), "patch_size"),
        (dict(images=x, targets=t, patch_size=(4, 4, 4, 3), batch_size=2), "channels"),
        (dict(images=[x], targets=[t, t], patch_size=(4, 4, 4), batch_size=2), "pair up"),
        (dict(images=x.double(), targets=t, patch_size=(4, 4, 4), batch_size=2), "float32, uint8 or uint16"),
        (dict(images=x, targets=t.to(torch.int64), patch_size=(4, 4, 4), batch_size=2), "uint8 or float32"),
        (dict(images=_pair(C=17)[0], targets=t, patch_size=(4, 4, 4), batch_size=2), "1 to 16"),
        (dict(images=x, targets=_pair(Ct=9)[1], patch_size=(4, 4, 4), batch_size=2), "1 to 8"),
        (dict(images=[x, _pair(C=2)[0]], targets=[t, t], patch_size=(4, 4, 4), batch_size=2), "like the first"),
        (dict(images=x, targets=t, patch_size=(4, 4, 4), batch_size=2, class_maps=m), "go together"),
        (dict(images=x, targets=t, patch_size=(4, 4, 4), batch_size=2, class_probs=(0.5, 0.5)), "go together"),
        (dict(images=x, targets=t, patch_size=(4, 4, 4), batch_size=2, class_maps=m, class_probs=(-0.1, 1.1)), "not negative"),
        (dict(images=x, targets=t, patch_size=(4, 4, 4), batch_size=2, class_maps=m, class_probs=(0.0, 0.0)), "sum to 0"),
        (dict(images=x, targets=t, patch_size=(4, 4, 4), batch_size=2, class_maps=m, class_probs=[0.1] * 9), "1 to 8 classes"),
        (dict(images=x, targets=t, patch_size=(4, 4, 4), batch_size=2, class_maps=m[:5], class_probs=(0.5, 0.5)), "class_maps\\[0\\]"),
        (dict(images=x, targets=t, patch_size=(4, 4, 4), batch_size=2, class_maps=m.float(), class_probs=(0.5, 0.5)), "class_maps\\[0\\]"),
        (dict(images=x, targets=t, patch_size=(4, 4, 4), batch_size=2, class_maps=[m, m], class_probs=(0.5, 0.5)), "one map per volume"),
        (dict(images=x, targets=t, patch_size=(4, 4, 4), batch_size=2, class_maps=m, class_probs=(0.5, 0.5)), "no CPU path"),
    ]
    for kw, word in cases:
        kw = dict(kw)
        images, targets, patch = kw.pop("images"), kw.pop("targets"), kw.pop("patch_size")
        with pytest.raises(ValueError, match=word):
            S(images, targets, patch, **kw)
    with pytest.raises(TypeError):
        S(x, t, (4, 4, 4), 2)                                              # batch_size and what follows are keyword-only
    from biapy_amd.sampler import DevicePatchLoader

    with pytest.raises(ValueError, match="DevicePatchSampler"):
        DevicePatchLoader([(x, t)], 3)


def test_from_cfg_and_foreground_map():
    from biapy_amd.sampler import DevicePatchSampler as S

    x, t = _pair()
    ns = types.SimpleNamespace
    with pytest.raises(ValueError, match="DATA.PATCH_SIZE"):
        S.from_cfg(ns(DATA=ns(), TRAIN=ns(BATCH_SIZE=2)), x, t)
    with pytest.raises(ValueError, match="TRAIN.BATCH_SIZE"):
        S.from_cfg(ns(DATA=ns(PATCH_SIZE=(4, 4, 4, 1)), TRAIN=ns()), x, t)
    with pytest.raises(ValueError, match="no CPU path"):
        S.from_cfg(ns(DATA=ns(PATCH_SIZE=(4, 4, 4, 1)), TRAIN=ns(BATCH_SIZE=2)), x, t)
    with pytest.raises(ValueError, match="smaller than the patch"):
        S.from_cfg({"DATA": {"PATCH_SIZE": (8, 4, 4, 1)}, "TRAIN": {"BATCH_SIZE": 2}}, x, t)
    with pytest.raises(ValueError, match="channels"):
        S.from_cfg(ns(DATA=ns(PATCH_SIZE=(4, 4, 4, 2)), TRAIN=ns(BATCH_SIZE=2)), x, t)
    # the probability map: the class mode over the targets' foreground, its weights checked as class_probs are
    with pytest.raises(ValueError, match="not negative"):
        S.from_cfg(ns(DATA=ns(PATCH_SIZE=(4, 4, 4, 1), PROBABILITY_MAP=True, W_FOREGROUND=-1.0, W_BACKGROUND=0.1), TRAIN=ns(BATCH_SIZE=2)), x, t)
    with pytest.raises(ValueError, match="no CPU path"):
        S.from_cfg(ns(DATA=ns(PATCH_SIZE=(4, 4, 4, 1), PROBABILITY_MAP=True, W_FOREGROUND=0.9, W_BACKGROUND=0.1), TRAIN=ns(BATCH_SIZE=2)), x, t)
    assert "unverified" in " ".join(S.from_cfg.__doc__.split()) or "could not be verified" in " ".join(S.from_cfg.__doc__.split())
    tt = torch.zeros(2, 3, 4, 2)
    tt[0, 1, 2, 0], tt[1, 0, 0, 0], tt[1, 2, 3, 1] = 5.0, -1.0, 9.0        # channel 0 alone decides
    m = S.foreground_map(tt)
    assert m.dtype == torch.uint8 and m.shape == (2, 3, 4) and m.is_contiguous()
    assert m.sum() == 2 and m[0, 1, 2] == 1 and m[1, 0, 0] == 1 and m[1, 2, 3] == 0


def test_class_cum_of_the_module_is_the_twins():
    from biapy_amd.sampler import class_cum

    for probs in ([1.0], [0.2, 0.5, 0.3], [0.06, 0.94], [0.5, 0.0, 0.5], [1.0, 0.0], [0.3, 0.7, 0.0], [0.1] * 8):
        norm = [p / sum(probs) for p in probs]
        want = SR.class_cum(probs)
        got = class_cum(norm)
        assert [np.float32(g) for g in got] == want, probs
        assert got[-1] == 1.0 and all(a <= b for a, b in zip(got, got[1:]))
        last = max(i for i, p in enumerate(probs) if p > 0)
        assert all(g == 1.0 for g in got[last:]) and all(g < 1.0 for g in got[:last])


def test_twin_origins_are_in_range_and_centres_lie_inside_their_patches():
    ext, patch = [(9, 21, 37), (12, 16, 40)], (4, 8, 16)
    seen = set()
    for counter in range(4):
        o = SR.draw(77, counter, 64, ext, patch)
        for v, z0, y0, x0 in o.tolist():
            Z, Y, X = ext[v]
            assert 0 <= z0 <= Z - 4 and 0 <= y0 <= Y - 8 and 0 <= x0 <= X - 16
            seen.add(v)
    assert seen == {0, 1}
    assert not SR.draw(77, 0, 16, [(4, 8, 16)], patch).any()               # a patch equal to its volume has one origin
    assert (SR.draw(77, 0, 64, ext, patch) != SR.draw(77, 1, 64, ext, patch)).any() and (SR.draw(77, 0, 64, ext, patch) != SR.draw(78, 0, 64, ext, patch)).any()
    maps, ext = SR.hard_class_case()
    for patch in ((2, 3, 7), (1, 1, 1), (2, 3, 9)):
        Pz, Py, Px = patch
        classes = set()
        for counter in range(3):
            o, cen = SR.draw(5, counter, 64, ext, patch, class_maps=maps, class_probs=(0.3, 0.4, 0.3), centres=True)
            for (v, z0, y0, x0), (vc, z, y, x) in zip(o.tolist(), cen.tolist()):
                Z, Y, X = ext[v]
                assert v == vc and 0 <= z0 <= Z - Pz and 0 <= y0 <= Y - Py and 0 <= x0 <= X - Px
                assert z0 <= z < z0 + Pz and y0 <= y < y0 + Py and x0 <= x < x0 + Px          # the centre is inside its patch
                for c0, o0, P, D in ((z, z0, Pz, Z), (y, y0, Py, Y), (x, x0, Px, X)):
                    assert o0 == c0 - P // 2 or (o0 == 0 and c0 - P // 2 < 0) or (o0 == D - P and c0 - P // 2 > D - P)   # centred unless clamped
                classes.add(int(maps[v][z, y, x]))
                if maps[v][z, y, x] == 2:
                    assert (v, z, y, x) == (0, 1, 2, 199)
        assert classes == {0, 1, 2}
    # a class without probability is never drawn, whatever the map holds
    o, cen = SR.draw(5, 0, 256, ext, (1, 1, 1), class_maps=maps, class_probs=(0.0, 1.0, 0.0), centres=True)
    assert all(maps[v][z, y, x] == 1 for v, z, y, x in cen.tolist())


def _many(seed, **case):
    return np.concatenate([SR.draw(seed, c, SR.FREQ_B, case["extents"], case["patch"], case.get("class_maps"), case.get("class_probs"))
                           for c in range(SR.FREQ_CALLS)])


def test_uniform_frequencies_of_the_twin():
    """16,384 draws over the 26 origins of two small volumes: every origin within five sigma of N / 26 - a volume is drawn in proportion to its
    number of origins, not one volume in two."""
    cells = SR.uniform_cells(**SR.FREQ_UNIFORM)
    assert len(cells) == 26
    worst = SR.check_frequencies(_many(SR.FREQ_SEED_UNIFORM, **SR.FREQ_UNIFORM), cells)
    print("uniform mode, worst |count - N p| / (5 sigma):", worst)


def test_class_frequencies_of_the_twin():
    """16,384 draws in class mode: every origin within five sigma of the probability its centres carry (class_probs[c] / count_c per voxel)."""
    case = SR.freq_class_case()
    cells = SR.class_cells(**case)
    assert abs(sum(cells.values()) - 1.0) < 1e-12 and len(cells) == 3 * 4 * 7
    worst = SR.check_frequencies(_many(SR.FREQ_SEED_CLASS, **case), cells)
    print("class mode, worst |count - N p| / (5 sigma):", worst)

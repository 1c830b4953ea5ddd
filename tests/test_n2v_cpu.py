"""Noise2Void masking and its masked MSE - what can be checked without a GPU: the entry points are declared, exported and bound; every host-side
refusal of the C entry points, the constructor, ``from_cfg`` and the call names its cause, in the stated order, before anything is launched;
the NumPy twin the GPU tests hold the device against (tests/n2v_ref.py) reproduces the known answers of the stated rule and has its properties;
the fp64 reference of the loss (tests/n2v_bounds.py) agrees with torch autograd in float64 and its bounds reject seeded defects; no kernel of
n2v.hip keeps scratch; and scripts/n2v_cpu_check.cpp walks n2v_core.h under ASan / UBSan as a stand-alone host program."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import n2v_bounds as NB
import n2v_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
A = 1 << 30                                # any non-null, aligned "device" address: nothing is launched


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _cfg(box=(4, 4, 4), radius=(2, 2, 2), manip=0, sigma=1.0, seed=31):
    from biapy_amd import _lib as L

    return L.N2VCfg(seed, (C.c_int32 * 3)(*box), (C.c_int32 * 3)(*radius), manip, sigma)


def test_entry_points_are_declared_exported_and_bound():
    import biapy_amd
    from biapy_amd import _lib as L
    from biapy_amd import losses, n2v

    header, source, core = _read("include", "biapy_amd.h"), _read("biapy_amd", "csrc", "n2v.hip"), _read("biapy_amd", "csrc", "n2v_core.h")
    names = ["bpx_n2v_boxes", "bpx_n2v_mask", "bpx_n2v_loss_blocks", "bpx_n2v_loss_sums", "bpx_n2v_loss_finish", "bpx_n2v_loss_bwd"]
    assert re.findall(r'extern "C" \w+ (\w+)\(', source) == names
    for n in names:
        assert re.search(r"^int(64_t)? %s\(" % n, header, re.M), n
    assert set(names) <= set(L.EXPORTS)
    vp, i, i64 = C.c_void_p, C.c_int, C.c_int64
    assert L._SIGS["bpx_n2v_boxes"] == ([vp, i, i, i], i64)
    assert L._SIGS["bpx_n2v_mask"] == ([vp, i, i, i, i, i, vp, vp, vp, vp, vp, vp, vp], i)
    assert L._SIGS["bpx_n2v_loss_sums"] == ([vp, vp, i, i, i64, vp, vp], i)
    assert L._SIGS["bpx_n2v_loss_finish"] == ([vp, i, i, i64, vp, vp], i)
    assert L._SIGS["bpx_n2v_loss_bwd"] == ([vp, vp, i, i, i64, vp, vp, vp, vp], i)
    assert C.sizeof(L.N2VCfg) == 40
    make = _read("biapy_amd", "csrc", "Makefile")
    assert "n2v.hip" in make and re.search(r"^n2v\.o:.*n2v_core\.h", make, re.M)
    # one text for device and host; no atomics anywhere
    assert '#include "n2v_core.h"' in source and "n2v_box(" in source and not re.search(r"\bN2V_HD\b", source)
    assert re.search(r"N2V_HD N2VPick n2v_box\(", core) and not re.search(r"atomic\w*\(", source + core)
    check = _read("scripts", "n2v_cpu_check.cpp")
    assert '#include "n2v_core.h"' in check and "int main()" in check and "-fsanitize=address,undefined" in check and "n2v_box(" in check
    assert biapy_amd.N2VMasker is n2v.N2VMasker and issubclass(losses.N2VLoss, torch.nn.Module)
    assert n2v.KEY_XOR == R.KEY_XOR == int(re.search(r"N2V_KEY_XOR (0x[0-9A-Fa-f]+)u", core).group(1), 16) == 0x4E32564D
    assert tuple(n2v.MANIPULATORS) == R.MANIPULATORS
    for name, code in n2v.MANIPULATORS.items():
        assert int(re.search(r"BPX_N2V_%s (\d)" % name.upper().replace("WITHCP", "WITH_CP").replace("WITHOUTCP", "WITHOUT_CP"), header).group(1)) == code
    assert not hasattr(losses.N2VLoss(), "fused_head_activations")
    assert L.lib.bpx_n2v_loss_blocks(1) == 1 and L.lib.bpx_n2v_loss_blocks(1025) == 2 and L.lib.bpx_n2v_loss_blocks(1024 * 512 + 1) == 512


def test_host_side_argument_checks_of_the_entry_points():
    """The order stated in include/biapy_amd.h: null pointers, B, C, extents, the 2^31-voxel sample, the manipulator, box and radius per axis,
    sigma, the box count, alignment, overlap - each call below is wrong in that one respect and in every later one listed after it."""
    from biapy_amd import _lib as L

    lib = L.lib

    def err():
        return lib.bpx_last_error()

    good = _cfg()
    ok = C.addressof(good)
    n = 4 * 8 * 8 * 8
    X_, S_, O_, T_, K_, Q_ = A, A + (1 << 20), A + (2 << 20), A + (3 << 20), A + (5 << 20), A + (6 << 20)

    def mask(x=X_, B=1, Z=8, Y=8, X=8, Cc=1, cfg=ok, st=S_, xo=O_, t=T_, co=K_, so=Q_):
        return lib.bpx_n2v_mask(x, B, Z, Y, X, Cc, cfg, st, xo, t, co, so, None)

    for kw in (dict(x=None), dict(cfg=None), dict(st=None), dict(xo=None), dict(t=None), dict(co=None), dict(so=None)):
        assert mask(B=0, **kw) != 0 and b"null pointer" in err(), kw
    assert mask(B=0, Cc=0) != 0 and b"samples" in err()
    assert mask(B=1 << 24, Cc=0) != 0 and b"samples" in err()
    assert mask(Cc=0, Z=0) != 0 and b"channels" in err()
    assert mask(Cc=9, Z=0) != 0 and b"channels" in err()
    bad_manip = _cfg(manip=4)
    assert mask(Z=0, cfg=C.addressof(bad_manip)) != 0 and b"bad extents" in err()
    assert mask(Z=2048, Y=1024, X=1024, cfg=C.addressof(bad_manip)) != 0 and b"2^31 or more" in err()
    bad = _cfg(manip=4, box=(0, 4, 4))
    assert mask(cfg=C.addressof(bad)) != 0 and b"unknown manipulator" in err()
    bad = _cfg(manip=-1)
    assert mask(cfg=C.addressof(bad)) != 0 and b"unknown manipulator" in err()
    for box in ((0, 4, 4), (4, 65, 4), (4, 4, -1)):
        bad = _cfg(box=box, sigma=float("inf"))
        assert mask(cfg=C.addressof(bad)) != 0 and b"box edge" in err(), box
    for radius in ((16, 2, 2), (2, -1, 2), (2, 2, 99)):
        bad = _cfg(radius=radius, sigma=float("inf"))
        assert mask(cfg=C.addressof(bad)) != 0 and b"radius" in err(), radius
    for sigma in (float("inf"), float("nan")):
        bad = _cfg(sigma=sigma)
        assert mask(cfg=C.addressof(bad), x=A + 2) != 0 and b"sigma must be finite" in err()
    for kw in (dict(x=A + 2), dict(xo=O_ + 1), dict(t=T_ + 2), dict(co=K_ + 2), dict(so=Q_ + 3), dict(st=S_ + 4)):
        assert mask(**kw) != 0 and b"aligned" in err(), kw
    for kw in (dict(xo=X_), dict(xo=X_ + n - 4), dict(t=X_ + 4), dict(t=X_ - 2 * n + 4), dict(xo=T_ + 2 * n - 4), dict(xo=T_ - n + 4)):
        assert mask(B=4, **kw) != 0 and b"cannot run in place" in err(), kw
    # an axis of extent 1 takes s = 1 and radius 0 whatever the configuration says; the box count
    wide = _cfg(box=(64, 22, 22), radius=(15, 5, 5))
    assert lib.bpx_n2v_boxes(C.addressof(wide), 1, 45, 50) == 9
    eight = _cfg(box=(8, 8, 8))
    assert lib.bpx_n2v_boxes(ok, 13, 22, 37) == 240 and lib.bpx_n2v_boxes(ok, 3, 5, 7) == 4 and lib.bpx_n2v_boxes(C.addressof(eight), 3, 5, 7) == 1
    ones = _cfg(box=(1, 1, 1))
    assert lib.bpx_n2v_boxes(C.addressof(ones), 8, 8, 8) == 512
    assert lib.bpx_n2v_boxes(C.addressof(ones), 1024, 1024, 2047) == 1024 * 1024 * 2047
    assert lib.bpx_n2v_boxes(None, 8, 8, 8) == -1 and b"null pointer" in err()
    assert lib.bpx_n2v_boxes(ok, 8, 0, 8) == -1 and b"bad extents" in err()
    # the loss
    for fn, args in (("bpx_n2v_loss_sums", (A, A, 1, 1, 4, A)), ("bpx_n2v_loss_finish", (A, 1, 1, 4, A)), ("bpx_n2v_loss_bwd", (A, A, 1, 1, 4, A, A, A))):
        f = getattr(lib, fn)
        for k, a in enumerate(args):
            if a == A:
                assert f(*args[:k], None, *args[k + 1:], None) != 0 and b"null pointer" in err(), (fn, k)
    assert lib.bpx_n2v_loss_sums(A, A, 0, 1, 4, A, None) != 0 and b"bad extents" in err()
    assert lib.bpx_n2v_loss_sums(A, A, 1, 9, 4, A, None) != 0 and b"bad extents" in err()
    assert lib.bpx_n2v_loss_finish(A, 1, 1, 0, A, None) != 0 and b"bad extents" in err()
    assert lib.bpx_n2v_loss_bwd(A, A, 8192, 8, 4, A, A, A, None) != 0 and b"exceed one launch" in err()


def test_constructor_from_cfg_and_call_refusals():
    from biapy_amd.augment import DeviceAugmenter
    from biapy_amd.losses import N2VLoss
    from biapy_amd.n2v import N2VMasker, derived_box

    for name in ("normal_withoutCP", "normal_fitted", "mean", "median", "structN2V"):
        with pytest.raises(NotImplementedError, match=name):
            N2VMasker(manipulator=name)
    with pytest.raises(ValueError, match="manipulator must be one of"):
        N2VMasker(manipulator="uniform")
    for p in (0.0, -1.0, 100.5, float("nan"), "x"):
        with pytest.raises(ValueError, match="perc_pix"):
            N2VMasker(perc_pix=p)
    for box in (0, 65, (4, 4), (4, 0, 4), (1, 2, 3, 4), "abc"):
        if box == (4, 4):
            assert N2VMasker(box=box, seed=1).box == (1, 4, 4)               # the 2-D spelling
            continue
        with pytest.raises(ValueError, match="box"):
            N2VMasker(box=box)
    for radius in (-1, 16, (1, 2, 3, 4), None):
        with pytest.raises(ValueError, match="radius"):
            N2VMasker(radius=radius)
    for sigma in (float("inf"), float("nan"), "s"):
        with pytest.raises(ValueError, match="sigma"):
            N2VMasker(sigma=sigma)
    with pytest.raises(ValueError, match="DeviceAugmenter"):
        N2VMasker(augment=lambda x, t: (x, t))
    with pytest.raises(ValueError, match="seed"):
        N2VMasker(seed="seed")
    m = N2VMasker(seed=-1, augment=DeviceAugmenter(seed=1))
    assert m.seed == 2 ** 64 - 1 and m.config()["box"] is None and m.radius == (5, 5, 5)
    assert derived_box(0.198, (32, 32, 32)) == 8 == R.derived_box(0.198, (32, 32, 32)) and derived_box(0.198, (1, 64, 64)) == 22 == R.derived_box(0.198, (1, 64, 64))
    assert m.grid(32, 32, 32) == ((8, 8, 8), (5, 5, 5)) and m.grid(1, 64, 64) == ((1, 22, 22), (0, 5, 5)) == R.grid((1, 64, 64))[:2]
    assert m.config((1, 64, 64))["box"] == (1, 22, 22) and derived_box(100.0, (8, 8, 8)) == 1
    with pytest.raises(ValueError, match="derives a box edge"):
        N2VMasker(perc_pix=0.001).grid(1, 512, 512)
    # the call: every refusal comes before anything touches a device
    with pytest.raises(ValueError, match="CUDA/HIP tensor"):
        m(torch.zeros(1, 8, 8, 8, 1))
    with pytest.raises(ValueError, match="CUDA/HIP tensor"):
        m(np.zeros((1, 8, 8, 8, 1), np.float32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        N2VLoss()(torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 2, 4, 4, 4))
    with pytest.raises(ValueError, match="twice its channels"):
        N2VLoss()(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 2, 4, 4, 4))
    with pytest.raises(NotImplementedError, match="1 to 8 channels"):
        N2VLoss()(torch.zeros(1, 9, 4, 4), torch.zeros(1, 18, 4, 4))
    # from_cfg
    ns = types.SimpleNamespace
    assert N2VMasker.from_cfg(ns(PROBLEM=ns(TYPE="SEMANTIC_SEG"))) is None
    d = ns(N2V_PERC_PIX=1.5, N2V_MANIPULATOR="uniform_withoutCP", N2V_NEIGHBORHOOD_RADIUS=3, N2V_STRUCTMASK=False)
    got = N2VMasker.from_cfg(ns(PROBLEM=ns(TYPE="DENOISING", DENOISING=d)), seed=7)
    assert (got.perc_pix, got.manipulator, got.radius, got.seed, got.box) == (1.5, "uniform_withoutCP", (3, 3, 3), 7, None)
    dflt = N2VMasker.from_cfg(ns(PROBLEM=ns(TYPE="DENOISING", DENOISING=ns())), seed=7)
    assert (dflt.perc_pix, dflt.manipulator, dflt.radius) == (0.198, "uniform_withCP", (5, 5, 5))
    d.N2V_STRUCTMASK = True
    with pytest.raises(NotImplementedError, match="N2V_STRUCTMASK"):
        N2VMasker.from_cfg(ns(PROBLEM=ns(TYPE="DENOISING", DENOISING=d)))
    d.N2V_STRUCTMASK, d.N2V_MANIPULATOR = False, "median"
    with pytest.raises(NotImplementedError, match="median"):
        N2VMasker.from_cfg(ns(PROBLEM=ns(TYPE="DENOISING", DENOISING=d)))
    assert "from memory" in " ".join(N2VMasker.from_cfg.__doc__.split())


# ---- the twin ----------------------------------------------------------------------------------------------------------------------------------------------

def _stats(shape, box, radius, manip):
    c, s, _, _ = R.draw(31, 0, 1, 1, shape, box, radius, manip)
    c, s = c[0, 0], s[0, 0]
    on = c >= 0
    assert len(np.unique(c[on])) == on.sum()                     # the masked voxels are distinct
    assert ((s >= 0) == on).all()
    return len(c), int(on.sum()), int((c[on] == s[on]).sum())


def test_known_answers_of_the_stated_rule():
    assert _stats((13, 22, 37), 4, 2, "uniform_withCP") == (240, 167, 3)
    assert _stats((13, 22, 37), 4, 2, "uniform_withoutCP") == (240, 167, 0)
    assert _stats((1, 45, 50), (1, 22, 22), (0, 5, 5), "uniform_withCP")[:2] == (9, 5)
    for radius in (0, 2, 15):
        assert _stats((3, 5, 7), 8, radius, "uniform_withCP")[:2] == (1, 0)
    assert _stats((8, 8, 8), 1, 1, "uniform_withCP") == (512, 512, 28)
    assert _stats((8, 8, 8), 1, 1, "uniform_withoutCP") == (512, 512, 0)
    c = R.draw(31, 0, 1, 1, (64, 64, 64), 4, 2)[0][0, 0]
    assert (c >= 0).all()
    z, y, x = c // 4096, (c // 64) % 64, c % 64
    cnt = np.bincount(((z % 4) * 4 + (y % 4)) * 4 + (x % 4), minlength=64)
    n, p = 4096, 1 / 64
    lo, hi = n * p - 5 * np.sqrt(n * p * (1 - p)), n * p + 5 * np.sqrt(n * p * (1 - p))
    assert (cnt.min(), cnt.max()) == (40, 77) and round(lo, 1) == 24.3 and round(hi, 1) == 103.7 and lo <= cnt.min() and cnt.max() <= hi


@pytest.mark.parametrize("manip", R.MANIPULATORS)
def test_twin_properties(manip):
    for shape, box, radius in (((13, 22, 37), 4, 2), ((1, 45, 50), None, 5), ((6, 7, 9), (2, 3, 4), (1, 0, 15)), ((8, 8, 8), 1, 1), ((12, 8, 16), 4, 3)):
        Z, Y, X = shape
        for counter in (0, 5, 2 ** 32 - 1, 2 ** 32):
            c, s, _, _ = R.draw(77, counter, 3, 2, shape, box, radius, manip)
            on = c >= 0
            assert ((s >= 0) == on).all() and c.max() < Z * Y * X and s.max() < Z * Y * X
            (sz, sy, sx), (rz, ry, rx), (nz, ny, nx) = R.grid(shape, box, radius)
            pz, py, px = c // (Y * X), (c // X) % Y, c % X
            qz, qy, qx = s // (Y * X), (s // X) % Y, s % X
            i = np.arange(nz * ny * nx)[None, None]
            assert ((pz // sz == i // (ny * nx)) & (py // sy == (i // nx) % ny) & (px // sx == i % nx))[on].all()            # inside its own box
            assert ((abs(qz - pz) <= rz) & (abs(qy - py) <= ry) & (abs(qx - px) <= rx))[on].all()                             # inside the clipped window
            if manip == "uniform_withoutCP":
                assert (c != s)[on].all()
            if manip in ("identity", "normal_additive"):
                assert (c == s).all()
            if all(n % e == 0 for n, e in zip(shape, (sz, sy, sx))):
                assert on.all()                                   # exactly one per box on divisible shapes
            for b in range(3):
                for ch in range(2):
                    assert len(np.unique(c[b, ch][on[b, ch]])) == on[b, ch].sum()
        a, b = R.draw(77, 0, 1, 1, shape, box, radius, manip)[0], R.draw(77, 1, 1, 1, shape, box, radius, manip)[0]
        assert box == 1 or a.size == 1 or not np.array_equal(a, b)          # the counter matters (box 1 masks every voxel in every call)


def test_window_picks_are_uniform_at_a_corner_an_edge_and_an_interior_voxel():
    """box = the whole sample would fix nothing; instead every voxel is its own box (box 1), so voxel p is masked in every call and its pick over
    many counter values is a sample of the window's uniform distribution: five-sigma bands of the multinomial counts."""
    shape, radius, calls = (5, 6, 7), 1, 1200
    Z, Y, X = shape
    picks = np.stack([R.draw(5, q, 1, 1, shape, 1, radius, "uniform_withCP")[1][0, 0] for q in range(calls)])      # (calls, V)
    picks_no = np.stack([R.draw(5, q, 1, 1, shape, 1, radius, "uniform_withoutCP")[1][0, 0] for q in range(calls)])
    for (z, y, x), n in (((0, 0, 0), 8), ((0, 3, 0), 12), ((2, 3, 3), 27)):
        p = (z * Y + y) * X + x
        for col, k in ((picks[:, p], n), (picks_no[:, p], n - 1)):
            vals, cnt = np.unique(col, return_counts=True)
            assert len(vals) == k, (z, y, x, len(vals))
            mean, sd = calls / k, np.sqrt(calls * (1 / k) * (1 - 1 / k))
            assert (abs(cnt - mean) <= 5 * sd).all(), (z, y, x, cnt)
        assert p not in picks_no[:, p]


def test_corner_seeds():
    """The GPU test's masking cases on the (6, 7, 9) sample: every one of the 8 corners is masked at least once across them."""
    Z, Y, X = R.CORNER_SHAPE
    corners = {(a * Y + b) * X + d for a in (0, Z - 1) for b in (0, Y - 1) for d in (0, X - 1)}
    hit = set()
    for case in R.CORNER_CASES:
        c = R.draw(case["seed"], 0, 1, 1, R.CORNER_SHAPE, case["box"], case["radius"], case["manipulator"])[0]
        hit |= corners & set(c.reshape(-1).tolist())
    assert hit == corners and {c["manipulator"] for c in R.CORNER_CASES} == set(R.MANIPULATORS)


def test_twin_mask_and_target():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 5, 6, 7, 3)).astype(np.float32)
    for manip in ("uniform_withCP", "uniform_withoutCP", "identity"):
        xm, t, c, s = R.mask(x, 9, 4, box=2, radius=1, manipulator=manip)
        assert t.shape == (2, 6, 5, 6, 7) and xm.shape == x.shape
        m = t[:, 3:].transpose(0, 2, 3, 4, 1).astype(bool)
        assert np.array_equal(xm[~m].view(np.uint32), x[~m].view(np.uint32)) and m.sum() == (c >= 0).sum()
        assert np.array_equal(t[:, :3].transpose(0, 2, 3, 4, 1)[m], x[m]) and (t[:, :3].transpose(0, 2, 3, 4, 1)[~m] == 0).all()
        xf = x.reshape(2, -1, 3)
        for b in range(2):
            for ch in range(3):
                on = c[b, ch] >= 0
                assert np.array_equal(xm.reshape(2, -1, 3)[b, c[b, ch][on], ch], xf[b, s[b, ch][on], ch])
        if manip == "identity":
            assert np.array_equal(xm, x)


# ---- the loss ----------------------------------------------------------------------------------------------------------------------------------------------

def _autograd(pred, target, g):
    p = pred.double().clone().requires_grad_(True)
    Cc = pred.shape[1]
    v, m = target.double()[:, :Cc], target.double()[:, Cc:]
    loss = ((v - p * m) ** 2).sum() / m.sum()
    (loss * g).backward()
    return loss.detach(), p.grad


@pytest.mark.parametrize("kind", ["sparse", "ones", "fraction"])
def test_reference_against_autograd_and_seeded_defects(kind):
    from biapy_amd import _lib as L

    for V in (1, 257, 1025):
        for Cc in (1, 3):
            gen = torch.Generator().manual_seed(NB.seed_of(V, Cc))
            pred, target = NB.fixture(gen, 2, Cc, V, kind)
            g = NB.f32(1.7)
            ref = NB.reference(pred, target, g)
            loss, grad = _autograd(pred, target, g)
            assert torch.allclose(ref["loss"], loss, rtol=1e-13, atol=0) and torch.allclose(ref["grad"], grad, rtol=1e-12, atol=1e-300)
            bnd = NB.bounds(ref, L.lib.bpx_n2v_loss_blocks(V))
            # the bounds are tight enough to matter: a few hundred ulp of the loss at most, and every seeded defect leaves them
            assert float(bnd["loss"]) <= 400 * NB.U32 * max(float(ref["loss"]), 1e-30)
            assert all(r["ok"] for r in NB.check("self", ref["loss"], ref["grad"], ref, bnd))
            for fault in NB.FAULTS:
                bad = NB.reference(pred, target, g, fault=fault)
                if torch.equal(bad["loss"], ref["loss"]) and torch.equal(bad["grad"], ref["grad"]):
                    # the defect cannot show on this input: a single voxel, or m = 1 everywhere (pred m = pred, sum m = the element count)
                    assert V == 1 or (kind == "ones" and fault in ("mask_not_applied_to_pred", "mean_over_voxels_not_sum_m")), (fault, V, Cc, kind)
                    continue
                rows = NB.check(fault, bad["loss"], bad["grad"], ref, bnd)
                assert not all(r["ok"] for r in rows), (fault, V, Cc, kind)


def test_reference_with_nothing_masked():
    pred, target = NB.fixture(torch.Generator().manual_seed(1), 2, 3, 300, "zeros")
    ref = NB.reference(pred, target, 1.7)
    assert float(ref["loss"]) == 0 and not ref["grad"].any() and NB.bounds(ref, 1)["exact"]
    rows = NB.check("zeros", torch.zeros(()), torch.zeros(2, 3, 300), ref, NB.bounds(ref, 1))
    assert all(r["ok"] for r in rows)
    rows = NB.check("zeros", torch.tensor(float("nan")), torch.zeros(2, 3, 300), ref, NB.bounds(ref, 1))
    assert not rows[0]["ok"]


# ---- the compiled code ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc to cross-compile the kernels to ISA")
def test_no_kernel_of_n2v_keeps_scratch(tmp_path):
    out = str(tmp_path / "n2v.s")
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-result", "-S", "--cuda-device-only",   # the Makefile's flags
           os.path.join(ROOT, "biapy_amd", "csrc", "n2v.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)} failed:\n{r.stderr[-3000:]}"
    text = open(out).read()
    kernels = re.findall(r"\.name:\s+(_Z\w*n2v_\w*kernel\w*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(kernels) == 5, kernels
    for name, private in kernels:
        assert int(private) == 0, f"{name} keeps {private} bytes of scratch per lane"
    assert "global_atomic" not in text and "flat_atomic" not in text and "ds_add" not in text


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host compiler")
def test_host_walk_of_the_core_under_sanitizers(tmp_path):
    """scripts/n2v_cpu_check.cpp as a stand-alone program of its own under ASan / UBSan, on the host only: nothing loaded into Python is checked this way."""
    exe = str(tmp_path / "n2v_cpu_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "biapy_amd", "csrc"),
           os.path.join(ROOT, "scripts", "n2v_cpu_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)} failed:\n{r.stderr[-3000:]}"
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "every index in range" in r.stdout, r.stdout + r.stderr[-3000:]

"""Intensity properties - what can be checked without a GPU: the entry points are declared, exported and bound; every host-side refusal of
``bpx_intensity_props`` names its cause, in the stated order, before anything is launched; ``prepost.intensity_props`` refuses in its order; the
twin the GPU tests hold the device against (tests/intensityprops_ref.py) agrees with independent statements on every input those tests use - its
limbs with the exact ``fractions.Fraction`` sum, its ``sum`` with ``math.fsum`` bit for bit, its ``min`` / ``max`` with ``scipy.ndimage``, its
``sum`` with ``scipy.ndimage.sum_labels`` within the bound of a naive float64 sum; the library's two host entry points run the core header's
per-voxel decomposition and rounding against the twin; hand-made cases; the comparisons catch three seeded defects; no kernel uses scratch."""
import ctypes as C
import math
import os
import random
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import intensityprops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NAMES = ("bpx_intensity_props", "bpx_debug_set_intensityprops_wave", "bpx_intensity_pieces_host", "bpx_intensity_round_host")
A = 4096                                   # any non-null, aligned "device" address: nothing is launched


def test_entry_points_are_declared_exported_and_bound():
    from biapy_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    source = open(os.path.join(ROOT, "biapy_amd", "csrc", "intensityprops.hip")).read()
    assert set(re.findall(r'extern "C" \w+ (\w+)\(', source)) == set(NAMES)
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in L.EXPORTS and getattr(L.lib._raw, name) is not None, name
        assert getattr(L.lib._raw, name).restype is L.C.c_int
    vp, i = L.C.c_void_p, L.C.c_int
    assert L._SIGS["bpx_intensity_props"][0] == [vp, vp, i, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp]
    assert L._SIGS["bpx_debug_set_intensityprops_wave"][0] == [i]
    lib_src = open(os.path.join(ROOT, "biapy_amd", "_lib.py")).read()
    assert re.search(r'\("BPX_INTENSITYPROPS_WAVE", "bpx_debug_set_intensityprops_wave"\)', lib_src)      # with the other BPX_* switches
    make = open(os.path.join(ROOT, "biapy_amd", "csrc", "Makefile")).read()
    assert "intensityprops.hip" in make and re.search(r"^intensityprops\.o:.*intensityprops_core\.h.*regionprops_core\.h.*peaks_core\.h.*label_walk\.h", make, re.M)
    core = open(os.path.join(ROOT, "biapy_amd", "csrc", "intensityprops_core.h")).read()
    assert '#include "intensityprops_core.h"' in source and not re.search(r"\bIP_HD \w+ ip_\w+\(", source)      # the shared steps, not a copy
    for fn in ("ip_voxel_f32", "ip_voxel_int", "ip_fits", "ip_absorb", "ip_apply", "ip_emit", "ip_merge", "ip_round_bits", "ip_sum_rule", "ip_init_row",
               "ip_finish_row"):
        assert re.search(r"IP_HD \w+ %s\(" % fn, core) and fn in source + core, fn
    assert "peaks_okey" in core and "peaks_unokey" in core and "rp_local_slot" in core      # the key and the slot scheme are the shared ones
    walk = open(os.path.join(ROOT, "biapy_amd", "csrc", "label_walk.h")).read()       # the table's key policy and the label load are the shared ones
    assert '#include "label_walk.h"' in source and ": LwKeysLds" in source and "lw_load4(" in source and "kcas(" not in source
    assert "atomicAdd" not in source + walk and set(re.findall(r"__hip_atomic_(\w+)\(", source)) == {"fetch_add", "fetch_min", "fetch_max"}
    assert set(re.findall(r"__hip_atomic_(\w+)\(", walk)) == {"fetch_add", "load", "compare_exchange_strong"}      # integer atomics only
    check = open(os.path.join(ROOT, "scripts", "intensityprops_cpu_check.cpp")).read()
    assert '#include "intensityprops_core.h"' in check and "int main()" in check and "-fsanitize=address,undefined" in check
    from biapy_amd import prepost

    assert prepost.IntensityProps._fields == R.FIELDS


def test_host_checks_answer_without_a_device_in_the_stated_order():
    from biapy_amd import _lib as L

    lib = L.lib
    F32, U16 = L.F32, L.U16

    def err():
        return lib.bpx_last_error().decode()

    def call(labels=A, image=A, dtype=F32, Z=4, Y=5, X=6, n_max=3, area=A, vmin=A, vmax=A, limbs=A, nonf=A, total=A, mean=A):
        return lib.bpx_intensity_props(labels, image, dtype, Z, Y, X, n_max, area, vmin, vmax, limbs, nonf, total, mean, None)

    for k in ("labels", "image", "area", "vmin", "vmax", "limbs", "nonf", "total", "mean"):
        assert call(**{k: None}) != 0 and "null pointer" in err(), k
        assert call(Y=0, n_max=-1, dtype=9, **{k: None}) != 0 and "null pointer" in err(), k         # the first refusal wins
    for kw in (dict(Z=0), dict(Y=0), dict(X=0), dict(X=-7), dict(Z=-1)):
        assert call(n_max=-1, dtype=9, **kw) != 0 and "extents must be at least 1" in err(), kw
    for Z, Y, X in ((1, 65536, 32768), (2048, 1024, 1024), (1, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert call(Z=Z, Y=Y, X=X, n_max=-1, dtype=9) != 0 and "2^31 voxels or more" in err(), (Z, Y, X)
    for n_max in (-1, -2 ** 31, 2 ** 31 - 1):
        assert call(n_max=n_max, dtype=9, labels=A + 2) != 0 and "n_max must be in [0, 2^31 - 1)" in err(), n_max
    for dtype in (L.BF16, L.F16, L.MIX16, L.I32, 7, -1):
        assert call(dtype=dtype, labels=A + 2) != 0 and "image dtype must be BPX_F32, BPX_U8 or BPX_U16" in err(), dtype
    for kw in (dict(labels=A + 2), dict(area=A + 1), dict(vmin=A + 2), dict(vmax=A + 3), dict(nonf=A + 2), dict(limbs=A + 4), dict(total=A + 4),
               dict(mean=A + 4), dict(image=A + 2), dict(image=A + 1), dict(image=A + 1, dtype=U16), dict(image=A + 3, dtype=U16)):
        assert call(**kw) != 0 and "aligned" in err(), kw
    # the largest admitted row and label range pass every check but the last one made here
    assert call(Z=1, Y=1, X=2 ** 31 - 1, n_max=2 ** 31 - 2, limbs=A + 4) != 0 and "aligned" in err()
    for name, args in (("bpx_intensity_pieces_host", (0, None, None, None)), ("bpx_intensity_round_host", (None, 9, None))):
        assert getattr(lib, name)(*args) != 0 and "null pointer" in err(), name
    out, limbs = C.c_double(), (C.c_int64 * 9)()
    for nl in (0, 2, 8, 10, -1):
        assert lib.bpx_intensity_round_host(limbs, nl, C.byref(out)) != 0 and "nl must be 9" in err(), nl
    assert lib.bpx_debug_set_intensityprops_wave(1) == 0 and lib.bpx_debug_set_intensityprops_wave(0) == 0 and lib.bpx_debug_set_intensityprops_wave(-1) == 0


def test_prepost_refuses_before_any_launch():
    from biapy_amd import prepost

    a = torch.zeros(4, 5, 6, dtype=torch.int32)
    x = torch.zeros(4, 5, 6, dtype=torch.float32)
    for bad in (a.view(-1), a[None], a[0, 0, 0]):
        with pytest.raises(ValueError, match="2-D .* or 3-D"):
            prepost.intensity_props(bad, x, -1)                                              # the first refusal wins
    for num in (-1, -100, torch.tensor(-2)):
        with pytest.raises(ValueError, match="num must not be negative"):
            prepost.intensity_props(a, x[:3], num)
    for bad in (x[:3], x[0], x.view(4, 6, 5), x[None]):
        with pytest.raises(ValueError, match="must have the labels' shape"):
            prepost.intensity_props(a, bad, 3)
    for lab, img in ((a, x), (a[0], x[0]), (a.long(), x), (a, x.double())):                  # the device is named before either dtype
        with pytest.raises(RuntimeError, match="no CPU path"):
            prepost.intensity_props(lab, img, 3)
    assert prepost._INTENSITY_DTYPES[torch.float32][1:] == (9, torch.float32) and prepost._INTENSITY_DTYPES[torch.uint8][1:] == (1, torch.int32)
    assert prepost._INTENSITY_DTYPES[torch.uint16][1:] == (1, torch.int32)
    assert prepost.RegionProps._fields == ("area", "bbox", "coord_sum", "centroid")          # left as they are
    assert prepost.ShapeProps._fields[:4] == prepost.RegionProps._fields and len(prepost.ShapeProps._fields) == 8


# ---- the twin against independent statements ---------------------------------------------------------------------------------------------------------

def _f64(a):
    with np.errstate(invalid="ignore"):                                                      # a signalling NaN among the inputs raises the flag when widened
        return np.asarray(a).astype(np.float64)


def _values_by_label(labels, image, n_max):
    c = R.clean(labels, n_max).ravel()
    order = np.argsort(c, kind="stable")
    cs, vs = c[order], np.asarray(image).ravel()[order]
    starts = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]])
    return {int(cs[s]): vs[s:e] for s, e in zip(starts, np.r_[starts[1:], cs.size]) if cs[s] > 0}


@pytest.mark.parametrize("name", list(R.cases()), ids=str)
def test_the_twin_sum_equals_fsum_and_its_limbs_the_exact_sum_on_every_gpu_input(name):
    labels, image, n_max = R.cases()[name]
    want = R.ref(name)
    groups = _values_by_label(labels, image, n_max)
    assert sorted(groups) == np.flatnonzero(want["area"]).tolist()
    unit = -149 if image.dtype == np.float32 else 0
    assert want["sum_limbs"].shape == (n_max + 1, 9 if unit else 1) and want["sum_limbs"].dtype == np.int64 and want["sum"].dtype == np.float64
    for k, l in enumerate(groups):
        v = _f64(groups[l])                                                                  # exact for all three image types
        finite = v[np.isfinite(v)]
        exact = R.sum_rule(math.fsum(finite.tolist()), np.isnan(v).sum(), (v == np.inf).sum(), (v == -np.inf).sum())
        if exact == 0:
            exact = 0.0                                                                      # an exact zero is +0.0, whatever the signs of the zeros
        assert R.same_bits(np.float64(want["sum"][l]), np.float64(exact)), (name, l, want["sum"][l], exact)
        if k < 300:                                                                          # 300 labels a case: Fractions are slow
            u, count = np.unique(finite, return_counts=True)
            assert R.limbs_value(want["sum_limbs"][l], unit) == sum((Fraction(float(t)) * int(c) for t, c in zip(u, count)), Fraction(0)), (name, l)
        assert (np.abs(want["sum_limbs"][l]) < 2 ** 63 - 2 ** 32).all()
        assert want["mean"][l] == want["sum"][l] / want["area"][l] or np.isnan(want["mean"][l])
    absent = want["area"] == 0
    assert absent[0] and np.isnan(want["mean"][absent]).all() and not want["sum_limbs"][absent].any() and not want["nonfinite"][absent].any()
    assert not want["sum"][absent].view(np.int64).any() and not want["min"][absent].view(np.int32).any() and not want["max"][absent].view(np.int32).any()
    assert int(np.abs(want["sum_limbs"]).max(initial=0)) < 2 ** 63 - 2 ** 32


@pytest.mark.parametrize("name", list(R.cases()), ids=str)
def test_the_twin_against_scipy_on_every_gpu_input(name):
    from scipy import ndimage

    labels, image, n_max = R.cases()[name]
    want = R.ref(name)
    present = np.flatnonzero(want["area"])
    if not len(present):
        return
    c = R.clean(labels, n_max)
    x = _f64(image)
    nan = np.isnan(x)
    if image.dtype == np.float32:
        lo, hi = ndimage.minimum(np.where(nan, np.inf, x), c, present), ndimage.maximum(np.where(nan, -np.inf, x), c, present)     # NaN voxels are left out
        some = want["area"][present] > want["nonfinite"][present, 0]                         # a label of NaN voxels alone has min = max = NaN
        np.testing.assert_array_equal(want["min"][present][some].astype(np.float64), np.asarray(lo)[some])                    # equal as values
        np.testing.assert_array_equal(want["max"][present][some].astype(np.float64), np.asarray(hi)[some])
        assert np.isnan(want["min"][present][~some]).all() and np.isnan(want["max"][present][~some]).all()
    else:
        np.testing.assert_array_equal(want["min"][present], np.asarray(ndimage.minimum(image, c, present)).astype(np.int32))
        np.testing.assert_array_equal(want["max"][present], np.asarray(ndimage.maximum(image, c, present)).astype(np.int32))
    # sum: within (n - 1) 2^-53 sum |x| of SciPy's own naive float64 sum, on the labels whose voxels are all finite
    fin = np.where(np.isfinite(x), x, 0.0)
    got = np.asarray(ndimage.sum_labels(fin, c, present))
    mass = np.asarray(ndimage.sum_labels(np.abs(fin), c, present))
    clean = want["nonfinite"][present].sum(1) == 0
    n = want["area"][present].astype(np.float64)
    bound = (n - 1) * 2.0 ** -53 * mass * (1 + 2.0 ** -40)                                   # the mass itself is a rounded sum
    assert (np.abs(got - want["sum"][present])[clean] <= bound[clean]).all(), name
    np.testing.assert_array_equal(want["area"][present], np.asarray(ndimage.sum_labels(np.ones_like(x), c, present)).astype(np.int32))


# ---- the library's host entry points against the twin --------------------------------------------------------------------------------------------------

def _pieces_host(bits):
    from biapy_amd import _lib as L

    limb, lo, hi = C.c_int(), C.c_int64(), C.c_int64()
    assert L.lib.bpx_intensity_pieces_host(int(bits), C.byref(limb), C.byref(lo), C.byref(hi)) == 0
    return limb.value, lo.value, hi.value


def _round_host(limbs):
    from biapy_amd import _lib as L

    out = C.c_double()
    assert L.lib.bpx_intensity_round_host((C.c_int64 * len(limbs))(*[int(v) for v in limbs]), len(limbs), C.byref(out)) == 0
    return out.value


def test_the_pieces_on_every_exponent_field_and_the_limb_boundary_mantissas():
    top = 0
    for E in range(255):
        for f in (0, 1, 2, 0x7FFFFF, 0x7FFFFE, 0x400000, 0x400001, 0x555555, 0x2AAAAA, 0x000FFF, 0x7FF000):
            for neg in (0, 1):
                bits = neg << 31 | E << 23 | f
                limb, lo, hi = _pieces_host(bits)
                wl, wlo, whi, cls = (int(v[0]) for v in R.pieces(np.array([bits], np.uint32)))
                assert (limb, lo, hi, cls) == (wl, wlo, whi, 0), hex(bits)
                m, q = (f, 0) if E == 0 else (f | 0x800000, E - 1)
                assert limb == q >> 5 and abs(lo) < 2 ** 32 and abs(hi) < 2 ** 23
                value = Fraction(float(np.array([bits], np.uint32).view(np.float32)[0]))
                assert (Fraction(lo) * 2 ** (32 * limb) + Fraction(hi) * 2 ** (32 * limb + 32)) / 2 ** 149 == value == Fraction((-1) ** neg * m * 2 ** q, 2 ** 149)
                top = max(top, limb + (hi != 0))
    assert top == 8                                                                          # nine limbs, and the ninth is reached
    for bits in (0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF):     # the infinities and NaN have no pieces
        assert _pieces_host(bits) == (-1, 0, 0)


def test_the_rounding_on_random_limb_vectors():
    rnd = random.Random(7)
    B = 2 ** 63 - 2 ** 32 - 1
    for k in range(100000):
        v = [0] * 9
        for _ in range(rnd.randint(1, 9)):
            kind = rnd.randint(0, 5)
            v[rnd.randint(0, 8)] = (rnd.randint(-B, B), rnd.randint(-2 ** 32, 2 ** 32), rnd.randint(-3, 3), 1 << rnd.randint(0, 62), -(1 << rnd.randint(0, 62)),
                                    rnd.choice((B, -B)))[kind]
        got = _round_host(v)
        assert R.same_bits(np.float64(got), np.float64(R.round_limbs(v))), (v, got, R.round_limbs(v))
    # ties: 2^53 + 1 and 2^53 + 3 units lie halfway; to even
    for units, want in ((2 ** 53 + 1, 2 ** 53), (2 ** 53 + 3, 2 ** 53 + 4), (2 ** 53 + 2, 2 ** 53 + 2), (2 ** 54 - 1, 2 ** 54), (-(2 ** 53 + 1), -2 ** 53),
                        (-(2 ** 53 + 3), -(2 ** 53 + 4))):
        v = [units & 0xFFFFFFFF, units >> 32] + [0] * 7
        assert _round_host(v) == want * 2.0 ** -149 == R.round_limbs(v), units
        assert _round_host([0] * 7 + [units & 0xFFFFFFFF, units >> 32]) == float(want) * 2.0 ** (224 - 149)
    assert _round_host([2 ** 40 + 123]) == float(2 ** 40 + 123) and _round_host([-5]) == -5.0 and _round_host([2 ** 53 + 1]) == float(2 ** 53)
    assert R.same_bits(np.float64(_round_host([0] * 9)), np.float64(0.0)) and R.same_bits(np.float64(_round_host([0])), np.float64(0.0))
    assert R.same_bits(np.float64(_round_host([2 ** 32, -1] + [0] * 7)), np.float64(0.0))     # limbs that cancel: +0.0


# ---- hand-made cases -------------------------------------------------------------------------------------------------------------------------------------

def _one_label(values, dtype=np.float32):
    x = np.array(values, dtype=dtype).reshape(1, -1)
    return R.intensity_props_ref(np.ones(x.shape, np.int32), x, 1)


def test_hand_made_sums():
    r = _one_label([1e30, 1.0, -1e30])
    assert r["sum"][1] == 1.0 and r["mean"][1] == 1.0 / 3.0 and r["min"][1] == np.float32(-1e30) and r["max"][1] == np.float32(1e30)
    assert float(np.float32(1e30) + np.float32(1.0) + np.float32(-1e30)) == 0.0               # what a float sum makes of it
    for x in (1.5, 3.4e38, 1e-45, 0.1):
        r = _one_label([x, -x])
        assert R.same_bits(r["sum"][1:], np.array([0.0])) and not r["sum_limbs"].any() and R.same_bits(r["mean"][1:], np.array([0.0]))
    tiny = np.array([1], np.uint32).view(np.float32)[0]                                       # the smallest denormal: one unit of limb 0
    r = _one_label([tiny])
    assert r["sum_limbs"][1].tolist() == [1] + [0] * 8 and r["sum"][1] == 2.0 ** -149 == float(tiny) and r["min"][1] == r["max"][1] == tiny
    assert _round_host([1] + [0] * 8) == 2.0 ** -149
    r = _one_label([-0.0, 0.0, -0.0])
    assert R.same_bits(r["sum"][1:], np.array([0.0])) and R.same_bits(r["min"][1:], np.array([-0.0], np.float32)) and R.same_bits(r["max"][1:], np.array([0.0], np.float32))
    r = _one_label([R.FLT_MAX] * 4)
    assert r["sum"][1] == 4.0 * float(R.FLT_MAX) and r["sum_limbs"][1, 7] == 4 * 0xE0000000 and r["sum_limbs"][1, 8] == 4 * 0x1FFFFF
    r = _one_label([7, 0, 255], np.uint8)
    assert r["sum_limbs"].tolist() == [[0], [262]] and r["sum"][1] == 262.0 and r["min"][1] == 0 and r["max"][1] == 255 and r["min"].dtype == np.int32


def test_the_non_finite_table():
    want = R.ref("the non-finite table")
    inf = np.inf
    assert want["nonfinite"].tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 1, 1], [1, 1, 0], [300, 0, 0], [0, 300, 0], [0, 0, 0]]
    s = want["sum"]
    assert np.isnan(s[[1, 4, 5, 6]]).all() and s[2] == inf and s[3] == -inf and s[7] == inf and np.isfinite(s[8]) and s[0] == 0
    assert np.isnan(want["mean"][[0, 1, 4, 5, 6]]).all() and want["mean"][2] == inf and want["mean"][3] == -inf
    assert want["max"][2] == inf and want["min"][3] == -inf and want["min"][4] == -inf and want["max"][4] == inf and want["max"][5] == inf
    assert np.isfinite(want["min"][[1, 2, 5, 8]]).all() and np.isfinite(want["max"][[1, 3, 8]]).all()        # NaN is left out, the infinities take part
    assert np.isnan(want["min"][6]) and np.isnan(want["max"][6]) and want["min"][7] == want["max"][7] == inf
    labels, image, n_max = R.cases()["the non-finite table"]
    finite = np.where(np.isfinite(image), image, 0).astype(np.float64)
    for l in range(1, 9):                                                                    # the limbs hold the finite voxels whatever else the label holds
        if l not in (6, 7):
            assert R.round_limbs(want["sum_limbs"][l]) == math.fsum(finite[labels == l].tolist()) != 0
    assert not want["sum_limbs"][[6, 7]].any()
    assert (R.sum_rule(1.0, 0, 0, 0), R.sum_rule(1.0, 0, 2, 0), R.sum_rule(1.0, 0, 0, 1)) == (1.0, inf, -inf)
    assert math.isnan(R.sum_rule(1.0, 1, 0, 0)) and math.isnan(R.sum_rule(1.0, 0, 1, 1)) and math.isnan(R.sum_rule(1.0, 1, 1, 0))


# ---- seeded defects the comparisons must catch -------------------------------------------------------------------------------------------------------------

def test_the_comparisons_catch_seeded_defects():
    def fsum_of(labels, image, n_max):
        return {l: math.fsum(_f64(v)[np.isfinite(v)].tolist()) for l, v in _values_by_label(labels, image, n_max).items()}

    # a dropped high piece: boundary mantissas reach past bit 32 of their window
    name = "boundaries (16, 32, 64) L40"
    labels, image, n_max = R.cases()[name]
    good, bad = R.ref(name), R.intensity_props_ref(labels, image, n_max, drop_high=True)
    exact = fsum_of(labels, image, n_max)
    assert all(good["sum"][l] == exact[l] for l in exact) and any(bad["sum"][l] != exact[l] for l in exact)
    assert not R.same_bits(good["sum_limbs"], bad["sum_limbs"])
    # truncation in place of round to even: uniform values, sums of a few hundred 24-bit numbers need more than 53 bits only with spread exponents
    name = "exponents (16, 32, 64) L40"
    labels, image, n_max = R.cases()[name]
    good, bad = R.ref(name), R.intensity_props_ref(labels, image, n_max, truncate=True)
    exact = fsum_of(labels, image, n_max)
    assert all(good["sum"][l] == exact[l] for l in exact) and any(bad["sum"][l] != exact[l] for l in exact)
    assert R.same_bits(good["sum_limbs"], bad["sum_limbs"]) and R.ulp_distance(good["sum"], bad["sum"]) == 1
    # NaN included in min: the key of a positive NaN lies above +inf, of a negative one below -inf
    from scipy import ndimage

    name = "nonfinite (16, 32, 64) L40"
    labels, image, n_max = R.cases()[name]
    good, bad = R.ref(name), R.intensity_props_ref(labels, image, n_max, nan_in_min=True)
    present = np.flatnonzero(good["area"])
    x = _f64(image)
    lo = np.asarray(ndimage.minimum(np.where(np.isnan(x), np.inf, x), R.clean(labels, n_max), present))
    hi = np.asarray(ndimage.maximum(np.where(np.isnan(x), -np.inf, x), R.clean(labels, n_max), present))
    assert np.array_equal(good["min"][present], lo) and np.array_equal(good["max"][present], hi)
    assert not (np.array_equal(bad["min"][present], lo) and np.array_equal(bad["max"][present], hi))


# ---- the compiled kernels ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc to cross-compile the kernels to ISA")
def test_no_kernel_uses_scratch(tmp_path):
    out = str(tmp_path / "intensityprops.s")
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-result", "-S", "--cuda-device-only",   # the Makefile's flags
           os.path.join(ROOT, "biapy_amd", "csrc", "intensityprops.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)} failed:\n{r.stderr[-3000:]}"
    kernels = re.findall(r"\.name:\s+(_Z\w*ip_\w*kernel\w*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", open(out).read())
    names = sorted(re.search(r"ip_\w+?_kernel", k).group(0) for k, _ in kernels)
    assert names == ["ip_accumulate_kernel"] * 6 + ["ip_finish_kernel"] * 2 + ["ip_init_kernel"] * 2, kernels      # three dtypes x two forms; NL 9 and 1
    for name, private in kernels:
        assert int(private) == 0, f"{name} keeps {private} bytes of scratch per lane"

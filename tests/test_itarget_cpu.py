"""Instance-segmentation targets - what can be checked without a GPU: the entry points are declared, exported and bound; every host-side refusal
of the C entry points, the constructor, ``from_cfg``, the call and ``prepost.instance_targets`` names its cause, in the stated order, before
anything is launched; the NumPy twin the GPU tests hold the device against (tests/itarget_ref.py) agrees with an independent SciPy statement on
every input of the GPU tests, reproduces the hand-made cases, and its comparator catches three seeded defects; no kernel of itarget.hip keeps
scratch; and scripts/itarget_cpu_check.cpp replays itarget_core.h under ASan / UBSan as a stand-alone host program."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import itarget_ref as R
import morph_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
A = 1 << 30                                # any non-null, aligned "device" address: nothing is launched
NAMES = ["bpx_itarget_records_bytes", "bpx_itarget_ids", "bpx_itarget_stats", "bpx_itarget_pack"]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


@pytest.fixture(autouse=True)
def product():
    """The twin is checked as the statement of THIS product: its channel letters, in their order, are the ones ``biapy_amd.targets`` offers.  The
    tests of the twin alone (against SciPy, the hand-made cases, the seeded defects) guard the reference the GPU tests use; they say nothing
    about the kernels."""
    from biapy_amd import targets

    assert tuple(targets.CHANNELS) == R.CHANNELS and targets.ID_LIMIT == 1 << 24
    return targets


def test_entry_points_are_declared_exported_and_bound():
    import biapy_amd
    from biapy_amd import _lib as L
    from biapy_amd import prepost, targets

    header, source, core = _read("include", "biapy_amd.h"), _read("biapy_amd", "csrc", "itarget.hip"), _read("biapy_amd", "csrc", "itarget_core.h")
    assert re.findall(r'extern "C" \w+ (\w+)\(', source) == NAMES
    for n in NAMES:
        assert re.search(r"^int(64_t)? %s\(" % n, header, re.M), n
    assert set(NAMES) <= set(L.EXPORTS)
    vp, i, i64, f, pd = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.POINTER(C.c_double)
    assert L._SIGS["bpx_itarget_records_bytes"] == ([i, i], i64)
    assert L._SIGS["bpx_itarget_ids"] == ([vp, i, i64, i, vp, vp, vp], i)
    assert L._SIGS["bpx_itarget_stats"] == ([vp, vp, i, i, i, i, i, pd, i, vp, vp], i)
    assert L._SIGS["bpx_itarget_pack"] == ([vp, vp, vp, i, i, i, i, i, C.c_uint32, i, i, i, i, i, f, pd, vp, vp], i)
    make = _read("biapy_amd", "csrc", "Makefile")
    assert "itarget.hip" in make and re.search(r"^itarget\.o:.*itarget_core\.h.*label_walk\.h", make, re.M)
    # one text for device and host: the walk, the table and the channel values are the shared code; integer atomics only
    assert '#include "itarget_core.h"' in source and '#include "label_walk.h"' in source and "lw_walk_runs(" in source and "rp_local_slot(" in core
    for step in ("it_id_f32(", "it_emit(", "it_merge(", "it_emit_rc(", "it_finish_row(", "it_value(", "it_differs("):
        assert step in source + core and step in core, step
    assert set(re.findall(r"__hip_atomic_fetch_(\w+)\(", source)) == {"add", "min", "max"} and "atomicAdd" not in source and "float*" not in source.split("it_pack_kernel")[0].split("ItLds")[1]
    check = _read("scripts", "itarget_cpu_check.cpp")
    assert '#include "itarget_core.h"' in check and "int main()" in check and "-fsanitize=address,undefined" in check and "std::thread" in check
    assert biapy_amd.InstanceTargets is targets.InstanceTargets and callable(prepost.instance_targets)
    assert tuple(targets.CHANNELS) == R.CHANNELS
    for name, code in targets.CHANNELS.items():
        assert int(re.search(r"#define BPX_ITARGET_%s (\d)" % name.upper(), header).group(1)) == code
        assert int(re.search(r"\bIT_%s = (\d)" % name.upper(), core).group(1)) == code
    for name, flag in (("F_EXCLUDES_C", targets.FLAG_F_EXCLUDES_C), ("D_RAW", targets.FLAG_D_RAW), ("D_CLIP", targets.FLAG_D_CLIP)):
        assert int(re.search(r"#define BPX_ITARGET_%s (\d)" % name, header).group(1)) == flag == int(re.search(r"IT_FLAG_%s = (\d)" % name, core).group(1))
    assert L.lib.bpx_itarget_records_bytes(1, 0) == 64 and L.lib.bpx_itarget_records_bytes(3, 9) == 1800 and L.lib.bpx_itarget_records_bytes(2, 2 ** 24 - 1) == 60 * 2 ** 25
    it = targets.InstanceTargets(("F", "C", "D", "Dc", "H", "V", "Z"), n_max=5)
    assert it.codes == 0x7654321 and it.flags == 0 and it.last_faults is None and it.last_ids is None
    assert targets.InstanceTargets(n_max=0, d_norm="none", d_clip=2, f_excludes_contour=True).flags == 7 and targets.InstanceTargets(n_max=0).codes == 0x321


def test_host_side_argument_checks_of_the_entry_points():
    """The order stated in include/biapy_amd.h: null pointers, extents, the voxel count, B, n_max (and the record count), the channel count and
    codes, connectivity, the contour mode, the flags and d_clip, sampling, alignment, overlap - each call below is wrong in that one respect and
    in every later one listed after it."""
    from biapy_amd import _lib as L

    lib = L.lib

    def err():
        return lib.bpx_last_error()

    I_, D_, R_, T_ = A, A + (1 << 22), A + (2 << 22), A + (3 << 22)
    bad_s, good_s = (C.c_double * 3)(1.0, 0.0, 1.0), (C.c_double * 3)(2.0, 1.0, 1.0)

    def pack(ids=I_, d=D_, rec=R_, B=1, Z=8, Y=8, X=8, n_max=5, codes=0x321, ch=3, ndim=3, conn=1, mode=0, flags=0, clip=0.0, samp=None, t=T_):
        return lib.bpx_itarget_pack(ids, d, rec, B, Z, Y, X, n_max, codes, ch, ndim, conn, mode, flags, clip, samp, t, None)

    for kw in (dict(ids=None), dict(d=None), dict(rec=None), dict(t=None)):
        assert pack(Z=0, **kw) != 0 and b"null pointer" in err(), kw
    assert pack(Z=0, Y=2048, X=1 << 20, B=0) != 0 and b"extents must be at least 1" in err()
    assert pack(Z=2048, Y=1024, X=1024, B=0) != 0 and b"2^31 or more" in err()
    for B in (0, 65536):
        assert pack(B=B, n_max=-1) != 0 and b"samples" in err()
    for n_max in (-1, 1 << 24):
        assert pack(n_max=n_max, ch=0) != 0 and b"n_max must be in [0, 2^24)" in err()
    assert pack(B=256, n_max=(1 << 24) - 1, ch=0) != 0 and b"records" in err()
    for ch in (0, 9):
        assert pack(ch=ch, codes=0) != 0 and b"channels (got" in err()
    assert pack(ndim=4, codes=0) != 0 and b"ndim must be 3, or 2 with Z = 1" in err()
    assert pack(ndim=2, codes=0) != 0 and b"ndim must be 3, or 2 with Z = 1" in err()
    for codes in (0x021, 0x821, 0xF21):
        assert pack(codes=codes, conn=0) != 0 and b"unknown channel code" in err(), codes
    assert pack(Z=1, ndim=2, codes=0x721, conn=0) != 0 and b"needs 3-D samples" in err()
    assert pack(codes=0x1321, conn=0) != 0 and b"channel codes past" in err()
    for conn in (0, 4):
        assert pack(conn=conn, mode=2) != 0 and b"connectivity must be in 1..3" in err()
    assert pack(Z=1, ndim=2, conn=3, mode=2) != 0 and b"connectivity must be in 1..2" in err()
    for mode in (-1, 2):
        assert pack(mode=mode, flags=8) != 0 and b"unknown contour mode" in err()
    for flags in (-1, 8, 4, 5):
        assert pack(flags=flags, samp=bad_s) != 0 and b"bad flags" in err()
    for clip in (-1.0, float("nan")):
        assert pack(flags=6, clip=clip, samp=bad_s) != 0 and b"d_clip must be a number >= 0" in err()
    for s in ((1.0, 0.0, 1.0), (1.0, 1.0, float("inf")), (float("nan"), 1.0, 1.0), (-2.0, 1.0, 1.0)):
        assert pack(samp=(C.c_double * 3)(*s), ids=A + 2) != 0 and b"sampling must be positive and finite" in err(), s
    for kw in (dict(ids=I_ + 2), dict(d=D_ + 1), dict(t=T_ + 2), dict(rec=R_ + 4)):
        assert pack(samp=good_s, t=kw.pop("t", I_), **kw) != 0 and b"aligned" in err(), kw
    n = 4 * 512
    for kw in (dict(t=I_), dict(t=I_ + n - 4), dict(t=D_ - 3 * n + 4), dict(t=R_ - 3 * n + 8), dict(t=R_ + 6 * 60 - 4)):
        assert pack(**kw) != 0 and b"the target overlaps an input" in err(), kw
    # the stats
    def stats(ids=I_, d=D_, B=1, Z=8, Y=8, X=8, n_max=5, samp=None, rc=1, rec=R_):
        return lib.bpx_itarget_stats(ids, d, B, Z, Y, X, n_max, samp, rc, rec, None)

    for kw in (dict(ids=None), dict(d=None), dict(rec=None)):
        assert stats(Z=0, **kw) != 0 and b"null pointer" in err(), kw
    assert stats(Z=0, B=0) != 0 and b"extents" in err()
    assert stats(Z=2048, Y=1024, X=1024, B=0) != 0 and b"2^31 or more" in err()
    assert stats(B=0, n_max=-1) != 0 and b"samples" in err()
    assert stats(n_max=1 << 24, samp=bad_s) != 0 and b"n_max" in err()
    assert stats(samp=bad_s, rec=R_ + 4) != 0 and b"sampling must be positive and finite" in err()
    for kw in (dict(ids=I_ + 1), dict(d=D_ + 2), dict(rec=R_ + 4)):
        assert stats(**kw) != 0 and b"aligned" in err(), kw
    # the ids
    def ids(t=D_, dt=L.F32, n=512, n_max=5, out=I_, faults=R_):
        return lib.bpx_itarget_ids(t, dt, n, n_max, out, faults, None)

    for kw in (dict(t=None), dict(out=None), dict(faults=None)):
        assert ids(n=0, **kw) != 0 and b"null pointer" in err(), kw
    assert ids(n=0, n_max=-1) != 0 and b"value count" in err()
    for n_max in (-1, 1 << 24):
        assert ids(n_max=n_max, dt=L.BF16) != 0 and b"n_max" in err()
    for dt in (L.BF16, L.F16, L.U16, 7):
        assert ids(dt=dt, t=D_ + 1) != 0 and b"float32, uint8 or int32" in err()
    for kw in (dict(t=D_ + 1), dict(t=D_ + 2, dt=L.I32), dict(out=I_ + 2), dict(faults=R_ + 1)):
        assert ids(**kw) != 0 and b"aligned" in err(), kw
    assert ids(t=I_ + 4 * 511) != 0 and b"overlap" in err()
    assert ids(t=I_ + 511, dt=L.U8) != 0 and b"overlap" in err()                   # a uint8 source may sit at any address, but not in the ids
    assert lib.bpx_itarget_records_bytes(0, 5) == -1 and b"samples" in err()
    assert lib.bpx_itarget_records_bytes(1, 1 << 24) == -1 and b"n_max" in err()


def test_constructor_from_cfg_and_call_refusals():
    from biapy_amd import prepost
    from biapy_amd.targets import InstanceTargets

    for letter in ("B", "P", "T", "Db", "Dn", "R", "A", "E_offset", "E_sigma", "E_seediness", "We", "M"):
        with pytest.raises(NotImplementedError, match=f"channel '{letter}' is not implemented"):
            InstanceTargets(("F", letter), n_max=3)
    with pytest.raises(ValueError, match="unknown channel 'Q'"):
        InstanceTargets(("Q",), n_max=3)
    with pytest.raises(ValueError, match="1 to 8 channels, got 9"):
        InstanceTargets(("F",) * 9, n_max=3)
    with pytest.raises(ValueError, match="1 to 8 channels, got 0"):
        InstanceTargets((), n_max=3)
    with pytest.raises(ValueError, match="sequence of channel letters"):
        InstanceTargets("FCD", n_max=3)
    for mode in ("outer", "subpixel"):
        with pytest.raises(NotImplementedError, match=f"contour_mode '{mode}' is not implemented"):
            InstanceTargets(n_max=3, contour_mode=mode)
    with pytest.raises(ValueError, match="contour_mode must be one of thick, inner"):
        InstanceTargets(n_max=3, contour_mode="thin")
    for n_max in (-1, 2 ** 24, "many"):
        with pytest.raises(ValueError, match="n_max must"):
            InstanceTargets(n_max=n_max)
    with pytest.raises(TypeError):
        InstanceTargets()                                                          # n_max has no default
    for conn in (0, 4):
        with pytest.raises(ValueError, match="contour_connectivity must lie in 1..3"):
            InstanceTargets(n_max=3, contour_connectivity=conn)
    with pytest.raises(ValueError, match="d_norm must be 'instance' or 'none'"):
        InstanceTargets(n_max=3, d_norm="global")
    with pytest.raises(ValueError, match="d_clip applies to d_norm='none' only"):
        InstanceTargets(n_max=3, d_clip=2.0)
    for clip in (-1.0, float("nan"), "x"):
        with pytest.raises(ValueError, match="d_clip must be a number"):
            InstanceTargets(n_max=3, d_norm="none", d_clip=clip)
    for s in ((1.0,), (1.0, 0.0, 1.0), (1.0, float("inf")), "ab", 3.0):
        with pytest.raises(ValueError, match="sampling must be 2 or 3 positive finite numbers"):
            InstanceTargets(n_max=3, sampling=s)
    with pytest.raises(ValueError, match="augment must be a biapy_amd.augment.DeviceAugmenter"):
        InstanceTargets(n_max=3, augment=lambda x, t: (x, t))
    # the call: dtype, rank, layout, the id channel, the options against the rank, the device - in this order
    it = InstanceTargets(("F", "C", "D", "Z"), n_max=3, contour_connectivity=3, sampling=(1.0, 1.0))
    with pytest.raises(ValueError, match="t must be a tensor"):
        it(None, np.zeros((1, 4, 4, 4, 1), np.float32))
    for dt in (torch.float64, torch.int64, torch.float16, torch.bool):
        with pytest.raises(ValueError, match="t must be float32, uint8 or int32"):
            it(None, torch.zeros(1, 4, 4, 4, 1, dtype=dt))
    for shape in ((4, 4), (4, 4, 4), (1, 2, 4, 4, 4, 1)):
        with pytest.raises(ValueError, match="t must have 4 or 5 dimensions"):
            it(None, torch.zeros(shape))
    for shape in ((4, 4), (1, 2, 4, 4, 4)):
        with pytest.raises(ValueError, match=r"int32 ids must be \(B,\[Z,\]Y,X\)"):
            it(None, torch.zeros(shape, dtype=torch.int32))
    with pytest.raises(ValueError, match="int32 ids must be contiguous"):
        it(None, torch.zeros(2, 4, 4, 6, dtype=torch.int32)[..., ::2])
    with pytest.raises(ValueError, match="permuted view"):
        it(None, torch.zeros(2, 4, 4, 6, 1)[..., ::2, :])
    with pytest.raises(ValueError, match="one id channel, got 2"):
        it(None, torch.zeros(2, 4, 4, 4, 2))
    with pytest.raises(ValueError, match="one id channel, got 3"):
        it(None, torch.zeros(2, 4, 4, 4, 3).permute(0, 4, 1, 2, 3))
    with pytest.raises(ValueError, match="empty batch"):
        it(None, torch.zeros(0, 4, 4, 4, 1))
    with pytest.raises(ValueError, match="channel 'Z' needs 3-D samples"):
        it(None, torch.zeros(2, 4, 4, 1))
    with pytest.raises(ValueError, match="channel 'Z' needs 3-D samples"):
        it(None, torch.zeros(2, 4, 4, dtype=torch.int32))
    it2 = InstanceTargets(("F", "C"), n_max=3, contour_connectivity=3, sampling=(1.0, 1.0))
    with pytest.raises(ValueError, match=r"contour_connectivity must lie in 1..2 for 2-D samples"):
        it2(None, torch.zeros(2, 4, 4, 1))
    with pytest.raises(ValueError, match="sampling has 2 entries for 3-D samples"):
        it2(None, torch.zeros(2, 4, 4, 4, 1))
    ok = InstanceTargets(n_max=3)
    for t in (torch.zeros(2, 4, 4, 4, 1), torch.zeros(2, 4, 4, 1, dtype=torch.uint8), torch.zeros(2, 4, 4, 4, dtype=torch.int32)):
        with pytest.raises(ValueError, match="there is no CPU path"):
            ok(None, t)
    # prepost.instance_targets
    lab = torch.zeros(4, 4, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="2-D .* or 3-D"):
        prepost.instance_targets(torch.zeros(2, 2, 2, 2, dtype=torch.int32), num=3)
    with pytest.raises(NotImplementedError, match="int32 labels"):
        prepost.instance_targets(lab.float(), num=3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        prepost.instance_targets(lab, num=3)
    with pytest.raises(ValueError, match="num must not be negative"):
        prepost.instance_targets(lab, num=-1)
    with pytest.raises(ValueError, match="takes num= and no augmenter"):
        prepost.instance_targets(lab, num=3, augment=None)
    with pytest.raises(NotImplementedError, match="channel 'We' is not implemented"):
        prepost.instance_targets(lab, ("F", "We"), num=3)
    # from_cfg
    ns = types.SimpleNamespace
    cfg = ns(PROBLEM=ns(TYPE="INSTANCE_SEG", INSTANCE_SEG=ns(DATA_CHANNELS=["F", "C", "Dc"])))
    got = InstanceTargets.from_cfg(cfg, n_max=9)
    assert got.channels == ("F", "C", "Dc") and got.n_max == 9 and got.augment is None and got.codes == 0x421
    assert InstanceTargets.from_cfg(ns(PROBLEM=ns(TYPE="SEMANTIC_SEG")), n_max=9) is None
    assert InstanceTargets.from_cfg(ns(PROBLEM=ns(TYPE="INSTANCE_SEG", INSTANCE_SEG=ns())), n_max=9).channels == ("F", "C", "D")
    assert InstanceTargets.from_cfg(ns(PROBLEM=ns(TYPE="instance_seg", INSTANCE_SEG=ns(DATA_CHANNELS="FCDcHVZ"))), n_max=2).channels == ("F", "C", "Dc", "H", "V", "Z")
    for chans, letter in (("BC", "B"), (["F", "Db"], "Db"), ("FCDn", "Dn"), (["A"], "A")):
        with pytest.raises(NotImplementedError, match=f"channel '{letter}' is not implemented"):
            InstanceTargets.from_cfg(ns(PROBLEM=ns(TYPE="INSTANCE_SEG", INSTANCE_SEG=ns(DATA_CHANNELS=chans))), n_max=9)
    with pytest.raises(ValueError, match="unknown channel 'X' in PROBLEM.INSTANCE_SEG.DATA_CHANNELS"):
        InstanceTargets.from_cfg(ns(PROBLEM=ns(TYPE="INSTANCE_SEG", INSTANCE_SEG=ns(DATA_CHANNELS=["F", "X"]))), n_max=9)
    for doc in (InstanceTargets.from_cfg.__doc__, __import__("biapy_amd.targets").targets.__doc__):
        assert "unverified" in doc or "could not be verified" in doc
    assert "ONE instance" in __import__("biapy_amd.targets").targets.__doc__ and "SENTINEL STAYS" in __import__("biapy_amd.targets").targets.__doc__


# ---- the twin ------------------------------------------------------------------------------------------------------------------------------------------
ULPS = {"Dc": 1, "H": 1, "V": 1, "Z": 1}


@pytest.mark.parametrize("name", list(R.cases()))
def test_twin_against_the_scipy_statement(name):
    """Per-label ``distance_transform_edt``, ``center_of_mass``, ``find_objects`` and ``grey_dilation != grey_erosion``: D, C and F bit for bit, Dc, H,
    V and Z within 1 float32 ulp; H, V, Z in [-1, 1], D in (0, 1] on the instances, and the thick contour is the any-neighbour-differs rule."""
    t, n_max = R.cases()[name]
    ch = R.ALL7 if t.ndim == 4 else R.ALL2D
    ids, _ = R.sanitise(t, n_max)
    for mode, conn in (("thick", 1), ("inner", t.ndim - 1)):
        want, _ = R.batch_targets(t, ch, n_max, contour_mode=mode, contour_connectivity=conn)
        sp = np.stack([R.scipy_targets(ids[b], ch, n_max, mode, conn) for b in range(len(ids))])
        bad = R.mismatch(want, sp, ch, ulps=ULPS)
        assert bad is None, bad
        for b in range(len(ids)):
            assert np.array_equal(want[b, 1], MR.find_boundaries_ref(ids[b], conn, mode).astype(np.float32))
    fg = ids > 0
    k = {c: i for i, c in enumerate(ch)}
    assert np.array_equal(want[:, k["F"]] > 0, fg)
    for c in ("H", "V", "Z"):
        if c in k:
            assert np.abs(want[:, k[c]]).max(initial=0) <= 1 and not want[:, k[c]][~fg].any()
    d = want[:, k["D"]]
    assert (d[fg] > 0).all() and (d[fg] <= 1).all() and not d[~fg].any()
    for b in range(len(ids)):                                                    # every instance reaches 1 in D, and its extremes in H
        for l in np.unique(ids[b][ids[b] > 0]):
            assert d[b][ids[b] == l].max() == 1
    dc = want[:, k["Dc"]]
    assert (dc[fg] >= 0).all() and (dc[fg] <= 1).all()


def test_the_pieces_input_holds_ids_that_are_not_connected():
    """The GPU tests' input for "one id in two pieces": at full connectivity id 1 has 2 components in sample 0 and 3 in sample 1, id 2 has 2 in
    sample 1 and id 3 has 2 in sample 2 - and the twin gives such an id one centroid, one box and one ``dmax``."""
    from scipy import ndimage

    t, n_max = R.cases()[R.PIECES]
    full = np.ones((3, 3, 3), bool)
    count = {(b, l): ndimage.label(t[b] == l, structure=full)[1] for b in range(3) for l in (1, 2, 3)}
    assert count == {(0, 1): 2, (0, 2): 1, (0, 3): 0, (1, 1): 3, (1, 2): 2, (1, 3): 0, (2, 1): 1, (2, 2): 1, (2, 3): 2}
    ids = R.sanitise(t, n_max)[0]
    got = R.sample_targets(ids[2], ("H", "D", "Dc"), n_max)
    face = ids[2] == 3
    assert got[0][face].min() == -1 and got[0][face].max() == 1 and set(np.unique(got[0][face])) == {-1.0, np.float32(-18.5 / 19.5), np.float32(-17.5 / 19.5),
                                                                                                     np.float32(17.5 / 19.5), np.float32(18.5 / 19.5), 1.0}
    assert (got[1][face][got[1][face] == 1].size == 2 * 6 * 10) and got[2][face].min() == 0          # both slabs reach dmax = 3; the far corners are rcmax
    only = [name for name, (v, n) in R.cases().items() for b in range(len(v)) for l in np.unique(R.sanitise(v, n)[0][b])
            if l > 0 and ndimage.label(R.sanitise(v, n)[0][b] == l, structure=np.ones((3,) * (v.ndim - 1), bool))[1] > 1]
    assert R.PIECES in only and "8^3, every voxel its own id" not in only


def test_sanitising_counts_what_is_no_id():
    t = np.array([[0.0, -0.0, 1.0, 5.0, 6.0, -1.0, 2.5, np.nan, np.inf, -np.inf, 1e30, 4.0]], np.float32)
    ids, faults = R.sanitise(t, 5)
    assert ids.tolist() == [[0, 0, 1, 5, 0, 0, 0, 0, 0, 0, 0, 4]] and ids.dtype == np.int32 and faults == 7
    assert R.sanitise(np.array([0, 3, 200, 255], np.uint8), 200)[1] == 1 and R.sanitise(np.array([-3, 0, 7, 8], np.int32), 7) == (pytest.approx([0, 0, 7, 0]), 2)
    want = {"blobs 2 x 13x22x37 int32, ids above n_max": None, "values that are no id": 8, "n_max = 0 under ids": None, "all background": 0}
    for name, count in want.items():
        t, n_max = R.cases()[name]
        faults = R.sanitise(t, n_max)[1]
        assert faults == (int(((t > n_max) | (t < 0)).sum()) if count is None else count), name


def test_hand_made_cases():
    one = np.zeros((3, 3, 3), np.int32)
    one[1, 1, 1] = 4
    got = R.sample_targets(one, R.ALL7, 4)
    assert got[:, 1, 1, 1].tolist() == [1, 1, 1, 1, 0, 0, 0]                    # F, C, D = 1, Dc = 1, the offsets 0
    assert got[1].sum() == 7 and got[[0, 2, 3, 4, 5, 6]].sum() == 3            # thick: the six face neighbours too; nothing else anywhere
    assert R.sample_targets(one, ("C",), 4, contour_mode="inner").sum() == 1
    assert R.sample_targets(one, ("C",), 4, contour_connectivity=3).sum() == 27
    full = np.full((2, 3, 4), 2, np.int32)
    got = R.sample_targets(full, R.ALL7, 2)
    assert (got[0] == 1).all() and not got[1].any() and (got[2] == 1).all()    # the sentinel: D = 1 everywhere, no contour
    assert np.isinf(R.sample_targets(full, ("D",), 2, d_norm="none")).all() and (R.sample_targets(full, ("D",), 2, d_norm="none", d_clip=3.0) == 3).all()
    assert got[4, 0, 0].tolist() == [-1, np.float32(-1 / 3), np.float32(1 / 3), 1] and got[5, 0, :, 0].tolist() == [-1, 0, 1] and got[6, :, 0, 0].tolist() == [-1, 1]
    rod = np.full((1, 1, 5), 1, np.int32)
    got = R.sample_targets(rod, R.ALL7, 1)
    assert got[4, 0, 0].tolist() == [-1, -0.5, 0, 0.5, 1] and not got[5].any() and not got[6].any()
    assert got[3, 0, 0].tolist() == [0, 0.5, 1, 0.5, 0]                         # Dc = 1 - |x - 2| / 2
    two = R.cases()["two touching instances"][0][0].astype(np.int32)
    got = R.sample_targets(two, ("F", "C", "D"), 2, f_excludes_contour=True)
    assert got[1][:, 2:7, 5:7].all() and not got[0][:, 2:7, 5:7].any() and got[0][:, 3:6, 2:5].all()      # the shared face is contour, not foreground
    pieces = np.zeros((1, 3, 9), np.int32)
    pieces[0, :, :2] = pieces[0, :, 7:] = 1                                      # one id in two pieces: one centroid between them, one box
    got = R.sample_targets(pieces, ("H", "Dc"), 1)
    assert got[0, 0, 1].tolist() == [-1, -0.75, 0, 0, 0, 0, 0, 0.75, 1] and got[1, 0, 1, 0] == got[1, 0, 1, 8] and got[1, 0, 0, 0] == 0


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_the_comparator_catches_seeded_defects(defect):
    t, n_max = R.cases()[next(iter(R.cases()))]
    ch = R.ALL7
    want, _ = R.batch_targets(t, ch, n_max)
    assert R.mismatch(want.copy(), want, ch) is None and R.mismatch(want.copy(), want, ch, ulps=ULPS) is None
    broken, _ = R.batch_targets(t, ch, n_max, defect=defect)
    found = R.mismatch(broken, want, ch, ulps=ULPS)
    hit = {"box_exclusive": "channel H", "dmax_other_sample": "channel D", "contour_ignores_background": "channel C"}[defect]
    assert found is not None and found.startswith(hit), found
    others = [c for c in ch if not hit.endswith(" " + c) and not (defect == "box_exclusive" and c in ("V", "Z"))]
    k = [ch.index(c) for c in others]
    assert R.mismatch(np.ascontiguousarray(broken[:, k]), np.ascontiguousarray(want[:, k]), others) is None      # and nothing else moved
    one_ulp = want.copy()
    one_ulp[0, 4].reshape(-1).view(np.uint32)[np.flatnonzero(want[0, 4])[0]] += 1
    assert R.mismatch(one_ulp, want, ch) is not None and R.mismatch(one_ulp, want, ch, ulps=ULPS) is None
    one_ulp[0, 2].reshape(-1).view(np.uint32)[np.flatnonzero(want[0, 2])[0]] += 1
    assert R.mismatch(one_ulp, want, ch, ulps=ULPS).startswith("channel D")


# ---- the compiled code -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc to cross-compile the kernels to ISA")
def test_no_kernel_of_itarget_keeps_scratch(tmp_path):
    out = str(tmp_path / "itarget.s")
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-result", "-S", "--cuda-device-only",   # the Makefile's flags
           os.path.join(ROOT, "biapy_amd", "csrc", "itarget.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)} failed:\n{r.stderr[-3000:]}"
    text = open(out).read()
    kernels = re.findall(r"\.name:\s+(_Z\w*it_\w*kernel\w*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(kernels) == 8, kernels                                          # ids x 3 dtypes, init, finish, accumulate x 2, pack
    for name, private in kernels:
        assert int(private) == 0, f"{name} keeps {private} bytes of scratch per lane"
    sizes = {n: int(v) for v, n in re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(_Z\w*it_\w*kernel\w*)", text)}
    assert all(v == 0 for n, v in sizes.items() if "pack" in n) and max(sizes.values()) <= 16 * 1024
    assert not re.search(r"_atomic_f?(add|min|max)_f(32|64)", text)             # integer atomics only


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host compiler")
def test_host_replay_of_the_core_under_sanitizers(tmp_path):
    """scripts/itarget_cpu_check.cpp as a stand-alone program of its own under ASan / UBSan, on the host only: nothing loaded into Python is checked this way."""
    exe = str(tmp_path / "itarget_cpu_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-pthread", "-I", os.path.join(ROOT, "biapy_amd", "csrc"), "-I", os.path.join(ROOT, "scripts"), os.path.join(ROOT, "scripts", "itarget_cpu_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)} failed:\n{r.stderr[-3000:]}"
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "every case agrees with the per-voxel loops" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]

"""Label stitching - what can be checked without a GPU: the entry points are declared, exported and bound; every host-side refusal names its
cause, in the stated order, before anything is launched; ``prepost.LabelStitcher`` / ``label_blocks`` refuse in their order, CPU tensors
included; the twin the GPU tests hold the device against (tests/stitch_ref.py) equals ``scipy.ndimage.label`` of the whole mask bit for bit on
EVERY input of those tests (rule "touch") and a position-by-position count on tiny volumes (rule "contact"); hand-made contact cases; the
closed form of the rods-and-slabs mask; no kernel of stitch.hip uses scratch."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import stitch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NAMES = ("bpx_stitch_begin", "bpx_stitch_first", "bpx_stitch_shell", "bpx_stitch_contact_workspace", "bpx_stitch_contact", "bpx_stitch_resolve",
         "bpx_stitch_apply")
A = 4096                                   # any non-null, aligned "device" address: nothing is launched


def test_entry_points_are_declared_exported_and_bound():
    from biapy_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    source = open(os.path.join(ROOT, "biapy_amd", "csrc", "stitch.hip")).read()
    assert set(re.findall(r'extern "C" \w+ (\w+)\(', source)) == set(NAMES)
    for name in NAMES:
        assert re.search(r"^(int|int64_t) %s\(" % name, header, re.M), name
        assert name in L.EXPORTS and getattr(L.lib._raw if hasattr(L.lib, "_raw") else L.lib, name) is not None, name
    vp, i, i64 = L.C.c_void_p, L.C.c_int, L.C.c_int64
    assert L._SIGS["bpx_stitch_begin"] == ([vp, i, i, vp, vp, vp, vp, vp, vp], i)
    assert L._SIGS["bpx_stitch_first"] == ([vp] + [i] * 8 + [vp, vp, i, vp, vp], i)
    assert L._SIGS["bpx_stitch_shell"] == ([vp] + [i] * 7 + [vp, vp, i, vp, vp], i)
    assert L._SIGS["bpx_stitch_contact_workspace"] == ([i] * 7 + [i64], i64)
    assert L._SIGS["bpx_stitch_contact"] == ([vp] + [i] * 6 + [vp, vp, i, i, i, i64, vp, vp, vp, i64, vp], i)
    assert L._SIGS["bpx_stitch_resolve"] == ([vp, vp, vp, vp, i, vp, vp], i)
    assert L._SIGS["bpx_stitch_apply"] == ([vp, i64, vp, vp, i, vp, vp, vp], i)
    assert L.C.sizeof(L.StitchBlock) == 32 and "typedef struct bpx_stitch_block" in header
    make = open(os.path.join(ROOT, "biapy_amd", "csrc", "Makefile")).read()
    assert "stitch.hip" in make and re.search(r"^stitch\.o:.*stitch_core\.h.*label_uf\.h", make, re.M)
    core = open(os.path.join(ROOT, "biapy_amd", "csrc", "stitch_core.h")).read()
    assert '#include "stitch_core.h"' in source and '#include "label_uf.h"' in core and "lbl_unite" in core
    assert not re.search(r"\bST_HD \w+ stitch_\w+\(", source)                                  # the shared steps, not a copy
    assert "atomicAdd" not in source and set(re.findall(r"__hip_atomic_(\w+)\(", source)) == {"fetch_add", "fetch_min", "load", "store"}      # integer atomics only
    check = open(os.path.join(ROOT, "scripts", "stitch_cpu_check.cpp")).read()
    assert '#include "stitch_core.h"' in check and '#include "label_uf.h"' in check and "int main()" in check and "-fsanitize=address,undefined" in check
    from biapy_amd import prepost

    assert callable(prepost.label_blocks) and {"add", "resolve", "apply"} <= set(dir(prepost.LabelStitcher))


def test_host_checks_answer_without_a_device_in_the_stated_order():
    from biapy_amd import _lib as L

    lib = L.lib

    def err():
        return lib.bpx_last_error().decode()

    def begin(nums=A, nb=4, t=100, offs=A, parent=A, first=A, key=A, flag=A):
        return lib.bpx_stitch_begin(nums, nb, t, offs, parent, first, key, flag, None)

    assert begin(nums=None, nb=0) and "null pointer" in err()
    assert begin(nb=0, t=0) and "number of blocks" in err()
    assert begin(nb=1 << 20) and "number of blocks" in err()
    assert begin(t=0, offs=A + 4) and "t_max" in err()
    assert begin(offs=A + 4) and "aligned" in err()

    def first(labels=A, ext=(2, 3, 4), org=(0, 0, 0), Y=3, X=4, num=A, off=A, t=100, fst=A):
        return lib.bpx_stitch_first(labels, *ext, *org, Y, X, num, off, t, fst, None)

    assert first(fst=None, ext=(0, 3, 4)) and "null pointer" in err()
    assert first(ext=(0, 3, 4), org=(-1, 0, 0)) and "block extents" in err()
    assert first(ext=(2048, 1024, 1024), org=(-1, 0, 0), Y=1024, X=1024) and "2^31" in err()
    assert first(org=(0, -1, 0), Y=1) and "origin" in err()
    assert first(org=(0, 1, 0), t=0) and "leaves the volume" in err()
    assert first(t=0, labels=A + 2) and "t_max" in err()
    assert first(labels=A + 2) and "aligned" in err()

    def shell(desc=A, vol=(13, 21, 70), blk=(5, 8, 33), c=1, nums=A, offs=A, t=100, parent=A):
        return lib.bpx_stitch_shell(desc, *vol, *blk, c, nums, offs, t, parent, None)

    assert shell(desc=None, vol=(0, 1, 1)) and "null pointer" in err()
    assert shell(vol=(0, 21, 70), blk=(0, 8, 33)) and "extents must be at least 1" in err()
    assert shell(blk=(5, 0, 33), c=0) and "block extents" in err()
    assert shell(vol=(4096, 1024, 1024), blk=(2048, 1024, 1024), c=0) and "per block" in err()
    assert shell(vol=(1024, 1024, 1024), blk=(1, 1, 1), c=0) and "2^20 blocks" in err()
    assert shell(c=0, t=0) and "connectivity" in err()
    assert shell(c=4, t=0) and "connectivity" in err()
    assert shell(t=0, nums=A + 2) and "t_max" in err()
    assert shell(nums=A + 2) and "aligned" in err()

    def contact(desc=A, vol=(13, 21, 70), blk=(5, 8, 33), nums=A, offs=A, t=100, p=1, q=2, mp=64, parent=A, flag=A, ws=A, wb=1 << 30):
        return lib.bpx_stitch_contact(desc, *vol, *blk, nums, offs, t, p, q, mp, parent, flag, ws, wb, None)

    assert contact(ws=None, vol=(0, 1, 1)) and "null pointer" in err()
    assert contact(vol=(13, 0, 70), t=0) and "extents must be at least 1" in err()
    assert contact(blk=(5, 8, 0), t=0) and "block extents" in err()
    assert contact(t=0, p=0) and "t_max" in err()
    for p, q in ((0, 2), (3, 2), (1, 32769)):
        assert contact(p=p, q=q, mp=0) and "min_contact" in err()
    assert contact(mp=0, wb=0) and "max_pairs" in err()
    assert contact(mp=1 << 31, wb=0) and "refused" in err()
    assert contact(wb=16, ws=A + 4) and "workspace too small" in err()
    assert contact(ws=A + 4) and "aligned" in err()
    assert lib.bpx_stitch_contact_workspace(13, 21, 70, 5, 8, 33, 100, 64) > 0 and lib.bpx_stitch_contact_workspace(13, 21, 70, 5, 8, 33, 0, 64) < 0
    assert lib.bpx_stitch_contact_workspace(0, 21, 70, 5, 8, 33, 100, 64) < 0 and lib.bpx_stitch_contact_workspace(13, 21, 70, 5, 8, 33, 100, 0) < 0

    def resolve(parent=A, first=A, key=A, total=A, t=100, flag=A):
        return lib.bpx_stitch_resolve(parent, first, key, total, t, flag, None)

    assert resolve(total=None, t=0) and "null pointer" in err()
    assert resolve(t=0, key=A + 4) and "t_max" in err()
    assert resolve(key=A + 4) and "aligned" in err()

    def apply(labels=A, n=24, num=A, off=A, t=100, mp=A, flag=A):
        return lib.bpx_stitch_apply(labels, n, num, off, t, mp, flag, None)

    assert apply(mp=None, n=0) and "null pointer" in err()
    assert apply(n=0, t=0) and "at least 1" in err()
    assert apply(n=1 << 31, t=0) and "2^31" in err()
    assert apply(t=0, off=A + 4) and "t_max" in err()
    assert apply(off=A + 4) and "aligned" in err()


def test_python_refusals_in_order():
    from biapy_amd import prepost as P

    S = P.LabelStitcher
    with pytest.raises(ValueError, match="2-D .* or 3-D"):
        S((2, 3, 4, 5), (1, 1, 1, 1), connectivity=9)
    with pytest.raises(ValueError, match="every extent"):
        S((0, 3, 4), (1, 1))
    with pytest.raises(ValueError, match="block_shape must have 3 entries"):
        S((2, 3, 4), (1, 1), connectivity=9)
    with pytest.raises(ValueError, match="block extents must be at least 1"):
        S((2, 3, 4), (1, 0, 1), connectivity=9)
    with pytest.raises(NotImplementedError, match="2\\^31 voxels or more"):
        S((4096, 1024, 1024), (2048, 1024, 1024), connectivity=9)
    with pytest.raises(ValueError, match="connectivity must be in 1..2"):
        S((30, 40), (8, 8), connectivity=3, rule="x")
    with pytest.raises(ValueError, match="rule must be"):
        S((2, 30, 40), (1, 8, 8), rule="iou", min_contact=(0, 1))
    with pytest.raises(ValueError, match="connectivity must be 1"):
        S((2, 30, 40), (1, 8, 8), connectivity=2, rule="contact", min_contact=(0, 1))
    for mc in ((0, 1), (3, 2), (1, 32769)):
        with pytest.raises(ValueError, match="min_contact"):
            S((2, 30, 40), (1, 8, 8), rule="contact", min_contact=mc, max_labels=0)
    with pytest.raises(ValueError, match="max_labels"):
        S((2, 30, 40), (1, 8, 8), max_labels=0)
    with pytest.raises(NotImplementedError, match="2\\^20 blocks"):
        S((128, 128, 128), (1, 1, 1))
    s = S((13, 21, 70), (5, 8, 33), 3)
    assert (s.grid, s.nblocks, s.max_labels, s.shape) == ((3, 3, 3), 27, 13 * 21 * 70, (13, 21, 70))
    assert S((1 << 12, 1 << 12, 1 << 12), (64, 1 << 12, 1 << 12)).max_labels == 2 ** 22 and S((33, 70), (8, 33)).grid == (1, 5, 3)
    with pytest.raises(NotImplementedError, match="int32"):
        s.add((9, 9, 9), torch.zeros((5, 8, 33), dtype=torch.int64))
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        s.add((9, 9, 9), torch.zeros((5, 8), dtype=torch.int32))
    with pytest.raises(ValueError, match="not been added"):
        s.resolve()
    with pytest.raises(ValueError, match="resolve\\(\\) comes first"):
        s.apply()
    with pytest.raises(NotImplementedError, match="uint8 or bool"):
        P.label_blocks(torch.zeros((4, 4), dtype=torch.float32))
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        P.label_blocks(torch.zeros((4, 4, 4, 4), dtype=torch.uint8), block_shape=(0,), connectivity=7)
    with pytest.raises(NotImplementedError, match="uint8 or bool"):                    # prepost.label itself is as it was
        P.label(torch.zeros((4, 4), dtype=torch.float32))


# ---- the twin ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.all_masks()))
def test_touch_twin_equals_scipy_on_every_gpu_input(name):
    mask, blocks = R.all_masks()[name]
    extra = ((4, 21, 70), (5, 21, 70)) if mask.shape == R.SHAPE and len(blocks) == 1 else ()       # the Z slabs label_blocks is forced to
    for c in range(1, mask.ndim + 1):
        want, n = R.scipy_label(mask, c)
        for block in tuple(blocks) + extra:
            per, nums = R.label_per_block(mask, block, c)
            got, M = R.stitch_ref(per, nums, mask.shape, block, c)
            assert M == n and np.array_equal(R.assemble(got, mask.shape, block), want), (name, c, block)


def test_twin_cases_say_what_they_should():
    s = R.structured()
    count = lambda name, c: R.scipy_label(s[name], c)[1]
    assert [count("corner pair", c) for c in (1, 2, 3)] == [2, 2, 1] and [count("edge pair", c) for c in (1, 2, 3)] == [2, 1, 1]
    assert [count("edge pair high x", c) for c in (1, 2, 3)] == [2, 1, 1]
    assert count("all zero", 3) == 0 and count("all one", 1) == 1 and count("checkerboard", 1) == s["checkerboard"].sum() and count("checkerboard", 2) == 1
    assert count("boustrophedon", 1) == 1
    slices = R.block_slices(R.SHAPE, R.BLOCK)
    assert not any(s["empty blocks between"][sl].any() for b, sl in enumerate(slices) if b % 3 == 1) and s["empty blocks between"][slices[2]].any()
    # numbering by the smallest id's block, or by the root id's own first voxel, gives another answer than SciPy's on this one
    m = s["first voxel in a later block"]
    want, n = R.scipy_label(m, 1)
    assert n == 6 and want[0, 8, 5] == 2 and want[0, 8, 30] == want[1, 7, 33] == 3 and want[0, 9, 0] == 4 and want[0, 20, 5] == 5 and want[1, 0, 50] == 6
    block_of = {p: next(b for b, sl in enumerate(slices) if all(q.start <= v < q.stop for q, v in zip(sl, p))) for p in ((0, 8, 30), (1, 7, 33), (0, 8, 5))}
    assert block_of[(1, 7, 33)] < block_of[(0, 8, 5)] == block_of[(0, 8, 30)]
    per, nums = R.label_per_block(m, R.BLOCK, 1)
    _, M = R.stitch_ref(per, nums, R.SHAPE, R.BLOCK, 1, max_labels=sum(nums))
    assert M == 6 and R.stitch_ref(per, nums, R.SHAPE, R.BLOCK, 1, max_labels=sum(nums) - 1)[1] == -1


def test_contact_twin_equals_the_brute_force_count():
    rng = np.random.default_rng(5)
    for shape, block in (((4, 6, 9), (2, 3, 4)), ((1, 7, 8), (1, 3, 3)), ((5, 5, 5), (5, 2, 5))):
        for mc in ((1, 2), (1, 4), (2, 3), (1, 1)):
            blocks = [rng.integers(-1, 5, tuple(sl.stop - sl.start for sl in s)).astype(np.int32) for s in R.block_slices(shape, block)]
            nums = [3] * len(blocks)                                              # label 4 is above n_b: background
            G, _, T = R._global_ids(blocks, nums, shape, block)
            offs = np.concatenate(([0], np.cumsum(nums)))
            want = {(int(offs[a[0]] + a[1]), int(offs[b[0]] + b[1])) for a, b in R.contact_brute(blocks, nums, shape, block, mc)}
            got = {(a, b) for a, b, c, sa, sb in R.contact_pairs(G, shape, block) if c * mc[1] >= mc[0] * min(sa, sb)}
            assert got == want and T == 3 * len(blocks)
            out, M = R.stitch_ref(blocks, nums, shape, block, 1, "contact", mc)
            whole = R.assemble(out, shape, block)
            assert M == whole.max() == len(np.unique(whole[whole > 0])) and np.array_equal(whole > 0, G > 0)
            for a, b in want:                                                     # every united pair carries one label, first voxels number them
                assert set(whole[G == a]) == set(whole[G == b])
            firsts = [np.flatnonzero(whole.ravel() == l)[0] for l in range(1, M + 1)]
            assert firsts == sorted(firsts)


@pytest.mark.parametrize("name", sorted(R.contact_cases()))
def test_hand_made_contact_cases(name):
    blocks, nums, shape, block, mc, expect = R.contact_cases()[name]
    out, M = R.stitch_ref(blocks, nums, shape, block, 1, "contact", mc)
    assert M == expect, name
    whole, before = R.assemble(out, shape, block), R.assemble(blocks, shape, block)
    assert np.array_equal(whole > 0, before > 0)
    if name == "ball cut by a face":
        assert set(whole[before > 0]) == {1}
    if name == "chain of three":
        assert set(whole[before > 0]) == {1} and not (set(zip(*np.nonzero(blocks[0][0, :, -1]))) & set(zip(*np.nonzero(blocks[2][0, :, 0]))))


def test_rods_closed_form_equals_scipy():
    for shape in ((5, 37, 45), (64, 64, 64), (2, 19, 18)):                                   # 64^3: the shape of the GPU test
        m = R.rods_mask(shape, "cpu").numpy()
        plane, count = R.rods_expected(shape, "cpu")
        want, n = R.scipy_label(m, 3)
        assert n == count and np.array_equal(want, np.broadcast_to(plane.numpy()[None], shape))
        assert R.rods_check(torch.from_numpy(want), shape) and not R.rods_check(torch.from_numpy(np.where(want == 2, 3, want)), shape)


# ---- the compiled kernels ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc to cross-compile the kernels to ISA")
def test_no_kernel_uses_scratch(tmp_path):
    out = str(tmp_path / "stitch.s")
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-result", "-S", "--cuda-device-only",   # the Makefile's flags
           os.path.join(ROOT, "biapy_amd", "csrc", "stitch.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)} failed:\n{r.stderr[-3000:]}"
    kernels = re.findall(r"\.name:\s+(_Z\w*stitch_\w*kernel\w*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", open(out).read())
    names = sorted(re.search(r"stitch_\w+?_kernel", k).group(0) for k, _ in kernels)
    assert names == ["stitch_apply_kernel"] * 2 + ["stitch_contact_kernel", "stitch_faces_kernel"] + ["stitch_first_kernel"] * 2 + [
        "stitch_init_kernel", "stitch_offsets_kernel", "stitch_resolve_kernel", "stitch_shell_kernel", "stitch_zero_kernel"], kernels
    for name, private in kernels:
        assert int(private) == 0, f"{name} keeps {private} bytes of scratch per lane"

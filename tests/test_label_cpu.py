"""Connected-component labelling - what can be checked without a GPU: the entry points are declared, exported and bound; every host-side
refusal names its cause before anything is launched; the workspace grows with the chunk count and is refused at 2^31 voxels; the NumPy
statement of the rule (tests/label_ref.py) equals ``scipy.ndimage.label`` bit for bit on the masks the device tests use; ``prepost.label``
refuses CPU tensors and other dtypes."""
import os
import re

import numpy as np
import pytest
import torch

import label_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bpx_label_workspace", "bpx_label_u8", "bpx_label_sizes", "bpx_label_filter")
A = 4096                                   # any non-null, aligned "device" address: nothing is launched


def test_entry_points_are_declared_exported_and_bound():
    from biapy_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    source = open(os.path.join(ROOT, "biapy_amd", "csrc", "label.hip")).read()
    assert set(re.findall(r'extern "C" \w+ (bpx_label_[a-z0-9_]+)\(', source)) == set(NAMES)
    for name in NAMES + ("bpx_debug_set_label_tiled",):
        assert re.search(r"^(int|int64_t) %s\(" % name, header, re.M), name
        assert name in L.EXPORTS and getattr(L.lib._raw, name) is not None, name
    make = open(os.path.join(ROOT, "biapy_amd", "csrc", "Makefile")).read()
    assert "label.hip" in make and "label_uf.h" in make
    assert "BPX_LABEL_TILED" in open(os.path.join(ROOT, "biapy_amd", "_lib.py")).read()
    assert L.lib._raw.bpx_label_workspace.restype is L.C.c_int64


def test_host_checks_answer_without_a_device():
    from biapy_amd import _lib as L

    lib = L.lib

    def err():
        return lib.bpx_last_error().decode()

    def label(mask=A, Z=9, Y=21, X=37, c=1, labels=A, num=A, ws=A, ws_bytes=None):
        need = lib.bpx_label_workspace(9, 21, 37) if ws_bytes is None else ws_bytes
        return lib.bpx_label_u8(mask, Z, Y, X, c, labels, num, ws, need, None)

    for kw in (dict(mask=None), dict(labels=None), dict(num=None), dict(ws=None)):
        assert label(**kw) != 0 and "null pointer" in err(), kw
    for kw in (dict(Z=0), dict(Y=0), dict(X=-1)):
        assert label(**kw) != 0 and "extents must be at least 1" in err(), kw
    for c in (0, 4, -1):
        assert label(c=c) != 0 and "connectivity must be 1, 2 or 3" in err(), c
    assert label(ws_bytes=lib.bpx_label_workspace(9, 21, 37) - 1) != 0 and "workspace too small" in err()
    assert label(ws_bytes=0) != 0 and "workspace too small" in err()
    assert label(Z=2048, Y=1024, X=1024, ws_bytes=1 << 40) != 0 and "2^31 voxels or more" in err()
    assert label(Z=1, Y=1, X=2 ** 31 - 1, ws_bytes=0) != 0 and "workspace too small" in err()      # one voxel short of the limit: admitted
    assert label(labels=A + 2) != 0 and "4-byte aligned" in err()

    assert lib.bpx_label_sizes(None, 100, 5, A, None) != 0 and "null pointer" in err()
    assert lib.bpx_label_sizes(A, 100, 5, None, None) != 0 and "null pointer" in err()
    assert lib.bpx_label_sizes(A, 0, 5, A, None) != 0 and "extents must be at least 1" in err()
    assert lib.bpx_label_sizes(A, 2 ** 31, 5, A, None) != 0 and "2^31 voxels or more" in err()
    assert lib.bpx_label_sizes(A, 100, -1, A, None) != 0 and "n_max" in err()
    assert lib.bpx_label_filter(None, 100, 5, A, 3, 0, A, None) != 0 and "null pointer" in err()
    assert lib.bpx_label_filter(A, 100, 5, None, 3, 0, A, None) != 0 and "null pointer" in err()
    assert lib.bpx_label_filter(A, 0, 5, A, 3, 1, A, None) != 0 and "extents must be at least 1" in err()
    assert lib.bpx_label_filter(A, 2 ** 31, 5, A, 3, 1, None, None) != 0 and "2^31 voxels or more" in err()
    assert lib.bpx_label_filter(A, 100, -2, A, 3, 1, A, None) != 0 and "n_max" in err()


def test_workspace_grows_with_the_chunks_and_is_refused_at_2_to_the_31():
    from biapy_amd import _lib as L

    ws = L.lib.bpx_label_workspace
    chunk = 4096
    assert ws(1, 1, 1) == 4 and ws(1, 1, chunk) == 4 and ws(1, 1, chunk + 1) == 8
    assert ws(9, 21, 37) == 4 * -(-9 * 21 * 37 // chunk)
    sizes = [ws(s, s, s) for s in (16, 64, 256, 1024)]
    assert sizes == [4 * (s ** 3 // chunk) for s in (16, 64, 256, 1024)] and sizes == sorted(set(sizes))     # 1024^3 = 2^30 fits: O(chunks)
    assert ws(1, 1, 2 ** 31 - 1) == 4 * 2 ** 19
    assert ws(2048, 1024, 1024) < 0 and ws(1, 2 ** 16, 2 ** 15) < 0 and ws(1300, 1300, 1300) < 0             # 2^31 and beyond
    assert ws(0, 4, 4) < 0 and ws(4, -1, 4) < 0


def test_generate_structure_is_scipys():
    from scipy import ndimage

    for nd in (2, 3):
        for c in range(1, nd + 1):
            assert np.array_equal(R.generate_structure(nd, c), ndimage.generate_binary_structure(nd, c))
    assert [int(R.generate_structure(3, c).sum()) - 1 for c in (1, 2, 3)] == [6, 18, 26]
    assert [int(R.generate_structure(2, c).sum()) - 1 for c in (1, 2)] == [4, 8]


def _same_as_scipy(mask, c):
    lab, n = R.label_ref(mask, c)
    want, wn = R.scipy_label(mask, c)
    assert lab.dtype == np.int32 and want.dtype == np.int32
    assert n == wn
    np.testing.assert_array_equal(lab, want)
    return n


@pytest.mark.parametrize("c", [1, 2, 3])
def test_reference_equals_scipy_on_the_random_masks(c):
    counts = []
    for p in R.DENSITIES:
        mask = R.random_masks((9, 21, 37))[c, p]
        counts.append(_same_as_scipy(mask, c))
        first = [int(np.flatnonzero(R.scipy_label(mask, c)[0].ravel() == k)[0]) for k in range(1, counts[-1] + 1)]
        assert first == sorted(first)                                     # labels 1..N in raster order of the components' first voxels
    assert all(n > 1 for n, p in zip(counts, R.DENSITIES) if p <= 0.32)   # the non-trivial cases are non-trivial
    if c in R.REF_COUNTS:
        assert tuple(counts) == R.REF_COUNTS[c]


@pytest.mark.parametrize("shape", [(2, 64, 128), (17, 16, 200), (1, 33, 70), (33, 70), (5, 1, 1), (1, 1, 300)], ids=str)
def test_reference_equals_scipy_on_the_other_shapes(shape):
    total = 0
    for (c, p), mask in R.random_masks(shape).items():
        total += _same_as_scipy(mask, c)
    assert total > 1


@pytest.mark.parametrize("name", R.STRUCTURED)
def test_reference_equals_scipy_on_the_structured_masks(name):
    mask = R.structured(name)
    counts = tuple(_same_as_scipy(mask, c) for c in (1, 2, 3))
    assert counts == R.STRUCTURED_COUNTS[name]
    if name in ("checkerboard", "pairs"):
        assert counts[0] > 1 and counts[0] > counts[2]
    if name == "checkerboard":
        assert counts[0] == int(mask.sum())                               # connectivity 1: one component per set voxel


def test_two_dimensional_masks_are_the_z_equals_one_volumes():
    for (c, p), mask in R.random_masks((33, 70)).items():
        flat, n = R.scipy_label(mask, c)
        vol, nv = R.scipy_label(mask[None], c)                             # the 3-D structure of the same connectivity on a one-plane volume
        assert n == nv
        np.testing.assert_array_equal(flat, vol[0])


def test_label_refuses_cpu_tensors_and_other_dtypes():
    from biapy_amd import prepost

    with pytest.raises(RuntimeError, match="no CPU path"):
        prepost.label(torch.zeros(4, 5, 6, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        prepost.label(torch.zeros(5, 6, dtype=torch.bool), connectivity=1, return_num=True)
    for dt in (torch.float32, torch.int32, torch.int64, torch.float16):
        with pytest.raises(NotImplementedError, match="uint8 or bool"):
            prepost.label(torch.zeros(4, 5, 6, dtype=dt))
    with pytest.raises(RuntimeError, match="no CPU path"):
        prepost.component_sizes(torch.zeros(4, 5, 6, dtype=torch.int32), 3)
    with pytest.raises(NotImplementedError, match="int32 labels"):
        prepost.component_sizes(torch.zeros(4, 5, 6, dtype=torch.int64), 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        prepost.remove_small_objects(torch.zeros(4, 5, 6, dtype=torch.int32), 4, num=3)
    with pytest.raises(NotImplementedError, match="int32 labels"):
        prepost.remove_small_objects(torch.zeros(4, 5, 6, dtype=torch.uint8), 4)

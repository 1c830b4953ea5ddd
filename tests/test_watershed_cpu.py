"""Seeded watershed - what can be checked without a GPU: the entry points are declared, exported and bound; every host-side refusal names its
cause before anything is launched; the workspace is 12 bytes per voxel plus the round flags and is refused at 2^31 voxels; ``prepost.watershed``
refuses CPU tensors, dtypes, ranks, shapes and connectivities; and the reference statement (tests/watershed_ref.py) holds together: Kruskal equals
the synchronous-Boruvka statement, has the pass-height property on every reachable voxel, the key map is monotone, the plateau example is the
documented one."""
import os
import re

import numpy as np
import pytest
import torch

import watershed_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bpx_watershed_workspace", "bpx_watershed")
A = 4096                                   # any non-null, aligned "device" address: nothing is launched


def test_entry_points_are_declared_exported_and_bound():
    from biapy_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    source = open(os.path.join(ROOT, "biapy_amd", "csrc", "watershed.hip")).read()
    assert set(re.findall(r'extern "C" \w+ (\w+)\(', source)) == set(NAMES)
    for name in NAMES:
        assert re.search(r"^(int|int64_t) %s\(" % name, header, re.M), name
        assert name in L.EXPORTS and getattr(L.lib._raw, name) is not None, name
    make = open(os.path.join(ROOT, "biapy_amd", "csrc", "Makefile")).read()
    assert "watershed.hip" in make and re.search(r"^watershed\.o:.*watershed_core\.h.*label_uf\.h", make, re.M)
    assert L.lib._raw.bpx_watershed_workspace.restype is L.C.c_int64
    assert L.lib._raw.bpx_watershed.restype is L.C.c_int
    core = open(os.path.join(ROOT, "biapy_amd", "csrc", "watershed_core.h")).read()
    assert '#include "label_uf.h"' in core and "lbl_unite(" in core and "lbl_find(" in core        # the labelling's union-find, not a copy
    assert not re.search(r"\blbl_(find|unite)\s*\(const M& m, int", core + source)


def test_host_checks_answer_without_a_device():
    from biapy_amd import _lib as L

    lib = L.lib

    def err():
        return lib.bpx_last_error().decode()

    def ws(image=A, dtype=L.F32, markers=A, mask=A, Z=9, Y=21, X=37, c=1, out=A, rounds=A, w=A, ws_bytes=None):
        need = lib.bpx_watershed_workspace(9, 21, 37) if ws_bytes is None else ws_bytes
        return lib.bpx_watershed(image, dtype, markers, mask, Z, Y, X, c, out, rounds, w, need, None)

    for kw in (dict(image=None), dict(markers=None), dict(out=None), dict(rounds=None), dict(w=None)):
        assert ws(**kw) != 0 and "null pointer" in err(), kw
    for dt in (L.U8, L.BF16, L.F16, 7, -1):
        assert ws(dtype=dt) != 0 and "BPX_F32 or BPX_I32" in err(), dt
    for kw in (dict(Z=0), dict(Y=0), dict(X=-1)):
        assert ws(**kw) != 0 and "extents must be at least 1" in err(), kw
    for c in (0, 4, -1):
        assert ws(c=c) != 0 and "connectivity must be 1, 2 or 3" in err(), c
    assert ws(ws_bytes=lib.bpx_watershed_workspace(9, 21, 37) - 1) != 0 and "workspace too small" in err()
    assert ws(ws_bytes=0) != 0 and "workspace too small" in err()
    assert ws(Z=2048, Y=1024, X=1024, ws_bytes=1 << 45) != 0 and "2^31 voxels or more" in err()
    assert ws(Z=1, Y=1, X=2 ** 31 - 1, ws_bytes=0) != 0 and "workspace too small" in err()      # one voxel short of the limit: admitted
    for kw in (dict(image=A + 2), dict(markers=A + 1), dict(out=A + 2), dict(rounds=A + 3), dict(w=A + 4)):
        assert ws(**kw) != 0 and "aligned" in err(), kw


def test_workspace_is_12_bytes_per_voxel_plus_the_flags_and_is_refused_at_2_to_the_31():
    from biapy_amd import _lib as L

    ws = L.lib.bpx_watershed_workspace
    sizes = []
    for shape in ((1, 1, 1), (1, 1, 2), (9, 21, 37), (64, 64, 64), (256, 256, 256), (1024, 1024, 1024), (1, 1, 2 ** 31 - 1)):
        n = shape[0] * shape[1] * shape[2]
        flags = ws(*shape) - 12 * n
        assert 4 * (W.rounds_bound(n) + 1) <= flags <= 4 * (W.rounds_bound(n) + 1) + 8, (shape, flags)       # one flag per round and one more
        sizes.append(ws(*shape))
    assert sizes == sorted(set(sizes))
    assert 12.8e9 < ws(1024, 1024, 1024) < 13.0e9                                                             # the docstring's 12.9 GB
    assert ws(2048, 1024, 1024) < 0 and ws(1, 2 ** 16, 2 ** 15) < 0 and ws(1300, 1300, 1300) < 0              # 2^31 and beyond
    assert ws(0, 4, 4) < 0 and ws(4, -1, 4) < 0


def test_rounds_bound_is_the_formula():
    assert [W.rounds_bound(n) for n in (1, 2, 3, 4, 5, 8, 9, 2 ** 18, 2 ** 18 + 1, 2 ** 30, 2 ** 31 - 1)] == [2, 2, 3, 3, 4, 4, 5, 19, 20, 31, 32]


def test_watershed_refuses_before_any_launch():
    from biapy_amd import prepost

    img, mk, m = torch.zeros(4, 5, 6), torch.zeros(4, 5, 6, dtype=torch.int32), torch.ones(4, 5, 6, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        prepost.watershed(img, mk)
    with pytest.raises(RuntimeError, match="no CPU path"):
        prepost.watershed(img.int(), mk, m.bool(), connectivity=3, return_rounds=True)
    for dt in (torch.float64, torch.float16, torch.int64, torch.uint8):
        with pytest.raises(NotImplementedError, match="float32 or int32 images"):
            prepost.watershed(img.to(dt), mk)
    for dt in (torch.int64, torch.uint8, torch.float32):
        with pytest.raises(NotImplementedError, match="int32 markers"):
            prepost.watershed(img, mk.to(dt))
    for dt in (torch.int32, torch.float32):
        with pytest.raises(NotImplementedError, match="uint8 or bool masks"):
            prepost.watershed(img, mk, m.to(dt))
    for shape in ((7,), (2, 3, 4, 5)):
        with pytest.raises(ValueError, match="2-D .* or 3-D"):
            prepost.watershed(torch.zeros(shape), torch.zeros(shape, dtype=torch.int32))
    with pytest.raises(ValueError, match="same shape"):
        prepost.watershed(img, mk[:3])
    with pytest.raises(ValueError, match="same shape"):
        prepost.watershed(img, mk, m[:, :, :5])
    with pytest.raises(ValueError, match="same shape"):
        prepost.watershed(img[0], mk[0], m)
    for c in (0, 4, -1):
        with pytest.raises(ValueError, match="connectivity must be in 1..3"):
            prepost.watershed(img, mk, m, connectivity=c)
    with pytest.raises(ValueError, match="connectivity must be in 1..2"):
        prepost.watershed(img[0], mk[0], connectivity=3)


def _small_cases():
    """60 random volumes up to 6^3: connectivity 1-3, 1 / 2 / 4 / 1000 image levels, both dtypes, masks at 60-100 %."""
    rng = np.random.default_rng(7)
    for k in range(60):
        shape = tuple(int(v) for v in rng.integers(1, 7, size=3))
        levels, dtype = (1, 2, 4, 1000)[k % 4], (np.int32, np.float32)[(k // 4) % 2]
        keep, seeds = (0.6, 0.8, 1.0)[k % 3], (0.03, 0.1)[(k // 2) % 2]
        yield W.random_case(shape, levels, dtype, keep, seeds, seed=k) + (1 + k % 3,)


def test_kruskal_equals_synchronous_boruvka_and_has_the_pass_height_property():
    reachable = seeded_cases = 0
    for image, markers, mask, c in _small_cases():
        want = W.watershed_ref(image, markers, mask, c)
        got, rounds = W.boruvka_ref(image, markers, mask, c)
        assert want.dtype == np.int32 and want.shape == image.shape
        np.testing.assert_array_equal(got, want)
        assert rounds <= W.rounds_bound(image.size)
        inside = np.ones(image.shape, bool) if mask is None else mask != 0
        seeded = inside & (markers > 0)
        np.testing.assert_array_equal(want[seeded], markers[seeded])             # a seed keeps its label
        assert not want[~inside].any()
        reachable += W.check_pass_heights(image, markers, mask, c, want)
        seeded_cases += bool(seeded.any())
    assert seeded_cases > 40 and reachable > 1000                                # the cases are not trivial


def test_two_dimensional_images_are_the_z_equals_one_volumes():
    image, markers, mask = W.random_case((13, 17), 4, np.int32, 0.9, 0.05)
    for c in (1, 2):
        flat = W.watershed_ref(image, markers, mask, c)
        vol = W.watershed_ref(image[None], markers[None], mask[None], c)
        assert flat.shape == (13, 17) and np.array_equal(flat, vol[0]) and flat.any()


def test_okey_is_monotone():
    f = np.array([-np.inf, -3.5, -1e-38, -1e-45, -0.0, 0.0, 1e-45, 1e-40, 1.17549435e-38, 1.0, 3.4e38, np.inf], np.float32)
    kf = W.okey(f).astype(np.int64)
    assert (np.diff(kf) > 0).all()                                               # strictly: -0.0 < +0.0, denormals in their place
    i = np.array([np.iinfo(np.int32).min, -2 ** 31 + 1, -1, 0, 1, 2 ** 31 - 2, np.iinfo(np.int32).max], np.int32)
    ki = W.okey(i).astype(np.int64)
    assert (np.diff(ki) > 0).all() and ki[0] == 0 and ki[-1] == 2 ** 32 - 1
    rng = np.random.default_rng(0)
    r = rng.standard_normal(1000).astype(np.float32)
    assert np.array_equal(np.argsort(W.okey(r), kind="stable"), np.argsort(r, kind="stable"))


def test_plateau_goes_to_the_raster_first_edge_and_the_recipe_splits_it():
    markers = np.zeros((1, 21), np.int32)
    markers[0, 0], markers[0, 20] = 1, 2
    flat = np.zeros((1, 21), np.int32)
    out = W.watershed_ref(flat, markers)
    assert (out == 1).sum() == 20 and (out == 2).sum() == 1                      # the index tie-break: no split in the middle
    out = W.watershed_ref(W.plateau_recipe(flat, markers), markers)
    assert out[0].tolist() == [1] * 11 + [2] * 10                                # the recipe: the Voronoi boundary
    both, rounds = W.boruvka_ref(W.plateau_recipe(flat, markers), markers)
    assert np.array_equal(both, out) and rounds <= W.rounds_bound(21)


def test_unreached_regions_and_ignored_markers():
    image = np.zeros((1, 5, 9), np.float32)
    mask = np.ones((1, 5, 9), np.uint8)
    mask[0, :, 4] = 0                                                            # a wall: the right half holds no seed
    markers = np.zeros((1, 5, 9), np.int32)
    markers[0, 2, 1], markers[0, 2, 4], markers[0, 0, 0] = 3, 8, -5              # one seed, one marker inside the wall, one negative marker
    out = W.watershed_ref(image, markers, mask)
    assert (out[0, :, :4] == 3).all() and not out[0, :, 4:].any()
    assert np.array_equal(W.boruvka_ref(image, markers, mask)[0], out)
    none, rounds = W.boruvka_ref(image, np.zeros_like(markers), mask)
    assert not none.any() and rounds == 0 and not W.watershed_ref(image, np.zeros_like(markers), mask).any()

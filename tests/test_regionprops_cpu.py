"""Region properties - what can be checked without a GPU: the entry points are declared, exported and bound; every host-side refusal of
``bpx_region_props`` names its cause before anything is launched; ``prepost.region_props`` / ``centroids`` / ``select_objects`` refuse on CPU
tensors; and the NumPy statement the GPU tests hold the device against (tests/regionprops_ref.py) agrees with ``np.bincount``,
``scipy.ndimage.find_objects`` and ``scipy.ndimage.center_of_mass`` on every input those tests use, and with hand-made cases."""
import os
import re

import numpy as np
import pytest
import torch

import regionprops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bpx_region_props", "bpx_debug_set_regionprops_local")
A = 4096                                   # any non-null, aligned "device" address: nothing is launched


def test_entry_points_are_declared_exported_and_bound():
    from biapy_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    source = open(os.path.join(ROOT, "biapy_amd", "csrc", "regionprops.hip")).read()
    assert set(re.findall(r'extern "C" \w+ (\w+)\(', source)) == set(NAMES)
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in L.EXPORTS and getattr(L.lib._raw, name) is not None, name
        assert getattr(L.lib._raw, name).restype is L.C.c_int
    vp, i = L.C.c_void_p, L.C.c_int
    assert L._SIGS["bpx_region_props"][0] == [vp, i, i, i, i, vp, vp, vp, vp]
    assert L._SIGS["bpx_debug_set_regionprops_local"][0] == [i]
    assert re.search(r"int bpx_region_props\(const int32_t\* labels_d, int Z, int Y, int X, int n_max, int32_t\* area_d, int64_t\* sums_d, "
                     r"int32_t\* bbox_d,\s+bpx_stream_t stream\);", header)
    make = open(os.path.join(ROOT, "biapy_amd", "csrc", "Makefile")).read()
    assert "regionprops.hip" in make and re.search(r"^regionprops\.o:.*regionprops_core\.h.*label_walk\.h", make, re.M)
    assert re.search(r"^shapeprops\.o:.*regionprops_core\.h.*label_walk\.h", make, re.M)
    csrc = os.path.join(ROOT, "biapy_amd", "csrc")
    core = open(os.path.join(csrc, "regionprops_core.h")).read()
    walk = open(os.path.join(csrc, "label_walk.h")).read()
    # the shared steps, not a copy: the one walk calls them, and both kernels that walk runs call the walk instead of writing it out
    assert '#include "regionprops_core.h"' in source and '#include "regionprops_core.h"' in walk
    assert "rp_carry_step(" in walk and "rp_is_head(" in walk and "ovl_first_head(" in walk
    for name in ("regionprops.hip", "shapeprops.hip"):
        text = source if name == "regionprops.hip" else open(os.path.join(csrc, name)).read()
        assert '#include "label_walk.h"' in text and "lw_walk_runs(" in text, name
        assert "rp_carry_step(" not in text and "__ballot(" not in text, name
    everything = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h", ".cpp"))}
    for definition in (r"void lw_walk_runs\(", r"int32_t kcas\(uint32_t s, int32_t label\)", r"void lw_load4\(", r"define LW_CHECK_VOLUME\("):
        assert [f for f, text in everything.items() for _ in re.findall(definition, text)] == ["label_walk.h"], definition      # one definition each
    assert not re.search(r"\bRP_HD \w+ rp_\w+\(", source)
    for fn in ("rp_label", "rp_is_head", "rp_step", "rp_advance", "rp_apply", "rp_local_slot", "rp_merge", "rp_carry_step", "rp_finish_row"):
        assert re.search(r"RP_HD \w+ %s\(" % fn, core), fn
    check = open(os.path.join(ROOT, "scripts", "regionprops_cpu_check.cpp")).read()
    assert '#include "regionprops_core.h"' in check and "int main()" in check and "-fsanitize=address,undefined" in check
    replay = open(os.path.join(ROOT, "scripts", "label_walk_host.h")).read()      # the host's one walk, called by both check programs
    assert "rp_carry_step(" in replay and "ovl_first_head(" in replay and "rp_carry_step(" not in check
    for prog in (check, open(os.path.join(ROOT, "scripts", "shapeprops_cpu_check.cpp")).read()):
        assert '#include "label_walk_host.h"' in prog and "lw_walk_runs_host(" in prog and "ovl_first_head(" not in prog
    assert "BPX_REGIONPROPS_LOCAL" in open(os.path.join(ROOT, "biapy_amd", "_lib.py")).read()


def test_host_checks_answer_without_a_device():
    from biapy_amd import _lib as L

    lib = L.lib

    def err():
        return lib.bpx_last_error().decode()

    def rp(labels=A, Z=4, Y=5, X=6, n_max=3, area=A, sums=A, bbox=A):
        return lib.bpx_region_props(labels, Z, Y, X, n_max, area, sums, bbox, None)

    for kw in (dict(labels=None), dict(area=None), dict(sums=None), dict(bbox=None)):
        assert rp(**kw) != 0 and "null pointer" in err(), kw
    for kw in (dict(Z=0), dict(Y=0), dict(X=0), dict(Z=-1), dict(X=-7)):
        assert rp(**kw) != 0 and "extents must be at least 1" in err(), kw
    for shape in ((2048, 1024, 1024), (1, 65536, 32768), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert rp(Z=shape[0], Y=shape[1], X=shape[2]) != 0 and "2^31 voxels or more" in err(), shape
    for n_max in (-1, -2 ** 31, 2 ** 31 - 1):
        assert rp(n_max=n_max) != 0 and "n_max must be in [0, 2^31 - 1)" in err(), n_max
    for kw in (dict(labels=A + 2), dict(area=A + 1), dict(bbox=A + 3), dict(sums=A + 4), dict(sums=A + 2)):
        assert rp(**kw) != 0 and "aligned" in err(), kw
    # the largest volume and n_max admitted pass every check but the last one made here: an unaligned sums pointer
    assert rp(Z=1, Y=1, X=2 ** 31 - 1, n_max=2 ** 31 - 2, sums=A + 4) != 0 and "aligned" in err()
    assert lib.bpx_debug_set_regionprops_local(1) == 0


def test_prepost_refuses_before_any_launch():
    from biapy_amd import prepost

    a = torch.zeros(4, 5, 6, dtype=torch.int32)
    for fn in (prepost.region_props, prepost.centroids):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(a)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(a[0], 3)
        for dt in (torch.int64, torch.uint8, torch.float32, torch.int16):
            with pytest.raises(NotImplementedError, match="int32 labels"):
                fn(a.to(dt), 3)
        for bad in (a.view(-1), a[None], a[0, 0, 0]):
            with pytest.raises(ValueError, match="2-D .* or 3-D"):
                fn(bad, 3)
        for num in (-1, -100, torch.tensor(-2)):
            with pytest.raises(ValueError, match="num must not be negative"):
                fn(a, num)
    keep = torch.ones(4, dtype=torch.bool)
    for dt in (torch.int32, torch.int64, torch.float32):
        with pytest.raises(NotImplementedError, match="keep must be a bool or uint8"):
            prepost.select_objects(a, keep.to(dt))
    for bad in (keep[:0], keep[None], keep[0]):
        with pytest.raises(ValueError, match=r"keep must have shape \(N \+ 1,\)"):
            prepost.select_objects(a, bad)
    for k in (keep, keep.to(torch.uint8)):
        with pytest.raises(RuntimeError, match="keep must be on the device"):
            prepost.select_objects(a, k)
    assert prepost.RegionProps._fields == ("area", "bbox", "coord_sum", "centroid")


def _scipy_props(labels, n_max):
    """area, bbox and centroid of the labels 1..n_max from np.bincount, scipy.ndimage.find_objects and center_of_mass."""
    from scipy import ndimage

    nd = labels.ndim
    clean = np.where((labels > 0) & (labels <= n_max), labels, 0)
    area = np.bincount(clean.ravel(), minlength=n_max + 1)[:n_max + 1].astype(np.int32)
    area[0] = 0
    bbox = np.zeros((n_max + 1, 2 * nd), np.int32)
    for l, sl in enumerate(ndimage.find_objects(clean, max_label=n_max), start=1):
        if sl is not None:
            bbox[l] = [s.start for s in sl] + [s.stop for s in sl]
    present = np.flatnonzero(area)
    centroid = np.full((n_max + 1, nd), np.nan)
    if present.size:
        centroid[present] = np.asarray(ndimage.center_of_mass((clean > 0).astype(np.float64), clean, present)).reshape(present.size, nd)
    return area, bbox, centroid


@pytest.mark.parametrize("name", list(R.cases()), ids=str)
def test_the_reference_agrees_with_scipy_on_every_gpu_input(name):
    labels, n_max = R.cases()[name]
    area, sums, bbox = R.region_props_ref(labels, n_max)
    want_area, want_bbox, want_centroid = _scipy_props(labels, n_max)
    np.testing.assert_array_equal(area, want_area)
    np.testing.assert_array_equal(bbox, want_bbox)
    centroid = R.centroid_ref(area, sums)
    assert np.array_equal(np.isnan(centroid), np.isnan(want_centroid))
    ok = area > 0
    # center_of_mass sums coordinate * weight in fp64 in another order: 1e-12 relative
    np.testing.assert_allclose(centroid[ok], want_centroid[ok], rtol=1e-12, atol=0)
    assert area.dtype == np.int32 and sums.dtype == np.int64 and bbox.dtype == np.int32
    assert int(area.sum()) == int(((labels > 0) & (labels <= n_max)).sum())


def test_one_voxel_in_each_corner():
    shape = (3, 4, 5)
    lab = np.zeros(shape, np.int32)
    corners = [(z, y, x) for z in (0, 2) for y in (0, 3) for x in (0, 4)]
    for l, c in enumerate(corners, start=1):
        lab[c] = l
    area, sums, bbox = R.region_props_ref(lab, 8)
    assert area.tolist() == [0] + [1] * 8
    for l, c in enumerate(corners, start=1):
        assert sums[l].tolist() == list(c) and bbox[l].tolist() == list(c) + [v + 1 for v in c]
    assert bbox[0].tolist() == [0] * 6 and sums[0].tolist() == [0] * 3
    lab[:] = 0
    for c in corners:
        lab[c] = 1                                                                          # one label in all eight corners: the whole volume's box
    area, sums, bbox = R.region_props_ref(lab, 1)
    assert area[1] == 8 and bbox[1].tolist() == [0, 0, 0, 3, 4, 5] and sums[1].tolist() == [8, 12, 16]
    assert R.centroid_ref(area, sums)[1].tolist() == [1.0, 1.5, 2.0]


def test_absent_labels_labels_above_n_max_and_negative_labels():
    lab = np.zeros((4, 6), np.int32)
    lab[1, 1:4], lab[2:4, 4:6], lab[0, 0], lab[3, 0] = 1, 3, 9, -4
    area, sums, bbox = R.region_props_ref(lab, 3)
    assert area.tolist() == [0, 3, 0, 4]
    assert bbox.tolist() == [[0, 0, 0, 0], [1, 1, 2, 4], [0, 0, 0, 0], [2, 4, 4, 6]]         # label 2 is absent between two present ones
    assert sums.tolist() == [[0, 0], [3, 6], [0, 0], [10, 18]]
    c = R.centroid_ref(area, sums)
    assert np.isnan(c[0]).all() and np.isnan(c[2]).all() and c[1].tolist() == [1.0, 2.0] and c[3].tolist() == [2.5, 4.5]
    area9, _, bbox9 = R.region_props_ref(lab, 9)                                              # with n_max = 9 the 9 counts; the -4 never does
    assert area9.tolist() == [0, 3, 0, 4, 0, 0, 0, 0, 0, 1] and bbox9[9].tolist() == [0, 0, 1, 1]
    area0, sums0, bbox0 = R.region_props_ref(lab, 0)
    assert area0.tolist() == [0] and not sums0.any() and not bbox0.any()

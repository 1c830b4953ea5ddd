"""Label overlap and instance matching - what can be checked without a GPU: the entry points are declared, exported and bound; every host-side
refusal of the C entry point names its cause before anything is launched; the workspace is the slots formula and is refused past 2^31 slots;
``prepost.label_overlap`` / ``prepost.matching`` refuse on CPU tensors; and the host half of the matcher (``prepost._match_stats``: sparse table,
one assignment per connected block) equals the reference's algorithm restated densely (tests/overlap_ref.py) on random and hand-made cases."""
import os
import re

import numpy as np
import pytest
import torch

import overlap_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bpx_overlap_workspace", "bpx_label_overlap", "bpx_debug_set_overlap_per_voxel")
A = 4096                                   # any non-null, aligned "device" address: nothing is launched
THRESHOLDS = (0.1, 0.3, 0.5, 0.75, 0.9)


def test_entry_points_are_declared_exported_and_bound():
    from biapy_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    source = open(os.path.join(ROOT, "biapy_amd", "csrc", "overlap.hip")).read()
    assert set(re.findall(r'extern "C" \w+ (\w+)\(', source)) == set(NAMES)
    for name in NAMES:
        assert re.search(r"^(int|int64_t) %s\(" % name, header, re.M), name
        assert name in L.EXPORTS and getattr(L.lib._raw, name) is not None, name
    make = open(os.path.join(ROOT, "biapy_amd", "csrc", "Makefile")).read()
    assert "overlap.hip" in make and re.search(r"^overlap\.o:.*overlap_core\.h.*label_walk\.h", make, re.M)
    assert L.lib._raw.bpx_overlap_workspace.restype is L.C.c_int64
    assert L.lib._raw.bpx_label_overlap.restype is L.C.c_int
    core = open(os.path.join(ROOT, "biapy_amd", "csrc", "overlap_core.h")).read()
    assert '#include "overlap_core.h"' in source and "ovl_insert(" in source and "ovl_carry_step(" in source      # the shared steps, not a copy
    assert not re.search(r"\bOVL_HD \w+ ovl_\w+\(", source)
    assert '#include "label_walk.h"' in source and "lw_load4(" in source and "label_walk" not in core      # the label load is the shared one; the core header stays the base
    for fn in ("ovl_key", "ovl_hash", "ovl_insert", "ovl_next_head", "ovl_carry_step", "ovl_slots"):
        assert re.search(r"OVL_HD \w+ %s\(" % fn, core), fn
    check = open(os.path.join(ROOT, "scripts", "overlap_cpu_check.cpp")).read()
    assert '#include "overlap_core.h"' in check and "int main()" in check and "-fsanitize=address,undefined" in check


def test_host_checks_answer_without_a_device():
    from biapy_amd import _lib as L

    lib = L.lib

    def err():
        return lib.bpx_last_error().decode()

    def ov(a=A, b=A, n=1000, mp=64, keys=A, counts=A, num=A, w=A, ws_bytes=None):
        need = lib.bpx_overlap_workspace(64) if ws_bytes is None else ws_bytes
        return lib.bpx_label_overlap(a, b, n, mp, keys, counts, num, w, need, None)

    for kw in (dict(a=None), dict(b=None), dict(keys=None), dict(counts=None), dict(num=None), dict(w=None)):
        assert ov(**kw) != 0 and "null pointer" in err(), kw
    for n in (0, -1):
        assert ov(n=n) != 0 and "n must be at least 1" in err(), n
    for n in (2 ** 31, 2 ** 33):
        assert ov(n=n) != 0 and "2^31 voxels or more" in err(), n
    assert ov(n=2 ** 31 - 1, ws_bytes=0) != 0 and "workspace too small" in err()                      # one voxel short of the limit: admitted
    for mp in (0, -5):
        assert ov(mp=mp) != 0 and "max_pairs must be at least 1" in err(), mp
    assert ov(mp=2 ** 30 + 1, ws_bytes=1 << 45) != 0 and "2^31 slots" in err()
    assert ov(ws_bytes=lib.bpx_overlap_workspace(64) - 1) != 0 and "workspace too small" in err()
    assert ov(ws_bytes=0) != 0 and "workspace too small" in err()
    assert ov(mp=65) != 0 and "workspace too small" in err()                                          # 65 pairs need 256 slots
    for kw in (dict(a=A + 2), dict(b=A + 1), dict(counts=A + 2), dict(num=A + 3), dict(keys=A + 4), dict(w=A + 4)):
        assert ov(**kw) != 0 and "aligned" in err(), kw


def test_workspace_is_the_slots_formula_and_is_refused_past_2_to_the_31_slots():
    from biapy_amd import _lib as L

    ws = L.lib.bpx_overlap_workspace
    sizes = []
    for mp in (1, 2, 3, 4, 5, 16, 17, 100, 128, 129, 8192, 2 ** 21, 2 ** 21 + 1, 2 ** 30 - 1, 2 ** 30):
        slots = 1 << max(1, (2 * mp - 1).bit_length())                       # the power of two >= 2 * max_pairs
        assert slots >= 2 * mp and (slots // 2 < 2 * mp or slots == 2)
        assert ws(mp) == 12 * slots + 16, mp                                 # a 64-bit key and a 32-bit count per slot, two counters
        sizes.append(ws(mp))
    assert sizes == sorted(sizes)
    assert 48e6 < ws(2 ** 21) < 51e6                                          # the docstring's 48 MB at the default
    assert ws(2 ** 30) == 12 * 2 ** 31 + 16                                   # 2^31 slots: the last size admitted
    assert ws(2 ** 30 + 1) < 0 and ws(2 ** 31) < 0 and ws(2 ** 40) < 0        # the table would pass 2^31 slots
    assert ws(0) < 0 and ws(-3) < 0


def test_label_overlap_and_matching_refuse_before_any_launch():
    from biapy_amd import prepost

    a = torch.zeros(4, 5, 6, dtype=torch.int32)
    for fn in (prepost.label_overlap, prepost.matching):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(a, a)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(a.view(-1), a.view(-1), max_pairs=7)
        for dt in (torch.int64, torch.uint8, torch.float32, torch.int16):
            with pytest.raises(NotImplementedError, match="int32 labels"):
                fn(a.to(dt), a)
            with pytest.raises(NotImplementedError, match="int32 labels"):
                fn(a, a.to(dt))
        with pytest.raises(NotImplementedError, match="empty"):
            fn(a[:0], a[:0])
        for mp in (2 ** 30 + 1, 2 ** 40):
            with pytest.raises(NotImplementedError, match="2\\^31 slots"):
                fn(a, a, max_pairs=mp)
        for other in (a[:3], a[0], a.view(-1), a.permute(2, 1, 0)):
            with pytest.raises(ValueError, match="same shape"):
                fn(a, other)
        for mp in (0, -1):
            with pytest.raises(ValueError, match="max_pairs must be at least 1"):
                fn(a, a, max_pairs=mp)
    for crit in ("iot", "iop", "IoU"):
        with pytest.raises(NotImplementedError, match="criterion"):
            prepost.matching(a, a, criterion=crit)


def test_the_package_does_not_import_scipy_at_load():
    import subprocess
    import sys

    code = "import sys; sys.path.insert(0, %r); import biapy_amd.prepost; assert 'scipy' not in sys.modules, 'scipy imported at load'" % ROOT
    subprocess.run([sys.executable, "-c", code], check=True)


def _stats(y_true, y_pred, thr):
    from biapy_amd import prepost

    pairs, counts = O.overlap_ref(y_true, y_pred)
    return prepost._match_stats(pairs, counts, thr)


def _cases():
    """64 random pairs, 2-D and 3-D, 6^3 .. 16^3 voxels, 0..40 labels per side: a ground truth, and a prediction that is the same blobs
    perturbed (another seed on a fifth of the cases: unrelated blobs) so that matches exist at every threshold."""
    rng = np.random.default_rng(2024)
    for k in range(64):
        side = int(rng.integers(6, 17))
        shape = (side, side, side) if k % 2 else (side * side, side)
        nt = int(rng.integers(0, 41)) if k % 16 else 0
        y_true = O.random_labels(shape, nt, fill=0.7, seed=1000 + k)
        if k % 5 == 0:
            y_pred = O.random_labels(shape, int(rng.integers(0, 41)), fill=0.6, seed=5000 + k)
        else:                                                                # shift by a voxel, drop some labels, merge some
            y_pred = np.roll(y_true, 1, axis=-1).copy()
            ids = np.unique(y_pred[y_pred > 0])
            for i in ids[rng.random(ids.size) < 0.15]:
                y_pred[y_pred == i] = 0
            for i in ids[rng.random(ids.size) < 0.15]:
                y_pred[y_pred == i] = int(rng.choice(ids))
            y_pred[rng.random(y_pred.shape) < 0.1] = 0
        yield k, y_true, y_pred


def _permuted(y, rng):
    """The same partition under other label ids (a random injection into 1 .. 10^6)."""
    ids = np.unique(y[y > 0])
    new = rng.choice(np.arange(1, 10 ** 6), size=ids.size, replace=False)
    out = np.zeros_like(y)
    for i, j in zip(ids, new):
        out[y == i] = j
    return out


def test_match_stats_equals_the_dense_reference_on_random_cases():
    rng = np.random.default_rng(5)
    with_tp = with_fp = with_fn = n = 0
    for k, y_true, y_pred in _cases():
        n += 1
        assert y_true.size <= 16 ** 3 and len(np.unique(y_true)) <= 41 and len(np.unique(y_pred)) <= 41
        pt, pp = _permuted(y_true, rng), _permuted(y_pred, rng)
        for thr in THRESHOLDS:
            want = O.matching_ref(y_true, y_pred, thr)
            # the optimum is unique as far as the statistics go: the dense reference gives the same sums under other label ids (another row and
            # column order of its cost matrix)
            O.assert_same_stats(O.matching_ref(pt, pp, thr), want, f"case {k} thr {thr}: the reference under permuted labels")
            O.assert_same_stats(_stats(y_true, y_pred, thr), want, f"case {k} thr {thr}")
            O.assert_same_stats(_stats(pt, pp, thr), want, f"case {k} thr {thr} permuted")
            assert want["tp"] + want["fn"] == want["n_true"] and want["tp"] + want["fp"] == want["n_pred"]
        w = O.matching_ref(y_true, y_pred, 0.5)
        with_tp += w["tp"] > 0
        with_fp += w["fp"] > 0
        with_fn += w["fn"] > 0
    assert n >= 60 and with_tp >= 40 and with_fp >= 5 and with_fn >= 5, (n, with_tp, with_fp, with_fn)      # the cases are not trivial


def test_identical_and_disjoint_volumes():
    y = O.random_labels((12, 12, 12), 9, fill=0.6, seed=3)
    n = len(np.unique(y[y > 0]))
    assert n >= 5
    for thr in THRESHOLDS:
        s = _stats(y, y, thr)
        assert s["tp"] == n and s["fp"] == 0 and s["fn"] == 0 and s["f1"] == 1 and s["precision"] == 1 and s["recall"] == 1
        assert s["mean_matched_score"] == 1.0 and s["mean_true_score"] == 1.0 and s["panoptic_quality"] == 1.0
        O.assert_same_stats(s, O.matching_ref(y, y, thr))
    a, b = np.zeros((8, 8), np.int32), np.zeros((8, 8), np.int32)
    a[:4, :4], a[:4, 4:], b[4:, :4], b[4:, 4:] = 1, 2, 1, 5
    for thr in THRESHOLDS:
        s = _stats(a, b, thr)
        assert s["tp"] == 0 and s["fp"] == 2 and s["fn"] == 2 and s["f1"] == 0 and s["panoptic_quality"] == 0.0
        O.assert_same_stats(s, O.matching_ref(a, b, thr))


def test_a_true_object_split_in_two_predictions():
    """20 voxels of truth; prediction 1 covers 10 of them (IoU 10 / 20 = 0.5), prediction 2 covers 8 (IoU 8 / 20 = 0.4): one of them matches."""
    y_true, y_pred = np.zeros(40, np.int32), np.zeros(40, np.int32)
    y_true[:20] = 1
    y_pred[:10], y_pred[10:18] = 1, 2
    pairs, counts = O.overlap_ref(y_true, y_pred)
    assert pairs.tolist() == [[0, 0], [1, 0], [1, 1], [1, 2]] and counts.tolist() == [20, 2, 10, 8]
    for thr, score in ((0.3, 0.5), (0.5, 0.5)):
        s = _stats(y_true, y_pred, thr)
        assert (s["tp"], s["fp"], s["fn"], s["n_true"], s["n_pred"]) == (1, 1, 0, 1, 2)
        assert s["mean_matched_score"] == score                                         # the better of the two is taken
        O.assert_same_stats(s, O.matching_ref(y_true, y_pred, thr))
    assert _stats(y_true, y_pred, 0.75)["tp"] == 0


def test_empty_prediction_empty_truth_and_non_sequential_ids():
    from biapy_amd import prepost

    y = O.random_labels((10, 10, 10), 6, fill=0.6, seed=8)
    zero = np.zeros_like(y)
    n = len(np.unique(y[y > 0]))
    for thr in (0.3, 0.5):
        s = _stats(y, zero, thr)
        assert (s["tp"], s["fp"], s["fn"], s["n_true"], s["n_pred"]) == (0, 0, n, n, 0)
        assert s["precision"] == 0 and s["recall"] == 0 and s["accuracy"] == 0 and s["f1"] == 0 and s["panoptic_quality"] == 0.0
        O.assert_same_stats(s, O.matching_ref(y, zero, thr))
        s = _stats(zero, y, thr)
        assert (s["tp"], s["fp"], s["fn"], s["n_true"], s["n_pred"]) == (0, n, 0, 0, n)
        O.assert_same_stats(s, O.matching_ref(zero, y, thr))
        O.assert_same_stats(_stats(zero, zero, thr), O.matching_ref(zero, zero, thr))
    a, b = np.zeros(60, np.int32), np.zeros(60, np.int32)
    a[:10], a[20:30], a[40:50] = 7, 1000, 2 ** 30
    b[:10], b[22:32], b[45:60] = 2 ** 30, 7, 1000                                         # IoU 1, 8 / 12, 5 / 20
    s = _stats(a, b, 0.5)
    assert (s["tp"], s["fp"], s["fn"], s["n_true"], s["n_pred"]) == (2, 1, 1, 3, 3)
    assert abs(s["mean_matched_score"] - (1 + 8 / 12) / 2) < 1e-15
    O.assert_same_stats(s, O.matching_ref(a, b, 0.5))
    assert _stats(a, b, 0.2)["tp"] == 3
    s = _stats(-a, b, 0.5)                                                                # negative labels are background
    assert (s["n_true"], s["tp"], s["fp"]) == (0, 0, 3)
    pairs, counts = O.overlap_ref(a, b)                                                   # the table may come as lists
    assert prepost._match_stats(pairs.tolist(), counts.tolist(), 0.5) == _stats(a, b, 0.5)

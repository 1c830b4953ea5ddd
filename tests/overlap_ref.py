"""Host references for the label-overlap table and the instance matcher (biapy_amd/prepost.py: label_overlap, matching): the statement the device
results are compared with, written as directly as NumPy allows.

* ``overlap_ref(a, b)``: labels clamped to >= 0, ``np.unique`` with counts on the packed int64 keys ``a << 32 | b``.
* ``matching_ref(y_true, y_pred, thresh)``: the reference's algorithm (biapy/utils/matching.py, the StarDist matcher) restated: labels made
  sequential, a DENSE overlap matrix from ``np.add.at``, dense IoU, ONE ``linear_sum_assignment`` over everything.
* ``random_labels(shape, n_labels, fill, seed)``: blob-like label images - nearest-seed regions of random points, masked by random balls.
"""
import numpy as np


def overlap_ref(a, b):
    """(pairs (K, 2) int32 sorted by (a, b), counts (K,) int32) of two label arrays of the same shape."""
    a64 = np.maximum(np.asarray(a).astype(np.int64).ravel(), 0)
    b64 = np.maximum(np.asarray(b).astype(np.int64).ravel(), 0)
    keys, counts = np.unique((a64 << 32) | b64, return_counts=True)
    pairs = np.stack((keys >> 32, keys & 0xFFFFFFFF), axis=1).astype(np.int32)
    return pairs, counts.astype(np.int32)


def _safe_divide(x, y, eps=1e-10):
    return x / y if abs(y) > eps else 0.0


def matching_ref(y_true, y_pred, thresh):
    """One dict (scalar ``thresh``) or a list of dicts with the reference's keys."""
    from scipy.optimize import linear_sum_assignment

    t = np.maximum(np.asarray(y_true).astype(np.int64).ravel(), 0)
    p = np.maximum(np.asarray(y_pred).astype(np.int64).ravel(), 0)
    ut, it = np.unique(np.concatenate(([0], t)), return_inverse=True)        # sequential labels, 0 stays 0
    up, ip = np.unique(np.concatenate(([0], p)), return_inverse=True)
    overlap = np.zeros((ut.size, up.size), np.int64)
    np.add.at(overlap, (it[1:], ip[1:]), 1)
    n_pixels_pred = overlap.sum(axis=0, keepdims=True)
    n_pixels_true = overlap.sum(axis=1, keepdims=True)
    union = n_pixels_pred + n_pixels_true - overlap
    scores = np.where(union > 0, overlap.astype(np.float64) / np.maximum(union, 1).astype(np.float64), 0.0)[1:, 1:]
    n_true, n_pred = scores.shape
    n_matched = min(n_true, n_pred)

    def one(thr):
        not_trivial = n_matched > 0 and bool(np.any(scores >= thr))
        tp, sum_matched = 0, 0.0
        if not_trivial:
            costs = -(scores >= thr).astype(float) - scores / (2 * n_matched)
            ti, pi = linear_sum_assignment(costs)
            ok = scores[ti, pi] >= thr
            tp = int(np.count_nonzero(ok))
            sum_matched = float(np.sum(scores[ti, pi][ok]))
        fp, fn = n_pred - tp, n_true - tp
        return dict(criterion="iou", thresh=thr, fp=fp, tp=tp, fn=fn,
                    precision=tp / (tp + fp) if tp > 0 else 0, recall=tp / (tp + fn) if tp > 0 else 0,
                    accuracy=tp / (tp + fp + fn) if tp > 0 else 0, f1=(2 * tp) / (2 * tp + fp + fn) if tp > 0 else 0,
                    n_true=n_true, n_pred=n_pred, mean_true_score=_safe_divide(sum_matched, n_true),
                    mean_matched_score=_safe_divide(sum_matched, tp), panoptic_quality=_safe_divide(sum_matched, tp + fp / 2 + fn / 2))

    return one(thresh) if np.isscalar(thresh) else [one(thr) for thr in thresh]


INT_KEYS = ("tp", "fp", "fn", "n_true", "n_pred", "precision", "recall", "accuracy", "f1")      # integers and ratios of integers: exact
SCORE_KEYS = ("mean_true_score", "mean_matched_score", "panoptic_quality")                      # float64 sums in another order: 1e-9 absolute


def assert_same_stats(got, want, what=""):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    assert got["criterion"] == want["criterion"] == "iou" and got["thresh"] == want["thresh"], what
    for k in INT_KEYS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in SCORE_KEYS:
        assert abs(got[k] - want[k]) <= 1e-9, (what, k, got[k], want[k])


def random_labels(shape, n_labels, fill=0.5, seed=0):
    """int32 labels of ``shape``: every voxel belongs to the nearest of ``n_labels`` random seed points (labels 1..n_labels, as far as a label
    wins any voxel) and is kept where one of a set of random balls covers it - about ``fill`` of the volume - else background 0."""
    rng = np.random.default_rng(seed)
    shape = tuple(int(s) for s in shape)
    out = np.zeros(shape, np.int32)
    if n_labels < 1:
        return out
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).reshape(-1, len(shape)).astype(np.float64)
    pts = rng.random((n_labels, len(shape))) * np.array(shape)
    from scipy.spatial import cKDTree

    lab = (cKDTree(pts).query(grid)[1] + 1).astype(np.int32)               # no (voxels x labels) matrix
    keep = np.zeros(grid.shape[0], bool)
    rmax = max(2.0, 0.35 * max(shape))
    for _ in range(64):                                                     # balls until the fill is reached, 64 at the most
        if keep.mean() >= fill:
            break
        c, r = rng.random(len(shape)) * np.array(shape), rng.uniform(1.0, rmax)
        keep |= ((grid - c) ** 2).sum(axis=1) <= r * r
    out.reshape(-1)[:] = np.where(keep, lab, 0)
    return out

"""Label overlap and instance matching on the MI355X (biapy_amd/prepost.py: label_overlap, matching; csrc/overlap.hip) against their statements
(tests/overlap_ref.py): ``pairs[:num]`` / ``counts[:num]`` bit for bit ``np.unique`` of the packed keys with its counts, ``num`` the number of
distinct pairs, the rows past it (-1, -1) and 0; ``matching`` the dense reference's statistics - integers and their ratios exactly, the three
score means within 1e-9 absolute (float64 sums of a few hundred terms in another order).  Volumes and references are built once per process."""
import numpy as np
import pytest
import torch

import overlap_ref as O
import watershed_ref as W

pytestmark = pytest.mark.gpu

SPAN = 8192                                 # OVL_SPAN of csrc/overlap_core.h: the voxels a wave owns


def _P():
    from biapy_amd import prepost

    return prepost


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(pairs, counts, num, a_np, b_np, max_pairs):
    """The device table == np.unique's, the filler past num, the types.  Returns K."""
    want_pairs, want_counts = O.overlap_ref(a_np, b_np)
    k = want_pairs.shape[0]
    assert num.dtype == torch.int32 and num.dim() == 0 and num.is_cuda                     # the count stays on the device
    assert pairs.dtype == torch.int32 and tuple(pairs.shape) == (max_pairs, 2) and pairs.is_cuda
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (max_pairs,) and counts.is_cuda
    assert int(num) == k
    p, c = pairs.cpu().numpy(), counts.cpu().numpy()
    np.testing.assert_array_equal(p[:k], want_pairs)
    np.testing.assert_array_equal(c[:k], want_counts)
    assert (p[k:] == -1).all() and (c[k:] == 0).all()
    assert int(c.sum()) == a_np.size
    return k


def _run(a_np, b_np, max_pairs=None):
    mp = min(a_np.size, 2 ** 21) if max_pairs is None else max_pairs
    return _check(*_P().label_overlap(_dev(a_np), _dev(b_np), max_pairs), a_np, b_np, mp)


def _labels(shape, n_labels, seed):
    """Labels in runs along the last axis (piecewise constant, as label volumes are), ids 1..n_labels, about 40 % background, some negative."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    starts = rng.random(n) < 0.15
    starts[0] = True
    ids = np.where(rng.random(n) < 0.4, np.where(rng.random(n) < 0.2, -2, 0), rng.integers(1, max(n_labels, 1) + 1, size=n) if n_labels else 0)
    return ids[np.maximum.accumulate(np.where(starts, np.arange(n), 0))].astype(np.int32).reshape(shape)


SHAPES = [(9, 21, 37), (8, 16, 64), (1, 33, 70), (33, 70), (5, 1, 1), (1, 1, 300), (7,), (SPAN - 1,), (SPAN,), (SPAN + 1,)]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_random_labels_bit_for_bit(shape):
    """Shapes unaligned everywhere, aligned, of every rank from 1 to 3, with axes of one voxel, and flat lengths one below, at and one above
    the span of a wave; crossed with 0, 1, 7 and 1000 labels on either side."""
    pairs_seen = 0
    for na in (0, 1, 7, 1000):
        for nb in (0, 1, 7, 1000):
            pairs_seen += _run(_labels(shape, na, 11 * na + 1), _labels(shape, nb, 13 * nb + 2))
    assert pairs_seen >= 16 + (20 if np.prod(shape) > 100 else 0)


def test_all_background_and_one_uniform_pair():
    for shape in ((9, 21, 37), (3 * SPAN + 5,), (1,)):
        zero = np.zeros(shape, np.int32)
        assert _run(zero, zero) == 1
        assert _run(zero, zero, max_pairs=1) == 1
        assert _run(np.full(shape, 5, np.int32), np.full(shape, 9, np.int32), max_pairs=1) == 1
        p, c, _ = _P().label_overlap(_dev(np.full(shape, 5, np.int32)), _dev(np.full(shape, 9, np.int32)), 3)
        assert p.tolist() == [[5, 9], [-1, -1], [-1, -1]] and c.tolist() == [int(np.prod(shape)), 0, 0]


def test_negative_labels_are_background_on_both_sides():
    a, b = _labels((9, 21, 37), 7, 3), _labels((9, 21, 37), 7, 4)
    a[a == 0], b[b == 3] = -5, np.iinfo(np.int32).min
    assert (a < 0).any() and (b < 0).any()
    k = _run(a, b)
    p, _, _ = _P().label_overlap(_dev(a), _dev(b))
    assert (p[:k] >= 0).all() and 3 not in p[:k, 1].tolist()
    assert _run(np.full(300, -1, np.int32), np.full(300, -7, np.int32), 2) == 1             # everything is (0, 0)
    big = np.iinfo(np.int32).max
    assert _run(np.array([big, big, 1, big], np.int32), np.array([big, 1, big, big], np.int32)) == 3      # the largest key stays below the filler


def test_all_distinct_pairs():
    n = 8192
    a, b = 1 + np.arange(n, dtype=np.int32), 1 + np.arange(n, dtype=np.int32)[::-1].copy()
    assert _run(a, b, max_pairs=n) == n
    _, c, _ = _P().label_overlap(_dev(a), _dev(b), n)
    assert (c == 1).all()
    assert _run(a[:100], b[:100], max_pairs=100) == 100                                     # max_pairs exactly K: a table of 256 slots, long probe chains
    assert _run(a[:100], b[:100], max_pairs=101) == 100


def test_overflow_reports_minus_one_and_leaves_the_next_call_alone():
    P = _P()
    a, b = 1 + np.arange(100, dtype=np.int32), np.arange(100, dtype=np.int32)[::-1].copy()
    da, db = _dev(a), _dev(b)
    pairs, counts, num = P.label_overlap(da, db, max_pairs=16)
    assert int(num) == -1 and tuple(pairs.shape) == (16, 2) and tuple(counts.shape) == (16,)
    assert _check(*P.label_overlap(da, db, max_pairs=100), a, b, 100) == 100               # the same stream, right after
    assert int(P.label_overlap(da, db, max_pairs=99)[2]) == -1                              # one pair too many
    big_a = _labels((40000,), 1000, 5)
    assert int(P.label_overlap(_dev(big_a), _dev(_labels((40000,), 1000, 6)), max_pairs=5)[2]) == -1      # a table that fills up completely
    assert _run(big_a, big_a) > 100
    with pytest.raises(RuntimeError, match="max_pairs"):
        P.matching(da, db, max_pairs=16)
    assert P.matching(da, db, max_pairs=100)["n_true"] == 100


def test_unaligned_and_non_contiguous_views():
    P = _P()
    a, b = _labels((9, 21, 37), 7, 21), _labels((9, 21, 37), 1000, 22)
    n = a.size
    want = O.overlap_ref(a, b)
    for off_a, off_b in ((1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 3), (2, 2)):       # 4, 8, 12 bytes past a 16-byte boundary, either input
        ba, bb = torch.zeros(n + 8, dtype=torch.int32, device="cuda"), torch.zeros(n + 8, dtype=torch.int32, device="cuda")
        va, vb = ba[off_a:off_a + n], bb[off_b:off_b + n]
        va.copy_(_dev(a).view(-1))
        vb.copy_(_dev(b).view(-1))
        assert va.data_ptr() % 16 == 4 * off_a and vb.data_ptr() % 16 == 4 * off_b and va.is_contiguous()
        _check(*P.label_overlap(va, vb), a.ravel(), b.ravel(), n)

    def perm(x):
        return _dev(x.transpose(1, 0, 2)).permute(1, 0, 2)

    def tall(x):
        t = torch.zeros((18,) + x.shape[1:], dtype=torch.int32, device="cuda")
        t[::2] = _dev(x)
        return t[::2]

    for va, vb in ((perm(a), perm(b)), (tall(a), tall(b)), (tall(a), perm(b)), (_dev(a), tall(b))):
        assert not (va.is_contiguous() and vb.is_contiguous())
        pairs, counts, num = P.label_overlap(va, vb)
        k = int(num)
        assert np.array_equal(pairs[:k].cpu().numpy(), want[0]) and np.array_equal(counts[:k].cpu().numpy(), want[1])


def test_two_calls_give_the_same_bits():
    P = _P()
    for shape, na, nb, mp in (((9, 21, 37), 7, 1000, None), ((SPAN + 1,), 1000, 1000, None), ((8, 16, 64), 1000, 7, 16)):
        a, b = _dev(_labels(shape, na, 31)), _dev(_labels(shape, nb, 32))
        first, second = P.label_overlap(a, b, mp), P.label_overlap(a, b, mp)
        assert torch.equal(first[2], second[2])
        if int(first[2]) >= 0:                                                              # on overflow the table is unspecified
            assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


_BLOBS = {}


def _blobs(shape, n_true, n_pred):
    """A ground truth and a prediction of it: the same blobs shifted by a voxel with a tenth of the voxels dropped, plus unrelated ones."""
    key = (shape, n_true, n_pred)
    if key not in _BLOBS:
        y_true = O.random_labels(shape, n_true, fill=0.5, seed=41)
        y_pred = np.roll(y_true, 1, axis=-1).copy()
        rng = np.random.default_rng(42)
        y_pred[rng.random(shape) < 0.1] = 0
        extra = O.random_labels(shape, n_pred, fill=0.2, seed=43)
        y_pred = np.where((y_pred == 0) & (extra > 0), extra + n_true, y_pred).astype(np.int32)
        _BLOBS[key] = (y_true, y_pred)
    return _BLOBS[key]


def test_64_cubed_against_the_reference():
    y_true, y_pred = _blobs((64, 64, 64), 300, 100)
    assert _run(y_true, y_pred) > 400


def test_matching_against_the_dense_reference():
    P = _P()
    y_true, y_pred = _blobs((24, 48, 64), 60, 30)
    thresholds = (0.3, 0.5, 0.75)
    got = P.matching(_dev(y_true), _dev(y_pred), thresh=thresholds)
    want = O.matching_ref(y_true, y_pred, thresholds)
    assert isinstance(got, list) and len(got) == 3
    for g, w in zip(got, want):
        O.assert_same_stats(g, w)
    assert want[0]["tp"] > 20 and want[0]["fp"] > 0 and want[2]["fn"] > 0
    one = P.matching(_dev(y_true), _dev(y_pred))                                            # one threshold, the default 0.5: one dict
    assert isinstance(one, dict)
    O.assert_same_stats(one, want[1])
    same = P.matching(_dev(y_true), _dev(y_true), thresh=0.9)
    assert same["f1"] == 1 and same["tp"] == same["n_true"] == len(np.unique(y_true[y_true > 0]))
    none = P.matching(_dev(y_true), torch.zeros_like(_dev(y_true)), thresh=0.5)
    assert none["tp"] == 0 and none["n_pred"] == 0 and none["fn"] == none["n_true"] and none["f1"] == 0


def test_binarize_to_watershed_to_matching_end_to_end():
    """The instance pipeline, scored on the device: a prediction of overlapping balls -> binarize -> distance -> label -> watershed, matched
    against the connected components of the ground-truth mask."""
    P = _P()
    shape = (24, 48, 64)
    rng = np.random.default_rng(3)
    blobs = W.balls(shape, fill=0.3, seed=3, rmin=3, rmax=6)
    pred = (0.2 * rng.random(shape) + 0.7 * blobs).astype(np.float32)
    mask = P.binarize(_dev(pred))
    d2 = P.distance_transform_edt(mask, squared=True)
    seeds = P.label((d2 > 6).to(torch.uint8), connectivity=1)
    instances = P.watershed(-d2, seeds, mask, connectivity=1)
    truth = P.label(_dev((blobs > 0).astype(np.uint8)), connectivity=1)
    thresholds = (0.3, 0.5, 0.75)
    got = P.matching(truth, instances, thresh=thresholds)
    want = O.matching_ref(truth.cpu().numpy(), instances.cpu().numpy(), thresholds)
    for g, w in zip(got, want):
        O.assert_same_stats(g, w)
        assert g["n_true"] >= 1 and g["n_pred"] > 5
    assert 0 < got[0]["f1"] <= 1


def test_graph_capture_of_label_overlap():
    """Captured once, replayed after both label volumes were overwritten in place: every replay gives the table of the inputs of that moment,
    -1 for the one that overflows."""
    P = _P()
    shape, mp = (12, 40, 56), 3000
    inputs = [(_labels(shape, 7, 51), _labels(shape, 7, 52)), (_labels(shape, 1000, 53), _labels(shape, 7, 54)),
              (np.zeros(shape, np.int32), np.zeros(shape, np.int32)), (_labels(shape, 1000, 55), _labels(shape, 1000, 56)),
              (_labels(shape, 7, 51), _labels(shape, 7, 52))]
    ks = [O.overlap_ref(a, b)[0].shape[0] for a, b in inputs]
    assert ks[2] == 1 and ks[3] > mp and max(ks[0], ks[1]) <= mp                            # all background; one that overflows
    a, b = _dev(inputs[0][0]), _dev(inputs[0][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        P.label_overlap(a, b, mp)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pairs, counts, num = P.label_overlap(a, b, mp)
    for (a_np, b_np), k in zip(inputs, ks):
        a.copy_(_dev(a_np))
        b.copy_(_dev(b_np))
        g.replay()
        if k > mp:
            assert int(num) == -1
        else:
            _check(pairs, counts, num, a_np, b_np, mp)


def test_refusals_on_device_tensors():
    P = _P()
    a = torch.zeros(4, 5, 6, dtype=torch.int32, device="cuda")
    for fn in (P.label_overlap, P.matching):
        with pytest.raises(NotImplementedError, match="int32 labels"):
            fn(a.long(), a)
        with pytest.raises(NotImplementedError, match="int32 labels"):
            fn(a, a.float())
        with pytest.raises(NotImplementedError, match="empty"):
            fn(a[:0], a[:0])
        with pytest.raises(NotImplementedError, match="2\\^31 slots"):
            fn(a, a, max_pairs=2 ** 30 + 1)
        with pytest.raises(ValueError, match="same shape"):
            fn(a, a[:, :, :5])
        with pytest.raises(ValueError, match="max_pairs must be at least 1"):
            fn(a, a, max_pairs=0)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(a, a.cpu())
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(a.cpu(), a)
    with pytest.raises(NotImplementedError, match="criterion"):
        P.matching(a, a, criterion="iot")
    big = torch.empty(2 ** 31, dtype=torch.int32, device="cuda")                           # both inputs at once: nothing is launched
    with pytest.raises(NotImplementedError, match="2\\^31"):
        P.label_overlap(big, big)

"""Seeded watershed on the MI355X (biapy_amd/prepost.py: watershed; csrc/watershed.hip) against its statement, Kruskal over the strictly ordered
edges (tests/watershed_ref.py): every comparison is bit for bit on the int32 labels - no permutation matching, no tolerance - and every call's
round count is held against R = ceil(log2(max(n, 2))) + 1 computed here from n.  Volumes and references are built once per process."""
import numpy as np
import pytest
import torch

import watershed_ref as W

pytestmark = pytest.mark.gpu


def _P():
    from biapy_amd import prepost

    return prepost


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(image, markers, mask, c, want=None):
    """watershed() on the device == the twin; rounds <= R.  Returns (labels as NumPy, rounds)."""
    out, rounds = _P().watershed(_dev(image), _dev(markers), _dev(mask), connectivity=c, return_rounds=True)
    assert out.dtype == torch.int32 and out.shape == tuple(image.shape) and out.is_cuda and out.is_contiguous()
    assert rounds.dtype == torch.int32 and rounds.dim() == 0 and rounds.is_cuda          # the count stays on the device
    assert 0 <= int(rounds) <= W.rounds_bound(image.size)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got, W.reference(image, markers, mask, c) if want is None else want)
    return got, int(rounds)


LEVELS, DTYPES, KEEPS, SEEDS = (1, 2, 4, 1000), (np.int32, np.float32), (0.6, 0.9, 1.0), (0.01, 0.1)


@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("shape", [(9, 21, 37), (8, 16, 64), (1, 33, 70), (33, 70), (5, 1, 1), (1, 1, 300), (3, 1, 40)], ids=str)
def test_random_volumes_bit_for_bit(shape, c):
    """Shapes unaligned everywhere, aligned, 2-D in both spellings and with axes of one voxel; per shape and connectivity every image level with
    both dtypes, the masks (60 %, 90 %, none) and the marker densities (1 %, 10 %, labels repeated) cycling so that each meets each."""
    if c > len(shape):
        with pytest.raises(ValueError, match="connectivity"):
            _P().watershed(torch.zeros(shape, device="cuda"), torch.zeros(shape, dtype=torch.int32, device="cuda"), connectivity=c)
        return
    labelled = 0
    for k, (levels, dtype) in enumerate((l, d) for l in LEVELS for d in DTYPES):
        keep, seeds = KEEPS[(k + c) % 3], SEEDS[(k // 2 + k // 3 + c) % 2]
        image, markers, mask = W.random_case(shape, levels, dtype, keep, seeds)
        got, _ = _run(image, markers, mask, c)
        labelled += int((got > 0).sum())
    if min(shape) > 1:
        assert labelled > 0


def test_no_marker_one_marker_every_voxel_a_marker():
    image, markers, mask = W.random_case((9, 21, 37), 4, np.float32, 0.9, 0.1)
    zero = np.zeros_like(markers)
    got, rounds = _run(image, zero, mask, 1)
    assert not got.any() and rounds == 0                                              # no marker at all: nothing to do
    got, rounds = _run(image, np.minimum(markers, 0), mask, 1)                        # only negative markers: the same
    assert not got.any() and rounds == 0
    one = zero.copy()
    one[4, 10, 20] = 7
    m1 = mask.copy()
    m1[4, 10, 20] = 1
    got, rounds = _run(image, one, m1, 3)
    assert set(np.unique(got).tolist()) == {0, 7} and rounds >= 1
    got, rounds = _run(np.zeros((6, 7, 8), np.int32), np.pad(np.full((1, 1, 1), 5, np.int32), ((2, 3), (3, 3), (4, 3))), None, 1)
    assert (got == 5).all()                                                           # a connected volume, one marker: everything is its basin
    every = (1 + np.arange(markers.size, dtype=np.int32).reshape(markers.shape) % 11)
    got, rounds = _run(image, every, mask, 2)
    assert np.array_equal(got, np.where(mask != 0, every, 0)) and rounds == 0         # a copy of the markers under the mask


def test_markers_outside_the_mask_negative_markers_and_unreached_regions():
    image = np.zeros((3, 9, 20), np.float32)
    mask = np.ones((3, 9, 20), np.uint8)
    mask[:, :, 10] = 0                                                                # a wall: x > 10 holds no seed inside the mask
    markers = np.zeros((3, 9, 20), np.int32)
    markers[1, 4, 2], markers[1, 4, 10], markers[0, 0, 15], markers[2, 8, 19] = 3, 8, -5, np.iinfo(np.int32).min
    got, rounds = _run(image, markers, mask, 3)
    assert (got[:, :, :10] == 3).all() and not got[:, :, 10:].any() and rounds >= 1
    assert 8 not in got


@pytest.mark.parametrize("dtype", DTYPES, ids=["int32", "float32"])
def test_long_paths_stay_inside_the_round_bound(dtype):
    """A one-voxel-wide boustrophedon path of 3170 voxels: one seed at its end (a flat image: every voxel's first edge is the one behind it), then
    a seed at each end and weights that strictly rise to the middle and strictly fall after it (the path splits at the peak)."""
    mask, order = W.snake_path(41, 150)
    markers = np.zeros(mask.shape, np.int32)
    markers[order[-1]] = 4
    image = np.zeros(mask.shape, dtype)
    got, rounds = _run(image, markers, mask, 1)
    assert np.array_equal(got, 4 * mask.astype(np.int32)) and 1 <= rounds <= W.rounds_bound(mask.size)
    n = len(order)
    image, markers = image.copy(), markers.copy()                                     # new arrays: the reference is cached per array
    for q, p in enumerate(order):
        image[p] = q if q < n // 2 else n - 1 - q
    markers[order[0]] = 9
    got, rounds = _run(image, markers, mask, 1)
    along = np.array([got[p] for p in order])
    assert set(along[:n // 2 - 1].tolist()) == {9} and set(along[n // 2 + 1:].tolist()) == {4} and rounds <= W.rounds_bound(mask.size)


def test_ridge_with_one_lower_pass_voxel():
    image = np.zeros((11, 15), np.int32)
    image[:, 7] = 10                                                                  # the ridge
    image[8, 7] = 5                                                                   # its one lower voxel
    markers = np.zeros((11, 15), np.int32)
    markers[2, 1], markers[3, 13] = 1, 2
    for c in (1, 2):
        got, _ = _run(image, markers, None, c)
        assert (got[:, :7] == 1).all() and (got[:, 8:] == 2).all() and (got[:, 7] > 0).all()
        assert W.check_pass_heights(image, markers, None, c, got) == image.size


def test_plateau_goes_to_the_raster_first_edge_and_the_recipe_splits_it():
    markers = np.zeros((1, 21), np.int32)
    markers[0, 0], markers[0, 20] = 1, 2
    flat = np.zeros((1, 21), np.int32)
    got, _ = _run(flat, markers, None, 1)
    assert got[0].tolist() == [1] * 20 + [2]
    got, _ = _run(W.plateau_recipe(flat, markers), markers, None, 1)
    assert got[0].tolist() == [1] * 11 + [2] * 10                                     # the midpoint
    # the same on the device alone: the squared distance to the nearest marker from distance_transform_edt
    P = _P()
    mk = _dev(markers)
    d2 = P.distance_transform_edt((mk <= 0).to(torch.uint8), squared=True)
    image = (torch.zeros_like(mk) << 15) | torch.clamp(d2, max=32767)
    assert P.watershed(image, mk).cpu().numpy()[0].tolist() == [1] * 11 + [2] * 10


def test_float_images_with_signed_zeros_infinities_and_denormals():
    vals = np.array([-0.0, 0.0, -np.inf, np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 1.0, -1.0, 0.0, -0.0], np.float32)
    rng = np.random.default_rng(11)
    image = vals[rng.integers(0, vals.size, size=(5, 12, 19))]
    assert np.signbit(image[image == 0]).any() and not np.signbit(image[image == 0]).all()
    markers = np.where(rng.random(image.shape) < 0.03, rng.integers(1, 4, size=image.shape), 0).astype(np.int32)
    mask = (rng.random(image.shape) < 0.9).astype(np.uint8)
    for c in (1, 3):
        got, _ = _run(image, markers, mask, c)
        assert W.check_pass_heights(image, markers, mask, c, got) > 500
    line = np.array([[0.0, 0.0, 0.0, -0.0, -0.0, 0.0, 0.0]], np.float32)              # -0.0 < +0.0: the one edge between the two -0.0 is the cheapest
    mk = np.array([[1, 0, 0, 0, 0, 0, 2]], np.int32)
    got, _ = _run(line, mk, None, 1)
    assert got[0, 3] == got[0, 4]


def test_64_cubed_against_the_twin():
    image, markers, mask = W.random_case((64, 64, 64), 1000, np.float32, 0.9, 0.01)
    got, rounds = _run(image, markers, mask, 1)
    assert (got > 0).mean() > 0.5 and rounds >= 2


def test_two_calls_give_the_same_bits():
    P = _P()
    for (shape, levels, dtype, keep, seeds), c in ((((9, 21, 37), 1, np.int32, 0.9, 0.01), 3), (((8, 16, 64), 2, np.float32, 0.6, 0.1), 1),
                                                   (((33, 70), 4, np.int32, 1.0, 0.01), 2)):
        image, markers, mask = (_dev(a) for a in W.random_case(shape, levels, dtype, keep, seeds))
        a, ra = P.watershed(image, markers, mask, c, return_rounds=True)
        b, rb = P.watershed(image, markers, mask, c, return_rounds=True)
        assert torch.equal(a, b) and torch.equal(ra, rb) and 1 <= int(ra) <= W.rounds_bound(image.numel())


def test_views_and_bool_masks_agree():
    P = _P()
    image, markers, mask = W.random_case((9, 21, 37), 4, np.float32, 0.6, 0.1)
    want = W.reference(image, markers, mask, 1)
    assert np.array_equal(P.watershed(_dev(image), _dev(markers), _dev(mask.astype(bool)), 1).cpu().numpy(), want)
    assert torch.is_tensor(P.watershed(_dev(image), _dev(markers)))                    # return_rounds defaults to False, the mask to None
    # non-contiguous views: the (Y, Z, X) permutation of a contiguous tensor, and every second plane of a taller one
    def perm(a):
        return _dev(a.transpose(1, 0, 2)).permute(1, 0, 2)

    def tall(a, dt=None):
        t = torch.zeros((18,) + a.shape[1:], dtype=_dev(a).dtype, device="cuda")
        t[::2] = _dev(a)
        return (t if dt is None else t.to(dt))[::2]

    for views in ((perm(image), perm(markers), perm(mask)), (tall(image), tall(markers), tall(mask)), (tall(image), perm(markers), tall(mask, torch.bool))):
        assert not any(v.is_contiguous() for v in views)
        out = P.watershed(*views, connectivity=1)
        assert out.is_contiguous() and np.array_equal(out.cpu().numpy(), want)


def _instance_inputs(shape, seed):
    """A bimodal prediction of overlapping balls: floor near 0.1, blobs near 0.8."""
    rng = np.random.default_rng(seed)
    blobs = W.balls(shape, fill=0.3, seed=seed, rmin=3, rmax=6)
    return (0.2 * rng.random(shape) + 0.7 * blobs).astype(np.float32)


def _instances(P, mask, core_d2):
    """mask -> (squared distance, seeds = the labelled eroded core, instances): the documented call sequence, device tensors throughout."""
    d2 = P.distance_transform_edt(mask, squared=True)
    seeds = P.label((d2 > core_d2).to(torch.uint8), connectivity=1)
    return d2, seeds, P.watershed(-d2, seeds, mask, connectivity=1, return_rounds=True)


def test_binarize_label_distance_watershed_end_to_end():
    P = _P()
    mask = P.binarize(_dev(_instance_inputs((24, 48, 64), 3)))
    d2, seeds, (out, rounds) = _instances(P, mask, 6)
    m, d, s, got = (t.cpu().numpy() for t in (mask, d2, seeds, out))
    assert 0.15 < m.mean() < 0.5 and s.max() > 5 and (m != 0)[s == 0].any()
    assert int(rounds) <= W.rounds_bound(m.size)
    np.testing.assert_array_equal(got, W.watershed_ref(-d, s, m, 1))
    assert np.array_equal(got[s > 0], s[s > 0])                                        # every region holds exactly the seed voxels of its own label
    assert set(np.unique(got).tolist()) <= set(np.unique(s).tolist())                 # and no region is without one
    assert not got[m == 0].any()
    assert (got[m != 0] > 0).mean() > 0.9                                              # the cores reach nearly all of the foreground


def test_graph_capture_of_label_distance_and_watershed():
    """Captured once, replayed after the mask was overwritten in place: the instances are the twin's for the NEW mask."""
    P = _P()
    shape = (12, 40, 56)
    masks = [(_instance_inputs(shape, s) > 0.5).astype(np.uint8) for s in (5, 6)] + [np.zeros(shape, np.uint8)]
    m = _dev(masks[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _instances(P, m, 6)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d2, seeds, (out, rounds) = _instances(P, m, 6)
    for mask in (masks[0], masks[1], masks[2], masks[0]):
        m.copy_(_dev(mask))
        g.replay()
        d, s, got = (t.cpu().numpy() for t in (d2, seeds, out))
        assert int(rounds) <= W.rounds_bound(mask.size) and (int(rounds) == 0) == (not s.any())
        np.testing.assert_array_equal(got, W.watershed_ref(-d, s, mask, 1))
        assert np.array_equal(got[s > 0], s[s > 0])


def test_refusals_on_device_tensors():
    P = _P()
    img = torch.zeros(4, 5, 6, device="cuda")
    mk = torch.zeros(4, 5, 6, dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError, match="float32 or int32 images"):
        P.watershed(img.double(), mk)
    with pytest.raises(NotImplementedError, match="int32 markers"):
        P.watershed(img, mk.long())
    with pytest.raises(NotImplementedError, match="uint8 or bool masks"):
        P.watershed(img, mk, mk)
    with pytest.raises(ValueError, match="2-D .* or 3-D"):
        P.watershed(img[None], mk[None])
    with pytest.raises(ValueError, match="same shape"):
        P.watershed(img, mk[:, :, :5])
    with pytest.raises(ValueError, match="connectivity"):
        P.watershed(img, mk, connectivity=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.watershed(img, mk.cpu())
    with pytest.raises(NotImplementedError, match="empty axis"):
        P.watershed(img[:0], mk[:0])
    big = torch.empty(2 ** 31, dtype=torch.int32, device="cuda").view(2048, 1024, 1024)      # image and markers at once: nothing is launched
    with pytest.raises(NotImplementedError, match="2\\^31"):
        P.watershed(big, big)

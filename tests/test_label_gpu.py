"""Connected-component labelling on the MI355X (biapy_amd/prepost.py: label, component_sizes, remove_small_objects; csrc/label.hip) against
``scipy.ndimage.label`` with the matching structure: every comparison is bit for bit on the int32 labels and on N - no permutation matching,
no tolerance.  Masks and references come from tests/label_ref.py, computed once per process."""
import numpy as np
import pytest
import torch

import label_ref as R

pytestmark = pytest.mark.gpu


def _P():
    from biapy_amd import prepost

    return prepost


def _check(mask_np, c, connectivity="same"):
    """label() of the mask on the device == SciPy's labels and count."""
    want, n = R.scipy_label(mask_np, c)
    lab, num = _P().label(torch.from_numpy(np.asarray(mask_np)).cuda(), connectivity=c if connectivity == "same" else connectivity, return_num=True)
    assert lab.dtype == torch.int32 and lab.shape == tuple(mask_np.shape) and lab.is_cuda
    assert num.dtype == torch.int32 and num.dim() == 0 and num.is_cuda                  # the count stays on the device
    assert int(num) == n
    np.testing.assert_array_equal(lab.cpu().numpy(), want)
    return n


def _tiled(on):
    from biapy_amd import _lib as L

    L.lib.bpx_debug_set_label_tiled(1 if on else 0)


@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("shape", [(9, 21, 37), (2, 64, 128), (17, 16, 200), (1, 33, 70), (33, 70), (5, 1, 1), (1, 1, 300)], ids=str)
def test_random_masks_bit_for_bit(shape, c):
    """Densities 0.1 ... 0.9 (0.32: near the 6-neighbour percolation threshold) on shapes unaligned everywhere, aligned, with a partial tile,
    2-D in both spellings and with axes of one voxel."""
    if c > len(shape):
        with pytest.raises(ValueError, match="connectivity"):
            _P().label(torch.zeros(shape, dtype=torch.uint8, device="cuda"), connectivity=c)
        return
    counts = [_check(R.random_masks(shape)[c, p], c) for p in R.DENSITIES]
    if shape == (9, 21, 37) and c in R.REF_COUNTS:
        assert tuple(counts) == R.REF_COUNTS[c]
    if min(shape) > 1:
        assert counts[0] > 1


@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("name", R.STRUCTURED)
def test_structured_masks_bit_for_bit(name, c):
    """20 x 43 x 150 - two full tiles and a partial one on every axis: all zero, all one, the last voxel alone, the checkerboard, the
    boustrophedon path, the interleaved combs, the edge and corner pairs across tile borders."""
    assert _check(R.structured(name), c) == R.STRUCTURED_COUNTS[name][c - 1]


def test_default_connectivity_is_the_full_one():
    m3, m2 = R.random_masks((9, 21, 37))[3, 0.1], R.random_masks((33, 70))[2, 0.25]
    assert _check(m3, 3, connectivity=None) > 1 and _check(m2, 2, connectivity=None) > 1
    lab = _P().label(torch.from_numpy(m3).cuda())                                       # return_num defaults to False: the labels alone
    assert torch.is_tensor(lab) and np.array_equal(lab.cpu().numpy(), R.scipy_label(m3, 3)[0])
    with pytest.raises(ValueError, match="connectivity"):
        _P().label(torch.from_numpy(m3).cuda(), connectivity=0)
    with pytest.raises(ValueError, match="2-D .* or 3-D"):
        _P().label(torch.zeros(2, 3, 4, 5, dtype=torch.uint8, device="cuda"))


def test_many_components_across_many_chunks():
    """64 x 128 x 128 at p = 0.1, connectivity 1: about 7e4 components - roots in every one of the 256 chunks, ranks far past one chunk."""
    n = _check(R.many_components(), 1)
    assert 5e4 < n < 1e5


def test_256_cubed_balls_against_scipy():
    """1.7e7 voxels (past 2^24) of random balls at about 30 % fill, full connectivity."""
    mask = R.balls((256, 256, 256))
    assert 0.2 < mask.mean() < 0.4
    assert _check(mask, 3) > 1


def test_foreground_is_every_nonzero_byte_and_views_and_bool_agree():
    base = R.random_masks((9, 21, 37))[1, 0.32]
    want, n = R.scipy_label(base, 1)
    P = _P()
    vals = np.random.default_rng(1).choice(np.array([1, 2, 255], np.uint8), size=base.shape)
    for m in (torch.from_numpy(base * vals), torch.from_numpy(base.astype(bool))):
        lab, num = P.label(m.cuda(), connectivity=1, return_num=True)
        assert int(num) == n and np.array_equal(lab.cpu().numpy(), want)
    # a non-contiguous view: the mask as the (Y, Z, X) permutation of a contiguous tensor, and every second plane of a taller one
    perm = torch.from_numpy(np.ascontiguousarray(base.transpose(1, 0, 2))).cuda().permute(1, 0, 2)
    tall = torch.zeros(18, 21, 37, dtype=torch.uint8, device="cuda")
    tall[::2] = torch.from_numpy(base).cuda()
    for view in (perm, tall[::2], tall.bool()[::2]):
        assert not view.is_contiguous()
        lab = P.label(view, connectivity=1)
        assert lab.is_contiguous() and np.array_equal(lab.cpu().numpy(), want)


def test_two_calls_give_the_same_bits():
    for mask, c in ((R.random_masks((17, 16, 200))[1, 0.32], 1), (R.structured("snake"), 1), (R.structured("checkerboard"), 3)):
        m = torch.from_numpy(mask).cuda()
        a, na = _P().label(m, c, return_num=True)
        b, nb = _P().label(m, c, return_num=True)
        assert torch.equal(a, b) and torch.equal(na, nb)


@pytest.mark.parametrize("c", [1, 2, 3])
def test_tiled_and_global_merge_bit_for_bit(c):
    """The tiled merge (tiles in LDS, then unions across tile borders) against the global-only merge, on the structured masks and the
    0.32-density ones; both equal SciPy."""
    masks = [R.structured(name) for name in R.STRUCTURED] + [R.random_masks(s)[c, 0.32] for s in ((9, 21, 37), (2, 64, 128), (17, 16, 200))]
    for mask in masks:
        m = torch.from_numpy(mask).cuda()
        out = []
        try:
            for on in (1, 0):
                _tiled(on)
                out.append(_P().label(m, c, return_num=True))
        finally:
            _tiled(1 if DEFAULT_TILED else 0)
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
        want, n = R.scipy_label(mask, c)
        assert int(out[1][1]) == n and np.array_equal(out[1][0].cpu().numpy(), want)


DEFAULT_TILED = False     # the library's default form of the merge (README: which one measured faster); the test above restores it


def test_graph_capture_of_label_and_component_sizes():
    """Captured once, replayed after the mask was overwritten in place: labels, N and sizes are SciPy's for the NEW mask."""
    P = _P()
    first, second = R.random_masks((17, 16, 200))[2, 0.25], R.random_masks((17, 16, 200))[2, 0.1]
    cap = 4096                                                                          # upper bound of N known to the host
    m = torch.from_numpy(first).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        P.component_sizes(P.label(m, 2), cap)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lab, num = P.label(m, 2, return_num=True)
        sizes = P.component_sizes(lab, cap)
    for mask in (first, second, np.zeros((17, 16, 200), np.uint8), first):
        m.copy_(torch.from_numpy(mask).cuda())
        g.replay()
        want, n = R.scipy_label(mask, 2)
        assert n < cap and int(num) == n
        assert np.array_equal(lab.cpu().numpy(), want)
        assert np.array_equal(sizes.cpu().numpy(), np.bincount(want.ravel(), minlength=cap + 1))


def test_component_sizes_against_bincount():
    P = _P()
    for mask, c in ((R.random_masks((9, 21, 37))[1, 0.25], 1), (R.structured("pairs"), 2), (R.structured("one"), 1), (R.structured("zero"), 3),
                    (R.structured("checkerboard"), 1)):
        want, n = R.scipy_label(mask, c)
        lab, num = P.label(torch.from_numpy(mask).cuda(), c, return_num=True)
        for arg in (n, num):                                                            # a host int, or the device count (read back)
            sizes = P.component_sizes(lab, arg)
            assert sizes.dtype == torch.int32 and sizes.shape == (n + 1,)
            assert np.array_equal(sizes.cpu().numpy(), np.bincount(want.ravel(), minlength=n + 1))
        if n > 3:                                                                       # a smaller num cuts the table, labels above it are not counted
            assert np.array_equal(P.component_sizes(lab, 3).cpu().numpy(), np.bincount(want.ravel())[:4])
        assert np.array_equal(P.component_sizes(lab, n + 5).cpu().numpy(), np.bincount(want.ravel(), minlength=n + 6))


@pytest.mark.parametrize("relabel", [False, True], ids=["ids_kept", "relabel"])
def test_remove_small_objects_against_numpy(relabel):
    """The NumPy statement: components with fewer than min_size voxels become 0; the others keep their ids, or (relabel) are renumbered
    1..N' in the same order.  min_size 1 removes nothing, a min_size above every component removes everything."""
    P = _P()
    mask = R.random_masks((17, 16, 200))[1, 0.32]
    want, n = R.scipy_label(mask, 1)
    sizes = np.bincount(want.ravel(), minlength=n + 1)
    lab = P.label(torch.from_numpy(mask).cuda(), 1)
    before = lab.clone()
    assert sizes[1:].max() > 8 and (sizes[1:] < 8).any()
    for min_size in (1, 2, 8, int(sizes[1:].max()), int(sizes[1:].max()) + 1):
        keep = sizes >= min_size
        keep[0] = False
        table = np.where(keep, np.cumsum(keep) if relabel else np.arange(n + 1), 0).astype(np.int32)
        for num in (n, None):
            out, left = P.remove_small_objects(lab, min_size, relabel=relabel, num=num, return_num=True)
            assert out.dtype == torch.int32 and int(left) == int(keep.sum())
            assert np.array_equal(out.cpu().numpy(), table[want])
        assert torch.equal(lab, before)                                                  # the input is left alone
        if min_size == 1:
            assert np.array_equal(out.cpu().numpy(), want)
        if min_size > sizes[1:].max():
            assert not out.any() and int(left) == 0
    plain = P.remove_small_objects(lab, 8, relabel=relabel)                              # skimage's call shape: the labels alone
    keep = (sizes >= 8) & (np.arange(n + 1) > 0)
    assert torch.is_tensor(plain) and np.array_equal(plain.cpu().numpy(), np.where(keep, np.cumsum(keep) if relabel else np.arange(n + 1), 0)[want])


def test_binarize_then_label_end_to_end():
    P = _P()
    rng = np.random.default_rng(3)
    blobs = R.balls((12, 40, 72), fill=0.15, rmin=2, rmax=4)                            # a bimodal prediction: blobs near 0.8 on a floor near 0.1
    pred = torch.from_numpy((0.2 * rng.random((12, 40, 72)) + 0.7 * blobs).astype(np.float32)).cuda()
    mask = P.binarize(pred)
    lab, num = P.label(mask, return_num=True)
    cpu = mask.cpu().numpy()
    want, n = R.scipy_label(cpu, 3)
    assert 0 < cpu.mean() < 1 and n > 1
    assert int(num) == n and np.array_equal(lab.cpu().numpy(), want)


def test_two_to_the_31_voxels_are_refused_before_any_launch():
    big = torch.empty(2 ** 31, dtype=torch.uint8, device="cuda").view(2048, 1024, 1024)
    with pytest.raises(NotImplementedError, match="2\\^31"):
        _P().label(big)

"""Label stitching on the device (``prepost.LabelStitcher`` / ``label_blocks``, csrc/stitch.hip) - everything bit for bit, no permutation
matching: per-block ``prepost.label`` + stitch against ``scipy.ndimage.label`` of the whole mask over ragged grids, blocks one voxel thick, faces
wider than a wave and a workgroup, 2-D, structured masks (the corner pair, the first voxel in a later block, ...); ``label_blocks`` against
``prepost.label``; the contact rule against the twin (tests/stitch_ref.py), on hand-made cases and on per-block watersheds; overflow; graph
capture; the closed-form rods-and-slabs mask compared on the device."""
import numpy as np
import pytest
import torch

import stitch_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


def P():
    from biapy_amd import prepost
    return prepost


def cut(a, block):
    """The blocks of a host array as contiguous device tensors, in raster order of the grid."""
    shape3, block3 = ((1,) + a.shape, (1,) + tuple(block)) if a.ndim == 2 else (a.shape, tuple(block))
    v = a.reshape(shape3)
    out = [torch.from_numpy(np.ascontiguousarray(v[s])).to(DEV) for s in R.block_slices(shape3, tuple(min(b, s) for b, s in zip(block3, shape3)))]
    return [t[0].contiguous() for t in out] if a.ndim == 2 else out


def index_of(st, b):
    return tuple(int(v) for v in np.unravel_index(b, st.grid))[3 - st.ndim:]


def stitch(labels, nums, shape, block, **kw):
    """Device blocks in, (stitcher, M as int, renumbered blocks on the host) out."""
    st = P().LabelStitcher(shape, block, **kw)
    for b, (lab, n) in enumerate(zip(labels, nums)):
        st.add(index_of(st, b), lab, n)
    M = st.resolve()
    st.apply()
    return st, int(M), [t.cpu().numpy() for t in labels]


def label_and_stitch(mask, block, c, **kw):
    per = [P().label(m, c, return_num=True) for m in cut(mask, block)]
    _, M, out = stitch([l for l, _ in per], [n for _, n in per], mask.shape, block, connectivity=c, **kw)
    return R.assemble(out, mask.shape, block), M


def check_against_scipy(name, blocks=None):
    mask, own = R.all_masks()[name]
    for c in range(1, mask.ndim + 1):
        want, n = R.scipy_label(mask, c)
        for block in blocks or own:
            got, M = label_and_stitch(mask, block, c)
            assert M == n and np.array_equal(got, want), (name, c, block)


@pytest.mark.parametrize("block", R.BLOCKS)
@pytest.mark.parametrize("density", R.DENSITIES)
def test_random_masks_equal_scipy(density, block):
    check_against_scipy(f"random {density}", (block,))


def test_faces_wider_than_a_wave_and_a_workgroup():
    check_against_scipy("lanes")


def test_two_dimensions_in_both_forms():
    check_against_scipy("2-D")
    mask, (block,) = R.all_masks()["2-D"]
    for c in (1, 2):
        want, n = R.scipy_label(mask, c)
        got, M = label_and_stitch(mask[None], (1,) + block, c)
        assert M == n and np.array_equal(got[0], want)


@pytest.mark.parametrize("name", sorted(R.structured()))
def test_structured_masks_equal_scipy(name):
    check_against_scipy(name)
    if name == "corner pair":
        assert [label_and_stitch(R.structured()[name], R.BLOCK, c)[1] for c in (1, 2, 3)] == [2, 2, 1]
    if name == "first voxel in a later block":
        got, M = label_and_stitch(R.structured()[name], R.BLOCK, 1)
        assert M == 6 and got[0, 8, 5] == 2 and got[0, 8, 30] == got[1, 7, 33] == 3 and got[0, 9, 0] == 4


def test_num_as_int_upper_bound_and_as_none():
    mask = R.all_masks()["random 0.32"][0]
    want, n = R.scipy_label(mask, 2)
    per = [P().label(m, 2) for m in cut(mask, R.BLOCK)]
    for nums in ([None] * 27, [int(l.max()) + 3 for l in per]):             # ids that no voxel carries take no number
        labels = [l.clone() for l in per]
        _, M, out = stitch(labels, nums, mask.shape, R.BLOCK, connectivity=2)
        assert M == n and np.array_equal(R.assemble(out, mask.shape, R.BLOCK), want)


# ---- label_blocks ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["random 0.32", "random 0.5", "corner pair", "first voxel in a later block", "boustrophedon", "empty blocks between"])
def test_label_blocks_equals_label(name):
    p = P()
    mask = torch.from_numpy(R.all_masks()[name][0]).to(DEV)
    for c in (1, 2, 3):
        want, n = p.label(mask, c, return_num=True)
        for block in ((4, 21, 70), (5, 21, 70), (1, 21, 70), R.BLOCK, (13, 21, 70)):
            got, M = p.label_blocks(mask, block, c, return_num=True)
            assert int(M) == int(n) and torch.equal(got, want), (name, c, block)


def test_label_blocks_balls_slabs_dtypes_and_repeats():
    p = P()
    mask_np = R.all_masks()["balls 64"][0]
    want, n = R.scipy_label(mask_np, 3)
    mask = torch.from_numpy(mask_np).to(DEV)
    got, M = p.label_blocks(mask, (16, 64, 64), return_num=True)
    assert int(M) == n and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(p.label_blocks(mask, (16, 64, 64)), got)                                  # two calls, the same bits
    assert torch.equal(p.label_blocks(mask.bool(), (16, 64, 64)), got) and torch.equal(p.label_blocks(mask * 200, (24, 64, 64)), got)
    one, m1 = p.label_blocks(mask, return_num=True)                                              # one slab: label itself
    assert torch.equal(one, p.label(mask)) and int(m1) == n and torch.equal(one, got)
    m2 = torch.from_numpy(R.all_masks()["2-D"][0]).to(DEV)
    for c in (1, 2):
        assert torch.equal(p.label_blocks(m2, (8, 33), c), p.label(m2, c)) and torch.equal(p.label_blocks(m2, (8, 70), c), p.label(m2, c))
    with pytest.raises(ValueError, match="connectivity"):
        p.label_blocks(m2, (8, 33), 3)
    with pytest.raises(ValueError, match="block extents"):
        p.label_blocks(mask, (0, 64, 64))
    odd = mask[:, :63, :63].contiguous()                                                         # slabs whose views are not 16-byte aligned
    assert torch.equal(p.label_blocks(odd, (5, 63, 63)), p.label(odd))


def test_rods_and_slabs_on_the_device():
    p = P()
    shape = (64, 64, 64)
    mask = R.rods_mask(shape, DEV)
    _, count = R.rods_expected(shape, DEV)
    got, M = p.label_blocks(mask, (24, 64, 64), return_num=True)
    assert int(M) == count and R.rods_check(got, shape)
    got, M = p.label_blocks(mask, (24, 40, 40), return_num=True)
    assert int(M) == count and R.rods_check(got, shape)


# ---- the contact rule --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.contact_cases()))
def test_contact_hand_made_cases_equal_the_twin(name):
    blocks, nums, shape, block, mc, expect = R.contact_cases()[name]
    want, Mw = R.stitch_ref(blocks, nums, shape, block, 1, "contact", mc)
    labels = [torch.from_numpy(b).to(DEV) for b in blocks]
    _, M, out = stitch(labels, nums, shape, block, rule="contact", min_contact=mc)
    assert M == Mw == expect and all(np.array_equal(a, b) for a, b in zip(out, want)), name


def test_contact_joins_per_block_watersheds():
    p = P()
    shape, block = (40, 40, 80), (40, 40, 40)
    g = np.ogrid[0:40, 0:40, 0:80]
    pred = np.zeros(shape, np.float32)
    for (cz, cy, cx), r in (((20, 20, 39.5), 10), ((12, 12, 12), 8), ((22, 14, 20), 8), ((20, 26, 64), 9), ((8, 8, 70), 6)):
        pred[(g[0] - cz) ** 2 + (g[1] - cy) ** 2 + (g[2] - cx) ** 2 <= r * r] = 1.0
    labels, nums = [], []
    for part in cut(pred, block):
        mask = p.binarize(part, 0.5)
        dist = p.distance_transform_edt(mask)
        seeds, n = p.label((dist > 4.0).to(torch.uint8), 1, return_num=True)
        labels.append(p.watershed(-dist, seeds, mask))
        nums.append(n)
    before = [l.cpu().numpy() for l in labels]
    want, Mw = R.stitch_ref(before, [int(n) for n in nums], shape, block, 1, "contact", (1, 2))
    _, M, out = stitch(labels, nums, shape, block, rule="contact")
    assert M == Mw and all(np.array_equal(a, b) for a, b in zip(out, want))
    whole = R.assemble(out, shape, block)
    assert whole[20, 20, 39] == whole[20, 20, 40] > 0 and before[0][20, 20, 39] > 0 and before[1][20, 20, 0] > 0      # the ball on the face: ONE instance
    assert M == sum(int(n) for n in nums) - 1 and np.array_equal(whole > 0, pred > 0.5)


# ---- overflow, graph capture -------------------------------------------------------------------------------------------------------------------

def test_overflow_leaves_the_blocks_alone():
    mask = R.all_masks()["random 0.32"][0]
    want, n = R.scipy_label(mask, 1)
    per, nums = R.label_per_block(mask, R.BLOCK, 1)
    T = sum(nums)
    assert R.stitch_ref(per, nums, mask.shape, R.BLOCK, 1, max_labels=T - 1)[1] == -1
    labels = [torch.from_numpy(b).to(DEV) for b in per]
    _, M, out = stitch(labels, nums, mask.shape, R.BLOCK, connectivity=1, max_labels=T - 1)
    assert M == -1 and all(np.array_equal(a, b) for a, b in zip(out, per))
    _, M, out = stitch(labels, nums, mask.shape, R.BLOCK, connectivity=1, max_labels=T)          # exactly T fits; the next stitcher is unaffected
    assert M == n and np.array_equal(R.assemble(out, mask.shape, R.BLOCK), want)
    got, M = P().label_blocks(torch.from_numpy(mask).to(DEV), R.BLOCK, 1, return_num=True, max_labels=T - 1)
    assert int(M) == -1 and np.array_equal(got.cpu().numpy(), R.assemble(per, mask.shape, R.BLOCK))


def test_resolve_and_apply_replay_in_a_graph():
    p = P()
    masks = [R.all_masks()[k][0] for k in ("random 0.32", "random 0.5", "all zero", "first voxel in a later block")]
    c = 3
    per = [R.label_per_block(m, R.BLOCK, c) for m in masks]
    labels = [torch.from_numpy(b).to(DEV) for b in per[0][0]]
    nums = torch.tensor(per[0][1], dtype=torch.int32, device=DEV)
    st = p.LabelStitcher(R.SHAPE, R.BLOCK, c)
    for b, lab in enumerate(labels):
        st.add(index_of(st, b), lab, nums[b])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        M = st.resolve()                                                                         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        M = st.resolve()
        st.apply()
    for (blocks, counts), mask in zip(per, masks):
        for lab, b in zip(labels, blocks):
            lab.copy_(torch.from_numpy(b))
        nums.copy_(torch.tensor(counts, dtype=torch.int32))
        graph.replay()
        want, n = R.scipy_label(mask, c)
        assert int(M) == n and np.array_equal(R.assemble([t.cpu().numpy() for t in labels], R.SHAPE, R.BLOCK), want)

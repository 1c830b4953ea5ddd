"""Morphology on the MI355X (biapy_amd/prepost.py: binary_erosion, binary_dilation, binary_opening, binary_closing, erosion, dilation,
find_boundaries, binary_fill_holes, clear_border; csrc/morph.hip) against its statement (tests/morph_ref.py, itself held against SciPy by
test_morph_cpu.py).  Every comparison is bit for bit: the functions are integer arithmetic (float32 minima and maxima are equal as values, and
the inputs hold no -0.0 and no NaN).  Inputs and references are built once per process."""
import numpy as np
import pytest
import torch

import morph_ref as R

pytestmark = pytest.mark.gpu


def _P():
    from biapy_amd import prepost

    return prepost


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                                  # a copy: the shared inputs are read-only


def _same(got, want, what=""):
    want = np.asarray(want)
    assert got.is_cuda and tuple(got.shape) == want.shape, what
    assert got.dtype == torch.from_numpy(want[:0].copy()).dtype, (what, got.dtype, want.dtype)
    np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=str(what))


# ---- the binary path ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.binary_cases()), ids=str)
def test_binary_erosion_and_dilation_at_both_border_values(name):
    P = _P()
    mask, c, dilate, _ = R.binary_cases()[name]
    fn = P.binary_dilation if dilate else P.binary_erosion
    d = _dev(mask)
    for bv in (0, 1):
        _same(fn(d, c, 1, bv), R.binary_ref(mask, dilate, c, 1, bv), (name, bv))
    assert torch.equal(d.cpu(), torch.from_numpy(mask))                                       # the input is left alone


def test_2d_in_both_spellings():
    P = _P()
    for name, (mask, c, dilate, _) in R.binary_cases().items():
        if mask.ndim != 2:
            continue
        fn = P.binary_dilation if dilate else P.binary_erosion
        for bv in (0, 1):                                                                     # (Y, X) against (1, Y, X): differs at border_value 0 only
            two, three = fn(_dev(mask), c, 1, bv), fn(_dev(mask[None]), c, 1, bv)
            _same(three, R.binary_ref(mask[None], dilate, c, 1, bv), (name, bv))
            if bv == (1 if dilate else 0):
                if mask.shape == (37, 41):
                    assert not torch.equal(two[None], three), (name, bv)                      # the absorbing border reaches in through z
            else:
                assert torch.equal(two[None], three), (name, bv)
    for key, x in R.grey_cases().items():
        if x.ndim == 2:
            for c in (1, 2):
                assert torch.equal(P.erosion(_dev(x), c)[None], P.erosion(_dev(x[None]), c)), key
                assert torch.equal(P.dilation(_dev(x), c)[None], P.dilation(_dev(x[None]), c)), key


def test_byte_values_bool_and_constant_masks():
    P = _P()
    mask = R.random_mask((9, 21, 37), 0.9, 1)
    for scale in (2, 255):                                                                    # every nonzero byte is foreground, 0 / 1 comes out
        _same(P.binary_erosion(_dev(mask * np.uint8(scale)), 1, 1, 1), R.binary_erosion_ref(mask, 1, 1, 1), scale)
        _same(P.binary_dilation(_dev((1 - mask) * np.uint8(scale)), 2), R.binary_dilation_ref(1 - mask, 2), scale)
    mixed = np.where(mask != 0, np.random.default_rng(2).integers(1, 256, mask.shape), 0).astype(np.uint8)
    _same(P.binary_erosion(_dev(mixed), 3, 1, 1), R.binary_erosion_ref(mask, 3, 1, 1), "mixed bytes")
    _same(P.binary_erosion(_dev(mask).bool(), 2, 1, 1), R.binary_erosion_ref(mask, 2, 1, 1), "bool")
    _same(P.binary_dilation(_dev(1 - mask).bool(), 1), R.binary_dilation_ref(1 - mask, 1), "bool")
    for shape in ((6, 7, 19), (7, 19)):
        for value in (0, 1):
            const = np.full(shape, value, np.uint8)
            for c in range(1, len(shape) + 1):
                for bv in (0, 1):
                    _same(P.binary_erosion(_dev(const), c, 1, bv), R.binary_erosion_ref(const, c, 1, bv), (shape, value, c, bv))
                    _same(P.binary_dilation(_dev(const), c, 1, bv), R.binary_dilation_ref(const, c, 1, bv), (shape, value, c, bv))
    for corner, m in R.corner_cases().items():
        for c in (1, 2, 3):
            _same(P.binary_dilation(_dev(m), c), R.binary_dilation_ref(m, c), corner)
            _same(P.binary_dilation(_dev(m), c, 1, 1), R.binary_dilation_ref(m, c, 1, 1), corner)
            _same(P.binary_erosion(_dev(1 - m), c, 1, 1), R.binary_erosion_ref(1 - m, c, 1, 1), corner)


@pytest.mark.parametrize("c", (1, 2, 3))
def test_iterations_opening_and_closing(c):
    P = _P()
    m = R.ball_volume()
    d = _dev(m)
    for bv in (0, 1):
        for k in (1, 2, 3, 7):
            _same(P.binary_erosion(d, c, k, bv), R.binary_erosion_ref(m, c, k, bv), ("erode", k, bv))
            _same(P.binary_dilation(d, c, k, bv), R.binary_dilation_ref(m, c, k, bv), ("dilate", k, bv))
        for k in (1, 2):
            _same(P.binary_opening(d, c, k, bv), R.binary_opening_ref(m, c, k, bv), ("open", k, bv))
            _same(P.binary_closing(d, c, k, bv), R.binary_closing_ref(m, c, k, bv), ("close", k, bv))
    small = np.zeros_like(m)
    small[:14, :14, :14] = m[:14, :14, :14]
    assert not P.binary_erosion(_dev(small), 1, 7, 1).any() and P.binary_erosion(_dev(small), 1, 3, 1).any()      # 7 erase the ball of radius 5


# ---- the grey paths and the spans --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.grey_cases()), ids=str)
def test_grey_erosion_and_dilation(name):
    P = _P()
    x = R.grey_cases()[name]
    d = _dev(x)
    for c in range(1, x.ndim + 1):
        _same(P.erosion(d, c), R.erosion_ref(x, c), (name, c))
        _same(P.dilation(d, c), R.dilation_ref(x, c), (name, c))


@pytest.mark.parametrize("key", list(R.span_cases()), ids=str)
def test_lane_and_wave_spans(key):
    P = _P()
    x = R.span_cases()[key]
    for v in (x, x[None]):                                                                    # two / three rows of a plane, and of a volume
        d = _dev(v)
        for c in (1, 2):
            _same(P.erosion(d, c), R.erosion_ref(v, c), (key, c))
            _same(P.dilation(d, c), R.dilation_ref(v, c), (key, c))
            _same(P.find_boundaries(d, c), R.find_boundaries_ref(v, c), (key, c))
            if x.dtype == np.uint8:
                for bv in (0, 1):
                    _same(P.binary_erosion(d, c, 1, bv), R.binary_erosion_ref(v, c, 1, bv), (key, c, bv))
                    _same(P.binary_dilation(d, c, 1, bv), R.binary_dilation_ref(v, c, 1, bv), (key, c, bv))


def test_unaligned_and_non_contiguous_views():
    P = _P()
    for dt, offsets in ((np.uint8, (1, 3, 4, 8, 12, 15)), (np.int32, (4, 8, 12)), (np.float32, (4, 8, 12))):
        for name in (f"{np.dtype(dt).name} (5, 7, 9)", f"{np.dtype(dt).name} (16, 32, 64)"):
            x = R.grey_cases()[name]
            es = x.dtype.itemsize
            want = {c: (R.erosion_ref(x, c), R.dilation_ref(x, c), R.find_boundaries_ref(x, c, "inner")) for c in (1, 3)}
            views = []
            for off in offsets:                                                               # bytes past a 16-byte boundary
                buf = torch.zeros(x.size + 16, dtype=_dev(x[:1]).dtype, device="cuda")
                assert buf.data_ptr() % 16 == 0
                view = buf[off // es:off // es + x.size].view(x.shape)
                view.copy_(_dev(x))
                assert view.data_ptr() % 16 == off and view.is_contiguous()
                views.append((view, f"{off} bytes"))
            perm = _dev(x.transpose(1, 0, 2)).permute(1, 0, 2)
            wide = torch.zeros(x.shape[:2] + (2 * x.shape[2],), dtype=perm.dtype, device="cuda")
            wide[:, :, ::2] = _dev(x)
            views += [(perm, "permuted"), (wide[:, :, ::2], "strided")]
            assert not perm.is_contiguous() and not wide[:, :, ::2].is_contiguous()
            for view, what in views:
                for c in (1, 3):
                    _same(P.erosion(view, c), want[c][0], (name, what))
                    _same(P.dilation(view, c), want[c][1], (name, what))
                    _same(P.find_boundaries(view, c, "inner"), want[c][2], (name, what))
                    if dt == np.uint8:
                        _same(P.binary_erosion(view, c), R.binary_erosion_ref(x, c), (name, what))
                        _same(P.binary_dilation(view, c, 1, 1), R.binary_dilation_ref(x, c, 1, 1), (name, what))


# ---- boundaries ---------------------------------------------------------------------------------------------------------------------------------------

def test_find_boundaries():
    P = _P()
    lab = P.label(_dev(R.ball_volume()), connectivity=1)
    host = lab.cpu().numpy()
    assert host.max() >= 3
    for c in (1, 2, 3):
        for mode in ("thick", "inner"):
            _same(P.find_boundaries(lab, c, mode), R.find_boundaries_ref(host, c, mode), (c, mode))
        _same(P.find_boundaries(lab, c, "inner", background=2), R.find_boundaries_ref(host, c, "inner", 2), (c, "background 2"))
        _same(P.find_boundaries(-lab, c, "inner", background=-1), R.find_boundaries_ref(-host, c, "inner", -1), (c, "negative labels"))
        _same(P.find_boundaries(lab.float(), c, "inner"), R.find_boundaries_ref(host.astype(np.float32), c, "inner"), (c, "float32"))
        _same(P.find_boundaries(lab > 0, c, "inner"), R.find_boundaries_ref(host > 0, c, "inner"), (c, "bool"))
    two = R.touching_labels()
    for c in (1, 2):
        for mode in ("thick", "inner"):
            _same(P.find_boundaries(_dev(two), c, mode), R.find_boundaries_ref(two, c, mode), ("touching", c, mode))
    thick = P.find_boundaries(_dev(two))
    assert thick[2, 3] == 1 and thick[2, 4] == 1 and thick[2, 2] == 0
    _same(P.dilation(lab, 1), R.dilation_ref(host, 1), "the largest neighbouring id wins")


# ---- radius --------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", (1, 3, 5))
def test_radius_against_scipy_with_the_ball_footprint(r):
    from scipy import ndimage

    P = _P()
    m = R.ball_volume()
    g = np.indices((2 * r + 1,) * 3) - r
    ball = (g ** 2).sum(0) <= r * r
    _same(P.binary_dilation(_dev(m), radius=r), ndimage.binary_dilation(m, ball, border_value=0).astype(np.uint8), "dilate")
    _same(P.binary_erosion(_dev(m), border_value=1, radius=r), ndimage.binary_erosion(m, ball, border_value=1).astype(np.uint8), "erode")
    _same(P.binary_dilation(_dev(m), radius=r), R.ball_ref(m, r, True), "dilate, the statement")
    plane = m[20]
    _same(P.binary_erosion(_dev(plane), border_value=1, radius=r), R.ball_ref(plane, r, False), "a disk")
    ones, zeros = torch.ones(6, 7, 8, dtype=torch.uint8, device="cuda"), torch.zeros(6, 7, 8, dtype=torch.uint8, device="cuda")
    assert P.binary_erosion(ones, border_value=1, radius=r).all() and not P.binary_dilation(zeros, radius=r).any()      # the transform's sentinel
    with pytest.raises(NotImplementedError, match="border_value=1 only"):
        P.binary_erosion(_dev(m), radius=r)
    with pytest.raises(NotImplementedError, match="border_value=0 only"):
        P.binary_dilation(_dev(m), border_value=1, radius=r)


# ---- hole filling and border clearing ---------------------------------------------------------------------------------------------------------------

def test_binary_fill_holes():
    from scipy import ndimage

    P = _P()
    for name, (mask, filled) in R.hand_cases().items():
        _same(P.binary_fill_holes(_dev(mask)), filled, name)
    h = R.holes_volume()
    want = R.fill_holes_ref(h)
    np.testing.assert_array_equal(want, ndimage.binary_fill_holes(h))
    n = int(ndimage.label(h == 0)[1])
    d = _dev(h)
    for num in (None, n, torch.tensor(n, dtype=torch.int32, device="cuda"), n + 100):
        _same(P.binary_fill_holes(d, num), want, f"num = {num}")
    _same(P.binary_fill_holes(d.bool()), want, "bool")
    _same(P.binary_fill_holes(_dev(h * np.uint8(255))), want, "bytes of 255")
    plane = h[32]
    _same(P.binary_fill_holes(_dev(plane)), ndimage.binary_fill_holes(plane).astype(np.uint8), "2-D")


def test_clear_border():
    P = _P()
    lab = P.label(_dev(R.holes_volume()), connectivity=1)
    host = lab.cpu().numpy()
    n = int(host.max())
    want, left = R.clear_border_ref(host, n)
    assert 0 < left < n                                                                       # some labels touch the border, some do not
    for num in (None, n, torch.tensor(n, dtype=torch.int32, device="cuda")):
        got, k = P.clear_border(lab, num, return_num=True)
        _same(got, want, f"num = {num}")
        assert int(k) == left
    got, k = P.clear_border(lab, n + 50, return_num=True)                                     # an upper bound: the absent ids count as survivors
    _same(got, want, "an upper bound")
    assert int(k) == left + 50
    want_r, _ = R.clear_border_ref(host, n, relabel=True)
    _same(P.clear_border(lab, n, relabel=True), want_r, "relabel")
    faces = R.face_labels()
    for n_max in (8, 9):
        for relabel in (False, True):
            _same(P.clear_border(_dev(faces), n_max, relabel=relabel), R.clear_border_ref(faces, n_max, relabel)[0], ("faces", n_max, relabel))
    two = R.touching_labels()
    _same(P.clear_border(_dev(two)), R.clear_border_ref(two, 3)[0], "2-D")
    inner = np.zeros((6, 7, 8), np.int32)
    inner[2:4, 2:5, 2:6] = 1
    _same(P.clear_border(_dev(inner)), inner, "all kept")
    edge = np.ones((3, 4, 5), np.int32)
    _same(P.clear_border(_dev(edge)), np.zeros_like(edge), "none kept")
    _same(P.clear_border(_dev(np.zeros((3, 4), np.int32))), np.zeros((3, 4), np.int32), "no labels")


# ---- whole calls ----------------------------------------------------------------------------------------------------------------------------------------

def test_two_calls_give_the_same_bits():
    P = _P()
    m, x = _dev(R.holes_volume()), _dev(R.grey_cases()["float32 (33, 37, 41)"])
    lab = P.label(m, connectivity=1)
    for call in (lambda: P.binary_erosion(m, 3, 2, 1), lambda: P.binary_dilation(m, 2), lambda: P.erosion(x, 3), lambda: P.dilation(lab, 1),
                 lambda: P.find_boundaries(lab, 2, "inner"), lambda: P.binary_fill_holes(m), lambda: P.clear_border(lab),
                 lambda: P.binary_dilation(m, radius=3)):
        first, second = call(), call()
        assert first.data_ptr() != second.data_ptr()
        assert torch.equal(first.view(torch.uint8) if first.dtype == torch.float32 else first, second.view(torch.uint8) if second.dtype == torch.float32 else second)


def test_graph_capture_of_fill_erode_label_watershed_clear():
    """Captured once with upper bounds for the counts, replayed after the mask was overwritten in place (an all-background one among them): every
    replay gives what the eager calls give on the mask of that moment."""
    P = _P()
    shape, bound = (24, 40, 56), 4000
    rng = np.random.default_rng(3)
    masks = [R.balls(shape, 10, 4, 8, 1), R.balls(shape, 5, 5, 9, 2), np.zeros(shape, np.uint8), R.balls(shape, 10, 4, 8, 1)]
    for mk in masks[:2]:
        mk[rng.random(shape) < 0.02] = 0                                                      # punched holes
    image = _dev(rng.random(shape).astype(np.float32))
    mask = _dev(masks[0])

    def pipeline(m, num):
        filled = P.binary_fill_holes(m, num)
        seeds = P.label(P.binary_erosion(filled, 1, 2, 1), connectivity=1)
        ws = P.watershed(image, seeds, mask=filled)
        return filled, ws, P.clear_border(ws, num, relabel=True, return_num=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pipeline(mask, bound)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        filled, ws, (kept, left) = pipeline(mask, bound)
    for k, mk in enumerate(masks):
        mask.copy_(_dev(mk))
        g.replay()
        torch.cuda.synchronize()
        efilled, ews, (ekept, eleft) = pipeline(_dev(mk), bound)
        assert torch.equal(filled, efilled) and torch.equal(ws, ews) and torch.equal(kept, ekept) and int(left) == int(eleft), k
        _same(filled, R.fill_holes_ref(mk), f"replay {k}")
        if not mk.any():
            assert not ws.any() and not kept.any()
        else:
            assert ws.any()


def test_binarize_fill_erode_label_watershed_end_to_end_against_the_host():
    from scipy import ndimage

    import watershed_ref as W

    P = _P()
    h = R.holes_volume()
    rng = np.random.default_rng(8)
    pred = np.where(h != 0, 0.6 + 0.4 * rng.random(h.shape), 0.4 * rng.random(h.shape)).astype(np.float32)
    d = _dev(pred)
    filled = P.binary_fill_holes(P.binarize(d, 0.5))
    seeds, n = P.label(P.binary_erosion(filled, border_value=1, radius=2), connectivity=1, return_num=True)
    ws = P.watershed(-d, seeds, mask=filled)
    g = np.indices((5, 5, 5)) - 2
    hfilled = ndimage.binary_fill_holes(pred > 0.5)
    hseeds, hn = ndimage.label(ndimage.binary_erosion(hfilled, (g ** 2).sum(0) <= 4, border_value=1))
    _same(filled, hfilled.astype(np.uint8), "filled")
    assert int(n) == hn and hn >= 3
    _same(seeds, hseeds.astype(np.int32), "seeds")
    _same(ws, W.watershed_ref(-pred, hseeds.astype(np.int32), hfilled.astype(np.uint8), 1), "watershed")


def test_refusals_on_device_tensors():
    P = _P()
    m = torch.ones(4, 5, 6, dtype=torch.uint8, device="cuda")
    lab = m.int()
    for fn in (P.binary_erosion, P.binary_dilation, P.binary_opening, P.binary_closing, P.binary_fill_holes, P.erosion, P.dilation, P.find_boundaries):
        with pytest.raises(NotImplementedError, match="works on"):
            fn(m.long())
        with pytest.raises(ValueError, match="2-D .* or 3-D"):
            fn(m.view(-1))
        with pytest.raises(NotImplementedError, match="empty axis"):
            fn(m[:0])
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(m.cpu())
    for fn in (P.binary_erosion, P.binary_dilation, P.binary_opening, P.binary_closing):
        with pytest.raises(NotImplementedError, match="iterations must be >= 1"):
            fn(m, 1, 0)
        with pytest.raises(ValueError, match="connectivity must be in 1.."):
            fn(m[0], 3)
        with pytest.raises(ValueError, match="border_value must be 0 or 1"):
            fn(m, 1, 1, 2)
    with pytest.raises(NotImplementedError, match="offers the modes"):
        P.find_boundaries(lab, mode="outer")
    with pytest.raises(NotImplementedError, match="int32 labels"):
        P.clear_border(m)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.clear_border(lab.cpu())
    big = torch.empty((2, 2 ** 15, 2 ** 15), dtype=torch.uint8, device="cuda")                # 2^31 voxels: nothing is launched
    for fn in (P.binary_erosion, P.erosion, P.find_boundaries, P.binary_fill_holes):
        with pytest.raises(NotImplementedError, match="2\\^31"):
            fn(big)
    from biapy_amd import _lib as L
    out = torch.empty_like(m)
    assert L.lib.bpx_morph(m.data_ptr(), L.U8, 4, 5, 6, 3, 1, 0, 0, 0, m.data_ptr(), L.stream_ptr()) != 0
    assert "out_d must not be in_d" in L.lib.bpx_last_error().decode()
    assert L.lib.bpx_morph(m.data_ptr(), L.U8, 4, 5, 6, 3, 1, 0, 0, 0, out.data_ptr(), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert out.all()

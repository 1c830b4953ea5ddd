"""Device patch sampler on the MI355X (biapy_amd/sampler.py, csrc/sampler.hip) against its statement: the gathered windows bit for bit against
torch slicing on the CPU, the drawn origins bit for bit against the host twin (tests/sampler_ref.py), the frequencies of device draws, a volume of
more than 2^31 voxels, graph capture and ``train_one_epoch`` fed by ``DevicePatchLoader``.  Every comparison is exact or a five-sigma count bound."""
import types

import numpy as np
import pytest
import torch

import sampler_ref as SR

pytestmark = pytest.mark.gpu

EXT = [(9, 21, 37), (12, 16, 40)]
HAS_U16 = hasattr(torch, "uint16")
_cache = {}


def _S(*a, **kw):
    from biapy_amd.sampler import DevicePatchSampler

    return DevicePatchSampler(*a, **kw)


def _volume(ext, ch, dtype, seed):
    """A CPU tensor (Z, Y, X, ch) of the dtype, seeded; computed once and shared."""
    key = (tuple(ext), ch, dtype, seed)
    if key not in _cache:
        g = np.random.RandomState(seed)
        if dtype == torch.float32:
            a = g.standard_normal((*ext, ch)).astype(np.float32)
        elif dtype == torch.uint8:
            a = g.randint(0, 256, (*ext, ch)).astype(np.uint8)
        else:
            a = g.randint(0, 65536, (*ext, ch)).astype(np.uint16)
        _cache[key] = torch.from_numpy(a)
    return _cache[key]


def _origins(ext, patch):
    """Every corner of every volume, then origins with an odd x0 (rows that start off every alignment) - 20 in all."""
    Pz, Py, Px = patch
    out = [(v, z, y, x) for v, (Z, Y, X) in enumerate(ext) for z in (0, Z - Pz) for y in (0, Y - Py) for x in (0, X - Px)]
    out += [(0, 1, 3, 1), (0, 2, 5, 7), (1, 3, 2, 13), (1, 5, 1, 5)]
    return out


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# ---- 1. gather ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch", [(4, 8, 16), (3, 5, 7)], ids=["p4x8x16", "p3x5x7"])
@pytest.mark.parametrize("idt", [torch.float32, torch.uint8] + ([torch.uint16] if HAS_U16 else []), ids=["f32", "u8"] + (["u16"] if HAS_U16 else []))
@pytest.mark.parametrize("C, Ct", [(1, 1), (3, 2), (16, 8)])
def test_gather_bit_for_bit(C, Ct, idt, patch):
    """Given ``origins=``: image and target against CPU slicing, both target dtypes, with and without ``scale``.  Patch (4, 8, 16) takes the
    16-byte pieces (for a uint8 target only where 16 * Ct is a multiple of 16: every Ct here), (3, 5, 7) the element path unless 7 * C is a multiple
    of 4 (C = 16)."""
    org = _origins(EXT, patch)
    od = torch.tensor(org, dtype=torch.int32, device="cuda")
    imgs = [_volume(e, C, idt, 10 + v) for v, e in enumerate(EXT)]
    for tdt in (torch.uint8, torch.float32):
        tgts = [_volume(e, Ct, tdt, 20 + v) for v, e in enumerate(EXT)]
        for scale in (None, 1.0 / 255.0):
            s = _S([a.cuda() for a in imgs], [a.cuda() for a in tgts], patch, batch_size=len(org), scale=scale, seed=1)
            x, t = s(origins=od)
            wx, wt = SR.gather(imgs, tgts, org, patch, scale)
            assert x.shape == (len(org), *patch, C) and x.dtype == torch.float32 and x.is_contiguous()
            assert t.shape == (len(org), *patch, Ct) and t.dtype == tdt and t.is_contiguous()
            assert torch.equal(_bits(x.cpu()), _bits(wx)), (tdt, scale)
            assert torch.equal(_bits(t.cpu()), _bits(wt)), (tdt, scale)
            assert torch.equal(s.last_origins, od) and int(s.counter) == 0          # given origins: nothing is drawn, the counter stays


def test_gather_patch_equal_to_its_volume_special_values_and_2d():
    """A patch that is the whole volume: one origin, the copy is the volume - NaN, infinities and -0.0 travel as their bits.  2-D volumes
    (Y, X, C) give (B, Py, Px, C) batches."""
    img = _volume((4, 8, 16), 3, torch.float32, 30).clone()
    img[0, 0, 0, 0], img[1, 2, 3, 1], img[3, 7, 15, 2], img[2, 2, 2, 0] = float("nan"), float("inf"), -0.0, float("-inf")
    img.view(torch.int32)[3, 0, 0, 0] = 0x7FC12345                         # a NaN with a payload
    tgt = _volume((4, 8, 16), 2, torch.float32, 31)
    other_i, other_t = _volume(EXT[0], 3, torch.float32, 32), _volume(EXT[0], 2, torch.float32, 33)
    s = _S([other_i.cuda(), img.cuda()], [other_t.cuda(), tgt.cuda()], (4, 8, 16), batch_size=3, seed=1)
    x, t = s(origins=torch.tensor([(1, 0, 0, 0), (0, 5, 13, 21), (1, 0, 0, 0)], dtype=torch.int32, device="cuda"))
    assert torch.equal(x[0].cpu().view(torch.int32), img.view(torch.int32)) and torch.equal(x[2].view(torch.int32), x[0].view(torch.int32))
    assert torch.equal(t[0].cpu(), tgt) and torch.equal(t[2].cpu(), tgt)
    assert torch.equal(x[1].cpu(), other_i[5:9, 13:21, 21:37])
    one = _S(img.cuda(), tgt.cuda(), (4, 8, 16), batch_size=5, seed=3)     # drawn: the only origin there is
    x, t = one()
    assert not one.last_origins.any() and all(torch.equal(x[b].cpu().view(torch.int32), img.view(torch.int32)) for b in range(5))
    # 2-D
    for C, Ct, patch in ((1, 1, (8, 16)), (3, 2, (5, 7))):
        imgs = [_volume((1, *e[1:]), C, torch.uint8, 40 + v)[0] for v, e in enumerate(EXT)]
        tgts = [_volume((1, *e[1:]), Ct, torch.uint8, 50 + v)[0] for v, e in enumerate(EXT)]
        org = [(0, 0, 0, 0), (0, 0, 21 - patch[0], 37 - patch[1]), (1, 0, 3, 5), (1, 0, 16 - patch[0], 40 - patch[1]), (0, 0, 2, 1)]
        s = _S([a.cuda() for a in imgs], [a.cuda() for a in tgts], patch, batch_size=len(org), seed=1)
        assert s.config()["patch"] == (1, *patch) and s.config()["extents"] == [(1, 21, 37), (1, 16, 40)]
        x, t = s(origins=torch.tensor(org, dtype=torch.int32, device="cuda"))
        wx, wt = SR.gather([a[None] for a in imgs], [a[None] for a in tgts], org, (1, *patch))
        assert x.shape == (len(org), *patch, C) and t.shape == (len(org), *patch, Ct)
        assert torch.equal(x.cpu(), wx[:, 0]) and torch.equal(t.cpu(), wt[:, 0])
        x, t = s()
        o = s.last_origins.cpu().numpy()
        assert np.array_equal(o, SR.draw(1, 0, len(org), [(1, 21, 37), (1, 16, 40)], (1, *patch))) and not o[:, 1].any()


def test_out_tensors_and_refusals():
    patch, B = (4, 8, 16), 4
    imgs = [_volume(e, 3, torch.float32, 10 + v).cuda() for v, e in enumerate(EXT)]
    tgts = [_volume(e, 2, torch.uint8, 20 + v).cuda() for v, e in enumerate(EXT)]
    s = _S(imgs, tgts, patch, batch_size=B, seed=5)
    od = torch.tensor([(0, 1, 3, 1), (1, 8, 8, 24), (0, 5, 13, 21), (1, 0, 0, 3)], dtype=torch.int32, device="cuda")
    want_x, want_t = s(origins=od)
    xo, to = torch.full((B, *patch, 3), 7.0, device="cuda"), torch.full((B, *patch, 2), 7, dtype=torch.uint8, device="cuda")
    got = s(out=(xo, to), origins=od)
    assert got[0].data_ptr() == xo.data_ptr() and got[1].data_ptr() == to.data_ptr()
    assert torch.equal(xo, want_x) and torch.equal(to, want_t)
    # an output that is not 16-byte aligned takes the element path: the same bits
    raw_x, raw_t = torch.zeros(xo.numel() + 1, device="cuda"), torch.zeros(to.numel() + 3, dtype=torch.uint8, device="cuda")
    ux, ut = raw_x[1:].view(xo.shape), raw_t[3:].view(to.shape)
    assert ux.data_ptr() % 16 and ut.data_ptr() % 16
    s(out=(ux, ut), origins=od)
    assert torch.equal(ux, want_x) and torch.equal(ut, want_t)
    both = torch.zeros(xo.numel() + 8, device="cuda")
    for out, word in (((both[:xo.numel()].view(xo.shape), both[8:].view(torch.uint8)[:to.numel()].view(to.shape)), "overlap"),
                      ((xo, tgts[1].view(-1)[:to.numel()].view(to.shape)), "overlaps a resident volume"),
                      ((imgs[0].view(-1)[:xo.numel()].view(xo.shape), to), "overlaps a resident volume"),
                      ((xo[:2], to), "out\\[0\\]"), ((xo, to.float()), "out\\[1\\]"), ((xo.double(), to), "out\\[0\\]"),
                      ((xo.permute(0, 2, 1, 3, 4), to), "out\\[0\\]"), ((xo, to.cpu()), "out\\[1\\]"), (xo, "pair")):
        with pytest.raises(ValueError, match=word):
            s(out=out)
    for bad, word in ((od[:3], "origins"), (od.long(), "origins"), (od.cpu(), "origins"),
                      (torch.tensor([(2, 0, 0, 0)] * 4, dtype=torch.int32, device="cuda"), "names volume 2"),
                      (torch.tensor([(0, 6, 0, 0)] * 4, dtype=torch.int32, device="cuda"), "outside volume 0"),
                      (torch.tensor([(1, 0, 0, 25)] * 4, dtype=torch.int32, device="cuda"), "outside volume 1"),
                      (torch.tensor([(0, 0, -1, 0)] * 4, dtype=torch.int32, device="cuda"), "outside volume 0")):
        with pytest.raises(ValueError, match=word):
            s(origins=bad)
    assert int(s.counter) == 0                                             # every refusal came before any launch
    # what only the device can tell the constructor
    m = [torch.zeros(e, dtype=torch.uint8, device="cuda") for e in EXT]
    with pytest.raises(ValueError, match="class 1 has probability"):
        _S(imgs, tgts, patch, batch_size=B, class_maps=m, class_probs=(0.5, 0.5))
    m[1][3, 3, 3] = 2
    with pytest.raises(ValueError, match="below the 2 classes"):
        _S(imgs, tgts, patch, batch_size=B, class_maps=m, class_probs=(1.0, 0.0))
    with pytest.raises(ValueError, match="non-contiguous"):
        _S([imgs[0].transpose(0, 1)], [tgts[0].transpose(0, 1)], patch, batch_size=B)
    assert _S(imgs, tgts, patch, batch_size=B, class_maps=[a * 0 for a in m], class_probs=(1.0, 0.0)).class_counts == [9 * 21 * 37 + 12 * 16 * 40, 0]


# ---- 2. draws -------------------------------------------------------------------------------------------------------------------------------------------
def _blank(ext):
    return ([torch.zeros(*e, 1, dtype=torch.uint8, device="cuda") for e in ext], [torch.zeros(*e, 1, dtype=torch.uint8, device="cuda") for e in ext])


DRAW_CASES = {
    "uniform_1": lambda: dict(ext=[EXT[0]], patch=(4, 8, 16)),
    "uniform_3": lambda: dict(ext=EXT + [(4, 8, 16)], patch=(4, 8, 16)),
    "class_k2": lambda: dict(ext=SR.hard_class_case()[1], patch=(2, 3, 7), maps=[np.minimum(m, 1) for m in SR.hard_class_case()[0]], probs=(0.4, 0.6)),
    "class_k3": lambda: dict(ext=SR.hard_class_case()[1], patch=(2, 3, 7), maps=SR.hard_class_case()[0], probs=(0.3, 0.4, 0.3)),
    "class_k3_wide_patch": lambda: dict(ext=SR.hard_class_case()[1], patch=(1, 1, 9), maps=SR.hard_class_case()[0], probs=(0.0, 0.5, 0.5)),
    "class_x1": lambda: dict(ext=SR.thin_class_case()[1], patch=(2, 3, 1), maps=SR.thin_class_case()[0], probs=(0.5, 0.5)),
}


@pytest.mark.parametrize("case", list(DRAW_CASES))
def test_draws_are_the_host_twins(case):
    """``last_origins`` of 8 consecutive calls at B = 7 against sampler_ref.draw with the same seed and counter, then the counter and the ticket."""
    c = DRAW_CASES[case]()
    imgs, tgts = _blank(c["ext"])
    kw = dict(class_maps=[torch.from_numpy(m).cuda() for m in c["maps"]], class_probs=c["probs"]) if "maps" in c else {}
    seed = 0x1234567887654321
    s = _S(imgs, tgts, c["patch"], batch_size=7, seed=seed, **kw)
    assert int(s.counter) == 0
    classes = set()
    for call in range(8):
        x, t = s()
        got = s.last_origins.cpu().numpy()
        want, cen = SR.draw(seed, call, 7, c["ext"], c["patch"], c.get("maps"), c.get("probs"), centres=True)
        assert got.dtype == np.int32 and got.shape == (7, 4)
        assert np.array_equal(got, want), (call, got, want)
        assert int(s.counter) == call + 1
        if "maps" in c:
            classes |= {int(c["maps"][v][z, y, x]) for v, z, y, x in cen.tolist()}
    assert int(s._state[1]) == 0                                           # the draw kernel's ticket is back at zero
    if "maps" in c:
        assert classes == {i for i, p in enumerate(c["probs"]) if p > 0}   # the 56 draws met every class that can be drawn


def test_many_samples_take_more_than_one_workgroup_and_other_seeds_draw_otherwise():
    imgs, tgts = _blank(EXT)
    a, b = _S(imgs, tgts, (4, 8, 16), batch_size=1003, seed=11), _S(imgs, tgts, (4, 8, 16), batch_size=1003, seed=12)
    a(), b()
    assert np.array_equal(a.last_origins.cpu().numpy(), SR.draw(11, 0, 1003, EXT, (4, 8, 16)))
    assert not torch.equal(a.last_origins, b.last_origins)
    first = a.last_origins.clone()
    a()
    assert not torch.equal(a.last_origins, first) and int(a.counter) == 2 and int(a._state[1]) == 0


def test_captured_call_draws_anew_at_every_replay():
    """A captured call replayed three times gives the twin's origins of three consecutive counters, and their windows."""
    imgs = [_volume(e, 1, torch.float32, 10 + v) for v, e in enumerate(EXT)]
    tgts = [_volume(e, 1, torch.uint8, 20 + v) for v, e in enumerate(EXT)]
    patch, B = (4, 8, 16), 7
    s = _S([a.cuda() for a in imgs], [a.cuda() for a in tgts], patch, batch_size=B, seed=77)
    xo, to = torch.empty(B, *patch, 1, device="cuda"), torch.empty(B, *patch, 1, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s(out=(xo, to))                                                    # counter 0, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s(out=(xo, to))
    assert int(s.counter) == 1                                             # capturing ran nothing
    for i in range(3):
        g.replay()
        want = SR.draw(77, 1 + i, B, EXT, patch)
        assert np.array_equal(s.last_origins.cpu().numpy(), want)
        wx, wt = SR.gather(imgs, tgts, want, patch)
        assert torch.equal(xo.cpu(), wx) and torch.equal(to.cpu(), wt)
        assert int(s.counter) == i + 2


# ---- 3. frequencies ---------------------------------------------------------------------------------------------------------------------------------------
def _device_draws(seed, extents, patch, class_maps=None, class_probs=None):
    imgs, tgts = _blank(extents)
    kw = dict(class_maps=[torch.from_numpy(m).cuda() for m in class_maps], class_probs=class_probs) if class_maps is not None else {}
    s = _S(imgs, tgts, patch, batch_size=SR.FREQ_B, seed=seed, **kw)
    out = []
    for _ in range(SR.FREQ_CALLS):
        s()
        out.append(s.last_origins.cpu().numpy())
    return np.concatenate(out)


def test_uniform_frequencies_of_device_draws():
    """The CPU file's test on device draws: 16,384 draws over 26 origins, five sigma per origin."""
    worst = SR.check_frequencies(_device_draws(SR.FREQ_SEED_UNIFORM, **SR.FREQ_UNIFORM), SR.uniform_cells(**SR.FREQ_UNIFORM))
    print("uniform mode on the device, worst |count - N p| / (5 sigma):", worst)


def test_class_frequencies_of_device_draws():
    case = SR.freq_class_case()
    worst = SR.check_frequencies(_device_draws(SR.FREQ_SEED_CLASS, **case), SR.class_cells(**case))
    print("class mode on the device, worst |count - N p| / (5 sigma):", worst)


# ---- 4. past 2^31 voxels -----------------------------------------------------------------------------------------------------------------------------------
def test_volume_of_more_than_2_31_voxels():
    """One uint8 volume of 1300^3 = 2.197e9 voxels with markers in its last planes: two patches whose rows start past voxel 2^31 (one at an odd
    x0), bit for bit."""
    N, patch = 1300, (3, 5, 64)
    try:
        img = torch.zeros(N, N, N, 1, dtype=torch.uint8, device="cuda")
        tgt = torch.zeros(N, N, N, 1, dtype=torch.uint8, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(0)
        img[N - 3:] = torch.randint(1, 256, (3, N, N, 1), generator=g, device="cuda", dtype=torch.uint8)
        tgt[N - 3:] = torch.randint(1, 256, (3, N, N, 1), generator=g, device="cuda", dtype=torch.uint8)
        org = [(0, N - 3, N - 5, N - 64), (0, N - 3, N - 7, 1101)]
        assert ((N - 3) * N + N - 7) * N + 1101 > 2 ** 31
        s = _S(img, tgt, patch, batch_size=2, seed=1)
        x, t = s(origins=torch.tensor(org, dtype=torch.int32, device="cuda"))
        tail_i, tail_t = img[N - 3:].cpu(), tgt[N - 3:].cpu()
        for b, (_, z0, y0, x0) in enumerate(org):
            wi, wt = tail_i[:, y0:y0 + 5, x0:x0 + 64], tail_t[:, y0:y0 + 5, x0:x0 + 64]
            assert wi.min() >= 1                                           # markers, not the zeros of a wrapped offset
            assert torch.equal(x[b].cpu(), wi.float()) and torch.equal(t[b].cpu(), wt), b
        s()                                                                # a drawn call stays inside the volume
        o = s.last_origins.cpu().numpy()
        assert np.array_equal(o, SR.draw(1, 0, 2, [(N, N, N)], patch))
    finally:
        img = tgt = s = x = t = None
        torch.cuda.empty_cache()


# ---- 5. train_one_epoch ---------------------------------------------------------------------------------------------------------------------------------------
AUG = dict(rot90=True, zflip=True, vflip=True, hflip=True, brightness=(-0.1, 0.3), contrast=(-0.2, 0.2), gaussian_noise=(0.01, 0.05),
           cutout=dict(n=(1, 4), size=(0.05, 0.3), cval=0.5))


class _Losses:
    """A log_writer that keeps what train_one_epoch reports per window - with sync_every = 1, the loss of every step."""

    def __init__(self):
        self.losses = []

    def update(self, head=None, **kw):
        if head == "loss":
            self.losses.append(kw["loss"])


def _epoch(data_loader):
    from biapy_amd import train_engine as TE
    from biapy_amd.augment import DeviceAugmenter
    from biapy_amd.losses import BCEWithLogitsLoss
    from biapy_amd.resunet import ResUNet

    torch.manual_seed(0)
    m = ResUNet(image_shape=(32, 32, 32, 1), activation="elu", feature_maps=[16, 32], drop_values=[0.0, 0.0], normalization="in", yx_down=[2],
                z_down=[2], isotropy=[True, True], larger_io=False, conv_layers=[2, 2], compute_dtype=torch.float32).cuda().train()
    cfg = types.SimpleNamespace(DATA=types.SimpleNamespace(PATCH_SIZE=(32, 32, 32, 1)),
                                TRAIN=types.SimpleNamespace(GRADIENT_CLIP_NORM=0.0, LR_SCHEDULER=types.SimpleNamespace(NAME=""), VERBOSE=False))
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, capturable=True)
    log = _Losses()
    TE.train_one_epoch(cfg, m, None, BCEWithLogitsLoss(), None, None, data_loader, [opt], torch.device("cuda"), 0, log_writer=log, loss_names=["loss"],
                       graph="on", sync_every=1, augment=DeviceAugmenter(seed=31, **AUG))
    torch.cuda.synchronize()
    assert hasattr(m, "_bpx_graph_step")
    return log.losses


def test_train_one_epoch_fed_by_the_device_loader():
    """sampler -> augmenter -> replayed step: the per-step losses of an epoch fed by ``DevicePatchLoader`` equal, bit for bit, those of an epoch fed
    from a plain list of the batches the twin's origins select, with the same augmenter seed."""
    from biapy_amd.sampler import DevicePatchLoader

    ext, patch, B, steps = [(40, 48, 56), (33, 32, 47)], (32, 32, 32), 2, 4
    g = torch.Generator().manual_seed(5)
    imgs = [torch.randn(*e, 1, generator=g) for e in ext]
    tgts = [(torch.rand(*e, 1, generator=g) > 0.5).float() for e in ext]
    s = _S([a.cuda() for a in imgs], [a.cuda() for a in tgts], patch + (1,), batch_size=B, seed=9)
    loader = DevicePatchLoader(s, steps)
    assert len(loader) == steps
    fed = _epoch(loader)
    assert int(s.counter) == steps
    plain = [SR.gather(imgs, tgts, SR.draw(9, step, B, ext, patch), patch) for step in range(steps)]
    want = _epoch(plain)
    print("per-step losses, device loader:", fed, "plain list:", want)
    assert len(fed) == len(want) == steps and all(np.isfinite(v) for v in fed)
    assert fed == want
    assert len(set(fed)) == steps                                          # four different batches

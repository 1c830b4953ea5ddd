"""CPU-side tests: the C-ABI library loads and exports every symbol the header declares, host geometry, module schema."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from biapy_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    declared = set(re.findall(r"\b(bpx_[a-zA-Z0-9_]+)\s*\(", hdr))
    declared = {d for d in declared if not d.startswith("bpx_PK") and d != "bpx_BF16"}
    declared = {d for d in declared if not d.startswith("bpx_stream")}
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(_lib.lib, name), f"{name} declared in include/biapy_amd.h but not exported by libbiapy_amd.so"
    assert set(_lib.EXPORTS) <= declared | {"bpx_debug_set_wgrad_tr"}
    assert _lib.lib.bpx_version() >= 100


def test_host_grid_matches_oracle(tiling_golden):
    from biapy_amd import tiling
    from oracle import tiling_oracle as T

    for name in ["c48", "docstring", "cfg3_1024", "template_pad10", "aniso", "odd", "single"]:
        a = tiling_golden[f"coords/{name}/args"]
        ov = tuple(float(v) for v in tiling_golden[f"coords/{name}/overlap"])
        g = tiling.crop_grid(a[0:3], a[4:7], ov, a[8:11])
        starts = [[tiling._start(g[ax], i) for i in range(g[ax].n)] for ax in range(3)]
        ref = tiling_golden[f"coords/{name}/coords"]
        assert sorted(set(ref[:, 0])) == sorted(set(starts[0]))
        assert sorted(set(ref[:, 2])) == sorted(set(starts[1]))
        assert sorted(set(ref[:, 4])) == sorted(set(starts[2]))
        assert len(ref) == g[0].n * g[1].n * g[2].n
    np.testing.assert_array_equal(tiling.taper_1d(128, 68), T.taper_1d(128, 68))


def test_dropin_argument_errors_match_reference():
    from biapy_amd import tiling

    v = np.zeros((16, 16, 16, 1), np.float32)
    with pytest.raises(ValueError, match="4 dimensional"):
        tiling.crop_3D_data_with_overlap(v[..., 0], (8, 8, 8, 1), verbose=False)
    with pytest.raises(ValueError, match="Padding"):
        tiling.crop_3D_data_with_overlap(v, (8, 8, 8, 1), padding=(4, 0, 0), verbose=False)
    with pytest.raises(ValueError, match="greater than"):
        tiling.crop_3D_data_with_overlap(v, (32, 8, 8, 1), verbose=False)
    with pytest.raises(ValueError, match="overlap"):
        tiling.crop_3D_data_with_overlap(v, (8, 8, 8, 1), overlap=(1.0, 0, 0), verbose=False)
    with pytest.raises(AssertionError):
        tiling.merge_3D_data_with_overlap(v, (16, 16, 16, 1), verbose=False)
    coords = tiling.crop_3D_data_with_overlap(v, (8, 8, 8, 1), overlap=(0.5, 0.5, 0.5), verbose=False, load_data=False)
    assert len(coords) == 64 and coords[1].x_start == 3 and coords[-1].z_end == 16


def test_module_state_dict_schema(resunet_golden):
    from biapy_amd.resunet import ResUNet

    m = ResUNet(image_shape=(128, 128, 128, 1), activation="elu", feature_maps=[16, 32, 64, 128, 256], drop_values=[0.0] * 5,
                normalization="in", yx_down=[2] * 4, z_down=[2] * 4, isotropy=[True] * 5, larger_io=False, conv_layers=[2] * 5)
    keys = list(resunet_golden["cfg2/keys"])
    shapes = dict(zip(keys, resunet_golden["cfg2/shapes"]))
    sd = m.state_dict()
    assert list(sd.keys()) == keys
    assert all(str(tuple(v.shape)) == shapes[k] for k, v in sd.items())
    with pytest.raises(RuntimeError, match="MI355X"):
        m(torch.zeros(1, 1, 16, 16, 16))
    with pytest.raises(NotImplementedError):                                     # (larger_io: still outside the hot path)
        ResUNet(image_shape=(64, 64, 1), feature_maps=[16, 32], normalization="in", larger_io=True)
    m = ResUNet(image_shape=(64, 64, 1), feature_maps=[16, 32], normalization="in", larger_io=False)      # the reference's default drop_values = 0.1: accepted since round 4
    assert m.cfg.dropout == (0.1, 0.1)


def test_losses_fail_loudly_without_gpu():
    """The device losses have no CPU fallback (product path rule): CPU tensors raise."""
    import pytest
    import torch

    from biapy_amd import losses

    with pytest.raises(RuntimeError, match="MI355X only"):
        losses.DiceCELoss()(torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))
    with pytest.raises(RuntimeError, match="MI355X only"):      # per-sample Dice (round 6) runs on the same fused passes: no CPU fallback either
        losses.DiceLoss(batch_dice=False)(torch.zeros(2, 1, 4, 4, 4), torch.zeros(2, 1, 4, 4, 4))
    with pytest.raises(RuntimeError, match="MI355X only"):      # multi-class cross entropy (round 6): the reference's constructor, device passes only
        losses.CrossEntropyLoss_wrapper(num_classes=3, ndim=3, class_rebalance="manual", class_weights=[0.2, 0.5, 0.3])(torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))
    # the IoU metric object of the reference (metrics.py:138-232): same constructor; what the kernels do not reproduce is refused at construction
    m = losses.jaccard_index(num_classes=2, device="cpu", ndim=3)
    assert m.num_classes == 2 and m.ignore_index is None and losses.jaccard_index(num_classes=4, device="cpu", ndim=3, ignore_index=255).ignore_index == 255
    with pytest.raises(NotImplementedError):
        losses.jaccard_index(num_classes=2, device="cpu", t=0.3)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))
    with pytest.raises(NotImplementedError):                      # beyond eight class channels: refused, not computed wrongly
        losses.CrossEntropyLoss_wrapper(num_classes=9, ndim=3)(torch.zeros(1, 9, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))


def test_instance_channels_loss_refuses_what_it_does_not_reproduce():
    """channels whose reference loss is not the plain per-channel term must be refused at construction, not computed wrongly:
    flow channels (targets scaled by flow_target_scale, metrics.py:235-246, :1700-1705), a discretised 'Db' (11 prediction channels, CE),
    multi-width and masked channels; every accepted letter is a plain one-channel term."""
    from biapy_amd.losses import InstanceChannelsLoss

    InstanceChannelsLoss(channel_weights=(1, 1, 1), out_channels=["B", "C", "D"], losses_to_use=["bce", "bce", "mse"])
    InstanceChannelsLoss(channel_weights=(1, 1), out_channels=["F", "Db"], losses_to_use=["bce", "mse"], head_activations=["ce_sigmoid", "linear"])
    for ch in ("Gv", "Gh", "Gz", "R", "A"):
        with pytest.raises(NotImplementedError):
            InstanceChannelsLoss(channel_weights=(1, 1), out_channels=["F", ch], losses_to_use=["bce", "mse"], head_activations=["ce_sigmoid", "linear"])
    with pytest.raises(NotImplementedError):
        InstanceChannelsLoss(channel_weights=(1, 1), out_channels=["F", "Db"], losses_to_use=["bce", "bce"], channel_extra_opts={"Db": {"val_type": "discretize"}})
    with pytest.raises(NotImplementedError):
        InstanceChannelsLoss(channel_weights=(1, 1), out_channels=["F", "Dc"], losses_to_use=["bce", "mse"], head_activations=["ce_sigmoid", "linear"],
                             channel_extra_opts={"Dc": {"mask_values": True}})


def test_prepost_fails_loudly_without_gpu():
    import pytest
    import torch

    from biapy_amd import prepost

    with pytest.raises(RuntimeError, match="MI355X only"):
        prepost.threshold_otsu(torch.zeros(4, 4, 4))


# ---- train_engine: step drivers (row T) -------------------------------------------------------------------------------
def _train_loop_case(name):
    """The seeded toy problem of tests/golden/make_golden.py::train_loop_case (kept in step with it)."""
    import types

    torch.manual_seed(11)
    net = torch.nn.Sequential(torch.nn.Conv3d(1, 4, 3, padding=1), torch.nn.ELU(), torch.nn.Conv3d(4, 1, 1))
    g = torch.Generator().manual_seed(12)
    data = [(torch.randn(2, 4, 6, 6, 1, generator=g), (torch.rand(2, 4, 6, 6, 1, generator=g) > 0.5).float()) for _ in range(13)]
    val = [(torch.randn(2, 4, 6, 6, 1, generator=g), (torch.rand(2, 4, 6, 6, 1, generator=g) > 0.5).float()) for _ in range(4)]
    clip, sched = {"plain": (0.0, ""), "clip_onecycle": (0.05, "onecycle"), "plateau": (0.0, "reduceonplateau")}[name]
    cfg = types.SimpleNamespace(DATA=types.SimpleNamespace(PATCH_SIZE=(4, 6, 6, 1)),
                                TRAIN=types.SimpleNamespace(GRADIENT_CLIP_NORM=clip, LR_SCHEDULER=types.SimpleNamespace(NAME=sched), VERBOSE=False))
    return net, data, val, cfg


@pytest.mark.parametrize("name", ["plain", "clip_onecycle", "plateau"])
def test_train_one_epoch_and_evaluate_at_the_reference_call_site(name):
    """biapy_amd.train_engine.train_one_epoch / evaluate called EXACTLY as Base_Workflow.train calls the reference's
    (base_workflow.py:1070-1088, :1114-1126: positional cfg, optimizer / lr_scheduler lists, log_writer, memory_bank, total_iters,
    contrast_warmup_iters, loss_names) reproduce what the reference's own functions returned on the same seeded problem
    (tests/golden/train_loop_golden.npz, generated by importing biapy/engine/train_engine.py): every returned meter (loss, the
    metric the workflow's metric_function records, lr), the step index and the trained weights - incl. gradient clipping + the
    per-step one-cycle schedule and ReduceLROnPlateau driven by evaluate()."""
    from biapy_amd import train_engine as TE

    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "train_loop_golden.npz"))
    net, data, val, cfg = _train_loop_case(name)
    dev = torch.device("cpu")
    opt = torch.optim.AdamW(net.parameters(), lr=1e-2)
    sched = None
    if name == "clip_onecycle":
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=3e-2, total_steps=len(data) * 2)
    if name == "plateau":
        sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.5, patience=0, threshold=10.0)
    loss_fn = torch.nn.BCEWithLogitsLoss()

    def call(batch, is_train=False):
        return net(batch.permute(0, 4, 1, 2, 3))

    def prep(targets, batch):
        return targets.permute(0, 4, 1, 2, 3)

    def metric(outputs, targets, metric_logger=None):
        p_ = (torch.sigmoid(outputs) > 0.5).float()
        iou = ((p_ * targets).sum() / torch.clamp(((p_ + targets) > 0).float().sum(), min=1.0)).item()
        if metric_logger:
            metric_logger.meters["IoU"].update(iou)

    class Writer:
        def __init__(self):
            self.heads = []

        def update(self, head="scalar", step=None, **kw):
            self.heads.append((head, sorted(kw)))

    w = Writer()
    for epoch in range(3 if name == "plateau" else 2):
        stats, step = TE.train_one_epoch(
            cfg,
            model=net,
            model_call_func=call,
            loss_function=loss_fn,
            metric_function=metric,
            prepare_targets=prep,
            data_loader=data,
            optimizer=[opt],
            device=dev,
            epoch=epoch,
            log_writer=w,
            lr_scheduler=[sched],
            verbose=False,
            memory_bank=None,
            total_iters=0,
            contrast_warmup_iters=0,
            loss_names=["loss"],
        )
        ev = TE.evaluate(
            cfg,
            model=net,
            model_call_func=call,
            loss_function=loss_fn,
            metric_function=metric,
            prepare_targets=prep,
            epoch=epoch,
            data_loader=val,
            lr_scheduler=[sched],
            memory_bank=None,
            loss_names=["loss"],
        )
        assert step == int(gold[f"{name}/e{epoch}/step"])
        assert set(stats) == {"loss", "IoU", "lr"} and set(ev) == {"loss", "IoU"}
        for k, v in stats.items():
            assert abs(v - float(gold[f"{name}/e{epoch}/train/{k}"])) < 1e-6, (epoch, k, v)
        for k, v in ev.items():
            assert abs(v - float(gold[f"{name}/e{epoch}/val/{k}"])) < 1e-6, (epoch, k, v)
    for k, v in net.state_dict().items():
        assert np.allclose(v.numpy(), gold[f"{name}/w/{k}"], atol=1e-6), k
    assert ("loss", ["loss"]) in w.heads and ("opt", ["lr"]) in w.heads


def test_train_one_epoch_multiple_losses_and_optimizers():
    """The dict form of a loss (train_engine.py:152-158: {"losses": [...], "metrics": {...}}): one backward / step per loss with
    its own optimizer, one meter per loss name and per lr name (loss_x -> lr_x), precalculated metrics instead of metric_function."""
    from biapy_amd import train_engine as TE

    net, data, _, cfg = _train_loop_case("plain")
    ref, _, _, _ = _train_loop_case("plain")
    bce = torch.nn.BCEWithLogitsLoss()

    def two_of(n):
        def two(outputs, targets):                                      # two losses with separate autograd graphs
            return {"losses": [bce(outputs, targets), (n[2].weight ** 2).sum() + (n[2].bias ** 2).sum()], "metrics": {"m": 0.25}}
        return two

    def make(n):
        ps = list(n.parameters())
        return [torch.optim.SGD(ps[:2], lr=0.1), torch.optim.SGD(ps[2:], lr=0.05)]

    oa, ob = make(net), make(ref)
    stats, step = TE.train_one_epoch(cfg, net, lambda b, is_train=False: net(b.permute(0, 4, 1, 2, 3)), two_of(net), None,
                                     lambda t, b: t.permute(0, 4, 1, 2, 3), data, oa, torch.device("cpu"), 0, None, [None, None], False, None, 0, 0,
                                     ["loss_a", "loss_b"])
    tot = [0.0, 0.0]
    for x, t in data:                                                   # the reference loop, written out (train_engine.py:127-180)
        out = ref(x.permute(0, 4, 1, 2, 3))
        r = two_of(ref)(out, t.permute(0, 4, 1, 2, 3))
        for i, l in enumerate(r["losses"]):
            l.backward()
            ob[i].step()
            ob[i].zero_grad()
            tot[i] += l.item()
    assert step == 12 and set(stats) == {"loss_a", "loss_b", "m", "lr_a", "lr_b"}
    assert abs(stats["loss_a"] - tot[0] / 13) < 1e-6 and abs(stats["loss_b"] - tot[1] / 13) < 1e-6 and abs(stats["m"] - 0.25) < 1e-12
    assert abs(stats["lr_a"] - 0.1) < 1e-9 and abs(stats["lr_b"] - 0.05) < 1e-9


def test_train_one_epoch_error_behaviour():
    """Same failures as the reference: wrong patch shape -> ValueError with its message (train_engine.py:139-143); a non-finite
    loss -> sys.exit(1) (:160-164); plus the errors of the acceleration switches."""
    import types

    from biapy_amd import train_engine as TE

    net, data, _, cfg = _train_loop_case("plain")
    loss_fn = torch.nn.BCEWithLogitsLoss()
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    call, prep = (lambda b, is_train=False: net(b.permute(0, 4, 1, 2, 3))), (lambda t, b: t.permute(0, 4, 1, 2, 3))
    bad_cfg = types.SimpleNamespace(DATA=types.SimpleNamespace(PATCH_SIZE=(8, 6, 6, 1)), TRAIN=cfg.TRAIN)
    with pytest.raises(ValueError, match="different shape than 'DATA.PATCH_SIZE'"):
        TE.train_one_epoch(bad_cfg, net, call, loss_fn, None, prep, data[:2], [opt], torch.device("cpu"), 0, loss_names=["loss"])
    bad = list(data[:4])
    bad[1] = (bad[1][0] * float("nan"), bad[1][1])
    with pytest.raises(SystemExit) as e:
        TE.train_one_epoch(cfg, net, call, loss_fn, None, prep, bad, [opt], torch.device("cpu"), 0, loss_names=["loss"], sync_every=2)
    assert e.value.code == 1
    with pytest.raises(ValueError, match="graph='on'"):
        TE.train_one_epoch(cfg, net, call, loss_fn, None, prep, data[:1], [opt], torch.device("cpu"), 0, loss_names=["loss"], graph="on")
    with pytest.raises(NotImplementedError, match="memory_bank"):
        TE.train_one_epoch(cfg, net, call, loss_fn, None, prep, data[:1], [opt], torch.device("cpu"), 0, memory_bank=object(), loss_names=["loss"])


def test_graph_lr_tensors_follow_schedulers_and_assignments():
    """graphs._LrTensors (a float lr is baked into a captured optimizer step): the learning rates become tensors that
    PyTorch's schedulers update in place, and a plain assignment ``group["lr"] = v`` is folded back into the captured tensor."""
    from biapy_amd.graphs import _LrTensors

    net = torch.nn.Linear(3, 2)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-2)
    lt = _LrTensors(opt, "cpu")
    t = opt.param_groups[0]["lr"]
    assert torch.is_tensor(t) and t is lt.lrs[0] and abs(t.item() - 1e-2) < 1e-9
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.5, patience=0)
    sched.step(1.0)
    sched.step(2.0)                                                     # worse: halves the lr - in place
    assert opt.param_groups[0]["lr"] is t and abs(t.item() - 5e-3) < 1e-9
    opt.param_groups[0]["lr"] = 1e-3                                    # what the reference's warm-up schedules do
    lt.sync()
    assert opt.param_groups[0]["lr"] is t and abs(t.item() - 1e-3) < 1e-9


def test_chunk_grid_rank_partition_covers_every_chunk_once():
    """ChunkedPredictor's ownership rule (a sampler pad-repeat is left to the rank holding the chunk's first occurrence): over all
    ranks every chunk is written exactly once and the written regions tile the volume, for ragged grids and world sizes that do
    not divide the chunk count."""
    from biapy_amd.chunked import ChunkGrid

    for dim, crop, pad in (((33, 47, 129), (16, 32, 64), (3, 5, 10)), ((18, 33, 65), (16, 32, 64), (6, 12, 24)), ((40, 64, 64), (32, 32, 32), (0, 0, 0))):
        grid = ChunkGrid(dim, crop, pad)
        for world in (1, 2, 3, 7, 8, 16):
            owned = []
            for rank in range(world):
                owned += [v for k, v in enumerate(grid.rank_order(world, rank)) if rank + k * world < grid.total]
            assert sorted(owned) == list(range(grid.total)), (dim, world)
        cover = np.zeros(dim, np.int32)
        for v in range(grid.total):
            r = grid.region(v)
            cover[r[3]:r[3] + r[6], r[4]:r[4] + r[7], r[5]:r[5] + r[8]] += 1
            t = grid.index_tables(v)
            assert len(t) == sum(crop) and t.min() >= 0 and (t[:crop[0]] < dim[0]).all() and (t[crop[0]:crop[0] + crop[1]] < dim[1]).all()
        assert (cover == 1).all()


def test_work_tiles_partition_the_chunk_grid():
    """chunked.TileGrid (TEST.BY_CHUNKS.WORKFLOW_PROCESS tiles, chunked_test_pair_data_generator.py:331-357): every chunk in exactly one tile,
    tile write regions tile the volume, a tile's read region contains the read regions of its chunks, ranks get disjoint tile lists."""
    from biapy_amd.chunked import ChunkGrid, TileGrid

    for dim, crop, pad, ppt in (((70, 64, 90), (32, 32, 32), (4, 4, 4), (2, 1, 2)), ((33, 50, 41), (16, 24, 16), (2, 0, 5), (3, 2, 1)),
                                ((64, 64, 64), (32, 32, 32), (0, 0, 0), (1, 1, 1))):
        g = ChunkGrid(dim, crop, pad)
        t = TileGrid(g, ppt)
        seen = sorted(v for tid in t.tile_ids for v in t.patches_of_tile[tid])
        assert seen == list(range(g.total))
        cov = np.zeros(dim, np.int32)
        for tid in t.tile_ids:
            w, r = t.write_region(tid), t.read_region(tid)
            cov[w.z_start:w.z_end, w.y_start:w.y_end, w.x_start:w.x_end] += 1
            for v in t.patches_of_tile[tid]:
                _, _, _, ext, real = g.patch_coords(v)
                assert r.z_start <= ext.z_start and ext.z_end <= r.z_end and r.y_start <= ext.y_start and ext.y_end <= r.y_end
                assert r.x_start <= ext.x_start and ext.x_end <= r.x_end
                assert w.z_start <= real.z_start and real.z_end <= w.z_end and w.x_start <= real.x_start and real.x_end <= w.x_end
                tab = g.index_tables(v)
                assert tab[: crop[0]].min() >= r.z_start and tab[: crop[0]].max() < r.z_end          # the reflection stays inside the tile's read region
        assert cov.min() == 1 and cov.max() == 1
        for world in (1, 2, 3, 5):
            lists = [t.rank_order(world, r) for r in range(world)]
            assert sorted(v for l in lists for v in l) == t.tile_ids


def test_lift_params_is_the_same_convolution():
    """engine.lift_params / unlift_grads (2D and (1,3,3) weights -> zero-padded 3x3x3): the lifted weights compute the same
    convolution on a one-slice / any volume, and gradients map back to the centre z-tap - checked with PyTorch's CPU convs."""
    import torch.nn.functional as F

    from biapy_amd.engine import lift_params, needs_lift, unlift_grads

    g = torch.Generator().manual_seed(0)
    P = {"c2d": torch.randn(5, 3, 3, 3, generator=g), "aniso": torch.randn(4, 3, 1, 3, 3, generator=g), "iso": torch.randn(4, 3, 3, 3, 3, generator=g),
         "ct2d": torch.randn(3, 5, 2, 2, generator=g), "k1": torch.randn(6, 3, 1, 1, generator=g), "bias": torch.randn(5, generator=g)}
    assert [needs_lift(v) for v in P.values()] == [True, True, False, True, True, False]
    Q = lift_params(P)
    assert Q["iso"] is P["iso"] and Q["bias"] is P["bias"] and Q["c2d"].shape == (5, 3, 3, 3, 3) and Q["ct2d"].shape == (3, 5, 1, 2, 2)
    x2 = torch.randn(2, 3, 9, 11, generator=g)
    assert torch.allclose(F.conv3d(x2.unsqueeze(2), Q["c2d"], padding=1)[:, :, 0], F.conv2d(x2, P["c2d"], padding=1), atol=1e-6)
    x3 = torch.randn(2, 3, 5, 9, 11, generator=g)
    assert torch.allclose(F.conv3d(x3, Q["aniso"], padding=1), F.conv3d(x3, P["aniso"], padding=(0, 1, 1)), atol=1e-6)
    assert torch.allclose(F.conv_transpose3d(x2.unsqueeze(2), Q["ct2d"], stride=(1, 2, 2))[:, :, 0], F.conv_transpose2d(x2, P["ct2d"], stride=2), atol=1e-6)
    G = {k: torch.randn(v.shape, generator=g) for k, v in Q.items()}
    U = unlift_grads(G, P)
    assert all(U[k].shape == P[k].shape for k in P)
    assert torch.equal(U["c2d"], G["c2d"][:, :, 1]) and torch.equal(U["aniso"][:, :, 0], G["aniso"][:, :, 1]) and torch.equal(U["k1"], G["k1"][:, :, 0])


@pytest.mark.parametrize("dim,d", [((10, 13, 16), 3), ((8, 8, 8), 6), ((5, 20, 7), 2)])
def test_dilated_conv_is_conv_on_sublattices(dim, d):
    """biapy_amd.dilation.lattice_tables: gathering the d^3 sub-lattices into the batch (zeros where a table says -1), an ordinary
    'same' 3x3x3 convolution and the inverse scatter reproduce torch's dilated convolution (padding = dilation) - the property the
    device path of ASPP (heads.py:77-104) rests on.  NumPy stands in for the two HIP kernels here."""
    import torch.nn.functional as F

    from biapy_amd.dilation import lattice_shape, lattice_tables

    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 3, *dim, generator=g)
    w = torch.randn(4, 3, 3, 3, 3, generator=g)
    ref = F.conv3d(x, w, padding=d, dilation=d)
    T = lattice_tables(dim, d)
    nz, ny, nx = lattice_shape(dim, d)
    assert T.shape == (d ** 3, nz + ny + nx)
    xs = torch.zeros(2 * d ** 3, 3, nz, ny, nx)
    for n in range(2):
        for q in range(d ** 3):
            tz, ty, tx = T[q, :nz], T[q, nz:nz + ny], T[q, nz + ny:]
            sub = x[n][:, np.clip(tz, 0, None)][:, :, np.clip(ty, 0, None)][:, :, :, np.clip(tx, 0, None)].clone()
            sub[:, tz < 0] = 0
            sub[:, :, ty < 0] = 0
            sub[:, :, :, tx < 0] = 0
            xs[n * d ** 3 + q] = sub
    ys = F.conv3d(xs, w, padding=1)
    out = torch.zeros_like(ref)
    for n in range(2):
        for q in range(d ** 3):
            tz, ty, tx = T[q, :nz], T[q, nz:nz + ny], T[q, nz + ny:]
            kz, ky, kx = np.where(tz >= 0)[0], np.where(ty >= 0)[0], np.where(tx >= 0)[0]
            out[n][:, tz[kz][:, None, None], ty[ky][None, :, None], tx[kx][None, None, :]] = ys[n * d ** 3 + q][:, kz][:, :, ky][:, :, :, kx]
    assert torch.allclose(out, ref, atol=1e-5)


@pytest.mark.parametrize("dim,d", [((10, 13, 16), 3), ((8, 8, 8), 6), ((5, 20, 7), 2), ((10, 10, 10), 18)])
def test_dilated_conv_is_one_conv_of_the_packed_volume(dim, d):
    """biapy_amd.dilation.packed_tables (the layout the ResUNet++ engine uses): the d^3 sub-lattices side by side with one zero plane
    between them; ONE 'same' 3x3x3 convolution of that volume, read back through the same tables, is torch's dilated convolution,
    and so are its input and weight gradients (zero separators contribute nothing)."""
    import torch.nn.functional as F

    from biapy_amd.dilation import lattice_shape, packed_shape, packed_tables

    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, *dim, generator=g, requires_grad=True)
    w = torch.randn(4, 3, 3, 3, 3, generator=g, requires_grad=True)
    gy = torch.randn(2, 4, *dim, generator=g)
    ref = F.conv3d(x, w, padding=d, dilation=d)
    gx_ref, gw_ref = torch.autograd.grad(ref, (x, w), gy)
    T = packed_tables(dim, d)
    P = packed_shape(dim, d)
    assert T.shape == (1, sum(P)) and P == tuple(d * (n + 1) - 1 for n in lattice_shape(dim, d))
    tz, ty, tx = T[0, :P[0]], T[0, P[0]:P[0] + P[1]], T[0, P[0] + P[1]:]
    for t, lim in zip((tz, ty, tx), dim):
        assert sorted(t[t >= 0].tolist()) == list(range(lim))                  # every source index exactly once
    kz, ky, kx = (torch.from_numpy(np.where(t >= 0)[0]) for t in (tz, ty, tx))
    sz, sy, sx = (torch.from_numpy(t[t >= 0].astype(np.int64)) for t in (tz, ty, tx))

    def pack(v):
        out = torch.zeros(v.shape[:2] + P, dtype=v.dtype)
        out[:, :, kz[:, None, None], ky[None, :, None], kx[None, None, :]] = v[:, :, sz[:, None, None], sy[None, :, None], sx[None, None, :]]
        return out

    def unpack(v):
        out = torch.zeros(v.shape[:2] + tuple(dim), dtype=v.dtype)
        out[:, :, sz[:, None, None], sy[None, :, None], sx[None, None, :]] = v[:, :, kz[:, None, None], ky[None, :, None], kx[None, None, :]]
        return out

    xp = pack(x.detach()).requires_grad_(True)
    wp = w.detach().clone().requires_grad_(True)
    yp = F.conv3d(xp, wp, padding=1)
    assert torch.allclose(unpack(yp.detach()), ref.detach(), atol=1e-5)
    gxp, gwp = torch.autograd.grad(yp, (xp, wp), pack(gy))
    assert torch.allclose(unpack(gxp), gx_ref, atol=1e-5)
    assert torch.allclose(gwp, gw_ref, atol=1e-4)


def test_chunk_planar_buffer_views():
    """_lib.Planar (bpx_tensor.cs != 0): the (C/16, B, D, H, W, 16) planes round-trip a dense NDHWC tensor, and channel slices are
    whole chunks addressed by (plane pointer, voxel pitch 16, plane stride) - what the kernels read as v*ld + (c/16)*cs + c%16."""
    from biapy_amd import _lib as L

    x = torch.randn(2, 3, 4, 5, 48)
    p = L.Planar(2, (3, 4, 5), 48, torch.float32, "cpu").copy_from_dense(x)
    assert torch.equal(p.dense(), x) and p.shape == (2, 3, 4, 5, 48)
    t = L.tview(p, 16, 32)
    assert (t.ld, t.C, t.cs) == (16, 32, p.plane) and t.ptr == p.t.data_ptr() + p.plane * 4
    flat = p.t.reshape(-1) if p.t.is_contiguous() else p._flat
    v, c = 37, 29                                              # voxel 37 of the (2,3,4,5) grid, channel 29 = chunk 1, lane 13
    assert flat[v * 16 + (c // 16) * p.plane + c % 16] == x.reshape(-1, 48)[v, c]
    with pytest.raises(AssertionError):
        L.tview(p, 8, 16)                                       # slices are whole 16-channel chunks
    d = L.tview(x, 8, 16)
    assert (d.ld, d.C, d.cs) == (48, 16, 0)


def test_modules_take_the_keyword_arguments_build_model_passes():
    """SURVEY 8b, model registry: ``biapy.models.build_model`` calls ``ResUNet(**args)`` / ``ResUNetPlusPlus(**args)`` with a fixed set of
    22-24 keyword arguments (models/__init__.py:120-179).  tests/golden/build_model_kwargs.json holds what the reference's own
    ``build_model`` handed to a recorder class placed where INTEGRATION.md places the MI355X classes (cfg 2, cfg 4, super-resolution):
    the drop-ins must construct from exactly those and expose the reference's parameter counts."""
    import json

    from biapy_amd.resunet import ResUNet
    from biapy_amd.resunetpp import ResUNetPlusPlus

    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "build_model_kwargs.json")))
    m = ResUNet(**{k: (tuple(v) if k in ("image_shape", "upsampling_factor") else v) for k, v in rec["cfg2_resunet"].items()})
    assert sum(p.numel() for p in m.parameters()) == 6693777 and len(m.state_dict()) == 98
    mpp = ResUNetPlusPlus(**{k: (tuple(v) if k == "image_shape" else v) for k, v in rec["cfg4_resunet++"].items()})
    assert sum(p.numel() for p in mpp.parameters()) == 11148710
    msr = ResUNet(**{k: (tuple(v) if k in ("image_shape", "upsampling_factor") else v) for k, v in rec["sr_resunet"].items()})
    assert any(k.startswith("pre_upsampling.") for k in msr.state_dict())
    # round 4: the MODEL lines of two of the reference's own 3-D ResUNet templates (widths beyond powers of two) - the reference's build_model kwargs,
    # and the REFERENCE class's parameter counts for them, recorded by the same script
    counts = rec["_reference_parameter_counts"]
    assert counts["cfg2_resunet"] == 6693777
    for name, padded in (("ovarian_reserve_resunet", None), ("cartocell_resunet", [64, 80, 96])):
        kw = {k: (tuple(v) if k in ("image_shape", "upsampling_factor") else v) for k, v in rec[name].items()}
        mt = ResUNet(**kw)
        assert sum(p.numel() for p in mt.parameters()) == counts[name], name        # parameters in the reference's shapes (padding happens inside the engine)
        assert (list(mt.cfg.feature_maps) == padded) if padded else (mt.cfg.true_feature_maps is None), name
        assert sum(mt.output_channels) == 3 and mt.heads[0].weight.shape[:2] == (3, kw["feature_maps"][0])


def test_epoch_drivers_refuse_a_model_call_func_beside_a_loss_that_fuses_the_head_activations():
    """InstanceChannelsLoss applies tanh to the 'D' channel inside its kernel; the reference's model_call_func applies it too (base_workflow.py:1403-1457):
    together they would do it twice without any error.  train_one_epoch / evaluate refuse the pair unless the function says it returns raw logits."""
    from biapy_amd import train_engine as TE

    class _Loss:
        fused_head_activations = ["ce_sigmoid", "ce_sigmoid", "tanh"]

    def mcf(batch, is_train=True):
        return batch

    with pytest.raises(ValueError, match="raw output"):
        TE._check_fused_activations(mcf, _Loss())
    TE._check_fused_activations(None, _Loss())                      # the default call is the identity around the model
    mcf.returns_raw_logits = True
    TE._check_fused_activations(mcf, _Loss())

    class _Plain:
        fused_head_activations = ["ce_sigmoid", "linear"]           # nothing is applied at training time: any model_call_func is fine
    mcf2 = lambda b, is_train=True: b                               # noqa: E731
    TE._check_fused_activations(mcf2, _Plain())
    TE._check_fused_activations(mcf2, object())


def _tta_spec_of(T, ndim, cout, groups):
    """biapy_amd.tta's spec dataclasses from the plain descriptions of oracle/tta_oracle.spec_cases()."""
    out = []
    for g in groups:
        if g["kind"] == "scalar":
            out.append(T.ScalarChannels(channels=tuple(g["channels"])))
        elif g["kind"] == "vector":
            out.append(T.VectorChannels(axis_channels=tuple(g["axis_channels"]), signed=g["signed"], axis_scale=None if g["axis_scale"] is None else tuple(g["axis_scale"])))
        elif g["kind"] == "rays":
            out.append(T.RayChannels(start=g["start"], dirs=np.asarray(g["dirs"])))
        else:
            out.append(T.AffinityChannels(layout=dict(g["layout"])))
    return T.TTASpec(ndim=ndim, n_channels=cout, groups=out)


def test_tta_spec_host_logic_matches_the_reference(tta_spec_golden):
    """The product's orientation filter and mode-reducible channel list (host logic of biapy_amd.tta) against what the reference's TTASpec kept."""
    from biapy_amd import tta as T
    from oracle import tta_oracle as TO

    for name, shape, ndim, cout, groups in TO.spec_cases():
        spec = _tta_spec_of(T, ndim, cout, groups)
        for level in ("full", "flips"):
            kept = T.filter_orientations(spec, T.build_axis_transform_group(ndim, level))
            np.testing.assert_array_equal(np.array([list(p) + list(s) for p, s in kept]), tta_spec_golden[f"{name}/kept/{level}"], err_msg=f"{name} {level}")
        assert T._mode_reducible(spec) == TO.mode_reducible_channels(groups)
    with pytest.raises(NotImplementedError):
        T._kind(object())
    # the reference names vector groups after their family ("flow", "E_sigma", ...): the kind comes from the fields, not from the name
    assert T._kind(T.VectorChannels(axis_channels=(0, 1, 2), name="flow")) == "vector" and T._kind(T.RayChannels(name="stardist")) == "rays"
    assert T._kind(T.AffinityChannels(name="aff")) == "affinities" and T._kind(T.ScalarChannels(channels=(0,))) == "scalar"


def test_build_tta_spec_reproduces_the_reference(tta_spec_golden):
    """biapy_amd.tta.build_tta_spec / parse_model_output_channel_names (host logic) against the structures the reference's functions returned for the
    same channel-name lists (flows, HoVer maps incl. a z component on 2-D data, EmbedSeg offsets / sigmas with anisotropy, 2-D and 3-D rays,
    affinities, plain B/C/D): group order, classes, names and every field; ray directions to 1e-6."""
    import json

    from biapy_amd import tta as T
    from oracle import tta_oracle as TO

    for k, (names, ndim, extra, aniso) in enumerate(TO.BUILD_SPEC_CASES):
        want = json.loads(str(tta_spec_golden[f"build/{k}"]))
        spec = T.build_tta_spec(names, ndim, extra, aniso)
        assert (spec.ndim, spec.n_channels, len(spec.groups)) == (want["ndim"], want["n_channels"], len(want["groups"])), names
        for g, w in zip(spec.groups, want["groups"]):
            assert type(g).__name__ == w["cls"] and g.name == w["name"], (names, g, w)
            if w["cls"] == "VectorChannels":
                assert list(g.axis_channels) == w["axis_channels"] and bool(g.signed) == w["signed"]
                assert (g.axis_scale is None) == (w["axis_scale"] is None) and (g.axis_scale is None or list(g.axis_scale) == w["axis_scale"])
            elif w["cls"] == "RayChannels":
                assert g.start == w["start"]
                np.testing.assert_allclose(np.asarray(g.dirs), np.asarray(w["dirs"]), atol=1e-6)
            elif w["cls"] == "AffinityChannels":
                assert sorted([a, o, c] for (a, o), c in g.layout.items()) == w["layout"]
            else:
                assert list(g.channels) == w["channels"]
    assert T.parse_model_output_channel_names(["Gv+Gh+B", "class"]) == json.loads(str(tta_spec_golden["parse/0"]))
    with pytest.raises(ValueError, match="contiguous"):
        T.build_tta_spec(["R_0", "B", "R_1"], 2)
    with pytest.raises(ValueError, match="nrays"):
        T.build_tta_spec(["R_0", "R_1"], 2, {"R": {"nrays": 4}})


def test_fused_adam_step_refuses_what_it_does_not_reproduce():
    """optim.fused_step touches nothing and answers False for host tensors, other optimizers and host-side step counters: the caller then
    runs torch's own ``optimizer.step()`` (train_engine.py:173-177)."""
    import torch
    from biapy_amd import optim as O

    p = [torch.nn.Parameter(torch.randn(8))]
    p[0].grad = torch.randn(8)
    for opt in (torch.optim.AdamW(p, lr=0.1), torch.optim.SGD(p, lr=0.1), torch.optim.Adam(p, lr=0.1, amsgrad=True)):
        opt.step()
        before = p[0].detach().clone()
        assert O.fused_step(opt) is False
        assert torch.equal(before, p[0])
        O.step(opt)                                   # falls through to torch
        assert not torch.equal(before, p[0])
    opt = torch.optim.AdamW(p, lr=0.1, capturable=False)
    assert O._has_step_hooks(opt) is False
    h = opt.register_step_post_hook(lambda o, a, k: None)    # hooks hang on optimizer.step(): the kernel path would skip them, so it declines
    assert O._has_step_hooks(opt) is True
    h.remove()
    assert O._has_step_hooks(opt) is False
    g = dict(opt.param_groups[0], capturable=True, betas=(torch.tensor(0.9), 0.999))
    assert O._group_ok(opt, g) is False                      # tensor-valued betas: refused before any launch


@pytest.mark.parametrize("s", [2, 3])
def test_rcan_upscale_stage_channel_orders_are_the_shuffles_adjoint(s):
    """Host algebra of the RCAN x-scale stage (rcan_engine.rows_to_/_from_subposition_major, gather_subpositions): the conv with its rows in the
    kernels' [sub-position][channel] order + the sub-position gather reproduce the oracle's conv + pixel_shuffle3d, and the stage's backward
    (gather the fine-grid gradient, the conv's weight / bias gradient per row, rows back to PyTorch's order) reproduces autograd through it."""
    import torch.nn.functional as F

    from biapy_amd.rcan_engine import gather_subpositions, rows_from_subposition_major, rows_to_subposition_major
    from oracle.rcan_oracle import pixel_shuffle3d

    g = torch.Generator().manual_seed(s)
    Fc, D, s3 = 4, 5, s ** 3
    x = torch.randn(2, Fc, D, D + 1, D + 2, generator=g, dtype=torch.float64)
    w = torch.randn(Fc * s3, Fc, 3, 3, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(Fc * s3, generator=g, dtype=torch.float64).requires_grad_(True)
    y = pixel_shuffle3d(F.conv3d(x, w, b, padding=1), s)
    r = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (y * r).sum().backward()
    wu, bu = rows_to_subposition_major(w.detach(), b.detach(), Fc, s3)
    cu = F.conv3d(x, wu, bu, padding=1)                                       # channels [sub-position][channel]
    B, _, Dz, Dy, Dx = cu.shape
    assert torch.equal(gather_subpositions(y.detach().permute(0, 2, 3, 4, 1).contiguous(), s), cu.permute(0, 2, 3, 4, 1).reshape(B, Dz, Dy, Dx, s3, Fc))
    dcu = gather_subpositions(r.permute(0, 2, 3, 4, 1).contiguous(), s).reshape(B, Dz, Dy, Dx, s3 * Fc).permute(0, 4, 1, 2, 3).contiguous()
    gwu = torch.nn.grad.conv3d_weight(x, wu.shape, dcu, padding=1)
    gw, gb = rows_from_subposition_major(gwu, dcu.sum((0, 2, 3, 4)), Fc, s3)
    assert torch.allclose(gw, w.grad, rtol=1e-10, atol=1e-10) and torch.allclose(gb, b.grad, rtol=1e-10, atol=1e-10)
    w2, b2 = rows_from_subposition_major(wu, bu, Fc, s3)
    assert torch.equal(w2, w.detach()) and torch.equal(b2, b.detach())


def test_bench_roofline_arithmetic_is_what_design_states():
    """bench.py's algorithmic bytes / FLOPs per launch (the numerators of `roofline.achieved`) for the shapes DESIGN.md section 6 quotes: every activation
    operand read once and the result written once; 2 FLOPs per MAC; the fused backward = the dgrad AND the wgrad of the conv; and the choice of the
    binding roof (bytes / 8 TB/s against FLOPs / the dense 16-bit MFMA peak)."""
    import bench

    vox = 4 * 128 ** 3
    fused = (4, 4, 128, 128, 128, "C16", "C48", 1, "C48")                        # dy 16 -> g 48 at the benched size (the line's `roofline` shape)
    assert bench.conv_bytes("bpx_conv3d_bwd_fused", fused, 2) == vox * (16 + 2 * 48) * 2 == 1879048192
    assert bench.conv_flops("bpx_conv3d_bwd_fused", fused) == 2 * 2 * vox * 27 * 16 * 48 == 695784701952
    fwd = (2, 4, 128, 128, 128, "C48", 1, "C0", "C16")
    assert bench.conv_bytes("bpx_conv3d_fwd", fwd, 2) == vox * (48 + 0 + 16) * 2
    assert bench.conv_flops("bpx_conv3d_fwd", fwd) == 2 * vox * 27 * 48 * 16
    fwd_sc = (2, 4, 128, 128, 128, "C16", 1, "C48", "C16")                      # + the fused 1x1x1 shortcut: csc more K per voxel, its input read once
    assert bench.conv_flops("bpx_conv3d_fwd", fwd_sc) == 2 * vox * (27 * 16 + 48) * 16
    assert bench.conv_bytes("bpx_conv3d_fwd", fwd_sc, 2) == vox * (16 + 48 + 16) * 2
    wg1 = (4, 4, 128, 128, 128, "C48", 0, "C16", 1, 802816)                      # k = 1 weight gradient (trailing int: a small workspace size)
    assert bench.wgrad_k(wg1) == 1 and bench.conv_flops("bpx_conv3d_wgrad", wg1) == 2 * vox * 48 * 16
    assert bench.conv_bytes("bpx_conv3d_wgrad", wg1, 2) == vox * (48 + 16) * 2
    assert bench.conv_flops("bpx_head_fwd", fused) == 0 and bench.conv_bytes("bpx_head_fwd", fused, 2) == 0
    assert bench._shape_name("bpx_conv3d_bwd_fused", fused) == "bpx_conv3d_bwd_fused[4x128^3 dy C16->g C48]"

    class Prof:                                                                   # what the per-launch HIP events hand to conv_roofline: {(entry, key): (launches, ms)}
        def summary(self):
            return {("bpx_conv3d_bwd_fused", fused): (5, 5 * 0.95), ("bpx_conv3d_fwd", fwd): (5, 5 * 0.58), ("bpx_head_fwd", (2, 4, "C16", 1, 1)): (5, 0.3)}

    head, top = bench.conv_roofline(Prof(), 5, "mix16", "test")
    assert head["kernel"].startswith("bpx_conv3d_bwd_fused") and head["launches"] == 5 and abs(head["avg_launch_ms"] - 0.95) < 1e-9
    tf, gb = 695784701952 / 0.95e-3 / 1e12, 1879048192 / 0.95e-3 / 1e9
    assert abs(head["tflops"] - tf) < 0.01 and abs(head["algorithmic_GBps"] - gb) < 0.1
    assert head["bound"] == "mfma" and abs(head["frac"] - tf / 2500.0) < 1e-3     # 0.29 of the MFMA roof outweighs 0.25 of the HBM roof
    assert abs(head["hbm_frac"] - gb / 8000.0) < 1e-3 and len(top) == 2 and "families" in head


def test_bench_dump_outputs_is_float32_sampled_and_bounded(tmp_path):
    """bench.py --dump-outputs: float32 .npy files, whole arrays kept whole, a large output reduced to the same seeded sample in every run, and a
    dump beyond the 64 MiB budget refused before anything is written."""
    import bench

    logits = torch.randn(2, 1, 40, 160, 170, generator=torch.Generator().manual_seed(0)).to(torch.float16)
    assert logits.numel() > bench.DUMP_SAMPLE
    params = torch.arange(1000, dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), whole=dict(loss=torch.tensor(0.25, requires_grad=True), params=params), sampled=dict(logits=logits))
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("loss", "params", "logits")}
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["loss"].shape == () and a["loss"] == 0.25 and np.array_equal(a["params"], params.numpy())
    flat = logits.reshape(-1).float().numpy()
    assert a["logits"].shape == (bench.DUMP_SAMPLE,) and np.isin(a["logits"], flat).all()
    assert np.array_equal(a["logits"], np.load(tmp_path / "b" / "logits.npy"))
    small = torch.randn(3, 4)
    bench.dump_outputs(str(tmp_path / "c"), whole={}, sampled=dict(y=small))
    assert np.array_equal(np.load(tmp_path / "c" / "y.npy"), small.reshape(-1).numpy())
    with pytest.raises(SystemExit, match="budget"):
        bench.dump_outputs(str(tmp_path / "big"), whole=dict(p=torch.zeros(bench.DUMP_MAX_BYTES // 4 + 1)), sampled={})
    assert not (tmp_path / "big").exists()


def test_bench_full_is_an_option_off_by_default():
    """bench.py --full: a plain `--gpus 1 --steps K --warmup W` run times the headline alone; everything else it measures or checks needs --full."""
    import bench

    ap = bench.arg_parser()
    assert ap.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"]).full is False
    assert ap.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1", "--full"]).full is True


def test_channel_pad_plan_covers_every_parameter_and_is_exact_on_the_oracle():
    """engine.channel_pad_plan / pad_channels / unpad_channel_grads (feature maps that are not multiples of 16, e.g. CartoCell's [52, 68, 84]): every
    parameter of the module has a plan entry, the padded tensors have exactly the shapes of the padded architecture, un-padding is the inverse, and
    - on the CPU oracle - the zero-padded network computes what the true-width network computes (a padded channel is written and read through zero weights)."""
    import torch

    from biapy_amd.engine import channel_pad_plan, pad_channels, unpad_channel_grads
    from biapy_amd.resunet import ResUNet
    from oracle import net_oracle

    kw = dict(image_shape=(8, 32, 32, 1), activation="elu", drop_values=[0.0] * 3, normalization="in", yx_down=[2, 2], z_down=[1, 2], isotropy=[True] * 3,
              larger_io=False, conv_layers=[2] * 3, output_channels=[2, 1], output_channel_info=["B", "C"])
    torch.manual_seed(3)
    m = ResUNet(feature_maps=[20, 36, 52], **kw)
    assert list(m.cfg.feature_maps) == [32, 48, 64] and tuple(m.cfg.true_feature_maps) == (20, 36, 52)
    plan = channel_pad_plan(m.cfg)
    P = {n: p.detach() + (0.1 if p.dim() == 1 else 0.0) for n, p in m.named_parameters()}
    assert all(k in plan for k in P if not k.endswith(".bias") or "heads" not in k)
    Q = pad_channels(P, plan)
    big = ResUNet(feature_maps=[32, 48, 64], **kw)
    assert {n: tuple(p.shape) for n, p in big.named_parameters()} == {n: tuple(q.shape) for n, q in Q.items()}
    back = unpad_channel_grads(Q, plan)
    assert all(torch.equal(back[n], P[n]) for n in P)
    x = torch.randn(1, 1, 8, 32, 32, generator=torch.Generator().manual_seed(4))
    y_true = net_oracle.resunet_forward(P, x, [20, 36, 52], z_down=[1, 2])
    y_pad = net_oracle.resunet_forward(Q, x, [32, 48, 64], z_down=[1, 2])
    assert (y_true - y_pad).abs().max().item() < 2e-5 * y_true.abs().max().item()
    assert channel_pad_plan(big.cfg) is None
    for act in ("sigmoid", "softplus"):                              # act(0) != 0: a padded channel holds a constant, and is read through zero weights
        ya = net_oracle.resunet_forward(P, x, [20, 36, 52], z_down=[1, 2], activation=act)
        yb = net_oracle.resunet_forward(Q, x, [32, 48, 64], z_down=[1, 2], activation=act)
        assert (ya - yb).abs().max().item() < 2e-5 * ya.abs().max().item(), act
    with pytest.raises(NotImplementedError):                         # GroupNorm groups would change with the padding
        ResUNet(feature_maps=[20, 36, 52], **dict(kw, normalization="gn"))


@pytest.mark.parametrize("tag", ["multiclass", "mask_then_softmax", "two_then_class"])
def test_explicit_activation_tail_follows_prepare_activation_layers(tag):
    """with explicit_activations the reference collects its activation list channel by channel and STOPS after the first softmax
    (prepare_activation_layers, blocks.py:2001-2051); one collected entry acts on the whole tensor (joint softmax of a multi-class head), several
    act on one-channel slices, channels behind the list stay raw (resunet.py:413-425).  The drop-in's tail is plain torch on the head kernel's
    logits, so it is held to the reference's own outputs here on the CPU (fixture: make_golden.py resunet_explicit_tail)."""
    import json

    from biapy_amd.resunet import ResUNet

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "resunet_explicit_tail_golden.npz"))
    kw = json.loads(str(g[f"{tag}/kwargs"]))
    m = ResUNet(image_shape=(8, 8, 8, 1), activation="elu", feature_maps=[16, 32], drop_values=[0.0] * 2, normalization="in", yx_down=[2], z_down=[2],
                explicit_activations=True, isotropy=[True] * 2, larger_io=False, conv_layers=[2] * 2, **kw)
    raw = {k: torch.from_numpy(g[f"{tag}/raw/{k}"]) for k in ("pred", "class") if f"{tag}/raw/{k}" in g.files}
    # the head kernel's logits: every head's rows in head order = pred and class channels interleaved by head
    n_out = sum(kw["output_channels"])
    logits = torch.empty((raw["pred"].shape[0], n_out) + tuple(raw["pred"].shape[2:]))
    logits[:, m._pred_channels] = raw["pred"]
    if "class" in raw:
        logits[:, m._class_channels] = raw["class"]
    out = m._finish_outputs(logits)
    out = out if isinstance(out, dict) else {"pred": out}
    for k in raw:
        ref = torch.from_numpy(g[f"{tag}/act/{k}"])
        assert out[k].shape == ref.shape and (out[k] - ref).abs().max().item() < 1e-6, (tag, k)
    if tag == "multiclass":          # the joint softmax: channels sum to one (a per-channel softmax would be all ones)
        assert (out["pred"].sum(1) - 1).abs().max().item() < 1e-5 and out["pred"].max().item() < 1.0


def test_fused_backward_plan_of_the_role_split_and_serial_forms():
    """Host side of bpx_conv3d_bwd_fused (no GPU: the planner assumes 256 CUs when there is no device): which shapes it takes, how many statistics
    rows per sample it writes and how much workspace it wants, for the role-split kernel (round 6: one 8-wave workgroup per CU for 48 channels, two
    for 16; one statistics row per D wave) and for the serial kernel behind the A/B mask."""
    from biapy_amd import _lib as L

    lib = L.lib
    N, S = 4, 128
    try:
        for mask, rows48, rows16, grid48, grid16 in ((3, 4 * 256, 4 * 512, 256, 512), (0, (S // 4) * (S // 4) * (S // 16), 768, 512, 768)):
            lib.bpx_debug_set_bwd_rs(mask)
            assert lib.bpx_conv3d_bwd_fused_supported(L.MIX16, N, S, S, S, 48, 16) == 1 and lib.bpx_conv3d_bwd_fused_supported(L.BF16, N, S, S, S, 16, 16) == 1
            assert lib.bpx_conv3d_bwd_fused_stats_tiles(N, S, S, S, 48, 16) == rows48          # serial 48-channel form: one row per 4 x 4 x 16 tile
            assert lib.bpx_conv3d_bwd_fused_stats_tiles(N, S, S, S, 16, 16) == rows16
            assert lib.bpx_conv3d_bwd_fused_workspace(N, S, S, S, 48, 16) == grid48 * (27 * 48 + 1) * 16 * 4
            assert lib.bpx_conv3d_bwd_fused_workspace(N, S, S, S, 16, 16) == grid16 * (27 * 16 + 1) * 16 * 4
        lib.bpx_debug_set_bwd_rs(3)
        # the dy.C == 32 shapes of level 1 stay on the serial kernel whatever the mask; unsupported: f32 storage, small volumes, other widths
        assert lib.bpx_conv3d_bwd_fused_supported(L.MIX16, N, 64, 64, 64, 32, 32) == 1 and lib.bpx_conv3d_bwd_fused_supported(L.MIX16, N, 64, 64, 64, 96, 32) == 0
        assert lib.bpx_conv3d_bwd_fused_supported(L.F32, N, S, S, S, 16, 16) == 0 and lib.bpx_conv3d_bwd_fused_supported(L.MIX16, 1, 16, 16, 16, 16, 16) == 0
        small = lib.bpx_conv3d_bwd_fused_stats_tiles(1, 32, 32, 32, 48, 16)      # 128 tiles: the grid is capped at the tile count (a multiple of 8)
        assert small == 4 * 128
    finally:
        lib.bpx_debug_set_bwd_rs(3)

"""What the affine warp of the device augmenter costs at 4 x 128^3 x 1 fp32 with a one-channel uint8 target, one call, the configurations
alternated, 40 repetitions per reading, three readings each (HIP events; the model of scripts/augment_timing.py):
  (a)   DeviceAugmenter with rotation, zoom, shear and shift on and da_prob = 1, nothing else: bpx_aug_draw + bpx_warp_draw + bpx_warp_apply into
        the scratch pair + bpx_aug_apply (a copy here) - eager, and captured alone in a HIP graph and replayed;
  (w)   bpx_warp_apply alone, replayed: the pass whose traffic floor is 84 MB (image and target read once and written once);
  (c)   the same transform from torch: F.affine_grid + F.grid_sample, z folded into the channels, bilinear image, nearest target.  grid_sample takes
        no uint8, so (c-u8) converts the target to float32 and back as a caller would have to, and (c-f32) is handed a float32 target and converts
        nothing; the condition is taken against the CHEAPER of the two;
  (e)   the cfg-2 train_one_epoch(graph="on") step with the augmenter (flips, rot90, intensity, cutout), with and without the affine options.
Conditions, written into the JSON with their verdicts: (a) lies below (c) by more than the largest spread of the readings, eager against eager and
replay against replay; the step's increase lies within (a) eager plus the spread.  Exit status 1 if one does not hold.
The ratio of (w) to its 84 MB floor at the 4.5 TB/s yardstick is reported as a number; back-to-back repetitions re-read the same 33.5 MB image,
which fits the last-level cache, so it is not an HBM figure.
Writes profiles/warp_timing.json.
python scripts/warp_timing.py [--steps 40] [--rounds 3] [--patch 128] [--batch 4]"""
import argparse
import json
import math
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from biapy_amd import _lib as L  # noqa: E402
from biapy_amd import train_engine as TE  # noqa: E402
from biapy_amd.augment import AFFINE_MODES, DeviceAugmenter  # noqa: E402
from biapy_amd.losses import BCEWithLogitsLoss  # noqa: E402
from biapy_amd.resunet import ResUNet  # noqa: E402

FM = [16, 32, 64, 128, 256]
YARDSTICK_TBPS = 4.5
AFFINE = dict(rotation=(-45, 45), zoom=(0.8, 1.25), shear=(-10, 10), shift=(-0.1, 0.1))
REST = dict(rot90=True, zflip=True, vflip=True, hflip=True, brightness=(-0.1, 0.1), contrast=(-0.1, 0.1), gaussian_noise=(0.01, 0.05),
            cutout=dict(n=(2, 2), size=(0.05, 0.3)))


def timed(fn, n, warm=1):
    """ms per call of n back-to-back calls between two HIP events (`warm` calls first)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def alternate(fns, steps, rounds):
    out = {k: [] for k in fns}
    for r in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, steps))
            print(f"round {r + 1} {k}: {out[k][-1]:.4f} ms", flush=True)
    return out


def summary(readings):
    return {k: dict(readings_ms=[round(v, 4) for v in vs], mean_ms=round(sum(vs) / len(vs), 4), spread_ms=round(max(vs) - min(vs), 4)) for k, vs in readings.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "warp_timing.py measures on the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda", 0)
    P, B = a.patch, a.batch
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((B, P, P, P, 1), device=dev, generator=g)
    t = (torch.rand((B, P, P, P, 1), device=dev, generator=g) > 0.5).float()
    t8 = t.to(torch.uint8)
    xo, to8 = torch.empty_like(x), torch.empty_like(t8)

    warp = DeviceAugmenter(da_prob=1.0, seed=1, **AFFINE)
    warp(x, t8, out=(xo, to8))                                             # one call: state, scratch and a drawn set of warp records
    wrec = warp.last_warp_records.clone()
    wx, wt8 = torch.empty_like(x), torch.empty_like(t8)

    def warp_pass():
        L.check(L.lib.bpx_warp_apply(x.data_ptr(), t8.data_ptr(), L.U8, B, P, P, P, 1, 1, wrec.data_ptr(), AFFINE_MODES["constant"], 0.0, wx.data_ptr(),
                                     wt8.data_ptr(), L.stream_ptr()))

    # torch: one 2x3 matrix per sample in grid_sample's normalised coordinates (a 30 degree turn, zoom 1.1, a small shift), z as channels
    ang = math.radians(30.0)
    theta = torch.tensor([[math.cos(ang) / 1.1, math.sin(ang) / 1.1, 0.05], [-math.sin(ang) / 1.1, math.cos(ang) / 1.1, -0.03]], device=dev).repeat(B, 1, 1)
    xv, tv, tv8 = x[..., 0], t[..., 0], t8[..., 0]                        # (B, Z, Y, X): N, C, H, W

    def torch_u8():
        grid = F.affine_grid(theta, xv.shape, align_corners=False)
        return (F.grid_sample(xv, grid, mode="bilinear", padding_mode="zeros", align_corners=False),
                F.grid_sample(tv8.float(), grid, mode="nearest", padding_mode="zeros", align_corners=False).to(torch.uint8))

    def torch_f32():
        grid = F.affine_grid(theta, xv.shape, align_corners=False)
        return (F.grid_sample(xv, grid, mode="bilinear", padding_mode="zeros", align_corners=False),
                F.grid_sample(tv, grid, mode="nearest", padding_mode="zeros", align_corners=False))

    fns = {
        "a warp call": lambda: warp(x, t8, out=(xo, to8)),
        "w bpx_warp_apply alone": warp_pass,
        "c-u8 torch affine_grid + grid_sample, uint8 target converted": torch_u8,
        "c-f32 torch affine_grid + grid_sample, float32 target": torch_f32,
    }

    def graphed(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            keep = fn()                                                    # the outputs stay alive with the graph's pool
        return lambda: gr.replay(), keep

    kept = []
    for k in list(fns):
        fn, keep = graphed(fns[k])
        kept.append(keep)
        fns["graph: " + k] = fn
    res = summary(alternate(fns, a.steps, a.rounds))
    torch.cuda.synchronize()

    # (e) the cfg-2 step through train_one_epoch(graph="on"), batches resident on the device
    cfg = types.SimpleNamespace(DATA=types.SimpleNamespace(PATCH_SIZE=(P, P, P, 1)),
                                TRAIN=types.SimpleNamespace(GRADIENT_CLIP_NORM=0.0, LR_SCHEDULER=types.SimpleNamespace(NAME=""), VERBOSE=False))
    data = [(x, t)] * a.steps
    loss_fn = BCEWithLogitsLoss()

    def epoch_fn(augment):
        torch.manual_seed(0)
        m = ResUNet(image_shape=(P,) * 3 + (1,), activation="elu", feature_maps=FM, drop_values=[0.0] * 5, normalization="in", yx_down=[2] * 4,
                    z_down=[2] * 4, isotropy=[True] * 5, larger_io=False, conv_layers=[2] * 5, compute_dtype=torch.float16).to(dev).train()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-4, capturable=True)
        state = dict(ep=0)

        def run():
            TE.train_one_epoch(cfg, m, None, loss_fn, None, None, data, [opt], dev, state["ep"], loss_names=["loss"], graph="on", augment=augment)
            state["ep"] += 1

        run()                                                              # captures
        return run

    ep = {"e step, augmenter": epoch_fn(DeviceAugmenter(da_prob=1.0, seed=2, **REST)),
          "e step, augmenter with the affine options": epoch_fn(DeviceAugmenter(da_prob=1.0, seed=2, **REST, **AFFINE))}
    step = {k: [] for k in ep}
    for r in range(a.rounds):
        for k, fn in ep.items():
            step[k].append(timed(fn, 1, warm=0) / a.steps)
            print(f"round {r + 1} {k}: {step[k][-1]:.4f} ms per step", flush=True)
    res.update(summary(step))

    ms = {k: v["mean_ms"] for k, v in res.items()}
    spread = max(v["spread_ms"] for v in res.values())
    c_eager = min(ms["c-u8 torch affine_grid + grid_sample, uint8 target converted"], ms["c-f32 torch affine_grid + grid_sample, float32 target"])
    c_graph = min(ms["graph: c-u8 torch affine_grid + grid_sample, uint8 target converted"], ms["graph: c-f32 torch affine_grid + grid_sample, float32 target"])
    extra = ms["e step, augmenter with the affine options"] - ms["e step, augmenter"]
    held = {True: "held", False: "not held"}
    cond = {
        "a below the cheaper c by more than the spread, eager": held[ms["a warp call"] + spread < c_eager],
        "a below the cheaper c by more than the spread, graph replays": held[ms["graph: a warp call"] + spread < c_graph],
        "e increase within a eager + spread": held[extra <= ms["a warp call"] + spread],
    }
    traffic = x.numel() * 4 * 2 + t8.numel() * 2
    floor_ms = traffic / (YARDSTICK_TBPS * 1e12) * 1e3
    out = dict(
        workload=f"{B} x {P}^3 x 1 fp32 image, one-channel uint8 target; {a.steps} repetitions per reading, {a.rounds} readings per configuration, "
                 f"configurations alternated; one call; (e): cfg-2 ResUNet {FM}, mixed mode, AdamW, graph='on'",
        device=torch.cuda.get_device_name(0), ms=res, largest_spread_ms=spread, torch_cheaper_ms=dict(eager=c_eager, graph=c_graph),
        step_increase_ms=round(extra, 4), conditions=cond,
        traffic=dict(what="bpx_warp_apply: image and uint8 target read once and written once (the call (a) adds the gather pass's copy of the same size)",
                     bytes=traffic, yardstick_tbps=YARDSTICK_TBPS, floor_ms=round(floor_ms, 4), warp_apply_replay_ms=ms["graph: w bpx_warp_apply alone"],
                     warp_apply_over_floor=round(ms["graph: w bpx_warp_apply alone"] / floor_ms, 2),
                     call_replay_ms=ms["graph: a warp call"], call_over_floor=round(ms["graph: a warp call"] / floor_ms, 2),
                     note="back-to-back repetitions re-read the same 33.5 MB image, which fits the last-level cache: not an HBM figure"),
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))
    print("wrote", a.out)
    return 0 if all(v == "held" for v in cond.values()) else 1


if __name__ == "__main__":
    sys.exit(main())

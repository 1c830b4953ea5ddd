"""What the device augmenter costs at 4 x 128^3 x 1 fp32 with a one-channel float32 target, one box, one call, the configurations alternated, 40
repetitions per reading, three readings each (HIP events):
  (a)   DeviceAugmenter with everything enabled and da_prob = 1 (draw + mean + apply; k drawn per sample); (a-u8) the same with a uint8 target, whose
        ~117 MB of traffic (image read twice - mean and apply - and written once, target read and written) is set against the 5.2 TB/s of the
        project's streaming passes;
  (b)   geometry only through records=: every sample k = 0, and every sample k = 1;
  (c)   the same transforms as (a) composed from torch device ops: rot90(...).contiguous(), flip, the contrast / brightness arithmetic, randn_like,
        two masked fills, and the target's rot90 + flip;
  (d)   torch.rot90(x, 1, (Y, X)).contiguous() of the image alone, and of image and target;
  (e)   the cfg-2 train_one_epoch(graph="on") step with and without augment= (device-resident batches, 40 steps per epoch);
  (copy) one clone of image and target;
  (graph: ...) every one of (a)-(d) also captured alone in a HIP graph and replayed: the device's share without the host's (argument checks,
        ctypes, three or four launch calls per augmenter call - an eager call is host-bound at this size).
Conditions, each against torch or the plain step, never against the code under test: (a) < (c); (b, k = 1) < (d) of image and target; (e) with
augmentation exceeds (e) without by no more than (a) + (copy) + the spread of the readings.  Exit status 1 if one fails.
Writes profiles/augment_timing.json.
python scripts/augment_timing.py [--steps 40] [--rounds 3] [--patch 128] [--batch 4]"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import augment_ref as AR  # noqa: E402
from biapy_amd import train_engine as TE  # noqa: E402
from biapy_amd.augment import DeviceAugmenter  # noqa: E402
from biapy_amd.losses import BCEWithLogitsLoss  # noqa: E402
from biapy_amd.resunet import ResUNet  # noqa: E402

FM = [16, 32, 64, 128, 256]
STREAM_TBPS = 5.2
ALL_ON = dict(rot90=True, zflip=True, vflip=True, hflip=True, brightness=(-0.1, 0.1), contrast=(-0.1, 0.1), gaussian_noise=(0.01, 0.05),
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "augment_timing.py measures on the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda", 0)
    P, B = a.patch, a.batch
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((B, P, P, P, 1), device=dev, generator=g)
    t = (torch.rand((B, P, P, P, 1), device=dev, generator=g) > 0.5).float()
    t8 = t.to(torch.uint8)
    xo, to, to8 = torch.empty_like(x), torch.empty_like(t), torch.empty_like(t8)

    full, full8, geo = DeviceAugmenter(da_prob=1.0, seed=1, **ALL_ON), DeviceAugmenter(da_prob=1.0, seed=1, **ALL_ON), DeviceAugmenter(seed=1)
    rec_k0 = torch.from_numpy(np.stack([AR.make_record(k=0)] * B)).to(dev)
    rec_k1 = torch.from_numpy(np.stack([AR.make_record(k=1)] * B)).to(dev)
    boxes = [(P // 8, P // 4, P // 8, P // 6, P // 6, P // 6), (P // 2, P // 2, P // 3, P // 6, P // 6, P // 6)]

    def torch_composed():
        v = torch.flip(torch.rot90(x, 1, (2, 3)).contiguous(), (1, 2, 3))
        u = torch.flip(torch.rot90(t, 1, (2, 3)).contiguous(), (1, 2, 3))
        m = x.mean(dim=(1, 2, 3, 4), keepdim=True)
        v = (v - m) * 1.05 + m
        v = v + 0.03
        v = v + 0.02 * torch.randn_like(v)
        for z0, y0, x0, dz, dy, dx in boxes:
            v[:, z0:z0 + dz, y0:y0 + dy, x0:x0 + dx] = 0.0
        return v, u

    fns = {
        "a augmenter all": lambda: full(x, t, out=(xo, to)),
        "a-u8 augmenter all, uint8 target": lambda: full8(x, t8, out=(xo, to8)),
        "b geometry k=0": lambda: geo(x, t, out=(xo, to), records=rec_k0),
        "b geometry k=1": lambda: geo(x, t, out=(xo, to), records=rec_k1),
        "c torch composed": torch_composed,
        "d torch rot90 image": lambda: torch.rot90(x, 1, (2, 3)).contiguous(),
        "d torch rot90 image+target": lambda: (torch.rot90(x, 1, (2, 3)).contiguous(), torch.rot90(t, 1, (2, 3)).contiguous()),
        "copy image+target": lambda: (xo.copy_(x), to.copy_(t)),
    }
    # the same calls replayed from a HIP graph each: device time without the host's share (argument checks, ctypes, launch calls)
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
    for k in [k for k in fns if not k.startswith("copy")]:
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

    ep = {"e step plain": epoch_fn(None), "e step augmented": epoch_fn(DeviceAugmenter(da_prob=1.0, seed=2, **ALL_ON))}
    step = {k: [] for k in ep}
    for r in range(a.rounds):
        for k, fn in ep.items():
            step[k].append(timed(fn, 1, warm=0) / a.steps)
            print(f"round {r + 1} {k}: {step[k][-1]:.4f} ms per step", flush=True)
    res.update(summary(step))

    ms = {k: v["mean_ms"] for k, v in res.items()}
    spread = max(v["spread_ms"] for v in res.values())
    traffic = x.numel() * 4 * 3 + t8.numel() * 2
    floor_ms = traffic / (STREAM_TBPS * 1e12) * 1e3
    a8 = ms["graph: a-u8 augmenter all, uint8 target"]
    extra = ms["e step augmented"] - ms["e step plain"]
    cond = {
        "a below c": bool(ms["a augmenter all"] < ms["c torch composed"]),
        "b k=1 below d of image and target": bool(ms["b geometry k=1"] < ms["d torch rot90 image+target"]),
        "graph replays: a below c": bool(ms["graph: a augmenter all"] < ms["graph: c torch composed"]),
        "graph replays: b k=1 below d of image and target": bool(ms["graph: b geometry k=1"] < ms["graph: d torch rot90 image+target"]),
        "e extra within a + copy + spread": bool(extra <= ms["a augmenter all"] + ms["copy image+target"] + spread),
    }
    out = dict(
        workload=f"{B} x {P}^3 x 1 fp32 image, one-channel float32 target (a-u8: uint8); {a.steps} repetitions per reading, {a.rounds} readings per "
                 f"configuration, configurations alternated; one box, one call; (e): cfg-2 ResUNet {FM}, mixed mode, AdamW, graph='on'",
        device=torch.cuda.get_device_name(0), ms=res, largest_spread_ms=spread, step_extra_ms=round(extra, 4), conditions=cond,
        traffic=dict(what="a-u8: image read by the mean pass and by the apply pass and written once, uint8 target read and written", bytes=traffic,
                     yardstick_tbps=STREAM_TBPS, floor_ms=round(floor_ms, 4), eager_call_ms=ms["a-u8 augmenter all, uint8 target"],
                     graph_replay_ms=a8, graph_replay_over_floor=round(a8 / floor_ms, 2),
                     note="back-to-back repetitions re-read the same 33.5 MB image, which fits the last-level cache: not an HBM figure"),
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))
    print("wrote", a.out)
    return 0 if all(cond.values()) else 1


if __name__ == "__main__":
    sys.exit(main())

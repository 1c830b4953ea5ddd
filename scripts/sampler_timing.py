"""What drawing a training batch on the device costs: 4 x 128^3 x 1 float32 patches with a uint8 target out of one resident 512^3 volume, one box, one
call, the configurations alternated, 40 repetitions per reading, three readings each (HIP events):
  (a)   DevicePatchSampler, uniform mode (draw + gather into given outputs); (a-class) the class mode over the target's foreground map with the
        probabilities (0.06, 0.94): the draw then searches 262,144 rows and one 512-voxel row per sample;
  (b)   the same batch composed from torch device ops at the same origins: four slices of the image and four of the target, torch.stack each;
  (copy) one clone of a resident batch and its target: the same bytes in one aligned streaming copy each;
  (graph: ...) (a), (a-class) and (b) also captured alone in a HIP graph and replayed: the device's share without the host's (argument checks,
        ctypes, two launch calls per sampler call - an eager call is host-bound at this size);
  (e)   the cfg-2 train_one_epoch(graph="on") step fed by DevicePatchLoader + DeviceAugmenter, and fed by the augmenter on one fixed resident batch
        of the same dtypes (the step as it was before the sampler: the baseline).
The sampler's traffic - the patches read once and written once, image and target, 84 MB - is set against the 4.5 TB/s yardstick of the project's
streaming passes.  Back-to-back calls draw other origins but from a volume whose neighbourhoods (and the outputs) may still sit
in the last-level cache: not an HBM figure.
Conditions, each against torch or the step without the sampler, never against the code under test: (a) and (a-class) below (b) by more than the
largest spread of the readings; (e) with the loader exceeds (e) on the fixed batch by no more than (a)'s eager time plus that spread.  Exit status 1 if
one fails.  Writes profiles/sampler_timing.json.
python scripts/sampler_timing.py [--steps 40] [--rounds 3] [--patch 128] [--batch 4] [--vol 512]"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from biapy_amd import train_engine as TE  # noqa: E402
from biapy_amd.augment import DeviceAugmenter  # noqa: E402
from biapy_amd.losses import BCEWithLogitsLoss  # noqa: E402
from biapy_amd.resunet import ResUNet  # noqa: E402
from biapy_amd.sampler import DevicePatchLoader, DevicePatchSampler  # noqa: E402

FM = [16, 32, 64, 128, 256]
STREAM_TBPS = 4.5
AUG = dict(rot90=True, zflip=True, vflip=True, hflip=True, brightness=(-0.1, 0.1), contrast=(-0.1, 0.1), gaussian_noise=(0.01, 0.05),
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
    ap.add_argument("--vol", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sampler_timing.py measures on the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda", 0)
    P, B, N = a.patch, a.batch, a.vol
    g = torch.Generator(device=dev).manual_seed(0)
    img = torch.randn((N, N, N, 1), device=dev, generator=g)
    tgt = (torch.rand((N, N, N, 1), device=dev, generator=g) > 0.7).to(torch.uint8)
    uni = DevicePatchSampler(img, tgt, (P, P, P), batch_size=B, seed=1)
    cls = DevicePatchSampler(img, tgt, (P, P, P), batch_size=B, seed=1, class_maps=DevicePatchSampler.foreground_map(tgt), class_probs=(0.06, 0.94))
    xo, to = torch.empty((B, P, P, P, 1), device=dev), torch.empty((B, P, P, P, 1), dtype=torch.uint8, device=dev)
    xb, tb = uni()                                                         # one resident batch: the fixed batch of (e), the operand of (copy)
    org = uni.last_origins.cpu().tolist()

    def torch_composed():
        return (torch.stack([img[z:z + P, y:y + P, x:x + P] for _, z, y, x in org]), torch.stack([tgt[z:z + P, y:y + P, x:x + P] for _, z, y, x in org]))

    check = torch_composed()
    assert torch.equal(check[0], xb) and torch.equal(check[1], tb)         # the two ways give the same batch
    del check
    fns = {
        "a sampler uniform": lambda: uni(out=(xo, to)),
        "a-class sampler class mode": lambda: cls(out=(xo, to)),
        "b torch slices + stack": torch_composed,
        "copy image+target": lambda: (xo.copy_(xb), to.copy_(tb)),
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
    for k in [k for k in fns if not k.startswith("copy")]:
        fn, keep = graphed(fns[k])
        kept.append(keep)
        fns["graph: " + k] = fn
    res = summary(alternate(fns, a.steps, a.rounds))
    torch.cuda.synchronize()

    # (e) the cfg-2 step through train_one_epoch(graph="on")
    cfg = types.SimpleNamespace(DATA=types.SimpleNamespace(PATCH_SIZE=(P, P, P, 1)),
                                TRAIN=types.SimpleNamespace(GRADIENT_CLIP_NORM=0.0, LR_SCHEDULER=types.SimpleNamespace(NAME=""), VERBOSE=False))
    loss_fn = BCEWithLogitsLoss()

    def epoch_fn(data):
        torch.manual_seed(0)
        m = ResUNet(image_shape=(P,) * 3 + (1,), activation="elu", feature_maps=FM, drop_values=[0.0] * 5, normalization="in", yx_down=[2] * 4,
                    z_down=[2] * 4, isotropy=[True] * 5, larger_io=False, conv_layers=[2] * 5, compute_dtype=torch.float16).to(dev).train()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-4, capturable=True)
        aug = DeviceAugmenter(da_prob=1.0, seed=2, **AUG)
        state = dict(ep=0)

        def run():
            TE.train_one_epoch(cfg, m, None, loss_fn, None, None, data, [opt], dev, state["ep"], loss_names=["loss"], graph="on", augment=aug)
            state["ep"] += 1

        run()                                                              # captures
        return run

    ep = {"e step, fixed resident batch + augmenter": epoch_fn([(xb, tb)] * a.steps),
          "e step, DevicePatchLoader + augmenter": epoch_fn(DevicePatchLoader(DevicePatchSampler(img, tgt, (P, P, P), batch_size=B, seed=3), a.steps))}
    step = {k: [] for k in ep}
    for r in range(a.rounds):
        for k, fn in ep.items():
            step[k].append(timed(fn, 1, warm=0) / a.steps)
            print(f"round {r + 1} {k}: {step[k][-1]:.4f} ms per step", flush=True)
    res.update(summary(step))

    ms = {k: v["mean_ms"] for k, v in res.items()}
    spread = max(v["spread_ms"] for v in res.values())
    traffic = 2 * (xb.numel() * 4 + tb.numel())
    floor_ms = traffic / (STREAM_TBPS * 1e12) * 1e3
    extra = ms["e step, DevicePatchLoader + augmenter"] - ms["e step, fixed resident batch + augmenter"]
    cond = {
        "a below b by more than the spread": bool(ms["a sampler uniform"] < ms["b torch slices + stack"] - spread),
        "a-class below b by more than the spread": bool(ms["a-class sampler class mode"] < ms["b torch slices + stack"] - spread),
        "e extra within a + spread": bool(extra <= ms["a sampler uniform"] + spread),
    }
    ga, gc = ms["graph: a sampler uniform"], ms["graph: a-class sampler class mode"]
    out = dict(
        workload=f"{B} x {P}^3 x 1 float32 patches with a uint8 target from one resident {N}^3 volume; {a.steps} repetitions per reading, {a.rounds} "
                 f"readings per configuration, configurations alternated; one box, one call; (e): cfg-2 ResUNet {FM}, mixed mode, AdamW, graph='on', "
                 f"DeviceAugmenter with everything fired",
        device=torch.cuda.get_device_name(0), ms=res, largest_spread_ms=spread, step_extra_ms=round(extra, 4), conditions=cond,
        traffic=dict(what="the patches read once and written once: float32 image and uint8 target", bytes=traffic, yardstick_tbps=STREAM_TBPS,
                     floor_ms=round(floor_ms, 4), eager_call_ms=ms["a sampler uniform"], graph_replay_ms=ga, graph_replay_over_floor=round(ga / floor_ms, 2),
                     class_mode_graph_replay_ms=gc, class_mode_graph_replay_over_floor=round(gc / floor_ms, 2),
                     note="back-to-back calls draw other origins, but 40 x 84 MB of windows out of a 671 MB volume revisit neighbourhoods that may still "
                          "sit in the 256 MiB last-level cache, and the 42 MB of outputs are rewritten in place: not an HBM figure"),
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))
    print("wrote", a.out)
    return 0 if all(cond.values()) else 1


if __name__ == "__main__":
    sys.exit(main())

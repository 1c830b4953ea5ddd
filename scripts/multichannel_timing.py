"""What an image of 2 to 15 channels costs on the cfg-2 ResUNet (feature_maps [16, 32, 64, 128, 256], 4 x 128^3, mixed mode), one box, one call:
the graph-replayed train step (forward + BCE + backward + AdamW) and the graph-replayed eval forward for in_ch = 1, 3 and 16, the three
configurations alternated, 40 replays per reading, three readings each; the HIP-event time of bpx_image_pack16 at C = 3 in both layouts and of
bpx_cast over the same voxels x 16 channels; and how many more kernels the C = 3 step dispatches than the in_ch = 16 step.

Conditions (recorded as booleans, exit status 1 if one is missed):
  (a) the C = 3 train step is not slower than the in_ch = 16 step by more than the largest spread between repeats of one configuration;
  (b) the pack kernel takes no longer than that bpx_cast.
The ratio to in_ch = 1 is reported, not conditioned.  Writes profiles/multichannel_timing.json.
python scripts/multichannel_timing.py [--steps 40] [--rounds 3] [--patch 128] [--batch 4]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from biapy_amd import _lib as L  # noqa: E402
from biapy_amd.graphs import GraphedInference, GraphedTrainStep  # noqa: E402
from biapy_amd.losses import BCEWithLogitsLoss  # noqa: E402
from biapy_amd.resunet import ResUNet  # noqa: E402

FM = [16, 32, 64, 128, 256]
CHANNELS = (1, 3, 16)


def timed(fn, n):
    """ms per call of n back-to-back calls between two HIP events (one warm call first)."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def kernels_per_call(fn):
    """Kernel launches of one eager call as the profiler counts them (a replayed graph dispatches the same kernels); None where the profiler
    records no device activity."""
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception as e:  # noqa: BLE001
        print("kernel count not available:", repr(e)[:200], flush=True)
        return None


def alternate(fns, steps, rounds):
    """{name: [ms per call, one reading per round]}: the configurations take turns inside every round."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multichannel_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "multichannel_timing.py measures on the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda", 0)
    Pz, B = a.patch, a.batch
    loss_fn = BCEWithLogitsLoss()
    g = torch.Generator(device=dev).manual_seed(0)
    tgt = (torch.rand((B, 1, Pz, Pz, Pz), device=dev, generator=g) > 0.5).float()
    models, xs, steps, eager = {}, {}, {}, {}
    for C in CHANNELS:
        torch.manual_seed(0)
        m = ResUNet(image_shape=(Pz,) * 3 + (C,), activation="elu", feature_maps=FM, drop_values=[0.0] * 5, normalization="in", yx_down=[2] * 4,
                    z_down=[2] * 4, isotropy=[True] * 5, larger_io=False, conv_layers=[2] * 5, compute_dtype=torch.float16).to(dev).train()
        x = torch.randn((B, C, Pz, Pz, Pz), device=dev, generator=g)
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, fused=True, capturable=True)

        def eager_step(m=m, x=x, opt=opt):
            opt.zero_grad(set_to_none=True)
            loss_fn(m(x), tgt).backward()
            opt.step()

        models[C], xs[C], eager[C] = m, x, eager_step
    counts = {C: kernels_per_call(eager[C]) for C in CHANNELS}
    for C in CHANNELS:
        opt = torch.optim.AdamW(models[C].parameters(), lr=1e-3, fused=True, capturable=True)
        steps[C] = GraphedTrainStep(models[C], loss_fn, opt, xs[C], tgt)
    train = alternate({f"in_ch={C}": (lambda s=steps[C]: s()) for C in CHANNELS}, a.steps, a.rounds)
    del steps
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    infer = {}
    for C in CHANNELS:
        models[C].eval()
        infer[C] = GraphedInference(models[C].predict_proba, xs[C])
    evalf = alternate({f"in_ch={C}": (lambda s=infer[C]: s()) for C in CHANNELS}, a.steps, a.rounds)
    del infer, models
    torch.cuda.synchronize()
    torch.cuda.empty_cache()

    # ---- the input conversion alone: bpx_image_pack16 at C = 3 (both layouts) against bpx_cast over the same voxels x 16 channels -----------
    vox, st = Pz ** 3, L.stream_ptr()
    x3 = xs[3]
    x3cl = x3.permute(0, 2, 3, 4, 1).contiguous()
    x16 = xs[16].permute(0, 2, 3, 4, 1).contiguous()
    out16 = torch.empty((B, vox, 16), dtype=torch.float16, device=dev)
    conv = alternate({
        "image_pack16 C=3 planar": lambda: L.check(L.lib.bpx_image_pack16(L.F16, B, vox, 3, x3.data_ptr(), 3 * vox, 1, vox, out16.data_ptr(), st)),
        "image_pack16 C=3 channels-last": lambda: L.check(L.lib.bpx_image_pack16(L.F16, B, vox, 3, x3cl.data_ptr(), 3 * vox, 3, 1, out16.data_ptr(), st)),
        "cast 16 channels": lambda: L.check(L.lib.bpx_cast(L.F32, x16.data_ptr(), L.F16, out16.data_ptr(), x16.numel(), st)),
    }, 20, a.rounds)

    tr, ev, cv = summary(train), summary(evalf), summary(conv)
    spread = max(v["spread_ms"] for v in tr.values())
    d3_16 = tr["in_ch=3"]["mean_ms"] - tr["in_ch=16"]["mean_ms"]
    cast = cv["cast 16 channels"]["mean_ms"]
    pack = max(cv["image_pack16 C=3 planar"]["mean_ms"], cv["image_pack16 C=3 channels-last"]["mean_ms"])
    more = None if counts[3] is None or counts[16] is None else counts[3] - counts[16]
    out = dict(
        workload=f"cfg-2 ResUNet, feature_maps {FM}, {B} x {Pz}^3, mixed mode (fp16 forward, bf16 gradients); graph replay, {a.steps} replays per reading, "
                 f"{a.rounds} readings per configuration, configurations alternated; one box, one call",
        device=torch.cuda.get_device_name(0), train_step=tr, eval_forward=ev, input_conversion=cv,
        train_in_ch3_minus_in_ch16_ms=round(d3_16, 4), largest_spread_ms=spread,
        condition_a_in_ch3_not_slower_than_in_ch16_beyond_spread=bool(d3_16 <= spread),
        condition_b_pack_no_longer_than_cast=bool(pack <= cast),
        reported_only=dict(train_in_ch3_over_in_ch1=round(tr["in_ch=3"]["mean_ms"] / tr["in_ch=1"]["mean_ms"], 4),
                           train_in_ch3_minus_in_ch1_ms=round(tr["in_ch=3"]["mean_ms"] - tr["in_ch=1"]["mean_ms"], 4),
                           eval_in_ch3_over_in_ch1=round(ev["in_ch=3"]["mean_ms"] / ev["in_ch=1"]["mean_ms"], 4),
                           kernels_per_eager_train_step={f"in_ch={C}": counts[C] for C in CHANNELS},
                           in_ch3_dispatches_more_than_in_ch16=more),
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))
    print("wrote", a.out)
    return 0 if out["condition_a_in_ch3_not_slower_than_in_ch16_beyond_spread"] and out["condition_b_pack_no_longer_than_cast"] else 1


if __name__ == "__main__":
    sys.exit(main())

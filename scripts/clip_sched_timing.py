"""What gradient clipping and a per-step (one-cycle) schedule cost on the cfg-2 train step (ResUNet, feature_maps [16, 32, 64, 128, 256], 4 x 128^3,
mixed mode), one box, one call, the four configurations alternated, 40 steps per reading, three readings each:
  (i)   the graph-replayed step as it is without either (forward + BCE + backward + AdamW);
  (ii)  the same with GraphedTrainStep(max_grad_norm=c): bpx_grad_norm + the scaling inside bpx_adam_step_dev;
  (iii) (ii) + OneCycleLR stepped after every replay (lr filled in place, beta1 through the device double), as train_one_epoch drives it;
  (iv)  the eager step train_one_epoch ran for (iii)'s configuration before: backward -> clip_grad_norm_ -> optimizer.step() -> scheduler.step().
(ii) and (iii) add one read and one write of the gradients (2 x 4 bytes per parameter) and two or three small launches to (i): the yardstick for
(ii) - (i) is the spread of (i)'s readings plus those bytes at 4.5 TB/s, the lower end of what DESIGN.md records for the streaming passes (reported
as a boolean).  Condition (exit status 1 if missed): (iii) is faster than (iv).  Writes profiles/clip_sched_timing.json.
python scripts/clip_sched_timing.py [--steps 40] [--rounds 3] [--patch 128] [--batch 4]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch.nn.utils import clip_grad_norm_  # noqa: E402
from torch.optim.lr_scheduler import OneCycleLR  # noqa: E402

from biapy_amd.graphs import GraphedTrainStep  # noqa: E402
from biapy_amd.losses import BCEWithLogitsLoss  # noqa: E402
from biapy_amd.resunet import ResUNet  # noqa: E402

FM = [16, 32, 64, 128, 256]
CLIP = 1.0
STREAM_TBPS = 4.5


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_sched_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "clip_sched_timing.py measures on the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda", 0)
    Pz, B = a.patch, a.batch
    loss_fn = BCEWithLogitsLoss()
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((B, 1, Pz, Pz, Pz), device=dev, generator=g)
    tgt = (torch.rand((B, 1, Pz, Pz, Pz), device=dev, generator=g) > 0.5).float()
    total_steps = 10 * (a.steps + 1) * a.rounds + 100                 # the one-cycle schedule never runs out inside the measurement

    def model():
        torch.manual_seed(0)
        return ResUNet(image_shape=(Pz,) * 3 + (1,), activation="elu", feature_maps=FM, drop_values=[0.0] * 5, normalization="in", yx_down=[2] * 4,
                       z_down=[2] * 4, isotropy=[True] * 5, larger_io=False, conv_layers=[2] * 5, compute_dtype=torch.float16).to(dev).train()

    def adamw(m):
        return torch.optim.AdamW(m.parameters(), lr=1e-3, fused=True, capturable=True)

    fns = {}
    # (iv) first: its eager backward must be gone before a step is captured (graphs._warm)
    m4 = model()
    o4 = adamw(m4)
    s4 = OneCycleLR(o4, max_lr=1e-3, total_steps=total_steps)
    p4 = list(m4.parameters())

    def eager_step():
        o4.zero_grad(set_to_none=True)
        loss_fn(m4(x), tgt).backward()
        clip_grad_norm_(p4, max_norm=CLIP)
        o4.step()
        s4.step()

    eager_step()
    o4.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    n_params = sum(p.numel() for p in p4)

    m1 = model()
    g1 = GraphedTrainStep(m1, loss_fn, adamw(m1), x, tgt)
    m2 = model()
    g2 = GraphedTrainStep(m2, loss_fn, adamw(m2), x, tgt, max_grad_norm=CLIP)
    m3 = model()
    o3 = adamw(m3)
    s3 = OneCycleLR(o3, max_lr=1e-3, total_steps=total_steps)
    g3 = GraphedTrainStep(m3, loss_fn, o3, x, tgt, max_grad_norm=CLIP)

    lr_acc = torch.zeros((), dtype=torch.float64, device=dev)

    def replay_sched():
        g3()
        s3.step()
        lr_acc.add_(o3.param_groups[0]["lr"])                         # the epoch's lr meter: summed on the device, read once at the end

    fns["i graph"] = lambda: g1()
    fns["ii graph+clip"] = lambda: g2()
    fns["iii graph+clip+onecycle"] = replay_sched
    fns["iv eager+clip+onecycle"] = eager_step
    res = summary(alternate(fns, a.steps, a.rounds))
    torch.cuda.synchronize()
    norm2, norm3 = g2.grad_norm.tolist(), g3.grad_norm.tolist()

    i, ii, iii, iv = (res[k] for k in fns)
    extra_bytes = 2 * 4 * n_params
    stream_ms = extra_bytes / (STREAM_TBPS * 1e12) * 1e3
    out = dict(
        workload=f"cfg-2 ResUNet, feature_maps {FM}, {B} x {Pz}^3, mixed mode (fp16 forward, bf16 gradients), AdamW; {a.steps} steps per reading, "
                 f"{a.rounds} readings per configuration, configurations alternated; one box, one call",
        device=torch.cuda.get_device_name(0), parameters=n_params, max_grad_norm=CLIP, step_ms=res,
        last_norm_and_coefficient={"ii": norm2, "iii": norm3},
        clip_minus_plain_ms=round(ii["mean_ms"] - i["mean_ms"], 4), clip_onecycle_minus_plain_ms=round(iii["mean_ms"] - i["mean_ms"], 4),
        plain_spread_ms=i["spread_ms"], extra_gradient_bytes=extra_bytes, extra_bytes_at_streaming_rate_ms=round(stream_ms, 4),
        clip_within_spread_plus_streaming_time=bool(ii["mean_ms"] - i["mean_ms"] <= i["spread_ms"] + stream_ms),
        eager_over_graph_clip_onecycle=round(iv["mean_ms"] / iii["mean_ms"], 3),
        condition_graph_clip_onecycle_beats_eager=bool(iii["mean_ms"] < iv["mean_ms"]),
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))
    print("wrote", a.out)
    return 0 if out["condition_graph_clip_onecycle_beats_eager"] else 1


if __name__ == "__main__":
    sys.exit(main())

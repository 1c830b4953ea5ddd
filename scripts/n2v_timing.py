"""What Noise2Void on the device costs at 4 x 128^3 x 1 fp32, one box, one call, the configurations alternated, 40 repetitions per reading, three
readings each (HIP events), medians:
  (a) N2VMasker (default grid: box 8, radius 5, uniform_withCP) against (a-torch) the same masking composed from torch device ops: clone, zeros,
      randint-drawn positions and window offsets, gather and scatter;
  (b) N2VLoss forward plus backward against (b-torch) the formula composed from torch ops with autograd;
  (c) the train_one_epoch(graph="on") step of a one-channel linear-head ResUNet with masker and N2VLoss against the same step on a fixed pre-masked
      batch (device-resident batches, 40 steps per epoch).
Neither reference is the code under test.  Conditions: (a) < (a-torch) and (b) < (b-torch).  Reported without a cap: the multiple of the traffic
floor - 16 B per voxel-channel for the masker (x read, x_masked and the two target planes written) and 16 B for the loss forward plus backward, at
4.5 TB/s - and the step's overhead in ms.  Exit status 1 if a condition fails.  Writes profiles/n2v_timing.json.
python scripts/n2v_timing.py [--steps 40] [--rounds 3] [--patch 128] [--batch 4]"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from biapy_amd import train_engine as TE  # noqa: E402
from biapy_amd.losses import N2VLoss  # noqa: E402
from biapy_amd.n2v import N2VMasker  # noqa: E402
from biapy_amd.resunet import ResUNet  # noqa: E402

FM = [16, 32, 64, 128, 256]
STREAM_TBPS = 4.5


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


def alternate(fns, steps, rounds, per=1):
    out = {k: [] for k in fns}
    for r in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, steps if per == 1 else 1, warm=1 if per == 1 else 0) / per)
            print(f"round {r + 1} {k}: {out[k][-1]:.4f} ms", flush=True)
    return out


def summary(readings):
    return {k: dict(readings_ms=[round(v, 4) for v in vs], median_ms=round(statistics.median(vs), 4), spread_ms=round(max(vs) - min(vs), 4))
            for k, vs in readings.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "n2v_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "n2v_timing.py measures on the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda", 0)
    P, B, C = a.patch, a.batch, 1
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((B, P, P, P, C), device=dev, generator=g)
    xo, tgt = torch.empty_like(x), torch.empty((B, 2 * C, P, P, P), device=dev)
    masker = N2VMasker(seed=1)
    s, r = masker.grid(P, P, P)[0][0], masker.radius[0]
    n = P // s
    V = P ** 3
    base = torch.arange(n, device=dev) * s
    bz, by, bx = torch.meshgrid(base, base, base, indexing="ij")
    brow = torch.arange(B, device=dev)[:, None] * V

    def torch_mask():
        o = x.clone()
        t = torch.zeros((B, 2 * C, V), device=dev)
        off = torch.randint(0, s, (3, B, n, n, n), device=dev)
        pz, py, px = bz + off[0], by + off[1], bx + off[2]
        d = torch.randint(-r, r + 1, (3, B, n, n, n), device=dev)
        qz, qy, qx = (pz + d[0]).clamp(0, P - 1), (py + d[1]).clamp(0, P - 1), (px + d[2]).clamp(0, P - 1)
        p = ((pz * P + py) * P + px).view(B, -1)
        q = ((qz * P + qy) * P + qx).view(B, -1)
        flat = x.view(-1)
        vals, orig = flat[(q + brow).view(-1)], flat[(p + brow).view(-1)]
        o.view(-1).scatter_(0, (p + brow).view(-1), vals)
        t[:, 0].scatter_(1, p, orig.view(B, -1))
        t[:, 1].scatter_(1, p, torch.ones_like(orig).view(B, -1))
        return o, t

    masker(x, None, out=(xo, tgt))
    pred = torch.randn((B, C, P, P, P), device=dev, generator=g).requires_grad_(True)
    crit = N2VLoss()

    def loss_device():
        pred.grad = None
        crit(pred, tgt).backward()

    def loss_torch():
        pred.grad = None
        v, m = tgt[:, :C], tgt[:, C:]
        (((v - pred * m) ** 2).sum() / m.sum()).backward()

    fns = {"a masker": lambda: masker(x, None, out=(xo, tgt)), "a-torch composed masking": torch_mask, "b N2VLoss fwd+bwd": loss_device,
           "b-torch composed loss fwd+bwd": loss_torch}
    res = summary(alternate(fns, a.steps, a.rounds))
    torch.cuda.synchronize()

    # (c) the step through train_one_epoch(graph="on"), batches resident on the device
    cfg = types.SimpleNamespace(DATA=types.SimpleNamespace(PATCH_SIZE=(P, P, P, 1)),
                                TRAIN=types.SimpleNamespace(GRADIENT_CLIP_NORM=0.0, LR_SCHEDULER=types.SimpleNamespace(NAME=""), VERBOSE=False))
    dummy = torch.zeros((B, P, P, P, 1), device=dev)
    fixed_x, fixed_t = N2VMasker(seed=2)(x)
    data = {"c step, masker + N2VLoss": ([(x, dummy)] * a.steps, N2VMasker(seed=2)),
            "c step, fixed pre-masked batch": ([(fixed_x, fixed_t.permute(0, 2, 3, 4, 1))] * a.steps, None)}

    def epoch_fn(batches, augment):
        torch.manual_seed(0)
        m = ResUNet(image_shape=(P,) * 3 + (1,), activation="elu", feature_maps=FM, drop_values=[0.0] * 5, normalization="in", yx_down=[2] * 4,
                    z_down=[2] * 4, isotropy=[True] * 5, larger_io=False, conv_layers=[2] * 5, compute_dtype=torch.float16,
                    head_activations=["linear"]).to(dev).train()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-4, capturable=True)
        state = dict(ep=0)

        def run():
            TE.train_one_epoch(cfg, m, None, crit, None, None, batches, [opt], dev, state["ep"], loss_names=["loss"], graph="on", augment=augment)
            state["ep"] += 1

        run()                                                              # captures
        return run

    res.update(summary(alternate({k: epoch_fn(*v) for k, v in data.items()}, a.steps, a.rounds, per=a.steps)))

    ms = {k: v["median_ms"] for k, v in res.items()}
    floor_ms = 16 * B * V * C / (STREAM_TBPS * 1e12) * 1e3
    overhead = ms["c step, masker + N2VLoss"] - ms["c step, fixed pre-masked batch"]
    cond = {"a masker below its torch composition": bool(ms["a masker"] < ms["a-torch composed masking"]),
            "b N2VLoss below its torch composition": bool(ms["b N2VLoss fwd+bwd"] < ms["b-torch composed loss fwd+bwd"])}
    out = dict(
        workload=f"{B} x {P}^3 x {C} fp32; {a.steps} repetitions per reading, {a.rounds} readings per configuration, configurations alternated, medians; "
                 f"one box, one call; (c): ResUNet {FM}, one linear output channel, mixed mode, AdamW, graph='on'",
        device=torch.cuda.get_device_name(0), ms=res, conditions=cond, step_overhead_ms=round(overhead, 4),
        traffic=dict(bytes_per_voxel_channel=16, yardstick_tbps=STREAM_TBPS, floor_ms=round(floor_ms, 4),
                     masker_over_floor=round(ms["a masker"] / floor_ms, 2), loss_fwd_bwd_over_floor=round(ms["b N2VLoss fwd+bwd"] / floor_ms, 2),
                     note="eager calls: the host's share (argument checks, ctypes, autograd) is inside; back-to-back repetitions re-use a working set "
                          "that fits the last-level cache in part: not an HBM figure"),
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))
    print("wrote", a.out)
    return 0 if all(cond.values()) else 1


if __name__ == "__main__":
    sys.exit(main())

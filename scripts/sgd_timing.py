"""What the replayed SGD step costs on the cfg-2 train step (ResUNet, feature_maps [16, 32, 64, 128, 256], 4 x 128^3, mixed mode; SGD with momentum
0.9, Nesterov, weight decay 1e-2), one box, one call, the configurations alternated, 40 steps per reading, three readings each:
  (i)   the graph-replayed step (forward + BCE + backward + bpx_sgd_step);
  (ii)  the same with GraphedTrainStep(max_grad_norm=c): bpx_grad_norm + the scaling inside bpx_sgd_step;
  (iii) (ii) + OneCycleLR stepped after every replay (lr filled in place, the momentum through the device double), as train_one_epoch drives it;
  (e-i) (e-ii) (e-iii) the eager steps train_one_epoch(graph="off") runs for the same three configurations - what an SGD run got before the
        replayed step accepted SGD: backward -> [clip_grad_norm_ ->] optimizer.step() [-> scheduler.step()].
The yardstick is the eager step: a replayed configuration is expected not to be slower than its eager twin by more than the spread of the alternated
readings (exit status 1 if one is).  Also the kernel alone: bpx_sgd_step over the model's parameters (HIP events around 20 launches after 5),
torch's foreach SGD step on the same tensors, and the 20 bytes per parameter (p, g, buffer read; p, buffer written) at the 4.5 TB/s that DESIGN.md
records as the lower end of the streaming passes.  Writes profiles/sgd_timing.json.
python scripts/sgd_timing.py [--steps 40] [--rounds 3] [--patch 128] [--batch 4]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch.nn.utils import clip_grad_norm_  # noqa: E402
from torch.optim.lr_scheduler import OneCycleLR  # noqa: E402

from biapy_amd import _lib as L  # noqa: E402
from biapy_amd import optim as O  # noqa: E402
from biapy_amd.graphs import GraphedTrainStep  # noqa: E402
from biapy_amd.losses import BCEWithLogitsLoss  # noqa: E402
from biapy_amd.resunet import ResUNet  # noqa: E402

FM = [16, 32, 64, 128, 256]
CLIP = 1.0
LR = 1e-2
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgd_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sgd_timing.py measures on the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda", 0)
    Pz, B = a.patch, a.batch
    loss_fn = BCEWithLogitsLoss()
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((B, 1, Pz, Pz, Pz), device=dev, generator=g)
    tgt = (torch.rand((B, 1, Pz, Pz, Pz), device=dev, generator=g) > 0.5).float()
    total_steps = 10 * (a.steps + 1) * a.rounds + 100                 # the one-cycle schedules never run out inside the measurement

    def model():
        torch.manual_seed(0)
        return ResUNet(image_shape=(Pz,) * 3 + (1,), activation="elu", feature_maps=FM, drop_values=[0.0] * 5, normalization="in", yx_down=[2] * 4,
                       z_down=[2] * 4, isotropy=[True] * 5, larger_io=False, conv_layers=[2] * 5, compute_dtype=torch.float16).to(dev).train()

    def sgd(m):
        decay = [p for p in m.parameters() if p.dim() > 1]
        rest = [p for p in m.parameters() if p.dim() <= 1]
        return torch.optim.SGD([dict(params=decay, weight_decay=1e-2), dict(params=rest, weight_decay=0.0)], lr=LR, momentum=0.9, nesterov=True)

    fns = {}
    # the eager steps first: their backward graphs must be gone before a step is captured (graphs._warm)
    def eager(clip, cycle):
        m = model()
        o = sgd(m)
        s = OneCycleLR(o, max_lr=LR, total_steps=total_steps) if cycle else None
        ps = list(m.parameters())

        def step():
            o.zero_grad(set_to_none=True)
            loss_fn(m(x), tgt).backward()
            if clip:
                clip_grad_norm_(ps, max_norm=CLIP)
            o.step()
            if s is not None:
                s.step()

        step()
        o.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        return step, ps

    e1, params = eager(False, False)
    e2, _ = eager(True, False)
    e3, _ = eager(True, True)
    n_params = sum(p.numel() for p in params)

    m1 = model()
    g1 = GraphedTrainStep(m1, loss_fn, sgd(m1), x, tgt)
    m2 = model()
    g2 = GraphedTrainStep(m2, loss_fn, sgd(m2), x, tgt, max_grad_norm=CLIP)
    m3 = model()
    o3 = sgd(m3)
    s3 = OneCycleLR(o3, max_lr=LR, total_steps=total_steps)
    g3 = GraphedTrainStep(m3, loss_fn, o3, x, tgt, max_grad_norm=CLIP)
    assert g1.device_momentum and g2.device_momentum and g3.device_momentum

    lr_acc = torch.zeros((), dtype=torch.float64, device=dev)

    def replay_sched():
        g3()
        s3.step()
        lr_acc.add_(o3.param_groups[0]["lr"])                         # the epoch's lr meter: summed on the device, read once at the end

    fns["i graph"] = lambda: g1()
    fns["e-i eager"] = e1
    fns["ii graph+clip"] = lambda: g2()
    fns["e-ii eager+clip"] = e2
    fns["iii graph+clip+onecycle"] = replay_sched
    fns["e-iii eager+clip+onecycle"] = e3
    res = summary(alternate(fns, a.steps, a.rounds))
    torch.cuda.synchronize()

    # the kernel alone, on tensors of the model's sizes
    ps = [torch.nn.Parameter(torch.randn_like(p)) for p in params]
    for p in ps:
        p.grad = torch.randn_like(p)
    ko = torch.optim.SGD(ps, lr=LR, momentum=0.9, nesterov=True, weight_decay=1e-2)
    ko.step()                                                          # torch creates the momentum buffers
    assert O.fused_sgd_step(ko)
    arr = O._tensor_list(ko, ps, m="momentum_buffer")                  # the C call itself, the tensor list built once: no Python between the launches
    st = L.stream_ptr()
    kernel_ms = timed(lambda: L.check(L.lib.bpx_sgd_step(len(ps), arr, None, LR, None, 0.9, 0.0, 1e-2, 1, None, st)), 20, warm=5)
    to = torch.optim.SGD(ps, lr=LR, momentum=0.9, nesterov=True, weight_decay=1e-2, foreach=True)
    to.load_state_dict(ko.state_dict())
    foreach_ms = timed(to.step, 20, warm=5)
    kernel_bytes = 20 * n_params
    stream_ms = kernel_bytes / (STREAM_TBPS * 1e12) * 1e3

    pairs = (("i graph", "e-i eager"), ("ii graph+clip", "e-ii eager+clip"), ("iii graph+clip+onecycle", "e-iii eager+clip+onecycle"))
    verdict = {}
    for gk, ek in pairs:
        spread = max(res[gk]["spread_ms"], res[ek]["spread_ms"])
        verdict[gk] = dict(eager_over_graph=round(res[ek]["mean_ms"] / res[gk]["mean_ms"], 3), spread_ms=spread,
                           not_slower_than_eager_beyond_spread=bool(res[gk]["mean_ms"] <= res[ek]["mean_ms"] + spread))
    out = dict(
        workload=f"cfg-2 ResUNet, feature_maps {FM}, {B} x {Pz}^3, mixed mode (fp16 forward, bf16 gradients), SGD momentum 0.9 Nesterov, weight decay "
                 f"1e-2 in one of two groups; {a.steps} steps per reading, {a.rounds} readings per configuration, configurations alternated; one box, "
                 f"one call",
        device=torch.cuda.get_device_name(0), parameters=n_params, max_grad_norm=CLIP, step_ms=res, replayed_against_eager=verdict,
        last_norm_and_coefficient={"ii": g2.grad_norm.tolist(), "iii": g3.grad_norm.tolist()},
        clip_minus_plain_ms=round(res["ii graph+clip"]["mean_ms"] - res["i graph"]["mean_ms"], 4),
        kernel=dict(what="bpx_sgd_step over the model's parameters in one group (momentum, Nesterov, weight decay): HIP events around 20 calls after 5",
                    bpx_sgd_step_ms=round(kernel_ms, 4), torch_foreach_sgd_step_ms=round(foreach_ms, 4), torch_over_bpx=round(foreach_ms / kernel_ms, 2),
                    bytes=kernel_bytes, achieved_tbps=round(kernel_bytes / (kernel_ms * 1e-3) / 1e12, 3), yardstick_tbps=STREAM_TBPS,
                    bytes_at_yardstick_ms=round(stream_ms, 4), fraction_of_yardstick=round(stream_ms / kernel_ms, 3),
                    launches=-(-len(ps) // 64)),
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))
    print("wrote", a.out)
    return 0 if all(v["not_slower_than_eager_beyond_spread"] for v in verdict.values()) else 1


if __name__ == "__main__":
    sys.exit(main())

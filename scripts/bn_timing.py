"""What BatchNorm ('bn') costs against InstanceNorm ('in'): graph-replayed train step and eval forward of cfg 2, one JSON line.

    python scripts/bn_timing.py [--steps 20] [--out profiles/bn_timing.json]

Both measured in one run on one device, the cfg-2 architecture (fm 16-32-64-128-256) at 4 x 128^3 in the mixed mode (fp16 forward, bf16 gradients):
* the graph-replayed training step (forward, BCE, backward, AdamW) with normalization 'in' and 'bn', the two alternated in rounds;
* the eval-mode forward (module.eval(), no gradients: BN records from the running buffers, cached) with both;
* per-call HIP-event times of the normalisation finalize entry points in one eager training step of each (L.Profile).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from biapy_amd import _lib as L

FIN = ("bpx_norm_finalize", "bpx_norm_bwd_finalize", "bpx_norm_bwd_finalize_deferred", "bpx_batchnorm_finalize", "bpx_batchnorm_bwd_finalize",
       "bpx_batchnorm_eval_records")


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps          # ms per call


def _model(norm):
    from biapy_amd.resunet import ResUNet

    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "build_model_kwargs.json")))["cfg2_resunet"]
    kw = {k: (tuple(v) if k == "image_shape" else v) for k, v in rec.items()}
    kw.update(normalization=norm, compute_dtype=torch.float16)
    torch.manual_seed(1)
    return ResUNet(**kw).cuda()


def _finalize_profile(m, x, tgt, loss_fn):
    m.train()
    loss_fn(m(x), tgt).backward()
    torch.cuda.synchronize()
    prof = L.Profile(FIN)
    L.lib.prof = prof
    try:
        loss_fn(m(x), tgt).backward()
        torch.cuda.synchronize()
    finally:
        L.lib.prof = None
    out = {}
    for (name, _), (n, ms) in prof.summary().items():
        c = out.setdefault(name, [0, 0.0])
        c[0] += n
        c[1] += ms
    m.zero_grad(set_to_none=True)
    return {k: dict(calls=n, total_us=round(ms * 1e3, 1), us_per_call=round(ms * 1e3 / n, 2)) for k, (n, ms) in sorted(out.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bn_timing.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    from biapy_amd.graphs import GraphedTrainStep
    from biapy_amd.losses import BCEWithLogitsLoss

    B, P = 4, 128
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 1, P, P, P, generator=g).cuda()
    tgt = (torch.rand(B, 1, P, P, P, generator=g) > 0.5).float().cuda()
    loss_fn = BCEWithLogitsLoss()
    models = {n: _model(n) for n in ("in", "bn")}
    prof = {n: _finalize_profile(m, x, tgt, loss_fn) for n, m in models.items()}
    steps = {}
    for n, m in models.items():
        m.train()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-4, fused=True, capturable=True)
        steps[n] = GraphedTrainStep(m, loss_fn, opt, x, tgt)
    train = {n: [] for n in models}
    evalf = {n: [] for n in models}
    for _ in range(a.rounds):                  # alternated: the two configurations see the same machine state
        for n in models:
            train[n].append(_time(steps[n], a.steps))
    for m in models.values():
        m.eval()
    with torch.no_grad():
        for _ in range(a.rounds):
            for n, m in models.items():
                evalf[n].append(_time(lambda: m(x), a.steps))
    tr = {n: min(v) for n, v in train.items()}
    ev = {n: min(v) for n, v in evalf.items()}
    out = dict(what="cfg-2 architecture, 4x128^3, mixed mode (fp16 forward, bf16 gradients); min over alternated rounds of HIP-event ms per call",
               train_step_ms={n: round(v, 3) for n, v in tr.items()}, eval_forward_ms={n: round(v, 3) for n, v in ev.items()},
               train_rounds_ms={n: [round(t, 3) for t in v] for n, v in train.items()}, eval_rounds_ms={n: [round(t, 3) for t in v] for n, v in evalf.items()},
               train_ratio_bn_over_in=round(tr["bn"] / tr["in"], 4), eval_ratio_bn_over_in=round(ev["bn"] / ev["in"], 4),
               bars=dict(train=1.10, eval=1.02), finalize_eager_step=prof, device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Per-sample time of the cfg-2 ResUNet (feature_maps [16, 32, 64, 128, 256], 128^3) as the batch grows past the kernels' 2^31 span, where
the engine runs the batch as sample groups (engine.batch_groups): the mixed-mode train step (forward + BCE + backward, eager) at batches
4, 8 and 12, and the fp16 inference forward at batches 4 and 16.  Writes profiles/large_batch_timing.json.
python scripts/large_batch_timing.py [--reps 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from biapy_amd.engine import NetConfig, ResUNetEngine  # noqa: E402
from oracle import net_oracle  # noqa: E402

FM = [16, 32, 64, 128, 256]
P = (128, 128, 128)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    sd = {k: v.cuda() for k, v in net_oracle.init_state_dict(1, FM, seed=0).items()}
    out = dict(workload="cfg-2 ResUNet, feature_maps %s, %d^3 patches; eager, one process; ms per call and per sample" % (FM, P[0]), train={}, infer={})
    for B in (4, 8, 12):
        eng = ResUNetEngine(NetConfig(in_ch=1, feature_maps=FM), torch.float16)
        x = torch.randn(B, 1, *P, device="cuda")
        tgt = (torch.rand(B, 1, *P, device="cuda") > 0.5).float()

        def step():
            lo, ctx = eng.forward(sd, x, save=True)
            lg = lo.detach().requires_grad_(True)
            F.binary_cross_entropy_with_logits(lg, tgt).backward()
            eng.backward(sd, ctx, lg.grad)

        ms = timed(step, a.reps)
        out["train"][str(B)] = dict(ms=round(ms, 3), ms_per_sample=round(ms / B, 3), groups=eng.last_groups)
        print("train B=%d: %.2f ms, %.3f ms/sample, groups %s" % (B, ms, ms / B, eng.last_groups), flush=True)
        del eng, x, tgt
        torch.cuda.empty_cache()
    for B in (4, 16):
        eng = ResUNetEngine(NetConfig(in_ch=1, feature_maps=FM), torch.float16)
        x = torch.randn(B, 1, *P, device="cuda")
        with torch.no_grad():
            ms = timed(lambda: eng.forward(sd, x, head_act=1, cache_weights=True), a.reps)
        out["infer"][str(B)] = dict(ms=round(ms, 3), ms_per_sample=round(ms / B, 3), groups=eng.last_groups)
        print("infer B=%d: %.2f ms, %.3f ms/sample, groups %s" % (B, ms, ms / B, eng.last_groups), flush=True)
        del eng, x
        torch.cuda.empty_cache()
    t4 = out["train"]["4"]["ms_per_sample"]
    out["train_per_sample_vs_batch4"] = {b: round(v["ms_per_sample"] / t4, 3) for b, v in out["train"].items()}
    i4 = out["infer"]["4"]["ms_per_sample"]
    out["infer_per_sample_vs_batch4"] = {b: round(v["ms_per_sample"] / i4, 3) for b, v in out["infer"].items()}
    path = os.path.join(ROOT, "profiles", "large_batch_timing.json")
    if os.environ.get("LARGE_BATCH_OUT"):
        path = os.environ["LARGE_BATCH_OUT"]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    json.dump(out, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()

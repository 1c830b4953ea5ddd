"""What a wider output head costs: eager HIP-event times of the head kernels and of the graph-replayed training step, one JSON line.

    python scripts/class_head_timing.py [--reps 50] [--steps 20]

* ``bpx_head_fwd`` (fp16 storage, logits only) and ``bpx_head_bwd`` (BPX_MIX16: fp16 x, bf16 dx, fp32 dlogits; the weight-gradient reduction
  included) at 4 x 128^3 voxels for Cout in {1, 4, 8} and Cin in {16, 32}, with the bytes each call moves and the rate that gives;
* the graph-replayed mixed-mode training step (fwd + loss + bwd + AdamW) of the cfg-2 architecture at 4 x 128^3: 1-channel BCE (bench.py's
  step) against 8 channels with CrossEntropyLoss_wrapper(num_classes=8).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from biapy_amd import _lib as L


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps          # us per call


def head_kernels(reps):
    lib, st = L.lib, L.stream_ptr()
    N, vps = 4, 128 ** 3
    rows = []
    for cin in (16, 32):
        x = torch.randn(N * vps, cin, device="cuda").to(torch.float16)
        dx = torch.empty(N * vps, cin, device="cuda", dtype=torch.bfloat16)
        for cout in (1, 4, 8):
            w = torch.randn(cout, cin, device="cuda") * 0.2
            b = torch.zeros(cout, device="cuda")
            out = torch.empty(N, cout, vps, device="cuda")
            dout = torch.randn(N, cout, vps, device="cuda")
            dw = torch.empty(cout, cin, device="cuda")
            db = torch.zeros(cout, device="cuda")
            ws = torch.empty(lib.bpx_head_bwd_workspace(cin, cout), dtype=torch.uint8, device="cuda")

            def fwd():
                L.check(lib.bpx_head_fwd(L.F16, vps, N, L.tview(x), w.data_ptr(), b.data_ptr(), cout, 0, out.data_ptr(), cout * vps, vps, st))

            def bwd():
                L.check(lib.bpx_head_bwd(L.MIX16, vps, N, L.tview(x), w.data_ptr(), cout, dout.data_ptr(), cout * vps, vps, L.tview(dx), dw.data_ptr(),
                                         db.data_ptr(), ws.data_ptr(), ws.numel(), st))

            tf, tb = _time(fwd, reps), _time(bwd, reps)
            bf = N * vps * (cin * 2 + cout * 4)                 # x read, logits written
            bb = N * vps * (cin * 2 + cout * 4 + cin * 2)       # x and dlogits read, dx written
            rows.append(dict(cin=cin, cout=cout, fwd_us=round(tf, 1), fwd_mb=round(bf / 1e6, 1), fwd_tbs=round(bf / tf / 1e6, 2),
                             bwd_us=round(tb, 1), bwd_mb=round(bb / 1e6, 1), bwd_tbs=round(bb / tb / 1e6, 2)))
    return rows


def train_steps(steps):
    from biapy_amd.graphs import GraphedTrainStep
    from biapy_amd.losses import BCEWithLogitsLoss, CrossEntropyLoss_wrapper
    from biapy_amd.resunet import ResUNet

    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "build_model_kwargs.json")))["cfg2_resunet"]
    B, P = 4, 128
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 1, P, P, P, generator=g).cuda()
    res = {}
    for name, n, loss_fn, tgt in (("bce_1ch", 1, BCEWithLogitsLoss(), (torch.rand(B, 1, P, P, P, generator=g) > 0.5).float()),
                                  ("ce_8class", 8, CrossEntropyLoss_wrapper(num_classes=8, ndim=3), torch.randint(0, 8, (B, 1, P, P, P), generator=g).float())):
        kw = {k: (tuple(v) if k == "image_shape" else v) for k, v in rec.items()}
        kw.update(output_channels=[n], head_activations=["ce_sigmoid" if n == 1 else "ce_softmax"], compute_dtype=torch.float16)
        torch.manual_seed(1)
        m = ResUNet(**kw).cuda().train()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, fused=True, capturable=True)
        step = GraphedTrainStep(m, loss_fn, opt, x, tgt.cuda())
        res[name + "_ms_per_step"] = round(_time(step, steps) / 1e3, 3)
        del step, opt, m
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = dict(what="head kernels at 4x128^3 (fwd: fp16 x; bwd: MIX16) and the graph-replayed mixed train step of cfg 2, eager HIP-event times",
               heads=head_kernels(a.reps))
    if a.steps > 0:
        out.update(train_steps(a.steps))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

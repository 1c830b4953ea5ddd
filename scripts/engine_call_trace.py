"""Which C entry points the four engines call, in which order, with which small arguments - and what they compute - as digests that two
revisions of the Python host code can be compared by (the kernels library is the same file for both: BPX_LIB_PATH).

For every configuration below: one eval-mode forward and one training forward + backward through the drop-in module, with `L.lib.prof =
L.Profile()` (the hook tests/test_batchnorm_gpu.py uses) collecting every call.  One JSON line per configuration: the number of launches,
the sha256 of the ordered list of (entry point, Profile key) of the launches and of all calls, and the sha256 of the eval logits, the
training logits and the flat parameter-gradient slab (`engine.last_flat_grad`).  A launch = every call that is not one of the host-side size
and capability queries (`*_workspace`, `*_tiles`, `*_supported`, `*_query`, `*_elems`), which put nothing on the stream: `trace` is the
digest two revisions must share, `all_calls` also covers the queries and tells where a revision asks one more or one less.

    python scripts/engine_call_trace.py --out run.jsonl [--tree OTHER_CHECKOUT] [--only NAME ...]
    python scripts/engine_call_trace.py --merge parent_a.jsonl parent_b.jsonl branch.jsonl --out profiles/engine_steps_trace.txt

`--tree`: import biapy_amd from another checkout (a `git worktree` of the parent commit), each run in a fresh process.  `--merge` writes the
two trace columns side by side and says, per tensor, whether the parent's two runs agree bit for bit and whether the branch matches them.
"""
import argparse
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FM = [16, 32, 64]
QUERY = re.compile(r"(_workspace|_tiles|_supported|_query|_elems)$")
LEAN = ("bpx_conv3d_bwd_fused", "bpx_conv3d_fwd_pool", "bpx_maxpool3d_bwd_r1", "bpx_conv1x1_fwd_split_wgrad")   # the large-level kernels


def configs(torch):
    """(name, module factory, input shape).  ResUNet: depth 2, feature_maps (16, 32, 64), 16^3, batch 2 unless the name says otherwise."""
    from biapy_amd.engine import batch_groups
    from biapy_amd.rcan import rcan
    from biapy_amd.resunet import ResUNet
    from biapy_amd.resunetpp import ResUNetPlusPlus
    from biapy_amd.unet import U_Net

    bf = torch.bfloat16

    def net(cls, shape, fm=FM, dtype=bf, norm="in", drop=0.0, zd=(2, 2), outs=(1,), **kw):
        n = len(fm)
        info = ["".join("BCDEFGHI"[:o]) for o in outs]
        return lambda: cls(image_shape=shape, activation="elu", feature_maps=list(fm), drop_values=[drop] * n, normalization=norm, yx_down=[2] * (n - 1),
                           z_down=list(zd), isotropy=[True] * n, larger_io=False, conv_layers=[2] * n, output_channels=list(outs), output_channel_info=info,
                           head_activations=["ce_sigmoid"] * sum(outs), compute_dtype=dtype, **kw)

    v16 = (16, 16, 16)
    out = []
    for norm in ("in", "gn", "bn"):
        out.append((f"resunet {norm}", net(ResUNet, v16 + (1,), norm=norm), (2, 1) + v16))
    for name, dt in (("fp16", torch.float16), ("fp32", torch.float32)):
        out.append((f"resunet {name}", net(ResUNet, v16 + (1,), dtype=dt), (2, 1) + v16))
    for c in (3, 16):
        out.append((f"resunet in_ch {c}", net(ResUNet, v16 + (c,)), (2, c) + v16))
    out.append(("resunet dropout 0.1", net(ResUNet, v16 + (1,), drop=0.1), (2, 1) + v16))
    out.append(("resunet post_up 2", net(ResUNet, v16 + (1,), upsampling_factor=(2, 2, 2), upsampling_position="post"), (2, 1) + v16))
    out.append(("resunet 2d 32^2", net(ResUNet, (32, 32, 1)), (2, 1, 32, 32)))
    out.append(("resunet z_down (1, 2)", net(ResUNet, v16 + (1,), zd=(1, 2)), (2, 1) + v16))
    out.append(("resunet heads (1, 2)", net(ResUNet, v16 + (1,), outs=(1, 2)), (2, 1) + v16))
    out.append(("resunet fm (48, 64, 80)", net(ResUNet, v16 + (1,), fm=(48, 64, 80)), (2, 1) + v16))
    out.append(("resunet fm (20, 36, 52)", net(ResUNet, v16 + (1,), fm=(20, 36, 52)), (2, 1) + v16))
    out.append(("resunet 64^3 batch 1", net(ResUNet, (64,) * 3 + (1,)), (1, 1, 64, 64, 64)))     # the smallest cubic patch whose trace holds all of LEAN
    probe = net(ResUNet, (64,) * 3 + (1,))().cfg
    B2 = next(b for b in range(2, 4096) if len(batch_groups(probe, bf, b, (64,) * 3, True)) == 2)
    out.append((f"resunet 64^3 batch {B2} (two sample groups)", net(ResUNet, (64,) * 3 + (1,)), (B2, 1, 64, 64, 64)))
    out.append(("unet 3d", net(U_Net, v16 + (1,)), (2, 1) + v16))
    out.append(("unet 2d 32^2", net(U_Net, (32, 32, 1)), (2, 1, 32, 32)))
    out.append(("resunet++ 16x32x32", net(ResUNetPlusPlus, (16, 32, 32, 1), outs=(3,), k_size=3, upsample_layer="convtranspose"), (2, 1, 16, 32, 32)))
    for scale, s in ((0, 16), (2, 32)):     # the up-scaling stage's kernel (bpx_conv3d_fwd_shuffle) takes volumes from 32^3
        out.append((f"rcan scale {scale} {s}^3", lambda scale=scale: rcan(3, num_channels=1, filters=16, scale=scale or 2, num_rg=1, num_rcab=2, reduction=4,
                                                                          upscaling_layer=bool(scale), head_activations=["linear"], compute_dtype=bf),
                    (2, 1, s, s, s)))
    return out


def sha(t):
    import torch

    return hashlib.sha256(t.detach().to(torch.float32).contiguous().cpu().numpy().tobytes()).hexdigest()


def run(a):
    sys.path.insert(0, os.path.abspath(a.tree or ROOT))
    import torch

    from biapy_amd import _lib as L

    assert torch.cuda.is_available(), "engine_call_trace.py traces runs on the MI355X"
    dev = torch.device("cuda", 0)
    with open(a.out, "w") as f:
        for name, make, shape in configs(torch):
            if a.only and not any(o in name for o in a.only):
                continue
            torch.manual_seed(0)
            m = make().to(dev)
            x = torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
            prof = L.lib.prof = L.Profile()
            try:
                with torch.no_grad():
                    y_eval = m.eval()(x)
                y = m.train()(x)
                (y * torch.linspace(-1, 1, y.numel(), device=dev).view(y.shape)).sum().backward()
                torch.cuda.synchronize()
            finally:
                L.lib.prof = None
            calls = [(r[0], list(r[1])) for r in prof.records]
            launches = [c for c in calls if not QUERY.search(c[0])]
            rec = dict(config=name, calls=len(launches), trace=hashlib.sha256(json.dumps(launches).encode()).hexdigest(),
                       all_calls=hashlib.sha256(json.dumps(calls).encode()).hexdigest(),
                       lean=[k for k in LEAN if any(c[0] == k for c in calls)], groups=len(m._engine.last_groups) if hasattr(m._engine, "last_groups") else 1,
                       logits_eval=sha(y_eval), logits_train=sha(y), flat_grad=sha(m._engine.last_flat_grad))
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
            del m, x, y, y_eval, prof
            torch.cuda.empty_cache()


def merge(a):
    pa, pb, br = ([json.loads(s) for s in open(p)] for p in a.merge)
    lines = ["Engine call traces (scripts/engine_call_trace.py): sha256 of the ordered (entry point, Profile key) list of the launches of one eval forward",
             "and one training forward + backward per configuration, parent commit and this commit on one library file, fresh processes.  `queries`:",
             "whether the list that also holds the host-side size / capability queries is the same.  Tensors: `same` = the parent's two runs agree",
             "bit for bit and the branch gives the same hash; `parent varies` = the parent's own two runs differ.", ""]
    ok = True
    for p1, p2, b in zip(pa, pb, br):
        assert p1["config"] == p2["config"] == b["config"]
        same = p1["trace"] == p2["trace"] == b["trace"] and p1["calls"] == b["calls"]
        ok &= same
        tens = []
        for k in ("logits_eval", "logits_train", "flat_grad"):
            v = "parent varies" if p1[k] != p2[k] else "same" if b[k] == p1[k] else "DIFFERS"
            ok &= v != "DIFFERS"
            tens.append(f"{k} {v}")
        lines.append(f"{b['config']}: {b['calls']} launches, {b['groups']} group(s), large-level kernels {len(b['lean'])}/{len(LEAN)}")
        lines.append(f"   parent {p1['trace']}")
        lines.append(f"   branch {b['trace']}  {'equal' if same else 'NOT EQUAL'}, queries {'equal' if b['all_calls'] == p1['all_calls'] else 'differ'};  " + ", ".join(tens))
    lines.append("")
    lines.append("every digest equal, every reproducible tensor identical" if ok else "MISMATCH (see above)")
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--merge", nargs=3, default=None, metavar=("PARENT_A", "PARENT_B", "BRANCH"))
    a = ap.parse_args()
    sys.exit(merge(a) if a.merge else run(a))

"""What the fused Dice + CE loss costs beside the cross entropy alone: kernel times of dice_sums_kernel / dice_bwd_kernel (class mode, CE mixed in)
and of softmax_ce_sums_kernel / softmax_ce_bwd_kernel on the same tensors, 4 x C x 128^3 for C = 3 and C = 8.

    python scripts/dice_loss_timing.py [--reps 20] [--out profiles/dice_losses.txt]

Each channel count runs as a child process of its own under ``rocprofv3 --kernel-trace --stats`` (the kernel names of the cross entropy do not carry
C); the child rotates through four sets of tensors so that no call finds its operands in the 256 MB Infinity Cache.  Reported per kernel: the median
of the traced durations, the algorithmic bytes - (C + 1) 4 N vox forward (logits and labels read), (2 C + 1) 4 N vox backward (logits and labels
read, dlogits written) - over that time, and its share of the 6.3 TB/s the streaming kernels can reach.  One derived condition: the fused sums pass
must take less than twice the cross-entropy sums pass of the same run; otherwise fusing bought nothing over two passes.
"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, VOX, SETS, PEAK = 4, 128 ** 3, 4, 6.3e12
KERNELS = ("dice_sums_kernel", "softmax_ce_sums_kernel", "dice_bwd_kernel", "softmax_ce_bwd_kernel")
CHANNEL = ("dice_sums_kernel[channel]", "dice_bwd_kernel[channel]")       # the channel-mode instances (sigmoid + BCE), reported beside them


def _key(name):
    """The row a traced kernel name belongs to: the class-mode instances carry `true` (or Lb1 in a mangled name) as their second template argument."""
    import re
    for k in KERNELS:
        if k in name:
            if k.startswith("dice_") and not re.search(r"kernel<\d+, ?(true|1)\b|kernelILi\dELb1", name):
                return k + "[channel]"
            return k
    return None


def worker(C, reps):
    import torch

    from biapy_amd import _lib as L
    lib, st = L.lib, L.stream_ptr()
    g = torch.Generator().manual_seed(C)
    sets = []
    for _ in range(SETS):
        z = (torch.randn(N, C, VOX, generator=g) * 2).cuda()
        t = torch.randint(0, C, (N, 1, VOX), generator=g).float().cuda()
        sets.append((z, t, torch.empty_like(z)))
    chan_t = [(torch.rand(N, C, VOX, generator=g) > 0.6).float().cuda() for _ in range(2)]
    coef2 = torch.empty(24, device="cuda")
    nb, row = lib.bpx_dice_blocks(VOX), lib.bpx_dice_row()
    part = torch.empty(N * nb, row, device="cuda")
    sums, coef, loss, gup = torch.empty(row, dtype=torch.float64, device="cuda"), torch.empty(24, device="cuda"), torch.empty((), device="cuda"), torch.ones((), device="cuda")
    nbc, rowc = lib.bpx_softmax_ce_blocks(VOX), lib.bpx_softmax_ce_row()
    partc = torch.empty(N * nbc, rowc, device="cuda")
    sumsc, lossc = torch.empty(rowc, dtype=torch.float64, device="cuda"), torch.empty((), device="cuda")
    for i in range(reps + 2):                         # the first two rounds warm up; the parent drops them from the trace
        z, t, dz = sets[i % SETS]
        L.check(lib.bpx_dice_sums(z.data_ptr(), t.data_ptr(), N, C, VOX, 1, -100, None, 1, part.data_ptr(), st))
        L.check(lib.bpx_dice_finish(part.data_ptr(), N, C, VOX, 1, 1, 1.0, 1.0, 1e-5, sums.data_ptr(), coef.data_ptr(), loss.data_ptr(), st))
        z, t, dz = sets[(i + 1) % SETS]
        L.check(lib.bpx_softmax_ce_sums(z.data_ptr(), t.data_ptr(), N, C, VOX, -100, None, partc.data_ptr(), st))
        L.check(lib.bpx_softmax_ce_finish(partc.data_ptr(), N, VOX, sumsc.data_ptr(), lossc.data_ptr(), st))
        z, t, dz = sets[(i + 2) % SETS]
        L.check(lib.bpx_dice_bwd(z.data_ptr(), t.data_ptr(), N, C, VOX, 1, 1, -100, None, coef.data_ptr(), gup.data_ptr(), dz.data_ptr(), st))
        z, t, dz = sets[(i + 3) % SETS]
        L.check(lib.bpx_softmax_ce_bwd(z.data_ptr(), t.data_ptr(), N, C, VOX, -100, None, sumsc.data_ptr(), gup.data_ptr(), dz.data_ptr(), st))
        z, tc, dz = sets[i % SETS][0], chan_t[i % 2], sets[i % SETS][2]          # channel mode: a target of the logits' shape
        L.check(lib.bpx_dice_sums(z.data_ptr(), tc.data_ptr(), N, C, VOX, 0, -100, None, 1, part.data_ptr(), st))
        L.check(lib.bpx_dice_finish(part.data_ptr(), N, C, VOX, 0, 1, 1.0, 1.0, 1e-5, sums.data_ptr(), coef2.data_ptr(), loss.data_ptr(), st))
        z, tc, dz = sets[(i + 2) % SETS][0], chan_t[(i + 1) % 2], sets[(i + 2) % SETS][2]
        L.check(lib.bpx_dice_bwd(z.data_ptr(), tc.data_ptr(), N, C, VOX, 0, 1, -100, None, coef2.data_ptr(), gup.data_ptr(), dz.data_ptr(), st))
    torch.cuda.synchronize()
    print("worker done", C, float(loss), float(lossc))


def profile(C, reps):
    """{kernel: median microseconds} of one traced child run."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", f"c{C}", "--", sys.executable, os.path.abspath(__file__),
               "--worker", str(C), "--reps", str(reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        traces = glob.glob(os.path.join(d, "**", f"c{C}_kernel_trace.csv"), recursive=True)
        if not traces:
            raise RuntimeError("rocprofv3 wrote no kernel trace:\n" + r.stderr[-2000:])
        durs = {k: [] for k in KERNELS + CHANNEL}
        for rec in csv.DictReader(open(traces[0])):
            k = _key(rec["Kernel_Name"])
            if k is not None:
                durs[k].append((int(rec["Start_Timestamp"]), int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])))
        out = {}
        for k, v in durs.items():
            v = [dt for _, dt in sorted(v)][2:]            # in launch order, without the two warm-up rounds
            if len(v) != reps and k in KERNELS:
                raise RuntimeError(f"{k}: {len(v)} traced calls, expected {reps}")
            if not v:
                continue
            out[k] = (statistics.median(v) / 1e3, min(v) / 1e3, max(v) / 1e3)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dice_losses.txt"))
    ap.add_argument("--worker", type=int, default=0)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.reps)
    lines = [f"Dice + CE loss kernels beside the cross entropy, {N} x C x 128^3 fp32 logits, class mode, rocprofv3 --kernel-trace, median of {a.reps} calls (min .. max),",
             "operands rotated through four tensor sets (no call finds them in the Infinity Cache); bytes = algorithmic: (C + 1) 4 N vox fwd, (2 C + 1) 4 N vox bwd;",
             "share = of 6.3 TB/s", ""]
    ok = True
    for C in (3, 8):
        t = profile(C, a.reps)
        for k in KERNELS:
            nbytes = ((2 * C + 1) if "bwd" in k else (C + 1)) * 4 * N * VOX
            med, lo, hi = t[k]
            rate = nbytes / (med * 1e-6)
            lines.append(f"C={C} {k:24s} {med:8.1f} us ({lo:.1f} .. {hi:.1f})  {nbytes / 1e6:7.1f} MB  {rate / 1e12:5.2f} TB/s  {100 * rate / PEAK:5.1f} %")
        for k in CHANNEL:
            if k in t:
                nbytes = ((3 * C) if "bwd" in k else (2 * C)) * 4 * N * VOX           # logits and a target of their shape read (+ dlogits written)
                med, lo, hi = t[k]
                rate = nbytes / (med * 1e-6)
                lines.append(f"C={C} {k:24s} {med:8.1f} us ({lo:.1f} .. {hi:.1f})  {nbytes / 1e6:7.1f} MB  {rate / 1e12:5.2f} TB/s  {100 * rate / PEAK:5.1f} %")
        ratio = t["dice_sums_kernel"][0] / t["softmax_ce_sums_kernel"][0]
        good = ratio < 2.0
        ok = ok and good
        lines.append(f"C={C} fused Dice + CE sums / cross-entropy sums = {ratio:.2f} (condition: < 2) -> {'holds' if good else 'DOES NOT HOLD'}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(a.out, "w") as f:
        f.write(text)
    if not ok:
        sys.exit("the fused sums pass takes twice the cross-entropy pass or more: fusing bought nothing over two passes")


if __name__ == "__main__":
    main()

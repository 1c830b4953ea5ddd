"""What the instance-segmentation targets cost on the device: microseconds per call of InstanceTargets for ("F", "C", "D") and for all seven
channels, at B = 2 and 4, on 80^3 (the benched configuration's patch) and 128^3 blobs; the share of each stage - ids, the distance transform (3
launches per sample), the records (init, accumulate, finish, and the rcmax pass when "Dc" is asked for), pack - each timed on its own on the
generator's scratch; and, in the same run, a ``torch.empty_like(target).copy_(target)`` of the same bytes as the memory-rate yardstick of the pack
kernel (it reads and writes what pack only writes).  Configurations alternated, 40 repetitions per reading, three readings each (HIP events),
medians.  Eager calls: the host's share (argument checks, ctypes) is inside, and back-to-back repetitions re-use a working set that fits the
last-level cache in part.  No threshold: the numbers are recorded.  Writes profiles/itarget_timing.json.
python scripts/itarget_timing.py [--steps 40] [--rounds 3]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from biapy_amd import _lib as L  # noqa: E402
from biapy_amd.targets import CONTOUR_MODES, InstanceTargets  # noqa: E402

lib = L.lib
ALL7 = ("F", "C", "D", "Dc", "H", "V", "Z")


def timed(fn, n, warm=1):
    """us per call of n back-to-back calls between two HIP events (`warm` calls first)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def blobs(B, P, count, dev):
    """float32 ids (B, P, P, P, 1): balls of radius 6..14 around random centres, a later ball over an earlier one."""
    g = torch.Generator(device=dev).manual_seed(0)
    ax = torch.arange(P, device=dev, dtype=torch.float32)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    t = torch.zeros((B, P, P, P), device=dev)
    for b in range(B):
        c = torch.rand((count, 3), device=dev, generator=g) * P
        r = 6 + 8 * torch.rand(count, device=dev, generator=g)
        for i in range(count):
            t[b][(z - c[i, 0]) ** 2 + (y - c[i, 1]) ** 2 + (x - c[i, 2]) ** 2 <= r[i] ** 2] = i + 1
    return t[..., None].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "itarget_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "itarget_timing.py measures on the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda", 0)
    rows = []
    for P in (80, 128):
        count = 60 if P == 80 else 240
        for B in (2, 4):
            t = blobs(B, P, count, dev)
            for ch in (("F", "C", "D"), ALL7):
                it = InstanceTargets(ch, n_max=count)
                target = torch.empty((B, len(ch), P, P, P), device=dev)
                it(None, t, out=target)
                V, s = P ** 3, L.stream_ptr()
                ws_bytes = it._ws.numel()

                def ids():
                    L.check(lib.bpx_itarget_ids(t.data_ptr(), L.F32, B * V, count, it._ids.data_ptr(), it._faults.data_ptr(), s))

                def edt():
                    for b in range(B):
                        L.check(lib.bpx_edt(it._ids.data_ptr() + 4 * b * V, L.I32, 1, P, P, P, None, 0, it._dist.data_ptr() + 4 * b * V, it._ws.data_ptr(), ws_bytes, s))

                def stats():
                    L.check(lib.bpx_itarget_stats(it._ids.data_ptr(), it._dist.data_ptr(), B, P, P, P, count, None, 1 if "Dc" in ch else 0, it._rec.data_ptr(), s))

                def pack():
                    L.check(lib.bpx_itarget_pack(it._ids.data_ptr(), it._dist.data_ptr(), it._rec.data_ptr(), B, P, P, P, count, it.codes, len(ch), 3, 1,
                                                 CONTOUR_MODES["thick"], 0, 0.0, None, target.data_ptr(), s))

                fns = {"call": lambda: it(None, t, out=target), "ids": ids, "edt": edt, "stats": stats, "pack": pack,
                       "torch copy of the target": lambda: torch.empty_like(target).copy_(target)}
                readings = {k: [] for k in fns}
                for r in range(a.rounds):
                    for k, fn in fns.items():
                        readings[k].append(timed(fn, a.steps))
                med = {k: round(statistics.median(v), 1) for k, v in readings.items()}
                stages = sum(med[k] for k in ("ids", "edt", "stats", "pack"))
                row = dict(patch=P, batch=B, channels="".join(ch), labels_drawn=count, us=med,
                           spread_us={k: round(max(v) - min(v), 1) for k, v in readings.items()},
                           share={k: round(med[k] / stages, 3) for k in ("ids", "edt", "stats", "pack")},
                           target_bytes=target.numel() * 4, pack_over_copy=round(med["pack"] / med["torch copy of the target"], 2))
                print(json.dumps(row), flush=True)
                rows.append(row)
    out = dict(workload=f"float32 ids of random balls; {a.steps} repetitions per reading, {a.rounds} readings per configuration, configurations "
                        "alternated, medians; eager calls on the current stream, unit grid, thick contour of connectivity 1",
               device=torch.cuda.get_device_name(0), rows=rows,
               note="share: a stage's median over the sum of the four stages' medians; the torch copy reads and writes the target's bytes once each, pack "
                    "writes them once and reads 8 bytes per voxel plus the neighbours' ids and the instance's record from cache")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

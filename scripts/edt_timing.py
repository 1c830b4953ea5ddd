"""What the exact Euclidean distance transform costs on the device, against the host path a user has without it.  One box, one call, the two
modes alternated, 20 calls per reading, three readings each (HIP events, after a warm-up call):
  (binary) prepost.distance_transform_edt of the uint8 mask, float32 distances (the exact integer path);
  (label)  prepost.label_distance of the int32 labels prepost.label made of the same mask, float32 distances;
  (host)   the same input through the host: device-to-host copy, scipy.ndimage.distance_transform_edt (label mode: once per label over the
           label's bounding box grown by one voxel), float32 host-to-device copy - timed once per input with the wall clock.
Masks: random balls of radius 3..9 at about 30 % fill.  256^3 and 512^3 are measured against the host path (at 512^3 in binary mode only: the
per-label SciPy loop is too slow there to be worth timing) and the device result is compared with SciPy's bit for bit; 1024^3 (the 512^3 mask
tiled 2 x 2 x 2) is timed on the device only.
The device time is set against the traffic floor of the call - the keys read once (1 or 4 bytes) and 4 bytes written per voxel - at the
4.5 TB/s yardstick of the project's streaming passes.  What the three passes move per voxel on the integer path (k = key bytes):
  row pass   k read twice (the second sweep from cache) + 4 written, 4 read, 4 written                              = 12 + 2 k
  Y pass     k + 4 read, 4 written per foreground voxel, + the envelope stack: <= 8 written and 8 read per foreground voxel
  Z pass     the same
so 28 + 4 k bytes per voxel besides the stacks, which stay in the last-level cache (they are as small as the threads in flight).  Back-to-back
calls at 256^3 work on 84 MB of mask and output, all of it inside the 256 MiB last-level cache: not an HBM figure.
There is one form of the kernels, so the only condition is: the device call is faster than the host path on every input measured.  Exit
status 1 otherwise.  Writes profiles/edt_timing.json.
python scripts/edt_timing.py [--calls 20] [--rounds 3] [--no-1024]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy import ndimage  # noqa: E402

from biapy_amd import prepost  # noqa: E402

STREAM_TBPS = 4.5


def balls(n, fill=0.3, seed=0, rmin=3, rmax=9):
    rng = np.random.default_rng(seed)
    m = np.zeros((n, n, n), bool)
    vol = np.mean([4.19 * r ** 3 for r in range(rmin, rmax + 1)])
    for _ in range(int(-np.log(1 - fill) * n ** 3 / vol)):
        r = int(rng.integers(rmin, rmax + 1))
        c = [int(rng.integers(0, n)) for _ in range(3)]
        lo, hi = [max(0, v - r) for v in c], [min(n, v + r + 1) for v in c]
        g = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= (g[0] - c[0]) ** 2 + (g[1] - c[1]) ** 2 + (g[2] - c[2]) ** 2 <= r * r
    return m.view(np.uint8)


def timed(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def host_binary(mask_np):
    return ndimage.distance_transform_edt(mask_np).astype(np.float32)


def host_labels(lab):
    out = np.zeros(lab.shape, np.float32)
    for l, box in enumerate(ndimage.find_objects(lab), start=1):
        if box is None:
            continue
        grown = tuple(slice(max(0, s.start - 1), min(n, s.stop + 1)) for s, n in zip(box, lab.shape))
        m = lab[grown] == l
        out[grown][m] = ndimage.distance_transform_edt(m)[m]
    return out


def host_path(name, dev_in, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = dev_in.cpu().numpy()
    t1 = time.perf_counter()
    want = fn(host)
    t2 = time.perf_counter()
    back = torch.from_numpy(want).cuda()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    ms = dict(d2h=round((t1 - t0) * 1e3, 1), scipy=round((t2 - t1) * 1e3, 1), h2d=round((t3 - t2) * 1e3, 1), total=round((t3 - t0) * 1e3, 1))
    print(f"{name}: host path {ms}", flush=True)
    return ms, back


def measure(size, mask_np, calls, rounds, host_modes):
    m = torch.from_numpy(mask_np).cuda()
    lab = prepost.label(m)
    n = m.numel()
    runs = {"binary": lambda: prepost.distance_transform_edt(m), "label": lambda: prepost.label_distance(lab)}
    inputs = {"binary": (m, host_binary, 1), "label": (lab, host_labels, 4)}
    res = {}
    for mode, run in runs.items():
        name = f"balls {size}^3 {mode}"
        dev_in, fn, kbytes = inputs[mode]
        out = dict(voxels=n, fill=round(float(mask_np.mean()), 4), labels=int(lab.max()), floor_ms=round(n * (kbytes + 4) / (STREAM_TBPS * 1e12) * 1e3, 4))
        got = run()                                                    # the warm-up call
        if mode in host_modes:
            out["host_ms"], want = host_path(name, dev_in, fn)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"{name}: the device result differs from SciPy's"
            print(f"{name}: equals SciPy bit for bit, largest distance {float(got.max()):.3f}", flush=True)
            del want
        print(f"{name}: one call {timed(run, 1):.2f} ms", flush=True)
        del got
        res[name] = out
    readings = {mode: [] for mode in runs}
    for r in range(rounds):
        for mode, run in runs.items():
            readings[mode].append(timed(run, calls))
            print(f"balls {size}^3 {mode}: round {r + 1}: {readings[mode][-1]:.3f} ms", flush=True)
    for mode, vs in readings.items():
        out = res[f"balls {size}^3 {mode}"]
        med = sorted(vs)[len(vs) // 2]
        out.update(readings_ms=[round(v, 4) for v in vs], median_ms=round(med, 4), spread_ms=round(max(vs) - min(vs), 4), over_floor=round(med / out["floor_ms"], 1))
        if "host_ms" in out:
            out["host_over_device"] = round(out["host_ms"]["total"] / med, 1)
    del m, lab
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-1024", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edt_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "edt_timing.py measures on the MI355X; there is nothing to measure without it"
    res = {}
    res.update(measure(256, balls(256), a.calls, a.rounds, ("binary", "label")))
    b512 = balls(512)
    res.update(measure(512, b512, a.calls, a.rounds, ("binary",)))
    if not a.no_1024:
        res.update(measure(1024, np.tile(b512, (2, 2, 2)), a.calls, a.rounds, ()))
    faster = bool(all(v["median_ms"] < v["host_ms"]["total"] for v in res.values() if "host_ms" in v))
    out = dict(
        workload=f"prepost.distance_transform_edt (uint8 mask) and prepost.label_distance (int32 labels) resident on the device, float32 distances, "
                 f"exact integer path; {a.calls} calls per reading, {a.rounds} readings per mode, modes alternated; one box, one call; host path timed once",
        device=torch.cuda.get_device_name(0), inputs=res, conditions={"device call faster than the host path on every input measured": faster},
        yardstick_tbps=STREAM_TBPS,
        note="floor = keys read once (1 or 4 bytes) + 4 bytes written per voxel; the three passes move 28 + 4 k bytes per voxel besides the envelope "
             "stacks (module docstring); back-to-back calls at 256^3 work on 84 MB, inside the 256 MiB last-level cache: not an HBM figure",
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))
    print("wrote", a.out)
    return 0 if faster else 1


if __name__ == "__main__":
    sys.exit(main())

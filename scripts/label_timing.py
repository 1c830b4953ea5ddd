"""What labelling the connected components of a binarised volume costs on the device, against the host path a user has without it.  One box,
one call, the configurations alternated, 20 calls per reading, three readings each (HIP events, after a warm-up call):
  (tiled)  prepost.label with the tiled merge (tiles resolved in LDS, then unions across tile borders);
  (global) the same call with the global-only merge (bpx_debug_set_label_tiled(0)); same bits, checked here;
  (host)   the same mask through the host: device-to-host copy of the uint8 mask, scipy.ndimage.label with the same structure, host-to-device
           copy of the int32 labels - timed once per mask with the wall clock.
Masks, at 512^3 and (unless --no-1024) at 1024^3: random balls of radius 3..9 at about 30 % fill, full connectivity (the realistic one; the
1024^3 one is the 512^3 one tiled 2 x 2 x 2), and ``random < 0.5`` at connectivity 1 (a hard one: far above the percolation threshold, one
ragged giant component and many small ones).  The labels of the first call of every configuration are compared with SciPy's.
The device time is set against the traffic floor of the call - 1 byte read and 4 bytes written per voxel - at the 4.5 TB/s yardstick of the
project's streaming passes.  Back-to-back calls at 512^3 work on 671 MB of mask and labels, part of which may still sit in
the 256 MiB last-level cache: not an HBM figure.
Conditions: (1) the device call (the library's default form) is faster than the host path on both masks at every shape; (2) the tiled form
deserves to be the default: its median reading is below the global-only form's by more than the spread of the three readings, on the realistic
mask at the largest shape measured.  Exit status 1 if (1) fails or (2) disagrees with the library's default.  Writes profiles/label_timing.json
and appends the component counts seen to profiles/label_values.txt.
python scripts/label_timing.py [--calls 20] [--rounds 3] [--no-1024]"""
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

from biapy_amd import _lib as L  # noqa: E402
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


def measure(name, mask_np, conn, calls, rounds, default_tiled):
    m = torch.from_numpy(mask_np).cuda()
    n = m.numel()
    # the host path, once
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = m.cpu().numpy()
    t1 = time.perf_counter()
    want, count = ndimage.label(host, structure=ndimage.generate_binary_structure(3, conn))
    t2 = time.perf_counter()
    back = torch.from_numpy(want.astype(np.int32, copy=False)).cuda()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    host_ms = dict(d2h_mask=round((t1 - t0) * 1e3, 1), scipy_label=round((t2 - t1) * 1e3, 1), h2d_labels=round((t3 - t2) * 1e3, 1), total=round((t3 - t0) * 1e3, 1))
    print(f"{name}: host path {host_ms}", flush=True)
    forms = {"tiled": 1, "global": 0}
    readings = {k: [] for k in forms}
    try:
        for k, on in forms.items():                                        # warm-up call of each form, checked against SciPy
            L.lib.bpx_debug_set_label_tiled(on)
            lab, num = prepost.label(m, conn, return_num=True)
            assert int(num) == count and torch.equal(lab, back), f"{name}: the {k} form disagrees with SciPy"
            t = timed(lambda: prepost.label(m, conn), 1)
            print(f"{name}: {k} form equals SciPy ({count} components), one call {t:.2f} ms", flush=True)
            del lab
        for r in range(rounds):
            for k, on in forms.items():
                L.lib.bpx_debug_set_label_tiled(on)
                readings[k].append(timed(lambda: prepost.label(m, conn), calls))
                print(f"{name}: round {r + 1} {k}: {readings[k][-1]:.3f} ms", flush=True)
    finally:
        L.lib.bpx_debug_set_label_tiled(1 if default_tiled else 0)
    floor_ms = n * 5 / (STREAM_TBPS * 1e12) * 1e3
    out = dict(voxels=n, connectivity=conn, components=int(count), fill=round(float(mask_np.mean()), 4), host_ms=host_ms, floor_ms=round(floor_ms, 4))
    for k, vs in readings.items():
        med = sorted(vs)[len(vs) // 2]
        out[k] = dict(readings_ms=[round(v, 4) for v in vs], median_ms=round(med, 4), spread_ms=round(max(vs) - min(vs), 4),
                      over_floor=round(med / floor_ms, 1), host_over_device=round(host_ms["total"] / med, 1))
    del m, back
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-1024", action="store_true")
    ap.add_argument("--default-tiled", type=int, default=0, help="the library's default form (1 tiled, 0 global-only): what condition (2) is held against")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_timing.json"))
    ap.add_argument("--values", default=os.path.join(ROOT, "profiles", "label_values.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "label_timing.py measures on the MI355X; there is nothing to measure without it"
    default = "tiled" if a.default_tiled else "global"
    b512 = balls(512)
    res = {}
    for size in (512,) if a.no_1024 else (512, 1024):
        realistic = b512 if size == 512 else np.tile(b512, (2, 2, 2))
        hard = (np.random.default_rng(size).random((size, size, size), dtype=np.float32) < 0.5).view(np.uint8)
        res[f"balls {size}^3"] = measure(f"balls {size}^3", realistic, 3, a.calls, a.rounds, bool(a.default_tiled))
        res[f"random 0.5 {size}^3"] = measure(f"random 0.5 {size}^3", hard, 1, a.calls, a.rounds, bool(a.default_tiled))
        del realistic, hard
    judge = res[[k for k in res if k.startswith("balls")][-1]]
    gap = judge["global"]["median_ms"] - judge["tiled"]["median_ms"]
    spread = max(judge["tiled"]["spread_ms"], judge["global"]["spread_ms"])
    tiled_wins = bool(gap > spread)
    cond = {
        "1 device call faster than the host path on every mask": bool(all(v[default]["median_ms"] < v["host_ms"]["total"] for v in res.values())),
        "2 tiled below global-only by more than the spread (realistic mask, largest shape)": tiled_wins,
        "2 agrees with the library's default": bool(tiled_wins == bool(a.default_tiled)),
    }
    out = dict(
        workload=f"prepost.label of a uint8 mask resident on the device, int32 labels; {a.calls} calls per reading, {a.rounds} readings per form, forms "
                 f"alternated; one box, one call; host path timed once per mask",
        device=torch.cuda.get_device_name(0), default_form=default, masks=res, conditions=cond,
        tiled_minus_global_ms=round(-gap, 4), spread_ms=round(spread, 4), yardstick_tbps=STREAM_TBPS,
        note="floor = 1 byte read + 4 bytes written per voxel; the call makes six passes (DESIGN.md section 4 lists their traffic); back-to-back calls "
             "at 512^3 work on 671 MB, part of which may sit in the 256 MiB last-level cache: not an HBM figure",
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    with open(a.values, "a") as f:
        f.write("scripts/label_timing.py: components seen (device == scipy.ndimage.label, both forms)\n")
        for k, v in res.items():
            f.write(f"  {k}: connectivity {v['connectivity']}, fill {v['fill']}, N = {v['components']}\n")
    print(json.dumps(out, indent=1))
    print("wrote", a.out)
    return 0 if cond["1 device call faster than the host path on every mask"] and cond["2 agrees with the library's default"] else 1


if __name__ == "__main__":
    sys.exit(main())

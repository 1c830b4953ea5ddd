"""What the seeded watershed costs on the device, against the host path a user has without it.  One box, one call form; per input 20 calls per
reading, three readings (HIP events, after a warm-up call); fewer calls per reading where one call takes long enough to be read without them (the
count used is recorded).
Inputs: random balls of radius 3..9 at about 30 % fill as the mask; the pipeline of INTEGRATION.md builds the rest on the device - the squared
distance d2 of the mask (prepost.distance_transform_edt), seeds = prepost.label of the eroded core d2 > 8, image = -d2 (int32).  256^3 and 512^3;
1024^3 (the 512^3 mask tiled 2 x 2 x 2) on the device only.  Before anything is timed the device result is compared bit for bit with the twin
(tests/watershed_ref.py) on a 40^3 crop of the 256^3 input.
Recorded per input: the call's time; the rounds that did work against R = ceil(log2(max(n, 2))) + 1 launched; the time of a call in which NO
round does work (every voxel a marker: the flag kernel, init, round 0's pick, which finds every tree seeded, 4 R - 1 launches that return at
once, the last pass) - what the R - rounds idle rounds cost, and more; the workspace; the ratio to the traffic floor of image + markers + mask read once and 4 bytes written per voxel (13 bytes) at the
4.5 TB/s yardstick of the project's streaming passes.
(host) at 256^3: device-to-host copies, scipy.ndimage.watershed_ift on a uint16 quantisation of the same image with the outside of the mask as a
background marker, host-to-device copy - wall clock, once.  watershed_ift is the marker-controlled watershed this machine's SciPy offers; it
breaks ties by ANOTHER rule (and is not the reference's scikit-image function), so its labels are not compared, only its time.
The one condition: the device call is faster than that host path on every input measured.  Exit status 1 otherwise.  Pass A (pick) has one form:
one 64-bit atomic min per voxel that found an edge, skipped when the root already holds a smaller key; a wave-level pre-reduction of lanes that
share a root was not built.  Writes profiles/watershed_timing.json; --sizes runs a subset and merges into the file.
python scripts/watershed_timing.py [--calls 20] [--rounds 3] [--sizes 256 512 1024]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy import ndimage  # noqa: E402

from biapy_amd import _lib as L  # noqa: E402
from biapy_amd import prepost  # noqa: E402

STREAM_TBPS = 4.5
CORE_D2 = 8


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


def pipeline(mask):
    d2 = prepost.distance_transform_edt(mask, squared=True)
    seeds = prepost.label((d2 > CORE_D2).to(torch.uint8), connectivity=1)
    return -d2, seeds


def check_crop(mask_np):
    import watershed_ref as W

    m = torch.from_numpy(np.ascontiguousarray(mask_np[:40, :40, :40])).cuda()
    image, seeds = pipeline(m)
    got = prepost.watershed(image, seeds, m).cpu().numpy()
    want = W.watershed_ref(image.cpu().numpy(), seeds.cpu().numpy(), m.cpu().numpy(), 1)
    assert np.array_equal(got, want), "the device result differs from the twin's on the 40^3 crop"
    print(f"40^3 crop: equals the twin bit for bit, {int(seeds.max())} seeds, {float((got > 0).mean()):.3f} of the voxels labelled", flush=True)


def host_path(name, image, seeds, mask):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    im, mk, m = image.cpu().numpy(), seeds.cpu().numpy(), mask.cpu().numpy()
    t1 = time.perf_counter()
    q = np.clip(im.astype(np.int64) - int(im.min()), 0, 65535).astype(np.uint16)
    mk = np.where(m != 0, mk, -1)
    out = ndimage.watershed_ift(q, mk)
    out[out < 0] = 0
    t2 = time.perf_counter()
    back = torch.from_numpy(out.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    del back
    ms = dict(d2h=round((t1 - t0) * 1e3, 1), scipy_watershed_ift=round((t2 - t1) * 1e3, 1), h2d=round((t3 - t2) * 1e3, 1), total=round((t3 - t0) * 1e3, 1))
    print(f"{name}: host path {ms}", flush=True)
    return ms


def measure(size, mask_np, calls, rounds, with_host):
    name = f"balls {size}^3"
    mask = torch.from_numpy(mask_np).cuda()
    image, seeds = pipeline(mask)
    n = mask.numel()
    R = max(n, 2) - 1
    R = R.bit_length() + 1
    run = lambda: prepost.watershed(image, seeds, mask, 1, return_rounds=True)      # noqa: E731
    out, used = run()                                                               # the warm-up call
    res = dict(voxels=n, fill=round(float(mask_np.mean()), 4), seeds=int(seeds.max()), seeded_voxels=round(float((seeds > 0).float().mean()), 4),
               labelled=round(float((out > 0).float().mean()), 4), rounds_used=int(used), rounds_launched=R, launches=4 * R + 3,
               workspace_bytes=int(L.lib.bpx_watershed_workspace(size, size, size)), floor_ms=round(n * 13 / (STREAM_TBPS * 1e12) * 1e3, 4))
    assert int(used) <= R
    if with_host:
        res["host_ms"] = host_path(name, image, seeds, mask)
    del out
    one = timed(run, 1)
    k = max(2, min(calls, int(4000.0 / max(one, 1e-3))))                            # a reading takes about 4 s at most
    print(f"{name}: one call {one:.2f} ms, rounds {int(used)} of {R}; {k} calls per reading", flush=True)
    every = torch.ones_like(seeds)
    idle = lambda: prepost.watershed(image, every, mask, 1, return_rounds=True)     # noqa: E731
    assert int(idle()[1]) == 0
    vs, idles = [], []
    for r in range(rounds):
        vs.append(timed(run, k))
        idles.append(timed(idle, k))
        print(f"{name}: round {r + 1}: {vs[-1]:.3f} ms; no round working: {idles[-1]:.3f} ms", flush=True)
    med, imed = sorted(vs)[len(vs) // 2], sorted(idles)[len(idles) // 2]
    res.update(calls_per_reading=k, readings_ms=[round(v, 4) for v in vs], median_ms=round(med, 4), spread_ms=round(max(vs) - min(vs), 4),
               over_floor=round(med / res["floor_ms"], 1), no_round_working_ms=[round(v, 4) for v in idles], no_round_working_median_ms=round(imed, 4))
    if "host_ms" in res:
        res["host_over_device"] = round(res["host_ms"]["total"] / med, 1)
    del mask, image, seeds, every
    torch.cuda.empty_cache()
    return {name: res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "watershed_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "watershed_timing.py measures on the MI355X; there is nothing to measure without it"
    res = json.load(open(a.out))["inputs"] if os.path.exists(a.out) else {}
    b256 = balls(256)
    check_crop(b256)
    b512 = balls(512) if any(s > 256 for s in a.sizes) else None
    for s in a.sizes:
        mask_np = b256 if s == 256 else b512 if s == 512 else np.tile(b512, (2, 2, 2))
        res.update(measure(s, mask_np, a.calls, a.rounds, s == 256))
    faster = bool(all(v["median_ms"] < v["host_ms"]["total"] for v in res.values() if "host_ms" in v))
    out = dict(
        workload=f"prepost.watershed(-d2, seeds, mask, connectivity=1) resident on the device: int32 image, int32 seeds from the labelled core d2 > "
                 f"{CORE_D2}, uint8 mask; up to {a.calls} calls per reading, {a.rounds} readings; one box; host path timed once",
        device=torch.cuda.get_device_name(0), inputs=res, conditions={"device call faster than the host path on every input measured": faster},
        yardstick_tbps=STREAM_TBPS,
        note="floor = image + markers + mask read once and 4 bytes written per voxel (13 bytes); no_round_working = a whole call on an all-seeded "
             "input: the flag kernel, init, round 0's pick (every tree turns out seeded), 4 R - 1 launches that return at once and the last pass; the host path is scipy.ndimage.watershed_ift on a "
             "uint16 quantisation - another tie-breaking rule, not scikit-image's function; pass A has one form (no wave-level pre-reduction built)",
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))
    print("wrote", a.out)
    return 0 if faster else 1


if __name__ == "__main__":
    sys.exit(main())

"""What prepost.median_filter costs on the device, against the host path a user has without it and against the only torch route to a median
filter.  One box; per input and size 20 calls per reading, three readings, the calls alternated reading by reading (HIP events, after a
warm-up call of each).
Inputs at 256^3, 512^3 and 1024^3: a float32 probability map (a smooth random field in 0..1 with 5 % salt noise, tiled from 128^3 with a
different flip per tile) and the uint8 mask ``prob > 0.5``.  Sizes (1, 3, 3), (1, 5, 5), (3, 3, 3), (5, 1, 1), (1, 7, 7), (5, 5, 5), mode "reflect".
Before anything is timed the device result of every size and both dtypes is compared bit for bit with tests/median_ref.py on a 40^3 crop, in
all three modes; at 256^3 (and for the sizes timed on the host at 512^3) the host path's own result is compared with the device's as well.
Recorded per reading: median and spread; the ratio of the median to the traffic floor at the 4.5 TB/s yardstick of the project's streaming
passes - the input read once and the output written once: 8 B per voxel for float32, 2 B for uint8.
(host) the device-to-host copy, scipy.ndimage.median_filter, the copy back - wall clock, once: every size at 256^3, the three sizes with the
smallest windows ((5, 1, 1), (1, 3, 3), (1, 5, 5)) at 512^3.
Condition 1: the device call is faster than that host path on every input measured at 256^3, and at 512^3 for those three sizes.
Condition 2: at 256^3 with (1, 5, 5) and (3, 3, 3) on float32 the device call is faster, beyond the spread of the three readings, than the only
torch route - F.pad(mode="reflect"), three unfolds, .median(-1) - alternated with it reading by reading.  (torch's "reflect" does not repeat
the edge voxel, so that route is not SciPy's filter at the faces; its interior is compared with the device's before it is timed.)
The conditions are reported as HELD or NOT; exit status 1 when one does not hold.
Back-to-back calls on one volume: at 256^3 the float32 input and output (67 MB each) and the uint8 ones (17 MB each) stay in the 256 MB
last-level cache between calls, so those readings are not HBM figures; 512^3 float32 (537 MB and as much written) and 1024^3 do not fit.
Writes profiles/median_timing.json; --sizes runs a subset and merges into the file.  On a shared box one size per run, each under its own limit:
  timeout -k 10 900 python scripts/median_timing.py --sizes 256 && timeout -k 10 900 python scripts/median_timing.py --sizes 512 && \\
  timeout -k 10 600 python scripts/median_timing.py --sizes 1024
python scripts/median_timing.py [--calls 20] [--rounds 3] [--sizes 256 512 1024]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from biapy_amd import prepost as P  # noqa: E402
from regionprops_timing import STREAM_TBPS, timed  # noqa: E402

SIZES = ((1, 3, 3), (1, 5, 5), (3, 3, 3), (5, 1, 1), (1, 7, 7), (5, 5, 5))
HOST_AT_512 = ((5, 1, 1), (1, 3, 3), (1, 5, 5))
TORCH_ROUTE = ((1, 5, 5), (3, 3, 3))
FLOOR_BYTES = {"float32": 8, "uint8": 2}


def probability(s):
    """(s, s, s) float32 on the device: tests/median_ref.py's 128^3 map, tiled with a different flip per tile so that no two tiles are equal."""
    import median_ref as R

    base = torch.from_numpy(np.array(R.probability((128, 128, 128)))).cuda()
    if s == 128:
        return base
    k = s // 128
    out = torch.empty((s, s, s), dtype=torch.float32, device="cuda")
    for i in range(k):
        for j in range(k):
            for l in range(k):
                flips = [d for d, f in enumerate((i & 1, j & 1, l & 1)) if f]
                out[128 * i:128 * (i + 1), 128 * j:128 * (j + 1), 128 * l:128 * (l + 1)] = base.flip(flips) if flips else base
    return out


def check_crop(prob):
    import median_ref as R

    crop = np.ascontiguousarray(prob[:40, :40, :40].cpu().numpy())
    for x in (crop, (crop > 0.5).astype(np.uint8)):
        d = torch.from_numpy(x).cuda()
        for size in SIZES:
            for mode, cval in (("reflect", 0), ("nearest", 0), ("constant", 1)):
                got = P.median_filter(d, size, mode, cval).cpu().numpy()
                assert np.array_equal(R.bits(got), R.bits(R.median_ref(x, size, mode, cval))), f"the device differs from the twin on the 40^3 crop ({x.dtype}, {size}, {mode})"
    print(f"40^3 crop: {len(SIZES)} sizes x 3 modes x 2 dtypes equal the twin bit for bit", flush=True)


def host_path(name, x, size, got):
    """D2H + scipy.ndimage.median_filter + H2D, wall clock; its result against the device's."""
    from scipy import ndimage

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = x.cpu().numpy()
    t1 = time.perf_counter()
    r = ndimage.median_filter(h, size=size)
    t2 = time.perf_counter()
    back = torch.from_numpy(r).cuda()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    assert torch.equal(back, got), f"{name}: the host path's result differs from the device's"
    ms = dict(d2h=round((t1 - t0) * 1e3, 1), scipy=round((t2 - t1) * 1e3, 1), h2d=round((t3 - t2) * 1e3, 1), total=round((t3 - t0) * 1e3, 1))
    print(f"{name}: host path {ms}; the device result equals it", flush=True)
    return ms


def torch_route(x, size):
    """The only torch route: reflect padding (torch's, without the edge voxel), three unfolds, the median of the last axis."""
    sz, sy, sx = size
    p = torch.nn.functional.pad(x[None, None], (sx // 2, sx // 2, sy // 2, sy // 2, sz // 2, sz // 2), mode="reflect")[0, 0]
    w = p.unfold(0, sz, 1).unfold(1, sy, 1).unfold(2, sx, 1)
    return w.reshape(x.shape + (-1,)).median(-1).values


def stats(vs):
    return dict(readings_ms=[round(v, 4) for v in vs], median_ms=round(sorted(vs)[len(vs) // 2], 4), spread_ms=round(max(vs) - min(vs), 4))


def measure(s, prob, calls, rounds):
    inputs = {"float32": prob, "uint8": (prob > 0.5).to(torch.uint8)}
    n = prob.numel()
    res, runs = {}, {}
    for dt, x in inputs.items():
        for size in SIZES:
            name = f"{dt} {size}"
            got = P.median_filter(x, size)                                          # the warm-up call
            row = dict(voxels=n, window=int(np.prod(size)), floor_ms=round(n * FLOOR_BYTES[dt] / (STREAM_TBPS * 1e12) * 1e3, 4),
                       floor_bytes_per_voxel=FLOOR_BYTES[dt])
            if s == 256:
                row["resident_in_last_level_cache"] = True                          # not an HBM figure
            if s == 256 or (s == 512 and size in HOST_AT_512):
                row["host_ms"] = host_path(f"{name} {s}^3", x, size, got)
            res[name] = row
            runs[name] = (lambda x=x, size=size: P.median_filter(x, size))
            del got
    if s == 256:
        for size in TORCH_ROUTE:
            name = f"torch pad + unfold + median {size}"
            r = [h // 2 for h in size]
            inner = tuple(slice(h, 256 - h) for h in r)
            assert torch.equal(torch_route(prob, size)[inner], P.median_filter(prob, size)[inner]), f"{name}: its interior differs from the device's"
            runs[name] = (lambda size=size: torch_route(prob, size))
            res[name] = dict(voxels=n)
    readings = {name: [] for name in runs}
    for _ in range(rounds):                                                         # alternated: every call once per round
        for name, run in runs.items():
            readings[name].append(timed(run, calls if not name.startswith("torch") else max(calls // 4, 1)))
    for name, vs in readings.items():
        res[name].update(stats(vs))
        if "floor_ms" in res[name]:
            res[name]["over_floor"] = round(res[name]["median_ms"] / res[name]["floor_ms"], 1)
        if "host_ms" in res[name]:
            res[name]["host_over_device"] = round(res[name]["host_ms"]["total"] / res[name]["median_ms"], 1)
        print(f"{name} {s}^3: {res[name]['median_ms']:.3f} ms (spread {res[name]['spread_ms']:.3f})"
              + (f", floor {res[name]['floor_ms']:.3f} ms" if "floor_ms" in res[name] else ""), flush=True)
    return dict(calls=res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "median_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "median_timing.py measures on the MI355X; there is nothing to measure without it"
    res = json.load(open(a.out))["inputs"] if os.path.exists(a.out) else {}
    check_crop(probability(128))
    for s in a.sizes:
        prob = probability(s)
        res[f"probability {s}^3"] = measure(s, prob, a.calls, a.rounds)
        del prob
        torch.cuda.empty_cache()
    hosted = [v for r in res.values() for v in r["calls"].values() if "host_ms" in v]
    at256, at512 = res.get("probability 256^3", {}).get("calls", {}), res.get("probability 512^3", {}).get("calls", {})
    cond1 = None
    if at256 and at512:
        cond1 = all(v["median_ms"] < v["host_ms"]["total"] for v in hosted) and all("host_ms" in at256[f"{dt} {size}"] for dt in FLOOR_BYTES for size in SIZES) \
            and all("host_ms" in at512[f"{dt} {size}"] for dt in FLOOR_BYTES for size in HOST_AT_512)
    cond2 = None
    if at256:
        cond2 = True
        for size in TORCH_ROUTE:
            d, t = at256[f"float32 {size}"], at256[f"torch pad + unfold + median {size}"]
            cond2 = cond2 and bool(d["median_ms"] + max(d["spread_ms"], t["spread_ms"]) < t["median_ms"])
    word = {True: "HELD", False: "NOT", None: "not measured"}
    out = dict(
        workload=f"biapy_amd.prepost.median_filter on volumes resident on the device, mode reflect; {a.calls} calls per reading, {a.rounds} readings per "
                 f"call, the calls alternated; one box; host path timed once",
        device=torch.cuda.get_device_name(0), inputs=res,
        conditions={"1: the device call faster than the host path (D2H + scipy.ndimage.median_filter + H2D) on every input at 256^3 and for (5,1,1), "
                    "(1,3,3), (1,5,5) at 512^3": word[cond1],
                    "2: faster than F.pad(reflect) + three unfolds + median(-1) at 256^3 with (1,5,5) and (3,3,3) on float32, beyond the spread": word[cond2]},
        yardstick_tbps=STREAM_TBPS,
        note="floor = the input read once + the output written once at the yardstick (8 B per voxel float32, 2 B uint8); over_floor = median / "
             "floor; the readings include the allocation of the result; at 256^3 input and output stay in the 256 MB last-level cache between the "
             "back-to-back calls (resident_in_last_level_cache): those readings are not HBM figures; the torch route is read with a quarter of the calls",
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out["conditions"], indent=1))
    print("wrote", a.out)
    return 0 if cond1 is not False and cond2 is not False else 1


if __name__ == "__main__":
    sys.exit(main())

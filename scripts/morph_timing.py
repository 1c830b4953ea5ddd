"""What the morphology calls cost on the device, against the host path a user has without them and against the only torch route to a dilation.
One box; per call 20 calls per reading, three readings, the calls alternated reading by reading (HIP events, after a warm-up call of each).
Inputs at 256^3, 512^3 and 1024^3 (the 512^3 mask tiled 2 x 2 x 2): random balls (radius 3..9, about 30 % fill) as a uint8 mask, and
prepost.label of them (connectivity 1) as int32 labels.
Timed: binary_erosion and binary_dilation at connectivity 1 and 3, binary_erosion(iterations=3), dilation of the labels, find_boundaries of the
labels, binary_fill_holes (num given as an int: nothing is read back).
Before anything is timed the device result of every call is compared bit for bit with tests/morph_ref.py on a 40^3 crop; at 256^3 and 512^3 the
host path's own results are compared with the device's as well.
Recorded per call: the readings, median and spread; the ratio of the median to the traffic floor at the 4.5 TB/s yardstick of the project's
streaming passes - input bytes read once plus output bytes written once (2 B per voxel on the binary path, per iteration; 8 B for the int32
dilation; 5 B for the boundary map; binary_fill_holes is held against its 2 B although it is label + select_objects + torch glue).
(host) at 256^3 and 512^3: the device-to-host copy, the SciPy function (find_boundaries: grey_dilation != grey_erosion), the copy back - wall
clock, once.
Condition 1: every device call is faster than that host path at 256^3 and 512^3.
Condition 2: binary_dilation at connectivity 3 is faster, beyond the spread of the three readings, than the only torch route at 512^3 - a float
copy, F.max_pool3d(kernel 3, stride 1, padding 1), a compare - alternated with it reading by reading.  Exit status 1 when one does not hold.
Back-to-back calls on one volume: at 256^3 the mask (17 MB) and the labels (67 MB) with their results stay in the 256 MB last-level cache
between calls, so those readings are not HBM figures; 512^3 (134 / 537 MB, and as much written) and 1024^3 do not fit.
Writes profiles/morph_timing.json; --sizes runs a subset and merges into the file.
python scripts/morph_timing.py [--calls 20] [--rounds 3] [--sizes 256 512 1024]"""
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
from regionprops_timing import STREAM_TBPS, balls, timed  # noqa: E402

def calls_of(n_bg):
    """{name: (input "mask" | "labels", the device call, bytes per voxel of the traffic floor, the statement, the host function)}; ``n_bg``: the
    number of background components, binary_fill_holes' ``num``."""
    import morph_ref as R
    from scipy import ndimage

    s1, s3 = ndimage.generate_binary_structure(3, 1), ndimage.generate_binary_structure(3, 3)
    return {
        "binary_erosion c1": ("mask", lambda m: P.binary_erosion(m, 1), 2, lambda h: R.binary_erosion_ref(h, 1), lambda h: ndimage.binary_erosion(h, s1)),
        "binary_erosion c3": ("mask", lambda m: P.binary_erosion(m, 3), 2, lambda h: R.binary_erosion_ref(h, 3), lambda h: ndimage.binary_erosion(h, s3)),
        "binary_dilation c1": ("mask", lambda m: P.binary_dilation(m, 1), 2, lambda h: R.binary_dilation_ref(h, 1), lambda h: ndimage.binary_dilation(h, s1)),
        "binary_dilation c3": ("mask", lambda m: P.binary_dilation(m, 3), 2, lambda h: R.binary_dilation_ref(h, 3), lambda h: ndimage.binary_dilation(h, s3)),
        "binary_erosion c1 iterations=3": ("mask", lambda m: P.binary_erosion(m, 1, 3), 6, lambda h: R.binary_erosion_ref(h, 1, 3),
                                           lambda h: ndimage.binary_erosion(h, s1, 3)),
        "dilation int32 c1": ("labels", lambda l: P.dilation(l, 1), 8, lambda h: R.dilation_ref(h, 1), lambda h: ndimage.grey_dilation(h, footprint=s1)),
        "find_boundaries c1": ("labels", lambda l: P.find_boundaries(l, 1), 5, lambda h: R.find_boundaries_ref(h, 1),
                               lambda h: ndimage.grey_dilation(h, footprint=s1) != ndimage.grey_erosion(h, footprint=s1)),
        "binary_fill_holes": ("mask", lambda m: P.binary_fill_holes(m, n_bg), 2, lambda h: R.fill_holes_ref(h), lambda h: ndimage.binary_fill_holes(h)),
    }


def check_crop(mask_np):
    crop = torch.from_numpy(np.ascontiguousarray(mask_np[:40, :40, :40])).cuda()
    inputs = {"mask": crop, "labels": P.label(crop, connectivity=1)}
    n_bg = int(P.label(crop == 0, connectivity=1, return_num=True)[1])
    for name, (which, run, _, ref, _) in calls_of(n_bg).items():
        want = ref(inputs[which].cpu().numpy())
        assert np.array_equal(run(inputs[which]).cpu().numpy(), want), f"the device result differs from the statement on the 40^3 crop ({name})"
    print(f"40^3 crop: all {len(calls_of(0))} calls equal the statement bit for bit", flush=True)


def host_path(name, x, host_fn, got):
    """D2H + the SciPy function + H2D, wall clock; its result against the device's."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = x.cpu().numpy()
    t1 = time.perf_counter()
    r = host_fn(h)
    t2 = time.perf_counter()
    back = torch.from_numpy(np.ascontiguousarray(r)).cuda()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    assert torch.equal(back.to(got.dtype), got), f"{name}: the host path's result differs from the device's"
    ms = dict(d2h=round((t1 - t0) * 1e3, 1), scipy=round((t2 - t1) * 1e3, 1), h2d=round((t3 - t2) * 1e3, 1), total=round((t3 - t0) * 1e3, 1))
    print(f"{name}: host path {ms}; the device result equals it", flush=True)
    return ms


def torch_route(m):
    """The only torch route to a dilation, and only for the full box: float copy, max pooling, compare."""
    return (torch.nn.functional.max_pool3d(m[None, None].float(), 3, 1, 1)[0, 0] > 0).to(torch.uint8)


def stats(vs):
    return dict(readings_ms=[round(v, 4) for v in vs], median_ms=round(sorted(vs)[len(vs) // 2], 4), spread_ms=round(max(vs) - min(vs), 4))


def measure(s, mask, calls, rounds, with_host, with_torch):
    labels, n_bg = P.label(mask, connectivity=1), int(P.label(mask == 0, connectivity=1, return_num=True)[1])
    inputs = {"mask": mask, "labels": labels}
    table = calls_of(n_bg)
    n = mask.numel()
    res, runs = {}, {}
    for name, (which, run, bpv, _, host_fn) in table.items():
        x = inputs[which]
        got = run(x)                                                                # the warm-up call
        row = dict(voxels=n, floor_ms=round(n * bpv / (STREAM_TBPS * 1e12) * 1e3, 4), floor_bytes_per_voxel=bpv)
        if s == 256:
            row["resident_in_last_level_cache"] = True                              # not an HBM figure
        if with_host:
            row["host_ms"] = host_path(f"{name} {s}^3", x, host_fn, got)
        res[name] = row
        runs[name] = (lambda run=run, x=x: run(x))
        del got
    if with_torch:
        assert torch.equal(torch_route(mask), P.binary_dilation(mask, 3)), "the torch route differs from binary_dilation at connectivity 3"
        runs["torch max_pool3d route"] = lambda: torch_route(mask)
        res["torch max_pool3d route"] = dict(voxels=n)
    readings = {name: [] for name in runs}
    for _ in range(rounds):                                                         # alternated: every call once per round
        for name, run in runs.items():
            readings[name].append(timed(run, calls))
    for name, vs in readings.items():
        res[name].update(stats(vs))
        if "floor_ms" in res[name]:
            res[name]["over_floor"] = round(res[name]["median_ms"] / res[name]["floor_ms"], 1)
        if "host_ms" in res[name]:
            res[name]["host_over_device"] = round(res[name]["host_ms"]["total"] / res[name]["median_ms"], 1)
        print(f"{name} {s}^3: {res[name]['median_ms']:.3f} ms (spread {res[name]['spread_ms']:.3f})"
              + (f", floor {res[name]['floor_ms']:.3f} ms" if "floor_ms" in res[name] else ""), flush=True)
    return dict(background_components=n_bg, labels=int(labels.max()), calls=res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morph_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "morph_timing.py measures on the MI355X; there is nothing to measure without it"
    res = json.load(open(a.out))["inputs"] if os.path.exists(a.out) else {}
    b256 = balls(256)
    check_crop(b256)
    for s in a.sizes:
        mask = torch.from_numpy(b256 if s == 256 else balls(512)).cuda()
        if s > 512:
            mask = mask.repeat(2, 2, 2)
        res[f"balls {s}^3"] = measure(s, mask, a.calls, a.rounds, s <= 512, s == 512)
        del mask
        torch.cuda.empty_cache()
    hosted = [(k, n, v) for k, r in res.items() for n, v in r["calls"].items() if "host_ms" in v]
    cond1 = bool(hosted) and all(v["median_ms"] < v["host_ms"]["total"] for _, _, v in hosted)
    cond2, at512 = None, res.get("balls 512^3", {}).get("calls", {})
    if "torch max_pool3d route" in at512:
        d, t = at512["binary_dilation c3"], at512["torch max_pool3d route"]
        cond2 = bool(d["median_ms"] + max(d["spread_ms"], t["spread_ms"]) < t["median_ms"])
    out = dict(
        workload=f"biapy_amd.prepost morphology calls on volumes resident on the device; {a.calls} calls per reading, {a.rounds} readings per call, "
                 f"the calls alternated; one box; host path timed once",
        device=torch.cuda.get_device_name(0), inputs=res,
        conditions={"1: every device call faster than the host path (D2H + SciPy + H2D) at 256^3 and 512^3": cond1,
                    "2: binary_dilation c3 faster than float copy + F.max_pool3d + compare at 512^3, beyond the spread": cond2},
        yardstick_tbps=STREAM_TBPS,
        note="floor = input bytes read once + output bytes written once at the yardstick; over_floor = median / floor; the readings include the "
             "allocation of the result (and of the scratch volume with iterations > 1); binary_fill_holes is label(mask == 0) + the labels of the "
             "faces + select_objects + an OR, held against the 2 B per voxel of its input and output; at 256^3 input and output stay in the 256 MB "
             "last-level cache between the back-to-back calls (resident_in_last_level_cache): those readings are not HBM figures",
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out["conditions"], indent=1))
    print("wrote", a.out)
    return 0 if cond1 and cond2 is not False else 1


if __name__ == "__main__":
    sys.exit(main())

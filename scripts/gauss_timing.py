"""What prepost.gaussian_filter costs on the device, against the host path a user has without it and against the only torch route to a
separable filter.  One box; per input and sigma 20 calls per reading, three readings, the calls alternated reading by reading (HIP events,
after a warm-up call of each).
Inputs at 256^3, 512^3 and 1024^3: a float32 probability map (tests/median_ref.py's smooth random field with salt noise, tiled from 128^3 with
a different flip per tile).  Sigma 1, 2 and 8 isotropic (radii 4, 8 and 32: three passes) and (0, 2, 2) (two passes), mode "reflect".
Before anything is timed the device result of every sigma is compared bit for bit with tests/gauss_ref.py on a 40^3 crop, in all four modes
and for orders 0 to 2; where the host path is timed its own result is compared with the device's within the bound of tests/gauss_ref.py
on a 64^3 corner.
Recorded per reading: median and spread; the ratio of the median to the traffic floor at the 4.5 TB/s yardstick of the project's streaming
passes - per active pass the input read once and the output written once: 8 B per voxel and pass.  For the isotropic sigmas each pass is also
timed alone (sigma on one axis), which says which of the three takes the time.
(host) the device-to-host copy, scipy.ndimage.gaussian_filter, the copy back - wall clock, once: every sigma at 256^3 and 512^3; 1024^3 is
device-only.
Condition 1: the device call is faster than that host path on every input measured.
Condition 2: at 256^3 the device call is faster, beyond the spread of the three readings, than the only torch route - F.pad(mode="reflect",
which is SciPy's "mirror") and three F.conv3d calls with (k,1,1), (1,k,1), (1,1,k) kernels - alternated with the device call in mode "mirror"
reading by reading; the two results are compared before they are timed.
The conditions are reported as HELD or NOT; exit status 1 when one does not hold.
Back-to-back calls on one volume: at 256^3 input, workspace and output (67 MB each) stay in the 256 MB last-level cache between calls, so
those readings are not HBM figures; 512^3 (537 MB each) and 1024^3 do not fit.
Writes profiles/gauss_timing.json; --sizes runs a subset and merges into the file.
python scripts/gauss_timing.py [--calls 20] [--rounds 3] [--sizes 256 512 1024]"""
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
from median_timing import probability, stats  # noqa: E402
from regionprops_timing import STREAM_TBPS, timed  # noqa: E402

SIGMAS = (1.0, 2.0, 8.0, (0.0, 2.0, 2.0))
FLOOR_BYTES_PER_PASS = 8
AXES = "zyx"


def per_axis(sigma):
    return tuple(sigma) if isinstance(sigma, tuple) else (sigma,) * 3


def check_crop(prob):
    import gauss_ref as R

    crop = np.ascontiguousarray(prob[:40, :40, :40].cpu().numpy())
    d = torch.from_numpy(crop).cuda()
    n = 0
    for sigma in SIGMAS:
        for mode, cval in R.MODES:
            for order in (0, 1, 2):
                got = P.gaussian_filter(d, sigma, order, mode, cval).cpu().numpy()
                R.same_bits(got, R.gaussian_ref(crop, sigma, order, mode, cval), f"the device differs from the twin on the 40^3 crop ({sigma}, {order}, {mode})")
                n += 1
    print(f"40^3 crop: {n} calls equal the twin bit for bit", flush=True)


def host_path(name, x, sigma, got):
    """D2H + scipy.ndimage.gaussian_filter + H2D, wall clock; its result against the device's on a 64^3 corner, within the bound."""
    import gauss_ref as R
    from scipy import ndimage

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = x.cpu().numpy()
    t1 = time.perf_counter()
    r = ndimage.gaussian_filter(h, sigma)
    t2 = time.perf_counter()
    back = torch.from_numpy(r).cuda()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    c = 64 + 40                                                                               # the corner's far faces see 40 voxels beyond them: more than r = 32
    ref, bound = R.reference_and_bound(h[:c, :c, :c], R.gaussian_axes(3, sigma))
    err = np.abs(got[:64, :64, :64].cpu().numpy().astype(np.float64) - ref[:64, :64, :64])
    assert (err <= bound[:64, :64, :64]).all(), f"{name}: the device result leaves the bound of the float64 reference"
    assert np.abs(r[:64, :64, :64] - ref[:64, :64, :64]).max() < 1e-5, f"{name}: the host path's result is not the reference's"
    ms = dict(d2h=round((t1 - t0) * 1e3, 1), scipy=round((t2 - t1) * 1e3, 1), h2d=round((t3 - t2) * 1e3, 1), total=round((t3 - t0) * 1e3, 1))
    print(f"{name}: host path {ms}; the device result lies within the bound of its float64 form", flush=True)
    return ms


def torch_route(x, sigma):
    """The only torch route: reflect padding (torch's: SciPy's "mirror"), then one conv3d per axis with a (k,1,1), (1,k,1), (1,1,k) kernel."""
    import gauss_ref as R

    F = torch.nn.functional
    ws = [None if w is None else torch.from_numpy(w.astype(np.float32)).cuda() for w in R.gaussian_axes(3, sigma)]
    r = [0 if w is None else (w.numel() - 1) // 2 for w in ws]
    v = F.pad(x[None, None], (r[2], r[2], r[1], r[1], r[0], r[0]), mode="reflect")
    for axis, w in enumerate(ws):
        if w is not None:
            shape = [1, 1, 1, 1, 1]
            shape[2 + axis] = w.numel()
            v = F.conv3d(v, w.view(shape))
    return v[0, 0]


def measure(s, prob, calls, rounds):
    n = prob.numel()
    res, runs = {}, {}
    for sigma in SIGMAS:
        name = f"sigma {sigma}"
        got = P.gaussian_filter(prob, sigma)                                        # the warm-up call
        passes = sum(sd > 0 for sd in per_axis(sigma))
        row = dict(voxels=n, passes=passes, radii=[int(4.0 * sd + 0.5) for sd in per_axis(sigma)],
                   floor_ms=round(n * FLOOR_BYTES_PER_PASS * passes / (STREAM_TBPS * 1e12) * 1e3, 4), floor_bytes_per_voxel_and_pass=FLOOR_BYTES_PER_PASS)
        if s == 256:
            row["resident_in_last_level_cache"] = True                              # not an HBM figure
        if s <= 512:
            row["host_ms"] = host_path(f"{name} {s}^3", prob, sigma, got)
        res[name] = row
        runs[name] = (lambda sigma=sigma: P.gaussian_filter(prob, sigma))
        del got
        if not isinstance(sigma, tuple):                                            # each pass alone
            for axis in range(3):
                one = tuple(sigma if a == axis else 0.0 for a in range(3))
                pname = f"sigma {sigma} {AXES[axis]} pass alone"
                P.gaussian_filter(prob, one)
                res[pname] = dict(voxels=n, passes=1, floor_ms=round(n * FLOOR_BYTES_PER_PASS / (STREAM_TBPS * 1e12) * 1e3, 4))
                runs[pname] = (lambda one=one: P.gaussian_filter(prob, one))
    if s == 256:
        for sigma in SIGMAS:
            name = f"torch pad + 3 conv3d sigma {sigma}"
            a, b = torch_route(prob, sigma), P.gaussian_filter(prob, sigma, mode="mirror")
            assert float((a - b).abs().max()) < 1e-5, f"{name}: its result differs from the device's"
            runs[name] = (lambda sigma=sigma: torch_route(prob, sigma))
            res[name] = dict(voxels=n)
            runs[f"sigma {sigma} mirror"] = (lambda sigma=sigma: P.gaussian_filter(prob, sigma, mode="mirror"))
            res[f"sigma {sigma} mirror"] = dict(voxels=n)
            del a, b
    readings = {name: [] for name in runs}
    for _ in range(rounds):                                                         # alternated: every call once per round
        for name, run in runs.items():
            readings[name].append(timed(run, calls if not name.startswith("torch") else max(calls // 4, 1)))
    for name, vs in readings.items():
        res[name].update(stats(vs))
        if "floor_ms" in res[name]:
            res[name]["over_floor"] = round(res[name]["median_ms"] / res[name]["floor_ms"], 2)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gauss_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gauss_timing.py measures on the MI355X; there is nothing to measure without it"
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
        cond1 = all(v["median_ms"] < v["host_ms"]["total"] for v in hosted) and all("host_ms" in at[f"sigma {sg}"] for at in (at256, at512) for sg in SIGMAS)
    cond2 = None
    if at256:
        cond2 = True
        for sg in SIGMAS:
            d, t = at256[f"sigma {sg} mirror"], at256[f"torch pad + 3 conv3d sigma {sg}"]
            cond2 = cond2 and bool(d["median_ms"] + max(d["spread_ms"], t["spread_ms"]) < t["median_ms"])
    word = {True: "HELD", False: "NOT", None: "not measured"}
    out = dict(
        workload=f"biapy_amd.prepost.gaussian_filter on float32 volumes resident on the device, mode reflect, truncate 4; {a.calls} calls per reading, "
                 f"{a.rounds} readings per call, the calls alternated; one box; host path timed once",
        device=torch.cuda.get_device_name(0), inputs=res,
        conditions={"1: the device call faster than the host path (D2H + scipy.ndimage.gaussian_filter + H2D) on every input at 256^3 and 512^3": word[cond1],
                    "2: faster than F.pad(reflect) + three F.conv3d at 256^3 for every sigma, mode mirror, beyond the spread": word[cond2]},
        yardstick_tbps=STREAM_TBPS,
        note="floor = per active pass the input read once + the output written once at the yardstick (8 B per voxel and pass); over_floor = median "
             "/ floor; the readings include the allocation of the result and the workspace; 'pass alone' rows filter one axis only; at 256^3 input, "
             "workspace and output stay in the 256 MB last-level cache between the back-to-back calls (resident_in_last_level_cache): those "
             "readings are not HBM figures; the torch route is read with a quarter of the calls",
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out["conditions"], indent=1))
    print("wrote", a.out)
    return 0 if cond1 is not False and cond2 is not False else 1


if __name__ == "__main__":
    sys.exit(main())

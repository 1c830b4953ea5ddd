"""What the local-maximum calls cost on the device, beside the 3 x 3 x 3 grey dilation that has the footprint of r = 1.
One box; per call 20 calls per reading, three readings, the calls alternated reading by reading (HIP events, after a warm-up call of each).
Input: a 256^3 float32 volume, a seeded random field box-averaged over 5^3 on the device (smooth, so that peaks are as sparse as in a
probability or distance map), threshold 0.5, no border margin.
Timed: prepost.peak_mask and prepost.peak_local_max (the default max_peaks = 2^20; with the values) at r = 1, 2, 4, 8 and (1, 4, 4), and
prepost.dilation(x, 3) on the same volume: value-only, no tie rule, one pass.
Before anything is timed the device result of every call is compared bit for bit with tests/peaks_ref.py on a 40^3 crop.
Recorded per call: the readings, median and spread; the bytes per voxel the design moves - the first pass reads the 4-byte image, every pass
but the last writes 8-byte keys that the next one reads, the last pass reads the image again and peak_mask writes 1 byte: 8 + 16 (p - 1) (+ 1)
for p passes - and the GB/s that makes of the median; for peak_local_max the sort and the decoding of 2^20 keys are in the readings and not in
the bytes.  The radii are there so that the growth with r can be read off: the one condition is that the time grows no faster than linearly
in r (r = 8 within 8 / 1 of r = 1, 4 / 1 of r = 2, 2 / 1 of r = 4; exit status 1 otherwise).
Back-to-back calls on one volume: the 67 MB image stays in the 256 MB last-level cache between calls and the 134 MB key volumes in part, so
these readings are not HBM figures.
Writes profiles/peaks_timing.json.
python scripts/peaks_timing.py [--calls 20] [--rounds 3] [--size 256]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from biapy_amd import prepost as P  # noqa: E402
from regionprops_timing import timed  # noqa: E402

RADII = (1, 2, 4, 8, (1, 4, 4))
THRESHOLD = 0.5


def field(n, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand((1, 1, n, n, n), device="cuda", generator=g)
    x = torch.nn.functional.avg_pool3d(x, 5, 1, 2, count_include_pad=False)[0, 0]
    return ((x - 0.5) * 4 + 0.5).contiguous()                          # about a third of the voxels above the threshold


def passes(r):
    return max(1, sum(1 for v in (r if isinstance(r, tuple) else (r,) * 3) if v > 0))


def check_crop(x):
    import peaks_ref as R
    from scipy import ndimage

    crop = x[:40, :40, :40].contiguous()
    h = crop.cpu().numpy()
    for r in RADII:
        assert np.array_equal(P.peak_mask(crop, r, THRESHOLD, False).cpu().numpy(), R.peak_mask_ref(h, r, THRESHOLD, False)), f"peak_mask r={r}"
        coords, values, num = P.peak_local_max(crop, r, THRESHOLD, False, return_values=True)
        wc, wv = R.peak_list_ref(h, r, THRESHOLD, False)
        K = int(num)
        assert K == len(wc) and np.array_equal(coords[:K].cpu().numpy(), wc) and np.array_equal(values[:K].cpu().numpy(), wv), f"peak_local_max r={r}"
    assert np.array_equal(P.dilation(crop, 3).cpu().numpy(), ndimage.grey_dilation(h, size=3)), "dilation"
    print(f"40^3 crop: peak_mask and peak_local_max equal the twin bit for bit at {len(RADII)} radii", flush=True)


def stats(vs):
    return dict(readings_ms=[round(v, 4) for v in vs], median_ms=round(sorted(vs)[len(vs) // 2], 4), spread_ms=round(max(vs) - min(vs), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peaks_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "peaks_timing.py measures on the MI355X; there is nothing to measure without it"
    x = field(a.size)
    check_crop(x)
    n = x.numel()
    runs, res = {}, {}
    for r in RADII:
        p = passes(r)
        runs[f"peak_mask r={r}"] = lambda r=r: P.peak_mask(x, r, THRESHOLD, False)
        res[f"peak_mask r={r}"] = dict(voxels=n, passes=p, bytes_per_voxel=8 + 16 * (p - 1) + 1)
        runs[f"peak_local_max r={r}"] = lambda r=r: P.peak_local_max(x, r, THRESHOLD, False, return_values=True)
        res[f"peak_local_max r={r}"] = dict(voxels=n, passes=p, bytes_per_voxel=8 + 16 * (p - 1),
                                            peaks=int(P.peak_local_max(x, r, THRESHOLD, False)[1]))
    runs["dilation float32 c3"] = lambda: P.dilation(x, 3)
    res["dilation float32 c3"] = dict(voxels=n, passes=1, bytes_per_voxel=8)
    for run in runs.values():                                          # the warm-up calls
        run()
    readings = {name: [] for name in runs}
    for _ in range(a.rounds):                                          # alternated: every call once per round
        for name, run in runs.items():
            readings[name].append(timed(run, a.calls))
    for name, vs in readings.items():
        res[name].update(stats(vs))
        res[name]["gb_per_s"] = round(n * res[name]["bytes_per_voxel"] / (res[name]["median_ms"] * 1e-3) / 1e9, 1)
        print(f"{name}: {res[name]['median_ms']:.3f} ms (spread {res[name]['spread_ms']:.3f}), {res[name]['bytes_per_voxel']} B per voxel, "
              f"{res[name]['gb_per_s']} GB/s", flush=True)
    dil = res["dilation float32 c3"]["median_ms"]
    ms = {r: res[f"peak_mask r={r}"]["median_ms"] for r in (1, 2, 4, 8)}
    linear = bool(ms[8] <= 8 * ms[1] and ms[8] <= 4 * ms[2] and ms[8] <= 2 * ms[4] and ms[4] <= 4 * ms[1] and ms[2] <= 2 * ms[1])
    out = dict(
        workload=f"biapy_amd.prepost.peak_mask / peak_local_max on a {a.size}^3 float32 volume resident on the device; {a.calls} calls per reading, "
                 f"{a.rounds} readings per call, the calls alternated; one box",
        device=torch.cuda.get_device_name(0), calls=res,
        peak_mask_r1_over_dilation=dict(expected_from_bytes=round(41 / 8, 1), measured=round(ms[1] / dil, 1)),
        conditions={"time grows no faster than linearly in r (peak_mask at r = 1, 2, 4, 8)": linear},
        note="bytes_per_voxel = what the design moves through memory (image read by the first and the last pass, 8-byte keys written and read "
             "between passes, the 1-byte mask); gb_per_s = that over the median; the readings include the allocation of the workspace and the "
             "results, and for peak_local_max the sort and the decoding of the 2^20-slot key array; the image and part of the key volumes stay in "
             "the 256 MB last-level cache between the back-to-back calls: these readings are not HBM figures",
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out["conditions"], indent=1))
    print("wrote", a.out)
    return 0 if linear else 1


if __name__ == "__main__":
    sys.exit(main())

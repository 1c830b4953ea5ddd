"""What the nearest-background index costs beside the distance transform, and what expand_labels costs against the host path a user has without
it.  One box, one call, the modes alternated, 20 calls per reading, three readings each (HIP events, after a warm-up call):
  (a) distance  prepost.distance_transform_edt of the uint8 mask, float32 distances (csrc/edt.hip, unchanged: the yardstick);
  (b) indices   the same call with return_indices="linear": distances and the int32 linear index of the nearest zero (csrc/edt_index.hip);
  (c) expand    prepost.expand_labels(labels, 2) of the int32 labels prepost.label made of the same mask: the transform on the labels
                (int32 squared distances, indices) and the gather;
  (host)        expand_labels through the host: device-to-host copy of the labels, scipy.ndimage.distance_transform_edt(labels == 0,
                return_indices=True), the gather and the threshold, host-to-device copy - timed once per input with the wall clock.
Masks: the random balls of scripts/edt_timing.py.  256^3 and 512^3 are measured against the host path and the device result is compared with
it (the same voxels grow; a label that differs from the host's must be that of a labelled voxel at exactly the host's distance); 1024^3
(the 512^3 mask tiled 2 x 2 x 2) is timed on the device only.
The ratio (b) / (a) is recorded, not capped.  What the index adds to the traffic per voxel, counted as edt_timing.py counts its passes (k = key
bytes; 28 + 4 k there): the index travels in the envelope's stack entries, so there is no second index volume and no gather -
  row pass   + 4 written (the index of the nearer source of the row)
  Y pass     + 4 read, + 4 written per foreground voxel, and the stack entries grow from 8 to 12 bytes
  Z pass     the same
so 40 + 4 k bytes per voxel against 28 + 4 k: 44 / 32 = 1.375 for a uint8 mask if both calls ran at the rate of their traffic.  The column
passes of (b) also run 6 waves per CU where (a) runs 8 (24 KiB of LDS per wave for the 12-byte entries, against 16).  Back-to-back calls at
256^3 work on 84 MB of mask and distances plus 67 MB of indices, inside the 256 MiB last-level cache: not an HBM figure.
There is one form of the kernels, so the only condition is: the device call (c) is faster than the host path on every input measured.  Exit
status 1 otherwise.  Writes profiles/edt_index_timing.json.
python scripts/edt_index_timing.py [--calls 20] [--rounds 3] [--no-1024]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy import ndimage  # noqa: E402

from biapy_amd import prepost  # noqa: E402
from edt_timing import balls, timed  # noqa: E402

DISTANCE = 2


def host_expand(lab):
    """skimage.segmentation.expand_labels as scikit-image writes it, and the host's distances."""
    dist, ind = ndimage.distance_transform_edt(lab == 0, return_indices=True)
    out = np.where(dist <= DISTANCE, lab[tuple(ind)], 0).astype(np.int32)
    return out, dist


def host_path(name, lab_dev):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = lab_dev.cpu().numpy()
    t1 = time.perf_counter()
    want, dist = host_expand(host)
    t2 = time.perf_counter()
    back = torch.from_numpy(want).cuda()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    ms = dict(d2h=round((t1 - t0) * 1e3, 1), scipy_and_gather=round((t2 - t1) * 1e3, 1), h2d=round((t3 - t2) * 1e3, 1), total=round((t3 - t0) * 1e3, 1))
    print(f"{name}: host path {ms}", flush=True)
    return ms, back, host, dist


def compare(name, got, want, lab_dev, lab, dist):
    """The device's labels against the host's: the same voxels grow; where the label differs, two labels are equally near (SciPy breaks such ties
    another way) - the device's nearest labelled voxel carries the device's label and lies at exactly the host's distance."""
    got = got.cpu().numpy().reshape(-1)
    assert np.array_equal(got != 0, want.reshape(-1) != 0), f"{name}: the device grows other voxels than the host"
    at = np.flatnonzero(got != want.reshape(-1))
    near = prepost.distance_transform_edt(lab_dev == 0, return_distances=False, return_indices="linear").cpu().numpy().reshape(-1)[at]
    delta = np.stack(np.unravel_index(near, lab.shape)).astype(np.int64) - np.stack(np.unravel_index(at, lab.shape))
    assert np.array_equal(lab.reshape(-1)[near], got[at]) and np.array_equal((delta ** 2).sum(axis=0), np.rint(dist.reshape(-1)[at] ** 2).astype(np.int64)), \
        f"{name}: a label that differs from the host's is not a nearest one"
    print(f"{name}: equals the host's expand_labels; {at.size} voxels carry another of two equally near labels", flush=True)
    return int(at.size)


def measure(size, mask_np, calls, rounds, host):
    m = torch.from_numpy(mask_np).cuda()
    lab = prepost.label(m)
    n = m.numel()
    runs = {"distance": lambda: prepost.distance_transform_edt(m), "indices": lambda: prepost.distance_transform_edt(m, return_indices="linear"),
            "expand": lambda: prepost.expand_labels(lab, DISTANCE)}
    res = dict(voxels=n, fill=round(float(mask_np.mean()), 4), labels=int(lab.max()))
    name = f"balls {size}^3"
    for mode, run in runs.items():
        got = run()                                                    # the warm-up call
        if mode == "expand" and host:
            res["host_ms"], want, lab_np, dist = host_path(name, lab)
            res["tie_voxels"] = compare(name, got, want.cpu().numpy(), lab, lab_np, dist)
            del want, lab_np, dist
        print(f"{name} {mode}: one call {timed(run, 1):.2f} ms", flush=True)
        del got
    readings = {mode: [] for mode in runs}
    for r in range(rounds):
        for mode, run in runs.items():
            readings[mode].append(timed(run, calls))
            print(f"{name} {mode}: round {r + 1}: {readings[mode][-1]:.3f} ms", flush=True)
    for mode, vs in readings.items():
        med = sorted(vs)[len(vs) // 2]
        res[mode] = dict(readings_ms=[round(v, 4) for v in vs], median_ms=round(med, 4), spread_ms=round(max(vs) - min(vs), 4))
    res["indices_over_distance"] = round(res["indices"]["median_ms"] / res["distance"]["median_ms"], 3)
    if host:
        res["host_over_expand"] = round(res["host_ms"]["total"] / res["expand"]["median_ms"], 1)
    del m, lab
    torch.cuda.empty_cache()
    return {name: res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-1024", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edt_index_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "edt_index_timing.py measures on the MI355X; there is nothing to measure without it"
    res = {}
    res.update(measure(256, balls(256), a.calls, a.rounds, True))
    b512 = balls(512)
    res.update(measure(512, b512, a.calls, a.rounds, True))
    if not a.no_1024:
        res.update(measure(1024, np.tile(b512, (2, 2, 2)), a.calls, a.rounds, False))
    faster = bool(all(v["expand"]["median_ms"] < v["host_ms"]["total"] for v in res.values() if "host_ms" in v))
    out = dict(
        workload=f"prepost.distance_transform_edt (uint8 mask, float32 distances) without and with return_indices='linear', and prepost.expand_labels "
                 f"(int32 labels, distance {DISTANCE}), resident on the device, exact integer path; {a.calls} calls per reading, {a.rounds} readings per "
                 "mode, modes alternated; one box, one call; host path timed once",
        device=torch.cuda.get_device_name(0), inputs=res, conditions={"expand_labels faster than the host path on every input measured": faster},
        note="indices_over_distance = median (b) / median (a), recorded, not capped: the index adds 12 bytes per voxel to the 32 of a uint8 call "
             "(1.375 by traffic) and its column passes run 6 waves per CU against 8 (module docstring); back-to-back calls at 256^3 work on 151 MB, "
             "inside the 256 MiB last-level cache: not an HBM figure",
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))
    print("wrote", a.out)
    return 0 if faster else 1


if __name__ == "__main__":
    sys.exit(main())

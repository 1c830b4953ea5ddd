"""What labelling a volume block by block and stitching the blocks costs on the device, against the single call and against the host path.
One box, one call, the configurations alternated, 20 calls per reading, three readings each (HIP events, after a warm-up call that is checked):
  (label)    prepost.label of the whole mask: the single call, in the same run;
  (slabs k)  prepost.label_blocks in k = 2 / 4 / 8 Z slabs, labelled and renumbered in place in views of the result (k = 1 IS the single call:
             label_blocks hands one slab to label, recorded as such);
  (grid)     prepost.label_blocks in a 2 x 2 x 2 grid: blocks copied in and out with torch;
  (stitch)   the stitch alone on 4 slabs that hold labels already: LabelStitcher.resolve() + apply() (begin, first, shell, resolve, the sort and
             the gathers, apply), set against its traffic floor of 12 bytes per voxel - 4 read by first, 4 read and 4 written by apply - at the
             4.5 TB/s yardstick of the project's streaming passes;
  (host)     device-to-host copy of the mask, scipy.ndimage.label, host-to-device copy of the labels - timed once per mask with the wall clock.
Masks: random balls of radius 3..9 at about 30 % fill, full connectivity, at 512^3 and (unless --no-1024) at 1024^3 (the 512^3 one tiled
2 x 2 x 2).  First of all label_blocks (4 slabs and the grid) is compared with SciPy bit for bit at 256^3; the warm-up call of every
configuration is compared with the single call's labels.  Back-to-back calls at 256^3 and, in part, at 512^3 (671 MB of mask and labels) sit in
the 256 MiB last-level cache: not HBM figures, and marked as such.
Past 2^31 voxels (unless --no-big): z-aligned rods and slabs at 1290 x 1290 x 1291, device only, the labels compared on the device with their
closed form (tests/stitch_ref.py: rods_mask, rods_expected, rods_check) - no host copy of the volume.
The one condition: label_blocks is faster than the host path on every mask where the host path was measured.  Exit status 1 if it fails.
Writes profiles/stitch_timing.json.
python scripts/stitch_timing.py [--calls 20] [--rounds 3] [--no-1024] [--no-big]"""
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

import stitch_ref as R  # noqa: E402
from biapy_amd import prepost  # noqa: E402

STREAM_TBPS = 4.5


def timed(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def host_path(m, conn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = m.cpu().numpy()
    t1 = time.perf_counter()
    want, count = ndimage.label(host, structure=ndimage.generate_binary_structure(3, conn))
    t2 = time.perf_counter()
    back = torch.from_numpy(want.astype(np.int32, copy=False)).cuda()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    ms = dict(d2h_mask=round((t1 - t0) * 1e3, 1), scipy_label=round((t2 - t1) * 1e3, 1), h2d_labels=round((t3 - t2) * 1e3, 1), total=round((t3 - t0) * 1e3, 1))
    return back, int(count), ms


def measure(name, mask_np, calls, rounds, with_host):
    m = torch.from_numpy(mask_np).cuda()
    n, size = m.numel(), m.shape[0]
    want, num = prepost.label(m, 3, return_num=True)
    count = int(num)
    host_ms = None
    if with_host:
        back, hcount, host_ms = host_path(m, 3)
        assert hcount == count and torch.equal(back, want), f"{name}: the single call disagrees with SciPy"
        del back
        print(f"{name}: host path {host_ms}, {count} components", flush=True)
    forms = {"label": lambda: prepost.label(m, 3)}
    for k in (2, 4, 8):
        forms[f"slabs {k}"] = (lambda k: lambda: prepost.label_blocks(m, (size // k, size, size), 3))(k)
    forms["grid 2x2x2"] = lambda: prepost.label_blocks(m, (size // 2,) * 3, 3)
    stitched = prepost.label_blocks(m, (size // 4, size, size), 3)
    st = prepost.LabelStitcher(m.shape, (size // 4, size, size), 3)
    for i in range(4):
        st.add((i, 0, 0), stitched[i * (size // 4):(i + 1) * (size // 4)], count)       # every slab holds labels 1..count already: the same unions, the same result

    def stitch_alone():
        st.resolve()
        st.apply()

    forms["stitch alone (4 slabs)"] = stitch_alone
    for k, fn in forms.items():                                            # warm-up call of each form, checked against the single call
        got = fn()
        got = stitched if got is None else got
        assert torch.equal(got, want), f"{name}: {k} disagrees with the single call"
        del got
    assert int(st.resolve()) == count
    one = prepost.label_blocks(m, (size, size, size), 3)
    assert torch.equal(one, want)
    del one
    readings = {k: [] for k in forms}
    for r in range(rounds):
        for k, fn in forms.items():
            readings[k].append(timed(fn, calls))
            print(f"{name}: round {r + 1} {k}: {readings[k][-1]:.3f} ms", flush=True)
    out = dict(voxels=n, connectivity=3, components=count, fill=round(float(mask_np.mean()), 4), host_ms=host_ms, calls_per_reading=calls, readings=rounds,
               stitch_floor_ms=round(n * 12 / (STREAM_TBPS * 1e12) * 1e3, 4), last_level_cache=bool(n * 5 <= 3 * 256 * 2 ** 20))
    for k, vs in readings.items():
        med = sorted(vs)[len(vs) // 2]
        out[k] = dict(readings_ms=[round(v, 4) for v in vs], median_ms=round(med, 4), spread_ms=round(max(vs) - min(vs), 4))
    base = out["label"]["median_ms"]
    for k in forms:
        if k.startswith(("slabs", "grid")):
            out[k]["over_single_call"] = round(out[k]["median_ms"] / base, 3)
            if host_ms:
                out[k]["host_over_device"] = round(host_ms["total"] / out[k]["median_ms"], 1)
    out["slabs 1"] = dict(note="label_blocks hands a single slab to label: the single call's launches", median_ms=base)
    out["stitch alone (4 slabs)"]["over_floor"] = round(out["stitch alone (4 slabs)"]["median_ms"] / out["stitch_floor_ms"], 1)
    del m, want, stitched, st
    torch.cuda.empty_cache()
    return out


def past_2_31(shape=(1290, 1290, 1291)):
    n = shape[0] * shape[1] * shape[2]
    assert n >= 2 ** 31
    mask = R.rods_mask(shape, "cuda")
    _, count = R.rods_expected(shape, "cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lab, num = prepost.label_blocks(mask, return_num=True)
    torch.cuda.synchronize()
    first_ms = (time.perf_counter() - t0) * 1e3
    ok = int(num) == count and R.rods_check(lab, shape)
    del lab
    ms = timed(lambda: prepost.label_blocks(mask), 2)
    del mask
    torch.cuda.empty_cache()
    return dict(shape=list(shape), voxels=n, slabs=-(-shape[0] // ((2 ** 31 - 1) // (shape[1] * shape[2]))), components=count, equals_closed_form=bool(ok),
                first_call_ms=round(first_ms, 1), call_ms=round(ms, 1), mask="z-aligned rods on a 4 x 4 lattice and y = 16 s + 2 slabs; labels compared on the device")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-1024", action="store_true")
    ap.add_argument("--no-big", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stitch_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "stitch_timing.py measures on the MI355X; there is nothing to measure without it"
    b256 = R.balls((256, 256, 256))
    want, n = R.scipy_label(b256, 3)
    m = torch.from_numpy(b256).cuda()
    for block in ((64, 256, 256), (128, 128, 128), (100, 90, 70)):
        got, num = prepost.label_blocks(m, block, 3, return_num=True)
        assert int(num) == n and np.array_equal(got.cpu().numpy(), want), f"256^3 in blocks {block} disagrees with SciPy"
    print(f"256^3: label_blocks equals scipy.ndimage.label bit for bit in 4 slabs, in a 2 x 2 x 2 grid and in a ragged 3 x 3 x 4 grid ({n} components)", flush=True)
    del m
    b512 = R.balls((512, 512, 512))
    res = {}
    for size in (512,) if a.no_1024 else (512, 1024):
        mask = b512 if size == 512 else np.tile(b512, (2, 2, 2))
        res[f"balls {size}^3"] = measure(f"balls {size}^3", mask, a.calls, a.rounds, True)
        del mask
    big = None if a.no_big else past_2_31()
    if big:
        print("past 2^31:", big, flush=True)
    faster = all(v[k]["median_ms"] < v["host_ms"]["total"] for v in res.values() if v["host_ms"] for k in v if k.startswith(("slabs ", "grid")) and "readings_ms" in v[k])
    cond = {"label_blocks faster than the host path on every mask measured": bool(faster), "past 2^31 voxels equals the closed form": None if big is None else big["equals_closed_form"]}
    out = dict(
        workload=f"prepost.label_blocks of a uint8 mask resident on the device, int32 labels, full connectivity; {a.calls} calls per reading, {a.rounds} readings per "
                 f"form, forms alternated; one box, one run; host path timed once per mask",
        device=torch.cuda.get_device_name(0), checked_at_256="label_blocks == scipy.ndimage.label bit for bit (4 slabs, 2 x 2 x 2, ragged 3 x 3 x 4)", masks=res,
        past_2_31=big, conditions=cond, yardstick_tbps=STREAM_TBPS,
        note="stitch floor = 12 bytes per voxel (first reads 4, apply reads 4 and writes 4); last_level_cache marks masks whose back-to-back calls may sit in "
             "the 256 MiB last-level cache in part: not HBM figures",
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))
    print("wrote", a.out)
    return 0 if faster and (big is None or big["equals_closed_form"]) else 1


if __name__ == "__main__":
    sys.exit(main())

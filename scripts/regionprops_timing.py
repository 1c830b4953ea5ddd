"""What the region properties cost on the device, against the host path a user has without them, and which form of the accumulate pass is the
default.  One box; per input and form 20 calls per reading, three readings, the two forms alternated reading by reading (HIP events, after a
warm-up call of each form).  Timed is prepost.region_props(labels, N) with N a Python int: bpx_region_props (init, accumulate, finish) and the
torch division that makes the centroid.
Inputs, at 256^3 and 512^3, and at 1024^3 on the device only (the 512^3 volume tiled 2 x 2 x 2 with the labels of every tile moved to a range of
their own):
  balls           prepost.label of random balls (radius 3..9, about 30 % fill), connectivity 1.
  instances       the project's own instances of the same mask: distance_transform_edt, label of the core d2 > 8, watershed.
  all background  a zero volume with N = 1000: what dropping the background runs is for.
  hard mask       prepost.label(random < 0.5, connectivity=1): hundreds of thousands of labels, most of them a few voxels - the block's table
                  overflows everywhere.
Before anything is timed the device result is compared bit for bit with tests/regionprops_ref.py on a 40^3 crop, in both forms; at 256^3 and
512^3 the host path's own results (np.bincount, find_objects, center_of_mass) are compared with the device's as well.
Recorded per input: both forms' readings, median and spread; the ratio of the default form to the traffic floor (4 bytes read per voxel at the
4.5 TB/s yardstick of the project's streaming passes).
(host) at 256^3 and 512^3: the device-to-host copy plus np.bincount + scipy.ndimage.find_objects + scipy.ndimage.center_of_mass - wall clock, once.
Condition 1: the device call (default form) is faster than that host path on every input measured.  Exit status 1 otherwise.
The default form: the one that is faster on the balls at 1024^3; form (a), the simpler one, when the difference is inside the spread of the three
readings.  The other form stays selectable only if it wins on some measured input.
Back-to-back calls on one volume: at 256^3 the 67 MB of labels stay in the 256 MB last-level cache between calls, so those readings are below
what a cold call costs; 512^3 (537 MB) and 1024^3 (4.3 GB) do not fit.
Writes profiles/regionprops_timing.json; --sizes runs a subset and merges into the file.
python scripts/regionprops_timing.py [--calls 20] [--rounds 3] [--sizes 256 512 1024]"""
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

from biapy_amd import _lib as L  # noqa: E402
from biapy_amd import prepost  # noqa: E402

STREAM_TBPS = 4.5
CORE_D2 = 8
HOOK = "bpx_debug_set_regionprops_local"
# both forms while the library has the hook that selects them; the one form that is left otherwise (recorded as form (b), the readings of the
# other form stay in the file as they were when it was last measured)
FORMS = {"a": 0, "b": 1} if HOOK in L.EXPORTS else {"b": 1}


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


def instances(mask):
    """The watershed instances of a mask, as scripts/overlap_timing.py makes its prediction."""
    d2 = prepost.distance_transform_edt(mask, squared=True)
    seeds = prepost.label((d2 > CORE_D2).to(torch.uint8), connectivity=1)
    return prepost.watershed(-d2, seeds, mask, connectivity=1)


def hard(n, seed=7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return prepost.label((torch.rand((n, n, n), device="cuda", generator=g) < 0.5).to(torch.uint8), connectivity=1)


def tiled(t):
    """2 x 2 x 2 copies of a label volume, the positive labels of copy q moved up by q * (max + 1)."""
    top = int(t.max()) + 1
    out = t.repeat(2, 2, 2)
    Z, Y, X = t.shape
    for q in range(1, 8):
        z, y, x = (q >> 2) & 1, (q >> 1) & 1, q & 1
        part = out[z * Z:(z + 1) * Z, y * Y:(y + 1) * Y, x * X:(x + 1) * X]
        part += (part > 0).to(torch.int32) * (q * top)
    return out


def set_form(form):
    if HOOK in L.EXPORTS:
        getattr(L.lib, HOOK)(form)


def check_crop(mask_np):
    import regionprops_ref as R

    crop = torch.from_numpy(np.ascontiguousarray(mask_np[:40, :40, :40])).cuda()
    for name, lab in (("label", prepost.label(crop, connectivity=1)), ("watershed", instances(crop))):
        n = int(lab.max())
        want = R.region_props_ref(lab.cpu().numpy(), n)
        for form in FORMS.values():
            set_form(form)
            p = prepost.region_props(lab, n)
            assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip((p.area, p.coord_sum, p.bbox), want)), \
                f"the device result differs from the reference on the 40^3 crop ({name}, form {form})"
        print(f"40^3 crop, {name}: form(s) {', '.join(FORMS)} equal the reference bit for bit, {n} labels", flush=True)
    set_form(-1)


def host_path(name, lab, n_max, p):
    """D2H + np.bincount + find_objects + center_of_mass, wall clock; their results against the device's."""
    from scipy import ndimage

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = lab.cpu().numpy()
    t1 = time.perf_counter()
    area = np.bincount(h.ravel(), minlength=n_max + 1)
    t2 = time.perf_counter()
    boxes = ndimage.find_objects(h, max_label=n_max) if n_max else []
    t3 = time.perf_counter()
    ids = np.flatnonzero(area[1:]) + 1
    com = np.asarray(ndimage.center_of_mass(h > 0, h, ids)) if ids.size else np.zeros((0, 3))
    t4 = time.perf_counter()
    ms = dict(d2h=round((t1 - t0) * 1e3, 1), bincount=round((t2 - t1) * 1e3, 1), find_objects=round((t3 - t2) * 1e3, 1),
              center_of_mass=round((t4 - t3) * 1e3, 1), total=round((t4 - t0) * 1e3, 1))
    assert np.array_equal(p.area.cpu().numpy()[1:], area[1:n_max + 1]), f"{name}: area differs from np.bincount"
    top = min(n_max, 100000)                                 # a Python loop over the slices: the first 10^5 labels of the hard mask's millions
    bbox = np.zeros((top + 1, 6), np.int32)
    for l, sl in enumerate(boxes[:top], start=1):
        if sl is not None:
            bbox[l] = [s.start for s in sl] + [s.stop for s in sl]
    assert np.array_equal(p.bbox[:top + 1].cpu().numpy(), bbox), f"{name}: bbox differs from find_objects"
    if ids.size:
        np.testing.assert_allclose(p.centroid.cpu().numpy()[ids], com, rtol=1e-12, atol=0, err_msg=f"{name}: centroid differs from center_of_mass")
    print(f"{name}: host path {ms}; the device result equals it", flush=True)
    return ms


def measure(name, lab, n_max, calls, rounds, with_host):
    n = lab.numel()
    run = lambda: prepost.region_props(lab, n_max)                                  # noqa: E731
    res = dict(voxels=n, n_max=n_max, floor_ms=round(n * 4 / (STREAM_TBPS * 1e12) * 1e3, 4))
    got, per = {}, {}
    for f, form in FORMS.items():                                                   # the warm-up call of each form; the two must agree
        set_form(form)
        got[f] = run()
        once = timed(run, 1)                                                        # a form that needs seconds per call gets fewer calls per reading
        per[f] = calls if once < 50 else 2 if once < 1000 else 1
    assert all(torch.equal(x, y) for g in got.values() for x, y in zip(g[:3], got["b"][:3])), f"{name}: the two forms differ"
    res["labels_present"] = int((got["b"].area > 0).sum())
    if with_host:
        res["host_ms"] = host_path(name, lab, n_max, got["b"])
    del got
    readings = {f: [] for f in FORMS}
    for _ in range(rounds):                                                         # alternated: a, b, a, b, a, b
        for f, form in FORMS.items():
            set_form(form)
            readings[f].append(timed(run, per[f]))
    set_form(-1)
    Z, Y, X = lab.shape                                                             # the three launches alone, default form, outputs allocated once
    area = torch.empty(n_max + 1, dtype=torch.int32, device=lab.device)
    sums = torch.empty((n_max + 1, 3), dtype=torch.int64, device=lab.device)
    bbox = torch.empty((n_max + 1, 6), dtype=torch.int32, device=lab.device)
    raw = lambda: L.check(L.lib.bpx_region_props(lab.data_ptr(), Z, Y, X, n_max, area.data_ptr(), sums.data_ptr(), bbox.data_ptr(), L.stream_ptr()))  # noqa: E731
    raw()
    res["launches_alone_ms"] = round(sorted(timed(raw, calls) for _ in range(rounds))[rounds // 2], 4)
    for f, vs in readings.items():
        res[f"form_{f}"] = dict(calls_per_reading=per[f], readings_ms=[round(v, 4) for v in vs], median_ms=round(sorted(vs)[len(vs) // 2], 4), spread_ms=round(max(vs) - min(vs), 4))
    print(f"{name}: {res['labels_present']} labels, " + ", ".join(f"form ({f}) {res['form_' + f]['median_ms']:.3f} ms" for f in readings)
          + f", floor {res['floor_ms']:.3f} ms", flush=True)
    return res


def decide(res):
    """The default form by the rule of the docstring, and whether the other one wins anywhere."""
    key = "balls 1024^3"
    if key not in res or "form_a" not in res[key]:
        return None
    a, b = res[key]["form_a"], res[key]["form_b"]
    spread = max(a["spread_ms"], b["spread_ms"])
    default = "b" if b["median_ms"] < a["median_ms"] - spread else "a"
    other = "a" if default == "b" else "b"
    wins = [k for k, v in res.items() if "form_a" in v and v[f"form_{other}"]["median_ms"] < v[f"form_{default}"]["median_ms"] - max(v["form_a"]["spread_ms"], v["form_b"]["spread_ms"])]
    return dict(default=default, rule_input=key, difference_ms=round(a["median_ms"] - b["median_ms"], 4), spread_ms=spread, other_form=other,
                other_form_wins_on=wins)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regionprops_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "regionprops_timing.py measures on the MI355X; there is nothing to measure without it"
    res = json.load(open(a.out))["inputs"] if os.path.exists(a.out) else {}
    b256 = balls(256)
    check_crop(b256)
    for s in a.sizes:
        base = 512 if s > 512 else s
        mask = torch.from_numpy(b256 if base == 256 else balls(512)).cuda()
        host = s <= 512
        up = tiled if s > 512 else (lambda t: t)
        for name, make in (("balls", lambda: prepost.label(mask, connectivity=1)), ("instances", lambda: instances(mask)),
                           ("all background", None), ("hard mask", lambda: hard(base))):
            lab = torch.zeros((s, s, s), dtype=torch.int32, device="cuda") if make is None else up(make())
            n_max = 1000 if make is None else int(lab.max())
            key = f"{name} {s}^3"
            res[key] = {**{k: v for k, v in res.get(key, {}).items() if k == "form_a"}, **measure(key, lab, n_max, a.calls, a.rounds, host)}
            del lab
            torch.cuda.empty_cache()
        del mask
    choice = decide(res)
    d = "form_" + (choice["default"] if choice else "b")
    for v in res.values():
        v["over_floor"] = round(v[d]["median_ms"] / v["floor_ms"], 1)
        if "host_ms" in v:
            v["host_over_device"] = round(v["host_ms"]["total"] / v[d]["median_ms"], 1)
    faster = bool(all(v[d]["median_ms"] < v["host_ms"]["total"] for v in res.values() if "host_ms" in v))
    out = dict(
        workload=f"prepost.region_props(labels, N) resident on the device: bpx_region_props (init, accumulate, finish) and the centroid's division; "
                 f"{a.calls} calls per reading, {a.rounds} readings per form, the forms alternated; one box; host path timed once",
        device=torch.cuda.get_device_name(0), inputs=res, default_form=choice,
        conditions={"device call faster than the host path on every input measured": faster},
        yardstick_tbps=STREAM_TBPS,
        note="floor = the label volume read once (4 bytes per voxel); over_floor and host_over_device are of the default form; form (a) = every "
             "run straight to the per-label arrays, form (b) = the block's table in LDS first; the init and finish passes over the N + 1 rows and "
             "the torch division are inside every reading (the hard mask has millions of rows); host path = device-to-host copy + np.bincount + "
             "scipy.ndimage.find_objects + scipy.ndimage.center_of_mass; at 256^3 the labels (67 MB) stay in the last-level cache between the "
             "back-to-back calls, at 512^3 and 1024^3 they do not fit",
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))
    print("wrote", a.out)
    return 0 if faster else 1


if __name__ == "__main__":
    sys.exit(main())

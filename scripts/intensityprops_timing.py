"""What the intensity properties cost on the device, against the host path a user has without them, and which form of the accumulate pass is
the default.  One box; per input and form 20 calls per reading, three readings, the forms and the inputs alternated reading by reading (HIP
events, after a warm-up call of each).  Timed is prepost.intensity_props(labels, image, N) with N a Python int: bpx_intensity_props (init,
accumulate, finish) and the allocation of its seven outputs.
Inputs, at 256^3 and 512^3, and at 1024^3 on the device only (the 512^3 volumes tiled 2 x 2 x 2 with the labels of every tile moved to a range of
their own): prepost.label of random balls (radius 3..9, about 30 % fill), connectivity 1, with
  float32   a probability map, 0.6 inside the balls plus uniform noise of 0.35: the confidence of an instance;
  uint8     a raw image, the same map scaled to 0..255;
and, beside the issue's inputs, `one label`: the float32 map under a label volume of ones - every trip uniform, every lane of the block at one
slot: what form (b) is for.
Before anything is timed the device result is compared bit for bit with tests/intensityprops_ref.py on a 40^3 crop, in both forms and both
image types.
Recorded per input: both forms' readings, median and spread; the ratio to prepost.region_props on the same labels in the same run; the ratio
of the default form to the traffic floor (labels and image read once: 8 bytes per voxel, 5 for uint8, at the 4.5 TB/s yardstick of the
project's streaming passes).
(host) at 256^3 and 512^3: the device-to-host copy of both volumes, scipy.ndimage.mean / minimum / maximum with an index, and the copy of the
three results back - wall clock, once; its mean is compared with the device's.
Condition 1: the device call (default form) is faster than that host path on every input measured.
Condition 2: the library's default form is the one this run chooses: the form that is faster on the float32 balls at 1024^3 by more than the
spread of the three readings; form (a), the simpler one, when neither is.  Exit status 1 when a condition does not hold.
Back-to-back calls on one pair of volumes: at 256^3 the 134 MB of labels and image (84 MB with uint8) stay in the 256 MB last-level cache
between calls, so those readings are below what a cold call costs; 512^3 and 1024^3 do not fit.
Writes profiles/intensityprops_timing.json.
python scripts/intensityprops_timing.py [--calls 20] [--rounds 3] [--sizes 256 512 1024]"""
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

from biapy_amd import _lib as L  # noqa: E402
from biapy_amd import prepost  # noqa: E402
from regionprops_timing import balls, tiled, timed  # noqa: E402

STREAM_TBPS = 4.5
HOOK = "bpx_debug_set_intensityprops_wave"
FORMS = {"a": 0, "b": 1}
RULE_INPUT = "balls float32 1024^3"


def set_form(form):
    getattr(L.lib, HOOK)(form)


def library_default():
    """The form the library runs when nothing is set, read from its source."""
    import re

    src = open(os.path.join(ROOT, "biapy_amd", "csrc", "intensityprops.hip")).read()
    return "ab"[int(re.search(r"constexpr int IP_DEFAULT_WAVE = (\d);", src).group(1))]


def images(mask):
    g = torch.Generator(device="cuda").manual_seed(11)
    prob = 0.6 * mask.to(torch.float32) + 0.35 * torch.rand(mask.shape, device="cuda", generator=g)
    return prob, (prob * (255.0 / 0.95)).to(torch.uint8)


def check_crop(mask_np):
    import intensityprops_ref as R

    crop = torch.from_numpy(np.ascontiguousarray(mask_np[:40, :40, :40])).cuda()
    lab = prepost.label(crop, connectivity=1)
    n = int(lab.max())
    for name, img in zip(("float32", "uint8"), images(crop)):
        want = R.intensity_props_ref(lab.cpu().numpy(), img.cpu().numpy(), n)
        for f, form in FORMS.items():
            set_form(form)
            p = prepost.intensity_props(lab, img, n)
            for field in R.FIELDS:
                assert R.same_bits(getattr(p, field).cpu().numpy(), want[field]), f"the device differs from the twin on the 40^3 crop ({name}, form {f}, {field})"
        print(f"40^3 crop, {name}: forms a, b equal the twin bit for bit, {n} labels", flush=True)
    set_form(-1)


def host_path(name, lab, img, n_max, p):
    """D2H of both volumes + scipy.ndimage.mean / minimum / maximum with an index + H2D of the results, wall clock."""
    from scipy import ndimage

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h, x = lab.cpu().numpy(), img.cpu().numpy()
    t1 = time.perf_counter()
    ids = np.arange(1, n_max + 1)
    mean = ndimage.mean(x, h, ids)
    t2 = time.perf_counter()
    lo = ndimage.minimum(x, h, ids)
    hi = ndimage.maximum(x, h, ids)
    t3 = time.perf_counter()
    back = [torch.from_numpy(np.asarray(v)).cuda() for v in (mean, lo, hi)]
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    ms = dict(d2h=round((t1 - t0) * 1e3, 1), mean=round((t2 - t1) * 1e3, 1), min_max=round((t3 - t2) * 1e3, 1), h2d=round((t4 - t3) * 1e3, 1),
              total=round((t4 - t0) * 1e3, 1))
    present = (p.area[1:] > 0).cpu().numpy()
    np.testing.assert_allclose(p.mean[1:].cpu().numpy()[present], np.asarray(mean, np.float64)[present], rtol=1e-9, err_msg=f"{name}: mean differs from scipy's")
    assert np.array_equal(p.min[1:].cpu().numpy()[present], np.asarray(lo)[present].astype(p.min.cpu().numpy().dtype)), f"{name}: min differs from scipy's"
    assert np.array_equal(p.max[1:].cpu().numpy()[present], np.asarray(hi)[present].astype(p.max.cpu().numpy().dtype)), f"{name}: max differs from scipy's"
    del back
    print(f"{name}: host path {ms}; the device result agrees with it", flush=True)
    return ms


def measure(jobs, calls, rounds):
    """jobs: name -> (labels, image, n_max, with_host).  The forms and the inputs alternated: every reading round visits every (input, form)."""
    res, runs, readings = {}, {}, {}
    for name, (lab, img, n_max, with_host) in jobs.items():
        n = lab.numel()
        runs[name] = (lambda lab=lab, img=img, n_max=n_max: prepost.intensity_props(lab, img, n_max))
        res[name] = dict(voxels=n, n_max=n_max, image=str(img.dtype).replace("torch.", ""),
                         floor_ms=round(n * (4 + img.element_size()) / (STREAM_TBPS * 1e12) * 1e3, 4))
        got = {}
        for f, form in FORMS.items():                                               # the warm-up call of each form; the two must agree
            set_form(form)
            got[f] = runs[name]()
        assert all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32) if x.dtype == torch.float32 else x,
                               y.view(torch.int64) if y.dtype == torch.float64 else y.view(torch.int32) if y.dtype == torch.float32 else y)
                   for x, y in zip(got["a"], got["b"])), f"{name}: the two forms differ"
        res[name]["labels_present"] = int((got["a"].area > 0).sum())
        if with_host:
            res[name]["host_ms"] = host_path(name, lab, img, n_max, got["a"])
        del got
        readings[name] = {f: [] for f in FORMS}
    region = {name: [] for name in jobs}
    for _ in range(rounds):
        for f, form in FORMS.items():
            set_form(form)
            for name in jobs:
                readings[name][f].append(timed(runs[name], calls))
        for name, (lab, img, n_max, _) in jobs.items():
            region[name].append(timed(lambda: prepost.region_props(lab, n_max), calls))
    set_form(-1)
    for name in jobs:
        for f, vs in readings[name].items():
            res[name][f"form_{f}"] = dict(readings_ms=[round(v, 4) for v in vs], median_ms=round(sorted(vs)[len(vs) // 2], 4), spread_ms=round(max(vs) - min(vs), 4))
        res[name]["region_props_ms"] = round(sorted(region[name])[rounds // 2], 4)
        print(f"{name}: {res[name]['labels_present']} labels, " + ", ".join(f"form ({f}) {res[name]['form_' + f]['median_ms']:.3f} ms" for f in FORMS)
              + f", region_props {res[name]['region_props_ms']:.3f} ms, floor {res[name]['floor_ms']:.3f} ms", flush=True)
    return res


def decide(res):
    if RULE_INPUT not in res:
        return None
    a, b = res[RULE_INPUT]["form_a"], res[RULE_INPUT]["form_b"]
    spread = max(a["spread_ms"], b["spread_ms"])
    default = "b" if b["median_ms"] < a["median_ms"] - spread else "a"       # (a), the simpler form, unless (b) wins by more than the spread
    other = "a" if default == "b" else "b"
    wins = [k for k, v in res.items() if v[f"form_{other}"]["median_ms"] < v[f"form_{default}"]["median_ms"] - max(v["form_a"]["spread_ms"], v["form_b"]["spread_ms"])]
    return dict(default=default, rule_input=RULE_INPUT, a_minus_b_ms=round(a["median_ms"] - b["median_ms"], 4), spread_ms=spread, other_form=other,
                other_form_wins_on=wins)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intensityprops_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "intensityprops_timing.py measures on the MI355X; there is nothing to measure without it"
    res = json.load(open(a.out))["inputs"] if os.path.exists(a.out) else {}
    b256 = balls(256)
    check_crop(b256)
    for s in a.sizes:
        base = 512 if s > 512 else s
        mask = torch.from_numpy(b256 if base == 256 else balls(512)).cuda()
        lab = prepost.label(mask, connectivity=1)
        prob, raw = images(mask)
        if s > 512:
            lab, prob, raw = tiled(lab), prob.repeat(2, 2, 2), raw.repeat(2, 2, 2)
        n_max = int(lab.max())
        host = s <= 512
        jobs = {f"balls float32 {s}^3": (lab, prob, n_max, host), f"balls uint8 {s}^3": (lab, raw, n_max, host),
                f"one label float32 {s}^3": (torch.ones_like(lab), prob, 1, False)}
        res.update(measure(jobs, a.calls, a.rounds))
        del jobs, lab, prob, raw, mask
        torch.cuda.empty_cache()
    choice = decide(res)
    lib_default = library_default()
    d = "form_" + (choice["default"] if choice else lib_default)
    for v in res.values():
        v["over_floor"] = round(v[d]["median_ms"] / v["floor_ms"], 1)
        v["over_region_props"] = round(v[d]["median_ms"] / v["region_props_ms"], 2)
        if "host_ms" in v:
            v["host_over_device"] = round(v["host_ms"]["total"] / v[d]["median_ms"], 1)
    faster = bool(all(v[d]["median_ms"] < v["host_ms"]["total"] for v in res.values() if "host_ms" in v))
    chosen = choice is not None and choice["default"] == lib_default
    out = dict(
        workload=f"prepost.intensity_props(labels, image, N) resident on the device: bpx_intensity_props (init, accumulate, finish); {a.calls} calls per "
                 f"reading, {a.rounds} readings per form, the forms and the inputs alternated; one box; host path timed once",
        device=torch.cuda.get_device_name(0), inputs=res, default_form=choice, library_default_form=lib_default,
        conditions={"device call faster than the host path on every input measured": faster,
                    "the library's default form is the one the rule chooses on the float32 balls at 1024^3": bool(chosen)},
        yardstick_tbps=STREAM_TBPS,
        note="floor = the label volume and the image read once (8 bytes per voxel, 5 for uint8); over_floor, over_region_props and host_over_device "
             "are of the chosen form; form (a) = each lane merges its four voxels and sends them to the block's table in LDS, form (b) = in addition a "
             "trip of 256 voxels of one label and one limb pair is reduced across the wave and sent once; the init and finish passes over the N + 1 "
             "rows and the allocation of the outputs are inside every reading; host path = device-to-host copy of both volumes + scipy.ndimage.mean "
             "/ minimum / maximum with an index + the copy of the results back; the 256^3 readings work inside the 256 MB last-level cache (labels "
             "and image are 134 MB, 84 MB with uint8, and stay there between the back-to-back calls), 512^3 and 1024^3 do not fit; `one label` is "
             "not one of the conditions' inputs",
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))
    print("wrote", a.out)
    return 0 if faster and chosen else 1


if __name__ == "__main__":
    sys.exit(main())

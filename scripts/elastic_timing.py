"""What the elastic deformation of the device augmenter costs, launch by launch and as a whole call, at the two shapes of its issue:
  3-D   4 x 128^3 x 1 fp32 image with a one-channel uint8 target;
  2-D   16 x 1 x 512 x 512 x 1 fp32 image with a one-channel uint8 target.
Per shape, after a warm-up call of each, `--steps` back-to-back repetitions between two HIP events per reading, `--rounds` readings each, the
configurations alternated reading by reading, the MEDIAN reading reported with the spread (the whole-call protocol of scripts/gauss_timing.py):
  (n)   bpx_elastic_noise alone: the (B, 2, Y, X) field written once;
  (s)   bpx_sepfilter alone on the field seen as (2B, Y, X): sigma 4, radius 16, y and x passes, mode reflect;
  (e)   bpx_elastic_apply alone, mode constant, every sample fired with alpha 14 through the smoothed field of a real call;
  (w)   bpx_warp_apply alone at the same shape and mode with drawn warp records (rotation, zoom, shear, shift all fired): THE YARDSTICK of (e) - it
        moves the same image and target bytes; (e) adds 8 B per (y, x) column, amortised over the z of a run and the channels;
  (c)   the whole call DeviceAugmenter(elastic={}, da_prob=1): bpx_aug_draw, bpx_elastic_draw, (n), (s), (e) and bpx_aug_apply (a copy here).
Reported, not asserted: (e), (w) and their ratio (expected within 1.25 on the 3-D shape).  Back-to-back repetitions re-read the same 33.5 MB
image, which fits the last-level cache, so these are not HBM figures.
Writes profiles/elastic_timing.json.
python scripts/elastic_timing.py [--steps 40] [--rounds 5] [--out profiles/elastic_timing.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from biapy_amd import _lib as L  # noqa: E402
from biapy_amd.augment import AFFINE_MODES, DeviceAugmenter  # noqa: E402

SHAPES = {"3-D 4 x 128^3 x 1": (4, 128, 128, 128), "2-D 16 x 1 x 512 x 512 x 1": (16, 1, 512, 512)}
AFFINE = dict(rotation=(-45, 45), zoom=(0.8, 1.25), shear=(-10, 10), shift=(-0.1, 0.1))
MODE = "constant"


def timed(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def stats(vs):
    return dict(readings_ms=[round(v, 4) for v in vs], median_ms=round(sorted(vs)[len(vs) // 2], 4), spread_ms=round(max(vs) - min(vs), 4))


def measure(name, shape, steps, rounds):
    B, Z, Y, X = shape
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((B, Z, Y, X, 1), device=dev, generator=g)
    t8 = (torch.rand((B, Z, Y, X, 1), device=dev, generator=g) > 0.5).to(torch.uint8)
    xo, to8 = torch.empty_like(x), torch.empty_like(t8)
    s = L.stream_ptr()

    aug = DeviceAugmenter(da_prob=1.0, seed=1, elastic=dict(mode=MODE))
    aug(x, t8, out=(xo, to8))                                              # one call: state, scratch, drawn records and a smoothed field
    erec, field = aug.last_elastic_records.clone(), aug.last_elastic_field.clone()
    assert bool((erec[:, 0] == 1).all()) and not torch.equal(xo, x)
    noise, ws, smooth = torch.empty_like(field), torch.empty_like(field), torch.empty_like(field)
    w, r = aug._ew, (len(aug._ew) - 1) // 2
    warp = DeviceAugmenter(da_prob=1.0, seed=1, affine_mode=MODE, **AFFINE)
    warp(x, t8, out=(xo, to8))
    wrec = warp.last_warp_records.clone()
    assert bool((wrec[:, 0] == 0xF).all())
    ex, et8 = torch.empty_like(x), torch.empty_like(t8)

    def noise_pass():
        L.check(L.lib.bpx_elastic_noise(1, B, Y, X, erec.data_ptr(), noise.data_ptr(), s))

    def smooth_pass():
        L.check(L.lib.bpx_sepfilter(noise.data_ptr(), 2 * B, Y, X, None, -1, w.ctypes.data, r, w.ctypes.data, r, 0, 0.0, smooth.data_ptr(), ws.data_ptr(),
                                    ws.numel() * 4, s))

    def elastic_pass():
        L.check(L.lib.bpx_elastic_apply(x.data_ptr(), t8.data_ptr(), L.U8, B, Z, Y, X, 1, 1, erec.data_ptr(), field.data_ptr(), AFFINE_MODES[MODE], 0.0,
                                        ex.data_ptr(), et8.data_ptr(), s))

    def warp_pass():
        L.check(L.lib.bpx_warp_apply(x.data_ptr(), t8.data_ptr(), L.U8, B, Z, Y, X, 1, 1, wrec.data_ptr(), AFFINE_MODES[MODE], 0.0, ex.data_ptr(),
                                     et8.data_ptr(), s))

    fns = {"n bpx_elastic_noise": noise_pass, "s bpx_sepfilter (sigma 4, y and x)": smooth_pass, "e bpx_elastic_apply": elastic_pass,
           "w bpx_warp_apply (yardstick)": warp_pass, "c whole call, elastic only": lambda: aug(x, t8, out=(xo, to8))}
    for fn in fns.values():                                                # warm-up
        fn()
    readings = {k: [] for k in fns}
    for rnd in range(rounds):
        for k, fn in fns.items():
            readings[k].append(timed(fn, steps))
            print(f"{name} round {rnd + 1} {k}: {readings[k][-1]:.4f} ms", flush=True)
    res = {k: stats(v) for k, v in readings.items()}
    e, wv = res["e bpx_elastic_apply"]["median_ms"], res["w bpx_warp_apply (yardstick)"]["median_ms"]
    moved = x.numel() * 4 * 2 + t8.numel() * 2
    return dict(shape=dict(B=B, Z=Z, Y=Y, X=X, C=1, Ct=1, target="uint8"), mode=MODE, ms=res,
                elastic_apply_over_warp_apply=round(e / wv, 3),
                bytes=dict(image_and_target_read_and_written=moved, field_read_by_elastic_apply=field.numel() * 4 * ((Z + 7) // 8),
                           note="bpx_elastic_apply reads the two displacement words of a (y, x) column once per run of 8 z planes"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "elastic_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "elastic_timing.py measures on the MI355X; there is nothing to measure without it"
    res = {name: measure(name, shape, a.steps, a.rounds) for name, shape in SHAPES.items()}
    out = dict(
        workload=f"biapy_amd.augment.DeviceAugmenter(elastic=...), sigma 4 (radius 16), alpha 12..16, mode {MODE}, every sample fired; {a.steps} "
                 f"repetitions per reading, {a.rounds} readings per configuration, alternated; median and spread; one box",
        device=torch.cuda.get_device_name(0), shapes=res,
        expectation="bpx_elastic_apply within 1.25 x bpx_warp_apply on the 3-D shape (a reported figure, not an assertion)",
        note="back-to-back repetitions re-read the same 33.5 MB image, which fits the last-level cache: not HBM figures",
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""A/B of the small-tile conv kernel's wave mapping (conv3_kernel<..., WN>, bpx_debug_set_conv_wn) on the <= 16^3 layers of cfg 2 (B = 4): the
six forward rows of tests/bench_kernels.py conv_fwd in the benched mixed mode (fp16 storage) and their input-gradient twins (MIX16: bf16 gradients,
fp16 t, ELU' epilogue with both sums).  One process, WN alternating 1 / 2 / 4 / 1 / 2 / 4 per layer; a WN without an instance reads "-".

    python scripts/bench_conv_wn.py [--reps 50] [--rounds 2]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from biapy_amd import _lib as L  # noqa: E402

lib = L.lib
DEV = "cuda"
# (spatial, Cin, Cout, shortcut C): tests/bench_kernels.py FWD_LAYERS, the <= 16^3 rows
LAYERS = [(16, 384, 128, 0), (16, 128, 128, 384), (16, 64, 128, 0), (16, 128, 128, 64), (8, 128, 256, 0), (8, 256, 256, 128)]
WNS = (1, 2, 4)


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def pack(w, mode, cin, cout, dt, T):
    out = torch.empty(lib.bpx_packed_weight_elems(mode, cin, cout, dt), dtype=T, device=DEV)
    L.check(lib.bpx_pack_weight(mode, w.data_ptr(), cin, cout, dt, out.data_ptr(), L.stream_ptr()))
    return out


def ab(name, fn, dt, S, cout, reps, rounds):
    cells = []
    for _ in range(rounds):
        for wn in WNS:
            if not lib.bpx_conv3d_wn_supported(dt, S, S, S, cout, wn):
                cells.append("      -")
                continue
            lib.bpx_debug_set_conv_wn(wn)
            cells.append(f"{timeit(fn, reps):7.1f}")
    lib.bpx_debug_set_conv_wn(-1)
    print(f"{name}: " + " ".join(cells), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    B, st = 4, L.stream_ptr()
    print("us per launch, WN = " + " / ".join(str(w) for w in WNS) + f", {a.rounds} rounds in turn")
    for (S, cin, cout, csc) in LAYERS:
        H = torch.float16
        x = torch.randn(B, S, S, S, cin, device=DEV).to(H)
        if cin == 384:
            x = L.Planar(B, (S, S, S), cin, H, DEV).copy_from_dense(x)
        y = torch.empty(B, S, S, S, cout, device=DEV, dtype=H)
        wp = pack(torch.randn(cout, cin, 3, 3, 3, device=DEV) * 0.05, L.PK_K3, cin, cout, L.F16, H)
        bias = torch.zeros(cout, device=DEV)
        rec = torch.rand(B, cin, 4, device=DEV)
        part = torch.empty(B, lib.bpx_conv3d_stats_tiles(L.F16, B, S, S, S, cout), 2, cout, device=DEV)
        sct, wscp, keep = L.NULL_T, None, []
        if csc:
            sc = torch.randn(B, S, S, S, csc, device=DEV).to(H)
            if csc == 384:
                sc = L.Planar(B, (S, S, S), csc, H, DEV).copy_from_dense(sc)
            wk = pack(torch.randn(cout, csc, 1, 1, 1, device=DEV), L.PK_K1, csc, cout, L.F16, H)
            sct, wscp, keep = L.tview(sc), wk.data_ptr(), [sc, wk]
        f = lambda: L.check(lib.bpx_conv3d_fwd(L.F16, B, S, S, S, L.tview(x), rec.data_ptr(), 1, wp.data_ptr(), bias.data_ptr(), sct, wscp,
                                               bias.data_ptr() if csc else None, L.tview(y), part.data_ptr(), st))
        ab(f"conv_fwd   {S:3d}^3 {cin:4d}->{cout:4d} sc={csc:4d}", f, L.F16, S, cout, a.reps, a.rounds)
        # the twin: dy of the forward's output channels -> g of its input channels
        G = torch.bfloat16
        dy = torch.randn(B, S, S, S, cout, device=DEV).to(G)
        t = torch.randn(B, S, S, S, cin, device=DEV).to(H)
        g = torch.empty(B, S, S, S, cin, device=DEV, dtype=G)
        wt = pack(torch.randn(cout, cin, 3, 3, 3, device=DEV) * 0.05, L.PK_K3_T, cin, cout, L.BF16, G)
        rect = torch.rand(B, cin, 4, device=DEV)
        red = torch.empty(B, lib.bpx_conv3d_stats_tiles(L.BF16, B, S, S, S, cin), 2, cin, device=DEV)
        f = lambda: L.check(lib.bpx_conv3d_dgrad(L.MIX16, B, S, S, S, L.tview(dy), wt.data_ptr(), L.tview(t), rect.data_ptr(), 1, L.tview(g), red.data_ptr(), st))
        ab(f"conv_dgrad {S:3d}^3 dy{cout:4d}->g{cin:4d}       ", f, L.MIX16, S, cin, a.reps, a.rounds)


if __name__ == "__main__":
    main()

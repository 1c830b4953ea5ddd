"""Parity checks of every C-ABI kernel against plain PyTorch CPU fp32 / the oracle.

Each ``check_*`` returns a list of result dicts ``{name, err, tol, ok}`` so that the same code serves the
pytest suite (asserts) and ``tests/gpu_diag.py`` (prints a full table without stopping at the first
failure - useful on the GPU box where a call costs minutes).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch
import torch.nn.functional as F

from biapy_amd import _lib as L
from biapy_amd import tiling
from biapy_amd.engine import NetConfig, ResUNetEngine
from oracle import net_oracle
from oracle import tiling_oracle as TO

lib = L.lib
DEV = "cuda"


def _res(name, err, tol, extra=""):
    return dict(name=name, err=float(err), tol=float(tol), ok=bool(err <= tol), extra=extra)


def tdtype(dt):
    return {L.BF16: torch.bfloat16, L.F16: torch.float16, L.MIX16: torch.bfloat16}.get(dt, torch.float32)   # MIX16: a 16-bit container (packed weights)


def rnd(t, dt):
    """Round an fp32 CPU tensor to the storage dtype and back (what the device actually holds)."""
    return t.to(tdtype(dt)).float()


def to_dev(t, dt):
    return t.to(tdtype(dt)).to(DEV).contiguous()


def relerr(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def tol_for(dt):
    return {L.BF16: 1.5e-2, L.F16: 2e-3}.get(dt, 2e-5)


def ncdhw(t):  # (B,D,H,W,C) -> (B,C,D,H,W)
    return t.permute(0, 4, 1, 2, 3).contiguous()


def ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def pack(w, mode, cin, cout, dt):
    n = lib.bpx_packed_weight_elems(mode, cin, cout, dt)
    out = torch.empty(n, dtype=tdtype(dt), device=DEV)
    wd = w.float().contiguous().to(DEV)
    L.check(lib.bpx_pack_weight(mode, wd.data_ptr(), cin, cout, dt, out.data_ptr(), L.stream_ptr()))
    return out


def check_pack_batched(dt, seed=0):
    """bpx_pack_weights_batched (one launch, blocks proportional to the operand sizes) == bpx_pack_weight operand by operand, bit for bit: every
    pack mode, tiny and 1.8 M-element operands in one batch, more than 64 jobs (two launches)."""
    import ctypes as C
    g = torch.Generator().manual_seed(seed)
    shapes = []     # (mode, Cin, Cout, weight shape)
    for cin, cout in ((16, 16), (48, 16), (256, 256), (384, 128), (32, 64)):
        shapes.append((L.PK_K3, cin, cout, (cout, cin, 3, 3, 3)))
        shapes.append((L.PK_K3_T, cin, cout, (cout, cin, 3, 3, 3)))
        shapes.append((L.PK_DENSE, cin, cout, (cout, cin, 1, 1, 1)))
        shapes.append((L.PK_DENSE_T, cin, cout, (cout, cin, 1, 1, 1)))
        shapes.append((L.PK_K1, cin, cout, (cout, cin, 1, 1, 1)))
    for c in (32, 128):
        shapes.append((L.PK_CT, c, c, (c, c, 2, 2, 2)))
        shapes.append((L.PK_CT_T, c, c, (c, c, 2, 2, 2)))
        shapes.append((L.PK_CT4, c, c, (c, c, 1, 2, 2)))
        shapes.append((L.PK_CT4_T, c, c, (c, c, 1, 2, 2)))
    shapes = shapes * 3                                   # 99 jobs: two launches
    ws = [torch.randn(*sh, generator=g).to(DEV) for _, _, _, sh in shapes]
    es = 4 if dt == L.F32 else 2
    sizes = [int(lib.bpx_packed_weight_elems(m, ci, co, dt)) for m, ci, co, _ in shapes]
    offs, tot = [], 0
    for n in sizes:
        offs.append(tot)
        tot += (n + 127) // 128 * 128
    buf = torch.full((tot * es,), 0x5A, dtype=torch.uint8, device=DEV)
    jobs = (L.PackJob * len(shapes))()
    for q, ((m, ci, co, _), off) in enumerate(zip(shapes, offs)):
        jobs[q] = L.PackJob(ws[q].data_ptr(), buf.data_ptr() + off * es, m, ci, co, 0)
    L.check(lib.bpx_pack_weights_batched(dt, len(shapes), C.cast(jobs, C.c_void_p), L.stream_ptr()))
    torch.cuda.synchronize()
    bad = 0
    for q, ((m, ci, co, _), off) in enumerate(zip(shapes, offs)):
        one = torch.empty(sizes[q] * es, dtype=torch.uint8, device=DEV)
        L.check(lib.bpx_pack_weight(m, ws[q].data_ptr(), ci, co, dt, one.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
        bad += int((buf[off * es:(off + sizes[q]) * es] != one).sum().item())
        gap = buf[(off + sizes[q]) * es:(offs[q + 1] if q + 1 < len(offs) else tot) * es]
        bad += int((gap != 0x5A).sum().item())             # nothing written past an operand
    return [_res(f"pack_batched[dt{dt} {len(shapes)} jobs].bytes_differ", bad, 0)]


def make_recs(B, Cc, seed):
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(B, Cc, generator=g) * 0.3
    rstd = 0.5 + torch.rand(B, Cc, generator=g)
    gamma = 1 + 0.2 * torch.randn(Cc, generator=g)
    beta = 0.2 * torch.randn(Cc, generator=g)
    scale = gamma[None] * rstd
    shift = beta[None] - mean * scale
    rec = torch.stack([mean, rstd, scale, shift], -1).contiguous()
    return rec, gamma, beta


# ---------------------------------------------------------------------------------------------------
def check_selftest():
    out = torch.zeros(1024, dtype=torch.float32, device=DEV)
    L.check(lib.bpx_selftest_layouts(out.data_ptr(), L.stream_ptr()))
    o = out.cpu().numpy()
    res = []
    i = np.arange(16)[:, None]
    for blk, K in ((0, 32), (1, 16)):
        k = np.arange(K)
        A = ((3 * i + 5 * k[None, :]) % 7 - 3).astype(np.float64)
        Bm = ((2 * k[:, None] + 7 * np.arange(16)[None, :]) % 5 - 2).astype(np.float64)
        ref = A @ Bm
        got = o[blk * 256:(blk + 1) * 256].reshape(16, 16)
        res.append(_res(f"mfma_layout_{'bf16_16x16x32' if blk == 0 else 'f32_16x16x4'}", np.abs(got - ref).max(), 0.0))
    tr = o[512:].reshape(64, 8)
    lane = np.arange(64)
    exp = ((8 * (lane >> 4))[:, None] + np.arange(8)[None, :]) * 16 + (lane & 15)[:, None]
    bad = int((tr != exp).sum())
    extra = ""
    if bad:
        extra = "lane0=%s lane1=%s lane5=%s lane17=%s" % (tr[0].tolist(), tr[1].tolist(), tr[5].tolist(), tr[17].tolist())
    res.append(_res("ds_read_tr16_b64_layout", bad, 0, extra))
    return res


# ---------------------------------------------------------------------------------------------------
def check_tiling(golden):
    res = []
    from make_golden import synth_pred, synth_volume

    for name in ["m48", "m_odd", "m_pad", "m_zeros", "m_median"]:
        a = golden[f"data/{name}/args"]
        vshape, pshape, pad, med = tuple(int(v) for v in a[0:4]), tuple(int(v) for v in a[4:8]), tuple(int(v) for v in a[8:11]), bool(a[11])
        ov = tuple(float(v) for v in golden[f"data/{name}/overlap"])
        seed = int(golden[f"data/{name}/seed"])
        pad_type = str(golden[f"data/{name}/pad_type"])
        vol, mask = synth_volume(seed, vshape)
        p, pm, coords = tiling.crop_3D_data_with_overlap(vol, pshape, data_mask=mask, overlap=ov, padding=pad, verbose=False,
                                                         median_padding=med, pad_type=pad_type)
        cref = golden[f"data/{name}/coords"]
        cgot = np.array([[c.z_start, c.z_end, c.y_start, c.y_end, c.x_start, c.x_end] for c in coords])
        e = int((cgot != cref).sum())
        e += int((p[0] != golden[f"data/{name}/patch0"]).sum()) + int((p[-1] != golden[f"data/{name}/patch_last"]).sum())
        e += int((pm[-1] != golden[f"data/{name}/mask_patch_last"]).sum())
        crc = int(np.frombuffer(p.tobytes(), dtype=np.uint8).astype(np.uint64).sum())
        e += int(crc != int(golden[f"data/{name}/patches_crc"][0]))
        res.append(_res(f"crop_dropin[{name}]", e, 0))
        pred = synth_pred(seed, p.shape)
        merged, merged_mask = tiling.merge_3D_data_with_overlap(pred, vshape, data_mask=pm, overlap=ov, padding=pad, verbose=False)
        e = int((merged.view(np.uint32) != golden[f"data/{name}/merged"].view(np.uint32)).sum())
        res.append(_res(f"merge_dropin_f32_bits[{name}]", e, 0))
        res.append(_res(f"merge_dropin_u8mask[{name}]", int((merged_mask != golden[f"data/{name}/merged_mask"]).sum()), 0))
    for lab in (1, 2, 3, 5, 255):
        pm = np.full((27, 32, 32, 32, 1), lab, dtype=np.uint8)
        pd = np.ones((27, 32, 32, 32, 1), dtype=np.float32)
        _, mm = tiling.merge_3D_data_with_overlap(pd, (48, 48, 48, 1), data_mask=pm, overlap=(0.5, 0.5, 0.5), verbose=False)
        res.append(_res(f"merge_label_truncation[{lab}]", int((mm != golden[f"label/{lab}/merged_mask"]).sum()), 0))
    # float16 patches (TEST.REDUCE_MEMORY) vs the oracle
    rs = np.random.RandomState(5)
    p16 = rs.rand(27, 32, 32, 32, 2).astype(np.float16)
    m_ref = TO.merge(p16, (48, 48, 48, 2), overlap=(0.5, 0.5, 0.5))
    m_got = tiling.merge_3D_data_with_overlap(p16, (48, 48, 48, 2), overlap=(0.5, 0.5, 0.5), verbose=False)
    res.append(_res("merge_f16", int((m_got.view(np.uint16) != m_ref.view(np.uint16)).sum()), 0))
    return res


def check_tiling_row_kernels(n_cases=40, seed=7):
    """The 16-byte row kernels of crop / merge (the production path) against the oracle AND against the element-per-thread
    kernels of round 1 (bpx_debug_set_tiling_scalar), bit for bit, over random geometries: channel counts 1-4 (vectors that
    straddle voxels and patch edges), odd volume / patch extents, overlaps, padding with reflect / zeros, f32 / f16 / u8,
    sharded blends (row range + z range, seeded and partial-sum modes)."""
    from biapy_amd import _lib as L

    rs = np.random.RandomState(seed)
    res, bad_crop, bad_merge, bad_shard, n_vec = [], 0, 0, 0, 0
    for case in range(n_cases):
        C = int(rs.choice([1, 1, 2, 3, 4]))
        patch = tuple(int(v) for v in (rs.randint(4, 13), rs.randint(4, 13), 4 * rs.randint(2, 7)))
        if C == 3:
            patch = patch[:2] + (4 * int(rs.randint(2, 7)),)          # x*C must be a multiple of 4 for the vector path
        pad = tuple(int(rs.randint(0, max(1, p // 2 - 1))) if rs.rand() < 0.5 else 0 for p in patch)
        vol = tuple(int(p + rs.randint(0, 2 * p)) for p in patch)
        if rs.rand() < 0.7:                                             # the merge's vector path needs X*C % 4 == 0
            vol = vol[:2] + (int(-(-vol[2] // 4) * 4),)
        ov = tuple(float(rs.choice([0.0, 0.25, 0.5, 0.6])) for _ in range(3))
        pad_type = str(rs.choice(["reflect", "zeros"]))
        np_dt = [np.float32, np.float32, np.float16, np.uint8][int(rs.randint(0, 4))]
        v = (rs.rand(*vol, C) * (255 if np_dt == np.uint8 else 1)).astype(np_dt)
        try:
            p_ref, _ = TO.crop(v, patch + (C,), ov, pad, pad_type=pad_type)
        except (ValueError, AssertionError):
            continue
        tv = torch.from_numpy(v.view({1: np.uint8, 2: np.int16, 4: np.int32}[v.dtype.itemsize])).to(DEV)
        outs = []
        for scalar in (0, 1):
            L.lib.bpx_debug_set_tiling_scalar(scalar)
            outs.append(tiling.crop_device(tv, patch, ov, pad, pad_type).cpu().numpy().view(np_dt))
        L.lib.bpx_debug_set_tiling_scalar(0)
        bad_crop += int((outs[0] != p_ref).sum()) + int((outs[0] != outs[1]).sum())
        # merge: random predictions shaped like the patches
        pred = (rs.rand(*p_ref.shape) * (255 if np_dt == np.uint8 else 1)).astype(np_dt)
        m_ref = TO.merge(pred, vol + (C,), overlap=ov, padding=pad)
        plan = tiling.MergePlan(vol, patch, ov, pad, torch.device(DEV))
        tp = torch.from_numpy(pred).to(DEV)
        outs = []
        for scalar in (0, 1):
            L.lib.bpx_debug_set_tiling_scalar(scalar)
            outs.append(tiling.merge_device(tp, plan).cpu().numpy())
        L.lib.bpx_debug_set_tiling_scalar(0)
        as_bits = lambda a: a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])  # noqa: E731
        bad_merge += int((as_bits(outs[0]) != as_bits(m_ref)).sum()) + int((as_bits(outs[0]) != as_bits(outs[1])).sum())
        n_vec += int((vol[2] * C) % (4 if np_dt == np.float32 else 8) == 0)
        # sharded: two row ranges, the boundary handed over as partial sums
        nz = plan.grid[0].n
        starts = [plan.row_start(i) for i in range(nz)]
        if nz >= 2 and np_dt == np.float32 and starts == sorted(starts):     # (non-monotonic starts cannot be sharded: workflow.plan_slabs)
            ny, nx = plan.grid[1].n, plan.grid[2].n
            h = nz // 2
            core = patch[0] - 2 * pad[0]
            z_split, z0_hi = plan.row_start(h), min(plan.row_start(h - 1) + core, vol[0])
            r0, r1 = tp[: h * ny * nx].contiguous(), tp[h * ny * nx:].contiguous()
            out = np.empty(vol + (C,), np.float32)
            if z_split > 0:
                out[:z_split] = tiling.merge_device(r0, plan, z_lo=0, z_hi=z_split, zrow_lo=0, zrow_hi=h).cpu().numpy()
            if z0_hi > z_split:
                nb = z0_hi - z_split
                acc = torch.zeros((nb, vol[1], vol[2], C), dtype=torch.float32, device=DEV)
                wacc = torch.zeros((nb, vol[1], vol[2], 1), dtype=torch.float32, device=DEV)
                tiling.merge_device(r0, plan, z_lo=z_split, z_hi=z0_hi, zrow_lo=0, zrow_hi=h, acc=acc, wacc=wacc, write_partial=True)
                out[z_split:z0_hi] = tiling.merge_device(r1, plan, z_lo=z_split, z_hi=z0_hi, zrow_lo=h, zrow_hi=nz, acc=acc, wacc=wacc, seed=True).cpu().numpy()
            if vol[0] > max(z0_hi, z_split):
                lo = max(z0_hi, z_split)
                out[lo:] = tiling.merge_device(r1, plan, z_lo=lo, z_hi=vol[0], zrow_lo=h, zrow_hi=nz).cpu().numpy()
            bad_shard += int((out.view(np.uint32) != m_ref.view(np.uint32)).sum())
    res.append(_res("crop_row_kernel_vs_oracle_and_scalar", bad_crop, 0))
    res.append(_res("merge_row_kernel_vs_oracle_and_scalar", bad_merge, 0, f"{n_vec} cases on the vector path"))
    res.append(_res("merge_row_kernel_sharded", bad_shard, 0))
    res.append(_res("row_kernel_cases_on_vector_path", 0 if n_vec >= n_cases // 3 else 1, 0))
    return res


def check_merge_sharded():
    """Two Z-slabs with the boundary partial sums handed over must equal the single-device merge bit for bit."""
    rs = np.random.RandomState(11)
    vshape, pshape, ov = (72, 40, 40, 1), (32, 32, 32, 1), (0.5, 0.5, 0.5)
    vol = rs.rand(*vshape).astype(np.float32)
    p, coords = TO.crop(vol, pshape, ov)
    pred = rs.rand(*p.shape).astype(np.float32)
    ref = TO.merge(pred, vshape, overlap=ov)
    plan = tiling.MergePlan(vshape[:3], pshape[:3], ov, (0, 0, 0), torch.device(DEV))
    nz, ny, nx = plan.grid[0].n, plan.grid[1].n, plan.grid[2].n
    t = torch.from_numpy(pred).to(DEV)
    full = tiling.merge_device(t, plan).cpu().numpy()
    res = [_res("merge_device_vs_oracle", int((full.view(np.uint32) != ref.view(np.uint32)).sum()), 0)]
    # rank 0 owns patch rows [0,h), rank 1 rows [h,nz)
    h = nz // 2
    z_split = plan.row_start(h)                      # first slice touched by rank 1's patches
    z0_hi = plan.row_start(h - 1) + pshape[0]        # one past the last slice touched by rank 0
    r0 = t[: h * ny * nx].contiguous()
    r1 = t[h * ny * nx:].contiguous()
    out = np.empty(vshape, np.float32)
    out[:z_split] = tiling.merge_device(r0, plan, z_lo=0, z_hi=z_split, zrow_lo=0, zrow_hi=h).cpu().numpy()
    nb = z0_hi - z_split
    acc = torch.zeros((nb, vshape[1], vshape[2], 1), dtype=torch.float32, device=DEV)
    wacc = torch.zeros((nb, vshape[1], vshape[2], 1), dtype=torch.float32, device=DEV)
    tiling.merge_device(r0, plan, z_lo=z_split, z_hi=z0_hi, zrow_lo=0, zrow_hi=h, acc=acc, wacc=wacc, write_partial=True)
    # (acc, wacc) is what travels over xGMI; rank 1 seeds its boundary with it
    out[z_split:z0_hi] = tiling.merge_device(r1, plan, z_lo=z_split, z_hi=z0_hi, zrow_lo=h, zrow_hi=nz, acc=acc, wacc=wacc, seed=True).cpu().numpy()
    out[z0_hi:] = tiling.merge_device(r1, plan, z_lo=z0_hi, z_hi=vshape[0], zrow_lo=h, zrow_hi=nz).cpu().numpy()
    res.append(_res("merge_two_slabs_bit_exact", int((out.view(np.uint32) != ref.view(np.uint32)).sum()), 0))
    return res


# ---------------------------------------------------------------------------------------------------
def _act_ref(u, act):
    return {0: lambda v: v, 1: lambda v: F.elu(v), 2: F.relu, 3: F.silu, 4: F.leaky_relu, 5: F.gelu, 6: torch.tanh, 7: torch.sigmoid, 8: F.softplus}[act](u)


def _dact_ref(u, act):
    """act'(u) by autograd of the PyTorch operator."""
    v = u.detach().clone().requires_grad_(True)
    _act_ref(v, act).sum().backward()
    return v.grad


def check_conv3d_fwd(dt, B, S, Cin, Cout, norm=True, sc_C=0, slices=False, seed=0, act=1):
    D, H, W = S
    g = torch.Generator().manual_seed(seed)
    x = rnd(torch.randn(B, D, H, W, Cin, generator=g), dt)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    rec = None
    a = x
    if norm:
        rec, _, _ = make_recs(B, Cin, seed + 1)
        a = rnd(_act_ref(x * rec[:, None, None, None, :, 2] + rec[:, None, None, None, :, 3], act), dt)
    y_ref = F.conv3d(ncdhw(a), rnd(w, dt), b, padding=1)
    sc = wsc = bsc = None
    if sc_C:
        if sc_C == 1:
            sc = torch.randn(B, D, H, W, generator=g)
            wsc = torch.randn(Cout, 1, 1, 1, 1, generator=g)
            bsc = torch.randn(Cout, generator=g) * 0.1
            y_ref = y_ref + sc[:, None] * wsc.view(1, Cout, 1, 1, 1) + bsc.view(1, Cout, 1, 1, 1)
        else:
            sc = rnd(torch.randn(B, D, H, W, sc_C, generator=g), dt)
            wsc = torch.randn(Cout, sc_C, 1, 1, 1, generator=g) / sc_C ** 0.5
            bsc = torch.randn(Cout, generator=g) * 0.1
            y_ref = y_ref + F.conv3d(ncdhw(sc), rnd(wsc, dt), bsc)
    # device buffers (optionally channel slices of wider buffers)
    xo, yo = (16, 32) if slices else (0, 0)
    xb = torch.zeros(B, D, H, W, Cin + 2 * xo, dtype=tdtype(dt), device=DEV)
    xb[..., xo:xo + Cin] = to_dev(x, dt)
    yb = torch.full((B, D, H, W, Cout + 2 * yo), 7.0, dtype=tdtype(dt), device=DEV)
    wp = pack(w, L.PK_K3, Cin, Cout, dt)
    tiles = lib.bpx_conv3d_stats_tiles(dt, B, D, H, W, Cout)
    part = torch.zeros(B, tiles, 2, Cout, dtype=torch.float32, device=DEV)
    recd = rec.to(DEV) if rec is not None else None
    bd = b.to(DEV)
    sct, wscp, bscd = L.NULL_T, None, None
    keep = []
    if sc_C == 1:
        scd = sc.to(DEV).contiguous(); wscd = wsc.to(DEV).contiguous(); bscd = bsc.to(DEV)
        sct, wscp = L.Tensor(scd.data_ptr(), 1, 1), wscd.data_ptr()
        keep += [scd, wscd]
    elif sc_C:
        scd = to_dev(sc, dt); wpk = pack(wsc, L.PK_K1, sc_C, Cout, dt); bscd = bsc.to(DEV)
        sct, wscp = L.tview(scd), wpk.data_ptr()
        keep += [scd, wpk]
    L.check(lib.bpx_conv3d_fwd(dt, B, D, H, W, L.tview(xb, xo, Cin), L.ptr(recd), act if norm else 0, wp.data_ptr(), bd.data_ptr(), sct, wscp,
                               L.ptr(bscd), L.tview(yb, yo, Cout), part.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    y = ndhwc(y_ref)
    got = yb[..., yo:yo + Cout].float().cpu()
    tag = f"conv3d_fwd[{ {L.BF16: 'bf16', L.F16: 'f16'}.get(dt, 'f32') } B{B} {S} {Cin}->{Cout} norm={int(norm)} sc={sc_C} sl={int(slices)}]"
    res = [_res(tag, relerr(got, y), tol_for(dt))]
    if slices:
        untouched = (yb[..., :yo].float() == 7).all().item() and (yb[..., yo + Cout:].float() == 7).all().item()
        res.append(_res(tag + ".neighbours_untouched", 0 if untouched else 1, 0))
    s = part.sum(1).cpu()
    s_ref = torch.stack([y.sum((1, 2, 3)), (y * y).sum((1, 2, 3))], 1)
    res.append(_res(tag + ".stats", relerr(s, s_ref), 5e-3 if dt in (L.BF16, L.F16) else 1e-4))
    return res


def check_conv3d_zmarch(f16, B, S, Cin, sc_C=0, pool=0, planar=False, norm=True, act=1, wgs=0, seed=0, role_split=True):
    """The z-marching forward kernel (conv3d_zmarch.hip, round 5) against the lean kernel it replaces on the same operands: the output, the
    statistics partial sums and the fused pool's tensor + sums must be BIT-IDENTICAL (same MFMAs in the same order, same reduction order) - so
    the lean kernel's own parity rows carry over and the choice between the two may depend on the batch size.  wgs: cap on the z-march
    workgroups, so that a run covers many z-steps and crosses columns on a small volume.  planar: x (and a 16+-channel shortcut operand) as
    chunk-planar buffers, as the decoder's concat tensors are.  role_split=False: mode bit 2, i.e. conv3_zm_kernel also where the role-split
    form (conv3_zs_kernel: 16 input channels, no wide shortcut) is the default."""
    dt = L.F16 if f16 else L.BF16
    T = tdtype(dt)
    D, H, W = S
    g = torch.Generator().manual_seed(seed)
    x = rnd(torch.randn(B, D, H, W, Cin, generator=g), dt)
    w = torch.randn(16, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    bias = (torch.randn(16, generator=g) * 0.1).to(DEV)
    rec = make_recs(B, Cin, seed + 1)[0].to(DEV) if norm else None
    wp = pack(w, L.PK_K3, Cin, 16, dt)
    xd = to_dev(x, dt)
    xin = L.Planar(B, S, Cin, T, DEV).copy_from_dense(xd) if planar else xd
    sct, wscp, bscd, keep = L.NULL_T, None, None, []
    if sc_C == 1:
        img = torch.randn(B, D, H, W, generator=g).to(DEV).contiguous(); wsc = torch.randn(16, generator=g).to(DEV); bscd = (torch.randn(16, generator=g) * 0.1).to(DEV)
        sct, wscp, keep = L.Tensor(img.data_ptr(), 1, 1), wsc.data_ptr(), [img, wsc]
    elif sc_C:
        scd = to_dev(rnd(torch.randn(B, D, H, W, sc_C, generator=g), dt), dt)
        scin = L.Planar(B, S, sc_C, T, DEV).copy_from_dense(scd) if planar else scd
        wk = pack(torch.randn(16, sc_C, 1, 1, 1, generator=g) / sc_C ** 0.5, L.PK_K1, sc_C, 16, dt); bscd = (torch.randn(16, generator=g) * 0.1).to(DEV)
        sct, wscp, keep = L.tview(scin), wk.data_ptr(), [scin, wk]
    tiles = lib.bpx_conv3d_stats_tiles(dt, B, D, H, W, 16)
    outs = []
    n_zm = []
    for mode in (0, (2 if role_split else 6) | (wgs << 8)):
        lib.bpx_debug_set_conv_zm(mode)
        n_zm.append(lib.bpx_debug_conv_zm_launches())
        try:
            y = torch.full((B, D, H, W, 16), 7.0, dtype=T, device=DEV)
            part = torch.zeros(B, tiles, 2, 16, device=DEV)
            if pool:
                Dp = D // pool
                pooled = torch.full((B, Dp, H // 2, W // 2, 16), 7.0, dtype=T, device=DEV)
                ppart = torch.zeros(B, tiles, 2, 16, device=DEV)
                L.check(lib.bpx_conv3d_fwd_pool(dt, B, D, H, W, L.tview(xin), L.ptr(rec), act if norm else 0, wp.data_ptr(), bias.data_ptr(), sct, wscp,
                                                L.ptr(bscd), L.tview(y), part.data_ptr(), pool, L.tview(pooled), ppart.data_ptr(), L.stream_ptr()))
                outs.append((y, part, pooled, ppart))
            else:
                L.check(lib.bpx_conv3d_fwd(dt, B, D, H, W, L.tview(xin), L.ptr(rec), act if norm else 0, wp.data_ptr(), bias.data_ptr(), sct, wscp, L.ptr(bscd),
                                           L.tview(y), part.data_ptr(), L.stream_ptr()))
                outs.append((y, part))
            torch.cuda.synchronize()
        finally:
            lib.bpx_debug_set_conv_zm(-1)
    tag = f"conv3d_zmarch[{'f16' if f16 else 'bf16'} B{B} {S} {Cin}->16 sc={sc_C} pool={pool} planar={int(planar)} norm={int(norm)} act={act} wgs={wgs} zs={int(role_split)}]"
    res = []
    for name, a, b in zip(("y", "stats", "pooled", "pool_stats"), outs[0], outs[1]):
        res.append(_res(f"{tag}.{name}_bits_equal_lean", float((a.contiguous().view(torch.uint8) != b.contiguous().view(torch.uint8)).sum()), 0))
    res.append(_res(tag + ".wrote_something", 0 if float((outs[1][0].float() != 7).float().mean()) > 0.99 else 1, 0))
    res.append(_res(tag + ".zmarch_kernel_ran_in_the_second_call_only", 0 if (n_zm[1] == n_zm[0] and lib.bpx_debug_conv_zm_launches() == n_zm[1] + 1) else 1, 0))
    return res


def check_conv3d_fwd_pool(B, S, Cin, Cout, sz, seed=0):
    """bpx_conv3d_fwd_pool (MaxPool3d fused into the lean kernel's epilogue) == bpx_conv3d_fwd followed by bpx_maxpool3d_fwd:
    the same bf16 output bits, the same pooled bits, the same statistics partial sums."""
    dt = L.BF16
    D, H, W = S
    g = torch.Generator().manual_seed(seed)
    x = rnd(torch.randn(B, D, H, W, Cin, generator=g), dt)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    bias = torch.randn(Cout, generator=g) * 0.1
    rec, _, _ = make_recs(B, Cin, seed + 1)
    xd, recd, bd = to_dev(x, dt), rec.to(DEV), bias.to(DEV)
    wp = pack(w, L.PK_K3, Cin, Cout, dt)
    tiles = lib.bpx_conv3d_stats_tiles(dt, B, D, H, W, Cout)
    tag = f"conv3d_fwd_pool[B{B} {S} {Cin}->{Cout} sz{sz}]"
    if not lib.bpx_conv3d_fwd_pool_supported(dt, B, D, H, W, Cin, Cout, Cout):
        return [_res(tag + ".supported", 1, 0)]
    outs = []
    for fused in (False, True):
        y = torch.zeros(B, D, H, W, Cout, dtype=torch.bfloat16, device=DEV)
        part = torch.zeros(B, tiles, 2, Cout, dtype=torch.float32, device=DEV)
        pooled = torch.zeros(B, D // sz, H // 2, W // 2, Cout, dtype=torch.bfloat16, device=DEV)
        if fused:
            ppart = torch.zeros(B, tiles, 2, Cout, dtype=torch.float32, device=DEV)
            L.check(lib.bpx_conv3d_fwd_pool(dt, B, D, H, W, L.tview(xd), recd.data_ptr(), 1, wp.data_ptr(), bd.data_ptr(), L.NULL_T, None, None,
                                            L.tview(y), part.data_ptr(), sz, L.tview(pooled), ppart.data_ptr(), L.stream_ptr()))
        else:
            L.check(lib.bpx_conv3d_fwd(dt, B, D, H, W, L.tview(xd), recd.data_ptr(), 1, wp.data_ptr(), bd.data_ptr(), L.NULL_T, None, None, L.tview(y),
                                       part.data_ptr(), L.stream_ptr()))
            pt = lib.bpx_maxpool3d_stats_tiles(dt, D, H, W, sz, Cout)
            ppart = torch.zeros(B, pt, 2, Cout, dtype=torch.float32, device=DEV)
            L.check(lib.bpx_maxpool3d_fwd(dt, B, D, H, W, sz, L.tview(y), L.tview(pooled), ppart.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
        outs.append((y, pooled, part.sum(1), ppart.sum(1)))
    (y0, p0, s0, q0), (y1, p1, s1, q1) = outs
    return [_res(tag + ".y_bits", int((y0.view(torch.int16) != y1.view(torch.int16)).sum().item()), 0),
            _res(tag + ".pooled_bits", int((p0.view(torch.int16) != p1.view(torch.int16)).sum().item()), 0),
            _res(tag + ".stats", relerr(s1, s0), 1e-5), _res(tag + ".pool_stats", relerr(q1, q0), 1e-5)]


def check_conv3d_dgrad(dt, B, S, Cin, Cout, seed=0, act=1):
    """g = conv_transpose(dy, W) * act'(scale*t+shift) and its two reductions."""
    D, H, W = S
    g = torch.Generator().manual_seed(seed)
    dy = rnd(torch.randn(B, D, H, W, Cout, generator=g), dt)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cout) ** 0.5
    t = rnd(torch.randn(B, D, H, W, Cin, generator=g), dt)
    rec, _, _ = make_recs(B, Cin, seed + 1)
    dA = F.conv_transpose3d(ncdhw(dy), rnd(w, dt), padding=1)
    u = t * rec[:, None, None, None, :, 2] + rec[:, None, None, None, :, 3]
    dact = _dact_ref(u, act)
    g_ref = ndhwc(dA) * dact
    xh = (t - rec[:, None, None, None, :, 0]) * rec[:, None, None, None, :, 1]
    gd = torch.empty(B, D, H, W, Cin, dtype=tdtype(dt), device=DEV)
    tiles = lib.bpx_conv3d_stats_tiles(dt, B, D, H, W, Cin)
    red = torch.zeros(B, tiles, 2, Cin, dtype=torch.float32, device=DEV)
    wp = pack(w, L.PK_K3_T, Cin, Cout, dt)
    dyd, td, recd = to_dev(dy, dt), to_dev(t, dt), rec.to(DEV)
    L.check(lib.bpx_conv3d_dgrad(dt, B, D, H, W, L.tview(dyd), wp.data_ptr(), L.tview(td), recd.data_ptr(), act, L.tview(gd), red.data_ptr(),
                                 L.stream_ptr()))
    torch.cuda.synchronize()
    tag = f"conv3d_dgrad[{'bf16' if dt == L.BF16 else 'f32'} B{B} {S} dy{Cout}->g{Cin}]"
    res = [_res(tag, relerr(gd, g_ref), tol_for(dt))]
    s = red.sum(1).cpu()
    s_ref = torch.stack([g_ref.sum((1, 2, 3)), (g_ref * xh).sum((1, 2, 3))], 1)
    res.append(_res(tag + ".reductions", relerr(s, s_ref), 1e-2 if dt == L.BF16 else 1e-4))
    # plain dgrad (no activation / statistics)
    g2 = torch.empty_like(gd)
    L.check(lib.bpx_conv3d_dgrad(dt, B, D, H, W, L.tview(dyd), wp.data_ptr(), L.NULL_T, None, 0, L.tview(g2), None, L.stream_ptr()))
    res.append(_res(tag + ".plain", relerr(g2, ndhwc(dA)), tol_for(dt)))
    return res


def check_conv3d_wgrad(dt, B, S, Cin, Cout, k=3, norm=True, use_tr=1, seed=0, act=1):
    D, H, W = S
    g = torch.Generator().manual_seed(seed)
    x = rnd(torch.randn(B, D, H, W, Cin, generator=g), dt)
    dy = rnd(torch.randn(B, D, H, W, Cout, generator=g), dt)
    rec = None
    a = x
    if norm:
        rec, _, _ = make_recs(B, Cin, seed + 1)
        a = rnd(_act_ref(x * rec[:, None, None, None, :, 2] + rec[:, None, None, None, :, 3], act), dt)
    an = ncdhw(a).requires_grad_(False)
    wz = torch.zeros(Cout, Cin, k, k, k, requires_grad=True)
    bz = torch.zeros(Cout, requires_grad=True)
    out = F.conv3d(an, wz, bz, padding=k // 2)
    out.backward(ncdhw(dy))
    dw = torch.zeros(Cout, Cin, k, k, k, dtype=torch.float32, device=DEV)
    db = torch.zeros(Cout, dtype=torch.float32, device=DEV)
    xd, dyd = to_dev(x, dt), to_dev(dy, dt)
    recd = rec.to(DEV) if rec is not None else None
    lib.bpx_debug_set_wgrad_tr(use_tr)
    ws = torch.empty(max(1, lib.bpx_conv3d_wgrad_workspace(B, D, H, W, Cin, Cout, k)), dtype=torch.uint8, device=DEV)
    dw.fill_(7.0)  # the kernel overwrites dW (no pre-zeroing contract)
    L.check(lib.bpx_conv3d_wgrad(dt, B, D, H, W, L.tview(xd), L.ptr(recd), act if norm else 0, L.tview(dyd), k, dw.data_ptr(), db.data_ptr(),
                                 ws.data_ptr(), ws.numel(), L.stream_ptr()))
    torch.cuda.synchronize()
    lib.bpx_debug_set_wgrad_tr(1)
    tag = f"conv3d_wgrad[{'bf16' if dt == L.BF16 else 'f32'} B{B} {S} {Cin}->{Cout} k{k} norm={int(norm)} tr={use_tr}]"
    return [_res(tag, relerr(dw, wz.grad), 2e-3 if dt == L.BF16 else 2e-5), _res(tag + ".bias", relerr(db, bz.grad), 2e-3 if dt == L.BF16 else 2e-5)]


def check_conv1x1(dt, B, vox, Cin, Cout, with_coef=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = rnd(torch.randn(B, vox, Cin, generator=g), dt)
    w = torch.randn(Cout, Cin, generator=g) / Cin ** 0.5           # y = x @ w.T ; dense mode packs W[co][ci]
    gg = rnd(torch.randn(B, vox, Cout, generator=g), dt)
    tt = rnd(torch.randn(B, vox, Cout, generator=g), dt)
    add = rnd(torch.randn(B, vox, Cout, generator=g), dt)
    coef = torch.randn(B, Cout, 4, generator=g)
    y_ref = x @ rnd(w, dt).t()
    if with_coef:
        y_ref = y_ref + coef[:, None, :, 0] * gg + coef[:, None, :, 1] * tt + coef[:, None, :, 2] + add
    wp = pack(w.view(Cout, Cin, 1, 1, 1), L.PK_DENSE, Cin, Cout, dt)
    y = torch.empty(B, vox, Cout, dtype=tdtype(dt), device=DEV)
    xd, gd, td, ad, cd = to_dev(x, dt), to_dev(gg, dt), to_dev(tt, dt), to_dev(add, dt), coef.to(DEV)
    if with_coef:
        L.check(lib.bpx_conv1x1_fwd(dt, B, vox, L.tview(xd), wp.data_ptr(), None, L.tview(gd), L.tview(td), cd.data_ptr(), L.tview(ad), L.tview(y),
                                    L.stream_ptr()))
    else:
        L.check(lib.bpx_conv1x1_fwd(dt, B, vox, L.tview(xd), wp.data_ptr(), None, L.NULL_T, L.NULL_T, None, L.NULL_T, L.tview(y), L.stream_ptr()))
    torch.cuda.synchronize()
    tag = f"conv1x1[{'bf16' if dt == L.BF16 else 'f32'} B{B} v{vox} {Cin}->{Cout} coef={int(with_coef)}]"
    res = [_res(tag, relerr(y, y_ref), tol_for(dt))]
    # the transposed (dgrad) packing: dx = dy @ W
    wpt = pack(w.view(Cout, Cin, 1, 1, 1), L.PK_DENSE_T, Cin, Cout, dt)
    dy = rnd(torch.randn(B, vox, Cout, generator=g), dt)
    dx = torch.empty(B, vox, Cin, dtype=tdtype(dt), device=DEV)
    dyd = to_dev(dy, dt)
    L.check(lib.bpx_conv1x1_fwd(dt, B, vox, L.tview(dyd), wpt.data_ptr(), None, L.NULL_T, L.NULL_T, None, L.NULL_T, L.tview(dx), L.stream_ptr()))
    torch.cuda.synchronize()
    res.append(_res(tag + ".dgrad_pack", relerr(dx, dy @ rnd(w, dt)), tol_for(dt)))
    # split output: columns [0, 2/3 Cout) and the rest into two dense tensors must equal the one-tensor result bit for bit
    if with_coef and Cout % 48 == 0:
        lo = Cout * 2 // 3
        y_lo = torch.empty(B, vox, lo, dtype=tdtype(dt), device=DEV)
        y_hi = torch.empty(B, vox, Cout - lo, dtype=tdtype(dt), device=DEV)
        L.check(lib.bpx_conv1x1_fwd_split(dt, B, vox, L.tview(xd), wp.data_ptr(), None, L.tview(gd), L.tview(td), cd.data_ptr(), L.tview(ad),
                                          L.tview(y_lo), L.tview(y_hi), L.stream_ptr()))
        torch.cuda.synchronize()
        same = torch.equal(torch.cat([y_lo, y_hi], -1).view(torch.int16 if dt == L.BF16 else torch.int32), y.view(torch.int16 if dt == L.BF16 else torch.int32))
        res.append(_res(tag + ".split_identical", 0 if same else 1, 0))
    return res


def check_convT(dt, B, S, Cc, seed=0, sz=2, Cout=None):
    """ConvTranspose3d k = s = (sz,2,2) forward / dgrad / wgrad (sz = 1: the anisotropic Z_DOWN = 1 level); Cout != Cin is the
    plain U-Net's UpBlock (blocks.py:603)."""
    D, H, W = S
    g = torch.Generator().manual_seed(seed)
    Cin, Cc = Cc, (Cout or Cc)
    x = rnd(torch.randn(B, D, H, W, Cin, generator=g), dt)
    w = torch.randn(Cin, Cc, sz, 2, 2, generator=g) / Cin ** 0.5
    b = torch.randn(Cc, generator=g) * 0.1
    xr = ncdhw(x).requires_grad_(True)
    wr = rnd(w, dt).requires_grad_(True)
    br = b.clone().requires_grad_(True)
    y_ref = F.conv_transpose3d(xr, wr, br, stride=(sz, 2, 2))
    dy = rnd(torch.randn(B, sz * D, 2 * H, 2 * W, Cc, generator=g), dt)
    y_ref.backward(ncdhw(dy))
    tag = f"convT[{'bf16' if dt == L.BF16 else 'f32'} B{B} {S} C{Cin}->{Cc} sz{sz}]"
    # forward into a channel slice of a concat buffer
    extra = 16
    yb = torch.full((B, sz * D, 2 * H, 2 * W, Cc + extra), 3.0, dtype=tdtype(dt), device=DEV)
    wp = pack(w, L.PK_CT if sz == 2 else L.PK_CT4, Cin, Cc, dt)
    tiles = lib.bpx_convT3d_stats_tiles(D, H, W, sz)
    part = torch.zeros(B, tiles, 2, Cc, dtype=torch.float32, device=DEV)
    xd, bd = to_dev(x, dt), b.to(DEV)
    L.check(lib.bpx_convT3d_k2s2_fwd(dt, B, D, H, W, sz, L.tview(xd), wp.data_ptr(), bd.data_ptr(), L.tview(yb, 0, Cc), part.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    y = ndhwc(y_ref.detach())
    res = [_res(tag + ".fwd", relerr(yb[..., :Cc], y), tol_for(dt))]
    res.append(_res(tag + ".fwd.neighbours_untouched", 0 if (yb[..., Cc:].float() == 3).all().item() else 1, 0))
    s_ref = torch.stack([y.sum((1, 2, 3)), (y * y).sum((1, 2, 3))], 1)
    res.append(_res(tag + ".stats", relerr(part.sum(1), s_ref), 5e-3 if dt == L.BF16 else 1e-4))
    # dgrad
    wpt = pack(w, L.PK_CT_T if sz == 2 else L.PK_CT4_T, Cin, Cc, dt)
    dyd = to_dev(dy, dt)
    dx = torch.empty(B, D, H, W, Cin, dtype=tdtype(dt), device=DEV)
    L.check(lib.bpx_convT3d_k2s2_dgrad(dt, B, D, H, W, sz, L.tview(dyd), wpt.data_ptr(), L.tview(dx), L.stream_ptr()))
    torch.cuda.synchronize()
    res.append(_res(tag + ".dgrad", relerr(dx, ndhwc(xr.grad)), tol_for(dt)))
    # wgrad
    dw = torch.zeros(Cin, Cc, sz, 2, 2, dtype=torch.float32, device=DEV)
    db = torch.zeros(Cc, dtype=torch.float32, device=DEV)
    ws = torch.empty(max(1, lib.bpx_convT3d_k2s2_wgrad_workspace(B, D, H, W, sz, Cin, Cc)), dtype=torch.uint8, device=DEV)
    L.check(lib.bpx_convT3d_k2s2_wgrad(dt, B, D, H, W, sz, L.tview(xd), L.tview(dyd), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(),
                                       L.stream_ptr()))
    torch.cuda.synchronize()
    res.append(_res(tag + ".wgrad", relerr(dw, wr.grad), 2e-3 if dt == L.BF16 else 2e-5))
    res.append(_res(tag + ".bgrad", relerr(db, br.grad), 2e-3 if dt == L.BF16 else 2e-5))
    return res


def check_c1_fwd_buffer_vs_pointer(dt, B, S, Cout=16, ld_extra=0, persist=2048, seed=0):
    """Round 5: the first layer's buffer-addressed instance (out-of-range offsets for the zero padding, for tiles beyond the launch and for output
    voxels outside the volume) against the pointer-addressed one (hook bit 30): output (with its neighbours in a wider buffer), statistics rows -
    BIT-IDENTICAL; and against torch.  persist: workgroup cap, so that a run covers several tiles per workgroup on a small volume."""
    D, H, W = S
    T = tdtype(dt)
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, D, H, W, generator=g)
    w1 = torch.randn(Cout, 1, 3, 3, 3, generator=g) * 0.2
    b1 = torch.randn(Cout, generator=g) * 0.1
    y_ref = ndhwc(F.conv3d(img[:, None], rnd(w1, dt), b1, padding=1))
    imgd, w1_d, b1_d = img.to(DEV).contiguous(), w1.to(DEV), b1.to(DEV)
    tiles = lib.bpx_conv3d_c1_stats_tiles(D, H, W)
    outs = []
    for flag in (1 << 30, 0):
        lib.bpx_debug_set_c1_persist(persist | flag)
        try:
            yb = torch.full((B, D, H, W, Cout + ld_extra), 3.0, dtype=T, device=DEV)
            part = torch.zeros(B, tiles, 2, Cout, dtype=torch.float32, device=DEV)
            L.check(lib.bpx_conv3d_c1_fwd(dt, B, D, H, W, imgd.data_ptr(), w1_d.data_ptr(), b1_d.data_ptr(), L.tview(yb, 0, Cout), part.data_ptr(), L.stream_ptr()))
            torch.cuda.synchronize()
            outs.append((yb, part))
        finally:
            lib.bpx_debug_set_c1_persist(2048)
    tag = f"c1_fwd_buffer[{ {L.F16: 'f16', L.BF16: 'bf16'}.get(dt, 'f32') } B{B} {S} C{Cout}+{ld_extra} wgs{persist}]"
    res = [_res(tag + ".y_bits_equal_pointer_instance", float((outs[0][0].view(torch.uint8) != outs[1][0].view(torch.uint8)).sum()), 0),
           _res(tag + ".stats_bits_equal_pointer_instance", float((outs[0][1].view(torch.uint8) != outs[1][1].view(torch.uint8)).sum()), 0),
           _res(tag + ".fwd_vs_torch", relerr(outs[1][0][..., :Cout], y_ref), 4e-3 if dt != L.F32 else 1e-5)]
    if ld_extra:
        res.append(_res(tag + ".neighbours_untouched", 0 if (outs[1][0][..., Cout:].float() == 3).all().item() else 1, 0))
    return res


def check_convT_planar_k1(dt, B, S, Cin, Cout, sz=2, seed=0):
    """Round 5: the transposed-conv forward with ONE K step (Cin <= 32) into channels [0, Cout) of a chunk-planar concat buffer - the branch-free
    buffer-addressed kernel (convt_k1_kernel: scalar run coordinates, out-of-range offsets instead of predicates) against the general kernel on
    the same operands: output planes, the untouched skip plane and the statistics rows BIT-IDENTICAL; and against torch."""
    D, H, W = S
    T = tdtype(dt)
    g = torch.Generator().manual_seed(seed)
    x = rnd(torch.randn(B, D, H, W, Cin, generator=g), dt)
    w = torch.randn(Cin, Cout, sz, 2, 2, generator=g) / Cin ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    y_ref = ndhwc(F.conv_transpose3d(ncdhw(x), rnd(w, dt), b, stride=(sz, 2, 2)))
    wp = pack(w, L.PK_CT if sz == 2 else L.PK_CT4, Cin, Cout, dt)
    xd, bd = to_dev(x, dt), b.to(DEV)
    S2 = (sz * D, 2 * H, 2 * W)
    tiles = lib.bpx_convT3d_stats_tiles(D, H, W, sz)
    outs = []
    for k1 in (0, 1):
        lib.bpx_debug_set_convt_k1(k1)
        try:
            cat = L.Planar(B, S2, Cout + 16, T, DEV)
            cat.t.fill_(3.0)
            part = torch.zeros(B, tiles, 2, Cout, dtype=torch.float32, device=DEV)
            L.check(lib.bpx_convT3d_k2s2_fwd(dt, B, D, H, W, sz, L.tview(xd), wp.data_ptr(), bd.data_ptr(), L.tview(cat, 0, Cout), part.data_ptr(), L.stream_ptr()))
            torch.cuda.synchronize()
            outs.append((cat.dense(), part))
        finally:
            lib.bpx_debug_set_convt_k1(-1)
    tag = f"convT_planar_k1[{'f16' if dt == L.F16 else 'bf16'} B{B} {S} C{Cin}->{Cout} sz{sz}]"
    res = [_res(tag + ".y_bits_equal_general_kernel", float((outs[0][0].view(torch.uint8) != outs[1][0].view(torch.uint8)).sum()), 0),
           _res(tag + ".stats_bits_equal_general_kernel", float((outs[0][1].view(torch.uint8) != outs[1][1].view(torch.uint8)).sum()), 0),
           _res(tag + ".fwd_vs_torch", relerr(outs[1][0][..., :Cout], y_ref), tol_for(dt)),
           _res(tag + ".skip_plane_untouched", 0 if (outs[1][0][..., Cout:].float() == 3).all().item() else 1, 0)]
    s_ref = torch.stack([y_ref.sum((1, 2, 3)), (y_ref * y_ref).sum((1, 2, 3))], 1)
    res.append(_res(tag + ".stats_vs_torch", relerr(outs[1][1].sum(1), s_ref), 5e-3))
    return res


def check_norm_pool_head(dt, seed=0):
    res = []
    g = torch.Generator().manual_seed(seed)
    B, D, H, W, Cc = 2, 8, 12, 16, 32
    tagd = "bf16" if dt == L.BF16 else "f32"
    x = rnd(torch.randn(B, D, H, W, Cc, generator=g) * 2 + 0.5, dt)
    xd = to_dev(x, dt)
    # tensor_stats + finalize == instance norm statistics
    vox = D * H * W
    tiles = lib.bpx_tensor_stats_tiles(vox)
    part = torch.zeros(B, tiles, 2, Cc, dtype=torch.float32, device=DEV)
    L.check(lib.bpx_tensor_stats(dt, B, vox, L.tview(xd), part.data_ptr(), L.stream_ptr()))
    gamma = (1 + 0.1 * torch.randn(Cc, generator=g)); beta = 0.1 * torch.randn(Cc, generator=g)
    gamma_d, beta_d = gamma.to(DEV), beta.to(DEV)   # NB: never pass `.to(DEV).data_ptr()` of a temporary - it is freed at once
    rec = torch.zeros(B, Cc, 4, dtype=torch.float32, device=DEV)
    L.check(lib.bpx_norm_finalize(part.data_ptr(), B, tiles, Cc, vox, gamma_d.data_ptr(), beta_d.data_ptr(), 1e-5, Cc, rec.data_ptr(), Cc, 0,
                                  L.stream_ptr()))
    torch.cuda.synchronize()
    xf = x.reshape(B, vox, Cc)
    mean = xf.mean(1); var = xf.var(1, unbiased=False); rstd = (var + 1e-5).rsqrt()
    ref = torch.stack([mean, rstd, gamma[None] * rstd, beta[None] - mean * gamma[None] * rstd], -1)
    res.append(_res(f"norm_finalize[{tagd}]", relerr(rec, ref), 1e-5))
    # the partial sums themselves for channel slices: 24 channels (3 vectors: 85 voxel slots), a 16-channel slice at offset 8 of the
    # 32-channel rows (ld != C), and 5 channels (one-channel-per-lane fallback); a ragged last tile (vox = 1536 + 40)
    xs = rnd(torch.randn(B, 1576, Cc, generator=g), dt)
    xsd = to_dev(xs, dt)
    for c0, cn in ((0, 24), (8, 16), (3, 5), (0, 32)):
        tl = lib.bpx_tensor_stats_tiles(1576)
        pp = torch.zeros(B, tl, 2, cn, dtype=torch.float32, device=DEV)
        L.check(lib.bpx_tensor_stats(dt, B, 1576, L.tview(xsd, c0, cn), pp.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
        sl = xs[..., c0:c0 + cn].double()
        want = torch.stack([sl.sum(1), (sl * sl).sum(1)], 1)                     # (B, 2, cn)
        res.append(_res(f"tensor_stats[{tagd}].c{c0}+{cn}", relerr(pp.double().sum(1).cpu(), want), 1e-5))
    # max pool (sz,2,2) fwd + stats, bwd with addend (ties are likely in bf16: the first maximum must win as in PyTorch)
    for sz in (2, 1):
        y = torch.empty(B, D // sz, H // 2, W // 2, Cc, dtype=tdtype(dt), device=DEV)
        pt = lib.bpx_maxpool3d_stats_tiles(dt, D, H, W, sz, Cc)
        ppart = torch.zeros(B, pt, 2, Cc, dtype=torch.float32, device=DEV)
        L.check(lib.bpx_maxpool3d_fwd(dt, B, D, H, W, sz, L.tview(xd), L.tview(y), ppart.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
        xr = ncdhw(x).requires_grad_(True)
        y_ref = F.max_pool3d(xr, (sz, 2, 2))
        res.append(_res(f"maxpool_fwd[{tagd} sz{sz}]", relerr(y, ndhwc(y_ref.detach())), 0.0))
        yr = ndhwc(y_ref.detach())
        res.append(_res(f"maxpool_stats[{tagd} sz{sz}]", relerr(ppart.sum(1), torch.stack([yr.sum((1, 2, 3)), (yr * yr).sum((1, 2, 3))], 1)), 1e-4))
        dy = rnd(torch.randn(B, D // sz, H // 2, W // 2, Cc, generator=g), dt)
        add = rnd(torch.randn(B, D, H, W, Cc, generator=g), dt)
        y_ref.backward(ncdhw(dy))
        dx = torch.empty(B, D, H, W, Cc, dtype=tdtype(dt), device=DEV)
        dy_d, add_d = to_dev(dy, dt), to_dev(add, dt)
        L.check(lib.bpx_maxpool3d_bwd(dt, B, D, H, W, sz, L.tview(xd), L.tview(dy_d), L.tview(add_d), L.tview(dx), L.stream_ptr()))
        torch.cuda.synchronize()
        res.append(_res(f"maxpool_bwd[{tagd} sz{sz}]", relerr(dx, rnd(ndhwc(xr.grad) + add, dt)), 1e-6))
    # norm backward: finalize + apply == autograd of instance norm
    t = x
    tn = ncdhw(t).requires_grad_(True)
    gm = gamma.clone().requires_grad_(True); bt = beta.clone().requires_grad_(True)
    out = F.instance_norm(tn, None, None, gm, bt, True, 0.1, 1e-5)
    gsig = rnd(torch.randn(B, D, H, W, Cc, generator=g), dt)      # g = dL/d(norm output)
    out.backward(ncdhw(gsig))
    xh = (t - ref[:, None, None, None, :, 0]) * ref[:, None, None, None, :, 1]
    red = torch.stack([gsig.sum((1, 2, 3)), (gsig * xh).sum((1, 2, 3))], 1).view(B, 1, 2, Cc).contiguous().to(DEV)
    coef = torch.zeros(B, Cc, 4, dtype=torch.float32, device=DEV)
    dgm = torch.zeros(Cc, dtype=torch.float32, device=DEV); dbt = torch.zeros(Cc, dtype=torch.float32, device=DEV)
    L.check(lib.bpx_norm_bwd_finalize(red.data_ptr(), B, 1, Cc, vox, rec.data_ptr(), gamma_d.data_ptr(), dgm.data_ptr(), dbt.data_ptr(), Cc,
                                      coef.data_ptr(), L.stream_ptr()))
    dxn = torch.empty(B, D, H, W, Cc, dtype=tdtype(dt), device=DEV)
    gsig_d = to_dev(gsig, dt)
    L.check(lib.bpx_norm_bwd_apply(dt, B, vox, L.tview(gsig_d), L.tview(xd), coef.data_ptr(), L.NULL_T, L.tview(dxn), L.stream_ptr()))
    torch.cuda.synchronize()
    res.append(_res(f"norm_bwd_dx[{tagd}]", relerr(dxn, ndhwc(tn.grad)), 2e-2 if dt == L.BF16 else 1e-4))
    res.append(_res(f"norm_bwd_dgamma[{tagd}]", relerr(dgm, gm.grad), 1e-4))
    res.append(_res(f"norm_bwd_dbeta[{tagd}]", relerr(dbt, bt.grad), 1e-4))
    # head fwd/bwd
    Cf, Co = 16, 2
    f = rnd(torch.randn(B, D, H, W, Cf, generator=g), dt)
    hw = torch.randn(Co, Cf, generator=g) * 0.3; hb = torch.randn(Co, generator=g) * 0.1
    fr = ncdhw(f).requires_grad_(True); hwr = hw.clone().requires_grad_(True); hbr = hb.clone().requires_grad_(True)
    lo_ref = F.conv3d(fr, hwr.view(Co, Cf, 1, 1, 1), hbr)
    fd = to_dev(f, dt)
    hw_d, hb_d = hw.to(DEV), hb.to(DEV)
    lo = torch.empty(B, Co, D, H, W, dtype=torch.float32, device=DEV)
    L.check(lib.bpx_head_fwd(dt, vox, B, L.tview(fd), hw_d.data_ptr(), hb_d.data_ptr(), Co, 0, lo.data_ptr(), Co * vox, vox, L.stream_ptr()))
    pr = torch.empty_like(lo)
    L.check(lib.bpx_head_fwd(dt, vox, B, L.tview(fd), hw_d.data_ptr(), hb_d.data_ptr(), Co, 0x11, pr.data_ptr(), Co * vox, vox, L.stream_ptr()))
    torch.cuda.synchronize()
    res.append(_res(f"head_fwd[{tagd}]", relerr(lo, lo_ref.detach()), 1e-5))
    res.append(_res(f"head_fwd_sigmoid[{tagd}]", relerr(pr, torch.sigmoid(lo_ref.detach())), 1e-5))
    # per-channel activation codes of apply_model_activations (base_workflow.py:1403-1457): 4 channels =
    # [sigmoid, softmax, softmax, tanh] -> the two softmax channels form one group
    hw4 = torch.randn(4, Cf, generator=g) * 0.3; hb4 = torch.randn(4, generator=g) * 0.1
    lo4 = F.conv3d(ncdhw(f), hw4.view(4, Cf, 1, 1, 1), hb4)
    ref4 = torch.cat([torch.sigmoid(lo4[:, 0:1]), torch.softmax(lo4[:, 1:3], dim=1), torch.tanh(lo4[:, 3:4])], 1)
    hw4d, hb4d = hw4.to(DEV), hb4.to(DEV)
    pr4 = torch.empty(B, 4, D, H, W, dtype=torch.float32, device=DEV)
    L.check(lib.bpx_head_fwd(dt, vox, B, L.tview(fd), hw4d.data_ptr(), hb4d.data_ptr(), 4, 0x2331, pr4.data_ptr(), 4 * vox, vox, L.stream_ptr()))
    torch.cuda.synchronize()
    res.append(_res(f"head_fwd_mixed_acts[{tagd}]", relerr(pr4, ref4), 1e-5))
    dlo = torch.randn(B, Co, D, H, W, generator=g)
    lo_ref.backward(dlo)
    dfe = torch.empty(B, D, H, W, Cf, dtype=tdtype(dt), device=DEV)
    dhw = torch.zeros(Co, Cf, dtype=torch.float32, device=DEV); dhb = torch.zeros(Co, dtype=torch.float32, device=DEV)
    dlo_d = dlo.to(DEV).contiguous()
    hws = torch.empty(lib.bpx_head_bwd_workspace(Cf, Co), dtype=torch.uint8, device=DEV)
    L.check(lib.bpx_head_bwd(dt, vox, B, L.tview(fd), hw_d.data_ptr(), Co, dlo_d.data_ptr(), Co * vox, vox, L.tview(dfe), dhw.data_ptr(),
                             dhb.data_ptr(), hws.data_ptr(), hws.numel(), L.stream_ptr()))
    torch.cuda.synchronize()
    res.append(_res(f"head_bwd_dx[{tagd}]", relerr(dfe, ndhwc(fr.grad)), tol_for(dt)))
    res.append(_res(f"head_bwd_dw[{tagd}]", relerr(dhw, hwr.grad), 1e-4))
    res.append(_res(f"head_bwd_db[{tagd}]", relerr(dhb, hbr.grad), 1e-4))
    # Cin = 1 first layer
    img = torch.randn(B, D, H, W, generator=g)
    w1 = torch.randn(16, 1, 3, 3, 3, generator=g) * 0.2; b1 = torch.randn(16, generator=g) * 0.1
    w1r = rnd(w1, dt).requires_grad_(True); b1r = b1.clone().requires_grad_(True)   # bf16 mode rounds weights like every layer
    y1_ref = F.conv3d(img[:, None], w1r, b1r, padding=1)
    y1 = torch.empty(B, D, H, W, 16, dtype=tdtype(dt), device=DEV)
    t1 = lib.bpx_conv3d_c1_stats_tiles(D, H, W)
    p1 = torch.zeros(B, t1, 2, 16, dtype=torch.float32, device=DEV)
    imgd = img.to(DEV).contiguous()
    w1_d, b1_d = w1.to(DEV), b1.to(DEV)
    L.check(lib.bpx_conv3d_c1_fwd(dt, B, D, H, W, imgd.data_ptr(), w1_d.data_ptr(), b1_d.data_ptr(), L.tview(y1), p1.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    yr1 = ndhwc(y1_ref.detach())
    res.append(_res(f"conv_c1_fwd[{tagd}]", relerr(y1, yr1), 4e-3 if dt == L.BF16 else 1e-5))
    res.append(_res(f"conv_c1_stats[{tagd}]", relerr(p1.sum(1), torch.stack([yr1.sum((1, 2, 3)), (yr1 * yr1).sum((1, 2, 3))], 1)), 1e-4))
    dy1 = rnd(torch.randn(B, D, H, W, 16, generator=g), dt)
    y1_ref.backward(ncdhw(dy1))
    dw1 = torch.zeros(16, 1, 3, 3, 3, dtype=torch.float32, device=DEV); db1 = torch.zeros(16, dtype=torch.float32, device=DEV)
    dy1_d = to_dev(dy1, dt)
    wsc = torch.empty(lib.bpx_conv3d_c1_wgrad_workspace(16), dtype=torch.uint8, device=DEV)
    L.check(lib.bpx_conv3d_c1_wgrad(dt, B, D, H, W, imgd.data_ptr(), L.tview(dy1_d), dw1.data_ptr(), db1.data_ptr(), wsc.data_ptr(), wsc.numel(),
                                    L.stream_ptr()))
    torch.cuda.synchronize()
    res.append(_res(f"conv_c1_wgrad[{tagd}]", relerr(dw1, w1r.grad), 1e-4))
    res.append(_res(f"conv_c1_bgrad[{tagd}]", relerr(db1, b1r.grad), 1e-4))
    # rank-1 shortcut of the first block: dW[co] = sum_v img[v] * dy[v][co]
    dws = torch.full((16,), 7.0, dtype=torch.float32, device=DEV)                 # overwritten, not accumulated
    ws1 = torch.empty(lib.bpx_conv1x1_c1_wgrad_workspace(16), dtype=torch.uint8, device=DEV)
    L.check(lib.bpx_conv1x1_c1_wgrad(dt, B * D * H * W, imgd.data_ptr(), L.tview(dy1_d), dws.data_ptr(), ws1.data_ptr(), ws1.numel(), L.stream_ptr()))
    torch.cuda.synchronize()
    res.append(_res(f"conv1x1_c1_wgrad[{tagd}]", relerr(dws, (img[..., None].double() * dy1.double()).sum((0, 1, 2, 3))), 1e-4))
    return res


def check_mix16_kernels(S=(8, 16, 32), B=2, Cin=32, Cout=16, seed=0):
    """BPX_MIX16 - the backward entry points of the mixed 16-bit training mode: ACTIVATION operands (t / x: what the fp16 forward pass
    stored) are fp16, GRADIENT operands (dy, g, dx, addend) and the MFMA operands bf16.  Each entry against the fp32 PyTorch operator on
    the same (rounded) inputs: conv dgrad (+ ELU', reductions), conv wgrad k = 3 / k = 1 with and without the fused normalisation, the
    shortcut-dgrad GEMM with the InstanceNorm-backward affine, norm_bwd_apply, pooling backward, transposed-conv wgrad, head backward."""
    D, H, W = S
    vox = D * H * W
    g = torch.Generator().manual_seed(seed)
    A, G_ = L.F16, L.BF16                      # activation / gradient storage
    st = L.stream_ptr()
    tag = f"mix16[B{B} {S} {Cin}->{Cout}]"
    res = []
    rec_t, _, _ = make_recs(B, Cin, seed + 1)
    # ---- dgrad: g = convT(dy, W) * ELU'(scale t + shift) ------------------------------------------------------------------
    dy = rnd(torch.randn(B, D, H, W, Cout, generator=g), G_)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cout) ** 0.5
    t = rnd(torch.randn(B, D, H, W, Cin, generator=g), A)
    dA = ndhwc(F.conv_transpose3d(ncdhw(dy), rnd(w, G_), padding=1))
    u = t * rec_t[:, None, None, None, :, 2] + rec_t[:, None, None, None, :, 3]
    g_ref = dA * torch.where(u > 0, torch.ones_like(u), torch.exp(u))
    xh = (t - rec_t[:, None, None, None, :, 0]) * rec_t[:, None, None, None, :, 1]
    gd = torch.empty(B, D, H, W, Cin, dtype=torch.bfloat16, device=DEV)
    tiles = lib.bpx_conv3d_stats_tiles(G_, B, D, H, W, Cin)
    red = torch.zeros(B, tiles, 2, Cin, dtype=torch.float32, device=DEV)
    wpt = pack(w, L.PK_K3_T, Cin, Cout, L.MIX16)
    dyd, td, recd = to_dev(dy, G_), to_dev(t, A), rec_t.to(DEV)
    L.check(lib.bpx_conv3d_dgrad(L.MIX16, B, D, H, W, L.tview(dyd), wpt.data_ptr(), L.tview(td), recd.data_ptr(), 1, L.tview(gd), red.data_ptr(), st))
    torch.cuda.synchronize()
    res.append(_res(tag + ".dgrad", relerr(gd, g_ref), tol_for(G_)))
    res.append(_res(tag + ".dgrad.reductions", relerr(red.sum(1).cpu(), torch.stack([g_ref.sum((1, 2, 3)), (g_ref * xh).sum((1, 2, 3))], 1)), 1e-2))
    # the transposed pack of MIX16 is the bf16 pack, bit for bit; the forward pack the fp16 one
    same_t = torch.equal(wpt.view(torch.int16), pack(w, L.PK_K3_T, Cin, Cout, L.BF16).view(torch.int16))
    same_f = torch.equal(pack(w, L.PK_K3, Cin, Cout, L.MIX16).view(torch.int16), pack(w, L.PK_K3, Cin, Cout, L.F16).view(torch.int16))
    res.append(_res(tag + ".pack_types", 0 if (same_t and same_f) else 1, 0))
    # ---- wgrad, k = 3 with the fused normalise + ELU prologue, k = 1 raw (the shortcut) -----------------------------------------
    for k, norm in ((3, True), (3, False), (1, False)):
        x = t
        a = _act_ref(x * rec_t[:, None, None, None, :, 2] + rec_t[:, None, None, None, :, 3], 1) if norm else x
        a = rnd(a, G_)                                                    # the MFMA operand is bf16
        wz = torch.zeros(Cout, Cin, k, k, k, requires_grad=True)
        bz = torch.zeros(Cout, requires_grad=True)
        F.conv3d(ncdhw(a), wz, bz, padding=k // 2).backward(ncdhw(dy))
        dw = torch.full((Cout, Cin, k, k, k), 7.0, dtype=torch.float32, device=DEV)
        db = torch.zeros(Cout, dtype=torch.float32, device=DEV)
        ws = torch.empty(max(1, lib.bpx_conv3d_wgrad_workspace(B, D, H, W, Cin, Cout, k)), dtype=torch.uint8, device=DEV)
        L.check(lib.bpx_conv3d_wgrad(L.MIX16, B, D, H, W, L.tview(td), recd.data_ptr() if norm else None, 1 if norm else 0, L.tview(dyd), k,
                                     dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), st))
        torch.cuda.synchronize()
        res.append(_res(tag + f".wgrad[k{k} norm={int(norm)}]", relerr(dw, wz.grad), 2e-3))
        res.append(_res(tag + f".wgrad[k{k} norm={int(norm)}].bias", relerr(db, bz.grad), 2e-3))
    # ---- shortcut dgrad GEMM + InstanceNorm-backward affine: dx = dOut W + a g + b t + c0 (t fp16, the rest bf16) -------------------
    dOut = dy.reshape(B, vox, Cout)
    wsc = torch.randn(Cout, Cin, generator=g) / Cout ** 0.5
    gg = rnd(torch.randn(B, vox, Cin, generator=g), G_)
    coef = torch.randn(B, Cin, 4, generator=g)
    tt = t.reshape(B, vox, Cin)
    y_ref = dOut @ rnd(wsc, G_) + coef[:, None, :, 0] * gg + coef[:, None, :, 1] * tt + coef[:, None, :, 2]
    wpd = pack(wsc.view(Cout, Cin, 1, 1, 1), L.PK_DENSE_T, Cin, Cout, L.MIX16)
    yd = torch.empty(B, vox, Cin, dtype=torch.bfloat16, device=DEV)
    ggd, cd = to_dev(gg, G_), coef.to(DEV)
    dOd = dyd.view(B, vox, Cout)
    ttd = td.view(B, vox, Cin)
    L.check(lib.bpx_conv1x1_fwd(L.MIX16, B, vox, L.tview(dOd), wpd.data_ptr(), None, L.tview(ggd), L.tview(ttd), cd.data_ptr(), L.NULL_T, L.tview(yd), st))
    torch.cuda.synchronize()
    res.append(_res(tag + ".conv1x1_affine", relerr(yd, y_ref), tol_for(G_)))
    if Cin % 48 == 0:
        lo = Cin * 2 // 3
        y_lo = torch.empty(B, vox, lo, dtype=torch.bfloat16, device=DEV)
        y_hi = torch.empty(B, vox, Cin - lo, dtype=torch.bfloat16, device=DEV)
        L.check(lib.bpx_conv1x1_fwd_split(L.MIX16, B, vox, L.tview(dOd), wpd.data_ptr(), None, L.tview(ggd), L.tview(ttd), cd.data_ptr(), L.NULL_T,
                                          L.tview(y_lo), L.tview(y_hi), st))
        torch.cuda.synchronize()
        res.append(_res(tag + ".conv1x1_affine.split_identical", 0 if torch.equal(torch.cat([y_lo, y_hi], -1).view(torch.int16), yd.view(torch.int16)) else 1, 0))
    # ---- norm_bwd_apply: dx = a g + b t + c0 --------------------------------------------------------------------------------------
    dxn = torch.empty(B, vox, Cin, dtype=torch.bfloat16, device=DEV)
    L.check(lib.bpx_norm_bwd_apply(L.MIX16, B, vox, L.tview(ggd), L.tview(ttd), cd.data_ptr(), L.NULL_T, L.tview(dxn), st))
    torch.cuda.synchronize()
    res.append(_res(tag + ".norm_bwd_apply", relerr(dxn, coef[:, None, :, 0] * gg + coef[:, None, :, 1] * tt + coef[:, None, :, 2]), tol_for(G_)))
    # ---- pooling backward: the arg-max comes from the fp16 input, the gradient is bf16 -----------------------------------------------
    for sz in (2, 1):
        xr = ncdhw(t).requires_grad_(True)
        y_ref = F.max_pool3d(xr, (sz, 2, 2))
        dyp = rnd(torch.randn(B, D // sz, H // 2, W // 2, Cin, generator=g), G_)
        add = rnd(torch.randn(B, D, H, W, Cin, generator=g), G_)
        y_ref.backward(ncdhw(dyp))
        dx = torch.empty(B, D, H, W, Cin, dtype=torch.bfloat16, device=DEV)
        dypd, addd = to_dev(dyp, G_), to_dev(add, G_)
        L.check(lib.bpx_maxpool3d_bwd(L.MIX16, B, D, H, W, sz, L.tview(td), L.tview(dypd), L.tview(addd), L.tview(dx), st))
        torch.cuda.synchronize()
        res.append(_res(tag + f".maxpool_bwd[sz{sz}]", relerr(dx, rnd(ndhwc(xr.grad) + add, G_)), 1e-6))
        need = int(lib.bpx_maxpool3d_bwd_r1_workspace(L.MIX16, B, D, H, W, sz, Cin))
        if need > 0:
            # round 6: the same pass with the rank-1 shortcut weight gradient riding along: dx keeps its bits; dWsc[co] = sum_v img[v] dx[v][co] over the STORED
            # values against the fp64 sum, against the kernel it replaces (bpx_conv1x1_c1_wgrad on dx), and run to run
            img = torch.randn(B, D, H, W, generator=g)
            imgd = img.to(DEV)

            def run_r1():
                dx2 = torch.empty(B, D, H, W, Cin, dtype=torch.bfloat16, device=DEV)
                dw = torch.full((Cin,), 7.0, dtype=torch.float32, device=DEV)
                wsr = torch.empty(need, dtype=torch.uint8, device=DEV)
                L.check(lib.bpx_maxpool3d_bwd_r1(L.MIX16, B, D, H, W, sz, L.tview(td), L.tview(dypd), L.tview(addd), L.tview(dx2), imgd.data_ptr(), dw.data_ptr(),
                                                 wsr.data_ptr(), wsr.numel(), st))
                torch.cuda.synchronize()
                return dx2, dw

            (dx2, dwa), (_, dwb) = run_r1(), run_r1()
            dwk = torch.full((Cin,), 7.0, dtype=torch.float32, device=DEV)
            wsk = torch.empty(lib.bpx_conv1x1_c1_wgrad_workspace(Cin), dtype=torch.uint8, device=DEV)
            L.check(lib.bpx_conv1x1_c1_wgrad(L.BF16, B * D * H * W, imgd.data_ptr(), L.tview(dx), dwk.data_ptr(), wsk.data_ptr(), wsk.numel(), st))
            torch.cuda.synchronize()
            ref = torch.einsum("bdhw,bdhwc->c", img.double(), dx.float().cpu().double())
            res.append(_res(tag + f".maxpool_bwd_r1[sz{sz}].same_dx_bits", 0 if torch.equal(dx2.view(torch.int16), dx.view(torch.int16)) else 1, 0))
            res.append(_res(tag + f".maxpool_bwd_r1[sz{sz}].dw_vs_fp64", relerr(dwa, ref), 1e-4))
            res.append(_res(tag + f".maxpool_bwd_r1[sz{sz}].dw_vs_rank1_kernel", relerr(dwa, dwk), 1e-4))
            res.append(_res(tag + f".maxpool_bwd_r1[sz{sz}].run_to_run_bits", 0 if torch.equal(dwa, dwb) else 1, 0))
    # ---- transposed-conv wgrad: x fp16 (raw), dy bf16 ---------------------------------------------------------------------------
    for sz in (2, 1):
        wt = torch.zeros(Cin, Cin, sz, 2, 2, requires_grad=True)
        bt = torch.zeros(Cin, requires_grad=True)
        dyt = rnd(torch.randn(B, sz * D, 2 * H, 2 * W, Cin, generator=g), G_)
        F.conv_transpose3d(ncdhw(rnd(t, G_)), wt, bt, stride=(sz, 2, 2)).backward(ncdhw(dyt))
        dw = torch.zeros(Cin, Cin, sz, 2, 2, dtype=torch.float32, device=DEV)
        db = torch.zeros(Cin, dtype=torch.float32, device=DEV)
        ws = torch.empty(max(1, lib.bpx_convT3d_k2s2_wgrad_workspace(B, D, H, W, sz, Cin, Cin)), dtype=torch.uint8, device=DEV)
        dytd = to_dev(dyt, G_)
        L.check(lib.bpx_convT3d_k2s2_wgrad(L.MIX16, B, D, H, W, sz, L.tview(td), L.tview(dytd), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), st))
        torch.cuda.synchronize()
        res.append(_res(tag + f".convT_wgrad[sz{sz}]", relerr(dw, wt.grad), 2e-3))
        res.append(_res(tag + f".convT_bgrad[sz{sz}]", relerr(db, bt.grad), 2e-3))
    # ---- head backward: features fp16, feature gradient bf16 ----------------------------------------------------------------------
    if Cin in (16, 32):
        Co = 2
        hw = torch.randn(Co, Cin, generator=g) * 0.3
        fr = ncdhw(t).requires_grad_(True); hwr = hw.clone().requires_grad_(True); hbr = torch.zeros(Co, requires_grad=True)
        lo_ref = F.conv3d(fr, hwr.view(Co, Cin, 1, 1, 1), hbr)
        dlo = torch.randn(B, Co, D, H, W, generator=g)
        lo_ref.backward(dlo)
        dfe = torch.empty(B, D, H, W, Cin, dtype=torch.bfloat16, device=DEV)
        dhw = torch.zeros(Co, Cin, dtype=torch.float32, device=DEV); dhb = torch.zeros(Co, dtype=torch.float32, device=DEV)
        dlo_d, hw_d = dlo.to(DEV).contiguous(), hw.to(DEV)
        hws = torch.empty(lib.bpx_head_bwd_workspace(Cin, Co), dtype=torch.uint8, device=DEV)
        L.check(lib.bpx_head_bwd(L.MIX16, vox, B, L.tview(td), hw_d.data_ptr(), Co, dlo_d.data_ptr(), Co * vox, vox, L.tview(dfe), dhw.data_ptr(),
                                 dhb.data_ptr(), hws.data_ptr(), hws.numel(), st))
        torch.cuda.synchronize()
        res.append(_res(tag + ".head_bwd_dx", relerr(dfe, ndhwc(fr.grad)), tol_for(G_)))
        res.append(_res(tag + ".head_bwd_dw", relerr(dhw, hwr.grad), 1e-4))
    return res


def check_bwd_fused(mix=True, B=2, S=(32, 32, 32), Ct=16, planar=False, seed=0, act=1, Cdy=16, rs=None):
    """bpx_conv3d_bwd_fused (dgrad + wgrad of one conv in one pass) against the two separate entry points on the same device operands
    (g bit for bit, statistics / dW / db to fp32 summation order) and against the fp32 PyTorch operators on the same rounded inputs."""
    D, H, W = S
    gen = torch.Generator().manual_seed(seed)
    A, G_ = (L.F16 if mix else L.BF16), L.BF16
    dtc = L.MIX16 if mix else L.BF16
    st = L.stream_ptr()
    tag = f"bwd_fused[{'mix16' if mix else 'bf16'} B{B} {S} dy{Cdy}->g{Ct}{' planar' if planar else ''} act{act}{'' if rs is None else f' rs{rs}'}]"
    res = []
    if rs is not None:      # role-split kernel mask (bpx_debug_set_bwd_rs): bit 0 = the 48-channel shape, bit 1 = the 16-channel shape
        lib.bpx_debug_set_bwd_rs(rs)
    try:
        return _check_bwd_fused(tag, res, mix, B, S, Ct, planar, seed, act, Cdy, dtc, A, G_, gen, st)
    finally:
        if rs is not None:
            lib.bpx_debug_set_bwd_rs(RS_DEFAULT)


RS_DEFAULT = int(os.environ.get("BPX_BWD_RS", "3"))


def _check_bwd_fused(tag, res, mix, B, S, Ct, planar, seed, act, Cdy, dtc, A, G_, gen, st):
    D, H, W = S
    if not lib.bpx_conv3d_bwd_fused_supported(dtc, B, D, H, W, Ct, Cdy):
        return [_res(tag + ".supported", 1, 0)]
    rec, _, _ = make_recs(B, Ct, seed + 1)
    dy = rnd(torch.randn(B, D, H, W, Cdy, generator=gen), G_)
    w = torch.randn(Cdy, Ct, 3, 3, 3, generator=gen) / (27 * Cdy) ** 0.5
    t = rnd(torch.randn(B, D, H, W, Ct, generator=gen), A)
    # fp32 references
    dA = ndhwc(F.conv_transpose3d(ncdhw(dy), rnd(w, G_), padding=1))
    u = t * rec[:, None, None, None, :, 2] + rec[:, None, None, None, :, 3]
    dact = _dact_ref(u, act)
    g_ref = dA * dact
    xh = (t - rec[:, None, None, None, :, 0]) * rec[:, None, None, None, :, 1]
    a = rnd(_act_ref(u, act), G_)
    wz = torch.zeros(Cdy, Ct, 3, 3, 3, requires_grad=True)
    bz = torch.zeros(Cdy, requires_grad=True)
    F.conv3d(ncdhw(a), wz, bz, padding=1).backward(ncdhw(dy))
    # device operands
    dyd, recd = to_dev(dy, G_), rec.to(DEV)
    if planar:
        tp = L.Planar(B, S, Ct, tdtype(A), DEV).copy_from_dense(to_dev(t, A))
        tv = L.tview(tp)
    else:
        td = to_dev(t, A)
        tv = L.tview(td)
    wpt = pack(w, L.PK_K3_T, Ct, Cdy, dtc)
    # separate kernels
    g_sep = torch.empty(B, D, H, W, Ct, dtype=torch.bfloat16, device=DEV)
    tiles = lib.bpx_conv3d_stats_tiles(G_, B, D, H, W, Ct)
    red_sep = torch.zeros(B, tiles, 2, Ct, dtype=torch.float32, device=DEV)
    L.check(lib.bpx_conv3d_dgrad(dtc, B, D, H, W, L.tview(dyd), wpt.data_ptr(), tv, recd.data_ptr(), act, L.tview(g_sep), red_sep.data_ptr(), st))
    dw_sep = torch.full((Cdy, Ct, 3, 3, 3), 7.0, dtype=torch.float32, device=DEV)
    db_sep = torch.zeros(Cdy, dtype=torch.float32, device=DEV)
    ws = torch.empty(max(1, lib.bpx_conv3d_wgrad_workspace(B, D, H, W, Ct, Cdy, 3)), dtype=torch.uint8, device=DEV)
    L.check(lib.bpx_conv3d_wgrad(dtc, B, D, H, W, tv, recd.data_ptr(), act, L.tview(dyd), 3, dw_sep.data_ptr(), db_sep.data_ptr(), ws.data_ptr(), ws.numel(), st))
    # fused
    g_f = torch.full((B, D, H, W, Ct), float("nan"), dtype=torch.bfloat16, device=DEV)
    ftiles = lib.bpx_conv3d_bwd_fused_stats_tiles(B, D, H, W, Ct, Cdy)
    red_f = torch.full((B, ftiles, 2, Ct), float("nan"), dtype=torch.float32, device=DEV)
    dw_f = torch.full((Cdy, Ct, 3, 3, 3), 7.0, dtype=torch.float32, device=DEV)
    db_f = torch.zeros(Cdy, dtype=torch.float32, device=DEV)
    db2_f = torch.zeros(Cdy, dtype=torch.float32, device=DEV)
    ws2 = torch.empty(max(1, lib.bpx_conv3d_bwd_fused_workspace(B, D, H, W, Ct, Cdy)), dtype=torch.uint8, device=DEV)
    L.check(lib.bpx_conv3d_bwd_fused(dtc, B, D, H, W, L.tview(dyd), wpt.data_ptr(), tv, recd.data_ptr(), act, L.tview(g_f), red_f.data_ptr(),
                                     dw_f.data_ptr(), db_f.data_ptr(), db2_f.data_ptr(), ws2.data_ptr(), ws2.numel(), st))
    torch.cuda.synchronize()
    res.append(_res(tag + ".g_bits_equal_separate", 0 if torch.equal(g_f.view(torch.int16), g_sep.view(torch.int16)) else 1, 0))
    res.append(_res(tag + ".g", relerr(g_f, g_ref), tol_for(G_)))
    s_ref = torch.stack([g_ref.sum((1, 2, 3)), (g_ref * xh).sum((1, 2, 3))], 1)
    res.append(_res(tag + ".reductions", relerr(red_f.sum(1).cpu(), s_ref), 1e-2))
    res.append(_res(tag + ".reductions_vs_separate", relerr(red_f.sum(1), red_sep.sum(1)), 1e-4))
    res.append(_res(tag + ".dw", relerr(dw_f, wz.grad), 2e-3))
    res.append(_res(tag + ".dw_vs_separate", relerr(dw_f, dw_sep), 1e-4))
    res.append(_res(tag + ".db", relerr(db_f, bz.grad), 2e-3))
    res.append(_res(tag + ".db2_equals_db", 0 if torch.equal(db_f, db2_f) else 1, 0))
    # a second run must reproduce every bit (fixed-order reductions, no atomics)
    g2 = torch.empty_like(g_f); red2 = torch.empty_like(red_f); dw2 = torch.empty_like(dw_f); db2 = torch.zeros_like(db_f)
    L.check(lib.bpx_conv3d_bwd_fused(dtc, B, D, H, W, L.tview(dyd), wpt.data_ptr(), tv, recd.data_ptr(), act, L.tview(g2), red2.data_ptr(),
                                     dw2.data_ptr(), db2.data_ptr(), None, ws2.data_ptr(), ws2.numel(), st))
    torch.cuda.synchronize()
    same = torch.equal(g2.view(torch.int16), g_f.view(torch.int16)) and torch.equal(red2, red_f) and torch.equal(dw2, dw_f) and torch.equal(db2, db_f)
    res.append(_res(tag + ".reproducible", 0 if same else 1, 0))
    return res


def check_f16_saturation(seed=0):
    """fp16 storage ends at 65504.  Raw conv / transposed-conv / first-layer outputs are stored through a SATURATING pack:
    an fp32 result beyond the range must land as +-65504 (finite), never as +-inf; the statistics partials still come from the unclamped
    fp32 values.  Forward conv (lean and double-buffered kernels), first layer, transposed conv with operands scaled far out of range; and a
    whole ResUNet forward in fp16 on an input of magnitude 3e4 must give finite logits."""
    res = []
    g = torch.Generator().manual_seed(seed)
    st = L.stream_ptr()
    F16 = L.F16
    for S, tagk in (((8, 8, 16), "double-buffered"), ((32, 32, 32), "lean")):
        B, Cin, Cout = 1, 16, 16
        D, H, W = S
        x = rnd(torch.randn(B, D, H, W, Cin, generator=g) * 900.0, F16)
        w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) * 4.0
        ref = ndhwc(F.conv3d(ncdhw(x), rnd(w, F16), padding=1))
        xd = to_dev(x, F16)
        yd = torch.empty(B, D, H, W, Cout, dtype=torch.float16, device=DEV)
        wp = pack(w, L.PK_K3, Cin, Cout, F16)
        bias = torch.zeros(Cout, device=DEV)
        tiles = lib.bpx_conv3d_stats_tiles(F16, B, D, H, W, Cout)
        part = torch.zeros(B, tiles, 2, Cout, device=DEV)
        L.check(lib.bpx_conv3d_fwd(F16, B, D, H, W, L.tview(xd), None, 0, wp.data_ptr(), bias.data_ptr(), L.NULL_T, None, None, L.tview(yd), part.data_ptr(), st))
        torch.cuda.synchronize()
        y = yd.float().cpu()
        over = ref.abs() > 65504
        tag = f"f16_saturation.conv3d_fwd[{tagk} {S}]"
        res.append(_res(tag + ".some_results_out_of_range", 0 if over.any() else 1, 0, extra=f"{int(over.sum())} of {over.numel()} beyond 65504, max |ref| {ref.abs().max().item():.3g}"))
        res.append(_res(tag + ".finite", 0 if torch.isfinite(y).all() else 1, 0))
        res.append(_res(tag + ".clamped_values", relerr(y, ref.clamp(-65504, 65504)), 2e-3))
        res.append(_res(tag + ".statistics_unclamped", relerr(part.sum(1)[:, 0].cpu(), ref.sum((1, 2, 3))), 2e-3))
    # the whole network in fp16 on an un-normalised input (raw 16-bit intensities): finite logits
    from biapy_amd.resunet import ResUNet
    torch.manual_seed(seed)
    m = ResUNet(image_shape=(32, 32, 32, 1), activation="elu", feature_maps=[16, 32], drop_values=[0.0, 0.0], normalization="in", yx_down=[2], z_down=[2],
                isotropy=[True, True], larger_io=False, conv_layers=[2, 2], compute_dtype=torch.float16).cuda().eval()
    with torch.no_grad():
        xin = (torch.randn(1, 1, 32, 32, 32, generator=g) * 3e4).cuda()
        lo = m(xin)
        m32 = m
        m32.compute_dtype = torch.float32
        lo32 = m32(xin)
    res.append(_res("f16_saturation.network_logits_finite[input magnitude 3e4]", 0 if torch.isfinite(lo).all() else 1, 0,
                    extra=f"max |logit| {lo.abs().max().item():.3g}; f32 mode {lo32.abs().max().item():.3g}"))
    return res


def check_planar_layouts(dt, S=(8, 16, 32), lean=False):
    """Chunk-planar operands (bpx_tensor.cs != 0, the layout of the decoder's concat buffers) against the ordinary interleaved layout:
    every entry point that accepts them must produce BIT-IDENTICAL results, the arithmetic does not change.  Covered: conv forward
    (x with the fused norm prologue, the fused 1x1x1 shortcut operand, the output), dgrad's t operand, wgrad's x operand for k = 3 and
    k = 1, the t operand of the fused shortcut-dgrad / norm-backward GEMM, the transposed conv's output, pooling forward / backward."""
    g = torch.Generator().manual_seed(11)
    T = tdtype(dt)
    tagd = ("bf16" if dt == L.BF16 else "f32") + ("-lean" if lean else "")
    st = L.stream_ptr()
    B = 1 if lean else 2
    D, H, W = S
    vox = D * H * W
    Cx, Cy = 48, 32                                         # Cy = 32: the output spans two planes
    res = []

    def dev_pair(shape_c):
        x = rnd(torch.randn(B, D, H, W, shape_c, generator=g), dt)
        xd = to_dev(x, dt)
        return xd, L.Planar(B, S, shape_c, T, DEV).copy_from_dense(xd)

    def same(name, a, b):
        a, b = (t.dense() if isinstance(t, L.Planar) else t for t in (a, b))
        res.append(_res(f"planar[{tagd}].{name}", float((a.contiguous().view(torch.uint8) != b.contiguous().view(torch.uint8)).sum()), 0))

    def pack(w, mode, cin, cout):
        out = torch.empty(lib.bpx_packed_weight_elems(mode, cin, cout, dt), dtype=T, device=DEV)
        L.check(lib.bpx_pack_weight(mode, w.data_ptr(), cin, cout, dt, out.data_ptr(), st))
        return out

    xd, xp = dev_pair(Cx)
    rec = torch.rand(B, Cx, 4, generator=g).to(DEV)
    w3 = (torch.randn(Cy, Cx, 3, 3, 3, generator=g) * 0.05).to(DEV)
    wk3, wk1 = pack(w3, L.PK_K3, Cx, Cy), pack((torch.randn(Cy, Cx, 1, 1, 1, generator=g) * 0.1).to(DEV), L.PK_K1, Cx, Cy)
    bias = torch.randn(Cy, generator=g).to(DEV)
    tiles = lib.bpx_conv3d_stats_tiles(dt, B, D, H, W, Cy)
    outs = []
    for xin, yout in ((xd, torch.empty(B, D, H, W, Cy, dtype=T, device=DEV)), (xp, L.Planar(B, S, Cy, T, DEV))):
        part = torch.zeros(B, tiles, 2, Cy, device=DEV)
        L.check(lib.bpx_conv3d_fwd(dt, B, D, H, W, L.tview(xin), rec.data_ptr(), L.ACT["elu"], wk3.data_ptr(), bias.data_ptr(), L.tview(xin), wk1.data_ptr(),
                                   bias.data_ptr(), L.tview(yout), part.data_ptr(), st))
        outs.append((yout, part))
    torch.cuda.synchronize()
    same("conv_fwd.y", outs[0][0], outs[1][0])
    same("conv_fwd.stats", outs[0][1], outs[1][1])
    # dgrad: dy (Cy) -> g (Cx), t = the conv input (planar) with its norm record
    dyd = to_dev(rnd(torch.randn(B, D, H, W, Cy, generator=g), dt), dt)
    wt = pack(w3, L.PK_K3_T, Cx, Cy)
    rt = lib.bpx_conv3d_stats_tiles(dt, B, D, H, W, Cx)
    outs = []
    for tin in (xd, xp):
        gq = torch.empty(B, D, H, W, Cx, dtype=T, device=DEV)
        red = torch.zeros(B, rt, 2, Cx, device=DEV)
        L.check(lib.bpx_conv3d_dgrad(dt, B, D, H, W, L.tview(dyd), wt.data_ptr(), L.tview(tin), rec.data_ptr(), L.ACT["elu"], L.tview(gq), red.data_ptr(), st))
        outs.append((gq, red))
    torch.cuda.synchronize()
    same("dgrad.g", outs[0][0], outs[1][0])
    same("dgrad.red", outs[0][1], outs[1][1])
    # wgrad k = 3 (with the prologue) and k = 1
    for k in (3, 1):
        outs = []
        for xin in (xd, xp):
            dw = torch.zeros(Cy, Cx, k, k, k, device=DEV)
            db = torch.zeros(Cy, device=DEV)
            ws = torch.empty(max(1, lib.bpx_conv3d_wgrad_workspace(B, D, H, W, Cx, Cy, k)), dtype=torch.uint8, device=DEV)
            L.check(lib.bpx_conv3d_wgrad(dt, B, D, H, W, L.tview(xin), rec.data_ptr() if k == 3 else None, L.ACT["elu"] if k == 3 else 0, L.tview(dyd), k,
                                         dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), st))
            outs.append((dw, db))
        torch.cuda.synchronize()
        same(f"wgrad_k{k}.dw", outs[0][0], outs[1][0])
        same(f"wgrad_k{k}.db", outs[0][1], outs[1][1])
    # shortcut dgrad fused with the norm-backward affine: y = dy * Wsc^T + a*g + b*t + c0, split into (32, 16) channels
    wsct = pack((torch.randn(Cy, Cx, 1, 1, 1, generator=g) * 0.1).to(DEV), L.PK_DENSE_T, Cx, Cy)
    coef = torch.randn(B, Cx, 4, generator=g).to(DEV)
    g0 = to_dev(rnd(torch.randn(B, D, H, W, Cx, generator=g), dt), dt)
    outs = []
    for tin in (xd, xp):
        lo = torch.empty(B, D, H, W, 32, dtype=T, device=DEV)
        hi = torch.empty(B, D, H, W, 16, dtype=T, device=DEV)
        L.check(lib.bpx_conv1x1_fwd_split(dt, B, vox, L.tview(dyd), wsct.data_ptr(), None, L.tview(g0), L.tview(tin), coef.data_ptr(), L.NULL_T,
                                          L.tview(lo), L.tview(hi), st))
        one = torch.empty(B, D, H, W, Cx, dtype=T, device=DEV)
        L.check(lib.bpx_conv1x1_fwd(dt, B, vox, L.tview(dyd), wsct.data_ptr(), None, L.tview(g0), L.tview(tin), coef.data_ptr(), L.NULL_T, L.tview(one), st))
        outs.append((lo, hi, one))
    torch.cuda.synchronize()
    for i, nm in enumerate(("split.lo", "split.hi", "conv1x1")):
        same("nbwd_gemm." + nm, outs[0][i], outs[1][i])
    # transposed conv k2s2: 32 -> 32 channels written into channels [0, 32) of a 48-channel buffer at twice the extent
    if not lean:
        xl = to_dev(rnd(torch.randn(B, D, H, W, 32, generator=g), dt), dt)
        wT = pack((torch.randn(32, 32, 2, 2, 2, generator=g) * 0.1).to(DEV), L.PK_CT, 32, 32)
        bT = torch.randn(32, generator=g).to(DEV)
        S2 = (2 * D, 2 * H, 2 * W)
        ct = lib.bpx_convT3d_stats_tiles(D, H, W, 2)
        outs = []
        for cat in (torch.zeros((B,) + S2 + (48,), dtype=T, device=DEV), L.Planar(B, S2, 48, T, DEV)):
            if isinstance(cat, L.Planar):
                cat.t.zero_()
            part = torch.zeros(B, ct, 2, 32, device=DEV)
            L.check(lib.bpx_convT3d_k2s2_fwd(dt, B, D, H, W, 2, L.tview(xl), wT.data_ptr(), bT.data_ptr(), L.tview(cat, 0, 32), part.data_ptr(), st))
            outs.append((cat, part))
        torch.cuda.synchronize()
        same("convT.y", outs[0][0], outs[1][0])
        same("convT.stats", outs[0][1], outs[1][1])
    # pooling of the skip slice [32, 48) of the concat buffer, forward and backward
    pt = lib.bpx_maxpool3d_stats_tiles(dt, D, H, W, 2, 16)
    dyp = to_dev(rnd(torch.randn(B, D // 2, H // 2, W // 2, 16, generator=g), dt), dt)
    outs = []
    for xin in (xd, xp):
        y = torch.empty(B, D // 2, H // 2, W // 2, 16, dtype=T, device=DEV)
        part = torch.zeros(B, pt, 2, 16, device=DEV)
        L.check(lib.bpx_maxpool3d_fwd(dt, B, D, H, W, 2, L.tview(xin, 32, 16), L.tview(y), part.data_ptr(), st))
        dx = torch.empty(B, D, H, W, 16, dtype=T, device=DEV)
        L.check(lib.bpx_maxpool3d_bwd(dt, B, D, H, W, 2, L.tview(xin, 32, 16), L.tview(dyp), L.NULL_T, L.tview(dx), st))
        outs.append((y, part, dx))
    torch.cuda.synchronize()
    for i, nm in enumerate(("fwd.y", "fwd.stats", "bwd.dx")):
        same("maxpool." + nm, outs[0][i], outs[1][i])
    # an entry point without support must refuse the layout instead of reading it as interleaved
    y = torch.empty(B, D, H, W, Cx, dtype=T, device=DEV)
    rc = lib.bpx_norm_act_fwd(dt, B, vox, L.tview(xp), rec.data_ptr(), 0, L.tview(y), st)
    res.append(_res(f"planar[{tagd}].unsupported_entry_refuses", 0.0 if rc != 0 else 1.0, 0))
    return res


def check_parameter_gradients_are_reproducible(dtype):
    """No atomics anywhere in the parameter gradients: conv / transposed-conv bias gradients are column sums of
    per-workgroup partials combined in a fixed order (wgrad.hip), the first layer, the rank-1 shortcut and the head likewise
    (ends.hip).  Two backward passes over the same tensors give bit-identical gradients for EVERY parameter."""
    from biapy_amd.resunet import ResUNet

    torch.manual_seed(0)
    m = ResUNet(image_shape=(32, 32, 32, 1), activation="elu", feature_maps=[16, 32, 64], drop_values=[0.0] * 3, normalization="in",
                yx_down=[2] * 2, z_down=[2] * 2, isotropy=[True] * 3, larger_io=False, conv_layers=[2] * 3, compute_dtype=dtype).to(DEV).train()
    x = torch.randn(2, 1, 32, 32, 32, device=DEV)
    t = (torch.rand(2, 1, 32, 32, 32, device=DEV) > 0.5).float()
    runs = []
    for _ in range(3):
        m.zero_grad(set_to_none=True)
        F.binary_cross_entropy_with_logits(m(x), t).backward()
        torch.cuda.synchronize()
        runs.append({n: p.grad.clone() for n, p in m.named_parameters()})
    bad = [n for n in runs[0] if not (torch.equal(runs[0][n], runs[1][n]) and torch.equal(runs[0][n], runs[2][n]))]
    tag = _mode(dtype)[0]
    return [_res(f"reproducible_grads[{tag}].params_that_differ", float(len(bad)), 0.5, extra=", ".join(bad[:8]))]


# ---------------------------------------------------------------------------------------------------
# Stated parity bar per storage mode (north_star: "Dice delta < 1e-4, integer label maps bit-exact"):
#   f32 mode : |Dice delta| < 1e-4 against the fp32 CPU oracle and identical label maps except where the oracle's probability is
#              within 1e-5 of the threshold;
#   fp16 mode (compute_dtype=torch.float16, the ResUNet default and what bench.py times): forward pass and stored activations in fp16
#              (11-bit mantissa), gradients and backward MFMA operands in bf16 (BPX_MIX16).  MEETS the north-star bar: |Dice delta| < 1e-4
#              asserted, label maps identical wherever the oracle's probability is more than F16_UNDECIDED from 0.5.
#   bf16 mode: the storage type of round 1-2, kept as the A/B baseline and for the engines whose backward is bf16-only.  Its forward
#              cannot meet 1e-4 (bf16 storage, operands and weights contribute ~0.3e-4 each: scripts/bf16_error_budget.py), so NO Dice
#              claim is made for it: its rows check logits / labels outside the undecided band only.
BF16_UNDECIDED = 2e-2
F16_UNDECIDED = 2.5e-3


def _mode(dtype):
    """(tag, undecided band, Dice tolerance) of a storage mode."""
    if dtype == torch.float32:
        return "f32", 1e-5, 1e-4
    if dtype == torch.float16:
        return "f16", F16_UNDECIDED, 1e-4
    return "bf16", BF16_UNDECIDED, None                      # no Dice claim in bf16 storage (see above)
# Parameters whose true gradient is zero (a conv bias in front of an InstanceNorm) hold rounding noise on both sides; relative
# gradient errors are therefore measured against max(|g_ref|, floor * largest gradient norm of the network).
GRAD_FLOOR_F32 = 1e-3
GRAD_FLOOR_BF16 = 5e-2
# network-level tolerances per storage mode: max |logit error| / max |logit|, |loss error|, worst relative L2 error of a parameter
# gradient.  fp16 mode: fp16 forward (logits ~1e-3), gradients carried in bf16 (same bar as the bf16 mode)
LOGITS_TOL = {"f32": 2e-4, "bf16": 6e-2, "f16": 4e-3}
LOSS_TOL = {"f32": 1e-5, "bf16": 2e-2, "f16": 2e-3}
GRAD_TOL = {"f32": 2e-3, "bf16": 0.15, "f16": 0.10}   # f16 = the mixed mode: measured worst 0.060 (round 4), 0.15 until round 3


def param_level(key, depth):
    """Resolution level (0 = full resolution) of a ResUNet parameter: down_path.i -> i, bottleneck -> depth, up_paths.0.j -> depth - 1 - j (the
    transposed conv and the conv block that produce level depth - 1 - j), heads -> 0."""
    part = key.split(".")
    if part[0] == "down_path":
        return int(part[1])
    if part[0] == "bottleneck":
        return depth
    if part[0] == "up_paths":
        return depth - 1 - int(part[2])
    return 0


# 16-bit modes: worst relative L2 error of a parameter gradient PER LEVEL (VERDICT r3 next #4c).  The error depends on the depth below the loss and
# on how many voxels a level's statistics average over, so ONE bar set by the worst level would let a regression at level 0 hide under the
# allowance of level 2.  Bars = ~1.6x the largest value measured in round 4 over the 3-level golden net (32^3, B = 2), the cfg-2 net at 64^3 and at
# the benched 128^3 shape (profiles/r04_gpu_diag.txt):
#   mixed mode (fp16 forward, bf16 gradients - the benched one): level 0 0.018, 1 0.051, 2 0.060, 3 0.047, 4 0.010
#   pure bf16:                                                    level 0 0.105, 1 0.127, 2 0.140, 3 0.108, 4 0.044
# (the mixed mode's gradients are 2-3x closer to fp32: only the gradient tensors are bf16, the activations they are multiplied with are fp16)
GRAD_TOL_LEVEL_16 = {"f16": {0: 0.03, 1: 0.08, 2: 0.10, 3: 0.08, 4: 0.03}, "bf16": {0: 0.15, 1: 0.15, 2: 0.15, 3: 0.15, 4: 0.08}}


def grad_rows(tag, G, grads_ref, tagd, depth):
    """Rows for the parameter gradients: worst relative L2 error over all parameters (the single bar of rounds 1-3, kept), and per level
    against the level's own bar in the 16-bit modes."""
    per_level = {}
    worst, worst_name = 0.0, ""
    for k, gr in grads_ref.items():
        gg = G[k].cpu()
        denom = gr.norm().item()
        e = (gg - gr).norm().item() / (denom + 1e-6 * max(1.0, gr.numel() ** 0.5))
        if denom < 1e-7:      # biases in front of an InstanceNorm: the true gradient is exactly zero
            e = (gg - gr).abs().max().item() / 1e-3
        if e > worst:
            worst, worst_name = e, k
        lv = param_level(k, depth)
        if e > per_level.get(lv, (0.0, ""))[0]:
            per_level[lv] = (e, k)
    rows = [_res(tag + ".grads_rel_l2_worst", worst, GRAD_TOL[tagd], extra=worst_name)]
    if tagd != "f32":
        for lv in sorted(per_level):
            e, k = per_level[lv]
            rows.append(_res(tag + f".grads_rel_l2_level{lv}", e, GRAD_TOL_LEVEL_16[tagd].get(lv, 0.15), extra=k))
    return rows


def parity_rows(tag, logits, lo_ref, tgt, dtype, trained=False):
    """Rows of the stated parity bar for one prediction (CPU tensors)."""
    f32 = dtype == torch.float32
    _, band, dice_tol = _mode(dtype)
    p_ref = torch.sigmoid(lo_ref)
    lab_ref, lab_got = p_ref > 0.5, torch.sigmoid(logits) > 0.5
    near = (p_ref - 0.5).abs() < band
    wrong = int(((lab_ref != lab_got) & ~near).sum())
    rows = [_res(tag + ".labels_away_from_threshold", wrong, 0,
                 extra=f"{int((lab_ref != lab_got).sum())} of {lab_ref.numel()} voxels differ in all, {int(near.sum())} lie within the undecided band")]
    if (f32 or trained) and dice_tol is not None:   # on a random-init network every probability sits at the threshold: Dice is only meaningful after training
        d_ref, d_got = net_oracle.dice(p_ref, tgt), net_oracle.dice(torch.sigmoid(logits), tgt)
        rows.append(_res(tag + ".dice_delta", abs(d_ref - d_got), dice_tol, extra=f"dice_ref={d_ref:.6f} dice_got={d_got:.6f}"))
    return rows


def check_network(dtype, fm, patch, B, golden=None, seed=0, train=True, normalization="in", activation="elu"):
    """Whole network vs the oracle: logits, Dice, loss and every parameter gradient.  normalization="gn": torch.nn.GroupNorm(8, C) for every
    norm layer (what the reference's 'gn' means; its own call raises) - the oracle then runs F.group_norm, incl. the groups of 6 / 12 / 24
    channels that straddle the up / skip boundary of the decoder's concatenated inputs."""
    tagd = _mode(dtype)[0]
    if golden is not None:
        sd = {k[len("small/sd/"):]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith("small/sd/")}
        x = torch.from_numpy(golden["small/x"]).permute(0, 4, 1, 2, 3).contiguous()
        tgt = torch.from_numpy(golden["small/target"]).float()
        fm = [int(v) for v in golden["small/feature_maps"]]
    else:
        sd = net_oracle.init_state_dict(1, fm, seed=seed)
        g = torch.Generator().manual_seed(seed + 7)
        x = torch.randn(B, 1, *patch, generator=g)
        tgt = (torch.rand(B, 1, *patch, generator=g) > 0.5).float()
    eng = ResUNetEngine(NetConfig(in_ch=1, feature_maps=fm, normalization=normalization, activation=activation), dtype)
    P = {k: v.to(DEV) for k, v in sd.items()}
    if normalization != "in":           # non-trivial affine parameters (the default initialisation is gamma = 1, beta = 0)
        g = torch.Generator().manual_seed(seed + 99)
        for k in sd:
            if sd[k].dim() == 1 and (".block.1." in k or k.endswith("block.0.weight") or k.endswith("block.0.bias")) and "block.0.block" not in k:
                sd[k] = sd[k] + 0.2 * torch.randn(sd[k].shape, generator=g)
        P = {k: v.to(DEV) for k, v in sd.items()}
    xd = x.to(DEV)
    logits, ctx = eng.forward(P, xd, head_act=0, save=train)
    torch.cuda.synchronize()
    tag = f"resunet[{tagd} {normalization}{'' if activation == 'elu' else ' ' + activation} fm={fm} {tuple(x.shape)}{' golden' if golden is not None else ''}]"
    res = []
    if golden is not None:
        lo_ref = torch.from_numpy(golden["small/logits"])
    else:
        lo_ref = net_oracle.resunet_forward(sd, x, fm, normalization=normalization, activation=activation)
    scale = lo_ref.abs().max().item()
    err = (logits.cpu() - lo_ref).abs().max().item() / scale
    res.append(_res(tag + ".logits_rel", err, LOGITS_TOL[tagd], extra=f"scale={scale:.3f}"))
    res += parity_rows(tag, logits.cpu(), lo_ref, tgt, dtype)
    if not train:
        return res
    lg = logits.detach().clone().requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(lg, tgt.to(DEV))
    loss.backward()
    G = eng.backward(P, ctx, lg.grad)
    torch.cuda.synchronize()
    loss_ref, _, grads_ref = net_oracle.train_step_grads(sd, x, tgt, feature_maps=fm, normalization=normalization, activation=activation)
    res.append(_res(tag + ".loss", abs(loss.item() - loss_ref.item()), LOSS_TOL[tagd]))
    res += grad_rows(tag, G, grads_ref, tagd, len(fm) - 1)
    return res


def check_network_activation(dtype, golden, act):
    """The drop-in network with a non-default block activation against the REFERENCE fixture (resunet_activations_golden.npz: logits, loss, all
    gradient norms, four full gradients of the reference ResUNet built with that activation)."""
    tagd = _mode(dtype)[0]
    fm = [int(v) for v in golden["feature_maps"]]
    sd = {k[3:]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith("sd/")}
    x = torch.from_numpy(golden["x"]).permute(0, 4, 1, 2, 3).contiguous()
    tgt = torch.from_numpy(golden["target"]).float()
    eng = ResUNetEngine(NetConfig(in_ch=1, feature_maps=fm, activation=act), dtype)
    P = {k: v.to(DEV) for k, v in sd.items()}
    logits, ctx = eng.forward(P, x.to(DEV), head_act=0, save=True)
    lg = logits.detach().clone().requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(lg, tgt.to(DEV))
    loss.backward()
    G = eng.backward(P, ctx, lg.grad)
    torch.cuda.synchronize()
    tag = f"resunet_activation[{tagd} {act}]"
    lo_ref = torch.from_numpy(golden[f"{act}/logits"])
    res = [_res(tag + ".logits_rel", (logits.cpu() - lo_ref).abs().max().item() / lo_ref.abs().max().item(), LOGITS_TOL[tagd]),
           _res(tag + ".loss", abs(loss.item() - float(golden[f"{act}/loss"])), LOSS_TOL[tagd])]
    gmax = max(float(golden[k]) for k in golden.files if k.startswith(f"{act}/gradnorm/"))
    worst, wname = 0.0, ""
    for k in golden.files:
        if k.startswith(f"{act}/gradnorm/"):
            name = k[len(f"{act}/gradnorm/"):]
            ref = float(golden[k])
            e = abs(G[name].norm().item() - ref) / max(ref, (GRAD_FLOOR_F32 if dtype == torch.float32 else GRAD_FLOOR_BF16) * gmax)
            if e > worst:
                worst, wname = e, name
    res.append(_res(tag + ".grad_norms_rel_worst", worst, GRAD_TOL[tagd], extra=wname))
    worst, wname = 0.0, ""
    for k in golden.files:
        if k.startswith(f"{act}/grad/"):
            name = k[len(f"{act}/grad/"):]
            ref = torch.from_numpy(golden[k])
            e = (G[name].cpu() - ref).norm().item() / max(ref.norm().item(), 1e-6 * gmax)
            if e > worst:
                worst, wname = e, name
    res.append(_res(tag + ".full_grads_rel_l2_worst", worst, GRAD_TOL[tagd], extra=wname))
    return res


_CFG2_CACHE = {}


def _cfg2_oracle():
    """One CPU oracle train step of the cfg-2 network on ONE 128^3 patch (about 10 s on the GPU box's cores), shared by the
    f32 and bf16 tests; plus three more seeded samples (inputs only) for the batch-4 consistency check."""
    if "ref" not in _CFG2_CACHE:
        fm = [16, 32, 64, 128, 256]
        sd = net_oracle.init_state_dict(1, fm, seed=0)
        g = torch.Generator().manual_seed(41)
        x = torch.randn(4, 1, 128, 128, 128, generator=g)
        n = torch.randn(4, 1, 128, 128, 128, generator=g)
        tgt = (F.avg_pool3d(n, 9, stride=1, padding=4) > 0).float()          # bench.py's blob targets
        loss_ref, lo_ref, grads_ref = net_oracle.train_step_grads(sd, x[:1], tgt[:1], feature_maps=fm)
        _CFG2_CACHE["ref"] = (fm, sd, x, tgt, loss_ref, lo_ref, grads_ref)
    return _CFG2_CACHE["ref"]


def check_network_cfg2_benched_shape(dtype):
    """The benched workload AT ITS OWN SIZE: cfg 2 = fm 16-32-64-128-256 on 128^3 patches, batch 4 - the
    (4,8,16) big-tile kernels, the XCD tile walk over 8192 tiles per sample, byte offsets up to 805 MB.
      * sample 0 alone (batch 1): logits, BCE loss and every parameter gradient against the CPU oracle;
      * the batch of 4: per-sample logits must equal - bit for bit - the four batch-1 forwards (InstanceNorm is per sample), and
        the batch gradient must equal the mean of the four batch-1 gradients."""
    fm, sd, x, tgt, loss_ref, lo_ref, grads_ref = _cfg2_oracle()
    f32 = dtype == torch.float32
    tagd = _mode(dtype)[0]
    tag = f"cfg2_128^3[{tagd}]"
    eng = ResUNetEngine(NetConfig(in_ch=1, feature_maps=fm), dtype)
    P = {k: v.to(DEV) for k, v in sd.items()}

    def step(xb, tb):
        logits, ctx = eng.forward(P, xb.to(DEV), head_act=0, save=True)
        lg = logits.detach().clone().requires_grad_(True)
        loss = F.binary_cross_entropy_with_logits(lg, tb.to(DEV))
        loss.backward()
        G = eng.backward(P, ctx, lg.grad)
        torch.cuda.synchronize()
        return logits.cpu(), loss.item(), {k: v.cpu() for k, v in G.items()}

    lo1, loss1, G1 = step(x[:1], tgt[:1])
    scale = lo_ref.abs().max().item()
    res = [_res(tag + ".b1.logits_rel", (lo1 - lo_ref).abs().max().item() / scale, LOGITS_TOL[tagd], extra=f"scale={scale:.3f}")]
    res += parity_rows(tag + ".b1", lo1, lo_ref, tgt[:1], dtype)
    res.append(_res(tag + ".b1.loss", abs(loss1 - loss_ref.item()), LOSS_TOL[tagd]))
    # conv biases in front of an InstanceNorm have a ZERO true gradient (what both sides hold is rounding noise of 2 M-term sums):
    # errors are measured against max(|g_ref|, GRAD_FLOOR * the largest gradient norm of the network)
    floor = GRAD_FLOOR_F32 if f32 else GRAD_FLOOR_BF16
    gmax = max(gr.norm().item() for gr in grads_ref.values())
    worst, wname, per_level = 0.0, "", {}
    for k, gr in grads_ref.items():
        e = (G1[k] - gr).norm().item() / max(gr.norm().item(), floor * gmax)
        if e > worst:
            worst, wname = e, k
        lv = param_level(k, len(fm) - 1)
        if e > per_level.get(lv, (0.0, ""))[0]:
            per_level[lv] = (e, k)
    res.append(_res(tag + ".b1.grads_rel_l2_worst", worst, GRAD_TOL[tagd], extra=wname))
    if not f32:
        for lv in sorted(per_level):
            res.append(_res(tag + f".b1.grads_rel_l2_level{lv}", per_level[lv][0], GRAD_TOL_LEVEL_16[tagd].get(lv, 0.15), extra=per_level[lv][1]))
    # batch 4 == four batch-1 steps
    lo4, loss4, G4 = step(x, tgt)
    singles = [(lo1, loss1, G1)] + [step(x[b:b + 1], tgt[b:b + 1]) for b in range(1, 4)]
    res.append(_res(tag + ".b4.logits_equal_batch1_runs", sum(int((lo4[b] != singles[b][0][0]).sum()) for b in range(4)), 0))
    res.append(_res(tag + ".b4.loss", abs(loss4 - sum(s_[1] for s_ in singles) / 4), 1e-6 if f32 else 1e-5))
    worst, wname = 0.0, ""
    gmax4 = max(v.norm().item() for v in G4.values())
    for k in G4:
        mean = sum(s_[2][k] for s_ in singles) / 4
        e = (G4[k] - mean).norm().item() / max(mean.norm().item(), floor * gmax4)
        if e > worst:
            worst, wname = e, k
    res.append(_res(tag + ".b4.grads_vs_mean_of_batch1_grads", worst, 1e-4 if f32 else 2e-3, extra=wname))
    return res


def check_sliding_window_cfg3_shape(dtype):
    """A cfg-3-shaped sliding window against the oracle pipeline: the cfg-2 network, 128^3 patches, 50 %
    overlap along z, a (320,128,128) volume = 5 patch rows (the reference's rule shrinks the step to 48, so up to three patches
    cover a slice - as at cfg 3, where overlap 68 > P/2), blended as TWO Z-slabs with the boundary partial sums handed over - against crop -> oracle forward -> sigmoid -> merge on the CPU."""
    from biapy_amd.resunet import ResUNet

    fm = [16, 32, 64, 128, 256]
    sd = net_oracle.init_state_dict(1, fm, seed=0)
    m = ResUNet(image_shape=(128, 128, 128, 1), activation="elu", feature_maps=fm, drop_values=[0.0] * 5, normalization="in", yx_down=[2] * 4,
                z_down=[2] * 4, isotropy=[True] * 5, larger_io=False, conv_layers=[2] * 5, compute_dtype=dtype)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    rs = np.random.RandomState(9)
    vshape, patch, ov = (320, 128, 128, 1), (128, 128, 128), (0.5, 0.0, 0.0)
    vol = rs.randn(*vshape).astype(np.float32)
    if "sw" not in _CFG2_CACHE:
        p, _ = TO.crop(vol, patch + (1,), ov)
        with torch.no_grad():
            pr = torch.cat([torch.sigmoid(net_oracle.resunet_forward(sd, torch.from_numpy(p[i:i + 1]).permute(0, 4, 1, 2, 3), fm)) for i in range(p.shape[0])])
        _CFG2_CACHE["sw"] = TO.merge(pr.permute(0, 2, 3, 4, 1).contiguous().numpy(), vshape, overlap=ov)
    ref = _CFG2_CACHE["sw"]
    plan = tiling.MergePlan(vshape[:3], patch, ov, (0, 0, 0), torch.device(DEV))
    nz = plan.grid[0].n
    tv = torch.from_numpy(vol).to(DEV)
    with torch.no_grad():
        pred = torch.cat([m.predict_proba(tiling.crop_device(tv, patch, ov, c_begin=i, c_count=1).permute(0, 4, 1, 2, 3)) for i in range(nz)])
    pred = pred.permute(0, 2, 3, 4, 1).contiguous()
    h = nz // 2
    z_split, z0_hi = plan.row_start(h), plan.row_start(h - 1) + patch[0]
    got = np.empty(vshape, np.float32)
    r0, r1 = pred[:h].contiguous(), pred[h:].contiguous()
    got[:z_split] = tiling.merge_device(r0, plan, z_lo=0, z_hi=z_split, zrow_lo=0, zrow_hi=h).cpu().numpy()
    nb = z0_hi - z_split
    acc = torch.zeros((nb, vshape[1], vshape[2], 1), dtype=torch.float32, device=DEV)
    wacc = torch.zeros((nb, vshape[1], vshape[2], 1), dtype=torch.float32, device=DEV)
    tiling.merge_device(r0, plan, z_lo=z_split, z_hi=z0_hi, zrow_lo=0, zrow_hi=h, acc=acc, wacc=wacc, write_partial=True)
    got[z_split:z0_hi] = tiling.merge_device(r1, plan, z_lo=z_split, z_hi=z0_hi, zrow_lo=h, zrow_hi=nz, acc=acc, wacc=wacc, seed=True).cpu().numpy()
    got[z0_hi:] = tiling.merge_device(r1, plan, z_lo=z0_hi, z_hi=vshape[0], zrow_lo=h, zrow_hi=nz).cpu().numpy()
    tagd, band, _ = _mode(dtype)
    res = [_res(f"sliding_cfg3_shape_prob[{tagd}]", float(np.abs(got - ref).max()), {"f32": 2e-5, "bf16": 3e-2, "f16": 4e-3}[tagd],
                extra=f"{nz} patches of 128^3, two slabs")]
    near = np.abs(ref - 0.5) < band
    res.append(_res(f"sliding_cfg3_shape_labels_away_from_threshold[{tagd}]", int((((ref > 0.5) != (got > 0.5)) & ~near).sum()), 0,
                    extra=f"undecided band: {int(near.sum())} of {near.size} voxels"))
    full = tiling.merge_device(pred, plan).cpu().numpy()
    res.append(_res(f"sliding_cfg3_shape_two_slabs_equal_one[{tagd}]", int((full.view(np.uint32) != got.view(np.uint32)).sum()), 0))
    return res


def check_resunetpp(dtype, golden):
    """biapy_amd.resunetpp.ResUNetPlusPlus (row X) against the reference's own ResUNetPlusPlus outputs
    (tests/golden/resunetpp_golden.npz: fm 16-32-64 on a 16x32x32 patch, B = 2, three output channels): logits, MSE loss, every
    gradient norm and the stored full gradients (residual block with 3x3x3 shortcut + norm, SE, ASPP with dilations 6/12/18,
    attention gate, transposed conv, heads), through the module and torch's autograd boundary."""
    from biapy_amd.resunetpp import ResUNetPlusPlus

    g = golden
    fm = [int(v) for v in g["feature_maps"]]
    m = ResUNetPlusPlus(image_shape=(16, 32, 32, 1), activation="elu", feature_maps=fm, drop_values=[0.0] * 3, normalization="in", k_size=3,
                        upsample_layer="convtranspose", yx_down=[2, 2], z_down=[2, 2], output_channels=[3], output_channel_info=["BCD"],
                        head_activations=["ce_sigmoid", "ce_sigmoid", "linear"], isotropy=[True] * 3, larger_io=False, conv_layers=[2] * 3,
                        compute_dtype=dtype)
    m.load_state_dict({k[3:]: torch.from_numpy(g[k].astype(np.float32)) for k in g.files if k.startswith("sd/")}, strict=True)
    m = m.to(DEV).train()
    x = torch.from_numpy(g["x"]).permute(0, 4, 1, 2, 3).to(DEV)
    tgt = torch.from_numpy(g["target"].astype(np.float32)).to(DEV)
    logits = m(x)
    loss = torch.nn.MSELoss()(logits, tgt)
    loss.backward()
    torch.cuda.synchronize()
    f32 = dtype == torch.float32
    mx = dtype == torch.float16      # the mixed mode (round 4): fp16 forward / activations - a forward an order of magnitude closer than bf16's - and bf16 gradients
    tag = f"resunet++[{'f32' if f32 else 'mix16' if mx else 'bf16'}]"
    lo_ref = torch.from_numpy(g["logits"])
    res = [_res(tag + ".logits_rel", (logits.detach().cpu() - lo_ref).abs().max().item() / lo_ref.abs().max().item(), 3e-4 if f32 else 1.5e-2 if mx else 8e-2)]
    res.append(_res(tag + ".loss", abs(loss.item() - float(g["loss"])) / float(g["loss"]), 1e-5 if f32 else 8e-3 if mx else 3e-2))
    names = dict(m.named_parameters())
    gmax = max(float(g[k]) for k in g.files if k.startswith("gradnorm/"))
    floor = GRAD_FLOOR_F32 if f32 else GRAD_FLOOR_BF16
    worst, wname = 0.0, ""
    for k in g.files:
        if k.startswith("gradnorm/"):
            ref = float(g[k])
            e = abs(names[k[9:]].grad.norm().item() - ref) / max(ref, floor * gmax)
            if e > worst:
                worst, wname = e, k[9:]
    res.append(_res(tag + ".gradnorms_rel_worst", worst, 3e-3 if f32 else 0.25, extra=wname))
    worst, wname = 0.0, ""
    for k in g.files:
        if k.startswith("grad/"):
            ref = torch.from_numpy(g[k])
            e = (names[k[5:]].grad.cpu() - ref).norm().item() / max(ref.norm().item(), floor * gmax)
            if e > worst:
                worst, wname = e, k[5:]
    res.append(_res(tag + ".full_grads_rel_l2_worst", worst, 3e-3 if f32 else 0.25, extra=wname))
    with torch.no_grad():
        pr = m.eval().predict_proba(x, ["ce_sigmoid", "ce_sigmoid", "tanh"]).cpu()
    lo_dev = logits.detach().cpu()                                   # the fused head activations, against torch's on the device's own logits
    want = torch.cat([torch.sigmoid(lo_dev[:, :2]), torch.tanh(lo_dev[:, 2:])], 1)
    res.append(_res(tag + ".predict_proba(sigmoid,sigmoid,tanh)", (pr - want).abs().max().item(), 2e-6))
    return res


_CFG4_CACHE = {}


def _cfg4_oracle():
    """One CPU oracle step (forward, MSE loss, every gradient) of the cfg-4 ResUNet++ on ONE 80^3 patch, shared by the f32 and bf16
    tests: seeded module weights, three output channels."""
    if "ref" not in _CFG4_CACHE:
        from biapy_amd.resunetpp import ResUNetPlusPlus
        from oracle import resunetpp_oracle

        fm = [16, 32, 64, 128, 256]
        torch.manual_seed(11)
        m = ResUNetPlusPlus(image_shape=(80, 80, 80, 1), activation="elu", feature_maps=fm, drop_values=[0.0] * 5, normalization="in", yx_down=[2] * 4,
                            z_down=[2] * 4, output_channels=[3], output_channel_info=["BCD"], head_activations=["ce_sigmoid", "ce_sigmoid", "linear"],
                            isotropy=[True] * 5, larger_io=False, conv_layers=[2] * 5)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        g = torch.Generator().manual_seed(12)
        x = torch.randn(2, 1, 80, 80, 80, generator=g)
        tgt = torch.randn(2, 3, 80, 80, 80, generator=g)
        P = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
        lo = resunetpp_oracle.resunetpp_forward(P, x[:1], fm)
        loss = F.mse_loss(lo, tgt[:1])
        names = [k for k, v in P.items() if v.requires_grad]
        grads = dict(zip(names, torch.autograd.grad(loss, [P[k] for k in names], allow_unused=True)))
        _CFG4_CACHE["ref"] = (fm, sd, x, tgt, loss.detach(), lo.detach(), {k: v for k, v in grads.items() if v is not None})
    return _CFG4_CACHE["ref"]


def check_resunetpp_cfg4_shape(dtype):
    """Row X AT THE BENCHED SIZE: cfg 4 = ResUNet++ fm 16-32-64-128-256 on an 80^3 patch - the ASPP's packed dilated convolutions at
    the real rates (6 / 12 / 18 on 80^3 -> 89^3 / 95^3 / 107^3 packed volumes; rate 6 on the 10^3 bridge -> 17^3, rates 12 / 18 there
    as the centre tap), squeeze-excite and attention gates at their true sizes - against the CPU oracle: logits, MSE loss and every
    parameter gradient of sample 0; then the batch of 2 against its two batch-1 runs (every normalisation / gate is per sample).

    bf16 bars at this size are wide on purpose, and measured: this randomly initialised network (un-squashed attention gates, SE
    products, five levels) amplifies rounding - in the f32 mode, rounding ONLY the input to bf16 moves the logits by 2.2 % (relative
    L2) and rounding ONLY the weights by 4.0 %; the bf16 mode does both and rounds every activation (9.2 %), and the weight gradients
    inherit it (norms within 6 %, directions within 0.54 relative L2).  What the bf16 rows pin down is therefore: the loss (1.5e-4),
    bounded logits / gradient error, and - exactly - that a batch is the same as its samples run alone."""
    from biapy_amd.resunetpp import ResUNetPlusPlus

    fm, sd, x, tgt, loss_ref, lo_ref, grads_ref = _cfg4_oracle()
    f32 = dtype == torch.float32
    mx = dtype == torch.float16      # mixed mode: the fp16 forward is held to an eighth of the bf16 forward bars, the bf16 gradient path to the bf16 bars
    tag = f"cfg4_80^3[{'f32' if f32 else 'mix16' if mx else 'bf16'}]"
    m = ResUNetPlusPlus(image_shape=(80, 80, 80, 1), activation="elu", feature_maps=fm, drop_values=[0.0] * 5, normalization="in", yx_down=[2] * 4,
                        z_down=[2] * 4, output_channels=[3], output_channel_info=["BCD"], head_activations=["ce_sigmoid", "ce_sigmoid", "linear"],
                        isotropy=[True] * 5, larger_io=False, conv_layers=[2] * 5, compute_dtype=dtype)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train()

    def step(xb, tb):
        m.zero_grad(set_to_none=True)
        lo = m(xb.to(DEV))
        loss = F.mse_loss(lo, tb.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        return lo.detach().cpu(), loss.item(), {k: p.grad.detach().cpu() for k, p in m.named_parameters()}

    lo1, loss1, G1 = step(x[:1], tgt[:1])
    scale = lo_ref.abs().max().item()
    res = [_res(tag + ".b1.logits_rel", (lo1 - lo_ref).abs().max().item() / scale, 3e-4 if f32 else 0.025 if mx else 0.2, extra=f"scale={scale:.3f}")]
    res.append(_res(tag + ".b1.logits_rel_l2", ((lo1 - lo_ref).norm() / lo_ref.norm()).item(), 1e-4 if f32 else 0.02 if mx else 0.15))
    res.append(_res(tag + ".b1.loss_rel", abs(loss1 - loss_ref.item()) / loss_ref.item(), 1e-5 if f32 else 1e-3 if mx else 5e-3))
    floor = GRAD_FLOOR_F32 if f32 else GRAD_FLOOR_BF16
    gmax = max(gr.norm().item() for gr in grads_ref.values())
    nworst, nname = 0.0, ""
    for k, gr in grads_ref.items():                       # gradient NORMS of the parameters that carry the gradient (> 5 % of the largest)
        if gr.norm().item() > 0.05 * gmax:
            e = abs(G1[k].norm().item() - gr.norm().item()) / gr.norm().item()
            if e > nworst:
                nworst, nname = e, k
    res.append(_res(tag + ".b1.gradnorms_rel_worst", nworst, 2e-3 if f32 else 0.15, extra=nname))
    # Biases of convolutions that feed an InstanceNorm directly (the shortcut conv, the first conv of a residual block, the two
    # attention branches whose sum is normalised) have a true gradient of exactly zero: what the oracle and the device hold there is the
    # rounding noise of 0.5 M-term sums (1e-4 on the CPU side at this size).  They are checked to BE noise on both sides; every other
    # parameter against max(|g_ref|, floor * the largest gradient norm) - the fp32 noise of these sums is ~1e-5 of the largest norm.
    import re
    zero = re.compile(r".*(\.shortcut\.0\.bias|\.block\.[02]\.block\.0\.bias|\.conv_(encoder|decoder)\.2\.bias)$")
    worst, wname, zworst, zname = 0.0, "", 0.0, ""
    for k, gr in grads_ref.items():
        if zero.match(k):
            e = max(G1[k].norm().item(), gr.norm().item()) / gmax
            if e > zworst:
                zworst, zname = e, k
            continue
        e = (G1[k] - gr).norm().item() / max(gr.norm().item(), floor * gmax)
        if e > worst:
            worst, wname = e, k
    res.append(_res(tag + ".b1.grads_rel_l2_worst", worst, 2e-2 if f32 else 0.7, extra=wname))
    res.append(_res(tag + ".b1.zero_gradient_biases_are_noise", zworst, 1e-3 if f32 else 5e-2, extra=zname))
    lo2, loss2, G2 = step(x, tgt)
    lo1b, loss1b, G1b = step(x[1:2], tgt[1:2])
    res.append(_res(tag + ".b2.logits_equal_batch1_runs", int((lo2[0] != lo1[0]).sum()) + int((lo2[1] != lo1b[0]).sum()), 0))
    res.append(_res(tag + ".b2.loss", abs(loss2 - (loss1 + loss1b) / 2), 1e-6 if f32 else 1e-5))
    worst, wname = 0.0, ""
    gmax2 = max(v.norm().item() for v in G2.values())
    for k in G2:
        mean = (G1[k] + G1b[k]) / 2
        e = (G2[k] - mean).norm().item() / max(mean.norm().item(), floor * gmax2)
        if e > worst:
            worst, wname = e, k
    res.append(_res(tag + ".b2.grads_vs_mean_of_batch1_grads", worst, 2e-3 if f32 else 2e-2, extra=wname))
    return res


def check_instance_loss():
    """biapy_amd.losses.InstanceChannelsLoss (B, C, D channels; fused tanh + BCE / MSE / L1) against the reference's own
    instance_segmentation_loss outputs (tests/golden/losses_golden.npz): value and gradient w.r.t. the raw logits."""
    import os

    from make_golden import loss_inputs

    from biapy_amd.losses import InstanceChannelsLoss

    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses_golden.npz"))
    _, _, z3, t3 = loss_inputs()
    res = []
    for tag, losses, w in (("bcd_mse", ["bce", "bce", "mse"], (1, 1, 1)), ("bcd_l1_w", ["bce", "bce", "l1"], (0.5, 0.25, 2.0))):
        crit = InstanceChannelsLoss(channel_weights=w, out_channels=["B", "C", "D"], losses_to_use=losses).to(DEV)
        z = z3.to(DEV).requires_grad_(True)
        val = crit(z, t3.to(DEV))
        val.backward()
        torch.cuda.synchronize()
        res.append(_res(f"instance_loss[{tag}].value", abs(val.item() - float(gold[f"instance_{tag}/value"])), 2e-6))
        gr = gold[f"instance_{tag}/grad"]
        res.append(_res(f"instance_loss[{tag}].grad", float(np.abs(z.grad.cpu().numpy() - gr).max() / np.abs(gr).max()), 2e-5))
    return res


def check_multiclass_ce():
    """biapy_amd.losses.CrossEntropyLoss_wrapper with num_classes > 2 (bpx_softmax_ce_*) against the reference class's own values and gradients
    (tests/golden/losses_multiclass_golden.npz), the confusion counts against the oracle's confusion matrix, and a large ragged case against the oracle."""
    import os

    from make_golden import loss_inputs_multiclass
    from oracle import loss_oracle as LO

    from biapy_amd.losses import CrossEntropyLoss_wrapper, class_confusion_counts, jaccard_index_multiclass

    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses_multiclass_golden.npz"))
    z3, y3, z5, y5 = loss_inputs_multiclass()
    res = []

    def run(name, crit, y, *zs):
        zz = [z.to(DEV).requires_grad_(True) for z in zs]
        val = crit(zz if len(zz) > 1 else zz[0], y.to(DEV))
        val.backward()
        torch.cuda.synchronize()
        res.append(_res(f"multiclass_ce[{name}].value", abs(val.item() - float(gold[f"{name}/value"])), 3e-6))
        for k, z in enumerate(zz):
            gr = gold[f"{name}/grad{k}"]
            res.append(_res(f"multiclass_ce[{name}].grad{k}", float(np.abs(z.grad.cpu().numpy() - gr).max() / np.abs(gr).max()), 2e-5))

    run("ce3", CrossEntropyLoss_wrapper(num_classes=3, ndim=3), y3, z3)
    run("ce3_w", CrossEntropyLoss_wrapper(num_classes=3, ndim=3, class_rebalance="manual", class_weights=[0.2, 0.5, 0.3]), y3, z3)
    run("ce5_ignore", CrossEntropyLoss_wrapper(num_classes=5, ndim=3, ignore_index=255), y5, z5)
    run("ce5_w_ignore", CrossEntropyLoss_wrapper(num_classes=5, ndim=3, class_rebalance="manual", class_weights=[1.0, 2.0, 0.5, 0.25, 4.0], ignore_index=255), y5, z5)
    run("ce3_deep", CrossEntropyLoss_wrapper(num_classes=3, ndim=3), y3, z3, torch.from_numpy(gold["ce3_deep/zh"]))
    res.append(_res("multiclass_ce.counts", (class_confusion_counts(z5.to(DEV), y5.to(DEV), 255).cpu() - LO.confusion_counts(z5, y5, 255)).abs().max().item(), 0))
    # a volume with many blocks per sample, a ragged voxel count, 8 classes, one class absent from the labels
    g = torch.Generator().manual_seed(5)
    zb = torch.randn(3, 8, 37, 61, 53, generator=g) * 3
    yb = torch.randint(0, 7, (3, 1, 37, 61, 53), generator=g).float()
    yb[torch.rand(yb.shape, generator=g) < 0.05] = -100.0
    w8 = torch.rand(8, generator=g) + 0.25
    zr = zb.clone().requires_grad_(True)
    ref = LO.softmax_ce(zr, yb, w8, -100)
    ref.backward()
    zd = zb.to(DEV).requires_grad_(True)
    val = CrossEntropyLoss_wrapper(num_classes=8, ndim=3, class_rebalance="manual", class_weights=w8.tolist())(zd, yb.to(DEV))
    val.backward()
    res.append(_res("multiclass_ce[8 classes, 3 x 37x61x53].value", abs(val.item() - ref.item()) / abs(ref.item()), 2e-6))
    res.append(_res("multiclass_ce[8 classes, 3 x 37x61x53].grad", ((zd.grad.cpu() - zr.grad).abs().max() / zr.grad.abs().max()).item(), 2e-5))
    cd, co = class_confusion_counts(zd.detach(), yb.to(DEV)).cpu(), LO.confusion_counts(zb, yb)
    res.append(_res("multiclass_ce[8 classes].counts", (cd - co).abs().max().item(), 0))
    union = co[1] + co[2] - co[0]
    iou_ref = (co[0][union > 0] / union[union > 0]).mean().item()
    res.append(_res("multiclass_ce[8 classes].macro_iou", abs(jaccard_index_multiclass(zd.detach(), yb.to(DEV)).item() - iou_ref), 1e-6))
    # the metric OBJECT of the reference's call sites: jaccard_index(num_classes=...)(y_pred, y_true), dict / list predictions
    from biapy_amd.losses import jaccard_index
    met = jaccard_index(num_classes=8, device=DEV, ndim=3)
    res.append(_res("jaccard_index[object, 8 classes, dict]", abs(met({"pred": zd.detach()}, yb.to(DEV)).item() - iou_ref), 1e-6))
    zb1 = torch.randn(2, 1, 9, 20, 24, generator=g)
    tb1 = (torch.rand(2, 1, 9, 20, 24, generator=g) > 0.5).float()
    P, T = torch.sigmoid(zb1) > 0.5, tb1 > 0.5
    ref1 = ((P & T).sum().double() / (P | T).sum().double()).item()
    met2 = jaccard_index(num_classes=2, device=DEV, ndim=3)
    res.append(_res("jaccard_index[object, binary]", abs(met2(zb1.to(DEV), tb1.to(DEV)).item() - ref1), 1e-6))
    res.append(_res("jaccard_index[functional form kept]", abs(jaccard_index(zb1.to(DEV), tb1.to(DEV)).item() - ref1), 1e-6))
    half = torch.nn.functional.interpolate(tb1, size=(5, 10, 12), mode="nearest")
    zh = torch.randn(2, 1, 5, 10, 12, generator=g)
    Ph, Th = torch.sigmoid(zh) > 0.5, half > 0.5
    ref2 = 0.5 * (ref1 + ((Ph & Th).sum().double() / (Ph | Th).sum().double()).item())
    res.append(_res("jaccard_index[object, list of two predictions]", abs(met2([zb1.to(DEV), zh.to(DEV)], tb1.to(DEV)).item() - ref2), 1e-6))
    return res


def check_resunet_sr(dtype, tag, golden):
    """3-D super-resolution through biapy_amd.resunet.ResUNet(upsampling_factor, upsampling_position) (row S) against the
    reference's own outputs, L1 loss and gradients (tests/golden/resunet_sr_golden.npz)."""
    from biapy_amd.resunet import ResUNet

    g = golden
    pre = f"{tag}/sd/"
    sd = {k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}
    xl = torch.from_numpy(g[f"{tag}/x"])
    m = ResUNet(image_shape=tuple(xl.shape[1:]), activation="elu", feature_maps=[16, 32], drop_values=[0.0] * 2, normalization="in", yx_down=[2],
                z_down=[2], isotropy=[True] * 2, larger_io=False, conv_layers=[2] * 2, head_activations=["linear"],
                upsampling_factor=tuple(int(v) for v in g[f"{tag}/factor"]), upsampling_position=str(g[f"{tag}/pos"]), compute_dtype=dtype)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train()
    y = m(xl.permute(0, 4, 1, 2, 3).to(DEV))
    loss = torch.nn.L1Loss()(y, torch.from_numpy(g[f"{tag}/target"]).to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    f32 = dtype == torch.float32
    name = f"resunet_sr[{tag} {'f32' if f32 else 'bf16'}]"
    ref = torch.from_numpy(g[f"{tag}/out"])
    res = [_res(name + ".out_rel", (y.detach().cpu() - ref).abs().max().item() / ref.abs().max().item(), 3e-4 if f32 else 8e-2)]
    res.append(_res(name + ".loss", abs(loss.item() - float(g[f"{tag}/loss"])), 1e-5 if f32 else 2e-2))
    names = dict(m.named_parameters())
    gmax = max(float(g[k]) for k in g.files if k.startswith(f"{tag}/gradnorm/"))
    floor = GRAD_FLOOR_F32 if f32 else GRAD_FLOOR_BF16
    worst, wname = 0.0, ""
    for k in g.files:
        if k.startswith(f"{tag}/gradnorm/"):
            r_ = float(g[k])
            e = abs(names[k[len(tag) + 10:]].grad.norm().item() - r_) / max(r_, floor * gmax)
            if e > worst:
                worst, wname = e, k
    res.append(_res(name + ".gradnorms_rel_worst", worst, 3e-3 if f32 else 0.25, extra=wname))
    worst, wname = 0.0, ""
    for k in g.files:
        if k.startswith(f"{tag}/grad/"):
            r_ = torch.from_numpy(g[k])
            e = (names[k[len(tag) + 6:]].grad.cpu() - r_).norm().item() / max(r_.norm().item(), floor * gmax)
            if e > worst:
                worst, wname = e, k
    res.append(_res(name + ".full_grads_rel_l2_worst", worst, 3e-3 if f32 else 0.25, extra=wname))
    with torch.no_grad():
        yi = m.eval()(xl.permute(0, 4, 1, 2, 3).to(DEV)).cpu()
    res.append(_res(name + ".inference_equals_training_forward", (yi - y.detach().cpu()).abs().max().item(), 0 if f32 else 1e-6))
    return res


def check_network_aniso(dtype, golden):
    """Anisotropic ResUNet (Z_DOWN = [1, 2]) against the reference fixture tests/golden/resunet_aniso_golden.npz: logits, loss
    and every gradient norm + the stored full gradients."""
    tagd = _mode(dtype)[0]
    fm = [int(v) for v in golden["feature_maps"]]
    zd = [int(v) for v in golden["z_down"]]
    sd = {k[3:]: torch.from_numpy(golden[k].astype(np.float32)) for k in golden.files if k.startswith("sd/")}
    x = torch.from_numpy(golden["x"]).permute(0, 4, 1, 2, 3).contiguous()
    tgt = torch.from_numpy(golden["target"]).float()
    eng = ResUNetEngine(NetConfig(in_ch=1, feature_maps=fm, z_down=zd), dtype)
    P = {k: v.to(DEV) for k, v in sd.items()}
    logits, ctx = eng.forward(P, x.to(DEV), head_act=0, save=True)
    lg = logits.detach().clone().requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(lg, tgt.to(DEV))
    loss.backward()
    G = eng.backward(P, ctx, lg.grad)
    torch.cuda.synchronize()
    tag = f"resunet_aniso[{tagd} fm={fm} z_down={zd}]"
    lo_ref = torch.from_numpy(golden["logits"])
    res = [_res(tag + ".logits_rel", (logits.cpu() - lo_ref).abs().max().item() / lo_ref.abs().max().item(), LOGITS_TOL[tagd])]
    res.append(_res(tag + ".loss", abs(loss.item() - float(golden["loss"])), LOSS_TOL[tagd]))
    gtol = GRAD_TOL[tagd]
    worst, wname = 0.0, ""
    for k in golden.files:
        if k.startswith("grad/"):
            gr = torch.from_numpy(golden[k])
            e = (G[k[5:]].cpu() - gr).norm().item() / (gr.norm().item() + 1e-12)
            if e > worst:
                worst, wname = e, k[5:]
    res.append(_res(tag + ".grads_rel_l2_worst", worst, gtol, extra=wname))
    worst, wname = 0.0, ""
    for k in golden.files:
        if k.startswith("gradnorm/"):
            ref = float(golden[k])
            if ref > 1e-6:
                e = abs(G[k[9:]].norm().item() - ref) / ref
                if e > worst:
                    worst, wname = e, k[9:]
    res.append(_res(tag + ".gradnorm_rel_worst", worst, gtol, extra=wname))
    return res


def check_norm_act(dt, B=2, S=(6, 10, 12), Cc=48, act="elu", seed=0, groups=None):
    """bpx_norm_act_fwd / bpx_norm_act_bwd (+ finalize + apply) against autograd through act(instance_norm(x)) - or, with
    ``groups``, through act(torch group_norm(x, groups)): GroupNorm(G < C) forward AND backward (blocks.py:2117-2125)."""
    D, H, W = S
    vox = D * H * W
    g = torch.Generator().manual_seed(seed)
    x = rnd(torch.randn(B, D, H, W, Cc, generator=g) * 1.5 + 0.3, dt)
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.2
    dy = rnd(torch.randn(B, D, H, W, Cc, generator=g), dt)
    xr = ncdhw(x).requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    fn = {"elu": F.elu, "relu": F.relu, "silu": F.silu}[act]
    G_ = Cc if groups is None else groups
    y_ref = fn(F.instance_norm(xr, None, None, gr, br, True, 0.1, 1e-5)) if groups is None else fn(F.group_norm(xr, groups, gr, br, 1e-5))
    y_ref.backward(ncdhw(dy))
    tag = f"norm_act[{'bf16' if dt == L.BF16 else 'f32'} B{B} {S} C{Cc} {act}{'' if groups is None else ' GN%d' % groups}]"
    st = L.stream_ptr()
    xd, dyd = to_dev(x, dt), to_dev(dy, dt)
    tiles = lib.bpx_tensor_stats_tiles(vox)
    part = torch.zeros(B, tiles, 2, Cc, dtype=torch.float32, device=DEV)
    L.check(lib.bpx_tensor_stats(dt, B, vox, L.tview(xd), part.data_ptr(), st))
    rec = torch.empty(B, Cc, 4, dtype=torch.float32, device=DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    L.check(lib.bpx_norm_finalize(part.data_ptr(), B, tiles, Cc, vox, gd.data_ptr(), bd.data_ptr(), 1e-5, G_, rec.data_ptr(), Cc, 0, st))
    extra = 16
    yb = torch.full((B, D, H, W, Cc + extra), 3.0, dtype=tdtype(dt), device=DEV)
    code = L.ACT[act]
    L.check(lib.bpx_norm_act_fwd(dt, B, vox, L.tview(xd), rec.data_ptr(), code, L.tview(yb, extra, Cc), st))
    torch.cuda.synchronize()
    res = [_res(tag + ".fwd", relerr(yb[..., extra:], ndhwc(y_ref.detach())), tol_for(dt))]
    res.append(_res(tag + ".fwd.neighbours_untouched", 0 if (yb[..., :extra].float() == 3).all().item() else 1, 0))
    nt = lib.bpx_norm_act_tiles(dt, vox, Cc)
    red = torch.zeros(B, nt, 2, Cc, dtype=torch.float32, device=DEV)
    gbuf = torch.empty(B, D, H, W, Cc, dtype=tdtype(dt), device=DEV)
    L.check(lib.bpx_norm_act_bwd(dt, B, vox, L.tview(dyd), L.tview(xd), rec.data_ptr(), code, L.NULL_T, L.tview(gbuf), red.data_ptr(), st))
    coef = torch.empty(B, Cc, 4, dtype=torch.float32, device=DEV)
    dg, db = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    L.check(lib.bpx_norm_bwd_finalize(red.data_ptr(), B, nt, Cc, vox, rec.data_ptr(), gd.data_ptr(), dg.data_ptr(), db.data_ptr(), G_, coef.data_ptr(), st))
    L.check(lib.bpx_norm_bwd_apply(dt, B, vox, L.tview(gbuf), L.tview(xd), coef.data_ptr(), L.NULL_T, L.tview(gbuf), st))
    torch.cuda.synchronize()
    tol = 3e-2 if dt == L.BF16 else 2e-4
    res.append(_res(tag + ".dx", relerr(gbuf, ndhwc(xr.grad)), tol))
    res.append(_res(tag + ".dgamma", relerr(dg, gr.grad), tol))
    res.append(_res(tag + ".dbeta", relerr(db, br.grad), tol))
    return res


def check_resunet_variant(dtype, tag, golden):
    """ResUNet configurations that run on zero-padded 3x3x3 kernels - 2D, and 3D with MODEL.ISOTROPY False levels ((1,3,3)
    kernels) - against the reference fixture tests/golden/resunet_variants_golden.npz, through the module."""
    from biapy_amd.resunet import ResUNet

    return check_unet(dtype, tag, golden, cls=ResUNet, name="resunet_" + tag)


def check_unet(dtype, tag, golden, cls=None, name=None):
    """Plain U-Net (2D / 3D) against the reference fixture tests/golden/unet_golden.npz: logits, loss, every gradient norm and
    the stored full gradients, through the module (load_state_dict strict -> forward -> autograd backward)."""
    from biapy_amd.unet import U_Net

    cls = cls or U_Net
    tagd = {torch.bfloat16: "bf16", torch.float16: "mix16"}.get(dtype, "f32")
    fm = [int(v) for v in golden[f"{tag}/feature_maps"]]
    zd = [int(v) for v in golden[f"{tag}/z_down"]]
    pre = f"{tag}/sd/"
    sd = {k[len(pre):]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith(pre)}
    xl = torch.from_numpy(golden[f"{tag}/x"])
    nd = xl.dim() - 2
    x = xl.permute(0, nd + 1, *range(1, nd + 1)).contiguous()
    tgt = torch.from_numpy(golden[f"{tag}/target"]).float()
    iso = [bool(v) for v in golden[f"{tag}/isotropy"]] if f"{tag}/isotropy" in golden.files else [True] * len(fm)
    m = cls(image_shape=tuple(xl.shape[1:]), activation="elu", feature_maps=fm, drop_values=[0.0] * len(fm), normalization="in",
            yx_down=[2] * (len(fm) - 1), z_down=zd, isotropy=iso, larger_io=False, conv_layers=[2] * len(fm), compute_dtype=dtype)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train()
    logits = m(x.to(DEV))
    loss = F.binary_cross_entropy_with_logits(logits, tgt.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    name = f"{name or 'unet' + tag}[{tagd} fm={fm}]"
    lo_ref = torch.from_numpy(golden[f"{tag}/logits"])
    bf = dtype == torch.bfloat16
    mx = dtype == torch.float16                # the mixed mode: fp16 forward / activations (the forward bars of LOGITS_TOL / LOSS_TOL), bf16 gradients
    res = [_res(name + ".logits_rel", (logits.detach().cpu() - lo_ref).abs().max().item() / lo_ref.abs().max().item(), 6e-2 if bf else 8e-3 if mx else 2e-4)]
    res.append(_res(name + ".loss", abs(loss.item() - float(golden[f"{tag}/loss"])), 2e-2 if bf else 2e-3 if mx else 1e-5))
    gtol = 0.15 if bf else 0.10 if mx else 2e-3
    G = {k: p.grad for k, p in m.named_parameters()}
    worst, wname = 0.0, ""
    pre = f"{tag}/grad/"
    for k in golden.files:
        if k.startswith(pre):
            gr = torch.from_numpy(golden[k])
            e = (G[k[len(pre):]].cpu() - gr).norm().item() / (gr.norm().item() + 1e-12)
            if e > worst:
                worst, wname = e, k[len(pre):]
    res.append(_res(name + ".grads_rel_l2_worst", worst, gtol, extra=wname))
    worst, wname = 0.0, ""
    pre = f"{tag}/gradnorm/"
    gmax = max(float(golden[k]) for k in golden.files if k.startswith(pre))
    for k in golden.files:
        if k.startswith(pre):
            ref = float(golden[k])
            if ref > 1e-5 * gmax:
                e = abs(G[k[len(pre):]].norm().item() - ref) / ref
                if e > worst:
                    worst, wname = e, k[len(pre):]
    res.append(_res(name + ".gradnorm_rel_worst", worst, gtol, extra=wname))
    with torch.no_grad():
        pr = m.eval().predict_proba(x.to(DEV))
    res.append(_res(name + ".predict_proba", (pr.cpu() - torch.sigmoid(lo_ref)).abs().max().item(), 3e-2 if bf else 4e-3 if mx else 2e-5))
    return res


def check_unet_cfg1(dtype=torch.float32):
    """BASELINE.json configs[0]: 2D U-Net, 256x256x1 patches, batch 2, fm 16-32-64-128-256 (1,944,241 parameters) - one train
    step's logits, BCE loss and gradients on the device against the CPU oracle on the same seeded inputs and weights."""
    from biapy_amd.unet import U_Net
    from oracle import unet_oracle

    fm = [16, 32, 64, 128, 256]
    torch.manual_seed(21)
    m = U_Net(image_shape=(256, 256, 1), activation="elu", feature_maps=fm, drop_values=[0.0] * 5, normalization="in", yx_down=[2] * 4,
              z_down=[2] * 4, isotropy=[True] * 5, larger_io=False, conv_layers=[2] * 5, compute_dtype=dtype)
    nparams = sum(p.numel() for p in m.parameters())
    g = torch.Generator().manual_seed(22)
    x = torch.randn(2, 1, 256, 256, generator=g)
    tgt = (torch.rand(2, 1, 256, 256, generator=g) > 0.5).float()
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    lo_ref = unet_oracle.unet_forward(sd, x, fm)
    loss_ref = F.binary_cross_entropy_with_logits(lo_ref, tgt)
    loss_ref.backward()
    m = m.to(DEV).train()
    logits = m(x.to(DEV))
    loss = F.binary_cross_entropy_with_logits(logits, tgt.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    bf = dtype == torch.bfloat16
    name = f"unet2d_cfg1[{'bf16' if bf else 'f32'}]"
    res = [_res(name + ".params", abs(nparams - 1944241), 0)]
    res.append(_res(name + ".logits_rel", (logits.detach().cpu() - lo_ref.detach()).abs().max().item() / lo_ref.abs().max().item(), 6e-2 if bf else 3e-4))
    res.append(_res(name + ".loss", abs(loss.item() - loss_ref.item()), 2e-2 if bf else 1e-5))
    gmax = max(v.grad.norm().item() for v in sd.values())
    worst, wname = 0.0, ""
    for k, p_ in m.named_parameters():
        ref = sd[k].grad
        if ref.norm().item() > 1e-5 * gmax:
            e = (p_.grad.cpu() - ref).norm().item() / ref.norm().item()
            if e > worst:
                worst, wname = e, k
    res.append(_res(name + ".grads_rel_l2_worst", worst, 0.2 if bf else 3e-3, extra=wname))
    return res


def all_kernel_checks(golden_tiling=None, quick=False):
    out = []
    out += check_selftest()
    if golden_tiling is not None:
        out += check_tiling(golden_tiling)
    out += check_merge_sharded()
    for dt in (L.F32, L.BF16):
        out += check_conv3d_fwd(dt, 2, (8, 8, 16), 16, 16, norm=True, sc_C=0)
        out += check_conv3d_fwd(dt, 1, (8, 12, 20), 48, 16, norm=True, sc_C=48, slices=True)
        out += check_conv3d_fwd(dt, 2, (6, 8, 8), 32, 64, norm=False, sc_C=1)
        out += check_conv3d_fwd(dt, 1, (4, 4, 8), 64, 128, norm=True, sc_C=64)
        out += check_conv3d_fwd(dt, 1, (32, 32, 32), 16, 32, norm=True, sc_C=16)
        out += check_conv3d_dgrad(dt, 2, (8, 8, 16), 48, 16)
        out += check_conv3d_dgrad(dt, 1, (4, 8, 8), 32, 64)
        out += check_conv3d_wgrad(dt, 2, (8, 8, 16), 16, 16, k=3, norm=True)
        out += check_conv3d_wgrad(dt, 1, (8, 12, 20), 48, 32, k=3, norm=True)
        out += check_conv3d_wgrad(dt, 1, (4, 8, 8), 64, 64, k=3, norm=False)
        out += check_conv3d_wgrad(dt, 2, (8, 8, 16), 48, 16, k=1, norm=False)
        if dt == L.BF16:
            out += check_conv3d_wgrad(dt, 2, (8, 8, 16), 16, 16, k=3, norm=True, use_tr=0)
        out += check_conv1x1(dt, 2, 1000, 16, 48, with_coef=True)
        out += check_conv1x1(dt, 1, 300, 128, 384, with_coef=False)
        out += check_convT(dt, 2, (4, 6, 8), 32)
        out += check_convT(dt, 1, (2, 2, 2), 256)
        out += check_norm_pool_head(dt)
    return out


# ---------------------------------------------------------------------------------------------------
def check_sliding_window(dtype=torch.float32):
    """crop -> forward -> merge on the device vs the same pipeline built from the oracle pieces on the CPU."""
    from biapy_amd.resunet import ResUNet
    from biapy_amd.workflow import SlidingWindowPredictor

    fm = [16, 32]
    sd = net_oracle.init_state_dict(1, fm, seed=5)
    m = ResUNet(image_shape=(32, 32, 32, 1), activation="elu", feature_maps=fm, drop_values=[0.0, 0.0], normalization="in", yx_down=[2], z_down=[2],
                isotropy=[True, True], larger_io=False, conv_layers=[2, 2], compute_dtype=dtype)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    rs = np.random.RandomState(2)
    vol = rs.randn(48, 40, 56, 1).astype(np.float32)
    ov, pad = (0.5, 0.25, 0.5), (0, 4, 0)
    patch = (32, 32, 32)
    p, _ = TO.crop(vol, patch + (1,), ov, pad)
    with torch.no_grad():
        pr = torch.sigmoid(net_oracle.resunet_forward(sd, torch.from_numpy(p).permute(0, 4, 1, 2, 3), fm)).permute(0, 2, 3, 4, 1).contiguous().numpy()
    ref = TO.merge(pr, vol.shape, overlap=ov, padding=pad)
    if dtype == torch.float16:
        # the way it is used after bf16 training: the predictor switches the model to the fp16 inference mode and back
        m.compute_dtype = torch.bfloat16
        sw = SlidingWindowPredictor(m, patch, ov, pad, batch_size=5, compute_dtype=torch.float16)
    else:
        sw = SlidingWindowPredictor(m, patch, ov, pad, batch_size=5)
    got = sw.predict(torch.from_numpy(vol).cuda()).cpu().numpy()
    tagd, band, _ = _mode(dtype)
    res = [_res(f"sliding_window_prob[{tagd}]", np.abs(got - ref).max(), {"f32": 2e-5, "bf16": 3e-2, "f16": 4e-3}[tagd])]
    if dtype == torch.float16:
        res.append(_res("sliding_window[f16].model_dtype_restored", 0.0 if m.compute_dtype == torch.bfloat16 else 1.0, 0))
    lab_ref, lab_got = (ref > 0.5), (got > 0.5)
    near = np.abs(ref - 0.5) < band                                              # voxels whose label is decided by the last bits
    res.append(_res(f"sliding_window_labels_away_from_threshold[{tagd}]", int(((lab_ref != lab_got) & ~near).sum()), 0,
                    extra=f"undecidable voxels: {int(near.sum())} of {near.size}"))
    return res


def check_sliding_window_tta():
    """SlidingWindowPredictor(tta="full"): every patch through the 16-orientation ensemble, vs the oracle pipeline on the CPU."""
    from biapy_amd.resunet import ResUNet
    from biapy_amd.workflow import SlidingWindowPredictor
    from oracle import tta_oracle

    fm = [16, 32]
    sd = net_oracle.init_state_dict(1, fm, seed=6)
    m = ResUNet(image_shape=(16, 16, 16, 1), activation="elu", feature_maps=fm, drop_values=[0.0, 0.0], normalization="in", yx_down=[2], z_down=[2],
                isotropy=[True, True], larger_io=False, conv_layers=[2, 2], compute_dtype=torch.float32)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    vol = np.random.RandomState(3).randn(24, 16, 28, 1).astype(np.float32)
    ov, pad, patch = (0.25, 0.0, 0.5), (0, 0, 0), (16, 16, 16)
    p, _ = TO.crop(vol, patch + (1,), ov, pad)

    def f(b):                                                                      # (n, Z, Y, X, C) numpy -> probabilities
        with torch.no_grad():
            return torch.sigmoid(net_oracle.resunet_forward(sd, torch.from_numpy(np.ascontiguousarray(b)).permute(0, 4, 1, 2, 3), fm)).permute(0, 2, 3, 4, 1).contiguous().numpy()

    pr = np.stack([tta_oracle.ensemble(p[i], f, 3, mode="mean", level="full", batch_size_value=4) for i in range(p.shape[0])])
    ref = TO.merge(pr, vol.shape, overlap=ov, padding=pad)
    sw = SlidingWindowPredictor(m, patch, ov, pad, batch_size=3, tta="full", tta_mode="mean")
    got = sw.predict(torch.from_numpy(vol).cuda()).cpu().numpy()
    return [_res("sliding_window_tta_prob[f32]", np.abs(got - ref).max(), 2e-5)]


def check_dice_parity_trained(steps=120):
    """Train a small ResUNet on synthetic blobs with the MI355X engine in its default (benched) mode - fp16 forward, bf16 gradients -
    then compare Dice of the device forward in every storage mode with the fp32 CPU oracle using the SAME weights (north_star:
    |Dice delta| < 1e-4, asserted for f32 and fp16; bf16 storage makes no Dice claim)."""
    from biapy_amd.resunet import ResUNet

    fm = [16, 32, 64]
    torch.manual_seed(0)
    m = ResUNet(image_shape=(32, 32, 32, 1), activation="elu", feature_maps=fm, drop_values=[0.0] * 3, normalization="in", yx_down=[2, 2],
                z_down=[2, 2], isotropy=[True] * 3, larger_io=False, conv_layers=[2] * 3).cuda().train()
    assert m.compute_dtype == torch.float16
    opt = torch.optim.AdamW(m.parameters(), lr=2e-3)
    g = torch.Generator(device="cuda").manual_seed(1)

    def batch(B):
        n = torch.randn(B, 1, 32, 32, 32, generator=g, device="cuda")
        t = (F.avg_pool3d(n, 5, stride=1, padding=2) > 0.05).float()
        x = t * 1.5 + 0.8 * torch.randn(B, 1, 32, 32, 32, generator=g, device="cuda")       # noisy image of the blobs
        return x, t

    first = last = None
    for it in range(steps):
        x, t = batch(4)
        opt.zero_grad(set_to_none=True)
        loss = F.binary_cross_entropy_with_logits(m(x), t)
        loss.backward()
        opt.step()
        first = loss.item() if first is None else first
        last = loss.item()
    res = [_res("train_loss_decreases[fp16 forward / bf16 gradients]", last / first, 0.6, extra=f"loss {first:.4f} -> {last:.4f} in {steps} steps")]
    m.eval()
    x, t = batch(4)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        lo_ref = net_oracle.resunet_forward(sd, x.cpu(), fm)
    d_ref = net_oracle.dice(torch.sigmoid(lo_ref), t.cpu())
    del d_ref
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        m.compute_dtype = dtype
        with torch.no_grad():
            lo = m(x).cpu()
        tagd = _mode(dtype)[0]
        res += parity_rows(f"trained_model[{tagd}]", lo, lo_ref, t.cpu(), dtype, trained=True)
        res.append(_res(f"trained_model[{tagd}].logits_rel", ((lo - lo_ref).abs().max() / lo_ref.abs().max()).item(),
                        {"f32": 1e-5, "bf16": 3e-2, "f16": 3e-3}[tagd]))
    return res



def check_c1_wgrad_nb(mix=True, B=2, S=(12, 20, 36), seed=0):
    """bpx_conv3d_c1_wgrad_nb (dy = a*g + b*t + c0 formed inside the first layer's weight-gradient kernel) against bpx_norm_bwd_apply followed by
    bpx_conv3d_c1_wgrad - the same bits, the kernels share arithmetic and summation order - and against the fp64 expression."""
    D, H, W = S
    gen = torch.Generator().manual_seed(seed)
    img = torch.randn(B, D, H, W, generator=gen)
    gq = torch.randn(B, D, H, W, 16, generator=gen).to(torch.bfloat16)
    tq = (torch.randn(B, D, H, W, 16, generator=gen) * 2).to(torch.float16 if mix else torch.bfloat16)
    coef = torch.randn(B, 16, 4, generator=gen) * torch.tensor([1.0, 0.3, 0.1, 0.0])
    dt = L.MIX16 if mix else L.BF16
    imgd, gd, td, cd = img.to(DEV).contiguous(), gq.to(DEV), tq.to(DEV), coef.to(DEV).contiguous()
    ws = torch.empty(lib.bpx_conv3d_c1_wgrad_workspace(16), dtype=torch.uint8, device=DEV)
    res = []
    tag = f"c1_wgrad_nb[{'mix' if mix else 'bf16'} B{B} {S}]"
    res.append(_res(tag + ".supported", 0 if lib.bpx_conv3d_c1_wgrad_nb_supported(dt, W) else 1, 0))

    def fused():
        dw = torch.zeros(16, 1, 3, 3, 3, dtype=torch.float32, device=DEV); db = torch.zeros(16, dtype=torch.float32, device=DEV)
        L.check(lib.bpx_conv3d_c1_wgrad_nb(dt, B, D, H, W, imgd.data_ptr(), L.tview(gd), L.tview(td), cd.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                           ws.numel(), L.stream_ptr()))
        torch.cuda.synchronize()
        return dw, db

    dwf, dbf = fused()
    dwf2, dbf2 = fused()
    res.append(_res(tag + ".run_to_run_bits", 0 if torch.equal(dwf, dwf2) and torch.equal(dbf, dbf2) else 1, 0))
    # round 5: the pointer-addressed instance (hook bit 30) against the buffer-addressed default, with a workgroup cap so that a workgroup walks
    # several tile pairs and an odd last tile
    lib.bpx_debug_set_c1_persist(2048 | (1 << 30))
    try:
        dwp, dbp = fused()
    finally:
        lib.bpx_debug_set_c1_persist(2048)
    res.append(_res(tag + ".buffer_instance_bits_equal_pointer_instance", 0 if torch.equal(dwf, dwp) and torch.equal(dbf, dbp) else 1, 0,
                    extra=f"max diff {(dwf - dwp).abs().max().item():.2e}"))
    few = []
    for flag in (0, 1 << 30):
        lib.bpx_debug_set_c1_persist(7 | flag)          # 7 workgroups: tile pairs in a loop and an odd last tile per workgroup
        try:
            few.append(fused())
        finally:
            lib.bpx_debug_set_c1_persist(2048)
    res.append(_res(tag + ".seven_workgroups.buffer_bits_equal_pointer", 0 if torch.equal(few[0][0], few[1][0]) and torch.equal(few[0][1], few[1][1]) else 1, 0))
    res.append(_res(tag + ".seven_workgroups.close_to_default_grid", relerr(few[0][0], dwf), 1e-5))
    dyd = torch.empty_like(gd)
    L.check(lib.bpx_norm_bwd_apply(dt, B, D * H * W, L.tview(gd), L.tview(td), cd.data_ptr(), L.NULL_T, L.tview(dyd), L.stream_ptr()))
    dws = torch.zeros(16, 1, 3, 3, 3, dtype=torch.float32, device=DEV); dbs = torch.zeros(16, dtype=torch.float32, device=DEV)
    L.check(lib.bpx_conv3d_c1_wgrad(L.BF16, B, D, H, W, imgd.data_ptr(), L.tview(dyd), dws.data_ptr(), dbs.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr()))
    torch.cuda.synchronize()
    res.append(_res(tag + ".same_bits_as_apply_then_wgrad", 0 if torch.equal(dwf, dws) and torch.equal(dbf, dbs) else 1, 0, extra=f"max diff {(dwf - dws).abs().max().item():.2e}"))
    dy = coef[:, None, None, None, :, 0].double() * gq.double() + coef[:, None, None, None, :, 1].double() * tq.double() + coef[:, None, None, None, :, 2].double()
    w = torch.zeros(16, 1, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    bb = torch.zeros(16, dtype=torch.float64, requires_grad=True)
    F.conv3d(img[:, None].double(), w, bb, padding=1).backward(ncdhw(dy))
    res.append(_res(tag + ".dw_vs_fp64", relerr(dwf, w.grad), 6e-3))      # dy is rounded to bf16 on the way to the MFMA operand, as the stored tensor was
    res.append(_res(tag + ".db_vs_fp64", relerr(dbf, bb.grad), 6e-3))
    return res


def check_fused_adam(seed=0):
    """optim.fused_step (bpx_adam_step) against torch.optim.Adam / AdamW (fused, capturable) on the same tensors: parameters and both moments after
    four steps, ragged sizes (1 ... 1.7 M elements, an unaligned view), lr as a device scalar that changes between steps; and the refusals."""
    from biapy_amd import optim as O
    res = []
    sizes = [(16,), (1,), (16, 1, 3, 3, 3), (256, 256, 3, 3, 3), (5, 7), (48, 16, 1, 1, 1), (4099,)]
    # torch's DEFAULT betas (0.9, 0.999) in two of the three cases: 0.999 is where a float hyper-parameter differs from the double torch uses
    # (1 - beta2 off by 1.3e-5 relative); the third keeps the round-4 setting
    for cls, wd, betas in ((torch.optim.AdamW, 1e-2, (0.9, 0.999)), (torch.optim.Adam, 1e-3, (0.9, 0.999)), (torch.optim.AdamW, 0.0, (0.9, 0.99))):
        gen = torch.Generator().manual_seed(seed)
        base = [torch.randn(*s, generator=gen) for s in sizes]
        slab = torch.zeros(sum(b.numel() for b in base) + 3, device=DEV)          # gradients as (partly unaligned) views of one slab, as in training
        pa = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
        pb = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
        oa = cls(pa, lr=torch.tensor(1e-2, device=DEV), weight_decay=wd, fused=True, capturable=True, betas=betas)
        ob = cls(pb, lr=torch.tensor(1e-2, device=DEV), weight_decay=wd, fused=True, capturable=True, betas=betas)
        used = []
        for it in range(4):
            off = 3 if it % 2 else 0
            for a, b in zip(pa, pb):
                gr = torch.randn(a.shape, generator=gen).to(DEV)
                a.grad = gr.clone()
                view = slab[off:off + a.numel()].view_as(a)
                view.copy_(gr)
                b.grad = view
                off += a.numel()
            oa.step()
            used.append(O.fused_step(ob))
            if not used[-1]:
                ob.step()                                                           # the first step initialises the state: torch's own
            for o in (oa, ob):
                o.param_groups[0]["lr"].mul_(0.7)
        torch.cuda.synchronize()
        tag = f"fused_adam[{cls.__name__} wd={wd} betas={betas}]"
        res.append(_res(tag + ".used_from_step_2", 0 if used == [False, True, True, True] else 1, 0, extra=str(used)))
        worst = {"p": 0.0, "m": 0.0, "v": 0.0, "step": 0.0}
        for a, b in zip(pa, pb):
            sa, sb = oa.state[a], ob.state[b]
            worst["p"] = max(worst["p"], relerr(b, a)); worst["m"] = max(worst["m"], relerr(sb["exp_avg"], sa["exp_avg"]))
            worst["v"] = max(worst["v"], relerr(sb["exp_avg_sq"], sa["exp_avg_sq"]))
            worst["step"] = max(worst["step"], abs(float(sa["step"]) - float(sb["step"])))
        for k, v in worst.items():
            res.append(_res(f"{tag}.{k}", v, 0 if k == "step" else 2e-6))
    # refusals: nothing is touched, the caller runs torch's step
    q = [torch.nn.Parameter(torch.randn(8, device=DEV))]
    q[0].grad = torch.randn(8, device=DEV)
    for name, o in (("sgd", torch.optim.SGD(q, lr=0.1)), ("not capturable", torch.optim.AdamW(q, lr=0.1)),
                    ("amsgrad", torch.optim.AdamW(q, lr=0.1, amsgrad=True, capturable=True))):
        o.step()
        before = q[0].detach().clone()
        took = O.fused_step(o)
        res.append(_res(f"fused_adam.refuses[{name}]", 0 if (not took and torch.equal(before, q[0])) else 1, 0))
    return res


def _blob_batch(B, S, gen):
    """bench.py-style synthetic sample: smooth blobs (~50 % foreground) and a noisy image of them (CPU tensors)."""
    tgt = (F.avg_pool3d(torch.randn(B, 1, S, S, S, generator=gen), 7, stride=1, padding=3) > 0.0).float()
    return tgt * 1.2 + 0.8 * torch.randn(B, 1, S, S, S, generator=gen), tgt


def check_dice_benched_arch(model=None, steps=30, S=64, big=128, seed=11):
    """the north-star Dice bar on the BENCHED architecture (five levels, 16 ... 256) in the BENCHED forward mode (fp16
    storage and MFMAs), not on a three-level toy net: a model trained in the mixed mode (the caller's, or `steps` AdamW steps at S^3 here), then
    the device forward against the fp32 CPU oracle on the SAME trained weights on held-out batches - one at S^3 and one at the benched
    `big`^3 x B = 1 shape.  |Dice delta| < 1e-4 and the label rows through parity_rows(trained=True); logits error recorded beside them."""
    from biapy_amd.resunet import ResUNet

    fm = [16, 32, 64, 128, 256]
    if model is None:
        torch.manual_seed(5)
        model = ResUNet(image_shape=(S, S, S, 1), activation="elu", feature_maps=fm, drop_values=[0.0] * 5, normalization="in", yx_down=[2] * 4,
                        z_down=[2] * 4, isotropy=[True] * 5, larger_io=False, conv_layers=[2] * 5, compute_dtype=torch.float16).cuda().train()
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
        g = torch.Generator().manual_seed(9)
        batches = [_blob_batch(1, S, g) for _ in range(3)]
        for it in range(steps):
            x, t = batches[it % 3]
            opt.zero_grad(set_to_none=True)
            F.binary_cross_entropy_with_logits(model(x.cuda()), t.cuda()).backward()
            opt.step()
    assert model.compute_dtype == torch.float16
    was_training = model.training
    model.eval()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(seed)
    res = []
    for size in (S, big):
        x, t = _blob_batch(1, size, g)                        # held out: never seen by the training loop
        with torch.no_grad():
            lo = model(x.cuda()).cpu()
            lo_ref = net_oracle.resunet_forward(sd, x, fm)
        tag = f"trained_cfg2_arch[f16 fm={fm} {size}^3 B=1]"
        res += parity_rows(tag, lo, lo_ref, t, torch.float16, trained=True)
        res.append(_res(tag + ".logits_rel", ((lo - lo_ref).abs().max() / lo_ref.abs().max()).item(), LOGITS_TOL["f16"],
                        extra=f"dice_ref={net_oracle.dice(torch.sigmoid(lo_ref), t):.6f} fg={t.mean().item():.3f}"))
    model.train(was_training)
    return res


def check_norm_bwd_finalize_deferred(N=4, tiles=768, Cc=16, groups=None, seed=0):
    """bpx_norm_bwd_finalize_deferred inside a bpx_wgrad_defer_begin / _flush window (one block per sample, dgamma / dbeta summed at the flush)
    against bpx_norm_bwd_finalize and against the fp64 formulas; bit-reproducible; outside a window it is the plain entry."""
    gen = torch.Generator().manual_seed(seed)
    part = torch.randn(N, tiles, 2, Cc, generator=gen)
    rec = make_recs(N, Cc, seed + 1)[0]
    gamma = torch.randn(Cc, generator=gen)
    count = 4096
    G = groups or Cc
    res = []
    tag = f"norm_bwd_finalize_deferred[N{N} tiles{tiles} C{Cc} g{G}]"

    def run(deferred, window):
        pd = part.to(DEV).clone()
        slab = torch.zeros(2 * Cc, device=DEV)                       # dgamma | dbeta adjacent, as in the engine's gradient slab
        coef = torch.zeros(N, Cc, 4, device=DEV)
        if window:
            L.check(lib.bpx_wgrad_defer_begin())
        fn = lib.bpx_norm_bwd_finalize_deferred if deferred else lib.bpx_norm_bwd_finalize
        L.check(fn(pd.data_ptr(), N, tiles, Cc, count, rec.to(DEV).data_ptr(), gamma.to(DEV).data_ptr(), slab.data_ptr(), slab[Cc:].data_ptr(), G, coef.data_ptr(),
                   L.stream_ptr()))
        if window:
            L.check(lib.bpx_wgrad_defer_flush(L.stream_ptr()))
        torch.cuda.synchronize()
        return coef.cpu(), slab.cpu()

    c0, s0 = run(False, False)
    c1, s1 = run(True, True)
    c2, s2 = run(True, True)
    c3, s3 = run(True, False)
    res.append(_res(tag + ".coef_vs_plain", relerr(c1[..., :3], c0[..., :3]), 2e-6))
    res.append(_res(tag + ".dgamma_dbeta_vs_plain", relerr(s1, s0), 2e-6))
    res.append(_res(tag + ".run_to_run_bits", 0 if torch.equal(c1, c2) and torch.equal(s1, s2) else 1, 0))
    res.append(_res(tag + ".outside_a_window_is_the_plain_entry", 0 if torch.equal(c3, c0) and torch.equal(s3, s0) else 1, 0))
    S = part.double().sum(1)                                          # (N, 2, C)
    res.append(_res(tag + ".dbeta_fp64", relerr(s1[Cc:], S[:, 0].sum(0)), 1e-5))
    res.append(_res(tag + ".dgamma_fp64", relerr(s1[:Cc], S[:, 1].sum(0)), 1e-5))
    return res


def check_wgrad_k1_stream(mix=True, B=2, S=(32, 32, 32), Cin=48, Cout=16, planar=False, seed=0):
    """The streaming k = 1 weight gradient of a raw input (the residual blocks' shortcut at the 128^3 / 64^3 levels): against the fp64 sum, against
    the generic tile kernel (bpx_debug_set_wgrad_k1(0)), run to run bits; fp16 x (mixed mode) and chunk-planar x (the decoder's concat buffer)."""
    D, H, W = S
    gen = torch.Generator().manual_seed(seed)
    xdt = torch.float16 if mix else torch.bfloat16
    xq = torch.randn(B, D, H, W, Cin, generator=gen).to(xdt)
    dyq = torch.randn(B, D, H, W, Cout, generator=gen).to(torch.bfloat16)
    ref = torch.einsum("bdhwi,bdhwo->oi", xq.double(), dyq.double())
    dt = L.MIX16 if mix else L.BF16
    xd = xq.to(DEV)
    xp = L.Planar(B, S, Cin, xdt, DEV).copy_from_dense(xd) if planar else None      # (kept alive: tview holds only the address)
    xv = L.tview(xp) if planar else L.tview(xd)
    dyd = dyq.to(DEV)
    ws = torch.empty(max(1, lib.bpx_conv3d_wgrad_workspace(B, D, H, W, Cin, Cout, 1)), dtype=torch.uint8, device=DEV)

    def run():
        dw = torch.full((Cout, Cin, 1, 1, 1), 7.0, dtype=torch.float32, device=DEV)
        L.check(lib.bpx_conv3d_wgrad(dt, B, D, H, W, xv, None, 0, L.tview(dyd), 1, dw.data_ptr(), None, ws.data_ptr(), ws.numel(), L.stream_ptr()))
        torch.cuda.synchronize()
        return dw.view(Cout, Cin)

    tag = f"wgrad_k1_stream[{'mix' if mix else 'bf16'} B{B} {S} {Cin}.{Cout} planar={int(planar)}]"
    a, b = run(), run()
    lib.bpx_debug_set_wgrad_k1(0)
    try:
        c = run()
    finally:
        lib.bpx_debug_set_wgrad_k1(1)
    # bf16 MFMA operands: in the mixed mode x is rounded fp16 -> bf16 on the way in (both kernels), so the fp64 sum of the fp16 values is ~2^-9 away
    return [_res(tag + ".vs_fp64", relerr(a, ref), 4e-3 if mix else 1e-4), _res(tag + ".vs_tile_kernel", relerr(a, c), 1e-4),
            _res(tag + ".run_to_run_bits", 0 if torch.equal(a, b) else 1, 0)]


def check_pw_stream(mix=True, B=2, vps=131072, K=16, planar=True, seed=0):
    """bpx_conv1x1_fwd_split with the IN-backward affine at the large levels (the decoder blocks' input gradient): the streaming kernel against the
    tile kernel (bpx_debug_set_pw_stream(0)) - the same arithmetic: equal bits - and against the fp32 expression; t fp16 (mixed mode) / planar."""
    gen = torch.Generator().manual_seed(seed)
    C3 = 3 * K
    tdt = torch.float16 if mix else torch.bfloat16
    x = torch.randn(B, vps, K, generator=gen).to(torch.bfloat16)
    w = torch.randn(C3, K, generator=gen) / K ** 0.5
    gg = torch.randn(B, vps, C3, generator=gen).to(torch.bfloat16)
    tt = (torch.randn(B, vps, C3, generator=gen) * 2).to(tdt)
    coef = torch.randn(B, C3, 4, generator=gen) * torch.tensor([1.0, 0.3, 0.1, 0.0])
    y_ref = x.float() @ w.to(torch.bfloat16).float().t() + coef[:, None, :, 0] * gg.float() + coef[:, None, :, 1] * tt.float() + coef[:, None, :, 2]
    dt = L.MIX16 if mix else L.BF16
    wp = pack(w.view(C3, K, 1, 1, 1), L.PK_DENSE, K, C3, L.BF16)
    xd, gd, td, cd = x.to(DEV), gg.to(DEV), tt.to(DEV), coef.to(DEV).contiguous()
    S = (vps // 1024, 32, 32)
    tp = L.Planar(B, S, C3, tdt, DEV).copy_from_dense(td.view(B, *S, C3)) if planar else None      # (kept alive: tview holds only the address)
    tv = L.tview(tp) if planar else L.tview(td)
    lo = 2 * K

    def run():
        y_lo = torch.full((B, vps, lo), 7.0, dtype=torch.bfloat16, device=DEV)
        y_hi = torch.full((B, vps, C3 - lo), 7.0, dtype=torch.bfloat16, device=DEV)
        L.check(lib.bpx_conv1x1_fwd_split(dt, B, vps, L.tview(xd), wp.data_ptr(), None, L.tview(gd), tv, cd.data_ptr(), L.NULL_T, L.tview(y_lo), L.tview(y_hi),
                                          L.stream_ptr()))
        torch.cuda.synchronize()
        return torch.cat([y_lo, y_hi], -1)

    tag = f"pw_stream[{'mix' if mix else 'bf16'} B{B} v{vps} K{K} planar={int(planar)}]"
    a, b = run(), run()
    lib.bpx_debug_set_pw_stream(0)
    try:
        c = run()
    finally:
        lib.bpx_debug_set_pw_stream(1)
    extra = []
    need = int(lib.bpx_conv1x1_fwd_split_wgrad_workspace(dt, B, vps, K))
    if need > 0:
        # round 6: the same pass with the block's shortcut weight gradient riding along: the outputs keep their bits, dWsc[co][ci] = sum_v t[v][ci] dOut[v][co]
        # against the fp64 sum, against the k = 1 weight-gradient kernel it replaces, and run to run
        def run_wg():
            y_lo = torch.full((B, vps, lo), 7.0, dtype=torch.bfloat16, device=DEV)
            y_hi = torch.full((B, vps, C3 - lo), 7.0, dtype=torch.bfloat16, device=DEV)
            dw = torch.full((K, C3), 7.0, dtype=torch.float32, device=DEV)
            wsw = torch.empty(need, dtype=torch.uint8, device=DEV)
            L.check(lib.bpx_conv1x1_fwd_split_wgrad(dt, B, vps, L.tview(xd), wp.data_ptr(), L.tview(gd), tv, cd.data_ptr(), L.tview(y_lo), L.tview(y_hi), dw.data_ptr(),
                                                    wsw.data_ptr(), wsw.numel(), L.stream_ptr()))
            torch.cuda.synchronize()
            return torch.cat([y_lo, y_hi], -1), dw

        (ya, dwa), (_, dwb) = run_wg(), run_wg()
        dw_ref = torch.einsum("bvk,bvc->kc", x.double(), tt.double())
        dwk = torch.full((K, C3), 7.0, dtype=torch.float32, device=DEV)
        wsk = torch.empty(lib.bpx_conv3d_wgrad_workspace(B, S[0], S[1], S[2], C3, K, 1), dtype=torch.uint8, device=DEV)
        L.check(lib.bpx_conv3d_wgrad(dt, B, S[0], S[1], S[2], tv, None, 0, L.tview(xd), 1, dwk.data_ptr(), None, wsk.data_ptr(), wsk.numel(), L.stream_ptr()))
        torch.cuda.synchronize()
        extra = [_res(tag + ".with_wgrad.same_output_bits", 0 if torch.equal(ya.view(torch.int16), a.view(torch.int16)) else 1, 0),
                 _res(tag + ".with_wgrad.dw_vs_fp64", relerr(dwa, dw_ref), 4e-3 if mix else 1e-4),
                 _res(tag + ".with_wgrad.dw_vs_k1_kernel", relerr(dwa, dwk), 1e-4),
                 _res(tag + ".with_wgrad.run_to_run_bits", 0 if torch.equal(dwa, dwb) else 1, 0)]
    return extra + [_res(tag + ".vs_fp32", relerr(a, y_ref), 1.5e-2), _res(tag + ".same_bits_as_tile_kernel", 0 if torch.equal(a.view(torch.int16), c.view(torch.int16)) else 1, 0,
                                                                   extra=f"max diff {(a.float() - c.float()).abs().max().item():.2e}"),
            _res(tag + ".run_to_run_bits", 0 if torch.equal(a.view(torch.int16), b.view(torch.int16)) else 1, 0)]


def _dropout_fixture_masks(golden):
    out = {}
    for k in golden.files:
        if k.startswith("mask/"):
            name = k[5:]
            shape = tuple(int(v) for v in golden[f"mask_shape/{name}"])
            n = int(np.prod(shape))
            out[name] = (float(golden[f"p/{name}"]), torch.from_numpy(np.unpackbits(golden[k])[:n].reshape(shape).astype(bool)))
    return out


def _dropout_sites(depth):
    """engine site index -> block prefix of the reference module tree"""
    s = {i: f"down_path.{i}" for i in range(depth)}
    s[depth] = "bottleneck"
    for j in range(depth):
        s[depth + 1 + j] = f"up_paths.0.{j}.conv_block"
    return s


def check_network_dropout(dtype, golden):
    """MODEL.DROPOUT_VALUES > 0 on the device.  (i) With the reference's own masks given to the kernels (mask mode 1): logits, loss, gradient norms
    and six full gradients of the REFERENCE's training-mode step (resunet_dropout_golden.npz).  (ii) With the device's random stream (mask mode 2
    records what was drawn): keep rates, a new mask per forward, forward and backward agree on the mask (the CPU oracle given the recorded
    masks reproduces logits and gradients), evaluation mode ignores dropout."""
    tagd = _mode(dtype)[0]
    fm = [int(v) for v in golden["feature_maps"]]
    depth = len(fm) - 1
    drops = [float(v) for v in golden["drop_values"]]
    sd = {k[3:]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith("sd/")}
    x = torch.from_numpy(golden["x"]).permute(0, 4, 1, 2, 3).contiguous()
    tgt = torch.from_numpy(golden["target"]).float()
    masks = _dropout_fixture_masks(golden)
    sites = _dropout_sites(depth)
    P = {k: v.to(DEV) for k, v in sd.items()}
    tag = f"resunet_dropout[{tagd}]"
    res = []

    def step(eng):
        logits, ctx = eng.forward(P, x.to(DEV), head_act=0, save=True)
        lg = logits.detach().clone().requires_grad_(True)
        loss = F.binary_cross_entropy_with_logits(lg, tgt.to(DEV))
        loss.backward()
        G = eng.backward(P, ctx, lg.grad)
        torch.cuda.synchronize()
        return logits, loss, G

    # (i) the reference's masks
    eng = ResUNetEngine(NetConfig(in_ch=1, feature_maps=fm, dropout=drops[:depth] + [drops[-1]]), dtype)
    eng.drop_active = True
    eng.drop_mask_mode = 1
    eng.drop_mask_io = {s: masks[pre][1].permute(0, 2, 3, 4, 1).contiguous().view(-1).to(torch.uint8).to(DEV) for s, pre in sites.items()}
    logits, loss, G = step(eng)
    lo_ref = torch.from_numpy(golden["logits"])
    res += [_res(tag + ".ref_masks.logits_rel", (logits.cpu() - lo_ref).abs().max().item() / lo_ref.abs().max().item(), LOGITS_TOL[tagd]),
            _res(tag + ".ref_masks.loss", abs(loss.item() - float(golden["loss"])), LOSS_TOL[tagd])]
    gmax = max(float(golden[k]) for k in golden.files if k.startswith("gradnorm/"))
    floor = (GRAD_FLOOR_F32 if dtype == torch.float32 else GRAD_FLOOR_BF16) * gmax
    worst, wname = 0.0, ""
    for k in golden.files:
        if k.startswith("gradnorm/"):
            ref = float(golden[k])
            e = abs(G[k[9:]].norm().item() - ref) / max(ref, floor)
            if e > worst:
                worst, wname = e, k[9:]
    res.append(_res(tag + ".ref_masks.grad_norms_rel_worst", worst, GRAD_TOL[tagd], extra=wname))
    worst, wname = 0.0, ""
    for k in golden.files:
        if k.startswith("grad/"):
            ref = torch.from_numpy(golden[k])
            e = (G[k[5:]].cpu() - ref).norm().item() / max(ref.norm().item(), 1e-6 * gmax)
            if e > worst:
                worst, wname = e, k[5:]
    res.append(_res(tag + ".ref_masks.full_grads_rel_l2_worst", worst, GRAD_TOL[tagd], extra=wname))

    # (ii) the device's own stream
    eng2 = ResUNetEngine(NetConfig(in_ch=1, feature_maps=fm, dropout=drops[:depth] + [drops[-1]]), dtype)
    eng2.drop_active = True
    eng2.drop_mask_mode = 2
    logits_a, loss_a, G_a = step(eng2)
    drawn_a = {s: m.clone() for s, m in eng2.drop_mask_io.items()}
    worst = 0.0
    for s, m in drawn_a.items():
        p = eng2.cfg.dropout[s if s <= depth else depth - 1 - (s - depth - 1)]
        n = m.numel()
        z = abs(m.float().mean().item() - (1 - p)) / ((p * (1 - p) / n) ** 0.5)
        worst = max(worst, z)
    res.append(_res(tag + ".keep_rate_sigmas_worst", worst, 5.0))
    from oracle import net_oracle
    B = x.shape[0]

    def as_ncdhw(s, m):
        C = fm[s] if s <= depth else fm[depth - 1 - (s - depth - 1)]
        S = tuple(int(v) >> (s if s <= depth else depth - 1 - (s - depth - 1)) for v in x.shape[2:])
        return m.view(B, *S, C).permute(0, 4, 1, 2, 3).bool().cpu()

    dm = {sites[s]: (eng2.cfg.dropout[s if s <= depth else depth - 1 - (s - depth - 1)], as_ncdhw(s, m)) for s, m in drawn_a.items()}
    sdr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    lo = net_oracle.resunet_forward(sdr, x, fm, dropout=dm)
    lref = F.binary_cross_entropy_with_logits(lo, tgt)
    lref.backward()
    res.append(_res(tag + ".own_masks.logits_vs_oracle", (logits_a.cpu() - lo.detach()).abs().max().item() / lo.detach().abs().max().item(), LOGITS_TOL[tagd]))
    gm = max(v.grad.norm().item() for v in sdr.values())
    worst, wname = 0.0, ""
    for kname, v in sdr.items():
        if v.grad is None or kname not in G_a:
            continue
        e = (G_a[kname].cpu() - v.grad).norm().item() / max(v.grad.norm().item(), (1e-3 if dtype == torch.float32 else 5e-2) * gm)
        if e > worst:
            worst, wname = e, kname
    res.append(_res(tag + ".own_masks.grads_vs_oracle_rel_l2_worst", worst, GRAD_TOL[tagd], extra=wname))
    eng2.drop_mask_io = None
    logits_b, _, _ = step(eng2)
    same = all(torch.equal(drawn_a[s], eng2.drop_mask_io[s]) for s in drawn_a)
    res.append(_res(tag + ".new_mask_every_forward", 1 if same else 0, 0))
    eng2.drop_active = False
    eng2.drop_mask_mode = 0
    lo_eval, _ = eng2.forward(P, x.to(DEV), head_act=0, save=False)
    torch.cuda.synchronize()
    le = torch.from_numpy(golden["logits_eval"])
    res.append(_res(tag + ".eval_mode_ignores_dropout", (lo_eval.cpu() - le).abs().max().item() / le.abs().max().item(), LOGITS_TOL[tagd]))
    return res


def check_convT_wgrad_stream(mix=True, B=2, S=(32, 32, 32), Cc=32, seed=0):
    """The streaming transposed-conv weight gradient (wgrad_ct_dma_kernel, the 32 -> 32 / 64 -> 64 levels) against the fp64 sums, against the tile
    kernel (bpx_debug_set_wgrad_k1(3): streaming k = 1 on, streaming transposed-conv off) and run to run; x fp16 in the mixed mode, bias gradient included."""
    D, H, W = S
    gen = torch.Generator().manual_seed(seed)
    xdt = torch.float16 if mix else torch.bfloat16
    xq = torch.randn(B, D, H, W, Cc, generator=gen).to(xdt)
    dyq = torch.randn(B, 2 * D, 2 * H, 2 * W, Cc, generator=gen).to(torch.bfloat16)
    w = torch.zeros(Cc, Cc, 2, 2, 2, dtype=torch.float64, requires_grad=True)
    bb = torch.zeros(Cc, dtype=torch.float64, requires_grad=True)
    F.conv_transpose3d(ncdhw(xq.double()), w, bb, stride=2).backward(ncdhw(dyq.double()))
    dt = L.MIX16 if mix else L.BF16
    xd, dyd = xq.to(DEV), dyq.to(DEV)
    ws = torch.empty(max(1, lib.bpx_convT3d_k2s2_wgrad_workspace(B, D, H, W, 2, Cc, Cc)), dtype=torch.uint8, device=DEV)

    def run():
        dw = torch.full((Cc, Cc, 2, 2, 2), 7.0, dtype=torch.float32, device=DEV)
        db = torch.zeros(Cc, dtype=torch.float32, device=DEV)
        L.check(lib.bpx_convT3d_k2s2_wgrad(dt, B, D, H, W, 2, L.tview(xd), L.tview(dyd), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr()))
        torch.cuda.synchronize()
        return dw, db

    tag = f"convT_wgrad_stream[{'mix' if mix else 'bf16'} B{B} {S} C{Cc}]"
    lib.bpx_debug_set_wgrad_k1(7)            # every streaming instance, incl. the 32 -> 32 one that is off by default
    (a, ab), (b, bbias) = run(), run()
    lib.bpx_debug_set_wgrad_k1(3)
    try:
        c, cb = run()
    finally:
        lib.bpx_debug_set_wgrad_k1(1)
    return [_res(tag + ".dw_vs_fp64", relerr(a, w.grad), 4e-3 if mix else 1e-4), _res(tag + ".db_vs_fp64", relerr(ab, bb.grad), 1e-4),
            _res(tag + ".dw_vs_tile_kernel", relerr(a, c), 1e-4), _res(tag + ".db_vs_tile_kernel", relerr(ab, cb), 1e-4),
            _res(tag + ".run_to_run_bits", 0 if torch.equal(a, b) and torch.equal(ab, bbias) else 1, 0)]


# ---------------------------------------------------------------------------------------------------
def check_rcan_upscale_train(scale, dtype, group, seed=None):
    """Round 4: training through rcan(upscaling_layer=True) in 3-D - a short trunk + conv(16 -> 16 s^3) + 3-D pixel shuffle + last conv on a 32^3 patch:
    output, MSE loss and EVERY parameter gradient against autograd through the oracle's restatement (oracle/rcan_oracle.py, fp32 on the CPU; the
    shuffle's semantics are DEFINED there, the reference's own 3-D branch raises).  `group`: sub-positions per backward kernel call of the stage.
    A wrong sub-position order shows as a relative error of ~1.4 on upscale.0.weight and on everything in front of it."""
    import torch.nn.functional as F

    from biapy_amd.rcan import rcan
    from oracle import rcan_oracle

    seed = 10 + scale if seed is None else seed
    torch.manual_seed(seed)
    m = rcan(ndim=3, num_channels=1, filters=16, scale=scale, num_rg=1, num_rcab=2, reduction=16, upscaling_layer=True, out_channels=1,
             head_activations=["linear"], compute_dtype=dtype)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for v in m.state_dict().values():
            if v.ndim == 1:
                v.add_(0.1 * (torch.rand(v.shape, generator=g) * 2 - 1))
    x = torch.randn(1, 1, 32, 32, 32, generator=torch.Generator().manual_seed(19))
    tgt = torch.randn(1, 1, 32 * scale, 32 * scale, 32 * scale, generator=torch.Generator().manual_seed(20))
    ref = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    want = rcan_oracle.rcan_forward(ref, x, 1, 2, scale=scale)
    lw = F.mse_loss(want, tgt)
    lw.backward()
    m = m.cuda().train()
    m.engine().up_group = group
    got = m(x.cuda())
    lg = F.mse_loss(got, tgt.cuda())
    lg.backward()
    torch.cuda.synchronize()
    tag = f"rcan_x{scale}[{'mix16' if dtype == torch.float16 else 'bf16'} group={group}]"
    res = [_res(f"{tag}.output_rel_max", ((got.detach().cpu() - want.detach()).abs().max() / want.detach().abs().max()).item(), 1.5e-2),
           _res(f"{tag}.loss_rel", abs(lg.item() - lw.item()) / lw.item(), 1e-3)]
    gmax = max(v.grad.norm().item() for v in ref.values())
    errs = {}
    for k, p_ in m.named_parameters():
        gr = ref[k].grad
        if gr.norm().item() > 1e-4 * gmax:
            errs[k] = ((p_.grad.cpu() - gr).norm() / gr.norm()).item()
    stage_keys = ("upscale.0.weight", "upscale.0.bias", "conv2.weight", "conv2.bias", "conv1.weight")
    for k in stage_keys + ("sf.weight",):
        res.append(_res(f"{tag}.grad_rel_l2[{k}]", errs.get(k, float("nan")), 0.03 if k in stage_keys else 0.05))
    worst = max(errs, key=errs.get)
    res.append(_res(f"{tag}.grads_rel_l2_worst", errs[worst], 0.05, f"{worst} ({len(errs)} tensors)"))   # bars: ~3x the recorded worst values (profiles/r04_gpu_diag_rcan_upscale.txt: 0.010 / 0.006)
    return res


# ---------------------------------------------------------------------------------------------------
def check_network_padded_widths(dtype, fm=(52, 68, 84), patch=(8, 32, 32), zd=(1, 1), B=2, seed=5):
    """MODEL.FEATURE_MAPS that are not multiples of 16 (the reference's CartoCell template: [52, 68, 84], Z_DOWN [1, 1]) through the MODULE: the parameters keep
    the reference's shapes (strict load of a true-width state dict), the engine runs them zero-padded to [64, 80, 96] and hands back gradients in the
    parameters' shapes; the 64-wide first level also takes the wide head.  Against the CPU oracle on the TRUE widths: logits, BCE loss, every gradient."""
    from biapy_amd.resunet import ResUNet

    tagd = _mode(dtype)[0]
    fm, zd = list(fm), list(zd)
    sd = net_oracle.init_state_dict(1, fm, z_down=zd, seed=seed)
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        for k, v in sd.items():
            if v.dim() == 1:
                v.add_(0.1 * (torch.rand(v.shape, generator=g) * 2 - 1))
    x = torch.randn(B, 1, *patch, generator=g)
    tgt = (torch.rand(B, 1, *patch, generator=g) > 0.5).float()
    m = ResUNet(image_shape=tuple(patch) + (1,), activation="elu", feature_maps=fm, drop_values=[0.0] * len(fm), normalization="in", yx_down=[2] * (len(fm) - 1),
                z_down=zd, isotropy=[True] * len(fm), larger_io=False, conv_layers=[2] * len(fm), compute_dtype=dtype)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train()
    logits = m(x.to(DEV))
    loss = F.binary_cross_entropy_with_logits(logits, tgt.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    ref = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    lo_ref = net_oracle.resunet_forward(ref, x, fm, z_down=zd)
    l_ref = F.binary_cross_entropy_with_logits(lo_ref, tgt)
    l_ref.backward()
    tag = f"resunet_padded[{tagd} fm={fm} -> {list(m.cfg.feature_maps)} {tuple(x.shape)}]"
    bf, mx = dtype == torch.bfloat16, dtype == torch.float16
    res = [_res(tag + ".logits_rel", (logits.detach().cpu() - lo_ref.detach()).abs().max().item() / lo_ref.detach().abs().max().item(), 6e-2 if bf else 8e-3 if mx else 2e-4),
           _res(tag + ".loss", abs(loss.item() - l_ref.item()), 2e-2 if bf else 2e-3 if mx else 1e-5)]
    gmax = max(v.grad.norm().item() for v in ref.values())
    worst, wname, shapes_ok = 0.0, "", True
    for k, p_ in m.named_parameters():
        shapes_ok &= p_.grad is not None and p_.grad.shape == ref[k].shape
        gr = ref[k].grad
        if gr.norm().item() > 1e-4 * gmax:
            e = ((p_.grad.cpu() - gr).norm() / gr.norm()).item()
            if e > worst:
                worst, wname = e, k
    res.append(_res(tag + ".grad_shapes_are_the_parameters", 0.0 if shapes_ok else 1.0, 0.0))
    res.append(_res(tag + ".grads_rel_l2_worst", worst, 0.15 if bf else 0.10 if mx else 2e-3, wname))
    with torch.no_grad():
        pr = m.eval()(x.to(DEV))
    res.append(_res(tag + ".eval_logits_rel", (pr.cpu() - lo_ref.detach()).abs().max().item() / lo_ref.detach().abs().max().item(), 6e-2 if bf else 8e-3 if mx else 2e-4))
    return res

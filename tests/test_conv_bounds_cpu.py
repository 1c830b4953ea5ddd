"""The element-wise conv comparator (tests/conv_bounds.py) on the CPU: correctly rounded results pass it, simulated kernel faults fail it at
every storage type, the forward route table and the bpx_conv3d_fwd_shuffle rows reach the tile configurations they name, and the fused
conv + pixel-shuffle reference is the oracle's pixel_shuffle3d of the conv.  No GPU: the faults are injected into fp64
simulations of a kernel's output, and the route checks call host functions of the library."""
import pytest
import torch
import torch.nn.functional as F

import conv_bounds as CB

KINDS = ("f32", "bf16", "f16")


_recs = CB.norm_recs


def _case(kind, B, S, C, seed):
    """Stored operands, the fp64 reference with its bound, and the simulated CORRECT kernel: prologue formed and rounded to the operand type,
    exact sum, bias, one rounding to the output type."""
    g = torch.Generator().manual_seed(seed)
    x = CB.round_to(torch.randn(B, *S, C, generator=g), kind)
    w = CB.round_to(torch.randn(C, C, 3, 3, 3, generator=g) / (27 * C) ** 0.5, kind)
    b = torch.randn(C, generator=g) * 0.1
    rec = _recs(B, C, g)
    ref, bound, pre = CB.fwd_reference(x, w, b, kind, rec=rec, act=1)
    a, _ = CB.prologue(x, rec, 1, kind)
    ad = CB.round_to(a, kind)
    v = CB.conv3(ad, w) + b.double()          # the fp32 value before the store (what the statistics sum), here exact
    return dict(x=x, w=w, b=b, rec=rec, ref=ref, bound=bound, pre=pre, ad=ad, v=v, good=CB.round_to(v, kind))


_CACHE = {}


def case_a(kind):
    """Shape of fault A: B 2, 12 x 20 x 24, 32 -> 32, InstanceNorm + ELU prologue."""
    if ("A", kind) not in _CACHE:
        _CACHE[("A", kind)] = _case(kind, 2, (12, 20, 24), 32, 0)
    return _CACHE[("A", kind)]


def case_b(kind):
    """Shape of fault B: B 2, 9 x 17 x 33, 16 -> 16."""
    if ("B", kind) not in _CACHE:
        _CACHE[("B", kind)] = _case(kind, 2, (9, 17, 33), 16, 1)
    return _CACHE[("B", kind)]


FAULT_A_CHANNEL = 10


def fault_a(kind):
    """The prologue applied to padding: the high-z halo face of one input channel holds act(shift) instead of zero."""
    c = case_a(kind)
    ap = F.pad(c["ad"], (0, 0, 1, 1, 1, 1, 1, 1))
    shift = c["rec"][:, FAULT_A_CHANNEL, 3].double()
    ap[:, -1, :, :, FAULT_A_CHANNEL] = CB.round_to(F.elu(shift), kind)[:, None, None]
    return CB.round_to(CB.conv3_padded(ap, c["w"]) + c["b"].double(), kind)


def fault_b(kind):
    """One weight swapped with its neighbouring input channel's, on the y = 0 border row only."""
    c = case_b(kind)
    w2 = c["w"].clone()
    w2[3, 5, 0, 1, 2], w2[3, 6, 0, 1, 2] = c["w"][3, 6, 0, 1, 2], c["w"][3, 5, 0, 1, 2]
    out = CB.conv3(c["ad"], c["w"])
    out[:, :, 0] = CB.conv3(c["ad"], w2)[:, :, 0]
    return CB.round_to(out + c["b"].double(), kind)


def fault_chunk(kind):
    """Input chunk 1 (channels 16..31) dropped for one tap (z + 1) in the last partial 4x4x16 tile (z 8..11, y 16..19, x 16..23)."""
    c = case_a(kind)
    out = CB.conv3(c["ad"], c["w"])
    ap = F.pad(c["ad"], (0, 0, 1, 1, 1, 1, 1, 1))
    kz, ky, kx = 2, 1, 1
    src = ap[:, 8 + kz:12 + kz, 16 + ky:20 + ky, 16 + kx:24 + kx, 16:32]
    out[:, 8:12, 16:20, 16:24] -= src @ c["w"][:, 16:32, kz, ky, kx].t()
    return CB.round_to(out + c["b"].double(), kind)


def fault_bias_twice(kind):
    """The bias added twice on one z slice."""
    c = case_a(kind)
    out = CB.conv3(c["ad"], c["w"]) + c["b"].double()
    out[:, 7] += c["b"].double()
    return CB.round_to(out, kind)


def fault_unwritten(kind):
    """One element never written (the NaN pre-fill survives)."""
    out = case_a(kind)["good"].clone()
    out[1, 11, 19, 23, 31] = float("nan")
    return out


FAULTS = {"halo_act_shift": (fault_a, case_a), "border_row_swapped_weight": (fault_b, case_b), "dropped_chunk_last_tile": (fault_chunk, case_a),
          "bias_twice_on_one_slice": (fault_bias_twice, case_a), "unwritten_element": (fault_unwritten, case_a)}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [case_a, case_b], ids=["A_shape", "B_shape"])
def test_correctly_rounded_result_passes(kind, case):
    c = case(kind)
    r = CB.compare("correct", c["good"], c["ref"], c["bound"])
    assert r["ok"], r
    assert r["err"] > 0.0, "the simulation must actually round"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_synthetic_fault_fails(kind, fault):
    make, case = FAULTS[fault]
    c = case(kind)
    r = CB.compare(fault, make(kind), c["ref"], c["bound"])
    assert not r["ok"], r


def test_fault_a_passes_the_old_bf16_relerr_bar():
    """Why the element-wise checks exist: the halo fault scores under the relerr bar (max |got - ref| / max |ref| < 1.5e-2) the kernel
    parity rows use at bf16, while the element-wise bound rejects it."""
    c = case_a("bf16")
    got = fault_a("bf16")
    relerr = ((got - c["ref"]).abs().max() / c["ref"].abs().max()).item()
    assert relerr < 1.5e-2, relerr
    assert CB.compare("A", got, c["ref"], c["bound"])["err"] > 1.0


def test_nonfinite_fails_even_inside_the_bound():
    c = case_a("f32")
    got = c["good"].clone()
    got[0, 0, 0, 0, 0] = float("inf")
    assert not CB.compare("inf", got, c["ref"], c["bound"])["ok"]


@pytest.mark.parametrize("kind", KINDS)
def test_statistics_bound_accepts_correct_sums_and_rejects_a_lost_tile(kind):
    """The statistics bound with the element bound fwd_reference returns (InstanceNorm + ELU prologue): the sums of the simulated correct
    kernel's pre-store values pass; losing one 4x4x16 tile's sums fails at f32 and f16.  At bf16 the prologue operand's rounding term
    (2^-8 per operand) makes the bound wider than one tile's contribution, so there the lost tile is only caught by the element rows of the
    same call (an unwritten tile is NaN) - conv_bounds.stats_reference says so."""
    c = case_a(kind)
    s, bnd = CB.stats_reference(c["ref"], c["pre"], 256)
    good = torch.stack([c["v"].sum((1, 2, 3)), (c["v"] * c["v"]).sum((1, 2, 3))], 1)
    assert ((good - s).abs() <= bnd).all()
    lost = good.clone()
    t = c["v"][:, 8:12, 16:20, 16:24]
    lost[:, 0] -= t.sum((1, 2, 3))
    lost[:, 1] -= (t * t).sum((1, 2, 3))
    caught = ((lost - s).abs() > bnd).any().item()
    assert caught or kind == "bf16"


# ---- the route table reaches what it names ------------------------------------------------------------------------------------------
_DT = {"f32": 0, "bf16": 1, "f16": 2}


@pytest.mark.parametrize("row", CB.FWD_ROUTES, ids=[r["name"] for r in CB.FWD_ROUTES])
def test_route_row_tile_count_matches_its_configuration(row):
    from biapy_amd import _lib as L

    tz, ty, tx, ns = row["cfg"]
    D, H, W = row["S"]
    want = -(-D // tz) * -(-H // ty) * -(-W // tx)
    for kind in row["kinds"]:
        assert L.lib.bpx_conv3d_stats_tiles(_DT[kind], row["B"], D, H, W, row["Cout"]) == want, (row["name"], kind)
    # 16 * ns output channels per workgroup: pick_cfg's rule (64 -> 4, 48 -> 3, 32 -> 2, else 1; 4 -> 2 at <= 512 voxels)
    n = 4 if row["Cout"] % 64 == 0 else 3 if row["Cout"] % 48 == 0 else 2 if row["Cout"] % 32 == 0 else 1
    assert ns == (2 if n == 4 and D * H * W <= 512 else n), row["name"]


def test_every_launch_conv3_configuration_is_in_the_route_table():
    for kind, cfgs in CB.LAUNCH_CONV3_CFGS.items():
        have = {r["cfg"] for r in CB.FWD_ROUTES if kind in r["kinds"] and CB.runs_plain_kernel(r, kind)}
        missing = [c for c in cfgs if c not in have]
        assert not missing, (kind, missing)


def test_route_table_covers_every_route_at_f16():
    names = {r["name"] for r in CB.FWD_ROUTES if "f16" in r["kinds"]}
    for prefix in ("s448_", "s4416_ns2", "s4416_ns3", "s4416_ns4", "s4816_ws4", "lean4816", "lean4416_ns1", "lean4416_ns2", "lean4416_ns3",
                   "lean4416_ns4", "zm_rolesplit", "zm_onechunk", "zm_threechunks", "pool_lean", "pool_zm", "s448_ns4_kg2", "s448_ns4_kg1"):
        assert any(n.startswith(prefix) for n in names), prefix
    assert all(f"s448_act{a}" in names for a in range(2, 9))


def test_fused_pool_and_fused_backward_gates():
    """bpx_conv3d_fwd_pool_supported / bpx_conv3d_bwd_fused_supported: the pool rows run where the gate answers 1 at the production size
    and the fused-backward rows of the GPU file are supported shapes."""
    from biapy_amd import _lib as L

    lib = L.lib
    assert lib.bpx_conv3d_fwd_pool_supported(1, 1, 64, 64, 64, 16, 16, 16) == 1
    assert lib.bpx_conv3d_fwd_pool_supported(2, 1, 64, 64, 64, 48, 16, 16) == 1
    assert lib.bpx_conv3d_fwd_pool_supported(0, 1, 64, 64, 64, 16, 16, 16) == 0
    assert lib.bpx_conv3d_fwd_pool_supported(1, 1, 64, 64, 8, 16, 16, 16) == 0
    for dtc, B, S, Ct, Cdy in CB.BWD_FUSED_ROWS:
        assert lib.bpx_conv3d_bwd_fused_supported(dtc, B, *S, Ct, Cdy) == 1, (dtc, S, Ct, Cdy)


# ---- the fused conv + 3-D pixel shuffle (bpx_conv3d_fwd_shuffle) ----------------------------------------------------------------------
W16 = ("bf16", "f16")
SH_S, SH_SHAPE = 2, (5, 6, 18)     # 4x4x16 tiles: an edge tile on every axis; y tile 1 holds rows 4..5, x tile 1 columns 16..17
SH_SUB = (1, 0, 1)                 # the sub-position (a, b, e) faults (b) hit: channel block 5, the second block of the NS = 4 workgroup 1


@pytest.mark.parametrize("s", [2, 3, 4])
def test_shuffle_reference_is_the_oracles_pixel_shuffle_of_the_conv(s):
    """shuffle_reference on the weight passed through rows_to_subposition_major == pixel_shuffle3d(conv3d(x, w, b)) with the weight in
    PyTorch's order, exactly: the operands are small integers, so every fp64 sum is exact whatever its order.  The bound and the
    pre-rounding bound move with the reference."""
    from biapy_amd.rcan_engine import rows_to_subposition_major
    from oracle.rcan_oracle import pixel_shuffle3d

    g = torch.Generator().manual_seed(40 + s)
    s3 = s ** 3
    x = torch.randint(-8, 9, (2, 3, 5, 6, 16), generator=g).double()
    w = torch.randint(-8, 9, (16 * s3, 16, 3, 3, 3), generator=g).double()
    b = torch.randint(-8, 9, (16 * s3,), generator=g).float()
    wu, bu = rows_to_subposition_major(w, b, 16, s3)
    ref, bound, pre = CB.shuffle_reference(x, wu, bu, "bf16", s)
    ncdhw, ndhwc = (lambda t: t.permute(0, 4, 1, 2, 3)), (lambda t: t.permute(0, 2, 3, 4, 1))
    want = ndhwc(pixel_shuffle3d(F.conv3d(ncdhw(x), w, b.double(), padding=1), s))
    assert ref.shape == (2, 3 * s, 5 * s, 6 * s, 16) and torch.equal(ref, want)
    r0, b0, p0 = CB.fwd_reference(x, w, b, "bf16")              # PyTorch's channel order: the oracle's shuffle applies as it stands
    assert torch.equal(ref, ndhwc(pixel_shuffle3d(ncdhw(r0), s)))
    assert torch.equal(bound, ndhwc(pixel_shuffle3d(ncdhw(b0), s))) and torch.equal(pre, ndhwc(pixel_shuffle3d(ncdhw(p0), s)))


def shuffle_case(kind):
    """Stored operands of a 16 -> 128 conv + shuffle by 2 (weight and bias drawn in PyTorch's order), the reference with its bound on the
    fine grid, and the simulated correct kernel's values on the coarse grid before the store (exact sum + bias)."""
    if ("S", kind) not in _CACHE:
        from biapy_amd.rcan_engine import rows_to_subposition_major

        g = torch.Generator().manual_seed(2)
        s3 = SH_S ** 3
        x = CB.round_to(torch.randn(1, *SH_SHAPE, 16, generator=g), kind)
        w = CB.round_to(torch.randn(16 * s3, 16, 3, 3, 3, generator=g) / (27 * 16) ** 0.5, kind)
        b = (torch.randn(16 * s3, generator=g) * 0.1).float()
        wu, bu = rows_to_subposition_major(w, b, 16, s3)
        ref, bound, _ = CB.shuffle_reference(x, wu, bu, kind, SH_S)
        conv = CB.conv3(x, wu)
        _CACHE[("S", kind)] = dict(ref=ref, bound=bound, conv=conv, b=b, bu=bu, v=conv + bu.double())
    return _CACHE[("S", kind)]


def _store(v, kind, s=SH_S):
    return CB.round_to(CB.shuffle_to_fine_grid(v, s), kind)


def _blocks(v, s=SH_S):
    """(B, D, H, W, 16 s^3) -> (B, D, H, W, a, b, e, 16): a view of the channel blocks by sub-position."""
    return v.reshape(*v.shape[:-1], s, s, s, 16)


def shfault_swapped_b_e(kind):
    """(a) Sub-positions b and e swapped: block (a, b, e) lands at (s z + a, s y + e, s x + b)."""
    return _store(_blocks(shuffle_case(kind)["v"]).transpose(5, 6).reshape(shuffle_case(kind)["v"].shape), kind)


def _edge_row(t):
    """The last y row (5) of the ragged edge tile (z 4, y 4..5, x 16..17) of a (B, D, H, W, a, b, e, 16) view, at sub-position SH_SUB."""
    a, b, e = SH_SUB
    return t[:, 4:5, 5, 16:18, a, b, e]


def shfault_edge_row_unwritten(kind):
    """(b) The last y row of a ragged edge tile of one sub-position never stored: the NaN pre-fill survives."""
    v = shuffle_case(kind)["v"].clone()
    _edge_row(_blocks(v))[...] = float("nan")
    return _store(v, kind)


def shfault_edge_row_neighbour(kind):
    """(b) The same row holding the neighbouring sub-position's (a, b, e - 1) values."""
    v = shuffle_case(kind)["v"].clone()
    a, b, e = SH_SUB
    _edge_row(_blocks(v))[...] = _blocks(shuffle_case(kind)["v"])[:, 4:5, 5, 16:18, a, b, e - 1]
    return _store(v, kind)


def shfault_second_block_first_ysub(kind):
    """(c) The second channel workgroup (sub-positions 4..7 at NS = 4) stores with the first one's ysub: its values land on sub-positions
    0..3 and its own voxels are never written."""
    v = _blocks(shuffle_case(kind)["v"]).clone()
    v[..., 0, :, :, :] = v[..., 1, :, :, :]
    v[..., 1, :, :, :] = float("nan")
    return _store(v.reshape(shuffle_case(kind)["v"].shape), kind)


def shfault_bias_in_pytorch_order(kind):
    """(d) The bias left in PyTorch's [channel][sub-position] order under a weight in [sub-position][channel] order."""
    c = shuffle_case(kind)
    return _store(c["conv"] + c["b"].double(), kind)


SHUFFLE_FAULTS = {"a_swapped_b_e": shfault_swapped_b_e, "b_edge_row_unwritten": shfault_edge_row_unwritten,
                  "b_edge_row_neighbour": shfault_edge_row_neighbour, "c_second_block_first_ysub": shfault_second_block_first_ysub,
                  "d_bias_in_pytorch_order": shfault_bias_in_pytorch_order}


@pytest.mark.parametrize("kind", W16)
def test_shuffle_correctly_rounded_result_passes(kind):
    c = shuffle_case(kind)
    r = CB.compare("correct", _store(c["v"], kind), c["ref"], c["bound"])
    assert r["ok"], r
    assert r["err"] > 0.0, "the simulation must actually round"


@pytest.mark.parametrize("kind", W16)
@pytest.mark.parametrize("fault", sorted(SHUFFLE_FAULTS))
def test_shuffle_synthetic_fault_fails(kind, fault):
    c = shuffle_case(kind)
    got = SHUFFLE_FAULTS[fault](kind)
    assert not torch.equal(torch.nan_to_num(got, nan=1e30), torch.nan_to_num(_store(c["v"], kind), nan=1e30)), "the fault must change the output"
    r = CB.compare(fault, got, c["ref"], c["bound"])
    assert not r["ok"], r


@pytest.mark.parametrize("row", CB.SHUFFLE_ROWS, ids=[r["name"] for r in CB.SHUFFLE_ROWS])
def test_shuffle_row_reaches_the_configuration_it_names(row):
    """pick_cfg of the 16 s^3-channel conv (what bpx_conv3d_fwd_shuffle launches the lean kernel with), seen through bpx_conv3d_stats_tiles,
    and the volume sizes the entry admits (>= 32^3 voxels, W > 8, fewer than 2^30 output elements)."""
    from biapy_amd import _lib as L

    tz, ty, tx, ns = row["cfg"]
    D, H, W = row["S"]
    Cout = 16 * row["s"] ** 3
    for kind in row["kinds"]:
        assert L.lib.bpx_conv3d_stats_tiles(_DT[kind], row["B"], D, H, W, Cout) == -(-D // tz) * -(-H // ty) * -(-W // tx), (row["name"], kind)
    assert ns == (4 if Cout % 64 == 0 else 3 if Cout % 48 == 0 else 2 if Cout % 32 == 0 else 1) and ns > 1 and tx == 16
    assert Cout // (16 * ns) == {2: 2, 3: 9, 4: 16}[row["s"]]                 # output-channel workgroups per tile
    assert D * H * W >= 32768 and W > 8 and row["B"] * D * H * W * Cout < 2 ** 30
    assert row["samples"] is None or max(row["samples"]) == row["B"] - 1


def test_shuffle_edge_row_fault_against_the_relerr_bar_of_the_network_tests():
    """Fault (b) with the neighbouring sub-position's values under max |got - want| / max |want|, the measure of test_rcan_upscaling_stage
    (bar 4e-2 at bf16), applied to the stage's own output.  Unlike the halo fault of test_fault_a_passes_the_old_bf16_relerr_bar this
    one does NOT score under that bar with these operands: the sub-positions' weight rows are independent draws, so two wrong voxels
    are off by the size of an output - relerr 0.51 at bf16 and at f16 (element-wise: err / bound 4.4e3 and 1.2e4).  What let such a fault
    through was the set of cases, not the measure: every volume the network tests run is a 32^3 or 64^3 cube, which has no edge tile, so the
    masked rows of this store never ran.  The value is printed; only the element-wise rejection is asserted."""
    c = shuffle_case("bf16")
    got = shfault_edge_row_neighbour("bf16")
    relerr = ((got - c["ref"]).abs().max() / c["ref"].abs().max()).item()
    print(f"fault (b), neighbouring values: relerr {relerr:.3e} against the 4e-2 bar")
    assert CB.compare("b", got, c["ref"], c["bound"])["err"] > 1.0

"""The element-wise conv comparator (tests/conv_bounds.py) on the CPU: correctly rounded results pass it, simulated kernel faults fail it at
every storage type, and the forward route table reaches the tile configurations it names.  No GPU: the faults are injected into fp64
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

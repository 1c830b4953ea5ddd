"""SGD on the replayed step - what can be checked without a GPU: the fp64 statement the device tests measure against (sgd_bounds.sgd_reference) is
torch.optim.SGD, its fp32 bound holds for torch's own fp32 step and rejects two simulated faults, the entry point is declared and bound, the host
functions decline CPU tensors untouched, and the device copy of the momentum follows the host double exactly."""
import os
import re

import numpy as np
import pytest
import torch

import optim_bounds as OB
import sgd_bounds as SB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(16,), (1,), (5, 7), (16, 1, 3, 3, 3), (300,)]


def _state(dtype, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=gen).to(dtype) for s in SIZES]


@pytest.mark.parametrize("name", list(SB.CONFIGS))
def test_fp64_statement_is_torchs_sgd(name):
    """Three steps of torch.optim.SGD on float64 CPU parameters (the first one seeds the momentum buffer) against sgd_reference step by step, each
    from torch's own state: 1e-12 relative to the largest magnitude of the tensor."""
    cfg = SB.CONFIGS[name]
    ps = [torch.nn.Parameter(t) for t in _state(torch.float64)]
    opt = SB.torch_sgd(ps, cfg)
    for it in range(3):
        grads, _ = OB.make_grads(SIZES, seed=10 + it)
        before = [p.detach().clone() for p in ps]
        bufs = [opt.state[p].get("momentum_buffer") for p in ps]
        bufs = [None if b is None else b.clone() for b in bufs]
        for p, g in zip(ps, grads):
            p.grad = g.double()
        opt.step()
        for p, p0, g, b in zip(ps, before, grads, bufs):
            assert (b is None) == (it == 0 or cfg["momentum"] == 0)
            want_p, want_b = SB.sgd_reference(p0, g, b, first=it == 0, **cfg)
            assert (p.detach() - want_p).abs().max() <= 1e-12 * want_p.abs().max()
            if cfg["momentum"] != 0:
                got_b = opt.state[p]["momentum_buffer"]
                assert (got_b - want_b).abs().max() <= 1e-12 * want_b.abs().max()
            else:
                assert want_b is None and "momentum_buffer" not in opt.state[p]


def _torch_f32_step(cfg, first, seed=0):
    """One fp32 step of torch's CPU SGD from a given state: (p0, g, buf0 or None, p1, buf1 or None) per tensor."""
    ps = [torch.nn.Parameter(t) for t in _state(torch.float32, seed)]
    opt = SB.torch_sgd(ps, cfg)
    bufs = [None] * len(ps)
    if cfg["momentum"] != 0 and not first:
        bufs = _state(torch.float32, seed + 1)
        for p, b in zip(ps, bufs):
            opt.state[p]["momentum_buffer"] = b.clone()
    grads, _ = OB.make_grads(SIZES, seed=seed + 2)
    p0 = [p.detach().clone() for p in ps]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    opt.step()
    return [(a, g, b, p.detach(), opt.state[p].get("momentum_buffer")) for a, g, b, p in zip(p0, grads, bufs, ps)]


@pytest.mark.parametrize("first", [False, True], ids=["with_state", "first"])
@pytest.mark.parametrize("name", list(SB.CONFIGS))
def test_bound_holds_for_torchs_fp32_step(name, first):
    cfg = SB.CONFIGS[name]
    worst = 0.0
    for p0, g, b0, p1, b1 in _torch_f32_step(cfg, first):
        want_p, want_b = SB.sgd_reference(p0, g, b0, first=first, **cfg)
        bp, bb = SB.sgd_bound(p0, g, b0, first=first, **cfg)
        worst = max(worst, SB.worst_ratio(p1, want_p, bp))
        if cfg["momentum"] != 0:
            worst = max(worst, SB.worst_ratio(b1, want_b, bb))
        else:
            assert bb is None and b1 is None
    print(f"torch fp32 SGD[{name}, first={first}]: worst err / bound = {worst:.3f}")
    assert worst <= 1.0


def test_bound_rejects_simulated_faults():
    """A momentum buffer left un-updated, and a weight decay dropped: both are far outside the bound."""
    cfg = SB.CONFIGS["nesterov_wd"]
    rows = _torch_f32_step(cfg, first=False)
    stale = max(SB.worst_ratio(b0, SB.sgd_reference(p0, g, b0, first=False, **cfg)[1], SB.sgd_bound(p0, g, b0, first=False, **cfg)[1])
                for p0, g, b0, _, _ in rows)
    assert stale > 1e3
    no_wd = dict(cfg, wd=0.0)
    dropped = 0.0
    for (p0, g, b0, _, _), (_, _, _, p1, _) in zip(rows, _torch_f32_step(no_wd, first=False)):
        dropped = max(dropped, SB.worst_ratio(p1, SB.sgd_reference(p0, g, b0, first=False, **cfg)[0], SB.sgd_bound(p0, g, b0, first=False, **cfg)[0]))
    assert dropped > 1e3
    print(f"faults: stale buffer {stale:.3g} x bound, dropped weight decay {dropped:.3g} x bound")


def test_sgd_entry_point_is_declared_and_bound():
    from biapy_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    assert re.search(r"^int bpx_sgd_step\(", header, re.M)
    assert "bpx_sgd_step" in L.EXPORTS and getattr(L.lib._raw, "bpx_sgd_step") is not None
    assert L.lib.bpx_sgd_step(1, None, None, 0.1, None, 0.9, 0.0, 0.0, 0, None, None) != 0 and b"bad tensor list" in L.lib.bpx_last_error()
    arr = (L.AdamTensor * 1)()
    arr[0].numel = 4
    assert L.lib.bpx_sgd_step(1, arr, None, 0.1, None, 0.9, 0.0, 0.0, 0, None, None) != 0 and b"null pointer" in L.lib.bpx_last_error()
    assert L.lib.bpx_sgd_step(0, None, 2, 0.1, None, 0.0, 0.0, 0.0, 0, None, None) != 0 and b"misaligned device scalar" in L.lib.bpx_last_error()
    assert L.lib.bpx_sgd_step(0, None, None, 0.1, None, 0.0, 0.0, 0.0, 1, None, None) != 0 and b"Nesterov" in L.lib.bpx_last_error()


def test_host_functions_decline_cpu_tensors_untouched():
    from biapy_amd import optim as O

    cfg = SB.CONFIGS["nesterov_wd"]
    ps = [torch.nn.Parameter(t) for t in _state(torch.float32)]
    twin = [torch.nn.Parameter(t) for t in _state(torch.float32)]
    opt, ref = SB.torch_sgd(ps, cfg), SB.torch_sgd(twin, cfg)
    assert O.supports_sgd(opt) and not O.supports(opt)
    for it in range(2):                                        # without state, then with momentum buffers
        grads, _ = OB.make_grads(SIZES, seed=20 + it)
        for p, q, g in zip(ps, twin, grads):
            p.grad, q.grad = g.clone(), g.clone()
        before = [p.detach().clone() for p in ps]
        bufs = [None if "momentum_buffer" not in opt.state[p] else opt.state[p]["momentum_buffer"].clone() for p in ps]
        out = torch.zeros(2)
        assert O.fused_step(opt) is False
        assert O.fused_sgd_step(opt, max_norm=0.5, momentum_d=[torch.tensor(0.9, dtype=torch.float64)], norm_out=out) is False
        assert all(torch.equal(a, b) for a, b in zip(before, ps)) and all(torch.equal(p.grad, g) for p, g in zip(ps, grads))
        assert all(b is None or torch.equal(b, opt.state[p]["momentum_buffer"]) for b, p in zip(bufs, ps)) and float(out.abs().sum()) == 0.0
        assert O.step(opt) is False                            # torch's own step ran
        ref.step()
        assert all(torch.equal(a, b) for a, b in zip(ps, twin))


def test_lr_tensors_carry_the_momentum_as_a_double():
    from biapy_amd.graphs import _LrTensors

    values = OB.onecycle_beta1(steps=10)                       # the doubles a one-cycle schedule assigns (0.95 ... 0.85), not float32 values
    p = [torch.nn.Parameter(torch.zeros(3))]
    q = [torch.nn.Parameter(torch.zeros(3))]
    opt = torch.optim.SGD([dict(params=p, momentum=values[0]), dict(params=q, momentum=0.0)], lr=0.1, nesterov=False)
    lt = _LrTensors(opt, "cpu")
    assert lt.beta1s == [None, None] and lt.momenta[1] is None
    m = lt.momenta[0]
    assert m.dtype == torch.float64 and m.dim() == 0 and m.item() == values[0]
    for v in values[1:]:
        opt.param_groups[0]["momentum"] = v                    # what OneCycleLR does on an optimizer with a "momentum" key
        before = m.data_ptr()
        lt.sync()
        assert m.item() == v and m.data_ptr() == before and lt.momenta[0] is m
        assert type(opt.param_groups[0]["momentum"]) is float
    assert any(float(np.float32(v)) != v for v in values)
    assert _LrTensors(torch.optim.SGD(p, lr=0.1), "cpu").beta1s == [None]
    assert _LrTensors(torch.optim.AdamW(p, lr=0.1), "cpu").momenta == [None]


def test_supports_sgd_refusals():
    from biapy_amd import optim as O

    p = [torch.nn.Parameter(torch.zeros(3))]
    assert O.supports_sgd(torch.optim.SGD(p, lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-2))
    assert not O.supports_sgd(torch.optim.SGD(p, lr=0.1, maximize=True))
    assert not O.supports_sgd(torch.optim.SGD(p, lr=0.1, differentiable=True))
    assert not O.supports_sgd(torch.optim.AdamW(p, lr=0.1))
    hooked = torch.optim.SGD(p, lr=0.1)
    hooked.register_step_post_hook(lambda *a: None)
    assert not O.supports_sgd(hooked)

    class MySGD(torch.optim.SGD):
        pass

    assert not O.supports_sgd(MySGD(p, lr=0.1))
    tensor_mom = torch.optim.SGD(p, lr=0.1, momentum=0.9)
    tensor_mom.param_groups[0]["momentum"] = torch.tensor(0.9)
    assert not O.supports_sgd(tensor_mom)


def test_graph_on_message_names_sgd():
    import types

    from biapy_amd import train_engine as TE

    cfg = types.SimpleNamespace(DATA=types.SimpleNamespace(PATCH_SIZE=(8, 8, 8, 1)),
                                TRAIN=types.SimpleNamespace(GRADIENT_CLIP_NORM=1.0, LR_SCHEDULER=types.SimpleNamespace(NAME="onecycle"), VERBOSE=False))
    net = torch.nn.Conv3d(1, 1, 1)
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9, nesterov=True)
    with pytest.raises(ValueError, match=r"^graph='on'.*SGD"):
        TE.train_one_epoch(cfg, net, None, torch.nn.BCEWithLogitsLoss(), None, None, [], [opt], torch.device("cpu"), 0, graph="on")

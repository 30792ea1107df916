"""The route builders and result checks of tests/_route_util.py without a GPU:
every builder on device "cpu" (arenas are then host arenas), the placement
rules, the transposed layout, the fed-back registered arena, and
result_problems against results with one fault each."""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch
from torch import nn

import _krum_util as ku
import _route_util as rt
from _sgd_util import BnNet
from dasklearn_amd import arena

CPU = torch.device("cpu")


def _cpu_models(n=5):
    return rt.filled(rt.Mixed, n, seed=40)


def _feed(models):
    return arena.to_device_arena(models[0], CPU)  # a module_from_arenas output, as an aggregate's result is


def test_names_and_sets():
    r = rt.routes(CPU, _feed)
    assert tuple(r) == rt.NAMES and len(rt.NAMES) == 9
    assert set(rt.BASELINE) | set(rt.MIXED_PLACEMENT) | set(rt.TRANSPOSED) <= set(rt.NAMES)
    assert set(rt.ONE_ROW_PER_MODEL) <= set(rt.NAMES) and "tensors" not in rt.ONE_ROW_PER_MODEL


def test_placement_rules():
    assert rt.kinds("arena0_host_peers", 4) == ["arena", "host", "host", "host"]
    assert rt.kinds("host0_device_peers", 5) == ["host", "arena", "tensors", "arena", "tensors"]
    assert rt.kinds("arena_and_tensors", 4) == ["arena", "tensors", "arena", "tensors"]
    # a peer that must be a host model, one that must be a device model
    assert rt.kinds("arena0_host_peers", 4, host=(0,), device=(2,)) == ["host", "host", "arena", "host"]
    assert rt.kinds("host0_device_peers", 4, host=(3,), device=(0, 2)) == ["arena", "arena", "tensors", "host"]
    with pytest.raises(AssertionError):
        rt.kinds("host", 3, host=(1,), device=(1,))


@pytest.mark.parametrize("name", rt.NAMES)
def test_every_route_keeps_every_value(name):
    cpu = _cpu_models()
    before = [ku.flat_bits(m) for m in cpu]
    models = rt.routes(CPU, _feed)[name](cpu)
    assert len(models) == len(cpu)
    for m, c, saved in zip(models, cpu, before):
        assert type(m) is rt.Mixed and np.array_equal(ku.flat_bits(m), saved)
        assert np.array_equal(ku.flat_bits(c), saved), "a builder changed a CPU model"
        assert [p.shape for p in m.parameters()] == [p.shape for p in c.parameters()]
    if name in ("host", "transposed_host"):
        assert (models[1] is cpu[1]) == (name == "host")
    if name in ("arena", "fed_back"):
        assert all(arena.registered_arenas(m) is not None for m in models)
    if name == "arena0_host_peers":
        assert arena.registered_arenas(models[0]) is not None and all(a is b for a, b in zip(models[1:], cpu[1:]))
    if name == "tensors":
        assert all(arena.registered_arenas(m) is None and m is not c for m, c in zip(models, cpu))


@pytest.mark.parametrize("name", rt.TRANSPOSED)
def test_transposed_routes_change_strides_only(name):
    cpu = _cpu_models()
    models = rt.routes(CPU, _feed)[name](cpu)
    flipped = [i for i, m in enumerate(models) if not m.a.is_contiguous()]
    assert flipped == [0, 2]
    for i in flipped:
        assert models[i].a.shape == (33, 7) and models[i].a.stride() == (1, 33)
        assert rt.same_params(models[i], rt.param_bits(cpu[i])) and cpu[i].a.is_contiguous()
    assert all(p.is_contiguous() for m in models for k, p in enumerate(m.parameters()) if k)
    with pytest.raises(AssertionError):
        rt.transpose_first_matrix(nn.Linear(1, 3))  # [3, 1]: contiguous either way
    with pytest.raises(AssertionError):
        rt.transpose_first_matrix(rt.EmptyNet())


def test_the_fed_back_model_is_a_registered_arena_with_its_own_row():
    cpu = [ku.model_of(np.full(50, float(i), dtype=np.float32), None, "f32", make=BnNet) for i in range(4)]
    with torch.no_grad():
        for i, m in enumerate(cpu):
            m.bn.running_mean.fill_(10.0 + i)
    seen = []

    def feed(models):
        seen.append(len(models))
        return _feed(models)
    models = rt.routes(CPU, feed)["fed_back"](cpu)
    assert seen == [3]
    reg = arena.registered_arenas(models[1])
    assert reg is not None and torch.equal(reg[1][torch.float32], torch.full((50,), 1.0))
    assert torch.equal(models[1].bn.running_mean, torch.full((5,), 11.0))
    assert all(float(p.detach().reshape(-1)[0]) == 0.0 for p in models[0].parameters())


def test_modules_with_empty_parameters():
    z = rt.ZeroNet()
    assert [(tuple(p.shape), p.dtype) for p in z.parameters()] == [
        ((7, 3), torch.float32), ((0,), torch.float32), ((5,), torch.float32), ((0,), torch.bfloat16)]
    layout = arena.ParamLayout(z)
    assert layout.totals == {torch.float32: 26, torch.bfloat16: 0}
    assert [tuple(p.shape) for p in rt.EmptyNet().parameters()] == [(0,)]
    ms = rt.filled(rt.ZeroNet, 3, seed=1)
    assert not torch.equal(ms[0].a, ms[1].a)


def test_mixed_models_hold_the_rows_in_layout_order():
    f32 = np.arange(2 * 236, dtype=np.float32).reshape(2, 236)
    b16 = (np.arange(2 * 165, dtype=np.uint16) + 0x3F80).reshape(2, 165)
    ms = rt.mixed_models(f32, b16)
    assert torch.equal(ms[1].a.reshape(-1), torch.from_numpy(f32[1, :231])) and float(ms[1].c.detach()[0]) == f32[1, 231]
    assert int(ms[1].b.view(torch.int16)[0]) == b16[1, 0] and int(ms[1].d.view(torch.int16)[3, 8]) == b16[1, 164]


# ---- result_problems -----------------------------------------------------------------------
def _bn_pair():
    torch.manual_seed(0)
    m0 = BnNet()
    with torch.no_grad():
        m0.bn.running_mean.uniform_(-1, 1)
    return m0, copy.deepcopy(m0)


def test_a_deep_copy_is_a_clean_result():
    m0, out = _bn_pair()
    assert rt.result_problems(out, [m0], "host") == []
    assert rt.result_problems(out, [m0], "host", to_host=True) == []
    t0 = rt.transpose_first_matrix(copy.deepcopy(m0))
    assert rt.result_problems(copy.deepcopy(t0), [t0], "transposed_host") == []


def test_each_fault_is_reported():
    m0, out = _bn_pair()
    assert any("on cpu" in p for p in rt.result_problems(out, [m0], "host", to_host=False))
    assert any("Linear" in p for p in rt.result_problems(nn.Linear(7, 5), [m0], "host"))
    assert any("parameters" in p for p in rt.result_problems(nn.Linear(7, 5, bias=False), [m0], "host"))
    bad = copy.deepcopy(m0)
    bad.fc.weight.requires_grad_(False)
    assert any("parameter 0" in p for p in rt.result_problems(bad, [m0], "host"))
    bad = copy.deepcopy(m0)
    bad.fc.bias.data = bad.fc.bias.data.double()
    assert any("parameter 1" in p for p in rt.result_problems(bad, [m0], "host"))
    # the strides count under the transposed routes only
    t0 = rt.transpose_first_matrix(copy.deepcopy(m0))
    assert rt.result_problems(out, [t0], "host") == []
    assert any("strides" in p for p in rt.result_problems(out, [t0], "transposed"))
    bad = copy.deepcopy(m0)
    bad.bn.running_mean.add_(1.0)
    assert any("buffer 0 differs" in p for p in rt.result_problems(bad, [m0], "host"))
    bad = copy.deepcopy(m0)
    bad.bn.running_var = m0.bn.running_var  # the very tensor
    assert any("buffer 1 shares" in p for p in rt.result_problems(bad, [m0], "host"))
    bad = copy.deepcopy(m0)
    del bad.bn._buffers["num_batches_tracked"]
    assert any("buffers" in p for p in rt.result_problems(bad, [m0], "host"))


def test_same_params_compares_bits_in_logical_order():
    m0, out = _bn_pair()
    want = rt.param_bits(m0)
    assert rt.same_params(out, want)
    assert rt.same_params(rt.transpose_first_matrix(copy.deepcopy(m0)), want)
    with torch.no_grad():
        out.fc.bias[2] = -out.fc.bias[2]
    assert not rt.same_params(out, want)
    with torch.no_grad():
        out.fc.bias[2] = -out.fc.bias[2]
        out.bn.weight[0] = float("nan")
    m0.bn.weight.data[0] = float("nan")
    assert rt.same_params(out, rt.param_bits(m0))  # NaN against the same NaN: bits, not values

"""The coordinate-wise median and trimmed mean on the MI355X
(dlsim_robust_reduce, dlsim_robust_reduce_tensors,
dasklearn_amd.gradient_aggregation.robust) against the CPU restatement of
their contract (tests/_robust_util.py), bit for bit."""
from __future__ import annotations

import copy
import types

import numpy as np
import pytest
import torch
from torch import nn

import _robust_util as ru
from _sgd_util import BnNet, Net
from sgd_inputs import GNLENET_SHAPES

pytestmark = pytest.mark.gpu

from dasklearn_amd import _native, arena, functions  # noqa: E402
from dasklearn_amd.gradient_aggregation.fedavg import FedAvg  # noqa: E402
from dasklearn_amd.gradient_aggregation.robust import CoordinateMedian, TrimmedMean  # noqa: E402

DEV = "cuda"
FAN_INS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)  # each capacity at its upper edge and one past the previous one
SIZES = {"f32": (1, 3, 4, 5, 1023, 1024, 1025, 4097, 85_354), "bf16": (1, 7, 8, 9, 4097), "f16": (1, 7, 8, 9, 4097),
         "f64": (1, 2, 3, 4097)}


def _check(got: torch.Tensor, want: torch.Tensor, what: str):
    got = got.detach().cpu().reshape(-1)
    assert ru.same_bits(got, want.reshape(-1)), f"{what}: {ru.diff_report(got, want)}"


def _run(xs_dev, lo, hi):
    out = torch.empty_like(xs_dev[0])
    _native.robust_reduce(xs_dev, lo, hi, out)
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "f64"])
@pytest.mark.parametrize("n", FAN_INS)
def test_flat_entry_over_sizes_and_windows(n, dtype):
    """Every size is a prefix of one set of rows, so one sort of the oracle
    serves them all (the result is element-wise)."""
    dt = ru.DTYPES[dtype]
    pmax = max(SIZES[dtype])
    xs = ru.random_rows(dt, n, pmax, seed=1000 + n)
    sb = ru.sorted_bits(xs, dt)
    xd = [x.to(DEV) for x in xs]
    for lo, hi in ru.windows(n):
        want = ru.window_mean_sorted(sb, dt, lo, hi)
        for p in SIZES[dtype]:
            got = _run([x[:p] for x in xd], lo, hi)
            _check(got, want[:p], f"{dtype} n={n} P={p} window=[{lo},{hi})")


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "f64"])
@pytest.mark.parametrize("n", FAN_INS)
def test_specials_in_every_row_position(n, dtype):
    """+-0, +-subnormal, +-finite, +-Inf and NaNs (both signs, a non-canonical
    payload) in every row; all-equal columns; columns already sorted ascending
    and descending across the rows."""
    dt = ru.DTYPES[dtype]
    xs = ru.special_rows(dt, n)
    sb = ru.sorted_bits(xs, dt)
    xd = [x.to(DEV) for x in xs]
    for lo, hi in ru.windows(n):
        _check(_run(xd, lo, hi), ru.window_mean_sorted(sb, dt, lo, hi), f"{dtype} n={n} window=[{lo},{hi})")
    # the scalar kernel on the same columns (a base one element off alignment)
    shifted = [_shifted(x, 1) for x in xs]
    lo = (n - 1) // 2
    for lo, hi in ((lo, lo + 1), (0, n)):
        _check(_run(shifted, lo, hi), ru.window_mean_sorted(sb, dt, lo, hi), f"{dtype} n={n} scalar [{lo},{hi})")


def _shifted(t: torch.Tensor, shift: int) -> torch.Tensor:
    """A device copy of flat `t` whose base is `shift` elements past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[shift:shift + t.numel()]
    v.copy_(t)
    return v


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f64"])
@pytest.mark.parametrize("n", (3, 8, 17, 32))
def test_row_order_does_not_matter(n, dtype):
    dt = ru.DTYPES[dtype]
    xs = ru.random_rows(dt, n, 4099, seed=77 + n)
    perm = np.random.default_rng(n).permutation(n)
    a = [x.to(DEV) for x in xs]
    b = [a[i] for i in perm]
    for lo, hi in ru.windows(n):
        ga, gb = _run(a, lo, hi), _run(b, lo, hi)
        assert ru.same_bits(ga.cpu(), gb.cpu()), f"window [{lo},{hi})"
    _check(ga, ru.window_mean(xs, lo, hi), "the last window against the oracle")


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "f64"])
def test_misaligned_input_then_output(dtype):
    dt = ru.DTYPES[dtype]
    n, p = 5, 4097
    xs = ru.random_rows(dt, n, p, seed=5)
    want = ru.trimmed_mean(xs, 1)
    xd = [x.to(DEV) for x in xs]
    one_off = list(xd)
    one_off[3] = _shifted(xs[3], 1)
    _check(_run(one_off, 1, n - 1), want, "one input off alignment")
    out = torch.empty(p + 16, dtype=dt, device=DEV)[1:p + 1]
    _native.robust_reduce(xd, 1, n - 1, out)
    _check(out, want, "the output off alignment")


def test_overlapping_output_is_refused_and_nothing_runs():
    p = 1000
    buf = torch.zeros(3 * p, device=DEV)
    xs = [buf[:p], buf[p:2 * p]]
    buf[:2 * p] = 1.0
    torch.cuda.synchronize()
    for out in (buf[:p], buf[p // 2:p // 2 + p], buf[2 * p - 1:3 * p - 1]):
        with pytest.raises(_native.DlsimError) as e:
            _native.robust_reduce(xs, 0, 1, out)
        assert e.value.rc == _native.DLSIM_E_ARG and "overlap" in str(e.value)
    torch.cuda.synchronize()
    assert bool((buf[:2 * p] == 1.0).all()) and bool((buf[2 * p:] == 0.0).all())


def _tensor_case(shapes, dtype, n, seed):
    dt = ru.DTYPES[dtype]
    numels = [int(np.prod(s)) for s in shapes]
    rows = ru.random_rows(dt, n, sum(numels), seed)
    offs = np.concatenate([[0], np.cumsum(numels)])[:-1]
    # separate allocations per tensor, as a model's parameters are
    tensors = [[r[o:o + k].clone().to(DEV) for o, k in zip(offs, numels)] for r in rows]
    return dt, numels, rows, offs, tensors


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f64"])
def test_tensors_entry_on_the_gnlenet_shapes(dtype):
    n = 8
    dt, numels, rows, offs, tensors = _tensor_case(GNLENET_SHAPES, dtype, n, seed=11)
    assert sum(numels) == 85_354
    esz = rows[0].element_size()
    for lo, hi in ((3, 4), (2, 6)):
        out = torch.zeros(sum(numels), dtype=dt, device=DEV)
        _native.robust_reduce_tensors_raw([t.data_ptr() for row in tensors for t in row], n, numels,
                                          [int(o) * esz for o in offs], lo, hi, out.data_ptr(),
                                          _native.dtype_code(dt, single_task=True),
                                          torch.cuda.current_stream().cuda_stream)
        _check(out, ru.window_mean(rows, lo, hi), f"{dtype} window [{lo},{hi})")


def test_tensors_entry_skips_a_zero_element_tensor():
    n = 3
    dt, numels, rows, offs, tensors = _tensor_case([[5], [0], [3, 7]], "f32", n, seed=12)
    out = torch.zeros(sum(numels), device=DEV)
    _native.robust_reduce_tensors_raw([t.data_ptr() for row in tensors for t in row], n, numels,
                                      [int(o) * 4 for o in offs], 1, 2, out.data_ptr(), _native.DLSIM_F32,
                                      torch.cuda.current_stream().cuda_stream)
    _check(out, ru.median(rows), "median over three tensors, one empty")


def test_eight_megabyte_rows():
    """The kernels use one launch shape per capacity for every size, so there
    is no class boundary to straddle: one 8 MB-per-row case instead (2049
    blocks and a ragged end)."""
    n, p = 4, 2 * 1024 * 1024 + 5
    rng = np.random.default_rng(8)
    xs = [torch.from_numpy(rng.standard_normal(p, dtype=np.float32)) for _ in range(n)]
    sb = ru.sorted_bits(xs, torch.float32)
    xd = [x.to(DEV) for x in xs]
    for lo, hi in ((1, 2), (1, 3)):
        _check(_run(xd, lo, hi), ru.window_mean_sorted(sb, torch.float32, lo, hi), f"window [{lo},{hi})")


def test_output_past_two_gib_runs_as_ranges():
    """Buffer stores address 32 bits of bytes: a longer output goes as
    consecutive launches. n = 1 copies (no NaN among the inputs), so the
    device checks the result itself."""
    p = ((1 << 31) - (1 << 20)) // 4 + 4099
    x = torch.empty(p, device=DEV).uniform_(-1.0, 1.0)
    out = torch.zeros(p, device=DEV)
    _native.robust_reduce([x], 0, 1, out)
    assert torch.equal(out.view(torch.int32), x.view(torch.int32))


# ---- the plugins, end to end -----------------------------------------------------------
class Mixed(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Parameter(torch.zeros(33, 7))
        self.b = nn.Parameter(torch.zeros(129, dtype=torch.bfloat16))
        self.c = nn.Parameter(torch.zeros(5))
        self.d = nn.Parameter(torch.zeros(4, 9, dtype=torch.bfloat16))


def _filled(make, n, seed, special_frac=0.05):
    """n models from make() whose parameters hold random_rows (specials
    included), every model another draw."""
    models = [make() for _ in range(n)]
    for k, ps in enumerate(zip(*[list(m.parameters()) for m in models])):
        rows = ru.random_rows(ps[0].dtype, n, ps[0].numel(), seed + k, special_frac=special_frac)
        with torch.no_grad():
            for p, r in zip(ps, rows):
                p.copy_(r.reshape(p.shape))
    return models


def _bn():
    m = BnNet()
    with torch.no_grad():
        m.bn.running_mean.uniform_(-1, 1)
        m.bn.num_batches_tracked.fill_(int(torch.randint(1, 99, ()).item()))
    return m


MAKERS = {"gnlenet": lambda: Net(GNLENET_SHAPES, "f32"), "mixed": Mixed, "bn": _bn,
          "f64": lambda: Net([[17, 3], [5]], "f64")}
PLACES = {"host": lambda m: m, "arena": lambda m: arena.to_device_arena(m, DEV),
          "tensors": lambda m: copy.deepcopy(m).to(DEV)}


def _expect(models_cpu, lo, hi):
    return [ru.window_mean([p.detach().reshape(-1) for p in ps], lo, hi)
            for ps in zip(*[list(m.parameters()) for m in models_cpu])]


@pytest.mark.parametrize("place", sorted(PLACES))
@pytest.mark.parametrize("maker", sorted(MAKERS))
def test_plugins_end_to_end(maker, place):
    n = 5
    cpu = _filled(MAKERS[maker], n, seed=500)
    models = [PLACES[place](m) for m in cpu]
    before = [[p.detach().clone() for p in m.parameters()] for m in models]
    for agg, (lo, hi) in ((CoordinateMedian, (2, 3)), (TrimmedMean, (1, 4)), (TrimmedMean.with_trim(2), (2, 3)),
                          (TrimmedMean.with_trim(0), (0, 5))):
        out = agg.aggregate(models)
        assert type(out) is type(models[0])
        want = _expect(cpu, lo, hi)
        got = list(out.parameters())
        assert len(got) == len(want)
        for k, (g, w, p0) in enumerate(zip(got, want, models[0].parameters())):
            assert g.device == p0.device and g.shape == p0.shape and g.dtype == p0.dtype
            assert g.requires_grad == p0.requires_grad
            _check(g, w, f"{agg.__name__} {maker}/{place} parameter {k}")
        for b, b0 in zip(out.buffers(), models[0].buffers()):
            assert b.device == b0.device and torch.equal(b, b0) and b.data_ptr() != b0.data_ptr()
    assert len(list(out.buffers())) == len(list(models[0].buffers()))
    for m, saved in zip(models, before):
        for p, s in zip(m.parameters(), saved):
            assert ru.same_bits(p.detach().cpu(), s.cpu()), "an input model changed"
    # to_host=False keeps a host task's result on the device; True brings a device one back
    out = CoordinateMedian.aggregate(models, to_host=(place != "host"))
    assert all(p.is_cuda == (place == "host") for p in out.parameters())
    for g, w in zip(out.parameters(), _expect(cpu, 2, 3)):
        _check(g, w, "median with to_host overridden")


def test_trim_keyword_and_mismatched_models():
    cpu = _filled(MAKERS["mixed"], 6, seed=900)
    out = TrimmedMean.aggregate(cpu, None, None, 2)
    for g, w in zip(out.parameters(), _expect(cpu, 2, 4)):
        _check(g, w, "trim passed by position")
    out = TrimmedMean.aggregate(cpu, weights=[], trim=0)
    for g, w in zip(out.parameters(), _expect(cpu, 0, 6)):
        _check(g, w, "trim = 0")
    with pytest.raises(ValueError):
        CoordinateMedian.aggregate([cpu[0], nn.Linear(3, 2), cpu[1]])
    with pytest.raises(ValueError):
        TrimmedMean.aggregate([cpu[0], Net([[33, 7], [129], [5]], "f32"), cpu[1]])


def test_a_minority_of_broken_peers_does_not_poison_the_result():
    n = 8
    cpu = _filled(MAKERS["gnlenet"], n, seed=700, special_frac=0.0)  # six honest peers: unit normals
    with torch.no_grad():
        for p in cpu[2].parameters():
            p.fill_(float("inf"))
        for p in cpu[5].parameters():
            p.fill_(float("nan"))
    med = CoordinateMedian.aggregate(cpu)
    tm = TrimmedMean.with_trim(2).aggregate(cpu)
    for got, (lo, hi) in ((med, (3, 4)), (tm, (2, 6))):
        for g, w in zip(got.parameters(), _expect(cpu, lo, hi)):
            assert bool(torch.isfinite(g).all())
            _check(g, w, f"window [{lo},{hi})")
    avg = FedAvg.aggregate(cpu)
    assert not any(bool(torch.isfinite(p).any()) for p in avg.parameters())


@pytest.mark.parametrize("method,trim,window", [(2, None, (2, 3)), (3, None, (1, 5)), (3, 2, (2, 4))])
def test_functions_aggregate_through_model_manager(method, trim, window):
    n = 6
    cpu = _filled(MAKERS["gnlenet"], n, seed=800)
    settings = types.SimpleNamespace(gradient_aggregation=method)
    if trim is not None:
        settings.aggregation_trim = trim
    res = functions.aggregate(settings, {"models": cpu, "round": 1, "peer": 0})
    assert isinstance(res, list) and len(res) == 1
    lo, hi = window
    for g, w in zip(res[0].parameters(), _expect(cpu, lo, hi)):
        assert not g.is_cuda
        _check(g, w, f"method {method} trim {trim}")
    settings.aggregate_on_device = True
    res = functions.aggregate(settings, {"models": cpu, "round": 1, "peer": None})
    for g, w in zip(res[0].parameters(), _expect(cpu, lo, hi)):
        assert g.is_cuda
        _check(g, w, f"method {method} on the device")
    with pytest.raises(ValueError, match="unweighted"):
        functions.aggregate(settings, {"models": cpu, "round": 1, "peer": 0, "weights": [1 / n] * n})

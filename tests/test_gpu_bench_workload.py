"""bench.py's workload on the GPU (round 6): step k reduces input set k mod S
into output k mod O, bit-exact against the oracle, and the decoy set
(ReduceWorkload._prime) is read before anything timed and
is never one of the rotating sets."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "decentralized-learning-simulator_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402
from oracle import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu


def _workload(n, p, monkeypatch, prime="1"):
    from dasklearn_amd import _native
    monkeypatch.setenv("DLSIM_BENCH_PRIME", prime)
    dev = torch.device("cuda", 0)
    w32 = _native.fp32_weights(bench.weights_for("dirichlet", n))
    wl = bench.ReduceWorkload(n, p, "f32", w32, _native.DLSIM_EXACT, 1, dev, 5, torch.cuda.current_stream(dev))
    return wl, w32


def _rows_of(plan):
    return np.stack([t.cpu().numpy() for t in plan._keep[0]])


def test_steps_rotate_sets_and_outputs_bit_exact(monkeypatch):
    n, p = 8, 1_397_760  # the 8-rank slice's shape
    wl, w32 = _workload(n, p, monkeypatch)
    assert wl.sets == 22 and wl.out_sets % wl.sets == 0 and wl.out_sets * p * 4 >= bench.MIN_OUT_FOOTPRINT
    for k in (0, 1, wl.sets - 1, wl.sets, wl.out_sets - 1):
        wl.launch(k)
        torch.cuda.synchronize()
        plan = wl.plans[k % wl.out_sets]
        assert plan._keep[0][0].data_ptr() == wl.plans[k % wl.sets]._keep[0][0].data_ptr()
        want = orc.wreduce_rows_f32(_rows_of(plan), w32)
        assert orc.same_bits(wl.outs[k % wl.out_sets].cpu().numpy(), want), k


def test_decoy_is_read_first_and_is_not_a_rotating_set(monkeypatch):
    n, p = 8, 1_397_760
    wl, w32 = _workload(n, p, monkeypatch)
    decoys = [x for x in wl._keep if isinstance(x, tuple) and len(x) == 3]
    assert len(decoys) == 1
    rows, out, plan = decoys[0]
    # the prime launches ran (synchronised in __init__): the decoy's output is its aggregate
    assert orc.same_bits(out.cpu().numpy(), orc.wreduce_rows_f32(_rows_of(plan), w32))
    lo, hi = rows.data_ptr(), rows.data_ptr() + rows.numel() * 4
    for pl in wl.plans:
        for t in pl._keep[0]:
            assert not lo <= t.data_ptr() < hi
    wl2, _ = _workload(n, p, monkeypatch, prime="0")
    assert not [x for x in wl2._keep if isinstance(x, tuple) and len(x) == 3]


def _plain_run(argv, monkeypatch, capsys):
    """One rank of bench.py in this process with small rotating footprints
    (the run's shape, not its timing, is under test)."""
    import json
    monkeypatch.setenv("DLSIM_BENCH_PRIME", "1")
    monkeypatch.setattr(bench, "MIN_SET_FOOTPRINT", 1 << 20)
    monkeypatch.setattr(bench, "MIN_OUT_FOOTPRINT", 1 << 20)
    assert bench.run_rank(bench.parse(argv), 0, 1, 0) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


@pytest.mark.parametrize("shape,batch", [("3:100003", 1), ("5:70001:bf16", 1), ("4:100003", 3)])
def test_dump_outputs_is_the_last_timed_step_and_repeats(tmp_path, monkeypatch, capsys, shape, batch):
    """--dump-outputs writes the aggregate of step K-1 (input set (K-1) mod S)
    bit for bit as the oracle computes it from that set's rows, the same
    in a second run; a plain line has no leg that takes runs of its own."""
    from dasklearn_amd import _native
    n, p = int(shape.split(":")[0]), int(shape.split(":")[1])
    bf16 = shape.endswith("bf16")
    K = 5
    argv = ["--gpus", "1", "--steps", str(K), "--warmup", "2", "--shape", shape, "--batch", str(batch)]
    lines, arrs = [], []
    for d in ("a", "b"):
        lines.append(_plain_run(argv + ["--dump-outputs", str(tmp_path / d)], monkeypatch, capsys))
        arrs.append(np.load(tmp_path / d / "aggregate.npy"))
    line = lines[0]
    assert line["steps"] == K and line["ms_per_step"] > 0 and line["unit"] == "GB/s" and line["higher_is_better"]
    assert line["dtype"] == ("bf16" if bf16 else "f32")
    assert line["launch_floor"] is None and line["cpu_baseline"] is None and line["roofline"]["traffic"] is None
    assert line["dumped_outputs"]["file"] == "aggregate.npy" and not line["dumped_outputs"]["sampled"]
    assert arrs[0].dtype == np.float32 and arrs[0].shape == ((p,) if batch == 1 else (batch, p))
    assert orc.same_bits(arrs[0], arrs[1])
    # the same workload rebuilt here (same seed, same generator): step K-1's rows through the oracle
    monkeypatch.setattr(bench, "MIN_SET_FOOTPRINT", 1 << 20)
    monkeypatch.setattr(bench, "MIN_OUT_FOOTPRINT", 1 << 20)
    dev = torch.device("cuda", 0)
    w32 = _native.fp32_weights(bench.weights_for("dirichlet", n))
    wl = bench.ReduceWorkload(n, p, "bf16" if bf16 else "f32", w32, _native.DLSIM_EXACT, batch, dev, 1234,
                              torch.cuda.current_stream(dev))
    assert wl.sets >= 3
    plan = wl.plans[(K - 1) % wl.out_sets]
    tasks = [plan._keep[0]] if batch == 1 else [xs for xs, _, _ in plan._keep]
    got = arrs[0].reshape(len(tasks), p)
    for b, rows in enumerate(tasks):
        if bf16:
            bits = [t.view(torch.int16).cpu().numpy().view(np.uint16) for t in rows]
            want = orc.bf16_bits_to_f32(orc.wreduce(bits, w32, "bf16"))
        else:
            want = orc.wreduce_rows_f32(np.stack([t.cpu().numpy() for t in rows]), w32)
        assert orc.same_bits(got[b], want), b


def test_dump_outputs_samples_a_large_output_the_same_way(tmp_path, monkeypatch, capsys):
    """Past the dump budget the file holds a fixed sample of the aggregate:
    the elements dump_sample_index names, in that order."""
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * 1000)
    argv = ["--gpus", "1", "--steps", "4", "--warmup", "1", "--shape", "3:100003"]
    line = _plain_run(argv + ["--dump-outputs", str(tmp_path / "s")], monkeypatch, capsys)
    sample = np.load(tmp_path / "s" / "aggregate.npy")
    assert line["dumped_outputs"]["sampled"] and sample.shape == (1000,)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 << 20)
    _plain_run(argv + ["--dump-outputs", str(tmp_path / "f")], monkeypatch, capsys)
    full = np.load(tmp_path / "f" / "aggregate.npy")
    assert orc.same_bits(sample, full[bench.dump_sample_index(100_003, 1000)])


def test_batched_workload_with_ragged_rows_builds_and_runs(monkeypatch):
    # p * 4 bytes not a multiple of 16: every task's rows and outputs must still
    # be 16-B aligned for the table batch (the decoy's included)
    from dasklearn_amd import _native
    monkeypatch.setenv("DLSIM_BENCH_PRIME", "1")
    dev = torch.device("cuda", 0)
    n, p = 4, 100_003
    w32 = _native.fp32_weights(bench.weights_for("dirichlet", n))
    wl = bench.ReduceWorkload(n, p, "f32", w32, _native.DLSIM_EXACT, 3, dev, 9, torch.cuda.current_stream(dev))
    for k in range(3):
        wl.launch(k)
    torch.cuda.synchronize()
    assert wl.kernel == "dlsim::k_wreduce_batch_table"
    assert all(torch.isfinite(o).all().item() for o in wl.outs[:3])

"""Child of tests/test_gpu_defer_issue.py (TEST INFRASTRUCTURE). The library
reads its A/B switches once per process, so every row count runs in a fresh
interpreter.

    _defer_issue_child.py rows   under DLSIM_AB=1 DLSIM_DEFER_MIN_MB=0 DLSIM_DEFER_R=<R>
    _defer_issue_child.py wide   no switches

Deferred launches checked against the oracle bit for bit; prints one JSON
line of named checks."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "decentralized-learning-simulator_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROW = 2048  # elements of one row of 512 float4


def inputs(n, p, dev):
    """n separately allocated inputs (16-B aligned whatever p is), their host
    copy and the reference's fp32 weights."""
    from oracle import oracle as orc
    g = torch.Generator(device=dev).manual_seed(p + n)
    xs = [torch.randn(p, generator=g, device=dev) * 0.05 for _ in range(n)]
    assert all(x.data_ptr() % 16 == 0 for x in xs)
    host = np.stack([x.cpu().numpy() for x in xs])
    w = orc.reference_weights(n, list(np.random.default_rng(n).dirichlet(np.ones(n))))
    return xs, host, w


def rows(checks):
    """Fan-in 3, 8 and 10 at the compiled R of the switch: two full blocks,
    then (a) a ragged block of one full row, a partial row and a 3-element
    tail, (b) neither, (c) a 2-element tail and no ragged block."""
    from dasklearn_amd import _native
    from oracle import oracle as orc
    dev = torch.device("cuda", 0)
    R = int(os.environ["DLSIM_DEFER_R"])
    checks["switches_seen"] = os.environ.get("DLSIM_AB") == "1" and os.environ.get("DLSIM_DEFER_MIN_MB") == "0"
    for n in (3, 8, 10):
        for p in (2 * R * ROW + ROW + 4 * 37 + 3, 2 * R * ROW, 2 * R * ROW + 2):
            key = f"n{n}_p{p}"
            checks[f"defers_{key}"] = _native.kernel_name(n, p, torch.float32) == "dlsim::k_wreduce_defer_pre"
            xs, host, w = inputs(n, p, dev)
            out = torch.empty_like(xs[0])
            _native.wreduce(xs, w, out)
            checks[f"exact_{key}"] = orc.same_bits(out.cpu().numpy(), orc.wreduce_rows_f32(host, w))
            out.zero_()
            _native.wreduce(xs, w, out, _native.DLSIM_FAST)
            checks[f"fast_{key}"] = orc.same_bits(out.cpu().numpy(), orc.wreduce(list(host), w, "f32", mode="fast"))
            out.zero_()
            _native.mean(xs, out)
            checks[f"mean_{key}"] = orc.same_bits(out.cpu().numpy(), orc.mean(list(host), "f32"))


def wide(checks):
    """Fan-in 12 and 14 defer only from 16 rows per CU: the smallest size that
    does, exact."""
    from dasklearn_amd import _native
    from oracle import oracle as orc
    dev = torch.device("cuda", 0)
    p = 8_400_000
    for n in (12, 14):
        checks[f"defers_n{n}"] = _native.kernel_name(n, p, torch.float32) == "dlsim::k_wreduce_defer_pre"
        xs, host, w = inputs(n, p, dev)
        out = torch.empty_like(xs[0])
        _native.wreduce(xs, w, out)
        checks[f"exact_n{n}"] = orc.same_bits(out.cpu().numpy(), orc.wreduce_rows_f32(host, w))
        del xs, host, out


def main():
    checks = {}
    {"rows": rows, "wide": wide}[sys.argv[1]](checks)
    torch.cuda.synchronize()
    print(json.dumps({"case": sys.argv[1], "r": os.environ.get("DLSIM_DEFER_R"), "checks": checks}), flush=True)


if __name__ == "__main__":
    main()

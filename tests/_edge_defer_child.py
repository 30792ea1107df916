"""Child of tests/test_gpu_edges_defer.py (TEST INFRASTRUCTURE). The library
reads its A/B switches once per process, so every row count runs in a fresh
interpreter.

    _edge_defer_child.py rows      under DLSIM_AB=1 DLSIM_DEFER_MIN_MB=0 DLSIM_DEFER_R=<R>
    _edge_defer_child.py default   no switches

Deferred launches into guarded outputs, specials at the edges of the R-row
blocks, every case through _edge_util.reduce_case (guards clean, view bit-equal
to the oracle, inputs unchanged); prints one JSON line of named checks, and
under "problems" what a failed check found, with the names of the specials
columns that differ."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "decentralized-learning-simulator_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _edge_util as eu  # noqa: E402

ROW = 2048  # elements of one row of 512 float4
CASES = (("exact", eu.WEIGHT_KINDS), ("fast", ("dirichlet", "zero_in_middle")), ("mean", ("dirichlet",)))


def differing_columns(rows, w, op, n, positions):
    """Names of the specials columns whose result differs from the oracle's
    (a second launch into a plain output: only to name them)."""
    from dasklearn_amd import _native
    dev = torch.device("cuda", 0)
    xs = eu.place(list(rows), "f32", dev)
    out = torch.empty(rows.shape[1], device=dev)
    if op == "mean":
        _native.mean(xs, out)
    else:
        _native.wreduce(xs, w, out, _native.DLSIM_EXACT if op == "exact" else _native.DLSIM_FAST)
    got, exp = out.cpu().numpy(), eu.expected_reduce(op, rows, w, "f32")
    both_nan = np.isnan(got) & np.isnan(exp)
    bad = (got.view(np.uint32) != exp.view(np.uint32)) & ~both_nan
    _, names = eu.special_block("f32", n)
    hit = set()
    for q in positions:
        for c, name in enumerate(names):
            if q + c < bad.size and bad[q + c]:
                hit.add(name)
    return sorted(hit)


def run(checks, problems, n, p, tile, want_kernel):
    from dasklearn_amd import _native
    dev = torch.device("cuda", 0)
    positions = eu.edge_positions(p, tile, 4)
    rows = eu.special_rows("f32", n, p, positions, seed=n + p % 997)
    for op, kinds in CASES:
        mode = None if op == "mean" else _native.DLSIM_EXACT if op == "exact" else _native.DLSIM_FAST
        checks[f"defers_{op}_n{n}_p{p}"] = _native.kernel_name(n, p, torch.float32, mode) == want_kernel
        for kind in kinds:
            w = eu.special_weights(n, kind, "f32")
            found = eu.reduce_case(op, "f32", rows, w, dev)
            key = f"{op}_{kind}_n{n}_p{p}"
            checks[key] = not found
            if found:
                problems[key] = found + ["specials columns that differ: " +
                                         ", ".join(differing_columns(rows, w, op, n, positions))]


def rows_case(checks, problems):
    """Fan-in 3 and 8 (exact: the kernel compiled for an even R, the runtime-R
    form for an odd one; FAST and mean: runtime R) and 17 (the grouped form)
    at P = 2 R 2048 + 2048 + 4*37 + 3 (two full blocks, a ragged block of one
    full row, a partial row and a 3-element tail), 2 R 2048 + 2 (a tail where
    a store to vector nvec would land, no ragged block) and 2 R 2048 (the
    guard there)."""
    R = int(os.environ["DLSIM_DEFER_R"])
    checks["switches_seen"] = os.environ.get("DLSIM_AB") == "1" and os.environ.get("DLSIM_DEFER_MIN_MB") == "0"
    for n in (3, 8, 17):
        for p in (2 * R * ROW + ROW + 4 * 37 + 3, 2 * R * ROW + 2, 2 * R * ROW):
            run(checks, problems, n, p, R * ROW, "dlsim::k_wreduce_defer_pre" if n <= 14 else "dlsim::k_wreduce_defer")


def default_case(checks, problems):
    """No switches: fan-in 3 at 2,500,003 elements, the smallest size class
    that defers by default (10 MB per stream; one round of blocks with every
    CU busy: dispatch.hpp defer_rows gives R = 6 on 256 CUs)."""
    checks["no_switches"] = not any(k.startswith("DLSIM_") for k in os.environ)
    p = 2_500_003
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    t = (p // 4 + 511) // 512
    r = max(((t + cus - 1) // cus + 1) & ~1, 4)
    checks["one_round_of_rows"] = r <= 24
    run(checks, problems, 3, p, r * ROW, "dlsim::k_wreduce_defer_pre")


def main():
    checks, problems = {}, {}
    {"rows": rows_case, "default": default_case}[sys.argv[1]](checks, problems)
    torch.cuda.synchronize()
    print(json.dumps({"case": sys.argv[1], "r": os.environ.get("DLSIM_DEFER_R"), "checks": checks,
                      "problems": problems}), flush=True)


if __name__ == "__main__":
    main()

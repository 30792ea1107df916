"""Child of tests/test_gpu_defer_matrix.py (TEST INFRASTRUCTURE). The library
reads its A/B switches once per process, so every row count runs in a fresh
interpreter, under DLSIM_AB=1 DLSIM_DEFER_MIN_MB=0 DLSIM_DEFER_R=<R>:

    _defer_matrix_child.py narrow <ops>      ops: exact, alias, fast, mean (comma separated)
    _defer_matrix_child.py wide <fan-ins>    fan-ins out of 11..14 (comma separated)

Deferred launches into guarded outputs, specials at the edges of the R-row
blocks, every case through _edge_util.reduce_case (guards clean, view bit-equal
to the oracle, inputs unchanged). Prints one JSON line of named checks, under
"problems" what a failed check found (with the names of the specials columns
that differ), and the child's wall time."""
import json
import os
import sys
import time

T0 = time.perf_counter()
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "decentralized-learning-simulator_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _edge_util as eu  # noqa: E402
from _edge_defer_child import differing_columns  # noqa: E402

ROW = 2048  # elements of one row of 512 float4
DEFER_PRE = "dlsim::k_wreduce_defer_pre"
KINDS = {"exact": ("dirichlet", "zero_in_middle"), "fast": ("dirichlet", "zero_in_middle"), "mean": ("dirichlet",)}
WIDE_ROWS_PER_CU = 16  # dispatch.hpp kDeferWideRowsPerCu
WIDE_MAX_FAN_IN = 14


def run_op(checks, problems, op, n, p, rows, positions, kinds, expected=None):
    """The kernel's name for (op, n, p), then one guarded launch per weight kind."""
    from dasklearn_amd import _native
    dev = torch.device("cuda", 0)
    mode = None if op == "mean" else _native.DLSIM_EXACT if op == "exact" else _native.DLSIM_FAST
    checks[f"defers_{op}_n{n}"] = _native.kernel_name(n, p, torch.float32, mode) == DEFER_PRE
    for kind in kinds:
        w = eu.special_weights(n, kind, "f32")
        exp = None if expected is None else expected(rows, w)
        found = eu.reduce_case(op, "f32", rows, w, dev, expected=exp)
        key = f"{op}_{kind}_n{n}"
        checks[key] = not found
        if found:
            problems[key] = found + ["specials columns that differ: " +
                                     ", ".join(differing_columns(rows, w, op, n, positions))]


def narrow(checks, problems, ops):
    """Fan-in 3..10 at P = 2 R 2048 + 2048 + 4*37 + 3: two full blocks, a
    ragged block of one full row and a partial row, and a 3-element tail.
    exact: the kernel compiled for an even R (the runtime-R form for an odd
    one); alias: exact with the output aliasing input 0, then the last input;
    fast and mean: the runtime-R form."""
    dev = torch.device("cuda", 0)
    R = int(os.environ["DLSIM_DEFER_R"])
    p = 2 * R * ROW + ROW + 4 * 37 + 3
    positions = eu.edge_positions(p, R * ROW, 4)
    for n in range(3, 11):
        rows = eu.special_rows("f32", n, p, positions, seed=n + p % 997)
        for op in ops:
            if op != "alias":
                run_op(checks, problems, op, n, p, rows, positions, KINDS[op])
                continue
            w = eu.special_weights(n, "dirichlet", "f32")
            for idx in (0, n - 1):
                found = eu.reduce_case("exact", "f32", rows, w, dev, alias=True, alias_index=idx)
                key = f"alias{'_first' if idx == 0 else '_last'}_dirichlet_n{n}"
                checks[key] = not found
                if found:
                    problems[key] = found


def wide(checks, problems, fan_ins):
    """Fan-in 11..14 defer only from 16 rows per CU: the smallest size that
    does, plus a ragged block and a 3-element tail. One 14-row random set
    drawn on the device; fan-in n takes its first n rows, with the specials
    block of fan-in n at the edges of the R-row blocks."""
    from oracle import oracle as orc
    dev = torch.device("cuda", 0)
    R = int(os.environ["DLSIM_DEFER_R"])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    p = WIDE_ROWS_PER_CU * cus * ROW + ROW + 4 * 37 + 3
    g = torch.Generator(device=dev).manual_seed(p)
    host = np.stack([(torch.randn(p, generator=g, device=dev) * 0.05).cpu().numpy() for _ in range(WIDE_MAX_FAN_IN)])
    host = eu.avoid_fill(host, "f32").reshape(WIDE_MAX_FAN_IN, p)
    torch.cuda.empty_cache()
    positions = eu.edge_positions(p, R * ROW, 4)
    for n in fan_ins:
        rows = host[:n].copy()
        block, _ = eu.special_block("f32", n)
        for q in positions:
            width = min(block.shape[1], p - q)
            rows[:, q:q + width] = block[:, :width]
        run_op(checks, problems, "exact", n, p, rows, positions, ("dirichlet",), expected=orc.wreduce_rows_f32)
        del rows
        torch.cuda.empty_cache()
    return p


def main():
    checks, problems = {}, {}
    case, arg = sys.argv[1], sys.argv[2]
    checks["switches_seen"] = os.environ.get("DLSIM_AB") == "1" and os.environ.get("DLSIM_DEFER_MIN_MB") == "0"
    if case == "narrow":
        narrow(checks, problems, arg.split(","))
    else:
        wide(checks, problems, [int(v) for v in arg.split(",")])
    torch.cuda.synchronize()
    print(json.dumps({"case": case, "arg": arg, "r": os.environ.get("DLSIM_DEFER_R"), "checks": checks,
                      "problems": problems, "wall_s": round(time.perf_counter() - T0, 2)}), flush=True)


if __name__ == "__main__":
    main()

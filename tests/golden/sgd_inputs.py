"""Deterministic inputs and file format of the SGD-step fixtures
(tests/golden/sgd/*.npz), shared by make_golden_sgd.py and the tests. Data
only: no reference code."""
from __future__ import annotations

import io
import json
import os
import zipfile

import numpy as np

SGD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sgd")

# GNLeNet(3, 10, (32, 32)).parameters(): 14 tensors, 85,354 elements
GNLENET_SHAPES = [[32, 3, 5, 5], [32], [32], [32], [32, 32, 5, 5], [32], [32], [32], [64, 32, 5, 5], [64], [64], [64],
                  [10, 576], [10]]

NP_DTYPES = {"f32": np.float32, "f64": np.float64, "bf16": np.uint16, "f16": np.float16}


def f32_to_bf16_bits(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 bit patterns, round to nearest even (NaN -> 0x7fc0)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7fc0), r)


def seeded_pair(p: int, seed: int, dtype: str):
    """(parameters, gradients): N(0,1) * 0.05 and N(0,1) * 0.01 from one PCG64
    stream, in the fixture's storage dtype (bf16 as uint16 bits)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal((2, p))
    a, g = x[0] * 0.05, x[1] * 0.01
    if dtype == "f64":
        return a, g
    a, g = a.astype(np.float32), g.astype(np.float32)
    if dtype == "bf16":
        return f32_to_bf16_bits(a), f32_to_bf16_bits(g)
    return a, g


def numel(shapes) -> int:
    return sum(int(np.prod(s)) for s in shapes)


def save_npz(path: str, arrays: dict) -> None:
    """np.savez_compressed with fixed member timestamps, so regenerating a
    fixture gives the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(zi, buf.getvalue())


def sgd_paths():
    import glob
    return sorted(glob.glob(os.path.join(SGD_DIR, "*.npz")))


def load_sgd(path: str) -> dict:
    """One fixture (no pickle): meta, params, grads (flat over the first
    meta["n_grads"] shapes), expected, buffers (flat, may be empty). Seeded
    inputs are regenerated and checked against the stored hash."""
    import hashlib
    with np.load(path, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    meta = d["meta"] = json.loads(str(d["meta"]))
    if "params" not in d:
        a, g = seeded_pair(numel(meta["shapes"]), meta["seed"], meta["dtype"])
        g = g[:numel(meta["shapes"][:meta["n_grads"]])]
        assert hashlib.sha256(a.tobytes() + g.tobytes()).hexdigest() == str(d["inputs_sha256"]), \
            "regenerated inputs differ from the ones the reference saw"
        d["params"], d["grads"] = a, g
    return d


def split(flat: np.ndarray, shapes):
    out, off = [], 0
    for s in shapes:
        k = int(np.prod(s))
        out.append(flat[off:off + k].reshape(s))
        off += k
    return out

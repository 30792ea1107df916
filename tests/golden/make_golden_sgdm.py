"""Golden vectors for the momentum-SGD step from the REFERENCE.

Runs the reference's own `SGDOptimizer` (/root/reference/dasklearn/optimizer/
sgd.py) the way `ModelTrainer.train` does (model_trainer.py:89-92,126): three
rounds, each a fresh SGDOptimizer, `load_state_dict` of the previous round's
optimizer, then zero_grad / gradients / `optimizer.optimizer.step()` for one or
two local steps, at the worker's 4 torch threads (broker.py:31). Writes the
final parameters and momentum buffers as .npz data under tests/golden/sgdm/
(format: sgdm_inputs.py). Skips when /root/reference is absent. Regenerating
gives the same bytes.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sgdm.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from sgd_inputs import GNLENET_SHAPES, f32_to_bf16_bits, save_npz, split  # noqa: E402
from sgdm_inputs import BUF_SUFFIX, MAX_BYTES, SGDM_DIR, case_inputs, inputs_hash  # noqa: E402


def main() -> int:
    if not os.path.isdir(REF):
        print("reference absent; nothing to do")
        return 0
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import torch
    from torch import nn
    from dasklearn.optimizer.sgd import SGDOptimizer

    torch.set_num_threads(4)
    tdt = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16}

    def to_t(a, dtype):
        if dtype == "bf16":
            return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16)
        return torch.from_numpy(a.copy())

    def to_np(t, dtype):
        t = t.detach().contiguous().reshape(-1)
        if dtype == "bf16":
            return t.view(torch.int16).numpy().view(np.uint16).copy()
        return t.numpy().copy()

    class Net(nn.Module):
        def __init__(self, shapes, dtype):
            super().__init__()
            self.ps = nn.ParameterList([nn.Parameter(torch.zeros(*s, dtype=tdt[dtype])) for s in shapes])

    os.makedirs(SGDM_DIR, exist_ok=True)
    written = []

    def run_case(case, dtype, shapes, lr, momentum, wd, rounds, none=(), seed=None, stored=None):
        meta = dict(case=case, dtype=dtype, shapes=shapes, lr=lr, momentum=momentum, weight_decay=wd,
                    rounds=list(rounds), none=[list(x) for x in none], seed=seed, torch_threads=4,
                    torch_version=torch.__version__, cpu_capability=torch.backends.cpu.get_cpu_capability())
        params, grads, buf0 = (*case_inputs(meta), None) if stored is None else stored
        model = Net(shapes, dtype)
        with torch.no_grad():
            for p, a in zip(model.parameters(), split(params, shapes)):
                p.copy_(to_t(a, dtype).reshape(p.shape))
        previous = None
        if buf0 is not None:  # the optimizer of an earlier round, holding these buffers
            previous = SGDOptimizer(model, lr, momentum, wd)
            for p, b in zip(model.parameters(), split(buf0, shapes)):
                previous.optimizer.state[p]["momentum_buffer"] = to_t(b, dtype).reshape(p.shape)
        skip = {tuple(x) for x in none}
        step = 0
        for n_steps in rounds:
            optimizer = SGDOptimizer(model, lr, momentum, wd)
            if previous is not None:
                optimizer.optimizer.load_state_dict(previous.optimizer.state_dict())
            previous = optimizer
            for _ in range(n_steps):
                optimizer.optimizer.zero_grad()
                for k, (p, g) in enumerate(zip(model.parameters(), split(grads[step], shapes))):
                    if (step, k) not in skip:
                        p.grad = to_t(g, dtype).reshape(p.shape)
                optimizer.optimizer.step()
                step += 1
        expected = np.concatenate([to_np(p, dtype) for p in model.parameters()])
        bufs = np.concatenate([to_np(previous.optimizer.state[p]["momentum_buffer"], dtype)
                               for p in model.parameters()])
        arrays = dict(meta=np.array(json.dumps(meta)), expected=expected, expected_buf=bufs)
        if seed is None:
            arrays.update(params=params, grads=np.stack(grads), buf0=buf0 if buf0 is not None else np.zeros(0))
        else:
            arrays["inputs_sha256"] = np.array(inputs_hash(params, grads))
        path = os.path.join(SGDM_DIR, case + ".npz")
        save_npz(path, arrays)
        if os.path.getsize(path) >= MAX_BYTES:  # parameters and buffers in separate files
            save_npz(path, {k: v for k, v in arrays.items() if k != "expected_buf"})
            save_npz(path[:-4] + BUF_SUFFIX + ".npz", dict(expected_buf=bufs))
            written.append(path[:-4] + BUF_SUFFIX + ".npz")
        written.append(path)

    # ---- GNLeNet's 14 shapes, 85,354 elements: three rounds of 1, 2 and 2 local steps ----
    for dtype, wd, seed in (("f32", 5e-4, 41), ("f32", 0.0, 51), ("bf16", 5e-4, 61), ("bf16", 0.0, 71),
                            ("f64", 5e-4, 81)):
        run_case(f"gnlenet_{dtype}_{'wd' if wd else 'nowd'}", dtype, GNLENET_SHAPES, 0.1, 0.9, wd, (1, 2, 2),
                 seed=seed)
    # ---- two tensors without a gradient on the first step: they get their buffers on step 2 ----
    for dtype, seed in (("f32", 91), ("bf16", 101)):
        run_case(f"none_{dtype}", dtype, GNLENET_SHAPES, 0.1, 0.9, 5e-4, (1, 2, 1), none=((0, 3), (0, 12)),
                 seed=seed)
    # ---- special values in parameter x gradient x buffer (9^3 = 729 elements), one later step ----
    for dtype in ("f32", "bf16", "f64"):
        f = np.float64 if dtype == "f64" else np.float32
        tiny = np.finfo(f).tiny
        vals = np.array([0.0, -0.0, tiny / 4, -tiny, np.inf, -np.inf, np.nan, 1.5, -2.25e-3], dtype=f)
        pa, ga, ba = [x.reshape(-1).copy() for x in np.meshgrid(vals, vals, vals, indexing="ij")]
        if dtype == "bf16":
            pa, ga, ba = f32_to_bf16_bits(pa), f32_to_bf16_bits(ga), f32_to_bf16_bits(ba)
        for wd in (0.0, 0.25):
            run_case(f"specials_{dtype}_{'wd' if wd else 'nowd'}", dtype, [[pa.size]], 0.5, 0.75, wd, (1,),
                     stored=(pa, [ga], ba))
    for p in written:
        assert os.path.getsize(p) < MAX_BYTES, (p, os.path.getsize(p))
    print("wrote %d files" % len(written))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Krum and Multi-Krum (Blanchard et al., 2017) on the MI355X: the fourth and
fifth plugins behind `GradientAggregationMethod` (KRUM = 4, MULTI_KRUM = 5),
and `model_distances`, the consensus distance between n models.

The reference has one aggregator, FedAvg (dasklearn/gradient_aggregation/
fedavg.py), and measures no distance between models; the coordinate-wise
rules of robust.py judge every element on its own. Against a peer that sends a
plausible-looking model that is wrong as a whole (scaled, sign-flipped,
trained on poisoned labels) the standard defences are distance-based.

The rule, for n models, a Byzantine count f >= 0 with n >= 2f + 3, and the
matrix d2 of squared L2 distances between the models' parameters
(`model_distances`: one HIP kernel per dtype group, csrc/pairdist_kernels.hpp,
every term in double):

    D[i][j]  = d2[i][j] if finite, else +Inf
    score[i] = the n - f - 2 smallest D[i][j], j != i, added in ascending order
    ranking  = by (score, index): ties and all-Inf scores go to the lower index

A peer with a NaN or Inf parameter has an infinite score and is never chosen
while enough finite peers remain. Krum returns the first-ranked model: its
parameters are a plain copy of that model's, bit for bit. Multi-Krum(m),
1 <= m <= n - f (default n - f), takes the m first-ranked models in ascending
index order through the exact weighted reduce with float(1./m) each: its
parameters equal FedAvg.aggregate(selected) bit for bit. Scores and selection
are computed on the host in Python floats.

As in every plugin here, buffers and attributes are copy.deepcopy(models[0])'s
and the inputs are only read. Both are unweighted: `weights` of None or [] is
accepted; a non-empty list of another length than the models raises
AssertionError (as FedAvg), one of the right length ValueError. An empty model
list raises IndexError; more than 32 models, or a model whose parameter list
differs from models[0]'s, ValueError.

Cost: the selection needs the matrix on the host, so a single aggregate pays
one D2H copy of n*n doubles and one stream synchronisation between the
distance kernel and the copy or reduce that follows. The aggregates of one
simulated round (`RoundExecutor`, `aggregate_batch`) share them: every task's
matrix comes from batched launches (csrc/pairdist_batch_kernels.hpp, DESIGN.md
§8n) into one device buffer, one D2H copy and one synchronisation per device
serve the whole wave, and the copies or reduces that follow are batched too
(`model_inputs.krum_arena_tasks`). `model_distances_batch` is that first phase
on its own. A device-side selection is not implemented.
"""
import math
from typing import List, Optional, Sequence

import torch
from torch import nn

from dasklearn_amd import _native
from dasklearn_amd.arena import _target_device, input_arenas
from dasklearn_amd.gradient_aggregation import GradientAggregation
from dasklearn_amd.gradient_aggregation.robust import _check_unweighted
from dasklearn_amd.model_inputs import (bulyan_modules, distances_arena_tasks, krum_modules,  # noqa: F401
                                        model_distances)  # (model_distances: public here)
from dasklearn_amd.wave_tasks import ArenaTask


def _resident_entry(models: List[nn.Module], device) -> Optional[ArenaTask]:
    """`models` as a task of distances_arena_tasks when every parameter is
    on one CUDA device (`device`, when given) as an arena or as contiguous
    separate tensors; None when something would have to be copied first."""
    layout, all_params, views = input_arenas(models)  # ZipMismatch is a ValueError
    dev = None
    resolved = {}
    for dt, idx in layout.groups.items():
        vs = views[dt]
        ts = list(vs) if vs is not None else [ps[k] for ps in all_params for k in idx]
        if vs is None:
            if not all(t.is_contiguous() for t in ts):
                return None
            vs = [None] * len(models)
        for t in ts:
            if not t.is_cuda or (dev is not None and t.device != dev):
                return None
            dev = t.device
        resolved[dt] = vs
    if dev is None or (device is not None and dev != _target_device((), device)):
        return None
    return ArenaTask(models[0], layout, resolved, None, all_params)


def model_distances_batch(tasks: Sequence[List[nn.Module]], device=None) -> List[torch.Tensor]:
    """model_distances for every list of models in `tasks` (the consensus
    distance of every neighbourhood of a round) in one call: the matrices of
    the device-resident tasks come from batched launches, one D2H copy and one
    stream synchronisation per device (model_inputs.distances_arena_tasks);
    a task with a host model, a model on another device or a non-contiguous
    parameter goes through model_distances. Each matrix is bit-identical to
    model_distances(models, device); the exceptions are its too."""
    results: List[Optional[torch.Tensor]] = [None] * len(tasks)
    prepared, where = [], []
    for ti, models in enumerate(tasks):
        models[0]  # IndexError for an empty list, as model_distances
        _native.check_pairdist_fan_in(len(models))
        entry = _resident_entry(models, device)
        if entry is None:
            results[ti] = model_distances(models, device)
            continue
        prepared.append(entry)
        where.append(ti)
    for ti, d2 in zip(where, distances_arena_tasks(prepared)):
        results[ti] = d2
    return results


def check_krum_params(n: int, f: int, m: int = 1) -> None:
    """ValueError unless f >= 0, n >= 2f + 3 and 1 <= m <= n - f."""
    if f < 0 or n < 2 * f + 3:
        raise ValueError(f"Krum over n = {n} models with f = {f} Byzantine ones: needs f >= 0 and n >= 2*f + 3")
    if not 1 <= m <= n - f:
        raise ValueError(f"Multi-Krum over n = {n} models with f = {f}: m = {m} must satisfy 1 <= m <= n - f")


def krum_scores(d2: Sequence[Sequence[float]], f: int) -> List[float]:
    """score[i] of the n x n matrix d2 (any nested sequence of floats): the
    sum, in ascending order, of the n - f - 2 smallest entries of row i off the
    diagonal, a non-finite entry counting as +Inf."""
    n = len(d2)
    f = int(f)
    check_krum_params(n, f)
    scores = []
    for i in range(n):
        row = sorted((float(d2[i][j]) if math.isfinite(d2[i][j]) else math.inf) for j in range(n) if j != i)
        s = 0.0
        for v in row[:n - f - 2]:
            s += v
        scores.append(s)
    return scores


def krum_select(d2: Sequence[Sequence[float]], f: int, m: int = 1) -> List[int]:
    """The indices of the m models ranked first by (score, index), in
    ascending index order."""
    n = len(d2)
    f, m = int(f), int(m)
    check_krum_params(n, f, m)
    scores = krum_scores(d2, f)
    return sorted(sorted(range(n), key=lambda i: (scores[i], i))[:m])


def check_bulyan_params(n: int, f: int) -> None:
    """ValueError unless f >= 0 and n >= 4f + 3."""
    if f < 0 or n < 4 * f + 3:
        raise ValueError(f"Bulyan over n = {n} models with f = {f} Byzantine ones: needs f >= 0 and n >= 4*f + 3")


def bulyan_select(d2: Sequence[Sequence[float]], f: int) -> List[int]:
    """Bulyan's first stage on the n x n matrix d2 (any nested sequence of
    floats): Krum run theta = n - 2f times, each time over the models that are
    left. D as for Krum (a non-finite entry counts as +Inf). R = all indices;
    theta times, with r = |R|:

        score[i] = the k = min(r - 1, max(1, r - f - 2)) smallest D[i][j],
                   j in R without i, added in ascending order (k = 0 for r = 1)
        the minimum by (score, index) leaves R and is chosen

    Returns the theta chosen indices in ascending order. While r >= 2f + 3, k
    is Krum's r - f - 2. The paper does not say what Krum means below 2f + 3
    remaining models, which the last rounds reach; clamping k into [1, r - 1]
    (the nearest neighbour at least, never more neighbours than there are) is
    this library's choice."""
    n = len(d2)
    f = int(f)
    check_bulyan_params(n, f)
    D = [[float(d2[i][j]) if math.isfinite(d2[i][j]) else math.inf for j in range(n)] for i in range(n)]
    left = list(range(n))
    chosen = []
    for _ in range(n - 2 * f):
        r = len(left)
        k = min(r - 1, max(1, r - f - 2))
        best = None
        for i in left:
            s = 0.0
            for v in sorted(D[i][j] for j in left if j != i)[:k]:
                s += v
            if best is None or (s, i) < best:
                best = (s, i)
        left.remove(best[1])
        chosen.append(best[1])
    return sorted(chosen)


class Krum(GradientAggregation):
    """The one model closest to its n - f - 2 nearest neighbours; f Byzantine
    peers are tolerated among n >= 2f + 3."""

    f = 1

    @classmethod
    def aggregate(cls, models: List[nn.Module], weights: Optional[List[float]] = None,
                  to_host: Optional[bool] = None) -> nn.Module:
        """to_host=None (default): the result lives where models[0] lives;
        False keeps it on the GPU."""
        _check_unweighted("Krum", models, weights)
        return krum_modules(models, cls.f, None, to_host=to_host)

    @classmethod
    def with_params(cls, f: int, m: Optional[int] = None):
        """A Krum class for Byzantine count f: the plugin signature
        ModelManager calls. m is accepted for symmetry and must be None or 1."""
        f = int(f)
        if f < 0:
            raise ValueError(f"f must be >= 0 (got {f})")
        if m is not None and int(m) != 1:
            raise ValueError(f"Krum selects one model (got m = {m}); MultiKrum takes m")
        return type(f"Krum{f}", (cls,), {"f": f})


class MultiKrum(GradientAggregation):
    """The mean of the m first-ranked models (default m = n - f)."""

    f = 1
    m: Optional[int] = None

    @classmethod
    def aggregate(cls, models: List[nn.Module], weights: Optional[List[float]] = None,
                  to_host: Optional[bool] = None) -> nn.Module:
        _check_unweighted("MultiKrum", models, weights)
        models[0]  # IndexError for an empty list, as FedAvg
        m = len(models) - cls.f if cls.m is None else cls.m
        return krum_modules(models, cls.f, m, to_host=to_host)

    @classmethod
    def with_params(cls, f: int, m: Optional[int] = None):
        """A MultiKrum class for Byzantine count f that averages m models
        (None: n - f of the n it is given)."""
        f = int(f)
        if f < 0:
            raise ValueError(f"f must be >= 0 (got {f})")
        if m is not None:
            m = int(m)
            if m < 1:
                raise ValueError(f"m must be >= 1 (got {m})")
        return type(f"MultiKrum{f}" + ("" if m is None else f"x{m}"), (cls,), {"f": f, "m": m})


class Bulyan(GradientAggregation):
    """Bulyan (El Mhamdi et al., 2018): Krum's selection run theta = n - 2f
    times (bulyan_select), then, per parameter element, the mean of the
    theta - 2f values closest to the median of the selected models' values
    (robust.MeanAroundMedian's rule and kernel). A distance-based selection
    followed by a coordinate-wise rule: a peer that passes Krum with one
    poisoned coordinate is caught by the second stage. f Byzantine peers are
    tolerated among n >= 4f + 3. A variant of MULTI_KRUM
    (`settings.aggregation_krum_rule = "bulyan"`).

    The parameters equal MeanAroundMedian.aggregate(selected, keep=theta - 2f)
    bit for bit, the selected models in ascending index order; buffers,
    attributes and strides are copy.deepcopy(models[0])'s. Cost: as Multi-Krum,
    one D2H copy of n*n doubles and one stream synchronisation; the second
    stage reads the rows the distances read. The aggregates of a round run
    task by task (no batched form yet)."""

    f = 1

    @classmethod
    def aggregate(cls, models: List[nn.Module], weights: Optional[List[float]] = None,
                  to_host: Optional[bool] = None) -> nn.Module:
        _check_unweighted("Bulyan", models, weights)
        return bulyan_modules(models, cls.f, to_host=to_host)

    @classmethod
    def with_params(cls, f: int):
        """A Bulyan class for Byzantine count f: the plugin signature
        ModelManager calls."""
        f = int(f)
        if f < 0:
            raise ValueError(f"f must be >= 0 (got {f})")
        return type(f"Bulyan{f}", (cls,), {"f": f})

"""The geometric median and centered clipping on the MI355X: the sixth and
seventh plugins behind `GradientAggregationMethod` (GEOMETRIC_MEDIAN = 6,
CENTERED_CLIP = 7), and `aggregate_with_distances` / `consensus_distance`, the
weighted mean together with every model's squared distance to it.

The reference has one aggregator, FedAvg (dasklearn/gradient_aggregation/
fedavg.py). Krum and Multi-Krum (krum.py) select a few peers; these two rules
keep information from every honest peer:

  * GeometricMedian: RFA, the smoothed Weiszfeld iteration (Pillutla, Kakade
    and Harchaoui, 2022);
  * CenteredClip: centered clipping (Karimireddy, He and Jaggi, 2021).

Both run one loop: the distance of every peer to the current centre, weights
from the distances, a weighted mean. One HIP kernel does the mean and the
distances to it in a single pass over the models (dlsim_wreduce_dist,
csrc/reducedist_kernels.hpp): T iterations are T + 1 launches
per dtype group. The scalar rules run on the host in Python floats, every sum
in index order:

  weights    `weights` alpha may be given; None or [] means float(1./n) each; a
             wrong length raises AssertionError (as FedAvg). Every weight
             handed to the kernel is first rounded to fp32,
             float(np.float32(w)), for fp64 models too.
  exclusion  a model with any non-finite parameter is excluded before anything
             else: the kept set K is exactly {i : all isfinite(x_i)}. (Pass 0
             runs over all models; only if some d2 of it is non-finite is each
             model checked alone, by a 1-way call with weight 1.0, whose d2 is
             +0.0 for a finite row and non-finite for any other.) If no model
             is finite the result is FedAvg over all of them (non-finite, as
             FedAvg's is); nothing is raised.
  pass 0     FedAvg over K: with alpha as given when K is everyone (zero
             iterations then equal FedAvg.aggregate(models, weights) bit for
             bit, for fp32-representable weights on fp64 models), else with
             alpha_i / sum_K alpha.
  GeometricMedian(nu > 0, T >= 0)
             iteration t uses the distances of pass t - 1:
             beta_i = alpha_i / max(nu, sqrt(d2_i)), 0 for a non-finite d2_i;
             w_i = beta_i / sum beta; pass t is the kernel over K with w. If
             sum beta is 0 or non-finite the iteration stops and the last
             centre stands.
  CenteredClip(tau > 0 or None, L >= 0; at most 31 models)
             iteration t: c_i = min(1, tau / sqrt(d2_i)), 1 for d2_i = 0, 0 for
             a non-finite d2_i; tau None takes the lower median of the kept
             peers' sqrt(d2_i) of that iteration (non-finite ones counting as
             +Inf). With alpha' = alpha / sum_K alpha, pass t is the kernel over
             [v_(t-1), x_K ...] with weights [1 - sum c_i alpha'_i,
             c_i alpha'_i ...] into a new arena (the output never aliases an
             input); entries 1.. of its d2 feed the next iteration.

As in every plugin here, buffers and attributes are copy.deepcopy(models[0])'s
(also when models[0] is excluded) and the inputs are only read. An empty model
list raises IndexError; more than 32 models (31 for CenteredClip), or a model
whose parameter list differs from models[0]'s, ValueError; so do bad nu, T, tau
or L.

Cost: the weights need the distances on the host, so every pass pays one D2H
copy of n doubles and one stream synchronisation. The aggregates of one
simulated round (`RoundExecutor`, `aggregate_batch`) share them: the tasks go
in lockstep, every pass of every task in batched launches
(csrc/reducedist_batch_kernels.hpp) with one D2H copy and one
synchronisation per device and pass (`model_inputs.geomed_arena_tasks`).
`consensus_distance_batch` is pass 0 on its own.
"""
import math
from typing import List, Optional, Sequence, Tuple

import torch
from torch import nn

from dasklearn_amd import _native
from dasklearn_amd.gradient_aggregation import GradientAggregation
from dasklearn_amd.model_inputs import (ReduceDistPlan, fp32_rounded, reduce_dist_arena_tasks, reduce_with_distances,
                                        vectors_to_host)
from dasklearn_amd.wave_tasks import finish_modules

aggregate_with_distances = reduce_with_distances  # public here, as krum.model_distances


def _alphas(models, weights) -> List[float]:
    # fedavg.py:14-17, same order of checks => same exceptions
    if not weights:
        weights = [float(1. / len(models)) for _ in range(len(models))]
    else:
        assert len(weights) == len(models)
    models[0]  # IndexError for an empty list, as FedAvg
    return [float(w) for w in weights]


def consensus_distance(models: List[nn.Module], weights: Optional[Sequence[float]] = None):
    """(mean_module, d2): FedAvg's weighted mean (its weight defaults) and the
    float64 tensor of every model's squared distance to it; the consensus
    distance of the D-PSGD literature is sum_i alpha_i * d2[i]."""
    return reduce_with_distances(models, _alphas(models, weights))


def consensus_distance_batch(tasks: Sequence[Tuple[List[nn.Module], Optional[Sequence[float]]]]):
    """consensus_distance for every (models, weights) of `tasks` (every
    neighbourhood of a round) in one call: [(mean_module, d2)], each
    bit-identical to consensus_distance(models, weights), its exceptions too.
    The device-resident tasks share batched launches, one D2H copy and one
    stream synchronisation per device (model_inputs.reduce_dist_arena_tasks);
    a task with a host model, a model on another device or a non-contiguous
    parameter goes through consensus_distance."""
    from dasklearn_amd.gradient_aggregation.krum import _resident_entry
    results = [None] * len(tasks)
    prepared, where, ws = [], [], []
    for ti, (models, weights) in enumerate(tasks):
        alphas = _alphas(models, weights)
        _native.check_reducedist_fan_in(len(models))
        entry = _resident_entry(models, None)
        if entry is None:
            results[ti] = reduce_with_distances(models, alphas)
            continue
        prepared.append(entry)
        where.append(ti)
        ws.append(fp32_rounded(alphas))
    outs, slots, bufs = reduce_dist_arena_tasks(prepared, [range(len(w)) for w in ws], ws)
    d2s = vectors_to_host(slots, bufs)  # waits for the stream
    for ti, mod, d2 in zip(where, finish_modules(prepared, outs), d2s):
        results[ti] = (mod, torch.tensor(d2, dtype=torch.float64))
    return results


def weiszfeld_weights(d2: Sequence[float], alphas: Sequence[float], nu: float) -> Optional[List[float]]:
    """The smoothed Weiszfeld weights of one iteration, rounded to fp32:
    beta_i = alpha_i / max(nu, sqrt(d2_i)) (0 for a non-finite d2_i),
    w_i = beta_i / sum beta with the sum in index order. None when the sum is
    0 or non-finite: the iteration stops."""
    assert len(d2) == len(alphas)
    nu = float(nu)
    beta = []
    for d, a in zip(d2, alphas):
        d = float(d)
        beta.append(float(a) / max(nu, math.sqrt(d)) if math.isfinite(d) and d >= 0.0 else 0.0)
    total = 0.0
    for b in beta:
        total += b
    if total == 0.0 or not math.isfinite(total):
        return None
    return fp32_rounded([b / total for b in beta])


def clip_weights(d2: Sequence[float], alphas: Sequence[float], tau: Optional[float]) -> List[float]:
    """The n + 1 weights of one centered-clipping pass over [centre, peers...],
    rounded to fp32, from the peers' squared distances to the centre and their
    normalised weights alpha': c_i = min(1, tau / sqrt(d2_i)) (1 for d2_i = 0,
    0 for a non-finite d2_i); [1 - sum c_i alpha'_i, c_i alpha'_i ...], the sum
    in index order. tau None: the lower median of sqrt(d2_i), non-finite ones
    counting as +Inf."""
    assert len(d2) == len(alphas)
    dist = [math.sqrt(float(d)) if math.isfinite(d) and d >= 0.0 else math.inf for d in d2]
    if tau is None:
        tau = sorted(dist)[(len(dist) - 1) // 2]
    tau = float(tau)
    terms = []
    for r, a in zip(dist, alphas):
        c = 0.0 if r == math.inf else 1.0 if r == 0.0 else min(1.0, tau / r)
        terms.append(c * float(a))
    moved = 0.0
    for v in terms:
        moved += v
    return fp32_rounded([1.0 - moved] + terms)


def _normalised(alphas: Sequence[float], kept: Sequence[int]) -> List[float]:
    total = 0.0
    for i in kept:
        total += alphas[i]
    return [alphas[i] / total for i in kept]


def _pass0(plan: ReduceDistPlan, alphas: List[float]):
    """Exclusion and pass 0. Returns (kept indices, pass-0 weights, arenas,
    d2 list of the kept); kept is empty when no model is finite (the arenas
    are then FedAvg's over all models)."""
    everyone = list(range(plan.n))
    w = fp32_rounded(alphas)
    outs, d2 = plan.run(everyone, w)
    d2 = d2.cpu().tolist()
    if all(math.isfinite(d) for d in d2):
        return everyone, w, outs, d2
    kept = []
    for i in everyone:
        _, di = plan.run([i], [1.0], want_out=False)
        if math.isfinite(di.cpu().item()):
            kept.append(i)
    if len(kept) == plan.n or not kept:
        return kept, w, outs, d2
    w = fp32_rounded(_normalised(alphas, kept))
    outs, d2 = plan.run(kept, w)
    return kept, w, outs, d2.cpu().tolist()


class GeometricMedian(GradientAggregation):
    """The smoothed geometric median of the models (RFA): T Weiszfeld
    iterations from the weighted mean, smoothing nu. The defaults (T = 3,
    nu = 1e-6) are a choice, not measured."""

    iters = 3
    nu = 1e-6

    @classmethod
    def aggregate(cls, models: List[nn.Module], weights: Optional[List[float]] = None,
                  to_host: Optional[bool] = None, trace: bool = False):
        """to_host=None (default): the result lives where models[0] lives;
        False keeps it on the GPU. trace=True returns (module, passes): per
        pass a dict of the kept indices, the fp32 weights handed to the kernel
        and the d2 vector it returned."""
        alphas = _alphas(models, weights)
        plan = ReduceDistPlan(models)
        kept, w, outs, d2 = _pass0(plan, alphas)
        passes = [{"kept": list(kept) or list(range(plan.n)), "weights": w, "d2": d2}]
        if kept:
            a = [alphas[i] for i in kept]
            for _ in range(cls.iters):
                w = weiszfeld_weights(d2, a, cls.nu)
                if w is None:
                    break
                outs, d2 = plan.run(kept, w)
                d2 = d2.cpu().tolist()
                passes.append({"kept": list(kept), "weights": w, "d2": d2})
        out = plan.module(outs, to_host)
        return (out, passes) if trace else out

    @classmethod
    def with_params(cls, iters: int = 3, nu: float = 1e-6):
        """A GeometricMedian class with T = iters iterations and smoothing nu:
        the plugin signature ModelManager calls."""
        if int(iters) != iters or int(iters) < 0:
            raise ValueError(f"iters must be an integer >= 0 (got {iters})")
        nu = float(nu)
        if not (nu > 0.0 and math.isfinite(nu)):
            raise ValueError(f"nu must be a finite number > 0 (got {nu})")
        return type(f"GeometricMedian{int(iters)}", (cls,), {"iters": int(iters), "nu": nu})


class CenteredClip(GradientAggregation):
    """Centered clipping: L iterations v <- v + sum alpha'_i clip(x_i - v, tau)
    from the weighted mean; tau None clips at the lower median of the peers'
    distances. The defaults (tau None, L = 3) are a choice, not measured."""

    tau: Optional[float] = None
    iters = 3

    @classmethod
    def aggregate(cls, models: List[nn.Module], weights: Optional[List[float]] = None,
                  to_host: Optional[bool] = None, trace: bool = False):
        """As GeometricMedian.aggregate; a pass's weights and d2 have the
        centre's entry first."""
        alphas = _alphas(models, weights)
        if len(models) > _native.MAX_REDUCEDIST_INPUTS - 1:
            raise ValueError(f"CenteredClip takes at most {_native.MAX_REDUCEDIST_INPUTS - 1} models "
                             f"(got {len(models)}): the centre is one more input of the kernel")
        plan = ReduceDistPlan(models)
        kept, w, outs, d2 = _pass0(plan, alphas)
        passes = [{"kept": list(kept) or list(range(plan.n)), "weights": w, "d2": d2}]
        if kept:
            a = _normalised(alphas, kept)
            for _ in range(cls.iters):
                w = clip_weights(d2, a, cls.tau)
                outs, full = plan.run(kept, w, center=outs)
                full = full.cpu().tolist()
                d2 = full[1:]
                passes.append({"kept": list(kept), "weights": w, "d2": full})
        out = plan.module(outs, to_host)
        return (out, passes) if trace else out

    @classmethod
    def with_params(cls, tau: Optional[float] = None, iters: int = 3):
        """A CenteredClip class with clipping radius tau (None: the lower
        median of the distances at each iteration) and L = iters iterations."""
        if int(iters) != iters or int(iters) < 0:
            raise ValueError(f"iters must be an integer >= 0 (got {iters})")
        if tau is not None:
            tau = float(tau)
            if not (tau > 0.0 and math.isfinite(tau)):
                raise ValueError(f"tau must be None or a finite number > 0 (got {tau})")
        name = f"CenteredClip{int(iters)}" + ("" if tau is None else f"t{tau:g}")
        return type(name, (cls,), {"tau": tau, "iters": int(iters)})

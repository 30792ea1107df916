"""Batched aggregation: many independent `aggregate` tasks in few launches.

In a simulated round every peer aggregates its neighbours' models
(dasklearn/simulation/dpsgd/client.py:142-151); the broker schedules those
tasks one by one (broker.py:261-275), so each is one call of
functions.aggregate (functions.py:89-106). For small models (GNLeNet: 3 MB
per 8-way task) one launch per task is launch-bound; `aggregate_batch` runs
the tasks that are ready together through `dlsim_wreduce_batched` (up to 32
tasks / 192 inputs per launch). Results are bit-identical to calling
FedAvg.aggregate on each task.

`method_route` decides, for `aggregate_batch` here and for RoundExecutor, which
batched launches a method's tasks take; the tasks travel as
wave_tasks.ArenaTask records, run by wave_tasks.aggregate_arena_tasks (FedAvg)
and model_inputs' robust_arena_tasks, krum_arena_tasks and geomed_arena_tasks.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

from torch import nn

from . import _native
from .arena import ZipMismatch, aggregate_modules, input_arenas
from .model_inputs import geomed_arena_tasks, krum_arena_tasks, robust_arena_tasks
from .wave_tasks import ArenaTask, _device_views, aggregate_arena_tasks


def _resolve(models, weights) -> List[float]:
    # fedavg.py:14-17 rules, same exceptions; the Python floats (each dtype
    # group rounds them as the reference's op does: _native.weights_for_dtype)
    if not weights:
        weights = [float(1. / len(models)) for _ in range(len(models))]
    else:
        assert len(weights) == len(models)
    return [float(w) for w in weights]


def method_window(method, settings):
    """lo_hi_fn (fan-in -> window [lo, hi)) of a batched method: MEDIAN, or
    TRIMMED_MEAN with settings.aggregation_trim (default 1, as ModelManager);
    None for every other method, and for TRIMMED_MEAN under
    settings.aggregation_trim_rule = "median" (MeanAroundMedian has no window
    per launch and no batched form: it runs as a plugin, per task)."""
    from .gradient_aggregation import GradientAggregationMethod as M
    from .gradient_aggregation.robust import median_window, trimmed_window
    from .model_manager import trim_rule
    if method == M.MEDIAN:
        return median_window
    if method == M.TRIMMED_MEAN:
        if trim_rule(settings) == "median":
            return None
        trim = int(getattr(settings, "aggregation_trim", 1))
        if trim < 0:  # TrimmedMean.with_trim's check
            raise ValueError(f"trim must be >= 0 (got {trim})")
        return lambda n: trimmed_window(n, trim)
    return None


def check_window_task(method, window, models, weights) -> None:
    """What CoordinateMedian / TrimmedMean raise for one task before they
    touch the models: AssertionError or ValueError for weights, IndexError for
    no model, ValueError for more than 32 or a trim that leaves no value."""
    from .gradient_aggregation import GradientAggregationMethod as M
    from .gradient_aggregation.robust import _check_unweighted
    _check_unweighted("CoordinateMedian" if method == M.MEDIAN else "TrimmedMean", models, weights)
    models[0]
    _native.check_robust_fan_in(len(models))
    window(len(models))


def method_plugin(method, settings):
    """The plugin class ModelManager picks for `method` (None for an unknown
    value, as there), with `settings`' parameters."""
    from .model_manager import ModelManager

    class _Settings:  # `settings` (may be None) with the method set
        gradient_aggregation = method

        def __getattr__(self, name):
            return getattr(settings, name)
    return ModelManager(None, _Settings(), 0).get_aggregation_method()


def krum_rule(plugin):
    """(name, f, m) when `plugin` is a Krum or MultiKrum class (a subclass
    too: with_params makes one), else None. m: None for Krum, for Multi-Krum
    the class's m or, by default, the function fan-in -> n - f."""
    from .gradient_aggregation.krum import Krum, MultiKrum
    if not isinstance(plugin, type):
        return None
    if issubclass(plugin, Krum):
        return "Krum", plugin.f, None
    if issubclass(plugin, MultiKrum):
        f = plugin.f
        return "MultiKrum", f, (lambda n: n - f) if plugin.m is None else plugin.m
    return None


def check_krum_task(rule, models, weights) -> None:
    """What Krum / MultiKrum raise for one task before they touch the models,
    in their order: AssertionError or ValueError for weights, IndexError for
    no model, ValueError for more than 32 or for (n, f, m) outside the rule."""
    from .gradient_aggregation.krum import check_krum_params
    from .gradient_aggregation.robust import _check_unweighted
    name, f, m = rule
    _check_unweighted(name, models, weights)
    models[0]
    n = len(models)
    _native.check_pairdist_fan_in(n)
    check_krum_params(n, f, 1 if m is None else m(n) if callable(m) else m)


def geomed_rule(plugin):
    """("GeometricMedian", iters, nu) or ("CenteredClip", iters, tau) when `plugin` is one of those classes
    or a subclass that keeps its `aggregate` (with_params makes such subclasses), else None: a foreign
    plugin installed for these methods runs per task."""
    from .gradient_aggregation.geomed import CenteredClip, GeometricMedian
    if not isinstance(plugin, type):
        return None
    for base, name, param in ((GeometricMedian, "GeometricMedian", "nu"), (CenteredClip, "CenteredClip", "tau")):
        if issubclass(plugin, base):
            if getattr(plugin.aggregate, "__func__", None) is not base.aggregate.__func__:
                return None
            return name, int(plugin.iters), getattr(plugin, param)
    return None


def check_geomed_task(rule, models, weights) -> List[float]:
    """What GeometricMedian / CenteredClip raise for one task before they resolve the models, in their
    order: AssertionError for a weight list of another length, IndexError for no model, ValueError for
    more than 31 models under CenteredClip (ModelInputs raises the rest: more than 32 models, differing
    parameter lists). Returns the task's weights alpha as the plugins settle them (geomed._alphas)."""
    from .gradient_aggregation.geomed import _alphas
    alphas = _alphas(models, weights)
    if rule[0] == "CenteredClip" and len(models) > _native.MAX_REDUCEDIST_INPUTS - 1:
        raise ValueError(f"CenteredClip takes at most {_native.MAX_REDUCEDIST_INPUTS - 1} models "
                         f"(got {len(models)}): the centre is one more input of the kernel")
    _native.check_reducedist_fan_in(len(models))
    return alphas


FEDAVG, WINDOW, KRUM, GEOMED, PLUGIN = "fedavg", "window", "krum", "geomed", "plugin"


class MethodRoute:
    """How a method's aggregate tasks run (method_route). kind: FEDAVG (the weighted reduce), WINDOW
    (the order statistics; rule: the lo_hi_fn), KRUM (rule: krum_rule's tuple), GEOMED (the geometric
    median and centered clipping in lockstep; rule: geomed_rule's tuple) or PLUGIN (no batched form: the
    plugin per task). plugin: the method's plugin class (None for FedAvg), looked up when the route is
    made for KRUM, GEOMED and PLUGIN, which it decides between, and on first use for WINDOW."""
    __slots__ = ("kind", "method", "rule", "_plugin", "_lookup")

    def __init__(self, kind, method=None, rule=None, plugin=None, lookup=None):
        self.kind, self.method, self.rule, self._plugin, self._lookup = kind, method, rule, plugin, lookup

    @property
    def plugin(self):
        if self._lookup is not None:
            self._plugin, self._lookup = self._lookup(), None
        return self._plugin

    def check(self, models, weights) -> None:
        """Raise what the method's plugin raises for one task before it touches the models
        (check_window_task, check_krum_task, check_geomed_task). FedAvg's weights rule is _resolve, which
        the dispatchers call for the weights it returns; GEOMED returns the task's settled weights too
        (the other kinds None: their aggregates are unweighted)."""
        if self.kind == WINDOW:
            check_window_task(self.method, self.rule, models, weights)
        elif self.kind == KRUM:
            check_krum_task(self.rule, models, weights)
        elif self.kind == GEOMED:
            return check_geomed_task(self.rule, models, weights)
        return None

    def run(self, prepared, on_launched=None, mode: int = _native.DLSIM_EXACT, launchers=None) -> List[nn.Module]:
        """One module per ArenaTask of `prepared`, in the method's batched launches (`mode`: FedAvg's).
        launchers: (aggregate_arena_tasks, robust_arena_tasks, krum_arena_tasks[, geomed_arena_tasks]) as
        the dispatcher's own module names them (default: this module's; a three-tuple leaves the fourth
        at this module's), so that a probe or a test that replaces one of them in the dispatcher's module
        sees that dispatcher's launches."""
        launchers = tuple(launchers or ())
        fedavg, window, krum, geomed = launchers + (aggregate_arena_tasks, robust_arena_tasks, krum_arena_tasks,
                                                    geomed_arena_tasks)[len(launchers):]
        if self.kind == FEDAVG:
            return fedavg(prepared, mode, on_launched)
        if self.kind == WINDOW:
            return window(prepared, self.rule, on_launched)
        if self.kind == GEOMED:
            return geomed(prepared, self.rule, on_launched)
        return krum(prepared, self.rule[1], self.rule[2], on_launched)

    def per_task(self, tasks) -> List[nn.Module]:
        """PLUGIN: a foreign plugin (and an unknown value, which
        fails as the per-task path fails): the plugin per (models, weights), the result kept on the device."""
        return [self.plugin.aggregate(models, weights=weights, to_host=False) for models, weights in tasks]


def method_route(method, settings, lookup=method_plugin) -> MethodRoute:
    """The one decision both dispatchers (aggregate_batch, RoundExecutor) make: FedAvg (None too) takes
    the FedAvg launches; else a method_window the order-statistic launches; else a Krum or MultiKrum
    plugin class (krum_rule) the Krum launches; else a GeometricMedian or CenteredClip class (geomed_rule)
    the lockstep reduce-and-measure launches; else the plugin runs per task (MeanAroundMedian and Bulyan,
    the variants of TRIMMED_MEAN and MULTI_KRUM, among them: no batched form yet). lookup(method,
    settings): the plugin class, as the caller's per-task path finds it."""
    from .gradient_aggregation import GradientAggregationMethod
    if method is None or method == GradientAggregationMethod.FEDAVG:
        return MethodRoute(FEDAVG)
    window = method_window(method, settings)
    if window is not None:
        return MethodRoute(WINDOW, method, window, lookup=lambda: lookup(method, settings))
    plugin = lookup(method, settings)
    rule = krum_rule(plugin)
    if rule is not None:
        return MethodRoute(KRUM, method, rule, plugin)
    rule = geomed_rule(plugin)
    return MethodRoute(PLUGIN if rule is None else GEOMED, method, rule, plugin)


def aggregate_batch(tasks: Sequence[Tuple[List[nn.Module], Optional[Sequence[float]]]],
                    mode: int = _native.DLSIM_EXACT, method=None, settings=None) -> List[nn.Module]:
    """tasks: [(models, weights)] -> one aggregated module per task.

    Tasks whose models are device-resident arenas (what this package returns
    for device inputs) are reduced together in batched launches; any other
    task goes through the single-task path. Output placement follows
    FedAvg.aggregate (where models[0] lives).

    method: a GradientAggregationMethod (None: FEDAVG), with its parameters
    read from `settings` as ModelManager reads them (method_route). MEDIAN and
    TRIMMED_MEAN batch their device-arena tasks through
    dlsim_robust_reduce_batched, KRUM and MULTI_KRUM theirs through
    dlsim_pairwise_sqdist_batched with one synchronisation for all of them
    (model_inputs.krum_arena_tasks), GEOMETRIC_MEDIAN and CENTERED_CLIP theirs
    in lockstep through dlsim_wreduce_dist_batched with one synchronisation
    per pass (model_inputs.geomed_arena_tasks), and raise, per task, what
    their plugins raise; any other plugin is called per task and keeps the
    result on the device. `mode` applies to FedAvg alone."""
    route = method_route(method, settings)
    if route.kind == PLUGIN:
        return route.per_task(tasks)
    results: List[Optional[nn.Module]] = [None] * len(tasks)
    prepared, where = [], []
    for ti, (models, weights) in enumerate(tasks):
        alphas = route.check(models, weights)
        ws = _resolve(models, weights) if route.kind == FEDAVG else alphas
        model0 = models[0]  # FedAvg: IndexError for an empty task, as the reference (the others: in check)
        try:
            layout, _, views = input_arenas(models)
        except ZipMismatch:  # parameter lists differ: FedAvg's per-parameter zip path; else the ValueError it is
            if route.kind != FEDAVG:
                raise
            layout, views = None, None
        if _device_views(views) is None:  # host models, separate tensors, several devices: staged per task
            if route.kind == FEDAVG:
                results[ti] = aggregate_modules(models, weights, mode)
            elif route.kind == WINDOW:
                results[ti] = route.plugin.aggregate(models, weights=None)
            elif route.kind == GEOMED:  # kept on the device, as when these methods ran task by task
                results[ti] = route.plugin.aggregate(models, weights=weights, to_host=False)
            else:  # Krum and Multi-Krum keep such a result on the device, as they did task by task
                results[ti] = route.plugin.aggregate(models, weights=None, to_host=False)
            continue
        prepared.append(ArenaTask(model0, layout, views, ws))
        where.append(ti)
    for ti, out in zip(where, route.run(prepared, None, mode)):
        results[ti] = out
    return results

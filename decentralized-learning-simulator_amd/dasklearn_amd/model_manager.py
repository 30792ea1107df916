"""ModelManager — mirrors dasklearn/model_manager.py:14-43 for the aggregate task.

Collects incoming models keyed by peer id (first one wins, :27-32) and
aggregates them with the method chosen by `settings.gradient_aggregation`
(:37-43): FEDAVG = 1 as in the reference, and the two robust aggregators it
does not have, MEDIAN = 2 and TRIMMED_MEAN = 3 (the latter trims
`settings.aggregation_trim` values, default 1, at each end), and the two
distance-based ones, KRUM = 4 and MULTI_KRUM = 5 (Byzantine count
`settings.aggregation_byzantine`, default 1; Multi-Krum averages
`settings.aggregation_multi_krum_m` models, default None = n - f), and the
two that keep every honest peer, GEOMETRIC_MEDIAN = 6
(`settings.aggregation_gm_iters` Weiszfeld iterations, default 3, smoothing
`settings.aggregation_gm_nu`, default 1e-6) and CENTERED_CLIP = 7
(`settings.aggregation_clip_tau`, default None = the lower median of the
distances, `settings.aggregation_clip_iters`, default 3). These four defaults
are a choice, not measured. The enum keeps the values 1 to 7; two further
rules are variants of existing members: TRIMMED_MEAN with
`settings.aggregation_trim_rule = "median"` (default "rank") is the mean around
the median, MeanAroundMedian, which keeps the n - 2*`aggregation_trim` values
closest to the median; MULTI_KRUM with `settings.aggregation_krum_rule =
"bulyan"` (default "multi_krum") is Bulyan with Byzantine count
`aggregation_byzantine` (`aggregation_multi_krum_m` must then be None). Any
other string raises ValueError. The
`dataset` argument is accepted and ignored, as the reference's aggregate task
passes None (functions.py:99).
"""
import logging
from typing import Dict, List, Optional

import torch.nn as nn

from dasklearn_amd.gradient_aggregation import GradientAggregationMethod
from dasklearn_amd.gradient_aggregation.fedavg import FedAvg
from dasklearn_amd.gradient_aggregation.geomed import CenteredClip, GeometricMedian
from dasklearn_amd.gradient_aggregation.krum import Bulyan, Krum, MultiKrum
from dasklearn_amd.gradient_aggregation.robust import CoordinateMedian, MeanAroundMedian, TrimmedMean


def _rule(settings, name: str, allowed) -> str:
    """settings.<name> (default allowed[0]); ValueError for any other value than `allowed`."""
    rule = getattr(settings, name, allowed[0])
    if rule not in allowed:
        raise ValueError(f"{name} must be one of {', '.join(repr(a) for a in allowed)} (got {rule!r})")
    return rule


def trim_rule(settings) -> str:
    """"rank" (TrimmedMean, the default) or "median" (MeanAroundMedian) for TRIMMED_MEAN."""
    return _rule(settings, "aggregation_trim_rule", ("rank", "median"))


def krum_rule_name(settings) -> str:
    """"multi_krum" (MultiKrum, the default) or "bulyan" (Bulyan) for MULTI_KRUM."""
    return _rule(settings, "aggregation_krum_rule", ("multi_krum", "bulyan"))


class ModelManager:

    def __init__(self, dataset, settings, participant_index: int):
        self.settings = settings
        self.participant_index: int = participant_index
        self.logger = logging.getLogger(self.__class__.__name__)
        self.incoming_trained_models: Dict[int, nn.Module] = {}

    def process_incoming_trained_model(self, peer_id: int, incoming_model: nn.Module):
        if peer_id in self.incoming_trained_models:
            return
        self.incoming_trained_models[peer_id] = incoming_model

    def reset_incoming_trained_models(self):
        self.incoming_trained_models = {}

    def get_aggregation_method(self):
        method = getattr(self.settings, "gradient_aggregation", GradientAggregationMethod.FEDAVG)
        if method == GradientAggregationMethod.FEDAVG:
            return FedAvg
        if method == GradientAggregationMethod.MEDIAN:
            return CoordinateMedian
        if method == GradientAggregationMethod.TRIMMED_MEAN:
            trim = getattr(self.settings, "aggregation_trim", 1)
            if trim_rule(self.settings) == "median":
                return MeanAroundMedian.with_trim(trim)
            return TrimmedMean.with_trim(trim)
        if method == GradientAggregationMethod.KRUM:
            return Krum.with_params(getattr(self.settings, "aggregation_byzantine", 1))
        if method == GradientAggregationMethod.MULTI_KRUM:
            f = getattr(self.settings, "aggregation_byzantine", 1)
            m = getattr(self.settings, "aggregation_multi_krum_m", None)
            if krum_rule_name(self.settings) == "bulyan":
                if m is not None:
                    raise ValueError(f"aggregation_krum_rule = 'bulyan' selects n - 2f models itself: "
                                     f"aggregation_multi_krum_m must be None (got {m})")
                return Bulyan.with_params(f)
            return MultiKrum.with_params(f, m)
        if method == GradientAggregationMethod.GEOMETRIC_MEDIAN:
            return GeometricMedian.with_params(getattr(self.settings, "aggregation_gm_iters", 3),
                                               getattr(self.settings, "aggregation_gm_nu", 1e-6))
        if method == GradientAggregationMethod.CENTERED_CLIP:
            return CenteredClip.with_params(getattr(self.settings, "aggregation_clip_tau", None),
                                            getattr(self.settings, "aggregation_clip_iters", 3))
        return None  # the reference returns None for unknown methods too

    def aggregate_trained_models(self, weights: List[float] = None) -> Optional[nn.Module]:
        models = list(self.incoming_trained_models.values())
        method = self.get_aggregation_method()
        # Opt-in (not a reference setting): keep the aggregate on the GPU so a
        # device-resident consumer skips the D2H/H2D round trip.
        if getattr(self.settings, "aggregate_on_device", False):
            return method.aggregate(models, weights=weights, to_host=False)
        return method.aggregate(models, weights=weights)

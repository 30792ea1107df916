"""Aggregation plugin API — mirrors dasklearn/gradient_aggregation/__init__.py:8-17.

`GradientAggregationMethod` keeps the reference's enum value (FEDAVG = 1,
selected through `SessionSettings.gradient_aggregation`,
dasklearn/session_settings.py:40 and model_manager.py:37-39), so settings
objects built for the reference select the HIP implementation unchanged.
MEDIAN and TRIMMED_MEAN (gradient_aggregation/robust.py), KRUM and MULTI_KRUM
(gradient_aggregation/krum.py) and GEOMETRIC_MEDIAN and CENTERED_CLIP
(gradient_aggregation/geomed.py) are new here: the reference has no such
members.
"""
from abc import abstractmethod
from enum import IntEnum
from typing import List, Optional

from torch import nn


class GradientAggregationMethod(IntEnum):
    FEDAVG = 1
    MEDIAN = 2
    TRIMMED_MEAN = 3
    KRUM = 4
    MULTI_KRUM = 5
    GEOMETRIC_MEDIAN = 6
    CENTERED_CLIP = 7


class GradientAggregation:

    @staticmethod
    @abstractmethod
    def aggregate(models: List[nn.Module], weights: Optional[List[float]]) -> nn.Module:
        """Return a new module whose parameters are the weighted sum of the
        models' parameters (buffers and attributes copied from models[0])."""

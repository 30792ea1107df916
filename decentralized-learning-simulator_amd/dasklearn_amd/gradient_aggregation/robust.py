"""Coordinate-wise median and trimmed mean on the MI355X: the second and third
plugins behind `GradientAggregationMethod` (MEDIAN = 2, TRIMMED_MEAN = 3).

The reference has one aggregator, FedAvg (dasklearn/gradient_aggregation/
fedavg.py); a weighted mean does not survive a peer that sends Inf, NaN or a
scaled model. Both aggregators here take, for every parameter element, the n
values of the n models, sort them ascending in the total order

    -Inf < ... < -0.0 < +0.0 < ... < +Inf < NaN     (all NaNs equal, largest)

and average a window [lo, hi) of the sorted values: acc = s[lo], then
acc += s[j] for j = lo+1 .. hi-1 in order, then acc / (hi - lo). fp32 and fp64
in their own precision; bf16 and fp16 values are widened to fp32, summed and
divided in fp32 and rounded once. A NaN result is the dtype's
canonical quiet NaN. Parameters only: buffers and attributes are
copy.deepcopy(models[0])'s, as in FedAvg. Inputs are only read.

Both are unweighted: `weights` of None or [] is accepted; a non-empty list of
another length than the models raises AssertionError (as FedAvg), one of the
right length ValueError. An empty model list raises IndexError; more than 32
models, or a model whose parameter list differs from models[0]'s, ValueError.

The arithmetic runs in one HIP kernel per dtype group
(csrc/robust_kernels.hpp: an in-register sorting network per element) through
dasklearn_amd.model_inputs.robust_modules.

MeanAroundMedian (MeaMed / Phocas, Xie et al., 2018; a variant of TRIMMED_MEAN:
`settings.aggregation_trim_rule = "median"`) averages, per element, the `keep`
sorted values closest to the lower median instead of a fixed rank window; its
kernels (csrc/robust_nearest_kernels.hpp) choose the window per
element, through dasklearn_amd.model_inputs.nearest_modules.
"""
from typing import List, Optional

from torch import nn

from dasklearn_amd.gradient_aggregation import GradientAggregation
from dasklearn_amd.model_inputs import nearest_modules, robust_modules


def _check_unweighted(name: str, models, weights) -> None:
    if weights:
        assert len(weights) == len(models)
        raise ValueError(f"{name} is unweighted: pass weights=None (got {len(weights)} weights)")


def median_window(n: int):
    """[lo, hi) of the lower median of n sorted values."""
    lo = (n - 1) // 2
    return lo, lo + 1


def trimmed_window(n: int, trim: int):
    """[lo, hi) of the mean of n sorted values without the `trim` smallest and
    the `trim` largest."""
    trim = int(trim)
    if trim < 0 or n - 2 * trim < 1:
        raise ValueError(f"trimmed mean of n = {n} models with trim = {trim}: needs trim >= 0 and n - 2*trim >= 1")
    return trim, n - trim


class CoordinateMedian(GradientAggregation):
    """The coordinate-wise lower median: element (n-1)//2 of the sorted values,
    bit-identical to one of the inputs (no arithmetic touches it), equal to
    `torch.sort(torch.stack(xs), 0).values[(n - 1) // 2]`.

    This is NOT `torch.median(torch.stack(xs), 0)`: torch.median returns NaN
    as soon as any input is NaN. Here NaNs sort above +Inf, so a NaN sent by a
    minority of peers is never selected; the result is NaN only where at
    least n - (n-1)//2 of the n values are NaN."""

    @staticmethod
    def aggregate(models: List[nn.Module], weights: Optional[List[float]] = None,
                  to_host: Optional[bool] = None) -> nn.Module:
        """to_host=None (default): the result lives where models[0] lives;
        False keeps it on the GPU."""
        _check_unweighted("CoordinateMedian", models, weights)
        return robust_modules(models, median_window, to_host=to_host)


class TrimmedMean(GradientAggregation):
    """The coordinate-wise trimmed mean: per element, the `trim` smallest and
    the `trim` largest of the n values are dropped and the rest averaged in
    ascending order. trim = 0 is the mean summed in sorted order; for even n,
    trim = n/2 - 1 is the mean of the two middle values. Up to `trim` peers
    sending Inf or NaN leave the result finite."""

    trim = 1

    @classmethod
    def aggregate(cls, models: List[nn.Module], weights: Optional[List[float]] = None,
                  to_host: Optional[bool] = None, trim: Optional[int] = None) -> nn.Module:
        _check_unweighted("TrimmedMean", models, weights)
        b = cls.trim if trim is None else trim
        return robust_modules(models, lambda n: trimmed_window(n, b), to_host=to_host)

    @classmethod
    def with_trim(cls, trim: int):
        """A TrimmedMean class whose aggregate(models, weights=None,
        to_host=None) trims `trim` values at each end: the plugin signature
        ModelManager calls."""
        trim = int(trim)
        if trim < 0:
            raise ValueError(f"trim must be >= 0 (got {trim})")
        return type(f"TrimmedMean{trim}", (cls,), {"trim": trim})


class MeanAroundMedian(GradientAggregation):
    """The coordinate-wise mean around the median: per element, of the n sorted
    values s the keep = n - 2*trim closest to the lower median p = s[(n-1)//2]
    are averaged in ascending order. TrimmedMean drops `trim` values at each
    end whatever they are; this drops the 2*trim values farthest from the
    centre, on whichever side they lie.

    The distance of s[j] is +0.0 where s[j] sorts equal to p (the same bits;
    any two NaNs), else |s[j] - p| rounded once in fp32 (fp64 for fp64 models),
    ranked 0 <= ... <= +Inf < NaN. The window starts at the median and grows
    keep - 1 times, by the right neighbour iff there is one and the left
    neighbour is missing or strictly farther: ties go left. keep = 1 is
    CoordinateMedian, keep = n the trim-0 TrimmedMean, bit for bit. Up to
    `trim` peers sending Inf or NaN leave the result finite."""

    trim = 1

    @classmethod
    def aggregate(cls, models: List[nn.Module], weights: Optional[List[float]] = None,
                  to_host: Optional[bool] = None, keep: Optional[int] = None) -> nn.Module:
        """keep: the kept count itself (1 <= keep <= n) instead of
        n - 2*trim."""
        _check_unweighted("MeanAroundMedian", models, weights)
        if keep is not None:
            return nearest_modules(models, lambda n: keep, to_host=to_host)
        b = cls.trim

        def kept(n):
            lo, hi = trimmed_window(n, b)
            return hi - lo
        return nearest_modules(models, kept, to_host=to_host)

    @classmethod
    def with_trim(cls, trim: int):
        """A MeanAroundMedian class that keeps n - 2*trim values: the plugin
        signature ModelManager calls."""
        trim = int(trim)
        if trim < 0:
            raise ValueError(f"trim must be >= 0 (got {trim})")
        return type(f"MeanAroundMedian{trim}", (cls,), {"trim": trim})

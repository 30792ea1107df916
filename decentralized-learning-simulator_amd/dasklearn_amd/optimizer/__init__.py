"""Optimizers of the reference's worker (dasklearn/optimizer/) on the MI355X."""
from .sgd import ArenaSGD, SGDOptimizer

__all__ = ["ArenaSGD", "SGDOptimizer"]

"""The abstract hyper-parameter optimizer (the contract of Pyesian/optimizers/hyperparameters/HyperparameterOptimizer.py):
compile(f, *space, **options) stores the objective and hands the space to the subclass, optimize() runs the search."""

import math
from abc import ABC, abstractmethod


class HyperparameterOptimizer(ABC):
    def __init__(self):
        self._f = None

    def compile(self, f, *args, **kwargs):
        """f: the cost function of the hyper-parameters (train and evaluate a model there); args: the search space
        (space.Number axes, space.Constant entries); kwargs: the subclass's options."""
        self._f = f
        self._compile_extra_components(*args, **kwargs)

    @abstractmethod
    def _compile_extra_components(self, *args, **kwargs):
        pass

    @abstractmethod
    def optimize(self):
        pass

    def _print_progress(self, progress: float, bar_length=10, suffix="Training", **kwargs):
        """The status line of Optimizer._print_progress: "<suffix> <pct> % [====>     ] key: value ..."."""
        filled = math.ceil(progress * bar_length)
        bar = "[" + "=" * filled + (">" if filled < bar_length else "") + "]"
        fields = " ".join(f"{k}: {v}" for k, v in kwargs.items())
        print(f"\r{suffix} {math.ceil(progress * 100)} % {bar} {fields}", end="")

from .Metrics import Metrics
from .Plotter import Plotter
from .Robustness import Robustness

__all__ = ["Metrics", "Plotter", "Robustness"]

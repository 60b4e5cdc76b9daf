from .Metrics import Metrics
from .Robustness import Robustness

__all__ = ["Metrics", "Robustness"]

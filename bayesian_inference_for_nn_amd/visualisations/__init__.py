from .Robustness import Robustness

__all__ = ["Robustness"]

"""`Metrics`, `Plotter` and `Robustness` are the library's own classes."""

from bayesian_inference_for_nn_amd.visualisations import Metrics, Plotter, Robustness  # noqa: F401

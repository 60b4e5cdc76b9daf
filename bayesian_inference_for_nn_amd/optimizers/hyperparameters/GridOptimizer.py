"""Grid search over hyper-parameters (the contract of Pyesian/optimizers/hyperparameters/GridOptimizer.py), and the
objective that evaluates a whole grid of SGLD learning-rate schedules side by side on one GPU.

    grid = GridOptimizer()
    grid.compile(f, Real(0, 1, "lr"), Integer(0, 100, "k"), n=10)                       # n points along every axis
    grid.compile(f, Real(0, 1, "lr"), Integer(0, 100, "k"), n=10, specify={"lr": [1e-3, 1e-2, 1e-1]})
    grid.optimize(); grid.save("grid.txt"); point, value = grid.best()

Axes: a Real gives n evenly spaced points with both bounds; an Integer every integer of its range when n covers it, else
the sorted distinct values of int(round(i * eps + lower)) (Python's round: halves go to the even neighbour);
specify[name] = [values] gives an axis as listed.  Only space.Number arguments make axes.  optimize() walks
itertools.product of the axes and keeps f's value per point in that order.

The reference calls f once per point (its process pool is commented out).  Here an f with an
evaluate_lanes(names, points) method gets the whole list in ONE call and returns the values in the same order:
SGLDGridObjective trains up to max_lanes points at a time as the lanes of one particle-batched SGLD run (SGLD.compile's
lanes) and scores them on the device (SGLD.lane_scores)."""

import math
from itertools import product

from .HyperParameters import HyperParameters
from .HyperparameterOptimizer import HyperparameterOptimizer
from .space import Integer, Number, Real


class GridOptimizer(HyperparameterOptimizer):
    def __init__(self):
        super().__init__()
        self._axes = []
        self._names = []
        self._results = {}
        self._verbose = True

    def _compile_extra_components(self, *args, **kwargs):
        self._n = kwargs["n"]
        self._verbose = bool(kwargs.get("verbose", True))
        specify = kwargs.get("specify", {})
        self._axes, self._names = [], []               # a second compile replaces the first space
        for arg in args:
            if not isinstance(arg, Number):
                continue
            n = specify.get(arg.name, self._n)
            self._names.append(arg.name)
            if isinstance(n, list):
                self._axes.append(n)
                continue
            if n < 2:
                raise ValueError("n can't be less than 2 for a grid search, do a constant parameter instead")
            lower, upper = arg.lower_bound, arg.upper_bound
            eps = (upper - lower) / (n - 1)
            if isinstance(arg, Real):
                self._axes.append([i * eps + lower for i in range(n)])
            elif isinstance(arg, Integer):
                size = upper - lower + 1
                if n >= size:
                    self._axes.append([lower + i for i in range(size)])
                else:
                    self._axes.append(sorted({int(round(i * eps + lower)) for i in range(n)}))

    def _progress(self, done, total):
        if self._verbose:
            self._print_progress(done / total, bar_length=20, suffix="Grid Optimizer", completed=f"{done}/{total}")

    def optimize(self):
        """Evaluates every point of the grid, in itertools.product order."""
        self._results = {}
        points = list(product(*self._axes))
        if hasattr(self._f, "evaluate_lanes"):
            values = list(self._f.evaluate_lanes(list(self._names), points))
            if len(values) != len(points):
                raise ValueError(f"evaluate_lanes returned {len(values)} values for {len(points)} points")
            for point, value in zip(points, values):
                self._results[point] = value
            self._progress(len(points), max(1, len(points)))
            return
        for point in points:
            self._results[point] = self._f(*point)
            self._progress(len(self._results), len(points))

    @property
    def results(self):
        """{point: value} in evaluation order."""
        return dict(self._results)

    def best(self, minimize=True):
        """(point, value) of the smallest (largest) value; the first one in grid order among equals."""
        if not self._results:
            raise ValueError("optimize() has not run")
        pick = min if minimize else max
        point = pick(self._results, key=self._results.get)
        return point, self._results[point]

    def save(self, path: str):
        """Text: the axis names joined by commas, then per point a line of its values and a line of its result."""
        with open(path, "w") as out:
            out.write(",".join(self._names) + "\n")
            for point, value in self._results.items():
                out.write(",".join(str(v) for v in point) + "\n")
                out.write(str(value) + "\n")


class SGLDGridObjective:
    """f(point) = the validation score of SGLD trained for nb_iterations steps with the point's hyper-parameters, for a
    GridOptimizer: axes named lr_upper, lr_lower, lr_gamma, batch_size; everything else from `hp`.

    evaluate_lanes groups the points by batch size (a particle-batched step has one) and trains every group in chunks of
    at most max_lanes lanes, each chunk ONE SGLD run with lane_seeds="shared": the same start, the same batches and the
    same noise for every point, so the scores differ by the hyper-parameters alone.  metric: "val_loss" (the mean per-row
    loss on the validation split) or "val_error" (the misclassified fraction); weights: "theta" or "mean"
    (SGLD.lane_scores).  A score that is not finite becomes math.inf.  seed=None: a fresh seed per training."""

    NAMES = ("lr_upper", "lr_lower", "lr_gamma", "batch_size")

    def __init__(self, hp, model_config, dataset, nb_iterations, metric="val_loss", weights="theta", seed=None, max_lanes=32):
        if metric not in ("val_loss", "val_error"):
            raise ValueError("metric must be 'val_loss' or 'val_error'")
        if weights not in ("theta", "mean"):
            raise ValueError("weights must be 'theta' or 'mean'")
        if int(max_lanes) < 1:
            raise ValueError("max_lanes must be at least 1")
        self._hp, self._model_config, self._dataset = hp, model_config, dataset
        self._nb_iterations, self._metric, self._weights = int(nb_iterations), metric, weights
        self._seed, self._max_lanes = seed, int(max_lanes)
        self.trainings = []                            # lanes of every SGLD run so far

    def _train_chunk(self, batch_size, lanes):
        from ..SGLD import SGLD
        hp = HyperParameters(**{**self._hp._params, "batch_size": batch_size})
        opt = SGLD()
        opt.compile(hp, self._model_config, self._dataset, verbose=False, seed=self._seed, lanes=lanes)
        opt.train(self._nb_iterations)
        scores = opt.lane_scores(split="valid", weights=self._weights)
        opt._plan.close()
        self.trainings.append(len(lanes))
        values = scores["loss" if self._metric == "val_loss" else "error"]
        return [float(v) if math.isfinite(v) else math.inf for v in values]

    def evaluate_lanes(self, names, points):
        names = list(names)
        unknown = [n for n in names if n not in self.NAMES]
        if unknown:
            raise ValueError(f"SGLDGridObjective cannot vary {unknown}: its axes are {list(self.NAMES)}")
        groups = {}                                    # batch size -> [(position, lane)], in order of appearance
        for pos, point in enumerate(points):
            given = dict(zip(names, point))
            batch_size = int(given.pop("batch_size", self._hp.batch_size))
            groups.setdefault(batch_size, []).append((pos, given))
        out = [None] * len(points)
        for batch_size, members in groups.items():
            for c0 in range(0, len(members), self._max_lanes):
                chunk = members[c0:c0 + self._max_lanes]
                for (pos, _), value in zip(chunk, self._train_chunk(batch_size, [lane for _, lane in chunk])):
                    out[pos] = value
        return out

    def __call__(self, *point, names=None):
        """One point as a one-lane chunk (the serial loop of the reference's optimize()).  The values are taken in the
        order of `names`, by default NAMES cut to the point's length."""
        names = list(names) if names is not None else list(self.NAMES[:len(point)])
        if len(names) != len(point):
            raise ValueError("one name per value")
        return self.evaluate_lanes(names, [tuple(point)])[0]

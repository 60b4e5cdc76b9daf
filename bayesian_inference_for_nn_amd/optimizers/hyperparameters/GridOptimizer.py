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
lanes) and scores them on the device (SGLD.lane_scores); BBBGridObjective does the same for the lr x alpha x pi grids of
the Bayes-by-Backprop drivers (BBB.compile's lanes, BBB.lane_scores).  Grouping by batch size, chunking and the rule for
scores that are not finite are LanesGridObjective's, the base of both."""

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


class LanesGridObjective:
    """What the lanes objectives share.  evaluate_lanes groups the points by batch size (a particle-batched step has one)
    and trains every group in chunks of at most max_lanes lanes, one run each (_train_chunk(batch_size, lanes) -> the
    chunk's scores, in lane order); `trainings` records the lanes of every run so far; a score that is not finite becomes
    math.inf.  A class gives NAMES (its axes; "batch_size" among them), WEIGHTS (the values of `weights`) and
    _train_chunk."""

    NAMES = ()
    WEIGHTS = ()

    def __init__(self, hp, model_config, dataset, nb_iterations, metric, weights, seed, max_lanes):
        if metric not in ("val_loss", "val_error"):
            raise ValueError("metric must be 'val_loss' or 'val_error'")
        if weights not in self.WEIGHTS:
            raise ValueError("weights must be " + " or ".join(repr(w) for w in self.WEIGHTS))
        if int(max_lanes) < 1:
            raise ValueError("max_lanes must be at least 1")
        self._hp, self._model_config, self._dataset = hp, model_config, dataset
        self._nb_iterations, self._metric, self._weights = int(nb_iterations), metric, weights
        self._seed, self._max_lanes = seed, int(max_lanes)
        self.trainings = []                            # lanes of every run so far

    def _train_chunk(self, batch_size, lanes):
        raise NotImplementedError

    def _values(self, n_lanes, scores):
        """Records a run of n_lanes lanes; its scores under the metric, not-finite ones as math.inf."""
        self.trainings.append(n_lanes)
        values = scores["loss" if self._metric == "val_loss" else "error"]
        if values is None:
            raise ValueError(f"metric {self._metric!r} is not defined for weights={self._weights!r}")
        return [float(v) if math.isfinite(v) else math.inf for v in values]

    def evaluate_lanes(self, names, points):
        names = list(names)
        unknown = [n for n in names if n not in self.NAMES]
        if unknown:
            raise ValueError(f"{type(self).__name__} cannot vary {unknown}: its axes are {list(self.NAMES)}")
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


class SGLDGridObjective(LanesGridObjective):
    """f(point) = the validation score of SGLD trained for nb_iterations steps with the point's hyper-parameters, for a
    GridOptimizer: axes named lr_upper, lr_lower, lr_gamma, batch_size; everything else from `hp`.

    Every chunk is ONE SGLD run with lane_seeds="shared": the same start, the same batches and the same noise for every
    point, so the scores differ by the hyper-parameters alone.  metric: "val_loss" (the mean per-row loss on the
    validation split) or "val_error" (the misclassified fraction); weights: "theta" or "mean" (SGLD.lane_scores).
    seed=None: a fresh seed per training."""

    NAMES = ("lr_upper", "lr_lower", "lr_gamma", "batch_size")
    WEIGHTS = ("theta", "mean")

    def __init__(self, hp, model_config, dataset, nb_iterations, metric="val_loss", weights="theta", seed=None, max_lanes=32):
        super().__init__(hp, model_config, dataset, nb_iterations, metric, weights, seed, max_lanes)

    def _train_chunk(self, batch_size, lanes):
        from ..SGLD import SGLD
        hp = HyperParameters(**{**self._hp._params, "batch_size": batch_size})
        opt = SGLD()
        opt.compile(hp, self._model_config, self._dataset, verbose=False, seed=self._seed, lanes=lanes)
        opt.train(self._nb_iterations)
        scores = opt.lane_scores(split="valid", weights=self._weights)
        opt._plan.close()
        return self._values(len(lanes), scores)


class BBBGridObjective(LanesGridObjective):
    """f(point) = the validation score of Bayes-by-Backprop trained for nb_iterations steps with the point's
    hyper-parameters, for a GridOptimizer: axes named lr, alpha, pi, batch_size (the grids of the reference's BBB drivers);
    everything else from `hp`, the priors as BBB.compile takes them.

    Every chunk is ONE BBB run with lane_seeds="shared": the same batches and the same eps stream for every point.
    metric: "val_error" (the misclassified fraction) or "val_loss" (the mean per-row loss; weights="mu" only); weights:
    "mu" (the posterior means, scored where they live) or "predictive" (predict(x, nb_samples) of each posterior, what the
    reference's drivers score).  seed=None: a fresh seed per training."""

    NAMES = ("lr", "alpha", "pi", "batch_size")
    WEIGHTS = ("mu", "predictive")

    def __init__(self, hp, model_config, dataset, nb_iterations, prior, prior2=None, metric="val_error", weights="mu",
                 nb_samples=100, seed=None, max_lanes=32):
        super().__init__(hp, model_config, dataset, nb_iterations, metric, weights, seed, max_lanes)
        if weights == "predictive" and metric == "val_loss":
            raise ValueError("metric 'val_loss' is not defined for weights='predictive'")
        if int(nb_samples) < 1:
            raise ValueError("nb_samples must be at least 1")
        self._prior, self._prior2, self._nb_samples = prior, prior2, int(nb_samples)

    def _train_chunk(self, batch_size, lanes):
        from ..BBB import BBB
        hp = HyperParameters(**{**self._hp._params, "batch_size": batch_size})
        priors = {"prior": self._prior, **({"prior2": self._prior2} if self._prior2 is not None else {})}
        opt = BBB()
        opt.compile(hp, self._model_config, self._dataset, verbose=False, seed=self._seed, lanes=lanes, **priors)
        opt.train(self._nb_iterations)
        scores = opt.lane_scores(split="valid", weights=self._weights, nb_samples=self._nb_samples)
        opt._plan.close()
        return self._values(len(lanes), scores)

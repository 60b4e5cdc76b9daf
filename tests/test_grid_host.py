"""GridOptimizer and the search space on the host: the axes, the evaluation order, the text format, best(), and the two
ways an objective is called (once per point, or once with every point through evaluate_lanes)."""

import itertools

import pytest

from bayesian_inference_for_nn_amd.optimizers.hyperparameters import (Constant, GridOptimizer, HyperParameters,
                                                                      HyperparameterOptimizer, Integer, Number, Parameter, Real,
                                                                      SGLDGridObjective)


def axes_of(*args, **kw):
    g = GridOptimizer()
    g.compile(lambda *p: 0.0, *args, verbose=False, **kw)
    return g._names, g._axes


def test_space_classes():
    r, i, c = Real(0.5, 2.0, "lr"), Integer(1, 9, "k"), Constant(3, "depth")
    assert (r.name, r.lower_bound, r.upper_bound) == ("lr", 0.5, 2.0) and (i.name, i.lower_bound, i.upper_bound) == ("k", 1, 9)
    assert (c.name, c.value) == ("depth", 3)
    assert isinstance(r, Number) and isinstance(i, Number) and isinstance(r, Parameter) and not isinstance(c, Number)
    assert issubclass(GridOptimizer, HyperparameterOptimizer)
    with pytest.raises(TypeError):
        HyperparameterOptimizer()                                        # abstract


@pytest.mark.parametrize("arg,n,expected", [
    (Real(0, 1, "a"), 3, [0.0, 0.5, 1.0]),
    (Integer(0, 100, "a"), 10, [0, 11, 22, 33, 44, 56, 67, 78, 89, 100]),
    (Integer(0, 3, "a"), 10, [0, 1, 2, 3]),
    (Integer(0, 5, "a"), 3, [0, 2, 5]),                                  # Python's round: 2.5 goes to the even 2
])
def test_axes(arg, n, expected):
    names, axes = axes_of(arg, n=n)
    assert names == ["a"] and axes == [expected]
    assert all(type(v) is type(e) for v, e in zip(axes[0], expected))


def test_specify_lists_and_constants():
    names, axes = axes_of(Real(0, 1, "lr"), Constant(7, "seed"), Integer(0, 100, "k"), n=3, specify={"lr": [1e-3, 1e-2, 1e-1]})
    assert names == ["lr", "k"]                                          # the Constant makes no axis
    assert axes == [[1e-3, 1e-2, 1e-1], [0, 50, 100]]
    names, axes = axes_of(Real(0, 1, "lr"), n=1, specify={"lr": [0.25]})  # a listed axis may have one value
    assert axes == [[0.25]]
    _, axes = axes_of(Real(0, 1, "lr"), Integer(0, 9, "k"), n=2, specify={"k": 4})   # a count for one axis
    assert axes == [[0.0, 1.0], [0, 3, 6, 9]]


def test_n_below_two_raises_with_the_reference_message():
    with pytest.raises(ValueError) as e:
        axes_of(Real(0, 1, "lr"), n=1)
    assert str(e.value) == "n can't be less than 2 for a grid search, do a constant parameter instead"
    with pytest.raises(ValueError):
        axes_of(Integer(0, 4, "k"), n=3, specify={"k": 1})


def test_second_compile_replaces_the_axes():
    g = GridOptimizer()
    g.compile(lambda *p: 0.0, Real(0, 1, "a"), Real(0, 1, "b"), n=2, verbose=False)
    g.compile(lambda *p: 0.0, Integer(0, 1, "c"), n=2, verbose=False)
    assert g._names == ["c"] and g._axes == [[0, 1]]


def test_optimize_walks_product_order_and_calls_a_plain_f_once_per_point():
    calls = []

    def f(a, k):
        calls.append((a, k))
        return 10.0 * a + k

    g = GridOptimizer()
    g.compile(f, Real(0, 1, "a"), Integer(0, 2, "k"), n=3, verbose=False)
    g.optimize()
    expected = list(itertools.product([0.0, 0.5, 1.0], [0, 1, 2]))
    assert calls == expected and list(g._results) == expected and list(g.results) == expected
    assert all(g._results[p] == 10.0 * p[0] + p[1] for p in expected)
    assert g.results is not g._results
    g.optimize()                                                         # a second search starts from nothing
    assert len(calls) == 18 and list(g._results) == expected


def test_progress_line(capsys):
    g = GridOptimizer()
    g.compile(lambda a: a, Real(0, 1, "a"), n=2)                         # verbose by default, as the reference
    g.optimize()
    out = capsys.readouterr().out
    assert out.endswith("\rGrid Optimizer 100 % [====================] completed: 2/2")
    assert "\rGrid Optimizer 50 % [==========>] completed: 1/2" in out
    g.compile(lambda a: a, Real(0, 1, "a"), n=2, verbose=False)
    g.optimize()
    assert capsys.readouterr().out == ""


def test_save_writes_the_reference_text_format(tmp_path):
    g = GridOptimizer()
    g.compile(lambda a, k: a - k, Real(0, 1, "alpha"), Integer(3, 4, "k"), n=2, verbose=False)
    g.optimize()
    path = tmp_path / "grid.txt"
    g.save(str(path))
    assert path.read_text() == "alpha,k\n0.0,3\n-3.0\n0.0,4\n-4.0\n1.0,3\n-2.0\n1.0,4\n-3.0\n"


def test_best():
    g = GridOptimizer()
    with pytest.raises(ValueError):
        g.best()
    g.compile(lambda a, k: (a - 0.5) ** 2 + k, Real(0, 1, "a"), Integer(0, 1, "k"), n=3, verbose=False)
    g.optimize()
    assert g.best() == ((0.5, 0), 0.0) and g.best(minimize=True) == ((0.5, 0), 0.0)
    assert g.best(minimize=False) == ((0.0, 1), 1.25)                    # the first of the two largest, in grid order


class Lanes:
    def __init__(self):
        self.calls, self.single = [], 0

    def evaluate_lanes(self, names, points):
        self.calls.append((list(names), list(points)))
        return [sum(p) for p in points]

    def __call__(self, *point):
        self.single += 1
        return sum(point)


def test_an_f_with_evaluate_lanes_gets_every_point_in_one_call():
    f = Lanes()
    g = GridOptimizer()
    g.compile(f, Real(0, 1, "a"), Constant(1, "c"), Integer(0, 2, "k"), n=3, verbose=False)
    g.optimize()
    expected = list(itertools.product([0.0, 0.5, 1.0], [0, 1, 2]))
    assert f.single == 0 and len(f.calls) == 1
    assert f.calls[0] == (["a", "k"], expected)
    assert list(g._results) == expected and all(g._results[p] == sum(p) for p in expected)

    class Short(Lanes):
        def evaluate_lanes(self, names, points):
            return [0.0]
    g.compile(Short(), Real(0, 1, "a"), n=2, verbose=False)
    with pytest.raises(ValueError):
        g.optimize()


def test_sgld_grid_objective_refuses_unknown_names_and_options():
    hp = HyperParameters(lr_upper=0.02, lr_lower=0.005, lr_gamma=0.9, batch_size=16)
    obj = SGLDGridObjective(hp, "{}", None, 10)
    with pytest.raises(ValueError, match="momentum"):
        obj.evaluate_lanes(["lr_upper", "momentum"], [(0.1, 0.9)])
    with pytest.raises(ValueError, match="momentum"):
        obj(0.1, 0.9, names=["lr_upper", "momentum"])
    assert obj.trainings == []
    assert SGLDGridObjective.NAMES == ("lr_upper", "lr_lower", "lr_gamma", "batch_size")
    for bad in ({"metric": "accuracy"}, {"weights": "median"}, {"max_lanes": 0}):
        with pytest.raises(ValueError):
            SGLDGridObjective(hp, "{}", None, 10, **bad)


def test_compat_package_exports_the_same_objects():
    import importlib
    import os
    import sys
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "compat")
    sys.path.insert(0, root)
    try:
        mod = importlib.import_module("Pyesian.optimizers.hyperparameters")
    finally:
        sys.path.remove(root)
    for name in ("HyperParameters", "Parameter", "Number", "Real", "Integer", "Constant", "HyperparameterOptimizer",
                 "GridOptimizer", "SGLDGridObjective"):
        assert getattr(mod, name) is getattr(importlib.import_module("bayesian_inference_for_nn_amd.optimizers.hyperparameters"), name)

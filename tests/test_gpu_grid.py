"""The SGLD surface with lanes, and a grid search through it (GridOptimizer + SGLDGridObjective), on the 1 -> 5 -> 1
regression of the chains surface test."""

import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BASE = dict(lr_upper=0.02, lr_lower=0.005, lr_gamma=0.9, batch_size=16)
LANES = [{"lr_upper": 0.03}, {"lr_gamma": 0.6}, {"lr_lower": 0.001, "lr_upper": 0.01}]
NEW = ("sgld_lanes_step", "sgld_lanes_run")
OLD = ("sgld_step", "sgld_run", "sgld_chains_step", "sgld_chains_run")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def regression():
    from bayesian_inference_for_nn_amd import synth
    from bayesian_inference_for_nn_amd.datasets import Dataset
    from bayesian_inference_for_nn_amd.losses import MeanSquaredError
    from bayesian_inference_for_nn_amd.nn import sequential_json
    x, y = synth.linreg(70)
    x, y = x / 20.0, y / 40.0
    return Dataset((x, y), MeanSquaredError, "Regression", seed=0), sequential_json(1, [5, 1], ["tanh", "linear"])


def compiled(seed=17, base=BASE, **kw):
    from bayesian_inference_for_nn_amd.optimizers import SGLD
    from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters
    ds, cfg = regression()
    opt = SGLD()
    opt.compile(HyperParameters(**base), cfg, ds, verbose=False, seed=seed, **kw)
    return opt


def count_calls(opt, names=NEW + OLD):
    """Counting wrappers on the plan's step and run methods."""
    calls = {name: 0 for name in names}
    for name in calls:
        inner = getattr(opt._plan, name)

        def wrapper(*a, _inner=inner, _name=name, **kw):
            calls[_name] += 1
            return _inner(*a, **kw)
        setattr(opt._plan, name, wrapper)
    return calls


def state(opt):
    return {name: getattr(opt, name).cpu().numpy().copy() for name in ("_theta", "_mean_dev", "_sq_mean_dev")}


def test_quiet_train_equals_step_calls_bit_for_bit(gpu_device):
    P, n = len(LANES), 20
    a, b = compiled(lanes=LANES), compiled(lanes=LANES)
    D = a._D
    assert a._theta.shape == (P, D) and a._plan.max_particles == P
    start = a._theta.cpu().numpy()
    assert all(np.array_equal(start[c], start[0]) for c in range(P))                  # shared: every lane from chain 0's draw
    assert np.array_equal(start[0], compiled()._theta.cpu().numpy())                  # ... which is the one-chain start
    calls_a, calls_b = count_calls(a), count_calls(b)
    a.train(n)                                        # quiet: pyz_sgld_lanes_run through _run_resident_chunks
    b._nb_iterations = n
    b._init_sgld_lr()
    for _ in range(n):
        ret = b.step()
    assert calls_a == {**{k: 0 for k in OLD}, "sgld_lanes_step": 0, "sgld_lanes_run": 1}
    assert calls_b == {**{k: 0 for k in OLD}, "sgld_lanes_step": n, "sgld_lanes_run": 0}
    sa, sb = state(a), state(b)
    for name in sa:
        assert np.array_equal(bits(sa[name]), bits(sb[name])), name
    assert a._n == b._n == n and a.last_losses.shape == (n, P)
    assert float(ret) == pytest.approx(float(a._running_dev.item()) / n, rel=1e-5)
    theta = sa["_theta"]
    assert len({theta[c].tobytes() for c in range(P)}) == P                           # the lanes did take their own rates
    # result() and r_hat() have nothing to pool; chain_results() has one model per lane
    with pytest.raises(ValueError):
        a.result()
    with pytest.raises(ValueError):
        a.r_hat()
    chains = a.chain_results()
    assert len(chains) == P
    for c, ch in enumerate(chains):
        assert np.array_equal(ch._model.weights_flat, theta[c])
    # lane_scores() is plan.lane_scores on the split, divided by its rows
    for split, weights in (("valid", "theta"), ("test", "mean"), ("train", "theta")):
        got = a.lane_scores(split=split, weights=weights)
        if split == "train":
            x_dev, y_dev = a._x_dev, a._y_dev
        else:
            xs, ys = getattr(a._dataset, split + "_data").as_numpy()
            x_dev = torch.as_tensor(np.asarray(xs, dtype=np.float32).reshape(len(xs), -1)).cuda()
            y_dev = torch.as_tensor(np.asarray(ys, dtype=np.float32).reshape(len(ys), -1)).cuda()
        w = a._theta if weights == "theta" else a._mean_dev
        B, rows = a._plan.max_batch, int(x_dev.shape[0])
        total = np.zeros(P)
        for r0 in range(0, rows, B):
            s, e = a._plan.lane_scores(w, x_dev[r0:r0 + B], y_dev[r0:r0 + B])
            total = total + s.cpu().numpy()
            assert not e.any()                                                        # MSE: no error count
        assert got["n"] == rows and got["loss"].dtype == np.float64 and got["loss"].shape == (P,)
        assert np.array_equal(got["loss"], total / rows) and np.array_equal(got["error"], np.zeros(P))
        assert np.all(np.isfinite(got["loss"])) and len(set(got["loss"].tolist())) == P
    assert rows > B                                                                    # the train split took more than one chunk
    with pytest.raises(ValueError):
        a.lane_scores(split="all")


def test_lanes_at_the_base_point_with_distinct_seeds_are_n_chains(gpu_device):
    P, n = 3, 12
    a = compiled(lanes=[{}] * P, lane_seeds="distinct")
    b = compiled(n_chains=P)
    assert np.array_equal(a._theta.cpu().numpy(), b._theta.cpu().numpy())
    a.train(n)
    b.train(n)
    sa, sb = state(a), state(b)
    for name in sa:
        assert np.array_equal(bits(sa[name]), bits(sb[name])), name
    assert np.array_equal(bits(a.last_losses.cpu().numpy()), bits(b.last_losses.cpu().numpy()))
    # one lane is a lane run as well (a (1, D) state), not the one-chain optimizer
    one = compiled(lanes=[{"lr_upper": 0.03}])
    calls = count_calls(one)
    one.train(5)
    one.step()
    assert one._theta.shape == (1, one._D) and calls["sgld_lanes_run"] == 1 and calls["sgld_lanes_step"] == 1
    assert sum(calls[k] for k in OLD) == 0 and len(one.chain_results()) == 1
    assert one.lane_scores()["loss"].shape == (1,)


def test_compile_refusals_and_the_untouched_paths(gpu_device):
    with pytest.raises(ValueError):
        compiled(lanes=LANES, n_chains=3)
    with pytest.raises(ValueError):
        compiled(lanes=LANES, lane_seeds="random")
    with pytest.raises(ValueError):
        compiled(lanes=[])
    with pytest.raises(ValueError):
        compiled(lanes=[{"batch_size": 8}])
    # without lanes nothing reaches the new methods
    for kw in ({}, {"n_chains": 2}):
        opt = compiled(**kw)
        calls = count_calls(opt)
        opt.train(6)
        opt._nb_iterations = 6
        opt.step()
        assert calls["sgld_lanes_step"] == calls["sgld_lanes_run"] == 0 and sum(calls.values()) == 2
        opt.result()


def test_lanes_refuse_a_world_of_several_ranks(gpu_device, monkeypatch):
    from bayesian_inference_for_nn_amd import parallel
    monkeypatch.setattr(parallel, "world_info", lambda: (0, 2))
    monkeypatch.setattr(parallel, "shared_seed", lambda seed: 17)
    with pytest.raises(ValueError, match="one rank"):
        compiled(lanes=LANES)


def test_grid_search_through_the_lanes(gpu_device):
    from bayesian_inference_for_nn_amd.optimizers.hyperparameters import GridOptimizer, HyperParameters, Real, SGLDGridObjective
    ds, cfg = regression()
    hp = HyperParameters(**BASE)
    n, seed = 15, 23
    obj = SGLDGridObjective(hp, cfg, ds, n, metric="val_loss", seed=seed, max_lanes=4)
    grid = GridOptimizer()
    grid.compile(obj, Real(0.01, 0.05, "lr_upper"), Real(0.5, 0.9, "lr_gamma"), n=3, specify={"lr_gamma": [0.5, 0.9]},
                 verbose=False)
    grid.optimize()
    eps = (0.05 - 0.01) / 2
    points = list(itertools.product([i * eps + 0.01 for i in range(3)], [0.5, 0.9]))
    assert obj.trainings == [4, 2]
    assert list(grid._results) == points
    assert all(isinstance(v, float) and np.isfinite(v) for v in grid._results.values())
    assert len(set(grid._results.values())) == len(points)
    for chunk in (points[:4], points[4:]):
        lanes = [{"lr_upper": u, "lr_gamma": g} for u, g in chunk]
        opt = compiled(seed=seed, lanes=lanes)
        opt.train(n)
        direct = opt.lane_scores(split="valid", weights="theta")["loss"]
        for p, v in zip(chunk, direct):
            assert grid._results[p] == float(v), p                                    # bit for bit: the same float64
    point, value = grid.best()
    assert value == min(grid._results.values()) and grid._results[point] == value
    # one point through __call__: a one-lane chunk (the reference's serial loop), its own training
    single = obj(0.03, names=["lr_upper"])
    assert obj.trainings == [4, 2, 1] and np.isfinite(single)
    # the error metric of a regression is 0 everywhere
    err = SGLDGridObjective(hp, cfg, ds, 5, metric="val_error", weights="mean", seed=seed, max_lanes=4)
    assert err.evaluate_lanes(["lr_upper", "batch_size"], [(0.02, 16), (0.03, 8), (0.04, 16)]) == [0.0, 0.0, 0.0]
    assert err.trainings == [2, 1]                                                    # grouped by batch size

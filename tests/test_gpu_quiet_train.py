"""The quiet train() skeleton every optimizer with a device-resident run shares (Optimizer._train_resident): a model the
run does not take goes to the step loop before anything is planned; a refusal of the first chunk gives the batches back
and takes the step loop; a refusal after a chunk went out is raised; and the bookkeeping replayed after a run leaves
SGD's running loss as the step loop's float32 additions do.

Two twins compiled alike, one driven by train() and one by step(), on moons: 500 rows (400 training rows, batches of 64:
seven per epoch, the last one of 16), 2 -> 16 -> C.  Where both twins take the step loop on the same batches, and for the
running loss -- the fold restates the step loop's additions -- the comparison is exact (torch.equal).

The library is never made to fail: a refusal is a PyzError raised by a stand-in for the run method of the Python plan."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from bayesian_inference_for_nn_amd import _lib, synth
from bayesian_inference_for_nn_amd.datasets import Dataset
from bayesian_inference_for_nn_amd.distributions import GaussianPrior
from bayesian_inference_for_nn_amd.losses import SparseCategoricalCrossentropy
from bayesian_inference_for_nn_amd.nn import model_from_json, sequential_json
from bayesian_inference_for_nn_amd.optimizers import ADAM, BBB, SGD, SWAG
from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters

HYPS = {
    SGD: dict(lr=0.05, frequency=4, batch_size=64),
    SWAG: dict(lr=0.03, k=4, frequency=5, scale=1.0, batch_size=64),
    BBB: dict(lr=5e-3, alpha=0.01, batch_size=64),
    ADAM: dict(lr=0.01, beta_1=0.9, beta_2=0.999, batch_size=64),
}
RUN = {SGD: "sgd_run", SWAG: "swag_run", BBB: "bbb_run", ADAM: "adam_run"}      # the plan method of the class's run
TENSORS = ("_theta", "_mean_dev", "_sq_mean_dev", "_dev_rows", "_m_dev", "_v_dev", "_mu", "_rho", "_w", "_cost",
           "_running_dev", "_loss_dev")
COUNTS = ("_n", "_step", "_n_cols", "_epoch", "_pos", "_epoch_num", "_seen_batches", "_total_batches")


def compiled(cls, classes=2, **kwargs):
    x, y = synth.moons(500, seed=42)
    ds = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", seed=5)
    cfg = sequential_json(2, [16, classes], ["relu", "softmax"])
    if cls is BBB:
        kwargs["prior"] = GaussianPrior(0.0, -2.0)
    else:
        start = model_from_json(cfg)
        start.reset_glorot(np.random.default_rng(9))
        kwargs["starting_model"] = start
    opt = cls()
    opt.compile(HyperParameters(**HYPS[cls]), cfg, ds, verbose=False, seed=11, **kwargs)
    return opt


def steps_done(opt):
    return opt._step if isinstance(opt, BBB) else opt._n


def assert_twins(a, b):
    """Every state tensor, count and iterator position the class has, and BBB's loss lists."""
    seen = 0
    for t in TENSORS:
        if hasattr(b, t):
            assert torch.equal(getattr(a, t), getattr(b, t)), t
            seen += 1
    assert seen >= 4
    for t in COUNTS:
        if hasattr(b, t):
            assert getattr(a, t) == getattr(b, t), (t, getattr(a, t), getattr(b, t))
    assert np.array_equal(a._perm_host, b._perm_host)
    if isinstance(b, BBB):
        for name in ("train_losses", "val_losses"):
            assert [float(v) for v in getattr(a, name)] == [float(v) for v in getattr(b, name)], name


def refuse_call(monkeypatch, opt, which):
    """The plan's run method raises the library's error on its `which`-th call (1-based); returns the list of calls."""
    real, calls = getattr(opt._plan, RUN[type(opt)]), []

    def run(*args, **kwargs):
        calls.append(len(calls) + 1)
        if calls[-1] == which:
            raise _lib.PyzError(-1, "refused by the test")
        return real(*args, **kwargs)
    monkeypatch.setattr(opt._plan, RUN[type(opt)], run)
    return calls


@pytest.mark.parametrize("cls", [SGD, SWAG, BBB])
def test_unfused_model_takes_the_step_loop(cls, gpu_device):
    """A last layer of 40 units, which the chained runs refuse: train() takes the step loop, decided before anything is
    planned or enqueued -- the first batch of the loop is the first batch of the iterator."""
    a, b = compiled(cls, classes=40), compiled(cls, classes=40)
    a.train(20)
    for _ in range(20):
        b.step()
    assert steps_done(a) == 20
    assert_twins(a, b)
    assert not hasattr(a, "last_losses") and not hasattr(a, "_res_idx")


@pytest.mark.parametrize("cls", [SGD, SWAG, BBB, ADAM])
def test_refused_first_chunk_gives_the_batches_back(cls, gpu_device, monkeypatch):
    """The library refuses the first chunk of the run: nothing ran, the batch iterator and its generator are put back
    and train() takes the step loop from the first batch."""
    a, b = compiled(cls), compiled(cls)
    calls = refuse_call(monkeypatch, a, 1)
    a.train(40)
    for _ in range(40):
        b.step()
    assert calls == [1], "one attempt at the run, then the step loop"
    assert steps_done(a) == 40
    assert_twins(a, b)
    assert not hasattr(a, "last_losses")


@pytest.mark.parametrize("cls", [SWAG, BBB])
def test_refused_later_chunk_is_raised(cls, gpu_device, monkeypatch):
    """A refusal after a chunk went out cannot fall back -- the steps of that chunk have run: train() raises, and the
    step count does not claim the run."""
    a = compiled(cls)
    a._resident_chunks = (16, 1.0, 16)
    calls = refuse_call(monkeypatch, a, 2)
    with pytest.raises(_lib.PyzError, match="refused by the test"):
        a.train(40)
    torch.cuda.synchronize()
    assert calls == [1, 2]
    assert steps_done(a) != 40


@pytest.mark.parametrize("members", [1, 3])
def test_sgd_quiet_running_loss_is_the_step_loops(members, gpu_device):
    """train(75) -- ten epoch changes -- and train(20) on top, a run that opens on the old epoch: the epoch's running loss
    after each equals the step loop's bit for bit (with members: of the device mean over members, as step() adds it)."""
    kwargs = {"n_members": members} if members > 1 else {}
    a, b = compiled(SGD, **kwargs), compiled(SGD, **kwargs)
    for n_it in (75, 20):
        a.train(n_it)
        per_step = []
        for _ in range(n_it):
            b.step()
            per_step.append(float(b._running_dev.item()))
        assert a.last_losses.shape == ((n_it,) if members == 1 else (n_it, members))
        for t in ("_n", "_epoch_num", "_seen_batches", "_epoch", "_pos"):
            assert getattr(a, t) == getattr(b, t), (t, getattr(a, t), getattr(b, t))
        if not torch.equal(a._running_dev, b._running_dev):
            # the first step at which the fold of the run's losses leaves the step loop's sums
            step_loss = a.last_losses if members == 1 else a.last_losses.mean(dim=1)
            acc, first = np.float32(0.0), None
            for s, v in enumerate(step_loss.cpu().numpy()[n_it - a._seen_batches:]):
                acc = np.float32(acc + v)
                if acc != np.float32(per_step[n_it - a._seen_batches + s]):
                    first = (n_it - a._seen_batches + s, float(acc), per_step[n_it - a._seen_batches + s])
                    break
            pytest.fail(f"running loss {float(a._running_dev.item())!r} != {float(b._running_dev.item())!r} after "
                        f"train({n_it}); first differing step (step, fold, step loop): {first}")
    assert a._n == 95 and a._epoch_num == 14

"""pyz_hmc_run (consecutive HMC proposals with the uniforms, the per-proposal scalars and the sample record of
HMC.py:92-103 on the device) against a loop of pyz_hmc_step from the same q0, seed, step0 and uniforms: q, every
proposal's statistics, the counts, the frequencies and the recorded rows bit for bit, on each of the four kernel paths,
replayed from graphs and launched eagerly.  Then the Python surface: a quiet HMC.train through the run against the
step loop (PYZ_HMC_RUN=0), and one sliced case against the float64 oracle proposal by proposal."""

import math
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import hmc_cases as hc  # noqa: E402
from hmc_cases import CASE_BY_NAME, case_data, compare, expected_path  # noqa: E402

from bayesian_inference_for_nn_amd import synth  # noqa: E402
from bayesian_inference_for_nn_amd.datasets import Dataset  # noqa: E402
from bayesian_inference_for_nn_amd.distributions import GaussianPrior  # noqa: E402
from bayesian_inference_for_nn_amd.losses import SparseCategoricalCrossentropy  # noqa: E402
from bayesian_inference_for_nn_amd.nn import sequential_json  # noqa: E402
from bayesian_inference_for_nn_amd.optimizers import HMC  # noqa: E402
from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters  # noqa: E402

SENTINEL = -12345.0
# (case of tests/hmc_cases.CASES, the path it must take): every path, chain counts 1, 2, 3 and 16, D % 4 == 0 and != 0
RUN_CASES = [("fused_b1_relu_l20_philox", "fused"), ("res_b0_relu_c3", "resident"), ("res_b0_linear_16_chains", "resident"),
             ("multi_b0_sigmoid_mse_sigmoid", "multi"), ("gen_d255_fused_off", "generic"), ("gen_vec_prior_two_layers", "generic")]
N_STEPS, N_BURN = 8, 2


@pytest.fixture(scope="module")
def eng(gpu_device):
    found = sorted(k for k in os.environ if k.startswith("PYZ_HMC_"))
    if found:
        pytest.fail(f"{', '.join(found)} set in the environment: the cases set the switches themselves -- unset them")
    from bayesian_inference_for_nn_amd import engine
    return engine


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def set_env(monkeypatch, case, chunk=None):
    for k in hc.PER_CALL_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if chunk is not None:
        monkeypatch.setenv("PYZ_HMC_RUN_CHUNK", str(chunk))


class Bench:
    """One plan, the device inputs of a case and a side stream (the legacy default stream cannot be captured)."""

    def __init__(self, eng, case):
        self.case, self.data = case, case_data(case)
        spec = case.spec
        self.plan = eng.MLPPlan(eng.MLPSpec(spec.dims, spec.acts, spec.loss), max_batch=case.rows, max_particles=case.P)
        self.x = dev(self.data.x)
        self.y = dev(self.data.y, torch.int32 if case.loss == "scce" else torch.float32)
        self.pm = dev(self.data.prior_mu) if case.vec_prior else None
        self.ps = dev(self.data.prior_sigma) if case.vec_prior else None
        self.mu, self.sg = (0.0, 1.0) if case.vec_prior else (self.data.prior_mu, self.data.prior_sigma)
        self.stream = torch.cuda.Stream()
        self.q_loop = dev(self.data.q0)          # the loop always runs on the same buffers: one graph of its own
        self.stats = torch.zeros((case.P, 8), device="cuda")

    def step(self, us, step, burning):
        c = self.case
        with torch.cuda.stream(self.stream):
            self.plan.hmc_step(self.q_loop, self.x, self.y, c.L, c.eps, c.m, self.mu, self.sg, us, step, c.seed, self.stats,
                               burning=burning, prior_mean_vec=self.pm, prior_sigma_vec=self.ps)
        self.stream.synchronize()
        return self.stats.cpu().numpy().copy()

    def loop(self, n_steps, n_burn):
        """n_steps calls of pyz_hmc_step from q0 with the bookkeeping of HMC.py:75-77, 92-103 on the host.  The uniform of
        a sampling proposal is placed a factor of two from the acceptance ratio of that very proposal (read from a
        burning call on the same state, undone afterwards): chain c of proposal i is accepted iff i + c is even."""
        c = self.case
        torch.cuda.synchronize()
        self.q_loop.copy_(dev(self.data.q0))
        us_all, stats_all = [], []
        rows, freq = [[] for _ in range(c.P)], [[] for _ in range(c.P)]
        for i in range(n_steps):
            burning = i < n_burn
            us = [0.5] * c.P
            if not burning:
                keep = self.q_loop.clone()
                lr = self.step(us, c.step + i, True)[:, 6]
                self.q_loop.copy_(keep)
                us = [float(np.float32(0.5 * math.exp(min(l, 50.0)) if (i + ch) % 2 == 0 else 2.0 * math.exp(min(l, 50.0)) + 0.1))
                      if np.isfinite(l) else 0.5 for ch, l in enumerate(lr)]
                for ch in range(c.P):
                    if not freq[ch]:
                        freq[ch].append(1)
                        rows[ch].append(self.q_loop[ch].clone())
            st = self.step(us, c.step + i, burning)
            assert (st[:, 7] == 0).all()
            if not burning:
                for ch in range(c.P):
                    if st[ch, 0] != 0:
                        freq[ch].append(1)
                        rows[ch].append(self.q_loop[ch].clone())
                    else:
                        freq[ch][-1] += 1
            us_all.append(us)
            stats_all.append(st)
        return np.asarray(us_all, dtype=np.float32), np.stack(stats_all), self.q_loop.clone(), rows, freq

    def record(self, cap, slots, guard_rows=0):
        P, D = self.case.P, self.case.D
        buf = torch.full((P * cap * D + guard_rows * D,), SENTINEL, device="cuda")
        fbuf = torch.full((P * cap + guard_rows,), -77, dtype=torch.int32, device="cuda")
        fbuf[:P * cap] = 0
        return dict(samples=buf[:P * cap * D].view(P, cap, D), freq=fbuf[:P * cap].view(P, cap), buf=buf, fbuf=fbuf,
                    count=torch.zeros(P, dtype=torch.int32, device="cuda"), fail=torch.zeros(4, dtype=torch.int32, device="cuda"),
                    stats_all=torch.full((slots, P, 8), SENTINEL, device="cuda"), q=dev(self.data.q0))

    def run(self, rec, us, n_burn, step0, use_graph=True, slot0=0):
        c = self.case
        with torch.cuda.stream(self.stream):
            self.plan.hmc_run(rec["q"], self.x, self.y, c.L, c.eps, c.m, self.mu, self.sg, us, n_burn, step0, c.seed,
                              rec["stats_all"], rec["samples"], rec["freq"], rec["count"], rec["fail"], use_graph=use_graph,
                              slot0=slot0, prior_mean_vec=self.pm, prior_sigma_vec=self.ps)
        self.stream.synchronize()

    def close(self):
        self.plan.close()


def assert_record_equals_loop(rec, ref, what):
    us, stats, q_end, rows, freq = ref
    assert torch.equal(rec["q"], q_end), f"{what}: the final q differs"
    assert torch.equal(rec["stats_all"][:len(stats)].cpu(), torch.as_tensor(stats)), f"{what}: the statistics differ"
    count = rec["count"].cpu().numpy()
    assert list(count) == [len(r) for r in rows], f"{what}: counts {list(count)}"
    for ch, (r, f) in enumerate(zip(rows, freq)):
        assert rec["freq"][ch, :len(f)].cpu().tolist() == f, f"{what}: chain {ch}: frequencies"
        assert torch.equal(rec["samples"][ch, :len(r)], torch.stack(r)), f"{what}: chain {ch}: recorded rows"
    assert rec["fail"].cpu().tolist()[:3] == [0, 0, 0]


@pytest.mark.parametrize("name,path", RUN_CASES, ids=[n for n, _ in RUN_CASES])
def test_run_equals_a_loop_of_steps(eng, monkeypatch, name, path):
    case = CASE_BY_NAME[name]
    set_env(monkeypatch, case, chunk=3)          # 8 proposals: one eager, two graphs of three, one graph of one
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert expected_path(case, cu).path == path
    b = Bench(eng, case)
    ref = b.loop(N_STEPS, N_BURN)
    us, stats = ref[0], ref[1]
    acc = stats[N_BURN:, :, 0]
    assert acc.any() and not acc.all(), f"{name}: the comparison needs accepted and rejected proposals"
    assert (stats[:N_BURN, :, 0] == 1).all()
    sliced = path in ("multi", "resident")
    for use_graph in (True, False):
        rec = b.record(cap=N_STEPS - N_BURN + 1, slots=N_STEPS)
        b.run(rec, us, N_BURN, case.step, use_graph=use_graph)
        assert_record_equals_loop(rec, ref, f"{name}, use_graph={use_graph}")
        kind, steps = b.plan.last_run_path()
        assert steps == N_STEPS and kind == ("mixed" if use_graph and sliced else "eager")
        if use_graph and sliced:
            assert b.plan.last_run_graph_launches() == 3 and b.plan.hmc_run_captures() == 2
            # the same length again: nothing new to capture, the same bits
            rec2 = b.record(cap=N_STEPS - N_BURN + 1, slots=N_STEPS)
            rec2["q"] = rec["q"]
            rec2["q"].copy_(dev(b.data.q0))
            for k in ("samples", "freq", "count", "fail", "stats_all"):   # (the record's addresses are words of the run, not of the graphs)
                assert rec2[k].data_ptr() != rec[k].data_ptr()
            b.run(rec2, us, N_BURN, case.step, use_graph=True)
            assert b.plan.hmc_run_captures() == 0 and b.plan.last_run_graph_launches() == 3
            assert_record_equals_loop(rec2, ref, f"{name}, replayed")
    # slots: two calls of four proposals == one call of eight
    rec = b.record(cap=N_STEPS - N_BURN + 1, slots=N_STEPS)
    half = N_STEPS // 2
    b.run(rec, us[:half], N_BURN, case.step, slot0=0)
    assert rec["fail"].cpu().tolist()[3] == half and bool((rec["stats_all"][half:] == SENTINEL).all())
    b.run(rec, us[half:], 0, case.step + half, slot0=half)
    assert_record_equals_loop(rec, ref, f"{name}, two calls")
    assert rec["fail"].cpu().tolist()[3] == N_STEPS
    b.close()


@pytest.mark.parametrize("name", ["res_b0_relu_c3", "gen_d255_fused_off"])
def test_a_record_out_of_rows_sets_the_word_and_stays_inside(eng, monkeypatch, name):
    case = CASE_BY_NAME[name]
    set_env(monkeypatch, case)
    b = Bench(eng, case)
    n = 6
    us = np.zeros((n, case.P), dtype=np.float32)            # u = 0: every proposal with a finite ratio is accepted
    rec = b.record(cap=3, slots=n, guard_rows=4)
    b.run(rec, us, 0, case.step)
    stats = rec["stats_all"].cpu().numpy()
    assert (stats[:, :, 0] == 1).all()
    P, D, cap = case.P, case.D, 3
    assert rec["count"].cpu().tolist() == [cap] * P
    assert rec["fail"].cpu().tolist() == [P * (n - (cap - 1)), 0, 0, n]
    assert bool((rec["buf"][P * cap * D:] == SENTINEL).all()) and bool((rec["fbuf"][P * cap:] == -77).all())
    assert bool((rec["freq"] == 1).all()) and not bool((rec["samples"] == SENTINEL).any())
    assert torch.equal(rec["samples"][:, 0], dev(b.data.q0))
    b.close()


# ---------------------------------------------------------------- the surface
def moons_dataset(n=500, seed=3):
    x, y = synth.moons(n, seed=42)
    return Dataset((x, y), SparseCategoricalCrossentropy, "Classification", seed=seed)


MOONS_JSON = sequential_json(2, [16, 2], ["relu", "softmax"])


def trained(monkeypatch, run, n_chains, prior, n_iter, eps=0.02, twice=False, seed=11):
    monkeypatch.setenv("PYZ_HMC_RUN", "1" if run else "0")
    random.seed(seed)
    opt = HMC()
    opt.compile(HyperParameters(epsilon=eps, m=0.5, L=6), MOONS_JSON, moons_dataset(), verbose=False, prior=prior, seed=5,
                n_chains=n_chains)
    opt.train(n_iter)
    if twice:
        opt.train(n_iter - 3)
    return opt


def assert_same_state(a, b):
    assert a._total_runs == b._total_runs and a._accepted_runs == b._accepted_runs and a._step_count == b._step_count
    assert a._chain_freq == b._chain_freq and a._frequency == b._frequency
    assert [len(s) for s in a._chain_samples] == [len(s) for s in b._chain_samples]
    for sa, sb in zip(a._chain_samples, b._chain_samples):
        for u, v in zip(sa, sb):
            assert torch.equal(u, v)
    assert len(a._samples) == len(b._samples) and all(torch.equal(u, v) for u, v in zip(a._samples, b._samples))
    assert np.array_equal(np.asarray(a.last_stats), np.asarray(b.last_stats))
    assert torch.equal(a._q, b._q)
    ds = moons_dataset()
    xt, _ = next(iter(ds.test_data.batch(ds.test_size)))
    random.seed(99)
    _, mean_a = a.result().predict(xt, nb_samples=12)
    random.seed(99)
    _, mean_b = b.result().predict(xt, nb_samples=12)
    assert np.array_equal(np.asarray(mean_a), np.asarray(mean_b))


@pytest.mark.parametrize("n_chains,prior", [(1, GaussianPrior(0.0, 1.0)), (4, GaussianPrior(0.0, 1.0)),
                                            (2, GaussianPrior([0.0, 0.0], [1.0, 2.0]))], ids=["one chain", "four chains", "list prior"])
def test_quiet_train_through_the_run_equals_the_step_loop(gpu_device, monkeypatch, n_chains, prior):
    a = trained(monkeypatch, True, n_chains, prior, 14)
    after_a = random.random()
    b = trained(monkeypatch, False, n_chains, prior, 14)
    assert random.random() == after_a, "the run and the loop consumed different numbers of uniforms"
    assert a._plan.last_run_path()[1] == 24 and b._plan.last_run_path()[1] != 24     # 10 burn-in + 14: a took the run, b did not
    assert a._total_runs == 14 and 0 < a._accepted_runs < 14, "accepted and rejected proposals must both occur"
    assert_same_state(a, b)


def test_train_twice_in_a_row_behaves_as_the_loop_does(gpu_device, monkeypatch):
    a = trained(monkeypatch, True, 2, GaussianPrior(0.0, 1.0), 9, twice=True)
    b = trained(monkeypatch, False, 2, GaussianPrior(0.0, 1.0), 9, twice=True)
    assert a._step_count == 10 + 9 + 10 + 6 and a._total_runs == 6 and all(sum(f) == 7 for f in a._chain_freq)
    assert_same_state(a, b)


def test_the_switches_take_the_step_loop(gpu_device, monkeypatch):
    monkeypatch.setenv("PYZ_HMC_RUN_MAX_BYTES", "64")
    a = trained(monkeypatch, True, 1, GaussianPrior(0.0, 1.0), 5)
    assert a._plan.last_run_path()[1] != 15 and a._total_runs == 5 and sum(a._frequency) == 6


def test_a_refusal_of_the_library_takes_the_step_loop(gpu_device, monkeypatch):
    """pyz_hmc_run refusing its arguments (PYZ_E_SHAPE here, raised in the plan's place): the uniforms drawn for the run
    go back to `random`, and the step loop leaves what it leaves on its own."""
    from bayesian_inference_for_nn_amd._lib import PyzError
    monkeypatch.setenv("PYZ_HMC_RUN", "1")
    random.seed(11)
    a = HMC()
    a.compile(HyperParameters(epsilon=0.02, m=0.5, L=6), MOONS_JSON, moons_dataset(), verbose=False, prior=GaussianPrior(0.0, 1.0),
              seed=5, n_chains=2)
    calls = []

    def refuse(*args, **kw):
        calls.append(1)
        raise PyzError(-2, "particle count outside the plan")
    monkeypatch.setattr(a._plan, "hmc_run", refuse)
    a.train(7)
    after_a = random.random()
    b = trained(monkeypatch, False, 2, GaussianPrior(0.0, 1.0), 7)
    assert calls == [1] and random.random() == after_a
    assert_same_state(a, b)


def test_a_give_up_raises_as_the_step_loop_does(gpu_device, monkeypatch):
    """PYZ_HMC_SPIN_LIMIT = -1 (the switch of tests/test_gpu_hmc_resident.py): no resident proposal completes.  The
    designed give-up branch, once."""
    monkeypatch.setenv("PYZ_HMC_SPIN_LIMIT", "-1")
    monkeypatch.setenv("PYZ_HMC_RUN", "1")
    random.seed(3)
    opt = HMC()
    opt.compile(HyperParameters(epsilon=0.02, m=0.5, L=6), MOONS_JSON, moons_dataset(), verbose=False,
                prior=GaussianPrior(0.3, 1.0), seed=5)
    opt._nb_burn_epoch = 1
    q_before = opt._q.clone()
    with pytest.raises(RuntimeError, match="gave up waiting for its row-slice workgroups"):
        opt.train(2)
    assert torch.equal(opt._q, q_before)
    assert opt._plan.last_run_path()[1] == 3


# ---------------------------------------------------------------- one sliced case against the oracle
def test_a_run_against_the_oracle_proposal_by_proposal(eng, monkeypatch):
    """Six Philox proposals of a sliced case in one run, the third rejected.  The q before every proposal is rebuilt from
    (samples, freq); the oracle starts each proposal from the device's own previous state, as the sequence test of
    tests/test_gpu_hmc_matrix.py does, with the same comparison and the tolerances of the float32 oracle over such a
    sequence.  The uniforms are placed on the CPU, a factor of two from the float64 oracle's acceptance ratio along its
    own trajectory, so no proposal has to be left out of the accept comparison (at most one in ten may be, and only
    with |log u - log_ratio| inside the case's own tolerance)."""
    case = CASE_BY_NAME["res_b0_relu_c3"]
    assert case.P == 1 and case.momentum == "philox"
    set_env(monkeypatch, case, chunk=3)
    assert expected_path(case, torch.cuda.get_device_properties(0).multi_processor_count).NW >= 2
    n = 6
    data = case_data(case)
    rel32 = hc.sequence_rel32(case, n)
    q, us = data.q0[0].copy(), []
    for k in range(n):
        z = hc.philox_z(case, 0, step=case.step + k)
        ref = hc.oracle_result(case, data, 0, u=0.5, q=q, z=z)
        ratio = math.exp(min(ref["log_ratio"], 50.0))
        us.append(float(np.float32(2.0 * ratio + 0.1 if k == 2 else 0.5 * ratio)))
        f32 = hc.oracle_result(case, data, 0, np.float32, u=us[k], q=q, z=z)
        assert f32["accepted"] == (k != 2)
        q = np.asarray(ref["q_proposed"], dtype=np.float32) if k != 2 else q
    b = Bench(eng, case)
    rec = b.record(cap=n + 1, slots=n)
    b.run(rec, np.asarray(us, dtype=np.float32).reshape(n, 1), 0, case.step)
    count = int(rec["count"][0])
    rows, freq = rec["samples"][0, :count].cpu().numpy(), rec["freq"][0, :count].cpu().tolist()
    assert sum(freq) == n + 1
    seq = [rows[r] for r, f in enumerate(freq) for _ in range(f)]      # seq[i]: q before proposal i, seq[i + 1]: after it
    stats = rec["stats_all"].cpu().numpy()
    left_out = 0
    keys = dict(U0=2, K0=3, U1=4, K1=5, log_ratio=6)
    for i in range(n):
        z = hc.philox_z(case, 0, step=case.step + i)
        ref = hc.oracle_result(case, data, 0, u=us[i], q=seq[i], z=z)
        b.q_loop.copy_(dev(seq[i][None, :]))
        burn_stats = b.step([us[i]], case.step + i, True)         # the proposal itself, from the same state
        burn = dict(q=b.q_loop[0].cpu().numpy(), loss=burn_stats[0, 1])
        s = stats[i, 0]
        accepted = bool(s[0] != 0)
        scale = max(abs(ref[k]) for k in ("U0", "K0", "U1", "K1"))
        tol = min(max(hc.FACTOR * rel32["log_ratio"] * scale, hc.F32_EPS * scale), hc.CAP * scale)
        if accepted != ref["accepted"] and abs(math.log(us[i]) - ref["log_ratio"]) <= tol:
            left_out += 1
            accepted = ref["accepted"]
        metro = dict(accepted=accepted, q=seq[i + 1] if accepted == bool(s[0] != 0) else (burn["q"] if accepted else seq[i]),
                     loss=s[1], **{k: s[j] for k, j in keys.items()})
        report = compare(hc.result_from(case, seq[i], z, burn, metro), ref, case, what=f"proposal {i}: ", rel32=rel32)
        for k, (err, t) in report.items():
            print(f"run proposal {i}: {k}: error {err:.3e}, tolerance {t:.3e}")
    assert left_out * 10 <= n
    b.close()

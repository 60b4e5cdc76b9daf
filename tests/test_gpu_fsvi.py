"""FSVI on the device against the restatement of tests/fsvi_checks.py: the batched float64 SPD solve alone (every size at
which k_spd_solve_f64 takes another path), the terms of a step with injected draws, the total gradient and the update over
chained steps, the Philox draws, and the optimizer class.  Shapes are the smallest that can go wrong."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import fsvi_checks as fc

from bayesian_inference_for_nn_amd import _lib
from bayesian_inference_for_nn_amd.datasets import Dataset
from bayesian_inference_for_nn_amd.distributions import GaussianPrior
from bayesian_inference_for_nn_amd.losses import MeanSquaredError
from bayesian_inference_for_nn_amd.nn import BayesianModel, sequential_json
from bayesian_inference_for_nn_amd.optimizers import FSVI
from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters

U = 2.0 ** -53            # unit roundoff of float64


@pytest.fixture(scope="module")
def eng(gpu_device):
    from bayesian_inference_for_nn_amd import engine
    return engine


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host(t):
    return t.detach().cpu().numpy()


def close(got, ref, rel, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(got - ref).max()
    print(f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.3e})")
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.3e})"


# ---------------------------------------------------------------- the solver alone
def residual(A, x, r):
    """|A x - r| / (|A| |x|), spectral and Euclidean norms."""
    return np.linalg.norm(A @ x - r) / (np.linalg.norm(A, 2) * np.linalg.norm(x))


def random_spd(n, rng):
    G = rng.normal(size=(n, n))
    return G @ G.T / n + 0.1 * np.eye(n)


# The bound: both routes are backward stable, |A x - r| <= c n u |A| |x| with a modest c that depends on the elimination
# order (LAPACK's pivoted LU there, an unpivoted right-looking Cholesky and two substitutions here), so the device may
# exceed NumPy's measured residual by a small factor, and NumPy's can be exactly zero (n = 1): 16 x max(NumPy's, u).
MARGIN = 16.0


def solve_and_check(eng, systems, what):
    A = np.stack([s[0] for s in systems])
    R = np.stack([s[1] for s in systems])
    a_dev, r_dev = dev(A, torch.float64), dev(R, torch.float64)
    fail = eng.spd_solve(a_dev, r_dev)
    X = host(r_dev)
    assert host(fail).tolist() == [0] * len(systems), what
    for s, (a, r) in enumerate(systems):
        mine, theirs = residual(a, X[s], r), residual(a, np.linalg.solve(a, r), r)
        print(f"{what} system {s}: residual {mine:.3e}, NumPy {theirs:.3e}, ratio {mine / max(theirs, U):.2f}")
        assert mine <= MARGIN * max(theirs, U), (what, s, mine, theirs)


@pytest.mark.parametrize("n", [1, 3, 32, 33, 64, 65, 128, 129, 300, 512, 513, 1024, 1025, 2048])
def test_spd_solve_residual_against_numpy(eng, n):
    """Both sides of each boundary: 1 and 3 (fewer rows than a wave), 32 / 33 (256 threads and 1024), 64 / 65, 128 / 129 (the
    last size factorised inside LDS and the first in global memory, panels of 32 columns and a ragged last panel), 300, 512 /
    513 (the last panel width of 32 and the first of 16), 1024 / 1025 (the largest LDS request; the first of 4) and 2048,
    the entry point's limit, with one system: NumPy's side of that case (the matrix, its solve and its spectral norm) is
    what takes the time, see DESIGN 5."""
    rng = np.random.default_rng(n)
    solve_and_check(eng, [(random_spd(n, rng), rng.normal(size=n)) for _ in range(1 if n == 2048 else 3)], f"n={n}")


def test_spd_solve_hard_gp_matrix_and_stein_matrix(eng):
    rng = np.random.default_rng(1)
    K = fc.hard_gp_matrix(256)                                   # cond 1.9e8
    assert 1e8 < np.linalg.cond(K) < 1e9
    solve_and_check(eng, [(K, rng.normal(size=256)) for _ in range(3)], "hard GP matrix")
    stein = [fc.stein_system(rng.normal(size=151).astype(np.float32)) for _ in range(3)]
    assert all(np.linalg.cond(a) < 1e6 for a, _ in stein)
    solve_and_check(eng, stein, "Stein matrix D=151")


@pytest.mark.parametrize("n", [4, 129])
def test_spd_solve_flags_a_matrix_that_is_not_positive_definite(eng, n):
    """A negative eigenvalue: the flag is set and the solution NaN; the systems beside it are solved.  A normal return."""
    rng = np.random.default_rng(9)
    good = random_spd(n, rng)
    bad = good.copy()
    bad[n // 2, n // 2] = -1.0
    assert np.linalg.eigvalsh(bad).min() < 0
    A = np.stack([good, bad, good])
    r = rng.normal(size=(3, n))
    a_dev, r_dev = dev(A, torch.float64), dev(r, torch.float64)
    fail = eng.spd_solve(a_dev, r_dev)
    X = host(r_dev)
    assert host(fail).tolist() == [0, 1, 0]
    assert np.isnan(X[1]).all()
    for s in (0, 2):
        assert residual(good, X[s], r[s]) <= MARGIN * max(residual(good, np.linalg.solve(good, r[s]), r[s]), U)


# ---------------------------------------------------------------- one step with injected draws
# The GP prior matrix of these step tests is the identity by construction: rows uniform in [-30, 30]^2 lie far apart on the
# kernel's length scale of 1, so alpha = f / (1 + 1e-6) whatever k_fsvi_gram computes off the diagonal.  What they see of
# it is an accidental pair of rows here and there (the median over the rows of the largest off-diagonal entry never
# exceeds 1.2e-8; the largest single entry is 0.71 in the terms test and 0.31, 0.068, 4.9e-3 in the chained tests of
# `dense1`, `tanh8`, `relu88`; 21 of the 36 chained steps have none above 1e-6:
# tests/test_fsvi_dispatch_table.py::test_the_older_step_tests_have_an_identity_gram).  They test the step's other terms at
# the smallest shapes; k_fsvi_gram, and every loop of the step past its first trip, is tested by
# tests/test_gpu_fsvi_matrix.py on the lattice inputs of tests/fsvi_cases.py.
class Run:
    """A plan, the device state of one FSVI run and the injected draws of its steps."""

    def __init__(self, eng, name, k, B, rows=9, seed=0):
        self.spec = fc.specs()[name]
        self.k, self.B = k, B
        self.x, self.y, mu, W = fc.make_problem(self.spec, rows, B, k, seed)
        self.plan = eng.MLPPlan(eng.MLPSpec(self.spec.dims, self.spec.acts, "mse"), max_batch=2 * B, max_particles=k)
        self.D, self.F = self.spec.n_params, self.spec.dims[0]
        self.mu, self.W = dev(mu), dev(W)
        self.m, self.v = torch.zeros(self.D, device="cuda"), torch.zeros(self.D, device="cuda")
        self.loss = torch.zeros(1, device="cuda")
        self.xd, self.yd = dev(self.x), dev(self.y)
        self.lo, self.hi = dev(self.x.min(axis=0)), dev(self.x.max(axis=0))
        self.rng = np.random.default_rng(seed + 100)

    def draws(self):
        xm = self.rng.uniform(-30, 30, size=(self.B, self.F)).astype(np.float32)
        z = (0.1 * self.rng.normal(size=(self.k, self.F))).astype(np.float32)
        eps = self.rng.normal(size=(self.k, self.D)).astype(np.float32)
        return xm, z, eps

    def step(self, t, idx, lr=0.05, seed=5, draws=None):
        xm, z, eps = draws if draws is not None else (None, None, None)
        return self.plan.fsvi_step(self.mu, self.W, self.m, self.v, self.xd, self.yd, self.B, lr, t, seed, self.loss,
                                   lo=self.lo, hi=self.hi, xm=None if xm is None else dev(xm),
                                   noise=None if z is None else dev(z), eps=None if eps is None else dev(eps),
                                   want_terms=True, batch=len(idx), row_idx=dev(idx, torch.int32))


def test_terms_with_injected_draws(eng):
    """xp bit for bit; alpha against a NumPy solve on the device's own f (float32 noise in f is amplified by |K^-1| and
    is not what this checks); the Stein term on the same float32 weights; f against the float64 forward."""
    run = Run(eng, "tanh8", k=3, B=6, seed=3)
    idx = np.array([7, 2, 5, 0, 8, 3], np.int32)
    W0 = host(run.W).copy()
    xm, z, eps = run.draws()
    got = run.step(1, idx, draws=(xm, z, eps))
    run.plan.check_finite()
    xp = host(got["xp"])
    np.testing.assert_array_equal(xp, fc.make_xp(run.x[idx], xm, z))
    f = host(got["f"]).astype(np.float64)
    for i in range(3):
        K = fc.gram(xp[i])
        assert np.linalg.cond(K) <= 1e3
        close(host(got["alpha"])[i], fc.gp_alpha(K, f[i]), 1e-9, f"alpha of particle {i}")
        close(host(got["stein"])[i], fc.stein_c2(W0[i]), 1e-6, f"c2 of particle {i}")
    ref = fc.terms(W0, run.x[idx], run.y[idx], xm, z, run.spec, run.B)
    close(f, ref["f"], 1e-4, "f")
    np.testing.assert_array_equal(host(run.W), host(run.mu)[None, :] + eps)     # the redraw: one float32 add


@pytest.mark.parametrize("b", ["full", "ragged"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", ["dense1", "tanh8", "relu88"])
def test_gradient_and_update_over_three_chained_steps(eng, name, k, b):
    """g against the float64 restatement at 1e-4 of its largest magnitude, on inputs whose cond(K_i) <= 1e3 (asserted from
    the device's xp: otherwise the comparison would measure the GP prior's conditioning); mu, m, v against legacy Adam
    applied to the DEVICE's g in float32; every step starts from the device's previous state."""
    B = 5
    run = Run(eng, name, k=k, B=B, seed=sum(map(ord, name)) + k)
    lr = 0.05
    for t in (1, 2, 3):
        idx = run.rng.permutation(len(run.x))[:B if b == "full" else 1].astype(np.int32)
        mu0, m0, v0, W0 = (host(a).copy() for a in (run.mu, run.m, run.v, run.W))
        xm, z, eps = run.draws()
        got = run.step(t, idx, lr=lr, draws=(xm, z, eps))
        xp = host(got["xp"])
        conds = [np.linalg.cond(fc.gram(xp[i])) for i in range(k)]
        assert max(conds) <= 1e3, conds
        ref = fc.terms(W0, run.x[idx], run.y[idx], xm, z, run.spec, B)
        np.testing.assert_array_equal(xp, ref["xp"])
        g = host(got["grad"])
        close(g, ref["g"], 1e-4, f"{name} k={k} {b} t={t}: g")
        close(host(run.loss), [ref["loss"]], 1e-4, f"{name} k={k} {b} t={t}: loss")
        mu1, m1, v1 = fc.adam32(mu0, g, m0, v0, t, lr)
        close(host(run.mu), mu1, 1e-6, "mu")
        close(host(run.m), m1, 1e-6, "m")
        close(host(run.v), v1, 1e-6, "v")
        np.testing.assert_array_equal(host(run.W), host(run.mu)[None, :] + eps)
    run.plan.check_finite()


def test_philox_draws_are_the_oracle_stream(eng):
    """No injected draws: the step equals the injected step fed with oracle.philox draws of stream 9 at steps 4 t, 4 t + 1,
    4 t + 2.  The device's float32 Box-Muller differs from the oracle's by at most 3.2e-5 per normal (tests/test_gpu_bsam.py)."""
    assert _lib.STREAM_FSVI == 9
    k, B, t, seed = 3, 5, 6, 4242
    idx = np.array([1, 4, 6, 0, 2], np.int32)

    def one(t, injected):
        run = Run(eng, "tanh8", k=k, B=B, seed=8)
        draws = None
        if injected:
            draws = (fc.draw_xm(seed, t, B, run.F, host(run.lo), host(run.hi)), fc.draw_noise(seed, t, k, run.F),
                     fc.draw_eps(seed, t, k, run.D))
        got = run.step(t, idx, seed=seed, draws=draws)
        run.plan.check_finite()
        return {"xp": host(got["xp"]), "g": host(got["grad"]), "mu": host(run.mu), "W": host(run.W), "loss": host(run.loss)}

    own, inj = one(t, False), one(t, True)
    for key in own:
        close(own[key], inj[key], 1e-4, f"Philox against injected oracle draws: {key}")
    again = one(t, False)
    assert all(np.array_equal(own[key], again[key]) for key in own), "same (seed, t): same step"
    other = one(t + 1, False)
    assert np.abs(other["xp"] - own["xp"]).max() > 1.0 and np.abs(other["W"] - own["W"]).max() > 0.1


def test_argument_errors_on_a_plan(eng):
    spec = eng.MLPSpec((2, 8, 2), ("relu", "linear"), "mse")
    plan = eng.MLPPlan(spec, max_batch=8, max_particles=2)
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(_lib.PyzError) as e:
        plan.fsvi_step(z(plan.D), z(2, plan.D), z(plan.D), z(plan.D), z(6, 2), z(6, 2), 4, 0.1, 1, 0, z(1), lo=z(2), hi=z(2),
                       batch=4)
    assert e.value.code == -1 and "one unit" in str(e.value)


# ---------------------------------------------------------------- the class
LINE_JSON = sequential_json(1, [1], ["linear"])


def _line_dataset():
    rng = np.random.default_rng(0)
    x = rng.uniform(-3, 3, size=(200, 1)).astype(np.float32)
    return Dataset((x, (2 * x + 2).astype(np.float32)), MeanSquaredError, "Regression", target_dim=1, seed=3)


def test_class_fits_a_line(gpu_device):
    opt = FSVI()
    opt.compile(HyperParameters(batch_size=32, lr=0.05, k=4), LINE_JSON, _line_dataset(), verbose=False,
                prior=GaussianPrior(0.0, 1.0), function_prior="GP", seed=17)
    losses = [float(opt.step()) for _ in range(50)]
    opt._plan.check_finite()
    assert np.isfinite(losses).all()
    assert np.mean(losses[-10:]) < 0.5 * np.mean(losses[:10]), (losses[:10], losses[-10:])
    ensemble = opt.result()
    assert len(ensemble) == 4 and ensemble.predict(np.zeros((3, 1), np.float32)).shape == (3, 1)
    W = host(opt._weights)
    np.testing.assert_array_equal(ensemble[2].weights_flat, W[2])
    bm = opt.posterior()
    assert isinstance(bm, BayesianModel)
    samples, pred = bm.predict(np.linspace(-1, 1, 5, dtype=np.float32).reshape(-1, 1), 3)
    assert len(samples) == 3 and np.isfinite(np.asarray(pred)).all()
    assert opt._step == 50 and opt._plan.workspace_bytes > 0


@pytest.mark.parametrize("missing", ["prior", "function_prior"])
def test_class_needs_both_priors(gpu_device, missing):
    kwargs = dict(prior=GaussianPrior(0.0, 1.0), function_prior="GP")
    del kwargs[missing]
    with pytest.raises(KeyError):
        FSVI().compile(HyperParameters(batch_size=32, lr=0.05, k=4), LINE_JSON, _line_dataset(), verbose=False, **kwargs)

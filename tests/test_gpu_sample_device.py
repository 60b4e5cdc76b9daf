"""Device draws of the two result distributions that used to be drawn on the host: k_sample_lowrank_rows (SWAG's
MultivariateNormalDiagPlusLowRank) against its formula in float64 on the device's own noise, bit for bit across
blockings of the rows over calls, with z1 and z2 on separate counters; k_gather_rows (HMC's Sampled) bit for bit; then
both through BayesianModel.sample_weights_device / predict with the host ``sample_n`` made to raise."""

import ctypes as C
import random
from math import sqrt

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import mlp as o_mlp  # noqa: E402
from oracle import predict as o_predict  # noqa: E402

from bayesian_inference_for_nn_amd import _lib, engine, synth  # noqa: E402
from bayesian_inference_for_nn_amd.datasets import Dataset  # noqa: E402
from bayesian_inference_for_nn_amd.distributions import GaussianPrior, MultivariateNormalDiagPlusLowRank, Sampled, tfd  # noqa: E402
from bayesian_inference_for_nn_amd.losses import SparseCategoricalCrossentropy  # noqa: E402
from bayesian_inference_for_nn_amd.nn import BayesianModel, sequential_json  # noqa: E402
from bayesian_inference_for_nn_amd.optimizers import HMC  # noqa: E402
from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters  # noqa: E402

SENT = -777.0
SEED, FIRST = 0x1234567812345, 11
MAX_K = _lib.LOWRANK_MAX_K
ROWS_PER_WG = 8            # PYZ_LOWRANK_ROWS of csrc/pyz_kernels.h: 37 rows are four full row blocks and one of five


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_device):
    return gpu_device


@pytest.fixture(autouse=True)
def _device_path(monkeypatch):
    monkeypatch.delenv("PYZ_SAMPLE_DEVICE", raising=False)
    monkeypatch.delenv("PYZ_SAMPLED_BANK_MAX", raising=False)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def inputs(length, k, seed=0):
    rng = np.random.default_rng([seed, length, k])
    mean = (rng.normal(size=length) * 0.3).astype(np.float32)
    diag = (rng.normal(size=length) * 0.05).astype(np.float32)            # (a scale "as written": signs and all)
    d = (rng.normal(size=(k, length)) * 0.1).astype(np.float32)
    return mean, diag, d


def noise(length, k, n_rows, first=FIRST):
    """(z1 (n_rows, len), z2 (n_rows, k)) float32: the device's own stream, element e and element 4 ceil(len / 4) + c."""
    n4 = 4 * ((length + 3) // 4)
    z = torch.empty((n_rows, n4 + k), dtype=torch.float32, device="cuda")
    for r in range(n_rows):
        engine.fill_normal(z[r], SEED, _lib.STREAM_PREDICT, first + r)
    z = z.cpu().numpy()
    return z[:, :length], z[:, n4:]


def draw(length, col0, k, n_rows, mean, diag, d, factor, first=FIRST, splits=None):
    stride = col0 + length + 5
    out = torch.full((n_rows, stride), SENT, dtype=torch.float32, device="cuda")
    md, dd, vd = dev(mean), dev(diag), dev(d)
    r0 = 0
    for n in (splits or [n_rows]):
        engine.sample_lowrank_rows(out[r0:r0 + n], col0, md, dd, vd, factor, SEED, first + r0)
        r0 += n
    assert r0 == n_rows
    return out.cpu().numpy()


# (len, col0, k, n_rows): the issue's lengths, offsets, ranks and row counts -- len = 1; an unaligned col0 with len % 4 =
# 1, 2 and 3; k at the cap; 37 rows (> 8 per workgroup, not a multiple); more than one 1024-column tile (1027, 4099) --
# and lengths that are multiples of four (1028, 4100), the only ones whose rows of dev take the 16-byte loads; with
# row_stride = col0 + len + 5 odd, consecutive rows of out then start 16-, 4-, 8- and 4-byte aligned: every store form.
LOWRANK_CASES = [(1, 0, 2, 1), (1, 3, 3, 3), (5, 3, 20, 3), (5, 0, 2, 37), (42, 3, 3, 37), (42, 0, 20, 1), (1027, 3, 2, 3),
                 (1027, 0, MAX_K, 3), (4099, 0, 20, 37), (4099, 3, 3, 1), (4099, 3, MAX_K, 37),
                 (1028, 0, 20, 37), (1028, 3, 2, 3), (4100, 3, 3, 37), (4100, 0, MAX_K, 9), (8, 0, 1, 3)]


@pytest.mark.parametrize("length,col0,k,n_rows", LOWRANK_CASES, ids=lambda v: str(v))
def test_lowrank_rows_match_the_formula_on_the_device_noise(length, col0, k, n_rows):
    """|got - ref| <= (k + 4) 2^-24 (|mean| + |diag z1| + factor sum_c |dev[c] z2[c]|): the float32 rounding of k + 2
    multiply-adds and two adds, around the float64 value of the formula.  (k = 1 is the kernel's alone -- the Python
    side never gets there -- with a factor of its own.)"""
    mean, diag, d = inputs(length, k)
    factor = float(np.float32(sqrt(1 / (2 * (k - 1))) if k > 1 else 0.75))
    z1, z2 = noise(length, k, n_rows)
    got = draw(length, col0, k, n_rows, mean, diag, d, factor)
    m64, g64, d64, a, b = mean.astype(np.float64), diag.astype(np.float64), d.astype(np.float64), z1.astype(np.float64), \
        z2.astype(np.float64)
    ref = m64[None, :] + g64[None, :] * a + factor * (b @ d64)
    bound = (k + 4) * 2.0 ** -24 * (np.abs(m64)[None, :] + np.abs(g64[None, :] * a) + factor * (np.abs(b) @ np.abs(d64)))
    err = np.abs(got[:, col0:col0 + length].astype(np.float64) - ref)
    print(f"len {length} col0 {col0} k {k} rows {n_rows}: max err / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), f"worst element at {float((err / bound).max()):.3f} of its bound"
    outside = np.ones(got.shape[1], dtype=bool)
    outside[col0:col0 + length] = False
    assert (got[:, outside].view(np.uint32) == np.float32(SENT).view(np.uint32)).all()      # the other columns keep their bits


@pytest.mark.parametrize("length,col0,k", [(1027, 3, 20), (1028, 0, 3), (42, 3, MAX_K)], ids=lambda v: str(v))
def test_lowrank_rows_do_not_depend_on_how_the_rows_are_cut_into_calls(length, col0, k):
    mean, diag, d = inputs(length, k, seed=1)
    factor = sqrt(1 / (2 * (k - 1)))
    whole = draw(length, col0, k, 37, mean, diag, d, factor)
    parts = draw(length, col0, k, 37, mean, diag, d, factor, splits=[5, 1, 31])
    assert np.array_equal(whole.view(np.uint32), parts.view(np.uint32))
    assert not np.array_equal(whole[0], whole[1])


def test_z1_and_z2_are_separate_elements_of_the_stream():
    length, k, n_rows = 42, 2, 3
    factor = np.float32(sqrt(1 / (2 * (k - 1))))
    z1, z2 = noise(length, k, n_rows)
    zero, one = np.zeros(length, np.float32), np.ones(length, np.float32)
    # diag = 0, dev = 1: every element of row r is factor * (z2_0 + z2_1), in float32 as the kernel's chain rounds it
    low = draw(length, 0, k, n_rows, zero, zero, np.ones((k, length), np.float32), float(factor))[:, :length]
    want = factor * (z2[:, 0] + z2[:, 1])
    assert want.dtype == np.float32
    assert np.array_equal(low.view(np.uint32), np.repeat(want[:, None], length, axis=1).view(np.uint32))
    # dev = 0, diag = 1: z1, the bits fill_normal gives for the same counter
    diag_only = draw(length, 0, k, n_rows, zero, one, np.zeros((k, length), np.float32), float(factor))[:, :length]
    assert np.array_equal(diag_only.view(np.uint32), z1.view(np.uint32))
    assert not np.isin(z2, z1).any() and not np.isin(want, diag_only).any()              # z2 is no element of z1
    for r in range(n_rows - 1):
        assert not np.array_equal(diag_only[r], diag_only[r + 1]) and low[r, 0] != low[r + 1, 0]


GATHER_IDX = [8, 0, 3, 3, 0, 8, 5, 8, 1]


@pytest.mark.parametrize("length", [1, 42, 1027, 1028])
@pytest.mark.parametrize("col0", [0, 3])
def test_gather_rows_copies_the_indexed_rows_bit_for_bit(length, col0):
    """(1028: rows of the bank and every fourth row of out are 16-byte aligned, the wide path; the others: the scalar one.)"""
    rng = np.random.default_rng([length, col0])
    bank = rng.normal(size=(9, length)).astype(np.float32)
    bank.view(np.uint32)[0, 0] = 0x7FC01234                                               # a NaN payload travels as bits
    out = torch.full((len(GATHER_IDX), col0 + length + 5), SENT, dtype=torch.float32, device="cuda")
    bank_d = dev(bank)
    engine.gather_rows(out, col0, bank_d, GATHER_IDX)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, col0:col0 + length].view(np.uint32), bank[GATHER_IDX].view(np.uint32))
    outside = np.ones(got.shape[1], dtype=bool)
    outside[col0:col0 + length] = False
    assert (got[:, outside] == np.float32(SENT)).all()
    for bad in ([9] + GATHER_IDX[1:], [-1] + GATHER_IDX[1:]):
        with pytest.raises(IndexError):
            engine.gather_rows(out, col0, bank_d, bad)
    with pytest.raises(ValueError):
        engine.gather_rows(out, col0, bank_d, GATHER_IDX[:-1])
    # the kernel itself (the wrapper out of the way): a row whose index is out of range is not written
    out.fill_(SENT)
    idx_d = torch.tensor([2, 9, -1, 7], dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().pyz_gather_rows(_lib.ptr(out), 4, out.shape[1], col0, length, _lib.ptr(bank_d), 9, _lib.ptr(idx_d),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    got = out.cpu().numpy()
    assert np.array_equal(got[[0, 3], col0:col0 + length].view(np.uint32), bank[[2, 7]].view(np.uint32))
    assert (got[[1, 2]] == np.float32(SENT)).all() and (got[4:] == np.float32(SENT)).all()


CFG = sequential_json(6, [40, 3], ["relu", "softmax"])
SPEC = o_mlp.MLPSpec((6, 40, 3), ("relu", "softmax"), "scce")


def _raise(*a, **k):
    raise AssertionError("the host sample_n was called")


def test_swag_posteriors_are_drawn_on_the_device(monkeypatch):
    bm = BayesianModel(CFG)
    rng = np.random.default_rng(1)
    k, factor = 3, sqrt(1 / (2 * (3 - 1)))
    parts = []
    for layer, sl in enumerate(bm._model.spec.layer_slices()):
        n = sl.stop - sl.start
        mean = (rng.normal(size=n) * 0.3).astype(np.float32)
        diag = np.full(n, 0.05, np.float32)
        D = (rng.normal(size=(n, k)) * 0.04).astype(np.float32)
        bm.apply_distribution(MultivariateNormalDiagPlusLowRank(mean, diag, D), layer, layer)
        parts.append((sl, mean, diag, D))
    monkeypatch.setattr(MultivariateNormalDiagPlusLowRank, "sample_n", _raise)
    tfd.seed(7)
    with engine.KernelProbe(16) as kp:
        Wd = bm.sample_weights_device(4000)
    assert [name for name, _ in kp.launches] == ["k_sample_lowrank_rows"] * 2
    W = Wd.cpu().numpy()
    for sl, mean, diag, D in parts:
        np.testing.assert_allclose(W[:, sl].mean(0), mean, atol=0.005)
        np.testing.assert_allclose(W[:, sl].std(0), np.sqrt(diag.astype(np.float64) ** 2 + factor ** 2 * (D.astype(np.float64) ** 2).sum(1)),
                                   rtol=0.08)
        # the low-rank part is SHARED by the columns of a draw: cov = diag(diag^2) + factor^2 D D^T.  An entry of the
        # empirical covariance of n draws has variance (s_ii s_jj + s_ij^2) / n; six of its standard deviations
        cov = np.diag(diag.astype(np.float64) ** 2) + factor ** 2 * D.astype(np.float64) @ D.astype(np.float64).T
        sd = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / len(W))
        assert (np.abs(np.cov(W[:, sl].astype(np.float64), rowvar=False) - cov) <= 6 * sd).all()
        assert np.abs(cov - np.diag(np.diag(cov))).max() > 20 * sd.max()                  # (and there is something to see)
    assert not np.array_equal(W[0], W[1])
    tfd.seed(7)
    assert np.array_equal(bm.sample_weights_device(4000).cpu().numpy().view(np.uint32), W.view(np.uint32))
    x = rng.normal(size=(50, 6)).astype(np.float32)
    tfd.seed(7)
    W16 = bm.sample_weights_device(16).cpu().numpy()
    tfd.seed(7)
    samples, mean = bm.predict(x, nb_samples=16)          # the same 16 draws
    rs, rm = o_predict.predict(W16, x, SPEC)
    np.testing.assert_allclose(np.stack(samples), rs, atol=1e-5)
    np.testing.assert_allclose(mean, rm, atol=1e-5)


def _sampled_model():
    rng = np.random.default_rng(2)
    samples = [(rng.normal(size=SPEC.n_params) * 0.3).astype(np.float32) for _ in range(7)]
    dist = Sampled(samples, [1, 2, 1, 5, 1, 1, 3])
    bm = BayesianModel(CFG)
    bm.apply_distribution(dist, 0, 1)
    return bm, dist


def test_sampled_posteriors_are_gathered_on_the_device(monkeypatch):
    bm, dist = _sampled_model()
    random.seed(3)
    want = bm.sample_weights_matrix(50)
    assert len({w.tobytes() for w in want}) > 3
    with monkeypatch.context() as mp:
        mp.setattr(Sampled, "sample_n", _raise)
        random.seed(3)
        with engine.KernelProbe(16) as kp:
            got = bm.sample_weights_device(50)
        assert [name for name, _ in kp.launches] == ["k_gather_rows"]
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
        bank = dist._bank
        assert tuple(bank.shape) == (7, SPEC.n_params) and bank.is_cuda
        random.seed(3)
        assert np.array_equal(bm.sample_weights_device(50).cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert dist._bank is bank                                                        # uploaded once
    # the bank cap sends a fresh distribution down the host path: the same matrix, nothing uploaded
    monkeypatch.setenv("PYZ_SAMPLED_BANK_MAX", "1")
    bm2, dist2 = _sampled_model()
    random.seed(3)
    with engine.KernelProbe(16) as kp:
        host = bm2.sample_weights_device(50)
    assert kp.launches == [] and getattr(dist2, "_bank", None) is None
    assert np.array_equal(host.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # a replaced sample_weights_matrix defines the draws, as it did when Sampled was drawn on the host
    monkeypatch.delenv("PYZ_SAMPLED_BANK_MAX")
    bm.sample_weights_matrix = lambda n: want[:n][::-1]
    with engine.KernelProbe(16) as kp:
        fixed = bm.sample_weights_device(50)
    assert kp.launches == [] and np.array_equal(fixed.cpu().numpy(), want[::-1])


def test_hmc_result_predicts_without_the_host_draws(monkeypatch):
    x, y = synth.moons(500, seed=42)
    ds = Dataset((x, y), SparseCategoricalCrossentropy, "Classification", seed=3)
    random.seed(0)
    opt = HMC()
    opt.compile(HyperParameters(epsilon=0.002, m=0.5, L=8), sequential_json(2, [50, 2], ["relu", "softmax"]), ds, verbose=False,
                prior=GaussianPrior(0.0, 1.0), seed=5)
    opt.train(12)
    bm = opt.result()
    monkeypatch.setattr(Sampled, "sample_n", _raise)
    xt, _ = next(iter(ds.test_data.batch(ds.test_size)))
    samples, mean = bm.predict(xt, nb_samples=20)
    assert len(samples) == 20
    np.testing.assert_allclose(mean.sum(axis=1), 1.0, atol=1e-5)
    stored = np.stack(bm._distributions[0]._samples)
    assert any(np.array_equal(bm._model.weights_flat, s) for s in stored)                # the last draw is a stored sample

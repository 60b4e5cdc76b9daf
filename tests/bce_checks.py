"""Float64 restatement of BinaryCrossentropy on a last layer of ONE sigmoid unit, for the tests (a plain module), built on
oracle.mlp.forward without editing the oracle (oracle.mlp.MLPSpec knows "scce" and "mse" only).

DESIGN A7: Keras caches the logit z of a sigmoid-activated Dense and BinaryCrossentropy(from_logits=False) evaluates from it:

    row loss = max(z, 0) - z y + log1p(exp(-|z|)),    delta_L = (sigmoid(z) - y) / batch,    loss = batch mean,

with targets y in [0, 1], one per row, and sigmoid(z) as the model's output.  Away from saturation this is the clipped form
-[y log p + (1 - y) log(1 - p)] with p in [1e-7, 1 - 1e-7] (`keras_clipped`).

`Spec` is the duck-typed model description the shared checks take (head_cases.close_blocks, ...).  `install` lets the
oracle's own step functions, and the test helpers written on top of oracle.mlp, run a BCE model unchanged: for the length of
one test it puts dispatching versions of loss_and_grad / loss_value where those modules look them up.  There are no
tolerances here: the tests use head_cases.close_blocks, 1e-4 relative for losses, and the rules of step_cases, run_cases and
hmc_cases as they stand."""

from __future__ import annotations

import importlib
from typing import List, NamedTuple, Tuple

import numpy as np

from oracle import mlp as o_mlp


class Spec(NamedTuple):
    """dims = [in, h1, ..., 1]; acts[-1] = "sigmoid"; the interface of oracle.mlp.MLPSpec."""
    dims: Tuple[int, ...]
    acts: Tuple[str, ...]
    loss: str = "bce"

    @property
    def n_layers(self) -> int:
        return len(self.acts)

    @property
    def n_params(self) -> int:
        return sum((i + 1) * o for i, o in zip(self.dims[:-1], self.dims[1:]))

    def offsets(self) -> List[Tuple[int, int]]:
        out, off = [], 0
        for i, o in zip(self.dims[:-1], self.dims[1:]):
            out.append((off, off + i * o))
            off += (i + 1) * o
        return out

    def layer_slices(self) -> List[slice]:
        out, off = [], 0
        for i, o in zip(self.dims[:-1], self.dims[1:]):
            out.append(slice(off, off + (i + 1) * o))
            off += (i + 1) * o
        return out


def spec(dims, acts) -> Spec:
    s = Spec(tuple(dims), tuple(acts))
    assert s.dims[-1] == 1 and s.acts[-1] == "sigmoid" and len(s.dims) == len(s.acts) + 1
    return s


# ---------------------------------------------------------------- the restatement
def row_losses(z, y):
    """max(z, 0) - z y + log1p(exp(-|z|)) per row, in the dtype of z."""
    z = np.asarray(z).reshape(-1)
    y = np.asarray(y, dtype=z.dtype).reshape(-1)
    return np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))


def sigmoid(z):
    """Without overflow on either side, in the dtype of z."""
    z = np.asarray(z)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1 / (1 + e), e / (1 + e)).astype(z.dtype)


def keras_clipped(p, y):
    """The batch mean of -[y log p + (1 - y) log(1 - p)] with p clipped to [1e-7, 1 - 1e-7] (float64)."""
    p = np.clip(np.asarray(p, dtype=np.float64).reshape(-1), 1e-7, 1 - 1e-7)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    return float(-(y * np.log(p) + (1 - y) * np.log(1 - p)).mean())


def loss_value(out, logits, y, spec_=None):
    """The signature of oracle.mlp.loss_value; `out` is not used: the loss comes from the logits."""
    return row_losses(logits, y).mean()


def backward(theta, acts, delta, spec_, dtype=np.float64):
    """The flat gradient from the last layer's delta: the loop of oracle.mlp.loss_and_grad."""
    grads = [None] * spec_.n_layers
    ws = o_mlp.unpack(theta, spec_)
    for l in range(spec_.n_layers - 1, -1, -1):
        h_in = acts[l]
        grads[l] = (h_in.T @ delta, delta.sum(axis=0))
        if l > 0:
            delta = (delta @ ws[l][0].T) * o_mlp._act_grad_from_output(h_in, spec_.acts[l - 1])
    return o_mlp.pack(grads).astype(dtype), delta


def loss_and_grad(theta, x, y, spec_, dtype=np.float64):
    """(mean loss, d loss / d theta as a flat vector, model output sigmoid(z)): oracle.mlp.loss_and_grad for BCE."""
    assert spec_.dims[-1] == 1 and spec_.acts[-1] == "sigmoid", "BCE is restated for one sigmoid output only"
    theta = np.asarray(theta, dtype=dtype)
    acts, z = o_mlp.forward(theta, x, spec_, dtype)
    n = len(z)
    yt = np.asarray(y, dtype=dtype).reshape(n, 1)
    out = sigmoid(z)
    delta = (out - yt) / dtype(n)
    g, _ = backward(theta, acts, delta, spec_, dtype)
    return dtype(row_losses(z, yt).mean()), g, out


def input_grad(thetas, x, y, spec_, scale=1.0):
    """(G (n, in), losses (draws,)) float64: G = scale * sum over the draws of d (the draw's mean loss) / d x."""
    x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
    G, losses = np.zeros_like(x), []
    for theta in np.asarray(thetas, dtype=np.float64).reshape(-1, spec_.n_params):
        acts, z = o_mlp.forward(theta, x, spec_)
        yt = np.asarray(y, dtype=np.float64).reshape(len(x), 1)
        losses.append(float(row_losses(z, yt).mean()))
        _, delta0 = backward(theta, acts, (sigmoid(z) - yt) / len(x), spec_)
        G += delta0 @ o_mlp.unpack(theta, spec_)[0][0].T
    return scale * G, np.asarray(losses)


# ---------------------------------------------------------------- the oracle's step functions on a BCE model
ORACLE_MODULES = ("sgd", "sgld", "swag", "bbb", "hmc", "svgd")


def install(monkeypatch):
    """For one test: oracle.mlp.MLPSpec accepts loss "bce", and oracle.mlp.loss_and_grad / loss_value -- as attributes of
    oracle.mlp (where step_cases, hmc_cases, adam_checks and bsam_checks look them up) and as the names imported into
    oracle.sgd, sgld, swag, bbb, hmc and svgd -- hand a BCE spec to this module and everything else to the originals."""
    orig_lag, orig_lv = o_mlp.loss_and_grad, o_mlp.loss_value

    def lag(theta, x, y, spec_, dtype=np.float64):
        return (loss_and_grad if spec_.loss == "bce" else orig_lag)(theta, x, y, spec_, dtype)

    def lv(out, logits, y, spec_):
        return (loss_value if spec_.loss == "bce" else orig_lv)(out, logits, y, spec_)

    monkeypatch.setattr(o_mlp, "LOSSES", tuple(o_mlp.LOSSES) + ("bce",))
    for mod in [o_mlp] + [importlib.import_module(f"oracle.{m}") for m in ORACLE_MODULES]:
        for name, fn in (("loss_and_grad", lag), ("loss_value", lv)):
            if hasattr(mod, name):
                monkeypatch.setattr(mod, name, fn)


# ---------------------------------------------------------------- the head cases
class Case(NamedTuple):
    name: str
    dims: tuple
    acts: tuple
    P: int = 1
    batch: int = 64
    gathered: bool = False
    extra: dict = {}         # logits: scale the last layer so that max |z| over the batch is this; x_offset, repeat: head_cases

    @property
    def spec(self) -> Spec:
        return spec(self.dims, self.acts)


def _c(name, dims, hidden, P=1, batch=64, gathered=False, **extra):
    return Case(name, tuple(dims), tuple(hidden) + ("sigmoid",), P, batch, gathered, extra)


SAT = {"logits": 150.0}      # float32 exp overflows past 88.7: log(1 + exp(z)) and -log(1 - p) are inf there

HEAD_CASES = [
    # ---- k_head_rows<UT, 4, 1> at both ends of every UT bucket
    _c("rows_1x4_lo", (9, 1, 1), ("tanh",), batch=37),
    _c("rows_1x4_hi", (16, 64, 1), ("relu",), P=2, batch=50, gathered=True),
    _c("rows_4x4_lo", (12, 65, 1), ("relu",)),
    _c("rows_4x4_hi", (16, 256, 1), ("tanh",), batch=80),
    _c("rows_8x4_lo", (12, 257, 1), ("tanh",), batch=52),
    _c("rows_8x4_hi", (16, 512, 1), ("relu",)),
    _c("rows_16x4_lo", (12, 513, 1), ("relu",), batch=47),
    _c("rows_16x4_hi", (16, 1024, 1), ("tanh",), gathered=True),
    # ---- k_head_rows<1, 4, 4>: P * batch = 32768, the first product that gives a wave four rows
    _c("rw4_edge", (12, 50, 1), ("relu",), P=64, batch=512, gathered=True),
    # ---- k_head
    _c("head_k1100", (12, 1100, 1), ("sigmoid",), batch=70),
    _c("head_k1152", (16, 1152, 1), ("linear",)),
    # ---- one layer, three layers, small and odd batches, unaligned x, repeated rows
    _c("l1_gathered", (20, 1), (), P=2, batch=83, gathered=True),
    _c("l3", (12, 40, 30, 1), ("relu", "tanh"), batch=75),
    _c("rows_batch1", (12, 40, 1), ("tanh",), batch=1),
    _c("rows_batch31", (12, 40, 1), ("tanh",), batch=31),
    _c("rows_batch33", (12, 40, 1), ("tanh",), batch=33),
    _c("head_batch1", (12, 1100, 1), ("tanh",), batch=1),
    _c("head_batch31", (12, 1100, 1), ("tanh",), batch=31),
    _c("head_batch33", (12, 1100, 1), ("tanh",), batch=33),
    _c("rows_xoff", (16, 256, 1), ("tanh",), batch=96, x_offset=True),
    _c("rows_repeat", (8, 64, 1), ("tanh",), P=2, batch=45, gathered=True, repeat=True),
    # ---- saturated, one per kernel family
    _c("rows_saturated", (12, 40, 1), ("tanh",), batch=70, **SAT),
    _c("head_saturated", (12, 1100, 1), ("tanh",), batch=70, **SAT),
]
HEAD_CASE_BY_NAME = {c.name: c for c in HEAD_CASES}
assert len(HEAD_CASE_BY_NAME) == len(HEAD_CASES), "case names must be unique"


def case_data(case: Case):
    """Seeded like head_cases.case_data: (x rows, targets (rows, 1) float32, row_idx or None, thetas (P, D)).  Targets: a
    third 0, a third 1, a third uniform in (0, 1).  A `logits` case scales each particle's last layer so that max |z| over
    the batch is that value, and then makes sure of the rows the case is about: the row with the largest logit gets
    target 0 and the one with the smallest target 1 (both past 88 in magnitude: asserted)."""
    sp = case.spec
    rng = np.random.default_rng(sum(map(ord, "bce_" + case.name)))
    n_rows = case.batch + case.batch // 5 + 3 if case.gathered else case.batch
    x = rng.normal(size=(n_rows, sp.dims[0])).astype(np.float32)
    kind = rng.integers(0, 3, size=n_rows)
    y = np.where(kind == 0, 0.0, np.where(kind == 1, 1.0, rng.uniform(0.0, 1.0, size=n_rows))).astype(np.float32).reshape(-1, 1)
    idx = None
    if case.gathered:
        idx = rng.permutation(n_rows)[:case.batch].astype(np.int32)
        if case.extra.get("repeat"):
            idx = rng.integers(0, n_rows, size=case.batch).astype(np.int32)
            idx[1::7] = idx[0]
    thetas = np.empty((case.P, sp.n_params), dtype=np.float32)
    for p in range(case.P):
        parts = []
        for fan_in, fan_out in zip(sp.dims[:-1], sp.dims[1:]):
            parts.append(rng.normal(size=fan_in * fan_out) * (1.5 / np.sqrt(fan_in)))
            parts.append(rng.normal(size=fan_out) * 0.2)
        thetas[p] = np.concatenate(parts).astype(np.float32)
    big = case.extra.get("logits")
    if big:
        assert case.P == 1 and idx is None
        ko, _ = sp.offsets()[-1]
        _, z = o_mlp.forward(thetas[0], x, sp)
        thetas[0, ko:] = (thetas[0, ko:].astype(np.float64) * (big / np.abs(z).max())).astype(np.float32)
        _, z = o_mlp.forward(thetas[0], x, sp)
        z = z.reshape(-1)
        y[int(z.argmax()), 0], y[int(z.argmin()), 0] = 0.0, 1.0
        assert np.any((z > 88.0) & (y[:, 0] == 0.0)) and np.any((z < -88.0) & (y[:, 0] == 1.0)), (z.min(), z.max())
    return x, y, idx, thetas


# ---------------------------------------------------------------- wrong heads (tests/test_bce_host.py: each must be seen)
def _with_delta(theta, x, y, spec_, delta_of):
    theta = np.asarray(theta, dtype=np.float64)
    acts, z = o_mlp.forward(theta, x, spec_)
    yt = np.asarray(y, dtype=np.float64).reshape(len(z), 1)
    return backward(theta, acts, delta_of(z, sigmoid(z), yt, len(z)), spec_)[0]


def grad_mse_on_sigmoid(theta, x, y, spec_):
    """The gradient of MeanSquaredError on the sigmoid output: an extra 2 sigmoid'(z)."""
    return _with_delta(theta, x, y, spec_, lambda z, p, yt, n: 2.0 * (p - yt) * p * (1.0 - p) / n)


def grad_without_batch_mean(theta, x, y, spec_):
    return _with_delta(theta, x, y, spec_, lambda z, p, yt, n: p - yt)


def loss_from_clipped_probabilities(theta, x, y, spec_):
    _, z = o_mlp.forward(np.asarray(theta, dtype=np.float64), x, spec_)
    return keras_clipped(sigmoid(z), y)


def loss_log1pexp_float32(theta, x, y, spec_):
    """max-free log(1 + exp(z)) - z y in float32: inf past z = 88.7."""
    _, z = o_mlp.forward(np.asarray(theta, dtype=np.float64), x, spec_)
    z = z.reshape(-1).astype(np.float32)
    with np.errstate(over="ignore"):
        return float((np.log(np.float32(1) + np.exp(z)) - z * np.asarray(y, dtype=np.float32).reshape(-1)).mean())

"""The float64 restatement of a conv net (Conv2D / MaxPooling2D stem, Flatten, Dense stack), the cases the conv tests share
and their comparisons (a plain module).

Written in NumPy from the definitions, not from the kernels:

  Conv2D      z[b, oy, ox, n] = bias[n] + sum_{i, j, c} xpad[b, oy + i, ox + j, c] W[i, j, c, n], stride 1; `same` pads k - 1
              zeros per axis, (k - 1) // 2 of them on top / left (TensorFlow's rule: an even kernel pads more on the
              bottom / right); h = act(z).
  MaxPooling  windows of (ph, pw) at stride (ph, pw), floor(H / ph) rows: the remainder is dropped and gets no gradient; the
              winner is the first maximum in row-then-column scan order of the window.
  Flatten     of the (h, w, c) map, row-major (channels last).
  flat order  per Conv2D the kernel (kh, kw, cin, cout) row-major then the bias, then per Dense the kernel (in, out), bias.
  losses      SparseCategoricalCrossentropy on a softmax last layer / MeanSquaredError, mean over the batch.

WRONG names restatements that are wrong in one way each; tests/test_conv_host.py shows that the comparisons used on the
GPU tell each of them from the right one.  torch-CPU autograd pins the right one there (this module does not use torch).

The last section restates the host rules that launch the conv kernels (waves per tile, rows per weight-gradient range,
the chunk walk, the tile counts) and names, in LAUNCH_CELLS, the paths they open; tests/test_conv_dispatch_table.py pins
both to the source and to the cases.
"""

from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

TOL = 1e-4          # of the reference block's largest magnitude, per layer block
MARGIN = 1e-5       # the generator keeps every ReLU pre-activation and every pool decision this far (of the layer's
#                     largest |z|) from a tie, so a float32 device takes the same branch as the float64 restatement

WRONG = ("kernel read as (cout, cin, kh, kw)", "extra same pad on top / left", "pool gradient to the last maximum",
         "remainder row pooled", "conv bias gradient dropped", "Flatten in CHW order", "act' of the wrong layer after a pool",
         "labels not gathered by row_idx", "no act' between two adjacent convs", "data gradient cropped at the bottom / right pad")
# the last two apply to none of A-T (wrong_applies): until H and I no case had a conv directly on a conv, or a data gradient
# through a padded conv


# ---------------------------------------------------------------- the cases
@dataclass(frozen=True)
class ConvCase:
    name: str
    shape: tuple             # (h, w, c)
    stem: tuple              # ("conv", filters, (kh, kw), padding, act) | ("pool", (ph, pw))
    units: tuple
    acts: tuple
    batches: tuple
    covers: str
    ties: bool = False       # channel 0 on three levels: pool windows tie exactly, which only the first-maximum rule resolves
    far_bias: float = 0.0    # > 0: conv biases of about this size, either sign -- with 135 168 ReLU pre-activations (F) a
    #                          centred draw has about five of them inside MARGIN whatever the seed; biases of 2.5 standard
    #                          deviations thin the density at zero a hundredfold and leave both ReLU branches in use

    @property
    def loss(self):
        return "scce" if self.acts[-1] == "softmax" else "mse"

    @property
    def ops(self):
        return tuple(("conv", op[1], op[2][0], op[2][1], op[3], op[4]) if op[0] == "conv" else ("pool", op[1][0], op[1][1])
                     for op in self.stem)

    def spec(self):
        from bayesian_inference_for_nn_amd.engine import ConvSpec, MLPSpec
        probe = ConvSpec(self.shape, self.ops, MLPSpec((1, 1), ("linear",), self.loss))
        return ConvSpec(self.shape, self.ops, MLPSpec((probe.features,) + tuple(self.units), tuple(self.acts), self.loss))

    def json(self):
        from bayesian_inference_for_nn_amd.nn.model import conv_sequential_json
        return conv_sequential_json(self.shape, self.stem, self.units, self.acts)


C3, P2 = (3, 3), (2, 2)
CASES = {c.name: c for c in (
    ConvCase("A", (7, 6, 3), (("conv", 5, C3, "same", "relu"),), (4,), ("softmax",), (1, 2, 33),
             "K = 27 + bias in one ragged k tile; 5 ragged columns; 42 B rows"),
    ConvCase("B", (6, 5, 5), (("conv", 33, (2, 3), "valid", "tanh"),), (3,), ("linear",), (7,),
             "even kernel; two column tiles, the second ragged; cin % 4 != 0"),
    ConvCase("C", (7, 6, 3), (("conv", 5, C3, "same", "relu"), ("pool", P2), ("conv", 33, (2, 3), "valid", "tanh")), (4,),
             ("softmax",), (33,), "dgrad, pool_bwd + act', the dropped remainder row"),
    ConvCase("D", (8, 8, 8), (("conv", 32, C3, "valid", "sigmoid"), ("pool", P2)), (16, 10), ("relu", "linear"), (9,),
             "cin % 4 = 0; K = 72 over several k steps; one column tile; feature gradient through two Dense layers"),
    ConvCase("E", (7, 7, 2), (("conv", 4, (1, 1), "valid", "linear"), ("pool", (3, 3))), (2,), ("softmax",), (5,),
             "1 x 1 kernel; pool 3 with remainder 1"),
    ConvCase("F", (32, 32, 3), (("conv", 4, C3, "same", "relu"),), (3,), ("softmax",), (33,),
             "M = 33 792 rows: the weight-gradient reduction over several workgroups; Dense layer 0 with K = 4096", far_bias=2.5),
    # beyond the specified six: the two rules of assumption A9 that no case above can tell from their neighbours
    ConvCase("G", (5, 4, 2), (("conv", 3, (2, 2), "same", "tanh"),), (2,), ("linear",), (6,),
             "even kernel with same padding: the extra zero row / column is on the bottom / right"),
    ConvCase("T", (7, 7, 2), (("conv", 4, (1, 1), "valid", "linear"), ("pool", (3, 3))), (2,), ("softmax",), (5,),
             "exact ties inside pool windows: the first maximum wins", ties=True),
    # the launch paths no case above reaches (LAUNCH_CELLS below names the cell each of these is the only one to reach)
    ConvCase("H", (6, 5, 3), (("conv", 16, C3, "same", "tanh"), ("conv", 33, C3, "same", "relu")), (3,), ("softmax",), (7,),
             "a conv on a conv: dgrad times tanh' of the conv below, with pt = pl = 1; K = 144: 73 steps over four waves "
             "(19 / 18 / 18 / 18); 5 k tiles x 2 column tiles in the weight-gradient reduce, the second column tile ragged"),
    ConvCase("I", (5, 4, 2), (("conv", 3, (2, 2), "same", "relu"), ("conv", 4, (2, 2), "same", "tanh")), (2,), ("linear",), (6,),
             "dgrad through the asymmetric pad of an even same kernel (pt = pl = 0, the zeros at the bottom / right); relu' "
             "of the conv below"),
    ConvCase("J", (2, 23, 89), (("conv", 3, (2, 23), "valid", "tanh"),), (2,), ("softmax",), (33,),
             "K = 4094, the limit: KT = 4096, the full tap table, S = 4 forward, 128 k tiles in the reduce, a ragged second "
             "row tile"),
    ConvCase("K", (2, 3, 2), (("conv", 3, (5, 5), "same", "tanh"),), (2,), ("linear",), (5,),
             "a same kernel larger than its map: most taps of every row fall outside the image"),
)}
TABLE = ("A", "B", "C", "D", "E", "F")      # the six cases the feature was specified with
OLD = TABLE + ("G", "T")                     # the cases the feature shipped with
NEW = ("H", "I", "J", "K")
ALL = OLD + NEW
P_CASES = ("A", "C", "H")                    # also run with three particles
EXTRA_ROWS = 4                               # images of the data set outside every batch
PLAN_SLACK = 3                               # the GPU tests' plans have max_batch = batch + PLAN_SLACK


# ---------------------------------------------------------------- the restatement
def _act(z, a):
    if a == "relu":
        return np.where(z < 0, 0.0, z).astype(z.dtype)
    if a == "tanh":
        return np.tanh(z)
    if a == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    return z          # linear; softmax belongs to the loss / the read-out


def _act_grad(h, a):
    if a == "relu":
        return (h > 0).astype(h.dtype)
    if a == "tanh":
        return 1.0 - h * h
    if a == "sigmoid":
        return h * (1.0 - h)
    return np.ones_like(h)


def _pads(k, padding, wrong):
    if padding != "same":
        return 0, 0
    lo = (k - 1) // 2
    if wrong == "extra same pad on top / left":
        lo = (k - 1) - lo
    return lo, (k - 1) - lo


def unpack(spec, theta, wrong=None):
    """[(W, b)] per weight layer from the flat vector: conv kernels (kh, kw, cin, cout), Dense kernels (in, out)."""
    out = []
    for sl, (ks, bs) in zip(spec.layer_slices(), spec.variable_shapes()):
        blk = theta[sl]
        n = int(np.prod(ks))
        if len(ks) == 4 and wrong == "kernel read as (cout, cin, kh, kw)":
            W = blk[:n].reshape(ks[3], ks[2], ks[0], ks[1]).transpose(2, 3, 1, 0)
        else:
            W = blk[:n].reshape(ks)
        out.append((W, blk[n:]))
    return out


def _windows(xp, kh, kw):
    return np.lib.stride_tricks.sliding_window_view(xp, (kh, kw), axis=(1, 2))      # (B, OH, OW, C, kh, kw)


def _pool_view(h, ph, pw, wrong):
    """(B, OH, OW, C, ph * pw) windows in row-then-column scan order, and the rows / columns they cover."""
    B, H, W, C = h.shape
    OH, OW = H // ph, W // pw
    v = h[:, :OH * ph, :OW * pw].reshape(B, OH, ph, OW, pw, C).transpose(0, 1, 3, 5, 2, 4).reshape(B, OH, OW, C, ph * pw)
    return v, OH, OW


def forward(spec, theta, x, wrong=None):
    """Every op's pre-activation and output, the features, the Dense layers' and the model output (softmax applied).
    theta (D,), x (B, h * w * c); everything in theta's dtype."""
    dt = theta.dtype
    B = len(x)
    h = np.asarray(x, dtype=dt).reshape((B,) + tuple(spec.input_shape))
    Wb = unpack(spec, theta, wrong)
    tape, wi = [], 0
    for op in spec.ops:
        if op[0] == "conv":
            _, f, kh, kw, padding, act = op
            W, b = Wb[wi]
            wi += 1
            (pt, pb), (pl, pr) = _pads(kh, padding, wrong), _pads(kw, padding, wrong)
            xp = np.pad(h, ((0, 0), (pt, pb), (pl, pr), (0, 0)))
            z = np.einsum("byxcij,ijcn->byxn", _windows(xp, kh, kw), W) + b
            out = _act(z, act)
            tape.append(dict(kind="conv", x=h, xp=xp, z=z, h=out, W=W, pads=(pt, pl), pads_br=(pb, pr), act=act, k=(kh, kw)))
            h = out
        else:
            _, ph, pw = op
            H, Wd = h.shape[1:3]
            src = h
            if wrong == "remainder row pooled" and (H % ph or Wd % pw):
                # the last window of each axis swallows the remainder: pad with -inf to whole windows and fold the extra one in
                OH, OW = H // ph, Wd // pw
                out = np.empty((B, OH, OW, h.shape[3]), dtype=dt)
                for oy in range(OH):
                    y1 = H if oy == OH - 1 else (oy + 1) * ph
                    for ox in range(OW):
                        x1 = Wd if ox == OW - 1 else (ox + 1) * pw
                        out[:, oy, ox] = h[:, oy * ph:y1, ox * pw:x1].max(axis=(1, 2))
                tape.append(dict(kind="pool_wrong", x=src, h=out, p=(ph, pw)))
                h = out
                continue
            v, OH, OW = _pool_view(h, ph, pw, wrong)
            if wrong == "pool gradient to the last maximum":
                win = v.shape[-1] - 1 - np.argmax(v[..., ::-1], axis=-1)
            else:
                win = np.argmax(v, axis=-1)               # the first maximum
            out = np.take_along_axis(v, win[..., None], axis=-1)[..., 0]
            tape.append(dict(kind="pool", x=src, h=out, win=win, p=(ph, pw)))
            h = out
    feat = h.transpose(0, 3, 1, 2).reshape(B, -1) if wrong == "Flatten in CHW order" else h.reshape(B, -1)
    a, dense = feat, []
    for (W, b), act in zip(Wb[wi:], spec.acts):
        z = a @ W + b
        out = z if act == "softmax" else _act(z, act)
        dense.append(dict(x=a, z=z, h=out, W=W, act=act))
        a = out
    y = a
    if spec.acts[-1] == "softmax":
        e = np.exp(a - a.max(axis=1, keepdims=True))
        y = e / e.sum(axis=1, keepdims=True)
    return dict(tape=tape, dense=dense, features=feat, out=y, map_shape=h.shape)


def loss_grad(spec, theta, x, y, wrong=None):
    """(loss, grad (D,), features (B, F), out (B, C)) of the batch x, y in theta's dtype."""
    dt = theta.dtype
    f = forward(spec, theta, x, wrong)
    B = len(x)
    last = f["dense"][-1]
    if spec.loss == "scce":
        z = last["z"]
        y = np.asarray(y).astype(np.int64).reshape(-1)
        mx = z.max(axis=1, keepdims=True)
        lse = (mx + np.log(np.exp(z - mx).sum(axis=1, keepdims=True)))[:, 0]
        loss = float(np.mean(lse - z[np.arange(B), y]))
        d = f["out"].copy()
        d[np.arange(B), y] -= 1.0
        d /= B
    else:
        o = last["h"]
        t = np.asarray(y, dtype=dt).reshape(o.shape)
        loss = float(np.mean(np.mean((o - t) ** 2, axis=1)))
        d = 2.0 * (o - t) / (B * o.shape[1]) * _act_grad(o, last["act"])
    blocks = []
    for li in range(len(f["dense"]) - 1, -1, -1):
        L = f["dense"][li]
        blocks.append(np.concatenate([(L["x"].T @ d).reshape(-1), d.sum(axis=0)]))
        d = d @ L["W"].T
        if li > 0:
            d = d * _act_grad(f["dense"][li - 1]["h"], f["dense"][li - 1]["act"])
    grad = np.concatenate([stem_grad(f, d, wrong, spec.acts[0])] + blocks[::-1]).astype(dt)
    assert grad.shape == theta.shape
    return loss, grad, f["features"], f["out"]


def stem_grad(f, dfeat, wrong=None, above_act="linear"):
    """The stem's block of the gradient (every conv's kernel then bias, in network order) from f = forward(...) and
    dfeat (B, F) = d loss / d features.  above_act: the activation of the first Dense layer (one WRONG reads it)."""
    dt = dfeat.dtype
    B = len(dfeat)
    ms = f["map_shape"]
    d = dfeat.reshape(B, ms[3], ms[1], ms[2]).transpose(0, 2, 3, 1) if wrong == "Flatten in CHW order" else dfeat.reshape(ms)
    tape = f["tape"]
    blocks = []
    for ti in range(len(tape) - 1, -1, -1):
        t = tape[ti]
        if t["kind"] == "conv":
            if ti == len(tape) - 1 or (tape[ti + 1]["kind"] == "conv" and wrong != "no act' between two adjacent convs"):
                d = d * _act_grad(t["h"], t["act"])        # (below a pool, the pool's backward has applied it)
            kh, kw = t["k"]
            dW = np.einsum("byxcij,byxn->ijcn", _windows(t["xp"], kh, kw), d)
            db = np.zeros_like(d.sum(axis=(0, 1, 2))) if wrong == "conv bias gradient dropped" else d.sum(axis=(0, 1, 2))
            blocks.append(np.concatenate([dW.reshape(-1), db]))
            if ti > 0:
                OH, OW = d.shape[1:3]
                dxp = np.zeros_like(t["xp"])
                for i in range(kh):
                    for j in range(kw):
                        dxp[:, i:i + OH, j:j + OW, :] += d @ t["W"][i, j].T
                pt, pl = t["pads_br"] if wrong == "data gradient cropped at the bottom / right pad" else t["pads"]
                H, Wd = t["x"].shape[1:3]
                d = dxp[:, pt:pt + H, pl:pl + Wd, :]
            above_act = t["act"]
        else:
            ph, pw = t["p"]
            below = tape[ti - 1]
            src = t["x"]
            dx = np.zeros_like(src)
            if t["kind"] == "pool_wrong":
                B_, H, Wd, C = src.shape
                OH, OW = d.shape[1:3]
                for oy in range(OH):
                    y1 = H if oy == OH - 1 else (oy + 1) * ph
                    for ox in range(OW):
                        x1 = Wd if ox == OW - 1 else (ox + 1) * pw
                        blk = src[:, oy * ph:y1, ox * pw:x1].reshape(B_, -1, C)
                        w = np.argmax(blk, axis=1)
                        g = np.zeros_like(blk)
                        np.put_along_axis(g, w[:, None, :], d[:, oy, ox][:, None, :], axis=1)
                        dx[:, oy * ph:y1, ox * pw:x1] = g.reshape(B_, y1 - oy * ph, x1 - ox * pw, C)
            else:
                B_, OH, OW, C = d.shape
                g = np.zeros((B_, OH, OW, C, ph * pw), dtype=dt)
                np.put_along_axis(g, t["win"][..., None], d[..., None], axis=-1)
                dx[:, :OH * ph, :OW * pw] = g.reshape(B_, OH, OW, C, ph, pw).transpose(0, 1, 4, 2, 5, 3).reshape(
                    B_, OH * ph, OW * pw, C)
            act = below["act"]
            if wrong == "act' of the wrong layer after a pool":
                act = "linear" if above_act == "softmax" else above_act
            d = dx * _act_grad(below["h"], act)
    return np.concatenate(blocks[::-1]).astype(dt)


def wrong_applies(case: ConvCase, wrong: str, gathered: bool = True) -> bool:
    convs = [op for op in case.stem if op[0] == "conv"]
    pools = [i for i, op in enumerate(case.stem) if op[0] == "pool"]
    if wrong == "kernel read as (cout, cin, kh, kw)" or wrong == "conv bias gradient dropped":
        return True
    if wrong == "extra same pad on top / left":
        return any(op[3] == "same" and (op[2][0] % 2 == 0 or op[2][1] % 2 == 0) for op in convs)
    if wrong == "pool gradient to the last maximum":
        return bool(pools) and case.ties
    if wrong == "remainder row pooled":
        shapes = case.spec().op_shapes()
        return any(shapes[i][0][0] % case.stem[i][1][0] or shapes[i][0][1] % case.stem[i][1][1] for i in pools)
    if wrong == "Flatten in CHW order":
        o = case.spec().op_shapes()[-1][1]
        return o[2] > 1 and o[0] * o[1] > 1
    if wrong == "act' of the wrong layer after a pool":
        for i in pools:
            above = case.stem[i + 1][4] if i + 1 < len(case.stem) else case.acts[0]
            above = "linear" if above == "softmax" else above
            if above != case.stem[i - 1][4]:
                return True
        return False
    if wrong == "labels not gathered by row_idx":
        return gathered
    if wrong == "no act' between two adjacent convs":       # (a linear conv below has act' = 1: nothing to skip)
        return any(a[0] == "conv" and b[0] == "conv" and a[4] != "linear" for a, b in zip(case.stem, case.stem[1:]))
    if wrong == "data gradient cropped at the bottom / right pad":      # a conv with something below it and unequal pads
        return any(op[0] == "conv" and op[3] == "same" and (op[2][0] % 2 == 0 or op[2][1] % 2 == 0) for op in case.stem[1:])
    raise KeyError(wrong)


# ---------------------------------------------------------------- data
@dataclass
class ConvData:
    case: ConvCase
    batch: int
    x: np.ndarray            # float32 (batch + EXTRA_ROWS, h * w * c): the data set
    y: np.ndarray            # int32 (rows,) labels or float32 (rows, out) targets
    idx: np.ndarray          # int32 (batch,): the batch's rows of the data set, not in order
    theta: np.ndarray        # float32 (3, D): three particles (the margins hold for all three in P_CASES, else for the first)
    margin: float            # the smallest distance from a tie the generator found (of the layer's largest |z|)
    seed: int


def _margins(spec, theta, x, ties):
    """The smallest distance of a ReLU pre-activation from zero and of a pool decision from a tie, each as a fraction of
    its layer's largest |z| (float64).  A pool window whose maximum is an exact post-ReLU zero is no decision: relu' kills
    the gradient whichever tie wins.  ties: exactly equal leaders are no decision either (the rule under test decides)."""
    f = forward(spec, theta.astype(np.float64), x.astype(np.float64))
    worst = np.inf
    for ti, t in enumerate(f["tape"]):
        if t["kind"] == "conv" and t["act"] == "relu":
            worst = min(worst, np.abs(t["z"]).min() / np.abs(t["z"]).max())
        if t["kind"] == "pool":
            below = f["tape"][ti - 1]
            v, _, _ = _pool_view(t["x"], t["p"][0], t["p"][1], None)
            s = np.sort(v, axis=-1)
            gap = (s[..., -1] - s[..., -2]) / np.abs(below["z"]).max()
            dead = (s[..., -1] == 0.0) if below["act"] == "relu" else np.zeros(gap.shape, dtype=bool)
            if ties:
                dead = dead | (s[..., -1] == s[..., -2])
            if (~dead).any():
                worst = min(worst, gap[~dead].min())
    for L in f["dense"]:
        if L["act"] == "relu":
            worst = min(worst, np.abs(L["z"]).min() / np.abs(L["z"]).max())
    return float(worst)


def _draw(case: ConvCase, batch: int, seed: int):
    spec = case.spec()
    rng = np.random.default_rng([seed, batch] + [ord(ch) for ch in case.name])
    rows = batch + EXTRA_ROWS
    n_in = int(np.prod(case.shape))
    if case.ties:      # channel 0 on three levels, the others continuous (and unseen by the conv: see below)
        x = rng.normal(size=(rows,) + tuple(case.shape)).astype(np.float32)
        x[..., 0] = rng.integers(0, 3, size=x.shape[:-1])
        x = x.reshape(rows, n_in)
    else:
        x = rng.normal(size=(rows, n_in)).astype(np.float32)
    C = case.units[-1]
    y = rng.integers(0, C, size=rows).astype(np.int32) if case.loss == "scce" else rng.normal(size=(rows, C)).astype(np.float32)
    idx = rng.permutation(rows)[:batch].astype(np.int32)
    theta = np.empty((3, spec.n_params), dtype=np.float32)
    for p in range(3):
        for sl, (ks, bs) in zip(spec.layer_slices(), spec.variable_shapes()):
            n, fan_in = int(np.prod(ks)), int(np.prod(ks[:-1]))
            theta[p, sl.start:sl.start + n] = rng.normal(size=n) / np.sqrt(fan_in)
            theta[p, sl.start + n:sl.stop] = 0.3 * rng.normal(size=bs[0])
            if case.ties and len(ks) == 4:
                # the conv reads channel 0 alone, so positions with equal pixels there tie exactly in its output while their
                # other channels differ: where the pool sends its gradient shows in the kernel's gradient for those channels
                theta[p, sl.start:sl.start + n].reshape(ks)[:, :, 1:, :] = 0.0
            if case.far_bias and len(ks) == 4:
                theta[p, sl.start + n:sl.stop] = case.far_bias * np.sign(rng.normal(size=bs[0])) * (1 + 0.1 * rng.normal(size=bs[0]))
    return spec, x, y, idx, theta


@lru_cache(maxsize=None)
def make(name: str, batch: int) -> ConvData:
    """The data of (case, batch): the generator walks seeds until every particle keeps MARGIN (both conditions of
    _margins), and asserts it."""
    case = CASES[name]
    for seed in range(64):
        spec, x, y, idx, theta = _draw(case, batch, seed)
        m = min(_margins(spec, theta[p], x[idx], case.ties) for p in range(3 if name in P_CASES else 1))
        # ... and the batch's labels differ from the first `batch` labels of the data set (a step that forgets the gather shows)
        if m > MARGIN and not np.array_equal(y[:batch], y[idx]):
            break
    assert m > MARGIN and not np.array_equal(y[:batch], y[idx]), (name, batch, m)
    for a in (x, y, idx, theta):
        a.setflags(write=False)
    return ConvData(case, batch, x, y, idx, theta, m, seed)


@lru_cache(maxsize=None)
def reference(name: str, batch: int, p: int = 0):
    """(loss, grad, features, out) in float64 of particle p on the batch's rows (computed once, shared, read-only)."""
    d = make(name, batch)
    loss, grad, feat, out = loss_grad(d.case.spec(), d.theta[p].astype(np.float64), d.x[d.idx].astype(np.float64), d.y[d.idx])
    for a in (grad, feat, out):
        a.setflags(write=False)
    return loss, grad, feat, out


# ---------------------------------------------------------------- comparisons
def block_errors(got, ref, spec):
    """{block: max |got - ref| / max |ref|} over the kernel and the bias of every weight layer."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    out = {}
    for li, (sl, (ks, bs)) in enumerate(zip(spec.layer_slices(), spec.variable_shapes())):
        n = int(np.prod(ks))
        for nm, a, b in ((f"W{li}", got[sl.start:sl.start + n], ref[sl.start:sl.start + n]),
                         (f"b{li}", got[sl.start + n:sl.stop], ref[sl.start + n:sl.stop])):
            scale = np.abs(b).max()
            out[nm] = float(np.abs(a - b).max() / scale) if scale > 0 else float(np.abs(a - b).max())
    return out


def rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = np.abs(ref).max()
    return float(np.abs(got - ref).max() / scale) if scale > 0 else float(np.abs(got - ref).max())   # (an all-zero reference: exact)


def errors(got_loss, got_grad, got_feat, ref, spec):
    """Every checked quantity's error as a fraction of its reference scale: features, loss, each gradient block."""
    loss, grad, feat, _ = ref
    e = {"features": rel(got_feat, feat), "loss": abs(float(got_loss) - loss) / abs(loss)}
    e.update(block_errors(got_grad, grad, spec))
    return e


def assert_close(e: dict, what: str, tol: float = TOL):
    print(what, {k: f"{v:.2e}" for k, v in e.items()})
    bad = {k: v for k, v in e.items() if not v <= tol}
    assert not bad, f"{what}: beyond {tol:g} of the reference scale: {bad}"


# ---------------------------------------------------------------- the toy task of the end-to-end training test
TOY = ConvCase("toy", (8, 8, 1), (("conv", 4, C3, "same", "relu"), ("pool", P2)), (2,), ("softmax",), (32,),
               "two classes of 8 x 8 x 1 images: the bright half on the left or on the right")
TOY_HP = dict(n=256, batch_size=32, lr=0.02, k=5, frequency=1, scale=1.0, steps=200)


def toy_data(seed: int = 0):
    """(x (n, 8, 8, 1) float32, y (n,) int32): half the image at 1, the other at 0, plus noise of 0.1."""
    rng = np.random.default_rng(seed)
    n = TOY_HP["n"]
    y = rng.integers(0, 2, size=n).astype(np.int32)
    x = 0.1 * rng.normal(size=(n, 8, 8, 1))
    for i in range(n):
        x[i, :, 4 * y[i]:4 * y[i] + 4, 0] += 1.0
    return x.astype(np.float32), y


def toy_training_losses(seed: int = 0):
    """(mean loss of the first 20 steps, of the last 20) of TOY_HP['steps'] SGD steps of the float64 restatement: shuffled
    epochs of batches, Glorot start (SWAG's weights follow plain SGD steps; its moments do not feed back)."""
    from bayesian_inference_for_nn_amd.nn.model import model_from_json
    spec = TOY.spec()
    x, y = toy_data(seed)
    x = x.reshape(len(x), -1).astype(np.float64)
    rng = np.random.default_rng(seed + 1)
    net = model_from_json(TOY.json())
    net.reset_glorot(rng)
    theta = net.weights_flat.astype(np.float64)
    losses, perm, pos = [], None, 0
    for _ in range(TOY_HP["steps"]):
        if perm is None or pos >= len(x):
            perm, pos = rng.permutation(len(x)), 0
        rows = perm[pos:pos + TOY_HP["batch_size"]]
        pos += TOY_HP["batch_size"]
        loss, grad, _, _ = loss_grad(spec, theta, x[rows], y[rows])
        theta = theta - TOY_HP["lr"] * grad
        losses.append(loss)
    return float(np.mean(losses[:20])), float(np.mean(losses[-20:]))


# ---------------------------------------------------------------- the learning rate of the chained steps
STEP_LRS = tuple(round(0.25 * 0.9 ** k, 4) for k in range(24))      # 0.25 down to 0.022


@lru_cache(maxsize=None)
def step_lr(name: str, batch: int, n_steps: int = 3) -> float:
    """The learning rate of the step tests of (case, batch): the largest of STEP_LRS for which the float64 chain of n_steps
    SGD steps from particle 0 keeps every state it computes a gradient at 1.5 MARGIN from a tie (the device's chain follows
    it to float32 rounding, and the test re-asserts MARGIN on the device's own states) and gives every kernel and bias
    block a gradient that is not zero (a dead ReLU layer would leave a step that checks nothing)."""
    d = make(name, batch)
    spec = d.case.spec()
    xb, yb = d.x[d.idx].astype(np.float64), d.y[d.idx]
    for lr in STEP_LRS:
        theta, ok = d.theta[0].astype(np.float64), True
        for k in range(n_steps):
            if k > 0 and not _margins(spec, theta, xb, d.case.ties) > 1.5 * MARGIN:
                ok = False
                break
            _, grad, _, _ = loss_grad(spec, theta, xb, yb)
            if not all(v > 0 for v in block_scales(grad, spec).values()):
                ok = False
                break
            theta = theta - lr * grad
        if ok:
            return lr
    raise AssertionError(f"{name} batch {batch}: no learning rate of {STEP_LRS} keeps the chained states off the ties")


def block_scales(vec, spec):
    """{block: max |vec|} over the kernel and the bias of every weight layer."""
    out = {}
    for li, (sl, (ks, bs)) in enumerate(zip(spec.layer_slices(), spec.variable_shapes())):
        n = int(np.prod(ks))
        out[f"W{li}"] = float(np.abs(vec[sl.start:sl.start + n]).max())
        out[f"b{li}"] = float(np.abs(vec[sl.start + n:sl.stop]).max())
    return out


def margin_of(name: str, batch: int, theta) -> float:
    """_margins of the case's batch at the weights theta (float64)."""
    d = make(name, batch)
    return _margins(d.case.spec(), np.asarray(theta, dtype=np.float64), d.x[d.idx].astype(np.float64), d.case.ties)


# ---------------------------------------------------------------- the launch rules, restated (pyz_api.hip / pyz_conv.h)
# tests/test_conv_dispatch_table.py compares each of these with the source text; the probe reports kernel names only, so
# this arithmetic is what ties a case to the path it takes.
CONV_WAVES, WGRAD_CHUNK, CONV_MAX_K, CONV_MAX_ROWS = 4, 512, 4094, 1 << 24


def cdiv(a, b):
    return -(-a // b)


def conv_waves(tiles, steps):
    S = 1
    while S < CONV_WAVES and tiles * S < 1024 and steps >= 16 * S:
        S *= 2
    return S


def rows_per_range(max_batch, OH, OW):
    m_max = max_batch * OH * OW
    return max(256, ((m_max + 255) // 256 + 1) // 2 * 2)


def wave_steps(steps, S):
    """The steps of each of the S waves: wave w takes steps w, w + S, ..."""
    return [(steps - w + S - 1) // S for w in range(S)]


def chunk_walk(M, rows_per_g):
    """[[rows of each chunk] per range] of k_conv_wgrad's walk over M rows."""
    out = []
    for m0 in range(0, M, rows_per_g):
        m1 = min(M, m0 + rows_per_g)
        out.append([min(WGRAD_CHUNK, m1 - c0) for c0 in range(m0, m1, WGRAD_CHUNK)])
    return out


@dataclass(frozen=True)
class ConvLaunch:
    """What the launch code derives for one conv layer of a plan at one batch (one particle unless P is given)."""
    layer: int               # index among the ops
    M: int
    K: int
    KT: int
    fwd_tiles: int           # k_conv_fwd: row tiles x column tiles
    fwd_S: int
    fwd_steps: tuple         # per wave
    k_tiles: int             # k_conv_wgrad / the reduce: tiles over the K + 1 rows of [dW; db]
    n_tiles: int
    rows_per_g: int
    G: int
    wgrad_S: int
    chunks: tuple            # chunk_walk
    reduce_blocks: int
    dgrad: bool              # k_conv_dgrad is launched (something is below)
    below: bool              # ... with the conv below's output for act'
    pads: tuple              # (pt, pb, pl, pr)
    kernel: tuple
    in_map: tuple            # (H, W, C)
    out_map: tuple           # (OH, OW, N)
    fwd_lds: int
    wgrad_lds: int


def conv_launches(shape, ops, batch, max_batch, P=1):
    """[ConvLaunch] per conv op of the stem `ops` (ConvCase.ops form) on a plan of max_batch at `batch`."""
    h, w, c = shape
    out = []
    for o, op in enumerate(ops):
        if op[0] == "pool":
            h, w = h // op[1], w // op[2]
            continue
        _, n, kh, kw, padding, _ = op
        (pt, pb), (pl, pr) = _pads(kh, padding, None), _pads(kw, padding, None)
        OH, OW = h + pt + pb - kh + 1, w + pl + pr - kw + 1
        K = kh * kw * c
        KT = (K + 2) & ~1
        M = batch * OH * OW
        n_tiles, k_tiles = cdiv(n, 32), cdiv(K + 1, 32)
        fwd_tiles = cdiv(M, 32) * n_tiles
        fwd_S = conv_waves(fwd_tiles * P, KT // 2)
        rpg = rows_per_range(max_batch, OH, OW)
        G = cdiv(M, rpg)
        wg_S = conv_waves(k_tiles * n_tiles * G * P, min(M, rpg) // 2)
        out.append(ConvLaunch(o, M, K, KT, fwd_tiles, fwd_S, tuple(wave_steps(KT // 2, fwd_S)), k_tiles, n_tiles, rpg, G, wg_S,
                              tuple(tuple(r) for r in chunk_walk(M, rpg)), cdiv((K + 1) * n, 16), o > 0,
                              o > 0 and ops[o - 1][0] == "conv", (pt, pb, pl, pr), (kh, kw), (h, w, c), (OH, OW, n),
                              KT * 8 + (fwd_S * 4096 if fwd_S > 1 else 0), (wg_S * 4096 if wg_S > 1 else 0) + WGRAD_CHUNK * 16))
        h, w, c = OH, OW, n
    return out


# the dedicated shapes of tests/test_gpu_conv_paths.py: name -> (input, stem, units, acts, max_batch, batches)
PATH_SHAPES = {
    "a1": ((32, 32, 1), (("conv", 2, C3, "same", "tanh"),), (3,), ("softmax",), 130, (5, 130)),
    "a2": ((33, 33, 1), (("conv", 2, C3, "valid", "tanh"),), (3,), ("softmax",), 200, (3,)),
    "b": ((63, 65, 1), (("conv", 2, C3, "same", "tanh"),), (2,), ("linear",), 4097, (4097,)),
}


def path_case(name):
    shape, stem, units, acts, max_batch, batches = PATH_SHAPES[name]
    return ConvCase(name, shape, stem, units, acts, batches, "a dedicated shape of tests/test_gpu_conv_paths.py"), max_batch


LAUNCH_CELLS = frozenset(
    [f"fwd S = {s}" for s in (1, 2, 4)] + [f"wgrad S = {s}" for s in (1, 2, 4)] +
    ["k tiles > 1", "column tiles > 1", "k tiles > 1 and column tiles > 1", "G = 1", "1 < G <= 16", "G > 16",
     "one chunk a range", "several chunks a range", "last chunk even", "last chunk odd", "last chunk of at most one step a wave",
     "several chunks a range where OW < W", "dgrad with below", "dgrad without below", "dgrad pad 0", "dgrad pad symmetric",
     "dgrad pad asymmetric", "kernel larger than the map", "K = PYZ_CONV_MAX_K", "the last image ends at PYZ_CONV_MAX_ROWS"])
# the cell each new case and each dedicated shape is the only one to reach (asserted by tests/test_conv_dispatch_table.py)
OWNED = {"H": "k tiles > 1 and column tiles > 1", "I": "dgrad pad asymmetric", "J": "K = PYZ_CONV_MAX_K",
         "K": "kernel larger than the map", "a1": "last chunk of at most one step a wave",
         "a2": "several chunks a range where OW < W", "b": "the last image ends at PYZ_CONV_MAX_ROWS"}


def launch_cells(L: ConvLaunch):
    """The cells of LAUNCH_CELLS one conv layer at one batch reaches.  The three `last chunk` cells speak of the last chunk
    of a range of several chunks: of a single chunk `rows` is all there is, and every case of the table has one."""
    cells = {f"fwd S = {L.fwd_S}", f"wgrad S = {L.wgrad_S}"}
    if L.k_tiles > 1:
        cells.add("k tiles > 1")
    if L.n_tiles > 1:
        cells.add("column tiles > 1")
    if L.k_tiles > 1 and L.n_tiles > 1:
        cells.add("k tiles > 1 and column tiles > 1")
    cells.add("G = 1" if L.G == 1 else "1 < G <= 16" if L.G <= 16 else "G > 16")
    for r in L.chunks:
        if len(r) == 1:
            cells.add("one chunk a range")
            continue
        cells.add("several chunks a range")
        cells.add("last chunk odd" if r[-1] % 2 else "last chunk even")
        if r[-1] <= 2 * L.wgrad_S:
            cells.add("last chunk of at most one step a wave")
        if L.out_map[1] < L.in_map[1]:      # the window's corner is then no linear function of the row number
            cells.add("several chunks a range where OW < W")
    if L.dgrad:
        pt, pb, pl, pr = L.pads
        cells.add("dgrad with below" if L.below else "dgrad without below")
        cells.add("dgrad pad 0" if not any(L.pads) else "dgrad pad symmetric" if (pt, pl) == (pb, pr) else "dgrad pad asymmetric")
    if L.kernel[0] > L.in_map[0] or L.kernel[1] > L.in_map[1]:
        cells.add("kernel larger than the map")
    if L.K == CONV_MAX_K:
        cells.add("K = PYZ_CONV_MAX_K")
    if L.M > CONV_MAX_ROWS - L.out_map[0] * L.out_map[1]:
        cells.add("the last image ends at PYZ_CONV_MAX_ROWS")
    return cells


def reached_cells(name):
    """The cells a case of CASES (at its batches, on the GPU tests' plan of batch + PLAN_SLACK) or a dedicated shape reaches."""
    if name in PATH_SHAPES:
        case, max_batch = path_case(name)
        runs = [(b, max_batch) for b in case.batches]
    else:
        case = CASES[name]
        runs = [(b, b + PLAN_SLACK) for b in case.batches]
    cells = set()
    for b, mb in runs:
        for L in conv_launches(case.shape, case.ops, b, mb):
            cells |= launch_cells(L)
    return cells

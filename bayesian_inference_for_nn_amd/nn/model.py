"""Keras-2.15 Sequential JSON -> Dense stack, and a small Keras-like model object.

The reference hands its model to every optimizer as ``model.to_json()``
(``Pyesian/optimizers/Optimizer.py:43`` ``model_config: str``; format fixture
``static/models/sl/dense1.json``) and rebuilds it with
``tf.keras.models.model_from_json`` (``SGLD.py:137``, ``HMC.py:56``, ``BBB.py:256``,
``SVGD.py:222``, ``nn/BayesianModel.py:18``).  TensorFlow is not part of this backend,
so the JSON is parsed here: ``Sequential`` of ``InputLayer`` / ``Flatten`` / ``Dense``.
"""

from __future__ import annotations

import json
from typing import List, Optional, Sequence

import numpy as np

from ..engine import MLPSpec

_ACTS = {"linear", "relu", "tanh", "sigmoid", "softmax"}


class Array(np.ndarray):
    """ndarray with the ``.numpy()`` accessor the reference scripts call on TF tensors."""

    def __new__(cls, a):
        return np.asarray(a).view(cls)

    def numpy(self):
        return np.asarray(self)


class Layer:
    def __init__(self, class_name: str, config: dict, in_dim: Optional[int], out_dim: Optional[int]):
        self.class_name, self.config = class_name, config
        self.name = config.get("name", class_name.lower())
        self.in_dim, self.out_dim = in_dim, out_dim
        self._model = None
        self._dense_index = None        # index among the Dense layers

    @property
    def trainable_variables(self) -> List[np.ndarray]:
        """[kernel (in, out), bias (out)] views of the model's flat weight vector."""
        if self._dense_index is None:
            return []
        sl = self._model.spec.layer_slices()[self._dense_index]
        flat = self._model.weights_flat[sl]
        i, o = self.in_dim, self.out_dim
        return [flat[: i * o].reshape(i, o), flat[i * o:]]

    @property
    def trainable_weights(self):
        return self.trainable_variables


def _activation_name(a) -> str:
    if isinstance(a, dict):          # Keras may serialise a function object as {"class_name": ...}
        a = a.get("config", a.get("class_name", "linear"))
    a = str(a)
    if a not in _ACTS:
        raise ValueError(f"unsupported activation '{a}' (supported: {sorted(_ACTS)})")
    return a


class DenseNet:
    """The subset of ``tf.keras.Model`` the hot path and its callers touch: ``layers``,
    ``trainable_variables``, ``get_weights`` / ``set_weights``, ``to_json``, ``__call__`` /
    ``predict`` (evaluated by the HIP kernels)."""

    def __init__(self, model_config: str):
        cfg = json.loads(model_config) if isinstance(model_config, str) else model_config
        if cfg.get("class_name") != "Sequential":
            raise ValueError("only Keras Sequential models of InputLayer / Flatten / Dense are supported")
        self._config = cfg
        self.layers: List[Layer] = []
        dims, acts = [], []
        cur = None
        for lc in cfg["config"]["layers"]:
            cn, c = lc["class_name"], lc.get("config", {})
            shape = c.get("batch_input_shape") or (lc.get("build_config", {}) or {}).get("input_shape")
            if cur is None and shape is not None:
                cur = int(np.prod([d for d in shape[1:]]))
                self.input_shape = tuple(shape[1:])
            if cn == "InputLayer":
                continue                                  # not part of Sequential.layers
            if cn == "Flatten":
                self.layers.append(Layer(cn, c, cur, cur))
            elif cn == "Dense":
                if cur is None:
                    raise ValueError("the first layer needs an input shape")
                if not c.get("use_bias", True):
                    raise ValueError("Dense layers without bias are not supported")
                units = int(c["units"])
                layer = Layer(cn, c, cur, units)
                layer._dense_index = len(acts)
                if not dims:
                    dims.append(cur)
                dims.append(units)
                acts.append(_activation_name(c.get("activation", "linear")))
                self.layers.append(layer)
                cur = units
            else:
                raise ValueError(f"unsupported layer class '{cn}'")
        if not acts:
            raise ValueError("the model has no Dense layer")
        self.dims, self.acts = tuple(dims), tuple(acts)
        self.spec = MLPSpec(self.dims, self.acts, "scce" if acts[-1] == "softmax" else "mse")
        for l in self.layers:
            l._model = self
        self.weights_flat = np.zeros(self.spec.n_params, dtype=np.float32)
        self._plan = None
        self.reset_glorot(np.random.default_rng())

    # ------------------------------------------------------------------ weights
    def reset_glorot(self, rng: np.random.Generator):
        """Keras default of model_from_json: GlorotUniform kernels, zero biases (Appendix A6)."""
        off = 0
        for i, o in zip(self.dims[:-1], self.dims[1:]):
            lim = np.sqrt(6.0 / (i + o))
            self.weights_flat[off:off + i * o] = rng.uniform(-lim, lim, size=i * o).astype(np.float32)
            self.weights_flat[off + i * o:off + (i + 1) * o] = 0.0
            off += (i + 1) * o

    @property
    def trainable_variables(self) -> List[np.ndarray]:
        return [v for l in self.layers for v in l.trainable_variables]

    def get_weights(self) -> List[np.ndarray]:
        return [v.copy() for v in self.trainable_variables]

    def set_weights(self, weights: Sequence[np.ndarray]):
        tv = self.trainable_variables
        if len(weights) != len(tv):
            raise ValueError(f"expected {len(tv)} weight arrays, got {len(weights)}")
        for dst, src in zip(tv, weights):
            dst[...] = np.asarray(src, dtype=np.float32).reshape(dst.shape)

    def set_flat(self, flat):
        self.weights_flat[...] = np.asarray(flat, dtype=np.float32).reshape(-1)

    def to_json(self) -> str:
        return json.dumps(self._config)

    def count_params(self) -> int:
        return self.spec.n_params

    # ------------------------------------------------------------------ inference
    def _forward(self, x) -> np.ndarray:
        import torch
        from ..engine import MLPPlan
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(len(x), -1))
        if self._plan is None or self._plan.max_batch < len(x):
            self._plan = MLPPlan(self.spec, max_batch=max(len(x), 1))
        th = torch.as_tensor(self.weights_flat).cuda()
        out = self._plan.forward(th, torch.as_tensor(x).cuda())
        return out[0].cpu().numpy()

    def __call__(self, x, training=False):
        return Array(self._forward(x))

    def predict(self, x, verbose=0, batch_size=None):
        return np.asarray(self._forward(x))


class PolicyNet:
    """A Deep-PILCO policy network with at least one RBF hidden layer (Pyesian/dynamics/deep_pilco.py:28-51):
    h[n] = exp(-gamma * sum_k (x[k] - mean[k][n])^2), one trainable variable `mean` (in, units), no bias.

    ``hidden``: per hidden layer ``("rbf", units, gamma)`` or ``("dense", units, activation)``; a Dense output layer of
    ``out_units`` follows.  The flat vector keeps the layers in network order: an RBF layer's means row-major (in, units),
    a Dense layer's kernel (in, out) then its bias.  Initial weights are Keras': means uniform in [-0.05, 0.05)
    (``'uniform'``), Dense kernels Glorot, biases zero.

    This is what NNPolicy, BayesianDynamics and engine.PilcoPlan use of a network, nothing more: it is not an MLPSpec, no
    optimizer or BayesianModel takes it, and it has no Keras config (the reference's layer has no ``get_config`` either).
    ``__call__`` is the policy forward of the rollout kernels (pyz_pilco_act)."""

    def __init__(self, in_dim: int, hidden: Sequence[tuple], out_units: int, out_activation: str, rng=None):
        dims, acts, kinds, gammas = [int(in_dim)], [], [], []
        for kind, units, arg in hidden:
            if kind == "rbf":
                gamma = float(arg)
                if not (np.isfinite(gamma) and gamma > 0):
                    raise ValueError(f"RBF gamma must be a finite number > 0, not {arg!r}")
                acts.append("linear")
                gammas.append(gamma)
            elif kind == "dense":
                acts.append(_activation_name(arg))
                gammas.append(0.0)
            else:
                raise ValueError(f"unknown layer kind {kind!r}")
            kinds.append(kind)
            dims.append(int(units))
        dims.append(int(out_units))
        acts.append(_activation_name(out_activation))
        kinds.append("dense")
        gammas.append(0.0)
        if "rbf" not in kinds:
            raise ValueError("a network of Dense layers only is a DenseNet")
        if min(dims) < 1:
            raise ValueError(f"layer widths must be >= 1: {dims}")
        self.dims, self.acts, self.kinds, self.gammas = tuple(dims), tuple(acts), tuple(kinds), tuple(gammas)
        self.weights_flat = np.zeros(self.n_params, dtype=np.float32)
        self._plan = None
        self.reset_keras(rng if rng is not None else np.random.default_rng())

    def layer_slices(self) -> List[slice]:
        out, off = [], 0
        for i, o, kind in zip(self.dims[:-1], self.dims[1:], self.kinds):
            n = i * o if kind == "rbf" else (i + 1) * o
            out.append(slice(off, off + n))
            off += n
        return out

    @property
    def n_params(self) -> int:
        return self.layer_slices()[-1].stop

    # ------------------------------------------------------------------ weights
    def reset_keras(self, rng: np.random.Generator):
        for sl, i, o, kind in zip(self.layer_slices(), self.dims[:-1], self.dims[1:], self.kinds):
            if kind == "rbf":
                self.weights_flat[sl] = rng.uniform(-0.05, 0.05, size=i * o).astype(np.float32)
            else:
                lim = np.sqrt(6.0 / (i + o))
                self.weights_flat[sl.start:sl.start + i * o] = rng.uniform(-lim, lim, size=i * o).astype(np.float32)
                self.weights_flat[sl.start + i * o:sl.stop] = 0.0

    @property
    def trainable_variables(self) -> List[np.ndarray]:
        """Views of the flat vector: [mean (in, units)] of an RBF layer, [kernel (in, out), bias (out)] of a Dense one."""
        out = []
        for sl, i, o, kind in zip(self.layer_slices(), self.dims[:-1], self.dims[1:], self.kinds):
            flat = self.weights_flat[sl]
            out.append(flat[: i * o].reshape(i, o))
            if kind == "dense":
                out.append(flat[i * o:])
        return out

    get_weights = DenseNet.get_weights
    set_weights = DenseNet.set_weights
    set_flat = DenseNet.set_flat

    def to_json(self) -> str:
        raise ValueError("a network with an RBF layer has no Keras config: the RBF layer defines no get_config")

    # ------------------------------------------------------------------ inference
    def _forward(self, x) -> np.ndarray:
        import torch
        from ..engine import MLPSpec, PilcoPlan
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(len(x), -1))
        if self._plan is None:      # the policy alone: the smallest dynamics net, particle count and horizon a plan takes
            S, A = self.dims[0], self.dims[-1]
            self._plan = PilcoPlan(self, MLPSpec((S + A, S), ("linear",), "mse"), 2, 1)
        out = self._plan.act(torch.as_tensor(self.weights_flat).cuda(), torch.as_tensor(x).cuda())
        return out.cpu().numpy()

    def __call__(self, x, training=False):
        return Array(self._forward(x))


class ConvLayer(Layer):
    """A Conv2D layer: [kernel (kh, kw, cin, cout), bias (cout)] views of the flat vector (Keras's variable order)."""

    def __init__(self, class_name, config, kernel_shape):
        super().__init__(class_name, config, None, None)
        self.kernel_shape = tuple(int(d) for d in kernel_shape)

    @property
    def trainable_variables(self) -> List[np.ndarray]:
        sl = self._model.spec.layer_slices()[self._dense_index]
        flat = self._model.weights_flat[sl]
        n = int(np.prod(self.kernel_shape))
        return [flat[:n].reshape(self.kernel_shape), flat[n:]]


def _pair(v, layer: str, field: str):
    """A Keras int-or-pair field as (a, b)."""
    if isinstance(v, (int, np.integer)):
        v = (v, v)
    v = tuple(v) if isinstance(v, (list, tuple)) else None
    if v is None or len(v) != 2 or any(int(d) != d or int(d) < 1 for d in v):
        raise ValueError(f"{layer}: {field} must be one or two integers >= 1")
    return int(v[0]), int(v[1])


class ConvNet(DenseNet):
    """``[InputLayer] (Conv2D [MaxPooling2D])+ Flatten Dense+``: what the reference's model builder emits
    (utils.py:129-150) and its image script trains (tests/tf_dataset_test.py:42-57).  Offers what DenseNet offers; ``dims``
    and ``acts`` are the Dense stack's (dims[0] = the flattened NHWC features), ``spec`` is a ConvSpec whose
    ``layer_slices()`` run over all weight layers in network order, ``_dense_index`` of a layer is its index among them.
    Anything else raises a ValueError that names the layer and the field."""

    def __init__(self, model_config: str):
        from ..engine import CONV_MAX_K, ConvSpec
        cfg = json.loads(model_config) if isinstance(model_config, str) else model_config
        if cfg.get("class_name") != "Sequential":
            raise ValueError("only Keras Sequential models are supported")
        self._config = cfg
        self.layers: List[Layer] = []
        ops, dims, acts = [], [], []
        shape = None          # (h, w, c) while in the stem
        cur = None            # width once flattened
        n_weight = 0
        for lc in cfg["config"]["layers"]:
            cn, c = lc["class_name"], lc.get("config", {})
            what = f"{cn} '{c.get('name', cn.lower())}'"
            given = c.get("batch_input_shape") or (lc.get("build_config", {}) or {}).get("input_shape")
            if shape is None and cur is None and given is not None:
                if len(given) != 4:
                    raise ValueError(f"{what}: a conv model needs an input shape (h, w, c), not {tuple(given[1:])}")
                shape = tuple(int(d) for d in given[1:])
                self.input_shape = shape
            if cn == "InputLayer":
                continue
            if cn in ("Conv2D", "MaxPooling2D"):
                if cur is not None:
                    raise ValueError(f"{what}: a {cn} after Flatten is not supported")
                if shape is None:
                    raise ValueError(f"{what}: the first layer needs an input shape")
                if c.get("data_format", "channels_last") != "channels_last":
                    raise ValueError(f"{what}: data_format {c.get('data_format')!r} is not supported (channels_last only)")
            if cn == "Conv2D":
                kh, kw = _pair(c.get("kernel_size"), what, "kernel_size")
                filters = c.get("filters")
                if not isinstance(filters, (int, np.integer)) or filters < 1:
                    raise ValueError(f"{what}: filters must be an integer >= 1")
                if _pair(c.get("strides", (1, 1)), what, "strides") != (1, 1):
                    raise ValueError(f"{what}: strides {tuple(c['strides'])} are not supported (only (1, 1))")
                if _pair(c.get("dilation_rate", (1, 1)), what, "dilation_rate") != (1, 1):
                    raise ValueError(f"{what}: dilation_rate {tuple(c['dilation_rate'])} is not supported (only (1, 1))")
                if c.get("groups", 1) != 1:
                    raise ValueError(f"{what}: groups {c['groups']} is not supported (only 1)")
                if not c.get("use_bias", True):
                    raise ValueError(f"{what}: use_bias false is not supported")
                pad = c.get("padding", "valid")
                if pad not in ("valid", "same"):
                    raise ValueError(f"{what}: padding {pad!r} is not supported ('valid' or 'same')")
                act = _activation_name(c.get("activation", "linear"))
                if act == "softmax":
                    raise ValueError(f"{what}: activation 'softmax' is not supported on a Conv2D")
                ph, pw = (kh - 1, kw - 1) if pad == "same" else (0, 0)
                if kh > shape[0] + ph or kw > shape[1] + pw:
                    raise ValueError(f"{what}: kernel_size ({kh}, {kw}) is larger than the padded "
                                     f"{shape[0] + ph} x {shape[1] + pw} image")
                if kh * kw * shape[2] > CONV_MAX_K:
                    raise ValueError(f"{what}: kernel_size ({kh}, {kw}) over {shape[2]} channels is {kh * kw * shape[2]} taps "
                                     f"per filter, more than the {CONV_MAX_K} the kernels hold")
                layer = ConvLayer(cn, c, (kh, kw, shape[2], int(filters)))
                layer._dense_index = n_weight
                n_weight += 1
                ops.append(("conv", int(filters), kh, kw, pad, act))
                shape = (shape[0] + ph - kh + 1, shape[1] + pw - kw + 1, int(filters))
                self.layers.append(layer)
            elif cn == "MaxPooling2D":
                if not ops or ops[-1][0] != "conv":
                    raise ValueError(f"{what}: a MaxPooling2D must follow a Conv2D")
                ph, pw = _pair(c.get("pool_size", (2, 2)), what, "pool_size")
                strides = c.get("strides")
                if strides is not None and _pair(strides, what, "strides") != (ph, pw):
                    raise ValueError(f"{what}: strides {tuple(strides) if isinstance(strides, (list, tuple)) else strides} "
                                     f"differ from pool_size ({ph}, {pw}): overlapping or skipping pools are not supported")
                if c.get("padding", "valid") != "valid":
                    raise ValueError(f"{what}: padding {c.get('padding')!r} is not supported (only 'valid')")
                if ph > shape[0] or pw > shape[1]:
                    raise ValueError(f"{what}: pool_size ({ph}, {pw}) is larger than its {shape[0]} x {shape[1]} input")
                ops.append(("pool", ph, pw))
                shape = (shape[0] // ph, shape[1] // pw, shape[2])
                self.layers.append(Layer(cn, c, None, None))
            elif cn == "Flatten":
                if not ops:
                    raise ValueError(f"{what}: a conv model needs a Conv2D before Flatten")
                if cur is not None:
                    raise ValueError(f"{what}: a second Flatten is not supported")
                if c.get("data_format", "channels_last") != "channels_last":
                    raise ValueError(f"{what}: data_format {c.get('data_format')!r} is not supported (channels_last only)")
                cur = int(np.prod(shape))
                self.layers.append(Layer(cn, c, cur, cur))
            elif cn == "Dense":
                if cur is None:
                    raise ValueError(f"{what}: a Dense layer needs a Flatten between it and the Conv2D / MaxPooling2D layers")
                if not c.get("use_bias", True):
                    raise ValueError(f"{what}: use_bias false is not supported")
                units = int(c["units"])
                layer = Layer(cn, c, cur, units)
                layer._dense_index = n_weight
                n_weight += 1
                if not dims:
                    dims.append(cur)
                dims.append(units)
                acts.append(_activation_name(c.get("activation", "linear")))
                self.layers.append(layer)
                cur = units
            else:
                raise ValueError(f"{what}: unsupported layer class '{cn}'")
        if not acts:
            raise ValueError("the model has no Dense layer after its Conv2D layers")
        self.dims, self.acts = tuple(dims), tuple(acts)
        self.spec = ConvSpec(tuple(self.input_shape), tuple(ops),
                             MLPSpec(self.dims, self.acts, "scce" if acts[-1] == "softmax" else "mse"))
        for l in self.layers:
            l._model = self
        self.weights_flat = np.zeros(self.spec.n_params, dtype=np.float32)
        self._plan = None
        self.reset_glorot(np.random.default_rng())

    def reset_glorot(self, rng: np.random.Generator):
        """Keras's GlorotUniform: a conv kernel's fan_in = kh kw cin, fan_out = kh kw cout; biases zero."""
        off = 0
        for kh, kw, ci, co in self.spec.conv_shapes():
            n = kh * kw * ci * co
            lim = np.sqrt(6.0 / (kh * kw * ci + kh * kw * co))
            self.weights_flat[off:off + n] = rng.uniform(-lim, lim, size=n).astype(np.float32)
            self.weights_flat[off + n:off + n + co] = 0.0
            off += n + co
        for i, o in zip(self.dims[:-1], self.dims[1:]):
            lim = np.sqrt(6.0 / (i + o))
            self.weights_flat[off:off + i * o] = rng.uniform(-lim, lim, size=i * o).astype(np.float32)
            self.weights_flat[off + i * o:off + (i + 1) * o] = 0.0
            off += (i + 1) * o

    def _forward(self, x) -> np.ndarray:
        import torch
        from ..engine import ConvPlan
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(len(x), -1))
        if self._plan is None or self._plan.max_batch < len(x):
            self._plan = ConvPlan(self.spec, max_batch=max(len(x), 1))
        th = torch.as_tensor(self.weights_flat).cuda()
        return self._plan.forward(th, torch.as_tensor(x).cuda())[0].cpu().numpy()


_CONV_CLASSES = ("Conv2D", "MaxPooling2D")


def is_conv_config(model_config) -> bool:
    """Whether a Keras JSON (text or parsed) holds a Conv2D or MaxPooling2D layer: such a model is a ConvNet."""
    try:
        cfg = json.loads(model_config) if isinstance(model_config, str) else model_config
    except ValueError:
        return False
    layers = ((cfg.get("config") or {}).get("layers") or []) if isinstance(cfg, dict) else []
    return isinstance(layers, list) and any(isinstance(lc, dict) and lc.get("class_name") in _CONV_CLASSES for lc in layers)


def model_from_json(model_config: str) -> DenseNet:
    if isinstance(model_config, PolicyNet):
        raise ValueError("a network with an RBF layer is a Deep-PILCO policy only: no optimizer, DynamicsTraining or "
                         "BayesianModel takes it")
    if is_conv_config(model_config):
        return ConvNet(model_config)
    return DenseNet(model_config)


def conv_sequential_json(input_shape, stem: Sequence[tuple], units: Sequence[int], activations: Sequence[str]) -> str:
    """The Keras-2.15 JSON of a Sequential conv net, for callers that have no TensorFlow to produce it.  input_shape =
    (h, w, c); stem entries: ("conv", filters, kernel_size, padding, activation) or ("pool", pool_size), kernel_size and
    pool_size an int or a pair; then Flatten and Dense layers of `units` / `activations`."""
    input_shape = tuple(int(d) for d in input_shape)
    glorot = {"module": "keras.initializers", "class_name": "GlorotUniform", "config": {"seed": None}, "registered_name": None}
    zeros = {"module": "keras.initializers", "class_name": "Zeros", "config": {}, "registered_name": None}
    layers = [{"module": "keras.layers", "class_name": "InputLayer",
               "config": {"batch_input_shape": [None, *input_shape], "dtype": "float32", "sparse": False,
                          "ragged": False, "name": "input_1"}, "registered_name": None}]
    pair = lambda v: [int(v), int(v)] if isinstance(v, (int, np.integer)) else [int(d) for d in v]
    n_conv = n_pool = 0
    for op in stem:
        if op[0] == "conv":
            _, filters, ksize, padding, act = op
            layers.append({"module": "keras.layers", "class_name": "Conv2D",
                           "config": {"name": "conv2d" if n_conv == 0 else f"conv2d_{n_conv}", "trainable": True,
                                      "dtype": "float32", "filters": int(filters), "kernel_size": pair(ksize),
                                      "strides": [1, 1], "padding": padding, "data_format": "channels_last",
                                      "dilation_rate": [1, 1], "groups": 1, "activation": act, "use_bias": True,
                                      "kernel_initializer": glorot, "bias_initializer": zeros, "kernel_regularizer": None,
                                      "bias_regularizer": None, "activity_regularizer": None, "kernel_constraint": None,
                                      "bias_constraint": None}, "registered_name": None})
            n_conv += 1
        elif op[0] == "pool":
            layers.append({"module": "keras.layers", "class_name": "MaxPooling2D",
                           "config": {"name": "max_pooling2d" if n_pool == 0 else f"max_pooling2d_{n_pool}",
                                      "trainable": True, "dtype": "float32", "pool_size": pair(op[1]), "padding": "valid",
                                      "strides": pair(op[1]), "data_format": "channels_last"}, "registered_name": None})
            n_pool += 1
        else:
            raise ValueError(f"unknown stem entry {op[0]!r}")
    layers.append({"module": "keras.layers", "class_name": "Flatten",
                   "config": {"name": "flatten", "trainable": True, "dtype": "float32", "data_format": "channels_last"},
                   "registered_name": None})
    for k, (u, a) in enumerate(zip(units, activations)):
        layers.append({"module": "keras.layers", "class_name": "Dense",
                       "config": {"name": "dense" if k == 0 else f"dense_{k}", "trainable": True, "dtype": "float32",
                                  "units": int(u), "activation": a, "use_bias": True, "kernel_initializer": glorot,
                                  "bias_initializer": zeros, "kernel_regularizer": None, "bias_regularizer": None,
                                  "activity_regularizer": None, "kernel_constraint": None, "bias_constraint": None},
                       "registered_name": None})
    return json.dumps({"class_name": "Sequential", "config": {"name": "sequential", "layers": layers},
                       "keras_version": "2.15.0", "backend": "tensorflow"})


def sequential_json(input_shape, units: Sequence[int], activations: Sequence[str], flatten: bool = False) -> str:
    """Builds the Keras-2.15 JSON a ``tf.keras.Sequential`` of Dense layers serialises to
    (for callers that have no TensorFlow to produce it)."""
    input_shape = tuple(int(d) for d in (input_shape if isinstance(input_shape, (tuple, list)) else (input_shape,)))
    layers = [{"module": "keras.layers", "class_name": "InputLayer",
               "config": {"batch_input_shape": [None, *input_shape], "dtype": "float32", "sparse": False,
                          "ragged": False, "name": "input_1"}, "registered_name": None}]
    if flatten or len(input_shape) > 1:
        layers.append({"module": "keras.layers", "class_name": "Flatten",
                       "config": {"name": "flatten", "trainable": True, "dtype": "float32",
                                  "batch_input_shape": [None, *input_shape], "data_format": "channels_last"},
                       "registered_name": None, "build_config": {"input_shape": [None, *input_shape]}})
    prev = int(np.prod(input_shape))
    for k, (u, a) in enumerate(zip(units, activations)):
        layers.append({"module": "keras.layers", "class_name": "Dense",
                       "config": {"name": "dense" if k == 0 else f"dense_{k}", "trainable": True, "dtype": "float32",
                                  "units": int(u), "activation": a, "use_bias": True,
                                  "kernel_initializer": {"module": "keras.initializers", "class_name": "GlorotUniform",
                                                         "config": {"seed": None}, "registered_name": None},
                                  "bias_initializer": {"module": "keras.initializers", "class_name": "Zeros",
                                                       "config": {}, "registered_name": None},
                                  "kernel_regularizer": None, "bias_regularizer": None, "activity_regularizer": None,
                                  "kernel_constraint": None, "bias_constraint": None},
                       "registered_name": None, "build_config": {"input_shape": [None, prev]}})
        prev = int(u)
    return json.dumps({"class_name": "Sequential", "config": {"name": "sequential", "layers": layers},
                       "keras_version": "2.15.0", "backend": "tensorflow"})

"""Conv models on the host: the parser and the flat layout, every refusal, the C-ABI's argument errors, and the float64
restatement of tests/conv_checks.py pinned three ways -- against torch-CPU float64 autograd on every GPU case (1e-10), by a
float32 stand-in that must lie four times inside the GPU tests' bound, and by ten wrong restatements that the GPU
tests' comparison must tell from the right one -- and the limits of the kernels (taps per filter, rows per launch), each
refused by name on one side and accepted on the other.  No GPU."""

import ctypes
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_checks as cc
from bayesian_inference_for_nn_amd.engine import ConvSpec
from bayesian_inference_for_nn_amd.nn.model import ConvNet, DenseNet, conv_sequential_json, model_from_json, sequential_json

PAIRS = [(n, b) for n in cc.ALL for b in cc.CASES[n].batches]


# ---------------------------------------------------------------- parser and layout
def builder_json():
    """What the reference's model builder emits (utils.py:129-150) for filters 8, 16, kernel 3, hidden 12, 10 classes on
    28 x 28 x 1: Conv2D(f, k, activation) + MaxPooling2D(2) per filter, Flatten, Dense layers."""
    return conv_sequential_json((28, 28, 1), [("conv", 8, 3, "valid", "relu"), ("pool", 2), ("conv", 16, 3, "valid", "tanh"),
                                               ("pool", 2)], (12, 10), ("relu", "softmax"))


def script_json(side=32, filters=32):
    """The model of the reference's image script (tests/tf_dataset_test.py:42-57)."""
    return conv_sequential_json((side, side, 3), [("conv", filters, 3, "same", "relu")], (50, 10), ("relu", "softmax"))


def test_builder_model_layout():
    net = model_from_json(builder_json())
    assert isinstance(net, ConvNet)
    assert net.spec.ops == (("conv", 8, 3, 3, "valid", "relu"), ("pool", 2, 2), ("conv", 16, 3, 3, "valid", "tanh"), ("pool", 2, 2))
    assert [o for _, o in net.spec.op_shapes()] == [(26, 26, 8), (13, 13, 8), (11, 11, 16), (5, 5, 16)]
    assert net.dims == (400, 12, 10) and net.acts == ("relu", "softmax")
    assert [l.class_name for l in net.layers] == ["Conv2D", "MaxPooling2D", "Conv2D", "MaxPooling2D", "Flatten", "Dense", "Dense"]
    shapes = [v.shape for v in net.trainable_variables]
    assert shapes == [(3, 3, 1, 8), (8,), (3, 3, 8, 16), (16,), (400, 12), (12,), (12, 10), (10,)]
    assert net.count_params() == 80 + 1168 + 4812 + 130 == net.spec.n_params == len(net.weights_flat)
    assert net.spec.layer_slices() == [slice(0, 80), slice(80, 1248), slice(1248, 6060), slice(6060, 6190)]
    assert [l._dense_index for l in net.layers] == [0, None, 1, None, None, 2, 3]


def test_script_model_layout_and_views():
    net = model_from_json(script_json())
    assert net.spec.features == 32 * 32 * 32 and net.dims == (32768, 50, 10)
    assert net.count_params() == 896 + 1638450 + 510          # Keras's model.summary() of that script
    # the views are the flat vector: kernel (kh, kw, cin, cout) row-major, then the bias, conv layers first
    net.set_flat(np.arange(net.count_params(), dtype=np.float32) % 1000)
    k, b = net.layers[0].trainable_variables
    assert k.shape == (3, 3, 3, 32) and k[1, 2, 0, 5] == ((1 * 3 + 2) * 3 + 0) * 32 + 5 and b[3] == (864 + 3) % 1000
    k[0, 0, 0, 0] = -7.0
    assert net.weights_flat[0] == -7.0
    w = net.get_weights()
    other = model_from_json(net.to_json())
    other.set_weights(w)
    assert np.array_equal(other.weights_flat, net.weights_flat)
    assert json.loads(other.to_json()) == json.loads(script_json())


def test_glorot_uses_the_receptive_field():
    net = model_from_json(script_json(8, 8))
    net.reset_glorot(np.random.default_rng(0))
    k, b = net.layers[0].trainable_variables
    lim = np.sqrt(6.0 / (3 * 3 * 3 + 3 * 3 * 8))
    assert np.abs(k).max() <= lim and np.abs(k).max() > 0.9 * lim and not b.any()
    k, b = net.layers[2].trainable_variables
    assert np.abs(k).max() <= np.sqrt(6.0 / (512 + 50)) and not b.any()


def test_dense_models_still_parse_as_before():
    net = model_from_json(sequential_json((4, 4), (5, 3), ("relu", "softmax")))
    assert type(net) is DenseNet and net.dims == (16, 5, 3)


def _edit(js, layer, **fields):
    cfg = json.loads(js)
    cfg["config"]["layers"][layer]["config"].update(fields)
    return json.dumps(cfg)


REFUSALS = [
    ("strides", lambda: _edit(script_json(8, 4), 1, strides=[2, 2]), ("Conv2D", "strides")),
    ("dilation", lambda: _edit(script_json(8, 4), 1, dilation_rate=[2, 2]), ("Conv2D", "dilation_rate")),
    ("groups", lambda: _edit(script_json(8, 4), 1, groups=3), ("Conv2D", "groups")),
    ("channels_first", lambda: _edit(script_json(8, 4), 1, data_format="channels_first"), ("Conv2D", "data_format")),
    ("no bias", lambda: _edit(script_json(8, 4), 1, use_bias=False), ("Conv2D", "use_bias")),
    ("padding", lambda: _edit(script_json(8, 4), 1, padding="causal"), ("Conv2D", "padding")),
    ("softmax on a conv", lambda: _edit(script_json(8, 4), 1, activation="softmax"), ("Conv2D", "activation")),
    ("kernel too large", lambda: _edit(conv_sequential_json((4, 4, 1), [("conv", 2, 3, "valid", "relu")], (2,), ("softmax",)),
                                       1, kernel_size=[5, 2]), ("Conv2D", "kernel_size")),
    ("overlapping pool", lambda: _edit(builder_json(), 2, strides=[1, 1]), ("MaxPooling2D", "strides")),
    ("same pool", lambda: _edit(builder_json(), 2, padding="same"), ("MaxPooling2D", "padding")),
    ("pool too large", lambda: _edit(builder_json(), 4, pool_size=[12, 12], strides=None), ("MaxPooling2D", "pool_size")),
]


@pytest.mark.parametrize("name", [r[0] for r in REFUSALS])
def test_refusals_name_the_layer_and_the_field(name):
    _, make, words = next(r for r in REFUSALS if r[0] == name)
    with pytest.raises(ValueError) as e:
        model_from_json(make())
    for w in words:
        assert w in str(e.value), str(e.value)


def test_other_layers_and_orders_are_refused():
    cfg = json.loads(builder_json())
    drop = {"module": "keras.layers", "class_name": "Dropout", "config": {"name": "dropout", "rate": 0.25}}
    cfg["config"]["layers"].insert(3, drop)
    with pytest.raises(ValueError, match="Dropout"):
        model_from_json(json.dumps(cfg))
    cfg = json.loads(builder_json())
    del cfg["config"]["layers"][5]                       # no Flatten
    with pytest.raises(ValueError, match="Flatten"):
        model_from_json(json.dumps(cfg))
    cfg = json.loads(builder_json())
    cfg["config"]["layers"].insert(3, cfg["config"]["layers"][2])      # a pool on a pool
    with pytest.raises(ValueError, match="MaxPooling2D"):
        model_from_json(json.dumps(cfg))
    with pytest.raises(ValueError, match="input shape"):
        model_from_json(_edit(script_json(8, 4), 0, batch_input_shape=[None, 192]))
    # Keras's default pool strides (None) mean pool_size
    assert model_from_json(_edit(builder_json(), 2, strides=None)).dims == (400, 12, 10)


def test_compat_stand_in_builds_conv_models(monkeypatch):
    """compat/tensorflow's Conv2D / MaxPooling2D give the JSON of the two model families the reference builds: its image
    script's (tests/tf_dataset_test.py:42-57) and its model builder's (utils.py:129-150)."""
    import os
    import sys
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "compat"))
    sys.modules.pop("tensorflow", None)
    import tensorflow as tf
    try:
        L = tf.keras.layers
        net = tf.keras.Sequential()
        for layer in (L.Conv2D(32, 3, padding="same", activation="relu", input_shape=(32, 32, 3)), L.Flatten(),
                      L.Dense(50, activation="relu"), L.Dense(10, activation="softmax")):
            net.add(layer)
        assert json.loads(net.to_json()) == json.loads(script_json())
        stack = [L.Conv2D(8, 3, activation="relu", input_shape=(28, 28, 1)), L.MaxPooling2D(2), L.Conv2D(16, 3, activation="tanh"),
                 L.MaxPooling2D(2), L.Flatten(), L.Dense(12, activation="relu"), L.Dense(10, activation="softmax")]
        assert json.loads(tf.keras.Sequential(stack).to_json()) == json.loads(builder_json())
        with pytest.raises(ValueError, match="strides"):
            tf.keras.Sequential([L.Conv2D(4, 3, strides=2, input_shape=(8, 8, 1)), L.Flatten(), L.Dense(2)]).to_json()
    finally:
        sys.modules.pop("tensorflow", None)


# ---------------------------------------------------------------- C-ABI: argument errors need no GPU
def _stem_create(shape, ops, max_batch=4):
    from bayesian_inference_for_nn_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    flat = [v for op in ops for v in op]
    rc = lib.pyz_stem_create(*shape, len(ops), (ctypes.c_int32 * len(flat))(*flat), max_batch, 1, ctypes.byref(h))
    return lib, rc, h, (lib.pyz_last_error() or b"").decode()


def test_stem_argument_errors_do_not_need_a_gpu():
    from bayesian_inference_for_nn_amd import _lib
    lib, rc, h, msg = _stem_create((8, 8, 1), [(7, 1, 1, 1, 0, 0)])
    assert rc == -1 and h.value is None and "unknown kind" in msg
    lib, rc, h, msg = _stem_create((4, 4, 1), [(0, 2, 5, 2, 0, 1)])
    assert rc == -2 and h.value is None and "larger than the padded" in msg
    lib, rc, h, msg = _stem_create((4, 4, 1), [(0, 2, 3, 3, 1, 1), (1, 5, 2, 0, 0, 0)])
    assert rc == -2 and "pool is larger" in msg
    lib, rc, h, msg = _stem_create((4, 4, 1), [(0, 2, 3, 3, 1, 4)])
    assert rc == -1 and "activation" in msg
    lib, rc, h, msg = _stem_create((4, 4, 1), [(1, 2, 2, 0, 0, 0)])
    assert rc == -1 and "must follow a Conv2D" in msg
    lib, rc, h, msg = _stem_create((64, 64, 512), [(0, 4, 3, 3, 1, 1)])
    assert rc == -2 and "taps" in msg
    assert lib.pyz_stem_param_count(None) == -1 and lib.pyz_stem_feature_count(None) == -1
    assert lib.pyz_stem_destroy(None) == 0
    assert lib.pyz_convnet_sgd_step(None, None, None, None, None, None, 1, 0.1, None, None) == -1
    with pytest.raises(_lib.PyzError):
        _lib.check(rc)


def test_limits_are_refused_by_name_and_their_neighbours_are_not():
    """The tap limit and the row limit, each from both sides.  pyz_stem_create checks shapes before it looks for a device:
    an accepted shape gets as far as the device (or, with one, to a plan), a refused one stops with the limit's name.  On
    the GPU case J (K = 4094) and the 2^24 - 1 rows of tests/test_gpu_conv_paths.py run the accepted neighbours."""
    from bayesian_inference_for_nn_amd import _lib, engine
    header = open(_lib._build.CSRC + "/pyz_conv.h").read()
    assert f"#define PYZ_CONV_MAX_K {engine.CONV_MAX_K} " in header and engine.CONV_MAX_K == cc.CONV_MAX_K == 4094
    assert "#define PYZ_CONV_MAX_ROWS (1 << 24) " in header and cc.CONV_MAX_ROWS == 1 << 24

    def outcome(shape, ops, max_batch):
        lib, rc, h, msg = _stem_create(shape, ops, max_batch)
        if h.value is not None:
            lib.pyz_stem_destroy(h)
        return rc, msg
    # K = 3 * 3 * 455 = 4095 is one tap too many; 2 * 23 * 89 = 4094 (case J) is not
    rc, msg = outcome((3, 3, 455), [(0, 2, 3, 3, 0, 1)], 4)
    assert rc == -2 and "op 0: 4095 taps per filter exceed 4094" in msg
    rc, msg = outcome((2, 23, 89), [(0, 3, 2, 23, 0, 2)], 36)
    assert rc == 0 or "no HIP device" in msg, (rc, msg)
    # 4098 images of the 63 x 65 map are 16 781 310 rows, 4097 are 16 777 215 = 2^24 - 1
    rc, msg = outcome((63, 65, 1), [(0, 2, 3, 3, 1, 2)], 4098)
    assert rc == -2 and "op 0: max_batch 4098 x the 63 x 65 x 2 map exceeds the kernels' row or index range" in msg
    assert 4097 * 63 * 65 == cc.CONV_MAX_ROWS - 1 < cc.CONV_MAX_ROWS < 4098 * 63 * 65
    # a same kernel larger than its map is a model (case K), a valid one is not
    assert ConvSpec((2, 3, 2), (("conv", 3, 5, 5, "same", "tanh"),), cc.CASES["K"].spec().tail).features == 18
    lib, rc, h, msg = _stem_create((2, 3, 2), [(0, 3, 5, 5, 0, 2)])
    assert rc == -2 and "larger than the padded" in msg


def test_python_surface_refuses_too_many_taps_by_layer():
    from bayesian_inference_for_nn_amd.engine import ConvPlan, MLPSpec
    with pytest.raises(ValueError, match="op 0: 4095 taps per filter exceed 4094"):
        ConvPlan(ConvSpec((3, 3, 455), (("conv", 2, 3, 3, "valid", "relu"),), MLPSpec((2, 2), ("softmax",))), max_batch=4)
    with pytest.raises(ValueError) as e:
        model_from_json(conv_sequential_json((3, 3, 455), [("conv", 2, 3, "valid", "relu")], (2,), ("softmax",)))
    assert "Conv2D" in str(e.value) and "kernel_size" in str(e.value) and "4095" in str(e.value) and "4094" in str(e.value)
    # the neighbour parses: 4094 taps
    net = model_from_json(conv_sequential_json((2, 23, 89), [("conv", 3, (2, 23), "valid", "tanh")], (2,), ("softmax",)))
    assert net.spec.conv_shapes() == [(2, 23, 89, 3)] and net.spec.features == 3


def test_plan_refuses_a_tail_that_does_not_fit_before_it_needs_a_device():
    from bayesian_inference_for_nn_amd.engine import ConvPlan, MLPSpec
    with pytest.raises(ValueError, match="features"):
        ConvPlan(ConvSpec((7, 6, 3), (("conv", 5, 3, 3, "same", "relu"),), MLPSpec((200, 4), ("softmax",))), max_batch=4)
    with pytest.raises(ValueError, match="larger than"):
        ConvPlan(ConvSpec((2, 2, 1), (("conv", 5, 3, 3, "valid", "relu"),), MLPSpec((5, 4), ("softmax",))), max_batch=4)


# ---------------------------------------------------------------- refusals of the Python surface (decided before any device work)
class _Data:
    def __init__(self, x, y, loss):
        from bayesian_inference_for_nn_amd.datasets import ArrayDataset
        self._ds, self._loss = ArrayDataset(x, y), loss

    def training_dataset(self):
        return self._ds


def test_read_outs_without_a_conv_form_refuse_by_name():
    from bayesian_inference_for_nn_amd.nn import BayesianModel
    bm = BayesianModel(script_json(8, 4))
    x = np.zeros((3, 8, 8, 3), dtype=np.float32)
    for call in (lambda: bm.adversarial_examples(x, np.zeros(3), "scce", 0.1, 2), lambda: bm.predictive_surface(x, 2),
                 lambda: bm.grid_surface(np.zeros((192, 2)), 0, 1, 2, 0, 1, 2, 2)):
        with pytest.raises(ValueError, match="conv model"):
            call()
    # the workspace rule counts the stem's maps: an output and a delta per op (and a pool's winners) per (draw, row)
    assert bm._stem_floats() == 2 * 8 * 8 * 4
    assert BayesianModel(builder_json())._stem_floats() == 2 * 26 * 26 * 8 + 3 * 13 * 13 * 8 + 2 * 11 * 11 * 16 + 3 * 5 * 5 * 16
    assert BayesianModel(sequential_json((4,), (3,), ("softmax",)))._stem_floats() == 0


def test_binary_crossentropy_on_a_conv_model_is_refused():
    """The conv net's loss goes through the unfused loss kernels, which have no BinaryCrossentropy arm (a Dense net with one
    sigmoid unit always takes the fused head): the combination is refused, by ConvPlan and at compile, before any device work."""
    from bayesian_inference_for_nn_amd.engine import ConvPlan, MLPSpec
    from bayesian_inference_for_nn_amd.losses import BinaryCrossentropy
    from bayesian_inference_for_nn_amd.optimizers import SGD, SWAG
    from bayesian_inference_for_nn_amd.optimizers.hyperparameters import HyperParameters
    ops = (("conv", 4, 3, 3, "same", "relu"),)
    with pytest.raises(ValueError, match="BinaryCrossentropy"):
        ConvPlan(ConvSpec((8, 8, 1), ops, MLPSpec((256, 1), ("sigmoid",), "bce")), max_batch=4)
    cfg = conv_sequential_json((8, 8, 1), [("conv", 4, 3, "same", "relu")], (1,), ("sigmoid",))
    x, y = cc.toy_data()
    for cls in (SGD, SWAG):
        with pytest.raises(ValueError, match="BinaryCrossentropy") as e:
            cls().compile(HyperParameters(lr=0.1, k=3, frequency=1, scale=1.0, batch_size=32), cfg,
                          _Data(x, y.astype(np.float32)[:, None], BinaryCrossentropy), verbose=False,
                          starting_model=model_from_json(cfg))
        assert cls.__name__ in str(e.value)


# ---------------------------------------------------------------- the restatement, pinned by torch autograd
def torch_loss_grad(case, theta, x, y, dtype):
    """loss, flat gradient, features and output of the batch by torch-CPU autograd (F.conv2d, F.max_pool2d) in `dtype`."""
    spec = case.spec()
    th = torch.tensor(np.asarray(theta), dtype=dtype, requires_grad=True)
    B = len(x)
    h = torch.tensor(np.asarray(x), dtype=dtype).reshape((B,) + tuple(case.shape)).permute(0, 3, 1, 2)    # NCHW
    slices, shapes = spec.layer_slices(), spec.variable_shapes()
    wi = 0
    acts = {"relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "linear": lambda t: t}
    for op in spec.ops:
        if op[0] == "conv":
            ks = shapes[wi][0]
            n = int(np.prod(ks))
            W = th[slices[wi].start:slices[wi].start + n].reshape(ks).permute(3, 2, 0, 1)     # (cout, cin, kh, kw)
            b = th[slices[wi].start + n:slices[wi].stop]
            wi += 1
            h = acts[op[5]](F.conv2d(h, W, b, padding=op[4]))
        else:
            h = F.max_pool2d(h, (op[1], op[2]))
    feat = h.permute(0, 2, 3, 1).reshape(B, -1)
    a = feat
    for act in spec.acts:
        ks = shapes[wi][0]
        n = ks[0] * ks[1]
        a = a @ th[slices[wi].start:slices[wi].start + n].reshape(ks) + th[slices[wi].start + n:slices[wi].stop]
        wi += 1
        if act != "softmax":
            a = acts[act](a)
    if case.loss == "scce":
        loss = F.cross_entropy(a, torch.tensor(np.asarray(y), dtype=torch.long))
        out = torch.softmax(a, dim=1)
    else:
        loss = F.mse_loss(a, torch.tensor(np.asarray(y), dtype=dtype).reshape(a.shape))
        out = a
    loss.backward()
    return float(loss), th.grad.numpy().astype(np.float64), feat.detach().numpy().astype(np.float64), out.detach().numpy()


@pytest.mark.parametrize("name,batch", PAIRS)
def test_restatement_matches_torch_float64_autograd(name, batch):
    d = cc.make(name, batch)
    spec = d.case.spec()
    for p in range(3 if name in cc.P_CASES else 1):
        ref = cc.reference(name, batch, p)
        loss, grad, feat, out = torch_loss_grad(d.case, d.theta[p].astype(np.float64), d.x[d.idx], d.y[d.idx], torch.float64)
        e = cc.errors(loss, grad, feat, ref, spec)
        e["out"] = cc.rel(out, ref[3])
        cc.assert_close(e, f"{name} batch {batch} particle {p}: restatement against torch float64", tol=1e-10)


@pytest.mark.parametrize("name,batch", PAIRS)
def test_float32_stand_in_lies_four_times_inside_the_gpu_bound(name, batch):
    d = cc.make(name, batch)
    ref = cc.reference(name, batch)
    loss, grad, feat, _ = torch_loss_grad(d.case, d.theta[0], d.x[d.idx], d.y[d.idx], torch.float32)
    cc.assert_close(cc.errors(loss, grad, feat, ref, d.case.spec()), f"{name} batch {batch}: float32 stand-in", tol=cc.TOL / 4)


def test_generator_conditions_hold():
    for name, batch in PAIRS:
        d = cc.make(name, batch)
        assert d.margin > cc.MARGIN, (name, batch, d.margin)
    # the ties case has exact ties inside its windows (or it would not test the rule)
    d = cc.make("T", 5)
    f = cc.forward(d.case.spec(), d.theta[0].astype(np.float64), d.x[d.idx].astype(np.float64))
    v, _, _ = cc._pool_view(f["tape"][0]["h"], 3, 3, None)
    s = np.sort(v, axis=-1)
    assert (s[..., -1] == s[..., -2]).mean() > 0.2


@pytest.mark.parametrize("wrong", cc.WRONG)
def test_wrong_restatements_fail_the_gpu_comparison(wrong):
    """Each wrong restatement misses the GPU tests' bound on every case it applies to, and applies to at least one."""
    applied = 0
    for name, batch in PAIRS:
        d = cc.make(name, batch)
        if not cc.wrong_applies(d.case, wrong):
            continue
        applied += 1
        spec = d.case.spec()
        y = d.y[:batch] if wrong == "labels not gathered by row_idx" else d.y[d.idx]
        loss, grad, feat, _ = cc.loss_grad(spec, d.theta[0].astype(np.float64), d.x[d.idx].astype(np.float64), y, wrong=wrong)
        e = cc.errors(loss, grad, feat, cc.reference(name, batch), spec)
        worst = max(e.values())
        print(f"{wrong} on {name} batch {batch}: worst {worst:.2e} of the scale ({max(e, key=e.get)})")
        assert worst > cc.TOL, (wrong, name, batch, e)
    assert applied >= 1, wrong


def test_at_least_ten_wrong_restatements():
    assert len(set(cc.WRONG)) >= 10


def test_the_two_new_wrong_restatements_apply_to_no_old_case():
    """The gap the rows H and I close, written down: a data gradient without the act' of the conv below, or cropped at the
    wrong pad, passed every comparison of the eight cases the feature shipped with."""
    no_act, crop = "no act' between two adjacent convs", "data gradient cropped at the bottom / right pad"
    assert no_act in cc.WRONG and crop in cc.WRONG
    assert [n for n in cc.ALL if cc.wrong_applies(cc.CASES[n], no_act)] == ["H", "I"]
    assert [n for n in cc.ALL if cc.wrong_applies(cc.CASES[n], crop)] == ["I"]
    for name in cc.OLD:       # where it does not apply the wrong restatement is the right one, bit for bit
        d = cc.make(name, cc.CASES[name].batches[-1])
        for wrong in (no_act, crop):
            _, grad, _, _ = cc.loss_grad(d.case.spec(), d.theta[0].astype(np.float64), d.x[d.idx].astype(np.float64), d.y[d.idx],
                                         wrong=wrong)
            assert np.array_equal(grad, cc.reference(name, cc.CASES[name].batches[-1])[1]), (name, wrong)


def test_stem_grad_is_the_stem_half_of_loss_grad():
    """cc.stem_grad from the feature gradient the Dense layer sends down is the stem's block of cc.loss_grad (which the
    torch pin above covers): the reference of the stem-only GPU tests."""
    for name in ("C", "H"):
        batch = cc.CASES[name].batches[-1]
        d = cc.make(name, batch)
        spec = d.case.spec()
        theta = d.theta[0].astype(np.float64)
        f = cc.forward(spec, theta, d.x[d.idx].astype(np.float64))
        W, _ = cc.unpack(spec, theta)[-1]
        delta = f["out"].copy()
        delta[np.arange(batch), d.y[d.idx]] -= 1.0
        g = cc.stem_grad(f, (delta / batch) @ W.T)
        ref = cc.reference(name, batch)[1]
        assert g.shape == (spec.stem_params,) and np.abs(g - ref[:spec.stem_params]).max() <= 1e-14 * np.abs(ref).max()


# ---------------------------------------------------------------- the training task of the end-to-end GPU test
def test_restatement_training_reaches_a_quarter():
    """200 SGD steps of the float64 restatement on the toy task: the mean loss of the last 20 is under a quarter of the
    first 20's (the GPU test asks the device for a half)."""
    first, last = cc.toy_training_losses()
    print(f"toy task, float64 restatement: first 20 {first:.4f}, last 20 {last:.4f}")
    assert last < 0.25 * first

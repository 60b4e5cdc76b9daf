"""Result container of every optimizer: a model + per-layer-interval weight distributions,
Monte-Carlo ``predict``, directory ``store`` / ``load``
(mirrors Pyesian/nn/BayesianModel.py:10-203; the read-out is batched on the GPU:
all ``nb_samples`` weight draws go through one particle-batched forward, pyz_predict)."""

from __future__ import annotations

import json
import os
import shutil

import numpy as np

from .model import Array, DenseNet, model_from_json


def _host(a) -> np.ndarray:
    """a (NumPy, array-like, or something with ``.numpy()``) as a NumPy array."""
    return np.asarray(a.numpy() if hasattr(a, "numpy") else a)


class BayesianModel:
    def __init__(self, model_config: str):
        self._model_config = model_config
        model: DenseNet = model_from_json(model_config)
        self._n_layers = len(model.layers)
        self._layers_dtbn_intervals = []
        self._distributions = []
        self._model = model
        self._plan = None
        self._grad_plan = None      # adversarial_examples: a plan of its own, it carries the loss

    # ------------------------------------------------------------------ distributions
    def apply_distribution(self, distribution, start_layer: int, end_layer: int):
        """Insertion rule of BayesianModel.py:25-48, as written: the first interval is appended;
        a later one is inserted after the first stored interval whose start is smaller; an
        interval that is not greater than any stored start is silently dropped."""
        if start_layer > end_layer:
            raise ValueError('starting_layer must be less than end_layer')
        elif start_layer < 0 or end_layer >= self._n_layers:
            raise ValueError('out of bounds')
        interval = [start_layer, end_layer]
        if len(self._layers_dtbn_intervals) == 0:
            self._layers_dtbn_intervals.append(interval)
            self._distributions.append(distribution)
            return
        for i in range(len(self._layers_dtbn_intervals)):
            if start_layer > self._layers_dtbn_intervals[i][0]:
                self._layers_dtbn_intervals = self._layers_dtbn_intervals[:i + 1] + [interval] + \
                    self._layers_dtbn_intervals[i + 1:]
                self._distributions = self._distributions[:i + 1] + [distribution] + self._distributions[i + 1:]
                break

    def apply_distributions_layers(self, layer_list, dtbn_list):
        self._layers_dtbn_intervals = layer_list
        self._distributions = dtbn_list

    # ------------------------------------------------------------------ sampling
    def _interval_slices(self):
        """flat slice of the parameters covered by each interval (layers start..end inclusive)."""
        lay_slices = {}
        for layer_idx, layer in enumerate(self._model.layers):
            if layer._dense_index is not None:
                lay_slices[layer_idx] = self._model.spec.layer_slices()[layer._dense_index]
        out = []
        for start, end in self._layers_dtbn_intervals:
            idxs = [i for i in range(start, end + 1) if i in lay_slices]
            if idxs:
                out.append(slice(lay_slices[idxs[0]].start, lay_slices[idxs[-1]].stop))
            else:
                out.append(slice(0, 0))
        return out

    def sample_weights_matrix(self, n: int) -> np.ndarray:
        """(n, D) float32: n joint draws, one ``Distribution`` draw per interval (BayesianModel.py:63-77)."""
        W = np.repeat(self._model.weights_flat[None, :], n, axis=0).astype(np.float32)
        for dist, sl in zip(self._distributions, self._interval_slices()):
            if sl.stop > sl.start:
                draws = np.asarray(dist.sample_n(n), dtype=np.float32)
                W[:, sl] = draws[:, : sl.stop - sl.start]
        return W

    def sample_weights_device(self, n: int):
        """The same n joint draws as a CUDA tensor.  Every result distribution of the package is drawn on the device:
        Normal and MultivariateNormalDiagPlusLowRank posteriors from the Philox stream of tfd.seed (100 draws of a
        159 010-parameter posterior cost 0.2 s of host random numbers otherwise), Deterministic ones are copied, Sampled
        ones are gathered from a device copy of their samples by indices drawn on the host as ``sample_n`` draws them.  A
        distribution without ``sample_n_device``, or whose ``sample_n_device`` returns False (PYZ_SAMPLE_DEVICE=0, more
        deviation columns than PYZ_LOWRANK_MAX_K, a sample bank beyond PYZ_SAMPLED_BANK_MAX), is drawn on the host with
        ``sample_n`` and uploaded.  A model whose ``sample_weights_matrix`` has been replaced (a subclass, an instance
        attribute) is drawn through the replacement: it defines the draws."""
        import torch
        if getattr(self.sample_weights_matrix, "__func__", None) is not BayesianModel.sample_weights_matrix:
            return torch.as_tensor(np.ascontiguousarray(self.sample_weights_matrix(n), dtype=np.float32)).cuda()
        slices = self._interval_slices()
        capable = [getattr(d, "sample_n_device", None) is not None and getattr(d, "_size", 0) <= sl.stop - sl.start
                   for d, sl in zip(self._distributions, slices)]
        if not any(capable):
            return torch.as_tensor(self.sample_weights_matrix(n)).cuda()
        W = torch.as_tensor(self._model.weights_flat.astype(np.float32)).cuda().repeat(n, 1).contiguous()
        for dist, sl, cap in zip(self._distributions, slices, capable):
            if sl.stop <= sl.start:
                continue
            if cap and dist.sample_n_device(n, W, sl.start):
                continue
            draws = np.asarray(dist.sample_n(n), dtype=np.float32)
            W[:, sl] = torch.as_tensor(np.ascontiguousarray(draws[:, : sl.stop - sl.start])).cuda()
        return W

    def _sample_weights(self):
        self._model.set_flat(self.sample_weights_matrix(1)[0])

    def sample_model(self) -> DenseNet:
        self._sample_weights()
        model = model_from_json(self._model_config)
        model.set_flat(self._model.weights_flat)
        return model

    def sample_n_models(self, n) -> list:
        return [self.sample_model() for _ in range(n)]

    # ------------------------------------------------------------------ read-out
    _predict_rows_cap = 16384      # rows per launch sequence of predict (more rows: several sequences, results joined on the device)

    def _read_out_plan(self, n: int, nb_samples: int, spec=None):
        """(rows per launch sequence, the plan that serves them) of a read-out of n rows and nb_samples draws: the plan of
        the model's own spec, kept in self._plan, or (adversarial_examples) of the given loss-carrying spec, kept in
        self._grad_plan.
        Bounds the activation workspace: rows x samples per launch (the plan keeps an activation and a delta buffer per
        layer: 2 * sum(widths) floats per (sample, row)).  2^29 floats = 2 GiB of the 288: 100 draws x 10 000 rows of the
        784 -> 200 -> 10 model go out as ONE launch per layer (3.35 ms for the wide layer against 7 x 0.61 ms in seven)."""
        from ..engine import make_plan
        rows = min(n, int(self._predict_rows_cap))
        per = 2 * sum(int(d) for d in self._model.dims[1:]) + self._stem_floats()
        chunk_s = max(1, min(nb_samples, int(os.environ.get("PYZ_PREDICT_WS", 1 << 29)) // max(1, rows * per)))
        attr, spec = ("_plan", self._model.spec) if spec is None else ("_grad_plan", spec)
        plan = getattr(self, attr)
        if plan is None or plan.spec != spec or plan.max_batch < rows or plan.max_particles < chunk_s:
            plan = make_plan(spec, max_batch=rows, max_particles=chunk_s)
            setattr(self, attr, plan)
        return rows, plan

    @staticmethod
    def _device_rows(x):
        """Rows given as NumPy, as something with ``.numpy()`` or as a CUDA tensor (rows made on the device stay there),
        as the (n, -1) contiguous float32 device tensor."""
        import torch
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.to(torch.float32).reshape(len(x), -1).contiguous()
        x = _host(x)
        return torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(len(x), -1))).cuda()   # (no host copy of float32 input)

    @staticmethod
    def _walk_rows(n: int, rows: int, chunk, row_axis=()):
        """``chunk(r0, count)`` -> a tuple of device tensors (None where an output is not wanted) for every chunk of at
        most `rows` of the n rows; returns the tuple for all n rows.  A single chunk's tensors are returned as they are, no
        copy; otherwise the full outputs are allocated once and each chunk's are written into their slices.  row_axis[k]:
        the axis of output k that runs over the rows (0 where not given)."""
        full = None
        for r0 in range(0, n, rows):
            part = chunk(r0, min(rows, n - r0))
            if rows >= n:
                return part
            axes = tuple(row_axis) + (0,) * (len(part) - len(row_axis))
            if full is None:
                full = tuple(None if t is None else t.new_empty(t.shape[:a] + (n,) + t.shape[a + 1:])
                             for t, a in zip(part, axes))
            for out, t, a in zip(full, part, axes):
                if t is not None:
                    out.narrow(a, r0, t.shape[a]).copy_(t)
        return full

    def _is_conv(self) -> bool:
        return hasattr(self._model.spec, "ops")

    def _stem_floats(self) -> int:
        """Workspace floats per (draw, row) of a conv model's stem: an output and a delta map per op, and a pool's
        winners (0 for a Dense model)."""
        if not self._is_conv():
            return 0
        spec = self._model.spec
        return sum((3 if op[0] == "pool" else 2) * o[0] * o[1] * o[2] for op, (_, o) in zip(spec.ops, spec.op_shapes()))

    def _refuse_conv(self, what: str):
        if self._is_conv():
            raise ValueError(f"{what} is not built for a conv model (a model with Conv2D layers): an input gradient "
                             "through the stem and surfaces over image space do not exist")

    def predict(self, x, nb_samples: int, y_true=None, loss_func=None):
        """(list of per-sample outputs, their mean); NaN outputs count as 0 (BayesianModel.py:106-129)."""
        import torch
        xd = self._device_rows(x)
        nb_samples = int(nb_samples)
        Wd = self.sample_weights_device(nb_samples)
        rows, plan = self._read_out_plan(len(xd), nb_samples)
        full, mean_full = self._walk_rows(len(xd), rows, lambda r0, cnt: plan.predict(Wd, xd[r0:r0 + cnt].contiguous()),
                                          row_axis=(1,))
        # one device-to-host copy of each result into pinned memory (the 40 MB sample tensor of 100 draws x 10 000 rows
        # moves at PCIe rate instead of through the driver's pageable staging); the NumPy views keep the buffers alive
        samples_h = torch.empty(full.shape, dtype=torch.float32, pin_memory=True)
        mean_h = torch.empty(mean_full.shape, dtype=torch.float32, pin_memory=True)
        samples_h.copy_(full, non_blocking=True)
        mean_h.copy_(mean_full, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        samples = samples_h.numpy()
        mean = mean_h.numpy()
        self._model.set_flat(Wd[-1].cpu().numpy())      # the reference leaves the last draw assigned
        return [Array(s) for s in samples], Array(mean)

    def _read_out(self, x, nb_samples: int, moments: bool):
        """predict's draws, row cap and workspace rule; per row chunk MLPPlan.predict_moments (moments) or the mean-only
        MLPPlan.predict: device (mean (n, C), m2 (n, C, C) or None).  No sample tensor is formed."""
        xd = self._device_rows(x)       # (rows made on the device, as corruption_scores', stay there)
        nb_samples = int(nb_samples)
        Wd = self.sample_weights_device(nb_samples)
        rows, plan = self._read_out_plan(len(xd), nb_samples)

        def chunk(r0, cnt):
            xc = xd[r0:r0 + cnt].contiguous()
            return plan.predict_moments(Wd, xc) if moments else (plan.predict(Wd, xc, want_samples=False)[1], None)
        mean, m2 = self._walk_rows(len(xd), rows, chunk)
        self._model.set_flat(Wd[-1].cpu().numpy())      # the reference leaves the last draw assigned
        return mean, m2

    def predictive_moments(self, x, nb_samples: int):
        """(mean (n, C), m2 (n, C, C), nb_samples) as NumPy float32 arrays: the Monte-Carlo mean of ``predict`` (bit for
        bit, for the same draws) and, per row, the sum over the draws of p p^T -- all that
        Metrics.classification_uncertainty needs of the draws.  Computed on the device by pyz_predict_moments: the
        (nb_samples, n, C) sample tensor is neither written nor copied to the host."""
        mean, m2 = self._read_out(x, nb_samples, True)
        return mean.cpu().numpy(), m2.cpu().numpy(), int(nb_samples)

    def predictive_mean(self, x, nb_samples: int):
        """(n, C) NumPy float32: ``predict``'s mean alone (MLPPlan.predict without the sample tensor)."""
        return self._read_out(x, nb_samples, False)[0].cpu().numpy()

    def _surface(self, n, nb_samples, column, want_cols, rows_of):
        """The read-out behind predictive_surface / grid_surface: predict's draws, row cap and workspace rule; per row
        chunk ``rows_of(r0, count)`` hands the device rows and MLPPlan.predict_surface reads them out.  NumPy
        (cols (S, n) or None, mean (n, C), top (n,), cls (n,) int32, ent (n,))."""
        nb_samples, n = int(nb_samples), int(n)
        if n < 1 or nb_samples < 1:
            raise ValueError("rows and nb_samples must be positive")
        C_out = int(self._model.dims[-1])
        if not 0 <= int(column) < C_out:
            raise ValueError(f"column {column} outside [0, {C_out})")
        Wd = self.sample_weights_device(nb_samples)
        rows, plan = self._read_out_plan(n, nb_samples)
        out = self._walk_rows(n, rows, lambda r0, cnt: plan.predict_surface(Wd, rows_of(r0, cnt), column=column,
                                                                            want_cols=want_cols), row_axis=(1,))
        self._model.set_flat(Wd[-1].cpu().numpy())      # the reference leaves the last draw assigned
        return tuple(None if t is None else t.cpu().numpy() for t in out)

    def predictive_surface(self, x, nb_samples: int, column: int = 0, want_cols: bool = False):
        """(cols, mean, top, cls, ent) as NumPy arrays for the rows of x: mean (n, C) = ``predict``'s mean (bit for bit,
        for the same draws); of each mean row q (one output: the pair (1 - m, m)) top = max q, cls = argmax q (int32),
        ent = -sum q log(q + 1e-5) in float32, raw; cols (nb_samples, n) = column `column` of every draw's prediction, or
        None.  Computed on the device by pyz_predict_surface: the sample tensor is neither written nor copied."""
        self._refuse_conv("predictive_surface")
        xd = self._device_rows(x)
        return self._surface(len(xd), nb_samples, column, want_cols, lambda r0, cnt: xd[r0:r0 + cnt].contiguous())

    def grid_surface(self, basis, a0, da, n1, b0, db, n2, nb_samples: int, column: int = 0, want_cols: bool = False):
        """``predictive_surface`` on the n1 x n2 grid u_i = a0 + i da, v_j = b0 + j db ('ij' row order), each grid point
        mapped to input space as u * basis[:, 0] + v * basis[:, 1] (basis (d, 2): the identity for a 2-D input, the PCA
        axes otherwise).  The weights are drawn once; the grid is walked in row chunks under predict's row cap and
        workspace rule, each chunk's rows made on the device (pyz_grid_rows) and read out there (pyz_predict_surface):
        no grid row and no sample tensor reaches the host.  NumPy: cols (nb_samples, n1 * n2) or None, mean, top, cls,
        ent."""
        self._refuse_conv("grid_surface")
        import torch
        from .. import engine
        basis = np.ascontiguousarray(np.asarray(basis, dtype=np.float32))
        if basis.ndim != 2 or basis.shape != (int(self._model.dims[0]), 2):
            raise ValueError(f"basis must be ({int(self._model.dims[0])}, 2), not {basis.shape}")
        n1, n2 = int(n1), int(n2)
        if n1 < 1 or n2 < 1:
            raise ValueError(f"the grid must be at least 1 x 1, not {n1} x {n2}")
        bd = torch.as_tensor(basis).cuda()
        return self._surface(n1 * n2, nb_samples, column, want_cols,
                             lambda r0, cnt: engine.grid_rows(bd, a0, da, n1, b0, db, n2, r0, cnt))

    def corruption_scores(self, x, y, image_shape, kind: int, severities=(1, 2, 3, 4, 5), nb_samples: int = 100,
                          regression: bool = False, pixel_max: float = 255.0, seed: int = 0):
        """Per-severity error (NumPy float64, one entry per severity) of the Monte-Carlo mean prediction on the rows of x
        under corruption `kind` (0..8 of Robustness.py:10-93 on images of image_shape = (h, w, ch); 9, the regression noise
        of :16-19, on rows of any length): the fraction of rows wrong (classification, :253-254), or sklearn's
        root_mean_squared_error, per output column, then their plain average (regression, :251).  The clean rows are
        uploaded once; the len(severities) * n corrupted rows are made on the device (pyz_corrupt_rows), read out like
        ``predict`` (the same row cap and workspace rule, fresh draws per call) and scored there (pyz_score_rows): no
        image and no mean leaves the device."""
        import torch
        from .. import engine
        x, y = _host(x), _host(y)
        n = len(x)
        if n < 1 or len(y) != n:
            raise ValueError("x and y must hold the same, positive number of rows")
        xd = self._device_rows(x)
        sev = [int(s) for s in severities]
        C_out = int(self._model.dims[-1])
        if regression:
            yd = torch.as_tensor(np.ascontiguousarray(y.astype(np.float32).reshape(n, -1))).cuda()
            if yd.shape[1] != C_out:
                raise ValueError(f"targets must be (rows, {C_out})")
        else:
            yd = torch.as_tensor(np.ascontiguousarray(y.reshape(-1).astype(np.int32))).cuda()
        rows = engine.corrupt_rows(xd, image_shape, kind, sev, pixel_max=pixel_max, quantise=True, seed=seed)
        # the moments form of the read-out: k_predict_moments normalises each draw's rows itself and keeps the sums in
        # registers, where the mean-only form first has k_predict_rows write every normalised (draw, row) back for
        # k_predict_mean to read again; the mean is the same bits (include/pyz.h), the second moment is dropped
        mean, _ = self._read_out(rows.reshape(len(sev) * n, -1), nb_samples, True)
        score = engine.score_rows(mean.reshape(len(sev), n, C_out).contiguous(), yd, 1 if regression else 0)
        score = score.cpu().numpy().astype(np.float64)
        if regression:
            return np.sqrt(score / n).mean(axis=1)
        return score / n

    def adversarial_examples(self, x, y, loss: str, epsilon: float, nb_samples: int):
        """(x_adv, x_grad) as NumPy arrays: x_grad = sum over nb_samples weight draws of the gradient of the draw's mean
        loss over all rows with respect to x, x_adv = x + epsilon * sign(x_grad) -- the FGSM step of
        Robustness.adversarial_robustness (visualisations/Robustness.py:127-137), the sum over draws inside one device
        GEMM (pyz_input_grad).  loss: "scce" (y = integer labels), "mse" (y = targets) or "bce" (y = 0/1
        labels or targets in [0, 1], one per row)."""
        self._refuse_conv("adversarial_examples")
        import torch
        from ..engine import MLPSpec
        if loss not in ("scce", "mse", "bce"):
            raise ValueError(f"loss must be 'scce', 'mse' or 'bce', not {loss!r}")
        spec = MLPSpec(tuple(self._model.spec.dims), tuple(self._model.spec.acts), loss)
        if (loss == "scce") != (spec.acts[-1] == "softmax") or \
                (loss == "bce" and (spec.dims[-1] != 1 or spec.acts[-1] != "sigmoid")):
            raise ValueError("'scce' needs a softmax last layer, 'mse' a last layer that is not softmax, "
                             "'bce' a last layer of one sigmoid unit")
        x, y = _host(x), _host(y)
        shape, n = x.shape, len(x)
        if loss == "scce":
            y = np.ascontiguousarray(y.reshape(-1).astype(np.int32))
        else:
            y = np.ascontiguousarray(y.astype(np.float32).reshape(n, -1))
        if n < 1 or len(y) != n:
            raise ValueError("x and y must hold the same, positive number of rows")
        nb_samples = int(nb_samples)
        Wd = self.sample_weights_device(nb_samples)
        rows, plan = self._read_out_plan(n, nb_samples, spec)       # the workspace rule of predict
        xd, yd = self._device_rows(x), torch.as_tensor(y).cuda()

        def chunk(r0, cnt):
            # a chunk's mean loss is over its own rows: chunk_rows / n of it is its share of the mean over all n
            return plan.input_grad(Wd, xd[r0:r0 + cnt].contiguous(), yd[r0:r0 + cnt].contiguous(), scale=cnt / n,
                                   epsilon=float(epsilon))[:2]
        grad, adv = self._walk_rows(n, rows, chunk)
        plan.check_finite()
        return adv.cpu().numpy().reshape(shape), grad.cpu().numpy().reshape(shape)

    # ------------------------------------------------------------------ persistence
    @classmethod
    def load(cls, model_path: str, custom_distribution_register=None) -> "BayesianModel":
        from ..distributions import Mixture, MultivariateNormalDiagPlusLowRank, Sampled
        from ..distributions.tf import TensorflowProbabilityDistribution
        register = {"Sampled": Sampled, "TensorflowProbabilityDistribution": TensorflowProbabilityDistribution,
                    "MultivariateNormalDiagPlusLowRank": MultivariateNormalDiagPlusLowRank, "Mixture": Mixture}
        register.update(custom_distribution_register or {})
        with open(os.path.join(model_path, "config.json"), "r") as f:
            bayesian_model = BayesianModel(f.read())
        layers_intervals = []
        with open(os.path.join(model_path, "layers_config.txt"), "r") as f:
            n_intervals = int(f.readline())
            for _ in range(n_intervals):
                layers_intervals.append((f.readline()[:-1], int(f.readline()), int(f.readline())))
        for i, (name, start, end) in enumerate(layers_intervals):
            dist = register[name].load(os.path.join(model_path, "distribution" + str(i)))
            bayesian_model.apply_distribution(dist, start, end)
        return bayesian_model

    def _empty_folder(self, path):
        from .._fs import empty_folder
        empty_folder(path)

    def store(self, model_path: str):
        """Directory format of BayesianModel.py:177-203: config.json, layers_config.txt
        (count, then ClassName / start / end per interval), distribution<i>/."""
        if not os.path.exists(model_path):
            os.makedirs(model_path)
        self._empty_folder(model_path)
        with open(os.path.join(model_path, "config.json"), "w") as f:
            f.write(self._model.to_json())
        with open(os.path.join(model_path, "layers_config.txt"), "w") as f:
            f.write(str(len(self._layers_dtbn_intervals)) + '\n')
            for (start, end), d in zip(self._layers_dtbn_intervals, self._distributions):
                f.write(d.__class__.__name__ + '\n' + str(start) + '\n' + str(end) + '\n')
        for i, d in enumerate(self._distributions):
            os.mkdir(os.path.join(model_path, "distribution" + str(i)))
            d.store(os.path.join(model_path, "distribution" + str(i)))

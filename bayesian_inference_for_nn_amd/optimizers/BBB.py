"""Bayes-by-Backprop (mirrors Pyesian/optimizers/BBB.py:12-326).  Hyperparameters: batch_size,
lr, alpha, [pi]; kwargs prior, [prior2].  Device step: sample w + log-likelihood sums, fused
forward/backward, closed-form mu/rho update (BBB.py:152-201).

Extension: kwarg lanes = [P dicts or HyperParameters] trains P posteriors that differ by any of lr, alpha, pi (the rest from
the optimizer's hyper-parameters) as the rows of ONE particle-batched step (pyz_bbb_lanes_step / _run): the points of the
grid searches the reference's BBB drivers walk one training at a time (hyperparameters.BBBGridObjective).  Each lane's prior
is mixed with its own pi by the formula below, and its posterior starts from its own mixed prior.  lane_seeds = "shared"
(the default): every lane draws eps from the optimizer's seed, so lanes differ by their hyper-parameters alone; "distinct":
lane c draws from seed + c -- the reference's n_runs repeats as lanes of equal hyper-parameters.  In lanes mode the
nine-in-ten validation forward of BBB.py:203-209 is not run (it reports and never feeds the update): train_losses /
val_losses stay empty, lane_costs() has the (steps, P, 4) costs, lane_scores() scores every lane on a split, lane_results()
gives one result per lane, and result() refuses."""

import math

import numpy as np

from ..distributions import GaussianPrior, tfd
from ..distributions.tf import TensorflowProbabilityDistribution
from ..nn import BayesianModel
from .Optimizer import DeviceScalar, Optimizer


class ResultTuple(tuple):
    """``BBB.result()`` returns ``(model, train_losses, val_losses)`` (BBB.py:323) while several
    reference drivers call ``.predict`` / ``.store`` on the return value (BBB_mnist.py:53,59):
    unpacks as three items and forwards attribute access to the model."""

    def __getattr__(self, name):
        return getattr(self[0], name)


def softplus(x):
    return np.logaddexp(0.0, x)


LANE_KEYS = ("lr", "alpha", "pi")


def mix_prior(prior, prior2, pi):
    """BBB.py:265-270: the scalar prior mixed with prior2 by pi (the sign of the first prior's rho is kept)."""
    sign = prior._std_dev / abs(prior._std_dev)
    return GaussianPrior(prior._mean * pi + prior2._mean * (1 - pi),
                         sign * math.sqrt((prior._std_dev * pi) ** 2 + (prior2._std_dev * (1 - pi)) ** 2))


def resolve_lanes(lanes, hyperparameters, prior=None):
    """lanes (dicts or HyperParameters, any of LANE_KEYS each) as a list of dicts with all three keys, the missing ones from
    `hyperparameters` (pi: 1 where it has none).  ValueError for an unknown key, an empty list, or a lane that sets pi under
    a list-valued prior (BBB.py:265 mixes scalar priors only)."""
    out = []
    for lane in lanes:
        given = dict(lane._params) if hasattr(lane, "_params") else dict(lane)
        unknown = sorted(k for k in given if k not in LANE_KEYS and not (k == "batch_size" and hasattr(lane, "_params")))
        if unknown:
            raise ValueError(f"a lane sets {unknown}: only {list(LANE_KEYS)} differ between lanes")
        if "pi" in given and prior is not None and not prior.is_scalar():
            raise ValueError("a lane sets pi under a list-valued prior: pi mixes scalar priors only")
        base = {"lr": getattr(hyperparameters, "lr"), "alpha": getattr(hyperparameters, "alpha"),
                "pi": getattr(hyperparameters, "pi") if hasattr(hyperparameters, "pi") else 1}
        out.append({k: given[k] if k in given else base[k] for k in LANE_KEYS})
    if not out:
        raise ValueError("lanes must hold at least one lane")
    return out


class BBB(Optimizer):
    def __init__(self):
        super().__init__()
        self._lanes = None
        self._lane_stride = 0
        self._lr = None
        self._alpha = None
        self._prior2 = None
        self._prior = None
        self._step = 0
        self.val_losses = []
        self.train_losses = []

    def compile_extra_components(self, **kwargs):
        import torch
        from ..engine import MLPPlan
        self._prior = kwargs["prior"]
        self._prior2 = kwargs["prior2"] if "prior2" in kwargs else GaussianPrior(0.0, 0.0)
        self._lr = self._hyperparameters.lr
        self._pi = getattr(self._hyperparameters, 'pi', None) if hasattr(self._hyperparameters, 'pi') else 1
        self._batch_size = int(self._hyperparameters.batch_size)
        self._lanes, self._lane_stride = None, 0
        if kwargs.get("lanes") is not None:
            return self._compile_lanes(**kwargs)
        if isinstance(self._prior._mean, int) or isinstance(self._prior._mean, float):      # BBB.py:265-270
            sign = self._prior._std_dev / abs(self._prior._std_dev)
            self._prior = GaussianPrior(
                self._prior._mean * self._pi + self._prior2._mean * (1 - self._pi),
                sign * math.sqrt((self._prior._std_dev * self._pi) ** 2 + (self._prior2._std_dev * (1 - self._pi)) ** 2),
            )
        self._alpha = self._hyperparameters.alpha
        self._setup_backend(seed=kwargs.get("seed"))
        self._base_model = self._net
        self._dataset_setup()
        self._priors_list = self._prior.get_model_priors(self._net)
        mu, rho = self._prior.flat(self._net)                   # BBB.py:277-296: posterior <- prior (raw rho)
        self._mu = torch.as_tensor(mu.copy()).cuda()
        self._rho = torch.as_tensor(rho.copy()).cuda()
        if self._prior.is_scalar():
            self._pm, self._pr, self._pm_vec, self._pr_vec = float(self._prior._mean), float(self._prior._std_dev), None, None
        else:                                                   # list-valued prior: no mixing (BBB.py:265), per-element vectors
            self._pm, self._pr = 0.0, 1.0
            self._pm_vec, self._pr_vec = self._mu.clone(), self._rho.clone()
        self._w = torch.zeros(self._D, device="cuda")
        self._cost = torch.zeros(4, device="cuda")
        self._weight_layers_indices = self._layer_indices()
        # validation split, forwarded with the sampled weights on 9 steps out of 10 (BBB.py:203-209)
        vx, vy = self._dataset.valid_data.as_numpy()
        self._val_n = len(vx)
        if self._val_n > 0:
            self._vx = torch.as_tensor(np.ascontiguousarray(np.asarray(vx, np.float32).reshape(len(vx), -1))).cuda()
            self._vy = self._labels_to_device(vy)
            self._val_plan = MLPPlan(self._spec, max_batch=self._val_n)

    # ------------------------------------------------------------------ lanes
    def _compile_lanes(self, **kwargs):
        """lanes = [...]: a plan for P particles and a (P, D) state; lane c's mu / rho start from its own mixed prior."""
        import torch
        from .. import parallel
        if parallel.world_info()[1] > 1:
            raise ValueError("lanes run on one rank (a grid is not split over ranks)")
        mode = kwargs.get("lane_seeds", "shared")
        if mode not in ("shared", "distinct"):
            raise ValueError("lane_seeds must be 'shared' or 'distinct'")
        self._lanes = resolve_lanes(kwargs["lanes"], self._hyperparameters, self._prior)
        self._lane_stride = 0 if mode == "shared" else 1
        P = len(self._lanes)
        self._alpha = self._hyperparameters.alpha
        self._setup_backend(seed=kwargs.get("seed"), max_particles=P)
        self._base_model = self._net
        self._dataset_setup()
        if self._prior.is_scalar():
            priors = [mix_prior(self._prior, self._prior2, lane["pi"]) for lane in self._lanes]
            self._pm_vec = self._pr_vec = None
        else:                                                   # list-valued prior: shared by the lanes, never mixed
            priors = [self._prior] * P
        flats = [p.flat(self._net) for p in priors]
        self._lane_priors = priors
        self._mu = torch.as_tensor(np.stack([m for m, _ in flats]).astype(np.float32)).cuda()
        self._rho = torch.as_tensor(np.stack([r for _, r in flats]).astype(np.float32)).cuda()
        if self._prior.is_scalar():
            pm, pr = [float(p._mean) for p in priors], [float(p._std_dev) for p in priors]
        else:
            pm, pr = [0.0] * P, [1.0] * P
            self._pm_vec, self._pr_vec = self._mu[0].clone(), self._rho[0].clone()
        f32 = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.float32))
        self._lane_tabs = (f32([lane["lr"] for lane in self._lanes]), f32([lane["alpha"] for lane in self._lanes]), f32(pm), f32(pr))
        self._w = torch.zeros((P, self._D), device="cuda")
        self._cost = torch.zeros((P, 4), device="cuda")
        self._loss_cols = 4 * P                                 # {cost, data loss, log q - log p, -} per lane and step
        self._lane_costs = []
        self._weight_layers_indices = self._layer_indices()
        self._val_n = 0                                         # no validation forward in lanes mode

    def _step_lanes(self, save_document_path=None):
        self._step += 1
        idx, b, _ = self._next_batch()
        self._plan.bbb_lanes_step(self._mu, self._rho, self._w, self._x_dev, self._y_dev, *self._lane_tabs, self._step,
                                  self._seed, self._cost, seed_stride=self._lane_stride, batch=b, row_idx=idx,
                                  prior_mean_vec=self._pm_vec, prior_rho_vec=self._pr_vec)
        self._lane_costs.append(self._cost.clone()[None])
        likelihood = DeviceScalar(self._lane_costs[-1], 0)      # lane 0's cost
        if save_document_path != None:
            self._append_loss(save_document_path, str(float(likelihood)) + "\n")
        return likelihood

    def lane_costs(self):
        """float32 (steps, P, 4) on the device: {cost, data loss, log q - log p, 0} of every lane and step so far."""
        import torch
        if self._lanes is None:
            raise ValueError("lane_costs() needs lanes (compile with lanes=[...])")
        if not self._lane_costs:
            return torch.zeros((0, len(self._lanes), 4), device="cuda")
        if len(self._lane_costs) > 1:
            self._lane_costs = [torch.cat(self._lane_costs)]
        return self._lane_costs[0]

    def lane_results(self):
        """One ResultTuple per lane, each built as result() builds its one from that lane's mu and rho."""
        if self._lanes is None:
            raise ValueError("lane_results() needs lanes (compile with lanes=[...])")
        mu, rho = self._mu.cpu().numpy(), self._rho.cpu().numpy()
        return [self._result_from(mu[c], rho[c]) for c in range(len(self._lanes))]

    def _split_device(self, split):
        import torch
        if split not in ("valid", "test", "train"):
            raise ValueError("split must be 'valid', 'test' or 'train'")
        if split == "train":
            return self._x_dev, self._y_dev
        cache = self.__dict__.setdefault("_split_dev", {})
        if split not in cache:
            x, y = getattr(self._dataset, split + "_data").as_numpy()
            cache[split] = (torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(len(x), -1))).cuda(),
                            self._labels_to_device(y))
        return cache[split]

    def lane_scores(self, split="valid", weights="mu", nb_samples=100):
        """Every lane's score on a split of the data set, computed where the weights live: {"loss": [...], "error": [...],
        "n": rows}, float64 (P,) each.  weights = "mu": the posterior means through plan.lane_scores in chunks of max_batch
        rows (the mean per-row loss and the misclassified fraction, 0 for regression; the host adds the chunks' float64
        sums in chunk order).  weights = "predictive": what the reference's drivers score, predict(x, nb_samples) of each
        lane's posterior -- per lane and layer nb_samples draws of Normal(mu, softplus(rho)) from the stream of tfd.seed
        (engine.sample_normal_rows, drawn as lane_results()[c].predict draws them), the plan's predict mean, and
        engine.score_rows; "loss" is not defined for it (None), and for regression "error" is the mean squared error."""
        import torch
        from .. import engine
        if self._lanes is None:
            raise ValueError("lane_scores() needs lanes (compile with lanes=[...])")
        if weights not in ("mu", "predictive"):
            raise ValueError("weights must be 'mu' or 'predictive'")
        x_dev, y_dev = self._split_device(split)
        n, P = int(x_dev.shape[0]), len(self._lanes)
        if n < 1:
            raise ValueError(f"the {split} split is empty")
        if weights == "mu":
            B = self._plan.max_batch
            sums, errs = [], []
            for r0 in range(0, n, B):
                s, e = self._plan.lane_scores(self._mu, x_dev[r0:r0 + B], y_dev[r0:r0 + B])
                sums.append(s)
                errs.append(e)
            loss = np.zeros(P, dtype=np.float64)
            wrong = np.zeros(P, dtype=np.int64)
            for s, e in zip(torch.stack(sums).cpu().numpy(), torch.stack(errs).cpu().numpy()):
                loss = loss + s
                wrong = wrong + e
            return {"loss": loss / n, "error": wrong.astype(np.float64) / n, "n": n}
        nb_samples = int(nb_samples)
        if nb_samples < 1:
            raise ValueError("nb_samples must be at least 1")
        rows = min(n, 16384)
        per = 2 * sum(int(d) for d in self._spec.dims[1:])
        chunk_s = max(1, min(nb_samples, (1 << 29) // max(1, rows * per)))
        plan = engine.make_plan(self._spec, max_batch=rows, max_particles=chunk_s)
        mu, rho = self._mu.cpu().numpy(), self._rho.cpu().numpy()
        regression = self._loss_kind == "mse"
        labels = y_dev if regression else y_dev.reshape(-1).to(torch.int32).contiguous()
        W = torch.empty((nb_samples, self._D), device="cuda")
        out = np.zeros(P, dtype=np.float64)
        for c in range(P):
            for sl in self._spec.layer_slices():                # one Normal per layer, drawn twice, the second kept
                loc = torch.as_tensor(mu[c][sl].copy()).cuda()
                scale = torch.as_tensor(softplus(rho[c][sl]).astype(np.float32)).cuda()
                tfd.take_device_draws(nb_samples)
                engine.sample_normal_rows(W, sl.start, loc, scale, tfd._dev_seed, tfd.take_device_draws(nb_samples))
            total = 0.0
            for r0 in range(0, n, rows):
                mean = plan.predict(W, x_dev[r0:r0 + rows].contiguous(), want_samples=False)[1]
                yc = labels[r0:r0 + rows].contiguous()
                total += float(engine.score_rows(mean[None].contiguous(), yc, 1 if regression else 0).sum().item())
            out[c] = total / (n * (self._spec.dims[-1] if regression else 1))
        plan.close()
        return {"loss": None, "error": out, "n": n}

    def step(self, save_document_path=None):
        if self._lanes is not None:
            return self._step_lanes(save_document_path)
        self._step += 1
        idx, b, _ = self._next_batch()
        self._plan.bbb_step(self._mu, self._rho, self._w, self._x_dev, self._y_dev, self._lr, self._alpha,
                            self._pm, self._pr, self._step, self._seed, self._cost, batch=b, row_idx=idx,
                            prior_mean_vec=self._pm_vec, prior_rho_vec=self._pr_vec)
        likelihood = DeviceScalar(self._cost.clone(), 0)
        if save_document_path != None:
            self._append_loss(save_document_path, str(float(likelihood)) + "\n")
        if self._step % 10:                                     # BBB.py:203: nine steps out of ten, as written
            if self._val_n > 0:
                vloss, _ = self._val_plan.loss_grad(self._w, self._vx, self._vy, want_grad=False)
                self.val_losses.append(DeviceScalar(vloss, 0))
            self.train_losses.append(likelihood)
        return likelihood

    # ------------------------------------------------------------------ quiet train(): device-resident runs
    _loss_cols = 4                                              # {cost, data loss, log q - log p, -} per step

    def _reserve_resident(self, n_steps: int):
        """The validation losses of the run ride along with the costs: a slot per step."""
        import torch
        super()._reserve_resident(n_steps)
        if getattr(self, "_res_val", None) is None or self._res_val.shape[0] < self._res_cap:
            self._res_val = torch.zeros(self._res_cap, device="cuda")

    def _resident_supported(self):
        return self._lanes is not None or self._fused_head()    # (the lanes run takes unfused heads as well)

    def _resident_launch(self, nb_iterations):
        """pyz_bbb_run: batches assembled one step ahead, the validation forward of BBB.py:203-209 inside the run.  Equal
        to the per-step loop bit for bit."""
        lr, step0 = self._lr, self._step + 1
        if self._lanes is not None:                             # pyz_bbb_lanes_run, no validation forward
            def launch(idx, costs, sizes, s0):
                self._plan.bbb_lanes_run(self._mu, self._rho, self._w, self._x_dev, self._y_dev, idx, sizes, *self._lane_tabs,
                                         step0 + s0, self._seed, costs, seed_stride=self._lane_stride, slot0=s0,
                                         prior_mean_vec=self._pm_vec, prior_rho_vec=self._pr_vec)
            return launch
        lr, has_val = float(lr), self._val_n > 0

        def launch(idx, costs, sizes, s0):
            self._plan.bbb_run(self._mu, self._rho, self._w, self._x_dev, self._y_dev, idx, sizes, [lr] * len(sizes),
                               self._alpha, self._pm, self._pr, step0 + s0, self._seed, costs, use_graph=True,
                               slot0=s0, prior_mean_vec=self._pm_vec, prior_rho_vec=self._pr_vec,
                               val_plan=self._val_plan if has_val else None, val_x=self._vx if has_val else None,
                               val_y=self._vy if has_val else None, val_losses_out=self._res_val if has_val else None)
        return launch

    def _after_resident(self, nb_iterations, costs):
        if self._lanes is not None:
            self._lane_costs.append(costs.clone().view(nb_iterations, len(self._lanes), 4))
            self._cost.copy_(self._lane_costs[-1][-1])
            self._step += nb_iterations
            return
        costs, vals = costs.clone(), self._res_val[:nb_iterations].clone()
        for i in range(nb_iterations):
            if (self._step + 1 + i) % 10:                       # BBB.py:203: nine steps out of ten, as written
                if self._val_n > 0:
                    self.val_losses.append(DeviceScalar(vals, i))
                self.train_losses.append(DeviceScalar(costs, 4 * i))
        self._cost[:4].copy_(costs[-1])
        self._step += nb_iterations

    def update_parameters_step(self):
        pass

    def result(self):
        if self._lanes is not None:
            raise ValueError("result() is ONE posterior: lanes differ by their hyper-parameters "
                             "(lane_results() gives one result per lane)")
        return self._result_from(self._mu.cpu().numpy(), self._rho.cpu().numpy())

    def _result_from(self, mu, rho):
        model = BayesianModel(self._model_config)
        for sl, layer_idx in zip(self._spec.layer_slices(), self._weight_layers_indices):
            dist = TensorflowProbabilityDistribution(tfd.Normal(mu[sl].copy(), softplus(rho[sl]).astype(np.float32)))
            model.apply_distribution(dist, layer_idx, layer_idx)
        return ResultTuple((model, self.train_losses, self.val_losses))

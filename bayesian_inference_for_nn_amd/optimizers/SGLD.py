"""Stochastic Gradient Langevin Dynamics (mirrors Pyesian/optimizers/SGLD.py:14-166).
Hyperparameters: batch_size, lr_upper, lr_lower, lr_gamma.  One fused device step: forward,
loss, backward and the noise + parameter + running-moment update (three kernel launches).

Extension: kwarg n_chains = P > 1 runs P independent chains on one GPU in one particle-batched step (the reference has one
chain).  Chain c of rank r has the seed base + r P + c for its Philox noise stream and for its Glorot start, so chain 0 of
rank 0 starts where the one-chain optimizer with the same seed starts.  Each chain is a valid SGLD chain with its own noise
and its own start, but the chains of a rank see the SAME minibatches (the rank's own): their gradient noise is shared, only
the injected Langevin noise and the initial point are independent.  result() pools the chains' running moments,
chain_results() gives one model per chain, r_hat() the Gelman-Rubin statistic between the chains.

Extension: kwarg lanes = [P dicts or HyperParameters] runs P chains that differ by their learning-rate schedule (any of
lr_upper, lr_lower, lr_gamma; the rest from the optimizer's hyper-parameters) in the same particle-batched step: the points
of a hyper-parameter grid side by side (hyperparameters.GridOptimizer).  lane_seeds = "shared" (the default): every lane
starts from chain 0's Glorot draw and draws the noise of the optimizer's seed, so lanes differ by their hyper-parameters
alone (common random numbers); "distinct": the starts and seeds of n_chains.  lane_scores() scores every lane on a split on
the device; chain_results() gives one model per lane; result() and r_hat() refuse (pooling over different hyper-parameters
means nothing)."""

import numpy as np

from ..distributions import tfd
from ..distributions.tf import TensorflowProbabilityDistribution
from ..nn import BayesianModel
from .Optimizer import DeviceScalar, Optimizer


def pool_chain_moments(mean, sq_mean):
    """Running moments of P chains with equal step counts, pooled by parallel.merge_moment_chains' rule
    sum_c n_c m_c / sum_c n_c = the average over chains, accumulated in float64.  mean, sq_mean: (P, D) arrays;
    returns two float64 (D,) arrays."""
    mean, sq_mean = np.asarray(mean, dtype=np.float64), np.asarray(sq_mean, dtype=np.float64)
    return mean.sum(axis=0) / mean.shape[0], sq_mean.sum(axis=0) / sq_mean.shape[0]


def gelman_rubin(mean, sq_mean, n: int):
    """Gelman-Rubin R-hat per parameter from the running moments of P chains of n draws each ((P, D) arrays), in float64:
    W = mean_c[(sq_c - mean_c^2) n / (n - 1)], B / n = var_c(mean_c, ddof=1), R-hat = sqrt(((n - 1) / n W + B / n) / W).
    A parameter no chain moved (W = 0) gives NaN."""
    mean, sq_mean = np.asarray(mean, dtype=np.float64), np.asarray(sq_mean, dtype=np.float64)
    if mean.ndim != 2 or mean.shape[0] < 2:
        raise ValueError("r_hat needs at least two chains")
    if n < 2:
        raise ValueError("r_hat needs at least two steps per chain")
    n = float(n)
    W = ((sq_mean - mean ** 2) * (n / (n - 1.0))).mean(axis=0)
    B_over_n = mean.var(axis=0, ddof=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(((n - 1.0) / n * W + B_over_n) / W)


LANE_KEYS = ("lr_upper", "lr_lower", "lr_gamma")


def resolve_lanes(lanes, hyperparameters):
    """lanes (dicts or HyperParameters, any of LANE_KEYS each) as a list of dicts with all three keys, the missing ones
    from `hyperparameters`."""
    out = []
    for lane in lanes:
        given = dict(lane._params) if hasattr(lane, "_params") else dict(lane)
        unknown = sorted(k for k in given if k not in LANE_KEYS and not (k == "batch_size" and hasattr(lane, "_params")))
        if unknown:
            raise ValueError(f"a lane sets {unknown}: only {list(LANE_KEYS)} differ between lanes")
        out.append({k: given[k] if k in given else getattr(hyperparameters, k) for k in LANE_KEYS})
    if not out:
        raise ValueError("lanes must hold at least one lane")
    return out


def lane_lr_table(lanes, nb_iterations, n0, n_steps):
    """The rates of steps n0 .. n0 + n_steps - 1 of every lane, float32 (n_steps, P): column c is SGLD._init_sgld_lr's
    schedule lr(step) = a (b + step)^-gamma with lr(0) = lr_upper, lr(nb_iterations) = lr_lower for lane c's three
    numbers (dicts with LANE_KEYS), evaluated in float64 as there and rounded once."""
    steps = n0 + np.arange(n_steps, dtype=np.float64)
    n = nb_iterations
    cols = []
    for lane in lanes:
        upper, lower, gamma = lane["lr_upper"], lane["lr_lower"], lane["lr_gamma"]
        l_g = np.power(lower, 1.0 / gamma)
        u_g = np.power(upper, 1.0 / gamma)
        b = -(n * l_g) / (l_g - u_g)
        a = upper * np.power(b, gamma)
        cols.append(np.asarray(a * np.power((b + steps), -gamma)).astype(np.float32))
    return np.ascontiguousarray(np.stack(cols, axis=1))


class SGLD(Optimizer):
    def __init__(self):
        super().__init__()
        self._n_chains = 1
        self._lanes = None
        self._lane_stride = 1
        self._n = None
        self._running_loss = None
        self._lr_upper = None
        self._lr_lower = None
        self._lr_gamma = None
        self._lr = None

    def _init_sgld_lr(self):
        """SGLD.py:112-118: lr(step) = a (b + step)^-gamma, lr(0) = lr_upper, lr(n) = lr_lower."""
        n = self._nb_iterations
        l_g = np.power(self._lr_lower, 1.0 / self._lr_gamma)
        u_g = np.power(self._lr_upper, 1.0 / self._lr_gamma)
        b = -(n * l_g) / (l_g - u_g)
        a = self._lr_upper * np.power(b, self._lr_gamma)
        self._lr = lambda step: a * np.power((b + step), -self._lr_gamma)

    def compile_extra_components(self, **kwargs):
        import torch
        self._batch_size = int(self._hyperparameters.batch_size)
        self._lr_upper = self._hyperparameters.lr_upper
        self._lr_lower = self._hyperparameters.lr_lower
        self._lr_gamma = self._hyperparameters.lr_gamma
        self._lanes, self._lane_stride = None, 1
        if kwargs.get("lanes") is not None:
            return self._compile_lanes(**kwargs)
        self._n_chains = int(kwargs.get("n_chains", 1))
        if self._n_chains < 1:
            raise ValueError("n_chains must be at least 1")
        if self._n_chains > 1:
            return self._compile_chains(**kwargs)
        self._setup_backend(seed=kwargs.get("seed"))
        self._merge_ranks = bool(kwargs.get("merge_ranks", True))
        self._base_model = self._net
        self._dataset_setup()
        self._theta = torch.as_tensor(self._net.weights_flat.copy()).cuda()
        self._mean_dev = torch.zeros(self._D, device="cuda")       # SGLD.py:97-110
        self._sq_mean_dev = torch.zeros(self._D, device="cuda")
        self._loss_dev = torch.zeros(1, device="cuda")
        self._running_dev = torch.zeros(1, device="cuda")
        self._weight_layers_indices = self._layer_indices()
        self._n = 0
        self._running_loss = 0

    def _compile_lanes(self, **kwargs):
        """lanes = [...]: the (P, D) state of n_chains = P, one learning-rate schedule per row."""
        from .. import parallel
        if "n_chains" in kwargs:
            raise ValueError("lanes and n_chains exclude each other: the lanes are the chains")
        if parallel.world_info()[1] > 1:
            raise ValueError("lanes run on one rank (a grid is not split over ranks)")
        mode = kwargs.get("lane_seeds", "shared")
        if mode not in ("shared", "distinct"):
            raise ValueError("lane_seeds must be 'shared' or 'distinct'")
        self._lanes = resolve_lanes(kwargs["lanes"], self._hyperparameters)
        self._lane_stride = 0 if mode == "shared" else 1
        self._n_chains = len(self._lanes)
        self._compile_chains(shared_start=(mode == "shared"), **kwargs)

    def _lane_rates(self, n0, n_steps):
        return lane_lr_table(self._lanes, self._nb_iterations, n0, n_steps)

    def _compile_chains(self, shared_start=False, **kwargs):
        """n_chains = P > 1: a plan for P particles and a (P, D) state; chain c starts from the Glorot draw of its own seed
        (shared_start: every row from chain 0's)."""
        import torch
        from ..nn.model import model_from_json
        P = self._n_chains
        self._setup_backend(seed=kwargs.get("seed"), max_particles=P, chains_per_rank=P)   # self._seed = base + rank * P
        self._merge_ranks = bool(kwargs.get("merge_ranks", True))
        self._base_model = self._net
        self._dataset_setup()
        starts = [self._net.weights_flat.copy()]               # chain 0: reset_glorot(default_rng(self._seed)), done by the backend
        for c in range(1, P):
            if shared_start:
                starts.append(starts[0].copy())
                continue
            scratch = model_from_json(self._model_config)
            scratch.reset_glorot(np.random.default_rng(self._seed + c))
            starts.append(scratch.weights_flat.copy())
        self._theta = torch.as_tensor(np.stack(starts).astype(np.float32)).cuda()
        self._mean_dev = torch.zeros((P, self._D), device="cuda")
        self._sq_mean_dev = torch.zeros((P, self._D), device="cuda")
        self._loss_dev = torch.zeros(P, device="cuda")
        self._loss_cols = P                                    # a loss per chain (lane) and step
        self._running_dev = torch.zeros(1, device="cuda")
        self._weight_layers_indices = self._layer_indices()
        self._n = 0
        self._running_loss = 0

    def _step_chains(self, save_document_path=None):
        idx, b, _ = self._next_batch()
        if self._lanes is not None:
            self._plan.sgld_lanes_step(self._theta, self._mean_dev, self._sq_mean_dev, self._x_dev, self._y_dev,
                                       self._lane_rates(self._n, 1)[0], self._n, self._seed, self._loss_dev,
                                       seed_stride=self._lane_stride, batch=b, row_idx=idx)
        else:
            lr = float(self._lr(self._n))
            self._plan.sgld_chains_step(self._theta, self._mean_dev, self._sq_mean_dev, self._x_dev, self._y_dev, lr, self._n,
                                        self._seed, self._loss_dev, batch=b, row_idx=idx)
        self._running_dev += self._loss_dev.mean()             # the mean over chains of the batch loss
        if save_document_path != None:
            self._append_loss(save_document_path, str(float(self._loss_dev.mean().item())))
        self._n += 1
        return DeviceScalar(self._running_dev.clone(), 0, 1.0 / self._n)

    def step(self, save_document_path=None):
        """One step; returns the running mean over steps of the batch loss (with n_chains > 1: of its mean over chains)
        as a DeviceScalar -- nothing synchronises until somebody reads it."""
        if self._n_chains > 1 or self._lanes is not None:
            return self._step_chains(save_document_path)
        idx, b, _ = self._next_batch()
        lr = float(self._lr(self._n))
        self._plan.sgld_step(self._theta, self._mean_dev, self._sq_mean_dev, self._x_dev, self._y_dev, lr, self._n,
                             self._seed, self._loss_dev, batch=b, row_idx=idx)
        self._running_dev += self._loss_dev                        # SGLD.py:58
        if save_document_path != None:
            self._append_loss(save_document_path, str(float(self._loss_dev.item())))
        self._n += 1
        return DeviceScalar(self._running_dev.clone(), 0, 1.0 / self._n)

    def train(self, nb_iterations: int, loss_save_document_path: str = None, model_save_frequency: int = None,
              model_save_path: str = None, weights_and_biases_log=False):
        self._nb_iterations = nb_iterations
        self._init_sgld_lr()
        super().train(nb_iterations, loss_save_document_path, model_save_frequency, model_save_path,
                      weights_and_biases_log)

    # ------------------------------------------------------------------ quiet train(): device-resident runs
    def _resident_supported(self):
        return True                                                # pyz_sgld_run and the rows runs take unfused models

    def _resident_launch(self, nb_iterations):
        if self._lanes is not None:
            rates = self._lane_rates(self._n, nb_iterations)

            def launch(idx, losses, sizes, s0):
                self._plan.sgld_lanes_run(self._theta, self._mean_dev, self._sq_mean_dev, self._x_dev, self._y_dev, idx, sizes,
                                          rates[s0:s0 + len(sizes)], self._n + s0, self._seed, losses,
                                          seed_stride=self._lane_stride, slot0=s0)
            return launch
        lrs = np.asarray(self._lr(self._n + np.arange(nb_iterations, dtype=np.float64))).astype(np.float32).tolist()
        run = self._plan.sgld_chains_run if self._n_chains > 1 else self._plan.sgld_run

        def launch(idx, losses, sizes, s0):
            run(self._theta, self._mean_dev, self._sq_mean_dev, self._x_dev, self._y_dev, idx, sizes,
                lrs[s0:s0 + len(sizes)], self._n + s0, self._seed, losses, use_graph=True, slot0=s0)
        return launch

    def _after_resident(self, nb_iterations, losses):
        # a (P, D) state has a loss per chain and step: a step adds their mean; the sum runs over epochs (SGLD.py:58)
        self._fold_run(losses if self._loss_cols is None else losses.mean(dim=1))
        self._n += nb_iterations
        self.last_losses = losses.clone()          # the buffer itself is reused by the next run

    def update_parameters_step(self):
        return super().update_parameters_step()

    def _model_from(self, mean, sq_mean, theta) -> BayesianModel:
        """result()'s model from host float32 moments and weights: per layer Normal(loc = mean, scale = sq_mean - mean^2)."""
        model = BayesianModel(self._model_config)
        for sl, layer_idx in zip(self._spec.layer_slices(), self._weight_layers_indices):
            dist = TensorflowProbabilityDistribution(tfd.Normal(mean[sl].copy(), (sq_mean[sl] - mean[sl] ** 2).copy()))
            model.apply_distribution(dist, layer_idx, layer_idx)
        model._model.set_flat(theta)
        return model

    def chain_results(self):
        """One BayesianModel per chain of this rank, each built as result() builds its one from that chain's moments and
        weights (no pooling, no merge across ranks)."""
        mean, sq, theta = self._mean_dev.cpu().numpy(), self._sq_mean_dev.cpu().numpy(), self._theta.cpu().numpy()
        if mean.ndim == 1:
            mean, sq, theta = mean[None, :], sq[None, :], theta[None, :]
        return [self._model_from(mean[c], sq[c], theta[c]) for c in range(self._n_chains)]

    def lane_scores(self, split="valid", weights="theta"):
        """Every lane's score on a split of the data set, computed where the weights live: {"loss": the mean per-row loss,
        float64 (P,), "error": the misclassified fraction, float64 (P,) (0 for regression), "n": the rows}.  weights:
        "theta" (the current point) or "mean" (the running mean).  The split goes through plan.lane_scores in chunks of
        max_batch rows; the host adds the chunks' float64 sums in chunk order."""
        import torch
        if split not in ("valid", "test", "train"):
            raise ValueError("split must be 'valid', 'test' or 'train'")
        if weights not in ("theta", "mean"):
            raise ValueError("weights must be 'theta' or 'mean'")
        w = self._theta if weights == "theta" else self._mean_dev
        if w.dim() == 1:
            w = w[None, :]
        if split == "train":
            x_dev, y_dev = self._x_dev, self._y_dev
        else:
            cache = self.__dict__.setdefault("_split_dev", {})
            if split not in cache:
                x, y = getattr(self._dataset, split + "_data").as_numpy()
                cache[split] = (torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(len(x), -1))).cuda(),
                                self._labels_to_device(y))
            x_dev, y_dev = cache[split]
        n, B = int(x_dev.shape[0]), self._plan.max_batch
        if n < 1:
            raise ValueError(f"the {split} split is empty")
        sums, errs = [], []
        for r0 in range(0, n, B):
            s, e = self._plan.lane_scores(w, x_dev[r0:r0 + B], y_dev[r0:r0 + B])
            sums.append(s)
            errs.append(e)
        loss = np.zeros(w.shape[0], dtype=np.float64)
        wrong = np.zeros(w.shape[0], dtype=np.int64)
        for s, e in zip(torch.stack(sums).cpu().numpy(), torch.stack(errs).cpu().numpy()):
            loss = loss + s
            wrong = wrong + e
        return {"loss": loss / n, "error": wrong.astype(np.float64) / n, "n": n}

    def r_hat(self):
        """Gelman-Rubin R-hat of every parameter between this rank's chains, float64 (D,), from the running moments (see
        gelman_rubin).  The moments run from step 0: there is no burn-in, so the chains' different starts count as
        between-chain variance and R-hat comes down only as the run outgrows them.  ValueError for fewer than two chains
        or fewer than two steps."""
        if self._lanes is not None:
            raise ValueError("r_hat compares chains of ONE posterior: lanes differ by their hyper-parameters")
        if self._n_chains < 2:
            raise ValueError("r_hat needs at least two chains (compile with n_chains >= 2)")
        return gelman_rubin(self._mean_dev.cpu().numpy(), self._sq_mean_dev.cpu().numpy(), int(self._n))

    def _result_chains(self) -> BayesianModel:
        import torch
        P = self._n_chains
        mean64, sq64 = pool_chain_moments(self._mean_dev.cpu().numpy(), self._sq_mean_dev.cpu().numpy())
        mean, sq_mean = mean64.astype(np.float32), sq64.astype(np.float32)
        if self._world > 1 and self._merge_ranks:
            # every rank pools its P chains first; the ranks' pools then merge with P n draws each
            from .. import parallel
            mean_dev, sq_dev, self.pooled_steps = parallel.merge_moment_chains(
                torch.as_tensor(mean).cuda(), torch.as_tensor(sq_mean).cuda(), P * self._n)
            mean, sq_mean = mean_dev.cpu().numpy(), sq_dev.cpu().numpy()
        return self._model_from(mean, sq_mean, self._theta[0].cpu().numpy())     # the net's weights: chain 0's

    def result(self) -> BayesianModel:
        """The posterior model.  With n_chains > 1 the chains' moments are pooled first (pool_chain_moments), the net's
        weights are chain 0's.  With lanes there is nothing to pool: chain_results() has one model per lane."""
        if self._lanes is not None:
            raise ValueError("result() pools chains of ONE posterior: lanes differ by their hyper-parameters "
                             "(chain_results() gives one model per lane)")
        if self._n_chains > 1:
            return self._result_chains()
        model = BayesianModel(self._model_config)
        mean_dev, sq_dev = self._mean_dev, self._sq_mean_dev
        if self._world > 1 and self._merge_ranks:
            # one chain per rank (no data-path collective): the running moments pool with the chains' step counts
            from .. import parallel
            mean_dev, sq_dev, self.pooled_steps = parallel.merge_moment_chains(mean_dev, sq_dev, self._n)
        mean = mean_dev.cpu().numpy()
        sq_mean = sq_dev.cpu().numpy()
        for sl, layer_idx in zip(self._spec.layer_slices(), self._weight_layers_indices):
            # Normal(loc = mean, scale = sq_mean - mean^2): the variance is used as the scale, as written (SGLD.py:151-154)
            dist = TensorflowProbabilityDistribution(tfd.Normal(mean[sl].copy(), (sq_mean[sl] - mean[sl] ** 2).copy()))
            model.apply_distribution(dist, layer_idx, layer_idx)
        model._model.set_flat(self._theta.cpu().numpy())
        return model

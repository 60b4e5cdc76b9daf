"""Hamiltonian Monte Carlo on the full training split (mirrors Pyesian/optimizers/HMC.py:13-187).
Hyperparameters: m, L, epsilon; kwarg prior (GaussianPrior).  Extension: kwarg n_chains runs
that many independent chains in one particle-batched launch (the reference has one).

A quiet train() (verbose off) is one device-resident run (pyz_hmc_run): every uniform of the burn-in and the sampling
proposals is drawn up front with random.random() in the step loop's order, the proposals run back to back on the
optimizer's stream with the sample record of HMC.py:92-103 kept on the device ((n_chains, nb_iterations + 1, D) rows,
their frequencies and counts), and after ONE join `fold_run_record` rebuilds the chain lists, the counters and
last_stats exactly as the step loop leaves them.  The step loop is taken instead when PYZ_HMC_RUN=0, when the record
would exceed PYZ_HMC_RUN_MAX_BYTES (default 1 GiB), or when the library refuses the shape; step(), a verbose train(),
result() and the multi-rank merge are the same either way."""

import os
import random

import numpy as np

from ..distributions import Sampled
from ..nn import BayesianModel
from .Optimizer import DeviceScalar, Optimizer


GAVE_UP = ("an HMC proposal gave up waiting for its row-slice workgroups (k_hmc_resident: the grid was not "
           "resident at once); set PYZ_HMC_RESIDENT=0 for one launch per gradient evaluation")


def fold_run_record(stats_all, count, freq, samples):
    """The device record of a run's sampling proposals as the step loop's bookkeeping (HMC.py:75-77, 92-103).
    stats_all: (n, P, 8) statistics of the n sampling proposals; count: (P,) rows recorded per chain; freq: (P, cap);
    samples: per chain, a sequence of at least count[c] rows.  Returns (chain_samples, chain_freq, accepted_runs,
    total_runs): per chain the first count[c] rows and their frequencies as lists, the accepted proposals of chain 0
    and n.  The record must be the one the statistics describe: a chain has 1 + its accepted proposals as rows (none
    before the first sampling proposal) and its frequencies add up to 1 + n."""
    stats_all = np.asarray(stats_all)
    n, P = stats_all.shape[0], stats_all.shape[1]
    chain_samples, chain_freq = [], []
    for c in range(P):
        k = int(count[c])
        accepted = int(np.count_nonzero(stats_all[:, c, 0])) if n else 0
        fr = [int(v) for v in np.asarray(freq[c])[:k]]
        if k != (1 + accepted if n else 0) or sum(fr) != (1 + n if n else 0):
            raise RuntimeError(f"HMC run: chain {c} recorded {k} rows with frequencies adding up to {sum(fr)}; its {n} "
                               f"proposals accepted {accepted}")
        chain_samples.append([samples[c][i] for i in range(k)])
        chain_freq.append(fr)
    accepted_runs = int(np.count_nonzero(stats_all[:, 0, 0])) if n else 0
    return chain_samples, chain_freq, accepted_runs, n


class HMC(Optimizer):
    def __init__(self):
        super().__init__()
        self._nb_burn_epoch = 10
        self._prior = None
        self._frequency = None
        self._samples = None
        self._epsilon = None
        self._L = None
        self._m = None
        self._total_runs = 0
        self._accepted_runs = 0
        self._current_loss = 0

    def compile_extra_components(self, **kwargs):
        import torch
        self._m = self._hyperparameters.m
        self._L = self._hyperparameters.L
        self._epsilon = self._hyperparameters.epsilon
        self._n_chains = int(kwargs.get("n_chains", 1))
        self._merge_ranks = bool(kwargs.get("merge_ranks", True))
        self._setup_backend(seed=kwargs.get("seed"), max_particles=self._n_chains, full_batch=True)
        self._model = self._net
        self._samples = []
        self._frequency = []
        self._prior_spec = kwargs["prior"]
        self._prior = self._prior_spec.get_model_priors(self._net)
        if "nb_burn_epoch" in kwargs:
            # the reference tests one key and reads another (HMC.py:61-62); kept as written
            self._nb_burn_epoch = kwargs["nb_burn_epochs"]
        self._dataset_setup()
        # q <- prior mean (HMC.py:69-72)
        mu, sg = self._prior_spec.flat(self._net)
        if self._prior_spec.is_scalar():
            self._prior_mean, self._prior_sigma = float(self._prior_spec._mean), float(self._prior_spec._std_dev)
            self._pm_vec = self._ps_vec = None
        else:                                                  # per-layer lists: per-element vectors on the device
            self._prior_mean, self._prior_sigma = 0.0, 1.0
            self._pm_vec, self._ps_vec = torch.as_tensor(mu.copy()).cuda(), torch.as_tensor(sg.copy()).cuda()
        self._q = torch.as_tensor(np.repeat(mu[None, :], self._n_chains, axis=0).copy()).cuda()
        self._stats = torch.zeros((self._n_chains, 8), device="cuda")
        # proposals run on a stream of their own: the library replays the launch sequence of a sliced
        # proposal as a hipGraph, and the legacy default stream cannot be captured
        self._stream = torch.cuda.Stream()
        self._step_count = 0
        self._chain_samples = [[] for _ in range(self._n_chains)]
        self._chain_freq = [[] for _ in range(self._n_chains)]
        # proposals are launched back to back; their statistics and state snapshots are read later, in
        # batches (the accept / reject decision itself is taken on the device)
        self._pending = []
        self._defer = False                                   # only train() defers the bookkeeping reads

    def step(self, save_document_path=None, sampling=True, burning=False):
        import torch
        if sampling and any(len(f) == 0 for f in self._chain_freq):
            self._resolve_pending()                             # the start of a chain must see the earlier bookkeeping
            for c in range(self._n_chains):                    # HMC.py:75-77: records the starting q
                if len(self._chain_freq[c]) == 0:
                    self._chain_freq[c].append(1)
                    self._chain_samples[c].append(self._q[c].clone())
        uniforms = [random.random() for _ in range(self._n_chains)]      # HMC.py:91 host Mersenne Twister
        if self._defer:                                       # train() already runs on the side stream
            stats_snap, q_snap = self._launch(uniforms, sampling, burning)
        else:
            self._stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self._stream):
                stats_snap, q_snap = self._launch(uniforms, sampling, burning)
            torch.cuda.current_stream().wait_stream(self._stream)
        self._step_count += 1
        self._total_runs += 1
        self._pending.append((stats_snap, q_snap, sampling))
        if self._verbose or not self._defer or len(self._pending) >= 64:   # (the progress bar shows every step's accept rate)
            self._resolve_pending()
        return DeviceScalar(stats_snap, 1)

    def _launch(self, uniforms, sampling, burning):
        self._plan.hmc_step(self._q, self._x_dev, self._y_dev, int(self._L), self._epsilon, self._m, self._prior_mean,
                            self._prior_sigma, uniforms, self._step_count, self._seed, self._stats, burning=burning,
                            prior_mean_vec=self._pm_vec, prior_sigma_vec=self._ps_vec)
        return self._stats.clone(), (self._q.clone() if sampling else None)

    def _resolve_pending(self):
        """Acceptance bookkeeping (HMC.py:92-104) of the proposals launched since the last call: one
        device-to-host copy for all of them."""
        import torch
        if not self._pending:
            return
        self._stream.synchronize()
        all_stats = torch.stack([p[0] for p in self._pending]).cpu().numpy()
        if (all_stats[:, :, 7] < 0).any():
            raise RuntimeError(GAVE_UP)
        for (_, q_snap, sampling), stats in zip(self._pending, all_stats):
            accepted = stats[:, 0] != 0
            if accepted[0]:
                self._accepted_runs += 1
            if sampling:
                for c in range(self._n_chains):
                    if accepted[c]:                             # HMC.py:92-96
                        self._chain_freq[c].append(1)
                        self._chain_samples[c].append(q_snap[c])
                    else:                                       # HMC.py:102-103
                        self._chain_freq[c][-1] += 1
            self.last_stats = stats
        self._pending = []
        self._frequency, self._samples = self._chain_freq[0], self._chain_samples[0]

    def train(self, nb_iterations: int, loss_save_document_path: str = None, model_save_frequency: int = None,
              model_save_path: str = None):
        import torch
        self._resolve_pending()
        if not self._verbose and self._train_resident(nb_iterations):
            return
        self._defer = True
        self._stream.wait_stream(torch.cuda.current_stream())
        try:
            with torch.cuda.stream(self._stream):            # (graph replay needs a stream of its own)
                self._train(nb_iterations)
        finally:
            self._defer = False
            self._resolve_pending()
            torch.cuda.current_stream().wait_stream(self._stream)

    def _train(self, nb_iterations: int):
        self._accepted_runs = 0
        self._total_runs = 0
        nb_burn_epoch = self._nb_burn_epoch
        for i in range(nb_burn_epoch):                          # HMC.py:111-116
            loss = self.step(sampling=False, burning=True)
            if self._verbose:                                   # (reading the loss waits for the proposal)
                accept_rate = self._accepted_runs / self._total_runs
                self._print_progress((i + 1) / nb_burn_epoch, suffix="HMC - Burning", loss=loss.numpy().item(),
                                     accept_rate=accept_rate, bar_length=20)
        self._new_progress_line()
        self._resolve_pending()
        self._accepted_runs = 0
        self._total_runs = 0
        self._chain_freq = [[] for _ in range(self._n_chains)]
        self._chain_samples = [[] for _ in range(self._n_chains)]
        for i in range(nb_iterations):                          # HMC.py:121-125
            loss = self.step(sampling=True, burning=False)
            if self._verbose:
                accept_rate = self._accepted_runs / self._total_runs
                self._print_progress((i + 1) / nb_iterations, suffix="HMC - Sampling", loss=loss.numpy().item(),
                                     accept_rate=accept_rate, bar_length=20)
        self._new_progress_line()
        self._resolve_pending()

    def _train_resident(self, nb_iterations: int) -> bool:
        """_train as one pyz_hmc_run (see the module docstring).  False: no proposal has run, q is untouched and no
        uniform is consumed; the step loop has to run."""
        import torch
        from .._lib import PyzError
        if os.environ.get("PYZ_HMC_RUN", "1") == "0":
            return False
        P, D = self._n_chains, int(self._q.shape[1])
        nb_burn, n = int(self._nb_burn_epoch), max(int(nb_iterations), 0)
        cap = n + 1
        if nb_burn + n <= 0 or 4 * P * cap * D > int(os.environ.get("PYZ_HMC_RUN_MAX_BYTES", str(1 << 30))):
            return False
        rng_state = random.getstate()
        uniforms = [[random.random() for _ in range(P)] for _ in range(nb_burn + n)]     # HMC.py:91, the step loop's order
        self._stream.wait_stream(torch.cuda.current_stream())
        try:
            with torch.cuda.stream(self._stream):
                stats_all = torch.zeros((nb_burn + n, P, 8), device="cuda")
                samples = torch.empty((P, cap, D), device="cuda")
                freq = torch.zeros((P, cap), dtype=torch.int32, device="cuda")
                count = torch.zeros((P,), dtype=torch.int32, device="cuda")
                fail = torch.zeros((4,), dtype=torch.int32, device="cuda")
                self._plan.hmc_run(self._q, self._x_dev, self._y_dev, int(self._L), self._epsilon, self._m, self._prior_mean,
                                   self._prior_sigma, uniforms, nb_burn, self._step_count, self._seed, stats_all, samples,
                                   freq, count, fail, prior_mean_vec=self._pm_vec, prior_sigma_vec=self._ps_vec)
        except PyzError as e:
            if e.code not in (-1, -2):                        # (an argument or shape the library refuses: no proposal has run, q is untouched)
                raise
            random.setstate(rng_state)
            return False
        self._stream.synchronize()                            # the one join of the run
        torch.cuda.current_stream().wait_stream(self._stream)
        self._step_count += nb_burn + n
        stats_host, fail_host = stats_all.cpu().numpy(), fail.cpu().numpy()
        if fail_host[1] > 0 or (stats_host[:, :, 7] < 0).any():
            raise RuntimeError(GAVE_UP)
        if fail_host[0] > 0:
            raise RuntimeError("HMC run: the sample record ran out of rows")
        count_host = count.cpu().numpy()
        rows = [samples[c, :int(count_host[c])].clone() for c in range(P)]     # (the record itself is released)
        self._chain_samples, self._chain_freq, self._accepted_runs, self._total_runs = fold_run_record(
            stats_host[nb_burn:], count_host, freq.cpu().numpy(), rows)
        self.last_stats = stats_host[-1]
        self._frequency, self._samples = self._chain_freq[0], self._chain_samples[0]
        return True

    def update_parameters_step(self):
        pass

    def result(self) -> BayesianModel:
        """Sampled(samples, frequencies) over all layers (HMC.py:176-187); with n_chains > 1 the chains'
        samples and frequencies are concatenated (independent chains of the same posterior)."""
        self._resolve_pending()
        samples, freqs = [], []
        for c in range(self._n_chains):
            samples += [s.cpu().numpy() for s in self._chain_samples[c]]
            freqs += list(self._chain_freq[c])
        if self._world > 1 and self._merge_ranks:
            # independent chains on every rank: one Sampled posterior over all of them (every rank gets it)
            from .. import parallel
            samples, freqs = parallel.merge_sampled_chains(samples, freqs)
        distribution = Sampled(samples, freqs)
        posterior_model = BayesianModel(self._model_config)
        posterior_model.apply_distribution(distribution, 0, len(self._net.layers) - 1)
        return posterior_model

"""Host-side handle over the C-ABI plan (`pyz_mlp`).  torch is used for device
memory and streams only; every numerical operation is a HIP kernel of libpyz.so.
All shapes are validated here before a pointer is handed to a kernel."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import ACT, LOSS, SWEEP, check, ptr

SVGD_GROUPS = 8   # PYZ_SVGD_GROUPS of include/pyz.h


@dataclass(frozen=True)
class MLPSpec:
    """dims = [in, h1, ..., out]; acts[l] = Keras activation name of Dense layer l."""
    dims: Tuple[int, ...]
    acts: Tuple[str, ...]
    loss: str = "scce"

    @property
    def n_layers(self):
        return len(self.acts)

    @property
    def n_params(self):
        return sum((i + 1) * o for i, o in zip(self.dims[:-1], self.dims[1:]))

    def layer_slices(self):
        out, off = [], 0
        for i, o in zip(self.dims[:-1], self.dims[1:]):
            out.append(slice(off, off + (i + 1) * o))
            off += (i + 1) * o
        return out

    def variable_shapes(self):
        """[(kernel shape, bias shape)] per layer, in flat order."""
        return [((i, o), (o,)) for i, o in zip(self.dims[:-1], self.dims[1:])]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gamma(gamma) -> float:
    """Fixed RBF bandwidth, or None / "median" for the median heuristic (PYZ_SVGD_GAMMA_MEDIAN)."""
    if gamma is None or gamma == "median":
        return _lib.GAMMA_MEDIAN
    if not float(gamma) > 0.0:
        raise ValueError("gamma must be positive, or None / 'median' for the median heuristic")
    return float(gamma)


def _f32(t: torch.Tensor, shape=None, name="tensor"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name} must be a CUDA(HIP) torch tensor")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise TypeError(f"{name} must be contiguous float32")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


class _NetPlan:
    """What a Dense plan and a conv plan share: the argument checks and output allocations of forward, loss_grad, the SGD
    and SWAG steps and the read-outs.  A class supplies n_in (the width of a row of x), _handles (what its library
    functions take first), _FN (their names) and _lib_predict."""

    def _net(self, name, *args):
        check(getattr(self.lib, self._FN[name])(*self._handles, *args, _stream()))

    def _check_xy(self, x, y, row_idx, batch):
        _f32(x, name="x")
        if x.dim() != 2 or x.shape[1] != self.n_in:
            raise ValueError(f"x must be (rows, {self.n_in})")
        n_rows = x.shape[0]
        if row_idx is not None:
            if row_idx.dtype != torch.int32 or not row_idx.is_cuda or not row_idx.is_contiguous():
                raise TypeError("row_idx must be a contiguous CUDA int32 tensor")
            if row_idx.numel() < batch:
                raise ValueError("row_idx holds fewer entries than the batch")
        elif batch > n_rows:
            raise ValueError("batch exceeds the rows of x")
        if y is not None:
            if self.spec.loss == "scce":
                if y.dtype != torch.int32 or not y.is_cuda or y.numel() != n_rows:
                    raise TypeError("labels must be CUDA int32, one per row of x")
            else:
                _f32(y, name="y")
                if y.numel() != n_rows * self.spec.dims[-1]:
                    raise ValueError("targets must be (rows, out)")
        if not (1 <= batch <= self.max_batch):
            raise ValueError(f"batch {batch} outside [1, {self.max_batch}]")

    def _particles(self, theta):
        P = 1 if theta.dim() == 1 else int(theta.shape[0])
        _f32(theta, name="theta")
        if theta.numel() != P * self.D or not 1 <= P <= self.max_particles:
            raise ValueError(f"theta must be ({self.D},) or (P <= {self.max_particles}, {self.D})")
        return P

    @staticmethod
    def _batch(batch, x, row_idx):
        return int(batch if batch is not None else (row_idx.numel() if row_idx is not None else x.shape[0]))

    # ------------------------------------------------------------------ G1-G3
    def forward(self, theta, x, batch=None, row_idx=None):
        P = self._particles(theta)
        batch = self._batch(batch, x, row_idx)
        self._check_xy(x, None, row_idx, batch)
        out = torch.empty((P, batch, self.spec.dims[-1]), dtype=torch.float32, device=self.device)
        self._net("forward", ptr(theta), P, ptr(x), ptr(row_idx), batch, ptr(out))
        return out

    def loss_grad(self, theta, x, y, batch=None, row_idx=None, want_grad=True, grad_out=None):
        P = self._particles(theta)
        batch = self._batch(batch, x, row_idx)
        self._check_xy(x, y, row_idx, batch)
        grad = None
        if want_grad:
            grad = grad_out if grad_out is not None else torch.empty((P, self.D), dtype=torch.float32, device=self.device)
            _f32(grad, (P, self.D), "grad_out")
        loss = torch.empty((P,), dtype=torch.float32, device=self.device)
        self._net("loss_grad", ptr(theta), P, ptr(x), ptr(y), ptr(row_idx), batch, ptr(grad), ptr(loss))
        return loss, grad

    # ------------------------------------------------------------------ S1
    def sgd_step(self, theta, x, y, lr, loss_out, batch=None, row_idx=None):
        _f32(theta, (self.D,), "theta")
        batch = self._batch(batch, x, row_idx)
        self._check_xy(x, y, row_idx, batch)
        self._net("sgd_step", ptr(theta), ptr(x), ptr(y), ptr(row_idx), batch, float(lr), ptr(loss_out))

    def swag_step(self, theta, mean, sq_mean, dev_row, x, y, lr, n, update_moments, loss_out, batch=None, row_idx=None):
        for t, nm in ((theta, "theta"), (mean, "mean"), (sq_mean, "sq_mean")):
            _f32(t, (self.D,), nm)
        if dev_row is not None:
            _f32(dev_row, (self.D,), "dev_row")
        batch = self._batch(batch, x, row_idx)
        self._check_xy(x, y, row_idx, batch)
        self._net("swag_step", ptr(theta), ptr(mean), ptr(sq_mean), ptr(dev_row), ptr(x), ptr(y), ptr(row_idx), batch,
                  float(lr), int(n), 1 if update_moments else 0, ptr(loss_out))

    # ------------------------------------------------------------------ R1
    def _check_read_out(self, weights, x):
        _f32(weights, name="weights")
        if weights.dim() != 2 or weights.shape[1] != self.D or weights.shape[0] < 1:
            raise ValueError(f"weights must be (draws >= 1, {self.D})")
        self._check_xy(x, None, None, int(x.shape[0]) if x.dim() == 2 else 0)
        return int(weights.shape[0]), int(x.shape[0]), self.spec.dims[-1]

    def predict(self, weights, x, want_samples=True):
        """(samples (S, n, out) or None, mean (n, out)) of the draws `weights` (S, D) on the rows of x."""
        S, n, C_out = self._check_read_out(weights, x)
        samples = torch.empty((S, n, C_out), dtype=torch.float32, device=self.device) if want_samples else None
        mean = torch.empty((n, C_out), dtype=torch.float32, device=self.device)
        self._lib_predict(ptr(weights), S, ptr(x), n, ptr(samples), ptr(mean), None)
        return samples, mean

    def predict_moments(self, weights, x):
        """(mean (n, out), m2 (n, out, out)) of the draws `weights` (S, D) on the rows of x: mean is predict's mean bit for
        bit, m2[j] = sum over the draws of p p^T with p = predict's sample of row j.  One kernel per chunk of
        max_particles draws (pyz_predict_moments); the (S, n, out) sample tensor is never formed."""
        S, n, C_out = self._check_read_out(weights, x)
        mean = torch.empty((n, C_out), dtype=torch.float32, device=self.device)
        m2 = torch.empty((n, C_out, C_out), dtype=torch.float32, device=self.device)
        self._lib_predict(ptr(weights), S, ptr(x), n, None, ptr(mean), ptr(m2))
        return mean, m2


class MLPPlan(_NetPlan):
    """Owns one `pyz_mlp` handle (device workspace for up to max_batch rows x max_particles)."""

    _FN = {"forward": "pyz_mlp_forward", "loss_grad": "pyz_mlp_loss_grad", "sgd_step": "pyz_sgd_step",
           "swag_step": "pyz_swag_step"}
    n_in = property(lambda self: self.spec.dims[0])
    _handles = property(lambda self: (self.h,))

    def __init__(self, spec: MLPSpec, max_batch: int, max_particles: int = 1, device=None):
        if spec.loss == "bce" and (spec.dims[-1] != 1 or spec.acts[-1] != "sigmoid"):
            raise ValueError("BinaryCrossentropy needs a last layer of exactly one sigmoid unit, not "
                             f"{spec.dims[-1]} x '{spec.acts[-1]}'")
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("bayesian_inference_for_nn_amd needs an MI355X (no HIP device visible); there is no CPU path")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.spec, self.max_batch, self.max_particles = spec, int(max_batch), int(max_particles)
        dims = (C.c_int32 * len(spec.dims))(*spec.dims)
        acts = (C.c_int32 * len(spec.acts))(*[ACT[a] for a in spec.acts])
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.pyz_mlp_create(spec.n_layers, dims, acts, LOSS[spec.loss], self.max_batch,
                                          self.max_particles, C.byref(h)))
        self.h = h
        self.D = int(self.lib.pyz_mlp_param_count(h))
        assert self.D == spec.n_params

    def close(self):
        if getattr(self, "h", None):
            self.lib.pyz_mlp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ S1
    def adam_step(self, theta, m, v, x, y, lr, beta_1, beta_2, epoch, loss_out, denom_eps=1e-3, decay=0.0, batch=None,
                  row_idx=None):
        """ADAM.step (ADAM.py:42-84); VADAM's update with decay = denom_eps = lam / N.  m / v are the moment vectors;
        beta_1 / beta_2 go to the library as float64 (it rounds 1 - beta and 1 - beta^epoch to float32 once)."""
        for t, nm in ((theta, "theta"), (m, "m"), (v, "v")):
            _f32(t, (self.D,), nm)
        batch = int(batch if batch is not None else (row_idx.numel() if row_idx is not None else x.shape[0]))
        self._check_xy(x, y, row_idx, batch)
        check(self.lib.pyz_adam_step(self.h, ptr(theta), ptr(m), ptr(v), ptr(x), ptr(y), ptr(row_idx), batch, float(lr),
                                     float(beta_1), float(beta_2), int(epoch), float(denom_eps), float(decay),
                                     ptr(loss_out), _stream()))

    def vadam_perturb(self, theta, v, lam, num_data, step, seed, eps=None):
        """VADAM.step's perturbation (VADAM.py:59-65): theta += eps / sqrt(num_data (v + lam)); eps from the device
        Philox stream (seed, STREAM_VADAM, step) or the given (D,) tensor."""
        _f32(theta, (self.D,), "theta")
        _f32(v, (self.D,), "v")
        if eps is not None:
            _f32(eps, (self.D,), "eps")
        check(self.lib.pyz_vadam_perturb(self.h, ptr(theta), ptr(v), float(lam), float(num_data), int(step), int(seed),
                                         ptr(eps), _stream()))

    def bsam_step(self, theta, m, v, x, y, lr, beta_1, beta_2, lam, rho, gam, num_data, step, seed, loss_out, eps=None,
                  batch=None, row_idx=None):
        """BSAM.step (BSAM.py:46-119): perturbation (Philox stream (seed, STREAM_BSAM, step), or the given (D,) eps),
        first pass + ascent, second pass + update of m, v and theta.  loss_out: (2,) float32, receives l1 and l2;
        beta_1 / beta_2 go to the library as float64 (it rounds 1 - beta and 1 / num_data to float32 once)."""
        for t, nm in ((theta, "theta"), (m, "m"), (v, "v")):
            _f32(t, (self.D,), nm)
        _f32(loss_out, (2,), "loss_out")
        if eps is not None:
            _f32(eps, (self.D,), "eps")
        batch = int(batch if batch is not None else (row_idx.numel() if row_idx is not None else x.shape[0]))
        self._check_xy(x, y, row_idx, batch)
        check(self.lib.pyz_bsam_step(self.h, ptr(theta), ptr(m), ptr(v), ptr(x), ptr(y), ptr(row_idx), batch, float(lr),
                                     float(beta_1), float(beta_2), float(lam), float(rho), float(gam), float(num_data),
                                     int(step), int(seed), ptr(eps), ptr(loss_out), _stream()))

    # ------------------------------------------------------------------ L2/L3
    def sgld_step(self, theta, mean, sq_mean, x, y, lr, n, seed, loss_out, batch=None, row_idx=None, unit_noise=None):
        for t, nm in ((theta, "theta"), (mean, "mean"), (sq_mean, "sq_mean")):
            _f32(t, (self.D,), nm)
        if unit_noise is not None:
            _f32(unit_noise, (self.D,), "unit_noise")
        batch = int(batch if batch is not None else (row_idx.numel() if row_idx is not None else x.shape[0]))
        self._check_xy(x, y, row_idx, batch)
        check(self.lib.pyz_sgld_step(self.h, ptr(theta), ptr(mean), ptr(sq_mean), ptr(x), ptr(y), ptr(row_idx), batch,
                                     float(lr), int(n), int(seed), ptr(unit_noise), ptr(loss_out), _stream()))

    def sgld_run(self, theta, mean, sq_mean, x, y, row_idx, batch_sizes: Sequence[int], lrs: Sequence[float], n0, seed,
                 losses_out, use_graph=True, slot0=0):
        """row_idx: int32 (slots, max_batch) on the device; step s of this call uses slot slot0+s of
        row_idx / losses_out; batch_sizes / lrs: host sequences for the n_steps of this call."""
        for t, nm in ((theta, "theta"), (mean, "mean"), (sq_mean, "sq_mean")):
            _f32(t, (self.D,), nm)
        n_steps = len(batch_sizes)
        assert len(lrs) == n_steps and n_steps > 0
        self._check_xy(x, y, row_idx, 1)
        if slot0 < 0 or row_idx.numel() < (slot0 + n_steps) * self.max_batch:
            raise ValueError("row_idx must hold (slot0 + n_steps) * max_batch entries")
        _f32(losses_out, name="losses_out")
        assert losses_out.numel() >= slot0 + n_steps
        if any(int(b) < 1 or int(b) > self.max_batch for b in batch_sizes):
            raise ValueError("batch size outside the plan")
        bs = (C.c_int32 * n_steps)(*[int(b) for b in batch_sizes])
        lr = (C.c_float * n_steps)(*[float(v) for v in lrs])
        check(self.lib.pyz_sgld_run(self.h, ptr(theta), ptr(mean), ptr(sq_mean), ptr(x), ptr(y), ptr(row_idx), bs, lr,
                                    n_steps, int(n0), int(slot0), int(seed), ptr(losses_out), 1 if use_graph else 0,
                                    _stream()))

    def _check_chains(self, theta, mean, sq_mean):
        P = int(theta.shape[0]) if theta.dim() == 2 else 0
        if not 1 <= P <= self.max_particles:
            raise ValueError(f"theta must be (n_chains, {self.D}) with 1 <= n_chains <= {self.max_particles}")
        for t, nm in ((theta, "theta"), (mean, "mean"), (sq_mean, "sq_mean")):
            _f32(t, (P, self.D), nm)
        return P

    def _check_rows_step(self, P, x, y, loss_out, batch, row_idx, unit_noise):
        """The noise, the losses and the batch of one step of P chains or lanes; returns the batch size."""
        if unit_noise is not None:
            _f32(unit_noise, (P, self.D), "unit_noise")
        _f32(loss_out, (P,), "loss_out")
        batch = int(batch if batch is not None else (row_idx.numel() if row_idx is not None else x.shape[0]))
        self._check_xy(x, y, row_idx, batch)
        return batch

    def _check_rows_run(self, P, rows, x, y, row_idx, batch_sizes, losses_out, slot0):
        """The tables of a run of P chains or lanes (`rows`: "n_chains" / "n_lanes"); returns the c_int32 batch sizes."""
        n_steps = len(batch_sizes)
        self._check_xy(x, y, row_idx, 1)
        if slot0 < 0 or row_idx.numel() < (slot0 + n_steps) * self.max_batch:
            raise ValueError("row_idx must hold (slot0 + n_steps) * max_batch entries")
        _f32(losses_out, name="losses_out")
        if losses_out.numel() < (slot0 + n_steps) * P:
            raise ValueError(f"losses_out must hold (slot0 + n_steps) * {rows} entries")
        if any(int(b) < 1 or int(b) > self.max_batch for b in batch_sizes):
            raise ValueError("batch size outside the plan")
        return (C.c_int32 * n_steps)(*[int(b) for b in batch_sizes])

    def sgld_chains_step(self, theta, mean, sq_mean, x, y, lr, n, seed, loss_out, batch=None, row_idx=None, unit_noise=None):
        """One SGLD step of the n_chains rows of theta / mean / sq_mean (n_chains, D) on ONE shared batch; chain c draws
        the noise of seed + c (or row c of the (n_chains, D) unit_noise); loss_out: (n_chains,) float32."""
        P = self._check_chains(theta, mean, sq_mean)
        batch = self._check_rows_step(P, x, y, loss_out, batch, row_idx, unit_noise)
        check(self.lib.pyz_sgld_chains_step(self.h, ptr(theta), ptr(mean), ptr(sq_mean), P, ptr(x), ptr(y), ptr(row_idx),
                                            batch, float(lr), int(n), int(seed), ptr(unit_noise), ptr(loss_out), _stream()))

    def sgld_chains_run(self, theta, mean, sq_mean, x, y, row_idx, batch_sizes: Sequence[int], lrs: Sequence[float], n0, seed,
                        losses_out, use_graph=True, slot0=0):
        """n = len(batch_sizes) steps of sgld_chains_step without host work in between (see sgld_run for the tables);
        losses_out: float32 (slots, n_chains), step s writes row slot0 + s."""
        P = self._check_chains(theta, mean, sq_mean)
        n_steps = len(batch_sizes)
        assert len(lrs) == n_steps and n_steps > 0
        bs = self._check_rows_run(P, "n_chains", x, y, row_idx, batch_sizes, losses_out, slot0)
        lr = (C.c_float * n_steps)(*[float(v) for v in lrs])
        check(self.lib.pyz_sgld_chains_run(self.h, ptr(theta), ptr(mean), ptr(sq_mean), P, ptr(x), ptr(y), ptr(row_idx), bs,
                                           lr, n_steps, int(n0), int(slot0), int(seed), ptr(losses_out),
                                           1 if use_graph else 0, _stream()))

    def _check_members(self, theta, mean, sq_mean=None, dev=None):
        """The (n_members, D) state of SGD / SWAG members (dev: (n_members, k, D)); returns (n_members, k)."""
        P = int(theta.shape[0]) if theta.dim() == 2 else 0
        if not 1 <= P <= self.max_particles:
            raise ValueError(f"theta must be (n_members, {self.D}) with 1 <= n_members <= {self.max_particles}")
        for t, nm in ((theta, "theta"), (mean, "mean")) + (((sq_mean, "sq_mean"),) if dev is not None else ()):
            _f32(t, (P, self.D), nm)
        k = 0
        if dev is not None:
            _f32(dev, name="dev")
            if dev.dim() != 3 or dev.shape[0] != P or dev.shape[1] < 1 or dev.shape[2] != self.D:
                raise ValueError(f"dev must be ({P}, k, {self.D}) with k >= 1")
            k = int(dev.shape[1])
        return P, k

    def sgd_members_step(self, theta, mean, x, y, lr, n, update_mean, loss_out, batch=None, row_idx=None):
        """One SGD step of the n_members rows of theta (n_members, D) on ONE shared batch; with update_mean the rows of
        mean receive the new weights (SGD.py:78-84); loss_out: (n_members,) float32."""
        P, _ = self._check_members(theta, mean)
        batch = self._check_rows_step(P, x, y, loss_out, batch, row_idx, None)
        check(self.lib.pyz_sgd_members_step(self.h, ptr(theta), ptr(mean), P, ptr(x), ptr(y), ptr(row_idx), batch, float(lr),
                                            int(n), 1 if update_mean else 0, ptr(loss_out), _stream()))

    def sgd_members_run(self, theta, mean, frequency, x, y, row_idx, batch_sizes: Sequence[int], lrs: Sequence[float], n0,
                        losses_out, use_graph=True, slot0=0):
        """n = len(batch_sizes) steps of sgd_members_step without host work in between (see sgld_run for the tables): step
        s has count n0 + s and copies the weights to mean when frequency divides it; losses_out: float32
        (slots, n_members), step s writes row slot0 + s."""
        P, _ = self._check_members(theta, mean)
        n_steps = len(batch_sizes)
        if len(lrs) != n_steps or n_steps < 1:
            raise ValueError("one learning rate per step, at least one step")
        bs = self._check_rows_run(P, "n_members", x, y, row_idx, batch_sizes, losses_out, slot0)
        lr = (C.c_float * n_steps)(*[float(v) for v in lrs])
        check(self.lib.pyz_sgd_members_run(self.h, ptr(theta), ptr(mean), P, int(frequency), ptr(x), ptr(y), ptr(row_idx), bs,
                                           lr, n_steps, int(n0), int(slot0), ptr(losses_out), 1 if use_graph else 0,
                                           _stream()))

    def swag_members_step(self, theta, mean, sq_mean, dev, x, y, lr, n, update_moments, dev_col, loss_out, batch=None,
                          row_idx=None):
        """One SWAG step of the n_members rows of theta / mean / sq_mean (n_members, D) on ONE shared batch; dev is
        (n_members, k, D).  With update_moments the moments move and theta - mean goes to row dev_col of every member's
        block (dev_col None: to no row); loss_out: (n_members,) float32."""
        P, k = self._check_members(theta, mean, sq_mean, dev)
        col = -1 if dev_col is None else int(dev_col)
        if col >= k:
            raise ValueError(f"dev_col {col} outside the {k} rows of a member")
        batch = self._check_rows_step(P, x, y, loss_out, batch, row_idx, None)
        check(self.lib.pyz_swag_members_step(self.h, ptr(theta), ptr(mean), ptr(sq_mean), ptr(dev), k, P, ptr(x), ptr(y),
                                             ptr(row_idx), batch, float(lr), int(n), 1 if update_moments else 0, col,
                                             ptr(loss_out), _stream()))

    def swag_members_run(self, theta, mean, sq_mean, dev, frequency, x, y, row_idx, batch_sizes: Sequence[int],
                         lrs: Sequence[float], n0, losses_out, use_graph=True, slot0=0):
        """n = len(batch_sizes) steps of swag_members_step without host work in between: the hit steps and the deviation
        row follow from the count n0 + s on the device (the members started at count 0); losses_out: float32
        (slots, n_members), step s writes row slot0 + s."""
        P, k = self._check_members(theta, mean, sq_mean, dev)
        n_steps = len(batch_sizes)
        if len(lrs) != n_steps or n_steps < 1:
            raise ValueError("one learning rate per step, at least one step")
        bs = self._check_rows_run(P, "n_members", x, y, row_idx, batch_sizes, losses_out, slot0)
        lr = (C.c_float * n_steps)(*[float(v) for v in lrs])
        check(self.lib.pyz_swag_members_run(self.h, ptr(theta), ptr(mean), ptr(sq_mean), ptr(dev), k, int(frequency), P,
                                            ptr(x), ptr(y), ptr(row_idx), bs, lr, n_steps, int(n0), int(slot0),
                                            ptr(losses_out), 1 if use_graph else 0, _stream()))

    def _lane_rates(self, lrs, shape):
        """Host float32 rates of the lanes, C-contiguous, of the given shape ((P,) for a step, (n_steps, P) for a run)."""
        lr = np.ascontiguousarray(np.asarray(lrs, dtype=np.float32))
        if lr.shape != tuple(shape):
            raise ValueError(f"lane rates have shape {lr.shape}, expected {tuple(shape)}")
        return lr

    def _check_lanes(self, theta, mean, sq_mean, seed_stride):
        P = self._check_chains(theta, mean, sq_mean)
        if P > _lib.MAX_LANES:
            raise ValueError(f"at most {_lib.MAX_LANES} lanes per call")
        if seed_stride not in (0, 1):
            raise ValueError("seed_stride must be 0 (one noise stream for every lane) or 1 (seed + lane)")
        return P

    def sgld_lanes_step(self, theta, mean, sq_mean, x, y, lrs, n, seed, loss_out, seed_stride=0, batch=None, row_idx=None,
                        unit_noise=None):
        """sgld_chains_step with a rate per lane (lrs: P host floats) and the seed seed + c * seed_stride for lane c."""
        P = self._check_lanes(theta, mean, sq_mean, seed_stride)
        lr = self._lane_rates(lrs, (P,))
        batch = self._check_rows_step(P, x, y, loss_out, batch, row_idx, unit_noise)
        check(self.lib.pyz_sgld_lanes_step(self.h, ptr(theta), ptr(mean), ptr(sq_mean), P, ptr(x), ptr(y), ptr(row_idx), batch,
                                           lr.ctypes.data_as(C.POINTER(C.c_float)), int(n), int(seed), int(seed_stride),
                                           ptr(unit_noise), ptr(loss_out), _stream()))

    def sgld_lanes_run(self, theta, mean, sq_mean, x, y, row_idx, batch_sizes: Sequence[int], lrs, n0, seed, losses_out,
                       seed_stride=0, slot0=0):
        """n = len(batch_sizes) steps of sgld_lanes_step without host work in between (see sgld_chains_run); lrs: host
        (n_steps, P) rates, row s for step s; losses_out: float32 (slots, P), step s writes row slot0 + s."""
        P = self._check_lanes(theta, mean, sq_mean, seed_stride)
        n_steps = len(batch_sizes)
        if n_steps < 1:
            raise ValueError("at least one step")
        lr = self._lane_rates(lrs, (n_steps, P))
        bs = self._check_rows_run(P, "n_lanes", x, y, row_idx, batch_sizes, losses_out, slot0)
        check(self.lib.pyz_sgld_lanes_run(self.h, ptr(theta), ptr(mean), ptr(sq_mean), P, ptr(x), ptr(y), ptr(row_idx), bs,
                                          lr.ctypes.data_as(C.POINTER(C.c_float)), n_steps, int(n0), int(slot0), int(seed),
                                          int(seed_stride), ptr(losses_out), _stream()))

    def lane_scores(self, weights, x, y, want_errors=True):
        """The score of every row of weights (n_lanes, D) on the rows of x / y (at most max_batch): (loss_sum float64
        (n_lanes,), errors int64 (n_lanes,) or None) on the device -- the sum over the rows of the plan's per-row loss,
        and the misclassified rows (0 for MSE).  More lanes than max_particles go through in chunks."""
        _f32(weights, name="weights")
        if weights.dim() != 2 or weights.shape[1] != self.D or weights.shape[0] < 1:
            raise ValueError(f"weights must be (n_lanes, {self.D})")
        n = int(x.shape[0])
        self._check_xy(x, y, None, n)
        S = int(weights.shape[0])
        loss_sum = torch.empty((S,), dtype=torch.float64, device=self.device)
        errors = torch.empty((S,), dtype=torch.int64, device=self.device) if want_errors else None
        check(self.lib.pyz_lane_scores(self.h, ptr(weights), S, ptr(x), ptr(y), n, ptr(loss_sum), ptr(errors), _stream()))
        return loss_sum, errors

    def sgd_run(self, theta, x, y, row_idx, batch_sizes, lrs, losses_out, use_graph=True, slot0=0):
        """n = len(batch_sizes) SGD steps without host work in between (see sgld_run for the table layout)."""
        n_steps = len(batch_sizes)
        assert len(lrs) == n_steps and n_steps > 0
        _f32(theta, (self.D,), "theta")
        self._check_xy(x, y, row_idx, 1)
        if slot0 < 0 or row_idx.numel() < (slot0 + n_steps) * self.max_batch or losses_out.numel() < slot0 + n_steps:
            raise ValueError("row_idx / losses_out too small")
        if any(int(b) < 1 or int(b) > self.max_batch for b in batch_sizes):
            raise ValueError("batch size outside the plan")
        bs = (C.c_int32 * n_steps)(*[int(b) for b in batch_sizes])
        lr = (C.c_float * n_steps)(*[float(v) for v in lrs])
        check(self.lib.pyz_sgd_run(self.h, ptr(theta), ptr(x), ptr(y), ptr(row_idx), bs, lr, n_steps, int(slot0),
                                   ptr(losses_out), 1 if use_graph else 0, _stream()))

    def swag_run(self, theta, mean, sq_mean, dev, frequency, x, y, row_idx, batch_sizes, lrs, n0, losses_out,
                 use_graph=True, slot0=0):
        """n = len(batch_sizes) SWAG steps without host work in between; dev is the (k, D) deviation matrix."""
        n_steps = len(batch_sizes)
        assert len(lrs) == n_steps and n_steps > 0
        for t, nm in ((theta, "theta"), (mean, "mean"), (sq_mean, "sq_mean")):
            _f32(t, (self.D,), nm)
        _f32(dev, name="dev")
        assert dev.dim() == 2 and dev.shape[1] == self.D
        self._check_xy(x, y, row_idx, 1)
        if slot0 < 0 or row_idx.numel() < (slot0 + n_steps) * self.max_batch or losses_out.numel() < slot0 + n_steps:
            raise ValueError("row_idx / losses_out too small")
        if any(int(b) < 1 or int(b) > self.max_batch for b in batch_sizes):
            raise ValueError("batch size outside the plan")
        bs = (C.c_int32 * n_steps)(*[int(b) for b in batch_sizes])
        lr = (C.c_float * n_steps)(*[float(v) for v in lrs])
        check(self.lib.pyz_swag_run(self.h, ptr(theta), ptr(mean), ptr(sq_mean), ptr(dev), int(dev.shape[0]), int(frequency),
                                    ptr(x), ptr(y), ptr(row_idx), bs, lr, n_steps, int(n0), int(slot0), ptr(losses_out),
                                    1 if use_graph else 0, _stream()))

    def last_run_path(self):
        """("graph" | "eager" | "mixed", steps) of the last sgld_run / sgld_chains_run / sgd_run / swag_run / adam_run / bsam_run call on
        this plan (sgld_chains_run: always "eager")."""
        g, e, n = C.c_int32(), C.c_int32(), C.c_int32()
        check(self.lib.pyz_last_run_info(self.h, C.byref(g), C.byref(e), C.byref(n)))
        kind = "graph" if e.value == 0 else ("eager" if g.value == 0 else "mixed")
        return kind, g.value + e.value

    def last_run_graph_launches(self) -> int:
        n = C.c_int32()
        check(self.lib.pyz_last_run_info(self.h, None, None, C.byref(n)))
        return n.value

    def sgld_run_captures(self) -> int:
        """Graphs the last sgd_run / swag_run / sgld_run / bbb_run call on this plan had to capture (0: every chunk was
        replayed from the cache, or launched eagerly)."""
        n = C.c_int32()
        check(self.lib.pyz_sgld_run_info(self.h, C.byref(n)))
        return n.value

    def run_batch_form(self) -> str:
        """Where the steps of the last device-resident run on this plan found their batch rows: "gather" (each step gathered
        its own), "rows" (assembled one step ahead as contiguous rows) or "images" (assembled one step ahead in the order the
        kernels' MFMA fragments read them: PYZ_BATCH_FRAG)."""
        n = C.c_int32()
        check(self.lib.pyz_run_batch_form(self.h, C.byref(n)))
        return ("gather", "rows", "images")[n.value]

    def check_finite(self):
        """Synchronises the current stream; raises PyzError (code E_NAN) if a step since the last check produced a
        NaN / Inf loss."""
        check(self.lib.pyz_check_finite(self.h, _stream()))

    # ------------------------------------------------------------------ B2-B4
    def bbb_step(self, mu, rho, w, x, y, lr, alpha, prior_mean, prior_rho, step, seed, cost_out, batch=None,
                 row_idx=None, eps=None, prior_mean_vec=None, prior_rho_vec=None):
        for t, nm in ((mu, "mu"), (rho, "rho"), (w, "w")):
            _f32(t, (self.D,), nm)
        for t, nm in ((eps, "eps"), (prior_mean_vec, "prior_mean_vec"), (prior_rho_vec, "prior_rho_vec")):
            if t is not None:
                _f32(t, (self.D,), nm)
        _f32(cost_out, name="cost_out")
        assert cost_out.numel() >= 3
        batch = int(batch if batch is not None else (row_idx.numel() if row_idx is not None else x.shape[0]))
        self._check_xy(x, y, row_idx, batch)
        check(self.lib.pyz_bbb_step(self.h, ptr(mu), ptr(rho), ptr(w), ptr(x), ptr(y), ptr(row_idx), batch, float(lr),
                                    float(alpha), float(prior_mean), float(prior_rho), ptr(prior_mean_vec),
                                    ptr(prior_rho_vec), int(step), int(seed), ptr(eps), ptr(cost_out), _stream()))

    def bbb_run(self, mu, rho, w, x, y, row_idx, batch_sizes, lrs, alpha, prior_mean, prior_rho, step0, seed, costs_out,
                use_graph=True, slot0=0, prior_mean_vec=None, prior_rho_vec=None, val_plan=None, val_x=None, val_y=None,
                val_losses_out=None):
        """n = len(batch_sizes) BBB steps without host work in between (see sgld_run for the table layout); costs_out
        (slots, 4): {cost, data loss, log q - log p, -} per step.  val_plan / val_x / val_y / val_losses_out (slots):
        the validation forward of BBB.py:203-209 inside the run (steps with step % 10 != 0)."""
        n_steps = len(batch_sizes)
        assert len(lrs) == n_steps and n_steps > 0
        for t, nm in ((mu, "mu"), (rho, "rho"), (w, "w")):
            _f32(t, (self.D,), nm)
        for t, nm in ((prior_mean_vec, "prior_mean_vec"), (prior_rho_vec, "prior_rho_vec")):
            if t is not None:
                _f32(t, (self.D,), nm)
        self._check_xy(x, y, row_idx, 1)
        _f32(costs_out, name="costs_out")
        if slot0 < 0 or row_idx.numel() < (slot0 + n_steps) * self.max_batch or costs_out.numel() < 4 * (slot0 + n_steps):
            raise ValueError("row_idx / costs_out too small")
        if any(int(b) < 1 or int(b) > self.max_batch for b in batch_sizes):
            raise ValueError("batch size outside the plan")
        n_val = 0
        if val_plan is not None:
            _f32(val_x, name="val_x")
            n_val = int(val_x.shape[0])
            if val_x.shape[1] != self.spec.dims[0] or n_val > val_plan.max_batch or val_plan.D != self.D:
                raise ValueError("validation split does not fit the validation plan")
            _f32(val_losses_out, name="val_losses_out")
            if val_losses_out.numel() < slot0 + n_steps:
                raise ValueError("val_losses_out too small")
        bs = (C.c_int32 * n_steps)(*[int(b) for b in batch_sizes])
        lr = (C.c_float * n_steps)(*[float(v) for v in lrs])
        check(self.lib.pyz_bbb_run(self.h, ptr(mu), ptr(rho), ptr(w), ptr(x), ptr(y), ptr(row_idx), bs, lr, n_steps, float(alpha),
                                   float(prior_mean), float(prior_rho), ptr(prior_mean_vec), ptr(prior_rho_vec), int(step0),
                                   int(slot0), int(seed), ptr(costs_out), val_plan.h if val_plan is not None else None,
                                   ptr(val_x), ptr(val_y), n_val, ptr(val_losses_out), 1 if use_graph else 0, _stream()))

    def _check_bbb_lanes(self, mu, rho, w, lrs, alphas, prior_means, prior_rhos, seed_stride, prior_mean_vec, prior_rho_vec):
        """The (n_lanes, D) state, the four host tables (P floats each) and the shared prior vectors of BBB lanes; returns
        (P, the tables as float32 arrays)."""
        P = int(mu.shape[0]) if mu.dim() == 2 else 0
        if not 1 <= P <= min(self.max_particles, _lib.MAX_LANES):
            raise ValueError(f"mu must be (n_lanes, {self.D}) with 1 <= n_lanes <= {min(self.max_particles, _lib.MAX_LANES)}")
        for t, nm in ((mu, "mu"), (rho, "rho"), (w, "w")):
            _f32(t, (P, self.D), nm)
        if seed_stride not in (0, 1):
            raise ValueError("seed_stride must be 0 (one noise stream for every lane) or 1 (seed + lane)")
        if (prior_mean_vec is None) != (prior_rho_vec is None):
            raise ValueError("prior_mean_vec and prior_rho_vec go together")
        for t, nm in ((prior_mean_vec, "prior_mean_vec"), (prior_rho_vec, "prior_rho_vec")):
            if t is not None:
                _f32(t, (self.D,), nm)
        return P, [self._lane_rates(v, (P,)) for v in (lrs, alphas, prior_means, prior_rhos)]

    def bbb_lanes_step(self, mu, rho, w, x, y, lrs, alphas, prior_means, prior_rhos, step, seed, cost_out, seed_stride=0,
                       batch=None, row_idx=None, eps=None, prior_mean_vec=None, prior_rho_vec=None):
        """bbb_step for the n_lanes rows of mu / rho / w (n_lanes, D) on ONE shared batch: lane c with lrs[c], alphas[c] and
        the scalar prior (prior_means[c], prior_rhos[c]) (P host floats each; or the shared (D,) prior vectors), and the
        seed seed + c * seed_stride (or row c of the (n_lanes, D) eps); cost_out: float32 (n_lanes, 4)."""
        P, tabs = self._check_bbb_lanes(mu, rho, w, lrs, alphas, prior_means, prior_rhos, seed_stride, prior_mean_vec,
                                        prior_rho_vec)
        if eps is not None:
            _f32(eps, (P, self.D), "eps")
        _f32(cost_out, name="cost_out")
        if cost_out.numel() < 4 * P:
            raise ValueError("cost_out must hold 4 * n_lanes entries")
        batch = int(batch if batch is not None else (row_idx.numel() if row_idx is not None else x.shape[0]))
        self._check_xy(x, y, row_idx, batch)
        fp = C.POINTER(C.c_float)
        check(self.lib.pyz_bbb_lanes_step(self.h, ptr(mu), ptr(rho), ptr(w), P, ptr(x), ptr(y), ptr(row_idx), batch,
                                          *[t.ctypes.data_as(fp) for t in tabs], ptr(prior_mean_vec), ptr(prior_rho_vec),
                                          int(step), int(seed), int(seed_stride), ptr(eps), ptr(cost_out), _stream()))

    def bbb_lanes_run(self, mu, rho, w, x, y, row_idx, batch_sizes: Sequence[int], lrs, alphas, prior_means, prior_rhos,
                      step0, seed, costs_out, seed_stride=0, slot0=0, prior_mean_vec=None, prior_rho_vec=None):
        """n = len(batch_sizes) steps of bbb_lanes_step without host work in between (see sgld_chains_run; the lanes' four
        tables hold for every step); costs_out: float32 (slots, n_lanes, 4), step s writes row slot0 + s."""
        P, tabs = self._check_bbb_lanes(mu, rho, w, lrs, alphas, prior_means, prior_rhos, seed_stride, prior_mean_vec,
                                        prior_rho_vec)
        n_steps = len(batch_sizes)
        if n_steps < 1:
            raise ValueError("at least one step")
        self._check_xy(x, y, row_idx, 1)
        _f32(costs_out, name="costs_out")
        if slot0 < 0 or row_idx.numel() < (slot0 + n_steps) * self.max_batch or costs_out.numel() < 4 * P * (slot0 + n_steps):
            raise ValueError("row_idx / costs_out too small")
        if any(int(b) < 1 or int(b) > self.max_batch for b in batch_sizes):
            raise ValueError("batch size outside the plan")
        bs = (C.c_int32 * n_steps)(*[int(b) for b in batch_sizes])
        fp = C.POINTER(C.c_float)
        check(self.lib.pyz_bbb_lanes_run(self.h, ptr(mu), ptr(rho), ptr(w), P, ptr(x), ptr(y),
                                         *[t.ctypes.data_as(fp) for t in tabs], ptr(prior_mean_vec), ptr(prior_rho_vec),
                                         ptr(row_idx), bs, n_steps, int(step0), int(slot0), int(seed), int(seed_stride),
                                         ptr(costs_out), _stream()))

    def _run_tables(self, row_idx, batch_sizes, lrs, losses_out, slot0, per_step=1):
        """The argument checks the chained runs share (see sgd_run); returns the host tables as ctypes arrays."""
        n_steps = len(batch_sizes)
        assert len(lrs) == n_steps and n_steps > 0
        _f32(losses_out, name="losses_out")
        if (slot0 < 0 or row_idx.numel() < (slot0 + n_steps) * self.max_batch
                or losses_out.numel() < per_step * (slot0 + n_steps)):
            raise ValueError("row_idx / losses_out too small")
        if any(int(b) < 1 or int(b) > self.max_batch for b in batch_sizes):
            raise ValueError("batch size outside the plan")
        return (C.c_int32 * n_steps)(*[int(b) for b in batch_sizes]), (C.c_float * n_steps)(*[float(v) for v in lrs])

    def adam_run(self, theta, m, v, x, y, row_idx, batch_sizes, lrs, epochs, beta_1, beta_2, losses_out, denom_eps=1e-3,
                 decay=0.0, perturb=False, lam=0.0, num_data=1.0, step0=0, seed=0, use_graph=True, slot0=0):
        """n = len(batch_sizes) ADAM steps (perturb: VADAM steps, each behind its weight perturbation) without host work in
        between (see sgld_run for the table layout).  epochs[s] >= 1: the epoch count of step s's bias correction; step s
        is optimizer step step0 + s (VADAM's Philox step) and writes its loss to losses_out[slot0 + s]."""
        for t, nm in ((theta, "theta"), (m, "m"), (v, "v")):
            _f32(t, (self.D,), nm)
        self._check_xy(x, y, row_idx, 1)
        bs, lr = self._run_tables(row_idx, batch_sizes, lrs, losses_out, slot0)
        n_steps = len(batch_sizes)
        if len(epochs) != n_steps:
            raise ValueError("one epoch count per step")
        ep = (C.c_int64 * n_steps)(*[int(e) for e in epochs])
        check(self.lib.pyz_adam_run(self.h, ptr(theta), ptr(m), ptr(v), ptr(x), ptr(y), ptr(row_idx), bs, lr, ep, n_steps,
                                    float(beta_1), float(beta_2), float(denom_eps), float(decay), 1 if perturb else 0,
                                    float(lam), float(num_data), int(step0), int(slot0), int(seed), ptr(losses_out),
                                    1 if use_graph else 0, _stream()))

    def bsam_run(self, theta, m, v, x, y, row_idx, batch_sizes, lrs, beta_1, beta_2, lam, rho, gam, num_data, step0, seed,
                 losses_out, use_graph=True, slot0=0):
        """n = len(batch_sizes) BSAM steps without host work in between; step s is optimizer step step0 + s (its Philox
        step) and writes l1, l2 to losses_out[2 (slot0 + s) ..]."""
        for t, nm in ((theta, "theta"), (m, "m"), (v, "v")):
            _f32(t, (self.D,), nm)
        self._check_xy(x, y, row_idx, 1)
        bs, lr = self._run_tables(row_idx, batch_sizes, lrs, losses_out, slot0, per_step=2)
        check(self.lib.pyz_bsam_run(self.h, ptr(theta), ptr(m), ptr(v), ptr(x), ptr(y), ptr(row_idx), bs, lr,
                                    len(batch_sizes), float(beta_1), float(beta_2), float(lam), float(rho), float(gam),
                                    float(num_data), int(step0), int(slot0), int(seed), ptr(losses_out),
                                    1 if use_graph else 0, _stream()))

    def adam_run_captures(self) -> int:
        """Graphs the last adam_run / bsam_run call on this plan had to capture (0: every stretch was replayed)."""
        n = C.c_int32()
        check(self.lib.pyz_adam_run_info(self.h, C.byref(n)))
        return n.value

    # ------------------------------------------------------------------ H2-H5
    def hmc_step(self, q, x, y, L, epsilon, m, prior_mean, prior_sigma, uniforms, step, seed, stats_out, burning=False,
                 unit_p=None, prior_mean_vec=None, prior_sigma_vec=None):
        P = 1 if q.dim() == 1 else q.shape[0]
        _f32(q, name="q")
        assert q.numel() == P * self.D
        if unit_p is not None:
            _f32(unit_p, name="unit_p")
            assert unit_p.numel() == P * self.D
        for t, nm in ((prior_mean_vec, "prior_mean_vec"), (prior_sigma_vec, "prior_sigma_vec")):
            if t is not None:
                _f32(t, (self.D,), nm)
        _f32(stats_out, name="stats_out")
        assert stats_out.numel() >= 8 * P
        n_rows = x.shape[0]
        self._check_xy(x, y, None, n_rows)
        u = np.ascontiguousarray(np.asarray(uniforms, dtype=np.float32).reshape(-1))
        assert u.size == P
        check(self.lib.pyz_hmc_step(self.h, ptr(q), P, ptr(x), ptr(y), n_rows, int(L), float(epsilon), float(m),
                                    float(prior_mean), float(prior_sigma), ptr(prior_mean_vec), ptr(prior_sigma_vec),
                                    1 if burning else 0, u.ctypes.data_as(C.POINTER(C.c_float)), int(step), int(seed),
                                    ptr(unit_p), ptr(stats_out), _stream()))

    def hmc_run(self, q, x, y, L, epsilon, m, prior_mean, prior_sigma, uniforms, n_burn, step0, seed, stats_all, samples,
                freq, count, fail, use_graph=True, slot0=0, prior_mean_vec=None, prior_sigma_vec=None):
        """len(uniforms) / P consecutive proposals of hmc_step without host work in between.  uniforms: host float32
        (n_steps, P), proposal-major; the first n_burn proposals burn and record nothing; proposal i writes its
        statistics to stats_all[slot0 + i] (slots, P, 8).  The sample record stays on the device: samples float32
        (P, cap, D), freq int32 (P, cap), count int32 (P,) (zeros for a fresh record), fail int32 (4,) (zeroed by the
        caller): {accepted proposals without a row, give-ups, non-finite losses, proposals done}."""
        P = 1 if q.dim() == 1 else q.shape[0]
        _f32(q, name="q")
        assert q.numel() == P * self.D
        for t, nm in ((prior_mean_vec, "prior_mean_vec"), (prior_sigma_vec, "prior_sigma_vec")):
            if t is not None:
                _f32(t, (self.D,), nm)
        n_rows = x.shape[0]
        self._check_xy(x, y, None, n_rows)
        u = np.ascontiguousarray(np.asarray(uniforms, dtype=np.float32).reshape(-1))
        if u.size == 0 or u.size % P:
            raise ValueError("uniforms must hold n_steps x P values")
        n_steps = u.size // P
        _f32(stats_all, name="stats_all")
        _f32(samples, name="samples")
        if samples.dim() != 3 or samples.shape[0] != P or samples.shape[2] != self.D:
            raise ValueError("samples must be (P, cap, D)")
        cap = int(samples.shape[1])
        for t, nm, n in ((freq, "freq", P * cap), (count, "count", P), (fail, "fail", 4)):
            if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or t.numel() < n:
                raise ValueError(f"{nm} must be a contiguous int32 device tensor of at least {n} entries")
        if slot0 < 0 or stats_all.numel() < (slot0 + n_steps) * P * 8:
            raise ValueError("stats_all must hold (slot0 + n_steps) * P * 8 entries")
        check(self.lib.pyz_hmc_run(self.h, ptr(q), P, ptr(x), ptr(y), n_rows, int(L), float(epsilon), float(m),
                                   float(prior_mean), float(prior_sigma), ptr(prior_mean_vec), ptr(prior_sigma_vec),
                                   u.ctypes.data_as(C.POINTER(C.c_float)), n_steps, int(n_burn), int(step0), int(slot0),
                                   int(seed), ptr(stats_all), ptr(samples), ptr(freq), ptr(count), cap, ptr(fail),
                                   1 if use_graph else 0, _stream()))

    def hmc_run_captures(self) -> int:
        """Graphs the last hmc_run call on this plan had to capture (0: every chunk was replayed from the cache)."""
        n = C.c_int32()
        check(self.lib.pyz_hmc_run_info(self.h, C.byref(n)))
        return n.value

    # ------------------------------------------------------------------ V2-V4
    def svgd_step(self, particles, all_particles, row0, adam_m, adam_v, x, y, lr, gamma, t, loss_out, sweep="gauss_seidel",
                  batch=None, row_idx=None):
        _f32(particles, name="particles")
        _f32(all_particles, name="all_particles")
        n_local, n_total = particles.shape[0], all_particles.shape[0]
        assert particles.shape[1] == self.D and all_particles.shape[1] == self.D
        _f32(adam_m, (n_local, self.D), "adam_m")
        _f32(adam_v, (n_local, self.D), "adam_v")
        batch = int(batch if batch is not None else (row_idx.numel() if row_idx is not None else x.shape[0]))
        self._check_xy(x, y, row_idx, batch)
        check(self.lib.pyz_svgd_step(self.h, ptr(particles), n_local, ptr(all_particles), n_total, int(row0),
                                     ptr(adam_m), ptr(adam_v), ptr(x), ptr(y), ptr(row_idx), batch, float(lr),
                                     _gamma(gamma), int(t), SWEEP[sweep], ptr(loss_out), _stream()))

    def svgd_gradients(self, particles, x, y, batch=None, row_idx=None):
        """Phase 1 of svgd_step: the loss gradients of the local particles (kept inside the plan)."""
        _f32(particles, name="particles")
        assert particles.dim() == 2 and particles.shape[1] == self.D
        batch = int(batch if batch is not None else (row_idx.numel() if row_idx is not None else x.shape[0]))
        self._check_xy(x, y, row_idx, batch)
        check(self.lib.pyz_svgd_gradients(self.h, ptr(particles), particles.shape[0], ptr(x), ptr(y), ptr(row_idx), batch,
                                          _stream()))

    def svgd_sweep(self, particles, all_particles, row0, adam_m, adam_v, lr, gamma, t, loss_out, sweep="gauss_seidel"):
        """Phase 2: kernel rows, repulsion and Adam on the gradients svgd_gradients left; first reader of all_particles."""
        _f32(particles, name="particles")
        _f32(all_particles, name="all_particles")
        n_local, n_total = particles.shape[0], all_particles.shape[0]
        assert particles.shape[1] == self.D and all_particles.shape[1] == self.D
        _f32(adam_m, (n_local, self.D), "adam_m")
        _f32(adam_v, (n_local, self.D), "adam_v")
        check(self.lib.pyz_svgd_sweep(self.h, ptr(particles), n_local, ptr(all_particles), n_total, int(row0), ptr(adam_m),
                                      ptr(adam_v), float(lr), _gamma(gamma), int(t), SWEEP[sweep], ptr(loss_out), _stream()))

    def svgd_tile_shape(self, n_local, n_total, row0) -> bool:
        """Shapes pyz_svgd_kernel_matrix / pyz_svgd_combine take (the all-rows-at-once Jacobi kernels)."""
        return n_total <= 64 and n_local % 4 == 0 and row0 % 4 == 0

    def svgd_kernel_matrix(self, all_particles, row0, n_local, gamma, stream=None):
        """First half of the Jacobi sweep: K rows of the local particles against the snapshot (kept inside the plan).
        Touches neither gradients nor losses: may run on `stream` while svgd_gradients runs on another."""
        _f32(all_particles, name="all_particles")
        assert all_particles.dim() == 2 and all_particles.shape[1] == self.D
        st = C.c_void_p(stream.cuda_stream) if stream is not None else _stream()
        check(self.lib.pyz_svgd_kernel_matrix(self.h, ptr(all_particles), all_particles.shape[0], int(row0), int(n_local),
                                              _gamma(gamma), st))

    def svgd_gram_groups(self, all_particles, g_lo, g_hi, groups, stream=None):
        """The distance pass over groups [g_lo, g_hi) of the SVGD_GROUPS groups of element blocks, all pairs: the group sums
        go to rows [g_lo, g_hi) of `groups` (SVGD_GROUPS, 64 * 64) float64 (a rank's share of a D-sharded pass)."""
        _f32(all_particles, name="all_particles")
        assert all_particles.dim() == 2 and all_particles.shape[1] == self.D
        assert groups.dtype == torch.float64 and groups.is_cuda and groups.is_contiguous() and groups.numel() == SVGD_GROUPS * 4096
        st = C.c_void_p(stream.cuda_stream) if stream is not None else _stream()
        check(self.lib.pyz_svgd_gram_groups(self.h, ptr(all_particles), all_particles.shape[0], int(g_lo), int(g_hi),
                                            ptr(groups), st))

    def svgd_kernel_matrix_groups(self, groups, all_particles, row0, n_local, gamma, stream=None):
        """svgd_kernel_matrix from the complete group sums (every rank's svgd_gram_groups, gathered) instead of a pass over
        the snapshot; same bits."""
        _f32(all_particles, name="all_particles")
        assert groups.dtype == torch.float64 and groups.is_cuda and groups.is_contiguous() and groups.numel() == SVGD_GROUPS * 4096
        st = C.c_void_p(stream.cuda_stream) if stream is not None else _stream()
        check(self.lib.pyz_svgd_kernel_matrix_groups(self.h, ptr(groups), ptr(all_particles), all_particles.shape[0], int(row0),
                                                     int(n_local), _gamma(gamma), st))

    def svgd_combine(self, particles, all_particles, row0, adam_m, adam_v, lr, gamma, t, loss_out):
        """Second half: phi, Adam and the loss of every local row; after svgd_gradients AND svgd_kernel_matrix.
        `particles` (n_local, D) is only written (the rows' current values are the snapshot's)."""
        _f32(particles, name="particles")
        _f32(all_particles, name="all_particles")
        n_local, n_total = particles.shape[0], all_particles.shape[0]
        assert particles.shape[1] == self.D and all_particles.shape[1] == self.D
        _f32(adam_m, (n_local, self.D), "adam_m")
        _f32(adam_v, (n_local, self.D), "adam_v")
        check(self.lib.pyz_svgd_combine(self.h, ptr(particles), n_local, ptr(all_particles), n_total, int(row0), ptr(adam_m),
                                        ptr(adam_v), float(lr), _gamma(gamma), int(t), ptr(loss_out), _stream()))

    # ------------------------------------------------------------------ F1
    def fsvi_step(self, mu, particles, adam_m, adam_v, x, y, batch_size, lr, t, seed, loss_out, lo=None, hi=None, xm=None,
                  noise=None, eps=None, want_terms=False, batch=None, row_idx=None):
        """FSVI.step (FSVI.py:60-147, DESIGN A8): one step of mu (D,), its Adam slots and the k rows of particles (k, D) on
        the `batch` rows of x picked by row_idx plus batch_size measurement rows; the plan needs max_batch >= batch +
        batch_size and max_particles >= k.  Draws come from the Philox stream (seed, STREAM_FSVI, 4 t ..) unless injected:
        xm (batch_size, F), noise (k, F), eps (k, D); lo / hi (F,) bound the measurement set when xm is None.  loss_out:
        (1,) float32.  want_terms: returns dict(alpha (k, n) float64, stein (k, D), grad (D,), xp (k, n, F), f (k, n))."""
        k = int(particles.shape[0]) if particles.dim() == 2 else 0
        F, B = self.spec.dims[0], int(batch_size)
        batch = int(batch if batch is not None else (row_idx.numel() if row_idx is not None else x.shape[0]))
        dims = (C.c_int32 * len(self.spec.dims))(*self.spec.dims)
        acts = (C.c_int32 * len(self.spec.acts))(*[ACT[a] for a in self.spec.acts])
        check(self.lib.pyz_fsvi_check(self.spec.n_layers, dims, acts, LOSS[self.spec.loss], k, batch, B))
        n = batch + B
        if n > self.max_batch or k > self.max_particles:
            raise ValueError(f"the plan holds {self.max_batch} rows x {self.max_particles} particles; FSVI needs "
                             f"batch + batch_size = {n} rows x {k}")
        _f32(mu, (self.D,), "mu")
        _f32(particles, (k, self.D), "particles")
        _f32(adam_m, (self.D,), "adam_m")
        _f32(adam_v, (self.D,), "adam_v")
        _f32(loss_out, (1,), "loss_out")
        self._check_xy(x, y, row_idx, batch)
        if row_idx is not None and row_idx.numel() < batch:
            raise ValueError("row_idx holds fewer than `batch` entries")
        for t_, shape, nm in ((xm, (B, F), "xm"), (noise, (k, F), "noise"), (eps, (k, self.D), "eps"), (lo, (F,), "lo"),
                              (hi, (F,), "hi")):
            if t_ is not None:
                _f32(t_, shape, nm)
        if xm is None and (lo is None or hi is None):
            raise ValueError("lo and hi are needed when xm is not given")
        terms = None
        if want_terms:
            terms = dict(alpha=torch.empty((k, n), dtype=torch.float64, device=self.device),
                         stein=torch.empty((k, self.D), dtype=torch.float32, device=self.device),
                         grad=torch.empty((self.D,), dtype=torch.float32, device=self.device),
                         xp=torch.empty((k, n, F), dtype=torch.float32, device=self.device),
                         f=torch.empty((k, n), dtype=torch.float32, device=self.device))
        g = terms or {}
        check(self.lib.pyz_fsvi_step(self.h, ptr(mu), ptr(particles), k, ptr(adam_m), ptr(adam_v), ptr(x), ptr(y),
                                     ptr(row_idx), batch, B, ptr(lo), ptr(hi), float(lr), int(t), int(seed), ptr(xm),
                                     ptr(noise), ptr(eps), ptr(g.get("alpha")), ptr(g.get("stein")), ptr(g.get("grad")),
                                     ptr(g.get("xp")), ptr(g.get("f")), ptr(loss_out), _stream()))
        return terms

    @property
    def workspace_bytes(self) -> int:
        return int(self.lib.pyz_mlp_workspace_bytes(self.h))

    # ------------------------------------------------------------------ R1
    def _lib_predict(self, weights, S, x, n, samples, mean, m2):
        if m2 is None:
            check(self.lib.pyz_predict(self.h, weights, S, x, n, samples, mean, _stream()))
        else:
            check(self.lib.pyz_predict_moments(self.h, weights, S, x, n, mean, m2, _stream()))

    def predict_surface(self, weights, x, column=0, want_cols=True, want_summary=True):
        """(cols, mean, top, cls, ent) of the draws `weights` (S, D) on the rows of x, for decision-surface plots:
        cols (S, n) = column `column` of every draw's prediction (None without want_cols), mean (n, out) = predict's mean
        bit for bit, and of each mean row q (one output: the pair (1 - m, m)) top (n,) = max q, cls (n,) int32 = its
        first index, ent (n,) = -sum q log(q + 1e-5), raw (all None without want_summary).  One kernel per chunk of
        max_particles draws (pyz_predict_surface); the (S, n, out) sample tensor is never formed."""
        S, n, C_out = self._check_read_out(weights, x)
        column = int(column)
        if not 0 <= column < C_out:
            raise ValueError(f"column {column} outside [0, {C_out})")
        dev = self.device
        cols = torch.empty((S, n), dtype=torch.float32, device=dev) if want_cols else None
        mean = torch.empty((n, C_out), dtype=torch.float32, device=dev)
        top = torch.empty((n,), dtype=torch.float32, device=dev) if want_summary else None
        cls = torch.empty((n,), dtype=torch.int32, device=dev) if want_summary else None
        ent = torch.empty((n,), dtype=torch.float32, device=dev) if want_summary else None
        check(self.lib.pyz_predict_surface(self.h, ptr(weights), S, ptr(x), n, column, ptr(cols), ptr(mean), ptr(top),
                                           ptr(cls), ptr(ent), _stream()))
        return cols, mean, top, cls, ent

    # ------------------------------------------------------------------ R2
    def input_grad(self, weights, x, y, scale=1.0, epsilon=None):
        """(xgrad, xadv or None, losses): xgrad (n, in) = scale * sum over the draws `weights` (S, D) of the gradient of
        each draw's mean loss over the n rows of x with respect to x; with epsilon, xadv = x + epsilon * sign(xgrad)
        (Robustness.py:115-144); losses (S,) = each draw's mean loss."""
        _f32(weights, name="weights")
        if weights.dim() != 2 or weights.shape[1] != self.D or weights.shape[0] < 1:
            raise ValueError(f"weights must be (draws >= 1, {self.D})")
        S = int(weights.shape[0])
        _f32(x, name="x")
        n = int(x.shape[0]) if x.dim() == 2 else 0
        self._check_xy(x, y, None, n)
        if y is None:
            raise TypeError("y is required")
        xgrad = torch.empty_like(x)
        xadv = torch.empty_like(x) if epsilon is not None else None
        losses = torch.empty((S,), dtype=torch.float32, device=self.device)
        check(self.lib.pyz_input_grad(self.h, ptr(weights), S, ptr(x), ptr(y), n, float(scale), ptr(xgrad),
                                      float(epsilon) if epsilon is not None else 0.0, ptr(xadv), ptr(losses), _stream()))
        return xgrad, xadv, losses


STEM_CONV, STEM_POOL = 0, 1     # PYZ_STEM_CONV / PYZ_STEM_POOL
CONV_MAX_K = 4094               # PYZ_CONV_MAX_K (csrc/pyz_conv.h)


@dataclass(frozen=True)
class ConvSpec:
    """A convolutional front end (the stem) in front of a Dense stack.  input_shape = (H, W, C), channels last;
    ops[k] = ("conv", filters, kh, kw, "valid" | "same", activation) or ("pool", ph, pw); tail = the Dense layers on the
    flattened (NHWC) features.  The flat vector: per conv the kernel (kh, kw, cin, cout) then the bias, then the tail."""
    input_shape: Tuple[int, int, int]
    ops: Tuple[tuple, ...]
    tail: MLPSpec

    def op_shapes(self):
        """[(in (H, W, C), out (OH, OW, N))] per op; ValueError where a kernel or a pool does not fit its input, or a
        filter has more taps than the kernels' tap table holds."""
        h, w, c = (int(d) for d in self.input_shape)
        out = []
        for k, op in enumerate(self.ops):
            if op[0] == "conv":
                _, f, kh, kw, pad, _ = op
                ph, pw = (kh - 1, kw - 1) if pad == "same" else (0, 0)
                if kh > h + ph or kw > w + pw:
                    raise ValueError(f"op {k}: a {kh} x {kw} kernel is larger than the padded {h + ph} x {w + pw} image")
                if kh * kw * c > CONV_MAX_K:
                    raise ValueError(f"op {k}: {kh * kw * c} taps per filter exceed {CONV_MAX_K}")
                o = (h + ph - kh + 1, w + pw - kw + 1, int(f))
            else:
                _, ph, pw = op
                if ph > h or pw > w:
                    raise ValueError(f"op {k}: a {ph} x {pw} pool is larger than its {h} x {w} input")
                o = (h // ph, w // pw, c)
            out.append(((h, w, c), o))
            h, w, c = o
        return out

    @property
    def features(self):
        o = self.op_shapes()[-1][1]
        return o[0] * o[1] * o[2]

    def conv_shapes(self):
        """[(kh, kw, cin, cout)] of the conv layers, in network order."""
        return [(op[2], op[3], i[2], op[1]) for op, (i, _) in zip(self.ops, self.op_shapes()) if op[0] == "conv"]

    @property
    def stem_params(self):
        return sum((kh * kw * ci + 1) * co for kh, kw, ci, co in self.conv_shapes())

    @property
    def n_params(self):
        return self.stem_params + self.tail.n_params

    # what the optimizers and BayesianModel read of an MLPSpec: the Dense stack's
    dims = property(lambda self: self.tail.dims)
    acts = property(lambda self: self.tail.acts)
    loss = property(lambda self: self.tail.loss)

    def layer_slices(self):
        """The flat slice of every weight layer, conv layers first, in network order."""
        out, off = [], 0
        for kh, kw, ci, co in self.conv_shapes():
            n = (kh * kw * ci + 1) * co
            out.append(slice(off, off + n))
            off += n
        return out + [slice(s.start + off, s.stop + off) for s in self.tail.layer_slices()]

    def variable_shapes(self):
        return [((kh, kw, ci, co), (co,)) for kh, kw, ci, co in self.conv_shapes()] + self.tail.variable_shapes()


class ConvPlan(_NetPlan):
    """Owns one `pyz_stem` handle and the MLPPlan of the Dense tail: the forward, gradient, SGD / SWAG step and read-out
    of a conv net (pyz_convnet_*), with MLPPlan's argument conventions.  x: (rows, H * W * C) float32, images row-major
    (h, w, c)."""

    _FN = {"forward": "pyz_convnet_forward", "loss_grad": "pyz_convnet_loss_grad", "sgd_step": "pyz_convnet_sgd_step",
           "swag_step": "pyz_convnet_swag_step"}
    n_in = property(lambda self: int(np.prod(self.spec.input_shape)))
    _handles = property(lambda self: (self.h, self.tail.h))

    def __init__(self, spec: ConvSpec, max_batch: int, max_particles: int = 1, device=None):
        self.lib = _lib.load()
        self.spec, self.max_batch, self.max_particles = spec, int(max_batch), int(max_particles)
        if spec.loss == "bce":       # the conv net's loss kernels are the unfused k_loss_scce / k_loss_mse: no BinaryCrossentropy arm
            raise ValueError("BinaryCrossentropy is not built for a conv model: use a softmax head with "
                             "SparseCategoricalCrossentropy, or MeanSquaredError")
        if spec.tail.dims[0] != spec.features:       # (also refuses a kernel or pool that does not fit, without a device)
            raise ValueError(f"the Dense stack takes {spec.tail.dims[0]} inputs, the stem gives {spec.features} features")
        ops = []
        for op in spec.ops:
            if op[0] == "conv":
                if op[4] not in ("valid", "same"):
                    raise ValueError(f"padding {op[4]!r} is neither 'valid' nor 'same'")
                if op[5] == "softmax":
                    raise ValueError("softmax is not an activation of a Conv2D here")
                ops += [STEM_CONV, int(op[1]), int(op[2]), int(op[3]), 1 if op[4] == "same" else 0, ACT[op[5]]]
            elif op[0] == "pool":
                ops += [STEM_POOL, int(op[1]), int(op[2]), 0, 0, 0]
            else:
                raise ValueError(f"unknown stem op {op[0]!r}")
        if not torch.cuda.is_available():
            raise RuntimeError("bayesian_inference_for_nn_amd needs an MI355X (no HIP device visible); there is no CPU path")
        self.tail = MLPPlan(spec.tail, max_batch, max_particles, device)
        self.device = self.tail.device
        h = C.c_void_p()
        H, W, Cin = spec.input_shape
        with torch.cuda.device(self.device):
            check(self.lib.pyz_stem_create(int(H), int(W), int(Cin), len(spec.ops), (C.c_int32 * len(ops))(*ops),
                                           self.max_batch, self.max_particles, C.byref(h)))
        self.h = h
        self.D_stem = int(self.lib.pyz_stem_param_count(h))
        self.F = int(self.lib.pyz_stem_feature_count(h))
        self.D = self.D_stem + self.tail.D
        assert self.D_stem == spec.stem_params and self.F == spec.features and self.D == spec.n_params

    def close(self):
        if getattr(self, "h", None):
            self.lib.pyz_stem_destroy(self.h)
            self.h = None
        if getattr(self, "tail", None) is not None:
            self.tail.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def workspace_bytes(self) -> int:
        return int(self.lib.pyz_stem_workspace_bytes(self.h)) + self.tail.workspace_bytes

    def check_finite(self):
        self.tail.check_finite()

    # ------------------------------------------------------------------ the stem alone
    def stem_forward(self, theta, x, batch=None, row_idx=None, out=None):
        """(P, batch, F) features (NHWC, flattened) of the stem's block of every row of theta (written to `out` if given)."""
        P = self._particles(theta)
        batch = self._batch(batch, x, row_idx)
        self._check_xy(x, None, row_idx, batch)
        if out is None:
            out = torch.empty((P, batch, self.F), dtype=torch.float32, device=self.device)
        _f32(out, (P, batch, self.F), "out")
        check(self.lib.pyz_stem_forward(self.h, ptr(theta), self.D, P, ptr(x), ptr(row_idx), batch, ptr(out), _stream()))
        return out

    def stem_backward(self, theta, x, feature_grad, batch=None, row_idx=None):
        """(P, D_stem): the stem's block of the gradient from d loss / d features (P, batch, F), after the stem_forward
        of the same theta and batch."""
        P = self._particles(theta)
        batch = self._batch(batch, x, row_idx)
        self._check_xy(x, None, row_idx, batch)
        _f32(feature_grad, (P, batch, self.F), "feature_grad")
        grad = torch.empty((P, self.D_stem), dtype=torch.float32, device=self.device)
        check(self.lib.pyz_stem_backward(self.h, ptr(theta), self.D, P, ptr(x), ptr(row_idx), batch, ptr(feature_grad),
                                         ptr(grad), self.D_stem, _stream()))
        return grad

    # ------------------------------------------------------------------ the whole net: _NetPlan's methods
    def _lib_predict(self, weights, S, x, n, samples, mean, m2):
        check(self.lib.pyz_convnet_predict(self.h, self.tail.h, weights, S, x, n, samples, mean, m2, _stream()))


def make_plan(spec, max_batch: int, max_particles: int = 1, device=None):
    """The plan of a model's spec: a ConvPlan for a ConvSpec, else an MLPPlan."""
    cls = ConvPlan if isinstance(spec, ConvSpec) else MLPPlan
    return cls(spec, max_batch=max_batch, max_particles=max_particles, device=device)


class PilcoPlan:
    """Owns one `pyz_pilco` handle: the policy update of Deep-PILCO (dynamics/deep_pilco.py:247-326) for a policy net
    `policy_spec` (dims (S, hidden..., A): a Dense-only MLPSpec, or a description with `dims`, `acts`, `n_params` and
    per-layer `kinds` ("dense" | "rbf") and `gammas`, such as nn.model.PolicyNet) and `particles` draws of a dynamics net
    `dynamics_spec` (dims (S + A, hidden..., S), last layer linear), with the tape of up to max_horizon steps.  The specs'
    `loss` is not used.  cost and grad live
    in buffers of the plan (so do states and actions unless the caller passes its own): a captured graph is replayed
    while the caller's tensors stay where they are, and the returned tensors are overwritten by the next call."""

    def __init__(self, policy_spec, dynamics_spec: MLPSpec, particles: int, max_horizon: int, device=None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("bayesian_inference_for_nn_amd needs an MI355X (no HIP device visible); there is no CPU path")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.policy_spec, self.dynamics_spec = policy_spec, dynamics_spec
        self.K, self.max_horizon = int(particles), int(max_horizon)
        self.S, self.A = int(policy_spec.dims[0]), int(policy_spec.dims[-1])
        self.D_pol, self.D_dyn = policy_spec.n_params, dynamics_spec.n_params
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self._create(self.lib, policy_spec, dynamics_spec, self.K, self.max_horizon, h))
        self.h = h
        f32 = dict(dtype=torch.float32, device=self.device)
        self._cost, self._grad = torch.zeros(1, **f32), torch.zeros(self.D_pol, **f32)
        self._states = torch.zeros((self.max_horizon + 1, self.K, self.S), **f32)
        self._actions = torch.zeros((self.max_horizon, self.K, self.A), **f32)

    @staticmethod
    def _create(lib, policy_spec, dynamics_spec, particles, max_horizon, h):
        """The return code of pyz_pilco_create (a Dense-only MLPSpec) or pyz_pilco_create_layers (a policy description
        with per-layer `kinds` and `gammas`: nn.model.PolicyNet)."""
        n = len(policy_spec.acts)
        pd = (C.c_int32 * (n + 1))(*policy_spec.dims)
        pa = (C.c_int32 * n)(*[ACT[a] for a in policy_spec.acts])
        dd = (C.c_int32 * len(dynamics_spec.dims))(*dynamics_spec.dims)
        da = (C.c_int32 * len(dynamics_spec.acts))(*[ACT[a] for a in dynamics_spec.acts])
        kinds = getattr(policy_spec, "kinds", None)
        if kinds is None:
            return lib.pyz_pilco_create(n, pd, pa, dynamics_spec.n_layers, dd, da, particles, max_horizon, C.byref(h))
        pk = (C.c_int32 * n)(*[_lib.PILCO_KIND[k] for k in kinds])
        pg = (C.c_float * n)(*policy_spec.gammas)
        return lib.pyz_pilco_create_layers(n, pd, pa, pk, pg, dynamics_spec.n_layers, dd, da, particles, max_horizon, C.byref(h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.pyz_pilco_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def workspace_bytes(self) -> int:
        return int(self.lib.pyz_pilco_workspace_bytes(self.h))

    @staticmethod
    def default_freq(horizon: int) -> int:
        """deep_pilco.py:280: every freq-th step's reward is counted."""
        return max(int(int(horizon) / 25), 1)

    def _steps(self, t, rows, inner, name):
        """A (>= rows, *inner) float32 buffer of per-step blocks: the kernels use its first `rows` blocks."""
        _f32(t, name=name)
        if t.dim() != 1 + len(inner) or tuple(t.shape[1:]) != tuple(inner) or t.shape[0] < rows:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected (>= {rows}, {', '.join(str(v) for v in inner)})")
        return t

    def policy_step(self, phi, m, v, t, W, s0, eps, horizon, gamma, reward, lr=1e-3, freq=None, use_graph=True, states=None,
                    actions=None):
        """One rollout of `horizon` steps from s0 (K, S) under the dynamics draws W (K, D_dyn) with the unit normals
        eps (>= horizon, K, S), its cost and gradient, and the t-th Keras-Adam update of phi (D_pol,) with moments
        m, v (in place; t >= 1).  reward: a name of dynamics.all_rewards.  Returns (cost (1,), grad (D_pol,))."""
        return self._call(phi, m, v, int(t), W, s0, eps, horizon, gamma, reward, lr, freq, use_graph, states, actions)[:2]

    def rollout_grad(self, phi, W, s0, eps, horizon, gamma, reward, freq=None, use_graph=True, states=None, actions=None):
        """(cost (1,), grad (D_pol,), states (horizon + 1, K, S), actions (horizon, K, A)) of one rollout; phi is not
        changed.  states / actions: optional buffers of at least that many steps to write into."""
        return self._call(phi, None, None, 0, W, s0, eps, horizon, gamma, reward, 0.0, freq, use_graph, states, actions)

    def _call(self, phi, m, v, t, W, s0, eps, horizon, gamma, reward, lr, freq, use_graph, states, actions):
        H = int(horizon)
        if not 1 <= H <= self.max_horizon:
            raise ValueError(f"horizon {H} outside [1, {self.max_horizon}]")
        freq = self.default_freq(H) if freq is None else int(freq)
        if freq < 1:
            raise ValueError("freq must be >= 1")
        if reward not in _lib.REWARD:
            raise ValueError(f"unknown reward {reward!r}: one of {sorted(_lib.REWARD)}")
        if t < 0:
            raise ValueError("t must be >= 0")
        _f32(phi, (self.D_pol,), "phi")
        if t > 0:
            _f32(m, (self.D_pol,), "m")
            _f32(v, (self.D_pol,), "v")
        _f32(W, (self.K, self.D_dyn), "W")
        _f32(s0, (self.K, self.S), "s0")
        self._steps(eps, H, (self.K, self.S), "eps")
        states = self._states if states is None else self._steps(states, H + 1, (self.K, self.S), "states")
        actions = self._actions if actions is None else self._steps(actions, H, (self.K, self.A), "actions")
        check(self.lib.pyz_pilco_policy_step(self.h, ptr(phi), ptr(m) if t > 0 else None, ptr(v) if t > 0 else None, t,
                                             ptr(W), ptr(s0), ptr(eps), H, freq, float(gamma), _lib.REWARD[reward], float(lr),
                                             ptr(self._cost), ptr(self._grad), ptr(states), ptr(actions),
                                             1 if use_graph else 0, _stream()))
        return self._cost, self._grad, states[:H + 1], actions[:H]

    def act(self, phi, states):
        """actions (N, A): the policy's outputs under phi (D_pol,) for states (N, S), N >= 1, in one launch of the rollout's
        own policy forward -- for the states of a rollout they are the rollout's actions bit for bit."""
        _f32(phi, (self.D_pol,), "phi")
        _f32(states, name="states")
        if states.dim() != 2 or states.shape[1] != self.S or states.shape[0] < 1:
            raise ValueError(f"states has shape {tuple(states.shape)}, expected (N >= 1, {self.S})")
        actions = torch.empty((states.shape[0], self.A), dtype=torch.float32, device=self.device)
        check(self.lib.pyz_pilco_act(self.h, ptr(phi), ptr(states), int(states.shape[0]), ptr(actions), _stream()))
        return actions


class KernelProbe:
    """with KernelProbe(max_launches) as kp: ...launch steps...  -> kp.launches = [(kernel expression, microseconds)]
    in launch order: each kernel's own begin / end timestamps (measurement only; runs launch eagerly inside)."""

    def __init__(self, max_launches: int = 4096):
        self.max = int(max_launches)
        self.launches = []

    def __enter__(self):
        check(_lib.load().pyz_probe_begin(self.max))
        return self

    def __exit__(self, *exc):
        us = (C.c_float * self.max)()
        names = C.create_string_buffer(self.max * 64)
        n = C.c_int()
        rc = _lib.load().pyz_probe_end(_stream(), us, names, 64, C.byref(n))
        if exc[0] is None:
            check(rc)
            raw = names.raw
            self.launches = [(raw[64 * i:64 * i + 64].split(b"\0", 1)[0].decode(), float(us[i])) for i in range(n.value)]
        return False

    def by_kernel(self):
        """{kernel expression: (launch count, mean microseconds)}"""
        acc = {}
        for name, v in self.launches:
            c, t = acc.get(name, (0, 0.0))
            acc[name] = (c + 1, t + v)
        return {k: (c, t / c) for k, (c, t) in acc.items()}


def spd_solve(a: torch.Tensor, rhs: torch.Tensor):
    """Solves the symmetric positive-definite float64 systems a (systems, n, n) x = rhs (systems, n) on the device
    (pyz_spd_solve_f64: one workgroup per system, Cholesky + two substitutions).  rhs receives the solutions, a is scratch
    afterwards.  Returns the int32 (systems,) flags: 1 where a pivot was not positive (that solution is NaN)."""
    for t, nm in ((a, "a"), (rhs, "rhs")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
            raise TypeError(f"{nm} must be a contiguous CUDA(HIP) float64 tensor")
    if a.dim() != 3 or a.shape[1] != a.shape[2] or tuple(rhs.shape) != tuple(a.shape[:2]):
        raise ValueError(f"a must be (systems, n, n) and rhs (systems, n), not {tuple(a.shape)} and {tuple(rhs.shape)}")
    fail = torch.zeros((a.shape[0],), dtype=torch.int32, device=a.device)
    check(_lib.load().pyz_spd_solve_f64(ptr(a), ptr(rhs), int(a.shape[1]), int(a.shape[0]), ptr(fail), _stream()))
    return fail


def fill_normal(out: torch.Tensor, seed: int, stream_id: int, step: int, mean: float = 0.0, std: float = 1.0):
    _f32(out, name="out")
    lib = _lib.load()
    check(lib.pyz_fill_normal(ptr(out), out.numel(), int(seed), int(stream_id), int(step), float(mean), float(std),
                              _stream()))
    return out


def sample_normal_rows(out: torch.Tensor, col0: int, loc: torch.Tensor, scale: torch.Tensor, seed: int, first_draw: int):
    """out[r, col0:col0+len] = loc + scale * z_r for every row r of the (n, stride) CUDA matrix `out`."""
    lib = _lib.load()
    _f32(out, name="out")
    _f32(loc, name="loc")
    _f32(scale, (loc.numel(),), "scale")
    assert out.dim() == 2
    check(lib.pyz_sample_normal_rows(ptr(out), out.shape[0], out.shape[1], int(col0), loc.numel(), ptr(loc), ptr(scale),
                                     int(seed), _lib.STREAM_PREDICT, int(first_draw) & 0xFFFFFFFF, _stream()))


def sample_lowrank_rows(out: torch.Tensor, col0: int, mean: torch.Tensor, diag: torch.Tensor, dev: torch.Tensor,
                        factor: float, seed: int, first_draw: int):
    """out[r, col0:col0+len] = mean + diag * z1_r + factor * (z2_r @ dev) for every row r of the (n, stride) CUDA matrix
    `out`; dev is (k, len), z1_r (len) and z2_r (k) come from draw first_draw + r of the predict stream."""
    lib = _lib.load()
    _f32(out, name="out")
    _f32(mean, name="mean")
    _f32(diag, (mean.numel(),), "diag")
    _f32(dev, name="dev")
    assert out.dim() == 2
    if dev.dim() != 2 or dev.shape[1] != mean.numel():
        raise ValueError(f"dev must be (k, {mean.numel()}), not {tuple(dev.shape)}")
    check(lib.pyz_sample_lowrank_rows(ptr(out), out.shape[0], out.shape[1], int(col0), mean.numel(), ptr(mean), ptr(diag),
                                      ptr(dev), int(dev.shape[0]), float(factor), int(seed), _lib.STREAM_PREDICT,
                                      int(first_draw) & 0xFFFFFFFF, _stream()))


def gather_rows(out: torch.Tensor, col0: int, bank: torch.Tensor, idx):
    """out[r, col0:col0+len] = bank[idx[r]] for every row r of the (n, stride) CUDA matrix `out`; bank is a CUDA
    (n_bank, len) matrix, idx n HOST integers (checked against n_bank here, then uploaded)."""
    lib = _lib.load()
    _f32(out, name="out")
    _f32(bank, name="bank")
    assert out.dim() == 2
    if bank.dim() != 2 or bank.shape[0] < 1:
        raise ValueError("bank must be a (rows >= 1, len) matrix")
    idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(-1))
    if idx.shape[0] != out.shape[0]:
        raise ValueError(f"{idx.shape[0]} indices for the {out.shape[0]} rows of out")
    if idx.size and (idx.min() < 0 or idx.max() >= bank.shape[0]):
        raise IndexError(f"index outside the bank's {bank.shape[0]} rows")
    idx_d = torch.as_tensor(idx.astype(np.int32)).to(out.device)
    check(lib.pyz_gather_rows(ptr(out), out.shape[0], out.shape[1], int(col0), bank.shape[1], ptr(bank), bank.shape[0],
                              ptr(idx_d), _stream()))


def grid_rows(basis: torch.Tensor, a0: float, da: float, n1: int, b0: float, db: float, n2: int, row0: int = 0, n=None):
    """(n, d) CUDA float32: rows [row0, row0 + n) of the n1 x n2 grid ('ij' order: row r is (r // n2, r % n2)) with
    u = a0 + i * da, v = b0 + j * db, mapped to input space as u * basis[:, 0] + v * basis[:, 1]; basis is a CUDA (d, 2)
    matrix.  Every operation is rounded to float32 on its own (pyz_grid_rows)."""
    lib = _lib.load()
    _f32(basis, name="basis")
    if basis.dim() != 2 or basis.shape[1] != 2 or basis.shape[0] < 1:
        raise ValueError(f"basis must be (d >= 1, 2), not {tuple(basis.shape)}")
    n1, n2, row0 = int(n1), int(n2), int(row0)
    if n1 < 1 or n2 < 1:
        raise ValueError(f"the grid must be at least 1 x 1, not {n1} x {n2}")
    n = n1 * n2 - row0 if n is None else int(n)
    if row0 < 0 or n < 1 or row0 + n > n1 * n2:
        raise ValueError(f"rows [{row0}, {row0 + n}) outside the {n1} x {n2} grid")
    out = torch.empty((n, basis.shape[0]), dtype=torch.float32, device=basis.device)
    check(lib.pyz_grid_rows(ptr(basis), int(basis.shape[0]), float(a0), float(da), n1, float(b0), float(db), n2, row0, n,
                            ptr(out), _stream()))
    return out


CORRUPTION_KINDS = 10          # PYZ_CORRUPT_KINDS: 0..8 the image corruptions of Robustness.py:10-93, 9 the regression noise


def corrupt_rows(x: torch.Tensor, shape, kind: int, severities, pixel_max: float = 255.0, quantise: bool = True, seed: int = 0):
    """(len(severities), n, row length) CUDA float32: the rows of x (n, h * w * ch) under corruption `kind` at every listed
    severity (1..5), one launch (pyz_corrupt_rows).  shape = (h, w, ch), ch 1 or 3; kind 9 (x + c z on rows of any
    length): shape = (1, row length, 1)."""
    lib = _lib.load()
    _f32(x, name="x")
    h, w, ch = (int(v) for v in shape)
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] != h * w * ch:
        raise ValueError(f"x must be (rows >= 1, {h * w * ch}) for shape {(h, w, ch)}, not {tuple(x.shape)}")
    sev = [int(s) for s in severities]
    if not 1 <= len(sev) <= 5 or any(not 1 <= s <= 5 for s in sev):
        raise ValueError(f"severities must be one to five values in 1..5, not {sev}")
    if not 0 <= int(kind) < CORRUPTION_KINDS:
        raise ValueError(f"kind {kind} outside [0, {CORRUPTION_KINDS})")
    out = torch.empty((len(sev), x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
    check(lib.pyz_corrupt_rows(ptr(x), x.shape[0], h, w, ch, int(kind), (C.c_int32 * len(sev))(*sev), len(sev),
                               float(pixel_max), 1 if quantise else 0, int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(out), _stream()))
    return out


def score_rows(mean: torch.Tensor, y: torch.Tensor, kind: int):
    """Scores of `groups` read-outs mean (groups, n, C) (pyz_score_rows).  kind 0: y int32 (n,) labels -> int64 (groups,),
    the rows whose predicted class (np.argmax; mean > 0.5 for C == 1) is wrong.  kind 1: y float32 (n, C) -> float64
    (groups, C), the sums over rows of (mean - y)^2."""
    lib = _lib.load()
    _f32(mean, name="mean")
    if mean.dim() != 3 or min(mean.shape) < 1:
        raise ValueError(f"mean must be (groups, n, C), not {tuple(mean.shape)}")
    groups, n, C_out = (int(v) for v in mean.shape)
    if not isinstance(y, torch.Tensor) or not y.is_cuda or not y.is_contiguous():
        raise TypeError("y must be a contiguous CUDA(HIP) torch tensor")
    if kind == 0:
        if y.dtype != torch.int32 or y.numel() != n:
            raise TypeError("labels must be CUDA int32, one per row")
        out = torch.empty((groups,), dtype=torch.int64, device=mean.device)
    elif kind == 1:
        _f32(y, name="y")
        if y.numel() != n * C_out:
            raise ValueError("targets must be (rows, out)")
        out = torch.empty((groups, C_out), dtype=torch.float64, device=mean.device)
    else:
        raise ValueError("kind must be 0 (classification) or 1 (regression)")
    check(lib.pyz_score_rows(ptr(mean), groups, n, C_out, ptr(y), int(kind), ptr(out), _stream()))
    return out

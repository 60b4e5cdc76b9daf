"""SWAG's posterior: diagonal + low-rank Gaussian (mirrors
Pyesian/distributions/MultivariateNormalDiagPlusLowRank.py:11-41): ``sample = mean + z1 + D z2 *
sqrt(1/(2(k-1)))`` with ``z1 ~ N(0, scale=diag)`` (diag is used as the scale, as written) and
``z2 ~ N(0, I_k)``."""

import json
import os
from math import sqrt

import numpy as np

from . import tfd
from .Distribution import Distribution


class MultivariateNormalDiagPlusLowRank(Distribution):
    def __init__(self, mean, diag, D):
        mean = np.asarray(mean, dtype=np.float32)
        super().__init__(mean.shape[0])
        self._mean = mean
        self._D = np.asarray(D, dtype=np.float32).reshape(mean.shape[0], -1)
        self._diag = np.asarray(diag, dtype=np.float32)

    def sample_n(self, n: int):
        k = self._D.shape[1]
        z1 = tfd._rng.standard_normal((n, self._size), dtype=np.float32) * self._diag
        z2 = tfd._rng.standard_normal((n, k), dtype=np.float32)
        return (self._mean[None, :] + z1 + (z2 @ self._D.T) * np.float32(sqrt(1 / (2 * (k - 1))))).astype(np.float32)

    def sample_n_device(self, n: int, out, col0: int) -> bool:
        """n draws into columns [col0, col0 + size) of the CUDA matrix `out`, generated on the device from the Philox
        stream of tfd.seed (k_sample_lowrank_rows); True when done.  False (the caller draws on the host with
        ``sample_n``) with PYZ_SAMPLE_DEVICE=0, for more than PYZ_LOWRANK_MAX_K deviation columns and for n outside 1 .. 65535."""
        if os.environ.get("PYZ_SAMPLE_DEVICE", "1") == "0":
            return False
        k = self._D.shape[1]
        factor = sqrt(1 / (2 * (k - 1)))               # (k = 1: ZeroDivisionError, k = 0: ValueError, as in sample_n)
        from .._lib import LOWRANK_MAX_K
        if k > LOWRANK_MAX_K or not 1 <= n <= 65535:   # (one launch takes at most that many rows)
            return False
        import torch
        from .. import engine
        if getattr(self, "_dev", None) is None:
            diag = np.array(np.broadcast_to(self._diag, self._mean.shape))
            self._dev = (torch.as_tensor(self._mean).cuda(), torch.as_tensor(diag).cuda(),
                         torch.as_tensor(np.ascontiguousarray(self._D.T)).cuda())      # (k, size): row c = column c of D
        engine.sample_lowrank_rows(out, col0, self._dev[0], self._dev[1], self._dev[2], factor, tfd._dev_seed,
                                   tfd.take_device_draws(n))
        return True

    def sample(self):
        return self.sample_n(1)[0]

    def store(self, path: str):
        data = json.dumps({"mean": self._mean.tolist(), "D": self._D.tolist(), "diag": self._diag.tolist()})
        with open(os.path.join(path, "distribution.json"), "w") as f:
            f.write(data)

    @classmethod
    def load(cls, path: str) -> "Distribution":
        with open(os.path.join(path, "distribution.json"), "r") as f:
            d = json.load(f)
        return MultivariateNormalDiagPlusLowRank(np.asarray(d["mean"]), np.asarray(d["diag"]), np.asarray(d["D"]))

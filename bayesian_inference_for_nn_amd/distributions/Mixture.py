"""Finite mixture of result distributions -- the posterior of a MultiSWAG run (Wilson & Izmailov 2020: a mixture of
the SWAG Gaussians of independently trained members).  An extension: the reference has no mixture.

A draw picks a component the way ``Sampled`` picks a sample (cumulative integer frequencies, ``random.randint`` +
``bisect_left``) and then draws from it."""

import bisect
import json
import os
import random

import numpy as np

from .Distribution import Distribution


def _builtin_classes():
    from .MultivariateNormalDiagPlusLowRank import MultivariateNormalDiagPlusLowRank
    from .Sampled import Sampled
    from .tf import TensorflowProbabilityDistribution
    return {"Sampled": Sampled, "TensorflowProbabilityDistribution": TensorflowProbabilityDistribution,
            "MultivariateNormalDiagPlusLowRank": MultivariateNormalDiagPlusLowRank, "Mixture": Mixture}


class Mixture(Distribution):
    def __init__(self, components, frequencies=None):
        components = list(components)
        if len(components) == 0:
            raise ValueError("Can't have distribution Mixture with 0 components")
        size = int(components[0].size)
        if any(int(c.size) != size for c in components):
            raise ValueError("The components of a Mixture must have the same size")
        super().__init__(size)
        if frequencies is None:
            frequencies = [1] * len(components)
        if len(frequencies) != len(components):
            raise ValueError("Number of components and list frequency do not have the same size")
        self._components = components
        self._frequencies = [int(f) for f in frequencies]
        self._acc_frequencies = []
        acc = 0
        for f in self._frequencies:
            if f <= 0:
                raise ValueError("Component frequencies must be positive")
            acc += f
            self._acc_frequencies.append(acc)

    @property
    def components(self):
        return list(self._components)

    def sample_index(self) -> int:
        w = random.randint(1, self._acc_frequencies[-1])
        return bisect.bisect_left(self._acc_frequencies, w)

    def sample(self):
        return np.asarray(self._components[self.sample_index()].sample(), dtype=np.float32)

    @staticmethod
    def _rows_of(idx):
        """component -> the rows it was drawn for, components in ascending order."""
        rows = {}
        for r, c in enumerate(idx):
            rows.setdefault(c, []).append(r)
        return sorted(rows.items())

    def sample_n(self, n: int):
        """(n, size) float32: the n component indices are drawn first (n calls of ``sample_index``), then every component
        that was drawn gives its rows in one ``sample_n`` call, components in ascending order: row r comes from component
        idx[r]."""
        idx = [self.sample_index() for _ in range(n)]
        out = np.empty((n, self._size), dtype=np.float32)
        for c, rows in self._rows_of(idx):
            out[rows] = np.asarray(self._components[c].sample_n(len(rows)), dtype=np.float32)[:, :self._size]
        return out

    def sample_n_device(self, n: int, out, col0: int) -> bool:
        """n draws into columns [col0, col0 + size) of the CUDA matrix `out`.  The indices are drawn on the host exactly as
        ``sample_n`` draws them; every component that was drawn writes its rows into a (n, size) scratch matrix on the
        device -- with its own ``sample_n_device`` or, when it has none or declines, ``sample_n`` and an upload --, and
        the rows are placed into `out` by one device gather (k_gather_rows).  True when done.  False (the caller draws on
        the host with ``sample_n``) under the conditions ``Sampled`` declines: PYZ_SAMPLE_DEVICE=0, a scratch matrix
        beyond PYZ_SAMPLED_BANK_MAX bytes, n outside 1 .. 65535."""
        if os.environ.get("PYZ_SAMPLE_DEVICE", "1") == "0":
            return False
        if not 1 <= n <= 65535:                        # (one launch takes at most that many rows)
            return False
        if 4 * n * self._size > int(os.environ.get("PYZ_SAMPLED_BANK_MAX", 1 << 33)):
            return False
        import torch
        from .. import engine
        idx = [self.sample_index() for _ in range(n)]
        scratch = torch.empty((n, self._size), dtype=torch.float32, device=out.device)
        where = [0] * n                                # row r of out <- row where[r] of the scratch
        r0 = 0
        for c, rows in self._rows_of(idx):
            comp, block = self._components[c], scratch[r0:r0 + len(rows)]
            draw = getattr(comp, "sample_n_device", None)
            if draw is None or not draw(len(rows), block, 0):
                host = np.asarray(comp.sample_n(len(rows)), dtype=np.float32)[:, :self._size]
                block.copy_(torch.as_tensor(np.ascontiguousarray(host)))
            for j, r in enumerate(rows):
                where[r] = r0 + j
            r0 += len(rows)
        engine.gather_rows(out, col0, scratch, where)
        return True

    def store(self, path: str):
        """mixture.json (frequencies and the components' class names) + component<i>/, written by component i's store."""
        info = {"size": self._size, "frequencies": self._frequencies,
                "components": [c.__class__.__name__ for c in self._components]}
        with open(os.path.join(path, "mixture.json"), "w") as f:
            f.write(json.dumps(info))
        for i, c in enumerate(self._components):
            sub = os.path.join(path, "component" + str(i))
            os.makedirs(sub, exist_ok=True)
            c.store(sub)

    @classmethod
    def load(cls, path: str) -> "Distribution":
        """The component class names are resolved against the built-in distributions."""
        with open(os.path.join(path, "mixture.json"), "r") as f:
            info = json.load(f)
        register = _builtin_classes()
        components = []
        for i, name in enumerate(info["components"]):
            if name not in register:
                raise ValueError(f"mixture component {i} is a {name!r}: not a built-in distribution")
            components.append(register[name].load(os.path.join(path, "component" + str(i))))
        return Mixture(components, info["frequencies"])

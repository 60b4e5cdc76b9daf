"""CPU-side checks of the device draws of SWAG's and HMC's result distributions: pyz_sample_lowrank_rows and
pyz_gather_rows are declared, typed and refuse bad arguments before any device is touched; the Python methods keep the
host path's errors and hand back to the host path when told to."""

import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
P = C.c_void_p(4096)        # a non-null "device pointer": every call below must fail before it is looked at


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pyz.h")).read(), flags=re.S)


def max_k():
    return int(re.search(r"#define\s+PYZ_LOWRANK_MAX_K\s+(\d+)", header_text()).group(1))


def test_header_and_ctypes_table_list_both_entry_points():
    from bayesian_inference_for_nn_amd import _lib
    names = set(re.findall(r"\b(pyz_[a-z0-9_]+)\s*\(", header_text()))
    for name, n_args in (("pyz_sample_lowrank_rows", 14), ("pyz_gather_rows", 9)):
        assert name in names and name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args
        assert hasattr(_lib.load(), name)
    assert _lib.LOWRANK_MAX_K == max_k() >= 20          # (20: the SWAG paper's rank)
    assert _lib.header_version() == 302


def lowrank_args(**kw):
    a = dict(out=P, n_rows=3, row_stride=20, col0=2, len=10, mean=P, diag=P, dev=P, k=3, factor=0.5)
    a.update(kw)
    return (a["out"], a["n_rows"], a["row_stride"], a["col0"], a["len"], a["mean"], a["diag"], a["dev"], a["k"], a["factor"],
            7, 4, 0, None)


def gather_args(**kw):
    a = dict(out=P, n_rows=3, row_stride=20, col0=2, len=10, bank=P, n_bank=5, idx=P)
    a.update(kw)
    return (a["out"], a["n_rows"], a["row_stride"], a["col0"], a["len"], a["bank"], a["n_bank"], a["idx"], None)


LOWRANK_BAD = [("null out", dict(out=None)), ("null mean", dict(mean=None)), ("null diag", dict(diag=None)),
               ("null dev", dict(dev=None)), ("no rows", dict(n_rows=0)), ("too many rows", dict(n_rows=65536)),
               ("columns past the row", dict(col0=11)), ("negative col0", dict(col0=-1)), ("no columns", dict(len=0)),
               ("k = 0", dict(k=0)), ("k above the cap", dict(k=None))]
GATHER_BAD = [("null out", dict(out=None)), ("null bank", dict(bank=None)), ("null idx", dict(idx=None)),
              ("no rows", dict(n_rows=0)), ("too many rows", dict(n_rows=65536)), ("columns past the row", dict(col0=11)),
              ("negative col0", dict(col0=-1)), ("no columns", dict(len=0)), ("empty bank", dict(n_bank=0))]


@pytest.mark.parametrize("what,kw", LOWRANK_BAD, ids=[w for w, _ in LOWRANK_BAD])
def test_lowrank_refuses_bad_arguments_without_a_device(what, kw):
    from bayesian_inference_for_nn_amd import _lib
    lib = _lib.load()
    if "k" in kw and kw["k"] is None:
        kw = dict(k=max_k() + 1)
    assert lib.pyz_sample_lowrank_rows(*lowrank_args(**kw)) == E_INVALID, what
    assert lib.pyz_last_error(), what


@pytest.mark.parametrize("what,kw", GATHER_BAD, ids=[w for w, _ in GATHER_BAD])
def test_gather_refuses_bad_arguments_without_a_device(what, kw):
    from bayesian_inference_for_nn_amd import _lib
    lib = _lib.load()
    assert lib.pyz_gather_rows(*gather_args(**kw)) == E_INVALID, what
    assert lib.pyz_last_error(), what


def test_lowrank_device_draw_keeps_the_host_errors_for_k_1_and_k_0(monkeypatch):
    from bayesian_inference_for_nn_amd.distributions import MultivariateNormalDiagPlusLowRank
    monkeypatch.delenv("PYZ_SAMPLE_DEVICE", raising=False)
    mean, diag = np.zeros(6, np.float32), np.ones(6, np.float32)
    one = MultivariateNormalDiagPlusLowRank(mean, diag, np.ones((6, 1), np.float32))
    with pytest.raises(ZeroDivisionError):
        one.sample_n(2)
    with pytest.raises(ZeroDivisionError):
        one.sample_n_device(2, None, 0)              # before any launch: `out` is never looked at
    none = MultivariateNormalDiagPlusLowRank(mean, diag, np.ones((6, 0), np.float32))
    with pytest.raises(ValueError):
        none.sample_n(2)
    with pytest.raises(ValueError):
        none.sample_n_device(2, None, 0)


def test_more_deviation_columns_than_the_cap_go_to_the_host_path(monkeypatch):
    from bayesian_inference_for_nn_amd.distributions import MultivariateNormalDiagPlusLowRank
    monkeypatch.delenv("PYZ_SAMPLE_DEVICE", raising=False)
    wide = MultivariateNormalDiagPlusLowRank(np.zeros(3, np.float32), np.ones(3, np.float32),
                                             np.ones((3, max_k() + 1), np.float32))
    assert wide.sample_n_device(2, None, 0) is False            # (`out` is never looked at)
    assert wide.sample_n(2).shape == (2, 3)


SWITCHED_OFF = """
import random, sys
import numpy as np
from bayesian_inference_for_nn_amd.distributions import MultivariateNormalDiagPlusLowRank, Sampled
mvn = MultivariateNormalDiagPlusLowRank(np.zeros(6, np.float32), np.ones(6, np.float32), np.ones((6, 3), np.float32))
smp = Sampled([np.zeros(6, np.float32), np.ones(6, np.float32)], [1, 2])
random.seed(5)
state = random.getstate()
assert mvn.sample_n_device(4, None, 0) is False
assert smp.sample_n_device(4, None, 0) is False
assert random.getstate() == state, "the refused call consumed host random numbers"
assert not hasattr(smp, "_bank") or smp._bank is None
assert "torch" not in sys.modules, "torch was imported"
print("ok")
"""


@pytest.mark.parametrize("env", [{"PYZ_SAMPLE_DEVICE": "0"}, {"PYZ_SAMPLE_DEVICE": "0", "PYZ_SAMPLED_BANK_MAX": "1"}],
                         ids=["switch", "switch and bank cap"])
def test_switched_off_both_methods_return_false_without_importing_torch(env):
    res = subprocess.run([sys.executable, "-c", SWITCHED_OFF], cwd=ROOT, env={**os.environ, **env}, capture_output=True,
                         text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr


def test_bank_cap_alone_sends_sampled_to_the_host_path_without_importing_torch():
    code = SWITCHED_OFF.replace("assert mvn.sample_n_device(4, None, 0) is False\n", "")
    env = {k: v for k, v in os.environ.items() if k != "PYZ_SAMPLE_DEVICE"}
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env={**env, "PYZ_SAMPLED_BANK_MAX": "1"},
                         capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr

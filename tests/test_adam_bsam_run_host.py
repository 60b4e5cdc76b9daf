"""Host side of the device-resident ADAM / VADAM / BSAM runs (pyz_adam_run, pyz_bsam_run): the entry points in the header
and the ctypes table, their refusal of a NULL plan without a GPU, the epoch counts a chunk of a quiet train() hands to
the library, and the float32 running-loss fold that must leave `_running_dev` as the step loop does."""

import ctypes
import os
import re

import numpy as np
import pytest

from bayesian_inference_for_nn_amd import _lib
from bayesian_inference_for_nn_amd.optimizers.ADAM import fold_running, run_epochs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pyz_adam_run", "pyz_bsam_run")


def header_arity(name):
    src = open(os.path.join(ROOT, "include", "pyz.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/pyz.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", NAMES)
def test_declared_in_header_and_ctypes_table_with_matching_arity(name):
    assert name in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int
    assert len(argtypes) == header_arity(name) == {"pyz_adam_run": 24, "pyz_bsam_run": 22}[name]
    assert _lib.header_version() == 302                                  # the new entry points do not move the version


@pytest.mark.parametrize("name", NAMES)
def test_null_plan_is_refused_without_a_gpu(name):
    lib = _lib.load()
    args = []
    for t in _lib.SIGNATURES[name][1]:
        if t in (ctypes.c_float, ctypes.c_double):
            args.append(0.5)
        elif t in (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64):
            args.append(1)
        else:
            args.append(None)
    assert getattr(lib, name)(*args) == -1                               # PYZ_E_INVALID
    assert b"null plan" in lib.pyz_last_error()


def step_loop_epochs(epoch_num, new_epoch_flags):
    """What _adam_step does (ADAM.py:49-55): the count goes up BEFORE the update of a step that opens an epoch."""
    out = []
    for new in new_epoch_flags:
        if new:
            epoch_num += 1
        out.append(epoch_num)
    return out


@pytest.mark.parametrize("epoch_num,starts,n", [
    (1, [], 5),                       # no boundary inside the chunk
    (3, [], 1),
    (1, [0], 4),                      # the chunk's first step opens an epoch
    (2, [0, 3, 6], 8),                # several, the first at step 0
    (7, [2, 5], 6),                   # ... and the last at the chunk's last step
    (1, [1, 2, 3], 4),                # one batch per epoch
])
def test_chunk_epochs_equal_the_step_loop(epoch_num, starts, n):
    flags = [s in starts for s in range(n)]
    got = run_epochs(epoch_num, starts, n)
    assert got == step_loop_epochs(epoch_num, flags)
    assert len(got) == n and got[-1] == epoch_num + len(starts) and all(isinstance(e, int) and e >= 1 for e in got)


def step_loop_running(running, losses, new_epoch_flags):
    """`_running_dev` of the step loop: a float32 tensor, zeroed at an epoch start, `+=` one step after the other."""
    r = np.float32(running)
    for l, new in zip(losses, new_epoch_flags):
        if new:
            r = np.float32(0.0)
        r = np.float32(r + (np.float32(l) if np.ndim(l) == 0 else np.float32(np.float32(l[0]) + np.float32(l[1]))))
    return r


@pytest.mark.parametrize("starts", [[], [0], [4], [3, 250, 611]])
@pytest.mark.parametrize("pairs", [False, True])
def test_running_loss_fold_equals_the_step_loop(starts, pairs):
    rng = np.random.default_rng(5)
    n = 1000
    # magnitudes spread over six decades: a pairwise or float64 sum rounds differently from the sequential float32 one
    losses = (rng.uniform(0.1, 3.0, size=(n, 2) if pairs else n) * 10.0 ** rng.integers(-3, 3, size=(n, 2) if pairs else n))
    losses = losses.astype(np.float32)
    flags = [s in starts for s in range(n)]
    want = step_loop_running(0.37, losses, flags)
    got = fold_running(np.float32(0.37), losses, starts[-1] if starts else None)
    assert got.dtype == np.float32 and got.tobytes() == np.float32(want).tobytes()

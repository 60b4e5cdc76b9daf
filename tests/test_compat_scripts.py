"""N1 (BASELINE.json north_star: "BBB_mnist.py / HMC_classification.py run unchanged"): every module / name the
two named driver scripts of the reference import resolves under the `compat/` stand-ins (tensorflow stand-in,
Pyesian -> this package, sklearn, numpy).

The scripts' import statements are held as names only in tests/golden/reference_script_imports.json (the reference's
source is not part of this repository).  The whole flow -- compile, train, result, predict, Metrics / Plotter -- is
exercised on the GPU by tests/test_gpu_surface.py::test_compat_* with a driver written in the same style."""

import importlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPORTS = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_script_imports.json")))["scripts"]
SCRIPTS = ("BBB_mnist.py", "HMC_classification.py")


@pytest.fixture()
def compat_path(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "compat"))
    for name in [n for n in sys.modules if n == "tensorflow" or n.startswith("tensorflow.") or n == "Pyesian" or n.startswith("Pyesian.")]:
        monkeypatch.delitem(sys.modules, name)
    yield
    for name in [n for n in sys.modules if n == "tensorflow" or n.startswith("tensorflow.") or n == "Pyesian" or n.startswith("Pyesian.")]:
        sys.modules.pop(name, None)


@pytest.mark.parametrize("script", SCRIPTS)
def test_import_set_of_the_named_script_resolves(script, compat_path):
    seen = 0
    for module, names in IMPORTS[script]:
        mod = importlib.import_module(module)
        if not names:                                   # `import module`
            seen += 1
        for name in names:                              # `from module import name, ...`
            assert hasattr(mod, name), f"{script}: from {module} import {name}"
            seen += 1
    assert seen >= 8
    import tensorflow as tf
    assert "standin" in tf.__version__            # the stand-in, not a TensorFlow that appeared on the path

import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wavelet-transformer_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run via gpurun)")


@pytest.fixture(scope="session")
def pywt_filters():
    with open(os.path.join(GOLDEN, "pywt_filters.json")) as f:
        return json.load(f)["filters"]


@pytest.fixture(scope="session")
def db4(pywt_filters):
    return {k: np.asarray(v) for k, v in pywt_filters["db4"].items()}


@pytest.fixture(scope="session")
def modwt_golden():
    # one fixture in two files (each under the 1 MiB limit for a committed file): the cases
    # of n = 4096 are in the second
    return {**np.load(os.path.join(GOLDEN, "modwt_golden.npz")),
            **np.load(os.path.join(GOLDEN, "modwt_golden_4096.npz"))}


@pytest.fixture(scope="session")
def dwt_golden():
    return np.load(os.path.join(GOLDEN, "dwt_golden.npz"))


def gpu_available():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def pytest_collection_modifyitems(config, items):
    if gpu_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this environment")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)

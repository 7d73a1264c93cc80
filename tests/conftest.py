import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# torch before any test loads the library (hashmergejoin_amd._lib.load_library), as build() does: the other way round
# the process holds two HIP runtimes -- torch asks for libamdhip64.so from its own lib/, the library for
# libamdhip64.so.7 -- and once torch's runtime has the GPU, hmj_create reports no usable HIP device.  A run of the
# whole suite loads the library in CPU tests (test_cabi_cpu.py) before the GPU tests need it.
try:
    import torch  # noqa: F401
except ImportError:
    pass


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    from oracle.pyoracle import Oracle

    return Oracle()


@pytest.fixture(scope="session")
def reference():
    """The real reference's results: recorded in tests/golden/ref_calls.json, and also computed by oracle/_ref's
    compiled reference where `make -C oracle ref` could build it (its results must then equal the record)."""
    import json

    from oracle.pyoracle import RecordedReference, Reference

    with open(os.path.join(ROOT, "tests", "golden", "ref_calls.json")) as f:
        calls = json.load(f)["calls"]
    ref = Reference()
    return RecordedReference(calls, live=ref if ref.available else None)


@pytest.fixture(scope="session")
def golden_dir():
    return os.path.join(ROOT, "tests", "golden")

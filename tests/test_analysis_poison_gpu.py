"""The analysis pipelines under the poisoning allocator on a real MI355X (tests/analysis_pipeline_cases.py): every case runs
plainly, then with every torch.empty / torch.empty_like of the wrapper modules AND of the pipeline modules handed out filled with
0xFF (NaN in the float types, -1 in the integers) and with 0x3C (small finite values; 0x3C3C3C3C in an int32).  The pipelines are
documented as functions of their arguments, bit for bit, so every returned array must equal the plain run's bit for bit: a buffer
element read before any kernel or torch op wrote it -- between two calls of a pipeline, where the per-kernel suites cannot look --
would differ under one of the two.  The table in the case module's docstring is the reading of the 56 allocations this holds to
the device; it found no element read unwritten, and neither did these runs."""
import numpy as np
import pytest
import torch

from tests import analysis_pipeline_cases as A
from tests import write_set_cases as W

pytestmark = pytest.mark.gpu

MODULES = W.WRAPPER_MODULES + W.ANALYSIS_MODULES


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from variantformer_amd import _lib as lib
    lib.load()      # must be the in-tree HIP library; raises if missing


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _drive(case):
    inputs = case.build()
    try:
        plain = case.run(inputs)
        torch.cuda.synchronize()
        for key in case.finite:
            assert np.isfinite(plain[key]).all(), f"{case.name}: {key} of the plain run is not finite"
        counts = {}
        for pattern in (0xFF, 0x3C):
            with W.poison_allocations(pattern, keep=False, modules=MODULES) as px:
                got = case.run(inputs)
                torch.cuda.synchronize()
            assert px.count > 0, f"{case.name}: nothing was allocated through the patched modules"
            counts[pattern] = px.count
            assert set(got) == set(plain)
            for key, want in plain.items():
                assert _same_bits(got[key], want), (f"{case.name}: {key} under {pattern:#04x} poison differs from the plain run "
                                                    f"(an element read before it was written)")
        assert counts[0xFF] == counts[0x3C], counts                          # the same path both times
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):       # a faulted device: launch nothing more on it
            pytest.exit(f"GPU fault in {case.name}: {e}", returncode=3)
        raise


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_pipeline_under_poisoned_allocations(case):
    _drive(case)

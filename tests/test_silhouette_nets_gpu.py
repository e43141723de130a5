"""The nets of the analysis pipelines, over the silhouette entries (they cannot be extended in place: tests/write_set_cases.py,
tests/analysis_pipeline_cases.py and tests/test_analysis_streams_gpu.py are yardsticks).

Write sets: each of the three entries through write_set_cases.check_write_set: operands as interior slices of poisoned buffers,
outputs inside poisoned arenas, under 0xFF, 0x00 and 0x3C; the bytes inside the documented write set are equal under the three
patterns and equal the restatement, every byte outside it keeps its pattern.

Poison: the pipeline calls of variantformer_amd/validation.py run plainly, then with every torch.empty of that module (named
explicitly) handing out memory filled with 0xFF and with 0x3C; every returned array must be equal bit for bit: no element is read
before the launch that writes it (the table in tests/silhouette_cases.py's docstring says which launch that is).

Streams: each of the three entries, and the pipeline, on a side stream behind the delay and the late copy of the fresh operands,
over buffers that hold a stale but valid operand set: the protocol, the delay, the probed side stream and the canary are those
of tests/test_analysis_streams_gpu.py, imported from there and called with the cases below."""
import os

import numpy as np
import pytest
import torch

from tests import analysis_pipeline_cases as A
from tests import kmeans_cases as K
from tests import silhouette_cases as C
from tests import test_analysis_streams_gpu as S
from tests import write_set_cases as W
from tests.conftest import REPO
from tests.test_analysis_streams_gpu import delay, side  # noqa: F401  (the module's fixtures, instantiated for this module)

pytestmark = pytest.mark.gpu

MODULES = ("variantformer_amd.validation",)
R, D, KC, ROW0, ROWS = 150, 5, 4, 3, 90           # the range starts off a multiple of 64 and holds the rows without a label


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from variantformer_amd import _lib as lib
    lib.load()      # must be the in-tree HIP library; raises if missing


def _ops():
    from variantformer_amd import ops
    return ops


def _np(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _operands():
    x, lab = C.device_case(R, D, KC, 3)                                   # finite rows; rows 5 and 6 have no label, id 3 is empty
    order, seg = C.csr(lab, KC)
    return x, lab, order, seg


# ---- write sets ----------------------------------------------------------------------------------------------------------------------
def _guarded_operands(p, x, lab, order, seg):
    t = torch.from_numpy
    return W.guarded(t(x), p, cols=W.GUARD_COLS), W.guarded(t(lab), p), W.guarded(t(order), p), W.guarded(t(seg), p)


@pytest.mark.parametrize("family", ("l2", "dot"))
def test_write_set_of_the_sums(family):
    x, lab, order, seg = _operands()
    if family == "l2":
        want = C.sums_l2(x, order, seg, ROW0, ROWS)
    else:
        want, want_m = C.sums_dot(x, order, seg, lab, ROW0, ROWS)
    extra = 7

    def run(p):
        xd, ld, od, sd = _guarded_operands(p, x, lab, order, seg)
        big, view = W.arena(KC, ROWS, torch.float64, p)
        if family == "l2":
            _ops().silhouette_sums_l2(xd, od, sd, ROW0, ROWS, S=view)
            return {"S": big}
        work = W.poisoned((KC * D + extra,), torch.float64, W.DEVICE, p)
        _ops().silhouette_sums_dot(xd, od, sd, ld, ROW0, ROWS, S=view, work=work)
        return {"S": big, "work": work}

    written = {"S": W.arena_mask(KC, ROWS)}
    if family == "dot":
        written["work"] = torch.arange(KC * D + extra) < KC * D

    def reference(out):
        assert C.same_bits(out["S"][8:8 + KC, W.GUARD_COLS:W.GUARD_COLS + ROWS].numpy(), want)
        if family == "dot":
            assert C.same_bits(out["work"][:KC * D].reshape(KC, D).numpy(), want_m)
    W.check_write_set(run, written, reference)


def test_write_set_of_finish():
    x, lab, order, seg = _operands()
    sums = C.sums_l2(x, order, seg, ROW0, ROWS)
    want = C.finish(sums, lab, seg, ROW0)
    names = ("a", "b", "s", "nearest")

    def run(p):
        _, ld, _, sd = _guarded_operands(p, x, lab, order, seg)
        Sd = W.guarded(torch.from_numpy(sums), p, cols=W.GUARD_COLS)
        outs = {n: W.poisoned((R,), torch.int32 if n == "nearest" else torch.float64, W.DEVICE, p) for n in names}
        _ops().silhouette_finish(Sd, ld, sd, ROW0, ROWS, **outs)
        return outs

    inside = (torch.arange(R) >= ROW0) & (torch.arange(R) < ROW0 + ROWS)
    nan_ok = {n: torch.from_numpy(np.concatenate([np.zeros(ROW0, bool), np.isnan(w), np.zeros(R - ROW0 - ROWS, bool)]))
              for n, w in zip(names[:3], want[:3])}
    assert bool(nan_ok["a"].any()) and not bool(nan_ok["b"].any()), "the rows without a label lie inside the range"

    def reference(out):
        for n, w in zip(names, want):
            assert C.same_bits(out[n][ROW0:ROW0 + ROWS].numpy(), w), n
    W.check_write_set(run, {n: inside for n in names}, reference, nan_ok)


# ---- poisoned allocations ------------------------------------------------------------------------------------------------------------
def _result_arrays(prefix, r):
    return {f"{prefix}.samples": _np(r.samples), f"{prefix}.a": _np(r.a), f"{prefix}.b": _np(r.b), f"{prefix}.nearest": _np(r.nearest_index),
            f"{prefix}.scalars": np.array([r.score], np.float64), f"{prefix}.means": r.cluster_means}


def _pipeline(x, lab):
    """Every allocating function of validation.py: _clusters and silhouette_samples, on both families, in one chunk and in many."""
    from variantformer_amd import validation as V
    out = {}
    out.update(_result_arrays("l2", V.silhouette_samples(x, lab, metric="euclidean")))
    out.update(_result_arrays("l2-chunks", V.silhouette_samples(x, lab, metric="euclidean", standardize="cosine", max_bytes=8 * 5 * 37)))
    out.update(_result_arrays("dot", V.silhouette_samples(x, lab, metric="correlation")))
    out.update(_result_arrays("dot-chunks", V.silhouette_samples(x, lab, metric="cosine", max_bytes=8 * 5 * 64)))
    sweep = V.silhouette_sweep(x, [3, 5], method="ward")
    out["sweep"] = np.array(sweep.scores)
    return out


def _pipeline_inputs():
    x = K.blobs(300, 12, 5, 0.6, 8)
    lab = (np.arange(300) % 5).astype(np.int64)
    lab[::29] = -1
    return x, lab


def test_poisoned_allocations_change_nothing():
    from variantformer_amd import validation
    x, lab = _pipeline_inputs()
    plain = _pipeline(x, lab)
    for pattern in (0xFF, 0x3C):
        with W.poison_allocations(pattern, modules=MODULES) as px:
            assert validation.torch is px
            got = _pipeline(x, lab)
            assert px.count >= 6 * 8 + 2, px.count                        # per call: labels, order, seg, a, b, s, nearest, S; work for the dot family
        assert validation.torch is torch
        S._assert_equal_results(got, plain, f"poisoned with {pattern:#x}")


# ---- every entry honours its stream ----------------------------------------------------------------------------------------------
def _l2_case():
    x, lab, order, seg = _operands()

    def call(b, o):
        _ops().silhouette_sums_l2(b["x"], b["order"], b["seg"], ROW0, ROWS, S=o["S"])
        return o
    return S.Built(dict(order=order, seg=seg), {"x": S._flip(x)}, {"x": x}, lambda: {"S": S._zeros((KC, ROWS), torch.float64)}, call, "x")


def _dot_case():
    x, lab, order, seg = _operands()

    def call(b, o):
        _ops().silhouette_sums_dot(b["z"], b["order"], b["seg"], b["labels"], ROW0, ROWS, S=o["S"], work=o["work"])
        return o
    return S.Built(dict(order=order, seg=seg, labels=lab), {"z": S._flip(x)}, {"z": x},
                   lambda: {"S": S._zeros((KC, ROWS), torch.float64), "work": S._zeros((KC * D,), torch.float64)}, call, "z")


def _finish_case():
    x, lab, order, seg = _operands()
    sums = C.sums_l2(x, order, seg, ROW0, ROWS)

    def call(b, o):
        _ops().silhouette_finish(b["S"], b["labels"], b["seg"], ROW0, ROWS, a=o["a"], b=o["b"], s=o["s"], nearest=o["nearest"])
        return o
    return S.Built(dict(labels=lab, seg=seg), {"S": np.ascontiguousarray(sums[:, ::-1])}, {"S": sums},
                   lambda: {"a": S._zeros((R,), torch.float64), "b": S._zeros((R,), torch.float64), "s": S._zeros((R,), torch.float64),
                            "nearest": S._zeros((R,), torch.int32)}, call, "S")


ENTRY_CASES = [S.EntryCase("vf_silhouette_sums_l2", _l2_case), S.EntryCase("vf_silhouette_sums_dot", _dot_case),
               S.EntryCase("vf_silhouette_finish", _finish_case)]


def test_the_stream_cases_name_every_entry_of_the_header():
    with open(os.path.join(REPO, "include", "vf_hip_silhouette.h")) as f:
        assert sorted(W.stream_entries(f.read())) == sorted(c.entry for c in ENTRY_CASES) == C.NAMES


@pytest.mark.parametrize("case", ENTRY_CASES, ids=lambda c: c.entry)
def test_entry_launches_on_the_current_stream(case, delay, side):  # noqa: F811
    S.test_entry_launches_on_the_current_stream(case, delay, side)


def _run_pipeline(inputs):
    from variantformer_amd import validation as V
    _, lab = _pipeline_inputs()
    out = _result_arrays("l2", V.silhouette_samples(inputs["x"], lab, metric="euclidean", max_bytes=8 * 5 * 100))
    out.update(_result_arrays("dot", V.silhouette_samples(inputs["x"], lab, metric="correlation")))
    return out


PIPELINE = A.PipelineCase("silhouette-blobs", lambda: {"x": _pipeline_inputs()[0]}, _run_pipeline,
                          ("validation.silhouette_samples", "validation._clusters"), ("l2.b", "dot.b"), "x")


def test_pipeline_behind_a_late_input_on_a_side_stream(delay, side):  # noqa: F811
    S.test_pipeline_behind_a_late_input_on_a_side_stream(PIPELINE, delay, side)

"""The two nets of the analysis pipelines, over k-means (they cannot be extended in place: tests/analysis_pipeline_cases.py and
tests/test_analysis_streams_gpu.py are yardsticks).

Poison: the pipeline calls of variantformer_amd/kmeans.py run plainly, then with every torch.empty of that module handing out
memory filled with 0xFF and with 0x3C (write_set_cases.poison_allocations); every returned array must be equal bit for bit: no
element is read before the launch that writes it (the table in tests/kmeans_cases.py's docstring says which launch that is).

Streams: each of the four entries, and the pipeline, on a side stream behind the delay and the late copy of the fresh operands,
over buffers that hold a stale but valid operand set: the protocol, the delay, the probed side stream and the canary are those
of tests/test_analysis_streams_gpu.py, imported from there and called with the cases below."""
import numpy as np
import pytest
import torch

from tests import analysis_pipeline_cases as A
from tests import kmeans_cases as K
from tests import test_analysis_streams_gpu as S
from tests import write_set_cases as W
from tests.test_analysis_streams_gpu import delay, side  # noqa: F401  (the module's fixtures, instantiated for this module)

pytestmark = pytest.mark.gpu

MODULES = ("variantformer_amd.kmeans",)
LLOYD_ITERATIONS = 2                       # vf_kmeans_lloyd: three launches per iteration and the last assignment


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from variantformer_amd import _lib as lib
    lib.load()      # must be the in-tree HIP library; raises if missing


def _np(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _model_arrays(prefix, m):
    return {f"{prefix}.labels": _np(m.labels), f"{prefix}.centers": _np(m.centers), f"{prefix}.counts": _np(m.counts), f"{prefix}.shift": _np(m.shift),
            f"{prefix}.scalars": np.array([m.inertia, m.n_iter], np.float64)}


def _pipeline(x):
    """Every allocating function of kmeans.py: seed_rows, _lloyd, _assign, and kmeans's own start buffers."""
    from variantformer_amd import kmeans
    out = {}
    out.update(_model_arrays("pp", kmeans.kmeans(x, 5, metric="correlation", init="k-means++", seed=3)))
    out.update(_model_arrays("random", kmeans.kmeans(x, 7, metric="euclidean", init="random", seed=3, n_init=2)))
    model = kmeans.kmeans(x, 4, metric="cosine", init=x[[0, 1, 2, 3]] / np.linalg.norm(x[[0, 1, 2, 3]], axis=1, keepdims=True), tol=0.0)
    out.update(_model_arrays("array", model))
    labels, dist = model.predict(x[::-1], chunk_rows=64, return_distance=True)
    out["predict.labels"], out["predict.dist"] = _np(labels), _np(dist)
    return out


def test_poisoned_allocations_change_nothing():
    from variantformer_amd import kmeans
    x = K.blobs(300, 12, 5, 0.6, 8)
    plain = _pipeline(x)
    for pattern in (0xFF, 0x3C):
        with W.poison_allocations(pattern, modules=MODULES) as px:
            assert kmeans.torch is px
            got = _pipeline(x)
            assert px.count >= 30, px.count                               # the seeding's four, Lloyd's eight per run, predict's two per call
        assert kmeans.torch is torch
        S._assert_equal_results(got, plain, f"poisoned with {pattern:#x}")


# ---- every entry honours its stream ----------------------------------------------------------------------------------------------
def _ops():
    from variantformer_amd import ops
    return ops


def _fixture():
    f = K.fixture("C-k7")
    x = f.make()
    return x, x[list(f.start)]


def _assign_case():
    x, cen = _fixture()

    def call(b, o):
        _ops().kmeans_assign(b["x"], b["cen"], labels=o["labels"], dist=o["dist"])
        return o
    return S.Built(dict(cen=cen), {"x": S._flip(x)}, {"x": x},
                   lambda: {"labels": S._zeros((x.shape[0],), torch.int32), "dist": S._zeros((x.shape[0],))}, call, "x")


def _update_case():
    x, cen = _fixture()
    labels = K.assign(x, cen)[0]

    def call(b, o):
        _ops().kmeans_update(b["x"], b["labels"], b["cen_old"], cen_new=o["cen_new"], counts=o["counts"])
        return o
    return S.Built(dict(x=x, cen_old=cen), {"labels": S._flip(labels)}, {"labels": labels},
                   lambda: {"cen_new": S._zeros(cen.shape), "counts": S._zeros((cen.shape[0],), torch.int32)}, call, "labels")


def _lloyd_case():
    x, cen = _fixture()
    other = x[[20, 21, 22, 23, 24, 25, 26]]
    for start in (cen, other):                                            # neither run stops within the iterations: all of them launch
        run = K.lloyd(x, start, LLOYD_ITERATIONS, 0.0)
        assert run.n_iter == LLOYD_ITERATIONS and not run.stopped
    R, d, k = x.shape[0], x.shape[1], cen.shape[0]

    def call(b, o):
        _ops().kmeans_lloyd(b["x"], b["cen"], max_iter=LLOYD_ITERATIONS, tol_abs=0.0, labels=o["labels"], dist=o["dist"], prev_labels=o["prev"],
                            counts=o["counts"], n_iter=o["n_iter"], shift=o["shift"], changed=o["changed"], work=o["work"])
        return {**{key: v for key, v in o.items() if key != "work"}, "cen": b["cen"]}
    return S.Built(dict(x=x), {"cen": other}, {"cen": cen},
                   lambda: {"labels": S._zeros((R,), torch.int32), "dist": S._zeros((R,)), "prev": S._zeros((R,), torch.int32),
                            "counts": S._zeros((k,), torch.int32), "n_iter": S._zeros((1,), torch.int32),
                            "shift": S._zeros((LLOYD_ITERATIONS,), torch.float64), "changed": S._zeros((LLOYD_ITERATIONS,), torch.int64),
                            "work": S._zeros((K.lloyd_work_bytes(R, d, k) // 8 + 1,), torch.int64)}, call, "cen")


def _seed_case():
    x, _ = _fixture()
    k, seed = 9, 5
    assert not np.array_equal(K.seed_rows(x, k, seed)[0], K.seed_rows(S._flip(x), k, seed)[0])

    def call(b, o):
        _ops().kmeans_seed(b["x"], k, seed, rows=o["rows"], cen=o["cen"], mind=o["mind"], work=o["work"])
        return {key: v for key, v in o.items() if key != "work"}
    return S.Built({}, {"x": S._flip(x)}, {"x": x},
                   lambda: {"rows": S._zeros((k,), torch.int32), "cen": S._zeros((k, x.shape[1])), "mind": S._zeros((x.shape[0],)),
                            "work": S._zeros((K.seed_work_bytes(x.shape[0]) // 8 + 1,), torch.int64)}, call, "x")


ENTRY_CASES = [S.EntryCase("vf_kmeans_assign", _assign_case), S.EntryCase("vf_kmeans_update", _update_case),
               S.EntryCase("vf_kmeans_lloyd", _lloyd_case), S.EntryCase("vf_kmeans_seed", _seed_case)]


def test_the_stream_cases_name_every_entry_of_the_header():
    import os
    from tests.conftest import REPO
    with open(os.path.join(REPO, "include", "vf_hip_kmeans.h")) as f:
        assert sorted(W.stream_entries(f.read())) == sorted(c.entry for c in ENTRY_CASES)
    assert LLOYD_ITERATIONS >= 2


@pytest.mark.parametrize("case", ENTRY_CASES, ids=lambda c: c.entry)
def test_entry_launches_on_the_current_stream(case, delay, side):  # noqa: F811
    S.test_entry_launches_on_the_current_stream(case, delay, side)


def _run_pipeline(inputs):
    from variantformer_amd import kmeans
    x = inputs["x"]
    model = kmeans.kmeans(x, 5, metric="correlation", init="k-means++", seed=3)
    out = _model_arrays("pp", model)
    out["predict"] = _np(model.predict(x, chunk_rows=100))
    return out


PIPELINE = A.PipelineCase("kmeans-blobs", lambda: {"x": K.blobs(300, 12, 5, 0.6, 8)}, _run_pipeline,
                          ("kmeans.kmeans", "kmeans.seed_rows", "kmeans._lloyd", "kmeans._assign"), ("pp.centers",), "x")


def test_pipeline_behind_a_late_input_on_a_side_stream(delay, side):  # noqa: F811
    S.test_pipeline_behind_a_late_input_on_a_side_stream(PIPELINE, delay, side)

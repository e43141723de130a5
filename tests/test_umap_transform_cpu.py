"""The UMAP transform without a GPU: the boundary of include/vf_hip_umap_transform.h (it parses, its three names are exported and
bound through _lib.ENTRIES), every refusal of every entry with
its argument named, the argument checks of manifold.fit / UMAPModel / transform and VCFProcessor.expression_umap_transform, and
the numpy restatements of tests/umap_transform_cases.py on their own: the due rule's count, a chunked run against a whole run,
and the blob case's condition."""
import inspect
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests import umap_cases as U
from tests import umap_transform_cases as T
from tests import write_set_cases as W
from tests.conftest import REPO

NAMES = ["vf_umap_init_transform", "vf_umap_layout_transform", "vf_umap_smooth_knn_query"]
ARGS = {"vf_umap_smooth_knn_query": 11, "vf_umap_init_transform": 13, "vf_umap_layout_transform": 23}


def _header(name="vf_hip_umap_transform.h") -> str:
    with open(os.path.join(REPO, "include", name)) as f:
        return f.read()


# ---- 1. header and binding ---------------------------------------------------------------------------------------------------------
def test_header_parses_and_its_names_are_exported_and_bound():
    from variantformer_amd import _lib
    from variantformer_amd.csrc import build as B
    text = _header()
    assert W.stream_entries(text) == NAMES
    assert sorted(_lib.ENTRIES["vf_hip_umap_transform.h"]) == NAMES, "ctypes binding and vf_hip_umap_transform.h disagree"
    assert "vf_umap_transform.hip" in B.SOURCES and any(h.endswith("vf_hip_umap_transform.h") for h in B.HEADERS)
    assert "vf_umap_transform.hip" not in B.EXTRA_FLAGS              # absent entries are recognised by NaN / Inf: no -fno-honor-nans
    with open(os.path.join(REPO, "variantformer_amd", "csrc", "vf_umap_transform.hip")) as f:
        assert "#pragma clang fp contract(off)" in f.read(), "the start equals its fp32 restatement only without an fma"
    bound = _lib.load()
    assert {name: len(_lib.SIGNATURES[name]) for name in NAMES} == ARGS
    assert _lib.ABI_VERSION == 13 and bound.vf_version() == 13
    assert "eleventh header" in text
    for word in ("Arguments", "Write set", "Arithmetic", "Non-finite operands", "Refused before anything is launched", "Not checked"):
        assert text.count(word) >= 3, f"an entry's comment contract has no `{word}` part"
    for macro, value in (("VF_UMAP_TRANSFORM_MAX_M", "64"), ("VF_UMAP_TRANSFORM_EPOCHS_PER_LAUNCH", str(T.EPOCHS_PER_LAUNCH))):
        assert re.search(rf"#define\s+{macro}\s+{re.escape(value)}\s", text), macro
    assert T.MAX_M == 64 and 1 <= T.EPOCHS_PER_LAUNCH < 10, "the table's N = 10 and 33 take more than one launch"
    assert "ANY SPLIT" in text and "IN PLACE" in text, "the header says that a split run is the same run and where the result is"
    assert "0x7FEB352D" in text and "0x846CA68B" in text and "0x9E3779B9" in text and "first_row + i" in text, "the header states the hash"


def _err(lib):
    return lib.vf_last_error().decode()


P = 4096                                                 # a non-null, aligned address; never dereferenced
INVALID = 1


def test_smooth_knn_query_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(idx=P, ld_idx=64, dist=P, ld_dist=64, Rq=0, m=30, mean_dist=0.5, sigma=P, strength=P, ld_strength=64):
        return lib.vf_umap_smooth_knn_query(idx, ld_idx, dist, ld_dist, Rq, m, mean_dist, sigma, strength, ld_strength, 0)
    assert call() == 0 and call(m=1) == 0 and call(m=64) == 0         # Rq = 0: nothing launched
    for name in ("idx", "dist", "sigma", "strength"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        assert call(**{name: P + 2}) == INVALID and re.search(rf"\b{name} must be 4-byte aligned", _err(lib)), _err(lib)
    for m in (0, -1, 65):
        assert call(m=m, ld_idx=99, ld_dist=99, ld_strength=99) == INVALID and _err(lib).split(": ")[1].startswith("m="), _err(lib)
    assert call(Rq=-1) == INVALID and "Rq=" in _err(lib)
    assert call(Rq=2 ** 24 + 1) == INVALID and "Rq=" in _err(lib) and "2^24" in _err(lib)
    for name in ("ld_idx", "ld_dist", "ld_strength"):
        assert call(**{name: 29}) == INVALID and _err(lib).split(": ")[1].startswith(f"{name}="), _err(lib)


def test_init_transform_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(idx=P, ld_idx=64, strength=P, ld_strength=64, Rq=0, m=30, Y=P, ldy=2, R=100, dim=2, Yq=2 * P, ldq=2):
        return lib.vf_umap_init_transform(idx, ld_idx, strength, ld_strength, Rq, m, Y, ldy, R, dim, Yq, ldq, 0)
    assert call() == 0 and call(R=0) == 0 and call(m=64, dim=8, ldy=8, ldq=8) == 0       # Rq = 0: nothing launched
    for name in ("idx", "strength", "Y", "Yq"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        assert call(**{name: P + 2}) == INVALID and re.search(rf"\b{name} must be 4-byte aligned", _err(lib)), _err(lib)
    assert call(Yq=P) == INVALID and "Y and Yq" in _err(lib)
    for m in (0, 65):
        assert call(m=m, ld_idx=99, ld_strength=99) == INVALID and _err(lib).split(": ")[1].startswith("m="), _err(lib)
    assert call(Rq=-1) == INVALID and "Rq=" in _err(lib)
    assert call(Rq=2 ** 24 + 1) == INVALID and "Rq=" in _err(lib) and "2^24" in _err(lib)
    assert call(R=-1) == INVALID and _err(lib).split(": ")[1].startswith("R=")
    assert call(R=2 ** 24 + 1) == INVALID and _err(lib).split(": ")[1].startswith("R=") and "2^24" in _err(lib)
    for dim in (0, 9):
        assert call(dim=dim, ldy=16, ldq=16) == INVALID and _err(lib).split(": ")[1].startswith("dim="), _err(lib)
    for name in ("ld_idx", "ld_strength"):
        assert call(**{name: 29}) == INVALID and _err(lib).split(": ")[1].startswith(f"{name}="), _err(lib)
    for name in ("ldy", "ldq"):
        assert call(**{name: 1}) == INVALID and _err(lib).split(": ")[1].startswith(f"{name}="), _err(lib)


def test_layout_transform_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(idx=P, ld_idx=64, samples=P, ld_samples=64, Rq=0, m=30, first_row=0, Y=P, ldy=2, R=100, dim=2, Yq=2 * P, ldq=2,
             epoch_begin=0, epoch_end=10, N=10, rate=5):
        return lib.vf_umap_layout_transform(idx, ld_idx, samples, ld_samples, Rq, m, first_row, Y, ldy, R, dim, Yq, ldq, epoch_begin, epoch_end,
                                            N, 1.5, 0.9, 1.0, 1.0, rate, 42, 0)
    # nothing launched: no queries, or no epochs (then R = 0 is no objection either)
    assert call() == 0 and call(Rq=9, epoch_begin=4, epoch_end=4) == 0 and call(Rq=9, R=0, epoch_begin=4, epoch_end=4) == 0 and call(R=0) == 0
    assert call(first_row=2 ** 32) == 0 and call(rate=0) == 0 and call(rate=2 ** 20) == 0
    for name in ("idx", "samples", "Y", "Yq"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        assert call(**{name: P + 2}) == INVALID and re.search(rf"\b{name} must be 4-byte aligned", _err(lib)), _err(lib)
    assert call(Yq=P) == INVALID and "Y and Yq" in _err(lib)
    for m in (0, 65):
        assert call(m=m, ld_idx=99, ld_samples=99) == INVALID and _err(lib).split(": ")[1].startswith("m="), _err(lib)
    assert call(Rq=-1) == INVALID and "Rq=" in _err(lib)
    assert call(Rq=2 ** 24 + 1) == INVALID and "Rq=" in _err(lib) and "2^24" in _err(lib)
    assert call(first_row=-1) == INVALID and _err(lib).split(": ")[1].startswith("first_row=")
    assert call(first_row=2 ** 32 + 1) == INVALID and "first_row=" in _err(lib) and "2^32" in _err(lib)
    assert call(Rq=7, first_row=2 ** 32 - 6) == INVALID and "first_row=" in _err(lib) and "2^32" in _err(lib)
    assert call(R=-1) == INVALID and _err(lib).split(": ")[1].startswith("R=")
    assert call(R=2 ** 24 + 1) == INVALID and _err(lib).split(": ")[1].startswith("R=") and "2^24" in _err(lib)
    assert call(Rq=7, R=0) == INVALID and _err(lib).split(": ")[1].startswith("R=0"), "queries and an epoch, but no training row"
    for dim in (0, 9):
        assert call(dim=dim, ldy=16, ldq=16) == INVALID and _err(lib).split(": ")[1].startswith("dim="), _err(lib)
    for name in ("ld_idx", "ld_samples"):
        assert call(**{name: 29}) == INVALID and _err(lib).split(": ")[1].startswith(f"{name}="), _err(lib)
    for name in ("ldy", "ldq"):
        assert call(**{name: 1}) == INVALID and _err(lib).split(": ")[1].startswith(f"{name}="), _err(lib)
    assert call(N=0, epoch_end=0) == INVALID and "N=" in _err(lib)
    assert call(epoch_begin=-1) == INVALID and "epoch_begin=" in _err(lib)
    assert call(epoch_begin=6, epoch_end=5) == INVALID and _err(lib).split(": ")[1].startswith("epoch_begin=")
    assert call(epoch_end=11) == INVALID and _err(lib).split(": ")[1].startswith("epoch_end=")
    assert call(rate=-1) == INVALID and "negative_sample_rate=" in _err(lib)
    assert call(rate=2 ** 20 + 1) == INVALID and "negative_sample_rate=" in _err(lib)


def test_the_wrappers_allocate_nothing_and_refuse_cpu_tensors():
    from variantformer_amd import manifold, ops
    for fn, outs in ((ops.umap_smooth_knn_query, ("sigma", "strength")), (ops.umap_init_transform, ("out",)), (ops.umap_layout_transform, ())):
        src = inspect.getsource(fn)
        assert not re.search(r"\b(empty|empty_like|zeros|zeros_like|ones|full|new_empty|new_zeros|new_full|tensor|arange|clone|contiguous)\s*\(", src)
        assert 'family="umap_transform"' not in src and "family or _SCOPE" in src
        prm = inspect.signature(fn).parameters
        for o in outs:
            assert prm[o].kind is inspect.Parameter.KEYWORD_ONLY and prm[o].default is inspect.Parameter.empty
        assert fn.__name__ not in W.allocating_wrappers()
    assert W.uncovered_wrappers() == []
    i, f, y = torch.zeros((4, 3), dtype=torch.int32), torch.zeros((4, 3)), torch.zeros((9, 2))
    with pytest.raises(Exception, match="GPU"):
        ops.umap_smooth_knn_query(i, f, 0.5, sigma=torch.zeros(4), strength=f.clone())
    with pytest.raises(Exception, match="GPU"):
        ops.umap_init_transform(i, f, y, out=torch.zeros(4, 2))
    with pytest.raises(Exception, match="GPU"):
        ops.umap_layout_transform(i, i.clone(), y, torch.zeros(4, 2), epoch_begin=0, epoch_end=1, n_epochs=1, a=1.5, b=0.9)
    assert inspect.getsource(manifold).count('family="umap_transform"') == 4, "the search and the three entries are recorded under the family"
    assert inspect.getsource(manifold).count('family="umap"') == 3, "the fit's launches are as they were"


# ---- 2. the restatements on their own -----------------------------------------------------------------------------------------------
def test_the_due_rule_draws_entry_s_exactly_samples_times():
    """The layout's restatement, asked through its trace: entry s of a row is attracted exactly samples[row, s] times in N epochs,
    never for an index outside [0, R) or a count outside 1 .. N."""
    for N in (1, 2, 10, 33):
        idx, cnt, Y, Yq = T.layout_case(65, 100, 2, 30, N)
        trace = []
        T.layout_transform(idx, cnt, Y, Yq, 0, N, N, *T.AB, rate=1, trace=trace)
        drawn = np.zeros_like(cnt)
        for n, s, rows, ks in trace:
            drawn[rows, s] += 1
            assert ks.shape == (rows.size, 1) and (ks >= 0).all() and (ks < 100).all()
        legal = (idx >= 0) & (idx < 100) & (cnt >= 1) & (cnt <= N)
        assert np.array_equal(drawn, np.where(legal, cnt, 0)), N
        assert (~legal).any() and (cnt == N + 1).any() and (cnt == -1).any() and (idx == 100).any() and (idx == -1).any()
    n, s, rows, ks = trace[0]
    want = U.negative_vertex(42, n, rows, s, 0, 100)
    assert np.array_equal(ks[:, 0], want), "the negative vertex is the header's hash of (seed, epoch, row number, entry, draw)"


def test_a_chunked_run_with_first_row_equals_the_whole_run():
    idx, cnt, Y, Yq = T.layout_case(65, 100, 3, 15, 10, special=False)
    whole = T.layout_transform(idx, cnt, Y, Yq, 0, 10, 10, *T.AB, first_row=5)
    for size in (1, 7, 64):
        parts = [T.layout_transform(idx[at:at + size], cnt[at:at + size], Y, Yq[at:at + size], 0, 10, 10, *T.AB, first_row=5 + at)
                 for at in range(0, 65, size)]
        assert np.array_equal(np.concatenate(parts), whole), size
    assert not np.array_equal(T.layout_transform(idx, cnt, Y, Yq, 0, 10, 10, *T.AB, first_row=6), whole), "the row number is in the hash"
    split = T.layout_transform(idx, cnt, Y, T.layout_transform(idx, cnt, Y, Yq, 0, 4, 10, *T.AB, first_row=5), 4, 10, 10, *T.AB, first_row=5)
    assert np.array_equal(split, whole), "and a run split at an epoch"
    big = T.layout_transform(idx[:3], cnt[:3], Y, Yq[:3], 0, 10, 10, *T.AB, first_row=2 ** 32 - 3)
    assert np.isfinite(big).all() and not np.array_equal(big, whole[:3]), "row numbers up to 2^32 - 1"


def test_the_restated_start_and_strengths_are_what_the_header_says():
    idx, dist = T.smooth_case("own-row", 65, 15)
    sigma, strength, converged, floored, open_ended = T.smooth_knn_query(idx, dist, 0.7)
    assert converged.all() and not floored.any() and not open_ended.any() and (strength[:, 0] > 0).all(), "an index equal to the row's number is not zeroed"
    resid = np.abs(np.exp(-dist.astype(np.float64) / sigma[:, None]).sum(1) - np.log2(15.0))
    assert (resid < 2e-5).all(), "sigma solves sum_t exp(-d_t / sigma) = log2(m): rho is 0"
    idx, dist = T.smooth_case("negatives", 65, 15)
    strength = T.smooth_knn_query(idx, dist, 0.7)[1]
    assert (dist[:, :5] <= 0).all() and (strength[:, :5] == 1).all() and dist[0, 0] == 0 and np.signbit(dist[0, 0])
    idx, dist = T.smooth_case("absent-row", 65, 15)
    sigma, strength = T.smooth_knn_query(idx, dist, 0.7)[:2]
    assert (sigma[::3] == 0).all() and (strength[::3] == 0).all() and (sigma[1::3] > 0).all()
    for mean_dist, want in ((np.nan, None), (np.inf, np.inf)):
        sigma, strength = T.smooth_knn_query(*T.smooth_case("random", 5, 15), mean_dist)[:2]
        assert np.isfinite(sigma).all() if want is None else ((sigma == np.inf).all() and (strength == 1).all())
    # the start: a weighted mean, NaN without a usable neighbour, indices -1 and R skipped
    g = np.random.default_rng(1)
    idx = g.integers(0, 50, (9, 6)).astype(np.int32)
    w = g.uniform(0.1, 1.0, (9, 6)).astype(np.float32)
    Y = g.uniform(0, 10, (50, 3)).astype(np.float32)
    idx[2], idx[3, 1], idx[3, 4] = -1, 50, -1
    w[4] = 0
    y0 = T.init_transform(idx, w, Y)
    assert y0.dtype == np.float32 and np.isnan(y0[2]).all() and np.isnan(y0[4]).all() and np.isfinite(np.delete(y0, (2, 4), 0)).all()
    ok = (idx[3] >= 0) & (idx[3] < 50)
    plain = (w[3, ok].astype(np.float64)[:, None] * Y[idx[3, ok]]).sum(0) / w[3, ok].astype(np.float64).sum()
    assert np.abs(y0[3] - plain).max() < 1e-5
    one = T.init_transform(np.array([[7]], dtype=np.int32), np.array([[0.3]], dtype=np.float32), Y)
    assert np.array_equal(one[0], Y[7]), "one neighbour: its weight is 0.3 / 0.3 = 1"
    s = T.samples(np.array([[1.0, 0.5, 0.004, 0.0], [0.0, 0.0, 0.0, 0.0], [0.2, 0.1, 0.2, 0.05]], dtype=np.float32), 100)
    assert s.dtype == np.int32 and s.tolist() == [[100, 50, 0, 0], [0, 0, 0, 0], [100, 50, 100, 25]], "normalised per row"


def test_the_restatement_places_every_blob_query_in_its_blob():
    x, lx, Y, q, lq = T.blobs()
    assert x.shape == (300, 16) and q.shape == (60, 16) and Y.shape == (300, 2) and T.BLOBS["n_neighbors"] == 15 and T.BLOBS["n_epochs"] == 100
    y, y0, mean_dist = T.blobs_reference()
    assert y is T.blobs_reference()[0], "a reference is computed once"
    found = T.nearest_training_label(Y, lx, y)
    print(f"[umap transform blobs] the restatement: {(found == lq).sum()} of 60 queries nearest to a training point of their own blob; "
          f"mean_dist {mean_dist:.4f}; moved from the start by up to {np.abs(y - y0).max():.3f}")
    assert np.isfinite(y).all() and (found == lq).all(), "every query ends nearest to a training point of its own blob"
    idx, dist = T.knn_queries(x, q, 15)
    strength = T.smooth_knn_query(idx, dist, mean_dist)[1]
    cnt = T.samples(strength.astype(np.float32), 100)
    assert cnt[0].max() == 100 and 0 < cnt[0].min() < 100, "row 0's draw counts run down from N"
    assert np.abs(y - y0).max() > 0.05, "the layout moves the queries from their start"


# ---- 3. argument checks --------------------------------------------------------------------------------------------------------------
def _model(**over):
    from variantformer_amd import manifold
    x, _, Y, _, _ = T.blobs()
    state = T.blobs_state(x, Y, 0.5)
    state.update(over)
    return manifold.UMAPModel.from_state(state)


def test_fit_and_transform_check_their_arguments_before_the_device():
    from variantformer_amd import manifold
    assert [(n, p.default) for n, p in inspect.signature(manifold.fit).parameters.items()] == \
        [(n, p.default) for n, p in inspect.signature(manifold.umap).parameters.items()], "fit takes the arguments of umap"
    assert [(n, p.default) for n, p in inspect.signature(manifold.UMAPModel.transform).parameters.items()][1:] == \
        [("queries", inspect.Parameter.empty), ("n_epochs", None), ("first_row", 0)]
    assert list(inspect.signature(manifold.transform).parameters) == ["model", "queries", "n_epochs", "first_row"]
    doc = manifold.umap.__doc__ + manifold.__doc__
    assert "out of scope" not in manifold.umap.__doc__ and "transform() of new points is out of scope" not in doc and "fit(x, ...)" in doc
    x, _, Y, q, _ = T.blobs()
    with pytest.raises(ValueError, match="n_neighbors"):
        manifold.fit(x, n_neighbors=1)
    with pytest.raises(ValueError, match="init"):
        manifold.fit(x, init="spectral")
    model = _model()
    assert (model.rows, model.columns, model.n_components, model.n_neighbors, model.metric, model.mean_dist) == (300, 16, 2, 15, "correlation", 0.5)
    assert (model.a, model.b) == T.AB and (model.seed, model.negative_sample_rate, model.repulsion_strength, model.learning_rate, model.n_epochs) == (42, 5, 1.0, 1.0, 500)
    assert model.embedding.dtype == np.float32 and np.array_equal(model.embedding, Y)
    with pytest.raises(TypeError, match="queries"):
        model.transform(q.tolist())
    with pytest.raises(ValueError, match="queries"):
        model.transform(q[0])
    with pytest.raises(ValueError, match=r"queries have 15 columns.*16"):
        model.transform(q[:, :15])
    for bad in (0, -3, 2 ** 31, 2.5, True):
        with pytest.raises(ValueError, match="n_epochs"):
            model.transform(q, n_epochs=bad)
    for bad in (-1, 2 ** 32 - 59, 1.0):
        with pytest.raises(ValueError, match="first_row"):
            model.transform(q, first_row=bad)
    with pytest.raises(ValueError, match=r"queries.*2\^24"):
        model.transform(np.broadcast_to(np.zeros((1, 16), dtype=np.float32), (2 ** 24 + 1, 16)))
    with pytest.raises(TypeError, match="model"):
        manifold.transform(Y, q)
    for queries in (q[:0], torch.from_numpy(q[:0])):                   # no queries: no device
        out = model.transform(queries)
        assert type(out) is type(queries) and tuple(out.shape) == (0, 2) and str(out.dtype).endswith("float32")
    with pytest.raises(ValueError, match="n_epochs"):
        model.transform(q[:0], n_epochs=0)
    # from_state: any embedding [rows, 1 .. 8] of the given training rows; n_neighbors above the training rows is allowed
    assert _model(embedding=np.zeros((300, 8), dtype=np.float32)).n_components == 8 and _model(n_neighbors=64).n_neighbors == 64
    assert manifold.UMAPModel.from_state(T.blobs_state(x[:5], Y[:5], 0.5)).rows == 5, "fewer training rows than n_neighbors"
    for over, name in ((dict(embedding=np.zeros((300, 9), dtype=np.float32)), "embedding"), (dict(embedding=np.zeros((299, 2), dtype=np.float32)), "rows"),
                       (dict(n_neighbors=0), "n_neighbors"), (dict(n_neighbors=65), "n_neighbors"), (dict(metric="euclidean"), "metric"),
                       (dict(a=0.0), "a must"), (dict(seed=-1), "seed"), (dict(negative_sample_rate=-1), "negative_sample_rate"),
                       (dict(learning_rate=0.0), "learning_rate"), (dict(mean_dist="x"), "mean_dist")):
        with pytest.raises(ValueError, match=name):
            _model(**over)
    state = T.blobs_state(x, Y, 0.5)
    del state["mean_dist"]
    with pytest.raises(ValueError, match="mean_dist"):
        manifold.UMAPModel.from_state(state)
    if not torch.cuda.is_available():
        for call in (lambda: model.transform(q), lambda: manifold.transform(model, q, n_epochs=10), lambda: manifold.fit(x, n_neighbors=5)):
            with pytest.raises(Exception, match="GPU"):
                call()


def test_expression_umap_transform_checks_the_model_and_the_frame():
    from variantformer_amd import manifold
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    prm = inspect.signature(VCFProcessor.expression_umap).parameters
    assert prm["return_model"].default is False and prm["umap_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert [(n, p.default) for n, p in inspect.signature(VCFProcessor.expression_umap_transform).parameters.items()][1:] == [
        ("model", inspect.Parameter.empty), ("df", inspect.Parameter.empty), ("on", "predicted_expression"), ("axis", "genes"),
        ("tissue", None), ("n_epochs", None)]
    vp = VCFProcessor(require_gpu=False)
    names = [f"tissue{t}" for t in range(4)]
    df = pd.DataFrame({"gene_id": [f"ENSG{i:03d}" for i in range(6)], "tissues": [list(range(4))] * 6, "tissue_names": [names] * 6,
                       "predicted_expression": [np.arange(4, dtype=np.float32).reshape(4, 1) * (i + 1) for i in range(6)]})
    g = np.random.default_rng(0)
    model = manifold.UMAPModel.from_state(T.blobs_state(g.standard_normal((9, 5)).astype(np.float32), g.standard_normal((9, 2)).astype(np.float32), 0.5))
    with pytest.raises(TypeError, match="model"):
        vp.expression_umap_transform({"coords": None}, df)
    with pytest.raises(ValueError, match=r"4 columns.*fitted on 5"):
        vp.expression_umap_transform(model, df)
    with pytest.raises(ValueError, match="format_output"):
        vp.expression_umap_transform(model, df.drop(columns=["predicted_expression"]))
    with pytest.raises(ValueError, match="axis"):
        vp.expression_umap_transform(model, df, axis="rows")
    assert "umap_1" not in df.columns, "a refused call leaves the frame as it was"
    four = manifold.UMAPModel.from_state(T.blobs_state(g.standard_normal((9, 4)).astype(np.float32), g.standard_normal((9, 2)).astype(np.float32), 0.5))
    with pytest.raises(ValueError, match="n_epochs"):
        vp.expression_umap_transform(four, df, n_epochs=0)
    if not torch.cuda.is_available():
        with pytest.raises(Exception, match="GPU"):
            vp.expression_umap_transform(four, df)
        with pytest.raises(Exception, match="GPU"):
            vp.expression_umap(df, n_neighbors=3, return_model=True)

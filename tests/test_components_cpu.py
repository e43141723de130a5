"""The component entries without a GPU: the boundary of include/vf_hip_components.h (it parses, its three names are exported and
bound through _lib.ENTRIES), every refusal of every entry with
its argument named, the argument checks of manifold.spectral_init_components, and the numpy restatements of
tests/components_cases.py on their own: the search against scipy, the renumbered graph against sub-graphs extracted on their
own, the centroids against a plain mean, the meta positions against scikit-learn, and the whole layout on the composite graph."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

from tests import components_cases as C
from tests import spectral_cases as S
from tests import umap_cases as U
from tests.conftest import REPO

NAMES = ["vf_csr_components", "vf_graph_components_rounds", "vf_segment_mean_gather"]
ARGS = {"vf_graph_components_rounds": 11, "vf_csr_components": 14, "vf_segment_mean_gather": 10}


def _header(name="vf_hip_components.h") -> str:
    with open(os.path.join(REPO, "include", name)) as f:
        return f.read()


# ---- 1. header and binding ---------------------------------------------------------------------------------------------------------
def test_header_parses_and_its_names_are_exported_and_bound():
    from variantformer_amd import _lib
    from variantformer_amd.csrc import build as B
    text = _header()
    assert sorted(_lib.ENTRIES["vf_hip_components.h"]) == NAMES, "ctypes binding and vf_hip_components.h disagree"
    assert "vf_components.hip" in B.SOURCES and any(h.endswith("vf_hip_components.h") for h in B.HEADERS)
    with open(os.path.join(REPO, "variantformer_amd", "csrc", "vf_components.hip")) as f:
        source = f.read()
    assert "#pragma clang fp contract(off)" in source, "the centroids equal their fp64 restatement only without an fma"
    assert "hipDeviceSynchronize" not in source and "hipStreamSynchronize" not in source, "no entry synchronises the stream"
    bound = _lib.load()
    assert {name: len(_lib.SIGNATURES[name]) for name in NAMES} == ARGS
    assert _lib.ABI_VERSION == 13 and bound.vf_version() == 13
    assert "twelfth header" in text
    for word in ("Arguments", "Write set", "Refused before anything is launched", "Not checked"):
        assert text.count(word) >= 3, f"an entry's comment contract has no `{word}` part"
    assert "THE ONE PLACE IN THESE HEADERS THAT USES AN ATOMIC" in text and "bit for bit" in text and "np.minimum.at(Pn, P, m)" in text
    assert re.search(r"#define\s+VF_COMPONENTS_MAX_R\s+\(1 << 24\)", text) and re.search(r"#define\s+VF_SEGMENT_MEAN_WAVES\s+4\s", text)


def _err(lib):
    return lib.vf_last_error().decode()


P = 4096                                                 # a non-null, aligned address; never dereferenced
INVALID = 1


def test_rounds_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(rowptr=P, col=P, w=P, nnz=10, R=0, parent=P, g=2 * P, m=3 * P, changed=4 * P, rounds=8):
        return lib.vf_graph_components_rounds(rowptr, col, w, nnz, R, parent, g, m, changed, rounds, 0)
    assert call() == 0 and call(R=5, rounds=0) == 0 and call(col=0, w=0, nnz=0) == 0          # nothing launched
    for name, word in (("rowptr", "rowptr"), ("col", "col"), ("w", "w"), ("parent", "P"), ("g", "g"), ("m", "m"), ("changed", "changed")):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {word}"), _err(lib)
        assert call(**{name: P + 2}) == INVALID and re.search(rf"\b{word} must be [48]-byte aligned", _err(lib)), _err(lib)
    assert call(rowptr=P + 4) == INVALID and "rowptr must be 8-byte aligned" in _err(lib)
    for same in (dict(g=P), dict(m=P), dict(m=2 * P)):
        assert call(**same) == INVALID and "three buffers" in _err(lib)
    assert call(R=-1) == INVALID and "R=" in _err(lib)
    assert call(R=2 ** 24 + 1) == INVALID and "2^24" in _err(lib)
    assert call(nnz=-1) == INVALID and "nnz=" in _err(lib)
    assert call(rounds=-1) == INVALID and "rounds=" in _err(lib)


def test_csr_components_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()
    names = ("rowptr", "col", "w", "order", "rank", "comp", "starts", "rowptr_new", "col_new", "w_new")

    def call(nnz=10, R=0, C=1, **kw):
        a = {n: (i + 1) * P for i, n in enumerate(names)}
        a.update(kw)
        return lib.vf_csr_components(a["rowptr"], a["col"], a["w"], nnz, R, a["order"], a["rank"], a["comp"], a["starts"], C, a["rowptr_new"],
                                     a["col_new"], a["w_new"], 0)
    assert call() == 0 and call(C=0) == 0 and call(nnz=0, col=0, w=0, col_new=0, w_new=0) == 0         # R = 0: nothing launched
    for name in names:
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        assert call(**{name: P + 2}) == INVALID and re.search(rf"\b{name} must be [48]-byte aligned", _err(lib)), _err(lib)
    assert call(rowptr_new=P + 4) == INVALID and "rowptr_new must be 8-byte aligned" in _err(lib)
    assert call(col_new=2 * P) == INVALID and "must not be col and w" in _err(lib)
    assert call(w_new=3 * P) == INVALID and "must not be col and w" in _err(lib)
    assert call(R=-1) == INVALID and "R=" in _err(lib)
    assert call(R=2 ** 24 + 1) == INVALID and "2^24" in _err(lib)
    assert call(nnz=-1) == INVALID and "nnz=" in _err(lib)
    for count in (0, 6):
        assert call(R=5, C=count) == INVALID and "C=" in _err(lib)


def test_segment_mean_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(x=P, ldx=64, R=100, d=49, order=2 * P, starts=3 * P, C=0, out=4 * P, ldo=64):
        return lib.vf_segment_mean_gather(x, ldx, R, d, order, starts, C, out, ldo, 0)
    assert call() == 0 and call(R=0) == 0 and call(d=1, ldx=1, ldo=1) == 0                    # C = 0: nothing launched
    for name in ("x", "order", "starts", "out"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        assert call(**{name: P + 2}) == INVALID and re.search(rf"\b{name} must be 4-byte aligned", _err(lib)), _err(lib)
    assert call(R=-1) == INVALID and "R=" in _err(lib)
    assert call(R=2 ** 24 + 1) == INVALID and "2^24" in _err(lib)
    for d in (0, -3, 64 * 65535 + 1):
        assert call(d=d, ldx=2 ** 40, ldo=2 ** 40) == INVALID and _err(lib).split(": ")[1].startswith("d="), _err(lib)
    for name in ("ldx", "ldo"):
        assert call(**{name: 48}) == INVALID and _err(lib).split(": ")[1].startswith(f"{name}="), _err(lib)
    for count in (-1, 2 ** 24 + 1):
        assert call(C=count) == INVALID and "C=" in _err(lib)


# ---- 2. the Python boundary ----------------------------------------------------------------------------------------------------------
def test_spectral_init_components_checks_its_arguments_before_the_device():
    from variantformer_amd import _lib, manifold
    graph = S.blobs(False)
    assert manifold.spectral_init_components.wants_rows is True and not hasattr(manifold.spectral_init, "wants_rows")
    for bad in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="n_components"):
            manifold.spectral_init_components(graph, bad, 42)
    with pytest.raises(ValueError, match="seed"):
        manifold.spectral_init_components(graph, 2, -1)
    with pytest.raises(ValueError, match="metric"):
        manifold.spectral_init_components(graph, 2, 42, metric="euclidean")
    with pytest.raises(ValueError, match="rows has 79 rows"):
        manifold.spectral_init_components(graph, 2, 42, rows=np.zeros((79, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="graph"):
        manifold.spectral_init_components((graph[0],), 2, 42)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.VFError, match="needs a GPU"):
            manifold.spectral_init_components(graph, 2, 42)
    with pytest.raises(ValueError, match="rows"):
        manifold.meta_positions(5, 2)
    assert manifold.COMPONENTS_MAX == C.COMPONENTS_MAX and manifold.COMPONENT_ROUNDS == 8


def test_the_wrappers_refuse_host_tensors():
    from variantformer_amd import _lib, ops
    rowptr, col, w = (torch.from_numpy(a) for a in S.path(5))
    v = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(_lib.VFError, match="GPU"):
        ops.graph_components_rounds(rowptr, col, w, v, v.clone(), v.clone(), torch.zeros(1, dtype=torch.int32), rounds=1)
    with pytest.raises(_lib.VFError, match="GPU"):
        ops.csr_components(rowptr, col, w, v, v, v, torch.zeros(2, dtype=torch.int32), rowptr, col_new=col.clone(), w_new=w.clone())
    with pytest.raises(_lib.VFError, match="GPU"):
        ops.segment_mean_gather(torch.zeros(5, 3), v, torch.zeros(2, dtype=torch.int32), out=torch.zeros(1, 3))


# ---- 3. the restatements ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", C.RS)
def test_the_search_settles_on_scipys_components(R):
    for name, graph in C.search_graphs(R).items():
        n = graph[0].shape[0] - 1
        labels, settled_after = C.fixed_point(*graph)
        count, ref = S.components(*C.clean(*graph))
        assert np.array_equal(labels, ref) and len(np.unique(labels)) == count, name
        assert settled_after <= 2 * int(n).bit_length() + 2, f"{name}: {settled_after} rounds"
        state, changed = np.arange(n), None
        r, c = C.edges(*graph)
        for t in range(settled_after + 2):
            nxt, changed = C.one_round(state, r, c)
            assert (nxt <= state).all() and (nxt >= 0).all() and changed == int(t < settled_after), "labels never grow; changed until settled"
            state = nxt
        assert C.rounds(*graph, np.arange(n), 0)[1] is None


def test_the_renumbered_graph_holds_every_component_as_its_own_sub_graph():
    for graph in (C.composite(), C.composite(True), C.spoiled_kernel_graph()):
        labels, _ = C.fixed_point(*graph)
        order, rank, comp, starts, rowptr_new = C.permutation(labels, graph[0])
        assert np.array_equal(rank[order], np.arange(order.shape[0])) and (np.diff(labels[order]) >= 0).all() and starts[-1] == order.shape[0]
        col_new, w_new = C.csr_components(*graph, order, rank, comp, starts, rowptr_new)
        for k in range(starts.shape[0] - 1):
            members = order[starts[k]:starts[k + 1]].astype(np.int64)
            assert (np.diff(members) > 0).all(), "a stable sort keeps a component's vertices ascending"
            for a, b in zip(C.component_slice(rowptr_new, col_new, w_new, starts, k), C.extract(*graph, members)):
                assert a.dtype == b.dtype and np.array_equal(a, b)
    graph = C.composite()
    assert graph[0].shape[0] - 1 == 726 and len(np.unique(C.fixed_point(*graph)[0])) == 5
    rows = U.entry_rows(graph[0])
    assert all((np.diff(graph[1][graph[0][i]:graph[0][i + 1]]) > 0).all() for i in range(726)) and (graph[1] != rows).all()


@pytest.mark.parametrize("d", C.SEGMENT_DS)
def test_the_restated_centroids_are_means(d):
    order, starts = C.segments(C.SEGMENT_LENGTHS, seed=d)
    x = np.random.default_rng(d).standard_normal((order.shape[0], d)).astype(np.float32)
    got = C.segment_mean(x, order, starts)
    exact = np.stack([x[order[starts[k]:starts[k + 1]]].astype(np.float64).mean(0) for k in range(starts.shape[0] - 1)])
    assert got.dtype == np.float32 and np.abs(got - exact).max() <= 2.0 ** -23 * np.abs(exact).max() + 1e-12


@pytest.mark.parametrize("count,dim", ((5, 2), (7, 3), (9, 3), (40, 3), (17, 8), (40, 8)))          # C > 2 dim: the branch that is taken
@pytest.mark.parametrize("metric", ("correlation", "cosine"))
def test_meta_positions_against_scikit_learn(count, dim, metric):
    """SpectralEmbedding(affinity="precomputed") takes the same affinity; its columns are compared after both sides are scaled
    to unit norm and signed alike.  Bound: META_FACTOR C u / gap (tests/components_cases.py)."""
    from sklearn.manifold import SpectralEmbedding
    from variantformer_amd import manifold
    centroids = np.random.default_rng(100 * count + dim).standard_normal((count, 12)).astype(np.float32)
    got = manifold.meta_positions(count, dim, centroids, metric)
    assert got.dtype == np.float64 and got.shape == (count, dim) and np.array_equal(got, C.meta_positions(count, dim, centroids, metric))
    assert np.abs(got).max() == 1.0 and (got[np.abs(got).argmax(0), np.arange(dim)] > 0).all(), "the largest magnitude is 1; the solver's sign rule"
    L, _, A = C.meta_laplacian(centroids, metric)
    lam = np.linalg.eigvalsh(L)
    gap = min(np.diff(lam[:dim + 2]).min(), 1.0)
    ref = SpectralEmbedding(n_components=dim, affinity="precomputed").fit_transform(A)
    unit = lambda y: y / np.linalg.norm(y, axis=0, keepdims=True)          # noqa: E731
    a, b = unit(got), unit(ref)
    b = b * np.sign((a * b).sum(0))[None, :]
    worst, bound = float(np.abs(a - b).max()), C.META_FACTOR * count * 2.0 ** -53 / gap
    print(f"[meta positions] C={count} dim={dim} {metric}: gap {gap:.2e}, against scikit-learn {worst:.2e} (bound {bound:.2e})")
    assert worst <= bound


def test_the_small_meta_positions_and_the_data_range():
    from variantformer_amd import manifold
    assert np.array_equal(manifold.meta_positions(2, 2), [[1, 0], [-1, 0]])
    assert np.array_equal(manifold.meta_positions(4, 2), [[1, 0], [0, 1], [-1, 0], [0, -1]])
    assert np.array_equal(manifold.meta_positions(3, 2), [[1, 0], [0, 1], [-1, 0]])
    assert np.array_equal(manifold.meta_positions(5, 3), [[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0]])
    assert np.array_equal(manifold.meta_positions(2, 1), [[1], [-1]])
    for count, dim in ((2, 2), (4, 2), (5, 3)):
        assert np.array_equal(manifold.meta_positions(count, dim), C.meta_positions(count, dim))
    assert np.array_equal(manifold.data_ranges(manifold.meta_positions(2, 2)), [1, 1])
    assert np.allclose(manifold.data_ranges(manifold.meta_positions(4, 2)), np.sqrt(2) / 2)
    meta = np.array([[0.0, 0.0], [3.0, 4.0], [0.0, 0.0], [0.0, 1.0]])
    assert np.array_equal(manifold.data_ranges(meta), [0.5, np.sqrt(18) / 2, 0.5, 0.5]) and np.array_equal(manifold.data_ranges(meta), C.data_ranges(meta))
    assert np.isinf(manifold.data_ranges(np.zeros((3, 2)))).all(), "positions that coincide have no positive distance"


def test_the_restated_layout_of_the_composite_graph():
    graph, rows = C.composite(), C.composite_rows()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        y, parts = C.layout(*graph, 2, 42, rows=rows)
    assert y.dtype == np.float32 and y.shape == (726, 2) and np.isfinite(y).all()
    order, starts, meta, spread = parts["order"], parts["starts"], parts["meta"], parts["data_range"]
    assert sorted(np.diff(starts).tolist()) == [1, 3, 65, 257, 400] and parts["solved"].sum() == 3
    for k in range(5):
        members = order[starts[k]:starts[k + 1]]
        far = np.abs(y[members].astype(np.float64) - meta[k].astype(np.float32).astype(np.float64)).max()
        last = float(np.spacing(np.float32(np.abs(meta[k]).max() + spread[k]))) / 2
        if parts["solved"][k]:
            info = parts["infos"][k]
            assert info["converged"] and info["iterations"] <= 3
            assert abs(far - spread[k]) <= 2.0 ** -23 * spread[k] + last
        else:
            assert far <= spread[k] + last
    four, parts4 = C.layout(*C.composite(True), 2, 7)
    assert np.array_equal(parts4["meta"], [[1, 0], [0, 1], [-1, 0], [0, -1]]) and np.isfinite(four).all()

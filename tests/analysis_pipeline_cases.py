"""The analysis pipelines as whole calls, shared by tests/test_analysis_cases_cpu.py, tests/test_analysis_poison_gpu.py and
tests/test_analysis_streams_gpu.py.  Importing this module needs no GPU; a case touches the device only when its `run` is called.

The wrappers of variantformer_amd/ops.py behind neighbours, Ward linkage, UMAP fit and transform, the spectral starts, components,
t-SNE, enrichment and the forests allocate nothing: their out= buffers and workspaces are made by the PIPELINES, with torch.empty /
torch.empty_like in the modules of write_set_cases.ANALYSIS_MODULES.  The per-kernel suites poison the buffers of one call; what
a pipeline does with a buffer BETWEEN calls -- ping-pong matrices, slots that take what is dropped, work vectors reused by every
round -- only a whole run under the poisoning allocator can see.  A fresh process hands out zeros, a long-lived one the previous
call's bytes: an element read before it is written is right in the first and wrong in the second.

Every case is (name, build, run, covers, finite, late):
  build()          the inputs, a dict of numpy arrays and plain objects, made on the CPU from the builders the suite already has;
  run(inputs)      the pipeline, returning {name: numpy array}; an input named by `late` may also be a device tensor;
  covers           the allocating functions of the analysis modules the case reaches, as "module.function" / "module.Class.method";
  finite           the returned arrays the pipeline promises finite on these inputs;
  late             the input that tests/test_analysis_streams_gpu.py writes behind a delay on a side stream (None: the pipeline
                   takes that input on the host only).

The 56 allocations, read before any run on a device: who writes every element that is later read.  "header" = the write set the
entry's header states, held per call by the entry's own test_*_gpu.py under poison.

  neighbors.standardize        z [R, d], norm [R]            vf_rows_standardize: every z[r, c < d] and norm[r] (header)
  neighbors._knn               indices, distances [rows, k]  vf_knn_dot: columns k - found .. k - 1 of every row, -1 / +0 padding
                                                             included (header); column 0 under include_self by the two torch
                                                             assignments; with found == 0 (k = 1, include_self) only column 0 exists
  neighbors.correlation_distance  out [R, R]                 vf_pairwise_dot: every out[r, j < Ry] (header)
  linkage.ward                 work[0], work[1] [n * n]      only the views matrix(k, m) = work[k][:m * m] are read, each right after
                                                             vf_linkage_contract wrote all m x m of it (ld = m, diagonal included:
                                                             header); torch.aminmax reads matrix(cur, n) after round 0 wrote it
                               nn_val, nn_idx [n]            vf_linkage_nearest writes [:m] (header); only [:m] is read, in that round
                               sizes[0], sizes[1] [n]        size_out[:m_out] by vf_linkage_contract; read as size[:m] one round later
                               pair_dist [n]                 [:m_out] by vf_linkage_contract, +0 at slots that stand alone (header);
                                                             read [:m_out] in the same round
                               slots [2, n + 1]              the two scatter_ of a round write [:, :m_out] completely (pos is a
                                                             bijection of the kept slots onto 0 .. m_out - 1) and column m_out, which
                                                             takes the dropped upper slots and is never read
                               rec_left / right / height / size [n]   scatter_ at rows made .. made + merges - 1 and at row n - 1, which
                                                             takes the slots that did not merge; rows [:n - 1] are read after the
                                                             loop, when made == n - 1 (asserted); row n - 1 is never read
  manifold._fuzzy_graph        rho, sigma [R], strength [R, m]   vf_umap_smooth_knn: all of them, absent entries included (header)
                               w [nnz]                       vf_umap_union: every entry of every row (header)
  manifold._layout             y1 like y0                    vf_umap_layout: every epoch writes all [R, dim] of its output buffer, a
                                                             vertex with nothing due is copied (header); the returned buffer is the
                                                             last epoch's output, or y0 (a clone) without an epoch
  manifold._components         g, m [R], changed [1]         launch 1 of every round writes g, m and changed[0] = 0 before launch 2
                                                             reads them (header); R >= 1 and rounds = 8 here, so int(changed) reads a
                                                             written value
  manifold._spectral           bufs[0] [R, p]                x.copy_(random_init - 0.5) writes all of it
                               bufs[1], bufs[2]              outputs of vf_spmm_recur / vf_tall_mul, all [R, p] per step (header).  A
                                                             recurrence reads W = the block before the newest only where coef[t][2]
                                                             != 0: _ONE_STEP and step 0 of chebyshev_coefficients have exactly 0
                                                             there, and a zero coefficient's operand is skipped, not multiplied
                               work [1024 p p] fp64          vf_tall_gram writes the nb p q partials it then sums (header)
                               gram: out [p, q] fp64         vf_tall_gram: every G[a, b] (header)
  manifold._degrees            deg, dinv [R]                 vf_graph_degree: every element, +0 for a row without entries (header)
  manifold.spectral_init_components   rank [R]               rank[order64] = arange: order64 is a permutation
                               col_new, w_new [nnz]          vf_csr_components: every entry of every new row, -1 / +0 where the entry
                                                             is no edge of the component (header; rowptr_new is the permuted rowptr)
                               centroids [C, d]              vf_segment_mean_gather: every out[k, c < d] (header)
  manifold.UMAPModel.transform idx, dist [Rq, m]             vf_knn_dot, as neighbors._knn
                               sigma [Rq], strength [Rq, m]  vf_umap_smooth_knn_query (header)
                               yq [Rq, dim]                  vf_umap_init_transform writes it, vf_umap_layout_transform reads and
                                                             rewrites it (header)
  manifold._tsne_affinities    beta [R], p_cond [R, m]       vf_tsne_perplexity (header);  p [nnz]  vf_tsne_joint (header)
  manifold._tsne_run           work, zsum [iterations]       vf_tsne_descent: step 1 of every iteration writes `part` into work
                                                             before step 3 reads it; zsum[n - iter_begin] per iteration (header)
  manifold._tsne_kl            part [splits, R, dim + 1]     vf_tsne_repulsion: every element (header)
  manifold._knn_panels         idx, dist [R, m]              the panels r0 .. r0 + n cover every row; s [n, R] by vf_pairwise_dot
  enrichment._hypergeom        count [T, k], size [T]        vf_enrich_counts (header);  csize [1, k] and the throw-away size [1] by
                                                             the second vf_enrich_counts call;  log_p, tail, steps [T, k] by
                                                             vf_hypergeom_tail (header)
  enrichment._bh               q like ordered                q[order] = ordered: order is the permutation of a sort
  ad_risk.ADrisk.__call__      out [R, K]                    vf_forest_predict: out[r, 0 .. K - 1] of every row (header)
  ad_risk.ADriskFromVCF._predict_ad_risk   out [rows, K]     the same entry in its row form

No element was found read unwritten by this reading; the integer buffers among them (nn_idx, slots, g, m, rank, col_new, idx,
count, size, steps) are all written whole before anything indexes with them, so -1 or 0x3C3C3C3C poison cannot become an index.
tests/test_analysis_poison_gpu.py holds the reading to the device: bit-identical results under 0xFF and 0x3C poison.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import numpy as np


class PipelineCase(NamedTuple):
    name: str
    build: Callable
    run: Callable
    covers: tuple
    finite: tuple
    late: str | None = None


CASES: list = []


def _case(name, build, run, covers, finite, late=None):
    CASES.append(PipelineCase(name, build, run, tuple(covers), tuple(finite), late))


def case(name: str) -> PipelineCase:
    return [c for c in CASES if c.name == name][0]


def _np(v) -> np.ndarray:
    import torch
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _load():
    from variantformer_amd import _lib
    _lib.load()


# ---- neighbours ------------------------------------------------------------------------------------------------------------------
NEIGHBOR_ROWS, NEIGHBOR_D = 257, 33
NEIGHBOR_COVERS = ("neighbors.standardize", "neighbors._knn", "neighbors.correlation_distance")


def _neighbor_inputs():
    from tests import neighbors_cases as N
    x = np.ascontiguousarray(N.random_case(NEIGHBOR_ROWS, NEIGHBOR_D).z[:, :NEIGHBOR_D])
    return {"x": x, "queries": np.ascontiguousarray(x[::-1][:70] * np.float32(1.5) + np.float32(0.25))}


def _run_neighbors(inputs):
    from variantformer_amd import neighbors
    _load()
    x, out = inputs["x"], {}
    for k in (15, 63):
        for include_self in (False, True):
            idx, dist = neighbors.knn(x, k=k, include_self=include_self)
            out[f"knn{k}-self{int(include_self)}-idx"], out[f"knn{k}-self{int(include_self)}-dist"] = _np(idx), _np(dist)
        idx, dist = neighbors.knn(x, k=k, metric="cosine", queries=inputs["queries"])
        out[f"knn{k}-queries-idx"], out[f"knn{k}-queries-dist"] = _np(idx), _np(dist)
    out["correlation_distance"] = _np(neighbors.correlation_distance(x))
    for metric in ("correlation", "cosine"):
        z, norm = neighbors.standardize(x, metric)
        out[f"standardize-{metric}-z"], out[f"standardize-{metric}-norm"] = _np(z), _np(norm)
    return out


_case("neighbours-257x33", _neighbor_inputs, _run_neighbors, NEIGHBOR_COVERS,
      [f"knn{k}-{f}-dist" for k in (15, 63) for f in ("self0", "self1", "queries")] +
      ["correlation_distance", "standardize-correlation-z", "standardize-cosine-z", "standardize-correlation-norm", "standardize-cosine-norm"],
      late="x")


# ---- linkage ---------------------------------------------------------------------------------------------------------------------
LINKAGE_COVERS = ("linkage.ward",) + NEIGHBOR_COVERS[:1] + NEIGHBOR_COVERS[2:]


def _linkage_inputs(n):
    def build():
        from tests import linkage_cases as L
        return {"x": L.clustered_rows(n, 49, 2000 + n).astype(np.float32)}
    return build


def _run_ward_of_rows(inputs):
    from variantformer_amd import linkage
    _load()
    Z, info = linkage.ward_of_rows(inputs["x"], return_info=True)
    n = Z.shape[0] + 1
    return {"Z": Z, "rounds": np.array([info["rounds"]]), "leaves": linkage.leaves_list(Z),
            "cut": linkage.cut(Z, [2, 7, n // 2, n])}


for _n in (65, 257):
    _case(f"ward_of_rows-{_n}", _linkage_inputs(_n), _run_ward_of_rows, LINKAGE_COVERS, ["Z"], late="x")


def _strided_inputs():
    from tests import linkage_cases as L
    wide = [c for c in L.cases() if c.name == "ld-above-n-63"][0].D
    assert wide.shape[1] > wide.shape[0]
    return {"D": wide}


def _run_ward_strided(inputs):
    """linkage.ward on a device matrix whose rows are further apart than its side: D[:, :n] of the [n, ld] buffer."""
    import torch
    from variantformer_amd import linkage
    _load()
    wide = inputs["D"]
    wide = wide if isinstance(wide, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(wide)).cuda()
    n = wide.shape[0]
    D = wide[:, :n]
    assert D.stride(0) > n
    Z, info = linkage.ward(D, return_info=True)
    return {"Z": Z, "rounds": np.array([info["rounds"]])}


_case("ward-device-ld-above-n-63", _strided_inputs, _run_ward_strided, ("linkage.ward",), ["Z"], late="D")


# ---- UMAP ------------------------------------------------------------------------------------------------------------------------
UMAP_COVERS = ("manifold._fuzzy_graph", "manifold._layout", "neighbors.standardize", "neighbors._knn")
SPECTRAL_COVERS = ("manifold._components", "manifold._spectral", "manifold._degrees")
UMAP_EPOCHS = 30


def _umap_inputs():
    from tests import umap_cases as U
    return {"x": U.blobs()}


def _inits():
    from variantformer_amd import manifold
    return {"random": "random", "pca": "pca", "spectral": manifold.spectral_init}


def _run_umap(inputs):
    import warnings
    from variantformer_amd import manifold
    _load()
    out = {}
    for name, init in _inits().items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)                 # a k-NN graph of blobs may be disconnected: the fallback warns
            out[name] = _np(manifold.umap(inputs["x"], n_neighbors=15, n_epochs=UMAP_EPOCHS, init=init))
    return out


_case("umap-blobs", _umap_inputs, _run_umap, UMAP_COVERS + SPECTRAL_COVERS, ["random", "pca", "spectral"], late="x")


def _composite_rows_inputs():
    from tests import components_cases as C
    return {"x": C.composite_rows()}


def _run_umap_components(inputs):
    import warnings
    from variantformer_amd import manifold
    _load()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        y = manifold.umap(inputs["x"], n_neighbors=15, n_epochs=UMAP_EPOCHS, init=manifold.spectral_init_components)
    return {"embedding": _np(y)}


_case("umap-spectral_init_components-726x7", _composite_rows_inputs, _run_umap_components,
      UMAP_COVERS + SPECTRAL_COVERS + ("manifold.spectral_init_components",), ["embedding"], late="x")


def _composite_inputs():
    from tests import components_cases as C
    rowptr, col, w = C.composite()
    return {"rowptr": rowptr, "col": col, "w": w, "rows": C.composite_rows()}


def _run_composite(inputs):
    """The composite graph itself: its components, and the per-component spectral start from its 726 x 7 rows (5 components are
    more than 2 n_components = 4, so the centroids and the meta layout are reached whatever a k-NN graph would have given)."""
    import warnings
    from variantformer_amd import manifold
    _load()
    graph = (inputs["rowptr"], inputs["col"], inputs["w"])
    labels, count = manifold.graph_components(graph)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        y = manifold.spectral_init_components(graph, 2, 42, rows=inputs["rows"])
    return {"labels": _np(labels), "count": np.array([count]), "start": _np(y)}


_case("components-composite", _composite_inputs, _run_composite, SPECTRAL_COVERS + ("manifold.spectral_init_components",),
      ["start"], late="w")


# ---- fit and transform -----------------------------------------------------------------------------------------------------------
def _transform_inputs():
    from tests import umap_transform_cases as T
    x, _, _, q, _ = T.blobs()
    return {"x": x, "q": q}


def _run_fit_transform(inputs):
    from variantformer_amd import manifold
    _load()
    model = manifold.fit(inputs["x"], n_neighbors=15, n_epochs=UMAP_EPOCHS)
    first = model.transform(inputs["q"], n_epochs=UMAP_EPOCHS)
    again = manifold.UMAPModel.from_state(model.state()).transform(inputs["q"], n_epochs=UMAP_EPOCHS)
    return {"embedding": _np(model.embedding), "transform": _np(first), "transform-from_state": _np(again)}


_case("umap-fit-transform-blobs", _transform_inputs, _run_fit_transform, UMAP_COVERS + ("manifold.UMAPModel.transform",),
      ["embedding", "transform", "transform-from_state"], late="x")


# ---- t-SNE -----------------------------------------------------------------------------------------------------------------------
TSNE_ITER, TSNE_EXAGGERATION_ITER = 40, 20


def _tsne_inputs(fixture):
    def build():
        from tests import tsne_cases as TS
        R, perplexity, m = TS.FIXTURES[fixture]
        return {"x": TS.clusters(R)[0], "perplexity": perplexity, "m": m}
    return build


def _run_tsne(inputs):
    from variantformer_amd import manifold
    _load()
    assert (inputs["m"] > manifold.N_NEIGHBORS_MAX - 1) == (inputs["m"] == 127)          # "A": neighbors.knn; "B": the panels
    out = {}
    for init in ("pca", "random"):
        y, kl = manifold.tsne(inputs["x"], perplexity=inputs["perplexity"], n_iter=TSNE_ITER, exaggeration_iter=TSNE_EXAGGERATION_ITER,
                              init=init, return_kl=True)
        out[init], out[f"{init}-kl"] = _np(y), np.array([kl])
    return out


TSNE_COVERS = ("manifold._tsne_affinities", "manifold._tsne_run", "manifold._tsne_kl")
_case("tsne-A", _tsne_inputs("A"), _run_tsne, TSNE_COVERS + ("neighbors.standardize", "neighbors._knn"),
      ["pca", "random", "pca-kl", "random-kl"], late="x")
_case("tsne-B", _tsne_inputs("B"), _run_tsne, TSNE_COVERS + ("neighbors.standardize", "manifold._knn_panels"),
      ["pca", "random", "pca-kl", "random-kl"], late="x")


# ---- enrichment ------------------------------------------------------------------------------------------------------------------
def _planted_inputs():
    from tests import enrich_cases as EC
    labels, annotations, universe = EC.planted()
    return {"labels": labels, "annotations": annotations, "universe": universe}


def _run_enrich(inputs):
    from variantformer_amd import enrichment
    _load()
    res = enrichment.enrich(inputs["labels"], inputs["annotations"], inputs["universe"])
    out = {k: np.asarray(res[k]) for k in ("count", "term_size", "cluster_size", "log_p", "p", "fold", "q")}
    frame = res["frame"]
    out.update({f"frame-{c}": frame[c].to_numpy() for c in ("cluster", "count", "fold", "log_p", "p", "q")})
    out["frame-term"] = np.array([res["terms"].index(t) for t in frame["term"]])
    return out


def _run_hypergeom(inputs):
    from variantformer_amd import enrichment
    _load()
    m = enrichment.membership(inputs["annotations"], inputs["universe"])
    out = {}
    for alternative in enrichment.ALTERNATIVES:                                 # "greater" and "less": the module has no two-sided test
        res = enrichment.hypergeom(inputs["labels"], m, alternative=alternative, return_steps=True)
        out.update({f"{alternative}-{k}": v for k, v in res.items()})
    return out


_case("enrich-planted", _planted_inputs, _run_enrich, ("enrichment._hypergeom", "enrichment._bh"),
      ["log_p", "p", "fold", "q"], late="labels")
_case("hypergeom-planted", _planted_inputs, _run_hypergeom, ("enrichment._hypergeom",),
      [f"{a}-{k}" for a in ("greater", "less") for k in ("log_p", "p", "tail")], late="labels")


# ---- AD risk ---------------------------------------------------------------------------------------------------------------------
class _MemoryStore:
    """A predictor store whose "paths" are keys of the models a processor already holds: nothing is read from a disk."""

    def get_file_path(self, gene_id, tissue_id):
        return f"memory:{gene_id}:{tissue_id}"


def _ad_risk_inputs():
    from tests import forest_cases as FC
    f = FC.load_ad_risk()["rf"]
    return {"x": np.ascontiguousarray(f["x"], dtype=np.float32), "model": f["model"]}


def _run_ad_risk(inputs):
    """The two predictor paths on the golden forest and its rows: ADrisk.__call__ (one forest, a cohort) and
    ADriskFromVCF._predict_ad_risk (every row through its own forest of a bank, one launch); the processors are made without their
    file and model loading, which is not what allocates."""
    import pandas as pd
    from tests import forest_cases as FC
    from variantformer_amd import forest
    from variantformer_amd.processors import ad_risk
    _load()
    x, model = inputs["x"], inputs["model"]
    one = ad_risk.ADrisk.__new__(ad_risk.ADrisk)
    one.bank = forest.ForestBank([model])
    out = {"cohort": one(x)}
    F = model.n_features
    pairs = [("ENSG_A", 3), ("ENSG_B", 5), ("ENSG_C", 3), ("ENSG_A", 7)]
    models = [model] + [FC.make_forest(500 + i, (64, 65, 130)[i - 1], F, 2, depth=5) for i in (1, 2, 3)]
    many = ad_risk.ADriskFromVCF.__new__(ad_risk.ADriskFromVCF)
    many.ad_preds = _MemoryStore()
    many._models = {many.ad_preds.get_file_path(g, t): m for (g, t), m in zip(pairs, models)}
    many._bank = (None, None)
    many.genes_map = pd.DataFrame({"gene_name": ["a", "b", "c"]}, index=pd.Index(["ENSG_A", "ENSG_B", "ENSG_C"], name="gene_id"))
    xs = _np(x)
    rows = [pairs[i % len(pairs)] for i in range(xs.shape[0])]
    frame = pd.DataFrame({"gene_id": [g for g, _ in rows], "tissue_id": [t for _, t in rows], "embedding": [r[None, :] for r in xs]})
    out["rows"] = many._predict_ad_risk(frame)["ad_risk"].to_numpy()
    return out


_case("ad_risk-golden-rf", _ad_risk_inputs, _run_ad_risk, ("ad_risk.ADrisk.__call__", "ad_risk.ADriskFromVCF._predict_ad_risk"),
      ["cohort", "rows"], late="x")


# ---- coverage --------------------------------------------------------------------------------------------------------------------
def analysis_modules() -> list:
    import importlib
    from tests import write_set_cases as W
    return [importlib.import_module(n) for n in W.ANALYSIS_MODULES]


def _short(module) -> str:
    return module.__name__.rsplit(".", 1)[-1]


def allocating_functions() -> dict:
    """"module.function" / "module.Class.method" -> the number of torch.empty( / torch.empty_like( in its source, for every
    module-level function and every method of a module-level class of the analysis modules that allocates; a nested helper
    counts with the function around it."""
    import inspect
    import re
    out = {}
    for mod in analysis_modules():
        for name, obj in vars(mod).items():
            if getattr(obj, "__module__", None) != mod.__name__:
                continue
            if inspect.isfunction(obj):
                members = [(f"{_short(mod)}.{name}", obj)]
            elif inspect.isclass(obj):
                members = [(f"{_short(mod)}.{name}.{m}", getattr(f, "__func__", f)) for m, f in vars(obj).items()
                           if inspect.isfunction(getattr(f, "__func__", f))]
            else:
                continue
            for qual, fn in members:
                try:
                    source = inspect.getsource(fn)
                except (OSError, TypeError):                                  # generated (a NamedTuple's __new__): no text, no allocation
                    continue
                n = len(re.findall(r"\btorch\.empty(?:_like)?\(", source))
                if n:
                    out[qual] = n
    return out


def uncovered_functions(cases=None) -> list:
    cases = CASES if cases is None else cases
    covered = {f for c in cases for f in c.covers}
    return sorted(f for f in allocating_functions() if f not in covered)

"""The neighbours of a finished prediction, end to end on the GPU: a synthetic format_output frame (60 genes x 54 tissues, embeddings
[54, 64]; neither a model nor a checkpoint is involved) through VCFProcessor.expression_neighbors for both `on` and both `axis`,
neighbors.knn(include_self=True), and neighbors.correlation_distance against 1 - np.corrcoef and through scipy's Ward linkage.
Tolerances are the a-priori bounds of tests/neighbors_cases.py: the standardize bound carried through the dot product, plus tau."""
import numpy as np
import pandas as pd
import pytest
import torch

from tests import neighbors_cases as N

pytestmark = pytest.mark.gpu

GENES, TISSUES, EMB, K = 60, 54, 64, 30
CONSTANT = 7                      # this gene has one expression value in every tissue


def _frame():
    g = np.random.default_rng(20251206)                               # a seed at which the tissue dendrogram's merge heights are well apart
    names = [f"tissue{t:02d}" for t in range(TISSUES)]
    programme = g.standard_normal((6, TISSUES))                       # six expression programmes the genes mix: correlated rows
    expr = (g.standard_normal((GENES, 6)) @ programme + 0.5 * g.standard_normal((GENES, TISSUES)) + 5.0).astype(np.float32)
    expr[CONSTANT] = 2.5
    emb = g.standard_normal((GENES, TISSUES, EMB)).astype(np.float32) + g.standard_normal((1, TISSUES, EMB)).astype(np.float32)
    return pd.DataFrame({"gene_id": [f"ENSG{i:05d}" for i in range(GENES)], "tissues": [list(range(TISSUES))] * GENES,
                         "tissue_names": [names] * GENES, "predicted_expression": [e.reshape(TISSUES, 1) for e in expr],
                         "embeddings": list(emb)}), expr, emb, names


def _distance_bound(m: np.ndarray, center: bool = True):
    """(fp64 distance 1 - corr with constant rows at 1, its error bound [R, R]): |z^_r . z^_j - z_r . z_j| <= |z_r| . e_j + e_r . |z_j| +
    e_r . e_j with e the standardize bound, plus tau of the fp32 chain over the computed rows, plus the subtraction's rounding."""
    z, _ = N.std_reference(m, center)
    e, _ = N.std_bound(m, center)
    a = np.abs(z)
    bound = a @ e.T + e @ a.T + e @ e.T + N.tau(a + e, a + e) + 2 * N.U * 2
    return 1.0 - z @ z.T, bound


def _check_knn(m, labels, ids, dist, flat, self_first=False):
    """ids [R, k] labels, dist fp32 [R, k], flat bool [R] against the fp64 distances of matrix m."""
    want, bound = _distance_bound(m)
    R, k = dist.shape
    pos = {label: n for n, label in enumerate(labels)}
    idx = np.array([[pos[x] for x in row] for row in ids])
    rows = np.arange(R)[:, None]
    assert not np.isnan(dist).any() and (np.diff(dist, axis=1) >= 0).all(), "ascending, never NaN"
    assert all(len(set(r)) == k for r in idx.tolist())
    if self_first:
        assert (idx[:, 0] == rows[:, 0]).all() and (dist[:, 0] == 0).all()
        idx, dist, k = idx[:, 1:], dist[:, 1:], k - 1
    assert (idx != rows).all()
    assert (np.abs(dist - want[rows, idx]) <= bound[rows, idx]).all()
    kept = np.zeros((R, R), dtype=bool)
    kept[rows, idx] = True
    kept[rows, rows] = True
    assert (kept | (want >= dist[:, -1:] - bound[rows, idx[:, -1:]] - bound)).all(), "a row that was left out is nearer than the last"
    const = np.ptp(m, axis=1) == 0
    assert np.array_equal(np.asarray(flat, dtype=bool), const)
    for c in np.flatnonzero(const):                                   # similarity +0.0 with everything: distance exactly 1
        assert (dist[c] == 1).all() and (dist[idx == c] == 1).all()


def test_expression_neighbors_of_genes_and_of_tissues():
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    vp = VCFProcessor()
    df, expr, emb, names = _frame()
    out = vp.expression_neighbors(df)                                 # k = 30, expression, genes
    assert out is df and {"neighbor_ids", "neighbor_distance", "neighbor_degenerate"} <= set(df.columns)
    ids, dist = np.stack(list(df["neighbor_ids"])), np.stack(list(df["neighbor_distance"]))
    assert dist.dtype == np.float32 and dist.shape == (GENES, K)
    _check_knn(expr, list(df["gene_id"]), ids, dist, df["neighbor_degenerate"].to_numpy())
    assert df["neighbor_degenerate"].tolist() == [i == CONSTANT for i in range(GENES)]
    assert (dist[CONSTANT] == 1).all() and ids[CONSTANT].tolist() == [f"ENSG{i:05d}" for i in range(K + 1) if i != CONSTANT][:K]
    tf = vp.expression_neighbors(df, k=10, axis="tissues")
    assert list(tf["tissue"]) == names and len(tf) == TISSUES and not tf["neighbor_degenerate"].any()
    _check_knn(np.ascontiguousarray(expr.T), names, np.stack(list(tf["neighbor_ids"])), np.stack(list(tf["neighbor_distance"])),
               tf["neighbor_degenerate"].to_numpy())


def test_embedding_neighbors_of_one_tissue_and_of_every_gene_tissue_row():
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    vp = VCFProcessor()
    df, expr, emb, names = _frame()
    vp.expression_neighbors(df, k=5, on="embeddings", tissue="tissue03")
    _check_knn(emb[:, 3], list(df["gene_id"]), np.stack(list(df["neighbor_ids"])), np.stack(list(df["neighbor_distance"])),
               df["neighbor_degenerate"].to_numpy())
    vp.expression_neighbors(df, k=4, on="embeddings")
    ids = np.empty((GENES * TISSUES, 4), dtype=object)
    for g, cell in enumerate(df["neighbor_ids"]):
        assert cell.shape == (TISSUES, 4)
        for t in range(TISSUES):
            for i in range(4):
                ids[g * TISSUES + t, i] = tuple(cell[t, i])
    dist = np.concatenate(list(df["neighbor_distance"]))
    flat = np.concatenate(list(df["neighbor_degenerate"]))
    labels = [(g, t) for g in df["gene_id"] for t in names]
    _check_knn(emb.reshape(-1, EMB), labels, ids, dist, flat)


def test_knn_with_the_row_itself_first_and_with_separate_queries():
    from variantformer_amd import neighbors
    df, expr, emb, names = _frame()
    m, labels = neighbors.from_predictions(df)
    i, dd = neighbors.knn(m, k=K, include_self=True)
    assert isinstance(i, np.ndarray) and i.dtype == np.int32 and dd.dtype == np.float32 and i.shape == dd.shape == (GENES, K)
    _check_knn(expr, list(range(GENES)), i, dd, np.ptp(expr, axis=1) == 0, self_first=True)
    i2, d2 = neighbors.knn(m, k=K - 1)
    assert np.array_equal(i[:, 1:], i2) and np.array_equal(dd[:, 1:], d2)
    ti, td = neighbors.knn(torch.from_numpy(m).cuda(), k=K - 1)       # a tensor in, tensors on the device out
    assert ti.is_cuda and np.array_equal(ti.cpu().numpy(), i2) and np.array_equal(td.cpu().numpy(), d2)
    qi, qd = neighbors.knn(m, k=3, queries=m[10:20])                  # separate queries: nothing is excluded, the row finds itself
    want, bound = _distance_bound(expr)
    own = np.arange(10, 20)
    assert (qi[:, 0] == own).all() and (np.abs(qd[:, 0] - want[own, own]) <= bound[own, own]).all()
    ci, cd = neighbors.knn(m, k=GENES + 4 if GENES + 4 <= 64 else 64, metric="cosine")
    assert (ci[:, GENES - 1:] == -1).all() and np.isposinf(cd[:, GENES - 1:]).all() and (ci[:, :GENES - 1] >= 0).all()
    want, bound = _distance_bound(expr, center=False)
    rows = np.arange(GENES)[:, None]
    assert (np.abs(cd[:, :GENES - 1] - want[rows, ci[:, :GENES - 1]]) <= bound[rows, ci[:, :GENES - 1]]).all()


def test_correlation_distance_is_one_minus_corrcoef_and_gives_the_same_dendrogram():
    from scipy.cluster.hierarchy import leaves_list, linkage
    from scipy.spatial.distance import squareform
    from variantformer_amd import neighbors
    df, expr, emb, names = _frame()
    m, labels = neighbors.from_predictions(df, axis="tissues")
    assert labels == names and m.shape == (TISSUES, GENES)
    D = neighbors.correlation_distance(m)
    assert D.dtype == np.float32 and D.shape == (TISSUES, TISSUES) and (np.diag(D) == 0).all() and not np.signbit(np.diag(D)).any()
    ref = 1.0 - np.corrcoef(m.astype(np.float64))
    np.fill_diagonal(ref, 0.0)
    want, bound = _distance_bound(m)
    off = ~np.eye(TISSUES, dtype=bool)
    assert np.abs(want - ref)[off].max() < 1e-12                      # the reference of the bound is numpy's matrix
    assert (np.abs(D - ref)[off] <= bound[off]).all()
    Z_ref = linkage(squareform(ref, checks=False), method="ward")
    Z = linkage(squareform(D.astype(np.float64), checks=False), method="ward")
    heights = np.sort(Z_ref[:, 2])
    # Ward's update weighs three distances with |weights| that sum to at most 3, so the error of a distance passes a level of the
    # tree multiplied by at most 3: 50 bounds between any two merge heights leave room for three levels of that
    assert np.diff(heights).min() > 50 * bound.max(), "the merge heights are well separated against the error of a distance"
    assert np.array_equal(leaves_list(Z), leaves_list(Z_ref)) and np.array_equal(Z[:, :2], Z_ref[:, :2])
    # genes as rows: the constant gene is at distance 1 from every other gene, where numpy has NaN
    G = neighbors.correlation_distance(expr)
    assert not np.isnan(G).any() and (np.delete(G[CONSTANT], CONSTANT) == 1).all() and G[CONSTANT, CONSTANT] == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.isnan(np.corrcoef(expr.astype(np.float64))[CONSTANT]).all()

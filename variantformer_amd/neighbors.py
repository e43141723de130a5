"""Expression and embedding neighbours: the two analysis steps behind vcf2exp that start from a correlation between rows.

  knn(x, k)                  the correlation (or cosine) k-nearest-neighbour graph of the rows of x: what UMAP's
                             metric="correlation", n_neighbors=30 computes first over ~18 000 genes x 49 tissues, and what
                             the same question needs over the registry-token embeddings, ~1 M rows of 1536, where a
                             rows x rows matrix cannot exist;
  correlation_distance(x)    1 - corrcoef(x) with a zero diagonal: what the tissue dendrogram hands to
                             scipy.cluster.hierarchy.linkage through squareform;
  from_predictions(df, ...)  the matrix of either, out of a VCFProcessor.format_output frame, with its row labels.

Both run on the device through three entries of include/vf_hip_neighbors.h: the rows are standardised in
fp32 with two passes (ops.rows_standardize), after which a correlation is a dot product, and the dot products are formed tile
by tile on the f32-input MFMA, either keeping the k best per row (ops.knn_dot: no buffer grows with rows x rows) or writing
the matrix (ops.pairwise_dot).  A similarity's bits depend on the two rows alone.  There is no CPU path: without a GPU the
calls raise, after their arguments have been checked.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .attn_maps import TOP_K_MAX as K_MAX          # VF_TOPK_MAX_K, the one limit of every ranking in the library

METRICS = ("correlation", "cosine")
ON = ("predicted_expression", "embeddings")
AXES = ("genes", "tissues")


def _check_matrix(x, name: str):
    if not isinstance(x, (np.ndarray, torch.Tensor)):
        raise TypeError(f"{name} must be a numpy array or a torch tensor, not {type(x).__name__}")
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError(f"{name} must be a matrix [rows, columns >= 1], not {tuple(x.shape)}")


def _to_device(x, nan_to_zero: bool) -> torch.Tensor:
    """fp32 on the current GPU; NaN -> 0 as np.nan_to_num(x, nan=0.0) does (an Inf becomes the largest finite fp32: the row's
    sum of squares then overflows and the row still comes out NaN)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) if isinstance(x, np.ndarray) else x
    if not torch.cuda.is_available():
        raise ops._lib.VFError("variantformer_amd.neighbors needs a GPU (no CPU fallback)")
    t = t.to(device="cuda", dtype=torch.float32)
    return torch.nan_to_num(t, nan=0.0) if nan_to_zero else t


def standardize(x, metric: str = "correlation", nan_to_zero: bool = True):
    """(z, norm) on the device: the rows of x at zero mean (metric="correlation") and unit norm, and the norms; a row with
    norm 0 (constant, for a correlation) is all zero in z."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, not {metric!r}")
    _check_matrix(x, "x")
    t = _to_device(x, nan_to_zero)
    z = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    norm = torch.empty((t.shape[0],), dtype=torch.float32, device=t.device)
    ops.rows_standardize(t, center=metric == "correlation", z=z, norm=norm, family="neighbors")
    return z, norm


def _back(like, *ts):
    return tuple(t.cpu().numpy() for t in ts) if isinstance(like, np.ndarray) else ts


def _knn(x, k, metric, queries, include_self, nan_to_zero):
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, not {metric!r}")
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= K_MAX:
        raise ValueError(f"k must be an integer in 1 .. {K_MAX}, not {k!r}")
    k = int(k)
    _check_matrix(x, "x")
    if queries is not None:
        _check_matrix(queries, "queries")
        if queries.shape[1] != x.shape[1]:
            raise ValueError(f"queries have {queries.shape[1]} columns, x has {x.shape[1]}")
        if include_self:
            raise ValueError("include_self needs queries=None: a separate query row is no row of x")
    z, norm = standardize(x, metric, nan_to_zero)
    if queries is None:
        zq, nq, self_offset = z, norm, 0
    else:
        zq, nq = standardize(queries, metric, nan_to_zero)
        self_offset = -1
    rows = zq.shape[0]
    indices = torch.empty((rows, k), dtype=torch.int32, device=z.device)
    distances = torch.empty((rows, k), dtype=torch.float32, device=z.device)
    found = k - 1 if include_self else k
    if found:
        ops.knn_dot(zq, z, found, self_offset=self_offset, values=distances[:, k - found:], indices=indices[:, k - found:],
                    family="neighbors")
        distances[:, k - found:].neg_().add_(1.0)                     # 1 - s: the negation is exact
        distances[:, k - found:].masked_fill_(indices[:, k - found:] < 0, float("inf"))
    if include_self:
        indices[:, 0] = torch.arange(rows, dtype=torch.int32, device=z.device)
        distances[:, 0] = 0.0
    return indices, distances, nq


def knn(x, k: int = 30, metric: str = "correlation", queries=None, include_self: bool = False, nan_to_zero: bool = True):
    """The k nearest rows of x for every row of x (or of `queries`), by correlation or cosine distance.

    x [R, d] and queries [Rq, d]: numpy arrays or torch tensors; the result has the type of x (numpy arrays on the host, or
    tensors on the device).  Returns (indices int32 [R, k], distances fp32 [R, k]): distance = 1 - similarity, ascending; the
    row itself is no neighbour of itself.  include_self=True (queries=None only) puts the row itself first at distance 0 and
    k - 1 neighbours behind it, the shape in which neighbour-descent libraries return a graph; umap-learn is not installed
    where this was written, so handing the pair to UMAP(precomputed_knn=...) is NOT pinned by a test.

    Ties go to the lower row.  A row with no variation (norm 0) is at similarity 0, distance 1, from every row, itself
    included; a row that is NaN after nan_to_zero (an Inf in it) is at distance NaN from every row, and NaN distances come
    FIRST, in row order, as in torch.topk.  Where x has fewer than k other rows the index is -1 and the distance +Inf.
    k <= 64.  nan_to_zero: NaN -> 0 before anything else, the notebooks' np.nan_to_num(M, nan=0.0)."""
    indices, distances, _ = _knn(x, k, metric, queries, include_self, nan_to_zero)
    return _back(x, indices, distances)


def correlation_distance(x, nan_to_zero: bool = True):
    """fp32 [R, R]: 1 - corrcoef(x) with the diagonal exactly 0 -- what vcf2exp's compute_ordered_leaves passes to
    scipy.spatial.distance.squareform(checks=False) and on to linkage.  For row counts at which R x R exists (the tissues of
    a dendrogram; 18 000 genes are 1.3 GB).  A constant row is at distance 1 from every other row where numpy gives NaN."""
    _check_matrix(x, "x")
    z, _ = standardize(x, "correlation", nan_to_zero)
    out = torch.empty((z.shape[0], z.shape[0]), dtype=torch.float32, device=z.device)
    ops.pairwise_dot(z, z, mode=1, self_offset=0, out=out, family="neighbors")
    return _back(x, out)[0]


def _tissue_names(df):
    col = "tissue_names" if "tissue_names" in df.columns else "tissues"
    names = [list(t.split(",")) if isinstance(t, str) else list(t) for t in df[col]]
    if any(n != names[0] for n in names):
        raise ValueError("every gene of the frame must have been predicted in the same tissues, in the same order")
    return names[0]


def from_predictions(df, on: str = "predicted_expression", axis: str = "genes", tissue=None, nan_to_zero: bool = True):
    """The matrix of a neighbour search out of a VCFProcessor.format_output frame (one row per gene; `predicted_expression`
    [tissues] and `embeddings` [tissues, emb] per row).  Returns (matrix fp32, labels), labels[i] naming row i:
      on="predicted_expression", axis="genes"    [genes, tissues], labels = gene ids       (the UMAP of vcf2embed);
      on="predicted_expression", axis="tissues"  [tissues, genes], labels = tissue names   (the tissue dendrogram);
      on="embeddings", tissue=name or position   [genes, emb] of that tissue, labels = gene ids;
      on="embeddings", tissue=None               [genes * tissues, emb], gene-major, labels = (gene id, tissue name).
    nan_to_zero: np.nan_to_num(matrix, nan=0.0), as the notebooks do before a correlation."""
    if on not in ON:
        raise ValueError(f"on must be one of {ON}, not {on!r}")
    if axis not in AXES:
        raise ValueError(f"axis must be one of {AXES}, not {axis!r}")
    if on not in df.columns or "gene_id" not in df.columns:
        raise ValueError(f"the frame has no `{on}` / `gene_id` column: pass what format_output returned")
    if len(df) == 0:
        raise ValueError("the frame has no rows")
    tissues = _tissue_names(df)
    genes = list(df["gene_id"])
    if on == "predicted_expression":
        if tissue is not None:
            raise ValueError("tissue selects among embeddings; an expression matrix has every tissue")
        m = np.stack([np.asarray(v, dtype=np.float32).reshape(-1) for v in df[on]])
        if m.shape[1] != len(tissues):
            raise ValueError(f"{m.shape[1]} expression values per gene for {len(tissues)} tissues")
        m, labels = (m, genes) if axis == "genes" else (np.ascontiguousarray(m.T), list(tissues))
    else:
        if axis != "genes":
            raise ValueError("embeddings have genes (or gene, tissue pairs) as rows: axis must be 'genes'")
        e = np.stack([np.asarray(v, dtype=np.float32).reshape(len(tissues), -1) for v in df[on]])       # [genes, tissues, emb]
        if tissue is None:
            m, labels = e.reshape(-1, e.shape[-1]), [(g, t) for g in genes for t in tissues]
        else:
            if isinstance(tissue, str):
                if tissue not in tissues:
                    raise ValueError(f"tissue {tissue!r} is not among the frame's {len(tissues)} tissues")
                pos = tissues.index(tissue)
            else:
                pos = int(tissue)
                if not 0 <= pos < len(tissues):
                    raise ValueError(f"tissue position {pos} outside 0 .. {len(tissues) - 1}")
            m, labels = np.ascontiguousarray(e[:, pos]), genes
    return (np.nan_to_num(m, nan=0.0) if nan_to_zero else m), labels

"""Cluster validation: the silhouette coefficient of a flat clustering, the answer to "how many clusters?" that kmeans.kmeans,
linkage.cut and expression_enrichment leave to the user.

  silhouette_samples(x, labels, metric)   per row: s = (b - a) / max(a, b), a, b and the nearest other cluster; the mean score;
  silhouette_score(x, labels, metric)     the mean of the labelled rows' s alone;
  silhouette_sweep(x, ks, method)         cluster at every k of `ks` (k-means, or one Ward tree cut once per k) and score each.

Definitions are scikit-learn's silhouette_samples.  Everything runs on the device through the three entries of
include/vf_hip_silhouette.h.  metric="euclidean" needs all pairs: every row against every member of every cluster,
the squared distance k-means' fp32 chain, then a correctly rounded square root and fp64 sums in a stated order.
metric="correlation" / "cosine" is linear: the sum of 1 - z_i . z_j over a cluster is n_c - z_i . M_c with M_c the cluster's
fp64 column sums of the standardised rows, O(rows k d), never all pairs.  There is no atomic, so a run has one result, bit for
bit, whatever `max_bytes` cuts the rows into, and tests/silhouette_cases.py restates every entry in numpy.  There is no CPU path:
without a GPU the calls raise, after their arguments have been checked.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import neighbors, ops

METRICS = ("euclidean", "correlation", "cosine")
STANDARDIZE = (None, "correlation", "cosine")
METHODS = ("kmeans", "ward")
MAX_K = ops.SILHOUETTE_MAX_K
DEFAULT_MAX_BYTES = 1 << 28


class SilhouetteResult(NamedTuple):
    """samples fp64 [rows]: s, NaN for a row without a label;  a, b fp64 [rows];  nearest [rows]: the label (a value of `classes`)
    of the cluster that gives b, for every row, `none` (-1 for numeric labels) where there is none;  nearest_index int32 [rows]:
    the same as a position in `classes`, -1 for none;  score: the mean of the labelled rows' s;  classes [k]: the distinct labels,
    ascending;  cluster_sizes int64 [k];  cluster_means fp64 [k]: the mean s of every cluster.  Arrays are numpy on the host for
    a numpy x, tensors on the device for a tensor x (classes, nearest and the cluster arrays are always numpy)."""
    samples: object
    a: object
    b: object
    nearest: np.ndarray
    nearest_index: object
    score: float
    classes: np.ndarray
    cluster_sizes: np.ndarray
    cluster_means: np.ndarray


def encode_labels(labels, rows: int):
    """(codes int32 [rows], classes [k]): the labels mapped through np.unique to 0 .. k - 1, ascending; -1 for a row without a
    label: a negative number (k-means gives a NaN row -1) or a NaN.  Labels of any dtype; strings are all labels."""
    if isinstance(labels, torch.Tensor):
        labels = labels.detach().cpu().numpy()
    lab = np.asarray(labels)
    if lab.ndim != 1 or lab.shape[0] != rows:
        raise ValueError(f"labels must be one per row, [{rows}], not {tuple(lab.shape)}")
    if lab.dtype.kind in "iuf":
        has = lab >= 0                                                    # a NaN compares false
    elif lab.dtype.kind == "b":
        has = np.ones(rows, bool)
    else:
        has = np.array([not (isinstance(v, (int, float, np.integer, np.floating)) and not v >= 0) for v in lab], bool)
    codes = np.full(rows, -1, np.int32)
    classes, inverse = np.unique(lab[has], return_inverse=True)
    codes[has] = inverse.astype(np.int32)
    return codes, classes


def _check(metric, standardize, max_bytes):
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, not {metric!r}")
    if standardize not in STANDARDIZE:
        raise ValueError(f"standardize must be one of {STANDARDIZE}, not {standardize!r}")
    if standardize is not None and metric != "euclidean":
        raise ValueError(f"standardize={standardize!r} goes with metric='euclidean': metric={metric!r} standardises the rows itself")
    if isinstance(max_bytes, bool) or not isinstance(max_bytes, (int, np.integer)) or max_bytes < 1:
        raise ValueError(f"max_bytes must be a positive integer, not {max_bytes!r}")


def chunk_rows(rows: int, k: int, max_bytes: int) -> int:
    """Query rows per launch: the fp64 [k, rows] buffer stays within max_bytes, at least one row."""
    return max(1, min(rows, int(max_bytes) // (8 * k)))


def _clusters(codes: np.ndarray, k: int, device):
    """(labels32 int32 [R], order int32 [n], seg int64 [k + 1]) on the device: the clusters as a CSR of rows, by a stable sort."""
    has = np.nonzero(codes >= 0)[0]
    order_h = has[np.argsort(codes[has], kind="stable")].astype(np.int32)
    seg_h = np.zeros(k + 1, np.int64)
    seg_h[1:] = np.cumsum(np.bincount(codes[has], minlength=k))
    labels32 = torch.empty((codes.shape[0],), dtype=torch.int32, device=device)
    order = torch.empty((order_h.shape[0],), dtype=torch.int32, device=device)
    seg = torch.empty((k + 1,), dtype=torch.int64, device=device)
    labels32.copy_(torch.from_numpy(codes))
    order.copy_(torch.from_numpy(order_h))
    seg.copy_(torch.from_numpy(seg_h))
    return labels32, order, seg, np.diff(seg_h)


def silhouette_samples(x, labels, metric: str = "euclidean", standardize=None, nan_to_zero: bool = True,
                       max_bytes: int = DEFAULT_MAX_BYTES) -> SilhouetteResult:
    """The silhouette of every row of x [R, d] (a numpy array or a torch tensor) under the flat clustering `labels` [R].

    metric       "euclidean": the rows as they are (UMAP / t-SNE coordinates, k-means clusters), all pairs on the device;
                 "correlation" / "cosine": the distance 1 - z_i . z_j of the standardised rows (the Ward tree's distance,
                 scikit-learn's metric="correlation"), linear in the rows.
    standardize  with metric="euclidean" only: "correlation" / "cosine" standardise the rows first (neighbors.standardize): the
                 space kmeans(metric="correlation") clusters in, where |a - b|^2 = 2 (1 - corr).
    labels       any dtype, mapped through np.unique; a negative number or a NaN is no label: that row has samples NaN and is left
                 out of the score, but still gets b and nearest.
    max_bytes    bounds the fp64 [clusters, rows] buffer: the rows are taken in chunks; the result does not depend on it.
    A cluster of one row has s = 0, as has a row with max(a, b) == 0.  Fewer than two non-empty clusters raise ValueError, as in
    scikit-learn; more than 4096 (k-means' limit) are refused."""
    _check(metric, standardize, max_bytes)
    neighbors._check_matrix(x, "x")
    R, d = int(x.shape[0]), int(x.shape[1])
    if R > ops.SILHOUETTE_MAX_R or d > ops.SILHOUETTE_MAX_D:
        raise ValueError(f"x is {R} x {d}: at most 2^24 rows and {ops.SILHOUETTE_MAX_D} columns")
    codes, classes = encode_labels(labels, R)
    k = int(classes.shape[0])
    if k < 2:
        raise ValueError(f"the labels name {k} cluster(s): a silhouette needs at least 2")
    if k > MAX_K:
        raise ValueError(f"the labels name {k} clusters: at most {MAX_K}")
    if metric == "euclidean" and standardize is None:
        z = neighbors._to_device(x, nan_to_zero).contiguous()
    else:
        z = neighbors.standardize(x, metric if metric != "euclidean" else standardize, nan_to_zero)[0]
    dev = z.device
    labels32, order, seg, sizes = _clusters(codes, k, dev)
    a = torch.empty((R,), dtype=torch.float64, device=dev)
    b = torch.empty((R,), dtype=torch.float64, device=dev)
    s = torch.empty((R,), dtype=torch.float64, device=dev)
    nearest = torch.empty((R,), dtype=torch.int32, device=dev)
    step = chunk_rows(R, k, max_bytes)
    S = torch.empty((k, step), dtype=torch.float64, device=dev)
    work = torch.empty((ops.silhouette_dot_work_bytes(d, k) // 8,), dtype=torch.float64, device=dev) if metric != "euclidean" else None
    for row0 in range(0, R, step):
        rows = min(step, R - row0)
        view = S[:, :rows]
        if metric == "euclidean":
            ops.silhouette_sums_l2(z, order, seg, row0, rows, S=view, family="validation")
        else:
            ops.silhouette_sums_dot(z, order, seg, labels32, row0, rows, S=view, work=work, family="validation")
        ops.silhouette_finish(view, labels32, seg, row0, rows, a=a, b=b, s=s, nearest=nearest, family="validation")
    s_host = s.cpu().numpy()
    near_host = nearest.cpu().numpy()
    has = codes >= 0
    score = math.fsum(s_host[has].tolist()) / int(has.sum())             # correctly rounded: no order to state
    with np.errstate(all="ignore"):
        means = np.array([math.fsum(s_host[codes == c].tolist()) / int(sizes[c]) for c in range(k)], np.float64)
    if classes.dtype.kind in "iuf":
        near_labels = np.where(near_host >= 0, classes[np.maximum(near_host, 0)], -1)
    else:
        near_labels = np.array([classes[c] if c >= 0 else None for c in near_host], dtype=object)
    s_out, a_out, b_out, near_out = neighbors._back(x, s, a, b, nearest)
    return SilhouetteResult(s_out, a_out, b_out, near_labels, near_out, score, classes, sizes.astype(np.int64), means)


def silhouette_score(x, labels, metric: str = "euclidean", standardize=None, nan_to_zero: bool = True,
                     max_bytes: int = DEFAULT_MAX_BYTES) -> float:
    """The mean silhouette of the labelled rows: math.fsum(samples) / n on the host, which is correctly rounded."""
    return silhouette_samples(x, labels, metric, standardize, nan_to_zero, max_bytes).score


class SweepResult(NamedTuple):
    """ks: the cluster counts tried;  scores: the silhouette score of each;  labels: the int32 [rows] labels of each;  inertia: the
    k-means inertia of each (None for method="ward");  best_k: the k of the largest score, ties to the first."""
    ks: list
    scores: list
    labels: list
    inertia: object
    best_k: int


def silhouette_sweep(x, ks, method: str = "kmeans", metric: str = "correlation", nan_to_zero: bool = True,
                     max_bytes: int = DEFAULT_MAX_BYTES, **kwargs) -> SweepResult:
    """Cluster the rows of x at every k of `ks` and score each clustering by its silhouette.

    method="kmeans"  kmeans.kmeans(x, k, metric=metric, **kwargs) per k; scored by the Euclidean silhouette in the space the loop
                     ran in: the rows themselves for metric="euclidean", the standardised rows for "correlation" / "cosine".
    method="ward"    one tree, linkage.ward_of_rows(x) (correlation distances, metric must be "correlation"), cut once per k by
                     linkage.cut; scored by the correlation silhouette, the tree's own distance.
    Every k must be an integer in 2 .. rows - 1."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, not {metric!r}")
    if method == "ward" and metric != "correlation":
        raise ValueError("method='ward' builds the tree on correlation distances: metric must be 'correlation'")
    if method == "ward" and kwargs:
        raise ValueError(f"method='ward' takes no further arguments, not {sorted(kwargs)}")
    neighbors._check_matrix(x, "x")
    R = int(x.shape[0])
    ks = [ks] if isinstance(ks, (int, np.integer)) and not isinstance(ks, bool) else list(ks)
    if not ks:
        raise ValueError("ks names no cluster count")
    for k in ks:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 2 <= int(k) <= R - 1:
            raise ValueError(f"every k must be an integer in 2 .. rows - 1 = {R - 1}, not {k!r}")
    ks = [int(k) for k in ks]
    _check("euclidean", None, max_bytes)
    scores, all_labels, inertia = [], [], ([] if method == "kmeans" else None)
    if method == "ward":
        from . import linkage
        cuts = np.asarray(linkage.cut(linkage.ward_of_rows(x, nan_to_zero=nan_to_zero), ks))
        cuts = cuts.reshape(R, len(ks))
    for i, k in enumerate(ks):
        if method == "kmeans":
            from . import kmeans
            model = kmeans.kmeans(x, k, metric=metric, nan_to_zero=nan_to_zero, **kwargs)
            labels = model.labels.cpu().numpy() if isinstance(model.labels, torch.Tensor) else np.asarray(model.labels)
            inertia.append(model.inertia)
            res = silhouette_samples(x, labels, "euclidean", None if metric == "euclidean" else metric, nan_to_zero, max_bytes)
        else:
            labels = cuts[:, i].astype(np.int32)
            res = silhouette_samples(x, labels, "correlation", None, nan_to_zero, max_bytes)
        scores.append(res.score)
        all_labels.append(labels.astype(np.int32))
    best = max(range(len(ks)), key=lambda i: (scores[i] == scores[i], scores[i] if scores[i] == scores[i] else -2.0, -i))
    return SweepResult(ks, scores, all_labels, inertia, ks[best])

"""k-means clustering of predictions and embeddings: the flat clusters the vcf2embed notebook wants for "GO term enrichment
within UMAP clusters", and the assignment of a second individual's rows to the clusters of a first.

  kmeans(x, n_clusters, ...)   Lloyd's algorithm, scikit-learn's KMeans(algorithm="lloyd"): returns a KMeansModel;
  KMeansModel.predict(q)       the nearest fitted centre of every query row: an assignment alone;
  random_rows / seed_rows      the two starts: k distinct rows from a counter hash, or plain D^2 seeding on the device.

Everything runs on the device through the four entries of include/vf_hip_kmeans.h: the squared distance is a
running fp32 sum of (x - c)^2 in column order with no fma, the means are fp64 sums in a stated order, all iterations of a run
come from one loop inside the library and the stop is decided on the device.  There is no atomic, so a run has one result, bit
for bit, and tests/kmeans_cases.py restates every entry in numpy.  It is linear in the rows: 262 144 x 64 with 1 024 centres
runs where a Ward tree cannot exist.  There is no CPU path: without a GPU the calls raise, after their arguments have been checked.

Deviations from scikit-learn, all three documented in DESIGN.md 5o: init="k-means++" is plain D^2 seeding (one candidate per
step, from a counter hash), not the greedy variant with 2 + log k trials; a cluster that ends empty keeps its centre and raises
a warning where scikit-learn relocates the centre; the distance is the direct form, not |c|^2 - 2 x.c.  Given the same start,
labels and n_iter equal scikit-learn's wherever no row sits within rounding of two centres (tests/test_kmeans_cpu.py).
"""
from __future__ import annotations

import math
import warnings

import numpy as np
import torch

from . import neighbors, ops

METRICS = ("correlation", "cosine", "euclidean")
INITS = ("k-means++", "random")
MAX_K = ops.KMEANS_MAX_K
_MASK = 0xFFFFFFFF


def _mix32(x: int) -> int:
    """The 32-bit mixer of include/vf_hip_umap.h on a Python integer."""
    x &= _MASK
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _MASK
    x ^= x >> 15
    x = (x * 0x846CA68B) & _MASK
    return x ^ (x >> 16)


def hash64(seed: int, t: int) -> int:
    """hash(seed, t) of include/vf_hip_kmeans.h: 64 bits from two words of the mixer."""
    a = _mix32((int(seed) & _MASK) + 0x9E3779B9)
    return (_mix32(a ^ (2 * t)) << 32) | _mix32(a ^ (2 * t + 1))


def mulhi64(h: int, n: int) -> int:
    return (h * n) >> 64


def random_rows(rows: int, k: int, seed: int) -> np.ndarray:
    """int32 [k]: k distinct rows out of `rows`, the first k steps of a Fisher-Yates shuffle whose step i swaps position i with
    position i + mulhi64(hash64(seed, i), rows - i).  Host integers alone: numpy restates it, and it does not depend on a generator."""
    moved = {}
    out = np.empty(k, dtype=np.int32)
    for i in range(k):
        j = i + mulhi64(hash64(seed, i), rows - i)
        vi, vj = moved.get(i, i), moved.get(j, j)
        moved[i], moved[j] = vj, vi
        out[i] = vj
    return out


def _check_seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 63:
        raise ValueError(f"seed must be an integer in 0 .. 2^63 - 1, not {seed!r}")
    return int(seed)


def _rows_of(x, metric: str, nan_to_zero: bool) -> torch.Tensor:
    """The rows Lloyd's loop sees, fp32 on the device: standardised for a correlation or a cosine, where |a - b|^2 = 2 (1 - corr)."""
    if metric == "euclidean":
        return neighbors._to_device(x, nan_to_zero).contiguous()
    return neighbors.standardize(x, metric, nan_to_zero)[0]


def seed_rows(z: torch.Tensor, k: int, seed: int):
    """(rows int32 [k], centres fp32 [k, d]) on the device: plain D^2 seeding of the rows of z (ops.kmeans_seed)."""
    R, d = z.shape
    rows = torch.empty((k,), dtype=torch.int32, device=z.device)
    cen = torch.empty((k, d), dtype=torch.float32, device=z.device)
    mind = torch.empty((R,), dtype=torch.float32, device=z.device)
    work = torch.empty((ops.kmeans_seed_work_bytes(R) + 7) // 8, dtype=torch.int64, device=z.device)
    ops.kmeans_seed(z, k, seed, rows=rows, cen=cen, mind=mind, work=work, family="kmeans")
    return rows, cen


def _assign(z: torch.Tensor, cen: torch.Tensor, chunk_rows=None):
    R = z.shape[0]
    labels = torch.empty((R,), dtype=torch.int32, device=z.device)
    dist = torch.empty((R,), dtype=torch.float32, device=z.device)
    step = R if chunk_rows is None else int(chunk_rows)
    for r0 in range(0, R, max(step, 1)):
        ops.kmeans_assign(z[r0:r0 + step], cen, labels=labels[r0:r0 + step], dist=dist[r0:r0 + step], family="kmeans")
    return labels, dist


def _inertia(labels: torch.Tensor, dist: torch.Tensor) -> float:
    """The fp64 sum of dist over the labelled rows."""
    return float(torch.where(labels >= 0, dist.to(torch.float64), torch.zeros((), dtype=torch.float64, device=dist.device)).sum())


def _lloyd(z: torch.Tensor, cen: torch.Tensor, max_iter: int, tol_abs: float):
    """One run from the centres in `cen` (overwritten): (labels, dist, n_iter, shift)."""
    R, d = z.shape
    k = cen.shape[0]
    dev = z.device
    labels = torch.empty((R,), dtype=torch.int32, device=dev)
    prev = torch.empty((R,), dtype=torch.int32, device=dev)
    dist = torch.empty((R,), dtype=torch.float32, device=dev)
    counts = torch.empty((k,), dtype=torch.int32, device=dev)
    n_iter = torch.empty((1,), dtype=torch.int32, device=dev)
    shift = torch.empty((max_iter,), dtype=torch.float64, device=dev)
    changed = torch.empty((max_iter,), dtype=torch.int64, device=dev)
    work = torch.empty((ops.kmeans_lloyd_work_bytes(R, d, k) + 7) // 8, dtype=torch.int64, device=dev)
    ops.kmeans_lloyd(z, cen, max_iter=max_iter, tol_abs=tol_abs, resume=False, labels=labels, dist=dist, prev_labels=prev, counts=counts,
                     n_iter=n_iter, shift=shift, changed=changed, work=work, family="kmeans")
    n = int(n_iter.item())
    return labels, dist, n, shift[:n]


class KMeansModel:
    """A fitted k-means: labels int32 [rows], centers fp32 [k, d] (in the standardised space for metric="correlation" /
    "cosine"), inertia (the fp64 sum of the labelled rows' squared distances), n_iter, counts int64 [k] (the members of every
    cluster among `labels`), metric.  Arrays have the type of the fitted x: numpy on the host, or tensors on the device."""

    def __init__(self, labels, centers, inertia, n_iter, counts, metric, nan_to_zero=True, shift=None):
        self.labels, self.centers, self.inertia, self.n_iter, self.counts = labels, centers, float(inertia), int(n_iter), counts
        self.metric, self.nan_to_zero, self.shift = metric, bool(nan_to_zero), shift

    @property
    def n_clusters(self) -> int:
        return int(self.centers.shape[0])

    @property
    def columns(self) -> int:
        return int(self.centers.shape[1])

    def predict(self, queries, chunk_rows=None, return_distance: bool = False):
        """int32 [rows]: the nearest centre of every row of `queries` (standardised like the fit's rows for a correlation or a
        cosine): ops.kmeans_assign alone, `chunk_rows` rows per launch (None: all at once; the result is the same, bit for bit).
        -1 for a row that is NaN.  return_distance=True adds the squared distances fp32 [rows]."""
        neighbors._check_matrix(queries, "queries")
        if queries.shape[1] != self.columns:
            raise ValueError(f"queries have {queries.shape[1]} columns, the model was fitted on {self.columns}")
        if chunk_rows is not None and (isinstance(chunk_rows, bool) or int(chunk_rows) != chunk_rows or int(chunk_rows) < 1):
            raise ValueError(f"chunk_rows must be a positive integer or None, not {chunk_rows!r}")
        z = _rows_of(queries, self.metric, self.nan_to_zero)
        cen = neighbors._to_device(self.centers, False).contiguous()
        labels, dist = _assign(z, cen, chunk_rows)
        out = neighbors._back(queries, labels, dist)
        return out if return_distance else out[0]

    def state(self) -> dict:
        """Plain numpy arrays and scalars: what np.savez takes and from_state gives back."""
        host = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        return {"labels": host(self.labels), "centers": host(self.centers), "inertia": self.inertia, "n_iter": self.n_iter,
                "counts": host(self.counts), "metric": self.metric, "nan_to_zero": self.nan_to_zero}

    @classmethod
    def from_state(cls, state: dict) -> "KMeansModel":
        metric = str(state["metric"])
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS}, not {metric!r}")
        centers = np.ascontiguousarray(state["centers"], dtype=np.float32)
        if centers.ndim != 2 or not 1 <= centers.shape[0] <= MAX_K:
            raise ValueError(f"centers must be [1 .. {MAX_K}, columns], not {centers.shape}")
        return cls(np.asarray(state["labels"], dtype=np.int32), centers, float(state["inertia"]), int(state["n_iter"]),
                   np.asarray(state["counts"], dtype=np.int64), metric, bool(state["nan_to_zero"]))


def kmeans(x, n_clusters: int, metric: str = "correlation", init="k-means++", n_init: int = 1, max_iter: int = 300, tol: float = 1e-4,
           seed: int = 0, nan_to_zero: bool = True) -> KMeansModel:
    """Lloyd's k-means of the rows of x [R, d] (a numpy array or a torch tensor) into n_clusters flat clusters.

    metric   "correlation" / "cosine": the rows are standardised (neighbors.standardize) and clustered by Euclidean distance
             there, |a - b|^2 = 2 (1 - corr); the centres are means of standardised rows and are not renormalised.  "euclidean":
             the rows as they are (the coordinates of an embedding).
    init     "k-means++": plain D^2 seeding on the device from a counter hash of (seed, step);  "random": k distinct rows from the
             same hash (random_rows);  an array [n_clusters, d]: the start itself, in the space Lloyd's loop runs in.
    n_init   runs with the seeds seed, seed + 1, ..; the lowest inertia is kept, ties to the first.  An array start runs once.
    tol      scikit-learn's: the loop stops when the summed squared shift of the centres is <= tol * the mean column variance of
             the rows (formed here in fp64), or when no label changes.  max_iter bounds the iterations.
    A cluster that ends without rows keeps its centre and raises a warning.  n_clusters above the rows, or above 4096 (what
    expression_enrichment takes), is refused."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, not {metric!r}")
    neighbors._check_matrix(x, "x")
    if isinstance(n_clusters, bool) or not isinstance(n_clusters, (int, np.integer)) or n_clusters < 1:
        raise ValueError(f"n_clusters must be a positive integer, not {n_clusters!r}")
    k, R, d = int(n_clusters), int(x.shape[0]), int(x.shape[1])
    if k > MAX_K:
        raise ValueError(f"n_clusters={k} is above {MAX_K}")
    if k > R:
        raise ValueError(f"n_clusters={k} is above the {R} rows")
    if R > ops.KMEANS_MAX_R or d > ops.KMEANS_MAX_D:
        raise ValueError(f"x is {R} x {d}: at most 2^24 rows and {ops.KMEANS_MAX_D} columns")
    start = None
    if isinstance(init, str):
        if init not in INITS:
            raise ValueError(f"init must be one of {INITS} or an array [n_clusters, columns], not {init!r}")
    else:
        if not isinstance(init, (np.ndarray, torch.Tensor)) or init.ndim != 2 or tuple(init.shape) != (k, d):
            raise ValueError(f"an init array must be [{k}, {d}], not {tuple(getattr(init, 'shape', ()))}")
        start = init
    if isinstance(n_init, bool) or not isinstance(n_init, (int, np.integer)) or n_init < 1:
        raise ValueError(f"n_init must be a positive integer, not {n_init!r}")
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError(f"max_iter must be a positive integer, not {max_iter!r}")
    if not (isinstance(tol, (int, float, np.floating)) and tol >= 0 and math.isfinite(tol)):
        raise ValueError(f"tol must be a finite number >= 0, not {tol!r}")
    seed = _check_seed(seed)
    z = _rows_of(x, metric, nan_to_zero)
    # scikit-learn's _tolerance: tol * mean(var(X, axis=0)); rows that are not finite would make it NaN, and then the labels alone stop the loop
    tol_abs = float(tol) * float(z.to(torch.float64).var(dim=0, unbiased=False).mean())
    if not math.isfinite(tol_abs):
        tol_abs = 0.0
    best = None
    for run in range(1 if start is not None else int(n_init)):
        if start is not None:
            cen = torch.empty((k, d), dtype=torch.float32, device=z.device)
            cen.copy_(neighbors._to_device(start, False))
        elif init == "random":
            cen = torch.empty((k, d), dtype=torch.float32, device=z.device)
            cen.copy_(z[torch.from_numpy(random_rows(R, k, seed + run).astype(np.int64)).to(z.device)])
        else:
            cen = seed_rows(z, k, seed + run)[1]
        labels, dist, n, shift = _lloyd(z, cen, int(max_iter), tol_abs)
        inertia = _inertia(labels, dist)
        if best is None or inertia < best[0]:
            best = (inertia, labels, cen, n, shift)
    inertia, labels, cen, n, shift = best
    counts = torch.bincount(labels[labels >= 0].to(torch.int64), minlength=k)
    empty = int((counts == 0).sum())
    if empty:
        warnings.warn(f"{empty} of the {k} clusters ended without rows and keep their centres (scikit-learn would relocate them)", RuntimeWarning)
    labels, cen, counts, shift = neighbors._back(x, labels, cen, counts, shift)
    return KMeansModel(labels, cen, inertia, n, counts, metric, nan_to_zero, shift)

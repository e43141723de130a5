"""References, fixtures and the case table of the silhouette entries (include/vf_hip_silhouette.h); importable
without a GPU.

The numpy restatement is THE CONTRACT: every operation of the header in the header's order, individually rounded, so the device
must equal it bit for bit (a NaN equals any NaN: its sign and payload are the hardware's).  The squared distance is
tests/kmeans_cases.distances, THE DISTANCE itself; np.sqrt on fp32 is correctly rounded; a range's ascending fp64 sum from +0.0 is
np.cumsum behind a leading zero (np.sum would add pairwise).  The restatement is pinned to scikit-learn 1.7.2's
silhouette_samples and to a brute-force definition on exhaustive tiny cases in tests/test_silhouette_cpu.py.

Which launch writes each element that is later read (the read-before-write table of variantformer_amd/validation.py's
allocations; tests/test_silhouette_nets_gpu.py poisons every one of them):
  _clusters            labels32, order, seg   Tensor.copy_ of the whole buffer, from the host arrays
  silhouette_samples   S[c, q]                silhouette_l2_kernel / silhouette_dot_kernel of the chunk: every (c, q) of the chunk's
                                              view, an empty cluster's +0.0 included; read by silhouette_finish_kernel of the chunk
                       work (M[c, col])       silhouette_colsum_kernel of every chunk, every (c, col), before the dot kernel reads it
                       a, b, s, nearest [i]   silhouette_finish_kernel of the chunk that holds row i; the chunks tile [0, R)
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from tests import kmeans_cases as K

F32, F64 = np.float32, np.float64
# include/vf_hip_silhouette.h
MAX_K, MAX_R, MAX_D = K.MAX_K, K.MAX_R, K.MAX_D
RANGES, ROWS, JT, DC_SMALL, DC, DC_WIDE = 4, 64, 8, 4, 32, 64
NAMES = ["vf_silhouette_finish", "vf_silhouette_sums_dot", "vf_silhouette_sums_l2"]

# The largest |s - scikit-learn's s| of the restatement over FIXTURES, measured on the CPU with scikit-learn 1.7.2 on the fp64
# copies of the same fp32 rows (tests/test_silhouette_cpu.py prints every fixture's figure: 1.7e-8 .. 5.4e-8 for the Euclidean
# fixtures; the largest is 1.309e-7, on D-corr-49: there the rows are standardised in fp32 before the entries see them, and
# 1 - z_i . z_j inherits that against scikit-learn's own centring and norms in fp64).  The tests allow 4 x this value, the rule of
# the t-SNE tests: fp32 distances against fp64.
MEASURED_ERROR = 1.31e-7
TOLERANCE = 4 * MEASURED_ERROR


def dot_work_bytes(d, k):
    return 8 * k * d


def same_bits(got, want) -> bool:
    """Bit equality, except that a NaN equals any NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    nan = np.isnan(want)
    view = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(view)[~nan], want.view(view)[~nan]))


# ---- THE CLUSTERS --------------------------------------------------------------------------------------------------------------------
def csr(labels, k):
    """(order int32 [n], seg int64 [k + 1]): the rows with a label in 0 .. k - 1 by a stable sort of the labels, and the offsets."""
    labels = np.asarray(labels)
    has = np.nonzero((labels >= 0) & (labels < k))[0]
    order = has[np.argsort(labels[has], kind="stable")].astype(np.int32)
    seg = np.zeros(k + 1, np.int64)
    seg[1:] = np.cumsum(np.bincount(labels[has].astype(np.int64), minlength=k))
    return order, seg


def ranged_sum(V):
    """THE RANGES over the last axis of V fp64 [.., n_c]: RANGES contiguous ranges of ceil(n_c / RANGES), each added ascending
    from +0.0, the ranges' sums added in range order."""
    V = np.asarray(V, dtype=F64)
    n = V.shape[-1]
    L = (n + RANGES - 1) // RANGES
    total = None
    with np.errstate(all="ignore"):
        for v in range(RANGES):
            lo, hi = min(v * L, n), min((v + 1) * L, n)
            lead = np.zeros(V.shape[:-1] + (1,), F64)
            p = np.cumsum(np.concatenate([lead, V[..., lo:hi]], axis=-1), axis=-1)[..., -1]
            total = p if total is None else total + p
    return total


# ---- the three entries ---------------------------------------------------------------------------------------------------------------
def sums_l2(x, order, seg, row0=0, rows=None):
    """vf_silhouette_sums_l2: S fp64 [k, rows]."""
    x = np.asarray(x, dtype=F32)
    rows = x.shape[0] - row0 if rows is None else rows
    k = len(seg) - 1
    S = np.zeros((k, rows), F64)
    with np.errstate(all="ignore"):
        for c in range(k):
            members = order[seg[c]:seg[c + 1]]
            if len(members):
                S[c] = ranged_sum(np.sqrt(K.distances(x[row0:row0 + rows], x[members])).astype(F64))
    return S


def col_sums(z, order, seg):
    """The first launch of vf_silhouette_sums_dot: M fp64 [k, d]."""
    z = np.asarray(z, dtype=F32)
    k = len(seg) - 1
    M = np.zeros((k, z.shape[1]), F64)
    for c in range(k):
        M[c] = ranged_sum(z[order[seg[c]:seg[c + 1]]].astype(F64).T)
    return M


def sums_dot(z, order, seg, labels, row0=0, rows=None):
    """vf_silhouette_sums_dot: (S fp64 [k, rows], M)."""
    z = np.asarray(z, dtype=F32)
    rows = z.shape[0] - row0 if rows is None else rows
    k = len(seg) - 1
    M = col_sums(z, order, seg)
    zq = z[row0:row0 + rows].astype(F64)
    lab = np.asarray(labels)[row0:row0 + rows]
    t, q = np.zeros((k, rows), F64), np.zeros(rows, F64)
    with np.errstate(all="ignore"):
        for col in range(z.shape[1]):
            t = t + zq[None, :, col] * M[:, col, None]
            q = q + zq[:, col] * zq[:, col]
        own = lab[None, :] == np.arange(k)[:, None]
        u = np.where(own, t - q[None, :], t)
        S = (np.diff(seg)[:, None] - own).astype(F64) - u
    return S, M


def finish(S, labels, seg, row0=0):
    """vf_silhouette_finish for the rows [row0, row0 + S.shape[1]): (a, b, s fp64, nearest int32), each [rows]."""
    k, rows = S.shape
    n = np.diff(np.asarray(seg)).astype(np.int64)
    lab = np.asarray(labels)[row0:row0 + rows].astype(np.int64)
    labelled = (lab >= 0) & (lab < k)
    best, nearest = np.full(rows, np.nan, F64), np.full(rows, -1, np.int32)
    with np.errstate(all="ignore"):
        for c in range(k):
            if n[c] <= 0:
                continue
            mean = S[c] / F64(n[c])
            take = (lab != c) & ~np.isnan(mean) & ((nearest < 0) | (mean < best))
            best[take], nearest[take] = mean[take], c
        safe = np.where(labelled, lab, 0)
        own, nl = S[safe, np.arange(rows)], n[safe]
        a = np.where(nl > 1, own / np.maximum(nl - 1, 1).astype(F64), 0.0)
        a[~labelled] = np.nan
        m = np.where(a < best, best, a)
        s = np.where(m == 0.0, 0.0, (best - a) / m)
        s[nl <= 1] = 0.0
        s[np.isnan(a) | (nearest < 0)] = np.nan
    return a, best, s, nearest


class Restated(NamedTuple):
    S: np.ndarray
    a: np.ndarray
    b: np.ndarray
    s: np.ndarray
    nearest: np.ndarray


def restate(rows, labels, k, family="l2") -> Restated:
    """The whole chain on the rows as they are given (standardised already for family "dot") and integer labels."""
    order, seg = csr(labels, k)
    S = sums_l2(rows, order, seg) if family == "l2" else sums_dot(rows, order, seg, labels)[0]
    return Restated(S, *finish(S, labels, seg))


def score_of(s, labels, k) -> float:
    lab = np.asarray(labels)
    keep = (lab >= 0) & (lab < k)
    return math.fsum(np.asarray(s)[keep].tolist()) / int(keep.sum())


# ---- the definition, one pair at a time (the exhaustive tiny cases) -----------------------------------------------------------------------
def brute(D, labels, k):
    """scikit-learn's definition from a distance matrix in Python floats: lists a, b, s, nearest."""
    R = len(labels)
    out = []
    for i in range(R):
        means = {}
        for c in range(k):
            members = [j for j in range(R) if labels[j] == c and j != i]
            if members and c != labels[i]:
                means[c] = math.fsum(D[i][j] for j in members) / len(members)
        near = min(means, key=lambda c: (means[c], c)) if means else -1
        b = means[near] if means else math.nan
        if not 0 <= labels[i] < k:
            out.append((math.nan, b, math.nan, near))
            continue
        own = [j for j in range(R) if labels[j] == labels[i] and j != i]
        a = math.fsum(D[i][j] for j in own) / len(own) if own else 0.0
        if not means:
            s = math.nan
        elif not own or max(a, b) == 0:
            s = 0.0
        else:
            s = (b - a) / max(a, b)
        out.append((a, b, s, near))
    return out


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
class Fixture(NamedTuple):
    name: str
    family: str                   # "l2" | "dot"
    metric: str                   # what scikit-learn is asked for
    make: object                  # () -> (rows fp32 [R, d] as the entries see them, labels int [R] with -1 for no label, k,
                                  #        the fp32 rows whose fp64 copy scikit-learn sees: before standardisation for "dot")


def _true(R, g):
    return (np.arange(R) % g).astype(np.int32)


def _e2():
    x = K.blobs(300, 2, 5, 1.2, 7, scale=4.0)
    return x, _true(300, 5), 5, x


def _e33():
    x = K.blobs(257, 33, 6, 1.0, 2, normalise=True)
    return x, _true(257, 6), 6, x


def _e7_poor():                                                            # a partition that ignores the blobs: small, mixed-sign s
    rng = np.random.default_rng(12)
    x = K.blobs(200, 7, 4, 0.7, 5)
    return x, rng.integers(0, 9, 200).astype(np.int32), 9, x


def _e3_gaps():                                                            # unlabelled rows, an empty cluster id, a singleton
    x = K.blobs(150, 3, 4, 0.9, 9, scale=3.0)
    lab = _true(150, 4)
    lab[lab == 2] = 5                                                      # ids 2, 3 -> 5, 3: ids 2 and 4 are empty
    lab[::17] = -1
    lab[7] = 6                                                             # alone in its cluster
    return x, lab, 7, x


def standardize32(x, center=True):
    """The two passes of vf_rows_standardize in fp32 numpy: the mean, t = x - mean, the norm of t, t / norm.  Its sums are numpy's,
    not the device's, so it is no bit-for-bit restatement of that entry: it carries the same kind of error into the rows."""
    x = np.asarray(x, dtype=F32)
    t = x - x.sum(axis=1, dtype=F32, keepdims=True) / F32(x.shape[1]) if center else x
    n = np.sqrt((t * t).sum(axis=1, dtype=F32, keepdims=True))
    return np.ascontiguousarray(t / np.where(n == 0, F32(1.0), n), dtype=F32)


def _corr49():
    x = K.blobs(300, 49, 5, 0.6, 8)
    return standardize32(x), _true(300, 5), 5, x


def _cos12():
    x = K.blobs(220, 12, 4, 0.8, 3)
    return standardize32(x, center=False), _true(220, 4), 4, x


def _corr5_poor():
    rng = np.random.default_rng(4)
    x = K.blobs(180, 5, 3, 1.0, 6)
    return standardize32(x), rng.integers(0, 6, 180).astype(np.int32), 6, x


FIXTURES = [Fixture("E-2", "l2", "euclidean", _e2), Fixture("E-33", "l2", "euclidean", _e33), Fixture("E-7-poor", "l2", "euclidean", _e7_poor),
            Fixture("E-3-gaps", "l2", "euclidean", _e3_gaps), Fixture("D-corr-49", "dot", "correlation", _corr49),
            Fixture("D-cos-12", "dot", "cosine", _cos12), Fixture("D-corr-5-poor", "dot", "correlation", _corr5_poor)]


def fixture(name: str) -> Fixture:
    return next(f for f in FIXTURES if f.name == name)


def sklearn_reference(f: Fixture):
    """(s, nearest) of scikit-learn on the fp64 copy of the fixture's labelled rows, scattered back to all rows (NaN, -1 for a row
    without a label); nearest by its definition from sklearn's own pairwise distances."""
    from sklearn.metrics import pairwise_distances, silhouette_samples
    _, lab, k, ref = f.make()
    keep = np.nonzero(lab >= 0)[0]
    x64, l = ref[keep].astype(F64), lab[keep]
    s = np.full(len(lab), np.nan)
    s[keep] = silhouette_samples(x64, l, metric=f.metric)
    D = pairwise_distances(x64, metric=f.metric)
    means = np.full((k, len(keep)), np.inf)
    for c in range(k):
        if (l == c).any():
            means[c] = D[:, l == c].mean(axis=1)
    means[l, np.arange(len(keep))] = np.inf
    nearest = np.full(len(lab), -1, np.int32)
    nearest[keep] = np.argmin(means, axis=0)
    two = np.sort(means, axis=0)[:2]
    gap = np.full(len(lab), np.inf)
    gap[keep] = (two[1] - two[0]) / two[1]
    return s, nearest, gap


# ---- device cases ----------------------------------------------------------------------------------------------------------------------
def device_case(R, d, k, seed, nonfinite=False):
    """(x fp32 [R, d], labels int32 [R]): one cluster larger than a staged tile where R allows, a singleton, an empty id, rows
    without a label (-1 and k), and optionally NaN and Inf rows."""
    rng = np.random.default_rng(seed)
    cen = (rng.standard_normal((k, d)) * 3.0).astype(F32)
    lab = rng.integers(0, k, R).astype(np.int32)
    x = (cen[lab] + rng.standard_normal((R, d))).astype(F32)
    if R >= 100:
        lab[: R // 2] = 0                                                  # more than RANGES * JT = 32 members: several staged tiles
    if R >= 8:
        if k >= 3:
            lab[lab == k - 1] = 0                                          # id k - 1 is empty
        if k >= 4:
            lab[lab == 1] = 0
            lab[3] = 1                                                     # a singleton
        lab[5], lab[6] = -1, k                                             # no label
    if nonfinite and R >= 8:
        x[2, 0] = np.nan
        x[4, d - 1] = np.inf
        x[R - 1] = -np.inf
    return x, lab


def sweep_blobs():
    """5 well-separated clusters, 300 x 7."""
    return K.blobs(300, 7, 5, 0.35, 21, scale=3.0)

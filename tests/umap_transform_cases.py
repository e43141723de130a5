"""References and the case table of the UMAP transform (include/vf_hip_umap_transform.h, manifold.UMAPModel.transform).

The references are numpy restatements with the header's operation order: `smooth_knn_query` is vf_umap_smooth_knn_query in fp64,
`init_transform` is vf_umap_init_transform in fp32, operation for operation (the entry calls no library function, so it is held
to equality), `samples` is manifold.transform_samples, `layout_transform` is vf_umap_layout_transform in fp64, vectorised across
the queries and looping over epochs and entries, and `transform` is the whole of UMAPModel.transform.  The due rule, the hash
and the curve are tests/umap_cases.py's, which restate include/vf_hip_umap.h.  Integers and selections are compared for
equality; what depends on the device's exp and pow is held within bounds that were measured once on an MI355X
(python -m pytest tests/test_umap_transform_gpu.py -s prints every figure before it asserts) and are asserted at 8 times the
measurement, the margin for ulp differences in exp / pow and a bisection that may stop one iteration apart:

  sigma, relative to the fp64 restatement's, over the smooth table            measured 8.01e-4 (SIGMA): typically 4e-6; the
      largest is a row of few present entries, whose sum is flat in sigma, so that the tolerance of 1e-5 on the sum is a wide
      interval of sigma: the bound is the tolerance's, not the arithmetic's.  A row that converges while the search is still
      open-ended is held to the nearest of sigma / 2, sigma and 2 sigma (`sigma_deviation`; measured: m = 2 with one present
      entry stops one doubling apart in two of the table's cases);
  strength, absolute                                                          measured 1.08e-5 (STRENGTH): the tolerance again;
  one epoch of the layout at learning_rate 1 (the entry runs it at 1/4), absolute, positions in [0, 10]
                                                                              measured 1.5e-3  (LAYOUT_1): 1e-8 .. 1.3e-4 in every
      case but R = 3, where thirty entries draw a query to the same three points and each draw repels it from them five times:
      at short range a repulsion changes y by alpha g (y - q) with g up to 1790, an expansion of up to 45 per move at alpha =
      0.025, so that fp32's 1e-7 grows to 1e-3 within one epoch;
  ten epochs at learning_rate 1/16 (LAYOUT_10_LR; why not 1: tests/umap_cases.py), absolute   measured 1.47e-3 (LAYOUT_10): the
      same case; 2e-6 .. 1.7e-4 in the others;
  the blob case's 100 epochs, device against the restatement on the device's neighbour lists, absolute   measured 3.1e-4  (WHOLE).
The integers do not rest on these bounds: test_the_due_sets_and_the_negative_vertices_are_the_restatements runs a case whose
positions spell them, with a bound from reasoning that is stated there.
"""
from __future__ import annotations

import numpy as np

from tests import umap_cases as U

F32, F64 = np.float32, np.float64

MAX_M = 64
EPOCHS_PER_LAUNCH = 8

SIGMA_MEASURED = 8.01e-4
STRENGTH_MEASURED = 1.08e-5
LAYOUT_1_MEASURED = 1.5e-3
LAYOUT_10_MEASURED = 1.47e-3
WHOLE_MEASURED = 3.1e-4
LAYOUT_10_LR = 1.0 / 16.0
SIGMA_RTOL, STRENGTH_ATOL = 8 * SIGMA_MEASURED, 8 * STRENGTH_MEASURED
LAYOUT_1_ATOL, LAYOUT_10_ATOL, WHOLE_ATOL = 8 * LAYOUT_1_MEASURED, 8 * LAYOUT_10_MEASURED, 8 * WHOLE_MEASURED
TRUST_MARGIN = 0.01                        # the spread the fit's commit observed between device and restatement (0.9522 / 0.9532)

RQS = (1, 2, 63, 64, 65, 257)
SMOOTH_MS = (1, 2, 15, 30, 63, 64)
AB = (1.5769436135065809, 0.895060719357739)                          # find_ab(0.1)


# ---- step 2: sigma and the strengths -----------------------------------------------------------------------------------------------
def smooth_knn_query(idx: np.ndarray, dist: np.ndarray, mean_dist: float):
    """(sigma fp64 [Rq], strength fp64 [Rq, m], converged bool [Rq], floored bool [Rq], open_ended bool [Rq]): rho = 0, target
    log2(m), the floor from mean_dist alone, no entry zeroed for naming the row's own number.  open_ended: the row converged
    while hi was still infinite or lo still 0, where a step doubles or halves mid (a row with as many present entries as
    log2(m), or m = 1): there a stop one iteration apart is a factor of two in sigma."""
    Rq, m = idx.shape
    p = U.present(idx, dist)
    x = np.where(p, np.where(p, dist, 0).astype(F64), 0.0)
    target = float(F32(np.log2(float(m))))
    lo, hi, mid = np.zeros(Rq), np.full(Rq, np.inf), np.ones(Rq)
    active = np.ones(Rq, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for _ in range(U.SMOOTH_ITERS):
            s = np.where(p, np.where(x > 0, np.exp(-(x / mid[:, None])), 1.0), 0.0).sum(1)
            active &= ~(np.abs(s - target) < U.SMOOTH_TOL)
            up, down = active & (s > target), active & ~(s > target)
            hi = np.where(up, mid, hi)
            lo = np.where(down, mid, lo)
            mid = np.where(up, (lo + hi) / 2, np.where(down, np.where(np.isinf(hi), mid * 2, (lo + hi) / 2), mid))
        count = p.sum(1)
        floor = float(F32(U.MIN_SCALE)) * float(F32(mean_dist))
        floored = (mid < floor) & (count > 0)
        sigma = np.where(count > 0, np.where(mid < floor, floor, mid), 0.0)
        strength = np.where(p, np.where((x <= 0) | (sigma[:, None] == 0), 1.0, np.exp(-(x / sigma[:, None]))), 0.0)
    return sigma, strength, ~active & (count > 0), floored, ~active & (count > 0) & (np.isinf(hi) | (lo == 0))


def sigma_deviation(sigma, sigma_ref, open_ended):
    """Relative deviation of sigma from the restatement's, per row; in an open-ended row from the nearest of sigma_ref / 2,
    sigma_ref and 2 sigma_ref: the two bisections may stop one iteration apart, and there an iteration is a factor of two."""
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(sigma - sigma_ref) / sigma_ref
        for f in (0.5, 2.0):
            rel = np.where(open_ended, np.minimum(rel, np.abs(sigma - f * sigma_ref) / (f * sigma_ref)), rel)
    return rel


SMOOTH_KINDS = ("random", "zeros", "negatives", "ties", "absent-tails", "absent-row", "nonfinite", "own-row", "wide", "tight")


def smooth_case(kind: str, Rq: int, m: int):
    """(idx, dist) of one case: lists of training rows (of 1000), ascending distances; what the kind is about is in row 0 and on."""
    g = np.random.default_rng(7000 * Rq + 13 * m + SMOOTH_KINDS.index(kind))
    idx = g.integers(0, 1000, (Rq, m)).astype(np.int32)
    dist = np.sort(g.uniform(0.05, 1.5, (Rq, m)).astype(F32), axis=1)
    if kind == "zeros":                                                # every other row all zero: every strength 1, the floor binds
        dist[::2] = 0
    elif kind == "negatives":                                          # 1 - s with s a little above 1
        dist[:, : max(1, m // 3)] = -g.uniform(0, 3e-7, (Rq, max(1, m // 3))).astype(F32)
        dist[0, 0] = F32(-0.0)
    elif kind == "ties":
        dist = (np.ceil(dist * 4) / 4).astype(F32)
    elif kind == "absent-tails":
        for i in range(Rq):
            cut = int(g.integers(0, m + 1))
            idx[i, cut:], dist[i, cut:] = -1, np.inf
    elif kind == "absent-row":
        idx[::3], dist[::3] = -1, np.inf
    elif kind == "nonfinite":                                          # mid-row: the entries behind them still count
        for i in range(Rq):
            t = int(g.integers(0, m))
            dist[i, t] = (np.nan, np.inf, -np.inf)[i % 3]
            if m > 2:
                idx[i, (t + 1) % m] = -1                               # a negative index beside a finite distance
    elif kind == "own-row":                                            # the row's own number names a training row: not zeroed
        idx[:, 0] = np.arange(Rq)
        dist[:, 0] = np.maximum(dist[:, 0], F32(0.05))
    elif kind == "wide":
        dist = (dist * F32(1e6)).astype(F32)
    elif kind == "tight":                                              # sigma would be ~1e-7 of the distances: the floor binds
        dist = (F32(1) + dist * F32(1e-6)).astype(F32)
    return idx, dist


# ---- step 3: the start ---------------------------------------------------------------------------------------------------------------
def init_transform(idx: np.ndarray, strength: np.ndarray, Y: np.ndarray) -> np.ndarray:
    """fp32 [Rq, dim], operation for operation in fp32: S ascending over the usable entries, one rounded quotient per entry, one
    rounded product per coordinate, the sum ascending from +0; NaN where S == 0."""
    Rq, m = idx.shape
    R, dim = Y.shape
    Y = np.asarray(Y, dtype=F32)
    w = np.asarray(strength, dtype=F32)
    usable = (idx >= 0) & (idx < R)
    S = np.zeros(Rq, dtype=F32)
    for t in range(m):
        S = np.where(usable[:, t], (S + w[:, t]).astype(F32), S)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = (w / S[:, None]).astype(F32)
        out = np.zeros((Rq, dim), dtype=F32)
        for t in range(m):
            rows = Y[np.where(usable[:, t], idx[:, t], 0)] if R else np.zeros((Rq, dim), dtype=F32)
            prod = (q[:, t, None] * rows).astype(F32)
            out = np.where(usable[:, t, None], (out + prod).astype(F32), out)
    out[S == 0] = np.nan
    return out


# ---- step 4: the draw counts -----------------------------------------------------------------------------------------------------------
def samples(strength: np.ndarray, N: int) -> np.ndarray:
    """manifold.transform_samples: floor(fl(fl(strength / rowmax) * N)) in individually rounded fp32, int32; 0 where rowmax is 0."""
    w = np.asarray(strength, dtype=F32)
    if w.size == 0:
        return np.zeros(w.shape, dtype=np.int32)
    rowmax = w.max(1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(rowmax > 0, w / rowmax, F32(0)).astype(F32)
    return np.clip(np.floor(ratio * F32(N)), 0, N).astype(np.int32)


# ---- step 5: the layout ----------------------------------------------------------------------------------------------------------------
def layout_transform(idx, cnt, Y, Yq, epoch_begin: int, epoch_end: int, N: int, a, b, gamma=1.0, learning_rate=1.0, rate: int = 5,
                     seed: int = 42, first_row: int = 0, trace: list | None = None):
    """fp64 [Rq, dim] after the epochs [epoch_begin, epoch_end) from Yq, in the header's order; Y stands still.  a, b, gamma and
    learning_rate / 4 are rounded to fp32 first and alpha is formed in fp32, as the entry receives and forms them.  trace, if a
    list, receives (n, s, rows due, their negative vertices [rows, rate]) for every (epoch, entry) with something due."""
    a, b, gamma = float(F32(a)), float(F32(b)), float(F32(gamma))
    lr4 = F32(learning_rate) / F32(4)
    Y, y = np.asarray(Y, dtype=F64), np.array(Yq, dtype=F64)
    R, (Rq, m) = Y.shape[0], idx.shape
    number = (first_row + np.arange(Rq, dtype=np.int64)).astype(np.uint64)
    for n in range(epoch_begin, epoch_end):
        alpha = float(lr4 * (F32(1) - F32(n) / F32(N)))
        for s in range(m):
            j = idx[:, s].astype(np.int64)
            rows = np.flatnonzero(U.due(cnt[:, s], n, N) & (j >= 0) & (j < R))
            if rows.size == 0:
                continue
            U._attract(y, rows, Y[j[rows]], a, b, alpha)
            ks = np.zeros((rows.size, rate), dtype=np.int64)
            for p in range(rate):
                k = ks[:, p] = U.negative_vertex(seed, n, number[rows], s, p, R)
                diff = y[rows] - Y[k]
                d2 = (diff * diff).sum(1)
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    g = ((2.0 * gamma) * b) / ((0.001 + d2) * (a * np.power(d2, b) + 1.0))
                    move = alpha * U._clip(g[:, None] * diff)
                y[rows] += np.where((d2 == 0)[:, None], 0.0, move)
            if trace is not None:
                trace.append((n, s, rows, ks))
    return y


def layout_case(Rq: int, R: int, dim: int, m: int, N: int, special: bool = True):
    """(idx int32 [Rq, m], cnt int32 [Rq, m], Y fp32 [R, dim], Yq fp32 [Rq, dim]): random lists with, where the shape allows,
    indices -1 and R, counts 0, N, N + 1 and -1, a query standing exactly on its first neighbour and a NaN query."""
    g = np.random.default_rng(100000 * Rq + 1000 * R + 100 * dim + m + N)
    idx = g.integers(0, R, (Rq, m)).astype(np.int32)
    cnt = g.integers(0, N + 1, (Rq, m)).astype(np.int32)
    Y = U.rescale(U.random_init(R, dim, 100 + R)) if R > 1 else np.full((1, dim), 2.5, dtype=F32)
    Yq = (10.0 * U.random_init(Rq, dim, 900 + Rq)).astype(F32)
    if special:
        flat_i, flat_c = idx.reshape(-1), cnt.reshape(-1)
        for pos, value in zip(g.permutation(flat_i.size)[:4], (-1, R, -1, R)):
            if flat_i.size >= 8:
                flat_i[pos] = value
        for pos, value in zip(g.permutation(flat_c.size)[:8], (0, N, N + 1, -1, 0, N, N + 1, -1)):
            flat_c[pos] = value
        cnt[0, 0] = N                                                  # something is due in every epoch
        idx[0, 0] = min(R - 1, 1)
        if Rq >= 63:
            idx[5, 0], cnt[5, 0] = 0, N
            Yq[5] = Y[0]                                               # d2 == 0 against its neighbour in epoch 0
            Yq[9] = np.nan
    return idx, cnt, Y, Yq


# ---- the whole, in numpy ---------------------------------------------------------------------------------------------------------------
def standardise(x: np.ndarray) -> np.ndarray:
    x = np.nan_to_num(np.asarray(x, dtype=F64), nan=0.0)
    t = x - x.mean(1, keepdims=True)
    nrm = np.sqrt((t * t).sum(1, keepdims=True))
    return np.divide(t, nrm, out=np.zeros_like(t), where=nrm > 0)


def knn_queries(x: np.ndarray, q: np.ndarray, k: int):
    """(idx int32 [Rq, k], dist fp32 [Rq, k]): the k training rows nearest to each query by correlation distance formed in fp64."""
    D = 1.0 - standardise(q) @ standardise(x).T
    order = np.argsort(D, axis=1, kind="stable")[:, :k]
    return order.astype(np.int32), np.take_along_axis(D, order, 1).astype(F32)


def transform(x, Y, q, n_neighbors: int, mean_dist: float, N: int, a, b, gamma=1.0, learning_rate=1.0, rate: int = 5, seed: int = 42,
              first_row: int = 0, lists=None):
    """(fp64 [Rq, dim], the fp32 start): UMAPModel.transform stage by stage in numpy; lists = (idx, dist) replaces the fp64 search."""
    idx, dist = knn_queries(x, q, n_neighbors) if lists is None else lists
    strength = smooth_knn_query(idx, dist, mean_dist)[1].astype(F32)
    y0 = init_transform(idx, strength, Y)
    return layout_transform(idx, samples(strength, N), Y, y0, 0, N, N, a, b, gamma, learning_rate, rate, seed, first_row), y0


BLOBS = dict(R=300, Rq=60, d=16, n_neighbors=15, n_epochs=100, min_dist=0.1)
CENTRES = np.array([[0.0, 0.0], [10.0, 0.0], [0.0, 10.0]])


def blobs():
    """(x fp32 [300, 16], labels, Y fp32 [300, 2], q fp32 [60, 16], query labels): three Gaussian blobs, a constructed embedding
    with the blobs at (0, 0), (10, 0), (0, 10) plus 0.7 noise, and 60 held-out rows."""
    g = np.random.default_rng(20261021)
    centres = 4.0 * g.standard_normal((3, BLOBS["d"]))
    lx, lq = np.arange(BLOBS["R"]) % 3, np.arange(BLOBS["Rq"]) % 3
    x = (centres[lx] + g.standard_normal((BLOBS["R"], BLOBS["d"]))).astype(F32)
    q = (centres[lq] + g.standard_normal((BLOBS["Rq"], BLOBS["d"]))).astype(F32)
    Y = (CENTRES[lx] + 0.7 * g.standard_normal((BLOBS["R"], 2))).astype(F32)
    return x, lx, Y, q, lq


def blobs_state(x, Y, mean_dist: float) -> dict:
    a, b = AB
    return dict(embedding=Y, x=x, n_neighbors=BLOBS["n_neighbors"], metric="correlation", a=a, b=b, n_epochs=500, seed=42,
                negative_sample_rate=5, repulsion_strength=1.0, learning_rate=1.0, mean_dist=mean_dist)


_BLOBS_REFERENCE = {}


def blobs_reference():
    """(positions fp64 [60, 2], start fp32 [60, 2], mean_dist) of the restatement on the blobs, computed once and shared; callers
    do not write to it.  mean_dist is that of the training rows' own 14-neighbour graph, as a fit would have kept it."""
    if not _BLOBS_REFERENCE:
        x, _, Y, q, _ = blobs()
        mean_dist = U.mean_distance(*U.knn(x, BLOBS["n_neighbors"] - 1))
        y, y0 = transform(x, Y, q, BLOBS["n_neighbors"], mean_dist, BLOBS["n_epochs"], *AB)
        y.setflags(write=False)
        _BLOBS_REFERENCE.update(y=y, y0=y0, mean_dist=mean_dist)
    return _BLOBS_REFERENCE["y"], _BLOBS_REFERENCE["y0"], _BLOBS_REFERENCE["mean_dist"]


def nearest_training_label(Y: np.ndarray, labels: np.ndarray, y: np.ndarray) -> np.ndarray:
    d = ((np.asarray(y, dtype=F64)[:, None, :] - np.asarray(Y, dtype=F64)[None, :, :]) ** 2).sum(2)
    return labels[d.argmin(1)]


def trust(x, q, Y, y) -> float:
    """scikit-learn's trustworthiness of [Y; y] against [x; q], cosine on standardised rows (= correlation), 15 neighbours."""
    from sklearn.manifold import trustworthiness
    z = standardise(np.concatenate((x, q)))
    return float(trustworthiness(z, np.concatenate((np.asarray(Y, dtype=F64), np.asarray(y, dtype=F64))), n_neighbors=BLOBS["n_neighbors"], metric="cosine"))

"""References and the case table of UMAP after the k-NN graph (include/vf_hip_umap.h, variantformer_amd/manifold.py).

The references are fp64 numpy restatements of the three stages with the header's operation order: `smooth_knn` is
vf_umap_smooth_knn, `csr` is manifold.py's graph plumbing, `union` is vf_umap_union, `layout` is vf_umap_layout -- vectorised
across vertices, looping over the position within the row, since a vertex walks its entries in order.  Everything that is an
integer or a selection is restated exactly and compared for equality: rho, the CSR arrays, the sample counts, the due rule
(`due`), the hash (`mix32`, `negative_vertex`), the random initialisation.  Everything else is held within bounds that were
measured once and are asserted at 8 times the measurement (exp and pow are library functions on the device, so the last bits
are the library's, not the algorithm's):

  find_ab against scipy.optimize.curve_fit at min_dist 0.001, 0.05, 0.1, 0.5, 0.99, on the host (python -m pytest
      tests/test_umap_cpu.py -s -k find_ab prints it): |a - a'| / a and |b - b'| / b   measured 2.4e-6  (AB): scipy stops at
      its own tolerance of 1e-8 on the cost, the iteration here at a step of 1e-14, and its cost is never the higher one;
  on an MI355X (python -m pytest tests/test_umap_gpu.py -s prints every figure before it asserts):
  sigma, relative to the fp64 reference's, over the smooth_knn table    measured 5.4e-5  (SIGMA): the bisection stops at
      |sum - log2(m + 1)| < 1e-5, and fp32 and fp64 may stop one step apart: the bound is the tolerance's, not the arithmetic's;
  strength, absolute                                                    measured 1.7e-5  (STRENGTH): sigma's deviation carried
      through exp(-(d - rho) / sigma);
  the residual |sum_t exp(-max(0, d_t - rho) / sigma) - log2(m + 1)| in fp64 at the device's sigma, over the rows whose
      bisection converged and whose floor does not bind                 measured 1.01e-5 (RESIDUAL);
  w of the union, absolute, from the same fp32 strengths                measured 8.5e-8  (UNION): three fp32 roundings;
  one epoch of the layout at learning_rate 1, absolute, positions in [0, 10]   measured 2.5e-4  (LAYOUT_1): an fp32 position
      near 10 has an ulp of 9.5e-7 and a vertex makes some 70 moves per epoch, which is a floor of a few 1e-5; the rest is the
      map's own expansion: a repulsion changes y by alpha g (y - q) with g up to 1790 at short range;
  ten epochs at learning_rate 1/16 (LAYOUT_10_LR), absolute             measured 1.5e-4  (LAYOUT_10): its own bound, because
      the map is expansive.  At learning_rate 1 from a random start it is chaotic in few dimensions: the fp32 and fp64
      trajectories of the table's cases part completely within ten epochs (measured 6.0 at dim 1, 2.4 and 4.0 at dim 2, 0.98 at
      dim 3, against 1.5e-5 at dim 8), so a bound there would let any output pass; at 1/4 the figures are 1e-5 .. 4e-3, at 1/16
      and 1/64 below 1.5e-4 in every case while the vertices still move by 1 to 2 units.  The ten-epoch comparison therefore
      runs at 1/16; bit-equality of two runs and of a split run is asserted at learning_rate 1, where nothing is lost to it.
  the spread (max - min) of the reference's trustworthiness on the blobs case over the seeds 42, 43, 44, 45, 46, on the host
      (python -m tests.umap_cases prints it: 0.9532, 0.9504, 0.9465, 0.9507, 0.9489; the random initialisation has 0.5101)
                                                                        measured 0.0067  (TRUST_MARGIN).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

F32, F64 = np.float32, np.float64
U64 = np.uint64
MASK = U64(0xFFFFFFFF)

AB_MEASURED = 2.4e-6
SIGMA_MEASURED = 5.4e-5
STRENGTH_MEASURED = 1.7e-5
RESIDUAL_MEASURED = 1.01e-5
UNION_MEASURED = 8.5e-8
LAYOUT_1_MEASURED = 2.5e-4
LAYOUT_10_MEASURED = 1.5e-4
LAYOUT_10_LR = 1.0 / 16.0
TRUST_MARGIN = 0.0067
AB_RTOL, SIGMA_RTOL, STRENGTH_ATOL, RESIDUAL_ATOL = 8 * AB_MEASURED, 8 * SIGMA_MEASURED, 8 * STRENGTH_MEASURED, 8 * RESIDUAL_MEASURED
UNION_ATOL, LAYOUT_1_ATOL, LAYOUT_10_ATOL = 8 * UNION_MEASURED, 8 * LAYOUT_1_MEASURED, 8 * LAYOUT_10_MEASURED

RS = (1, 63, 64, 65, 257)
MS = (1, 2, 29, 63)
SMOOTH_ITERS, SMOOTH_TOL, MIN_SCALE = 64, 1e-5, 1e-3


# ---- integers: the hash, the negative vertex, the due rule, the random initialisation ----------------------------------------------
def mix32(x):
    """The header's mixer on uint64 arrays (or ints) that hold uint32 values."""
    x = np.asarray(x, dtype=U64)
    x = x ^ (x >> U64(16))
    x = (x * U64(0x7FEB352D)) & MASK
    x = x ^ (x >> U64(15))
    x = (x * U64(0x846CA68B)) & MASK
    return x ^ (x >> U64(16))


def negative_vertex(seed: int, n: int, i, s, p: int, R: int):
    """k = (uint64(h) * R) >> 32 with h = mix(mix(mix(mix(mix(seed + 0x9E3779B9) ^ n) ^ i) ^ s) ^ p): int64 array like i."""
    h = mix32((int(seed) + 0x9E3779B9) & 0xFFFFFFFF)
    h = mix32(h ^ U64(n))
    h = mix32(h ^ np.asarray(i, dtype=U64))
    h = mix32(h ^ np.asarray(s, dtype=U64))
    h = mix32(h ^ U64(p))
    return ((h * U64(R)) >> U64(32)).astype(np.int64)


def due(samples, n: int, N: int):
    """bool like samples: floor((n + 1) s / N) > floor(n s / N) in 64-bit integers; never for an s outside 1 .. N."""
    s = np.asarray(samples, dtype=np.int64)
    ok = (s >= 1) & (s <= N)
    s = np.where(ok, s, 0)
    return ok & (((n + 1) * s) // N > (n * s) // N)


def random_init(rows: int, dim: int, seed: int) -> np.ndarray:
    """manifold.random_init: fp32 [rows, dim] in [0, 1)."""
    s = mix32((int(seed) + 0x85EBCA6B) & 0xFFFFFFFF)
    hi = mix32(s ^ np.arange(rows, dtype=U64))[:, None]
    h = mix32(hi ^ np.arange(dim, dtype=U64)[None, :])
    return ((h >> U64(8)).astype(F64) / float(1 << 24)).astype(F32)


def rescale(y: np.ndarray) -> np.ndarray:
    """manifold.rescale in fp32 numpy, operation for operation."""
    y = np.asarray(y, dtype=F32)
    lo, hi = y.min(0, keepdims=True), y.max(0, keepdims=True)
    span = hi - lo
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(span > 0, F32(10.0) * (y - lo) / np.where(span > 0, span, F32(1)), F32(0)).astype(F32)


# ---- stage 1: rho, sigma, strengths ------------------------------------------------------------------------------------------------
def present(idx: np.ndarray, dist: np.ndarray) -> np.ndarray:
    return (idx >= 0) & np.isfinite(dist)


def mean_distance(idx, dist) -> float:
    p = present(idx, dist)
    return float(dist[p].astype(F64).mean()) if p.any() else 0.0


def smooth_knn(idx: np.ndarray, dist: np.ndarray, mean_dist: float):
    """(rho fp32 [R] -- a selection, exact --, sigma fp64 [R], strength fp64 [R, m], converged bool [R], floored bool [R])."""
    R, m = idx.shape
    p = present(idx, dist)
    positive = p & (dist > 0)
    rho32 = np.where(positive.any(1), np.where(positive, dist, np.inf).min(1), 0).astype(F32)
    x = np.where(p, np.where(p, dist, 0).astype(F64) - rho32.astype(F64)[:, None], 0.0)
    target = np.log2(m + 1.0)
    lo, hi, mid = np.zeros(R), np.full(R, np.inf), np.ones(R)
    active = np.ones(R, dtype=bool)

    def total(scale):
        with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
            return np.where(p, np.where(x > 0, np.exp(-(x / scale[:, None])), 1.0), 0.0).sum(1)
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(SMOOTH_ITERS):
            s = total(mid)
            active &= ~(np.abs(s - target) < SMOOTH_TOL)
            up, down = active & (s > target), active & ~(s > target)
            hi = np.where(up, mid, hi)
            lo = np.where(down, mid, lo)
            mid = np.where(up, (lo + hi) / 2, np.where(down, np.where(np.isinf(hi), mid * 2, (lo + hi) / 2), mid))
    count = p.sum(1)
    row_mean = np.where(p, dist, 0).astype(F64).sum(1) / np.maximum(count, 1)
    floor = MIN_SCALE * np.where(rho32 > 0, row_mean, float(F32(mean_dist)))
    floored = (mid < floor) & (count > 0)
    sigma = np.where(count > 0, np.where(mid < floor, floor, mid), 0.0)
    own = idx == np.arange(R)[:, None]
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        strength = np.where(p & ~own, np.where((x <= 0) | (sigma[:, None] == 0), 1.0, np.exp(-(x / sigma[:, None]))), 0.0)
    return rho32, sigma, strength, ~active & (count > 0), floored


def smooth_residual(idx, dist, rho32, sigma) -> np.ndarray:
    """fp64 [R]: |sum_t exp(-max(0, d_t - rho) / sigma) - log2(m + 1)| at the given sigma."""
    p = present(idx, dist)
    x = np.where(p, np.where(p, dist, 0).astype(F64) - rho32.astype(F64)[:, None], 0.0)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        s = np.where(p, np.where(x > 0, np.exp(-(x / np.asarray(sigma, dtype=F64)[:, None])), 1.0), 0.0).sum(1)
    return np.abs(s - np.log2(idx.shape[1] + 1.0))


# ---- stage 2: the symmetric graph and the union ---------------------------------------------------------------------------------------
def csr(idx: np.ndarray, dist: np.ndarray):
    """(rowptr int64 [R + 1], col int32 [nnz]): {i, j} is an edge if either lists the other (present, i != j); both directions."""
    R, m = idx.shape
    rows = np.broadcast_to(np.arange(R, dtype=np.int64)[:, None], (R, m))
    edge = present(idx, dist) & (idx != rows)
    i, j = rows[edge], idx[edge].astype(np.int64)
    keys = np.unique(np.concatenate((i * R + j, j * R + i)))
    row = keys // R
    rowptr = np.zeros(R + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(row, minlength=R))
    return rowptr, (keys - row * R).astype(np.int32)


def entry_rows(rowptr: np.ndarray) -> np.ndarray:
    return np.repeat(np.arange(rowptr.shape[0] - 1, dtype=np.int64), np.diff(rowptr))


def union(idx: np.ndarray, strength: np.ndarray, rowptr: np.ndarray, col: np.ndarray) -> np.ndarray:
    """w fp64 [nnz] = a + b - a b from the given strengths (the first match of a list counts)."""
    R, m = idx.shape
    S = np.zeros((R, R), dtype=F64)
    for t in range(m - 1, -1, -1):                                     # descending: the first match is written last
        ok = (idx[:, t] >= 0) & (idx[:, t] < R)
        S[np.flatnonzero(ok), idx[ok, t]] = np.asarray(strength, dtype=F64)[ok, t]
    listed = np.zeros((R, R), dtype=bool)
    ok = (idx >= 0) & (idx < R)
    listed[np.broadcast_to(np.arange(R)[:, None], idx.shape)[ok], idx[ok]] = True
    S = np.where(listed, S, 0.0)
    i, j = entry_rows(rowptr), col.astype(np.int64)
    a, b = S[i, j], S[j, i]
    return (a + b) - a * b


def edge_samples(w: np.ndarray, N: int) -> np.ndarray:
    """manifold.edge_samples: floor(fl(fl(w / w_max) * N)) in individually rounded fp32, int32."""
    w = np.asarray(w, dtype=F32)
    if w.size == 0:
        return np.zeros(0, dtype=np.int32)
    w_max = w.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(w_max > 0, w / w_max, F32(0)).astype(F32)
    return np.clip(np.floor(ratio * F32(N)), 0, N).astype(np.int32)


# ---- stage 3: the layout ------------------------------------------------------------------------------------------------------------
def _clip(v):
    return np.where(v > 4.0, 4.0, np.where(v < -4.0, -4.0, v))


def _attract(y, rows, other, a, b, alpha):
    diff = y[rows] - other
    d2 = (diff * diff).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.power(d2, b)
        g = np.where(d2 > 0, ((-2.0 * a * b) * (p / d2)) / (a * p + 1.0), 0.0)
    y[rows] += alpha * _clip(g[:, None] * diff)


def layout(rowptr, col, samples, Y, epoch_begin: int, epoch_end: int, N: int, a, b, gamma=1.0, learning_rate=1.0, rate: int = 5, seed: int = 42):
    """fp64 [R, dim] after the epochs [epoch_begin, epoch_end) from Y, in the header's order.  a, b, gamma, learning_rate are
    rounded to fp32 first and alpha is formed in fp32, as the entry receives and forms them: they are inputs, not results."""
    a, b, gamma = float(F32(a)), float(F32(b)), float(F32(gamma))
    Y = np.array(Y, dtype=F64)
    R = Y.shape[0]
    deg = np.diff(rowptr)
    for n in range(epoch_begin, epoch_end):
        alpha = float(F32(learning_rate) * (F32(1) - F32(n) / F32(N)))
        y = Y.copy()
        for s in range(int(deg.max()) if R else 0):
            rows = np.flatnonzero(deg > s)
            e = rowptr[rows] + s
            j = col[e].astype(np.int64)
            keep = due(samples[e], n, N) & (j >= 0) & (j < R)
            rows, j = rows[keep], j[keep]
            if rows.size == 0:
                continue
            _attract(y, rows, Y[j], a, b, alpha)
            for p in range(rate):
                k = negative_vertex(seed, n, rows, s, p, R)
                diff = y[rows] - Y[k]
                d2 = (diff * diff).sum(1)
                with np.errstate(divide="ignore", invalid="ignore"):
                    g = np.where(d2 > 0, ((2.0 * gamma) * b) / ((0.001 + d2) * (a * np.power(d2, b) + 1.0)), 0.0)
                y[rows] += np.where((d2 > 0)[:, None], alpha * _clip(g[:, None] * diff), 0.0)
            _attract(y, rows, Y[j], a, b, alpha)
        Y = y
    return Y


# ---- the whole, in numpy ------------------------------------------------------------------------------------------------------------
def knn(x: np.ndarray, k: int):
    """(idx int32 [R, k], dist fp32 [R, k]): the k nearest OTHER rows by correlation distance formed in fp64, ties to the lower row."""
    x = np.asarray(x, dtype=F64)
    t = x - x.mean(1, keepdims=True)
    nrm = np.sqrt((t * t).sum(1, keepdims=True))
    z = np.divide(t, nrm, out=np.zeros_like(t), where=nrm > 0)
    D = 1.0 - z @ z.T
    np.fill_diagonal(D, np.inf)
    order = np.argsort(D, axis=1, kind="stable")[:, :k]
    dist = np.take_along_axis(D, order, 1)
    idx = np.where(np.isinf(dist), -1, order).astype(np.int32)
    return idx, dist.astype(F32)


def umap_reference(x, n_neighbors: int, min_dist: float, n_epochs: int, dim: int = 2, seed: int = 42, rate: int = 5):
    """fp64 [R, dim]: manifold.umap(x, init="random") stage by stage in numpy."""
    from variantformer_amd import manifold
    idx, dist = knn(x, n_neighbors - 1)
    _, _, strength, _, _ = smooth_knn(idx, dist, mean_distance(idx, dist))
    rowptr, col = csr(idx, dist)
    w = union(idx, strength.astype(F32), rowptr, col).astype(F32)
    a, b = manifold.find_ab(min_dist)
    y0 = rescale(random_init(x.shape[0], dim, seed))
    return layout(rowptr, col, edge_samples(w, n_epochs), y0, 0, n_epochs, n_epochs, a, b, 1.0, 1.0, rate, seed)


BLOBS = dict(R=400, d=10, n_neighbors=15, min_dist=0.1, n_epochs=100)


def blobs() -> np.ndarray:
    """fp32 [400, 10]: four Gaussian blobs of 100 rows, centres drawn at scale 4, unit noise."""
    g = np.random.default_rng(20261020)
    centres = 4.0 * g.standard_normal((4, BLOBS["d"]))
    return (centres[np.arange(BLOBS["R"]) % 4] + g.standard_normal((BLOBS["R"], BLOBS["d"]))).astype(F32)


def trust(x: np.ndarray, y: np.ndarray) -> float:
    from sklearn.manifold import trustworthiness
    return float(trustworthiness(np.asarray(x, dtype=F64), np.asarray(y, dtype=F64), n_neighbors=BLOBS["n_neighbors"], metric="correlation"))


_BLOBS_REFERENCE = {}


def blobs_reference(seed: int = 42) -> np.ndarray:
    """The reference's embedding of the blobs, computed once per seed and shared; callers do not write to it."""
    if seed not in _BLOBS_REFERENCE:
        y = umap_reference(blobs(), BLOBS["n_neighbors"], BLOBS["min_dist"], BLOBS["n_epochs"], seed=seed)
        y.setflags(write=False)
        _BLOBS_REFERENCE[seed] = y
    return _BLOBS_REFERENCE[seed]


# ---- the case tables ------------------------------------------------------------------------------------------------------------------
SMOOTH_KINDS = ("random", "zeros", "zeros-then-positives", "ties", "absent-tails", "absent-row", "nonfinite", "wide", "tight")


def knn_lists(R: int, m: int, seed: int):
    """Random others-only lists: idx int32 [R, m] without the row itself and without repeats where R allows, dist fp32 ascending."""
    g = np.random.default_rng(seed)
    idx = np.empty((R, m), dtype=np.int32)
    for i in range(R):
        others = np.delete(np.arange(R), i)
        take = g.permutation(others)[:m] if R - 1 >= m else np.concatenate((g.permutation(others), np.full(m - (R - 1), -1)))
        idx[i] = take
    dist = np.sort(g.uniform(0.05, 1.5, (R, m)).astype(F32), axis=1)
    dist[idx < 0] = np.inf
    return idx, dist


def smooth_case(kind: str, R: int, m: int):
    """(idx, dist) of one smooth_knn case; row 0 (and others where R allows) carries what the kind is about."""
    idx, dist = knn_lists(R, m, 1000 * R + m + 17 * SMOOTH_KINDS.index(kind))
    g = np.random.default_rng(R + m)
    live = idx >= 0
    if kind == "zeros":                                                # every other row all zero: rho = 0, the floor is the global mean's
        dist[::2] = np.where(live[::2], F32(0), dist[::2])
    elif kind == "zeros-then-positives":
        dist[:, : max(1, m // 3)] = np.where(live[:, : max(1, m // 3)], F32(0), dist[:, : max(1, m // 3)])
    elif kind == "ties":
        dist[live] = (np.ceil(dist[live] * 4) / 4).astype(F32)
    elif kind == "absent-tails":
        for i in range(R):
            cut = int(g.integers(0, m + 1))
            idx[i, cut:], dist[i, cut:] = -1, np.inf
    elif kind == "absent-row":
        idx[::3], dist[::3] = -1, np.inf
    elif kind == "nonfinite":                                          # mid-row: the entries behind them still count
        for i in range(R):
            t = int(g.integers(0, m))
            dist[i, t] = (np.nan, np.inf, -np.inf)[i % 3]
            if m > 2:
                idx[i, (t + 1) % m] = -1                               # a negative index beside a finite distance
    elif kind == "wide":                                               # hi stays infinite for some twenty doublings
        dist[live] = (dist[live] * F32(1e6)).astype(F32)
    elif kind == "tight":                                              # sigma would be ~1e-7 of the distances: the floor binds
        dist[live] = (F32(1) + dist[live] * F32(1e-6)).astype(F32)
    if kind == "random" and R > 2 and m > 1:
        idx[1, 0] = 1                                                  # a row that lists itself: strength 0, no edge
    return idx, dist


@dataclass(frozen=True)
class LayoutCase:
    name: str
    rowptr: np.ndarray
    col: np.ndarray
    samples: np.ndarray
    Y: np.ndarray                 # fp32 [R, dim]
    N: int
    a: float
    b: float
    rate: int
    seed: int
    isolated: int                 # a vertex without entries, or -1
    idle: int                     # a vertex whose entries are never drawn, or -1


def layout_case(R: int, dim: int, m: int = 5, N: int = 10, rate: int = 5, seed: int = 7) -> LayoutCase:
    idx, dist = knn_lists(R, min(m, 63), 5000 + R + dim)
    isolated = idle = -1
    if R >= 63:
        isolated, idle = 3, 11
        idx[isolated], dist[isolated] = -1, np.inf
        idx[idx == isolated] = -1
    dist[idx < 0] = np.inf
    rowptr, col = csr(idx, dist)
    i, j = entry_rows(rowptr), col.astype(np.int64)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    w = ((mix32(mix32(lo.astype(U64)) ^ hi.astype(U64)) >> U64(8)).astype(F64) / float(1 << 24)).astype(F32)       # symmetric by construction
    w[(i == idle) | (j == idle)] *= F32(1e-3)
    samples = edge_samples(w, N)
    Y = rescale(random_init(R, dim, 100 + R))
    a, b = 1.5769436135065809, 0.895060719357739                     # find_ab(0.1)
    return LayoutCase(f"R{R}-dim{dim}", rowptr, col, samples, Y, N, a, b, rate, seed, isolated, idle)


if __name__ == "__main__":
    x = blobs()
    values = [trust(x, blobs_reference(seed)) for seed in (42, 43, 44, 45, 46)]
    print("trustworthiness of the reference over five seeds:", [f"{v:.4f}" for v in values], f"spread {max(values) - min(values):.4f}")
    print("of the random initialisation (seed 42):", f"{trust(x, rescale(random_init(BLOBS['R'], 2, 42))):.4f}")

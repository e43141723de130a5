"""References, fixtures and the case table of the k-means entries (include/vf_hip_kmeans.h); importable without a GPU.

Two restatements in numpy.  The fp32 one is THE CONTRACT: every operation of the header in the header's order, individually
rounded, so the device must equal it bit for bit -- labels, distance bits, centre bits, counts, changed, shift, n_iter and the
seeded rows.  The fp64 one is the same loop in double precision with centres kept in fp64: the one that is pinned to
scikit-learn 1.7.2's KMeans(algorithm="lloyd") (tests/test_kmeans_cpu.py), and the one the fixture condition is checked on.

Which launch writes each element that is later read (the read-before-write table of variantformer_amd/kmeans.py's allocations;
tests/test_kmeans_nets_gpu.py poisons every one of them):
  seed_rows   rows[0], cen[0, :]   kmeans_take_kernel;           rows[t], cen[t, :]  kmeans_select_kernel of step t
              mind[r]              kmeans_mind_kernel of step 1 (its old value is not read there); read by steps 2 .. and qsum
              work: blockmax       kmeans_mind_kernel;  m  kmeans_max_kernel;  blocksum  kmeans_qsum_kernel (every step, before the select)
  _lloyd      work: stop word, n_iter   kmeans_begin_kernel, before any kernel reads the stop word
              prev[r]              the assignment of iteration 0 (resume = 0: the old value is not read)
              work: block counts   the assignment of every iteration;  shift partials  the update of every iteration
              counts[j], cen       the update (cen holds the start before it);  shift[n], changed[n]  kmeans_finish_kernel, n < n_iter
              labels[r], dist[r]   the last assignment, which always runs
              shift[n_iter:], changed[n_iter:] are never written and never read: kmeans.py returns shift[:n_iter] alone
  _assign     labels, dist         the assignment of every chunk; the chunks tile [0, R)
  kmeans      cen (init array or random rows)  Tensor.copy_ of the whole buffer
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

F32, F64 = np.float32, np.float64
# include/vf_hip_kmeans.h
MAX_K, MAX_R, MAX_D = 4096, 1 << 24, 65536
ROWS, SPLITS, JT, DC, DC_SMALL = 64, 4, 8, 32, 4
GROUP = SPLITS * JT
UPDATE_WAVES, UPDATE_COLS, RED_THREADS = 16, 64, 256
NAN_BITS = 0x7FC00000
_MASK = 0xFFFFFFFF


def lloyd_work_bytes(R, d, k):
    return 8 + 8 * k * ((d + UPDATE_COLS - 1) // UPDATE_COLS) + 4 * ((R + ROWS - 1) // ROWS)


def seed_work_bytes(R):
    return 16 + 12 * ((R + RED_THREADS - 1) // RED_THREADS)


# ---- the distance and the winner -------------------------------------------------------------------------------------------------
def distances(x, cen, dtype=F32):
    """[R, k]: acc from +0 over the columns ascending, t = x - c, p = t * t, acc = acc + p, each rounded once in `dtype`."""
    x, cen = np.asarray(x, dtype=dtype), np.asarray(cen, dtype=dtype)
    acc = np.zeros((x.shape[0], cen.shape[0]), dtype=dtype)
    with np.errstate(all="ignore"):
        for c in range(x.shape[1]):
            t = x[:, c, None] - cen[None, :, c]
            p = t * t
            acc = acc + p
    return acc


def winners(D):
    """(labels int32, dist): the smallest by IEEE comparison, ties to the lower j, a NaN never; -1 and NaN (0x7FC00000) without one."""
    D = np.asarray(D)
    nan = np.isnan(D)
    key = np.where(nan, 2e300, np.where(np.isinf(D), 1e300, D.astype(F64)))          # finite < +Inf < NaN; no distance is negative
    lab = np.argmin(key, axis=1).astype(np.int32)                         # the first minimum: the lower j
    rows = np.arange(D.shape[0])
    none = nan[rows, lab]
    dist = D[rows, lab].copy()
    dist[none] = np.array([NAN_BITS], dtype=np.uint32).view(F32)[0] if D.dtype == F32 else np.nan
    lab[none] = -1
    return lab, dist


def winners_brute(D):
    """The rule of the header, one comparison at a time (the exhaustive small cases of tests/test_kmeans_cpu.py)."""
    lab, dist = np.full(D.shape[0], -1, np.int32), np.full(D.shape[0], np.nan, D.dtype)
    for r in range(D.shape[0]):
        for j in range(D.shape[1]):
            v = D[r, j]
            if v == v and (lab[r] < 0 or v < dist[r]):
                lab[r], dist[r] = j, v
    return lab, dist


def assign(x, cen, dtype=F32):
    return winners(distances(x, cen, dtype))


# ---- the update --------------------------------------------------------------------------------------------------------------------
def update(x, labels, cen_old, dtype=F32, waves=UPDATE_WAVES):
    """(cen_new, counts): the fp64 mean of every cluster in the header's order: `waves` contiguous row ranges, each summed in
    ascending row order from +0, the ranges' sums added in range order, one division; rounded to `dtype` (fp32: the contract;
    fp64: nothing is rounded).  A centre without members keeps cen_old's bits."""
    x64 = np.asarray(x).astype(F64)
    R, d = x64.shape
    cen_old = np.asarray(cen_old, dtype=dtype)
    k = cen_old.shape[0]
    L = (R + waves - 1) // waves
    new, counts = cen_old.copy(), np.zeros(k, np.int32)
    with np.errstate(all="ignore"):
        for j in range(k):
            S, n = None, 0
            for v in range(waves):
                lo, hi = min(v * L, R), min((v + 1) * L, R)
                p = np.zeros(d, F64)
                for r in np.nonzero(labels[lo:hi] == j)[0]:
                    p = p + x64[lo + r]
                    n += 1
                S = p if S is None else S + p
            counts[j] = n
            if n:
                new[j] = (S / F64(n)).astype(dtype)
    return new, counts


def shift_of(new, old):
    """fp64: per (centre, 64-column tile) the squares of (double)new - (double)old added over the columns ascending from +0;
    then thread u of 256 adds the tiles u, u + 256, .. ascending from +0 and a tree (stride 128 .. 1) adds the threads."""
    e = np.asarray(new).astype(F64) - np.asarray(old).astype(F64)
    k, d = e.shape
    tiles = (d + UPDATE_COLS - 1) // UPDATE_COLS
    parts = []
    with np.errstate(all="ignore"):
        for j in range(k):
            for t in range(tiles):
                q = F64(0.0)
                for c in range(t * UPDATE_COLS, min((t + 1) * UPDATE_COLS, d)):
                    q = q + e[j, c] * e[j, c]
                parts.append(q)
        s = np.zeros(RED_THREADS, F64)
        for u in range(min(RED_THREADS, len(parts))):
            a = F64(0.0)
            for i in range(u, len(parts), RED_THREADS):
                a = a + parts[i]
            s[u] = a
        stride = RED_THREADS // 2
        while stride:
            s[:stride] = s[:stride] + s[stride:2 * stride]
            stride //= 2
    return s[0]


# ---- Lloyd's loop ------------------------------------------------------------------------------------------------------------------
class Run(NamedTuple):
    cen: np.ndarray
    labels: np.ndarray
    dist: np.ndarray
    prev: np.ndarray
    counts: np.ndarray
    n_iter: int
    shift: list
    changed: list
    stopped: bool
    min_gap: float               # the smallest relative gap (second - best) / second of any row in any assignment (fp64 runs)
    any_empty: bool


def _gap(D):
    if D.shape[1] < 2:
        return np.inf
    two = np.sort(D, axis=1)[:, :2]
    with np.errstate(all="ignore"):
        return float(np.min((two[:, 1] - two[:, 0]) / two[:, 1]))


def lloyd(x, cen, max_iter, tol_abs, resume=False, prev=None, dtype=F32):
    """vf_kmeans_lloyd restated: scikit-learn's _kmeans_single_lloyd.  dtype=F32 is the contract; F64 the double-precision twin."""
    x = np.asarray(x, dtype=dtype)
    cen = np.array(cen, dtype=dtype)
    R, k = x.shape[0], cen.shape[0]
    prev = np.array(prev, dtype=np.int32) if resume else np.zeros(R, np.int32)
    counts = np.zeros(k, np.int32)
    shift, changed, stopped, gap, empty = [], [], False, np.inf, False
    for n in range(max_iter):
        first = n == 0 and not resume
        D = distances(x, cen, dtype)
        gap = min(gap, _gap(D))
        lab, _ = winners(D)
        ch = R if first else int(np.count_nonzero(lab != prev))
        prev = lab
        new, counts = update(x, lab, cen, dtype)
        empty |= bool((counts == 0).any())
        sh = shift_of(new, cen)
        cen = new
        changed.append(ch)
        shift.append(sh)
        if (ch == 0 and not first) or sh <= tol_abs:
            stopped = True
            break
    D = distances(x, cen, dtype)
    gap = min(gap, _gap(D))
    labels, dist = winners(D)
    return Run(cen, labels, dist, prev, counts, len(shift), shift, changed, stopped, gap, empty)


# ---- seeding -----------------------------------------------------------------------------------------------------------------------
def mix32(x: int) -> int:
    x &= _MASK
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _MASK
    x ^= x >> 15
    x = (x * 0x846CA68B) & _MASK
    return x ^ (x >> 16)


def hash64(seed: int, t: int) -> int:
    a = mix32((seed & _MASK) + 0x9E3779B9)
    return (mix32(a ^ (2 * t)) << 32) | mix32(a ^ (2 * t + 1))


def mulhi64(h: int, n: int) -> int:
    return (h * n) >> 64


def quanta(mind):
    """(q uint64 [R], m): q = (uint64)((double)mind / (double)m * 2^32), 0 for a non-finite mind or m == 0; m the largest finite mind."""
    mind = np.asarray(mind, dtype=F32)
    fin = np.isfinite(mind)
    m = F32(mind[fin].max()) if fin.any() else F32(0.0)
    q = np.zeros(mind.shape[0], np.uint64)
    if m > 0:
        q[fin] = (mind[fin].astype(F64) / F64(m) * F64(4294967296.0)).astype(np.uint64)
    return q, m


def pick(q, target: int) -> int:
    """The lowest r whose inclusive prefix sum exceeds target."""
    return int(np.searchsorted(np.cumsum(q, dtype=np.uint64), np.uint64(target), side="right"))      # the total is below 2^56


def pick_brute(q, target: int) -> int:
    run = 0
    for r, v in enumerate(q.tolist()):
        run += v
        if run > target:
            return r
    raise AssertionError("target is not below the total")


def seed_rows(x, k, seed):
    """(rows int32 [k], mind fp32 [R] as the last step left it): vf_kmeans_seed restated."""
    x = np.asarray(x, dtype=F32)
    R = x.shape[0]
    rows = [mulhi64(hash64(seed, 0), R)]
    mind = None
    for t in range(1, k):
        dnew = distances(x, x[rows[-1]][None, :])[:, 0]
        with np.errstate(all="ignore"):
            mind = dnew if mind is None else np.where(dnew < mind, dnew, mind)
        q, _ = quanta(mind)
        total = int(q.astype(object).sum())
        if total > 0:
            rows.append(pick(q, mulhi64(hash64(seed, t), total)))
        else:
            rows.append(min(set(range(t + 1)) - set(rows)))
    return np.array(rows, np.int32), mind


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def blobs(R, d, g, noise, s, scale=1.0, center=False, normalise=False):
    rng = np.random.default_rng(s)
    cen = rng.standard_normal((g, d)) * scale
    x = cen[np.arange(R) % g] + noise * rng.standard_normal((R, d))
    if center:
        x = x - x.mean(axis=1, keepdims=True)
    if normalise:
        x = x / np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x, dtype=F32)


class Fixture(NamedTuple):
    name: str
    make: object                  # () -> x fp32 [R, d]
    start: tuple                  # the rows of x that start the centres
    n_iter: dict                  # tol -> the iterations scikit-learn, the fp64 and the fp32 restatement all take (measured)
    min_gap: float                # the smallest relative gap of the fp64 run at tol 0 (measured); the condition is 32 d 2^-24


TOLS = (0.0, 1e-4, 1e-2, 1e-1)
# (C) has g = 5 generating centres.  Measured with scikit-learn 1.7.2: every fixture meets its condition with the seeds as given;
# its centres and the fp64 restatement's differ by at most 3.6e-15, and the fp32 restatement's centres equal the rounded fp64 ones.
_A = lambda: blobs(96, 12, 4, 0.8, 1, center=True, normalise=True)
_B = lambda: blobs(257, 33, 6, 1.0, 2, normalise=True)
_C = lambda: blobs(130, 2, 5, 1.2, 7, scale=4.0)
FIXTURES = [
    Fixture("A-k4", _A, (0, 1, 2, 3), {0.0: 5, 1e-4: 5, 1e-2: 5, 1e-1: 3}, 4.201e-3),
    Fixture("A-k4-b", _A, (0, 4, 2, 3), {0.0: 7, 1e-4: 7, 1e-2: 7, 1e-1: 6}, 6.130e-4),
    Fixture("B-k6", _B, (0, 6, 2, 3, 4, 5), {0.0: 5, 1e-4: 5, 1e-2: 5, 1e-1: 4}, 8.558e-5),     # condition 6.29e-5,
    Fixture("B-k9", _B, tuple(range(9)), {0.0: 7, 1e-4: 7, 1e-2: 7, 1e-1: 5}, 8.558e-5),        # its first iteration shares B-k6's closest call,
    Fixture("C-k5", _C, (0, 5, 10, 3, 4), {0.0: 9, 1e-4: 9, 1e-2: 6, 1e-1: 2}, 2.971e-3),
    Fixture("C-k7", _C, tuple(range(7)), {0.0: 11, 1e-4: 11, 1e-2: 4, 1e-1: 2}, 1.370e-2),
]


def fixture(name: str) -> Fixture:
    return next(f for f in FIXTURES if f.name == name)


def gap_condition(d: int) -> float:
    """d 2^-24 bounds the relative error of the fp32 chain of d products and d sums; 32 is the safety factor."""
    return 32.0 * d * 2.0 ** -24


def tol_abs_of(x, tol: float) -> float:
    """scikit-learn's _tolerance on the fp64 copy of the rows."""
    return float(tol) * float(np.mean(np.var(np.asarray(x, dtype=F64), axis=0)))

"""References and the case table of the enrichment entries (include/vf_hip_enrich.h): the overlap counts in numpy, the tail rule
restated cell by cell in IEEE fp64 (Python floats and ints: the same + * / and comparisons the device does, so `tail` and
`steps` are compared bit for bit; math.log / exp / log1p stand where the device has its own), exact integer arithmetic to hold
the rule to (math.comb sums), and Benjamini-Hochberg as scipy.stats.false_discovery_control states it.

How log_p is bounded against exact arithmetic: the rule's only inexact inputs are the nine logfact values, each within half an
ulp of itself after the subtractions' roundings, so BOUND_LF * 2^-52 * sum |the nine terms|; the running sum adds one rounding
per step and the last log / exp / log1p a few more, BOUND_STEPS * 2^-50 * (1 + steps).  Both constants are 1: the largest deviation
measured on the exhaustive grid and on random cells is 0.66 of this bound (tests/test_enrich_cpu.py prints it on every run)."""
import math

import numpy as np

MAX_K, MAX_N, THREADS = 4096, 1 << 24, 256         # VF_ENRICH_MAX_K, VF_ENRICH_MAX_N, VF_ENRICH_THREADS
STOP = 2.0 ** -60                                  # VF_ENRICH_STOP
GREATER, LESS = 0, 1
BOUND_LF, BOUND_STEPS = 1.0, 1.0                   # the constants of the derived bound: not widened
LOG_P_ULPS = 4                                     # device log_p from the restatement's, in ulp at max(1, |log_p|)


# ---- counts ----------------------------------------------------------------------------------------------------------------------
def counts(termptr, gene, labels, k: int):
    """(count int32 [T, k], size int32 [T]) as the header states them."""
    T, G = termptr.shape[0] - 1, labels.shape[0]
    count, size = np.zeros((T, k), dtype=np.int32), np.zeros(T, dtype=np.int32)
    for t in range(T):
        g = gene[termptr[t]:termptr[t + 1]]
        g = g[(g >= 0) & (g < G)]
        size[t] = g.shape[0]
        c = labels[g]
        c = c[(c >= 0) & (c < k)]
        count[t] = np.bincount(c, minlength=k)
    return count, size


TERM_SIZES = (0, 1, 63, 64, 65)                    # then: every gene; one with -1 and G among its entries; random ones


def counts_case(G: int, k: int, T: int = 40, seed: int = 0):
    """(termptr int64 [T + 1], gene int32 [nnz], labels int32 [G]): terms of the sizes above, one listing all G genes, one with
    the indices -1 and G among its entries, the rest of random sizes around the block width; labels in -1 .. k, both present."""
    rng = np.random.default_rng(1000 * G + k + seed)
    lists = [np.sort(rng.permutation(G)[:s]) for s in TERM_SIZES]
    lists.append(np.arange(G))
    odd = rng.permutation(G)[:70]
    odd[3], odd[40], odd[69] = -1, G, G + 5
    lists.append(odd)
    while len(lists) < T:
        lists.append(np.sort(rng.permutation(G)[:int(rng.integers(2, min(G, 2 * THREADS + 9)))]))
    termptr = np.zeros(T + 1, dtype=np.int64)
    termptr[1:] = np.cumsum([len(v) for v in lists])
    labels = rng.integers(-1, k + 1, size=G).astype(np.int32)
    labels[:4] = (-1, k, 0, k - 1)
    return termptr, np.concatenate(lists).astype(np.int32), labels


# ---- the tail rule ---------------------------------------------------------------------------------------------------------------
def log_factorials(N: int) -> np.ndarray:
    return np.array([math.lgamma(i + 1.0) for i in range(N + 1)], dtype=np.float64)


def support(N: int, K: int, n: int):
    return max(0, n - (N - K)), min(K, n), ((n + 1) * (K + 1)) // (N + 2)


def sum_up(x0: int, hi: int, K: int, n: int, N: int):
    t = s = 1.0
    steps = 0
    i = x0
    while i < hi:
        t = (t * float((K - i) * (n - i))) / float((i + 1) * (N - K - n + i + 1))
        s = s + t
        steps += 1
        i += 1
        if t < s * STOP:
            break
    return s, steps


def sum_down(x0: int, lo: int, K: int, n: int, N: int):
    t = s = 1.0
    steps = 0
    i = x0
    while i > lo:
        t = (t * float(i * (N - K - n + i))) / float((K - i + 1) * (n - i + 1))
        s = s + t
        steps += 1
        i -= 1
        if t < s * STOP:
            break
    return s, steps


def nine(lf, x0: int, K: int, n: int, N: int):
    return (lf[K], lf[x0], lf[K - x0], lf[N - K], lf[n - x0], lf[N - K - n + x0], lf[N], lf[n], lf[N - n])


def log_pmf(lf, x0: int, K: int, n: int, N: int) -> float:
    v = [float(u) for u in nine(lf, x0, K, n, N)]
    a = (v[0] - v[1]) - v[2]
    b = (v[3] - v[4]) - v[5]
    c = (v[6] - v[7]) - v[8]
    return (a + b) - c


def tail_cell(x: int, K: int, n: int, N: int, alternative: int, lf):
    """One cell of the header's rule: (log_p, tail, steps, kind, x0).  kind: "nan", "-inf", "zero", "direct" or "complement"."""
    if K < 0 or K > N or n < 0 or n > N:
        return math.nan, math.nan, 0, "nan", None
    lo, hi, mode = support(N, K, n)
    if alternative == GREATER:
        if x > hi:
            return -math.inf, 0.0, 0, "-inf", None
        if x <= lo:
            return 0.0, 0.0, 0, "zero", None
        if x > mode:
            s, steps = sum_up(x, hi, K, n, N)
            return log_pmf(lf, x, K, n, N) + math.log(s), s, steps, "direct", x
        s, steps = sum_down(x - 1, lo, K, n, N)
        return math.log1p(-math.exp(log_pmf(lf, x - 1, K, n, N) + math.log(s))), s, steps, "complement", x - 1
    if x < lo:
        return -math.inf, 0.0, 0, "-inf", None
    if x >= hi:
        return 0.0, 0.0, 0, "zero", None
    if x < mode:
        s, steps = sum_down(x, lo, K, n, N)
        return log_pmf(lf, x, K, n, N) + math.log(s), s, steps, "direct", x
    s, steps = sum_up(x + 1, hi, K, n, N)
    return math.log1p(-math.exp(log_pmf(lf, x + 1, K, n, N) + math.log(s))), s, steps, "complement", x + 1


def tail_cells(count, size, csize, N: int, alternative: int, lf=None):
    """The rule over a [T, k] table: dict of log_p, tail fp64, steps int32, kind (object) and bound fp64 [T, k], bound being the
    derived bound of log_p against exact arithmetic (0 where the cell has no sum)."""
    lf = log_factorials(N) if lf is None else lf
    T, k = count.shape
    out = {"log_p": np.zeros((T, k)), "tail": np.zeros((T, k)), "steps": np.zeros((T, k), dtype=np.int32),
           "kind": np.empty((T, k), dtype=object), "bound": np.zeros((T, k))}
    for t in range(T):
        for c in range(k):
            x, K, n = int(count[t, c]), int(size[t]), int(csize[c])
            lp, s, steps, kind, x0 = tail_cell(x, K, n, N, alternative, lf)
            out["log_p"][t, c], out["tail"][t, c], out["steps"][t, c], out["kind"][t, c] = lp, s, steps, kind
            if x0 is not None:
                out["bound"][t, c] = derived_bound(lf, x0, K, n, N, steps)
    return out


def derived_bound(lf, x0, K, n, N, steps) -> float:
    """The absolute bound of log_p against exact arithmetic: 2^-52 * sum |the nine logfact terms| + 2^-50 * (1 + steps)."""
    return BOUND_LF * 2.0 ** -52 * float(sum(abs(float(u)) for u in nine(lf, x0, K, n, N))) + BOUND_STEPS * 2.0 ** -50 * (1 + steps)


# ---- exact arithmetic ------------------------------------------------------------------------------------------------------------
def _log_ratio(num: int, den: int) -> float:
    """log(num / den) of two positive integers, to an ulp or two: the division is Python's correctly rounded one, on operands
    shifted so that the quotient is near 1; a quotient above a half goes through log1p of the small side."""
    if num == den:
        return 0.0
    if 2 * num > den:
        return math.log1p(-_ratio(den - num, den))
    e = num.bit_length() - den.bit_length()
    return math.log((num << max(-e, 0)) / (den << max(e, 0))) + e * math.log(2.0)


def _ratio(num: int, den: int) -> float:
    if num == 0:
        return 0.0
    e = num.bit_length() - den.bit_length()
    return math.ldexp((num << max(-e, 0)) / (den << max(e, 0)), e) if e > -1000 else 0.0


def exact_log_tail(x: int, K: int, n: int, N: int, alternative: int) -> float:
    """log P[X >= x] or log P[X <= x] from math.comb sums: exact integers up to the last logarithm."""
    lo, hi, _ = support(N, K, n)
    rng = range(max(x, lo), hi + 1) if alternative == GREATER else range(lo, min(x, hi) + 1)
    num = sum(math.comb(K, i) * math.comb(N - K, n - i) for i in rng)
    return -math.inf if num == 0 else _log_ratio(num, math.comb(N, n))


def grid(N: int):
    """The exhaustive table of one N: rows are every (K, x) with 0 <= K <= N and -1 <= x <= N + 1, columns every n in 0 .. N.
    Returns (count int32 [T, k], size int32 [T], csize int32 [k])."""
    Ks, xs = np.meshgrid(np.arange(N + 1), np.arange(-1, N + 2), indexing="ij")
    size = Ks.ravel().astype(np.int32)
    count = np.repeat(xs.ravel()[:, None], N + 1, axis=1).astype(np.int32)
    return count, size, np.arange(N + 1, dtype=np.int32)


GRID_MAX_N = 12
BIG_N = 18000


def big_table(N: int = BIG_N, T: int = 50, k: int = 40, seed: int = 0):
    """About 2 000 cells at the notebook's universe: term sizes 5 .. 500 and cluster sizes 50 .. 2 000, beside K = 0, n = 0, a
    term of half and of all the universe and a cluster of nearly all of it; x walks through lo, hi, the mode and its two
    neighbours, the expected overlap and random places of the support."""
    rng = np.random.default_rng(seed + N)
    size = rng.integers(5, 501, size=T).astype(np.int32)
    size[:4] = (0, N // 2, N, 1)
    csize = rng.integers(50, 2001, size=k).astype(np.int32)
    csize[:3] = (0, N - 10, 1)
    count = np.zeros((T, k), dtype=np.int32)
    for t in range(T):
        for c in range(k):
            lo, hi, mode = support(N, int(size[t]), int(csize[c]))
            pick = (lo, hi, mode, mode - 1, mode + 1, int(rng.integers(lo, hi + 1)), min(hi, mode + int(rng.integers(0, 12))),
                    min(hi, 3 * mode + 2), lo - 1, hi + 1)
            count[t, c] = pick[(t * k + c) % len(pick)]
    return count, size, csize


# ---- Benjamini-Hochberg ------------------------------------------------------------------------------------------------------------
def bh(p):
    """scipy.stats.false_discovery_control(p.ravel(), method="bh"), restated: the same operations in the same order."""
    ps = np.asarray(p, dtype=np.float64).ravel()
    m = ps.shape[0]
    order = np.argsort(ps, kind="stable")
    ps = ps[order]
    ps *= m / np.arange(1, m + 1)
    ps = np.minimum.accumulate(ps[::-1])[::-1]
    out = np.empty_like(ps)
    out[order] = ps
    return np.clip(out, 0, 1).reshape(np.shape(p))


# ---- end to end --------------------------------------------------------------------------------------------------------------------
PLANTED_GENES, PLANTED_CLUSTERS, PLANTED_TERMS = 600, 6, 30


def planted(seed: int = 0):
    """(labels int32 [600], annotations dict, universe): six clusters of 100 genes; term "planted_c" draws 40 genes from cluster c
    alone, 24 "random_j" terms draw 20 .. 80 genes from everywhere."""
    rng = np.random.default_rng(seed)
    universe = [f"G{i:04d}" for i in range(PLANTED_GENES)]
    labels = (rng.permutation(PLANTED_GENES) % PLANTED_CLUSTERS).astype(np.int32)
    members = {}
    for c in range(PLANTED_CLUSTERS):
        members[f"planted_{c}"] = rng.permutation(np.flatnonzero(labels == c))[:40]
    for j in range(PLANTED_TERMS - PLANTED_CLUSTERS):
        members[f"random_{j:02d}"] = rng.permutation(PLANTED_GENES)[:int(rng.integers(20, 81))]
    annotations = {g: [] for g in universe}
    for term, rows in members.items():
        for i in rows:
            annotations[universe[i]].append(term)
    return labels, annotations, universe

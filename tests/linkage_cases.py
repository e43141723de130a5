"""References and the case table of the Ward linkage (include/vf_hip_linkage.h, variantformer_amd/linkage.py).

The reference is fp32 numpy restating the algorithm round by round with the same operation order: `nearest` is
vf_linkage_nearest, `contract_round` is vf_linkage_contract, `ward_reference` is linkage.ward's loop.  Every fp32 operation of
the device code is individually rounded (no fma, IEEE division and square root), and so is every numpy operation on float32
arrays, so the two agree bit for bit and the GPU tests compare with array_equal.  The reference itself is held against scipy
on the host (tests/test_linkage_cpu.py).

The case table: correlation distances of random rows and of cluster-structured rows at n = 2, 3, 5, 54, 63, 64, 65, 200, 257
and one 1000 x 49 case (no ties: the reference must equal scipy's tree), then the tie cases, on which any valid linkage is right
and the device must still equal the reference: a geometric chain (one merge per round), 54 constant rows (all distances equal),
duplicated rows (zero distances).  Two more cases carry the first matrix in another layout: a garbage lower triangle, and a
slice with ld > n.

Height bounds (relative, against scipy's fp64 linkage of the same fp32 matrix; measured over the no-tie cases where this was
written, asserted at 8 times the measurement because the deviation grows with the depth of the tree, not with the code):
  the reference against scipy on the table's matrices              measured 2.8e-7, asserted 2.3e-6  (REF_HEIGHT_RTOL);
  ward_of_rows on 54 x 300 against scipy on numpy's fp64 1 - corrcoef  measured 5.1e-6 on an MI355X, asserted 4.1e-5
                                                                   (ROWS_HEIGHT_RTOL; why it is larger: below).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

F32 = np.float32
NS = (2, 3, 5, 54, 63, 64, 65, 200, 257)
REF_HEIGHT_MEASURED = 2.8e-7
REF_HEIGHT_RTOL = 8 * REF_HEIGHT_MEASURED
# ward_of_rows(54 x 300) against scipy on 1 - np.corrcoef in fp64.  Here the distances themselves differ: they are formed in fp32
# from rows that sit at 5 +- 1 (an ulp of 4.8e-7 before the mean is taken off), so a distance is a few 1e-7 absolute off the
# fp64 one (the bound of tests/neighbors_cases.py), and the lowest merges of the cluster-structured rows stand at 0.08: a few
# 1e-6 relative, which the tree carries upwards.  The trees are the same, ids and sizes.
ROWS_HEIGHT_MEASURED = 5.1e-6
ROWS_HEIGHT_RTOL = 8 * ROWS_HEIGHT_MEASURED


# ---- the two entries -------------------------------------------------------------------------------------------------------------
def ascending_key(x: np.ndarray) -> np.ndarray:
    """uint32 whose unsigned order is the header's: ascending, -0 tied with +0, every NaN above +Inf."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).copy()
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    u[u == 0x80000000] = 0
    key = np.where((u & np.uint32(0x80000000)) != 0, ~u, u | np.uint32(0x80000000))
    key[nan] = 0xFFFFFFFF
    return key


def nearest(D: np.ndarray):
    """(nn_val fp32 [m], nn_idx int32 [m]) of the square matrix D: vf_linkage_nearest."""
    m = D.shape[0]
    if m == 1:
        return np.array([np.inf], dtype=F32), np.array([-1], dtype=np.int32)
    pair = (ascending_key(D).astype(np.uint64) << np.uint64(32)) | np.arange(m, dtype=np.uint64)[None, :]
    pair[np.arange(m), np.arange(m)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    idx = pair.argmin(axis=1).astype(np.int32)
    return np.ascontiguousarray(D, dtype=F32)[np.arange(m), idx].copy(), idx


def lance_williams(dxi, dyi, dxy, sx, sy, si):
    """The header's LW on fp32 arrays (sizes integer arrays): one rounding per operation, in its order."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t1 = (sx + si).astype(F32) * (dxi * dxi)
        t2 = (sy + si).astype(F32) * (dyi * dyi)
        t3 = si.astype(F32) * (dxy * dxy)
        q = ((t1 + t2) - t3) / (sx + sy + si).astype(F32)
        return np.sqrt(np.where(q < 0, F32(0), q))


def contract_round(D: np.ndarray, size: np.ndarray, first: np.ndarray, second: np.ndarray, upper_only: bool):
    """(D_out fp32 [m_out, m_out], size_out int32, pair_dist fp32): vf_linkage_contract."""
    D = np.asarray(D, dtype=F32)
    if upper_only:
        D = np.where(np.triu(np.ones(D.shape, dtype=bool), 1), D, D.T)  # the upper triangle mirrored, bits kept; the diagonal is not used
    first = first.astype(np.int64)
    merged = second >= 0
    sec = np.where(merged, second, 0).astype(np.int64)
    size = size.astype(np.int64)
    m_out = first.shape[0]
    s1, s2 = size[first], np.where(merged, size[sec], 0)
    pd = np.where(merged, D[first, sec], F32(0)).astype(F32)
    a, b = np.meshgrid(np.arange(m_out), np.arange(m_out), indexing="ij")
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    A, B, C, Dd = first[lo], sec[lo], first[hi], sec[hi]
    sA, sB, sC, sD = s1[lo], s2[lo], s1[hi], s2[hi]
    mlo, mhi = merged[lo], merged[hi]
    dAC, dBC, dAD, dBD = D[A, C], D[B, C], D[A, Dd], D[B, Dd]
    dAB, dCD = pd[lo], pd[hi]
    lo_only = lance_williams(dAC, dBC, dAB, sA, sB, sC)
    hi_only = lance_williams(dAC, dAD, dCD, sC, sD, sA)
    u = lo_only
    v = lance_williams(dAD, dBD, dAB, sA, sB, sD)
    both = lance_williams(u, v, dCD, sC, sD, sA + sB)
    out = np.where(mlo & mhi, both, np.where(mlo, lo_only, np.where(mhi, hi_only, dAC))).astype(F32)
    out[np.arange(m_out), np.arange(m_out)] = F32(0)
    return out, (s1 + s2).astype(np.int32), pd


def select_pairs(nn_idx: np.ndarray):
    """(first, second) int32 [m_out] of a round from the nearest rows: mutual pairs merge, a pair takes its lower slot's place."""
    m = nn_idx.shape[0]
    ar = np.arange(m)
    nn = nn_idx.astype(np.int64)
    mutual = nn[nn] == ar
    lower, upper = mutual & (ar < nn), mutual & (ar > nn)
    first = ar[~upper]
    return first.astype(np.int32), np.where(lower, nn, -1)[~upper].astype(np.int32)


def to_scipy(child, height, size, n):
    order = np.argsort(height, kind="stable")
    new_id = np.arange(2 * n - 1, dtype=np.int64)
    new_id[n + order] = n + np.arange(n - 1)
    Z = np.empty((n - 1, 4), dtype=np.float64)
    Z[:, :2] = np.sort(new_id[child[order]], axis=1)
    Z[:, 2] = height[order]
    Z[:, 3] = size[order]
    return Z


def ward_reference(D: np.ndarray):
    """(Z float64 [n - 1, 4], rounds): linkage.ward, round by round, in fp32 numpy."""
    n = D.shape[0]
    ident = np.arange(n, dtype=np.int32)
    W, size, _ = contract_round(D, np.ones(n, dtype=np.int32), ident, np.full(n, -1, dtype=np.int32), True)
    node = np.arange(n, dtype=np.int64)
    height = np.zeros(n, dtype=F32)
    child, heights, sizes = [], [], []
    made = rounds = 0
    while W.shape[0] > 1:
        _, nn_idx = nearest(W)
        first, second = select_pairs(nn_idx)
        assert first.shape[0] < W.shape[0], "no mutually nearest pair"
        W, size, pd = contract_round(W, size, first, second, False)
        merged = second >= 0
        f, s = first.astype(np.int64), np.where(merged, second, 0).astype(np.int64)
        h = np.maximum(pd, np.maximum(height[f], height[s])).astype(F32)
        k = made + np.cumsum(merged) - 1
        child.append(np.stack((node[f], node[s]), 1)[merged])
        heights.append(h[merged])
        sizes.append(size[merged])
        node = np.where(merged, n + k, node[f])
        height = np.where(merged, h, height[f]).astype(F32)
        made += int(merged.sum())
        rounds += 1
    return to_scipy(np.concatenate(child), np.concatenate(heights), np.concatenate(sizes), n), rounds


# ---- the case table --------------------------------------------------------------------------------------------------------------
def correlation_distance(x: np.ndarray) -> np.ndarray:
    """fp32 1 - corrcoef with a zero diagonal, a constant row at distance 1 from every other: what neighbors.correlation_distance
    gives, to the last bits or so (the table's cases start from this matrix, not from the rows)."""
    x = np.asarray(x, dtype=np.float64)
    t = x - x.mean(axis=1, keepdims=True)
    nrm = np.sqrt((t * t).sum(axis=1, keepdims=True))
    z = np.divide(t, nrm, out=np.zeros_like(t), where=nrm > 0)
    D = np.maximum(1.0 - z @ z.T, 0.0).astype(F32)                      # duplicated rows: exactly 0, never a rounding's -1e-16
    D = np.triu(D, 1)
    return D + D.T


def random_rows(n: int, d: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal((n, d))


def clustered_rows(n: int, d: int, seed: int) -> np.ndarray:
    g = np.random.default_rng(seed)
    centres = g.standard_normal((max(2, n // 9), d))
    return centres[g.integers(0, centres.shape[0], n)] + 0.3 * g.standard_normal((n, d))


@dataclass(frozen=True)
class Case:
    name: str
    D: np.ndarray                 # fp32 [n, ld]; the matrix is D[:, :n]
    ties: bool                    # a tie case: scipy may build another valid tree

    @property
    def n(self) -> int:
        return self.D.shape[0]

    @property
    def matrix(self) -> np.ndarray:
        return self.D[:, :self.n]


def _chain(n: int) -> np.ndarray:
    """Points on a line at 0, 1, 5, 21, ...: every gap is four times the one before, more than the Ward distance from everything
    to its left (below 1.9 gaps), so only the leftmost pair is ever mutually nearest and a round merges one pair."""
    p = (4.0 ** np.arange(n) - 1.0) / 3.0
    return np.abs(p[:, None] - p[None, :]).astype(F32)


_CASES = None


def cases():
    """The table, built once.  Seeds: d = 49 throughout but for n = 54 (d = 300, the tissues of a few hundred genes).  A seed whose
    fp32 matrix has a near-tie at fp32 resolution (the reference then builds another valid tree than scipy's fp64 run) would be
    replaced here and named; none of the seeds below needed that."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    for n in NS:
        d = 300 if n == 54 else 49
        out.append(Case(f"random-{n}x{d}", correlation_distance(random_rows(n, d, 1000 + n)), False))
        out.append(Case(f"clustered-{n}x{d}", correlation_distance(clustered_rows(n, d, 2000 + n)), False))
    out.append(Case("clustered-1000x49", correlation_distance(clustered_rows(1000, 49, 3000)), False))
    out.append(Case("chain-12", _chain(12), True))
    out.append(Case("constant-54", correlation_distance(np.full((54, 49), 2.5)), True))
    which = np.random.default_rng(4001).permutation(60) % 20            # 20 distinct rows, each three times: distance exactly 0 within a triple
    out.append(Case("duplicates-60", np.ascontiguousarray(correlation_distance(random_rows(20, 49, 4000))[which][:, which]), True))
    base = correlation_distance(clustered_rows(65, 49, 5000))
    garbage = base.copy()
    garbage[np.tril_indices(65, -1)] = np.random.default_rng(5001).standard_normal(65 * 64 // 2).astype(F32) - F32(3.0)
    garbage[np.arange(65), np.arange(65)] = np.nan
    out.append(Case("garbage-lower-65", garbage, False))
    wide = np.full((63, 63 + 11), np.nan, dtype=F32)
    wide[:, :63] = correlation_distance(random_rows(63, 49, 6000))
    out.append(Case("ld-above-n-63", wide, False))
    _CASES = out
    return out


def upper(D: np.ndarray) -> np.ndarray:
    """The symmetric matrix of D's upper triangle, zero diagonal: what the algorithm sees of a case."""
    U = np.triu(np.asarray(D, dtype=F32), 1)
    return U + U.T


_REFERENCE = {}


def reference(case: Case):
    """(Z, rounds) of a case, computed once and shared; callers do not write to it."""
    if case.name not in _REFERENCE:
        Z, rounds = ward_reference(case.matrix)
        Z.setflags(write=False)
        _REFERENCE[case.name] = (Z, rounds)
    return _REFERENCE[case.name]


def rows_case():
    """The 54 x 300 matrix of the ward_of_rows test: 54 tissues over 300 genes, cluster-structured."""
    return (clustered_rows(54, 300, 7000) + 5.0).astype(F32)


# ---- inputs of the entry tests ---------------------------------------------------------------------------------------------------
def nearest_case(m: int, seed: int = 0) -> np.ndarray:
    """fp32 [m, m] full of what the order is about: few distinct values (ties), +0 and -0, +Inf, NaN; rows that are all NaN, all
    +Inf, and one whose minimum stands in the last column."""
    g = np.random.default_rng(100 + m + seed)
    pool = np.array([0.0, -0.0, 0.25, 0.25, 0.5, 1.0, np.inf, np.nan, 2.0, -1.0], dtype=F32)
    D = pool[g.integers(0, pool.shape[0], (m, m))]
    if m >= 3:
        D[0] = np.nan
        D[1] = np.inf
        D[2] = 1.0
        D[2, m - 1] = -0.0 if m - 1 != 2 else 1.0
    if m >= 63:
        D[5, :] = 3.0
        D[5, m - 2:] = np.float32(-np.inf)
        D[6, :] = np.nan
        D[6, m - 1] = np.inf                                            # +Inf ranks before NaN
    return D


def contract_case(kind: str):
    """(D fp32 [m, m] symmetric, size int32 [m], first, second int32 [m_out]) of one reference round."""
    g = np.random.default_rng({"none": 1, "single": 2, "all": 3, "mixed": 4}[kind])
    m = {"none": 65, "single": 65, "all": 64, "mixed": 257}[kind]
    D = upper(np.abs(g.standard_normal((m, m))).astype(F32) + F32(0.1))
    size = np.ones(m, dtype=np.int32) if kind in ("none", "single") else g.integers(1, 9, m).astype(np.int32)
    second_of = np.full(m, -1, dtype=np.int64)
    if kind == "single":
        second_of[17] = 40
    elif kind == "all":
        perm = g.permutation(m)
        for x, y in zip(perm[0::2], perm[1::2]):
            second_of[min(x, y)] = max(x, y)
    elif kind == "mixed":
        perm = g.permutation(m)[:160]                                   # 80 pairs among 257 slots: merged rows meet merged columns
        for x, y in zip(perm[0::2], perm[1::2]):
            second_of[min(x, y)] = max(x, y)
    removed = np.zeros(m, dtype=bool)
    removed[second_of[second_of >= 0]] = True
    first = np.flatnonzero(~removed)
    return D, size, first.astype(np.int32), second_of[first].astype(np.int32)


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))

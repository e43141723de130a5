"""The references and the case table of vf_rows_standardize, vf_knn_dot and vf_pairwise_dot (include/vf_hip_neighbors.h), shared by
tests/test_neighbors_cpu.py, tests/test_neighbors_gpu.py and tests/test_expression_neighbors_gpu.py.  Importing this module
needs no GPU.

There is one ordering in the library and one reference of it: a ranking here is tests/topk_cases.reference applied to the
full similarity matrix with the self column removed.

Two kinds of data.  EXACT: integer-valued fp32 in [-8, 8].  Every product is an integer of at most 64 and every partial sum
of d <= 1536 of them stays below 64 * 1536 < 2^24, so every admissible summation order gives the same bits as the contract's
fmaf chain and every comparison is np.array_equal; ties are plentiful.  RANDOM: standard normal rows, standardised on the
host, compared through the a-priori bound of an fp32 chain (tau below), which is derived and not measured.
"""
from __future__ import annotations

import math
import os
import re
import zlib
from typing import NamedTuple

import numpy as np

from tests import topk_cases as T
from tests.conftest import REPO

HEADER = os.path.join(REPO, "include", "vf_hip_neighbors.h")


def header_text() -> str:
    with open(HEADER) as f:
        return f.read()


def tile_constants() -> dict:
    src = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)          # as tests/test_abi_cpu.py::_declared strips comments
    return {k: int(v) for k, v in re.findall(r"#define\s+VF_KNN_(B[MNK])\s+(\d+)", src)}


_TC = tile_constants()
BM, BN, BK = _TC["BM"], _TC["BN"], _TC["BK"]
KS = (1, 30, 31, 64)
EXTRA_LD = 5                       # ld = d + 5: odd for the even d, so rows are only 4-byte aligned
EXTRA_LDO = 3
PAST_TOPK = T.MAX_N + BN + 1       # more rows of y than vf_topk_rows has columns
SELF_MODES = ("none", "zero", "slice", "outside")
EXACT_KINDS = ("dense", "ties", "first_tile", "last_tile", "per_tile", "edges", "nonfinite", "zero_row")
SLICE_AT = 3                       # "slice": q is y[3 : 3 + Rq] on the device, self_offset = 3


def _around(tile: int) -> tuple:
    return (1, tile - 1, tile, tile + 1, 2 * tile + 1)


def geometries() -> list:
    """(Rq, Ry, d, k, self_mode): each of Rq / BM, Ry / BN, d / BK at 1, tile - 1, tile, tile + 1, 2 tile + 1 around the base
    (BM + 1, 2 BN + 1, BK + 1); Ry at k - 1, k, k + 1; every k; every self mode; the largest exact d; Ry past top-k's limit."""
    base = (BM + 1, 2 * BN + 1, BK + 1)
    out = []
    n = 0

    def add(Rq, Ry, d, k, mode=None):
        nonlocal n
        if mode is None:
            mode = SELF_MODES[n % len(SELF_MODES)]
            n += 1
        if mode == "slice" and Ry < SLICE_AT + Rq:                     # a slice needs its rows: fall back to the other self form
            mode = "zero"
        g = (Rq, Ry, d, k, mode)
        if g not in out:
            out.append(g)
    for Rq in _around(BM):
        add(Rq, base[1], base[2], 30)
    for Ry in _around(BN):
        add(base[0], Ry, base[2], 30)
    for d in _around(BK):
        add(base[0], base[1], d, 30)
    for k in KS:
        for Ry in (k - 1, k, k + 1):                                   # k = 1: Ry = 0, no candidate at all, every rank is padding
            add(5, Ry, 7, k)
        add(base[0], base[1], base[2], k)
    for mode in SELF_MODES:
        add(base[0], 3 * BN + 2, base[2], 31, mode)
    add(BM + 1, 2 * BN + 1, 1536, 30, "zero")
    add(3, PAST_TOPK, 5, 30, "zero")
    return out


class Case(NamedTuple):
    Rq: int
    Ry: int
    d: int
    k: int
    mode: str
    kind: str
    q: np.ndarray                   # fp32 [Rq, d + EXTRA_LD]; 0xFF bytes behind d.  In "slice" mode a copy of y[SLICE_AT : SLICE_AT + Rq]
    y: np.ndarray                   # fp32 [Ry, d + EXTRA_LD]
    self_offset: int

    @property
    def name(self):
        return f"Rq{self.Rq}-Ry{self.Ry}-d{self.d}-k{self.k}-{self.mode}-{self.kind}"


def self_offset_of(mode: str, Rq: int, Ry: int) -> int:
    return {"none": -1, "zero": 0, "slice": SLICE_AT, "outside": Ry}[mode]


def planted(kind: str, Ry: int, k: int) -> list:
    """The rows of y that hold the winners of a planted kind."""
    tiles = (Ry + BN - 1) // BN
    if kind == "first_tile":
        return list(range(min(k, BN, Ry)))
    if kind == "last_tile":
        return list(range(max((tiles - 1) * BN, Ry - k, 0), Ry))
    if kind == "per_tile":
        return [min(t * BN + (7 * t + 3) % BN, Ry - 1) for t in range(tiles)]     # the last tile may be a few rows only
    assert kind == "edges"
    return sorted(j for j in {j for t in range(tiles + 1) for j in (t * BN - 1, t * BN)} | {0, Ry - 1} if 0 <= j < Ry)


def _poisoned(rows: int, d: int) -> np.ndarray:
    a = np.empty((rows, d + EXTRA_LD), dtype=np.float32)
    a.view(np.uint8)[:] = T.POISON
    return a


def exact_case(geometry: tuple, kind: str) -> Case:
    Rq, Ry, d, k, mode = geometry
    g = np.random.default_rng(zlib.crc32(f"knn {geometry} {kind}".encode()))
    q, y = _poisoned(Rq, d), _poisoned(Ry, d)
    if kind in ("dense", "nonfinite", "zero_row"):
        q[:, :d] = g.integers(-8, 9, (Rq, d))
        y[:, :d] = g.integers(-8, 9, (Ry, d))
    elif kind == "ties":
        q[:, :d] = g.integers(-1, 2, (Rq, d))
        y[:, :d] = g.integers(-1, 2, (Ry, d))
    else:                                                              # planted: the q rows share one sign pattern, winners are 8 * it
        sign = g.choice(np.array([-1.0, 1.0], dtype=np.float32), d)
        q[:, :d] = g.integers(1, 3, (Rq, d)) * sign
        y[:, :d] = g.integers(-2, 3, (Ry, d))
        y[planted(kind, Ry, k), :d] = 8.0 * sign
    if kind == "nonfinite":
        words = np.array(T.NANS[:3] + (0x7F800000, 0xFF800000, 0x80000000), dtype=np.uint32)
        for a, rows in ((y, Ry), (q, Rq)):
            for n, r in enumerate(g.permutation(rows)[:max(1, min(rows // 3, 9))]):
                a.view(np.uint32)[r, g.integers(0, d)] = words[n % len(words)]
    if kind == "zero_row":
        y[g.permutation(Ry)[:max(1, Ry // 8)], :d] = 0.0
        q[g.integers(0, Rq), :d] = 0.0
    if mode == "slice":
        q = y[SLICE_AT:SLICE_AT + Rq].copy()
    finite = lambda a: np.where(np.isfinite(a[:, :d]), np.abs(a[:, :d]), 0).max(initial=0)
    assert finite(q) <= 8 and finite(y) <= 8 and 64 * d < 2 ** 24 and d <= 1536, "partial sums must stay exact"
    return Case(Rq, Ry, d, k, mode, kind, q, y, self_offset_of(mode, Rq, Ry))


def chain(q: np.ndarray, y: np.ndarray) -> np.ndarray:
    """s(r, j) of the header in fp32, column by column from +0.0f: on EXACT data product and sum are exact, so fmaf and
    multiply-then-add agree; NaN and Inf take the route they take on the device (Inf * 0, Inf - Inf -> NaN)."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    acc = np.zeros((q.shape[0], y.shape[0]), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(q.shape[1]):
            acc = acc + q[:, c:c + 1] * y[None, :, c]
    return acc


def rank(sim: np.ndarray, k: int, self_offset: int):
    """tests/topk_cases.reference on each row of sim with the column r + self_offset removed: (values fp32, indices int32) [Rq, k]."""
    Rq, Ry = sim.shape
    values = np.zeros((Rq, k), dtype=np.float32)
    indices = np.full((Rq, k), -1, dtype=np.int32)
    for r in range(Rq):
        cols = np.arange(Ry)
        s = r + self_offset
        if self_offset >= 0 and s < Ry:
            cols = np.delete(cols, s)
        v, i = T.reference(sim[r:r + 1, cols], k)
        have = i[0] >= 0
        indices[r, have] = cols[i[0][have]]
        values[r] = v[0]
    return values, indices


def expected(c: Case):
    return rank(chain(c.q[:, :c.d], c.y[:, :c.d]), c.k, c.self_offset)


def same_bits(got: np.ndarray, want: np.ndarray) -> bool:
    """Bit equality, except that a NaN equals any NaN: the payload an accumulator ends with is the hardware's."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(T.bits(got)[~np.isnan(got)], T.bits(want)[~np.isnan(want)]))


# ---- random data -----------------------------------------------------------------------------------------------------------
U = 2.0 ** -24                     # the unit roundoff of fp32
RANDOM_SHAPES = ((200, 5), (1000, 5), (333, 33), (1000, 49), (1000, 64))            # (rows, d); k = 30; q is y, self excluded
RANDOM_K = 30


def host_standardize(x: np.ndarray, center: bool = True) -> np.ndarray:
    x = x.astype(np.float64)
    t = x - x.mean(axis=1, keepdims=True) if center else x
    n = np.sqrt((t * t).sum(axis=1, keepdims=True))
    return (t / np.where(n == 0, 1.0, n)).astype(np.float32)


class RandomCase(NamedTuple):
    rows: int
    d: int
    z: np.ndarray                   # fp32 [rows, d + EXTRA_LD], standardised on the host; 0xFF bytes behind d
    sim: np.ndarray                 # fp64 [rows, rows]: the similarities of the fp32 rows
    tau: np.ndarray                 # fp64 [rows, rows]

    @property
    def name(self):
        return f"random-{self.rows}x{self.d}"


def tau(q: np.ndarray, y: np.ndarray) -> np.ndarray:
    """(d + 4) * 2^-24 * sum_k |q_k y_k|: the a-priori bound of a length-d fp32 chain against the exact sum, gamma_d with room
    for its second-order terms (d u / (1 - d u) < (d + 4) u for d <= 1536).  Derived, not measured."""
    d = q.shape[1]
    return (d + 4) * U * (np.abs(q.astype(np.float64)) @ np.abs(y.astype(np.float64)).T)


_RANDOM: dict = {}


def random_case(rows: int, d: int) -> RandomCase:
    if (rows, d) not in _RANDOM:                                       # computed once, shared, never modified
        g = np.random.default_rng(zlib.crc32(f"knn random {rows} {d}".encode()))
        z = _poisoned(rows, d)
        z[:, :d] = host_standardize(g.standard_normal((rows, d)))
        zz = z[:, :d].astype(np.float64)
        c = RandomCase(rows, d, z, zz @ zz.T, tau(z[:, :d], z[:, :d]))
        for a in c[2:]:
            a.setflags(write=False)
        _RANDOM[(rows, d)] = c
    return _RANDOM[(rows, d)]


def fp64_ranking(c: RandomCase, k: int = RANDOM_K):
    """Per row the columns in descending fp64 similarity with self removed, k + 1 of them: (indices, sims, taus) [rows, k + 1]."""
    s = c.sim.copy()
    np.fill_diagonal(s, -np.inf)
    order = np.argsort(-s, axis=1, kind="stable")[:, :k + 1]
    rows = np.arange(c.rows)[:, None]
    return order, s[rows, order], c.tau[rows, order]


def decided(c: RandomCase, k: int = RANDOM_K) -> np.ndarray:
    """bool [rows, k]: the (row, rank) pairs at which the index is decided -- the fp64 gaps to both neighbouring ranks (rank k,
    the first column not returned, included) exceed the sum of the two taus."""
    _, s, t = fp64_ranking(c, k)
    gap_ok = (s[:, :-1] - s[:, 1:]) > (t[:, :-1] + t[:, 1:])             # [rows, k]: rank i against rank i + 1
    before = np.concatenate([np.ones((c.rows, 1), dtype=bool), gap_ok[:, :-1]], axis=1)
    return gap_ok & before


def check_random(c: RandomCase, values: np.ndarray, indices: np.ndarray, k: int = RANDOM_K, self_excluded: bool = True) -> float:
    """The four checks on every row, then exact indices wherever they are decided.  Returns the decided fraction."""
    rows = np.arange(c.rows)[:, None]
    assert indices.shape == values.shape == (c.rows, k)
    # 2. distinct, in range, not self
    assert ((indices >= 0) & (indices < c.rows)).all(), "an index out of range"
    assert all(len(set(r)) == k for r in indices.tolist()), "an index twice in a row"
    if self_excluded:
        assert (indices != rows).all(), "a row is its own neighbour"
    # 1. the value is the similarity of the index it stands beside
    err = np.abs(values.astype(np.float64) - c.sim[rows, indices])
    assert (err <= c.tau[rows, indices]).all(), f"a value is {(err / c.tau[rows, indices]).max():.2f} tau from its fp64 similarity"
    # 3. the returned order is the kernel's own: descending, ties by ascending index
    v = values.astype(np.float64)
    assert ((v[:, :-1] > v[:, 1:]) | ((v[:, :-1] == v[:, 1:]) & (indices[:, :-1] < indices[:, 1:]))).all(), "ranks out of order"
    # 4. nothing left out is better than the last rank by more than the two bounds
    kept = np.zeros((c.rows, c.rows), dtype=bool)
    kept[rows, indices] = True
    if self_excluded:
        kept[rows, rows] = True
    last = v[:, -1:] + c.tau[rows, indices[:, -1:]]
    assert (kept | (c.sim <= last + c.tau)).all(), "a column that was not returned beats the last rank"
    want, _, _ = fp64_ranking(c, k) if self_excluded else (None, None, None)
    if want is None:
        return 1.0
    dec = decided(c, k)
    assert np.array_equal(indices[dec], want[:, :k][dec]), f"{int((indices != want[:, :k])[dec].sum())} decided ranks hold another index"
    return float(dec.mean())


# ---- standardize -----------------------------------------------------------------------------------------------------------
STD_KINDS = ("normal", "offset", "constant", "zero", "nan", "inf", "mixed_inf", "constant_inexact")
INEXACT = np.float32(3.0671477)    # a constant whose fp32 mean over 49, 63, 65 or 200 columns is not itself (device_mean; asserted on the CPU)
STD_DS = (1, 5, 49, 63, 64, 65, 200)


def std_rows(d: int, g: np.random.Generator) -> np.ndarray:
    """One row of each kind of STD_KINDS, fp32 [8, d]."""
    x = np.empty((len(STD_KINDS), d), dtype=np.float32)
    x[0] = g.standard_normal(d)
    x[1] = 1000.0 + g.standard_normal(d)
    x[2] = 3.0
    x[3] = 0.0
    x[4] = g.standard_normal(d)
    x[4, g.integers(0, d)] = np.nan
    x[5] = g.standard_normal(d)
    x[5, g.integers(0, d)] = np.inf
    x[6] = g.standard_normal(d)
    x[6, 0], x[6, d - 1] = np.inf, -np.inf
    x[7] = INEXACT
    return x


def std_case(d: int) -> np.ndarray:
    x = _poisoned(len(STD_KINDS), d)
    x[:, :d] = std_rows(d, np.random.default_rng(zlib.crc32(f"standardize {d}".encode())))
    return x


def device_mean(row: np.ndarray) -> np.float32:
    """The mean of one row in the header's order, in fp32: lane l adds the columns l, l + 64, ... from +0.0f, the 64 partial sums
    meet in the xor butterfly 32 .. 1, and the sum is divided by d."""
    row = np.asarray(row, dtype=np.float32)
    part = np.zeros(64, dtype=np.float32)
    for c in range(len(row)):
        part[c % 64] = part[c % 64] + row[c]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        part = part + part[lanes ^ off]
    return np.float32(part[0] / np.float32(len(row)))


def std_reference(x: np.ndarray, center: bool):
    """fp64 (z, norm) of finite rows; a row with norm 0 is zero with norm 0 -- under centring that is every row whose values are
    all equal, whatever a rounded mean leaves of them; a non-finite row is NaN with norm NaN."""
    x = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        mean = x.mean(axis=1, keepdims=True)
        mean = np.where((x == x[:, :1]).all(axis=1, keepdims=True), x[:, :1], mean)        # a constant row's mean is its value
        t = x - mean if center else x
        n = np.sqrt((t * t).sum(axis=1))
        z = t / np.where(n == 0, 1.0, n)[:, None]
    bad = ~np.isfinite(x).all(axis=1)
    z[bad], n[bad] = np.nan, np.nan
    return z, n


def std_bound(x: np.ndarray, center: bool):
    """(tol_z [R, d], tol_norm [R]): the a-priori error of the two-pass fp32 algorithm of the header against fp64, u = 2^-24.
    A lane adds ceil(d / 64) terms, the butterfly six more, so a sum carries at most L = ceil(d / 64) + 6 roundings:
      mean:  |m^ - m| <= dm = (L + 1) u mean|x|              (the sum, then the division; 0 without centring)
      t^ = fl(x - m^):  |t^ - t| <= dm + u |t|
      norm:  |n^ - n| <= sqrt(d) dm + n (L / 2 + 3) u         (||t^ - t||_2 <= sqrt(d) dm + u n; the fmaf sum L u relative, halved by
                                                               the root; the root and the product roundings)
      z^ = fl(t^ / n^):  |z^ - z| <= (dm + u |t|) / n + |z| (sqrt(d) dm / n + (L / 2 + 4) u)
    times 1.05 for the second-order terms.  Not tuned to any kernel's output."""
    x = x.astype(np.float64)
    d = x.shape[1]
    L = math.ceil(d / 64) + 6
    z, n = std_reference(x, center)
    dm = (L + 1) * U * np.abs(x).mean(axis=1) if center else np.zeros(x.shape[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(n > 0, dm / n, 0.0)[:, None]
        tol_z = 1.05 * (rel + U * np.abs(z) + np.abs(z) * (math.sqrt(d) * rel + (L / 2 + 4) * U))
        tol_n = 1.05 * (math.sqrt(d) * dm + n * (L / 2 + 3) * U)
    return tol_z, tol_n


def one_pass_fp32(x: np.ndarray) -> np.ndarray:
    """The formula the header forbids, in fp32 numpy: z = (x - m) / sqrt(sum x^2 - (sum x)^2 / d)."""
    x = x.astype(np.float32)
    d = np.float32(x.shape[1])
    s1 = x.sum(axis=1, dtype=np.float32)
    s2 = (x * x).sum(axis=1, dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (x - (s1 / d)[:, None]) / np.sqrt(s2 - s1 * s1 / d)[:, None]

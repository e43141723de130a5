"""The numpy reference, the case table and the plausible mistakes of vf_topk_rows (include/vf_hip_topk.h), shared by
tests/test_topk_cpu.py, tests/test_topk_gpu.py and tests/test_attention_topk_gpu.py.  Importing this module needs no GPU.

Everything here is compared bit for bit (int32 views of the fp32 values): there is no tolerance in a selection.

A case is one call: R = 7 rows of n columns, ldx = n + 5, ldo = k + 3, row_len NULL ("full") or ragged.  Its host array holds
0xFF bytes (a NaN, which would rank first) in every column at or past len(r), the 5 columns behind n included, so a kernel
that reads one of them shows it in the first rank.
"""
from __future__ import annotations

import zlib
from typing import NamedTuple

import numpy as np

NS = (0, 1, 2, 63, 64, 65, 200, 1024, 1025, 4097, 16384)
KS = (1, 2, 31, 64)
R = 7
EXTRA_LDX, EXTRA_LDO = 5, 3
FORMS = ("full", "ragged")
KINDS = ("distinct", "ties3", "equal", "softmax", "nonfinite")
MAX_N, MAX_K = 16384, 64
POISON = 0xFF

# A wrong implementation by name -> (the data kind that shows it, the row_len forms in which it can show).
MUTATIONS = {
    "ties_high": ("equal", FORMS),                 # ties to the higher column
    "nan_last": ("nonfinite", FORMS),              # NaN ranked below everything
    "nan_dropped": ("nonfinite", FORMS),           # NaN never selected
    "neg_zero_below": ("nonfinite", FORMS),        # -0 ranked below +0
    "padding_read": ("distinct", FORMS),           # the whole row stride is a candidate
    "row_len_ignored": ("distinct", ("ragged",)),  # every row has n columns
    "unsorted": ("distinct", FORMS),               # the right columns, in column order
    "pad_neg_inf": ("distinct", ("ragged",)),      # -Inf where the contract says +0.0
}


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def lengths(n: int, k: int, form: str):
    """row_len as passed (None for the NULL form): 0, 1, a value below k, n, one above n, a negative one, and one inside."""
    if form == "full":
        return None
    return np.array([0, 1, max(min(k, n) - 1, 0), n, n + 1, -3, n // 2 + 1], dtype=np.int32)


def clamped(n: int, row_len, rows: int = R) -> np.ndarray:
    return np.full(rows, n, dtype=np.int64) if row_len is None else np.clip(np.asarray(row_len, dtype=np.int64), 0, n)


def _select(row: np.ndarray, width: int, k: int, mistake: str | None = None):
    """Rank the columns 0 .. width-1 of one row and take k: (values fp32 [k], indices int32 [k])."""
    v = row[:width]
    cols = np.arange(width)
    nan = np.isnan(v)
    if mistake == "nan_dropped":
        v, cols, nan = v[~nan], cols[~nan], nan[~nan]
    neg = -np.where(nan, np.float32(0), v).astype(np.float64)          # -(+0) and -(-0) compare equal: +0 and -0 tie
    tie = -cols if mistake == "ties_high" else cols
    keys = [tie, neg, nan if mistake == "nan_last" else ~nan]          # the last key is the first criterion
    if mistake == "neg_zero_below":
        keys.insert(1, np.signbit(v) & (v == 0))
    order = cols[np.lexsort(keys)][:k]
    if mistake == "unsorted":
        order = np.sort(order)
    values = np.full(k, -np.inf if mistake == "pad_neg_inf" else 0.0, dtype=np.float32)
    indices = np.full(k, -1, dtype=np.int32)
    indices[:len(order)] = order
    values.view(np.int32)[:len(order)] = row.view(np.int32)[order]     # bits, not values: payloads and -0 survive
    return values, indices


def reference(x: np.ndarray, k: int, row_len=None, n: int | None = None, mistake: str | None = None):
    """x fp32 [rows, >= n].  Per row: the columns 0 .. len-1 sorted by (not isnan, -x, column), the first k, then -1 / +0.0.
    mistake: one of MUTATIONS -- what that wrong implementation returns instead."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.shape[1] if n is None else n
    lens = clamped(n, row_len, x.shape[0])
    if mistake == "row_len_ignored":
        lens = np.full(x.shape[0], n)
    elif mistake == "padding_read":
        lens = np.full(x.shape[0], x.shape[1])
    out = [_select(x[r], int(lens[r]), k, mistake) for r in range(x.shape[0])]
    return np.stack([v for v, _ in out]), np.stack([i for _, i in out])


NANS = (0x7FC00000, 0xFFC00001, 0x7F800123, 0xFFFFFFFF, 0x7FC0BEEF)           # quiet and signalling, both signs, five payloads


def make_row(kind: str, length: int, g: np.random.Generator) -> np.ndarray:
    if kind == "distinct":
        return ((g.permutation(length) - length // 2) * 0.37).astype(np.float32)
    if kind == "ties3":
        return g.choice(np.array([-1.5, 0.25, 2.0], dtype=np.float32), length)
    if kind == "equal":
        return np.full(length, 0.75, dtype=np.float32)
    if kind == "softmax":                                              # a few large weights, a tail of denormals and exact zeros
        z = g.normal(size=length) * 40.0
        p = np.exp(z - z.max()) if length else z
        p = (p / p.sum()).astype(np.float32) if length else p.astype(np.float32)
        where = g.permutation(length)
        p[where[:length // 4]] = 0.0
        p[where[length // 4:length // 4 + length // 8]] = np.float32(1e-42) * g.integers(1, 5, length // 8).astype(np.float32)
        return p
    assert kind == "nonfinite"
    # negative values, and on top of them: zeros of both signs (a -0 in the lowest zero column), three NaNs, +Inf and -Inf.
    # Above the zeros stand only the NaNs and +Inf, so both zeros are among the first 6 ranks wherever the row has 8 columns.
    row = (-np.abs(g.normal(size=length)) - 0.5).astype(np.float32)
    where = g.permutation(length)
    zeros = np.sort(where[:max(2, length // 8)]) if length >= 2 else where[:0]
    row[zeros] = np.where(np.arange(len(zeros)) % 2 == 0, np.float32(-0.0), np.float32(0.0))
    rest = where[len(zeros):]
    special = list(g.choice(np.array(NANS, dtype=np.uint32), 3, replace=False)) + [0x7F800000, 0xFF800000]
    for pos, word in zip(rest, special):
        row.view(np.uint32)[pos] = word
    return row


class Case(NamedTuple):
    n: int
    k: int
    form: str
    kind: str
    x: np.ndarray              # fp32 [R, n + EXTRA_LDX]; 0xFF bytes at and past len(r)
    row_len: np.ndarray | None

    @property
    def name(self):
        return f"n{self.n}-k{self.k}-{self.form}-{self.kind}"


def case(n: int, k: int, form: str, kind: str) -> Case:
    g = np.random.default_rng(zlib.crc32(f"topk {n} {k} {form} {kind}".encode()))
    row_len = lengths(n, k, form)
    x = np.empty((R, n + EXTRA_LDX), dtype=np.float32)
    x.view(np.uint8)[:] = POISON
    for r, length in enumerate(clamped(n, row_len)):
        x[r, :length] = make_row(kind, int(length), g)
    return Case(n, k, form, kind, x, row_len)


def expected(c: Case, mistake: str | None = None):
    return reference(c.x, c.k, c.row_len, c.n, mistake)


def rows_changed(c: Case, mistake: str) -> int:
    """In how many rows the wrong implementation's output differs from the contract's, in bits."""
    v, i = expected(c)
    wv, wi = expected(c, mistake)
    return int(((bits(v) != bits(wv)) | (i != wi)).any(axis=1).sum())

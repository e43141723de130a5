"""Exact-arithmetic operands for the attention kernels: every output element has ONE admissible bit pattern.

Shared by tests/test_attn_exact_cpu.py and tests/test_attn_exact_gpu.py; plain torch / numpy on the CPU, no GPU import.

The construction
----------------
A key sequence of n keys; L = the largest power of two <= n, e = n - L.  Exactly 2e keys carry a flag b_j = 1, the others
b_j = 0.  With base-2 logits s_j = off - b_j the softmax weights are 1 (b = 0) and 1/2 (b = 1) relative to the maximum, and
the denominator is (L - e) + 2e / 2 = L: a power of two for every n.

K   per (sequence, head) three distinct columns c0, c1, c2 (a fourth, c3, with a real ALiBi bias), different from head to
    head: c0 and c1 hold two independent flag patterns b and b' (2e ones each), c2 holds 1, c3 the key's position j, every
    other column random integers in [-2, 2].
Q   per (query, head): -1 in c0 or in c1 (drawn per query and head, so neighbouring queries have different answers), the
    integer `off` in c2, 0 elsewhere.  q . k = off - b_j (or off - b'_j): every product and partial sum is a small integer,
    exact in the fp32 MFMA accumulator in any order.
scale  with VF_ATTN_Q_LOG2 the logit is q . k itself; without it scale = float32(ln 2), for which
    scale * 1.4426950408889634f == 1.0f in fp32 (LN2_F32 below; neither neighbouring float has the property).
V   integers in {-1, 0, 1}, non-zero with probability 1/8, independent per (key, head, column).
out[i, h, :] = (2 sum_{b_j = 0} v_j + sum_{b_j = 1} v_j) / (2 L) for the pattern query i selected in head h.

Premise (asserted by the builder on every element): |2 S0 + S1| < 256, so the value is an integer of at most 8 significant
bits times a power of two -- representable in bf16 and in fp16.  It follows that the kernel's bits cannot depend on the order
of its sums (all partial sums are exact), on whether it rounds P to 16 bits (1 and 1/2 are exact), on how it rescales (by
powers of two), nor on a last-ulp error of the hardware exp2 / reciprocal (a representable value times (1 +- 2^-22) rounds
back to itself).

ALiBi, two forms: "zero" = all slopes 0 (runs the ALIBI = true code objects, every row compared); "real" =
slopes[h] = float32(ln 2) * 2^-k_h, k_h in {0, 1, 2}, so that the kernels' slope2 = slopes[h] * 1.4426950408889634f is exactly
2^-k_h.  A row at position 0 of its key sequence gets q[c3] = 2^-k_h, a row at position n - 1 gets q[c3] = -2^-k_h and
q[c2] = off + (n - 1) 2^-k_h: for these rows fma(-slope2, |i - j|, q . k) is exactly off - b_j.  Other rows of such a launch are
not compared (their distance to the keys is not linear in j).

What the screen cannot see: ALiBi on interior rows, the rounding of P, and a permutation of V rows among keys whose flags
agree in every head (attention is symmetric under it) -- the oracle tests keep covering those.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

LN2_F32 = np.float32(0.6931471824645996)
LOG2E_F32 = np.float32(1.4426950408889634)          # the kernels' constant, as fp32 arithmetic sees it
NUM_LIMIT = 256                                      # |2 S0 + S1| stays below it: 8 significant bits
ALIBI_MAX_KEYS = {"bf16": 256, "fp16": 2048}         # c3 holds the position j: exact in the operand type up to here
EDGES = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
OFFSETS = (0, -20, -200, 200)


def torch_dtype(dtype: str):
    return {"bf16": torch.bfloat16, "fp16": torch.float16}[dtype]


def pow2_floor(n: int) -> int:
    assert n >= 1
    return 1 << (int(n).bit_length() - 1)


def edges(lo: int, hi: int, extra=()) -> tuple:
    """1, 2, 3 and t - 1, t, t + 1 for t in {16, 32, 64, 128, 256}, restricted to [lo, hi], plus hi and `extra`."""
    return tuple(sorted({x for x in EDGES + (hi,) + tuple(extra) if lo <= x <= hi}))


def _exact_in(x: np.ndarray, dtype: str) -> bool:
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return bool(torch.equal(t.to(torch_dtype(dtype)).to(torch.float32), t))


def reference_table(V: np.ndarray, B: np.ndarray):
    """The two-weight softmax of ONE key sequence in exact integers: V int64 [n, H, dh], B {0,1} [n, H, P] (P flag patterns).
    Returns (num, den): num int64 [H, P, dh] = 2 sum_{b=0} v + sum_{b=1} v, den int64 [H, P] = 2 #{b=0} + #{b=1}; the output of
    a query that selected pattern p in head h is num[h, p] / den[h, p].  O(n H dh P)."""
    n = V.shape[0]
    B = B.astype(np.int64)
    s_all = V.sum(axis=0)                                             # [H, dh]
    s_one = np.einsum("nhp,nhd->hpd", B, V)                           # [H, P, dh]
    num = 2 * s_all[:, None, :] - s_one
    den = 2 * n - B.sum(axis=0)                                       # [H, P]
    return num, den


def rounded_table(V, B, dtype: str) -> torch.Tensor:
    """reference_table's quotient rounded once to the operand type (float64 division: exact to 2^-53, then one rounding)."""
    num, den = reference_table(V, B)
    return torch.from_numpy(num.astype(np.float64) / den.astype(np.float64)[:, :, None]).to(torch_dtype(dtype))


# ----------------------------------------------------------------------------------------------------------------------
# forward attention (vf_attn_varlen_fwd_v2 / _v3 / _rows) and the probabilities entry share one builder
# ----------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class FwdCase:
    name: str
    kernel: str                      # what ops.last_kernel("attn") must report
    dh: int
    H: int
    q_lens: tuple
    k_lens: tuple | None = None      # None: self attention (cu_seqlens_k = cu_seqlens_q)
    q_log2: bool = True
    alibi: str | None = None         # None | "zero" | "real"
    off: int = 0
    order: str = "random"            # "random" | "flagged_first"
    q_at_start: bool = False
    rows: bool = False               # the row-map entry (the test builds the table)
    seed: int = 0
    dtypes: tuple = ("bf16", "fp16")

    @property
    def id(self):
        return self.name


class Built:
    """Operands (fp32 tensors whose values are exact in the operand type) and the expected output of one case."""


def _positions(case: FwdCase, i: np.ndarray, lq: int, lk: int) -> np.ndarray:
    return i + (0 if case.q_at_start else lk - lq)


def build(case: FwdCase, q_pos=None) -> Built:
    """The operands and the expected output of a case (the same for both operand types; assert_premises checks a type).
    q_pos: None = the forward entries' alignment (case.q_at_start); else a callable (seq, len_q, len_k, rng) -> int array of
    the rows' positions (the probabilities entry names them explicitly)."""
    rng = np.random.default_rng(1000 + case.seed)
    H, dh = case.H, case.dh
    real = case.alibi == "real"
    ncol = 4 if real else 3
    assert dh >= ncol + 1
    q_lens = list(case.q_lens)
    k_lens = list(case.k_lens) if case.k_lens is not None else q_lens
    assert len(q_lens) == len(k_lens)
    n_seq, tq, tk = len(q_lens), sum(q_lens), sum(k_lens)
    cu_q = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int64)
    cu_k = np.concatenate([[0], np.cumsum(k_lens)]).astype(np.int64)
    K = rng.integers(-2, 3, (tk, H, dh)).astype(np.float32)
    V = ((rng.integers(0, 2, (tk, H, dh)) * 2 - 1) * (rng.random((tk, H, dh)) < 0.125)).astype(np.int8)
    Q = np.zeros((tq, H, dh), np.float32)
    expected = np.zeros((tq, H, dh), np.float64)
    compare = np.ones(tq, bool)
    k_exp = rng.integers(0, 3, H) if real else None                   # slope2 = 2^-k_h
    slope2 = (2.0 ** -k_exp.astype(np.float64)) if real else None
    flags, choices, cols, max_num = [], [], [], 0
    hh = np.arange(H)
    for s in range(n_seq):
        lq, n = q_lens[s], k_lens[s]
        qa, ka = int(cu_q[s]), int(cu_k[s])
        c = np.argsort(rng.random((H, dh)), axis=1)[:, :ncol]        # distinct columns per head, varied over the heads
        cols.append(c)
        choice = rng.integers(0, 2, (lq, H))
        choices.append(choice)
        if n == 0:
            flags.append(np.zeros((0, H, 2), np.int64))
            continue                                                  # queries without keys: Q stays 0, expected 0
        L = pow2_floor(n)
        e = n - L
        if case.order == "random":
            rank = np.argsort(np.argsort(rng.random((n, H, 2)), axis=0), axis=0)
            B = (rank < 2 * e).astype(np.int64)
        else:
            # all flagged keys first: the running maximum rises from off - 1 to off in a later tile (pattern b' starts one key
            # later, so the two patterns still differ)
            j = np.arange(n)
            B = np.stack([np.broadcast_to((j < 2 * e)[:, None], (n, H)),
                          np.broadcast_to(((j >= 1) & (j < 2 * e + 1))[:, None], (n, H))], axis=2).astype(np.int64)
        assert (B.sum(axis=0) == 2 * e).all()
        flags.append(B)
        Ks = K[ka:ka + n]
        Ks[:, hh, c[:, 0]] = B[:, :, 0]
        Ks[:, hh, c[:, 1]] = B[:, :, 1]
        Ks[:, hh, c[:, 2]] = 1.0
        if real:
            Ks[:, hh, c[:, 3]] = np.arange(n, dtype=np.float32)[:, None]
        num, den = reference_table(V[ka:ka + n].astype(np.int64), B)
        assert (den == 2 * L).all(), "the denominator is the power of two L"
        max_num = max(max_num, int(np.abs(num).max()))
        if lq == 0:
            continue
        i = np.arange(lq)
        Qs = Q[qa:qa + lq]
        Qs[i[:, None], hh[None, :], c[hh, choice]] = -1.0
        Qs[:, hh, c[:, 2]] = float(case.off)
        expected[qa:qa + lq] = num[hh[None, :], choice, :] / float(2 * L)
        if real:
            pos = _positions(case, i, lq, n) if q_pos is None else np.asarray(q_pos(s, lq, n, rng))
            first, last = pos == 0, (pos == n - 1) & (pos != 0)
            for rows_, sign in ((np.nonzero(first)[0], 1.0), (np.nonzero(last)[0], -1.0)):
                if rows_.size:
                    Qs[rows_[:, None], hh[None, :], c[:, 3][None, :]] = (sign * slope2)[None, :].astype(np.float32)
            lr = np.nonzero(last)[0]
            if lr.size:
                Qs[lr[:, None], hh[None, :], c[:, 2][None, :]] = (case.off + (n - 1) * slope2)[None, :].astype(np.float32)
            compare[qa:qa + lq] = first | last
    assert max_num < NUM_LIMIT, f"premise |2 S0 + S1| < {NUM_LIMIT} violated: {max_num}"
    b = Built()
    b.case = case
    b.q = torch.from_numpy(Q.reshape(tq, H * dh))
    b.k = torch.from_numpy(K.reshape(tk, H * dh))
    b.v = torch.from_numpy(V.astype(np.float32).reshape(tk, H * dh))
    b.V_int, b.flags, b.choices, b.cols = V, flags, choices, cols
    b.cu_q = torch.from_numpy(cu_q.astype(np.int32))
    b.cu_k = torch.from_numpy(cu_k.astype(np.int32))
    b.q_lens, b.k_lens = q_lens, k_lens
    b.max_q, b.max_k = max(q_lens + [0]), max(k_lens + [0])
    b.expected = torch.from_numpy(expected.astype(np.float32).reshape(tq, H * dh))
    b.compare = torch.from_numpy(compare)
    b.max_num = max_num
    b.k_exp = k_exp
    if case.alibi == "zero":
        b.slopes = torch.zeros(H, dtype=torch.float32)
    elif real:
        b.slopes = torch.from_numpy((LN2_F32 * (2.0 ** -k_exp).astype(np.float32)).astype(np.float32))
        assert ((b.slopes.numpy() * LOG2E_F32).astype(np.float32) == (2.0 ** -k_exp).astype(np.float32)).all()
    else:
        b.slopes = None
    b.scale = None if case.q_log2 else float(LN2_F32)
    assert np.array_equal(expected.astype(np.float32).astype(np.float64), expected)
    if case.rows:
        _duplicate_sequences(b)
    return b


def _duplicate_sequences(b: Built) -> None:
    """The row-map form: every sequence occurs twice, the copy reading the SAME table rows (b.row_of_token: token -> row of the
    table of distinct rows; the test permutes the table, so the map is out of order as well)."""
    T = b.q.shape[0]
    b.row_of_token = torch.cat([torch.arange(T), torch.arange(T)])
    b.table = (b.q, b.k, b.v)
    b.q, b.k, b.v = (torch.cat([x, x]) for x in (b.q, b.k, b.v))
    b.expected, b.compare = torch.cat([b.expected, b.expected]), torch.cat([b.compare, b.compare])
    b.cu_q = torch.cat([b.cu_q, b.cu_q[1:] + b.cu_q[-1]])
    b.cu_k = torch.cat([b.cu_k, b.cu_k[1:] + b.cu_k[-1]])
    b.q_lens, b.k_lens = b.q_lens * 2, b.k_lens * 2
    b.flags, b.choices, b.cols = b.flags * 2, b.choices * 2, b.cols * 2
    b.V_int = np.concatenate([b.V_int, b.V_int])


def assert_premises(b: Built, dtype: str) -> None:
    """Every operand and every expected value has ONE bit pattern in the operand type."""
    for name in ("q", "k", "v", "kv", "expected"):
        x = getattr(b, name, None)
        if x is not None:
            assert torch.equal(x.to(torch_dtype(dtype)).to(torch.float32), x), f"{name} is not exact in {dtype}"
    if getattr(b.case, "alibi", None) == "real":
        assert b.max_k <= ALIBI_MAX_KEYS[dtype], "the key position must be exact in the operand type"


@functools.lru_cache(maxsize=3)
def built(case) -> Built:
    return build(case)


def expected_rows(b: Built) -> torch.Tensor:
    """Indices of the rows whose bits the screen fixes."""
    return torch.nonzero(b.compare)[:, 0]


def emulate_tiled(b: Built, tile: int, max_rows: int = 8) -> tuple:
    """fp32 online softmax over key tiles of `tile` keys with a running maximum, rescaling and a final o * (1 / l), on the
    first `max_rows` rows of every sequence (no bias: for cases without a real ALiBi bias).  Returns (rows, out fp32)."""
    case = b.case
    H, dh = case.H, case.dh
    rows, outs = [], []
    for s in range(len(b.q_lens)):
        lq, n = min(b.q_lens[s], max_rows), b.k_lens[s]
        qa, ka = int(b.cu_q[s]), int(b.cu_k[s])
        if lq == 0:
            continue
        q = b.q[qa:qa + lq].view(lq, H, dh).permute(1, 0, 2)          # [H, lq, dh]
        o = torch.zeros(H, lq, dh)
        m = torch.full((H, lq, 1), float("-inf"))
        l = torch.zeros(H, lq, 1)
        for t0 in range(0, n, tile):
            k = b.k[ka + t0:ka + min(n, t0 + tile)].view(-1, H, dh).permute(1, 0, 2)
            v = b.v[ka + t0:ka + min(n, t0 + tile)].view(-1, H, dh).permute(1, 0, 2)
            sc = q @ k.transpose(1, 2)
            m_new = torch.maximum(m, sc.max(dim=-1, keepdim=True).values)
            alpha = torch.exp2(m - m_new)
            p = torch.exp2(sc - m_new)
            l = l * alpha + p.sum(dim=-1, keepdim=True)
            o = o * alpha + p @ v
            m = m_new
        out = o * (1.0 / l) if n > 0 else o
        rows.append(torch.arange(qa, qa + lq))
        outs.append(out.permute(1, 0, 2).reshape(lq, H * dh))
    return torch.cat(rows), torch.cat(outs)


# ---- the case table: every instantiation launch_attn can select (thresholds read from vf_attn.hip) -------------------------------
F64, F128 = "attn_fwd_kernel<64-query blocks>", "attn_fwd_kernel<128-query blocks>"
X32, X64 = "attn_x32_kernel<32 queries per wave>", "attn_x32_kernel<64 queries per wave>"
SHORT = "attn_short_kernel"
S2_1, S2_2 = "attn_short2_kernel<1 pass>", "attn_short2_kernel<2 passes>"
S2_1R, S2_2R = "attn_short2_kernel<1 pass,rows>", "attn_short2_kernel<2 passes,rows>"


def _cycle(values, n, shift=0):
    return tuple(values[(i + shift) % len(values)] for i in range(n))


E300 = edges(1, 300)                 # 1 .. 257, 300
E128 = edges(1, 128)
E256 = edges(1, 256)
E1300 = edges(1, 1300, extra=(603, 1000, 1024))


def _cross(q_edges, k_edges, n_seq=None, seed=0):
    """Ragged cross attention: every query edge and every key edge occurs, paired off against each other in a seeded order; one
    sequence without keys and one without queries."""
    n = max(len(q_edges), len(k_edges)) if n_seq is None else n_seq
    rng = np.random.default_rng(77 + seed)
    ql = list(_cycle(q_edges, n))
    kl = list(_cycle(k_edges, n))
    rng.shuffle(kl)
    return tuple(ql) + (4, 0), tuple(kl) + (0, 9)


def _self(edge_list, n_seq=None):
    n = len(edge_list) if n_seq is None else n_seq
    return _cycle(edge_list, n) + (0,)


def _forward_cases():
    cs = []

    def add(name, kernel, dh, H, q_lens, k_lens=None, **kw):
        cs.append(FwdCase(name, kernel, dh, H, tuple(q_lens), None if k_lens is None else tuple(k_lens), seed=len(cs), **kw))

    # attn_fwd_kernel, 64-query blocks: dh 128; classes 192 / 256 (padded 136 / 200); a long cross attention at dh 64
    add("fwd64_dh128_self", F64, 128, 4, _self(E300))
    add("fwd64_dh128_self_plain_first", F64, 128, 4, _self(E300), q_log2=False, order="flagged_first", off=-20)
    add("fwd64_dh128_self_alibi0", F64, 128, 4, _self(E300), alibi="zero", off=200)
    add("fwd64_dh128_self_alibi", F64, 128, 4, _self(E256), alibi="real")
    qc, kc = _cross(E300, E1300, seed=1)
    add("fwd64_dh128_cross", F64, 128, 2, qc, kc, off=-200, order="flagged_first")
    add("fwd64_dh64_long_cross", F64, 64, 4, qc, kc)
    add("fwd64_dh64_long_cross_plain", F64, 64, 4, qc, kc, q_log2=False, off=200, order="flagged_first")
    add("fwd64_dh64_long_cross_alibi0", F64, 64, 4, qc, kc, alibi="zero", off=-20)
    for dh, H in ((136, 2), (200, 2)):
        add(f"fwd64_pad{dh}_self", F64, dh, H, _self(E300), order="flagged_first")
        add(f"fwd64_pad{dh}_cross_plain_alibi0", F64, dh, H, qc, kc, q_log2=False, alibi="zero", off=-20)
    # the other padded classes through vf_attn_varlen_fwd_v3: 24 -> 32, 40 -> 48, 56 -> 64, 80 -> 96, 104 -> 128
    for dh, kern in ((24, F64), (40, X32), (56, F64), (80, F64), (104, F64)):
        add(f"pad{dh}_self", kern, dh, 2, _self(E300))
        add(f"pad{dh}_cross_plain_first", kern, dh, 2, qc, kc, q_log2=False, order="flagged_first", off=200)
    add("pad40_self_alibi", S2_2, 40, 2, _self(edges(1, 220) + (129, 200)), alibi="real")
    add("pad24_self_alibi", SHORT, 24, 2, _self(E256), alibi="real")

    # attn_fwd_kernel, 128-query blocks: dh <= 64 with max_q > 256 and n_seq H ceil(max_q / 128) >= 1024; dh 96 windows
    l22 = _self(E300, 21) + (300,)                                    # 22 non-empty sequences + the empty one
    assert 23 * 16 * 3 >= 1024
    add("fwd128_dh64_self", F128, 64, 16, l22)
    add("fwd128_dh64_self_plain_first", F128, 64, 16, l22, q_log2=False, order="flagged_first", off=-200)
    add("fwd128_dh64_self_alibi0", F128, 64, 16, l22, alibi="zero", off=-20)
    add("fwd128_dh32_self_alibi0", F128, 32, 16, l22, alibi="zero", off=200)
    q128, k128 = _cross(E300, E1300, n_seq=22, seed=2)
    add("fwd128_dh64_cross", F128, 64, 16, q128, k128, order="flagged_first")
    w96 = _self(E128, 64)
    assert len(w96) * 16 >= 1024
    add("fwd128_dh96_windows", F128, 96, 16, w96)
    add("fwd128_dh96_windows_plain_alibi0", F128, 96, 16, w96, q_log2=False, alibi="zero", off=200, order="flagged_first")
    add("fwd128_dh96_windows_alibi", F128, 96, 16, w96, alibi="real")
    q96, k96 = _cross(edges(1, 128), E1300, n_seq=64, seed=3)
    add("fwd128_dh96_cross", F128, 96, 16, q96, k96, off=-20)

    # attn_x32_kernel (dh 48 without bias), 32 queries per wave; 64 per wave once n_seq H ceil(max_q / 256) >= 2048
    for off in OFFSETS:
        add(f"x32_cross_off{off}", X32, 48, 4, qc, kc, off=off)
    add("x32_cross_plain_first", X32, 48, 4, qc, kc, q_log2=False, order="flagged_first", off=-200)
    add("x32_self", X32, 48, 4, _self(E300 + (603, 1000, 1300)), order="flagged_first")
    q64, k64 = _cross(E256, E1300 + _cycle(E128, 41), n_seq=63, seed=4)        # every long key stream once, short ones beside
    assert len(q64) * 32 * 1 >= 2048
    for off in OFFSETS:
        add(f"x64_cross_off{off}", X64, 48, 32, q64, k64, off=off)
        add(f"x64_cross_first_off{off}", X64, 48, 32, q64, k64, off=off, order="flagged_first")
    add("x64_cross_plain", X64, 48, 32, q64, k64, q_log2=False, off=200)
    add("x64_self", X64, 48, 32, _self(E256, 64))

    # attn_short_kernel: dh <= 48 with a bias (or dh 32), max_q in (128, 256], an LDS image too large for three blocks
    # (225..256 keys); 3 query groups up to 192 queries, 4 above
    q3, k3 = _cross(edges(1, 192), E256, seed=5)
    add("short3_dh48_cross_alibi0", SHORT, 48, 8, q3, k3, alibi="zero")
    add("short3_dh48_cross_alibi0_plain_first", SHORT, 48, 8, q3, k3, alibi="zero", q_log2=False, order="flagged_first", off=-200)
    add("short3_dh32_cross", SHORT, 32, 8, q3, k3, off=200)
    add("short4_dh48_self_alibi0", SHORT, 48, 8, _self(E256), alibi="zero", off=-20)
    add("short4_dh48_self_alibi", SHORT, 48, 8, _self(E256), alibi="real")
    add("short4_dh48_self_alibi_plain", SHORT, 48, 8, _self(E256), alibi="real", q_log2=False, order="flagged_first")
    add("short4_dh32_self_plain_first", SHORT, 32, 8, _self(E256), q_log2=False, order="flagged_first", off=200)
    qs1, ks1 = tuple([1] * len(E256)) + (1, 0), tuple(E256) + (0, 7)
    add("fwd64_dh48_registry_q_at_start", F64, 48, 8, qs1, ks1, alibi="real", q_at_start=True)

    # attn_short2_kernel in one pass: dh 64 and dh 32, at most 128 tokens, n_seq H >= 1024
    w128 = _self(E128, 128)
    assert len(w128) * 8 >= 1024
    add("short2_1pass_dh64_self", S2_1, 64, 8, w128)
    add("short2_1pass_dh64_self_plain_first", S2_1, 64, 8, w128, q_log2=False, order="flagged_first", off=-200)
    add("short2_1pass_dh64_self_alibi0", S2_1, 64, 8, w128, alibi="zero", off=200)
    add("short2_1pass_dh64_self_alibi", S2_1, 64, 8, w128, alibi="real")
    qw, kw = _cross(E128, E128, n_seq=128, seed=6)
    add("short2_1pass_dh64_cross", S2_1, 64, 8, qw, kw, off=-20, order="flagged_first")
    add("short2_1pass_dh32_self", S2_1, 32, 8, w128, off=-20)
    add("short2_1pass_dh32_cross_plain", S2_1, 32, 8, qw, kw, q_log2=False, off=200)
    # ... in two passes: dh 48 with ALiBi at 129-220 tokens; dh 64 at 129-256 tokens with n_seq H >= 1024
    g220 = _self(edges(1, 220, extra=(200, 201)))
    add("short2_2pass_dh48_self_alibi0", S2_2, 48, 8, g220, alibi="zero")
    add("short2_2pass_dh48_self_alibi0_plain_first", S2_2, 48, 8, g220, alibi="zero", q_log2=False, order="flagged_first", off=-200)
    add("short2_2pass_dh48_self_alibi", S2_2, 48, 8, g220, alibi="real")
    qg, kg = _cross(edges(1, 256), edges(1, 220), seed=7)
    add("short2_2pass_dh48_cross_alibi0", S2_2, 48, 8, qg, kg, alibi="zero", off=200)
    c256 = _self(E256, 128)
    add("short2_2pass_dh64_self", S2_2, 64, 8, c256)
    add("short2_2pass_dh64_self_plain_first", S2_2, 64, 8, c256, q_log2=False, order="flagged_first", off=-20)
    add("short2_2pass_dh64_self_alibi0", S2_2, 64, 8, c256, alibi="zero", off=-200)
    qc2, kc2 = _cross(E256, E256, n_seq=128, seed=8)
    add("short2_2pass_dh64_cross", S2_2, 64, 8, qc2, kc2, off=200)

    # the row-map forms (the three geometries vf_attn_rows_supported reports): the model's call form only (q_log2, self)
    w64, c64 = _self(E128, 64), _self(E256, 64)                                  # (every sequence occurs twice: see build)
    assert 2 * len(w64) * 8 >= 1024
    add("rows_windows_dh64", S2_1R, 64, 8, w64, rows=True)
    add("rows_windows_dh64_first", S2_1R, 64, 8, w64, rows=True, order="flagged_first", off=-200)
    add("rows_chunks_dh64", S2_2R, 64, 8, c64, rows=True, off=200)
    add("rows_gene_self_dh48_alibi0", S2_2R, 48, 8, g220, rows=True, alibi="zero", off=-20)
    add("rows_gene_self_dh48_alibi", S2_2R, 48, 8, g220, rows=True, alibi="real")
    return cs


FORWARD_CASES = _forward_cases()
assert len({c.name for c in FORWARD_CASES}) == len(FORWARD_CASES)
KERNELS = (F64, F128, X32, X64, SHORT, S2_1, S2_2, S2_1R, S2_2R)
assert {c.kernel for c in FORWARD_CASES} == set(KERNELS)
for _c in FORWARD_CASES:
    assert (2 if _c.rows else 1) * sum(_c.q_lens) <= 20000 and sum(_c.k_lens or _c.q_lens) <= 20000 and _c.H * _c.dh <= 1536, _c.name
    if _c.alibi == "real":      # both operand types run the same lengths: bf16's limit on the position column
        assert max(_c.k_lens or _c.q_lens) <= ALIBI_MAX_KEYS["bf16"], _c.name


# ----------------------------------------------------------------------------------------------------------------------
# the probabilities entry (vf_attn_probs / vf_attn_probs_v2)
# ----------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class ProbsCase:
    name: str
    dh: int
    H: int
    per_head: bool
    q_log2: bool = True
    alibi: str | None = None         # None | "real" (form (b))
    q_pos: str | None = None         # with alibi: None = NULL (every row at position 0: the registry token) | "ends" = 0 or n - 1
    q_rows: bool = False             # selected rows with repeats from a table of queries
    k_rows: bool = False             # the keys through a row map
    off: int = 0
    seed: int = 0

    @property
    def id(self):
        return self.name


# (keys, distinct query rows) per sequence; 0 rows, 0 keys, 1, the 32-key / 32-row / 64-row tile edges
PROBS_SEQS = ((256, 40), (33, 3), (0, 3), (1, 1), (31, 65), (32, 0), (63, 1), (64, 33), (65, 64), (201, 7), (129, 2), (255, 5),
              (2, 2), (3, 1), (15, 1), (16, 2), (17, 1), (127, 3), (128, 32))
PROBS_SEQS_LONG = PROBS_SEQS + ((257, 9), (300, 31), (1300, 2))
PROBS_RTOL = 2.0 ** -20


def _probs_cases():
    cs = []

    def add(name, dh, H, per_head, **kw):
        cs.append(ProbsCase(name, dh, H, per_head, seed=len(cs), **kw))

    for dh, H in ((32, 4), (48, 8), (64, 4), (96, 2), (128, 2)):
        add(f"dh{dh}_mean", dh, H, False, off=-20)
        add(f"dh{dh}_per_head_plain_qrows", dh, H, True, q_log2=False, q_rows=True, off=200)
        add(f"dh{dh}_mean_krows_qrows", dh, H, False, k_rows=True, q_rows=True, off=-200)
        add(f"dh{dh}_per_head_alibi_registry", dh, H, True, alibi="real")
        add(f"dh{dh}_mean_alibi_ends_krows", dh, H, False, alibi="real", q_pos="ends", k_rows=True, q_rows=True)
        add(f"dh{dh}_per_head_alibi_ends_plain", dh, H, True, alibi="real", q_pos="ends", q_log2=False)
    return cs


PROBS_CASES = _probs_cases()


def build_probs(case: ProbsCase):
    """The forward builder's operands with the selected rows as the query sequences.  Returns a Built with, in addition,
    P [R, H, max_k] float64 (2^-b_j / L on the sequence's keys, 0 beyond), stats [R, H, 2] = (off, L) ((0, 0) without keys),
    q_pos int32 [R] or None, sel int64 [R] (the selected rows as indices into b.q, with repeats when case.q_rows)."""
    seqs = PROBS_SEQS if case.alibi else PROBS_SEQS_LONG
    fc = FwdCase(case.name, "", case.dh, case.H, tuple(r for _, r in seqs), tuple(n for n, _ in seqs), q_log2=case.q_log2,
                 alibi=case.alibi, off=case.off, seed=500 + case.seed)
    pos_of = {}

    def q_pos(s, lq, n, rng):
        p = np.zeros(lq, np.int64) if case.q_pos is None else rng.integers(0, 2, lq) * max(n - 1, 0)
        pos_of[s] = p
        return p
    b = build(fc, q_pos=q_pos if case.alibi else None)
    assert bool(b.compare.all())                                       # every selected row sits at position 0 or n - 1
    rng = np.random.default_rng(9000 + case.seed)
    H = case.H
    sel, n_sel = [], []
    for s, (n, r) in enumerate(seqs):
        a = int(b.cu_q[s])
        idx = a + (np.sort(rng.integers(0, r, r + 3)) if (case.q_rows and r > 0) else np.arange(r))
        sel.append(idx)
        n_sel.append(len(idx))
    sel = np.concatenate(sel).astype(np.int64)
    R, max_k = len(sel), b.max_k
    P = np.zeros((R, H, max_k))
    stats = np.zeros((R, H, 2), np.float32)
    pos = np.zeros(R, np.int32)
    cu_rows = np.concatenate([[0], np.cumsum(n_sel)]).astype(np.int32)
    hh = np.arange(H)
    for s, (n, r) in enumerate(seqs):
        a = int(b.cu_q[s])
        for o in range(cu_rows[s], cu_rows[s + 1]):
            i = sel[o] - a
            if case.alibi:
                pos[o] = pos_of[s][i] if s in pos_of else 0            # (a sequence without keys draws no positions)
            if n == 0:
                continue
            ch = b.choices[s][i]                                       # [H]
            P[o, :, :n] = (0.5 ** b.flags[s][:, hh, ch].T) / pow2_floor(n)
            stats[o, :, 0], stats[o, :, 1] = case.off, pow2_floor(n)
    b.P, b.stats = torch.from_numpy(P), torch.from_numpy(stats)
    b.sel, b.cu_rows = torch.from_numpy(sel), torch.from_numpy(cu_rows)
    b.max_rows = max(n_sel)
    b.q_pos = torch.from_numpy(pos) if (case.alibi and case.q_pos is not None) else None
    assert torch.allclose(b.P.sum(dim=-1)[b.stats[:, :, 1] > 0], torch.ones((), dtype=torch.float64), rtol=0, atol=1e-12)
    return b


# ----------------------------------------------------------------------------------------------------------------------
# keys that are copies of C distinct rows (vf_attn_counted_keys) and the softmax of counted logits (vf_softmax_counted)
# ----------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class CountedCase:
    name: str
    C: int
    dh: int
    H: int
    lens: tuple
    q_per_block: int                 # what launch_counted_keys picks for this batch (asserted from its rule by the CPU test)
    seed: int = 0

    @property
    def id(self):
        return self.name


def counted_q_per_block(n_seq: int, max_q: int) -> int:
    """launch_counted_keys' rule, restated."""
    qpb = 256
    while qpb > 64 and n_seq * ((max_q + qpb - 1) // qpb) < 1024:
        qpb >>= 1
    return qpb


def _ragged(n, top, seed):
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in rng.integers(1, 7, n)]
    lens[0], lens[1], lens[2] = top, 0, 1
    for i, x in enumerate((63, 64, 65, 127, 128, 129, 255, 256, 257)):
        if x <= top:
            lens[3 + i] = x
    return tuple(lens)


COUNTED_GEOMETRIES = ((64, _ragged(16, 300, 1)), (128, _ragged(350, 300, 2)), (256, _ragged(512, 300, 3)))
COUNTED_CASES = []
for _i, _C in enumerate((1, 2, 9, 15, 16)):
    for _j, (_qpb, _lens) in enumerate(COUNTED_GEOMETRIES):
        _dh, _H = ((32, 5), (48, 3), (64, 7))[(_i + _j) % 3]
        COUNTED_CASES.append(CountedCase(f"C{_C}_dh{_dh}_H{_H}_qpb{_qpb}", _C, _dh, _H, _lens, _qpb, seed=10 * _i + _j))
N_VARIANTS, N_PATTERNS = 4, 3


def build_counted(case: CountedCase):
    """The two-weight multiset over the rows a sequence holds: L_C - e_C rows of weight 1, 2 e_C of weight 1/2, realised through
    (count, logit) pairs (1, 0), (2, -1), (4, -2) for weight 1 and (1, -1), (2, -2) for weight 1/2: log2_count is exact and both
    the count path and the logit path carry part of the weight.  A sequence follows one of N_VARIANTS `variants` (which rows it
    holds -- the others have log2_count = -inf -- and their counts); a (query, head) selects one of the variant's N_PATTERNS
    flag patterns by a -1 in that pattern's column of K (which holds count-exponent + flag), and carries `off` (cycled over the
    sequences through 0, -20, 200, -200) against a column of ones."""
    rng = np.random.default_rng(3000 + case.seed)
    C, H, dh = case.C, case.H, case.dh
    NP = N_VARIANTS * N_PATTERNS
    assert dh >= NP + 1
    lens = list(case.lens)
    n_seq, T = len(lens), sum(lens)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Kt = rng.integers(-2, 3, (C, H, dh)).astype(np.float32)
    Vt = rng.integers(-3, 4, (C, H, dh)).astype(np.int64)
    perm = np.argsort(rng.random((H, dh)), axis=1)                     # column of pattern p in head h: perm[h, p]; ones: perm[h, NP]
    hh = np.arange(H)
    lc = np.full((N_VARIANTS, C), -np.inf, np.float32)
    Bv = np.zeros((N_VARIANTS, N_PATTERNS, C), np.int64)
    present = np.zeros((N_VARIANTS, C), bool)
    for v in range(N_VARIANTS):
        c_v = C if v == 0 else int(rng.integers(1, C + 1))
        rows = np.sort(rng.permutation(C)[:c_v])
        present[v, rows] = True
        Lc = pow2_floor(c_v)
        e = c_v - Lc
        for p in range(N_PATTERNS):
            Bv[v, p, rng.permutation(rows)[:2 * e]] = 1
        any_flag = Bv[v].max(axis=0)
        lc_v = np.where(any_flag[rows] == 1, rng.integers(0, 2, c_v), rng.integers(0, 3, c_v))   # count 1, 2 (or 4: weight 1 only)
        lc[v, rows] = lc_v
        for p in range(N_PATTERNS):
            g = np.where(present[v], np.where(present[v], lc[v], 0) + Bv[v, p], rng.integers(0, 3, C)).astype(np.float32)
            assert g.max() <= 2 and g.min() >= 0                        # logits 0, -1, -2
            Kt[:, hh, perm[:, v * N_PATTERNS + p]] = g[:, None]
    Kt[:, hh, perm[:, NP]] = 1.0
    Q = np.zeros((T, H, dh), np.float32)
    expected = np.zeros((T, H, dh), np.float64)
    log2_count = np.zeros((n_seq, C), np.float32)
    max_num = 0
    for s in range(n_seq):
        v = s % N_VARIANTS
        log2_count[s] = lc[v]
        a, n = int(cu[s]), lens[s]
        if n == 0:
            continue
        off = OFFSETS[(s // N_VARIANTS) % 4]
        pat = rng.integers(0, N_PATTERNS, (n, H))
        Q[a + np.arange(n)[:, None], hh[None, :], perm[hh[None, :], v * N_PATTERNS + pat]] = -1.0
        Q[a:a + n, hh, perm[:, NP]] = float(off)
        rows = np.nonzero(present[v])[0]
        Bs = np.broadcast_to(Bv[v][:, rows].T[:, None, :], (len(rows), H, N_PATTERNS))    # [rows, H, P]
        num, den = reference_table(Vt[rows], Bs)
        assert (den == 2 * pow2_floor(len(rows))).all()
        max_num = max(max_num, int(np.abs(num).max()))
        expected[a:a + n] = num[hh[None, :], pat, :] / den[0, 0]
    assert max_num < NUM_LIMIT
    b = Built()
    b.case = case
    b.q = torch.from_numpy(Q.reshape(T, H * dh))
    b.kv = torch.from_numpy(np.concatenate([Kt.reshape(C, H * dh), Vt.astype(np.float32).reshape(C, H * dh)], axis=1))
    b.log2_count = torch.from_numpy(log2_count)
    b.cu = torch.from_numpy(cu.astype(np.int32))
    b.lens, b.max_q = lens, max(lens)
    b.expected = torch.from_numpy(expected.astype(np.float32).reshape(T, H * dh))
    b.present, b.lc, b.Bv = present, lc, Bv
    assert np.array_equal(expected.astype(np.float32).astype(np.float64), expected)
    return b


@dataclasses.dataclass(frozen=True)
class SoftmaxCase:
    name: str
    C: int
    Cp: int
    H: int
    lens: tuple
    seed: int = 0

    @property
    def id(self):
        return self.name


SOFTMAX_CASES = []
for _i, _C in enumerate((1, 2, 9, 15, 16)):
    for _Cp in sorted({_C + (_C & 1), 16}):
        _H = (5, 3, 7)[_i % 3]
        SOFTMAX_CASES.append(SoftmaxCase(f"C{_C}_Cp{_Cp}_H{_H}", _C, _Cp, _H, (300, 0, 1, 77, 257, 5, 64), seed=_i))


def build_softmax(case: SoftmaxCase):
    """fp32 base-2 logits [T, H * Cp] and log2 counts whose sum is off - b - (a power-of-two count's exponent) + that exponent:
    weights 2^-b / L_C over the rows the sequence holds (2 e_C flags per (token, head), drawn independently), exact zeros for
    absent rows and for the padding slots c >= C, whatever finite values those slots' logits hold."""
    rng = np.random.default_rng(7000 + case.seed)
    C, Cp, H = case.C, case.Cp, case.H
    lens = list(case.lens)
    n_seq, T = len(lens), sum(lens)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    sc = rng.integers(-300, 1000, (T, H, Cp)).astype(np.float32)       # what absent rows and padding slots hold
    log2_count = np.full((n_seq, C), -np.inf, np.float32)
    want = np.zeros((T, H, Cp), np.float64)
    for s in range(n_seq):
        c_s = C if s % 2 == 0 else int(rng.integers(1, C + 1))
        rows = np.sort(rng.permutation(C)[:c_s])
        lcs = rng.integers(0, 3, c_s).astype(np.float32)
        log2_count[s, rows] = lcs
        a, n = int(cu[s]), lens[s]
        if n == 0:
            continue
        Lc = pow2_floor(c_s)
        e = c_s - Lc
        rank = np.argsort(np.argsort(rng.random((n, H, c_s)), axis=2), axis=2)
        B = (rank < 2 * e).astype(np.float32)
        off = np.asarray(OFFSETS + (7,), np.float32)[rng.integers(0, 5, (n, H, 1))]
        sc[a:a + n][:, :, rows] = off - B - lcs[None, None, :]
        want[a:a + n][:, :, rows] = 0.5 ** B / Lc
    b = Built()
    b.case = case
    b.scores = torch.from_numpy(sc.reshape(T, H * Cp))
    b.log2_count = torch.from_numpy(log2_count)
    b.cu = torch.from_numpy(cu.astype(np.int32))
    b.lens, b.max_q = lens, max(lens)
    b.expected = torch.from_numpy(want.astype(np.float32).reshape(T, H * Cp))
    assert _exact_in(want, "bf16") and _exact_in(want, "fp16")
    return b

"""Non-finite operands and 16-bit store rounding ("Non-finite operands"): the geometries, the poison placements,
the special values and a plain float64 reference of every operation, shared by tests/test_nonfinite_gpu.py (the kernels
against the contract) and tests/test_nonfinite_cpu.py (which shows, on the references alone, that these inputs discriminate).
Importable without a GPU.

Every set of outputs that is expected to be NaN comes from the float64 reference evaluated on the poisoned operands
(`*_ref` below), never from a kernel; `region()` / `gemm_region()` state the same sets in closed form, and the CPU tests
hold the two against each other."""
import functools
import math
from typing import NamedTuple

import numpy as np
import torch

from oracle import vf_oracle as O
from tests import attn_edge_cases as E
from tests.helpers import _rand

NAN, INF = float("nan"), float("inf")


def tdt(dtype: str):
    return torch.bfloat16 if dtype == "bf16" else torch.float16


# ---------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------
class NFCase(NamedTuple):
    name: str
    dh: int
    H: int
    ql: tuple
    kl: tuple
    kernel: str
    q_log2: tuple
    seed: int
    alibi: bool = True
    rows: bool = False        # the row-map form: q / k / v are tables, token t's row is rows[t] (self attention)


X32_32, X32_64 = "attn_x32_kernel<32 queries per wave>", "attn_x32_kernel<64 queries per wave>"
SHORT2_ROWS = "attn_short2_kernel<2 passes,rows>"

_rng64 = np.random.default_rng(1320)
_q64 = (7, 40, 33) + tuple(int(x) for x in _rng64.integers(1, 41, 61))
_k64 = (50, 23, 100) + tuple(int(x) for x in _rng64.integers(1, 101, 61))
_ROWS_LENS = (201, 130, 150, 37, 1, 220)

ATTN_CASES = [NFCase(*c) for c in E.ATTN_EDGE_CASES] + [
    # dh 48 without ALiBi: attn_x32_kernel for every geometry; 32 queries per wave while n_seq * H * ceil(max_q / 256) < 2048
    NFCase("x32_32q", 48, 8, (70, 33, 200, 1, 129), (100, 65, 37, 130, 9), X32_32, (True, False), 1300, alibi=False),
    NFCase("x32_64q", 48, 32, _q64, _k64, X32_64, (True, False), 1310, alibi=False),        # 64 * 32 * 1 = 2048 blocks
    # the row-map form at a geometry vf_attn_rows_supported reports: dh 48 with ALiBi, 129 ... 224 tokens, pre-scaled q
    NFCase("rows_dh48", 48, 8, _ROWS_LENS, _ROWS_LENS, SHORT2_ROWS, (True,), 1330, rows=True),
]
ATTN_BY_NAME = {c.name: c for c in ATTN_CASES}
ATTN_PARAMS = [(c.name, ql2) for c in ATTN_CASES for ql2 in c.q_log2]
assert len(_q64) * 32 * ((max(_q64) + 255) // 256) >= 2048 > 5 * 8 * 1

NAN_POISONS = ("k_nan_last", "k_nan_first", "v_nan_last", "v_nan_first", "q_nan")
INF_POISONS = ("v_inf_last", "v_inf_first", "k_inf")
POISONS = NAN_POISONS + INF_POISONS


def victim(c: NFCase) -> int:
    """The poisoned sequence: neighbours with queries and keys on both sides, at least two keys of its own (so that the
    first and the last key row differ), and no key count of the three a multiple of the 64-key tile -- the tile that holds
    a sequence's last key is staged past that key in all three.  Of those the first with at least two queries (so that Q-NaN
    has other query rows to hold to the clean bits); the first of all where the geometry has no such sequence (registry)."""
    ok = [b for b in range(1, len(c.ql) - 1)
          if all(c.ql[i] > 0 and c.kl[i] % 64 != 0 for i in (b - 1, b, b + 1)) and c.kl[b] >= 2]
    assert ok, f"{c.name}: no sequence qualifies as the victim"
    return next((b for b in ok if c.ql[b] >= 2), ok[0])


def witnesses(c: NFCase) -> tuple:
    """The clean neighbours whose bits witness the containment: the sequence in front of the victim and the one behind."""
    b = victim(c)
    return b - 1, b + 1


def head_star(c: NFCase) -> int:
    return c.H // 2


def col_star(c: NFCase) -> int:
    return c.dh - 3                  # inside the head's last 16-byte chunk


def q_row_star(c: NFCase) -> int:
    return c.ql[victim(c)] // 2      # position inside the victim


@functools.lru_cache(maxsize=4)
def operands(name: str, dtype: str, q_log2: bool):
    """(q, k, v) fp32 tensors holding values of the operand type: E.operands for the geometries of ATTN_EDGE_CASES, the same
    recipe for the others.  Treat as read-only."""
    if name in E.CASES_BY_NAME:
        return E.operands(name, dtype, q_log2)
    c = ATTN_BY_NAME[name]
    rnd = O.Rounding(dtype)
    D = c.H * c.dh
    q = _rand((sum(c.ql), D), c.seed, E.INPUT_SCALE)
    kv = rnd.r(_rand((sum(c.kl), 2 * D), c.seed + 1, E.INPUT_SCALE))
    q = rnd.r(q * (math.log2(math.e) / math.sqrt(c.dh))) if q_log2 else rnd.r(q)
    return q, kv[:, :D].contiguous(), kv[:, D:].contiguous()


def row_map(c: NFCase) -> torch.Tensor:
    """rows_dh48: token t reads table row row_map[t] -- a permutation, so one poisoned table row is one token."""
    return torch.randperm(sum(c.ql), generator=torch.Generator().manual_seed(c.seed + 2))


def slopes_of(c: NFCase):
    return torch.tensor(O.alibi_slopes(c.H), dtype=torch.float32) if c.alibi else None


def poison_site(c: NFCase, poison: str):
    """(operand 'q' | 'k' | 'v', token row, column, value) of the one poisoned element."""
    b, h = victim(c), head_star(c)
    k0, q0 = int(E.cu_of(c.kl)[b]), int(E.cu_of(c.ql)[b])
    val = NAN if "nan" in poison else INF
    if poison == "q_nan":
        return "q", q0 + q_row_star(c), h * c.dh + 1, val
    row = k0 + (c.kl[b] - 1 if poison.endswith("last") else 0)          # (k_inf: the first key row)
    if poison[0] == "k":
        return "k", row, h * c.dh + 5, val
    return "v", row, h * c.dh + col_star(c), val


def poisoned(c: NFCase, qkv, poison: str):
    t = {"q": qkv[0], "k": qkv[1], "v": qkv[2]}
    which, row, col, val = poison_site(c, poison)
    t[which] = t[which].clone()
    t[which][row, col] = val
    return t["q"], t["k"], t["v"]


def region(c: NFCase, poison: str) -> torch.Tensor:
    """bool [tq, H * dh]: the outputs that depend on the poisoned element mathematically -- every row and column of (victim,
    head*) for a K element, one column of it for a V element, one row of it for a Q element.  Everything outside must keep
    the bits of the clean launch; for the NaN poisons the region is exactly the reference's NaN set."""
    b, h = victim(c), head_star(c)
    cu_q = E.cu_of(c.ql)
    a, e = int(cu_q[b]), int(cu_q[b + 1])
    m = torch.zeros((sum(c.ql), c.H * c.dh), dtype=torch.bool)
    if poison[0] == "k":
        m[a:e, h * c.dh:(h + 1) * c.dh] = True
    elif poison[0] == "v":
        m[a:e, h * c.dh + col_star(c)] = True
    else:
        m[a + q_row_star(c), h * c.dh:(h + 1) * c.dh] = True
    return m


def _attention_ref_seq(c: NFCase, q, k, v, q_log2: bool) -> torch.Tensor:
    """One sequence in float64: softmax_j(scale * q . k - slope * |i + (sk - sq) - j|) v, per head.  q [sq, D], k / v [sk, D]."""
    H, dh = c.H, c.dh
    sq, sk = q.shape[0], k.shape[0]
    s = torch.einsum("qhd,khd->hqk", q.double().view(sq, H, dh), k.double().view(sk, H, dh))
    s = s * (math.log(2.0) if q_log2 else 1.0 / math.sqrt(dh))           # natural-log logits either way
    if c.alibi:
        d = (torch.arange(sq)[:, None] + (sk - sq) - torch.arange(sk)[None, :]).abs().double()
        s = s - slopes_of(c).double()[:, None, None] * d[None]
    p = torch.softmax(s, dim=-1)
    return torch.einsum("hqk,khd->qhd", p, v.double().view(sk, H, dh)).reshape(sq, H * dh)


def attention_ref(c: NFCase, qkv, q_log2: bool, base=None, only=None) -> torch.Tensor:
    """float64 [tq, D] over every sequence (zeros where a sequence has no keys).  `base` / `only`: the reference treats the
    sequences independently, so a result for other operands (`base`) may be reused for every sequence outside `only`
    whose operands are bit-for-bit the same -- checked here, not assumed."""
    q, k, v = qkv
    cu_q, cu_k = E.cu_of(c.ql), E.cu_of(c.kl)
    out = torch.zeros((q.shape[0], c.H * c.dh), dtype=torch.float64)
    for b in range(len(c.ql)):
        a, e, ka, ke = int(cu_q[b]), int(cu_q[b + 1]), int(cu_k[b]), int(cu_k[b + 1])
        if e == a or ke == ka:
            continue
        if base is not None and b not in only:
            bq, bk, bv, bo = base
            same = all(torch.equal(x[s0:s1].view(torch.int32), y[s0:s1].view(torch.int32))
                       for x, y, s0, s1 in ((q, bq, a, e), (k, bk, ka, ke), (v, bv, ka, ke)))
            assert same, "a sequence outside `only` has other operands than the base"
            out[a:e] = bo[a:e]
            continue
        out[a:e] = _attention_ref_seq(c, q[a:e], k[ka:ke], v[ka:ke], q_log2)
    return out


@functools.lru_cache(maxsize=None)
def _clean_ref(name: str, q_log2: bool):
    c = ATTN_BY_NAME[name]
    qkv = operands(name, "bf16", q_log2)
    return qkv + (attention_ref(c, qkv, q_log2),)


@functools.lru_cache(maxsize=None)
def poisoned_ref(name: str, q_log2: bool, poison: str) -> torch.Tensor:
    """The float64 reference on the poisoned operands (bf16-valued ones: where a NaN or an Inf goes does not depend on the
    operand type).  Only the victim sequence is evaluated again; see attention_ref."""
    c = ATTN_BY_NAME[name]
    base = _clean_ref(name, q_log2)
    return attention_ref(c, poisoned(c, base[:3], poison), q_log2, base=base, only=(victim(c),))


def oracle_rows(c: NFCase, dtype: str, q_log2: bool) -> torch.Tensor:
    """The clean launch's yardstick: O.attention per sequence (the kernels' rounding points), as E.oracle_rows."""
    if c.name in E.CASES_BY_NAME:
        return E.oracle_rows(E.CASES_BY_NAME[c.name], dtype, q_log2, False)
    q, k, v = operands(c.name, dtype, q_log2)
    rnd = O.Rounding(dtype)
    H, dh = c.H, c.dh
    cu_q, cu_k = E.cu_of(c.ql), E.cu_of(c.kl)
    out = torch.zeros(q.shape[0], H * dh)
    for b in range(len(c.ql)):
        a, e, ka, ke = int(cu_q[b]), int(cu_q[b + 1]), int(cu_k[b]), int(cu_k[b + 1])
        if e > a and ke > ka:
            out[a:e] = O.attention(q[a:e].view(-1, H, dh), k[ka:ke].view(-1, H, dh), v[ka:ke].view(-1, H, dh), slopes_of(c), rnd,
                                   q_log2=q_log2).reshape(e - a, H * dh)
    return out


# ---------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------
EPILOGUES = ("bf16", "f32", "res", "geglu", "gelu_f32", "gelu_bf16")
OUT16_EPILOGUES = ("bf16", "geglu", "gelu_bf16")
# (path, M, N, K): the smallest shapes with a ragged last tile in M and N against the 64, 128 and 256 tiles, K = 128 for the
# persistent form (variant 22); rows 127 | 128 sit either side of a tile boundary.  GEGLU takes N = 224 (N % 32 == 0).
GEMM_PATHS = [("v0", 270, 200, 128), ("v1", 270, 200, 128), ("v5", 270, 200, 128), ("v20", 270, 200, 128), ("v22", 270, 200, 128),
              ("generic", 77, 40, 72)]
GEGLU_N = {200: 224, 40: 96}
LN_M, LN_N, LN_K = 270, 224, 128          # LayerNorm consumer / producers (a producer needs N % 32 == 0)


def variant_of(path: str) -> int:
    return 0 if path in ("v0", "generic") else int(path[1:])


def gemm_rows(M: int):
    """m*: M - 1 (the row the clamped loads replicate into the rows >= M of the last tile) and 127 | 128 where M allows."""
    return [m for m in (M - 1, 127, 128) if m < M]


def gemm_operands(M, N, K, dtype: str, seed: int = 700):
    """a [M, K], w [N, K] (values of the operand type), bias [N] fp32, residual [M, N] fp32."""
    rd = (lambda t: t.to(tdt(dtype)).float())
    return (rd(_rand((M, K), seed)), rd(_rand((N, K), seed + 1, 1.0 / math.sqrt(K))), _rand((N,), seed + 2, 0.5),
            _rand((M, N), seed + 3))


def gemm_ref(a, w, bias, res, epi: str) -> torch.Tensor:
    """float64: epilogue(a @ w^T + bias); "geglu": w / bias in the UNPACKED order [value rows | gate rows]."""
    y = a.double() @ w.double().t() + bias.double()
    if epi == "res":
        y = y + res.double()
    if epi in ("gelu_f32", "gelu_bf16"):
        y = torch.nn.functional.gelu(y)
    if epi == "geglu":
        x, gate = y.chunk(2, dim=-1)
        y = x * torch.nn.functional.gelu(gate)
    return y


def gemm_region(M, n_out, kind: str, m=None, n=None) -> torch.Tensor:
    """Closed form of the NaN sets: 'row' m (A), 'col' n (W, bias), 'elem' (m, n) (residual)."""
    r = torch.zeros((M, n_out), dtype=torch.bool)
    if kind == "row":
        r[m] = True
    elif kind == "col":
        r[:, n] = True
    else:
        r[m, n] = True
    return r


def ln_stats_ref(x: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """float64 [M, 2] (mean, rstd) of every row."""
    x = x.double()
    mean = x.mean(dim=1)
    var = ((x - mean[:, None]) ** 2).mean(dim=1)
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], dim=1)


def ln_consumer_ref(a16, stats, w, bias, colsum, epi: str) -> torch.Tensor:
    """float64 of the folded LayerNorm -> Linear: rstd * (a16 . w^T - mean * colsum) + bias; "geglu" as gemm_ref."""
    y = stats.double()[:, 1:2] * (a16.double() @ w.double().t() - stats.double()[:, 0:1] * colsum.double()[None]) + bias.double()
    if epi == "geglu":
        x, gate = y.chunk(2, dim=-1)
        y = x * torch.nn.functional.gelu(gate)
    return y


# ---------------------------------------------------------------------------------------------
# 16-bit store rounding: the special values of contract item 3
# ---------------------------------------------------------------------------------------------
def round16(v, dtype: str) -> torch.Tensor:
    return torch.as_tensor(v, dtype=torch.float32).to(tdt(dtype))


def special_values(dtype: str):
    """[(label, fp32 value)].  u = half a unit in the last place of the type at 1.0; the ties come at 1 and at 32 (the GELU
    epilogue only delivers values >= 16 unchanged).  No fp32 subnormals."""
    u = 2.0 ** -8 if dtype == "bf16" else 2.0 ** -11
    e = 2.0 ** -20                       # far below u, well inside fp32's 24 bits at 1 and at 32
    top = 3.3895313892515355e38 if dtype == "bf16" else 65504.0
    vals = []
    for base in (1.0, 32.0):
        vals += [(f"tie_down_to_even@{base:g}", base * (1 + u)), (f"tie_up_to_even@{base:g}", base * (1 + 3 * u)),
                 (f"just_above_tie@{base:g}", base * (1 + u + e)), (f"just_below_tie@{base:g}", base * (1 + u - e))]
    vals += [("minus_zero", -0.0), ("plus_inf", INF), ("minus_inf", -INF), ("nan", NAN), ("largest_finite", top),
             ("minus_largest_finite", -top), ("fp32_max", 3.4028234663852886e38)]
    if dtype == "fp16":
        vals += [("65519", 65519.0), ("65520", 65520.0), ("minus_65520", -65520.0), ("1e6", 1e6), ("minus_1e6", -1e6),
                 ("smallest_subnormal", 2.0 ** -24), ("subnormal_with_rounding", 3e-6), ("tie_to_zero", 2.0 ** -25),
                 ("normal_subnormal_boundary", 6.1e-5)]
    return [(name, float(np.float32(v))) for name, v in vals]


def special_tensor(dtype: str) -> torch.Tensor:
    return torch.tensor([v for _, v in special_values(dtype)], dtype=torch.float32)


def same_16bit(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Bit equality of two 16-bit tensors, any NaN equal to any NaN (the contract fixes "NaN", not its payload)."""
    g, w = got.cpu(), want.cpu()
    gn, wn = torch.isnan(g), torch.isnan(w)
    return bool(torch.equal(gn, wn) and torch.equal(g.view(torch.int16)[~gn], w.view(torch.int16)[~wn]))


# ---------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------
def model_batch():
    """The three-gene batch of the model-level test and a CRE token id that occurs in gene 1's valid window tokens only."""
    from variantformer_amd.utils.synthetic import TISSUES_54, make_batch
    batch = make_batch(5, [6, 5, 7], [3, 4, 2], [TISSUES_54[:4], [9, 33], TISSUES_54[5:8]], 200)
    ids = [set(s[~m].tolist()) for s, m in zip(batch["cre_sequences"], batch["cre_attention_masks"])]
    only1 = sorted(ids[1] - ids[0] - ids[2])
    assert only1, "no token id is private to gene 1"
    return batch, only1[0]

"""ALiBi x unequal query / key lengths: the geometries and seeded operands shared by tests/test_ops_edges_gpu.py (every
kernel family against the oracle, both alignments) and tests/test_oracle_alibi_cpu.py (which shows, on the oracle alone,
that these very operands tell a wrong alignment from the right one).  One entry per kernel family of launch_attn
(variantformer_amd/csrc/vf_attn.hip); `kernel` is the string vf_last_kernel(1) must report for it.

Every list holds a sequence with more queries than keys, one with sk - sq == 1 and one with sk == sq; in the registry
shape, whose single query per sequence cannot outnumber a non-empty key sequence, that is a sequence without keys."""
import functools
import math
from typing import NamedTuple

import numpy as np
import torch

from oracle import vf_oracle as O
from tests.helpers import _rand

INPUT_SCALE = 2.0            # q, k, v uniform in [-2, 2): the operands the attention tolerances of test_ops_gpu.py were set for


class AttnCase(NamedTuple):
    name: str
    dh: int
    H: int
    ql: tuple
    kl: tuple
    kernel: str
    q_log2: tuple            # the VF_ATTN_Q_LOG2 settings the case runs with
    seed: int


def _ragged(seed, n, q_range, k_range, q_head, k_head):
    """n lengths: the explicit heads (boundaries and the three required relations) followed by seeded draws."""
    rng = np.random.default_rng(seed)
    m = n - len(q_head)
    ql = list(q_head) + [int(x) for x in rng.integers(q_range[0], q_range[1] + 1, m)]
    kl = list(k_head) + [int(x) for x in rng.integers(k_range[0], k_range[1] + 1, m)]
    return tuple(ql), tuple(kl)


_BOTH = (True, False)
FWD64, FWD128 = "attn_fwd_kernel<64-query blocks>", "attn_fwd_kernel<128-query blocks>"
SHORT2_1, SHORT2_2, SHORT = "attn_short2_kernel<1 pass>", "attn_short2_kernel<2 passes>", "attn_short_kernel"

_q96, _k96 = _ragged(101, 130, (65, 128), (1, 200), (128, 65, 100, 127, 96, 66, 113), (1, 66, 100, 200, 128, 65, 64))
_q1p, _k1p = _ragged(102, 130, (1, 128), (1, 128), (128, 1, 64, 17, 100, 127, 33, 5), (128, 2, 65, 17, 3, 128, 1, 120))
_q2p, _k2p = _ragged(103, 130, (129, 256), (1, 256), (256, 129, 200, 192, 193, 255, 130), (256, 130, 201, 1, 64, 256, 65))
# one block per (sequence, head), dh <= 48: the three-blocks-per-CU LDS image of attn_short2_kernel holds key tiles of up to
# 224 rows (3 x 224 x (128 + 96) bytes <= 160 KiB); 225 ... 256 keys fall to attn_short_kernel, 3 query groups per wave up
# to 192 queries, 4 beyond
_SHORT2_Q, _SHORT2_K = (129, 192, 193, 256, 1, 17, 100, 64), (130, 0, 224, 100, 2, 17, 1, 65)

ATTN_EDGE_CASES = [
    # the last gene layer: one registry query per sequence against every token of the sequence (and one without any)
    AttnCase("registry", 48, 8, (1,) * 10, (201, 1, 2, 16, 17, 64, 65, 200, 129, 0), FWD64, (True,), 1100),
    AttnCase("fwd64_dh48", 48, 4, (10, 50, 7, 128, 1, 20, 33, 70), (9, 300, 64, 1, 77, 21, 33, 200), FWD64, _BOTH, 1110),
    AttnCase("fwd64_dh128", 128, 2, (130, 3, 20, 33), (40, 257, 21, 33), FWD64, _BOTH, 1120),
    AttnCase("fwd128_dh48", 48, 32, (300, 1, 50, 128, 129, 257, 64, 200, 20, 33, 256, 90),
             (100, 400, 1, 129, 128, 64, 65, 201, 21, 33, 300, 7), FWD128, _BOTH, 1130),
    AttnCase("fwd128_dh96", 96, 8, _q96, _k96, FWD128, _BOTH, 1140),
    AttnCase("short2_2pass_dh48", 48, 8, _SHORT2_Q, _SHORT2_K, SHORT2_2, _BOTH, 1150),
    AttnCase("short2_1pass_dh64", 64, 8, _q1p, _k1p, SHORT2_1, _BOTH, 1160),
    AttnCase("short2_1pass_dh32", 32, 8, _q1p, _k1p, SHORT2_1, _BOTH, 1170),
    AttnCase("short2_2pass_dh64", 64, 8, _q2p, _k2p, SHORT2_2, _BOTH, 1180),
    AttnCase("short_3groups", 48, 8, (192, 129, 150, 17, 1, 160), (256, 130, 150, 240, 2, 3), SHORT, _BOTH, 1190),
    AttnCase("short_4groups", 48, 8, (256, 193, 150, 17, 1, 160), (225, 194, 150, 256, 2, 3), SHORT, _BOTH, 1200),
    AttnCase("short2_2pass_dh40", 40, 8, _SHORT2_Q, _SHORT2_K, SHORT2_2, _BOTH, 1210),     # padded class 48
]
CASES_BY_NAME = {c.name: c for c in ATTN_EDGE_CASES}
CASE_PARAMS = [(c.name, ql2) for c in ATTN_EDGE_CASES for ql2 in c.q_log2]        # (name, q_log2): every operand set the GPU test runs on

for _c in ATTN_EDGE_CASES:
    _d = [k - q for q, k in zip(_c.ql, _c.kl)]
    assert len(_c.ql) == len(_c.kl) and 1 in _d and 0 in _d and min(_d) < 0, _c.name


def tolerance(dtype: str) -> dict:
    """The attention tolerances of tests/test_ops_gpu.py: 16-bit output + 16-bit P rounded at another running maximum."""
    return dict(rtol=2 ** -7, atol=6e-3) if dtype == "bf16" else dict(rtol=2 ** -9, atol=2e-3)


def cu_of(lens) -> torch.Tensor:
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)


@functools.lru_cache(maxsize=4)
def operands(name: str, dtype: str, q_log2: bool):
    """(q [tq, D], k [tk, D], v [tk, D]) fp32 tensors holding values of the operand type; with q_log2 the queries carry
    softmax_scale * log2(e) before their rounding, as a pre-scaled Wq hands them over."""
    c = CASES_BY_NAME[name]
    rnd = O.Rounding(dtype)
    D = c.H * c.dh
    q = _rand((sum(c.ql), D), c.seed, INPUT_SCALE)
    kv = rnd.r(_rand((sum(c.kl), 2 * D), c.seed + 1, INPUT_SCALE))
    q = rnd.r(q * (math.log2(math.e) / math.sqrt(c.dh))) if q_log2 else rnd.r(q)
    return q, kv[:, :D].contiguous(), kv[:, D:].contiguous()


def slopes_of(c: AttnCase) -> torch.Tensor:
    return torch.tensor(O.alibi_slopes(c.H), dtype=torch.float32)


def oracle_rows(c: AttnCase, dtype: str, q_log2: bool, q_at_start: bool, shift: int = 0) -> torch.Tensor:
    """O.attention per sequence on operands(...), [tq, D] fp32 (not yet rounded to the output type); zero rows where the
    key sequence is empty.  shift = 1 evaluates the bias with every query position WRONG BY ONE, through the oracle's own
    two alignments: a dummy query in front of a start-aligned sequence moves the others one position up, a dummy query
    behind an end-aligned sequence moves them one position down."""
    q, k, v = operands(c.name, dtype, q_log2)
    rnd = O.Rounding(dtype)
    H, dh = c.H, c.dh
    cu_q, cu_k = cu_of(c.ql), cu_of(c.kl)
    sl = slopes_of(c)
    out = torch.zeros(q.shape[0], H * dh)
    for b in range(len(c.ql)):
        a, e, ka, ke = int(cu_q[b]), int(cu_q[b + 1]), int(cu_k[b]), int(cu_k[b + 1])
        if e == a or ke == ka:
            continue
        qs = q[a:e].view(-1, H, dh)
        if shift:
            dummy = torch.zeros(1, H, dh)
            qs = torch.cat([dummy, qs] if q_at_start else [qs, dummy])
        o = O.attention(qs, k[ka:ke].view(-1, H, dh), v[ka:ke].view(-1, H, dh), sl, rnd, q_log2=q_log2, q_at_start=q_at_start)
        if shift:
            o = o[1:] if q_at_start else o[:-1]
        out[a:e] = o.reshape(e - a, H * dh)
    return out

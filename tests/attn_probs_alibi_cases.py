"""Operands and float64 references for vf_attn_probs_v2 (ALiBi, explicit query positions, a row map for the keys), shared by
tests/test_attn_probs_alibi_cpu.py and tests/test_attn_probs_alibi_gpu.py.

The operands are the planted-direction operands of tests/test_attn_probs_gpu.py (`Case` there: every row has a dominant key
in every head, a uniform map proves nothing), taken from that file so the two stay one recipe; this module adds the slopes of
layers.get_alibi_slopes(H), a position per selected row, and the reference with the bias -- and with each of the five ways of
getting the bias wrong that the CPU test shows the operands to discriminate."""
import math

import numpy as np
import torch

from tests.test_attn_probs_gpu import P_TOL as P_TOL_PLAIN
from tests.test_attn_probs_gpu import SENTINEL, Case, _cu

GEOMETRIES = [(32, 48), (8, 64), (4, 32), (2, 96), (2, 128)]
# (keys, selected rows) per sequence: the sequences of tests/test_attn_probs_gpu.py plus 201 keys (registry token + 200 chunks)
SEQS = [(300, 54), (33, 3), (0, 3), (1, 1), (31, 65), (32, 0), (63, 1), (64, 54), (65, 65), (201, 54)]
MUTATIONS = ("no_bias", "off_by_one", "q_pos_ignored", "sign_flipped", "end_aligned")
LOG2E = math.log2(math.e)

# max |P - P64| / rowmax(P64).  MEASURED: the largest value on MI355X over the whole parametrisation of
# tests/test_attn_probs_alibi_gpu.py::test_alibi_probs_against_float64 (1.080e-06, at H = 8, dh = 64, fp16 operands, scale applied
# by the kernel; the bias-free entry's figure is 6.9e-7: the biased logits reach magnitude ~360, where one fp32 ulp is 3e-5, but
# the keys that carry a row's weight are those whose biased logit is near the row maximum, and the error is taken relative to that
# maximum).  The limit is 4 x that (another compiler's fp32 summation order), and never above 1e-4: beyond it the arithmetic is
# not fp32.  P_TOL_PLAIN is the bias-free entry's limit (tests/test_attn_probs_gpu.py).
MEASURED = 1.1e-6
P_TOL = min(4 * MEASURED, 1e-4)
assert P_TOL <= 1e-4


def prob_err(P, P64):
    """max |P - P64| / rowmax(P64) over the rows that have keys."""
    rowmax = P64.max(dim=-1, keepdim=True).values
    ok = rowmax[..., 0] > 0
    return float(((P.double() - P64).abs() / rowmax.clamp_min(1e-300))[ok].max())


def plain_reference(case, qsel):
    """The float64 softmax WITHOUT a bias of an AlibiCase's operands (the reference of tests/test_attn_probs_gpu.py)."""
    return Case.reference(case, qsel)


class AlibiCase(Case):
    def __init__(self, H, dh, dtype, q_log2, seqs=SEQS, gain=1.0, seed=0):
        from variantformer_amd.seq2gene.modules.layers import get_alibi_slopes
        super().__init__(H, dh, dtype, q_log2, seqs=seqs, gain=gain, seed=seed)
        self.slopes = get_alibi_slopes(H).float().contiguous()
        g = torch.Generator().manual_seed(77 * H + dh + seed)
        pos = []
        for n, rows in zip(self.kl, self.rl):
            p = torch.randint(0, max(n, 1), (rows,), generator=g, dtype=torch.int32)
            if rows > 0:
                p[0] = 0
            if rows > 1:
                p[1] = max(n - 1, 0)
            pos.append(p)
        self.q_pos = torch.cat(pos).contiguous()

    def reference(self, qsel, k16=None, mutation=None, slopes=None, q_pos=None):
        """float64 softmax of the 16-bit operands with the fp32 slope values: P [R, H, max_k], log2-sum-exp [R, H].
        mutation: one of MUTATIONS -- a wrong bias, for the discrimination test."""
        H, dh = self.H, self.dh
        k16 = self.k16 if k16 is None else k16
        c = 1.0 if self.q_log2 else self.scale * LOG2E
        slopes = (self.slopes if slopes is None else slopes).double()
        q_pos = self.q_pos if q_pos is None else q_pos
        if mutation == "no_bias":
            slopes = torch.zeros_like(slopes)
        elif mutation == "sign_flipped":
            slopes = -slopes
        max_k = max(self.kl)
        P = torch.zeros(self.R, H, max_k, dtype=torch.float64)
        lse = torch.zeros(self.R, H, dtype=torch.float64)
        q64 = qsel.double().view(self.R, H, dh)
        k64 = k16[:, :self.D].double().view(-1, H, dh)
        for s in range(len(self.kl)):
            a, e, ka, ke = int(self.cu_rows[s]), int(self.cu_rows[s + 1]), int(self.cu_k[s]), int(self.cu_k[s + 1])
            if e > a and ke > ka:
                pos = q_pos[a:e].double()
                if mutation == "off_by_one":
                    pos = pos + 1
                elif mutation == "q_pos_ignored":
                    pos = torch.zeros_like(pos)
                elif mutation == "end_aligned":
                    pos = pos + ((ke - ka) - (e - a))
                dist = (pos[:, None] - torch.arange(ke - ka, dtype=torch.float64)[None, :]).abs()          # [rows, keys]
                S = torch.einsum("rhd,jhd->rhj", q64[a:e], k64[ka:ke]) * c - LOG2E * slopes[None, :, None] * dist[:, None, :]
                m = S.max(dim=-1, keepdim=True).values
                E = torch.exp2(S - m)
                l = E.sum(dim=-1, keepdim=True)
                P[a:e, :, :ke - ka] = E / l
                lse[a:e] = (m + torch.log2(l))[..., 0]
        return P, lse

    def run(self, ops, q16, mapped, per_head, k16=None, extra_cols=5, max_rows=None, max_k=None, cu_rows=None, cu_k=None,
            q_rows=None, slopes="own", q_pos="own", k_rows=None):
        """ops.attn_probs on the device; slopes / q_pos: "own" = the case's, None = not passed, or a tensor."""
        k16 = self.k16 if k16 is None else k16
        H, D = self.H, self.D
        cu_rows = self.cu_rows if cu_rows is None else cu_rows
        cu_k = self.cu_k if cu_k is None else cu_k
        if q_rows is None and mapped:
            q_rows = self.q_rows
        slopes = self.slopes if isinstance(slopes, str) else slopes
        q_pos = self.q_pos if isinstance(q_pos, str) else q_pos
        R = int(cu_rows[-1])
        max_k = max(self.kl) if max_k is None else max_k
        max_rows = max(self.rl) if max_rows is None else max_rows
        out = torch.full((R * (H if per_head else 1), max_k + extra_cols), SENTINEL, dtype=torch.float32, device="cuda")
        dq = q16.cuda()
        dq = dq[:, :D] if mapped else dq[:R, :D]
        dev = lambda t: None if t is None else t.cuda()        # noqa: E731
        got, stats = ops.attn_probs(dq, k16.cuda()[:, :D], cu_rows.cuda(), cu_k.cuda(), max_rows, max_k, H, self.dh,
                                    q_rows=dev(q_rows), q_log2=self.q_log2, per_head=per_head, scale=self.scale, out=out,
                                    slopes=dev(slopes), q_pos=dev(q_pos), k_rows=dev(k_rows))
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        return out.cpu(), stats.cpu()


def moved_share(P, P_mut, has_keys):
    """Per head: the share of the rows with keys that the mutation moves by more than 1e-3 of the row maximum."""
    rowmax = P.max(dim=-1).values.clamp_min(1e-300)
    moved = ((P_mut - P).abs().max(dim=-1).values / rowmax) > 1e-3            # [R, H]
    return moved[has_keys].double().mean(dim=0)


def rows_with_keys(case):
    return torch.tensor(np.repeat(np.array(case.kl) > 0, case.rl))


__all__ = ["AlibiCase", "GEOMETRIES", "MUTATIONS", "P_TOL", "P_TOL_PLAIN", "SENTINEL", "SEQS", "_cu", "moved_share", "plain_reference",
           "prob_err", "rows_with_keys"]

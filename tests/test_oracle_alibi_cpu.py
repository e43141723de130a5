"""The oracle's ALiBi alignments (oracle.vf_oracle.attention, q_at_start) without any kernel: against a float64 evaluation
of the formula in include/vf_hip.h written as plain loops, and -- on the very operands tests/test_ops_edges_gpu.py gives
the kernels -- the proof that a kernel with the wrong alignment could not pass there."""
import math

import numpy as np
import pytest
import torch

from oracle import vf_oracle as O
from tests import attn_edge_cases as E
from tests.helpers import _rand

EPS32 = 2.0 ** -24


def _brute(q, k, v, slopes, q_at_start, q_log2, p_round):
    """out[i, h, :] = softmax_j(scale * q[i,h,:].k[j,h,:] - slope[h] * |i + (sk - sq) - j|) v[j,h,:] (start alignment:
    |i - j|) in float64, one (h, i, j) at a time.  p_round (None or a torch dtype) restates where the oracle rounds the
    weights to the operand type.  Returns (out [sq, H, dh], largest |logit|)."""
    sq, H, dh = q.shape
    sk = k.shape[0]
    qd, kd, vd = q.double().numpy(), k.double().numpy(), v.double().numpy()
    out = np.zeros((sq, H, dh))
    s_max = 0.0
    for h in range(H):
        for i in range(sq):
            pos = i if q_at_start else i + (sk - sq)
            s = np.zeros(sk)
            for j in range(sk):
                dot = float(np.dot(qd[i, h], kd[j, h]))
                if q_log2:
                    s[j] = dot - float(slopes[h]) * math.log2(math.e) * abs(pos - j)
                else:
                    s[j] = dot / math.sqrt(dh) - float(slopes[h]) * abs(pos - j)
            s_max = max(s_max, float(np.abs(s).max()))
            if q_log2:
                p = np.exp2(s - math.ceil(s.max()))
            else:
                p = np.exp(s - s.max())
            pr = p if p_round is None else torch.from_numpy(p).float().to(p_round).double().numpy()
            den = pr.sum() if q_log2 else p.sum()          # the base-2 form divides by the sum of the ROUNDED weights
            out[i, h] = (pr[:, None] * vd[:, h]).sum(0) / den
    return out, s_max


@pytest.mark.parametrize("sq,sk", [(1, 37), (37, 1), (20, 21), (50, 17)])
@pytest.mark.parametrize("mode", [None, "bf16"])
@pytest.mark.parametrize("q_log2", [False, True])
def test_attention_alignments_equal_the_header_formula(sq, sk, mode, q_log2):
    H, dh = 4, 16
    rnd = O.Rounding(mode)
    slopes = torch.tensor(O.alibi_slopes(H), dtype=torch.float32)
    q = rnd.r(_rand((sq, H, dh), 7, 2.0) * (math.log2(math.e) / math.sqrt(dh) if q_log2 else 1.0))
    k, v = rnd.r(_rand((sk, H, dh), 8, 2.0)), rnd.r(_rand((sk, H, dh), 9, 2.0))
    for q_at_start in (False, True):
        got = O.attention(q, k, v, slopes, rnd, q_log2=q_log2, q_at_start=q_at_start).double().numpy()
        want, s_max = _brute(q, k, v, slopes, q_at_start, q_log2, None if mode is None else torch.bfloat16)
        # fp32 round-off of the oracle: the logit is a dh-term dot product plus the bias (error (dh + 4) eps32 max|s|, which the
        # exponential turns into a RELATIVE error of every weight), then sums over sk keys in the numerator and the
        # denominator (sk eps32 each); |out| <= max|v|.
        v_max = float(v.abs().max())
        tol = (2 * (dh + 4) * max(s_max, 1.0) + 2 * sk + 8) * EPS32 * v_max
        if mode is not None:
            # a weight whose fp32 value sits within that relative error of a bf16 rounding boundary may round the other way:
            # one bf16 ulp (2^-8) of that weight.  At most a few of the sk weights do; allow each of them half its share.
            tol += 2.0 ** -8 * v_max * min(1.0, 4.0 / sk)
        assert np.abs(got - want).max() <= tol, (sq, sk, mode, q_log2, q_at_start, float(np.abs(got - want).max()), tol)
    if sq != sk:                       # the two alignments are different functions on these inputs
        a = O.attention(q, k, v, slopes, rnd, q_log2=q_log2)
        b = O.attention(q, k, v, slopes, rnd, q_log2=q_log2, q_at_start=True)
        assert sk == 1 or float((a - b).abs().max()) > 1e-2


@pytest.mark.parametrize("sq,sk", [(33, 33), (20, 45)])
@pytest.mark.parametrize("q_log2", [False, True])
def test_attention_default_alignment_is_unchanged(sq, sk, q_log2):
    """The flag left out and the flag set to False are the same bits (one self-attention case, one cross case), and equal to
    the end-aligned expression the function evaluated before it had the flag (restated here for the plain branch)."""
    H, dh = 8, 48
    rnd = O.Rounding("bf16")
    slopes = torch.tensor(O.alibi_slopes(H), dtype=torch.float32)
    q, k, v = rnd.r(_rand((sq, H, dh), 17, 2.0)), rnd.r(_rand((sk, H, dh), 18, 2.0)), rnd.r(_rand((sk, H, dh), 19, 2.0))
    a = O.attention(q, k, v, slopes, rnd, q_log2)
    b = O.attention(q, k, v, slopes, rnd, q_log2, q_at_start=False)
    assert torch.equal(a, b)
    if sq == sk:
        assert torch.equal(a, O.attention(q, k, v, slopes, rnd, q_log2, q_at_start=True))
    if not q_log2:
        s = torch.einsum("qhd,khd->hqk", q, k) * (1.0 / math.sqrt(dh))
        i = torch.arange(sq)[:, None] + (sk - sq)
        j = torch.arange(sk)[None, :]
        s = s - slopes[:, None, None] * (i - j).abs().to(s.dtype)[None]
        p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
        o = torch.einsum("hqk,khd->hqd", rnd.r(p), v) / p.sum(dim=-1, keepdim=True)
        assert torch.equal(a, o.permute(1, 0, 2))


def _row_fraction(wrong, ref, c, tol):
    """Per head: the fraction of (query, head) rows in which `wrong` leaves the tolerance around `ref` somewhere."""
    bad = (wrong - ref).abs() > tol["atol"] + tol["rtol"] * ref.abs()
    return bad.view(-1, c.H, c.dh).any(-1).float().mean(0)


def one_position_floor(c, dtype):
    """The flattest slope at which an offset wrong by ONE position can leave the tolerance at all.  Such an offset multiplies
    the weight of every key on one side of the query by e^-slope and on the other side by e^+slope, so to first order the
    output moves by 2 slope W_l W_r (m_r - m_l) <= slope |m_r - m_l| / 2 (W: the weight either side holds, m: its mean of
    V).  The means of several values uniform in [-scale, scale) differ by about scale / 2 at most, so the output moves by
    about slope scale / 4: under atol for slope < 4 atol / scale whatever the lengths (the gap sk - sq does not enter).
    With ONE query per sequence every key lies on the same side: the shift changes all biases alike except between the two
    nearest keys, whose weights are about `slope` each in a steep head -- the output moves by about slope^2 scale, over atol
    from slope = sqrt(atol / scale).  These are first-order estimates, and where above them a QUARTER of the rows is
    reached is not derived: the factor 8 (twice the estimate) was chosen from the measured fractions -- at bf16 the head
    of slope 2^-6, between 4 and 8 atol / scale, reaches 0.20 ... 0.45 depending on the case, every head from
    8 atol / scale up reaches 0.4 or more in every case, the heads below 2^-6 stay under 0.15.  Flatter heads are outside what any check at
    these tolerances can see of a single position (two keys bound the shift by 2 slope); a kernel's offset error is the
    same in every head, so the steep heads show it.  The opposite alignment (the gap times the slope) is asserted in EVERY
    head."""
    atol = E.tolerance(dtype)["atol"]
    if max(c.ql) == 1:
        return math.sqrt(atol / E.INPUT_SCALE)
    return 8 * atol / E.INPUT_SCALE


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name,q_log2", E.CASE_PARAMS)
def test_edge_case_operands_tell_the_alignments_apart(name, q_log2, dtype):
    """On every operand set tests/test_ops_edges_gpu.py runs on (the queries pre-scaled for VF_ATTN_Q_LOG2 are other tensors
    than the plain ones), at its tolerances: the oracle with the OPPOSITE alignment is outside the tolerance in at least a
    quarter of the rows of EVERY head, for both alignments; with the offset wrong by one position, in a quarter of the rows
    of every head at or above one_position_floor()."""
    c = E.CASES_BY_NAME[name]
    rnd = O.Rounding(dtype)
    tol = E.tolerance(dtype)
    right = {s: rnd.r(E.oracle_rows(c, dtype, q_log2, s)) for s in (False, True)}
    slopes = E.slopes_of(c)
    steep = slopes >= one_position_floor(c, dtype)
    assert int(steep.sum()) >= 1
    for s in (False, True):
        opposite = _row_fraction(right[not s], right[s], c, tol)
        by_one = _row_fraction(rnd.r(E.oracle_rows(c, dtype, q_log2, s, shift=1)), right[s], c, tol)
        fractions = (name, q_log2, dtype, s, [round(float(x), 2) for x in opposite], [round(float(x), 2) for x in by_one])
        assert float(opposite.min()) >= 0.25, fractions
        assert float(by_one[steep].min()) >= 0.25, (fractions, steep.tolist())

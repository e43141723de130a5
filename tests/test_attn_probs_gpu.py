"""ops.attn_probs (vf_attn_probs): the fp32 softmax probabilities of selected query rows, against a float64 softmax of the
same 16-bit q and k computed in torch on the CPU.  Every geometry with a kernel of its own, both operand types, both logit
forms; ragged key tiles, row tiles and empty sequences; strided operands, a wider output with sentinels; logits of magnitude
300; batch independence, determinism and non-finite containment, all on operands whose maps are SELECTIVE (a uniform map
cannot tell a correct kernel from 1 / N)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
GEOMETRIES = [(32, 48), (8, 64), (4, 32), (2, 96), (2, 128)]
# (keys, selected rows) per sequence: every key length of {0, 1, 31, 32, 33, 63, 64, 65, 300} (empty, one key, around the
# 32-key tile of pass 1 and the 64-key tile of pass 2, several tiles) and every row count of {0, 1, 3, 54, 65} (none, one
# tile, more than the 32-row and the 64-row tile)
SEQS = [(300, 54), (33, 3), (0, 3), (1, 1), (31, 65), (32, 0), (63, 1), (64, 54), (65, 65)]
SENTINEL = -7.0
# max |P - P64| / rowmax(P64).  MEASURED: the largest value on MI355X over the whole parametrisation below (6.871e-07, at H = 2,
# dh = 96; the magnitude-300 cases are one-hot to 1e-33).  The limit is 4 x that (another compiler's fp32 summation order), and
# may never exceed 1e-4: one 16-bit rounding of P or of the logits shows at >= 1e-3, so anything above 1e-4 is not fp32 arithmetic.
MEASURED = 6.9e-7
P_TOL = min(4 * MEASURED, 1e-4)
assert P_TOL <= 1e-4


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from variantformer_amd import ops as _ops
    return _ops


def _cu(lens):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)


class Case:
    """Operands with structure: per (sequence, head) a unit direction u; every query of the sequence is alpha * u + noise,
    three of its keys are beta * u (beta = 6, 3, -6 times `gain`), the other keys are noise.  The planted keys' base-2 logits
    are then about +-6 alpha gain against |logit| ~ 1 elsewhere: every row has a dominant key.
    q lives in the first D columns of a [rows, 3D] buffer, k in the first D columns of a [keys, 2D] K|V buffer."""

    def __init__(self, H, dh, dtype, q_log2, seqs=SEQS, gain=1.0, seed=0):
        g = torch.Generator().manual_seed(1000 * H + dh + seed)
        self.H, self.dh, self.D, self.q_log2 = H, dh, H * dh, q_log2
        D = self.D
        self.kl, self.rl = [s[0] for s in seqs], [s[1] for s in seqs]
        self.cu_k, self.cu_rows = _cu(self.kl), _cu(self.rl)
        self.R, Tk = sum(self.rl), sum(self.kl)
        self.Tq = self.R + 7
        # with the scale applied by the kernel (q_log2 off) the operands carry sqrt(dh) / log2(e) more, for the same logits
        self.scale = 1.0 / math.sqrt(dh)
        amp = 1.0 if q_log2 else math.sqrt(1.0 / (self.scale * math.log2(math.e)))
        perm = torch.randperm(self.Tq, generator=g)[:self.R].contiguous()
        if self.rl[0] > 40:
            perm[40] = perm[5]                                      # a repeated query row (both in sequence 0)
        self.q_rows = perm.long()
        q = torch.zeros(self.Tq, 3 * D)
        k = torch.zeros(max(Tk, 1), 2 * D)
        k[:, D:] = torch.randn(max(Tk, 1), D, generator=g)          # the V half: never read
        q[:, D:] = torch.randn(self.Tq, 2 * D, generator=g)
        seq_of_row = np.repeat(np.arange(len(seqs)), self.rl)
        u = torch.randn(len(seqs), H, dh, generator=g)
        u = u / u.norm(dim=-1, keepdim=True)
        alpha = 1.0 + torch.rand(self.Tq, H, 1, generator=g)
        qd = 0.3 * torch.randn(self.Tq, H, dh, generator=g) / math.sqrt(dh)
        # query row q_rows[r] serves selected row r of sequence seq_of_row[r] (the NULL-map call reads rows 0 .. R-1 instead:
        # both get the direction of the sequence they serve in THAT call through `direction_rows`)
        self._alpha, self._qd, self._u, self._seq_of_row, self._amp, self._gain = alpha, qd, u, seq_of_row, amp, gain
        kk = 0.5 * torch.randn(max(Tk, 1), H, dh, generator=g)
        self.planted = {}
        for s, n in enumerate(self.kl):
            a = int(self.cu_k[s])
            js = sorted(set(int(j) for j in (n // 2, 0, n - 1)))[:3] if n else []
            for j, beta in zip(js, (6.0, 3.0, -6.0)):
                kk[a + j] = beta * gain * u[s]
            self.planted[s] = js
        k[:, :D] = (kk * amp).reshape(-1, D)
        self._k32 = k
        self.dtype = TDT[dtype]
        self.k16 = k.to(self.dtype)
        self._q_template = q

    def queries(self, mapped: bool):
        """(16-bit q buffer [Tq, 3D], the selected queries [R, D] as fp32 of the 16-bit values)."""
        H, dh, D = self.H, self.dh, self.D
        q = self._q_template.clone()
        rows = self.q_rows if mapped else torch.arange(self.R)
        qq = torch.zeros(self.Tq, H, dh)
        for r in range(self.R):
            qq[rows[r]] = self._alpha[rows[r]] * self._u[self._seq_of_row[r]] * self._gain + self._qd[rows[r]]
        q[:, :D] = (qq * self._amp).reshape(-1, D)
        q16 = q.to(self.dtype)
        return q16, q16[rows][:, :D].float()

    def reference(self, qsel, k16=None):
        """float64 softmax of the 16-bit operands: P [R, H, max_k] (zeros past a sequence's keys), log2-sum-exp [R, H]."""
        H, dh = self.H, self.dh
        k16 = self.k16 if k16 is None else k16
        c = 1.0 if self.q_log2 else self.scale * math.log2(math.e)
        max_k = max(self.kl)
        P = torch.zeros(self.R, H, max_k, dtype=torch.float64)
        lse = torch.zeros(self.R, H, dtype=torch.float64)
        q64 = qsel.double().view(self.R, H, dh)
        k64 = k16[:, :self.D].double().view(-1, H, dh)
        for s in range(len(self.kl)):
            a, e, ka, ke = int(self.cu_rows[s]), int(self.cu_rows[s + 1]), int(self.cu_k[s]), int(self.cu_k[s + 1])
            if e > a and ke > ka:
                S = torch.einsum("rhd,jhd->rhj", q64[a:e], k64[ka:ke]) * c
                m = S.max(dim=-1, keepdim=True).values
                E = torch.exp2(S - m)
                l = E.sum(dim=-1, keepdim=True)
                P[a:e, :, :ke - ka] = E / l
                lse[a:e] = (m + torch.log2(l))[..., 0]
        return P, lse

    def run(self, ops, q16, mapped, per_head, k16=None, extra_cols=5, max_rows=None, max_k=None, cu_rows=None, cu_k=None,
            q_rows=None):
        k16 = self.k16 if k16 is None else k16
        H, D = self.H, self.D
        cu_rows = self.cu_rows if cu_rows is None else cu_rows
        cu_k = self.cu_k if cu_k is None else cu_k
        if q_rows is None and mapped:
            q_rows = self.q_rows
        R = int(cu_rows[-1])
        max_k = max(self.kl) if max_k is None else max_k
        max_rows = max(self.rl) if max_rows is None else max_rows
        out = torch.full((R * (H if per_head else 1), max_k + extra_cols), SENTINEL, dtype=torch.float32, device="cuda")
        dq = q16.cuda()
        dq = dq[:, :D] if mapped else dq[:R, :D]
        got, stats = ops.attn_probs(dq, k16.cuda()[:, :D], cu_rows.cuda(), cu_k.cuda(), max_rows, max_k, H, self.dh,
                                    q_rows=None if q_rows is None else q_rows.cuda(), q_log2=self.q_log2, per_head=per_head,
                                    scale=self.scale, out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        return out.cpu(), stats.cpu()


def _err(P, P64):
    """max |P - P64| / rowmax(P64) over the rows that have keys."""
    rowmax = P64.max(dim=-1, keepdim=True).values
    ok = rowmax[..., 0] > 0
    return float(((P.double() - P64).abs() / rowmax.clamp_min(1e-300))[ok].max())


def _check_layout(case, out, P64, per_head):
    """Sentinels beyond max_k, zeros between a sequence's keys and max_k, values against the reference; returns the error."""
    H, max_k = case.H, max(case.kl)
    assert torch.all(out[:, max_k:] == SENTINEL), "columns >= max_seqlen_k were written"
    body = out[:, :max_k]
    assert torch.isfinite(body).all()
    got = body.view(case.R, H, max_k) if per_head else body
    want = P64 if per_head else P64.mean(dim=1)
    for s, n in enumerate(case.kl):
        a, e = int(case.cu_rows[s]), int(case.cu_rows[s + 1])
        assert torch.all(got[a:e][..., n:] == 0.0), f"sequence {s}: columns past its {n} keys are not zero"
    return _err(got, want)


@pytest.mark.parametrize("q_log2", [True, False], ids=["qlog2", "scaled"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("H,dh", GEOMETRIES)
def test_probs_against_float64(ops, H, dh, dtype, q_log2):
    case = Case(H, dh, dtype, q_log2)
    worst = 0.0
    for mapped in (True, False):
        q16, qsel = case.queries(mapped)
        P64, lse64 = case.reference(qsel)
        # structure: every row over enough keys for the bound to be satisfiable (10 / N < 1) has a dominant key in every head
        for s, n in enumerate(case.kl):
            a, e = int(case.cu_rows[s]), int(case.cu_rows[s + 1])
            if n > 10 and e > a:
                assert float(P64[a:e].max(dim=-1).values.min()) > 10.0 / n, f"sequence {s}: the reference map is not selective"
        ph, stats = case.run(ops, q16, mapped, per_head=True)
        hm, stats2 = case.run(ops, q16, mapped, per_head=False)
        e_ph, e_hm = _check_layout(case, ph, P64, True), _check_layout(case, hm, P64, False)
        print(f"[attn_probs] H={H} dh={dh} {dtype} q_log2={q_log2} mapped={mapped}: per-head err {e_ph:.3e}, head-mean err {e_hm:.3e}")
        worst = max(worst, e_ph, e_hm)
        assert torch.equal(stats, stats2)
        max_k = max(case.kl)
        mean_of_heads = ph[:, :max_k].view(case.R, H, max_k).double().mean(dim=1)
        assert float((hm[:, :max_k].double() - mean_of_heads).abs().max()) <= H * 2.0 ** -24      # fp32 sum of H values <= 1
        has_keys = torch.tensor(np.repeat(np.array(case.kl) > 0, case.rl))
        lse = stats[..., 0].double() + torch.log2(stats[..., 1].double())
        assert float((lse - lse64)[has_keys].abs().max()) < 1e-4 * max(1.0, float(lse64.abs().max()))
        assert torch.all(stats[~has_keys] == 0.0)                         # a row without keys: stats (0, 0)
    assert worst <= P_TOL, f"max |P - P64| / rowmax = {worst:.3e} > {P_TOL:.1e}"
    assert ops.last_kernel("attn") == "attn_probs_kernel"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_logits_of_magnitude_300(ops, dtype):
    """alpha * beta * gain reaches +-300 and beyond: exp2 of the raw logit would overflow; the result stays finite and correct
    and m + log2 l is the reference's log2-sum-exp."""
    H, dh = 32, 48
    case = Case(H, dh, dtype, True, seqs=[(300, 54), (65, 3), (33, 1)], gain=5.5)
    q16, qsel = case.queries(True)
    P64, lse64 = case.reference(qsel)
    S = torch.einsum("rhd,jhd->rhj", qsel[:54].double().view(54, H, dh), case.k16[:300, :case.D].double().view(300, H, dh))
    assert float(S.max()) > 300 and float(S.min()) < -300
    ph, stats = case.run(ops, q16, True, per_head=True)
    hm, _ = case.run(ops, q16, True, per_head=False)
    assert torch.isfinite(stats).all()
    e_ph, e_hm = _check_layout(case, ph, P64, True), _check_layout(case, hm, P64, False)
    print(f"[attn_probs] magnitude 300 {dtype}: per-head err {e_ph:.3e}, head-mean err {e_hm:.3e}")
    assert max(e_ph, e_hm) <= P_TOL
    lse = stats[..., 0].double() + torch.log2(stats[..., 1].double())
    # an fp32 dot product of dh terms whose magnitudes sum to ~|logit|: <= dh * 2^-24 * 400 absolute
    assert float((lse - lse64).abs().max()) <= dh * 2.0 ** -24 * 400


def test_rows_do_not_depend_on_the_rest_of_the_call(ops):
    """The bits of a row: the same run to run, with other sequences removed, and with max_rows / max_seqlen_k raised."""
    H, dh = 32, 48
    case = Case(H, dh, "bf16", True)
    q16, _ = case.queries(True)
    max_k = max(case.kl)
    for per_head in (False, True):
        n_out = H if per_head else 1
        a, _ = case.run(ops, q16, True, per_head)
        b, _ = case.run(ops, q16, True, per_head)
        assert torch.equal(a, b)
        keep = [0, 4, 8]                                                  # sequences kept, with their own rows and keys
        cu_rows, cu_k = _cu([case.rl[s] for s in keep]), _cu([case.kl[s] for s in keep])
        rows = torch.cat([torch.arange(int(case.cu_rows[s]), int(case.cu_rows[s + 1])) for s in keep])
        keys = torch.cat([torch.arange(int(case.cu_k[s]), int(case.cu_k[s + 1])) for s in keep])
        c, _ = case.run(ops, q16, True, per_head, k16=case.k16[keys].contiguous(), cu_rows=cu_rows, cu_k=cu_k,
                        q_rows=case.q_rows[rows].contiguous(), max_rows=max(case.rl) + 70, max_k=max_k + 100)
        want = a.view(case.R, n_out, -1)[rows][..., :max_k]
        got = c.view(len(rows), n_out, -1)
        assert torch.equal(got[..., :max_k], want)
        assert torch.all(got[..., max_k:max_k + 100] == 0.0) and torch.all(got[..., max_k + 100:] == SENTINEL)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_nan_stays_in_its_sequence_and_row(ops, dtype):
    H, dh = 8, 64
    case = Case(H, dh, dtype, True)
    q16, _ = case.queries(True)
    max_k = max(case.kl)
    clean_ph, _ = case.run(ops, q16, True, True)
    clean_hm, _ = case.run(ops, q16, True, False)
    k_bad, q_bad = case.k16.clone(), q16.clone()
    k_bad[17, 3 * dh + 5] = float("nan")                                  # a K row of sequence 0, head 3
    bad_row = int(case.cu_rows[1]) + 1                                    # a selected row of sequence 1 ...
    q_bad[case.q_rows[bad_row], 6 * dh + 1] = float("nan")                # ... its query, head 6
    hit = (case.q_rows == case.q_rows[bad_row]).nonzero().flatten().tolist()      # (every selected row that reads this query)
    ph, _ = case.run(ops, q_bad, True, True, k16=k_bad)
    hm, _ = case.run(ops, q_bad, True, False, k16=k_bad)
    ph, clean = ph[:, :max_k].view(case.R, H, max_k), clean_ph[:, :max_k].view(case.R, H, max_k)
    n0 = case.rl[0]
    assert torch.isnan(ph[:n0, 3, :case.kl[0]]).all() and torch.isnan(hm[:n0, :case.kl[0]]).all()
    same = torch.ones(case.R, H, dtype=torch.bool)
    same[:n0, 3] = False
    for r in hit:
        s = int(np.searchsorted(case.cu_rows.numpy(), r, side="right") - 1)
        assert torch.isnan(ph[r, 6, :case.kl[s]]).all() and torch.isnan(hm[r, :case.kl[s]]).all()
        same[r, 6] = False
    assert torch.equal(ph[same], clean[same])
    rows_same = same.all(dim=1)
    assert torch.equal(hm[rows_same], clean_hm[rows_same])
    assert torch.all(ph[:n0, 3, case.kl[0]:] == 0.0)                      # masked columns stay 0 beside the NaN

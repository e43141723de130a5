"""ops.attn_probs with ALiBi, explicit query positions and a row map for the keys (vf_attn_probs_v2), against a float64 softmax
of the same 16-bit operands with the fp32 slope values, computed in torch on the CPU.  Every geometry with a kernel of its own,
both operand types, both logit forms, head mean and per head, on the selective operands of tests/attn_probs_alibi_cases.py
(tests/test_attn_probs_alibi_cpu.py shows that they tell every wrong bias from the right one); then the bit-identities of the
contract, the non-finite containment and the refusals."""
import numpy as np
import pytest
import torch

from tests.attn_probs_alibi_cases import GEOMETRIES, P_TOL, SENTINEL, AlibiCase, _cu, rows_with_keys
from tests.attn_probs_alibi_cases import prob_err as _err              # (the limit and its measurement are stated there)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from variantformer_amd import ops as _ops
    return _ops


def _check_layout(case, out, P64, per_head):
    """Sentinels beyond max_k, zeros between a sequence's keys and max_k, row sums, values against the reference -> the error."""
    H, max_k = case.H, max(case.kl)
    assert torch.all(out[:, max_k:] == SENTINEL), "columns >= max_seqlen_k were written"
    body = out[:, :max_k]
    assert torch.isfinite(body).all()
    got = body.view(case.R, H, max_k) if per_head else body
    want = P64 if per_head else P64.mean(dim=1)
    for s, n in enumerate(case.kl):
        a, e = int(case.cu_rows[s]), int(case.cu_rows[s + 1])
        assert torch.all(got[a:e][..., n:] == 0.0), f"sequence {s}: columns past its {n} keys are not zero"
    has_keys = rows_with_keys(case)
    assert float((got.double().sum(dim=-1)[has_keys] - 1.0).abs().max()) <= 1e-5, "row sums"
    assert torch.all(got[~has_keys] == 0.0)
    return _err(got, want)


@pytest.mark.parametrize("q_log2", [True, False], ids=["qlog2", "scaled"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("H,dh", GEOMETRIES)
def test_alibi_probs_against_float64(ops, H, dh, dtype, q_log2):
    case = AlibiCase(H, dh, dtype, q_log2)
    q16, qsel = case.queries(True)
    P64, lse64 = case.reference(qsel)
    ph, stats = case.run(ops, q16, True, per_head=True)
    assert ops.last_kernel("attn") == "attn_probs_alibi_kernel"
    hm, stats2 = case.run(ops, q16, True, per_head=False)
    e_ph, e_hm = _check_layout(case, ph, P64, True), _check_layout(case, hm, P64, False)
    print(f"[attn_probs_alibi] H={H} dh={dh} {dtype} q_log2={q_log2}: per-head err {e_ph:.3e}, head-mean err {e_hm:.3e}")
    assert torch.equal(stats, stats2)
    max_k = max(case.kl)
    mean_of_heads = ph[:, :max_k].view(case.R, H, max_k).double().mean(dim=1)
    assert float((hm[:, :max_k].double() - mean_of_heads).abs().max()) <= H * 2.0 ** -24      # fp32 sum of H values <= 1
    has_keys = rows_with_keys(case)
    lse = stats[..., 0].double() + torch.log2(stats[..., 1].double())
    assert float((lse - lse64)[has_keys].abs().max()) < 1e-4 * max(1.0, float(lse64.abs().max()))
    assert torch.all(stats[~has_keys] == 0.0)                             # a row without keys: stats (0, 0)
    assert max(e_ph, e_hm) <= P_TOL, f"max |P - P64| / rowmax = {max(e_ph, e_hm):.3e} > {P_TOL:.1e}"


def test_null_positions_are_position_zero(ops):
    case = AlibiCase(32, 48, "bf16", True)
    q16, _ = case.queries(True)
    for per_head in (False, True):
        a, sa = case.run(ops, q16, True, per_head, q_pos=None)
        b, sb = case.run(ops, q16, True, per_head, q_pos=torch.zeros(case.R, dtype=torch.int32))
        c, _ = case.run(ops, q16, True, per_head)
        assert torch.equal(a, b) and torch.equal(sa, sb)
        assert not torch.equal(a, c)                                      # and the positions of the case are not all 0


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_all_null_v2_is_vf_attn_probs(ops, dtype):
    """vf_attn_probs (called directly) and vf_attn_probs_v2 with three NULLs (ops.attn_probs without the new arguments)."""
    from variantformer_amd import _lib
    lib = _lib.load()
    case = AlibiCase(8, 64, dtype, True)
    q16, _ = case.queries(True)
    H, D, max_k = case.H, case.D, max(case.kl)
    q, k = q16.cuda(), case.k16.cuda()
    cu_rows, cu_k, q_rows = case.cu_rows.cuda(), case.cu_k.cuda(), case.q_rows.cuda()
    for per_head in (False, True):
        new, new_stats = case.run(ops, q16, True, per_head, slopes=None, q_pos=None)
        assert ops.last_kernel("attn") == "attn_probs_kernel"
        out = torch.full_like(new, SENTINEL, device="cuda")
        stats = torch.empty((case.R, H, 2), dtype=torch.float32, device="cuda")
        rc = lib.vf_attn_probs(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), q_rows.data_ptr(), cu_rows.data_ptr(),
                               cu_k.data_ptr(), len(case.kl), max(case.rl), max_k, H, case.dh, case.scale, _lib.VF_BF16 if
                               dtype == "bf16" else _lib.VF_F16, 2, int(per_head), stats.data_ptr(), out.data_ptr(), out.stride(0),
                               torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.vf_last_error()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), new) and torch.equal(stats.cpu(), new_stats)


@pytest.mark.parametrize("with_bias", [True, False], ids=["alibi", "nobias"])
def test_key_row_map_equals_the_gathered_keys(ops, with_bias):
    """K as a table of distinct rows read through k_rows (rows repeat: the tissue copies of a gene share their chunk rows)
    against the same call on the gathered rows."""
    case = AlibiCase(32, 48, "bf16", True)
    q16, _ = case.queries(True)
    g = torch.Generator().manual_seed(5)
    Tk = sum(case.kl)
    table = case.k16[torch.randperm(Tk, generator=g)[:Tk // 3]].contiguous()
    k_rows = torch.randint(0, table.shape[0], (Tk,), generator=g, dtype=torch.int64)
    assert len(set(k_rows.tolist())) < Tk                                 # rows repeat
    gathered = table[k_rows].contiguous()
    kw = {} if with_bias else {"slopes": None, "q_pos": None}
    for per_head in (False, True):
        a, sa = case.run(ops, q16, True, per_head, k16=table, k_rows=k_rows, **kw)
        b, sb = case.run(ops, q16, True, per_head, k16=gathered, **kw)
        assert torch.equal(a, b) and torch.equal(sa, sb)


def test_rows_do_not_depend_on_the_rest_of_the_call(ops):
    """The bits of a row: the same run to run, and with the other sequences removed and max_rows / max_seqlen_k raised."""
    case = AlibiCase(32, 48, "bf16", True)
    q16, _ = case.queries(True)
    H, max_k = case.H, max(case.kl)
    for per_head in (False, True):
        n_out = H if per_head else 1
        a, _ = case.run(ops, q16, True, per_head)
        b, _ = case.run(ops, q16, True, per_head)
        assert torch.equal(a, b)
        for keep in ([9], [0, 4, 9]):                                     # a sequence alone; three of them
            cu_rows, cu_k = _cu([case.rl[s] for s in keep]), _cu([case.kl[s] for s in keep])
            rows = torch.cat([torch.arange(int(case.cu_rows[s]), int(case.cu_rows[s + 1])) for s in keep])
            keys = torch.cat([torch.arange(int(case.cu_k[s]), int(case.cu_k[s + 1])) for s in keep])
            c, _ = case.run(ops, q16, True, per_head, k16=case.k16[keys].contiguous(), cu_rows=cu_rows, cu_k=cu_k,
                            q_rows=case.q_rows[rows].contiguous(), q_pos=case.q_pos[rows].contiguous(),
                            max_rows=max(case.rl) + 70, max_k=max_k + 100)
            want = a.view(case.R, n_out, -1)[rows][..., :max_k]
            got = c.view(len(rows), n_out, -1)
            assert torch.equal(got[..., :max_k], want)
            assert torch.all(got[..., max_k:max_k + 100] == 0.0) and torch.all(got[..., max_k + 100:] == SENTINEL)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_non_finite_operands_stay_where_they_are(ops, dtype):
    """Each against the clean launch's bits: a NaN slope (its head, every row with keys, no other head); a NaN K row reached
    through k_rows by one sequence only (that sequence's head); a NaN query (its row's head)."""
    H, dh = 8, 64
    case = AlibiCase(H, dh, dtype, True)
    q16, _ = case.queries(True)
    max_k = max(case.kl)
    has_keys = rows_with_keys(case)
    Tk = sum(case.kl)
    table = torch.cat([case.k16, case.k16[:1]])                           # one more row: the one that will hold the NaN
    k_rows = torch.arange(Tk, dtype=torch.int64)
    view = lambda t: t[:, :max_k].view(case.R, H, max_k)                  # noqa: E731
    clean_ph, _ = case.run(ops, q16, True, True, k16=table, k_rows=k_rows)
    clean_hm, _ = case.run(ops, q16, True, False, k16=table, k_rows=k_rows)
    clean = view(clean_ph)

    def valid(r):                                                         # the columns of row r that hold keys
        return case.kl[int(np.searchsorted(case.cu_rows.numpy(), r, side="right") - 1)]

    def check(ph, hm, bad):
        """bad [R, H]: the (row, head) pairs that must be NaN over their keys and 0 behind them; the rest keeps its bits."""
        ph = view(ph)
        for r, h in bad.nonzero().tolist():
            n = valid(r)
            assert torch.isnan(ph[r, h, :n]).all() and torch.all(ph[r, h, n:] == 0.0)
            assert torch.isnan(hm[r, :n]).all()
        assert torch.equal(ph[~bad], clean[~bad])
        rows_same = ~bad.any(dim=1)
        assert torch.equal(hm[rows_same], clean_hm[rows_same])

    # a NaN slope on head 5
    slopes = case.slopes.clone()
    slopes[5] = float("nan")
    bad = torch.zeros(case.R, H, dtype=torch.bool)
    bad[has_keys, 5] = True
    check(case.run(ops, q16, True, True, k16=table, k_rows=k_rows, slopes=slopes)[0],
          case.run(ops, q16, True, False, k16=table, k_rows=k_rows, slopes=slopes)[0], bad)

    # a NaN K row (head 3) that only sequence 9 reaches, through its key 17
    t_bad, kr = table.clone(), k_rows.clone()
    t_bad[Tk] = case.k16[int(case.cu_k[9]) + 17]
    t_bad[Tk, 3 * dh + 5] = float("nan")
    kr[int(case.cu_k[9]) + 17] = Tk
    bad = torch.zeros(case.R, H, dtype=torch.bool)
    bad[int(case.cu_rows[9]):int(case.cu_rows[10]), 3] = True
    check(case.run(ops, q16, True, True, k16=t_bad, k_rows=kr)[0], case.run(ops, q16, True, False, k16=t_bad, k_rows=kr)[0], bad)

    # a NaN query: a selected row of sequence 1, head 6 (and every selected row that reads the same query row)
    q_bad = q16.clone()
    bad_row = int(case.cu_rows[1]) + 1
    q_bad[case.q_rows[bad_row], 6 * dh + 1] = float("nan")
    bad = torch.zeros(case.R, H, dtype=torch.bool)
    bad[(case.q_rows == case.q_rows[bad_row]) & has_keys, 6] = True
    check(case.run(ops, q_bad, True, True, k16=table, k_rows=k_rows)[0],
          case.run(ops, q_bad, True, False, k16=table, k_rows=k_rows)[0], bad)


def test_refusals_name_their_cause(ops):
    from variantformer_amd import _lib
    lib = _lib.load()
    case = AlibiCase(4, 32, "bf16", True)
    q16, _ = case.queries(True)
    q, k = q16.cuda(), case.k16.cuda()
    cu_rows, cu_k, q_rows = case.cu_rows.cuda(), case.cu_k.cuda(), case.q_rows.cuda()
    slopes, q_pos = case.slopes.cuda(), case.q_pos.cuda()
    max_k = max(case.kl)
    out = torch.full((case.R, max_k), SENTINEL, dtype=torch.float32, device="cuda")
    stats = torch.full((case.R, case.H, 2), SENTINEL, dtype=torch.float32, device="cuda")

    def call(flags=2, dh=case.dh, stats_ptr=stats.data_ptr()):
        return lib.vf_attn_probs_v2(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), q_rows.data_ptr(), cu_rows.data_ptr(),
                                    cu_k.data_ptr(), len(case.kl), max(case.rl), max_k, case.H, dh, case.scale, _lib.VF_BF16, flags,
                                    0, stats_ptr, out.data_ptr(), out.stride(0), slopes.data_ptr(), q_pos.data_ptr(), 0,
                                    torch.cuda.current_stream().cuda_stream)
    assert call(flags=3) == 1 and b"VF_ATTN_Q_AT_START" in lib.vf_last_error()
    assert call(dh=40) == 1 and b"head_dim" in lib.vf_last_error()
    assert call(stats_ptr=0) == 1 and b"stats" in lib.vf_last_error()
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL) and torch.all(stats == SENTINEL)    # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()

"""Exact-arithmetic indexing and race screens for the attention kernels (the cases of tests/attn_exact_cases.py on the device).

Every output element has one admissible bit pattern: whole outputs are compared with torch.equal on the 16-bit patterns, every
launch is repeated, and the kernel a case is routed to is asserted by name, so that a stale LDS stage, a missing barrier, a tail
mask off by one or a key paired with the wrong V row shows up as a bit mismatch in whichever row, head and column it occurs."""
import numpy as np
import pytest
import torch

from tests import attn_exact_cases as X

pytestmark = pytest.mark.gpu

IDS = lambda c: c.id          # noqa: E731
LAUNCHES = 3
EXTRA_ROWS = 5                # rows past cu_seqlens_q[n_seq]: never written


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from variantformer_amd import ops as _ops
    from variantformer_amd import _lib
    _lib.load()      # must be the in-tree HIP library; raises if missing
    return _ops


def _where(b, bad_rows, got, want, H, dh):
    """Name the first mismatches: sequence, row in the sequence, head, column, got and expected value."""
    cu = b.cu_q.numpy()
    lines = []
    for r in bad_rows[:8].tolist():
        s = int(np.searchsorted(cu, r, side="right") - 1)
        cols = torch.nonzero(got[r] != want[r])[:, 0]
        c = int(cols[0]) if cols.numel() else -1
        lines.append(f"seq {s} ({b.q_lens[s]} q x {b.k_lens[s]} k) row {r - int(cu[s])} head {c // dh} col {c % dh}: "
                     f"got {float(got[r, c])!r} want {float(want[r, c])!r} ({cols.numel()} of {H * dh} elements)")
    return "\n".join(lines)


def _assert_bits(b, got16, want16, rows, H, dh, what):
    g, w = got16[rows], want16[rows]
    if torch.equal(g.view(torch.int16), w.view(torch.int16)):
        return
    bad = (g.view(torch.int16) != w.view(torch.int16)).any(dim=1)
    bad_rows = rows[bad]
    gf, wf = got16.float(), want16.float()
    raise AssertionError(f"{what}: {int(bad.sum())} of {rows.numel()} rows differ from the one admissible bit pattern\n"
                         + _where(b, bad_rows, gf, wf, H, dh))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", X.FORWARD_CASES, ids=IDS)
def test_forward_attention_bits(ops, case, dtype):
    """vf_attn_varlen_fwd_v2 / _v3 / _rows: LAUNCHES launches into outputs prefilled with NaN; the 16-bit patterns of every
    compared row (all rows, or with a real ALiBi bias the rows at position 0 / n - 1) equal the closed form; rows of queries
    without keys are zero, rows past cu_seqlens_q[n_seq] keep their NaN, every other row is finite; the launch went to the
    kernel the case names."""
    td = X.torch_dtype(dtype)
    b = X.built(case)
    X.assert_premises(b, dtype)
    H, dh = case.H, case.dh
    D = H * dh
    tq = b.q.shape[0]
    want16 = b.expected.to(td)
    rows = X.expected_rows(b)
    cu_q = b.cu_q.cuda()
    cu_k = None if case.k_lens is None else b.cu_k.cuda()
    slopes = None if b.slopes is None else b.slopes.cuda()
    kw = dict(slopes=slopes, scale=b.scale, q_at_start=case.q_at_start, q_log2=case.q_log2)
    if case.rows:
        # a table of the distinct rows in a seeded order, unread NaN rows between them; every sequence occurs twice, so every
        # table row is read through two entries of the map
        t0 = b.table[0].shape[0]
        n_tab = t0 + 37
        pos = torch.from_numpy(np.random.default_rng(case.seed).permutation(n_tab))
        tab = torch.full((n_tab, 3 * D), float("nan"))
        tab[pos[:t0]] = torch.cat(b.table, dim=1)
        tab = tab.cuda().to(td)
        q, k, v = tab[:, :D], tab[:, D:2 * D], tab[:, 2 * D:]
        kw["rows"] = pos[b.row_of_token].cuda().contiguous()
        assert ops.attn_rows_supported(dh, slopes is not None, len(b.q_lens), H, b.max_q, b.max_k, True)
    else:
        q = b.q.cuda().to(td)
        kv = torch.cat([b.k, b.v], dim=1).cuda().to(td)
        k, v = kv[:, :D], kv[:, D:]
    no_keys = torch.cat([torch.arange(int(b.cu_q[s]), int(b.cu_q[s + 1])) for s in range(len(b.q_lens)) if b.k_lens[s] == 0]
                        + [torch.zeros(0, dtype=torch.int64)])
    assert no_keys.numel() > 0 or case.k_lens is None        # (self attention: the empty sequence has no queries either)
    for launch in range(LAUNCHES):
        out = torch.full((tq + EXTRA_ROWS, D), float("nan"), device="cuda", dtype=td)
        ops.attn_varlen(q, k, v, cu_q, cu_k, b.max_q, b.max_k, H, dh, out=out, **kw)
        torch.cuda.synchronize()
        assert ops.last_kernel("attn") == case.kernel
        got = out.cpu()
        _assert_bits(b, got[:tq], want16, rows, H, dh, f"{case.name} {dtype} launch {launch}")
        assert no_keys.numel() == 0 or float(got[no_keys].float().abs().max()) == 0.0
        assert bool(torch.isnan(got[tq:].float()).all()), "rows past cu_seqlens_q[n_seq] were written"
        assert bool(torch.isfinite(got[:tq].float()).all())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", X.COUNTED_CASES, ids=IDS)
def test_counted_keys_bits(ops, case, dtype):
    """vf_attn_counted_keys: the two-weight multiset through (count, logit) pairs, rows with log2_count = -inf, C in
    {1, 2, 9, 15, 16}, the three q_per_block values of launch_counted_keys; every element's bits, LAUNCHES launches."""
    td = X.torch_dtype(dtype)
    b = X.build_counted(case)
    X.assert_premises(b, dtype)
    assert X.counted_q_per_block(len(case.lens), b.max_q) == case.q_per_block
    want16 = b.expected.to(td)
    q, kv, lc, cu = b.q.cuda().to(td), b.kv.cuda().to(td), b.log2_count.cuda().contiguous(), b.cu.cuda()
    for launch in range(LAUNCHES):
        got = ops.attn_counted_keys(q, kv, lc, cu, b.max_q, case.H, case.dh)
        torch.cuda.synchronize()
        assert ops.last_kernel("attn") == "attn_counted_keys_kernel"
        bad = (got.cpu().view(torch.int16) != want16.view(torch.int16))
        assert not bool(bad.any()), f"{case.name} {dtype} launch {launch}: {int(bad.sum())} elements differ, first at " \
                                    f"{torch.nonzero(bad)[0].tolist()}"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", X.SOFTMAX_CASES, ids=IDS)
def test_softmax_counted_bits(ops, case, dtype):
    """vf_softmax_counted at Cp = C rounded up to even and at Cp = 16: weights that are powers of two, exact zeros for absent
    rows and for the padding slots (whose logits hold arbitrary finite values)."""
    td = X.torch_dtype(dtype)
    b = X.build_softmax(case)
    want16 = b.expected.to(td)
    assert torch.equal(want16.float(), b.expected)
    sc, lc, cu = b.scores.cuda(), b.log2_count.cuda().contiguous(), b.cu.cuda()
    for launch in range(LAUNCHES):
        got = ops.softmax_counted(sc, lc, cu, b.max_q, case.H, case.Cp, out_dtype=td)
        torch.cuda.synchronize()
        bad = (got.cpu().view(torch.int16) != want16.view(torch.int16))
        assert not bool(bad.any()), f"{case.name} {dtype} launch {launch}: {int(bad.sum())} elements differ, first at " \
                                    f"{torch.nonzero(bad)[0].tolist()}"


def _probs_v1(ops, q, k, sel, cu_rows, cu_k, max_rows, max_k, H, dh, scale, q_log2, per_head, out):
    """The first entry (vf_attn_probs: no bias, no key row map), which ops.attn_probs no longer calls."""
    from variantformer_amd import _lib
    stats = torch.empty((sel.numel(), H, 2), dtype=torch.float32, device=q.device)
    _lib.check(_lib.load().vf_attn_probs(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), sel.data_ptr(), cu_rows.data_ptr(),
                                         cu_k.data_ptr(), cu_rows.numel() - 1, int(max_rows), int(max_k), H, dh, float(scale),
                                         ops._dt(q.dtype), ops.ATTN_Q_LOG2 if q_log2 else 0, int(per_head), stats.data_ptr(),
                                         out.data_ptr(), out.stride(0), torch.cuda.current_stream().cuda_stream), "vf_attn_probs")
    return out, stats


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", X.PROBS_CASES, ids=IDS)
def test_attn_probs_exact(ops, case, dtype):
    """vf_attn_probs_v2 (and vf_attn_probs where the case has neither bias nor key row map): P[r, h, j] = 2^-b_j / L on the
    sequence's keys and 0 beyond, (m, l) = (off, L).  m bit-exact; l and P within 2^-20 relative (a handful of fp32 operations
    each specified to about an ulp; the smallest indexing error moves P by a factor of two or to / from zero) and exactly zero
    where the expectation is zero; repeated launches bit-identical."""
    td = X.torch_dtype(dtype)
    b = X.build_probs(case)
    X.assert_premises(b, dtype)
    H, dh = case.H, case.dh
    R, max_k = b.sel.numel(), b.max_k
    want = b.P if case.per_head else b.P.mean(dim=1, keepdim=True)
    want = want.reshape(-1, max_k)
    n_out = want.shape[0]
    q_tab = b.q.cuda().to(td)
    sel = b.sel.cuda().contiguous()
    if case.q_rows:
        q, q_rows = q_tab, sel
    else:
        q, q_rows = q_tab[sel].contiguous(), None
    k = b.k.cuda().to(td)
    k_rows = None
    if case.k_rows:
        perm = torch.from_numpy(np.random.default_rng(case.seed).permutation(k.shape[0] + 11))
        tab = torch.full((k.shape[0] + 11, k.shape[1]), float("nan"), device="cuda", dtype=td)
        tab[perm[:k.shape[0]].cuda()] = k
        k, k_rows = tab, perm[:b.k.shape[0]].cuda().contiguous()
    slopes = None if b.slopes is None else b.slopes.cuda()
    q_pos = None if b.q_pos is None else b.q_pos.cuda()
    cu_rows, cu_k = b.cu_rows.cuda(), b.cu_k.cuda()
    scale = 1.0 if case.q_log2 else b.scale
    first = None
    runs = [None] * LAUNCHES + (["v1"] if (case.alibi is None and not case.k_rows) else [])
    for entry in runs:
        out = torch.full((n_out, max_k), float("nan"), device="cuda")
        if entry == "v1":
            rows_arg = sel if case.q_rows else torch.arange(R, device="cuda")
            out, stats = _probs_v1(ops, q, k, rows_arg, cu_rows, cu_k, b.max_rows, max_k, H, dh, scale, case.q_log2, case.per_head, out)
        else:
            out, stats = ops.attn_probs(q, k, cu_rows, cu_k, b.max_rows, max_k, H, dh, q_rows=q_rows, q_log2=case.q_log2,
                                        per_head=case.per_head, scale=scale, out=out, slopes=slopes, q_pos=q_pos, k_rows=k_rows)
        torch.cuda.synchronize()
        assert ops.last_kernel("attn") == ("attn_probs_alibi_kernel" if case.alibi else "attn_probs_kernel")
        got, st = out.cpu(), stats.cpu()
        if first is None:
            first = (got, st)
            assert torch.equal(st[:, :, 0], b.stats[:, :, 0]), "the row maxima are not bit-exact"
            l_err = ((st[:, :, 1].double() - b.stats[:, :, 1].double()).abs() / b.stats[:, :, 1].double().clamp_min(1.0)).max()
            zero = want == 0
            assert float(got[zero].abs().max()) == 0.0, "a probability past the sequence's keys (or of a row without keys) is not 0"
            p_err = ((got.double() - want).abs()[~zero] / want[~zero]).max()
            print(f"[attn-exact] {case.name} {dtype}: max rel err of l {float(l_err):.3e}, of P {float(p_err):.3e}")
            assert float(l_err) <= X.PROBS_RTOL and float(p_err) <= X.PROBS_RTOL
        else:
            assert torch.equal(got.view(torch.int32), first[0].view(torch.int32)), f"launch {entry}: P differs from the first launch"
            assert torch.equal(st.view(torch.int32), first[1].view(torch.int32)), f"launch {entry}: stats differ from the first launch"

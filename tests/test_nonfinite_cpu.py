"""The inputs of tests/test_nonfinite_gpu.py discriminate -- shown on the float64 references of tests/nonfinite_cases.py
alone, no GPU: every poison makes exactly the claimed outputs NaN, the witnesses of the containment are sequences whose last
key tile is staged past their last key, and the list of special values holds every rounding situation contract item 3 of
DESIGN.md ("Non-finite operands") names."""
import math

import pytest
import torch

from tests import attn_edge_cases as E
from tests import nonfinite_cases as N


# ---------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------
def test_every_kernel_family_and_every_edge_geometry_is_listed():
    names = {c.name for c in N.ATTN_CASES}
    assert {c.name for c in E.ATTN_EDGE_CASES} <= names
    for c in E.ATTN_EDGE_CASES:
        assert N.ATTN_BY_NAME[c.name][:8] == tuple(c)              # the same geometry, kernel, q_log2 settings, seed
    kernels = {c.kernel for c in N.ATTN_CASES}
    assert kernels >= {E.FWD64, E.FWD128, E.SHORT2_1, E.SHORT2_2, E.SHORT, N.X32_32, N.X32_64, N.SHORT2_ROWS}
    assert any(c.dh == 40 for c in N.ATTN_CASES)                 # a padded head dim
    for c in N.ATTN_CASES:
        if c.kernel in (N.X32_32, N.X32_64):
            blocks = len(c.ql) * c.H * ((max(c.ql) + 255) // 256)
            assert c.dh == 48 and not c.alibi and (blocks >= 2048) == (c.kernel == N.X32_64)
        if c.rows:
            assert c.ql == c.kl and c.q_log2 == (True,)
            assert sorted(N.row_map(c).tolist()) == list(range(sum(c.ql)))


@pytest.mark.parametrize("name", [c.name for c in N.ATTN_CASES])
def test_victim_and_witnesses(name):
    """Non-empty neighbours on both sides; no witness (and not the victim) has a key count that is a multiple of 64, so each
    one's last key tile holds rows past its end -- the rows a staging bug would fill from the next sequence; the victim's
    first and last key rows are different rows; every poison touches one element, inside the victim and head*."""
    c = N.ATTN_BY_NAME[name]
    b = N.victim(c)
    assert N.witnesses(c) == (b - 1, b + 1)
    for w in N.witnesses(c) + (b,):
        assert c.ql[w] > 0 and c.kl[w] > 0 and c.kl[w] % 64 != 0
    assert c.kl[b] >= 2 and (c.ql[b] >= 2 or max(c.ql) == 1)           # other query rows for Q-NaN, where the geometry has any
    cu_q, cu_k = E.cu_of(c.ql), E.cu_of(c.kl)
    h = N.head_star(c)
    clean = N.operands(name, "bf16", c.q_log2[0])
    sites = set()
    for poison in N.POISONS:
        which, row, col, val = N.poison_site(c, poison)
        cu = cu_q if which == "q" else cu_k
        assert int(cu[b]) <= row < int(cu[b + 1]) and h * c.dh <= col < (h + 1) * c.dh
        bad = N.poisoned(c, clean, poison)
        changed = sum(int((x.view(torch.int32) != y.view(torch.int32)).sum()) for x, y in zip(clean, bad))
        assert changed == 1 and (math.isnan(val) or math.isinf(val))
        sites.add((poison, which, row - int(cu[b])))
    assert ("k_nan_first", "k", 0) in sites and ("k_nan_last", "k", c.kl[b] - 1) in sites
    assert ("v_nan_first", "v", 0) in sites and ("v_inf_last", "v", c.kl[b] - 1) in sites


@pytest.mark.parametrize("name,q_log2", N.ATTN_PARAMS)
def test_reference_nan_sets_are_the_claimed_regions(name, q_log2):
    """K-NaN: every row and column of (victim, head*) and nothing else; V-NaN: one column of it; Q-NaN: one row of it.
    V-Inf: that column is non-finite in every row, everything else finite; K-Inf: nothing outside (victim, head*) moves."""
    c = N.ATTN_BY_NAME[name]
    clean = N._clean_ref(name, q_log2)[3]
    assert torch.isfinite(clean).all()
    b, h = N.victim(c), N.head_star(c)
    n_rows = c.ql[b]
    for poison in N.NAN_POISONS:
        ref = N.poisoned_ref(name, q_log2, poison)
        reg = N.region(c, poison)
        assert torch.equal(torch.isnan(ref), reg), poison
        assert torch.equal(ref[~reg], clean[~reg]), poison
        assert int(reg.sum()) == {"k": n_rows * c.dh, "v": n_rows, "q": c.dh}[poison[0]]
    for poison in ("v_inf_last", "v_inf_first"):
        ref = N.poisoned_ref(name, q_log2, poison)
        reg = N.region(c, poison)
        assert not torch.isfinite(ref[reg]).any() and torch.equal(ref[~reg], clean[~reg]), poison
    ref = N.poisoned_ref(name, q_log2, "k_inf")
    reg = N.region(c, "k_inf")
    assert torch.equal(ref[~reg], clean[~reg])         # (inside: NaN where q_d > 0, the other keys' mix where q_d < 0)


def test_mutation_staging_clamped_against_the_batch_end_is_seen():
    """By reading the code, not by running a kernel's staging: a staging that clamps a key row against the batch's total
    tokens instead of len_k - 1 would fill the masked rows of the PRECEDING sequence's last tile with the victim's first rows.
    This test only checks the two facts that argument rests on: the rows such a staging would fetch begin with the poisoned
    row, and a weight of exactly zero (the mask) times that row is NaN -- while the preceding sequence lies outside `region`,
    i.e. is held to the clean bits by the GPU test."""
    c = N.ATTN_BY_NAME["fwd64_dh48"]
    b, h, d = N.victim(c), N.head_star(c), N.col_star(c)
    cu_k = E.cu_of(c.kl)
    prev_end = int(cu_k[b])
    for poison in ("k_nan_first", "v_nan_first"):
        q, k, v = N.poisoned(c, N.operands(c.name, "bf16", True), poison)
        pad = 64 - c.kl[b - 1] % 64
        rows = torch.arange(prev_end, prev_end + pad).clamp(max=k.shape[0] - 1)       # what the mutated staging would fetch
        assert rows[0] == prev_end and N.poison_site(c, poison)[1] == prev_end
        p_masked = torch.zeros(pad, dtype=torch.float64)                               # exactly zero: the mask
        if poison[0] == "k":
            leak = (k[rows, h * c.dh:(h + 1) * c.dh].double().sum(dim=1) * p_masked).sum()      # the masked scores q . k
        else:
            leak = (p_masked * v[rows, h * c.dh + d].double()).sum()
        assert math.isnan(float(leak))
        region = N.region(c, poison)
        cu_q = E.cu_of(c.ql)
        assert not region[int(cu_q[b - 1]):int(cu_q[b])].any()       # the preceding sequence is held to the clean bits


def test_mutation_guarded_normalise_is_seen():
    """`l > 0 ? o / l : 0` launders a NaN denominator into zeros: the reference's K-NaN set is non-empty and NaN != 0."""
    c = N.ATTN_BY_NAME["short2_2pass_dh48"]
    ref = N.poisoned_ref(c.name, True, "k_nan_last")
    reg = N.region(c, "k_nan_last")
    l = torch.tensor(N.NAN)
    laundered = torch.where(l > 0, ref[reg] / l, torch.zeros(()).double())
    assert reg.any() and torch.isnan(ref[reg]).all() and not torch.isnan(laundered).any()


# ---------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,M,N_,K", N.GEMM_PATHS)
@pytest.mark.parametrize("epi", N.EPILOGUES)
def test_gemm_reference_nan_sets(path, M, N_, K, epi):
    """One NaN in A makes its output row NaN, one in W or the bias a column (under GEGLU the column that row feeds), one in
    the residual one element; shapes ragged against every tile, and K on the path's side of the K % 64 split."""
    n = N.GEGLU_N[N_] if epi == "geglu" else N_
    assert M % 64 and n % 64 and M <= 300 and (K % 64 != 0) == (path == "generic") and (path != "v22" or K % 128 == 0)
    a, w, bias, res = N.gemm_operands(M, n, K, "bf16")
    clean = N.gemm_ref(a, w, bias, res, epi)
    n_out = clean.shape[1]
    assert n_out == (n // 2 if epi == "geglu" else n) and torch.isfinite(clean).all()
    for m in N.gemm_rows(M):
        ap = a.clone()
        ap[m, 3] = N.NAN
        assert torch.equal(torch.isnan(N.gemm_ref(ap, w, bias, res, epi)), N.gemm_region(M, n_out, "row", m=m))
    assert M - 1 in N.gemm_rows(M) and (M <= 128 or {127, 128} <= set(N.gemm_rows(M)))
    for ns in (n - 3, 2):
        wp, bp = w.clone(), bias.clone()
        wp[ns, K - 1] = N.NAN
        bp[ns] = N.NAN
        col = N.gemm_region(M, n_out, "col", n=ns % n_out)
        assert torch.equal(torch.isnan(N.gemm_ref(a, wp, bias, res, epi)), col)
        assert torch.equal(torch.isnan(N.gemm_ref(a, w, bp, res, epi)), col)
    if epi == "res":
        rp = res.clone()
        rp[M - 1, n - 3] = N.NAN
        assert torch.equal(torch.isnan(N.gemm_ref(a, w, bias, rp, epi)), N.gemm_region(M, n_out, "elem", m=M - 1, n=n - 3))


def test_ln_references_nan_sets():
    M, n, K = N.LN_M, N.LN_N, N.LN_K
    assert n % 32 == 0 and K % 64 == 0 and M % 64 and n % 64
    a, w, bias, res = N.gemm_operands(M, n, K, "bf16", seed=720)
    x = N.gemm_ref(a, w, bias, res, "res")
    rp = res.clone()
    rp[128, 5] = N.NAN
    st = N.ln_stats_ref(N.gemm_ref(a, w, bias, rp, "res"))
    want = torch.zeros((M, 2), dtype=torch.bool)
    want[128] = True
    assert torch.equal(torch.isnan(st), want) and torch.isfinite(N.ln_stats_ref(x)).all()
    stats = N.ln_stats_ref(a).float()
    colsum = w.sum(dim=1)
    for epi in ("bf16", "f32", "geglu"):
        clean = N.ln_consumer_ref(a, stats, w, bias, colsum, epi)
        assert torch.isfinite(clean).all()
        ap = a.clone()
        ap[M - 1, 0] = N.NAN
        assert torch.equal(torch.isnan(N.ln_consumer_ref(ap, stats, w, bias, colsum, epi)),
                           N.gemm_region(M, clean.shape[1], "row", m=M - 1))
        sp = stats.clone()
        sp[127, 1] = N.NAN
        assert torch.equal(torch.isnan(N.ln_consumer_ref(a, sp, w, bias, colsum, epi)), N.gemm_region(M, clean.shape[1], "row", m=127))


# ---------------------------------------------------------------------------------------------
# the special values of the store-rounding contract
# ---------------------------------------------------------------------------------------------
def _neighbours(v: float, dtype: str):
    """(below, above): the two values of the type that bracket the finite v (equal when v is representable)."""
    t = N.tdt(dtype)
    r = torch.tensor(v, dtype=torch.float32).to(t)
    bits = int(r.view(torch.int16))
    cand = [torch.tensor(bits + d, dtype=torch.int16).view(t).double().item() for d in (-1, 0, 1) if 0 <= (bits & 0x7FFF) + d <= 0x7C00]
    return max(x for x in cand if x <= v), min(x for x in cand if x >= v)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_special_values_hold_every_rounding_situation(dtype):
    t = N.tdt(dtype)
    vals = dict(N.special_values(dtype))
    r16 = lambda v: N.round16(v, dtype)
    even = lambda x: int(torch.tensor(x, dtype=torch.float64).to(t).view(torch.int16)) % 2 == 0
    for base in ("1", "32"):
        v = vals[f"tie_down_to_even@{base}"]
        lo, hi = _neighbours(v, dtype)
        assert hi - v == v - lo > 0 and float(r16(v)) == lo and even(lo) and not even(hi)
        v = vals[f"tie_up_to_even@{base}"]
        lo, hi = _neighbours(v, dtype)
        assert hi - v == v - lo > 0 and float(r16(v)) == hi and even(hi) and not even(lo)
        v, tie = vals[f"just_above_tie@{base}"], vals[f"tie_down_to_even@{base}"]
        lo, hi = _neighbours(v, dtype)
        assert v > tie and _neighbours(tie, dtype) == (lo, hi) and float(r16(v)) == hi        # truncation would give lo
        v = vals[f"just_below_tie@{base}"]
        assert v < tie and _neighbours(v, dtype) == (lo, hi) and float(r16(v)) == lo
    z = r16(vals["minus_zero"])
    assert float(z) == 0.0 and int(z.view(torch.int16)) == -32768
    assert float(r16(vals["plus_inf"])) == N.INF and float(r16(vals["minus_inf"])) == -N.INF and math.isnan(float(r16(vals["nan"])))
    top = vals["largest_finite"]
    assert float(r16(top)) == top == float(torch.finfo(t).max) and float(r16(vals["minus_largest_finite"])) == -top
    assert float(r16(vals["fp32_max"])) == N.INF                    # beyond the type's range, both types
    if dtype == "fp16":
        assert top == 65504.0
        assert float(r16(vals["65519"])) == 65504.0 and float(r16(vals["65520"])) == N.INF           # a saturating store: 65504
        assert float(r16(vals["minus_65520"])) == -N.INF and float(r16(vals["1e6"])) == N.INF and float(r16(vals["minus_1e6"])) == -N.INF
        tiny = 2.0 ** -24
        assert vals["smallest_subnormal"] == tiny and float(r16(tiny)) == tiny                       # a flushing store: 0
        v = vals["subnormal_with_rounding"]
        assert float(r16(v)) == 50 * tiny != v and 50 * tiny < 2.0 ** -14                            # 3e-6 / 2^-24 = 50.33
        assert vals["tie_to_zero"] == tiny / 2 and float(r16(tiny / 2)) == 0.0
        v = vals["normal_subnormal_boundary"]
        assert 2.0 ** -14 - tiny < v < 2.0 ** -14 and float(r16(v)) == 1023 * tiny                   # the largest subnormal
    # no fp32 subnormals among the inputs, nor among the products the tests form from them (x 32, x 2^-4)
    for v in vals.values():
        for s in (1.0, 32.0, 2.0 ** -4):
            x = abs(float(torch.tensor(v, dtype=torch.float32) * s))
            assert not (0.0 < x < 2.0 ** -126)
    # the values a GELU epilogue hands to its store unchanged (v >= 16): ties, the range boundary and Inf are among them
    big = [k for k, v in vals.items() if v >= 16]
    assert {"tie_down_to_even@32", "tie_up_to_even@32", "just_above_tie@32", "just_below_tie@32", "largest_finite", "plus_inf"} <= set(big)
    g = torch.nn.functional.gelu(torch.tensor([vals[k] for k in big], dtype=torch.float64))
    assert torch.equal(g, torch.tensor([vals[k] for k in big], dtype=torch.float64))
    assert float(torch.nn.functional.gelu(torch.tensor(32.0, dtype=torch.float64))) == 32.0          # the GEGLU gate


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_mutation_saturating_or_truncating_pack_is_seen(dtype):
    """A store that saturates at the largest finite value, or rounds toward zero, or flushes subnormals, differs from torch's
    cast on named entries of the list -- so the bit-exact comparison of the GPU test cannot pass with one."""
    t = N.tdt(dtype)
    names = [k for k, _ in N.special_values(dtype)]
    x = N.special_tensor(dtype)
    want = x.to(t)
    top = float(torch.finfo(t).max)
    saturating = torch.where(torch.isinf(want) & torch.isfinite(x), torch.sign(x) * top, want.float()).to(t)
    if dtype == "bf16":
        toward_zero = (x.view(torch.int32) & ~0xFFFF).view(torch.float32).to(t)
    else:
        lo_hi = [_neighbours(float(v), dtype) if math.isfinite(float(v)) and abs(float(v)) <= top else (float(v), float(v)) for v in x]
        toward_zero = torch.tensor([(lo if v >= 0 else hi) for (lo, hi), v in zip(lo_hi, x.tolist())], dtype=torch.float64).to(t)
    differs = lambda mut: {names[i] for i in range(len(names)) if not N.same_16bit(mut[i:i + 1], want[i:i + 1])}
    assert differs(saturating) >= ({"fp32_max"} if dtype == "bf16" else {"65520", "minus_65520", "1e6", "minus_1e6", "fp32_max"})
    assert differs(toward_zero) >= {"tie_up_to_even@1", "just_above_tie@1", "tie_up_to_even@32", "just_above_tie@32"}
    if dtype == "fp16":
        flushing = torch.where(want.float().abs() < 2.0 ** -14, torch.zeros(()), want.float()).to(t)
        assert differs(flushing) >= {"smallest_subnormal", "subnormal_with_rounding", "normal_subnormal_boundary"}


def test_model_batch_has_a_token_private_to_gene_1():
    batch, tok = N.model_batch()
    assert len(batch["cre_sequences"]) == 3
    for g in range(3):
        valid = batch["cre_sequences"][g][~batch["cre_attention_masks"][g]]
        assert bool((valid == tok).any()) == (g == 1)

"""The contract of DESIGN.md, "Non-finite operands", on a real MI355X, kernel by kernel:

  1. containment  -- a NaN / Inf changes only the outputs that depend on it; every other element of the launch keeps the
                     bits of the launch without it;
  2. no laundering -- what the float64 reference (tests/nonfinite_cases.py) makes NaN is NaN;
  3. stores round like torch -- a value handed to a 16-bit store equals torch's cast of it, bit for bit.

tests/test_nonfinite_cpu.py shows on the references alone that the inputs used here tell a wrong kernel from a right one.
Every NaN set comes from the reference on the poisoned operands.  vf_layernorm has no entry in the store-rounding tests: it
hands its store (x - mean) * rstd * gamma + beta, for which no input makes every special value come out exactly."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attn_edge_cases as E
from tests import nonfinite_cases as N
from tests.helpers import SEQ2REG_512, _rand, build_model, seq2gene_kw

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "fp16"]
NAN = N.NAN


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from variantformer_amd import ops as _ops
    from variantformer_amd import _lib
    _lib.load()      # must be the in-tree HIP library; raises if missing
    return _ops


@pytest.fixture(autouse=True)
def _leave_no_alert_behind(ops):
    """The statistics kernels raise the stream's LayerNorm-fold flag for rows with a large mean or a large FINITE element
    (not for rows that hold a NaN or an Inf: test_fold_alert_and_non_finite_rows); no later test may find the flag set."""
    yield
    ops.ln_fold_alert(torch.device("cuda", torch.cuda.current_device()), reset=True)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _held(tag, got, clean, ref_nan):
    """'' when isnan(got) is exactly `ref_nan` (bool, CPU, the reference's NaN set) and every other element keeps the bits of
    `clean`; else what went wrong."""
    g, c = got.detach().cpu(), clean.detach().cpu()
    ref_nan = ref_nan.reshape(g.shape)
    gn = torch.isnan(g.float())
    if not torch.equal(gn, ref_nan):
        return (f"{tag}: NaN set differs from the reference's: {int((gn & ~ref_nan).sum())} extra, "
                f"{int((~gn & ref_nan).sum())} missing of {int(ref_nan.sum())}")
    moved = (_bits(g) != _bits(c)) & ~ref_nan
    if moved.any():
        return f"{tag}: {int(moved.sum())} elements outside the NaN set lost the clean bits, first at {moved.nonzero()[0].tolist()}"
    return ""


def _no(failures):
    failures = [f for f in failures if f]
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------
def _attn_run(ops, c, qkv, dtype, q_log2):
    t = N.tdt(dtype)
    q, k, v = (x.cuda().to(t) for x in qkv)
    cu_q, sl = E.cu_of(c.ql).cuda(), N.slopes_of(c)
    sl = None if sl is None else sl.cuda()
    if c.rows:                            # the operands as tables: token i reads row rm[i]
        rm = N.row_map(c).cuda()
        tabs = []
        for x in (q, k, v):
            tab = torch.empty_like(x)
            tab[rm] = x
            tabs.append(tab)
        out = ops.attn_varlen(*tabs, cu_q, None, max(c.ql), max(c.kl), c.H, c.dh, sl, q_log2=q_log2, rows=rm)
    else:
        out = ops.attn_varlen(q, k, v, cu_q, E.cu_of(c.kl).cuda(), max(c.ql), max(c.kl), c.H, c.dh, sl, q_log2=q_log2)
    kernel = ops.last_kernel("attn")
    torch.cuda.synchronize()
    assert kernel == c.kernel, kernel
    return out.cpu()


_CLEAN = {}


def _attn_clean(ops, name, q_log2, dtype):
    key = (name, q_log2, dtype)
    if key not in _CLEAN:
        _CLEAN.clear()                    # the poisons of one (geometry, type) run back to back: one entry is enough
        _CLEAN[key] = _attn_run(ops, N.ATTN_BY_NAME[name], N.operands(name, dtype, q_log2), dtype, q_log2)
    return _CLEAN[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,q_log2", N.ATTN_PARAMS)
def test_attention_clean_run_matches_oracle(ops, name, q_log2, dtype):
    """The launch every poisoned one is compared with: the expected kernel, and the oracle at the attention tolerances."""
    from oracle import vf_oracle as O
    c = N.ATTN_BY_NAME[name]
    got = _attn_clean(ops, name, q_log2, dtype).float()
    assert torch.isfinite(got).all()
    want = O.Rounding(dtype).r(N.oracle_rows(c, dtype, q_log2))
    np.testing.assert_allclose(got.numpy(), want.numpy(), **E.tolerance(dtype))


@pytest.mark.parametrize("poison", N.POISONS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,q_log2", N.ATTN_PARAMS)
def test_attention_poisons(ops, name, q_log2, dtype, poison):
    """One NaN / +Inf in K (the victim's last key row -- the one the staging replicates into the masked rows -- or its first,
    the one a load running past the preceding sequence's end would fetch), in V (both rows, one column) or in one query row,
    in head*: every row of every other sequence, every other head, for V every other column and for Q every other query row
    keep the bits of the clean launch; the NaN poisons make exactly the reference's NaN set NaN; V-Inf makes its column
    non-finite in every row of the victim (Inf or NaN: the 16-bit rounding of P decides); K-Inf: containment only."""
    c = N.ATTN_BY_NAME[name]
    clean = _attn_clean(ops, name, q_log2, dtype)
    got = _attn_run(ops, c, N.poisoned(c, N.operands(name, dtype, q_log2), poison), dtype, q_log2)
    reg = N.region(c, poison)
    outside = (_bits(got) != _bits(clean)) & ~reg
    assert not outside.any(), (f"{int(outside.sum())} elements outside the region lost the clean bits, first at "
                               f"{outside.nonzero()[0].tolist()} (victim rows {int(E.cu_of(c.ql)[N.victim(c)])}..)")
    if poison in N.NAN_POISONS:
        ref_nan = torch.isnan(N.poisoned_ref(name, q_log2, poison))
        gn = torch.isnan(got.float())
        assert torch.equal(gn, ref_nan), f"{int((gn & ~ref_nan).sum())} extra, {int((~gn & ref_nan).sum())} missing NaN"
    elif poison[0] == "v":
        assert not torch.isfinite(got.float()[reg]).any()


# (dh, H, ALiBi, queries, keys, kernel): one-key sequences in every kernel family; `short` needs one long key sequence (its
# LDS image must not fit three times), whose rows are not compared
ONE_KEY = {"fwd": (64, 4, False, [3, 17, 1, 5], [1, 1, 1, 1], E.FWD64),
           "x32": (48, 4, False, [3, 17, 1, 5], [1, 1, 1, 1], N.X32_32),
           "short2": (48, 8, True, [130, 3, 17, 200], [1, 1, 1, 1], E.SHORT2_2),
           "short": (48, 8, True, [130, 3, 17, 200, 5], [1, 1, 1, 1, 256], E.SHORT)}


@pytest.mark.parametrize("kind", ["finite_and_nan", "inf"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", list(ONE_KEY))
def test_attention_one_key_returns_v(ops, family, dtype, kind):
    """A sequence with ONE key: p = 1 (every family here runs a running maximum: exp2(s - s)), so every query row is the V
    row, bit for bit -- subnormals, the largest finite value and NaN (`finite_and_nan`), +-Inf (`inf`: the V rows staged past
    the sequence end are zeros, not copies of the last row, so no 0 x Inf meets them).  -0.0 is left out: the accumulator
    starts at +0 and +0 + 1 x -0 = +0, which is arithmetic, not rounding."""
    t = N.tdt(dtype)
    dh, H, alibi, ql, kl, kernel = ONE_KEY[family]
    D = H * dh
    x = N.round16([v for k, v in N.special_values(dtype) if k != "minus_zero"], dtype)
    x = x[torch.isinf(x.float()) == (kind == "inf")]
    v = _rand((sum(kl), D), 1402, 2.0).to(t)
    cu_k = E.cu_of(kl)
    one = [b for b, n in enumerate(kl) if n == 1]
    for b in one:
        v[int(cu_k[b])] = x[(torch.arange(D) + b) % x.numel()]
    q = _rand((sum(ql), D), 1400, 2.0).to(t)
    k = _rand((sum(kl), D), 1401, 2.0).to(t)
    sl = torch.tensor(N.O.alibi_slopes(H), dtype=torch.float32).cuda() if alibi else None
    out = ops.attn_varlen(q.cuda(), k.cuda(), v.cuda(), E.cu_of(ql).cuda(), cu_k.cuda(), max(ql), max(kl), H, dh, sl).cpu()
    assert ops.last_kernel("attn") == kernel, ops.last_kernel("attn")
    cu_q = E.cu_of(ql)
    for b in one:
        rows = out[int(cu_q[b]):int(cu_q[b + 1])]
        assert N.same_16bit(rows, v[int(cu_k[b])][None].expand(ql[b], D)), b


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["fwd", "x32"])
def test_attention_inf_in_v_of_a_later_tile_stays_inf(ops, family, dtype):
    """The tiled kernels stage a tile per 64 keys: 65 and 130 keys put the last key in the second / third tile, beside 63 / 62
    masked rows.  +Inf and -Inf in that key's V row, with small logits (every p about 1 / keys, far from underflow in either
    type), must come out as +Inf / -Inf in their columns for every query -- a masked row that still held a copy of the V row
    would make them NaN (0 x Inf) -- and nothing else may move."""
    t = N.tdt(dtype)
    dh, H, alibi, _, _, kernel = ONE_KEY[family]
    D, h, d = H * dh, H // 2, dh - 3
    ql, kl = [5, 70, 3, 20], [9, 65, 130, 7]
    cu_q, cu_k = E.cu_of(ql), E.cu_of(kl)
    q = _rand((sum(ql), D), 1410, 0.25).to(t)
    k = _rand((sum(kl), D), 1411, 1.0).to(t)
    v = _rand((sum(kl), D), 1412, 2.0).to(t)
    vp = v.clone()
    for b in (1, 2):
        vp[int(cu_k[b + 1]) - 1, h * dh + d] = N.INF
        vp[int(cu_k[b + 1]) - 1, h * dh + d - 8] = -N.INF
    run = lambda v_: ops.attn_varlen(q.cuda(), k.cuda(), v_.cuda(), cu_q.cuda(), cu_k.cuda(), max(ql), max(kl), H, dh).cpu()
    clean, got = run(v), run(vp)
    assert ops.last_kernel("attn") == kernel, ops.last_kernel("attn")
    want = clean.clone()
    rows = slice(int(cu_q[1]), int(cu_q[3]))
    want[rows, h * dh + d] = N.INF
    want[rows, h * dh + d - 8] = -N.INF
    assert torch.isfinite(clean.float()).all() and N.same_16bit(got, want)


# ---------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------
KERNEL_OF = {"v0": "gemm_mfma_kernel<64x64>", "v1": "gemm_mfma_kernel<128x128>", "v5": "gemm_mfma_kernel<64x64>",
             "v20": "gemm8_kernel", "v22": "gemm8x_kernel", "generic": "gemm_generic_kernel"}


def _epi_code(ops, epi):
    return {"bf16": ops.EPI_BF16, "f32": ops.EPI_F32, "res": ops.EPI_RES_F32, "geglu": ops.EPI_GEGLU_BF16,
            "gelu_f32": ops.EPI_GELU_F32, "gelu_bf16": ops.EPI_GELU_BF16}[epi]


def _gemm(ops, path, epi, dtype, a, w, bias, res):
    """ops.gemm on CPU operands in the UNPACKED order (GEGLU rows are permuted here, as a checkpoint load does)."""
    t = N.tdt(dtype)
    wd, bd = w.cuda().to(t), bias.cuda()
    if epi == "geglu":
        wd, bd = ops.pack_geglu_rows(wd, bd)
    out = ops.gemm(a.cuda().to(t), wd, bd, _epi_code(ops, epi), residual=res.cuda() if epi == "res" else None,
                   variant=N.variant_of(path))
    assert ops.last_kernel("gemm") == KERNEL_OF[path], ops.last_kernel("gemm")
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("epi", N.EPILOGUES)
@pytest.mark.parametrize("path,M,N_,K", N.GEMM_PATHS)
def test_gemm_poisons(ops, path, M, N_, K, epi, dtype):
    """One NaN in A (row M - 1, which the clamped loads replicate into the tile's rows >= M, and rows 127 | 128), in a W row,
    in the bias, in the residual: the reference's NaN set -- a row, a column (under GEGLU the column the row feeds), one
    element -- and the clean bits everywhere else."""
    n = N.GEGLU_N[N_] if epi == "geglu" else N_
    a, w, bias, res = N.gemm_operands(M, n, K, dtype)
    clean = _gemm(ops, path, epi, dtype, a, w, bias, res)
    assert torch.isfinite(clean.float()).all()
    fails = []
    for m in N.gemm_rows(M):
        ap = a.clone()
        ap[m, 3] = NAN
        fails.append(_held(f"A[{m}]", _gemm(ops, path, epi, dtype, ap, w, bias, res), clean,
                           torch.isnan(N.gemm_ref(ap, w, bias, res, epi))))
    for ns in (n - 3, 2):
        wp, bp = w.clone(), bias.clone()
        wp[ns, K - 1] = NAN
        bp[ns] = NAN
        fails.append(_held(f"W[{ns}]", _gemm(ops, path, epi, dtype, a, wp, bias, res), clean,
                           torch.isnan(N.gemm_ref(a, wp, bias, res, epi))))
        fails.append(_held(f"bias[{ns}]", _gemm(ops, path, epi, dtype, a, w, bp, res), clean,
                           torch.isnan(N.gemm_ref(a, w, bp, res, epi))))
    if epi == "res":
        for m in N.gemm_rows(M):
            rp = res.clone()
            rp[m, n - 3] = NAN
            fails.append(_held(f"residual[{m}]", _gemm(ops, path, epi, dtype, a, w, bias, rp), clean,
                               torch.isnan(N.gemm_ref(a, w, bias, rp, epi))))
    _no(fails)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("epi", ["bf16", "f32", "geglu"])
def test_gemm_ln_consumer_poisons(ops, epi, dtype):
    """The LayerNorm consumer: a NaN in the 16-bit stream copy or in a row's statistics makes the row NaN, one in W or the
    folded bias a column; every other element keeps the clean bits."""
    M, n, K = N.LN_M, N.LN_N, N.LN_K
    t = N.tdt(dtype)
    x, w, bias, _ = N.gemm_operands(M, n, K, dtype, seed=720)
    with ops.compute_dtype(t):
        s = ops.ln_stream(x.cuda())
    x16, stats = s.x16.float().cpu(), s.stats.cpu()
    code = _epi_code(ops, epi)

    def run(x16_, stats_, w_, bias_):
        wd, bd = w_.cuda().to(t), bias_.cuda()
        cs = wd.float().sum(dim=1).contiguous()
        if epi == "geglu":
            wd, bd = ops.pack_geglu_rows(wd, bd)
            cs = wd.float().sum(dim=1).contiguous()
        return ops.gemm_ln_consumer(ops.LnStream(None, x16_.cuda().to(t), stats_.cuda(), s.scale), wd, bd, cs, code)

    ref = lambda x16_, stats_, w_, bias_: torch.isnan(N.ln_consumer_ref(x16_, stats_, w_, bias_, w_.double().sum(dim=1), epi))
    clean = run(x16, stats, w, bias)
    assert torch.isfinite(clean.float()).all()
    fails = []
    for m in N.gemm_rows(M):
        xp, sp = x16.clone(), stats.clone()
        xp[m, 3] = NAN
        sp[m, 1] = NAN
        fails.append(_held(f"x16[{m}]", run(xp, stats, w, bias), clean, ref(xp, stats, w, bias)))
        fails.append(_held(f"stats[{m}]", run(x16, sp, w, bias), clean, ref(x16, sp, w, bias)))
    wp, bp = w.clone(), bias.clone()
    wp[n - 3, K - 1] = NAN
    bp[n - 3] = NAN
    fails.append(_held("W", run(x16, stats, wp, bias), clean, ref(x16, stats, wp, bias)))
    fails.append(_held("bias", run(x16, stats, w, bp), clean, ref(x16, stats, w, bp)))
    _no(fails)


def _producer(ops, kind, dtype, a, w, bias, res):
    """gemm_ln_producer in one of its four forms on CPU operands; `res` is the residual as the kernel reads it: fp32, or
    16-bit values times their scale."""
    t = N.tdt(dtype)
    A, W, B = a.cuda().to(t), w.cuda().to(t), bias.cuda()
    with ops.compute_dtype(t):
        if kind == "f32":
            return ops.gemm_ln_producer(A, W, B, None)
        if kind == "res32":
            return ops.gemm_ln_producer(A, W, B, res.cuda())
        if kind == "res16":
            sc = ops.x16_scale_for(t)
            return ops.gemm_ln_producer(A, W, B, ops.LnStream(None, (res * sc).cuda().to(t), None, sc))
        return ops.gemm_ln_producer(A, W, B, None, trunk16=(res * ops.T16_SCALE).cuda().half(), need_t16=True)


def _producer_residual(ops, kind, dtype, res):
    """The fp32 values the kernel adds: the residual after its own 16-bit storage."""
    if kind == "res16":
        sc = ops.x16_scale_for(N.tdt(dtype))
        return (res * sc).to(N.tdt(dtype)).float() / sc
    if kind == "t16":
        return (res * ops.T16_SCALE).half().float() / ops.T16_SCALE
    return res


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["f32", "res32", "res16", "t16"])
def test_gemm_ln_producer_poisons(ops, kind, dtype):
    """The LayerNorm producers (no residual, fp32 residual, 16-bit stream residual, fp16 trunk): the fp32 rows, their 16-bit
    copy, the trunk copy and the row statistics after vf_ln_finalize2 all follow the reference's pattern -- a NaN row (A), a
    NaN column and therefore NaN statistics in every row (W, bias), one element and one row's statistics (residual) -- and
    keep the clean bits elsewhere, the statistics of every other row included."""
    M, n, K = N.LN_M, N.LN_N, N.LN_K
    a, w, bias, res = N.gemm_operands(M, n, K, dtype, seed=740)
    clean = _producer(ops, kind, dtype, a, w, bias, res)
    fails = []

    def check(tag, a_, w_, bias_, res_):
        got = _producer(ops, kind, dtype, a_, w_, bias_, res_)
        x = N.gemm_ref(a_, w_, bias_, _producer_residual(ops, kind, dtype, res_), "f32" if kind == "f32" else "res")
        x_nan = torch.isnan(x)
        st_nan = torch.isnan(N.ln_stats_ref(x))
        fails.append(_held(tag + " x", got.x, clean.x, x_nan))
        fails.append(_held(tag + " x16", got.x16, clean.x16, x_nan))
        fails.append(_held(tag + " stats", got.stats, clean.stats, st_nan))
        if kind == "t16":
            fails.append(_held(tag + " t16", got.t16, clean.t16, x_nan))

    for m in N.gemm_rows(M):
        ap = a.clone()
        ap[m, 3] = NAN
        check(f"A[{m}]", ap, w, bias, res)
        if kind != "f32":
            rp = res.clone()
            rp[m, n - 3] = NAN
            check(f"residual[{m}]", a, w, bias, rp)
    wp, bp = w.clone(), bias.clone()
    wp[n - 3, K - 1] = NAN
    bp[n - 3] = NAN
    check("W", a, wp, bias, res)
    check("bias", a, w, bp, res)
    assert torch.isfinite(clean.x).all() and torch.isfinite(clean.stats).all()
    _no(fails)


# ---------------------------------------------------------------------------------------------
# streaming and small kernels
# ---------------------------------------------------------------------------------------------
OUT_TYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.mark.parametrize("gelu", [False, True])
def test_layernorm_poison(ops, gelu):
    rows, D = 37, 200
    x, g, b = _rand((rows, D), 1500, 2.0), 1.0 + _rand((D,), 1501, 0.3), _rand((D,), 1502, 0.2)
    xp = x.clone()
    xp[5, 7] = NAN
    ref = F.layer_norm(xp.double(), (D,), g.double(), b.double(), 1e-5)
    ref = F.gelu(ref) if gelu else ref
    fails = []
    for t in OUT_TYPES:
        run = lambda x_: ops.layernorm(x_.cuda(), g.cuda(), b.cuda(), t, gelu=gelu)
        fails.append(_held(str(t), run(xp), run(x), torch.isnan(ref)))
    assert int(torch.isnan(ref).sum()) == D
    _no(fails)


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_stats_cast_poison(ops, dtype):
    """vf_row_stats_cast2: the poisoned row's statistics are NaN; its 16-bit copy keeps every finite element."""
    rows, D = 37, 200
    x = _rand((rows, D), 1510, 2.0)
    xp = x.clone()
    xp[5, 7] = NAN
    with ops.compute_dtype(N.tdt(dtype)):
        clean, got = ops.ln_stream(x.cuda()), ops.ln_stream(xp.cuda())
    _no([_held("x16", got.x16, clean.x16, torch.isnan(xp.double() * clean.scale)),
         _held("stats", got.stats, clean.stats, torch.isnan(N.ln_stats_ref(xp)))])


@pytest.mark.parametrize("dtype", DTYPES)
def test_embed_poison(ops, dtype):
    """One element of one table row: vf_embed_pack's rows, vf_embed_stream's 16-bit copy, trunk copy and statistics change
    for the tokens with that id only."""
    W, L, d, V = 9, 70, 128, 50
    g = torch.Generator().manual_seed(1520)
    ids = torch.randint(0, V, (W, L), generator=g)
    pad = torch.rand((W, L), generator=g) < 0.3
    pad[2] = True
    table, pos = _rand((V, d), 1521, 2.0), _rand((L, d), 1522)
    tp = table.clone()
    tp[17, 5] = NAN
    keep = ~pad
    x = (tp[ids] + pos[None])[keep].double()
    assert 0 < int(torch.isnan(x).any(dim=1).sum()) == int((ids[keep] == 17).sum()) < x.shape[0]
    n = int(keep.sum())
    with ops.compute_dtype(N.tdt(dtype)):
        cu = ops.mask_to_cu_seqlens(pad.cuda())
        run_p = lambda tb: ops.embed_pack(ids.cuda(), pad.cuda(), cu, tb.cuda(), pos.cuda(), n)
        run_s = lambda tb: ops.embed_stream(ids.cuda(), pad.cuda(), cu, tb.cuda(), pos.cuda(), n, need_x=True, need_t16=True)
        got, clean = run_s(tp), run_s(table)
        fails = [_held("embed_pack", run_p(tp), run_p(table), torch.isnan(x))]
    fails += [_held("x", got.x, clean.x, torch.isnan(x)), _held("x16", got.x16, clean.x16, torch.isnan(x)),
              _held("t16", got.t16, clean.t16, torch.isnan(x)), _held("stats", got.stats, clean.stats, torch.isnan(N.ln_stats_ref(x)))]
    _no(fails)


def test_segment_pools_poison(ops):
    """vf_segment_mean, vf_segment_mean16 (fp32 and split outputs), vf_segment_linear: one window, one column."""
    lens, d = [3, 1, 70, 20], 64
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    x = _rand((sum(lens), d), 1530, 2.0)
    xp = x.clone()
    xp[int(cu[2]) + 40, 9] = NAN
    fails = []
    mean = lambda x_: torch.stack([x_[int(cu[w]):int(cu[w + 1])].double().mean(dim=0) for w in range(len(lens))])
    ref = torch.isnan(mean(xp))
    assert int(ref.sum()) == 1 and bool(ref[2, 9])
    for t in OUT_TYPES:
        fails.append(_held(f"mean {t}", ops.segment_mean(xp.cuda(), cu.cuda(), t), ops.segment_mean(x.cuda(), cu.cuda(), t), ref))
    for t in OUT_TYPES[1:]:
        f32 = lambda x_: ops.segment_mean16(x_.cuda().to(t), cu.cuda(), 0.5)
        fails.append(_held(f"mean16 {t}", f32(xp), f32(x), ref))
        split = lambda x_: ops.segment_mean16(x_.cuda().to(t), cu.cuda(), 0.5, split=True)
        fails.append(_held(f"mean16 split {t}", split(xp), split(x), torch.cat([ref, ref], dim=1)))
    L = 80
    pad = torch.ones((len(lens), L), dtype=torch.bool)
    for w, n in enumerate(lens):
        pad[w, 2:2 + n] = False
    lin_w, lin_b = _rand((L,), 1531), torch.tensor([0.37])
    lin = lambda x_: torch.stack([(lin_w[2:2 + n, None].double() * x_[int(cu[w]):int(cu[w]) + n].double()).sum(dim=0) + 0.37
                                  for w, n in enumerate(lens)])
    assert int(torch.isnan(lin(xp)).sum()) == 1
    for t in OUT_TYPES:
        run = lambda x_: ops.segment_linear(x_.cuda(), cu.cuda(), pad.cuda(), lin_w.cuda(), lin_b.cuda(), t)
        fails.append(_held(f"linear {t}", run(xp), run(x), torch.isnan(lin(xp))))
    _no(fails)


def test_row_movers_poison(ops):
    """vf_gather_rows_f32 (fp32 and 16-bit outputs, wide and narrow rows), vf_gather_rows_bf16, vf_affine_rows_f32,
    vf_add_rows_f32: the output rows that read the poisoned source row, at the poisoned column."""
    fails = []
    for d in (64, 6):
        a, b = _rand((20, d), 1540, 2.0), _rand((7, d), 1541, 2.0)
        ap, bp = a.clone(), b.clone()
        ap[11, 1], bp[3, 2] = NAN, NAN
        idx = torch.tensor([0, 11, -1, -4, 11, 19, -4, 5], dtype=torch.int64)
        want = lambda a_, b_: torch.stack([a_[i] if i >= 0 else b_[-i - 1] for i in idx.tolist()])
        ref = torch.isnan(want(ap, bp))
        assert int(ref.sum()) == 4
        for t in (OUT_TYPES if d % 4 == 0 else OUT_TYPES[:1]):
            run = lambda a_, b_: ops.gather_rows_f32(a_.cuda(), b_.cuda(), idx.cuda(), t)
            fails.append(_held(f"gather_f32 d={d} {t}", run(ap, bp), run(a, b), ref))
    a = _rand((20, 64), 1542, 2.0)
    ap = a.clone()
    ap[11, 1] = NAN
    idx = torch.tensor([0, 11, 3, 11, 19], dtype=torch.int64)
    for t in OUT_TYPES[1:]:
        run = lambda a_: ops.gather_rows_bf16(a_.cuda().to(t), idx.cuda())
        fails.append(_held(f"gather16 {t}", run(ap), run(a), torch.isnan(ap[idx])))
    scale, shift = _rand((5,), 1543, 3.0), _rand((5,), 1544, 3.0)
    run = lambda a_, sc, sh: ops.affine_rows(a_.cuda(), idx.cuda(), sc.cuda(), sh.cuda())
    fails.append(_held("affine src", run(ap, scale, shift), run(a, scale, shift), torch.isnan(ap[idx])))
    sp = scale.clone()
    sp[2] = NAN
    fails.append(_held("affine scale", run(a, sp, shift), run(a, scale, shift),
                       torch.isnan(a[idx].double() * sp.double()[:, None] + shift.double()[:, None])))
    b = _rand((5, 64), 1545, 2.0)
    bp = b.clone()
    bp[4, 60] = NAN
    run = lambda a_, b_: ops.add_rows(a_.cuda(), b_.cuda(), idx.cuda(), None)
    fails.append(_held("add_rows a", run(ap, b), run(a, b), torch.isnan(ap[idx] + b)))
    fails.append(_held("add_rows b", run(a, bp), run(a, b), torch.isnan(a[idx] + bp)))
    _no(fails)


@pytest.mark.parametrize("softplus", [True, False])
def test_rowdot_softplus_poison(ops, softplus):
    n, d = 9, 64
    x, w, b = _rand((n, d), 1550, 2.0), _rand((d,), 1551, 0.5), torch.tensor([0.25])
    x[1] *= 30.0                                             # beyond the threshold 20
    xp = x.clone()
    xp[6, 3] = NAN
    y = xp.double() @ w.double() + 0.25
    ref = (F.softplus(y) if softplus else y)[:, None]
    run = lambda x_: ops.rowdot_softplus(x_.cuda(), w.cuda(), b.cuda(), softplus=softplus)
    assert int(torch.isnan(ref).sum()) == 1
    _no([_held("rowdot", run(xp), run(x), torch.isnan(ref))])


@pytest.mark.parametrize("dtype", DTYPES)
def test_softmax_counted_poison(ops, dtype):
    """One logit of one (token, head): its C weights are NaN (softmax of a NaN, as torch.softmax gives it; the padding slots
    c >= C stay zero, as include/vf_hip.h defines them), nothing else moves."""
    H, Cp, C = 8, 10, 9
    lens = [40, 1, 0, 33]
    T = sum(lens)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    sc = _rand((T, H * Cp), 1560, 4.0)
    cnt = torch.from_numpy(np.random.default_rng(2).integers(0, 50, (len(lens), C))).float()
    cnt[3, 0] = 0
    cnt[:, 4] += 1
    scp = sc.clone()
    tok, h = int(cu[3]) + 7, 5
    scp[tok, h * Cp + 4] = NAN

    def ref(s):
        out = torch.zeros(T, H, Cp, dtype=torch.float64)
        for b in range(len(lens)):
            a, e = int(cu[b]), int(cu[b + 1])
            lg = s[a:e].double().view(-1, H, Cp)[:, :, :C] * math.log(2.0) + torch.log(cnt[b].double())     # -inf: absent
            out[a:e, :, :C] = torch.softmax(lg, dim=-1)
        return out.view(T, H * Cp)
    run = lambda s: ops.softmax_counted(s.cuda(), torch.log2(cnt).cuda().contiguous(), cu.cuda(), max(lens), H, Cp, out_dtype=N.tdt(dtype))
    want = torch.isnan(ref(scp))
    assert int(want.sum()) == C and bool(want[tok, h * Cp:h * Cp + C].all())
    _no([_held("softmax_counted", run(scp), run(sc), want)])


@pytest.mark.parametrize("where", ["k", "v"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dh,H", [(48, 8), (64, 4)])
def test_attn_counted_keys_poison(ops, dh, H, dtype, where):
    """A NaN in table row c* (K half: every column of head*; V half: one column of it) reaches exactly the sequences whose
    count for c* is non-zero; a sequence with log2_count = -inf for it keeps the bits of the clean launch.  The reference
    attends over the rows a sequence holds."""
    t = N.tdt(dtype)
    D, C, cs, hs = H * dh, 9, 4, H // 2
    lens = [30, 1, 77, 5]
    tq = sum(lens)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    q = _rand((tq, D), 1570, 1.2).to(t).float()
    tab = _rand((C, 2 * D), 1571, 1.5).to(t).float()
    cnt = torch.from_numpy(np.random.default_rng(3).integers(1, 20, (len(lens), C))).float()
    cnt[0, cs] = 0                                            # sequences 0 and 3 do not hold row c*
    cnt[3, cs] = 0
    cnt[3, 1] = 0
    tp = tab.clone()
    tp[cs, (0 if where == "k" else D) + hs * dh + 5] = NAN

    def ref(tb):
        out = torch.zeros(tq, D, dtype=torch.float64)
        for b in range(len(lens)):
            a, e = int(cu[b]), int(cu[b + 1])
            present = cnt[b] > 0
            kk, vv = tb[present, :D].double().view(-1, H, dh), tb[present, D:].double().view(-1, H, dh)
            s = torch.einsum("qhd,chd->hqc", q[a:e].double().view(-1, H, dh), kk) * math.log(2.0) + torch.log(cnt[b][present].double())
            out[a:e] = torch.einsum("hqc,chd->qhd", torch.softmax(s, dim=-1), vv).reshape(e - a, D)
        return out
    run = lambda tb: ops.attn_counted_keys(q.cuda().to(t), tb.cuda().to(t), torch.log2(cnt).cuda().contiguous(), cu.cuda(), max(lens), H, dh)
    want = torch.isnan(ref(tp))
    rows = torch.zeros(tq, dtype=torch.bool)
    rows[int(cu[1]):int(cu[3])] = True                        # sequences 1 and 2
    assert torch.equal(want.any(dim=1), rows) and int(want[int(cu[1])].sum()) == (dh if where == "k" else 1)
    _no([_held("attn_counted_keys", run(tp), run(tab), want)])


# ---------------------------------------------------------------------------------------------
# store rounding: bit-exact against torch's cast
# ---------------------------------------------------------------------------------------------
def _bias_of(vals: torch.Tensor, n: int) -> torch.Tensor:
    return vals[torch.arange(n) % vals.numel()].contiguous()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("epi", N.OUT16_EPILOGUES)
@pytest.mark.parametrize("path,M,N_,K", N.GEMM_PATHS)
def test_gemm_16bit_epilogues_round_like_torch(ops, path, M, N_, K, epi, dtype):
    """A = 0, so the accumulator is +0 and the epilogue hands its store exactly 0 + bias (-0.0 arrives as +0.0: an addition,
    not a rounding): every special value through VF_EPI_BF16; those with gelu(v) = v in fp32 (v >= 16) through
    VF_EPI_GELU_BF16; 32 v through VF_EPI_GEGLU_BF16 with the gate bias 32 (gelu(32) = 32)."""
    t = N.tdt(dtype)
    vals = N.special_tensor(dtype)
    if epi == "gelu_bf16":
        vals = vals[vals >= 16]
    n = N.GEGLU_N[N_] if epi == "geglu" else N_
    n_val = n // 2 if epi == "geglu" else n
    assert n_val >= vals.numel()
    bias = _bias_of(vals, n_val)
    want = (torch.zeros(()) + bias)
    if epi == "geglu":
        bias = torch.cat([bias, torch.full((n_val,), 32.0)])
        want = want * 32.0
    a = torch.zeros((M, K))
    w = N.gemm_operands(M, n, K, dtype)[1]
    got = _gemm(ops, path, epi, dtype, a, w, bias, None)
    assert N.same_16bit(got, want.to(t)[None].expand(M, n_val))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("epi", ["bf16", "geglu"])
def test_gemm_ln_consumer_rounds_like_torch(ops, epi, dtype):
    """The LayerNorm consumer's 16-bit stores: x16 = 0 and statistics (mean, rstd) = (0, 1) make rstd * (0 - 0 * colsum) + bias
    = 0 + bias what the epilogue hands over; VF_EPI_GEGLU_BF16 with the gate bias 32 as above."""
    t = N.tdt(dtype)
    M, n, K = N.LN_M, N.LN_N, N.LN_K
    vals = N.special_tensor(dtype)
    n_val = n // 2 if epi == "geglu" else n
    bias = _bias_of(vals, n_val)
    want = torch.zeros(()) + bias
    if epi == "geglu":
        bias = torch.cat([bias, torch.full((n_val,), 32.0)])
        want = want * 32.0
    wd, bd = N.gemm_operands(M, n, K, dtype)[1].cuda().to(t), bias.cuda()
    if epi == "geglu":
        wd, bd = ops.pack_geglu_rows(wd, bd)
    stats = torch.tensor([0.0, 1.0]).repeat(M, 1).cuda()
    s = ops.LnStream(None, torch.zeros((M, K), dtype=t, device="cuda"), stats, 1.0)
    got = ops.gemm_ln_consumer(s, wd, bd, wd.float().sum(dim=1).contiguous(), _epi_code(ops, epi))
    assert N.same_16bit(got, want.to(t)[None].expand(M, n_val))


@pytest.mark.parametrize("dtype", DTYPES)
def test_fold_alert_and_non_finite_rows(ops, dtype, monkeypatch):
    """The range bit of the LayerNorm-fold alert (bit 1) says that a 16-bit copy of a FINITE fp32 row may overflow -- which the
    separate LayerNorm mends.  A row that holds a NaN or an Inf has NaN statistics, nothing mends it, and recomputing the
    batch for it would move its batch-mates' bits: such rows raise nothing, from the producer GEMM's statistics
    (vf_ln_finalize2) and from vf_row_stats_cast2 alike; 2e6 next to them in the same launch still raises bit 1."""
    monkeypatch.delenv("VF_TRUNK16", raising=False)        # the default (fp16 trunk copy) whatever the ambient switch
    t = N.tdt(dtype)
    dev = torch.device("cuda", torch.cuda.current_device())
    M, n, K = N.LN_M, N.LN_N, N.LN_K
    a, w, bias, res = N.gemm_operands(M, n, K, dtype, seed=760)
    with ops.compute_dtype(t):
        assert ops.ln_fold_abs_limit() > 0                 # the default configuration has an fp16 copy: the bit is armed
        for label, value, want in (("clean", None, 0), ("nan", NAN, 0), ("+inf", N.INF, 0), ("-inf", -N.INF, 0), ("2e6", 2.0e6, 2)):
            rp = res.clone()
            if value is not None:
                rp[5, 7] = value
            ops.ln_fold_alert(dev)
            _producer(ops, "res32", dtype, a, w, bias, rp)
            assert ops.ln_fold_alert(dev) == want, ("producer", label)
            ops.ln_stream(rp.cuda())
            assert ops.ln_fold_alert(dev) == want, ("row_stats_cast", label)
        rp = res.clone()
        rp[5, 7], rp[200, 3] = NAN, 2.0e6                   # both in one launch: the finite row still speaks
        _producer(ops, "res32", dtype, a, w, bias, rp)
        assert ops.ln_fold_alert(dev) == 2
        ops.ln_stream(rp.cuda())
        assert ops.ln_fold_alert(dev) == 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["f32", "t16"])
def test_gemm_ln_producer_copies_round_like_torch(ops, kind, dtype):
    """out16 = round16(x * x16_scale) and t16_out = fp16(x * t16_scale), x = 0 + bias: the special values and 16 times them
    (the scales are 1 or 2^-4, so both sides of every boundary reach the store)."""
    t = N.tdt(dtype)
    M, n, K = N.LN_M, N.LN_N, N.LN_K
    vals = torch.cat([N.special_tensor(dtype), N.special_tensor("fp16"), N.special_tensor(dtype) * 16.0, N.special_tensor("fp16") * 16.0])
    assert vals.numel() <= n
    bias = _bias_of(vals, n)
    w = N.gemm_operands(M, n, K, dtype)[1]
    got = _producer(ops, kind, dtype, torch.zeros((M, K)), w, bias, torch.zeros((M, n)))
    x = torch.zeros(()) + bias
    assert N.same_16bit(got.x16, (x * got.scale).to(t)[None].expand(M, n))
    if kind == "t16":
        assert N.same_16bit(got.t16, (x * ops.T16_SCALE).half()[None].expand(M, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_streaming_stores_round_like_torch(ops, dtype):
    """The special values handed over directly: vf_cast_f32_bf16 / _f16 (lengths with and without a scalar tail),
    vf_gather_rows_f32 to 16 bits, vf_segment_mean of one-token windows (x / 1)."""
    t = N.tdt(dtype)
    x = N.special_tensor(dtype)
    n = x.numel()
    for m in (n, n - 1, n - 2, n - 3):
        assert N.same_16bit(ops.cast16(x[:m].contiguous().cuda(), t), x[:m].to(t)), m
    assert any(m % 4 for m in (n, n - 1)) and any(m % 4 == 0 for m in (n, n - 1, n - 2, n - 3))
    d = 8
    rows = x[torch.arange(5 * n * d) % n].view(5 * n, d)[torch.randperm(5 * n, generator=torch.Generator().manual_seed(1600))].contiguous()
    idx = torch.randperm(5 * n, generator=torch.Generator().manual_seed(1601))
    assert N.same_16bit(ops.gather_rows_f32(rows.cuda(), None, idx.cuda(), t), rows[idx].to(t))
    cu = torch.arange(5 * n + 1, dtype=torch.int32)
    # (the kernel's sum starts at +0: (0 + x) * (1 / 1) -- exact, except that -0.0 arrives as +0.0, an addition, not a rounding)
    assert N.same_16bit(ops.segment_mean(rows.cuda(), cu.cuda(), t), (torch.zeros(()) + rows).to(t))


# ---------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16-mixed", "16-mixed"])
def test_model_nan_gene_stays_in_its_gene(precision):
    """The two-layer model of test_tissue_invariance_and_batch_independence, three genes; the CRE tokenizer's embedding row of
    a token that only gene 1's windows hold is set to NaN in place (the parameter's version moves, so the caches of
    weights.derived rebuild): genes 0 and 2 keep the bits of the clean run of the same batch, every tissue of gene 1 is NaN,
    and with the row restored a third run gives the clean bits again."""
    model = build_model(SEQ2REG_512, seq2gene_kw(layers=2), seed=7).cuda()
    model.precision = precision
    batch, tok = N.model_batch()
    clean = model.predict_step(batch, 0)
    weight = model.cre_tokenizer.token_embedding.weight
    saved = weight.detach()[tok].clone()
    with torch.no_grad():
        weight[tok] = NAN
    bad = model.predict_step(batch, 0)
    with torch.no_grad():
        weight[tok] = saved
    again = model.predict_step(batch, 0)
    for key in ("pred_gene_exp", "embeddings"):
        for g in range(3):
            assert np.isfinite(clean[key][g]).all()
            np.testing.assert_array_equal(again[key][g].view(np.int32), clean[key][g].view(np.int32))
        for g in (0, 2):
            np.testing.assert_array_equal(bad[key][g].view(np.int32), clean[key][g].view(np.int32))
    assert np.isnan(bad["pred_gene_exp"][1]).all() and bad["pred_gene_exp"][1].shape == clean["pred_gene_exp"][1].shape

"""Edges the per-kernel suite (tests/test_ops_gpu.py) does not reach, on a real MI355X: ALiBi with len_q != len_k in both
alignments for every attention kernel family, row-strided operands and outputs with sentinels around them, and the
streaming kernels that had no test of their own.  References are the CPU oracle (attention) or float64 torch.

ops.gemm_ln_producer / gemm_ln_consumer take no `out`, `out16` or `x16` argument -- they allocate contiguous results
themselves -- so there is no strided OUTPUT of theirs to surround with sentinels; the producer's row-strided INPUTS
(a, residual, trunk16) are held to the bits of the contiguous call."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vf_oracle as O
from tests import attn_edge_cases as E
from tests.helpers import _bf, _rand

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from variantformer_amd import ops as _ops
    from variantformer_amd import _lib
    _lib.load()      # must be the in-tree HIP library; raises if missing
    return _ops


def _tdt(dtype):
    return torch.bfloat16 if dtype == "bf16" else torch.float16


def _sentinel(shape, tdt):
    """A buffer no kernel result can be mistaken for: NaN (fp32) / the quiet-NaN pattern 0x7FC1 (16-bit types)."""
    if tdt == torch.float32:
        return torch.full(shape, float("nan"), device="cuda")
    return torch.full(shape, 0x7FC1, dtype=torch.int16, device="cuda").view(tdt)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _assert_outside_untouched(big, before, c0, c1):
    """Every element of `big` outside the columns [c0, c1) still holds the bits of `before`."""
    now, was = _bits(big), _bits(before)
    assert torch.equal(now[:, :c0], was[:, :c0]) and torch.equal(now[:, c1:], was[:, c1:])


# ---------------------------------------------------------------------------------------------
# B. ALiBi x unequal lengths x both alignments, per kernel family
# ---------------------------------------------------------------------------------------------
def _run_case(ops, c, dtype, q_log2, q_at_start):
    tdt = _tdt(dtype)
    q, k, v = E.operands(c.name, dtype, q_log2)
    out = ops.attn_varlen(q.cuda().to(tdt), k.cuda().to(tdt), v.cuda().to(tdt), E.cu_of(c.ql).cuda(), E.cu_of(c.kl).cuda(),
                          max(c.ql), max(c.kl), c.H, c.dh, E.slopes_of(c).cuda(), q_at_start=q_at_start, q_log2=q_log2)
    name = ops.last_kernel("attn")
    torch.cuda.synchronize()
    return out, name


@pytest.mark.parametrize("q_at_start", [False, True])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name,q_log2", E.CASE_PARAMS)
def test_alibi_unequal_lengths_both_alignments(ops, name, q_log2, dtype, q_at_start):
    """Every output element of every kernel family against O.attention(..., q_at_start=...) on sequences with sq > sk,
    sk - sq == 1, sk == sq and large gaps either way, at the tolerances of test_ops_gpu.py.  tests/test_oracle_alibi_cpu.py
    shows on the same operands that the opposite alignment could not pass.  attn_short_kernel is reachable: 225 ... 256
    keys at dh <= 48 do not fit three LDS images per CU (tests/attn_edge_cases.py)."""
    c = E.CASES_BY_NAME[name]
    out, kernel = _run_case(ops, c, dtype, q_log2, q_at_start)
    assert kernel == c.kernel, kernel
    rnd = O.Rounding(dtype)
    want = rnd.r(E.oracle_rows(c, dtype, q_log2, q_at_start))
    got = out.float().cpu()
    cu_q = E.cu_of(c.ql)
    for b, sk in enumerate(c.kl):
        if sk == 0:
            assert float(got[int(cu_q[b]):int(cu_q[b + 1])].abs().max()) == 0.0
    np.testing.assert_allclose(got.numpy(), want.numpy(), **E.tolerance(dtype))


@pytest.mark.parametrize("q_at_start", [False, True])
def test_alibi_unequal_lengths_are_kernel_independent(ops, q_at_start):
    """With VF_ATTN_Q_LOG2 the ALiBi bias is the same fused multiply-add in every kernel: unequal-length sequences give the
    same bits in a batch the one-block-per-sequence kernel serves and next to a 300-token sequence (tiled kernel)."""
    c = E.CASES_BY_NAME["short2_2pass_dh48"]
    H, dh = c.H, c.dh
    D = H * dh
    q, k, v = E.operands(c.name, "bf16", True)
    q = torch.cat([q, _bf(_rand((300, D), 81, 0.4))])
    kv = torch.cat([torch.cat([k, v], dim=1), _bf(_rand((300, 2 * D), 82, 2.0))])
    dq, dkv = q.cuda().bfloat16(), kv.cuda().bfloat16()
    slopes = E.slopes_of(c).cuda()

    def run(ql, kl):
        tq, tk = sum(ql), sum(kl)
        o = ops.attn_varlen(dq[:tq], dkv[:tk, :D], dkv[:tk, D:], E.cu_of(ql).cuda(), E.cu_of(kl).cuda(), max(ql), max(kl), H, dh,
                            slopes, q_at_start=q_at_start, q_log2=True)
        return o, ops.last_kernel("attn")
    short, k_short = run(list(c.ql), list(c.kl))
    tiled, k_tiled = run(list(c.ql) + [300], list(c.kl) + [300])
    torch.cuda.synchronize()
    assert k_short == E.SHORT2_2 and k_tiled.startswith("attn_fwd_kernel"), (k_short, k_tiled)
    assert torch.equal(short.view(torch.int16), tiled[:sum(c.ql)].view(torch.int16))


# ---------------------------------------------------------------------------------------------
# C. strided operands, with sentinels
# ---------------------------------------------------------------------------------------------
def _gemm_strided(ops, M, N, K, epi, variant, dtype, check_ref=False):
    tdt = _tdt(dtype)
    rd = (lambda t: t.to(tdt).float())
    code = {"bf16": ops.EPI_BF16, "f32": ops.EPI_F32, "res": ops.EPI_RES_F32, "gelu_bf16": ops.EPI_GELU_BF16,
            "geglu": ops.EPI_GEGLU_BF16}[epi]
    n_out = N // 2 if epi == "geglu" else N
    odt = torch.float32 if epi in ("f32", "res") else tdt
    big_a = rd(_rand((M, K + 24), 91)).cuda().to(tdt)
    a = big_a[:, 8:8 + K]
    w32 = rd(_rand((N, K), 92, 1.0 / math.sqrt(K)))
    b32 = _rand((N,), 93, 0.5)
    w, b = w32.cuda().to(tdt), b32.cuda()
    if epi == "geglu":
        w, b = ops.pack_geglu_rows(w, b)
    big_r = _rand((M, N + 24), 94).cuda()
    res = big_r[:, 8:8 + N] if epi == "res" else None
    big_o = _sentinel((M, n_out + 24), odt)
    before = big_o.clone()
    ops.gemm(a, w, b, code, residual=res, out=big_o[:, 8:8 + n_out], variant=variant)
    dense = ops.gemm(a.contiguous(), w, b, code, residual=None if res is None else res.contiguous(), variant=variant)
    torch.cuda.synchronize()
    assert torch.equal(_bits(big_o[:, 8:8 + n_out]), _bits(dense))
    _assert_outside_untouched(big_o, before, 8, 8 + n_out)
    if check_ref:                                  # (the tolerances of test_ops_gpu.py::test_gemm_epilogues / test_gemm_geglu)
        ref = big_a[:, 8:8 + K].float().cpu() @ w32.t() + b32
        if epi == "res":
            ref = ref + big_r[:, 8:8 + N].cpu()
        if epi == "gelu_bf16":
            ref = F.gelu(ref)
        if epi == "geglu":
            x, gate = ref.chunk(2, dim=-1)
            ref = x * F.gelu(gate)
        if odt == torch.float32:
            np.testing.assert_allclose(dense.cpu().numpy(), ref.numpy(), rtol=2e-5, atol=2e-5 * math.sqrt(K))
        else:
            np.testing.assert_allclose(dense.float().cpu().numpy(), ref.numpy(), rtol=2 ** -8, atol=2e-3)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("epi", ["bf16", "f32", "res", "gelu_bf16", "geglu"])
@pytest.mark.parametrize("variant", [0, 1, 5, 20, 22])
def test_gemm_row_strided_operands_leave_the_padding_alone(ops, variant, epi, dtype):
    """a, out and residual as column slices of wider buffers (row strides K + 24 / N_out + 24 / N + 24), M and N ragged
    against every tile: the slice holds the bits of the same call on contiguous copies and no store lands in the sentinel
    columns either side of it (a wide store stepping past column N would).  GEGLU needs N % 32 == 0: N = 800 there."""
    M, N, K = 515, (800 if epi == "geglu" else 776), 192
    _gemm_strided(ops, M, N, K, epi, variant, dtype, check_ref=(variant == 0))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("epi", ["bf16", "f32", "res", "gelu_bf16", "geglu"])
def test_gemm_row_strided_operands_generic_path(ops, epi, dtype):
    """The same on the generic path (K % 64 != 0; forced tile configurations do not apply).  GEGLU: N = 64."""
    _gemm_strided(ops, 77, 64 if epi == "geglu" else 40, 72, epi, 0, dtype, check_ref=True)


@pytest.mark.parametrize("res", ["f32", "trunk16"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gemm_ln_producer_row_strided_inputs(ops, dtype, res):
    """a and the residual (fp32 rows, or the fp16 trunk copy) as column slices of wider buffers: the fp32 rows, their 16-bit
    copy, the row statistics and the trunk copy hold the bits of the same call on contiguous copies (which
    tests/test_ops_gpu.py compares with the oracle)."""
    M, N, K = 515, 1536, 512
    tdt = _tdt(dtype)
    a = _rand((M, K + 24), 95).cuda().to(tdt)[:, 8:8 + K]
    w, b = _rand((N, K), 96, 1.0 / math.sqrt(K)).cuda().to(tdt), _rand((N,), 97, 0.5).cuda()
    r = _rand((M, N + 24), 98).cuda()
    if res == "trunk16":
        r = (r * ops.T16_SCALE).half()
    r = r[:, 8:8 + N]
    assert not a.is_contiguous() and not r.is_contiguous()

    def run(a_, r_):
        if res == "trunk16":
            return ops.gemm_ln_producer(a_, w, b, None, trunk16=r_, need_t16=True)
        return ops.gemm_ln_producer(a_, w, b, r_)
    with ops.compute_dtype(tdt):
        s, d = run(a, r), run(a.contiguous(), r.contiguous())
    torch.cuda.synchronize()
    assert torch.equal(_bits(s.x), _bits(d.x)) and torch.equal(_bits(s.x16), _bits(d.x16))
    assert torch.equal(_bits(s.stats), _bits(d.stats))
    if res == "trunk16":
        assert torch.equal(_bits(s.t16), _bits(d.t16))
    assert torch.isfinite(s.x).all()


@pytest.mark.parametrize("name", ["registry", "fwd128_dh48", "fwd128_dh96", "short2_2pass_dh48", "short2_1pass_dh64",
                                  "short2_2pass_dh64", "short_3groups", "short2_2pass_dh40"])
def test_attention_strided_output_and_packed_operands(ops, name):
    """out = a column slice of a sentinel-filled [tq, D + 32] buffer, q / k / v = slices of one [t, 3 D + 24] buffer: the bits
    of the contiguous call inside the slice, the sentinel outside; rows of a sequence without keys are zero inside only."""
    c = E.CASES_BY_NAME[name]
    q_log2 = c.q_log2[0]
    H, dh = c.H, c.dh
    D = H * dh
    ql, kl = list(c.ql), list(c.kl)
    if 0 not in kl:
        ql, kl = ql + [5], kl + [0]
    q, k, v = E.operands(c.name, "bf16", q_log2)
    tq, tk = sum(ql), sum(kl)
    q = torch.cat([q, _bf(_rand((tq - q.shape[0], D), 83, 0.4))])
    big = torch.zeros((max(tq, tk), 3 * D + 24), dtype=torch.bfloat16, device="cuda")
    big[:tq, 8:8 + D] = q.cuda().bfloat16()
    big[:tk, 8 + D:8 + 2 * D] = k.cuda().bfloat16()
    big[:tk, 8 + 2 * D:8 + 3 * D] = v.cuda().bfloat16()
    dq, dk, dv = big[:tq, 8:8 + D], big[:tk, 8 + D:8 + 2 * D], big[:tk, 8 + 2 * D:8 + 3 * D]
    args = (E.cu_of(ql).cuda(), E.cu_of(kl).cuda(), max(ql), max(kl), H, dh, E.slopes_of(c).cuda())
    big_o = _sentinel((tq, D + 32), torch.bfloat16)
    before = big_o.clone()
    ops.attn_varlen(dq, dk, dv, *args, out=big_o[:, 16:16 + D], q_log2=q_log2)
    assert ops.last_kernel("attn") == c.kernel, ops.last_kernel("attn")
    dense = ops.attn_varlen(dq.contiguous(), dk.contiguous(), dv.contiguous(), *args, q_log2=q_log2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(big_o[:, 16:16 + D]), _bits(dense))
    _assert_outside_untouched(big_o, before, 16, 16 + D)
    cu_q = E.cu_of(ql)
    z = kl.index(0)
    assert float(dense[int(cu_q[z]):int(cu_q[z + 1])].float().abs().max()) == 0.0
    assert torch.isfinite(dense.float()).all()


# ---------------------------------------------------------------------------------------------
# D. streaming kernels with no test of their own
# ---------------------------------------------------------------------------------------------
DS = [4, 100, 512, 1536, 2052]      # one vector; not a multiple of 256 lanes; two sizes that need a second stride of the block


@pytest.mark.parametrize("d", DS)
def test_segment_max(ops, d):
    """Equal to torch.max over each window: negative values only (a maximum started at 0 would show), -inf for the empty
    window, and a NaN in a window makes that column NaN as torch.max does (include/vf_hip.h states the rule)."""
    lens = [3, 1, 200, 0, 77]
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    x = -(_rand((sum(lens), d), 111).abs() * 3.0 + 0.01)
    x[int(cu[2]) + 5, 1] = float("nan")                 # followed by 194 ordinary rows: the fold must not drop it again
    x[int(cu[5]) - 1, d - 1] = float("nan")             # the last row of the last window
    got = ops.segment_max(x.cuda(), cu.cuda()).cpu()
    for w, n in enumerate(lens):
        a = int(cu[w])
        want = x[a:a + n].max(dim=0).values if n else torch.full((d,), float("-inf"))
        assert torch.equal(torch.isnan(got[w]), torch.isnan(want)), w
        ok = ~torch.isnan(want)
        assert torch.equal(got[w][ok], want[ok]), w
    assert bool(torch.isnan(got[2, 1])) and bool(torch.isnan(got[4, d - 1])) and int(torch.isnan(got).sum()) == 2


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("L", [1, 63, 64, 65, 200])
def test_segment_linear(ops, L, d):
    """out[w] = sum over the valid positions p of lin_w[p] * x[row(w, p)] + lin_b against the dense zero-masked [W, L, d]
    tensor times lin_w in float64: non-suffix masks, a fully padded window (the result is lin_b), a fully valid one; with
    and without lin_b; fp32 to rtol 1e-6 plus the bound of a sequential fp32 sum of L terms (L eps32 sum |terms|), the
    16-bit outputs equal to RNE of the fp32 output."""
    W = 6
    g = torch.Generator().manual_seed(120 + L)
    pad = torch.rand((W, L), generator=g) < 0.4
    pad[0] = True                       # fully padded
    pad[1] = False                      # fully valid
    pad[2] = False
    pad[2, 0] = True                    # a hole at the front: not a suffix mask
    pad[3, L - 1] = False
    keep = ~pad
    n = int(keep.sum())
    x = _rand((max(n, 1), d), 121, 2.0)[:n]
    lin_w, lin_b = _rand((L,), 122), torch.tensor([0.37])
    dense = torch.zeros((W, L, d), dtype=torch.float64)
    dense[keep] = x.double()
    lens = keep.sum(1)
    cu = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).to(torch.int32)
    base = torch.einsum("wld,l->wd", dense, lin_w.double())
    bound = L * EPS32 * (torch.einsum("wld,l->wd", dense.abs(), lin_w.double().abs()) + 0.37)
    for b in (lin_b, None):
        want = base + (0.37 if b is not None else 0.0)
        o32 = ops.segment_linear(x.cuda(), cu.cuda(), pad.cuda(), lin_w.cuda(), None if b is None else b.cuda(), torch.float32).cpu()
        err = (o32.double() - want).abs()
        assert bool((err <= 1e-6 * want.abs() + bound).all()), float((err - bound).max())
        assert torch.equal(o32[0], torch.full((d,), 0.37 if b is not None else 0.0))
        for tdt in (torch.bfloat16, torch.float16):
            o16 = ops.segment_linear(x.cuda(), cu.cuda(), pad.cuda(), lin_w.cuda(), None if b is None else b.cuda(), tdt).cpu()
            assert torch.equal(o16, o32.to(tdt))


@pytest.mark.parametrize("d,n", [(4, 2048 * 256 + 77), (100, 37), (512, 37), (1536, 37), (2052, 300)])
@pytest.mark.parametrize("use_scale,use_shift", [(False, False), (True, False), (False, True), (True, True)])
def test_affine_rows(ops, d, n, use_scale, use_shift):
    """out[i] = src[idx[i]] * scale[i] + shift[i], repeated and out-of-order idx; d = 4 with more rows than one pass of the
    grid covers.  With one of the two absent the value is a single fp32 operation: bit exact.  With both the kernel
    computes the FUSED form fma(src, scale, shift) (the compiler contracts the expression): within one fp32 ulp of the
    float64 value, which the unfused form is not held to."""
    rows = 23
    src = _rand((rows, d), 131, 2.0)
    idx = torch.randint(0, rows, (n,), generator=torch.Generator().manual_seed(132))
    idx[:4] = torch.tensor([rows - 1, 0, 0, rows - 1])
    scale = _rand((n,), 133, 3.0) if use_scale else None
    shift = _rand((n,), 134, 3.0) if use_shift else None
    got = ops.affine_rows(src.cuda(), idx.cuda(), None if scale is None else scale.cuda(),
                          None if shift is None else shift.cuda()).cpu()
    g = src[idx]
    if use_scale and use_shift:
        want = g.double() * scale.double()[:, None] + shift.double()[:, None]
        ulp = torch.from_numpy(np.spacing(np.abs(want.float().numpy()))).double()
        assert bool(((got.double() - want).abs() <= ulp).all())
    else:
        want = g * scale[:, None] if use_scale else (g + shift[:, None] if use_shift else g)
        assert torch.equal(got, want)


@pytest.mark.parametrize("d,n", [(4, 2048 * 256 + 77), (100, 41), (512, 41), (1536, 41), (2052, 300)])
@pytest.mark.parametrize("use_a,use_b", [(False, False), (True, False), (False, True), (True, True)])
def test_add_rows(ops, d, n, use_a, use_b):
    ra, rb = (19 if use_a else n), (7 if use_b else n)
    a, b = _rand((ra, d), 141, 2.0), _rand((rb, d), 142, 2.0)
    ia = torch.randint(0, ra, (n,), generator=torch.Generator().manual_seed(143)) if use_a else None
    ib = torch.randint(0, rb, (n,), generator=torch.Generator().manual_seed(144)) if use_b else None
    got = ops.add_rows(a.cuda(), b.cuda(), None if ia is None else ia.cuda(), None if ib is None else ib.cuda()).cpu()
    want = (a[ia] if use_a else a) + (b[ib] if use_b else b)
    assert torch.equal(got, want)                                  # one fp32 add


@pytest.mark.parametrize("d", [4, 1536])
@pytest.mark.parametrize("n", [1, 4, 5])
@pytest.mark.parametrize("softplus,use_b", [(True, True), (True, False), (False, True), (False, False)])
def test_rowdot_softplus_branches(ops, d, n, softplus, use_b):
    """Affine value or softplus of it, with and without b; four rows per block (n = 1, 4, 5); pre-activations of -100
    (log1p(exp) underflows), either side of the threshold 20, and ordinary ones; against float64."""
    targets = torch.tensor([19.6, -100.0, 20.4, 0.3, 33.0])[:n]
    x = _rand((n, d), 151, 0.01)
    w = _rand((d,), 152, 0.05)
    w[0] = 1.0
    b = torch.tensor([0.25]) if use_b else None
    x[:, 0] = 0.0
    x[:, 0] = targets - (x.double() @ w.double()).float() - (0.25 if use_b else 0.0)
    y = x.double() @ w.double() + (0.25 if use_b else 0.0)
    want = torch.log1p(torch.exp(y)) if softplus else y          # (float64: no threshold needed; the kernel's 20 is its own)
    got = ops.rowdot_softplus(x.cuda(), w.cuda(), None if b is None else b.cuda(), softplus=softplus).cpu()
    assert got.shape == (n, 1)
    # fp32 dot product of d terms (d eps32 sum |terms|), then expf / log1pf to a few ulp
    atol = (d + 2) * EPS32 * float((x.double().abs() @ w.double().abs()).max() + 0.25)
    np.testing.assert_allclose(got[:, 0].double().numpy(), want.numpy(), rtol=1e-6, atol=atol)
    if softplus and n >= 2:
        assert 0.0 <= float(got[1, 0]) <= 1e-40                     # -100: exp underflows to (almost) nothing, not to garbage


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 4099])
def test_cast16_tail(ops, n, dtype):
    """n % 4 != 0 runs the scalar tail: bit exact against tensor.to(), and the element after n stays as it was."""
    from variantformer_amd import _lib
    tdt = _tdt(dtype)
    x = _rand((n,), 161, 4.0)
    x[0] = 1.0 + 2.0 ** -8 if dtype == "bf16" else 1.0 + 2.0 ** -11           # a tie: rounds to even
    if n >= 3:
        x[n - 1], x[n - 2] = -0.0, 70000.0                                          # (beyond fp16's range: inf there)
    assert torch.equal(ops.cast16(x.cuda(), tdt).cpu(), x.to(tdt))
    out = _sentinel((1, n + 9), tdt)
    before = out.clone()
    lib = _lib.load()
    fn = lib.vf_cast_f32_f16 if dtype == "fp16" else lib.vf_cast_f32_bf16
    xd = x.cuda()
    _lib.check(fn(xd.data_ptr(), out.data_ptr(), n, torch.cuda.current_stream().cuda_stream), "vf_cast_f32_16")
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[:, :n]), _bits(x.to(tdt)[None].cuda()))
    _assert_outside_untouched(out, before, 0, n)


@pytest.mark.parametrize("d", [2, 6, 1])
def test_gather_rows_f32_narrow_rows(ops, d):
    """d % 4 != 0 (the [rows, 2] LayerNorm statistics) runs the one-element-per-thread kernel; negative indices pick b."""
    a, b = _rand((50, d), 171), _rand((9, d), 172)
    idx = torch.tensor([0, 49, -1, -9, 7, 7, -3, 48], dtype=torch.int64)
    want = torch.stack([a[i] if i >= 0 else b[-i - 1] for i in idx.tolist()])
    assert torch.equal(ops.gather_rows_f32(a.cuda(), b.cuda(), idx.cuda()).cpu(), want)
    big = torch.randint(-9, 50, (70001,), generator=torch.Generator().manual_seed(173))
    want = torch.where((big >= 0)[:, None], a[big.clamp(min=0)], b[(-big - 1).clamp(min=0)])
    assert torch.equal(ops.gather_rows_f32(a.cuda(), b.cuda(), big.cuda()).cpu(), want)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("d", [8, 384, 2056])
def test_gather_rows16_strided(ops, d, dtype):
    """Row-strided source and destination (ld_src, ld_out != d), through the C entry: exact rows, sentinels untouched."""
    from variantformer_amd import _lib
    tdt = _tdt(dtype)
    big_s = _rand((9, d + 24), 181).to(tdt).cuda()
    idx = torch.tensor([8, 0, 0, 3, 5, 8, 1], dtype=torch.int64)
    big_o = _sentinel((idx.numel(), d + 40), tdt)
    before = big_o.clone()
    src, out = big_s[:, 8:8 + d], big_o[:, 16:16 + d]
    di = idx.cuda()
    _lib.check(_lib.load().vf_gather_rows_bf16(src.data_ptr(), src.stride(0), di.data_ptr(), out.data_ptr(), out.stride(0),
                                               idx.numel(), d, torch.cuda.current_stream().cuda_stream), "vf_gather_rows_bf16")
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(src[di]))
    _assert_outside_untouched(big_o, before, 16, 16 + d)


@pytest.mark.parametrize("with_pos", [False, True])
def test_token_keys(ops, with_pos):
    """keys = id * key_L + position (key_L = L) or the ids themselves (key_L = 1) of the packed valid tokens, ids clamped
    to [0, vocab); non-suffix masks over two 64-position rounds, an empty window; equal to a Python loop."""
    W, L, V = 7, 70, 500
    g = torch.Generator().manual_seed(191)
    ids = torch.randint(0, V, (W, L), generator=g)
    ids[1, 3], ids[1, 4], ids[3, 69], ids[4, 0] = -5, V, V + 1000, -1
    pad = torch.rand((W, L), generator=g) < 0.35
    pad[1] = False
    pad[2] = True                                   # empty window
    pad[4, 0] = False
    pad[3, 69] = False
    key_L = L if with_pos else 1
    want = []
    for w in range(W):
        for p in range(L):
            if not pad[w, p]:
                want.append(min(max(int(ids[w, p]), 0), V - 1) * key_L + (p if with_pos else 0))
    cu = ops.mask_to_cu_seqlens(pad.cuda())
    got = ops.token_keys(ids.cuda(), pad.cuda(), cu, len(want), V, key_L).cpu()
    assert got.tolist() == want


def test_streaming_kernels_reject_bad_arguments(ops):
    """Each of these raises VFError from the entry's own argument check, before any launch; the message names the check."""
    from variantformer_amd import _lib
    VFError = _lib.VFError
    f = lambda *s: torch.zeros(s, device="cuda")
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device="cuda")
    cu = torch.tensor([0, 3], dtype=torch.int32, device="cuda")
    with pytest.raises(VFError, match=r"vf_segment_max: bad arguments \(d=6\)"):
        ops.segment_max(f(3, 6), cu)                                                   # d % 4 != 0
    with pytest.raises(VFError, match=r"vf_affine_rows_f32: bad arguments \(d=6\)"):
        ops.affine_rows(f(3, 6), i64(3))
    with pytest.raises(VFError, match=r"vf_add_rows_f32: bad arguments \(d=6\)"):
        ops.add_rows(f(3, 6), f(3, 6))
    with pytest.raises(VFError, match=r"vf_rowdot_softplus: bad arguments \(d=6\)"):
        ops.rowdot_softplus(f(3, 6), f(6), None)
    with pytest.raises(VFError, match=r"vf_gather_rows_f32: 16-bit outputs need d % 4 == 0 \(d=6\)"):
        ops.gather_rows_f32(f(3, 6), None, i64(3), torch.bfloat16)                     # narrow rows have no 16-bit form
    pad3 = torch.zeros((1, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(VFError, match=r"vf_segment_linear: bad arguments \(L=3 d=6\)"):
        ops.segment_linear(f(3, 6), cu, pad3, f(3), None, torch.float32)               # d % 4 != 0
    big_pad = torch.ones((1, 8193), dtype=torch.uint8, device="cuda")
    with pytest.raises(VFError, match=r"vf_segment_linear: bad arguments \(L=8193 d=4\)"):
        ops.segment_linear(f(1, 4), torch.tensor([0, 0], dtype=torch.int32, device="cuda"), big_pad, f(8193), None,
                           torch.float32)                                             # L > 8192
    ids = torch.zeros((1, 10), dtype=torch.int64, device="cuda")
    pad10 = torch.zeros((1, 10), dtype=torch.uint8, device="cuda")
    with pytest.raises(VFError, match=r"vf_token_keys: bad arguments \(L=10 key_L=5\)"):
        ops.token_keys(ids, pad10, torch.tensor([0, 10], dtype=torch.int32, device="cuda"), 10, 500, 5)   # 1 < key_L < L
    q = torch.zeros((4, 64), dtype=torch.bfloat16, device="cuda")
    out = torch.empty_like(q)
    cu4 = torch.tensor([0, 4], dtype=torch.int32, device="cuda")
    lib = _lib.load()

    def attn(flags):
        return lib.vf_attn_varlen_fwd_v2(q.data_ptr(), q.data_ptr(), q.data_ptr(), out.data_ptr(), 64, 64, 64, 64, cu4.data_ptr(),
                                         cu4.data_ptr(), 1, 4, 4, 1, 64, None, 0.125, _lib.VF_BF16, flags,
                                         torch.cuda.current_stream().cuda_stream)
    for flags in (4, 8 | 1, -1):
        rc = attn(flags)
        with pytest.raises(VFError, match="unknown flag bits"):
            _lib.check(rc, "vf_attn_varlen_fwd_v2")
    for flags in (0, 1, 2, 3):                        # the same arguments with the defined bits only: accepted
        _lib.check(attn(flags), "vf_attn_varlen_fwd_v2")
    torch.cuda.synchronize()

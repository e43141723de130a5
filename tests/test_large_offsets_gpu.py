"""Every kernel's addressing past 2^31 elements and 4 GiB, on a real MI355X.

One operand of a call at a time is made BIG: a view into a 24 GiB arena, placed behind 8 GiB of headroom, whose rows start
beyond element 2^31 / byte 2^32 -- a few hundred rows millions of elements apart where the entry takes a row stride, the
smallest natural shape above 2^31 elements where it takes none (tests/large_offset_cases.py is the table;
tests/test_large_offsets_cpu.py proves from it that an offset narrowed to 32 bits lands elsewhere INSIDE the arena).  The arena
is 0xFF everywhere before a case (NaN in fp32 / bf16 / fp16, -1 in int64).  Each case asserts
  1. bit identity with the same entry on small contiguous operands outside the arena -- the identical call for the huge-stride
     cases, calls on copies of three row slices (first, around element 2^31, last) for the natural ones -- and the same
     vf_last_kernel string for both;
  2. the small call against its high-precision reference (the CPU oracle for attention, float64 torch otherwise) at the
     tolerance of the entry's existing test, named where it is used; the reference of a geometry is computed once;
  3. every element of a big output is finite (it was NaN), and after the written regions are reset the whole arena is 0xFF.
No big tensor is copied to the host.

Left out: part_stats / row_stats of the LayerNorm-folding GEMMs have no stride and hold 2 floats per row and 32-column part
(far below 2^31 elements at any M that fits the card); vf_token_keys / vf_mask_to_cu_seqlens would need 17 GB of ids to cross."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vf_oracle as O
from tests import attn_edge_cases as E
from tests import large_offset_cases as C
from tests.helpers import _rand

pytestmark = pytest.mark.gpu

TDT = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}
IDT = {2: torch.int16, 4: torch.int32}
EPS32 = 2.0 ** -24
LOG2E = math.log2(math.e)
GPU_SEED = 20240
SPECS = C.attn_specs()


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from variantformer_amd import ops as _ops
    from variantformer_amd import _lib
    _lib.load()      # must be the in-tree HIP library; raises if missing
    return _ops


@pytest.fixture(scope="module")
def lib():
    from variantformer_amd import _lib
    return _lib.load()


class Arena:
    def __init__(self):
        self.buf = torch.empty(C.ARENA_BYTES, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % C.ALIGN == 0
        self.placed = []

    def begin(self, case):
        """0xFF everywhere; the case's big operands as integer-typed [rows, cols] views (strided by their ld)."""
        self.buf.fill_(0xFF)
        self.placed = []
        for b, off in zip(case.bigs, C.layout(case.bigs)):
            flat = self.buf[off:off + b.nbytes].view(IDT[b.esize])
            self.placed.append(flat.as_strided((b.rows, b.cols), (b.ld, 1)))
        return list(self.placed)

    def finish(self):
        """Reset the logical region of every big operand, then the whole arena must read 0xFF again (1 GiB at a time)."""
        for bits in self.placed:
            bits.fill_(-1)
        v = self.buf.view(torch.int64)
        step = C.GiB // 8
        for a in range(0, v.numel(), step):
            bad = v[a:a + step] != -1
            if bool(bad.any()):
                raise AssertionError(f"the arena was disturbed at byte {8 * (a + int(bad.nonzero()[0]))}")


@pytest.fixture(scope="module")
def arena():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    free = torch.cuda.mem_get_info()[0]
    need = C.ARENA_BYTES + 8 * C.GiB
    if free < need:
        pytest.skip(f"free device memory {free} B is below the arena of {C.ARENA_BYTES} B plus 8 GiB = {need} B")
    a = Arena()
    print(f"[large_offsets] arena {C.ARENA_BYTES / C.GiB:.0f} GiB, free device memory at start {free / C.GiB:.1f} GiB")
    yield a
    for memo in (_GEMM_SMALL, _LN_PROD_SMALL, _LN_CONS_SMALL, _ATTN_SMALL, _PROBS):      # the small twins: device tensors too
        memo.clear()
    a.placed = []
    del a.buf
    torch.cuda.empty_cache()


def test_arena_check_sees_one_disturbed_byte(arena):
    """The containment check itself: one byte of the headroom, and one between two rows of a huge-stride operand, is noticed."""
    case = C.BY_ID["gemm-bf16-1-bf16-out"]
    for where in (C.HEADROOM - (1 << 31) - 2, C.HEADROOM + 2 * case.bigs[0].cols + 6):
        arena.begin(case)
        arena.buf[where] = 0x7F
        with pytest.raises(AssertionError, match=f"disturbed at byte {where // 8 * 8}"):
            arena.finish()
    arena.begin(case)
    arena.finish()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(IDT[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _finite(t):
    """Every element finite, 2^28 elements at a time (t contiguous of any size, or a small strided view)."""
    if not t.is_contiguous():
        return bool(torch.isfinite(t.float()).all())
    f = t.view(-1)
    return all(bool(torch.isfinite(f[a:a + (1 << 28)]).all()) for a in range(0, f.numel(), 1 << 28))


def _gen():
    return torch.Generator(device="cuda").manual_seed(GPU_SEED)


def _check(rc, lib):
    assert rc == 0, lib.vf_last_error()


# ---------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------
_GEMM_SMALL = {}


def _gemm_small(ops, dtype, path, epi):
    """Operands, the small contiguous call and its float64 check, once per (dtype, path, epilogue)."""
    key = (dtype, path, epi)
    if key in _GEMM_SMALL:
        return _GEMM_SMALL[key]
    M, N, K = C.gemm_shape(path, epi)
    tdt = TDT[dtype]
    code = {"bf16": ops.EPI_BF16, "f32": ops.EPI_F32, "res": ops.EPI_RES_F32, "geglu": ops.EPI_GEGLU_BF16}[epi]
    variant = {"generic": 0, "22-K256": 22}.get(path, path)
    a32 = _rand((M, K), 91).to(tdt).float()
    w32 = _rand((N, K), 92, 1.0 / math.sqrt(K)).to(tdt).float()
    b32, r32 = _rand((N,), 93, 0.5), _rand((M, N), 94)
    a, w, b = a32.cuda().to(tdt), w32.cuda().to(tdt), b32.cuda()
    if epi == "geglu":
        w, b = ops.pack_geglu_rows(w, b)
    res = r32.cuda() if epi == "res" else None
    out = ops.gemm(a, w, b, code, residual=res, variant=variant)
    kernel = ops.last_kernel("gemm")
    torch.cuda.synchronize()
    assert kernel == C.GEMM_KERNEL[path], kernel
    ref = a32.double() @ w32.double().t() + b32.double()
    if epi == "res":
        ref = ref + r32.double()
    if epi == "geglu":
        x, gate = ref.chunk(2, dim=-1)
        ref = x * F.gelu(gate)
    # the tolerances of tests/test_ops_gpu.py::test_gemm_epilogues / test_gemm_geglu
    if out.dtype == torch.float32:
        np.testing.assert_allclose(out.double().cpu().numpy(), ref.numpy(), rtol=2e-5, atol=2e-5 * math.sqrt(K))
    else:
        np.testing.assert_allclose(out.double().cpu().numpy(), ref.numpy(), rtol=2 ** -8, atol=2e-3)
    _GEMM_SMALL[key] = (a, w, b, res, out, kernel, code, variant)
    return _GEMM_SMALL[key]


@pytest.mark.parametrize("cid", C.ids("gemm"))
def test_gemm_huge_stride(ops, arena, cid):
    """vf_gemm_bf16 / _f16 (_ex): A (lda), out (ldo) or the residual (ldr) with rows millions of elements apart, for every tile
    configuration and the generic path."""
    case = C.BY_ID[cid]
    p = case.p
    a, w, b, res, small, kernel, code, variant = _gemm_small(ops, p["dtype"], p["path"], p["epi"])
    (bits,) = arena.begin(case)
    big = bits.view(TDT[p["dtype"]] if case.bigs[0].esize == 2 else torch.float32)
    out = None
    if p["big"] == "A":
        big.copy_(a)
        a = big
    elif p["big"] == "residual":
        big.copy_(res)
        res = big
    else:
        out = big
    got = ops.gemm(a, w, b, code, residual=res, out=out, variant=variant)
    assert ops.last_kernel("gemm") == kernel
    torch.cuda.synchronize()
    assert _same(got, small)
    assert _finite(got)
    arena.finish()


def _ln_scale(ops, tdt):
    return ops.x16_scale_for(tdt)


def _ln_producer_call(ops, lib, form, tdt, a, w, b, res, out, out16, part, t16_out):
    from variantformer_amd import _lib as L
    M, K = a.shape
    N = w.shape[0]
    dt = ops._dt(tdt)
    scale = _ln_scale(ops, tdt)
    if form == "t16":
        _check(lib.vf_gemm_ln_t16(a.data_ptr(), a.stride(0), w.data_ptr(), b.data_ptr(), res.data_ptr(), res.stride(0),
                                  1.0 / ops.T16_SCALE, out.data_ptr(), out.stride(0), M, N, K, dt, out16.data_ptr(), out16.stride(0),
                                  part.data_ptr(), scale, t16_out.data_ptr(), t16_out.stride(0), ops.T16_SCALE, _st()), lib)
        return
    r_dt, r_scale = (L.VF_F32, 1.0) if form == "f32" else (dt, 1.0 / scale)
    _check(lib.vf_gemm_ln(a.data_ptr(), a.stride(0), w.data_ptr(), b.data_ptr(), res.data_ptr(), res.stride(0), r_dt, out.data_ptr(),
                          out.stride(0), M, N, K, ops.EPI_RES_F32, dt, 0, 0, out16.data_ptr(), out16.stride(0), part.data_ptr(), scale,
                          r_scale, _st()), lib)


_LN_PROD_SMALL = {}


def _ln_producer_small(ops, lib, dtype, form):
    key = (dtype, form)
    if key in _LN_PROD_SMALL:
        return _LN_PROD_SMALL[key]
    M, N, K = C.LN_M, C.LN_N, C.LN_K
    tdt = TDT[dtype]
    scale = _ln_scale(ops, tdt)
    a = _rand((M, K), 341).cuda().to(tdt)
    w = _rand((N, K), 342, 1.0 / math.sqrt(K)).cuda().to(tdt)
    b = _rand((N,), 343, 0.5).cuda()
    r32 = (_rand((M, N), 344, 3.0) + 0.7).cuda()
    if form == "f32":
        res, res_val = r32, r32
    elif form == "r16":
        res = (r32 * scale).to(tdt)
        res_val = res.float() / scale
    else:
        res = (r32 * ops.T16_SCALE).half()
        res_val = res.float() / ops.T16_SCALE
    out = torch.empty((M, N), dtype=torch.float32, device="cuda")
    out16 = torch.empty((M, N), dtype=tdt, device="cuda")
    part = torch.empty((N // 32, M, 2), dtype=torch.float32, device="cuda")
    t16 = torch.empty((M, N), dtype=torch.float16, device="cuda")
    _ln_producer_call(ops, lib, form, tdt, a, w, b, res, out, out16, part, t16)
    kernel = ops.last_kernel("gemm")
    stats = torch.empty((M, 2), dtype=torch.float32, device="cuda")
    _check(lib.vf_ln_finalize2(part.data_ptr(), M, N // 32, N, 1e-5, scale, 1e30, 0.0, 0, stats.data_ptr(), _st()), lib)
    torch.cuda.synchronize()
    # tests/test_ops_gpu.py::test_gemm_ln_producer (fp32 rows, statistics) / _with_16bit_residual / _with_fp16_trunk (the copies)
    ref = a.double() @ w.double().t() + b.double() + res_val.double()
    np.testing.assert_allclose(out.double().cpu().numpy(), ref.cpu().numpy(), rtol=2e-5, atol=2e-5 * math.sqrt(K))
    assert torch.equal(out16, (out * scale).to(tdt))
    if form == "t16":
        assert torch.equal(t16, (out * ops.T16_SCALE).half())
    xd = out.double()
    mean, rstd = xd.mean(dim=1), 1.0 / torch.sqrt(xd.var(dim=1, unbiased=False) + 1e-5)
    np.testing.assert_allclose(stats[:, 0].double().cpu().numpy(), (mean * scale).cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(stats[:, 1].double().cpu().numpy(), (rstd / scale).cpu().numpy(), rtol=2e-5)
    _LN_PROD_SMALL[key] = (a, w, b, res, out, out16, part, t16, kernel)
    return _LN_PROD_SMALL[key]


@pytest.mark.parametrize("cid", C.ids("ln_producer"))
def test_gemm_ln_producer_huge_stride(ops, lib, arena, cid):
    """vf_gemm_ln / vf_gemm_ln_t16 as producers, through the C entries (ops.gemm_ln_producer allocates its own outputs): out16
    (ld16), the fp32 rows (ldo), the 16-bit residual copy (ldr, R16), the fp16 trunk residual (ldr) and t16_out (ldt16, T16)."""
    case = C.BY_ID[cid]
    p = case.p
    tdt = TDT[p["dtype"]]
    a, w, b, res, out_s, out16_s, part_s, t16_s, kernel = _ln_producer_small(ops, lib, p["dtype"], p["form"])
    M, N = out_s.shape
    (bits,) = arena.begin(case)
    out = torch.empty_like(out_s)
    out16, part, t16 = torch.empty_like(out16_s), torch.empty_like(part_s), torch.empty_like(t16_s)
    if p["big"] == "out16":
        out16 = bits.view(tdt)
    elif p["big"] == "out":
        out = bits.view(torch.float32)
    elif p["big"] == "t16_out":
        t16 = bits.view(torch.float16)
    else:
        big = bits.view(res.dtype)
        big.copy_(res)
        res = big
    _ln_producer_call(ops, lib, p["form"], tdt, a, w, b, res, out, out16, part, t16)
    assert ops.last_kernel("gemm") == kernel
    torch.cuda.synchronize()
    assert _same(out, out_s) and _same(out16, out16_s) and _same(part, part_s)
    if p["form"] == "t16":
        assert _same(t16, t16_s)
    assert _finite(out) and _finite(out16)
    arena.finish()


def _ln_consumer_call(ops, lib, tdt, a16, stats, w, bias, cs, out, epi):
    from variantformer_amd import _lib as L
    M, K = a16.shape
    _check(lib.vf_gemm_ln(a16.data_ptr(), a16.stride(0), w.data_ptr(), bias.data_ptr(), 0, 0, L.VF_F32, out.data_ptr(), out.stride(0),
                          M, w.shape[0], K, epi, ops._dt(tdt), stats.data_ptr(), cs.data_ptr(), 0, 0, 0, 1.0, 1.0, _st()), lib)


_LN_CONS_SMALL = {}


def _ln_consumer_small(ops, lib, dtype, epi, N):
    key = (dtype, epi)
    if key in _LN_CONS_SMALL:
        return _LN_CONS_SMALL[key]
    from variantformer_amd.seq2gene.modules.layers import packed_linear_ln
    M, K = C.LN_M, C.LN_K
    tdt = TDT[dtype]
    geglu = epi == "geglu"
    if dtype == "bf16":        # the operands of tests/test_ops_gpu.py::test_gemm_ln_consumer_matches_folded_oracle
        x = _rand((M, K), 321, 2.0) + _rand((M, 1), 322, 1.5) + 0.3 * _rand((1, K), 323, 4.0)
        tol = dict(rtol=2 ** -7, atol=4e-3)
    else:                      # ... and of test_gemm_ln_fp16_consumer_matches_folded_oracle_and_unfolded_pair
        x = (_rand((M, K), 351, 2.0) + _rand((M, 1), 352, 1.5)) * (10.0 ** _rand((M, 1), 353, 1.5))
        tol = dict(rtol=2 ** -10, atol=1e-3)
    lin, norm = torch.nn.Linear(K, N), torch.nn.LayerNorm(K)
    with torch.no_grad():
        lin.weight.copy_(_rand((N, K), 324, 1.0 / math.sqrt(K)))
        lin.bias.copy_(_rand((N,), 325, 0.5))
        norm.weight.copy_(1.0 + _rand((K,), 326, 0.3))
        norm.bias.copy_(_rand((K,), 327, 0.2))
    rnd = O.Rounding(dtype, fold_ln=True)
    ref = O.linear(rnd.ln(x, norm.weight.detach(), norm.bias.detach()), lin.weight.detach(), lin.bias.detach(), rnd)
    if geglu:
        ref = ref[:, :N // 2] * F.gelu(ref[:, N // 2:])
    lin, norm = lin.cuda(), norm.cuda()
    with ops.compute_dtype(tdt):
        wp, bp, cs = packed_linear_ln(lin, norm, geglu=geglu)
        s = ops.ln_stream(x.cuda())
    code = ops.EPI_GEGLU_BF16 if geglu else ops.EPI_BF16
    out = torch.empty((M, N // 2 if geglu else N), dtype=tdt, device="cuda")
    _ln_consumer_call(ops, lib, tdt, s.x16, s.stats, wp, bp, cs, out, code)
    kernel = ops.last_kernel("gemm")
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.float().cpu().numpy(), ref.detach().numpy(), **tol)
    _LN_CONS_SMALL[key] = (s.x16, s.stats, wp, bp, cs, out, code, kernel)
    return _LN_CONS_SMALL[key]


@pytest.mark.parametrize("cid", C.ids("ln_consumer"))
def test_gemm_ln_consumer_huge_stride(ops, lib, arena, cid):
    """vf_gemm_ln as the LayerNorm consumer: A = the 16-bit stream copy (lda) and out (ldo), 16-bit and GEGLU epilogues."""
    case = C.BY_ID[cid]
    p = case.p
    tdt = TDT[p["dtype"]]
    a16, stats, wp, bp, cs, small, code, kernel = _ln_consumer_small(ops, lib, p["dtype"], p["epi"], p["N"])
    (bits,) = arena.begin(case)
    big = bits.view(tdt)
    if p["big"] == "A":
        big.copy_(a16)
        a16, out = big, torch.empty_like(small)
    else:
        out = big
    _ln_consumer_call(ops, lib, tdt, a16, stats, wp, bp, cs, out, code)
    assert ops.last_kernel("gemm") == kernel
    torch.cuda.synchronize()
    assert _same(out, small) and _finite(out)
    arena.finish()


@pytest.mark.parametrize("cid", C.ids("gemm_wqkv"))
def test_gemm_wqkv_of_44_genes(ops, arena, cid):
    """The 44-gene Wqkv: out bf16 [477 576, 4608] = 2.2e9 elements in the arena (K = 64: the K loop is not under test).  Rows
    [0, 256), [465 900, 466 156) -- element 2^31 falls in row 466 033 -- and the last 256 hold the bits of calls on copies of
    those rows of A, in the same tile configuration; those calls against float64 (tests/test_ops_gpu.py::test_gemm_epilogues)."""
    case = C.BY_ID[cid]
    M, N, K = C.WQKV_M, C.WQKV_N, C.WQKV_K
    (bits,) = arena.begin(case)
    out = bits.view(torch.bfloat16)
    assert out.is_contiguous() and out.shape == (M, N)
    a = torch.empty((M, K), dtype=torch.bfloat16, device="cuda").uniform_(-1, 1, generator=_gen())
    w = _rand((N, K), 92, 1.0 / math.sqrt(K)).cuda().bfloat16()
    b = _rand((N,), 93, 0.5).cuda()
    ops.gemm(a, w, b, ops.EPI_BF16, out=out, variant=case.p["variant"])
    kernel = ops.last_kernel("gemm")
    twin_variant = C.GEMM_VARIANT[kernel]
    if case.p["variant"]:
        assert twin_variant == case.p["variant"]
    for r0, r1 in C.WQKV_SLICES:
        rows = a[r0:r1].clone()
        small = ops.gemm(rows, w, b, ops.EPI_BF16, variant=twin_variant)
        assert ops.last_kernel("gemm") == kernel
        torch.cuda.synchronize()
        assert _same(out[r0:r1], small), (r0, r1)
        ref = rows.double() @ w.double().t() + b.double()
        np.testing.assert_allclose(small.double().cpu().numpy(), ref.cpu().numpy(), rtol=2 ** -8, atol=2e-3)
    assert _finite(out)
    arena.finish()


def test_gemm_generic_path_grid_limit(ops, lib):
    """gemm_generic_kernel (K % 64 != 0) puts ceil(M / 64) blocks on grid.y.  65 537 row blocks are REFUSED (VF_ERR_INVALID_ARG,
    never a failed or a successful launch): the message names grid.y, the attribute and the device's limit, and the NaN-filled
    output is untouched.  The limit the message reports (65 536 on MI355X; 65 535 at the least) is then taken at its word:
    exactly that many row blocks, the last one ragged, run and are right to the last row, and one row more is refused again."""
    import re
    K = N = 8
    M_over = 64 * 65536 + 64
    a = torch.randint(-4, 5, (M_over, K), generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).cuda()
    w = torch.randint(-3, 4, (N, K), generator=torch.Generator().manual_seed(4)).to(torch.bfloat16).cuda()
    out = torch.full((M_over, N), float("nan"), device="cuda")
    ref = a.double() @ w.double().t()                                   # small integers: exact in fp32

    def call(M, fn=lib.vf_gemm_bf16):
        return fn(a.data_ptr(), K, w.data_ptr(), 0, 0, 0, out.data_ptr(), N, M, N, K, ops.EPI_F32, _st())

    def refused(M, fn=lib.vf_gemm_bf16):
        assert call(M, fn) == 1, lib.vf_last_error()
        msg = lib.vf_last_error().decode()
        torch.cuda.synchronize()
        assert "grid.y" in msg and "hipDeviceAttributeMaxGridDimY" in msg and f"= {(M + 63) // 64} row blocks" in msg, msg
        assert bool(torch.isnan(out).all())                               # nothing was launched
        return int(re.search(r"limit of (\d+)", msg).group(1))
    limit = refused(M_over)
    assert limit in (65535, 65536), limit
    assert refused(M_over, lib.vf_gemm_f16) == limit
    assert refused((1 << 31) - 1) == limit                                # (M + 63 must not wrap on its way to the check)
    M_ok = 64 * limit - 3
    assert call(M_ok) == 0, lib.vf_last_error()
    assert ops.last_kernel("gemm") == "gemm_generic_kernel"
    torch.cuda.synchronize()
    assert torch.equal(out[:M_ok].double(), ref[:M_ok]) and bool(torch.isnan(out[M_ok:]).all())
    out.fill_(float("nan"))
    assert refused(64 * limit + 1) == limit


# ---------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------
def _attn_operands(spec, dtype):
    """(q [tq, D], k, v [tk, D]) fp32 holding values of the operand type: the recipe of tests/attn_edge_cases.py."""
    if spec.edge_case:
        q, k, v = E.operands(spec.edge_case, dtype, spec.q_log2)
        return torch.cat([q] * spec.rep), torch.cat([k] * spec.rep), torch.cat([v] * spec.rep)
    rnd = O.Rounding(dtype)
    D = spec.H * spec.dh
    q = _rand((sum(spec.ql), D), spec.seed, E.INPUT_SCALE)
    kv = rnd.r(_rand((sum(spec.kl), 2 * D), spec.seed + 1, E.INPUT_SCALE))
    q = rnd.r(q * (LOG2E / math.sqrt(spec.dh))) if spec.q_log2 else rnd.r(q)
    return q, kv[:, :D].contiguous(), kv[:, D:].contiguous()


def _slopes(spec):
    return torch.tensor(O.alibi_slopes(spec.H), dtype=torch.float32) if spec.alibi else None


def _oracle_seqs(q, k, v, ql, kl, H, dh, slopes, dtype, q_log2, heads=None):
    """O.attention per sequence (end-aligned ALiBi) -> [tq, len(heads) * dh] fp32, rounded to the output type; zero rows where
    the key sequence is empty.  heads: a subset of the heads (wide geometries)."""
    rnd = O.Rounding(dtype)
    heads = list(range(H)) if heads is None else list(heads)
    cu_q, cu_k = E.cu_of(ql), E.cu_of(kl)
    sl = None if slopes is None else slopes[heads]
    out = torch.zeros(q.shape[0], len(heads) * dh)
    for s in range(len(ql)):
        a, e, ka, ke = int(cu_q[s]), int(cu_q[s + 1]), int(cu_k[s]), int(cu_k[s + 1])
        if e == a or ke == ka:
            continue
        pick = lambda t: t.view(-1, H, dh)[:, heads].contiguous()          # noqa: E731
        o = O.attention(pick(q[a:e]), pick(k[ka:ke]), pick(v[ka:ke]), sl, rnd, q_log2=q_log2)
        out[a:e] = o.reshape(e - a, -1)
    return rnd.r(out)


def _pick_heads(t, H, dh, heads):
    return t.view(t.shape[0], H, dh)[:, list(heads)].reshape(t.shape[0], -1)


_ATTN_SMALL = {}


def _attn_small(ops, spec, dtype, heads=None):
    """The contiguous call of a geometry and its check against the oracle (tests/attn_edge_cases.tolerance, i.e. the attention
    tolerances of tests/test_ops_gpu.py), once per (geometry, operand type)."""
    key = (spec.name, dtype)
    if key in _ATTN_SMALL:
        return _ATTN_SMALL[key]
    tdt = TDT[dtype]
    q, k, v = _attn_operands(spec, dtype)
    slopes = _slopes(spec)
    dq, dk, dv = q.cuda().to(tdt), k.cuda().to(tdt), v.cuda().to(tdt)
    args = (E.cu_of(spec.ql).cuda(), E.cu_of(spec.kl).cuda(), max(spec.ql), max(spec.kl), spec.H, spec.dh,
            None if slopes is None else slopes.cuda())
    out = ops.attn_varlen(dq, dk, dv, *args, q_log2=spec.q_log2)
    kernel = ops.last_kernel("attn")
    torch.cuda.synchronize()
    assert kernel == spec.kernel, kernel
    got = out.float().cpu()
    if spec.edge_case:
        c = E.CASES_BY_NAME[spec.edge_case]
        want = O.Rounding(dtype).r(E.oracle_rows(c, dtype, spec.q_log2, False)).repeat(spec.rep, 1)
    else:
        want = _oracle_seqs(q, k, v, spec.ql, spec.kl, spec.H, spec.dh, slopes, dtype, spec.q_log2, heads)
        if heads is not None:
            got = _pick_heads(got, spec.H, spec.dh, heads)
    np.testing.assert_allclose(got.numpy(), want.numpy(), **E.tolerance(dtype))
    _ATTN_SMALL[key] = (dq, dk, dv, args, out, kernel)
    return _ATTN_SMALL[key]


def _attn_big(ops, arena, case, spec, dtype, which, heads=None):
    dq, dk, dv, args, small, kernel = _attn_small(ops, spec, dtype, heads)
    D = spec.H * spec.dh
    (bits,) = arena.begin(case)
    big = bits.view(TDT[dtype])
    out = None
    if which == "q":
        big.copy_(dq)
        dq = big
    elif which == "kv":
        big[:, :D].copy_(dk)
        big[:, D:].copy_(dv)
        dk, dv = big[:, :D], big[:, D:]
        assert dk.stride(0) == case.bigs[0].ld
    else:
        out = big
    got = ops.attn_varlen(dq, dk, dv, *args, out=out, q_log2=spec.q_log2)
    assert ops.last_kernel("attn") == kernel
    torch.cuda.synchronize()
    assert _same(got, small) and _finite(got)
    arena.finish()


@pytest.mark.parametrize("cid", C.ids("attn"))
def test_attention_huge_stride(ops, arena, cid):
    """vf_attn_varlen_fwd_v2 / _v3, one case per kernel family (the geometries of tests/attn_edge_cases.py, repeated to about 700
    tokens, plus the two attn_x32_kernel forms): q (q_stride), k and v as slices of one [tokens, ld] buffer (k_stride, v_stride),
    out (o_stride)."""
    case = C.BY_ID[cid]
    _attn_big(ops, arena, case, SPECS[case.p["spec"]], case.p["dtype"], case.p["big"])


WIDE_HEADS = {"kv24_fwd128": range(0, 128, 16), "kv24_x32_64": range(0, 256, 32), "longk_fwd128": (0, 13, 22, 31),
              "longk_x32_64": (0, 13, 22, 31)}


@pytest.mark.parametrize("cid", C.ids("attn_kv24"))
def test_attention_key_offset_at_the_24_bit_guard(ops, arena, cid):
    """The tiled kernels address a key as base + umul24(key, stride).  K | V in one buffer with row stride exactly 2^23, two
    sequences of 255 keys (255 * 2^23 < 2^31 is accepted; the second sequence starts at byte 2^32 - 2^24, one row short of 2^32 --
    256 keys would be refused -- so every key of it but the first lies beyond byte 2^32, its last beyond element 2^31): the bits
    of the contiguous call, which is checked against the oracle (8 of the heads where H >= 128)."""
    case = C.BY_ID[cid]
    spec = {s.name: s for s in C.KV24_SPECS}[case.p["spec"]]
    _attn_big(ops, arena, case, spec, "bf16", "kv", WIDE_HEADS.get(spec.name))


@pytest.mark.parametrize("name", [s.name for s in C.LONGK_SPECS])
def test_attention_key_offset_past_2_pow_24(ops, name):
    """key * stride beyond 2^24 at a natural stride: 6000 keys x 4608 elements (2.8e7; a multiply that kept 24 bits of the
    PRODUCT would wrap), 600 queries, ordinary memory, K and V as column slices of one [keys, 4608] buffer; against the oracle
    (4 of the 32 heads where the kernel form needs H 32)."""
    spec = {s.name: s for s in C.LONGK_SPECS}[name]
    heads = WIDE_HEADS.get(name)
    H, dh = spec.H, spec.dh
    D = H * dh
    q, k, v = _attn_operands(spec, "bf16")
    slopes = _slopes(spec)
    buf = torch.zeros((sum(spec.kl), C.LONGK_STRIDE), dtype=torch.bfloat16, device="cuda")
    c0 = C.LONGK_STRIDE - 2 * D                                           # H 32: the K | V thirds of a packed QKV row
    buf[:, c0:c0 + D] = k.cuda().bfloat16()
    buf[:, c0 + D:] = v.cuda().bfloat16()
    dk, dv = buf[:, c0:c0 + D], buf[:, c0 + D:]
    assert dk.stride(0) == C.LONGK_STRIDE and max(spec.kl) * dk.stride(0) > (1 << 24)
    out = ops.attn_varlen(q.cuda().bfloat16(), dk, dv, E.cu_of(spec.ql).cuda(), E.cu_of(spec.kl).cuda(), max(spec.ql), max(spec.kl),
                          H, dh, None if slopes is None else slopes.cuda(), q_log2=spec.q_log2)
    assert ops.last_kernel("attn") == spec.kernel, ops.last_kernel("attn")
    torch.cuda.synchronize()
    got = out.float().cpu()
    assert bool(torch.isfinite(got).all())
    want = _oracle_seqs(q, k, v, spec.ql, spec.kl, H, dh, slopes, "bf16", spec.q_log2, heads)
    if heads is not None:
        got = _pick_heads(got, H, dh, heads)
    np.testing.assert_allclose(got.numpy(), want.numpy(), **E.tolerance("bf16"))


@pytest.mark.parametrize("entry", ["vf_attn_varlen_fwd_v2", "vf_attn_varlen_fwd_v3"])
def test_attention_refuses_key_offsets_beyond_the_guard(lib, entry):
    """max_seqlen_k * stride = 2^31 (256 keys at stride 2^23) and a stride of 2^24 are refused with VF_ERR_INVALID_ARG before
    anything is launched, and vf_last_error() names the limit; the same arguments inside the limits are accepted."""
    from variantformer_amd import _lib as L
    q = torch.zeros((8, 64), dtype=torch.bfloat16, device="cuda")
    out = torch.full((8, 64), 0x7FC1, dtype=torch.int16, device="cuda")
    cu = torch.tensor([0, 4], dtype=torch.int32, device="cuda")
    fn = getattr(lib, entry)

    def call(k_stride, v_stride, max_k):
        return fn(q.data_ptr(), q.data_ptr(), q.data_ptr(), out.data_ptr(), 64, k_stride, v_stride, 64, cu.data_ptr(), cu.data_ptr(),
                  1, 4, max_k, 1, 64, None, 0.125, L.VF_BF16, 0, _st())
    for k_stride, v_stride, max_k in ((1 << 23, 64, 256), (64, 1 << 23, 256), (1 << 24, 64, 4), (64, 1 << 24, 4), (64, 64, 1 << 24)):
        assert call(k_stride, v_stride, max_k) == 1
        msg = lib.vf_last_error().decode()
        # the message states the rule (both bounds) and the three values it was applied to
        assert "below 2^24" in msg and "below 2^31" in msg, msg
        assert f"max_seqlen_k={max_k}, k_stride={k_stride}, v_stride={v_stride}:" in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 0x7FC1).all())                                    # nothing was launched
    assert call(64, 64, 4) == 0, lib.vf_last_error()
    torch.cuda.synchronize()
    assert bool((out[:4] != 0x7FC1).all()) and bool((out[4:] == 0x7FC1).all())


def test_sequence_counts_beyond_the_grid_are_refused(lib):
    """Three entries put the sequences on grid.y / grid.z: n_seq = 65 536 (vf_attn_probs_v2 also max_rows = 64 * 65 535 + 1) is
    refused by name before anything is launched, n_seq = 1 with the same arguments is accepted."""
    from variantformer_amd import _lib as L
    H, dh, Cn = 1, 32, 2
    q = torch.zeros((8, 32), dtype=torch.bfloat16, device="cuda")
    tab = torch.zeros((Cn, 64), dtype=torch.bfloat16, device="cuda")
    cnt = torch.zeros((1, Cn), device="cuda")
    sc = torch.zeros((8, 2), device="cuda")
    cu = torch.tensor([0, 4], dtype=torch.int32, device="cuda")
    out16 = torch.full((8, 32), 0x7FC1, dtype=torch.int16, device="cuda")
    out32 = torch.full((8, 8), -7.0, device="cuda")
    stats = torch.full((8, 2), -7.0, device="cuda")
    calls = {
        "vf_attn_counted_keys": lambda n, rows: lib.vf_attn_counted_keys(
            q.data_ptr(), 32, tab.data_ptr(), 64, cnt.data_ptr(), cu.data_ptr(), n, 4, Cn, H, dh, out16.data_ptr(), 32, L.VF_BF16, _st()),
        "vf_softmax_counted": lambda n, rows: lib.vf_softmax_counted(
            sc.data_ptr(), 2, cnt.data_ptr(), cu.data_ptr(), n, 4, H, 2, Cn, out16.data_ptr(), 32, L.VF_BF16, _st()),
        "vf_attn_probs": lambda n, rows: lib.vf_attn_probs_v2(
            q.data_ptr(), 32, q.data_ptr(), 32, 0, cu.data_ptr(), cu.data_ptr(), n, rows, 4, H, dh, 1.0, L.VF_BF16, 2, 0,
            stats.data_ptr(), out32.data_ptr(), 8, 0, 0, 0, _st()),
    }
    for name, call in calls.items():
        assert call(65536, 4) == 1, name
        msg = lib.vf_last_error().decode()
        assert msg.startswith(name + ":") and "n_seq=65536" in msg and "grid limit" in msg, msg
    assert calls["vf_attn_probs"](1, 64 * 65535 + 1) == 1
    assert "max_rows=4194241" in lib.vf_last_error().decode() and "grid limit" in lib.vf_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out16 == 0x7FC1).all()) and bool((out32 == -7.0).all()) and bool((stats == -7.0).all())     # nothing was launched
    for name, call in calls.items():
        assert call(1, 4) == 0, (name, lib.vf_last_error())
    torch.cuda.synchronize()
    assert bool((out16[:4] != 0x7FC1).any()) and bool((out32[:4, :4] != -7.0).all())


def _rowmap_lens(geom):
    rng = np.random.default_rng(11)                                      # (the lists of tests/test_ops_gpu.py's row-map test)
    if geom == "seq2reg_windows":
        return [int(x) for x in rng.integers(1, 129, 160)] + [128, 1]
    return [201, 201, 130, 37, 201, 1, 220]


@pytest.mark.parametrize("cid", C.ids("attn_rows"))
def test_attention_row_map_over_a_huge_table(ops, arena, cid):
    """vf_attn_varlen_fwd_rows: q / k / v as the thirds of ONE table of 700 rows millions of elements apart, addressed through
    q_rows / kv_rows (a quarter of the table rows, and so of the tokens, beyond element 2^31)."""
    case = C.BY_ID[cid]
    geom = case.p["geom"]
    dh, H, alibi = C.ROWMAP_GEOMS[geom]
    D = H * dh
    lens = _rowmap_lens(geom)
    T, n_tab = sum(lens), C.ROWMAP_TABLE_ROWS
    rnd = O.Rounding("bf16")
    tab = _rand((n_tab, 3 * D), 71, E.INPUT_SCALE)
    tab[:, :D] *= LOG2E / math.sqrt(dh)
    tab = rnd.r(tab)
    rows = torch.from_numpy(np.random.default_rng(12).integers(0, n_tab, T)).long()
    rows[:7] = rows[0]
    rows[-1] = n_tab - 1
    assert int((rows >= 512).sum()) * 5 >= T
    slopes = torch.tensor(O.alibi_slopes(H), dtype=torch.float32) if alibi else None
    cu = E.cu_of(lens).cuda()
    small_tab = tab.cuda().bfloat16()
    drows = rows.cuda()
    dsl = None if slopes is None else slopes.cuda()
    assert ops.attn_rows_supported(dh, alibi, len(lens), H, max(lens), max(lens), True)

    def run(t):
        o = ops.attn_varlen(t[:, :D], t[:, D:2 * D], t[:, 2 * D:], cu, None, max(lens), max(lens), H, dh, dsl, q_log2=True, rows=drows)
        return o, ops.last_kernel("attn")
    small, kernel = run(small_tab)
    (bits,) = arena.begin(case)
    big = bits.view(torch.bfloat16)
    big.copy_(small_tab)
    got, kernel_big = run(big)
    torch.cuda.synchronize()
    assert kernel == kernel_big and kernel.endswith(",rows>"), (kernel, kernel_big)
    assert _same(got, small) and _finite(got)
    g = tab[rows]
    want = _oracle_seqs(g[:, :D].contiguous(), g[:, D:2 * D].contiguous(), g[:, 2 * D:].contiguous(), lens, lens, H, dh, slopes,
                        "bf16", True)
    np.testing.assert_allclose(small.float().cpu().numpy(), want.numpy(), **E.tolerance("bf16"))
    arena.finish()


@pytest.mark.parametrize("cid", C.ids("counted_keys"))
def test_attention_counted_keys_huge_stride(ops, lib, arena, cid):
    """vf_attn_counted_keys: q (q_stride) and out (o_stride); the geometry, operands, reference and tolerance of
    tests/test_ops_gpu.py::test_attention_counted_keys_matches_oracle_and_the_expanded_form."""
    from variantformer_amd import _lib as L
    case = C.BY_ID[cid]
    dh, H, Cn, lens = (C.COUNTED[k] for k in ("dh", "H", "C", "lens"))
    D = H * dh
    rnd = O.Rounding("bf16")
    rng = np.random.default_rng(3)
    tq = sum(lens)
    cu = E.cu_of(lens)
    labels = torch.from_numpy(rng.integers(0, Cn, tq)).long()
    labels[cu[3]:cu[4]] = 4
    q = rnd.r(_rand((tq, D), 81, 1.2))
    tab = rnd.r(_rand((Cn, 2 * D), 82, 1.5))
    cnt = torch.stack([torch.bincount(labels[cu[b]:cu[b + 1]], minlength=Cn).float() for b in range(len(lens))])
    dq, dtab, dcnt, dcu = q.cuda().bfloat16(), tab.cuda().bfloat16(), torch.log2(cnt).cuda().contiguous(), cu.cuda()

    def run(q_, out_):
        _check(lib.vf_attn_counted_keys(q_.data_ptr(), q_.stride(0), dtab.data_ptr(), dtab.stride(0), dcnt.data_ptr(), dcu.data_ptr(),
                                        len(lens), max(lens), Cn, H, dh, out_.data_ptr(), out_.stride(0), L.VF_BF16, _st()), lib)
        return ops.last_kernel("attn")
    small = torch.empty((tq, D), dtype=torch.bfloat16, device="cuda")
    kernel = run(dq, small)
    (bits,) = arena.begin(case)
    big = bits.view(torch.bfloat16)
    if case.p["big"] == "q":
        big.copy_(dq)
        got = torch.empty_like(small)
        assert run(big, got) == kernel
    else:
        got = big
        assert run(dq, big) == kernel
    torch.cuda.synchronize()
    assert kernel == "attn_counted_keys_kernel" and _same(got, small) and _finite(got)
    ref = torch.zeros(tq, D)
    for b in range(len(lens)):
        a, e = int(cu[b]), int(cu[b + 1])
        if e > a:
            present = [c for c in range(Cn) if cnt[b, c] > 0]
            ref[a:e] = O.attention_counted(q[a:e].view(-1, H, dh), tab[present, :D].view(-1, H, dh), tab[present, D:].view(-1, H, dh),
                                           cnt[b, present], True).reshape(e - a, D)
    ulp = 2 ** -7
    np.testing.assert_allclose(small.float().cpu().numpy(), rnd.r(ref).numpy(), rtol=ulp, atol=ulp * 1e-2)
    arena.finish()


@pytest.mark.parametrize("cid", C.ids("softmax_counted"))
def test_softmax_counted_huge_stride(ops, lib, arena, cid):
    """vf_softmax_counted: scores (lds) and out (ldo); geometry, reference and tolerance of
    tests/test_ops_gpu.py::test_lowrank_context_attention_pieces."""
    from variantformer_amd import _lib as L
    case = C.BY_ID[cid]
    H, Cp, Cn, lens = (C.SOFTMAX_COUNTED[k] for k in ("H", "Cp", "C", "lens"))
    T = sum(lens)
    cu = E.cu_of(lens)
    sc = _rand((T, H * Cp), 96, 4.0)
    cnt = torch.from_numpy(np.random.default_rng(2).integers(0, 50, (len(lens), Cn))).float()
    cnt[1] = 0
    cnt[1, 4] = 1
    cnt[3, 0] = 0
    dsc, dcnt, dcu = sc.cuda(), torch.log2(cnt).cuda().contiguous(), cu.cuda()

    def run(sc_, out_):
        _check(lib.vf_softmax_counted(sc_.data_ptr(), sc_.stride(0), dcnt.data_ptr(), dcu.data_ptr(), len(lens), max(lens), H, Cp, Cn,
                                      out_.data_ptr(), out_.stride(0), L.VF_BF16, _st()), lib)
    small = torch.empty((T, H * Cp), dtype=torch.bfloat16, device="cuda")
    run(dsc, small)
    (bits,) = arena.begin(case)
    if case.p["big"] == "scores":
        big = bits.view(torch.float32)
        big.copy_(dsc)
        got = torch.empty_like(small)
        run(big, got)
    else:
        got = bits.view(torch.bfloat16)
        run(dsc, got)
    torch.cuda.synchronize()
    assert _same(got, small) and _finite(got)
    ref = torch.zeros(T, H, Cp)
    for bb in range(len(lens)):
        a, e = int(cu[bb]), int(cu[bb + 1])
        if e > a:
            t = sc[a:e].view(-1, H, Cp)[:, :, :Cn] + torch.log2(cnt[bb])[None, None, :]
            pr = torch.exp2(t - t.max(dim=-1, keepdim=True).values)
            ref[a:e, :, :Cn] = pr / pr.sum(dim=-1, keepdim=True)
    np.testing.assert_allclose(small.float().cpu().numpy(), O.Rounding("bf16").r(ref.view(T, -1)).numpy(), rtol=2 ** -7, atol=1e-7)
    arena.finish()


_PROBS = {}


def _probs_setup(ops, alibi, per_head):
    """The case, the small call (q and k contiguous, k read through k_rows from a permuted table) and its float64 check."""
    key = (alibi, per_head)
    if key in _PROBS:
        return _PROBS[key]
    from tests.attn_probs_alibi_cases import P_TOL as TOL_ALIBI
    from tests.attn_probs_alibi_cases import P_TOL_PLAIN as TOL_PLAIN
    from tests.attn_probs_alibi_cases import SENTINEL, AlibiCase, plain_reference, prob_err
    case = AlibiCase(C.PROBS_H, C.PROBS_DH, "bf16", True, seqs=list(C.PROBS_SEQS))
    assert case.R == C.PROBS_R and sum(case.kl) == C.PROBS_TK and case.Tq == C.PROBS_R + 7
    H, D, max_k = case.H, case.D, max(case.kl)
    q16, qsel = case.queries(True)
    perm = torch.randperm(C.PROBS_TK, generator=torch.Generator().manual_seed(5))
    table = torch.empty((C.PROBS_TK, D), dtype=case.k16.dtype)
    table[perm] = case.k16[:, :D]                                         # key t is row perm[t] of the table
    dev = dict(q=q16[:, :D].contiguous().cuda(), k=case.k16[:, :D].contiguous().cuda(), table=table.cuda(), k_rows=perm.cuda(),
               cu_rows=case.cu_rows.cuda(), cu_k=case.cu_k.cuda(), q_rows=case.q_rows.cuda(),
               slopes=case.slopes.cuda() if alibi else None, q_pos=case.q_pos.cuda() if alibi else None)
    n_out = case.R * (H if per_head else 1)

    def run(q, k, out, k_rows=None):
        got, stats = ops.attn_probs(q, k, dev["cu_rows"], dev["cu_k"], max(case.rl), max_k, H, case.dh, q_rows=dev["q_rows"],
                                    q_log2=True, per_head=bool(per_head), scale=case.scale, out=out, slopes=dev["slopes"],
                                    q_pos=dev["q_pos"], k_rows=k_rows)
        return got, stats, ops.last_kernel("attn")
    small = torch.full((n_out, max_k + 5), SENTINEL, dtype=torch.float32, device="cuda")
    _, stats, kernel = run(dev["q"], dev["k"], small)
    mapped = torch.full((n_out, max_k + 5), SENTINEL, dtype=torch.float32, device="cuda")
    _, stats_m, kernel_m = run(dev["q"], dev["table"], mapped, dev["k_rows"])
    torch.cuda.synchronize()
    assert kernel == kernel_m == ("attn_probs_alibi_kernel" if alibi else "attn_probs_kernel")
    assert torch.equal(small, mapped) and torch.equal(stats, stats_m) and bool((small[:, max_k:] == SENTINEL).all())
    P64, _ = case.reference(qsel) if alibi else plain_reference(case, qsel)
    body = small[:, :max_k].cpu()
    got = body.view(case.R, H, max_k) if per_head else body
    err = prob_err(got, P64 if per_head else P64.mean(dim=1))
    # the limits of tests/test_attn_probs_alibi_gpu.py / tests/test_attn_probs_gpu.py: max |P - P64| / rowmax(P64) <= P_TOL
    tol = TOL_ALIBI if alibi else TOL_PLAIN
    assert err <= tol, f"max |P - P64| / rowmax = {err:.3e} > {tol:.1e}"
    _PROBS[key] = (case, dev, run, small, stats, kernel)
    return _PROBS[key]


@pytest.mark.parametrize("cid", C.ids("attn_probs"))
def test_attention_probs_huge_stride(ops, arena, cid):
    """vf_attn_probs_v2, with and without ALiBi, head mean and per head: q (q_stride), k as a table read through k_rows
    (k_stride), out with ldo millions of elements (720 per-head rows / 180 head-mean rows); the columns >= max_seqlen_k of
    out keep 0xFF (the arena check after resetting columns < max_seqlen_k only)."""
    case_t = C.BY_ID[cid]
    p = case_t.p
    case, dev, run, small, stats_s, kernel = _probs_setup(ops, p["alibi"], p["per_head"])
    max_k = max(case.kl)
    (bits,) = arena.begin(case_t)
    q, k, k_rows = dev["q"], dev["k"], None
    out = torch.full_like(small, -7.0)
    if p["big"] == "q":
        q = bits.view(torch.bfloat16)
        q.copy_(dev["q"])
    elif p["big"] == "k":
        k, k_rows = bits.view(torch.bfloat16), dev["k_rows"]
        k.copy_(dev["table"])
    else:
        out = bits.view(torch.float32)
        assert out.shape == (small.shape[0], max_k) and out.stride(0) == case_t.bigs[0].ld
    got, stats, kernel_big = run(q, k, out, k_rows)
    torch.cuda.synchronize()
    assert kernel_big == kernel
    assert _same(got[:, :max_k], small[:, :max_k]) and torch.equal(stats, stats_s)
    assert _finite(got[:, :max_k])
    arena.finish()


def test_gene_stream_self_attention_of_44_genes(ops, arena):
    """2376 sequences of 201 tokens, H 32, dh 48, ALiBi, q_log2, packed QKV bf16 [477 576, 4608] = 2.2e9 elements in the arena
    (attn_short2_kernel<2 passes>).  The first 54 sequences, the 54 around token 466 033 (element 2^31) and the last 54 hold
    the bits of calls on copies of those rows; four sequences against the oracle."""
    case = C.BY_ID["attn_gene_self_44"]
    H, dh, L, n_seq = C.GENE_H, C.GENE_DH, C.GENE_LEN, C.GENE_SEQS
    D = H * dh
    (bits,) = arena.begin(case)
    qkv = bits.view(torch.bfloat16)
    assert qkv.is_contiguous() and qkv.shape == (n_seq * L, 3 * D)
    qkv.uniform_(-E.INPUT_SCALE, E.INPUT_SCALE, generator=_gen())
    qkv[:, :D].mul_(LOG2E / math.sqrt(dh))
    slopes = torch.tensor(O.alibi_slopes(H), dtype=torch.float32)
    dsl = slopes.cuda()

    def run(t, n):
        cu = (torch.arange(n + 1, dtype=torch.int32) * L).cuda()
        o = ops.attn_varlen(t[:, :D], t[:, D:2 * D], t[:, 2 * D:], cu, cu, L, L, H, dh, dsl, q_log2=True)
        return o, ops.last_kernel("attn")
    out, kernel = run(qkv, n_seq)
    assert kernel == E.SHORT2_2, kernel
    slices = C.gene_seq_slices()
    for sa, se in slices:
        small, k2 = run(qkv[sa * L:se * L].clone(), se - sa)
        torch.cuda.synchronize()
        assert k2 == kernel and _same(out[sa * L:se * L], small), (sa, se)
    mid = C.straddle_row(3 * D) // L
    for s in (0, mid, mid + 1, n_seq - 1):
        rows = qkv[s * L:(s + 1) * L].float().cpu()
        want = _oracle_seqs(rows[:, :D].contiguous(), rows[:, D:2 * D].contiguous(), rows[:, 2 * D:].contiguous(), [L], [L], H, dh,
                            slopes, "bf16", True)
        np.testing.assert_allclose(out[s * L:(s + 1) * L].float().cpu().numpy(), want.numpy(), **E.tolerance("bf16"))
    assert _finite(out)
    arena.finish()


# ---------------------------------------------------------------------------------------------
# streaming kernels
# ---------------------------------------------------------------------------------------------
def _stats64(x):
    xd = x.double()
    return xd.mean(dim=1), 1.0 / torch.sqrt(xd.var(dim=1, unbiased=False) + 1e-5)


def test_layernorm_natural(ops, lib, arena):
    """vf_layernorm: x fp32 [524 288 + 37, 4096] (element 2^31 = row 524 288, byte 2^32 = row 262 144) and its bf16 output, both
    in the arena.  Row slices against calls on copies; those against float64 at tests/test_ops_gpu.py::test_layernorm's
    tolerance (fp32 output 1e-5; the bf16 output is its RNE)."""
    from variantformer_amd import _lib as L
    case = C.BY_ID["layernorm"]
    rows, D = C.LN_ROWS, C.LN_D
    xb, ob = arena.begin(case)
    x, out = xb.view(torch.float32), ob.view(torch.bfloat16)
    x.uniform_(-2.5, 3.5, generator=_gen())
    g, b = (1 + 0.1 * _rand((D,), 42)).cuda(), (0.1 * _rand((D,), 43)).cuda()
    _check(lib.vf_layernorm(x.data_ptr(), g.data_ptr(), b.data_ptr(), out.data_ptr(), rows, D, 1e-5, L.VF_BF16, 0, _st()), lib)
    for a, e in C.row_slices(rows, D, extra=[C.T32 // 4 // D]):
        xs = x[a:e].clone()
        o16, o32 = ops.layernorm(xs, g, b, torch.bfloat16), ops.layernorm(xs, g, b, torch.float32)
        torch.cuda.synchronize()
        assert _same(out[a:e], o16), (a, e)
        ref = F.layer_norm(xs.double(), (D,), g.double(), b.double(), 1e-5)
        np.testing.assert_allclose(o32.double().cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-5)
        assert torch.equal(o16, o32.bfloat16())
    assert _finite(out)
    arena.finish()


def test_row_stats_cast2_natural(ops, lib, arena):
    """vf_row_stats_cast2 on the same rows: the scaled fp16 copy (in the arena) is fp16(x * 2^-4) exactly, the statistics
    against float64 (tests/test_ops_gpu.py::test_ln_stream_stats_and_copy)."""
    from variantformer_amd import _lib as L
    case = C.BY_ID["row_stats_cast2"]
    rows, D, scale = C.LN_ROWS, C.LN_D, 2.0 ** -4
    xb, ob = arena.begin(case)
    x, out16 = xb.view(torch.float32), ob.view(torch.float16)
    x.uniform_(-2.5, 3.5, generator=_gen())
    stats = torch.empty((rows, 2), dtype=torch.float32, device="cuda")

    def run(x_, o_, s_, n):
        _check(lib.vf_row_stats_cast2(x_.data_ptr(), n, D, 1e-5, o_.data_ptr(), L.VF_F16, scale, 1e30, 0.0, 0, s_.data_ptr(), _st()), lib)
    run(x, out16, stats, rows)
    for a, e in C.row_slices(rows, D, extra=[C.T32 // 4 // D]):
        xs = x[a:e].clone()
        o_s = torch.empty((e - a, D), dtype=torch.float16, device="cuda")
        s_s = torch.empty((e - a, 2), dtype=torch.float32, device="cuda")
        run(xs, o_s, s_s, e - a)
        torch.cuda.synchronize()
        assert _same(out16[a:e], o_s) and _same(stats[a:e], s_s), (a, e)
        assert torch.equal(o_s, (xs * scale).half())
        mean, rstd = _stats64(xs)
        np.testing.assert_allclose(s_s[:, 0].double().cpu().numpy(), (mean * scale).cpu().numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(s_s[:, 1].double().cpu().numpy(), (rstd / scale).cpu().numpy(), rtol=1e-5)
    assert _finite(out16) and _finite(stats)
    arena.finish()


def _embed_inputs():
    W, Lw, d, V = C.EMB_W, C.EMB_L, C.EMB_D, C.EMB_V
    ids = torch.randint(0, V, (W, Lw), generator=torch.Generator().manual_seed(7)).cuda()
    pad = torch.zeros((W, Lw), dtype=torch.uint8, device="cuda")
    table, pos = _rand((V, d), 8, 2.0).cuda(), _rand((Lw, d), 9).cuda()
    return ids, pad, table, pos


def _cu_windows(n, Lw):
    return (torch.arange(n + 1, dtype=torch.int32) * Lw).cuda()


def _window_slices():
    mid = C.straddle_row(C.EMB_D) // C.EMB_L                              # the window that holds element 2^31 (its first token)
    return [(0, 2), (mid - 1, mid + 1), (C.EMB_W - 2, C.EMB_W)]


def test_embed_pack_natural(ops, lib, arena):
    """vf_embed_pack: 8200 windows of 128 valid tokens, d 2048 -- out fp32 [1 049 600, 2048] in the arena.  Windows at both ends
    and either side of element 2^31: table[id] + pos exactly (one fp32 add, tests/test_ops_gpu.py::
    test_embed_pack_and_cu_seqlens_bit_exact) and the bits of a call on those windows alone."""
    case = C.BY_ID["embed_pack"]
    W, Lw, d, V = C.EMB_W, C.EMB_L, C.EMB_D, C.EMB_V
    ids, pad, table, pos = _embed_inputs()
    (bits,) = arena.begin(case)
    out = bits.view(torch.float32)
    _check(lib.vf_embed_pack(ids.data_ptr(), pad.data_ptr(), _cu_windows(W, Lw).data_ptr(), table.data_ptr(), pos.data_ptr(),
                             out.data_ptr(), W, Lw, d, V, _st()), lib)
    for w0, w1 in _window_slices():
        small = ops.embed_pack(ids[w0:w1].contiguous(), pad[w0:w1].contiguous(), _cu_windows(w1 - w0, Lw), table, pos, (w1 - w0) * Lw)
        torch.cuda.synchronize()
        assert _same(out[w0 * Lw:w1 * Lw], small), (w0, w1)
        assert torch.equal(small, (table[ids[w0:w1]] + pos[None]).reshape(-1, d))
    assert _finite(out)
    arena.finish()


def test_embed_stream_natural(ops, lib, arena):
    """vf_embed_stream with out = NULL on the same windows: the bf16 operand copy and the fp16 trunk copy (2.1e9 elements each,
    in the arena) and the row statistics against a call on the slice windows, which must be the three-kernel form's bits
    (tests/test_ops_gpu.py::test_embed_stream_equals_embed_pack_then_stream_passes)."""
    from variantformer_amd import _lib as L
    case = C.BY_ID["embed_stream"]
    W, Lw, d, V = C.EMB_W, C.EMB_L, C.EMB_D, C.EMB_V
    ids, pad, table, pos = _embed_inputs()
    ob, tb = arena.begin(case)
    out16, t16 = ob.view(torch.bfloat16), tb.view(torch.float16)
    stats = torch.empty((W * Lw, 2), dtype=torch.float32, device="cuda")
    alert = torch.zeros(1, dtype=torch.int32, device="cuda")
    _check(lib.vf_embed_stream(ids.data_ptr(), pad.data_ptr(), _cu_windows(W, Lw).data_ptr(), table.data_ptr(), pos.data_ptr(), 0,
                               out16.data_ptr(), L.VF_BF16, 1.0, t16.data_ptr(), ops.T16_SCALE, stats.data_ptr(), 1e-5,
                               ops.LN_FOLD_RATIO_LIMIT, 0.0, alert.data_ptr(), W, Lw, d, V, _st()), lib)
    for w0, w1 in _window_slices():
        n = (w1 - w0) * Lw
        i_s, p_s, cu_s = ids[w0:w1].contiguous(), pad[w0:w1].contiguous(), _cu_windows(w1 - w0, Lw)
        got = ops.embed_stream(i_s, p_s, cu_s, table, pos, n, need_x=False, need_t16=True)
        x = ops.embed_pack(i_s, p_s, cu_s, table, pos, n)
        want, t_want = ops.ln_stream(x), ops.trunk16_of(x)
        torch.cuda.synchronize()
        a, e = w0 * Lw, w1 * Lw
        assert _same(out16[a:e], got.x16) and _same(t16[a:e], got.t16) and _same(stats[a:e], got.stats), (w0, w1)
        assert torch.equal(got.x16, want.x16) and torch.equal(got.stats, want.stats) and torch.equal(got.t16, t_want)
    assert _finite(out16) and _finite(t16) and _finite(stats)
    arena.finish()


def _big_x(arena, case):
    (bits,) = arena.begin(case)
    x = bits.view(torch.float32)
    x.uniform_(-2.0, 2.0, generator=_gen())
    return x


@pytest.mark.parametrize("cid", C.ids("segment"))
def test_segment_pools_natural(ops, arena, cid):
    """vf_segment_mean / _max / _linear over x fp32 [1 049 600, 2048] in the arena, 8200 windows of 128 rows: the windows at both
    ends and either side of element 2^31 hold the bits of calls on copies of their rows; those against float64 at the
    tolerances of test_segment_mean (tests/test_ops_gpu.py), test_segment_max and test_segment_linear
    (tests/test_ops_edges_gpu.py)."""
    case = C.BY_ID[cid]
    op = case.p["op"]
    W, Lw, d = C.EMB_W, C.SEG_WIN, C.SEG_D
    x = _big_x(arena, case)
    pad = torch.zeros((W, Lw), dtype=torch.uint8, device="cuda")
    lin_w, lin_b = _rand((Lw,), 122).cuda(), torch.tensor([0.37], device="cuda")

    def run(x_, n):
        cu = _cu_windows(n, Lw)
        if op == "mean":
            return ops.segment_mean(x_, cu, torch.float32)
        if op == "max":
            return ops.segment_max(x_, cu)
        return ops.segment_linear(x_, cu, pad[:n], lin_w, lin_b, torch.float32)
    out = run(x, W)
    for w0, w1 in _window_slices():
        xs = x[w0 * Lw:w1 * Lw].clone()
        small = run(xs, w1 - w0)
        torch.cuda.synchronize()
        assert _same(out[w0:w1], small), (w0, w1)
        xw = xs.view(w1 - w0, Lw, d).double()
        if op == "mean":
            np.testing.assert_allclose(small.double().cpu().numpy(), xw.mean(dim=1).cpu().numpy(), rtol=1e-5, atol=1e-6)
        elif op == "max":
            assert torch.equal(small, xs.view(w1 - w0, Lw, d).max(dim=1).values)
        else:
            want = torch.einsum("wld,l->wd", xw, lin_w.double()) + 0.37
            bound = Lw * EPS32 * (torch.einsum("wld,l->wd", xw.abs(), lin_w.double().abs()) + 0.37)
            assert bool(((small.double() - want).abs() <= 1e-6 * want.abs() + bound).all())
    assert _finite(out)
    arena.finish()


def test_rowdot_softplus_natural(ops, arena):
    """vf_rowdot_softplus over the same x: row slices against calls on copies, those against float64
    (tests/test_ops_gpu.py::test_rowdot_softplus: 1e-5)."""
    case = C.BY_ID["rowdot_softplus"]
    n, d = C.SEG_ROWS, C.SEG_D
    x = _big_x(arena, case)
    w, b = _rand((d,), 72, 0.05).cuda(), torch.tensor([0.3], device="cuda")
    out = ops.rowdot_softplus(x, w, b)
    for a, e in C.row_slices(n, d, extra=[C.T32 // 4 // d]):
        xs = x[a:e].clone()
        small = ops.rowdot_softplus(xs, w, b)
        torch.cuda.synchronize()
        assert _same(out[a:e], small), (a, e)
        ref = F.softplus(xs.double() @ w.double()[:, None] + 0.3)
        np.testing.assert_allclose(small.double().cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert _finite(out)
    arena.finish()


@pytest.mark.parametrize("cid", C.ids("cast"))
def test_cast_natural(ops, lib, arena, cid):
    """vf_cast_f32_bf16 / _f16 over n = 2^31 + 4100 elements, source and destination in the arena: EVERY element equals
    tensor.to() (round to nearest even, tests/test_ops_gpu.py), compared 2^28 elements at a time on the device; three slices
    also against calls of their own."""
    case = C.BY_ID[cid]
    tdt = TDT[case.p["dtype"]]
    n = C.CAST_N
    xb, ob = arena.begin(case)
    x, out = xb.view(torch.float32).view(-1), ob.view(tdt).view(-1)
    assert x.numel() == n == out.numel()
    x.uniform_(-4.0, 4.0, generator=_gen())
    fn = lib.vf_cast_f32_f16 if tdt == torch.float16 else lib.vf_cast_f32_bf16
    _check(fn(x.data_ptr(), out.data_ptr(), n, _st()), lib)
    torch.cuda.synchronize()
    for a in range(0, n, 1 << 28):
        assert torch.equal(out[a:a + (1 << 28)], x[a:a + (1 << 28)].to(tdt)), a
    for a, e in ((0, 4096), (C.T31 - 2048, C.T31 + 2048), (n - 4100, n)):
        assert _same(ops.cast16(x[a:e].clone(), tdt), out[a:e])
    arena.finish()


def _source_rows():
    """Rows of the big [1 049 600, 2048] source that hold data: both ends, either side of byte 2^32 (row 524 288) and of element
    2^31 (row 1 048 576), and seeded draws of which half lie beyond element 2^31."""
    rng = np.random.default_rng(31)
    edge = [0, 1, 524287, 524288, 1048575, 1048576, 1048577, C.ROWS_N - 1]
    draws = list(rng.integers(2, 1048575, 28)) + list(rng.integers(1048578, C.ROWS_N - 1, 28))
    return torch.tensor(sorted(set(int(r) for r in edge + draws)), dtype=torch.int64)


@pytest.mark.parametrize("cid", C.ids("rows_source"))
def test_row_kernels_read_a_big_source(ops, arena, cid):
    """vf_gather_rows_f32 / vf_add_rows_f32 / vf_affine_rows_f32 with indices that point beyond element 2^31 (and byte 2^32) of
    a big fp32 source of which only the indexed rows hold data (every other row reads as NaN): exact, as their tests in
    tests/test_ops_gpu.py and tests/test_ops_edges_gpu.py hold them, and the bits of the call on a compact copy."""
    case = C.BY_ID[cid]
    op, d = case.p["op"], C.ROWS_D
    (bits,) = arena.begin(case)
    src = bits.view(torch.float32)
    held = _source_rows()
    data = _rand((held.numel(), d), 171, 2.0).cuda()
    for i, r in enumerate(held.tolist()):
        src[r].copy_(data[i])
    pick = torch.randint(0, held.numel(), (300,), generator=torch.Generator().manual_seed(32))
    pick[:held.numel()] = torch.arange(held.numel())                      # every held row at least once
    idx, idx_small = held[pick].cuda(), pick.cuda()
    assert int((held[pick] * d >= C.T31).sum()) >= 75
    other = _rand((300, d), 172, 2.0).cuda()
    scale = _rand((300,), 173, 3.0).cuda()

    def run(s, i):
        if op == "gather":
            return ops.gather_rows_f32(s, None, i)
        if op == "add":
            return ops.add_rows(s, other, idx_a=i)
        return ops.affine_rows(s, i, scale=scale)
    got, small = run(src, idx), run(data, idx_small)
    torch.cuda.synchronize()
    assert _same(got, small) and _finite(got)
    g = data[idx_small]
    want = g if op == "gather" else (g + other if op == "add" else g * scale[:, None])
    assert torch.equal(small, want)
    arena.finish()


@pytest.mark.parametrize("cid", C.ids("rows_out"))
def test_row_kernels_write_a_big_output(ops, lib, arena, cid):
    """The same three entries writing n x d > 2^31 elements (out in the arena) from small sources with repeating indices: row
    slices exact against torch and equal to calls on those indices alone; every element finite."""
    case = C.BY_ID[cid]
    op, n, d = case.p["op"], C.ROWS_N, C.ROWS_D
    odt = TDT[case.p["out"]]
    (bits,) = arena.begin(case)
    out = bits.view(odt)
    a, b = _rand((23, d), 141, 2.0).cuda(), _rand((7, d), 142, 2.0).cuda()
    ar = torch.arange(n, dtype=torch.int64, device="cuda")
    ia, ib = (ar % 23).contiguous(), (ar % 7).contiguous()
    scale = ((ar % 13).float() - 6.5).contiguous()

    def run(o, i0, i1, m):
        if op == "gather":
            rc = lib.vf_gather_rows_f32(a.data_ptr(), 0, i0.data_ptr(), o.data_ptr(), m, d, ops._dt(odt), _st())
        elif op == "add":
            rc = lib.vf_add_rows_f32(a.data_ptr(), i0.data_ptr(), b.data_ptr(), i1.data_ptr(), o.data_ptr(), m, d, _st())
        else:
            rc = lib.vf_affine_rows_f32(a.data_ptr(), i0.data_ptr(), i1.data_ptr(), 0, o.data_ptr(), m, d, _st())
        _check(rc, lib)
    second = scale if op == "affine" else ib
    run(out, ia, second, n)
    extra = [C.T32 // 4 // d] if odt == torch.float32 else []
    for r0, r1 in C.row_slices(n, d, extra=extra):
        small = torch.empty((r1 - r0, d), dtype=odt, device="cuda")
        run(small, ia[r0:r1].contiguous(), second[r0:r1].contiguous(), r1 - r0)
        torch.cuda.synchronize()
        assert _same(out[r0:r1], small), (r0, r1)
        g = a[ia[r0:r1]]
        want = g.to(odt) if op == "gather" else (g + b[ib[r0:r1]] if op == "add" else g * scale[r0:r1, None])
        assert torch.equal(small, want)
    assert _finite(out)
    arena.finish()


@pytest.mark.parametrize("cid", C.ids("segment_mean16"))
def test_segment_mean16_huge_stride(ops, arena, cid):
    """vf_segment_mean16 over a 16-bit stream whose rows are ldx = 2^22 + 64 elements apart: the bits of the contiguous call,
    which is held to tests/test_ops_gpu.py::test_segment_mean16_vs_float64's bounds."""
    case = C.BY_ID[cid]
    tdt = TDT[case.p["dtype"]]
    lens, d, scale = list(C.MEAN16_LENS), C.MEAN16_D, 16.0
    cu = E.cu_of(lens).cuda()
    xs = _rand((sum(lens), d), 81, 3.0).cuda().to(tdt)
    (bits,) = arena.begin(case)
    big = bits.view(tdt)
    big.copy_(xs)
    f, sp = ops.segment_mean16(big, cu, in_scale=scale), ops.segment_mean16(big, cu, in_scale=scale, split=True)
    f_s, sp_s = ops.segment_mean16(xs, cu, in_scale=scale), ops.segment_mean16(xs, cu, in_scale=scale, split=True)
    torch.cuda.synchronize()
    assert _same(f, f_s) and _same(sp, sp_s)
    xd = xs.double().cpu()
    for w, ln in enumerate(lens):
        a = int(cu[w])
        if ln == 0:
            assert torch.isnan(f_s[w]).all() and torch.isnan(sp_s[w].float()).all()
            continue
        ref = xd[a:a + ln].mean(dim=0) * scale
        tol = float(ref.abs().max())
        assert float((f_s[w].double().cpu() - ref).abs().max()) <= 2e-6 * tol + 1e-30
        rec = sp_s[w, :d].double().cpu() + sp_s[w, d:].double().cpu()
        assert float((rec - ref).abs().max()) <= 2 ** -15 * tol
    arena.finish()


@pytest.mark.parametrize("cid", C.ids("gather16"))
def test_gather_rows16_huge_stride(lib, arena, cid):
    """vf_gather_rows_bf16 with ld_src, then ld_out, of 2^22 + 64 elements: exact rows
    (tests/test_ops_edges_gpu.py::test_gather_rows16_strided)."""
    case = C.BY_ID[cid]
    rows, d = C.GATHER16_ROWS, C.GATHER16_D
    (bits,) = arena.begin(case)
    big = bits.view(torch.bfloat16)
    g = torch.Generator().manual_seed(181)

    def run(src, idx, out):
        _check(lib.vf_gather_rows_bf16(src.data_ptr(), src.stride(0), idx.data_ptr(), out.data_ptr(), out.stride(0), idx.numel(), d,
                                       _st()), lib)
    if case.p["big"] == "src":
        table = _rand((rows, d), 182).bfloat16().cuda()
        big.copy_(table)
        idx = torch.randint(0, rows, (256,), generator=g)
        idx[:4] = torch.tensor([rows - 1, 0, 512, 511])
        assert int((idx >= 512).sum()) >= 40
        idx = idx.cuda()
        got, small = (torch.empty((256, d), dtype=torch.bfloat16, device="cuda") for _ in range(2))
        run(big, idx, got)
        run(table, idx, small)
    else:
        table = _rand((9, d), 182).bfloat16().cuda()
        idx = torch.randint(0, 9, (rows,), generator=g).cuda()
        got, small = big, torch.empty((rows, d), dtype=torch.bfloat16, device="cuda")
        run(table, idx, got)
        run(table, idx, small)
    torch.cuda.synchronize()
    assert _same(got, small) and torch.equal(small, table[idx]) and _finite(got)
    arena.finish()

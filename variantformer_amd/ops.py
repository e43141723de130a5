"""Tensor-level wrappers over the C ABI of libvf_hip.so.

torch is used only as the owner of device memory and of the HIP stream; every computation is a
hand-written HIP kernel.  All wrappers require CUDA(ROCm) tensors and raise otherwise.
"""
from __future__ import annotations

import contextlib
import contextvars
import math

import numpy as np
import torch

from . import _lib, runtime
from ._lib import (EPI_BF16, EPI_F32, EPI_GEGLU_BF16, EPI_GELU_BF16, EPI_GELU_F32, EPI_RES_F32, VF_BF16,  # noqa: F401
                   VF_F16, VF_F32, check)

# The 16-bit operand type of the GEMM / attention kernels: torch.bfloat16 (the reference's shipped `bf16-mixed`) or
# torch.float16 (its `16-mixed` / fp16 flash-attn path; BASELINE configs[4]).  fp32 accumulation either way.  The
# "*_BF16" epilogue names mean "16-bit output in the operand type".  Per context, like runtime.Switches (a thread starts with bf16).
_CDT: contextvars.ContextVar = contextvars.ContextVar("vf_compute_dtype", default=torch.bfloat16)


@contextlib.contextmanager
def compute_dtype(dtype):
    """with ops.compute_dtype(torch.float16): ...  -- 16-bit tensors created inside (LayerNorm outputs, casts, packed
    weights) use this operand type; kernels themselves follow the dtype of the tensors they are handed."""
    assert dtype in (torch.bfloat16, torch.float16), dtype
    token = _CDT.set(dtype)
    try:
        yield
    finally:
        _CDT.reset(token)


def cdt():
    return _CDT.get()


def _is16(dtype) -> bool:
    return dtype in (torch.bfloat16, torch.float16)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class KernelTimer:
    """Brackets individual kernel launches with HIP events ON THE STREAM THE KERNEL IS LAUNCHED ON (torch's
    current stream, which is the stream handed to the C ABI).  Used by bench.py for the roofline numbers."""

    def __init__(self, detail: bool = False):
        self.records = {}
        self.detail = detail          # also key records by launch geometry (scripts/shape_breakdown.py)
        self.order = []               # (name, geometry, family, flops | None, bytes | None) of every launch, in launch order
                                      # (scripts/pmc_shapes.py joins it with the dispatch order of a rocprofv3 counter pass)

    def time(self, name: str, flops, nbytes: float, launch, geometry: str = "", family: str = ""):
        """flops: a number, or a zero-argument callable evaluated in summary() (attention: the per-sequence lengths
        live on the device, and reading them here would put a host sync between the launches being timed).  nbytes: the
        same (topk_rows: the rows' lengths live on the device)."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = launch()
        b.record()
        rec = [a, b, flops, nbytes]
        self.records.setdefault(name, []).append(rec)
        if self.detail:
            self.order.append((name, geometry, family, None if callable(flops) else float(flops),
                               None if callable(nbytes) else float(nbytes)))
        if family:
            self.records.setdefault(f"{name}:{family}", []).append(rec)
        if self.detail and geometry:
            self.records.setdefault(f"{name}[{geometry}]", []).append(rec)
        return out

    def summary(self) -> dict:
        torch.cuda.synchronize()
        out = {}
        for name, recs in self.records.items():
            for r in recs:
                if callable(r[2]):
                    r[2] = float(r[2]())
                if callable(r[3]):
                    r[3] = float(r[3]())
            ms = sum(a.elapsed_time(b) for a, b, _, _ in recs)
            out[name] = {"launches": len(recs), "total_ms": ms, "flops": sum(r[2] for r in recs),
                         "bytes": sum(r[3] for r in recs)}
        return out


TIMER: KernelTimer | None = None
_SCOPE = ""          # default family label of launches made inside a `scope(...)` block (timer bookkeeping only)


class scope:
    """with ops.scope("seq2reg"): ...  -- launches without an explicit family are recorded under this label."""

    def __init__(self, name: str):
        self.name = name

    def __enter__(self):
        global _SCOPE
        self.prev, _SCOPE = _SCOPE, self.name

    def __exit__(self, *exc):
        global _SCOPE
        _SCOPE = self.prev
        return False


def _run(launch, record) -> None:
    """launch(), bracketed by the installed KernelTimer if there is one (ops.TIMER).  record() -> (name, flops, bytes,
    geometry, family) as KernelTimer.time takes them; evaluated only when a timer is installed."""
    if TIMER is not None:
        name, flops, nbytes, geometry, family = record()
        TIMER.time(name, flops, nbytes, launch, geometry, family)
    else:
        launch()


def _dev(*ts):
    """Every tensor must live on the CURRENT device: the C ABI launches on torch's current stream and never switches
    devices (one process per GPU; use torch.cuda.set_device / torch.cuda.device(...) around calls otherwise)."""
    cur = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.VFError("variantformer_amd ops need tensors on the GPU (no CPU fallback)")
        if cur is None:
            cur = torch.cuda.current_device()
        if t.device.index != cur:
            raise _lib.VFError(f"tensor on cuda:{t.device.index} but the current device is cuda:{cur}: "
                               "libvf_hip launches on the current device's stream (wrap the call in torch.cuda.device)")


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _dt(dtype) -> int:
    if dtype == torch.float32:
        return VF_F32
    if dtype == torch.bfloat16:
        return VF_BF16
    if dtype == torch.float16:
        return VF_F16
    raise _lib.VFError(f"unsupported dtype {dtype}")


def gemm(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None, epilogue: int,
         residual: torch.Tensor | None = None, out: torch.Tensor | None = None, variant: int = 0,
         family: str = "") -> torch.Tensor:
    """out = epilogue(a[M,K] @ w[N,K]^T + bias).  a, w both bf16 or both fp16 (a may be a row-strided view); 16-bit
    outputs come back in the operand type.  variant != 0 forces a tile configuration (vf_gemm_*_ex; tests only)."""
    _dev(a, w, bias, residual, out)
    assert _is16(a.dtype) and w.dtype == a.dtype and a.dim() == 2 and w.dim() == 2
    assert a.stride(1) == 1 and w.is_contiguous() and a.shape[1] == w.shape[1]
    M, K = a.shape
    N = w.shape[0]
    n_out = N // 2 if epilogue == EPI_GEGLU_BF16 else N
    odt = torch.float32 if epilogue in (EPI_F32, EPI_RES_F32, EPI_GELU_F32) else a.dtype
    if out is None:
        out = torch.empty((M, n_out), dtype=odt, device=a.device)
    assert out.dtype == odt and out.shape == (M, n_out) and out.stride(1) == 1
    ldr = 0
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.shape == (M, N) and residual.stride(1) == 1
        ldr = residual.stride(0)
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == N and bias.is_contiguous()
    lib = _lib.load()

    def launch():
        lda = a.stride(0) if M > 1 else max(a.stride(0), K)
        ldo = out.stride(0) if M > 1 else max(out.stride(0), n_out)
        f16 = a.dtype == torch.float16
        if variant:
            fn = lib.vf_gemm_f16_ex if f16 else lib.vf_gemm_bf16_ex
            check(fn(a.data_ptr(), lda, w.data_ptr(), _ptr(bias), _ptr(residual), ldr, out.data_ptr(),
                     ldo, M, N, K, epilogue, variant, _stream()), "vf_gemm_ex")
        else:
            fn = lib.vf_gemm_f16 if f16 else lib.vf_gemm_bf16
            check(fn(a.data_ptr(), lda, w.data_ptr(), _ptr(bias), _ptr(residual), ldr, out.data_ptr(),
                     ldo, M, N, K, epilogue, _stream()), "vf_gemm")
    _run(launch, lambda: ("gemm", 2.0 * M * N * K,
                          2.0 * (M * K + N * K) + out.numel() * out.element_size() + (0 if residual is None else 4.0 * M * N),
                          f"M={M} N={N} K={K} epi={epilogue}", family or _SCOPE))
    return out


class LnStream:
    """A residual stream as the LayerNorm-folding GEMMs exchange it: x fp32 [M, D] (None when the fp32 rows have no
    reader), x16 its 16-bit copy -- for fp16 streams stored SCALED, x16 = fp16(x * scale) --, stats fp32 [M, 2] =
    (mean * scale, rstd / scale) of every row: exactly the pair the consumer GEMM applies to its accumulator of the
    scaled operand (vf_gemm_ln / vf_ln_finalize2 / vf_row_stats_cast2).  scale = 1 for bf16 streams."""
    __slots__ = ("x", "x16", "stats", "scale", "t16")

    def __init__(self, x, x16, stats, scale: float = 1.0, t16=None):
        self.x, self.x16, self.stats, self.scale = x, x16, stats, float(scale)
        # fp16 trunk copy fp16(x * T16_SCALE) (layers.trunk16_mode() == "f16"): what the NEXT layer's down-projection adds
        # as its residual when the fp32 rows are not stored (vf_gemm_ln_t16)
        self.t16 = t16

    def operand16(self):
        """The stream as a plain 16-bit GEMM operand (un-normalised use: the K/V projection of a cross attention):
        the copy itself when it is unscaled, else a cast of the fp32 rows."""
        return self.x16 if self.scale == 1.0 else cast16(self.x, self.x16.dtype)


def x16_scale_for(dtype) -> float:
    """Power-of-two scale of the 16-bit copy of a residual stream: 1 for bf16 (fp32's exponent range); 2^-4 for fp16, which
    keeps |x| < 1e6 representable (the reference's own fp16 autocast overflows at 65504) at no cost in precision --
    10 mantissa bits at every magnitude above 1e-3 -- and LayerNorm is scale-invariant."""
    return 1.0 if dtype != torch.float16 else 2.0 ** -4


# Rows whose |mean| exceeds this many standard deviations make the folded LayerNorm -> Linear lose accuracy (it rounds
# the UNCENTRED row to 16 bits; tests/test_ops_gpu.py::test_ln_fold_rows_with_large_mean: error ~ 2^-9 x |mean| / std).
# The statistics kernels raise a device flag; ln_fold_alert() reads it (one int, with the outputs of a batch).
LN_FOLD_RATIO_LIMIT = 8.0
_ALERT: dict = {}


def _alert_flag(device) -> torch.Tensor:
    """The flag of the CURRENT STREAM of `device`: kernels raise the flag of the stream they run on, so concurrent streams
    (one model per stream / thread) never see each other's rows, and ln_fold_alert_take() -- enqueued on the same stream
    right after a batch's kernels -- cuts out exactly that batch's bits."""
    sid = torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0
    key = (device.type, device.index, sid)
    if key not in _ALERT:
        _ALERT[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _ALERT[key]


def ln_fold_alert_clear(device) -> None:
    """Enqueue a reset of the current stream's flag (start of a batch: bits left by direct forward() calls, benchmarks or a
    discarded batch belong to nobody)."""
    if device.type == "cuda":
        _alert_flag(device).zero_()


def ln_fold_alert_take(device):
    """Enqueue `bits = flag; flag = 0` on the current stream and return the device tensor `bits` ([1] int32): the alert of
    everything this stream ran since the last clear / take, i.e. of ONE batch when called where the batch's last kernel was
    enqueued.  Does not synchronise; read it with the batch's outputs.  None on a CPU device."""
    if device.type != "cuda":
        return None
    flag = _alert_flag(device)
    bits = flag.clone()
    flag.zero_()
    return bits


# Elements at or beyond this magnitude could overflow a scaled fp16 copy of a stream (65504 / 2^-4 with some margin): the
# statistics kernels bound every element of a row by |mean| + sqrt(D * var) and raise bit 1 of the flag (ABI 6).
def ln_fold_abs_limit() -> float:
    """Largest |x| the 16-bit copies of a LayerNorm-folded stream represent: unbounded (0 = no check) when every copy is
    bf16; 60000 / scale for the fp16 copy with the least headroom (fp16 operand copy, fp16 trunk copy)."""
    scales = []
    if cdt() == torch.float16:
        scales.append(x16_scale_for(torch.float16))
    if runtime.env().trunk16 == "f16":           # VF_TRUNK16, read once per forward (runtime.forward_env)
        scales.append(T16_SCALE)
    return 60000.0 / max(scales) if scales else 0.0


def ln_fold_alert(device, reset: bool = True) -> int:
    """Non-zero when, since the last reset, a LayerNorm-folded stream ON THE CURRENT STREAM left the regime its 16-bit copies
    serve: bit 0 -- some row had |mean| > LN_FOLD_RATIO_LIMIT standard deviations; bit 1 -- some row may hold an element
    beyond ln_fold_abs_limit() (a scaled fp16 copy could overflow).  Synchronises (op-level callers and tests; the model
    carries a per-batch copy instead: ln_fold_alert_take).  The model recomputes a flagged batch with the separate LayerNorm
    on fp32 rows (layers.ln_fold_forced_off) -- degraded numbers are never returned."""
    if device.type != "cuda":
        return 0
    sid = torch.cuda.current_stream(device).cuda_stream
    key = (device.type, device.index, sid)
    if key not in _ALERT:
        return 0
    hit = int(_ALERT[key].item())
    if hit and reset:
        _ALERT[key].zero_()
    return hit


def ln_stream(x: torch.Tensor, eps: float = 1e-5, raise_alert: bool = True) -> LnStream:
    """(x, 16-bit copy, row statistics) for a stream no GEMM produced: one pass over x (vf_row_stats_cast2).
    raise_alert=False: the rows are a TABLE of which a batch uses only some (the registry table in front of the first gene
    layer); the caller raises the alert for the rows in use itself."""
    _dev(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
    M, D = x.shape
    x16 = torch.empty((M, D), dtype=cdt(), device=x.device)
    stats = torch.empty((M, 2), dtype=torch.float32, device=x.device)
    scale = x16_scale_for(x16.dtype)
    alert_ptr = _alert_flag(x.device).data_ptr() if raise_alert else 0

    def launch():
        check(_lib.load().vf_row_stats_cast2(x.data_ptr(), M, D, eps, x16.data_ptr(), _dt(x16.dtype), scale, LN_FOLD_RATIO_LIMIT,
                                             ln_fold_abs_limit(), alert_ptr, stats.data_ptr(), _stream()),
              "vf_row_stats_cast")
    _run(launch, lambda: ("layernorm", 0.0, float(M) * D * 6, f"stats_cast D={D}", _SCOPE))
    return LnStream(x, x16, stats, scale)


def ln_stream_rows(s: LnStream, rows: torch.Tensor) -> LnStream:
    """The rows `rows` (int64) of a stream, statistics included (bit-identical to the full stream's)."""
    return LnStream(None if s.x is None else gather_rows_f32(s.x, None, rows), gather_rows_bf16(s.x16, rows),
                    gather_rows_f32(s.stats, None, rows), s.scale,
                    None if s.t16 is None else gather_rows_bf16(s.t16, rows))


T16_SCALE = 2.0 ** -4          # the fp16 trunk copy is fp16(x * 2^-4): |x| < 1e6 representable (x16_scale_for(fp16))


def trunk16_of(x: torch.Tensor, raise_alert: bool = True) -> torch.Tensor:
    """fp16(x * T16_SCALE) of an fp32 stream no trunk-writing GEMM produced (a stack's input): one pass
    (vf_row_stats_cast2 with an fp16 output; its statistics are not used).  raise_alert=False: a table of which a batch uses
    only some rows (see ln_stream)."""
    _dev(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
    M, D = x.shape
    t16 = torch.empty((M, D), dtype=torch.float16, device=x.device)
    stats = torch.empty((M, 2), dtype=torch.float32, device=x.device)

    alert_ptr = _alert_flag(x.device).data_ptr() if raise_alert else 0

    def launch():       # ratio limit off (1e30): this stream's statistics are the caller's business; range check on
        check(_lib.load().vf_row_stats_cast2(x.data_ptr(), M, D, 1e-5, t16.data_ptr(), VF_F16, T16_SCALE, 1e30,
                                             60000.0 / T16_SCALE, alert_ptr, stats.data_ptr(), _stream()),
              "vf_row_stats_cast")
    _run(launch, lambda: ("layernorm", 0.0, float(M) * D * 6, f"trunk16_of D={D}", _SCOPE))
    return t16


def gemm_ln_consumer(s: LnStream, w: torch.Tensor, bias: torch.Tensor, colsum: torch.Tensor, epilogue: int,
                     family: str = "") -> torch.Tensor:
    """epilogue(LN(s.x) @ W^T + b) without materialising LN(s.x): w = 16-bit(gamma (.) W) [N, K], bias = W beta + b,
    colsum = rowsum(w) (layers.packed_linear_ln).  epilogue EPI_BF16 or EPI_GEGLU_BF16 (16-bit output, operand type), or
    EPI_F32 (fp32 rows: the logits of softmax_counted)."""
    a = s.x16
    _dev(a, w, bias, colsum, s.stats)
    assert _is16(a.dtype) and w.dtype == a.dtype and a.shape[1] == w.shape[1] and a.stride(1) == 1
    assert epilogue in (EPI_BF16, EPI_GEGLU_BF16, EPI_F32)
    M, K = a.shape
    N = w.shape[0]
    n_out = N // 2 if epilogue == EPI_GEGLU_BF16 else N
    out = torch.empty((M, n_out), dtype=torch.float32 if epilogue == EPI_F32 else a.dtype, device=a.device)
    lib = _lib.load()

    def launch():
        check(lib.vf_gemm_ln(a.data_ptr(), a.stride(0) if M > 1 else max(a.stride(0), K), w.data_ptr(), bias.data_ptr(),
                             0, 0, VF_F32, out.data_ptr(), n_out, M, N, K, epilogue, _dt(a.dtype), s.stats.data_ptr(),
                             colsum.data_ptr(), 0, 0, 0, 1.0, 1.0, _stream()), "vf_gemm_ln")
    _run(launch, lambda: ("gemm", 2.0 * M * N * K, 2.0 * (M * K + N * K) + out.numel() * out.element_size() + 8.0 * M,
                          f"M={M} N={N} K={K} epi={epilogue} ln=consumer", family or _SCOPE))
    return out


def gemm_ln_producer(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None, residual,
                     eps: float = 1e-5, family: str = "", need_x: bool = True, trunk16: torch.Tensor | None = None,
                     need_t16: bool = False) -> LnStream:
    """x = a @ w^T + bias (+ residual), fp32, returned together with its 16-bit copy and row statistics (the next
    LayerNorm's): EPI_RES_F32 when a residual is given, else EPI_F32.  `residual`: an fp32 tensor [M, N], or an LnStream
    whose 16-BIT COPY is the residual (its fp32 rows need not exist).  need_x=False: the fp32 x itself has no reader (a
    layer's intermediate stream feeds only the next LayerNorm -> Linear pair) and is not stored; .x is None.
    `trunk16` (instead of `residual`): the residual as the fp16 trunk copy fp16(r * T16_SCALE) of the layer input
    (vf_gemm_ln_t16); need_t16: also write that copy of the result (.t16) for the next layer."""
    assert residual is None if trunk16 is not None else not need_t16
    res16 = residual if isinstance(residual, LnStream) else None
    res32 = None if res16 is not None else residual
    _dev(a, w, bias, res32, None if res16 is None else res16.x16, trunk16)
    assert _is16(a.dtype) and w.dtype == a.dtype and a.shape[1] == w.shape[1] and a.stride(1) == 1
    M, K = a.shape
    N = w.shape[0]
    out = torch.empty((M, N), dtype=torch.float32, device=a.device) if need_x else None
    t_out = torch.empty((M, N), dtype=torch.float16, device=a.device) if need_t16 else None
    x16 = torch.empty((M, N), dtype=a.dtype, device=a.device)
    n_parts = (N + 31) // 32
    part = torch.empty((n_parts, M, 2), dtype=torch.float32, device=a.device)
    stats = torch.empty((M, 2), dtype=torch.float32, device=a.device)
    scale = x16_scale_for(a.dtype)
    alert = _alert_flag(a.device)
    lib = _lib.load()
    lda = a.stride(0) if M > 1 else max(a.stride(0), K)
    if trunk16 is not None:
        assert trunk16.dtype == torch.float16 and trunk16.shape == (M, N) and trunk16.stride(1) == 1
        epi, res_bytes = EPI_RES_F32, (2.0 + (2.0 if need_t16 else 0.0)) * M * N
        tag = "-t16" + ("" if need_t16 else "-in")

        def launch():
            check(lib.vf_gemm_ln_t16(a.data_ptr(), lda, w.data_ptr(), _ptr(bias), trunk16.data_ptr(), trunk16.stride(0),
                                     1.0 / T16_SCALE, _ptr(out), N, M, N, K, _dt(a.dtype), x16.data_ptr(), N, part.data_ptr(),
                                     scale, _ptr(t_out), N, T16_SCALE, _stream()), "vf_gemm_ln_t16")
    else:
        epi = EPI_F32 if residual is None else EPI_RES_F32
        if res32 is not None:
            assert res32.dtype == torch.float32 and res32.shape == (M, N) and res32.stride(1) == 1
            r_ptr, r_ld, r_dt, r_scale, res_bytes, tag = res32.data_ptr(), res32.stride(0), VF_F32, 1.0, 4.0 * M * N, ""
        elif res16 is not None:
            r = res16.x16
            assert r.dtype == a.dtype and r.shape == (M, N) and r.stride(1) == 1
            r_ptr, r_ld, r_dt, r_scale, res_bytes, tag = r.data_ptr(), r.stride(0), _dt(r.dtype), 1.0 / res16.scale, 2.0 * M * N, "-r16"
        else:
            r_ptr, r_ld, r_dt, r_scale, res_bytes, tag = 0, 0, VF_F32, 1.0, 0.0, ""

        def launch():
            check(lib.vf_gemm_ln(a.data_ptr(), lda, w.data_ptr(), _ptr(bias), r_ptr, r_ld, r_dt, _ptr(out), N, M, N, K, epi,
                                 _dt(a.dtype), 0, 0, x16.data_ptr(), N, part.data_ptr(), scale, r_scale, _stream()), "vf_gemm_ln")

    def finalize():
        check(lib.vf_ln_finalize2(part.data_ptr(), M, n_parts, N, eps, scale, LN_FOLD_RATIO_LIMIT, ln_fold_abs_limit(),
                                  alert.data_ptr(), stats.data_ptr(), _stream()), "vf_ln_finalize")
    _run(launch, lambda: ("gemm", 2.0 * M * N * K,
                          2.0 * (M * K + N * K) + M * N * ((4.0 if need_x else 0.0) + 2.0) + res_bytes + 8.0 * M * n_parts,
                          f"M={M} N={N} K={K} epi={epi} ln=producer{'' if need_x else '-nox'}{tag}", family or _SCOPE))
    _run(finalize, lambda: ("layernorm", 0.0, 8.0 * M * (n_parts + 1), f"finalize D={N}", _SCOPE))
    return LnStream(out, x16, stats, scale, t_out)


def pack_geglu_rows(w: torch.Tensor, bias: torch.Tensor | None):
    """Permute a [2F,K] 16-bit weight (+ fp32 bias) into the GEGLU-epilogue row order."""
    _dev(w, bias)
    assert _is16(w.dtype) and w.is_contiguous()
    wo = torch.empty_like(w)
    bo = torch.empty_like(bias) if bias is not None else None
    check(_lib.load().vf_pack_geglu_rows(w.data_ptr(), _ptr(bias), wo.data_ptr(), _ptr(bo), w.shape[0], w.shape[1],
                                         _stream()), "vf_pack_geglu_rows")
    return wo, bo


ATTN_Q_AT_START, ATTN_Q_LOG2 = 1, 2          # enum vf_attn_flags


def attn_counted_keys(q: torch.Tensor, kv_table: torch.Tensor, log2_count: torch.Tensor, cu_q: torch.Tensor, max_q: int,
                      n_heads: int, head_dim: int, family: str = "") -> torch.Tensor:
    """Cross attention against keys that are copies of the C <= 16 distinct rows of kv_table [C, 2 H dh] (K | V), row c
    occurring 2^log2_count[s, c] times among sequence s's keys (vf_attn_counted_keys): softmax over the distinct rows with
    log2(count) added to the base-2 logit.  q [tokens, >= H dh] 16-bit, pre-scaled (the model's q_log2 form)."""
    _dev(q, kv_table, log2_count, cu_q)
    assert _is16(q.dtype) and kv_table.dtype == q.dtype and q.stride(1) == 1 and kv_table.stride(1) == 1
    assert log2_count.dtype == torch.float32 and log2_count.is_contiguous() and cu_q.dtype == torch.int32
    D = n_heads * head_dim
    n_seq, C = cu_q.numel() - 1, kv_table.shape[0]
    assert log2_count.shape == (n_seq, C) and kv_table.shape[1] >= 2 * D
    out = torch.empty((q.shape[0], D), dtype=q.dtype, device=q.device)

    def launch():
        check(_lib.load().vf_attn_counted_keys(q.data_ptr(), q.stride(0), kv_table.data_ptr(), kv_table.stride(0),
                                               log2_count.data_ptr(), cu_q.data_ptr(), n_seq, int(max_q), C, n_heads, head_dim,
                                               out.data_ptr(), out.stride(0), _dt(q.dtype), _stream()), "vf_attn_counted_keys")
    _run(launch, lambda: ("attn", 4.0 * q.shape[0] * C * D, 2.0 * D * 2 * q.shape[0],       # executed work: 4 * tokens * C * width
                          f"H={n_heads} dh={head_dim} max_q={int(max_q)} counted_keys={C}", family or _SCOPE))
    return out


def softmax_counted(scores: torch.Tensor, log2_count: torch.Tensor, cu_q: torch.Tensor, max_q: int, n_heads: int, slots: int,
                    out_dtype=None, family: str = "") -> torch.Tensor:
    """16-bit softmax over the C = log2_count.shape[1] distinct keys of every (token, head), log2(count) added to the base-2
    logits scores fp32 [tokens, H * slots] (slots >= C per head, the padding gets weight 0): vf_softmax_counted."""
    _dev(scores, log2_count, cu_q)
    assert scores.dtype == torch.float32 and scores.stride(1) == 1 and log2_count.dtype == torch.float32 and log2_count.is_contiguous()
    T, n_seq, C = scores.shape[0], cu_q.numel() - 1, log2_count.shape[1]
    assert scores.shape[1] >= n_heads * slots and log2_count.shape[0] == n_seq
    dt = cdt() if out_dtype is None else out_dtype
    out = torch.empty((T, n_heads * slots), dtype=dt, device=scores.device)

    def launch():
        check(_lib.load().vf_softmax_counted(scores.data_ptr(), scores.stride(0), log2_count.data_ptr(), cu_q.data_ptr(), n_seq,
                                             int(max_q), n_heads, slots, C, out.data_ptr(), out.stride(0), _dt(dt), _stream()),
              "vf_softmax_counted")
    _run(launch, lambda: ("attn", 0.0, float(T) * n_heads * slots * 6, f"softmax_counted H={n_heads} C={C}", family or _SCOPE))
    return out


def attn_rows_supported(head_dim: int, alibi: bool, n_seq: int, n_heads: int, max_q: int, max_k: int, q_log2: bool) -> bool:
    """Whether attn_varlen(rows=...) has a kernel for this geometry (vf_attn_rows_supported); otherwise the caller gathers the
    rows (gather_rows_bf16) and calls the plain form -- same bits either way."""
    return bool(_lib.load().vf_attn_rows_supported(int(head_dim), int(bool(alibi)), int(n_seq), int(n_heads), int(max_q),
                                                   int(max_k), ATTN_Q_LOG2 if q_log2 else 0))


# head dims with kernels of their own; every other multiple of 8 up to 256 runs the kernels of its class (vf_attn_varlen_fwd_v3)
ATTN_CLASS_DIMS = (32, 48, 64, 96, 128)


def attn_varlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_q: torch.Tensor, cu_k: torch.Tensor | None,
                max_q: int, max_k: int, n_heads: int, head_dim: int, slopes: torch.Tensor | None = None,
                scale: float | None = None, out: torch.Tensor | None = None, q_at_start: bool = False,
                family: str = "", q_log2: bool = False, rows: torch.Tensor | None = None) -> torch.Tensor:
    """q [tq, >=H*dh] / k, v [tk, >=H*dh] bf16 row-strided views whose first H*dh columns are the heads.
    q_at_start: ALiBi positions of the queries count from the start of the key sequence (default: flash-attn's
    end alignment).  q_log2: q was projected with weights pre-multiplied by scale * log2(e) (layers.q_prescale): q . k is the
    base-2 logit, `scale` is not applied again (VF_ATTN_Q_LOG2).
    rows int64 [tokens] (self attention only, vf_attn_varlen_fwd_rows): q / k / v are tables of distinct rows, token t's
    row is rows[t]; the gather happens in the kernel's loads (attn_rows_supported says for which geometries)."""
    _dev(q, k, v, cu_q, cu_k, slopes, out, rows)
    for t in (q, k, v):
        assert _is16(t.dtype) and t.dtype == q.dtype and t.dim() == 2 and t.stride(1) == 1
    assert cu_q.dtype == torch.int32 and (cu_k is None or cu_k.dtype == torch.int32)
    D = n_heads * head_dim
    tq = q.shape[0] if rows is None else rows.numel()
    tk = k.shape[0] if rows is None else rows.numel()
    if rows is not None:
        assert rows.dtype == torch.int64 and rows.is_contiguous() and cu_k is None
    if out is None:
        out = torch.empty((tq, D), dtype=q.dtype, device=q.device)
    if scale is None:
        scale = 1.0 / math.sqrt(head_dim)
    if slopes is not None:
        assert slopes.dtype == torch.float32 and slopes.numel() == n_heads
    def launch():
        lib = _lib.load()
        flags = (ATTN_Q_AT_START if q_at_start else 0) | (ATTN_Q_LOG2 if q_log2 else 0)
        if rows is not None:
            check(lib.vf_attn_varlen_fwd_rows(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), q.stride(0), k.stride(0),
                                              v.stride(0), out.stride(0), cu_q.data_ptr(), None, cu_q.numel() - 1, int(max_q),
                                              int(max_k), n_heads, head_dim, _ptr(slopes), float(scale), _dt(q.dtype), flags,
                                              rows.data_ptr(), rows.data_ptr(), _stream()), "vf_attn_varlen_fwd_rows")
            return
        # the five class head dims keep the v2 entry; any other multiple of 8 up to 256 runs its padded class (v3)
        fwd = lib.vf_attn_varlen_fwd_v2 if head_dim in ATTN_CLASS_DIMS else lib.vf_attn_varlen_fwd_v3
        check(fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), q.stride(0), k.stride(0),
                  v.stride(0), out.stride(0), cu_q.data_ptr(), _ptr(cu_k), cu_q.numel() - 1, int(max_q),
                  int(max_k), n_heads, head_dim, _ptr(slopes), float(scale), _dt(q.dtype), flags,
                  _stream()), "vf_attn_varlen_fwd")

    def flops():       # 4 * sum_seq(len_q * len_k) * H * dh (QK^T and PV), evaluated after the timed replay
        lq = (cu_q[1:] - cu_q[:-1]).double()
        lk = lq if cu_k is None else (cu_k[1:] - cu_k[:-1]).double()
        return 4.0 * float((lq * lk).sum().item()) * D
    _run(launch, lambda: ("attn", flops, 2.0 * D * (2 * tq + 2 * tk),
                          f"H={n_heads} dh={head_dim} max_q={int(max_q)} max_k={int(max_k)}" + (" rows" if rows is not None else ""),
                          family or _SCOPE))
    return out


def attn_probs(q: torch.Tensor, k: torch.Tensor, cu_rows: torch.Tensor, cu_k: torch.Tensor, max_rows: int, max_k: int,
               n_heads: int, head_dim: int, q_rows: torch.Tensor | None = None, q_log2: bool = True, per_head: bool = False,
               scale: float | None = None, out: torch.Tensor | None = None, family: str = "",
               slopes: torch.Tensor | None = None, q_pos: torch.Tensor | None = None, k_rows: torch.Tensor | None = None):
    """fp32 softmax probabilities of selected query rows against their sequence's keys (vf_attn_probs_v2; attention maps).
    q [*, >=H*dh] / k [tk, >=H*dh] 16-bit row-strided views; selected row r (cu_rows int32 [n_seq + 1] groups them per key
    sequence) is row q_rows[r] of q (int64; None: row r, and q holds exactly the selected rows).  Returns (out, stats):
    out fp32 [R, max_k] = the head mean, or [R * H, max_k] per head (columns past a sequence's keys are 0; a caller's `out`
    may be wider: columns >= max_k are left alone); stats fp32 [R, H, 2] = (m, l) of every row and head, base 2.
    slopes fp32 [H]: ALiBi, the base-2 logit loses log2(e) * slopes[h] * |q_pos[r] - j| (j = the key's position in its sequence);
    q_pos int32 [R]: the position of every selected row in its key sequence (None: 0; ignored without slopes);
    k_rows int64 [total keys]: k is a table and key t (in cu_k's numbering) is its row k_rows[t] -- the bits of a call on
    k[k_rows]."""
    _dev(q, k, cu_rows, cu_k, q_rows, out, slopes, q_pos, k_rows)
    for t in (q, k):
        assert _is16(t.dtype) and t.dtype == q.dtype and t.dim() == 2 and t.stride(1) == 1
    assert cu_rows.dtype == torch.int32 and cu_k.dtype == torch.int32 and cu_rows.numel() == cu_k.numel()
    D = n_heads * head_dim
    if q_rows is not None:
        assert q_rows.dtype == torch.int64 and q_rows.is_contiguous()
    R = q.shape[0] if q_rows is None else q_rows.numel()
    n_out = R * n_heads if per_head else R
    if out is None:
        out = torch.empty((n_out, int(max_k)), dtype=torch.float32, device=q.device)
    assert out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == n_out and out.shape[1] >= max_k and out.stride(1) == 1
    stats = torch.empty((R, n_heads, 2), dtype=torch.float32, device=q.device)
    if scale is None:
        scale = 1.0 / math.sqrt(head_dim)
    if slopes is not None:
        assert slopes.dtype == torch.float32 and slopes.is_contiguous() and slopes.numel() == n_heads
    if q_pos is not None:
        assert q_pos.dtype == torch.int32 and q_pos.is_contiguous() and q_pos.numel() == R
    if k_rows is not None:
        assert k_rows.dtype == torch.int64 and k_rows.is_contiguous()
    tk = k.shape[0] if k_rows is None else k_rows.numel()
    # index loads per pass: the key row map (8 bytes per key) and, with a bias, the positions and the slopes
    idx_bytes = 2.0 * ((8.0 * tk if k_rows is not None else 0.0) + (4.0 * R if slopes is not None and q_pos is not None else 0.0)
                       + (4.0 * n_heads if slopes is not None else 0.0) + (8.0 * R if q_rows is not None else 0.0))

    def launch():
        if R == 0:
            return
        check(_lib.load().vf_attn_probs_v2(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), _ptr(q_rows), cu_rows.data_ptr(),
                                        cu_k.data_ptr(), cu_rows.numel() - 1, int(max_rows), int(max_k), n_heads, head_dim,
                                        float(scale), _dt(q.dtype), ATTN_Q_LOG2 if q_log2 else 0, int(bool(per_head)),
                                           stats.data_ptr(), out.data_ptr(), out.stride(0), _ptr(slopes),
                                           _ptr(q_pos), _ptr(k_rows), _stream()),
              "vf_attn_probs_v2")

    def flops():       # 2 passes x 2 * sum_seq(rows * len_k) * H * dh (+ 3 per biased logit), evaluated after the timed replay
        lr = (cu_rows[1:] - cu_rows[:-1]).double()
        lk = (cu_k[1:] - cu_k[:-1]).double()
        pairs = float((lr * lk).sum().item())
        return 4.0 * pairs * D + (6.0 * pairs * n_heads if slopes is not None else 0.0)
    # K is read once per pass (every key of every sequence, through the row map where there is one); the selected queries
    # twice; out and stats written once; the index loads once per pass
    _run(launch, lambda: ("attn_probs_alibi" if slopes is not None else "attn_probs", flops,
                          2.0 * D * (2 * tk + 2 * R) + 4.0 * n_out * int(max_k) + 16.0 * R * n_heads + idx_bytes,
                          f"H={n_heads} dh={head_dim} max_rows={int(max_rows)} max_k={int(max_k)}" + (" per_head" if per_head else "")
                          + (" k_rows" if k_rows is not None else ""),
                          family or _SCOPE))
    return out, stats


def attn_contrib(v: torch.Tensor, s_gram: torch.Tensor, probs: torch.Tensor, cu_rows: torch.Tensor, cu_k: torch.Tensor,
                 max_rows: int, max_k: int, n_heads: int, head_dim: int, gram: torch.Tensor, out: torch.Tensor,
                 per_head: bool = False, family: str = ""):
    """Value-weighted norms beside an attention map (vf_attn_contrib, include/vf_hip_attn_contrib.h): out[r, j] = || sum_h P[r, h, j] *
    Wo_h v[j, h] ||_2, or per head out[r * H + h, j] = P[r, h, j] * || Wo_h v[j, h] ||_2.  v [tk, >= H*dh] 16-bit row-strided view
    (the value rows the attention kernel reads); s_gram fp32 [H, H, dh, dh] = Wo_h^T Wo_h' (per weights); probs fp32 [R * H, >=
    max_k] = ops.attn_probs(per_head=True) of the same rows and grouping.  The caller owns every buffer, and nothing is made
    here: gram fp32 [>= tk, H, H] (an output: the keys' Gram matrices) and out fp32 [R or R * H, >= max_k] are reused across
    layers by the capture.  Columns past a sequence's keys are 0, columns >= max_k are left alone.  Returns out."""
    _dev(v, s_gram, probs, cu_rows, cu_k, gram, out)
    assert _is16(v.dtype) and v.dim() == 2 and v.stride(1) == 1
    assert cu_rows.dtype == torch.int32 and cu_k.dtype == torch.int32 and cu_rows.numel() == cu_k.numel()
    H, dh = int(n_heads), int(head_dim)
    assert s_gram.dtype == torch.float32 and s_gram.is_contiguous() and tuple(s_gram.shape) == (H, H, dh, dh)
    for t in (probs, out):
        assert t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[1] >= max_k
    assert probs.shape[0] % H == 0
    R = probs.shape[0] // H
    assert out.shape[0] == (R * H if per_head else R)
    tk = v.shape[0]
    assert gram.dtype == torch.float32 and gram.is_contiguous() and gram.numel() >= tk * H * H

    def launch():
        if R == 0:
            return
        check(_lib.load().vf_attn_contrib(v.data_ptr(), v.stride(0), s_gram.data_ptr(), probs.data_ptr(), probs.stride(0),
                                          cu_rows.data_ptr(), cu_k.data_ptr(), cu_rows.numel() - 1, int(max_rows), int(max_k), H, dh,
                                          _dt(v.dtype), int(bool(per_head)), gram.data_ptr(), out.data_ptr(), out.stride(0),
                                          _stream()), "vf_attn_contrib")

    def flops():       # the Gram stage: every key x the upper triangle of head pairs x (dh^2 + dh) MACs; the norms: H^2 per (row, key)
        lr = (cu_rows[1:] - cu_rows[:-1]).double()
        lk = (cu_k[1:] - cu_k[:-1]).double()
        return 2.0 * float(lk.sum().item()) * (H * (H + 1) / 2) * (dh * dh + dh) + 2.0 * float((lr * lk).sum().item()) * H * H
    # v is read once per key chunk (the other head pairs of a chunk hit L2), S once, gram written and read once, P and out once
    _run(launch, lambda: ("attn_contrib", flops,
                          2.0 * tk * H * dh + 4.0 * s_gram.numel() + 8.0 * tk * H * H + 4.0 * R * H * int(max_k) + 4.0 * out.shape[0] * int(max_k),
                          f"H={H} dh={dh} max_rows={int(max_rows)} max_k={int(max_k)}" + (" per_head" if per_head else ""),
                          family or _SCOPE))
    return out


def attn_contrib_self(v: torch.Tensor, wo: torch.Tensor, probs: torch.Tensor, cu_k: torch.Tensor, max_k: int, n_heads: int,
                      head_dim: int, out: torch.Tensor, per_head: bool = False, v_rows: torch.Tensor | None = None,
                      family: str = ""):
    """Value-weighted norms beside a SELF attention map with one selected row per sequence (vf_attn_contrib_self,
    include/vf_hip_gene_contrib.h): out[s, j] = || sum_h P[s, h, j] * Wo_h v[t, h] ||_2, t = cu_k[s] + j, or per head
    out[s * H + h, j] = P[s, h, j] * || Wo_h v[t, h] ||_2.  v [*, >= H*dh] 16-bit row-strided view (the value rows the attention
    kernel reads); v_rows int64 [keys] or None: key t is row v_rows[t] of v; wo 16-bit [Do, >= H*dh] row-strided, out_proj's
    weight as packed_linear returns it; probs fp32 [n_seq * H, >= max_k] = ops.attn_probs(per_head=True) with one row per
    sequence.  The caller owns every buffer, nothing is made here and the kernel needs no workspace: out fp32 [n_seq or
    n_seq * H, >= max_k].  Columns past a sequence's keys are 0, columns >= max_k are left alone.  Returns out."""
    _dev(v, wo, probs, cu_k, out)
    assert _is16(v.dtype) and v.dim() == 2 and v.stride(1) == 1
    assert wo.dtype == v.dtype and wo.dim() == 2 and wo.stride(1) == 1
    assert cu_k.dtype == torch.int32 and cu_k.dim() == 1
    H, dh = int(n_heads), int(head_dim)
    n_seq = cu_k.numel() - 1
    for t in (probs, out):
        assert t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[1] >= max_k
    assert probs.shape[0] == n_seq * H and out.shape[0] == (n_seq * H if per_head else n_seq)
    if v_rows is not None:
        _dev(v_rows)
        assert v_rows.dtype == torch.int64 and v_rows.dim() == 1 and v_rows.is_contiguous()
    Do = wo.shape[0]

    def launch():
        check(_lib.load().vf_attn_contrib_self(v.data_ptr(), v.stride(0), 0 if v_rows is None else v_rows.data_ptr(),
                                               wo.data_ptr(), wo.stride(0), probs.data_ptr(), probs.stride(0), cu_k.data_ptr(),
                                               n_seq, int(max_k), H, dh, Do, _dt(v.dtype), int(bool(per_head)), out.data_ptr(),
                                               out.stride(0), _stream()), "vf_attn_contrib_self")

    def keys():
        return float(cu_k[-1].item()) if n_seq > 0 else 0.0
    # algorithmic bytes: every value row and P once, wo once, out once (the kernel re-reads v once per group of Wo tiles and
    # wo once per block; both are traffic of the tiling, not of the problem)
    _run(launch, lambda: ("attn_contrib_self", lambda: 2.0 * keys() * H * dh * Do,
                          2.0 * keys() * H * dh + 2.0 * Do * H * dh + 4.0 * n_seq * H * int(max_k) + 4.0 * out.shape[0] * int(max_k),
                          f"H={H} dh={dh} Do={Do} max_k={int(max_k)}" + (" per_head" if per_head else "") + (" rows" if v_rows is not None else ""),
                          family or _SCOPE))
    return out


def tissue_heads(x: torch.Tensor, n_strands: int, strand_agg, w: torch.Tensor, bias: torch.Tensor,
                 tissue_of_row: torch.Tensor | None = None, tissues: torch.Tensor | None = None, probabilities: bool = False, *,
                 out: torch.Tensor, argmax: torch.Tensor | None, checked: bool = False, family: str = ""):
    """The tokenizer's per-tissue classifier heads (vf_tissue_heads, include/vf_hip_cre_heads.h).  x fp32 [B * n_strands, >= d]
    row-strided, the strands of a sample adjacent; strand_agg "mean" / "concat" (or 0 / 1); w fp32 [T, C, F] and bias fp32 [T, C]
    contiguous, F = d or n_strands * d.  Row form: tissue_of_row int64 [B] on the device, sample b through the head of its own
    tissue -> out fp32 [B, >= C], argmax int32 [B].  All form: tissues int32 [n_sel] on the device, every sample through each of
    them -> out fp32 [B, >= n_sel * C], argmax int32 [B, n_sel].  Logits, or with probabilities=True the softmax over the
    classes; argmax is the first largest logit, -1 where a logit is NaN.  The caller owns every buffer and nothing is made here,
    as in attn_contrib: out (2-D, row stride >= the values of a row; columns past them are left alone) and argmax (contiguous;
    None: not wanted, none is written) must be passed.  The ids are checked with one read-back of their minimum and maximum (the reference's
    torch.unique(...).item() loop syncs too), and an id without a head raises KeyError like the reference's ModuleDict lookup;
    checked=True skips the read-back for ids the caller built from host data it has checked itself (the kernel reads nothing
    for an id without a head either way).  Returns (out, argmax)."""
    _dev(x, w, bias, tissue_of_row, tissues, out, argmax)
    ns = int(n_strands)
    agg = {"mean": 0, "concat": 1}.get(strand_agg, strand_agg)
    assert agg in (0, 1), f"strand_agg must be 'mean' or 'concat', not {strand_agg!r}"
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and ns >= 1 and x.shape[0] % ns == 0
    assert w.dtype == torch.float32 and w.dim() == 3 and w.is_contiguous()
    T, C, F = w.shape
    assert bias.dtype == torch.float32 and bias.is_contiguous() and tuple(bias.shape) == (T, C)
    d = F // ns if agg == 1 else F
    assert d * (ns if agg == 1 else 1) == F and x.shape[1] >= d
    B = x.shape[0] // ns
    if (tissue_of_row is None) == (tissues is None):
        raise ValueError("tissue_heads takes tissue_of_row (one head per sample) or tissues (every sample through each): "
                         + ("not both" if tissues is not None else "one of them is required"))
    if tissue_of_row is not None:
        assert tissue_of_row.dtype == torch.int64 and tissue_of_row.is_contiguous() and tuple(tissue_of_row.shape) == (B,)
        ids, n_sel = tissue_of_row, 1
    else:
        assert tissues.dtype == torch.int32 and tissues.dim() == 1 and tissues.is_contiguous()
        ids, n_sel = tissues, tissues.numel()
    if not checked and ids.numel():
        lo, hi = torch.stack(torch.aminmax(ids)).tolist()
        if lo < 0 or hi >= T:
            raise KeyError(str(lo if lo < 0 else hi))
    assert out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] == B and out.shape[1] >= n_sel * C
    assert argmax is None or (argmax.dtype == torch.int32 and argmax.is_contiguous() and argmax.numel() == B * n_sel)

    def launch():
        if B == 0 or n_sel == 0:                      # nothing to do (an empty tensor has no address to hand over)
            return
        check(_lib.load().vf_tissue_heads(x.data_ptr(), x.stride(0), ns, agg, w.data_ptr(), bias.data_ptr(), T, C, d,
                                          _ptr(tissue_of_row), _ptr(tissues), n_sel, B, int(bool(probabilities)),
                                          out.data_ptr(), out.stride(0), _ptr(argmax), _stream()), "vf_tissue_heads")
    # algorithmic bytes: x, the heads and the outputs once (the kernel re-reads a head per sample, from L2)
    _run(launch, lambda: ("tissue_heads", 2.0 * B * n_sel * C * F, 4.0 * (B * ns * d + T * C * (F + 1) + B * n_sel * (C + (argmax is not None))),
                          f"d={d} C={C} ns={ns} n_sel={n_sel}" + (" concat" if agg else "") + (" rows" if tissue_of_row is not None else ""),
                          family or _SCOPE))
    return out, argmax


def forest_predict(x: torch.Tensor, bank, *, model_of_row: torch.Tensor | None = None, model: int | None = None,
                   out: torch.Tensor, family: str = ""):
    """A bank of decision forests on fp32 rows (vf_forest_predict, include/vf_hip_forest.h).  x fp32 [R, >= F] row-strided;
    bank a forest.DeviceBank on x's device (forest.ForestBank.to).  Row form: model_of_row int32 [R] on the device, row r
    through the forest model_of_row[r].  Cohort form: model, a host int, every row through that forest.  out fp32 [R, >= K],
    row-strided; columns past K are left alone.  The caller owns every buffer and nothing is made here, as in tissue_heads.
    A host `model` outside the bank raises IndexError; a device id outside it is not read back: the kernel reads nothing for
    that row and writes NaN.  Returns out."""
    b = bank
    _dev(x, b.nodes, b.tree_root, b.leaf_values, b.base_scores, b.model_node_base, b.model_tree_base, b.model_leaf_base,
         b.model_n_trees, model_of_row, out)
    F, K, M = int(b.n_features), int(b.n_outputs), int(b.n_models)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] >= F
    R = x.shape[0]
    if (model_of_row is None) == (model is None):
        raise ValueError("forest_predict takes model_of_row (one forest per row) or model (one forest for every row): "
                         + ("not both" if model is not None else "one of them is required"))
    if model_of_row is not None:
        assert model_of_row.dtype == torch.int32 and model_of_row.is_contiguous() and tuple(model_of_row.shape) == (R,)
        mid = -1
    else:
        mid = int(model)
        if not 0 <= mid < M:
            raise IndexError(f"model {mid} is not one of the bank's {M}")
    assert out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] == R and out.shape[1] >= K
    assert b.nodes.dtype == torch.int32 and b.nodes.is_contiguous() and b.leaf_values.is_contiguous()
    post = {"identity": 0, "sigmoid": 1, "softmax": 2}[b.postprocessor]

    def launch():
        if R == 0:                                    # nothing to do (an empty tensor has no address to hand over)
            return
        check(_lib.load().vf_forest_predict(x.data_ptr(), x.stride(0), R, F, b.nodes.data_ptr(),
                                            b.tree_root.data_ptr(), b.leaf_values.data_ptr(), b.base_scores.data_ptr(),
                                            b.model_node_base.data_ptr(), b.model_tree_base.data_ptr(), b.model_leaf_base.data_ptr(),
                                            b.model_n_trees.data_ptr(), M, K, int(b.average), post, _ptr(model_of_row), mid,
                                            out.data_ptr(), out.stride(0), _stream()),
              "vf_forest_predict")
    # algorithmic bytes: the rows and the outputs once; the walks' node loads are gathers the caches serve (depth unknown here)
    _run(launch, lambda: ("forest_predict", 0.0, 4.0 * R * (F + K), f"F={F} K={K} M={M}" + (" rows" if model_of_row is not None else ""),
                          family or _SCOPE))
    return out


def topk_rows(x: torch.Tensor, k: int, *, row_len: torch.Tensor | None = None, values: torch.Tensor, indices: torch.Tensor,
              family: str = ""):
    """The k first-ranked values of every row and their columns (vf_topk_rows, include/vf_hip_topk.h).  x fp32 [R, n]
    row-strided, n <= 16384, k in 1 .. 64; row_len int32 [R] on the device (None: every row has n columns): columns at or past
    it are never read.  NaNs rank first, then descending by IEEE comparison; ties (+0 / -0, all NaNs) go to the lower column.
    values fp32 [R, >= k] and indices int32 [R, >= k], both row-strided with ONE row stride; columns past k are left alone;
    ranks a row has no column for are -1 / +0.0.  The caller owns every buffer and nothing is made here, as in forest_predict.
    Returns (values, indices)."""
    _dev(x, row_len, values, indices)
    k = int(k)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    R, n = x.shape
    assert row_len is None or (row_len.dtype == torch.int32 and row_len.is_contiguous() and tuple(row_len.shape) == (R,))
    assert values.dtype == torch.float32 and values.dim() == 2 and values.stride(1) == 1 and values.shape[0] == R and values.shape[1] >= k
    assert indices.dtype == torch.int32 and indices.dim() == 2 and indices.stride(1) == 1 and indices.shape[0] == R and indices.shape[1] >= k
    assert R <= 1 or values.stride(0) == indices.stride(0), "values and indices share one row stride"
    ldx = x.stride(0) if R > 1 else max(x.stride(0), n)
    ldo = values.stride(0) if R > 1 else max(values.stride(0), k)

    def launch():
        if R == 0:                                    # nothing to do (an empty tensor has no address to hand over)
            return
        # n == 0: every rank is padding, nothing is read, and an empty tensor has no address: `values` stands in for it
        check(_lib.load().vf_topk_rows(x.data_ptr() if n else values.data_ptr(), ldx, R, n, _ptr(row_len), k, values.data_ptr(),
                                       indices.data_ptr(), ldo, _stream()), "vf_topk_rows")
    # algorithmic bytes: the rows' valid values once and the outputs (the lengths live on the device: summed in summary())
    _run(launch, lambda: ("topk_rows", 0.0,
                          (lambda: 4.0 * (float(row_len.clamp(0, n).sum()) + 2.0 * R * k)) if row_len is not None else 4.0 * R * (n + 2 * k),
                          f"n={n} k={k}" + (" ragged" if row_len is not None else ""), family or _SCOPE))
    return values, indices


def _rows(t: torch.Tensor, width: int, name: str):
    """(row count, row stride in elements) of a row-strided fp32 / int32 matrix that holds at least `width` columns."""
    assert t.dim() == 2 and (t.stride(1) == 1 or t.shape[1] <= 1) and t.shape[1] >= width, f"{name}: a [rows, >= {width}] matrix with unit column stride"
    return t.shape[0], (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1], width, 1))


def rows_standardize(x: torch.Tensor, *, center: bool = True, z: torch.Tensor, norm: torch.Tensor | None = None, family: str = ""):
    """Rows to zero mean (center) and unit norm (vf_rows_standardize, include/vf_hip_neighbors.h): after it a dot product of two
    rows is their Pearson correlation (center=True) or cosine.  x fp32 [R, d] row-strided; z fp32 [R, d] row-strided (z may be
    x); norm None or fp32 [R] contiguous.  Two-pass fp32; a row with norm 0 becomes +0.0 with norm 0, a row with a NaN or an
    Inf becomes NaN with norm NaN.  The caller owns every buffer and nothing is made here.  Returns (z, norm)."""
    _dev(x, z, norm)
    assert x.dtype == torch.float32 and z.dtype == torch.float32 and x.dim() == 2 and x.shape[1] >= 1
    d = x.shape[1]
    R, ldx = _rows(x, d, "x")
    Rz, ldz = _rows(z, d, "z")
    assert Rz == R and z.shape[1] == d, "z has x's shape"
    assert norm is None or (norm.dtype == torch.float32 and norm.is_contiguous() and tuple(norm.shape) == (R,))

    def launch():
        if R == 0:
            return
        check(_lib.load().vf_rows_standardize(x.data_ptr(), ldx, R, d, int(bool(center)), z.data_ptr(), ldz, _ptr(norm), _stream()),
              "vf_rows_standardize")
    _run(launch, lambda: ("rows_standardize", 4.0 * R * d, 4.0 * R * (2 * d + 1), f"d={d}", family or _SCOPE))
    return z, norm


def knn_dot(q: torch.Tensor, y: torch.Tensor, k: int, *, self_offset: int = -1, values: torch.Tensor, indices: torch.Tensor,
            family: str = ""):
    """For every row of q the k rows of y with the largest dot product (vf_knn_dot, include/vf_hip_neighbors.h), formed tile by
    tile on the f32 MFMA: no [Rq, Ry] buffer exists.  q fp32 [Rq, d] and y fp32 [Ry, d] row-strided; self_offset -1, or the
    row of y at which q starts as a slice of it (row r then skips y[r + self_offset]).  The order is topk_rows's: NaN first,
    descending, ties to the lower row.  values fp32 [Rq, >= k] and indices int32 [Rq, >= k] with ONE row stride; columns past
    k are left alone; ranks a row has no candidate for are -1 / +0.0.  The caller owns every buffer.  Returns (values, indices)."""
    _dev(q, y, values, indices)
    k = int(k)
    assert q.dtype == torch.float32 and y.dtype == torch.float32 and q.dim() == 2 and y.dim() == 2 and q.shape[1] == y.shape[1] >= 1
    d = q.shape[1]
    Rq, ldq = _rows(q, d, "q")
    Ry, ldy = _rows(y, d, "y")
    assert values.dtype == torch.float32 and indices.dtype == torch.int32
    Rv, ldo = _rows(values, k, "values")
    Ri, ldi = _rows(indices, k, "indices")
    assert Rv == Ri == Rq and (Rq <= 1 or ldo == ldi), "values and indices have Rq rows and share one row stride"

    def launch():
        if Rq == 0:
            return
        # Ry == 0: every rank is padding, nothing is read, and an empty tensor has no address: `q` stands in for it
        check(_lib.load().vf_knn_dot(q.data_ptr(), ldq, Rq, y.data_ptr() if Ry else q.data_ptr(), ldy, Ry, d, int(self_offset), k,
                                     values.data_ptr(), indices.data_ptr(), ldo, _stream()), "vf_knn_dot")
    _run(launch, lambda: ("knn_dot", 2.0 * Rq * Ry * d, 4.0 * (Rq * d + Ry * d + 2 * Rq * k), f"Ry={Ry} d={d} k={k}", family or _SCOPE))
    return values, indices


def pairwise_dot(q: torch.Tensor, y: torch.Tensor, *, mode: int = 0, self_offset: int = -1, out: torch.Tensor, family: str = ""):
    """out[r, j] = the dot product of q[r] and y[j] (mode 0), bit for bit what knn_dot ranks, or 1 - it with exactly 0 at
    j == r + self_offset (mode 1: 1 - corrcoef with a zero diagonal, on standardised rows).  vf_pairwise_dot,
    include/vf_hip_neighbors.h.  q fp32 [Rq, d], y fp32 [Ry, d], out fp32 [Rq, Ry], all row-strided; the caller owns out."""
    _dev(q, y, out)
    assert q.dtype == torch.float32 and y.dtype == torch.float32 and q.dim() == 2 and y.dim() == 2 and q.shape[1] == y.shape[1] >= 1
    d = q.shape[1]
    Rq, ldq = _rows(q, d, "q")
    Ry, ldy = _rows(y, d, "y")
    assert out.dtype == torch.float32 and out.dim() == 2 and tuple(out.shape) == (Rq, Ry)
    ldo = _rows(out, Ry, "out")[1]

    def launch():
        if Rq == 0 or Ry == 0:
            return
        check(_lib.load().vf_pairwise_dot(q.data_ptr(), ldq, Rq, y.data_ptr(), ldy, Ry, d, int(self_offset), int(mode), out.data_ptr(),
                                          ldo, _stream()), "vf_pairwise_dot")
    _run(launch, lambda: ("pairwise_dot", 2.0 * Rq * Ry * d, 4.0 * (Rq * d + Ry * d + Rq * Ry), f"Ry={Ry} d={d} mode={int(mode)}", family or _SCOPE))
    return out


def _square(t: torch.Tensor, name: str):
    """(side, row stride in elements) of a row-strided fp32 square matrix."""
    assert t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] == t.shape[1], f"{name}: a square fp32 matrix"
    return _rows(t, t.shape[0], name)


def _vec(t: torch.Tensor, n: int, dtype, name: str):
    assert t.dtype == dtype and t.dim() == 1 and t.shape[0] == n and (n <= 1 or t.stride(0) == 1), f"{name}: a contiguous {dtype} [{n}]"


def linkage_nearest(D: torch.Tensor, *, nn_val: torch.Tensor, nn_idx: torch.Tensor, family: str = ""):
    """For every row i of the square matrix D its smallest D[i, j], j != i, and that j (vf_linkage_nearest,
    include/vf_hip_linkage.h).  D fp32 [m, m] row-strided, only read; nn_val fp32 [m] and nn_idx int32 [m] contiguous.  Ascending
    by IEEE comparison, NaN last (above +Inf), +0 and -0 tie, ties to the lower j; m == 1 gives -1 / +Inf.  The caller owns
    every buffer and nothing is made here.  Returns (nn_val, nn_idx)."""
    _dev(D, nn_val, nn_idx)
    m, ld = _square(D, "D")
    _vec(nn_val, m, torch.float32, "nn_val")
    _vec(nn_idx, m, torch.int32, "nn_idx")

    def launch():
        if m == 0:
            return
        check(_lib.load().vf_linkage_nearest(D.data_ptr(), ld, m, nn_val.data_ptr(), nn_idx.data_ptr(), _stream()), "vf_linkage_nearest")
    _run(launch, lambda: ("linkage_nearest", 0.0, 4.0 * (m * m + 2 * m), f"m={m}", family or _SCOPE))
    return nn_val, nn_idx


def linkage_contract(D: torch.Tensor, size: torch.Tensor, first: torch.Tensor, second: torch.Tensor, *, upper_only: bool = False,
                     out: torch.Tensor, size_out: torch.Tensor, pair_dist: torch.Tensor, family: str = ""):
    """One round of Ward merges (vf_linkage_contract, include/vf_hip_linkage.h): new cluster a is old cluster first[a] alone
    (second[a] == -1) or the merge of first[a] < second[a]; out [m_out, m_out] gets the Lance-Williams distances between the new
    clusters (symmetric bit for bit, diagonal +0), size_out [m_out] their sizes and pair_dist [m_out] each merged pair's own
    distance (+0 for a cluster that stands alone).  D fp32 [m, m] row-strided and size int32 [m] are only read; first and second
    int32 [m_out], first strictly increasing, constituents disjoint (not checked).  upper_only: read D's upper triangle alone
    (the first round, on the caller's matrix).  out must not overlap D.  The caller owns every buffer and nothing is made here.
    Returns (out, size_out, pair_dist)."""
    _dev(D, size, first, second, out, size_out, pair_dist)
    m, ld = _square(D, "D")
    m_out, ld_out = _square(out, "out")
    assert m_out <= m
    _vec(size, m, torch.int32, "size")
    _vec(first, m_out, torch.int32, "first")
    _vec(second, m_out, torch.int32, "second")
    _vec(size_out, m_out, torch.int32, "size_out")
    _vec(pair_dist, m_out, torch.float32, "pair_dist")

    def launch():
        if m_out == 0:
            return
        check(_lib.load().vf_linkage_contract(D.data_ptr(), ld, m, size.data_ptr(), first.data_ptr(), second.data_ptr(), m_out,
                                              out.data_ptr(), ld_out, size_out.data_ptr(), pair_dist.data_ptr(), int(bool(upper_only)),
                                              _stream()), "vf_linkage_contract")
    # algorithmic bytes: every old row once (it belongs to one new slot), the output, the per-slot vectors; operations: one
    # Lance-Williams update of about 12 per element (none where both slots stand alone, three where both are pairs)
    _run(launch, lambda: ("linkage_contract", 12.0 * m_out * m_out, 4.0 * (m * m + m_out * m_out + 6 * m_out), f"m={m} m_out={m_out}",
                          family or _SCOPE))
    return out, size_out, pair_dist


def umap_smooth_knn(idx: torch.Tensor, dist: torch.Tensor, mean_dist: float, *, rho: torch.Tensor, sigma: torch.Tensor,
                    strength: torch.Tensor, family: str = ""):
    """rho, sigma and the directed membership strengths of every row's neighbour list (vf_umap_smooth_knn,
    include/vf_hip_umap.h): umap-learn's smooth_knn_dist (local_connectivity 1) and compute_membership_strengths.  idx int32
    [R, m] and dist fp32 [R, m] row-strided, the others-only lists of neighbors.knn, only read; m in 1 .. 63; an entry with a
    negative index or a NaN / infinite distance is absent.  mean_dist: the mean of the present distances.  rho, sigma fp32 [R]
    contiguous; strength fp32 [R, m] row-strided.  The caller owns every buffer and nothing is made here.  Returns
    (rho, sigma, strength)."""
    _dev(idx, dist, rho, sigma, strength)
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and strength.dtype == torch.float32 and idx.dim() == 2
    m = idx.shape[1]
    assert 1 <= m <= 63, f"m={m} outside 1 .. 63"
    R, ld_idx = _rows(idx, m, "idx")
    assert dist.shape == idx.shape and strength.shape == idx.shape
    _, ld_dist = _rows(dist, m, "dist")
    _, ld_strength = _rows(strength, m, "strength")
    _vec(rho, R, torch.float32, "rho")
    _vec(sigma, R, torch.float32, "sigma")

    def launch():
        if R == 0:
            return
        check(_lib.load().vf_umap_smooth_knn(idx.data_ptr(), ld_idx, dist.data_ptr(), ld_dist, R, m, float(mean_dist), rho.data_ptr(),
                                             sigma.data_ptr(), strength.data_ptr(), ld_strength, _stream()), "vf_umap_smooth_knn")
    # operations: up to 64 bisection steps of one exp per entry; bytes: the two lists in, strengths and two vectors out
    _run(launch, lambda: ("umap_smooth_knn", 65.0 * 4 * R * m, 4.0 * (3 * R * m + 2 * R), f"R={R} m={m}", family or _SCOPE))
    return rho, sigma, strength


def umap_union(idx: torch.Tensor, strength: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor, *, w: torch.Tensor, family: str = ""):
    """The fuzzy union of the directed strengths over the symmetric graph (vf_umap_union, include/vf_hip_umap.h): for every CSR
    entry (i, j = col[e]) w[e] = (a + b) - a * b with a the strength of j in row i's list and b that of i in row j's, +0 where
    it is not listed; w[i -> j] and w[j -> i] have the same bits.  idx int32 [R, m] and strength fp32 [R, m] row-strided;
    rowptr int64 [R + 1], col int32 [nnz], w fp32 [nnz] contiguous.  The caller owns every buffer and nothing is made here.
    Returns w."""
    _dev(idx, strength, rowptr, col, w)
    assert idx.dtype == torch.int32 and strength.dtype == torch.float32 and idx.dim() == 2 and strength.shape == idx.shape
    m = idx.shape[1]
    assert 1 <= m <= 63, f"m={m} outside 1 .. 63"
    R, ld_idx = _rows(idx, m, "idx")
    _, ld_strength = _rows(strength, m, "strength")
    nnz = col.shape[0]
    _vec(rowptr, R + 1, torch.int64, "rowptr")
    _vec(col, nnz, torch.int32, "col")
    _vec(w, nnz, torch.float32, "w")

    def launch():
        if R == 0 or nnz == 0:
            return
        check(_lib.load().vf_umap_union(idx.data_ptr(), ld_idx, strength.data_ptr(), ld_strength, R, m, rowptr.data_ptr(),
                                        col.data_ptr(), nnz, w.data_ptr(), _stream()), "vf_umap_union")
    # bytes: per entry its column and weight, and two lists of m indices scanned (half of each on average)
    _run(launch, lambda: ("umap_union", 3.0 * nnz, 4.0 * nnz * (2 + m) + 8.0 * R, f"R={R} m={m} nnz={nnz}", family or _SCOPE))
    return w


def umap_layout(rowptr: torch.Tensor, col: torch.Tensor, samples: torch.Tensor, y0: torch.Tensor, y1: torch.Tensor, *, epoch_begin: int,
                epoch_end: int, n_epochs: int, a: float, b: float, gamma: float = 1.0, learning_rate: float = 1.0,
                negative_sample_rate: int = 5, seed: int = 42, family: str = ""):
    """The epochs [epoch_begin, epoch_end) of the UMAP layout (vf_umap_layout, include/vf_hip_umap.h), one kernel per epoch
    launched from a loop inside the library: epoch epoch_begin reads y0 and writes y1, the next the other way round.  rowptr
    int64 [R + 1], col int32 [nnz], samples int32 [nnz] contiguous, only read; y0, y1 fp32 [R, dim] row-strided with the same
    stride, dim in 1 .. 8.  Every vertex reads the others where they stood when the epoch began and writes its own row alone:
    no race, one result, and [0, 10) equals [0, 5) then [5, 10) bit for bit.  The caller owns every buffer and nothing is made
    here.  Returns the buffer that holds the result: y0 if epoch_end - epoch_begin is even, y1 if it is odd."""
    _dev(rowptr, col, samples, y0, y1)
    assert y0.dtype == torch.float32 and y1.dtype == torch.float32 and y0.dim() == 2 and y0.shape == y1.shape
    dim = y0.shape[1]
    assert 1 <= dim <= 8, f"dim={dim} outside 1 .. 8"
    R, ld = _rows(y0, dim, "y0")
    _, ld1 = _rows(y1, dim, "y1")
    assert ld == ld1, "y0 and y1 have one row stride"
    nnz = col.shape[0]
    _vec(rowptr, R + 1, torch.int64, "rowptr")
    _vec(col, nnz, torch.int32, "col")
    _vec(samples, nnz, torch.int32, "samples")
    epochs = int(epoch_end) - int(epoch_begin)

    def launch():
        if R == 0:
            return
        check(_lib.load().vf_umap_layout(rowptr.data_ptr(), col.data_ptr(), samples.data_ptr(), nnz, R, dim, y0.data_ptr(), y1.data_ptr(),
                                         ld, int(epoch_begin), int(epoch_end), int(n_epochs), float(a), float(b), float(gamma),
                                         float(learning_rate), int(negative_sample_rate), int(seed) & 0xFFFFFFFF, _stream()), "vf_umap_layout")
    # per epoch: every entry's sample count and column walked, every row read and written; force evaluations are counted by the
    # caller who knows the samples (scripts/umap_bench.py); here an upper figure of one per entry
    _run(launch, lambda: ("umap_layout", 40.0 * max(epochs, 0) * nnz, 4.0 * max(epochs, 0) * (2 * nnz + 2 * R * dim) + 8.0 * R,
                          f"R={R} dim={dim} nnz={nnz} epochs={epochs}", family or _SCOPE))
    return y0 if epochs % 2 == 0 else y1


TSNE_MAX_M, TSNE_MAX_DIM, TSNE_Z_BLOCKS = 255, 4, 64      # VF_TSNE_MAX_M, VF_TSNE_MAX_DIM, VF_TSNE_Z_BLOCKS


def tsne_work_bytes(R: int, dim: int, splits: int) -> int:
    """VF_TSNE_WORK_BYTES(R, dim, splits) of include/vf_hip_tsne.h: the bytes of tsne_descent's workspace."""
    return 8 * TSNE_Z_BLOCKS + 4 * (int(splits) * int(R) * (int(dim) + 1) + int(R) * int(dim))


def tsne_perplexity(idx: torch.Tensor, d2: torch.Tensor, perplexity: float, *, beta: torch.Tensor, p_cond: torch.Tensor, family: str = ""):
    """The conditional probabilities of every row's neighbour list at the given perplexity (vf_tsne_perplexity,
    include/vf_hip_tsne.h): scikit-learn's _binary_search_perplexity, the row's smallest squared distance subtracted before the
    exponential.  idx int32 [R, m] and d2 fp32 [R, m] (SQUARED distances) row-strided, only read; m in 1 .. 255; an entry with
    a negative index, a NaN / infinite distance or idx == the row is left out and gets +0.  1 <= perplexity < m.  beta fp32 [R]
    contiguous; p_cond fp32 [R, m] row-strided.  The caller owns every buffer and nothing is made here.  Returns (beta, p_cond)."""
    _dev(idx, d2, beta, p_cond)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and p_cond.dtype == torch.float32 and idx.dim() == 2
    m = idx.shape[1]
    assert 1 <= m <= TSNE_MAX_M, f"m={m} outside 1 .. {TSNE_MAX_M}"
    R, ld_idx = _rows(idx, m, "idx")
    assert d2.shape == idx.shape and p_cond.shape == idx.shape
    _, ld_d2 = _rows(d2, m, "d2")
    _, ld_p = _rows(p_cond, m, "p_cond")
    _vec(beta, R, torch.float32, "beta")

    def launch():
        if R == 0:
            return
        check(_lib.load().vf_tsne_perplexity(idx.data_ptr(), ld_idx, d2.data_ptr(), ld_d2, R, m, float(perplexity), beta.data_ptr(),
                                             p_cond.data_ptr(), ld_p, _stream()), "vf_tsne_perplexity")
    # operations: up to 100 search steps of one exp, one division and a few more per entry; bytes: the two lists in, P and beta out
    _run(launch, lambda: ("tsne_perplexity", 100.0 * 8 * R * m, 4.0 * (3 * R * m + R), f"R={R} m={m}", family or _SCOPE))
    return beta, p_cond


def tsne_joint(idx: torch.Tensor, p_cond: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor, *, p: torch.Tensor, family: str = ""):
    """The symmetric sum of the conditional probabilities over the symmetric graph (vf_tsne_joint, include/vf_hip_tsne.h): for
    every CSR entry (i, j = col[e]) p[e] = a + b with a the p_cond of j in row i's list and b that of i in row j's, +0 where it
    is not listed; p[i -> j] and p[j -> i] have the same bits.  Not normalised.  idx int32 [R, m] and p_cond fp32 [R, m]
    row-strided; rowptr int64 [R + 1], col int32 [nnz], p fp32 [nnz] contiguous.  The caller owns every buffer and nothing is
    made here.  Returns p."""
    _dev(idx, p_cond, rowptr, col, p)
    assert idx.dtype == torch.int32 and p_cond.dtype == torch.float32 and idx.dim() == 2 and p_cond.shape == idx.shape
    m = idx.shape[1]
    assert 1 <= m <= TSNE_MAX_M, f"m={m} outside 1 .. {TSNE_MAX_M}"
    R, ld_idx = _rows(idx, m, "idx")
    _, ld_p = _rows(p_cond, m, "p_cond")
    nnz = col.shape[0]
    _vec(rowptr, R + 1, torch.int64, "rowptr")
    _vec(col, nnz, torch.int32, "col")
    _vec(p, nnz, torch.float32, "p")

    def launch():
        if R == 0 or nnz == 0:
            return
        check(_lib.load().vf_tsne_joint(idx.data_ptr(), ld_idx, p_cond.data_ptr(), ld_p, R, m, rowptr.data_ptr(), col.data_ptr(), nnz,
                                        p.data_ptr(), _stream()), "vf_tsne_joint")
    _run(launch, lambda: ("tsne_joint", 1.0 * nnz, 4.0 * nnz * (2 + m) + 8.0 * R, f"R={R} m={m} nnz={nnz}", family or _SCOPE))
    return p


def tsne_repulsion(y: torch.Tensor, *, dof: int, splits: int, part: torch.Tensor, family: str = ""):
    """One all-pairs pass of t-SNE's repulsive force (vf_tsne_repulsion, include/vf_hip_tsne.h).  y fp32 [R, dim] row-strided,
    dim in 1 .. 4, only read; dof in 1 .. 3; part fp32 [splits, R, dim + 1] contiguous: for vertex i and split s, over the rows
    j != i of the split's contiguous range in ascending order, columns 0 .. dim - 1 get sum w w (y_i - y_j) and column dim
    gets sum w, w = (1 + d2 / dof)^-((dof + 1) / 2).  No atomic: one result, bit for bit.  The caller owns every buffer and
    nothing is made here.  Returns part."""
    _dev(y, part)
    assert y.dtype == torch.float32 and y.dim() == 2 and part.dtype == torch.float32
    dim = y.shape[1]
    assert 1 <= dim <= TSNE_MAX_DIM, f"dim={dim} outside 1 .. {TSNE_MAX_DIM}"
    R, ld = _rows(y, dim, "y")
    splits = int(splits)
    assert part.dim() == 3 and tuple(part.shape) == (splits, R, dim + 1) and (part.numel() == 0 or part.is_contiguous()), \
        f"part: a contiguous fp32 [{splits}, {R}, {dim + 1}]"

    def launch():
        if R == 0:
            return
        check(_lib.load().vf_tsne_repulsion(y.data_ptr(), ld, R, dim, int(dof), splits, part.data_ptr(), _stream()), "vf_tsne_repulsion")
    # per pair: the differences, d2, one reciprocal, the weight and dim + 1 accumulations
    _run(launch, lambda: ("tsne_repulsion", (5.0 * dim + 6) * R * R, 4.0 * (R * dim + splits * R * (dim + 1)),
                          f"R={R} dim={dim} dof={int(dof)} splits={splits}", family or _SCOPE))
    return part


def tsne_descent(rowptr: torch.Tensor, col: torch.Tensor, p: torch.Tensor, y: torch.Tensor, update: torch.Tensor, gains: torch.Tensor, *,
                 iter_begin: int, iter_end: int, exaggeration: float, momentum: float, learning_rate: float, min_gain: float = 0.01,
                 dof: int, splits: int, work: torch.Tensor, zsum: torch.Tensor, family: str = ""):
    """The iterations [iter_begin, iter_end) of t-SNE's gradient descent with the exact gradient (vf_tsne_descent,
    include/vf_hip_tsne.h), from one loop inside the library: scikit-learn's _gradient_descent over its _kl_divergence.  rowptr
    int64 [R + 1], col int32 [nnz], p fp32 [nnz] (normalised) contiguous, only read; y, update, gains fp32 [R, dim] row-strided
    with one stride, the state, written in place; work a contiguous uint8 / any-dtype tensor of at least
    tsne_work_bytes(R, dim, splits) bytes; zsum fp64 [iter_end - iter_begin], each iteration's Z.  One result, bit for bit, and
    [0, 20) equals [0, 7) then [7, 20) on the carried state.  The caller owns every buffer and nothing is made here.  Returns
    (y, update, gains, zsum)."""
    _dev(rowptr, col, p, y, update, gains, work, zsum)
    assert y.dtype == torch.float32 and y.dim() == 2 and update.dtype == torch.float32 and gains.dtype == torch.float32
    assert update.shape == y.shape and gains.shape == y.shape
    dim = y.shape[1]
    assert 1 <= dim <= TSNE_MAX_DIM, f"dim={dim} outside 1 .. {TSNE_MAX_DIM}"
    R, ld = _rows(y, dim, "y")
    assert _rows(update, dim, "update")[1] == ld and _rows(gains, dim, "gains")[1] == ld, "y, update and gains have one row stride"
    nnz = col.shape[0]
    _vec(rowptr, R + 1, torch.int64, "rowptr")
    _vec(col, nnz, torch.int32, "col")
    _vec(p, nnz, torch.float32, "p")
    iters = int(iter_end) - int(iter_begin)
    _vec(zsum, max(iters, 0), torch.float64, "zsum")
    splits = int(splits)
    assert work.is_contiguous(), "work: a contiguous buffer"
    work_bytes = work.numel() * work.element_size()

    def launch():
        if R == 0:
            return
        check(_lib.load().vf_tsne_descent(rowptr.data_ptr(), _ptr(col) if nnz else 0, _ptr(p) if nnz else 0, nnz, R, dim, y.data_ptr(),
                                          update.data_ptr(), gains.data_ptr(), ld, int(iter_begin), int(iter_end), float(exaggeration),
                                          float(momentum), float(learning_rate), float(min_gain), int(dof), splits, work.data_ptr(),
                                          work_bytes, zsum.data_ptr() if iters > 0 else 0, _stream()), "vf_tsne_descent")
    _run(launch, lambda: ("tsne_descent", max(iters, 0) * ((5.0 * dim + 6) * R * R + (5.0 * dim + 6) * nnz),
                          4.0 * max(iters, 0) * (2 * nnz + 2 * splits * R * (dim + 1) + 8 * R * dim),
                          f"R={R} dim={dim} nnz={nnz} dof={int(dof)} splits={splits} iters={iters}", family or _SCOPE))
    return y, update, gains, zsum


ENRICH_MAX_K, ENRICH_MAX_N = 4096, 1 << 24                # VF_ENRICH_MAX_K, VF_ENRICH_MAX_N


def enrich_counts(termptr: torch.Tensor, gene: torch.Tensor, labels: torch.Tensor, k: int, *, count: torch.Tensor, size: torch.Tensor,
                  family: str = ""):
    """The overlap of every annotation term with every cluster (vf_enrich_counts, include/vf_hip_enrich.h).  termptr int64
    [T + 1] and gene int32 [nnz]: the term-major CSR annotation, universe rows; an entry outside [0, G) is skipped.  labels int32
    [G]: 0 .. k - 1 names a cluster, any other value no cluster.  count int32 [T, k] row-strided: count[t, c] = the entries of
    term t whose gene has label c; size int32 [T]: the entries of term t inside the universe.  Integers: exact, whatever the
    order.  The cluster sizes are this call with the one term that lists every gene.  The caller owns every buffer and nothing
    is made here.  Returns (count, size)."""
    _dev(termptr, gene, labels, count, size)
    k = int(k)
    assert 1 <= k <= ENRICH_MAX_K, f"k={k} outside 1 .. {ENRICH_MAX_K}"
    assert count.dtype == torch.int32 and count.dim() == 2 and count.shape[1] == k
    T, ldc = _rows(count, k, "count")
    nnz, G = gene.shape[0], labels.shape[0]
    _vec(termptr, T + 1, torch.int64, "termptr")
    _vec(gene, nnz, torch.int32, "gene")
    _vec(labels, G, torch.int32, "labels")
    _vec(size, T, torch.int32, "size")

    def launch():
        if T == 0:
            return
        # G == 0: nothing reads labels, and an empty tensor has no address: `termptr` stands in for it
        check(_lib.load().vf_enrich_counts(termptr.data_ptr(), _ptr(gene) if nnz else 0, nnz, T, labels.data_ptr() if G else termptr.data_ptr(),
                                           G, k, count.data_ptr(), ldc, size.data_ptr(), _stream()), "vf_enrich_counts")
    _run(launch, lambda: ("enrich_counts", 0.0, 4.0 * (2 * nnz + T * (k + 1)) + 8.0 * T, f"T={T} k={k} nnz={nnz} G={G}", family or _SCOPE))
    return count, size


def hypergeom_tail(count: torch.Tensor, size: torch.Tensor, csize: torch.Tensor, N: int, logfact: torch.Tensor, alternative: int, *,
                   log_p: torch.Tensor, tail: torch.Tensor, steps: torch.Tensor, family: str = ""):
    """The hypergeometric tail of every (term, cluster) cell (vf_hypergeom_tail, include/vf_hip_enrich.h): for x = count[t, c],
    K = size[t], n = csize[c] and the universe N, log P[X >= x] (alternative 0: scipy's hypergeom.sf(x - 1, N, K, n)) or
    log P[X <= x] (alternative 1: hypergeom.cdf).  count int32 [T, k] row-strided, size int32 [T], csize int32 [k]; logfact fp64
    [N + 1] = lgamma(i + 1), from the host.  log_p and tail fp64 [T, k], steps int32 [T, k], row-strided with ONE stride: the
    natural log of the tail, the sum behind it and the number of terms it added.  One thread per cell, a sum that runs away
    from the mode: one result, bit for bit.  The caller owns every buffer and nothing is made here.  Returns (log_p, tail, steps)."""
    _dev(count, size, csize, logfact, log_p, tail, steps)
    assert count.dtype == torch.int32 and count.dim() == 2
    k, N = count.shape[1], int(N)
    assert 1 <= k <= ENRICH_MAX_K, f"k={k} outside 1 .. {ENRICH_MAX_K}"
    assert 0 <= N <= ENRICH_MAX_N, f"N={N} outside 0 .. 2^24"
    T, ldc = _rows(count, k, "count")
    _vec(size, T, torch.int32, "size")
    _vec(csize, k, torch.int32, "csize")
    _vec(logfact, N + 1, torch.float64, "logfact")
    assert log_p.dtype == torch.float64 and tail.dtype == torch.float64 and steps.dtype == torch.int32
    assert tuple(log_p.shape) == tuple(tail.shape) == tuple(steps.shape) == (T, k)
    ldo = _rows(log_p, k, "log_p")[1]
    assert T <= 1 or (_rows(tail, k, "tail")[1] == ldo and _rows(steps, k, "steps")[1] == ldo), "log_p, tail and steps share one row stride"

    def launch():
        if T == 0:
            return
        check(_lib.load().vf_hypergeom_tail(count.data_ptr(), ldc, size.data_ptr(), csize.data_ptr(), T, k, N, logfact.data_ptr(),
                                            int(alternative), log_p.data_ptr(), tail.data_ptr(), steps.data_ptr(), ldo, _stream()),
              "vf_hypergeom_tail")
    # operations: a few hundred fp64 + * / per cell is typical, the count depends on the cell; bytes: the three outputs and the counts
    _run(launch, lambda: ("hypergeom_tail", 300.0 * T * k, 24.0 * T * k + 4.0 * (T + k) + 8.0 * (N + 1), f"T={T} k={k} N={N} alternative={int(alternative)}",
                          family or _SCOPE))
    return log_p, tail, steps


# include/vf_hip_kmeans.h: VF_KMEANS_MAX_K, _MAX_R, _MAX_D, _ROWS, _UPDATE_COLS, _RED_THREADS
KMEANS_MAX_K, KMEANS_MAX_R, KMEANS_MAX_D, KMEANS_ROWS, KMEANS_UPDATE_COLS, KMEANS_RED_THREADS = 4096, 1 << 24, 65536, 64, 64, 256


def kmeans_lloyd_work_bytes(R: int, d: int, k: int) -> int:
    """VF_KMEANS_LLOYD_WORK_BYTES(R, d, k)."""
    return 8 + 8 * k * ((d + KMEANS_UPDATE_COLS - 1) // KMEANS_UPDATE_COLS) + 4 * ((R + KMEANS_ROWS - 1) // KMEANS_ROWS)


def kmeans_seed_work_bytes(R: int) -> int:
    """VF_KMEANS_SEED_WORK_BYTES(R)."""
    return 16 + 12 * ((R + KMEANS_RED_THREADS - 1) // KMEANS_RED_THREADS)


def _kmeans_operands(x: torch.Tensor, cen: torch.Tensor, name: str = "cen"):
    assert x.dtype == torch.float32 and cen.dtype == torch.float32 and x.dim() == 2 and cen.dim() == 2 and x.shape[1] == cen.shape[1]
    d = x.shape[1]
    assert 1 <= d <= KMEANS_MAX_D, f"d={d} outside 1 .. {KMEANS_MAX_D}"
    R, ldx = _rows(x, d, "x")
    k, ldc = _rows(cen, d, name)
    assert 1 <= k <= KMEANS_MAX_K, f"k={k} outside 1 .. {KMEANS_MAX_K}"
    assert R <= KMEANS_MAX_R, f"R={R} is above 2^24"
    return R, d, ldx, k, ldc


def kmeans_assign(x: torch.Tensor, cen: torch.Tensor, *, labels: torch.Tensor, dist: torch.Tensor, family: str = ""):
    """The nearest centre of every row (vf_kmeans_assign, include/vf_hip_kmeans.h).  x fp32 [R, d] and cen fp32 [k, d] row-strided,
    only read; labels int32 [R] and dist fp32 [R] contiguous.  The squared distance is a running fp32 sum of (x - c)^2 over the
    columns in ascending order, every operation rounded once, no fma; the smallest wins, ties to the lower centre, a NaN never;
    a row with no winner has label -1 and dist NaN.  The caller owns every buffer and nothing is made here.  Returns
    (labels, dist)."""
    _dev(x, cen, labels, dist)
    R, d, ldx, k, ldc = _kmeans_operands(x, cen)
    _vec(labels, R, torch.int32, "labels")
    _vec(dist, R, torch.float32, "dist")

    def launch():
        if R == 0:
            return
        check(_lib.load().vf_kmeans_assign(x.data_ptr(), ldx, R, d, cen.data_ptr(), ldc, k, labels.data_ptr(), dist.data_ptr(), _stream()),
              "vf_kmeans_assign")
    _run(launch, lambda: ("kmeans_assign", 3.0 * R * k * d, 4.0 * (R * d + k * d + 2 * R), f"R={R} d={d} k={k}", family or _SCOPE))
    return labels, dist


def kmeans_update(x: torch.Tensor, labels: torch.Tensor, cen_old: torch.Tensor, *, cen_new: torch.Tensor, counts: torch.Tensor,
                  family: str = ""):
    """The fp64 mean of every cluster's rows (vf_kmeans_update, include/vf_hip_kmeans.h).  x fp32 [R, d] row-strided and labels int32
    [R], only read (a label outside 0 .. k - 1 belongs to no centre); cen_old fp32 [k, d] row-strided; cen_new fp32 [k, d]
    row-strided, which may be cen_old itself; counts int32 [k].  The sums run over VF_KMEANS_UPDATE_WAVES contiguous row ranges
    in ascending row order and are added in range order; a centre without members keeps cen_old's bits.  No atomic: one result,
    bit for bit.  The caller owns every buffer and nothing is made here.  Returns (cen_new, counts)."""
    _dev(x, labels, cen_old, cen_new, counts)
    R, d, ldx, k, ldc = _kmeans_operands(x, cen_old, "cen_old")
    assert cen_new.dtype == torch.float32 and cen_new.dim() == 2 and tuple(cen_new.shape) == (k, d)
    ldn = _rows(cen_new, d, "cen_new")[1]
    _vec(labels, R, torch.int32, "labels")
    _vec(counts, k, torch.int32, "counts")

    def launch():
        # R == 0: nothing reads x or labels, and an empty tensor has no address: `cen_old` stands in for them
        check(_lib.load().vf_kmeans_update(x.data_ptr() if R else cen_old.data_ptr(), ldx, R, d, labels.data_ptr() if R else cen_old.data_ptr(),
                                           cen_old.data_ptr(), ldc, k, cen_new.data_ptr(), ldn, counts.data_ptr(), _stream()), "vf_kmeans_update")
    _run(launch, lambda: ("kmeans_update", 1.0 * R * d, 4.0 * (R * d + R * k * ((d + 63) // 64) + 2 * k * d + k), f"R={R} d={d} k={k}",
                          family or _SCOPE))
    return cen_new, counts


def kmeans_lloyd(x: torch.Tensor, cen: torch.Tensor, *, max_iter: int, tol_abs: float, resume: bool = False, labels: torch.Tensor,
                 dist: torch.Tensor, prev_labels: torch.Tensor, counts: torch.Tensor, n_iter: torch.Tensor, shift: torch.Tensor,
                 changed: torch.Tensor, work: torch.Tensor, family: str = ""):
    """Up to max_iter iterations of Lloyd's loop and a last assignment (vf_kmeans_lloyd, include/vf_hip_kmeans.h), from one loop inside
    the library with the stop decided on the device: scikit-learn's _kmeans_single_lloyd.  x fp32 [R, d] row-strided, only read;
    cen fp32 [k, d] row-strided: in, the start; out, the result.  labels int32 [R] and dist fp32 [R]: the last assignment;
    prev_labels int32 [R]: the labels of the last iteration that ran (read with resume=True); counts int32 [k]; n_iter int32 [1];
    shift fp64 [max_iter] and changed int64 [max_iter], written up to n_iter alone; work a contiguous buffer of at least
    kmeans_lloyd_work_bytes(R, d, k) bytes.  An iteration stops the loop when no label changed (not the first of a fresh run) or
    when the summed squared shift of the centres is <= tol_abs.  One result, bit for bit; a then b iterations on the carried
    state equal a + b.  The caller owns every buffer and nothing is made here.  Returns (cen, labels, dist, n_iter)."""
    _dev(x, cen, labels, dist, prev_labels, counts, n_iter, shift, changed, work)
    R, d, ldx, k, ldc = _kmeans_operands(x, cen)
    max_iter = int(max_iter)
    assert max_iter >= 0, f"max_iter={max_iter} must not be negative"
    _vec(labels, R, torch.int32, "labels")
    _vec(dist, R, torch.float32, "dist")
    _vec(prev_labels, R, torch.int32, "prev_labels")
    _vec(counts, k, torch.int32, "counts")
    _vec(n_iter, 1, torch.int32, "n_iter")
    _vec(shift, max_iter, torch.float64, "shift")
    _vec(changed, max_iter, torch.int64, "changed")
    assert work.is_contiguous(), "work: a contiguous buffer"
    work_bytes = work.numel() * work.element_size()

    def launch():
        if R == 0:
            return
        check(_lib.load().vf_kmeans_lloyd(x.data_ptr(), ldx, R, d, cen.data_ptr(), ldc, k, max_iter, float(tol_abs), int(bool(resume)),
                                          labels.data_ptr(), dist.data_ptr(), prev_labels.data_ptr(), counts.data_ptr(), n_iter.data_ptr(),
                                          shift.data_ptr() if max_iter else 0, changed.data_ptr() if max_iter else 0, work.data_ptr(),
                                          work_bytes, _stream()), "vf_kmeans_lloyd")
    _run(launch, lambda: ("kmeans_lloyd", 3.0 * R * k * d * (max_iter + 1), 4.0 * (max_iter + 1) * (R * d + k * d + 2 * R),
                          f"R={R} d={d} k={k} max_iter={max_iter}", family or _SCOPE))
    return cen, labels, dist, n_iter


def kmeans_seed(x: torch.Tensor, k: int, seed: int, *, rows: torch.Tensor, cen: torch.Tensor, mind: torch.Tensor, work: torch.Tensor,
                family: str = ""):
    """Plain D^2 seeding (vf_kmeans_seed, include/vf_hip_kmeans.h): k rows of x, each drawn with probability proportional to its
    squared distance to the nearest row drawn before, in exact integer arithmetic from a counter hash of (seed, step).  x fp32
    [R, d] row-strided, only read; rows int32 [k]: the chosen rows; cen fp32 [k, d] row-strided: copies of them; mind fp32 [R];
    work a contiguous buffer of at least kmeans_seed_work_bytes(R) bytes.  One result, bit for bit, which numpy restates
    (tests/kmeans_cases.py).  The caller owns every buffer and nothing is made here.  Returns (rows, cen)."""
    _dev(x, rows, cen, mind, work)
    R, d, ldx, kc, ldc = _kmeans_operands(x, cen)
    k = int(k)
    assert kc == k and 1 <= k <= R, f"k={k}: cen has {kc} rows, x has {R}"
    _vec(rows, k, torch.int32, "rows")
    _vec(mind, R, torch.float32, "mind")
    assert work.is_contiguous(), "work: a contiguous buffer"
    work_bytes = work.numel() * work.element_size()

    def launch():
        check(_lib.load().vf_kmeans_seed(x.data_ptr(), ldx, R, d, k, int(seed), rows.data_ptr(), cen.data_ptr(), ldc, mind.data_ptr(),
                                         work.data_ptr(), work_bytes, _stream()), "vf_kmeans_seed")
    _run(launch, lambda: ("kmeans_seed", 3.0 * R * d * k, 4.0 * k * (R * d + 3 * R), f"R={R} d={d} k={k}", family or _SCOPE))
    return rows, cen


# include/vf_hip_silhouette.h: VF_SILHOUETTE_MAX_K, _MAX_R, _MAX_D (k-means'), _RANGES
SILHOUETTE_MAX_K, SILHOUETTE_MAX_R, SILHOUETTE_MAX_D, SILHOUETTE_RANGES = KMEANS_MAX_K, KMEANS_MAX_R, KMEANS_MAX_D, 4


def silhouette_dot_work_bytes(d: int, k: int) -> int:
    """VF_SILHOUETTE_DOT_WORK_BYTES(d, k)."""
    return 8 * k * d


def _silhouette_operands(x, order, seg, S, row0, rows):
    assert x.dtype == torch.float32 and x.dim() == 2
    d = x.shape[1]
    assert 1 <= d <= SILHOUETTE_MAX_D, f"d={d} outside 1 .. {SILHOUETTE_MAX_D}"
    R, ldx = _rows(x, d, "x")
    assert R <= SILHOUETTE_MAX_R, f"R={R} is above 2^24"
    assert seg.dtype == torch.int64 and seg.dim() == 1 and seg.shape[0] >= 2 and seg.is_contiguous(), "seg: a contiguous int64 [k + 1]"
    k = seg.shape[0] - 1
    assert k <= SILHOUETTE_MAX_K, f"k={k} outside 1 .. {SILHOUETTE_MAX_K}"
    n = order.shape[0]
    _vec(order, n, torch.int32, "order")
    assert n <= R, f"order has {n} rows, x has {R}"
    row0, rows = int(row0), int(rows)
    assert 0 <= row0 and 0 <= rows and row0 + rows <= R, f"rows [{row0}, {row0 + rows}) outside 0 .. {R}"
    assert S.dtype == torch.float64 and S.dim() == 2 and tuple(S.shape) == (k, rows), f"S: an fp64 [{k}, {rows}]"
    lds = _rows(S, rows, "S")[1]
    return R, d, ldx, n, k, row0, rows, lds


def silhouette_sums_l2(x: torch.Tensor, order: torch.Tensor, seg: torch.Tensor, row0: int, rows: int, *, S: torch.Tensor, family: str = ""):
    """Every query row's summed Euclidean distance to the members of every cluster, by all pairs (vf_silhouette_sums_l2,
    include/vf_hip_silhouette.h).  x fp32 [R, d] row-strided, only read; order int32 [n] and seg int64 [k + 1]: the clusters as a CSR of
    rows (the rows with a label, sorted by label and ascending within one; the offsets); the query rows are [row0, row0 + rows);
    S fp64 [k, rows] row-strided: S[c, i - row0].  The squared distance is k-means' fp32 chain, then a correctly rounded square
    root and an fp64 sum over the members in VF_SILHOUETTE_RANGES contiguous ranges: one result, bit for bit, the same for any row
    range.  The caller owns every buffer and nothing is made here.  Returns S."""
    _dev(x, order, seg, S)
    R, d, ldx, n, k, row0, rows, lds = _silhouette_operands(x, order, seg, S, row0, rows)

    def launch():
        if rows == 0:
            return
        check(_lib.load().vf_silhouette_sums_l2(x.data_ptr(), ldx, R, d, order.data_ptr(), n, seg.data_ptr(), k, row0, rows, S.data_ptr(), lds,
                                                _stream()), "vf_silhouette_sums_l2")
    _run(launch, lambda: ("silhouette_sums_l2", (3.0 * d + 3.0) * rows * n, 4.0 * (rows * d + n * d + n) + 8.0 * rows * k,
                          f"R={R} d={d} k={k} rows={rows}", family or _SCOPE))
    return S


def silhouette_sums_dot(z: torch.Tensor, order: torch.Tensor, seg: torch.Tensor, labels: torch.Tensor, row0: int, rows: int, *,
                        S: torch.Tensor, work: torch.Tensor, family: str = ""):
    """Every query row's summed distance 1 - z_i . z_j to the members of every cluster other than itself, from the clusters' fp64
    column sums (vf_silhouette_sums_dot, include/vf_hip_silhouette.h): linear in the rows.  z fp32 [R, d] row-strided: standardised
    rows, only read; order, seg as in silhouette_sums_l2; labels int32 [R] (a value outside 0 .. k - 1: no label); S fp64 [k, rows]
    row-strided; work a contiguous buffer of at least silhouette_dot_work_bytes(d, k) bytes, which afterwards holds the column
    sums.  Two launches; every sum in a stated order: one result, bit for bit.  The caller owns every buffer and
    nothing is made here.  Returns S."""
    _dev(z, order, seg, labels, S, work)
    R, d, ldz, n, k, row0, rows, lds = _silhouette_operands(z, order, seg, S, row0, rows)
    _vec(labels, R, torch.int32, "labels")
    assert work.is_contiguous(), "work: a contiguous buffer"
    work_bytes = work.numel() * work.element_size()

    def launch():
        if rows == 0:
            return
        check(_lib.load().vf_silhouette_sums_dot(z.data_ptr(), ldz, R, d, order.data_ptr(), n, seg.data_ptr(), k, labels.data_ptr(), row0, rows,
                                                 S.data_ptr(), lds, work.data_ptr(), work_bytes, _stream()), "vf_silhouette_sums_dot")
    _run(launch, lambda: ("silhouette_sums_dot", 2.0 * rows * k * d + 1.0 * n * d, 4.0 * (rows * d + n * d) + 8.0 * (k * d + rows * k),
                          f"R={R} d={d} k={k} rows={rows}", family or _SCOPE))
    return S


def silhouette_finish(S: torch.Tensor, labels: torch.Tensor, seg: torch.Tensor, row0: int, rows: int, *, a: torch.Tensor, b: torch.Tensor,
                      s: torch.Tensor, nearest: torch.Tensor, family: str = ""):
    """From the sums to the silhouette of the rows [row0, row0 + rows) (vf_silhouette_finish, include/vf_hip_silhouette.h).  S fp64
    [k, rows] row-strided: what either sums entry wrote for the same range; labels int32 [R]; seg int64 [k + 1]; a, b, s fp64 [R]
    and nearest int32 [R], written at the range alone: the mean distance to the own cluster's other members, the smallest mean to
    another non-empty cluster (ties to the lower one, a NaN never), (b - a) / max(a, b), and that cluster.  The caller owns
    every buffer and nothing is made here.  Returns (a, b, s, nearest)."""
    _dev(S, labels, seg, a, b, s, nearest)
    assert seg.dtype == torch.int64 and seg.dim() == 1 and seg.shape[0] >= 2 and seg.is_contiguous(), "seg: a contiguous int64 [k + 1]"
    k, R = seg.shape[0] - 1, labels.shape[0]
    assert k <= SILHOUETTE_MAX_K, f"k={k} outside 1 .. {SILHOUETTE_MAX_K}"
    assert R <= SILHOUETTE_MAX_R, f"R={R} is above 2^24"
    row0, rows = int(row0), int(rows)
    assert 0 <= row0 and 0 <= rows and row0 + rows <= R, f"rows [{row0}, {row0 + rows}) outside 0 .. {R}"
    assert S.dtype == torch.float64 and S.dim() == 2 and tuple(S.shape) == (k, rows), f"S: an fp64 [{k}, {rows}]"
    lds = _rows(S, rows, "S")[1]
    _vec(labels, R, torch.int32, "labels")
    for t, name in ((a, "a"), (b, "b"), (s, "s")):
        _vec(t, R, torch.float64, name)
    _vec(nearest, R, torch.int32, "nearest")

    def launch():
        if rows == 0:
            return
        check(_lib.load().vf_silhouette_finish(S.data_ptr(), lds, labels.data_ptr(), R, seg.data_ptr(), k, row0, rows, a.data_ptr(), b.data_ptr(),
                                               s.data_ptr(), nearest.data_ptr(), _stream()), "vf_silhouette_finish")
    _run(launch, lambda: ("silhouette_finish", 2.0 * rows * k, 8.0 * rows * k + 32.0 * rows, f"R={R} k={k} rows={rows}", family or _SCOPE))
    return a, b, s, nearest


def umap_smooth_knn_query(idx: torch.Tensor, dist: torch.Tensor, mean_dist: float, *, sigma: torch.Tensor, strength: torch.Tensor,
                          family: str = ""):
    """sigma and the directed membership strengths of every QUERY's list of training neighbours (vf_umap_smooth_knn_query,
    include/vf_hip_umap_transform.h): umap-learn's smooth_knn_dist with local_connectivity - 1 = 0 (rho = +0) and its bipartite
    compute_membership_strengths.  idx int32 [Rq, m] and dist fp32 [Rq, m] row-strided, what neighbors.knn(x, m, queries=q)
    returned, only read; m in 1 .. 64; an entry with a negative index or a NaN / infinite distance is absent; an index equal to
    the row's own number is a training row like any other.  mean_dist: the FIT's mean distance.  sigma fp32 [Rq] contiguous;
    strength fp32 [Rq, m] row-strided.  The caller owns every buffer and nothing is made here.  Returns (sigma, strength)."""
    _dev(idx, dist, sigma, strength)
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and strength.dtype == torch.float32 and idx.dim() == 2
    m = idx.shape[1]
    assert 1 <= m <= 64, f"m={m} outside 1 .. 64"
    Rq, ld_idx = _rows(idx, m, "idx")
    assert dist.shape == idx.shape and strength.shape == idx.shape
    _, ld_dist = _rows(dist, m, "dist")
    _, ld_strength = _rows(strength, m, "strength")
    _vec(sigma, Rq, torch.float32, "sigma")

    def launch():
        if Rq == 0:
            return
        check(_lib.load().vf_umap_smooth_knn_query(idx.data_ptr(), ld_idx, dist.data_ptr(), ld_dist, Rq, m, float(mean_dist),
                                                   sigma.data_ptr(), strength.data_ptr(), ld_strength, _stream()), "vf_umap_smooth_knn_query")
    # operations: up to 64 bisection steps of one exp per entry; bytes: the two lists in, strengths and one vector out
    _run(launch, lambda: ("umap_smooth_knn_query", 65.0 * 4 * Rq * m, 4.0 * (3 * Rq * m + Rq), f"Rq={Rq} m={m}", family or _SCOPE))
    return sigma, strength


def umap_init_transform(idx: torch.Tensor, strength: torch.Tensor, y: torch.Tensor, *, out: torch.Tensor, family: str = ""):
    """The start of every query: the mean of its training neighbours' positions weighted by strength / (the row's sum of
    strengths) (vf_umap_init_transform, include/vf_hip_umap_transform.h), in fp32 with every operation rounded once and the sums
    ascending.  idx int32 [Rq, m] and strength fp32 [Rq, m] row-strided; y fp32 [R, dim] row-strided, the fitted embedding, only
    read; out fp32 [Rq, dim] row-strided; m in 1 .. 64, dim in 1 .. 8.  An entry whose index is outside [0, R) is skipped; a row
    without a usable neighbour comes out NaN.  The caller owns every buffer and nothing is made here.  Returns out."""
    _dev(idx, strength, y, out)
    assert idx.dtype == torch.int32 and strength.dtype == torch.float32 and idx.dim() == 2 and strength.shape == idx.shape
    assert y.dtype == torch.float32 and out.dtype == torch.float32 and y.dim() == 2 and out.dim() == 2 and y.shape[1] == out.shape[1]
    m, dim = idx.shape[1], y.shape[1]
    assert 1 <= m <= 64, f"m={m} outside 1 .. 64"
    assert 1 <= dim <= 8, f"dim={dim} outside 1 .. 8"
    Rq, ld_idx = _rows(idx, m, "idx")
    _, ld_strength = _rows(strength, m, "strength")
    R, ldy = _rows(y, dim, "y")
    rows_out, ldq = _rows(out, dim, "out")
    assert rows_out == Rq, "out has one row per query"

    def launch():
        if Rq == 0:
            return
        check(_lib.load().vf_umap_init_transform(idx.data_ptr(), ld_idx, strength.data_ptr(), ld_strength, Rq, m, y.data_ptr(), ldy, R,
                                                 dim, out.data_ptr(), ldq, _stream()), "vf_umap_init_transform")
    _run(launch, lambda: ("umap_init_transform", 2.0 * Rq * m * (dim + 1), 4.0 * Rq * (m * (2 + dim) + dim), f"Rq={Rq} m={m} dim={dim}",
                          family or _SCOPE))
    return out


def umap_layout_transform(idx: torch.Tensor, samples: torch.Tensor, y: torch.Tensor, yq: torch.Tensor, *, epoch_begin: int,
                          epoch_end: int, n_epochs: int, a: float, b: float, gamma: float = 1.0, learning_rate: float = 1.0,
                          negative_sample_rate: int = 5, seed: int = 42, first_row: int = 0, family: str = ""):
    """The epochs [epoch_begin, epoch_end) of the layout of the queries IN PLACE on yq, the training points y standing still
    (vf_umap_layout_transform, include/vf_hip_umap_transform.h): all epochs of a query run inside one kernel, a bounded number
    per launch from a loop inside the library.  idx int32 [Rq, m] and samples int32 [Rq, m] row-strided, only read; y fp32
    [R, dim] row-strided, only read; yq fp32 [Rq, dim] row-strided; m in 1 .. 64, dim in 1 .. 8.  learning_rate is the FIT's:
    the entry divides it by 4.  Row i is vertex first_row + i of the hash, so a query's result depends on its own row, y and
    that number alone: any split of the epochs, and any split of the rows that keeps the numbers, gives the same bits.  The
    caller owns every buffer and nothing is made here.  Returns yq."""
    _dev(idx, samples, y, yq)
    assert idx.dtype == torch.int32 and samples.dtype == torch.int32 and idx.dim() == 2 and samples.shape == idx.shape
    assert y.dtype == torch.float32 and yq.dtype == torch.float32 and y.dim() == 2 and yq.dim() == 2 and y.shape[1] == yq.shape[1]
    m, dim = idx.shape[1], y.shape[1]
    assert 1 <= m <= 64, f"m={m} outside 1 .. 64"
    assert 1 <= dim <= 8, f"dim={dim} outside 1 .. 8"
    Rq, ld_idx = _rows(idx, m, "idx")
    _, ld_samples = _rows(samples, m, "samples")
    R, ldy = _rows(y, dim, "y")
    rows_q, ldq = _rows(yq, dim, "yq")
    assert rows_q == Rq, "yq has one row per query"
    epochs = max(int(epoch_end) - int(epoch_begin), 0)

    def launch():
        if Rq == 0:
            return
        check(_lib.load().vf_umap_layout_transform(idx.data_ptr(), ld_idx, samples.data_ptr(), ld_samples, Rq, m, int(first_row),
                                                   y.data_ptr(), ldy, R, dim, yq.data_ptr(), ldq, int(epoch_begin), int(epoch_end),
                                                   int(n_epochs), float(a), float(b), float(gamma), float(learning_rate),
                                                   int(negative_sample_rate), int(seed) & 0xFFFFFFFF, _stream()), "vf_umap_layout_transform")
    # an upper figure: every entry due in every epoch, 40 operations per move; bytes: the lists and the neighbours' rows once per
    # launch, a negative vertex's row per repulsion
    _run(launch, lambda: ("umap_layout_transform", 40.0 * epochs * Rq * m * (1 + int(negative_sample_rate)),
                          4.0 * Rq * (m * (2 + dim) * -(-epochs // 8) + 2 * dim) + 4.0 * epochs * Rq * m * int(negative_sample_rate) * dim,
                          f"Rq={Rq} m={m} dim={dim} R={R} epochs={epochs}", family or _SCOPE))
    return yq


def _csr(rowptr: torch.Tensor, col: torch.Tensor, w: torch.Tensor):
    """(vertices, entries) of a CSR graph: rowptr int64 [R + 1], col int32 [nnz], w fp32 [nnz], contiguous."""
    assert rowptr.dim() == 1 and rowptr.shape[0] >= 1, "rowptr: int64 [R + 1]"
    R, nnz = rowptr.shape[0] - 1, col.shape[0]
    _vec(rowptr, R + 1, torch.int64, "rowptr")
    _vec(col, nnz, torch.int32, "col")
    _vec(w, nnz, torch.float32, "w")
    return R, nnz


def graph_degree(rowptr: torch.Tensor, col: torch.Tensor, w: torch.Tensor, *, deg: torch.Tensor, dinv_sqrt: torch.Tensor, family: str = ""):
    """The weighted degree of every vertex of a CSR graph and its inverse square root (vf_graph_degree,
    include/vf_hip_spectral.h): deg[i] the sum of row i's w in the header's fixed order, dinv_sqrt[i] = 1 / sqrt(deg[i]) where
    deg[i] > 0 and +0 elsewhere.  rowptr int64 [R + 1], col int32 [nnz], w fp32 [nnz], deg and dinv_sqrt fp32 [R], contiguous.
    The caller owns every buffer and nothing is made here.  Returns (deg, dinv_sqrt)."""
    _dev(rowptr, col, w, deg, dinv_sqrt)
    R, nnz = _csr(rowptr, col, w)
    _vec(deg, R, torch.float32, "deg")
    _vec(dinv_sqrt, R, torch.float32, "dinv_sqrt")

    def launch():
        if R == 0:
            return
        check(_lib.load().vf_graph_degree(rowptr.data_ptr(), col.data_ptr(), w.data_ptr(), nnz, R, deg.data_ptr(), dinv_sqrt.data_ptr(),
                                          _stream()), "vf_graph_degree")
    _run(launch, lambda: ("graph_degree", 1.0 * nnz, 4.0 * nnz + 16.0 * R, f"R={R} nnz={nnz}", family or _SCOPE))
    return deg, dinv_sqrt


def spmm_recur(rowptr: torch.Tensor, col: torch.Tensor, w: torch.Tensor, dinv_sqrt: torch.Tensor, x0: torch.Tensor, x1: torch.Tensor,
               x2: torch.Tensor, coef, *, family: str = ""):
    """coef.shape[0] steps of Z = coef[t][0] * (S Y) + coef[t][1] * Y + coef[t][2] * W with S = D^-1/2 W D^-1/2 (vf_spmm_recur,
    include/vf_hip_spectral.h), one kernel per step launched from a loop inside the library.  x0 holds the newest block, x2 the
    one before it, x1 is overwritten first; step t reads x[t mod 3] and x[(t + 2) mod 3] and writes x[(t + 1) mod 3].  x0, x1, x2
    fp32 [R, p] row-strided with one stride, p in 1 .. 32, three distinct buffers.  coef: a HOST numpy array fp32 [steps, 3],
    read before the call returns; a coefficient of exactly 0 skips its term, whose operand is then not read.  The caller owns
    every buffer and nothing is made here.  Returns the buffer that holds the result: x[steps mod 3]."""
    _dev(rowptr, col, w, dinv_sqrt, x0, x1, x2)
    R, nnz = _csr(rowptr, col, w)
    _vec(dinv_sqrt, R, torch.float32, "dinv_sqrt")
    assert x0.dtype == x1.dtype == x2.dtype == torch.float32 and x0.dim() == 2 and x0.shape == x1.shape == x2.shape and x0.shape[0] == R
    p = x0.shape[1]
    assert 1 <= p <= 32, f"p={p} outside 1 .. 32"
    ld = _rows(x0, p, "x0")[1]
    assert ld == _rows(x1, p, "x1")[1] == _rows(x2, p, "x2")[1], "x0, x1 and x2 have one row stride"
    assert isinstance(coef, np.ndarray) and coef.dtype == np.float32 and coef.ndim == 2 and coef.shape[1] == 3 and coef.flags.c_contiguous, \
        "coef: a host numpy array fp32 [steps, 3]"
    steps = coef.shape[0]

    def launch():
        if R == 0 or steps == 0:
            return
        check(_lib.load().vf_spmm_recur(rowptr.data_ptr(), col.data_ptr(), w.data_ptr(), nnz, R, dinv_sqrt.data_ptr(), p, x0.data_ptr(),
                                        x1.data_ptr(), x2.data_ptr(), ld, steps, coef.ctypes.data, _stream()), "vf_spmm_recur")
    # per step: every entry's column, weight and the neighbour's scale, a row of p values gathered per entry, the block read
    # twice and written once
    _run(launch, lambda: ("spmm_recur", steps * (2.0 * nnz * p + nnz + 6.0 * R * p), steps * (4.0 * nnz * (3 + p) + 12.0 * R * p + 12.0 * R),
                          f"R={R} p={p} nnz={nnz} steps={steps}", family or _SCOPE))
    return (x0, x1, x2)[steps % 3]


TALL_GRAM_MAX_BLOCKS = 1024                # VF_TALL_GRAM_MAX_BLOCKS: the workspace of tall_gram holds at most this many p x q partials


def tall_gram(a: torch.Tensor, b: torch.Tensor, *, out: torch.Tensor, work: torch.Tensor, family: str = ""):
    """out = a^T b in fp64 (vf_tall_gram, include/vf_hip_spectral.h): a fp32 [R, p] and b fp32 [R, q] row-strided (they may be
    one tensor), p and q in 1 .. 32; out fp64 [p, q] contiguous; work a contiguous fp64 workspace of at least
    ceil(R / chunk) * p * q elements, chunk as the header states it (1024 * p * q always suffice).  Products and sums in fp64 in two stages of fixed
    order, no atomics: two runs are equal bit for bit.  The caller owns every buffer and nothing is made here.  Returns out."""
    _dev(a, b, out, work)
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.dim() == 2 and b.dim() == 2 and a.shape[0] == b.shape[0]
    p, q = a.shape[1], b.shape[1]
    assert 1 <= p <= 32 and 1 <= q <= 32, f"p={p}, q={q} outside 1 .. 32"
    R, lda = _rows(a, p, "a")
    ldb = _rows(b, q, "b")[1]
    assert out.dtype == torch.float64 and tuple(out.shape) == (p, q) and out.is_contiguous(), "out: a contiguous fp64 [p, q]"
    chunk = 64 * max(-(-R // (64 * TALL_GRAM_MAX_BLOCKS)), 1)          # the header's partition: nb = ceil(R / chunk) <= 1024 partials
    assert work.dtype == torch.float64 and work.dim() == 1 and work.is_contiguous() and work.shape[0] >= -(-R // chunk) * p * q, \
        "work: fp64, at least ceil(R / chunk) * p * q elements (1024 * p * q always suffice)"

    def launch():
        check(_lib.load().vf_tall_gram(a.data_ptr(), lda, b.data_ptr(), ldb, R, p, q, out.data_ptr(), work.data_ptr(), _stream()), "vf_tall_gram")
    _run(launch, lambda: ("tall_gram", 2.0 * R * p * q, 4.0 * R * (p + q) + 8.0 * p * q, f"R={R} p={p} q={q}", family or _SCOPE))
    return out


def tall_mul(x: torch.Tensor, t: torch.Tensor, *, out: torch.Tensor, family: str = ""):
    """out = x t with the sum in fp64, rounded once to fp32 (vf_tall_mul, include/vf_hip_spectral.h): x fp32 [R, p] row-strided,
    t fp64 [p, q] contiguous on the device, out fp32 [R, q] row-strided, not overlapping x; p and q in 1 .. 32.  One thread per
    output element, k ascending.  The caller owns every buffer and nothing is made here.  Returns out."""
    _dev(x, t, out)
    assert x.dtype == torch.float32 and out.dtype == torch.float32 and t.dtype == torch.float64 and x.dim() == 2 and t.dim() == 2 and out.dim() == 2
    p, q = t.shape
    assert 1 <= p <= 32 and 1 <= q <= 32 and t.is_contiguous() and x.shape[1] == p and out.shape[1] == q and x.shape[0] == out.shape[0]
    R, ldx = _rows(x, p, "x")
    ldo = _rows(out, q, "out")[1]

    def launch():
        if R == 0:
            return
        check(_lib.load().vf_tall_mul(x.data_ptr(), ldx, R, p, t.data_ptr(), q, out.data_ptr(), ldo, _stream()), "vf_tall_mul")
    _run(launch, lambda: ("tall_mul", 2.0 * R * p * q, 4.0 * R * (p + q) + 8.0 * p * q, f"R={R} p={p} q={q}", family or _SCOPE))
    return out


def graph_components_rounds(rowptr: torch.Tensor, col: torch.Tensor, w: torch.Tensor, parent: torch.Tensor, g: torch.Tensor,
                            m: torch.Tensor, changed: torch.Tensor, *, rounds: int, family: str = ""):
    """`rounds` rounds of the component search over a CSR graph (vf_graph_components_rounds, include/vf_hip_components.h):
    shortcut g = P[P], every row's minimum over its neighbours' g, and that minimum hooked onto the row and onto its parent
    with an atomic integer minimum, three launches per round from a loop inside the library.  parent int32 [R] is the state
    (the caller starts it as the identity; 0 <= parent[i] <= i), g and m int32 [R] are work vectors, changed int32 [1] is 1
    if the last round run lowered a parent and 0 if not (untouched with rounds == 0); three distinct buffers.  An entry is an
    edge only if w > 0 and 0 <= col < R.  A settled state is a fixed point; on a graph of symmetric structure it is
    parent[i] = the smallest vertex of i's component.  The caller owns every buffer, nothing is made here and nothing is read
    back.  Returns parent."""
    _dev(rowptr, col, w, parent, g, m, changed)
    R, nnz = _csr(rowptr, col, w)
    _vec(parent, R, torch.int32, "parent")
    _vec(g, R, torch.int32, "g")
    _vec(m, R, torch.int32, "m")
    _vec(changed, 1, torch.int32, "changed")
    rounds = int(rounds)
    assert rounds >= 0, f"rounds={rounds} must not be negative"

    def launch():
        if R == 0 or rounds == 0:
            return
        check(_lib.load().vf_graph_components_rounds(rowptr.data_ptr(), col.data_ptr(), w.data_ptr(), nnz, R, parent.data_ptr(), g.data_ptr(),
                                                     m.data_ptr(), changed.data_ptr(), rounds, _stream()), "vf_graph_components_rounds")
    # per round: every entry's column, weight and the neighbour's g; the three vectors read and written
    _run(launch, lambda: ("graph_components_rounds", rounds * (1.0 * nnz + 4.0 * R), rounds * (12.0 * nnz + 8.0 * R + 36.0 * R),
                          f"R={R} nnz={nnz} rounds={rounds}", family or _SCOPE))
    return parent


def csr_components(rowptr: torch.Tensor, col: torch.Tensor, w: torch.Tensor, order: torch.Tensor, rank: torch.Tensor, comp: torch.Tensor,
                   starts: torch.Tensor, rowptr_new: torch.Tensor, *, col_new: torch.Tensor, w_new: torch.Tensor, family: str = ""):
    """The CSR graph renumbered by components (vf_csr_components, include/vf_hip_components.h): new row r is old row order[r]
    with its entries in their order, a column j written as rank[j] - starts[comp[r]] and its weight copied; an entry that is
    no edge (w <= 0 or NaN, a column outside [0, R) or outside the row's component) as column -1 with weight +0.  order, rank
    and comp int32 [R], starts int32 [C + 1], rowptr_new int64 [R + 1] (the cumulative permuted row lengths), col_new int32
    [nnz] and w_new fp32 [nnz], contiguous.  The caller owns every buffer and nothing is made here.  Returns (col_new, w_new)."""
    _dev(rowptr, col, w, order, rank, comp, starts, rowptr_new, col_new, w_new)
    R, nnz = _csr(rowptr, col, w)
    for t, name in ((order, "order"), (rank, "rank"), (comp, "comp")):
        _vec(t, R, torch.int32, name)
    assert starts.dim() == 1 and starts.shape[0] >= 1, "starts: int32 [C + 1]"
    C = starts.shape[0] - 1
    _vec(starts, C + 1, torch.int32, "starts")
    _vec(rowptr_new, R + 1, torch.int64, "rowptr_new")
    _vec(col_new, nnz, torch.int32, "col_new")
    _vec(w_new, nnz, torch.float32, "w_new")
    assert R == 0 or 1 <= C <= R, f"C={C} outside 1 .. R={R}"

    def launch():
        if R == 0:
            return
        check(_lib.load().vf_csr_components(rowptr.data_ptr(), col.data_ptr(), w.data_ptr(), nnz, R, order.data_ptr(), rank.data_ptr(),
                                            comp.data_ptr(), starts.data_ptr(), C, rowptr_new.data_ptr(), col_new.data_ptr(),
                                            w_new.data_ptr(), _stream()), "vf_csr_components")
    _run(launch, lambda: ("csr_components", 1.0 * nnz, 20.0 * nnz + 40.0 * R, f"R={R} nnz={nnz} C={C}", family or _SCOPE))
    return col_new, w_new


def segment_mean_gather(x: torch.Tensor, order: torch.Tensor, starts: torch.Tensor, *, out: torch.Tensor, family: str = ""):
    """out[k] = the mean of the rows x[order[q]] for starts[k] <= q < starts[k + 1] (vf_segment_mean_gather,
    include/vf_hip_components.h): summed in fp64 in the header's fixed order (four interleaved partials, added in order),
    divided in fp64 and rounded once to fp32; no atomics.  x fp32 [R, d] and out fp32 [C, d] row-strided, order int32 [R],
    starts int32 [C + 1] non-decreasing from 0 to R.  A segment without positions gets NaN.  One block per (segment, 64
    columns).  The caller owns every buffer and nothing is made here.  Returns out."""
    _dev(x, order, starts, out)
    assert x.dtype == torch.float32 and out.dtype == torch.float32 and x.dim() == 2 and out.dim() == 2 and x.shape[1] == out.shape[1] >= 1
    d = x.shape[1]
    R, ldx = _rows(x, d, "x")
    assert starts.dim() == 1 and starts.shape[0] >= 1, "starts: int32 [C + 1]"
    C = starts.shape[0] - 1
    assert out.shape[0] == C, f"out has {out.shape[0]} rows for {C} segments"
    ldo = _rows(out, d, "out")[1]
    _vec(order, R, torch.int32, "order")
    _vec(starts, C + 1, torch.int32, "starts")

    def launch():
        if C == 0:
            return
        check(_lib.load().vf_segment_mean_gather(x.data_ptr(), ldx, R, d, order.data_ptr(), starts.data_ptr(), C, out.data_ptr(), ldo,
                                                 _stream()), "vf_segment_mean_gather")
    _run(launch, lambda: ("segment_mean_gather", 1.0 * R * d, 4.0 * R * d + 4.0 * R * -(-d // 64) + 4.0 * C * d, f"R={R} d={d} C={C}",
                          family or _SCOPE))
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out_dtype=None, gelu: bool = False,
              eps: float = 1e-5, out: torch.Tensor | None = None) -> torch.Tensor:
    """out_dtype None = the current compute dtype (ops.cdt())."""
    _dev(x, gamma, beta, out)
    out_dtype = cdt() if out_dtype is None else out_dtype
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
    rows, D = x.shape
    if out is None:
        out = torch.empty((rows, D), dtype=out_dtype, device=x.device)

    def launch():
        check(_lib.load().vf_layernorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), rows, D, eps,
                                       _dt(out.dtype), int(gelu), _stream()), "vf_layernorm")
    _run(launch, lambda: ("layernorm", 0.0, float(rows) * D * (4 + out.element_size()), f"D={D}", _SCOPE))
    return out


def mask_to_cu_seqlens(pad: torch.Tensor) -> torch.Tensor:
    """pad bool/uint8 [W, L] (True = pad) -> int32 [W+1] exclusive prefix sum of valid counts."""
    _dev(pad)
    pad = pad.view(torch.uint8) if pad.dtype == torch.bool else pad
    assert pad.dtype == torch.uint8 and pad.is_contiguous() and pad.dim() == 2
    W, L = pad.shape
    cu = torch.empty(W + 1, dtype=torch.int32, device=pad.device)
    check(_lib.load().vf_mask_to_cu_seqlens(pad.data_ptr(), cu.data_ptr(), W, L, _stream()), "vf_mask_to_cu_seqlens")
    return cu


def embed_pack(ids: torch.Tensor, pad: torch.Tensor, cu: torch.Tensor, table: torch.Tensor,
               pos_table: torch.Tensor | None, n_tokens: int) -> torch.Tensor:
    _dev(ids, pad, cu, table, pos_table)
    pad = pad.view(torch.uint8) if pad.dtype == torch.bool else pad
    assert ids.dtype == torch.int64 and ids.is_contiguous() and ids.dim() == 2 and pad.shape == ids.shape
    assert table.dtype == torch.float32 and table.is_contiguous()
    W, L = ids.shape
    d = table.shape[1]
    out = torch.empty((n_tokens, d), dtype=torch.float32, device=ids.device)
    check(_lib.load().vf_embed_pack(ids.data_ptr(), pad.data_ptr(), cu.data_ptr(), table.data_ptr(), _ptr(pos_table),
                                    out.data_ptr(), W, L, d, table.shape[0], _stream()), "vf_embed_pack")
    return out


def embed_stream(ids: torch.Tensor, pad: torch.Tensor, cu: torch.Tensor, table: torch.Tensor,
                 pos_table: torch.Tensor | None, n_tokens: int, need_x: bool = False, need_t16: bool = True,
                 eps: float = 1e-5) -> LnStream:
    """embed_pack + ln_stream (+ trunk16_of) in one kernel (vf_embed_stream): the encoder input as an LnStream whose fp32
    rows exist only on request; bit-identical copies and statistics to the three-step form."""
    _dev(ids, pad, cu, table, pos_table)
    pad = pad.view(torch.uint8) if pad.dtype == torch.bool else pad
    assert ids.dtype == torch.int64 and ids.is_contiguous() and ids.dim() == 2 and pad.shape == ids.shape
    assert table.dtype == torch.float32 and table.is_contiguous()
    W, L = ids.shape
    d = table.shape[1]
    dev = ids.device
    x = torch.empty((n_tokens, d), dtype=torch.float32, device=dev) if need_x else None
    x16 = torch.empty((n_tokens, d), dtype=cdt(), device=dev)
    t16 = torch.empty((n_tokens, d), dtype=torch.float16, device=dev) if need_t16 else None
    stats = torch.empty((n_tokens, 2), dtype=torch.float32, device=dev)
    scale = x16_scale_for(x16.dtype)
    alert = _alert_flag(dev)

    def launch():
        check(_lib.load().vf_embed_stream(ids.data_ptr(), pad.data_ptr(), cu.data_ptr(), table.data_ptr(), _ptr(pos_table),
                                          _ptr(x), x16.data_ptr(), _dt(x16.dtype), scale, _ptr(t16), T16_SCALE, stats.data_ptr(),
                                          eps, LN_FOLD_RATIO_LIMIT, ln_fold_abs_limit(), alert.data_ptr(), W, L, d, table.shape[0],
                                          _stream()),
              "vf_embed_stream")
    _run(launch, lambda: ("layernorm", 0.0, float(n_tokens) * d * (2 + (2 if need_t16 else 0) + (4 if need_x else 0)),
                          f"embed_stream D={d}", _SCOPE))
    return LnStream(x, x16, stats, scale, t16)


def token_keys(ids: torch.Tensor, pad: torch.Tensor, cu: torch.Tensor, n_tokens: int, vocab: int, key_L: int) -> torch.Tensor:
    """int64 [n_tokens]: id * key_L + position of every packed valid token (vf_token_keys; key_L = 1: the ids themselves)."""
    _dev(ids, pad, cu)
    pad = pad.view(torch.uint8) if pad.dtype == torch.bool else pad
    assert ids.dtype == torch.int64 and ids.is_contiguous() and ids.dim() == 2 and pad.shape == ids.shape and pad.is_contiguous()
    W, L = ids.shape
    keys = torch.empty((n_tokens,), dtype=torch.int64, device=ids.device)
    check(_lib.load().vf_token_keys(ids.data_ptr(), pad.data_ptr(), cu.data_ptr(), keys.data_ptr(), W, L, int(vocab), int(key_L),
                                    _stream()), "vf_token_keys")
    return keys


def segment_mean(x: torch.Tensor, cu: torch.Tensor, out_dtype=None) -> torch.Tensor:
    _dev(x, cu)
    out_dtype = cdt() if out_dtype is None else out_dtype
    assert x.dtype == torch.float32 and x.is_contiguous() and cu.dtype == torch.int32
    W = cu.numel() - 1
    out = torch.empty((W, x.shape[1]), dtype=out_dtype, device=x.device)
    check(_lib.load().vf_segment_mean(x.data_ptr(), cu.data_ptr(), out.data_ptr(), W, x.shape[1], _dt(out_dtype),
                                      _stream()), "vf_segment_mean")
    return out


def segment_mean16(x16: torch.Tensor, cu: torch.Tensor, in_scale: float = 1.0, split: bool = False) -> torch.Tensor:
    """Per-window mean of a 16-bit stream [n_tok, d] (rows may be strided), values times in_scale (vf_segment_mean16):
    fp32 [W, d], or with split=True the means as two 16-bit halves [W, 2 d] = [hi | lo] (lo = rn16(mean - hi)) in the type
    of x16 -- a 16-bit GEMM operand that carries the fp32 mean to ~2^-17."""
    _dev(x16, cu)
    assert _is16(x16.dtype) and x16.dim() == 2 and x16.stride(1) == 1 and cu.dtype == torch.int32
    W, d = cu.numel() - 1, x16.shape[1]
    out = torch.empty((W, 2 * d), dtype=x16.dtype, device=x16.device) if split else torch.empty((W, d), dtype=torch.float32,
                                                                                               device=x16.device)
    check(_lib.load().vf_segment_mean16(x16.data_ptr(), x16.stride(0), _dt(x16.dtype), cu.data_ptr(), float(in_scale),
                                        None if split else out.data_ptr(), out.data_ptr() if split else None, W, d,
                                        _stream()), "vf_segment_mean16")
    return out


def segment_max(x: torch.Tensor, cu: torch.Tensor) -> torch.Tensor:
    _dev(x, cu)
    assert x.dtype == torch.float32 and x.is_contiguous() and cu.dtype == torch.int32
    W = cu.numel() - 1
    out = torch.empty((W, x.shape[1]), dtype=torch.float32, device=x.device)
    check(_lib.load().vf_segment_max(x.data_ptr(), cu.data_ptr(), out.data_ptr(), W, x.shape[1], _stream()),
          "vf_segment_max")
    return out


def segment_linear(x: torch.Tensor, cu: torch.Tensor, pad: torch.Tensor, lin_w: torch.Tensor, lin_b: torch.Tensor | None,
                   out_dtype=None) -> torch.Tensor:
    """seq2reg "linear" pooling: out[w] = sum_p lin_w[p] * x[row(w, p)] over the valid positions p, + lin_b."""
    _dev(x, cu, pad, lin_w, lin_b)
    out_dtype = cdt() if out_dtype is None else out_dtype
    pad = pad.view(torch.uint8) if pad.dtype == torch.bool else pad
    assert x.dtype == torch.float32 and x.is_contiguous() and cu.dtype == torch.int32 and pad.dtype == torch.uint8
    W, L = pad.shape
    assert lin_w.dtype == torch.float32 and lin_w.numel() == L and lin_w.is_contiguous() and cu.numel() == W + 1
    out = torch.empty((W, x.shape[1]), dtype=out_dtype, device=x.device)
    check(_lib.load().vf_segment_linear(x.data_ptr(), cu.data_ptr(), pad.data_ptr(), lin_w.data_ptr(), _ptr(lin_b),
                                        out.data_ptr(), W, L, x.shape[1], _dt(out_dtype), _stream()), "vf_segment_linear")
    return out


def affine_rows(src: torch.Tensor, idx: torch.Tensor, scale: torch.Tensor | None = None,
                shift: torch.Tensor | None = None) -> torch.Tensor:
    """out[i] = src[idx[i]] * scale[i] + shift[i] (fp32 rows; scale / shift optional per-row scalars)."""
    _dev(src, idx, scale, shift)
    assert src.dtype == torch.float32 and src.is_contiguous() and idx.dtype == torch.int64 and idx.is_contiguous()
    for t in (scale, shift):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == idx.numel())
    out = torch.empty((idx.numel(), src.shape[1]), dtype=torch.float32, device=src.device)
    check(_lib.load().vf_affine_rows_f32(src.data_ptr(), idx.data_ptr(), _ptr(scale), _ptr(shift), out.data_ptr(),
                                         idx.numel(), src.shape[1], _stream()), "vf_affine_rows_f32")
    return out


def add_rows(a: torch.Tensor, b: torch.Tensor, idx_a: torch.Tensor | None = None, idx_b: torch.Tensor | None = None) -> torch.Tensor:
    """out[i] = a[idx_a[i]] + b[idx_b[i]] (identity where an index is None), fp32 rows."""
    _dev(a, b, idx_a, idx_b)
    for t in (a, b):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2
    for t in (idx_a, idx_b):
        assert t is None or (t.dtype == torch.int64 and t.is_contiguous())
    n = idx_a.numel() if idx_a is not None else (idx_b.numel() if idx_b is not None else a.shape[0])
    assert a.shape[1] == b.shape[1] and (idx_a is not None or a.shape[0] == n) and (idx_b is not None or b.shape[0] == n)
    out = torch.empty((n, a.shape[1]), dtype=torch.float32, device=a.device)
    check(_lib.load().vf_add_rows_f32(a.data_ptr(), _ptr(idx_a), b.data_ptr(), _ptr(idx_b), out.data_ptr(), n, a.shape[1],
                                      _stream()), "vf_add_rows_f32")
    return out


def gather_rows_f32(a: torch.Tensor, b: torch.Tensor | None, idx: torch.Tensor, out_dtype=torch.float32) -> torch.Tensor:
    """out[i] = a[idx[i]] if idx[i] >= 0 else b[-idx[i]-1]."""
    _dev(a, b, idx)
    assert a.dtype == torch.float32 and a.is_contiguous() and idx.dtype == torch.int64
    assert b is None or (b.dtype == torch.float32 and b.is_contiguous() and b.shape[1] == a.shape[1])
    out = torch.empty((idx.numel(), a.shape[1]), dtype=out_dtype, device=a.device)
    check(_lib.load().vf_gather_rows_f32(a.data_ptr(), _ptr(b), idx.data_ptr(), out.data_ptr(), idx.numel(), a.shape[1],
                                         _dt(out_dtype), _stream()), "vf_gather_rows_f32")
    return out


def gather_rows_bf16(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    _dev(src, idx)
    assert _is16(src.dtype) and src.stride(1) == 1 and idx.dtype == torch.int64
    out = torch.empty((idx.numel(), src.shape[1]), dtype=src.dtype, device=src.device)

    def launch():
        check(_lib.load().vf_gather_rows_bf16(src.data_ptr(), src.stride(0), idx.data_ptr(), out.data_ptr(), out.stride(0),
                                              idx.numel(), src.shape[1], _stream()), "vf_gather_rows_bf16")
    _run(launch, lambda: ("layernorm", 0.0, float(idx.numel()) * (src.shape[1] * 4 + 8), f"gather_rows16 D={src.shape[1]}", _SCOPE))
    return out


def rowdot_softplus(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor | None, softplus: bool = True) -> torch.Tensor:
    _dev(x, w, b)
    assert x.dtype == torch.float32 and x.is_contiguous() and w.dtype == torch.float32 and w.numel() == x.shape[1]
    out = torch.empty((x.shape[0], 1), dtype=torch.float32, device=x.device)
    check(_lib.load().vf_rowdot_softplus(x.data_ptr(), w.data_ptr(), _ptr(b), out.data_ptr(), x.shape[0], x.shape[1],
                                         int(softplus), _stream()), "vf_rowdot_softplus")
    return out


def last_kernel(which: str = "gemm") -> str:
    """Name of the kernel this thread's most recent GEMM ("gemm") or attention ("attn") entry dispatched to (vf_last_kernel:
    a diagnostic for sweeps over shapes, scripts/s2r_dims_sweep.py)."""
    name = _lib.load().vf_last_kernel(0 if which == "gemm" else 1)
    return name.decode() if name else ""


def cast16(x: torch.Tensor, dtype=None) -> torch.Tensor:
    """fp32 -> 16-bit operand type (default: the current compute dtype), round to nearest even."""
    _dev(x)
    dtype = cdt() if dtype is None else dtype
    assert x.dtype == torch.float32 and x.is_contiguous() and _is16(dtype)
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    lib = _lib.load()
    fn = lib.vf_cast_f32_f16 if dtype == torch.float16 else lib.vf_cast_f32_bf16
    check(fn(x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "vf_cast_f32_16")
    return out


def cast_bf16(x: torch.Tensor) -> torch.Tensor:
    return cast16(x, torch.bfloat16)

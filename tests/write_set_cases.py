"""Write sets and read sets of the C ABI (include/vf_hip.h), shared by tests/test_write_sets_cpu.py and
tests/test_write_sets_gpu.py.  Importing this module needs no GPU; a case touches the device only when its `run` is called.

The contract, per entry: the bytes a call changes are exactly the documented output set, and those bytes depend on nothing
outside the documented operands.  Every output and workspace of variantformer_amd/ops.py comes from torch.empty, and within
one process the caching allocator hands a freed block to the next request of the same size -- so without help a launch's
output buffer often already holds the previous launch's correct answer, and a kernel that skipped a tail store or read a
workspace before writing it would pass every bit-identity test of the suite.  The help is three things:

  poison patterns     0xFF (NaN in fp32 / bf16 / fp16, -1 in integers), 0x00 (what a fresh process sees) and 0x3C (small
                      plausible finite values in all three float types: what a recycled block looks like).  The third is a
                      condition, not an option: fmaxf(NaN, x) = x, so a stale read inside a running maximum is invisible
                      under NaN, and zero is neutral in sums.
  poisoning allocator `poison_allocations(pattern)` / `install(monkeypatch, pattern)`: every torch.empty / torch.empty_like
                      made inside the wrapper modules returns memory filled with the pattern, the fill enqueued on the current
                      stream.  Installed with pytest's MonkeyPatch on the `torch` NAME of those modules (a pass-through
                      proxy), undone when the block or the test ends; nothing global is touched.
  guarded operands    every input is an interior slice of a larger buffer filled with the pattern: GUARD_ROWS = 256 rows
                      before and after (one full tile of the largest kernel, so a masked over-read of a tile still lands in
                      memory the test owns) and GUARD_COLS = 8 columns either side wherever the entry takes a row stride;
                      pointers stay 16-byte aligned.  Row-map tables carry poisoned rows that no index names.

`check_write_set(run, written, ...)` calls run(pattern) once per pattern -- guards, outputs and workspaces all hold that
pattern -- and asserts: (a) inside the expected-write mask the three runs are bit-identical (which is also the read-set half:
the run with 0xFF guards equals the run with 0x00 guards bit for bit, so no 0 x NaN from a masked key and no wide load past dh
reaches a result); (b) outside it every byte still holds the run's pattern; (c) inside it the 0xFF run has a NaN only where the
case's reference has one; (d) the 0x00 run meets the case's reference (tolerances are those of the existing suites: nothing
new but bit equality is introduced here).

What this cannot catch: an over-read whose value is DISCARDED (loaded and then masked out by a select rather than by
arithmetic) leaves no trace in any output; the guards only keep such a load inside the test's own memory.
"""
from __future__ import annotations

import contextlib
import functools
import math
import re
from typing import Callable, NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vf_oracle as O
from tests import attn_edge_cases as E
from tests.helpers import _rand

PATTERNS = (0xFF, 0x00, 0x3C)
GUARD_ROWS, GUARD_COLS = 256, 8
DEVICE = "cuda"
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
WRAPPER_MODULES = ("variantformer_amd.ops", "variantformer_amd.attn_maps", "variantformer_amd.seq2gene.modules.layers")
# the analysis pipelines: their out= buffers and workspaces are allocated by the pipeline, not by the wrappers of ops.py
# (tests/analysis_pipeline_cases.py); poisoned only where a caller passes modules=
ANALYSIS_MODULES = ("variantformer_amd.manifold", "variantformer_amd.linkage", "variantformer_amd.enrichment",
                    "variantformer_amd.neighbors", "variantformer_amd.processors.ad_risk")


# ---------------------------------------------------------------------------------------------
# poison
# ---------------------------------------------------------------------------------------------
def fill_bytes(t: torch.Tensor, pattern: int) -> torch.Tensor:
    """Every byte of the (contiguous) tensor = pattern, enqueued on the current stream."""
    if t.numel():
        assert t.is_contiguous()
        t.view(torch.uint8).fill_(pattern)
    return t


def poisoned(shape, dtype, device, pattern: int) -> torch.Tensor:
    return fill_bytes(torch.empty(shape, dtype=dtype, device=device), pattern)


class TorchProxy:
    """Stands in for the `torch` module inside a wrapper module: everything passes through, except that empty / empty_like
    return memory filled with the pattern.  `allocated` lists what was handed out, in order."""

    def __init__(self, pattern: int, keep: bool = True):
        self.pattern = pattern
        self.keep = keep              # False: count only (a whole forward's buffers must not be kept alive)
        self.count = 0
        self.allocated = []

    def _hand_out(self, t):
        self.count += 1
        if self.keep:
            self.allocated.append(t)
        return fill_bytes(t, self.pattern)

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *args, **kw):
        return self._hand_out(torch.empty(*args, **kw))

    def empty_like(self, *args, **kw):
        return self._hand_out(torch.empty_like(*args, **kw))


def install(monkeypatch, pattern: int, keep: bool = True, modules=None) -> TorchProxy:
    """Replace the `torch` name of the wrapper modules (or of `modules`) with a poisoning proxy; monkeypatch undoes it."""
    import importlib
    proxy = TorchProxy(pattern, keep)
    for name in WRAPPER_MODULES if modules is None else modules:
        monkeypatch.setattr(importlib.import_module(name), "torch", proxy)
    return proxy


@contextlib.contextmanager
def poison_allocations(pattern: int, keep: bool = True, modules=None):
    import pytest
    with pytest.MonkeyPatch.context() as mp:
        yield install(mp, pattern, keep, modules)


def guarded(x: torch.Tensor, pattern: int, cols: int = 0, device=None, rows: int = GUARD_ROWS) -> torch.Tensor:
    """x as an interior slice of a buffer filled with the pattern: `rows` guard rows (elements, for a 1-D tensor) before and
    after, `cols` guard columns either side (only where the entry takes a row stride: the slice is contiguous otherwise)."""
    device = DEVICE if device is None else device
    if x.dim() == 1:
        big = poisoned((x.numel() + 2 * rows,), x.dtype, device, pattern)
        view = big[rows:rows + x.numel()]
    else:
        assert x.dim() == 2
        big = poisoned((x.shape[0] + 2 * rows, x.shape[1] + 2 * cols), x.dtype, device, pattern)
        view = big[rows:rows + x.shape[0], cols:cols + x.shape[1]]
    view.copy_(x)
    assert view.data_ptr() % 16 == 0, "guard offsets must keep 16-byte alignment"
    return view


def arena(rows: int, cols: int, dtype, pattern: int, device=None, pad_rows: int = 8, pad_cols: int = GUARD_COLS):
    """(big, view): an output slice [rows, cols] inside a poisoned buffer, and the slice's expected-write mask frame."""
    device = DEVICE if device is None else device
    big = poisoned((rows + 2 * pad_rows, cols + 2 * pad_cols), dtype, device, pattern)
    return big, big[pad_rows:pad_rows + rows, pad_cols:pad_cols + cols]


def arena_mask(rows: int, cols: int, inner: torch.Tensor | None = None, pad_rows: int = 8, pad_cols: int = GUARD_COLS):
    m = torch.zeros((rows + 2 * pad_rows, cols + 2 * pad_cols), dtype=torch.bool)
    m[pad_rows:pad_rows + rows, pad_cols:pad_cols + cols] = True if inner is None else inner
    return m


def spread_rows(x: torch.Tensor, pattern: int, cols: int = 0, device=None):
    """A row-map table: row i of x at table row 2 i + 1, every even row poisoned and named by no index.  Returns (table, map)."""
    device = DEVICE if device is None else device
    n = x.shape[0]
    tab = guarded(torch.zeros((2 * n + 1, x.shape[1]), dtype=x.dtype), pattern, cols, device)
    fill_rows = torch.arange(n) * 2 + 1
    even = torch.arange(0, 2 * n + 1, 2, device=tab.device)
    tab[even] = poisoned((even.numel(), x.shape[1]), x.dtype, tab.device, pattern)
    tab[fill_rows.to(tab.device)] = x.to(tab.device)
    return tab, fill_rows


# ---------------------------------------------------------------------------------------------
# checker
# ---------------------------------------------------------------------------------------------
def _bytes(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view(torch.uint8).reshape(*t.shape, t.element_size())


def check_write_set(run: Callable, written: dict, reference: Callable | None = None, nan_ok: dict | None = None,
                    patterns=PATTERNS) -> dict:
    """run(pattern) -> {name: buffer}: the call with outputs, workspaces and guards holding `pattern`; every buffer the call
    may write is returned whole (explicit out= arenas included).  written[name]: bool mask, one flag per element, built on the
    CPU from the header text.  nan_ok[name]: where the reference itself has a NaN (default: nowhere).  reference(buffers of
    the 0x00 run) asserts the case's existing reference.  Returns the 0x00 run's buffers."""
    nan_ok = nan_ok or {}
    runs = {}
    for p in patterns:
        bufs = run(p)
        assert set(bufs) == set(written), (sorted(bufs), sorted(written))
        runs[p] = {k: v.detach().cpu() for k, v in bufs.items()}
    first = patterns[0]
    for name, mask in written.items():
        ref_bytes = _bytes(runs[first][name])
        assert tuple(mask.shape) == tuple(runs[first][name].shape), (name, tuple(mask.shape), tuple(runs[first][name].shape))
        for p in patterns:
            b = _bytes(runs[p][name])
            # (b) outside the mask every byte still holds the pattern
            stray = (b != p).any(dim=-1) & ~mask
            assert not bool(stray.any()), (f"{name}: {int(stray.sum())} elements outside the documented write set were written "
                                           f"(pattern {p:#04x}); first at {tuple(int(i) for i in stray.nonzero()[0])}")
            # (a) inside the mask the runs are bit-identical
            diff = (b != ref_bytes).any(dim=-1) & mask
            assert not bool(diff.any()), (f"{name}: {int(diff.sum())} elements differ between the runs poisoned with {first:#04x} "
                                          f"and {p:#04x} (unwritten, or computed from stale / guard memory); first at "
                                          f"{tuple(int(i) for i in diff.nonzero()[0])}")
        # (c) the NaN-poisoned run has a NaN only where the reference has one
        t = runs[0xFF][name] if 0xFF in runs else None
        if t is not None and t.is_floating_point():
            bad = torch.isnan(t.float()) & mask & ~nan_ok.get(name, torch.zeros_like(mask))
            assert not bool(bad.any()), f"{name}: {int(bad.sum())} NaNs inside the write set; first at {tuple(int(i) for i in bad.nonzero()[0])}"
    out = runs[0x00] if 0x00 in runs else runs[first]
    if reference is not None:
        reference(out)                                  # (d)
    return out


# ---------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------
class Built(NamedTuple):
    run: Callable
    written: dict
    reference: Callable | None = None
    nan_ok: dict | None = None


class WSCase(NamedTuple):
    name: str
    family: str
    entries: tuple            # C-ABI entries the case launches
    wrappers: tuple           # functions of variantformer_amd/ops.py whose allocations the case poisons
    make: Callable            # () -> Built; CPU work only, the device is touched inside Built.run / Built.reference


CASES: list = []


def _case(name, family, entries, wrappers, make):
    CASES.append(WSCase(name, family, tuple(entries), tuple(wrappers), make))


def cases_of(family: str):
    return [c for c in CASES if c.family == family]


def full(*shape):
    return torch.ones(shape, dtype=torch.bool)


def _ops():
    from variantformer_amd import _lib, ops
    _lib.load()
    return ops


def _sync():
    torch.cuda.synchronize()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rd(x, dtype):
    return x.to(TDT[dtype]).float()


def _tol16(dtype):            # tests/test_ops_gpu.py::test_gemm_epilogues (bf16) / test_gemm_fp16_operands (half an fp16 ulp)
    return dict(rtol=2 ** -8, atol=2e-3) if dtype == "bf16" else dict(rtol=2 ** -11, atol=3e-4)


def _close(got, want, **tol):
    np.testing.assert_allclose(got.double().numpy(), want.double().numpy(), **tol)


# ---- vf_gemm_* ------------------------------------------------------------------------------------------------------------
GEMM_EPIS = {"bf16": 0, "f32": 1, "res": 2, "geglu": 3, "gelu_f32": 4, "gelu_bf16": 5}
GEMM_VARIANTS = (0, 1, 5, 20, 22)


@functools.lru_cache(maxsize=None)
def _gemm_operands(dtype, epi, generic):
    geglu = epi == "geglu"
    M, N, K = (77, 64 if geglu else 40, 72) if generic else (515, 800 if geglu else 776, 192)
    a, w = _rd(_rand((M, K), 91), dtype), _rd(_rand((N, K), 92, 1.0 / math.sqrt(K)), dtype)
    b, res = _rand((N,), 93, 0.5), _rand((M, N), 94)
    ref = a.double() @ w.double().t() + b.double()
    if epi == "res":
        ref = ref + res.double()
    if epi in ("gelu_f32", "gelu_bf16"):
        ref = F.gelu(ref)
    if geglu:
        x, gate = ref.chunk(2, dim=-1)
        ref = x * F.gelu(gate)
    return M, N, K, a, w, b, res, ref


def _make_gemm(dtype, epi, variant, generic):
    def make():
        M, N, K, a32, w32, b32, res32, ref = _gemm_operands(dtype, epi, generic)
        tdt = TDT[dtype]
        n_out = N // 2 if epi == "geglu" else N
        odt = torch.float32 if epi in ("f32", "res", "gelu_f32") else tdt

        def run(p):
            ops = _ops()
            w, b = w32.to(tdt).to(DEVICE), b32.to(DEVICE)
            if epi == "geglu":
                w, b = ops.pack_geglu_rows(w, b)
            a = guarded(a32.to(tdt), p, GUARD_COLS)
            w, b = guarded(w, p), guarded(b, p)
            r = guarded(res32, p, GUARD_COLS) if epi == "res" else None
            big, out = (None, None) if generic else arena(M, n_out, odt, p)       # generic cases: the wrapper's own allocation
            with poison_allocations(p):
                got = ops.gemm(a, w, b, GEMM_EPIS[epi], residual=r, out=out, variant=variant)
            _sync()
            return {"out": got if generic else big}

        def reference(bufs):
            got = bufs["out"] if generic else bufs["out"][8:8 + M, GUARD_COLS:GUARD_COLS + n_out]
            if odt == torch.float32:          # tests/test_ops_gpu.py::test_gemm_epilogues
                _close(got, ref, rtol=2e-5, atol=2e-5 * math.sqrt(K))
            else:
                # 16-bit outputs: ::test_gemm_epilogues / test_gemm_fp16_operands; GEGLU: ::test_gemm_geglu / test_gemm_geglu_fp16;
                # fp16 GELU: tests/test_ops_edges_gpu.py::_gemm_strided
                tol = _tol16(dtype) if epi == "bf16" else (dict(rtol=2 ** -10, atol=3e-4) if (dtype, epi) == ("fp16", "geglu")
                                                            else dict(rtol=2 ** -8, atol=2e-3))
                _close(got.float(), ref, **tol)
        return Built(run, {"out": full(M, n_out) if generic else arena_mask(M, n_out)}, reference)
    return make


for _dt in TDT:
    for _epi in GEMM_EPIS:
        for _v in GEMM_VARIANTS:
            _ent = f"vf_gemm_{'bf16' if _dt == 'bf16' else 'f16'}" + ("_ex" if _v else "")
            _case(f"gemm-{_dt}-{_epi}-v{_v}", "gemm", [_ent], ["gemm"], _make_gemm(_dt, _epi, _v, False))
        _case(f"gemm-{_dt}-{_epi}-generic", "gemm", [f"vf_gemm_{'bf16' if _dt == 'bf16' else 'f16'}"], ["gemm"],
              _make_gemm(_dt, _epi, 0, True))


# ---- vf_gemm_ln as consumer -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _consumer_operands(dtype, epi):
    M, N, K = 515, (800 if epi == "geglu" else 776), 192
    scale = 1.0 if dtype == "bf16" else 2.0 ** -4
    x = _rand((M, K), 321, 2.0) + _rand((M, 1), 322, 1.5)
    x16 = _rd(x * scale, dtype)
    xd = x.double()
    stats = torch.stack([xd.mean(1) * scale, 1.0 / torch.sqrt(xd.var(1, unbiased=False) + 1e-5) / scale], dim=1).float()
    w = _rd(_rand((N, K), 324, 1.0 / math.sqrt(K)), dtype)
    b = _rand((N,), 325, 0.5)
    colsum = w.double().sum(1).float()
    y = (x16.double() @ w.double().t() - stats[:, :1].double() * colsum.double()[None]) * stats[:, 1:].double() + b.double()
    if epi == "geglu":
        y = y[:, :N // 2] * F.gelu(y[:, N // 2:])
    return M, N, K, x16, stats, w, b, colsum, y


def _make_consumer(dtype, epi, direct=False):
    def make():
        M, N, K, x16, stats, w32, b32, cs32, ref = _consumer_operands(dtype, epi)
        tdt = TDT[dtype]
        n_out = N // 2 if epi == "geglu" else N
        odt = torch.float32 if epi == "f32" else tdt

        def run(p):
            ops = _ops()
            w, b, cs = w32.to(tdt).to(DEVICE), b32.to(DEVICE), cs32.to(DEVICE)
            if epi == "geglu":               # the packed operand's own row sums, permuted like its rows (bias travels as "bias")
                w, perm = ops.pack_geglu_rows(w, torch.arange(N, dtype=torch.float32, device=DEVICE))
                b, cs = b[perm.long()], cs[perm.long()]
            s = ops.LnStream(None, guarded(x16.to(tdt), p, GUARD_COLS), guarded(stats, p), 1.0)
            w, b, cs = guarded(w, p), guarded(b.contiguous(), p), guarded(cs.contiguous(), p)
            if direct:
                from variantformer_amd import _lib
                big, out = arena(M, n_out, odt, p)
                _lib.check(_lib.load().vf_gemm_ln_bf16(s.x16.data_ptr(), s.x16.stride(0), w.data_ptr(), b.data_ptr(), None, 0,
                                                       out.data_ptr(), out.stride(0), M, N, K, GEMM_EPIS[epi], s.stats.data_ptr(),
                                                       cs.data_ptr(), None, 0, None, _stream()), "vf_gemm_ln_bf16")
                _sync()
                return {"out": big}
            with poison_allocations(p):
                out = ops.gemm_ln_consumer(s, w, b, cs, GEMM_EPIS[epi])
            _sync()
            return {"out": out}

        def reference(bufs):
            got = bufs["out"][8:8 + M, GUARD_COLS:GUARD_COLS + n_out] if direct else bufs["out"]
            if epi == "f32":                  # tests/test_ops_gpu.py::test_lowrank_context_attention_pieces
                _close(got, ref, rtol=2e-4, atol=2e-4)
            elif dtype == "bf16":             # ::test_gemm_ln_consumer_matches_folded_oracle
                _close(got.float(), ref, rtol=2 ** -7, atol=4e-3)
            else:                             # ::test_gemm_ln_fp16_consumer_matches_folded_oracle_and_unfolded_pair
                _close(got.float(), ref, rtol=2 ** -10, atol=1e-3)
        return Built(run, {"out": arena_mask(M, n_out) if direct else full(M, n_out)}, reference)
    return make


for _dt in TDT:
    for _epi in ("bf16", "geglu", "f32"):
        _case(f"gemm_ln-consumer-{_dt}-{_epi}", "gemm_ln", ["vf_gemm_ln"], ["gemm_ln_consumer"], _make_consumer(_dt, _epi))
_case("gemm_ln-consumer-bf16-bf16-direct", "gemm_ln", ["vf_gemm_ln_bf16"], [], _make_consumer("bf16", "bf16", direct=True))


# ---- vf_gemm_ln as producer, vf_gemm_ln_t16, vf_ln_finalize2 ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _producer_operands(dtype):
    M, N, K = 515, 800, 192
    a, w = _rd(_rand((M, K), 301), dtype), _rd(_rand((N, K), 302, 1.0 / math.sqrt(K)), dtype)
    return M, N, K, a, w, _rand((N,), 303, 0.5), _rand((M, N), 304, 3.0) + 0.7


def _make_producer(dtype, res, need_x, need_t16=False):
    """res: "none" | "f32" | "r16" (the 16-bit copy of a stream) | "t16" (the fp16 trunk copy: vf_gemm_ln_t16)."""
    def make():
        M, N, K, a32, w32, b32, res32 = _producer_operands(dtype)
        tdt = TDT[dtype]
        scale = 1.0 if dtype == "bf16" else 2.0 ** -4
        t16_scale = 2.0 ** -4
        if res == "r16":
            r_in = _rd(res32 * scale, dtype)
            r_val = r_in.double() / scale
        elif res == "t16":
            r_in = (res32 * t16_scale).half().float()
            r_val = r_in.double() / t16_scale
        else:
            r_in, r_val = res32, (res32.double() if res == "f32" else None)
        n_parts = N // 32

        def call(ops, a, w, b, r):
            with ops.compute_dtype(tdt):
                if res == "t16":
                    return ops.gemm_ln_producer(a, w, b, None, need_x=need_x, trunk16=r, need_t16=need_t16)
                if res == "r16":
                    r = ops.LnStream(None, r, None, scale)
                return ops.gemm_ln_producer(a, w, b, r, need_x=need_x)

        def run(p):
            ops = _ops()
            a, w, b = guarded(a32.to(tdt), p, GUARD_COLS), guarded(w32.to(tdt), p), guarded(b32, p)
            r = None
            if res != "none":
                r = guarded(r_in.to({"f32": torch.float32, "r16": tdt, "t16": torch.float16}[res]), p, GUARD_COLS)
            with poison_allocations(p) as px:
                s = call(ops, a, w, b, r)
            _sync()
            part = [t for t in px.allocated if t.dim() == 3]
            assert len(part) == 1 and len(px.allocated) == 3 + int(need_x) + int(need_t16)
            bufs = {"x16": s.x16, "stats": s.stats, "part_stats": part[0]}
            if need_x:
                bufs["x"] = s.x
            if need_t16:
                bufs["t16"] = s.t16
            return bufs

        def reference(bufs):
            ops = _ops()
            r = None if res == "none" else r_in.to({"f32": torch.float32, "r16": tdt, "t16": torch.float16}[res]).to(DEVICE)
            if need_x:
                x = bufs["x"]
                want = a32.double() @ w32.double().t() + b32.double() + (0 if r_val is None else r_val)
                _close(x, want, rtol=2e-5, atol=2e-5 * math.sqrt(K))          # ::test_gemm_ln_producer
                assert torch.equal(bufs["x16"], (x * scale).to(tdt))
                xd = x.double()
                _close(bufs["stats"][:, 0], xd.mean(1) * scale, rtol=1e-5, atol=1e-6)
                _close(bufs["stats"][:, 1], 1.0 / torch.sqrt(xd.var(1, unbiased=False) + 1e-5) / scale, rtol=2e-5)
                if need_t16:
                    assert torch.equal(bufs["t16"], (x * t16_scale).half())
            else:                             # the launch without the fp32 store keeps the bits of the one with it
                s = _plain_producer(ops, dtype, res, need_t16, a32, w32, b32, r, scale)
                _sync()
                assert torch.equal(bufs["x16"], s.x16.cpu()) and torch.equal(bufs["stats"], s.stats.cpu())
                if need_t16:
                    assert torch.equal(bufs["t16"], s.t16.cpu())
        written = {"x16": full(M, N), "stats": full(M, 2), "part_stats": full(n_parts, M, 2)}
        if need_x:
            written["x"] = full(M, N)
        if need_t16:
            written["t16"] = full(M, N)
        return Built(run, written, reference)
    return make


def _plain_producer(ops, dtype, res, need_t16, a32, w32, b32, r, scale):
    tdt = TDT[dtype]
    a, w, b = a32.to(tdt).to(DEVICE), w32.to(tdt).to(DEVICE), b32.to(DEVICE)
    with ops.compute_dtype(tdt):
        if res == "t16":
            return ops.gemm_ln_producer(a, w, b, None, need_x=True, trunk16=r, need_t16=need_t16)
        if res == "r16":
            r = ops.LnStream(None, r, None, scale)
        return ops.gemm_ln_producer(a, w, b, r, need_x=True)


for _dt in TDT:
    for _res in ("none", "f32", "r16"):
        for _nx in (True, False):
            _case(f"gemm_ln-producer-{_dt}-res_{_res}-{'x' if _nx else 'nox'}", "gemm_ln", ["vf_gemm_ln", "vf_ln_finalize2"],
                  ["gemm_ln_producer"], _make_producer(_dt, _res, _nx))
    for _nx in (True, False):
        for _nt in (True, False):
            _case(f"gemm_ln-t16-{_dt}-{'x' if _nx else 'nox'}-{'t16' if _nt else 'not16'}", "gemm_ln",
                  ["vf_gemm_ln_t16", "vf_ln_finalize2"], ["gemm_ln_producer"], _make_producer(_dt, "t16", _nx, _nt))


# ---- vf_ln_finalize, vf_row_stats_cast(2), vf_pack_geglu_rows, vf_layernorm, casts ---------------------------------------------
def _stats_ref(x, scale=1.0):
    xd = x.double()
    return xd.mean(1) * scale, 1.0 / torch.sqrt(xd.var(1, unbiased=False) + 1e-5) / scale


def _check_stats(stats, x, scale=1.0):           # tests/test_ops_gpu.py::test_ln_stream_stats_and_copy / test_gemm_ln_producer
    mean, rstd = _stats_ref(x, scale)
    _close(stats[:, 0], mean, rtol=1e-5, atol=1e-6)
    _close(stats[:, 1], rstd, rtol=2e-5)


def _make_ln_finalize():
    def make():
        M, D = 77, 160
        x = _rand((M, D), 341, 2.0) + _rand((M, 1), 342, 1.0)
        parts = x.double().view(M, D // 32, 32)
        pm = parts.mean(-1, keepdim=True)
        part = torch.stack([parts.sum(-1), ((parts - pm) ** 2).sum(-1)], dim=-1).permute(1, 0, 2).contiguous().float()   # [n_parts, M, 2]

        def run(p):
            from variantformer_amd import _lib
            ps = guarded(part.view(-1, 2), p)
            out = poisoned((M, 2), torch.float32, DEVICE, p)
            _lib.check(_lib.load().vf_ln_finalize(ps.data_ptr(), M, D // 32, D, 1e-5, out.data_ptr(), _stream()), "vf_ln_finalize")
            _sync()
            return {"row_stats": out}
        return Built(run, {"row_stats": full(M, 2)}, lambda bufs: _check_stats(bufs["row_stats"], x))
    return make


_case("ln_finalize", "stats", ["vf_ln_finalize"], [], _make_ln_finalize())


def _make_row_stats(dtype, form):
    """form: "ln_stream" (vf_row_stats_cast2 through ops.ln_stream), "trunk16" (ops.trunk16_of), "direct" (vf_row_stats_cast)."""
    def make():
        M, D = 37, 200
        x = _rand((M, D), 351, 2.0) + _rand((M, 1), 352, 1.0)
        tdt = TDT[dtype]
        scale = {"ln_stream": 1.0 if dtype == "bf16" else 2.0 ** -4, "trunk16": 2.0 ** -4, "direct": 1.0}[form]

        def run(p):
            ops = _ops()
            xg = guarded(x, p)
            if form == "direct":
                from variantformer_amd import _lib
                x16, st = poisoned((M, D), tdt, DEVICE, p), poisoned((M, 2), torch.float32, DEVICE, p)
                _lib.check(_lib.load().vf_row_stats_cast(xg.data_ptr(), M, D, 1e-5, x16.data_ptr(), ops._dt(tdt), st.data_ptr(),
                                                         _stream()), "vf_row_stats_cast")
                _sync()
                return {"x16": x16, "stats": st}
            with poison_allocations(p) as px, ops.compute_dtype(tdt):
                if form == "ln_stream":
                    s = ops.ln_stream(xg)
                    bufs = {"x16": s.x16, "stats": s.stats}
                else:
                    t16 = ops.trunk16_of(xg)
                    bufs = {"x16": t16, "stats": [t for t in px.allocated if t.shape == (M, 2)][0]}
            _sync()
            return bufs

        def reference(bufs):
            assert torch.equal(bufs["x16"], (x * scale).to(torch.float16 if form == "trunk16" else tdt))
            # trunk16_of passes eps = 1e-5 and x16_scale = T16_SCALE: its (unused) statistics are the scaled pair too
            _check_stats(bufs["stats"], x, scale)
        return Built(run, {"x16": full(M, D), "stats": full(M, 2)}, reference)
    return make


for _dt in TDT:
    _case(f"row_stats-ln_stream-{_dt}", "stats", ["vf_row_stats_cast2"], ["ln_stream"], _make_row_stats(_dt, "ln_stream"))
    _case(f"row_stats-direct-{_dt}", "stats", ["vf_row_stats_cast"], [], _make_row_stats(_dt, "direct"))
_case("row_stats-trunk16", "stats", ["vf_row_stats_cast2"], ["trunk16_of"], _make_row_stats("bf16", "trunk16"))


def _make_pack_geglu(dtype, with_bias):
    def make():
        two_f, K = 96, 40
        w, b = _rand((two_f, K), 361).to(TDT[dtype]), _rand((two_f,), 362)
        perm = torch.empty(two_f, dtype=torch.long)
        for blk in range(two_f // 32):
            for t in range(16):
                perm[32 * blk + t], perm[32 * blk + 16 + t] = 16 * blk + t, two_f // 2 + 16 * blk + t

        def run(p):
            ops = _ops()
            wg, bg = guarded(w, p), guarded(b, p) if with_bias else None
            with poison_allocations(p):
                wo, bo = ops.pack_geglu_rows(wg, bg)
            _sync()
            return {"W_out": wo, "bias_out": bo} if with_bias else {"W_out": wo}

        def reference(bufs):
            assert torch.equal(bufs["W_out"], w[perm]) and (not with_bias or torch.equal(bufs["bias_out"], b[perm]))
        written = {"W_out": full(two_f, K)}
        if with_bias:
            written["bias_out"] = full(two_f)
        return Built(run, written, reference)
    return make


for _dt in TDT:
    for _wb in (True, False):
        _case(f"pack_geglu-{_dt}-{'bias' if _wb else 'nobias'}", "stream", ["vf_pack_geglu_rows"], ["pack_geglu_rows"],
              _make_pack_geglu(_dt, _wb))


def _make_layernorm(out_dtype, gelu, use_arena):
    def make():
        rows, D = 37, 200
        x = _rand((rows, D), 41, 3.0) + 0.5
        g, b = 1 + 0.1 * _rand((D,), 42), 0.1 * _rand((D,), 43)
        ref = F.layer_norm(x, (D,), g, b, 1e-5)
        ref = F.gelu(ref) if gelu else ref

        def run(p):
            ops = _ops()
            xg, gg, bg = guarded(x, p), guarded(g, p), guarded(b, p)
            if use_arena:
                big, out = arena(rows, D, out_dtype, p, pad_cols=0)
                ops.layernorm(xg, gg, bg, out_dtype, gelu, out=out)
                _sync()
                return {"out": big}
            with poison_allocations(p):
                out = ops.layernorm(xg, gg, bg, out_dtype, gelu)
            _sync()
            return {"out": out}

        def reference(bufs):
            got = bufs["out"][8:8 + rows] if use_arena else bufs["out"]
            if out_dtype == torch.float32:                  # tests/test_ops_gpu.py::test_layernorm
                _close(got, ref, rtol=1e-5, atol=1e-5)
            else:                                           # the fp32 result rounded to nearest even
                o32 = _ops().layernorm(x.to(DEVICE), g.to(DEVICE), b.to(DEVICE), torch.float32, gelu).cpu()
                assert torch.equal(got, o32.to(out_dtype))
        return Built(run, {"out": arena_mask(rows, D, pad_cols=0) if use_arena else full(rows, D)}, reference)
    return make


for _od in (torch.float32, torch.bfloat16, torch.float16):
    for _g in (False, True):
        _case(f"layernorm-{str(_od)[6:]}-{'gelu' if _g else 'plain'}", "stream", ["vf_layernorm"], ["layernorm"],
              _make_layernorm(_od, _g, use_arena=(_od == torch.float32)))


def _make_cast(dtype, n):
    def make():
        x = _rand((n,), 161, 4.0)
        tdt = TDT[dtype]

        def run(p):
            from variantformer_amd import _lib
            xg = guarded(x, p)
            out = poisoned((n + 9,), tdt, DEVICE, p)
            lib = _lib.load()
            fn = lib.vf_cast_f32_f16 if dtype == "fp16" else lib.vf_cast_f32_bf16
            _lib.check(fn(xg.data_ptr(), out.data_ptr(), n, _stream()), "vf_cast_f32_16")
            with poison_allocations(p):
                w = _ops().cast16(xg, tdt)
            _sync()
            return {"out": out, "wrapper_out": w}
        m = torch.zeros(n + 9, dtype=torch.bool)
        m[:n] = True

        def reference(bufs):
            assert torch.equal(bufs["out"][:n], x.to(tdt)) and torch.equal(bufs["wrapper_out"], x.to(tdt))
        return Built(run, {"out": m, "wrapper_out": full(n)}, reference)
    return make


for _dt in TDT:
    for _n in (1, 5, 4099):
        _case(f"cast-{_dt}-n{_n}", "stream", [f"vf_cast_f32_{'bf16' if _dt == 'bf16' else 'f16'}"], ["cast16"], _make_cast(_dt, _n))


# ---- forward attention ----------------------------------------------------------------------------------------------------------
def attn_written_mask(ql, tq: int, H: int, dh: int, n_cols: int) -> torch.Tensor:
    """include/vf_hip.h, vf_attn_varlen_fwd: the output rows of the tokens of every sequence, [0, cu_seqlens_q[n_seq]), are
    written in their first H * dh columns -- zeros where the key sequence is empty; a sequence with 0 queries has no rows;
    rows at or past cu_seqlens_q[n_seq] and columns at or past H * dh are not written."""
    m = torch.zeros((tq, n_cols), dtype=torch.bool)
    m[:sum(ql), :H * dh] = True
    return m


EXTRA_Q_ROWS = 6            # query / output rows past cu_seqlens_q[n_seq]
ATTN_FAMILY_CASES = ("registry", "fwd128_dh48", "short2_1pass_dh64", "short2_2pass_dh48", "short_3groups", "short2_2pass_dh40")
assert {E.CASES_BY_NAME[n].kernel for n in ATTN_FAMILY_CASES} == {c.kernel for c in E.ATTN_EDGE_CASES}


def attn_geometry(name):
    """The edge case's sequences followed by one without queries (3 keys) and one without keys (5 queries)."""
    c = E.CASES_BY_NAME[name]
    return c, list(c.ql) + [0, 5], list(c.kl) + [3, 0]


def _make_attn(name, dtype, q_at_start, entry=None, q_log2=None):
    """entry None: through ops.attn_varlen (vf_attn_varlen_fwd_v2, or _v3 for a padded head dim), out an arena when the
    alignment is flash-attn's and the wrapper's own allocation otherwise; else the named pre-ABI-4 entry, called directly."""
    def make():
        c, ql, kl = attn_geometry(name)
        ql2 = c.q_log2[0] if q_log2 is None else q_log2
        H, dh, D = c.H, c.dh, c.H * c.dh
        tdt = TDT[dtype]
        q0, k0, v0 = E.operands(c.name, dtype, ql2)
        n0 = q0.shape[0]
        tq, tk = sum(ql) + EXTRA_Q_ROWS, sum(kl)
        q = torch.cat([q0, _rd(_rand((tq - n0, D), c.seed + 7, 0.4), dtype)])
        k = torch.cat([k0, _rd(_rand((tk - k0.shape[0], D), c.seed + 8, 2.0), dtype)])
        v = torch.cat([v0, _rd(_rand((tk - v0.shape[0], D), c.seed + 9, 2.0), dtype)])
        use_arena = entry is not None or not q_at_start

        def run(p):
            ops = _ops()
            dq, dk, dv = (guarded(t.to(tdt), p, GUARD_COLS) for t in (q, k, v))
            cu_q, cu_k, sl = guarded(E.cu_of(ql), p), guarded(E.cu_of(kl), p), guarded(E.slopes_of(c), p)
            if use_arena:
                big, out = arena(tq, D, tdt, p)
            if entry is None:
                with poison_allocations(p):
                    got = ops.attn_varlen(dq, dk, dv, cu_q, cu_k, max(ql), max(kl), H, dh, sl, out=out if use_arena else None,
                                          q_at_start=q_at_start, q_log2=ql2)
            else:
                from variantformer_amd import _lib
                fn = getattr(_lib.load(), entry)
                _lib.check(fn(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), out.data_ptr(), dq.stride(0), dk.stride(0), dv.stride(0),
                              out.stride(0), cu_q.data_ptr(), cu_k.data_ptr(), len(ql), max(ql), max(kl), H, dh, sl.data_ptr(),
                              1.0 / math.sqrt(dh), _stream()), entry)
            kernel = ops.last_kernel("attn")
            assert kernel == c.kernel, kernel
            _sync()
            return {"out": big if use_arena else got}

        def reference(bufs):
            got = (bufs["out"][8:8 + tq, GUARD_COLS:GUARD_COLS + D] if use_arena else bufs["out"]).float()
            want = O.Rounding(dtype).r(E.oracle_rows(c, dtype, ql2, q_at_start))
            np.testing.assert_allclose(got[:n0].numpy(), want.numpy(), **E.tolerance(dtype))
            cu = E.cu_of(ql)
            for b, sk in enumerate(kl):                       # flash-attn's convention: no keys, zero rows
                if sk == 0 and ql[b]:
                    assert float(got[int(cu[b]):int(cu[b + 1])].abs().max()) == 0.0
        inner = attn_written_mask(ql, tq, H, dh, D)
        return Built(run, {"out": arena_mask(tq, D, inner) if use_arena else inner}, reference)
    return make


for _n in ATTN_FAMILY_CASES:
    for _dt in TDT:
        for _qs in (False, True):
            _ent = "vf_attn_varlen_fwd_v3" if E.CASES_BY_NAME[_n].dh not in (32, 48, 64, 96, 128) else "vf_attn_varlen_fwd_v2"
            _case(f"attn-{_n}-{_dt}-{'qstart' if _qs else 'qend'}", "attn", [_ent], ["attn_varlen"], _make_attn(_n, _dt, _qs))
for _ent, _dt, _qs in (("vf_attn_varlen_fwd", "bf16", False), ("vf_attn_varlen_fwd_qstart", "bf16", True),
                       ("vf_attn_varlen_fwd_f16", "fp16", False), ("vf_attn_varlen_fwd_qstart_f16", "fp16", True)):
    _case(f"attn-direct-{_ent}", "attn", [_ent], [], _make_attn("fwd64_dh48", _dt, _qs, entry=_ent, q_log2=False))


def _make_attn_padded(name, dtype):
    """The family's case at head dim dh - 8 (vf_attn_varlen_fwd_v3: the kernels of class dh, told the true head dim): the
    operands are the case's with the last 8 columns of every head dropped.  Reference, from the header: bit for bit the class-dh
    call on operands zero-padded per head, same scale and flags -- which the case above holds to the oracle's tolerance on the
    unpadded operands."""
    def make():
        c, ql, kl = attn_geometry(name)
        ql2 = c.q_log2[0]
        H, dh = c.H, c.dh
        dp = dh - 8
        D, Dp = H * dh, H * dp
        tdt = TDT[dtype]
        q0, k0, v0 = E.operands(c.name, dtype, ql2)
        tq, tk = sum(ql) + EXTRA_Q_ROWS, sum(kl)
        full_ops = [torch.cat([q0, _rd(_rand((tq - q0.shape[0], D), c.seed + 7, 0.4), dtype)]),
                    torch.cat([k0, _rd(_rand((tk - k0.shape[0], D), c.seed + 8, 2.0), dtype)]),
                    torch.cat([v0, _rd(_rand((tk - v0.shape[0], D), c.seed + 9, 2.0), dtype)])]
        cut = [t.view(-1, H, dh)[:, :, :dp].reshape(-1, Dp).contiguous() for t in full_ops]
        scale = 1.0 / math.sqrt(dh)

        def run(p):
            ops = _ops()
            dq, dk, dv = (guarded(t.to(tdt), p, GUARD_COLS) for t in cut)
            cu_q, cu_k, sl = guarded(E.cu_of(ql), p), guarded(E.cu_of(kl), p), guarded(E.slopes_of(c), p)
            big, out = arena(tq, Dp, tdt, p)
            with poison_allocations(p):
                ops.attn_varlen(dq, dk, dv, cu_q, cu_k, max(ql), max(kl), H, dp, sl, scale=scale, out=out, q_log2=ql2)
            kernel = ops.last_kernel("attn")
            assert kernel == c.kernel, kernel
            _sync()
            return {"out": big}

        def reference(bufs):
            ops = _ops()
            padded = []
            for t in cut:
                z = torch.zeros((t.shape[0], H, dh))
                z[:, :, :dp] = t.view(-1, H, dp)
                padded.append(z.view(-1, D).to(tdt).to(DEVICE))
            want = ops.attn_varlen(*padded, E.cu_of(ql).to(DEVICE), E.cu_of(kl).to(DEVICE), max(ql), max(kl), H, dh,
                                   E.slopes_of(c).to(DEVICE), scale=scale, q_log2=ql2)
            _sync()
            n = sum(ql)
            want = want.cpu()[:n].view(n, H, dh)[:, :, :dp].reshape(n, Dp)
            got = bufs["out"][8:8 + n, GUARD_COLS:GUARD_COLS + Dp]
            assert torch.equal(got.view(torch.int16), want.contiguous().view(torch.int16))
        return Built(run, {"out": arena_mask(tq, Dp, attn_written_mask(ql, tq, H, dp, Dp))}, reference)
    return make


for _n in ATTN_FAMILY_CASES:
    if E.CASES_BY_NAME[_n].dh in (32, 48, 64, 96, 128):
        for _dt in TDT:
            _case(f"attn-{_n}-{_dt}-padded_dh{E.CASES_BY_NAME[_n].dh - 8}", "attn", ["vf_attn_varlen_fwd_v3"], ["attn_varlen"],
                  _make_attn_padded(_n, _dt))


def _make_attn_rows(dtype, alibi):
    """vf_attn_varlen_fwd_rows: q / k / v tables with poisoned rows between the named ones; reference = the plain entry on the
    gathered rows, bit for bit (the header's statement; tests/test_ops_gpu.py holds that call to the oracle)."""
    def make():
        H, dh = (32, 48) if alibi else (8, 64)      # the geometries of tests/test_ops_gpu.py's row-map test
        D = H * dh
        # (the dh 64 row-map kernel serves batches of >= 128 sequences x 8 heads only: vf_attn_rows_supported)
        lens = [129, 17, 201, 1, 64] if alibi else [200, 129, 7, 1] * 33
        T, n_tab = sum(lens), 150
        tdt = TDT[dtype]
        tab = _rand((n_tab, 3 * D), 71, 1.5).to(tdt)
        rows = torch.randint(0, n_tab, (T,), generator=torch.Generator().manual_seed(72))
        rows[:7] = rows[0]
        slopes = torch.tensor(O.alibi_slopes(H), dtype=torch.float32) if alibi else None

        def run(p):
            ops = _ops()
            t, where = spread_rows(tab, p, GUARD_COLS)
            r = guarded(where[rows].contiguous(), p)
            cu = guarded(E.cu_of(lens), p)
            sl = None if slopes is None else guarded(slopes, p)
            assert ops.attn_rows_supported(dh, alibi, len(lens), H, max(lens), max(lens), True)
            with poison_allocations(p):
                out = ops.attn_varlen(t[:, :D], t[:, D:2 * D], t[:, 2 * D:], cu, None, max(lens), max(lens), H, dh, sl, q_log2=True,
                                      rows=r)
            _sync()
            return {"out": out}

        def reference(bufs):
            ops = _ops()
            g = tab[rows].to(DEVICE)
            want = ops.attn_varlen(g[:, :D], g[:, D:2 * D], g[:, 2 * D:], E.cu_of(lens).to(DEVICE), None, max(lens), max(lens), H, dh,
                                   None if slopes is None else slopes.to(DEVICE), q_log2=True)
            _sync()
            assert torch.equal(bufs["out"].view(torch.int16), want.cpu().view(torch.int16))
            assert torch.isfinite(bufs["out"].float()).all()
        return Built(run, {"out": full(T, D)}, reference)
    return make


for _dt in TDT:
    for _al in (False, True):
        _case(f"attn_rows-{_dt}-{'alibi_dh48' if _al else 'dh64'}", "attn", ["vf_attn_varlen_fwd_rows"], ["attn_varlen"],
              _make_attn_rows(_dt, _al))


def _make_counted_keys(dtype):
    def make():
        H, dh, C = 8, 64, 9
        D = H * dh
        lens = [300, 1, 0, 77, 5]
        tq = sum(lens)
        rnd = O.Rounding(dtype)
        cu = E.cu_of(lens)
        labels = torch.from_numpy(np.random.default_rng(3).integers(0, C, tq)).long()
        labels[int(cu[3]):int(cu[4])] = 4
        q = rnd.r(_rand((tq + EXTRA_Q_ROWS, D), 81, 1.2))
        tab = rnd.r(_rand((C, 2 * D), 82, 1.5))
        cnt = torch.zeros(len(lens), C)
        for b in range(len(lens)):
            cnt[b] = torch.bincount(labels[int(cu[b]):int(cu[b + 1])], minlength=C).float()
        cnt[2, 0] = 1                       # (every sequence holds >= 1 key: the header's precondition, also for the one without queries)
        tdt = TDT[dtype]

        def run(p):
            ops = _ops()
            with poison_allocations(p):
                out = ops.attn_counted_keys(guarded(q.to(tdt), p, GUARD_COLS), guarded(tab.to(tdt), p, GUARD_COLS),
                                            guarded(torch.log2(cnt), p), guarded(cu, p), max(lens), H, dh)
            _sync()
            return {"out": out}

        def reference(bufs):                # tests/test_ops_gpu.py::test_attention_counted_keys_matches_oracle_and_the_expanded_form
            ref = torch.zeros(tq, D)
            for b in range(len(lens)):
                a, e = int(cu[b]), int(cu[b + 1])
                if e > a:
                    present = [c for c in range(C) if cnt[b, c] > 0]
                    ref[a:e] = O.attention_counted(q[a:e].view(-1, H, dh), tab[present, :D].view(-1, H, dh),
                                                   tab[present, D:].view(-1, H, dh), cnt[b, present], True).reshape(e - a, D)
            ulp = 2 ** -7 if dtype == "bf16" else 2 ** -10
            np.testing.assert_allclose(bufs["out"][:tq].float().numpy(), rnd.r(ref).numpy(), rtol=ulp, atol=ulp * 1e-2)
        m = full(tq + EXTRA_Q_ROWS, D)
        m[tq:] = False                      # vf_hip.h: rows at or past cu_seqlens_q[n_seq] are not written
        return Built(run, {"out": m}, reference)
    return make


def _make_softmax_counted(dtype, direct):
    def make():
        H, Cp, C = 32, 10, 9
        lens = [70, 1, 0, 33, 130]
        T = sum(lens)
        cu = E.cu_of(lens)
        sc = _rand((T + EXTRA_Q_ROWS, H * Cp), 96, 4.0)
        cnt = torch.from_numpy(np.random.default_rng(2).integers(0, 50, (len(lens), C))).float()
        cnt[1] = 0
        cnt[1, 4] = 1
        cnt[3, 0] = 0
        tdt = TDT[dtype]
        rnd = O.Rounding(dtype)

        def run(p):
            ops = _ops()
            scg, lc, cug = guarded(sc, p, GUARD_COLS), guarded(torch.log2(cnt), p), guarded(cu, p)
            if direct:
                from variantformer_amd import _lib
                big, out = arena(T + EXTRA_Q_ROWS, H * Cp, tdt, p)
                _lib.check(_lib.load().vf_softmax_counted(scg.data_ptr(), scg.stride(0), lc.data_ptr(), cug.data_ptr(), len(lens),
                                                          max(lens), H, Cp, C, out.data_ptr(), out.stride(0), ops._dt(tdt), _stream()),
                           "vf_softmax_counted")
                _sync()
                return {"out": big}
            with poison_allocations(p):
                out = ops.softmax_counted(scg, lc, cug, max(lens), H, Cp, out_dtype=tdt)
            _sync()
            return {"out": out}

        def reference(bufs):                # tests/test_ops_gpu.py::test_lowrank_context_attention_pieces
            got = (bufs["out"][8:8 + T, GUARD_COLS:GUARD_COLS + H * Cp] if direct else bufs["out"][:T]).float()
            ref = torch.zeros(T, H, Cp)
            for bb in range(len(lens)):
                a, e = int(cu[bb]), int(cu[bb + 1])
                if e > a:
                    t = sc[a:e].view(-1, H, Cp)[:, :, :C] + torch.log2(cnt[bb])[None, None, :]
                    pr = torch.exp2(t - t.max(dim=-1, keepdim=True).values)
                    ref[a:e, :, :C] = pr / pr.sum(dim=-1, keepdim=True)
            ulp = 2 ** -7 if dtype == "bf16" else 2 ** -10
            np.testing.assert_allclose(got.numpy(), rnd.r(ref.view(T, -1)).numpy(), rtol=ulp, atol=1e-7)
            assert float(got.view(T, H, Cp)[:, :, C:].abs().max()) == 0.0          # slots c >= C are written, as 0
        inner = full(T + EXTRA_Q_ROWS, H * Cp)
        inner[T:] = False                   # rows at or past cu_seqlens_q[n_seq]; columns past H * Cp are the arena's frame
        return Built(run, {"out": arena_mask(T + EXTRA_Q_ROWS, H * Cp, inner) if direct else inner}, reference)
    return make


for _dt in TDT:
    _case(f"counted_keys-{_dt}", "attn", ["vf_attn_counted_keys"], ["attn_counted_keys"], _make_counted_keys(_dt))
    for _d in (False, True):
        _case(f"softmax_counted-{_dt}-{'wide_out' if _d else 'wrapper'}", "attn", ["vf_softmax_counted"],
              [] if _d else ["softmax_counted"], _make_softmax_counted(_dt, _d))


# ---- vf_attn_probs / _v2 ----------------------------------------------------------------------------------------------------
PROBS_EXTRA_COLS = 5


def _make_probs(dtype, per_head, form):
    """form: "plain" (ops.attn_probs without bias: vf_attn_probs_v2 with the three new pointers NULL), "alibi" (slopes, q_pos and a
    key row map), "v1" (vf_attn_probs, called directly).  The planted-direction operands of tests/test_attn_probs_gpu.py."""
    def make():
        from tests import attn_probs_alibi_cases as A
        H, dh = 8, 64
        case = (A.AlibiCase if form == "alibi" else A.Case)(H, dh, dtype, True)
        D, R = case.D, case.R
        max_k = max(case.kl)
        q16, qsel = case.queries(True)
        n_out = R * (H if per_head else 1)
        k16 = case.k16[:, :D].contiguous()

        def run(p):
            ops = _ops()
            dq, qr = guarded(q16[:, :D].contiguous(), p, GUARD_COLS), guarded(case.q_rows, p)
            cu_rows, cu_k = guarded(case.cu_rows, p), guarded(case.cu_k, p)
            big, out = arena(n_out, max_k + PROBS_EXTRA_COLS, torch.float32, p)
            if form == "v1":
                from variantformer_amd import _lib
                dk = guarded(k16, p, GUARD_COLS)
                stats = poisoned((R, H, 2), torch.float32, DEVICE, p)
                _lib.check(_lib.load().vf_attn_probs(dq.data_ptr(), dq.stride(0), dk.data_ptr(), dk.stride(0), qr.data_ptr(),
                                                     cu_rows.data_ptr(), cu_k.data_ptr(), len(case.kl), max(case.rl), max_k, H, dh,
                                                     case.scale, ops._dt(TDT[dtype]), ops.ATTN_Q_LOG2, int(per_head), stats.data_ptr(),
                                                     out.data_ptr(), out.stride(0), _stream()), "vf_attn_probs")
            else:
                kw = {}
                if form == "alibi":
                    dk, where = spread_rows(k16, p, GUARD_COLS)
                    kw = dict(slopes=guarded(case.slopes, p), q_pos=guarded(case.q_pos, p), k_rows=guarded(where.contiguous(), p))
                else:
                    dk = guarded(k16, p, GUARD_COLS)
                with poison_allocations(p):
                    _, stats = ops.attn_probs(dq, dk, cu_rows, cu_k, max(case.rl), max_k, H, dh, q_rows=qr, q_log2=True,
                                              per_head=per_head, scale=case.scale, out=out, **kw)
            assert ops.last_kernel("attn") == ("attn_probs_alibi_kernel" if form == "alibi" else "attn_probs_kernel")
            _sync()
            return {"out": big, "stats": stats}

        def reference(bufs):
            P64, lse64 = case.reference(qsel)
            body = bufs["out"][8:8 + n_out, GUARD_COLS:GUARD_COLS + max_k]
            got = body.view(R, H, max_k) if per_head else body
            for s, n in enumerate(case.kl):
                a, e = int(case.cu_rows[s]), int(case.cu_rows[s + 1])
                assert torch.all(got[a:e][..., n:] == 0.0), f"sequence {s}: columns past its {n} keys are not zero"
            err = A.prob_err(got, P64 if per_head else P64.mean(dim=1))
            assert err <= (A.P_TOL if form == "alibi" else A.P_TOL_PLAIN), err
            has_keys = A.rows_with_keys(case)
            assert torch.all(bufs["stats"][~has_keys] == 0.0)                     # a row without keys: stats (0, 0)
            if form != "alibi":               # tests/test_attn_probs_gpu.py::test_probs_against_float64
                lse = bufs["stats"][..., 0].double() + torch.log2(bufs["stats"][..., 1].double())
                assert float((lse - lse64)[has_keys].abs().max()) < 1e-4 * max(1.0, float(lse64.abs().max()))
        inner = torch.zeros((n_out, max_k + PROBS_EXTRA_COLS), dtype=torch.bool)
        inner[:, :max_k] = True             # every selected row belongs to a sequence; columns >= max_seqlen_k are not touched
        return Built(run, {"out": arena_mask(n_out, max_k + PROBS_EXTRA_COLS, inner), "stats": full(R, H, 2)}, reference)
    return make


for _dt in TDT:
    for _ph in (False, True):
        for _form, _ent in (("plain", "vf_attn_probs_v2"), ("alibi", "vf_attn_probs_v2"), ("v1", "vf_attn_probs")):
            _case(f"attn_probs-{_form}-{_dt}-{'per_head' if _ph else 'head_mean'}", "attn_probs", [_ent],
                  [] if _form == "v1" else ["attn_probs"], _make_probs(_dt, _ph, _form))


# ---- embedding, token keys, cu_seqlens -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _windows():
    W, L, V, d = 9, 70, 50, 136
    g = torch.Generator().manual_seed(17)
    ids = torch.randint(0, V, (W, L), generator=g)
    ids[1, 3], ids[1, 4], ids[3, 69] = -5, V, V + 1000            # clamped to [0, vocab)
    pad = torch.rand((W, L), generator=g) < 0.4
    pad[0] = True
    pad[0, 7] = False
    pad[1] = False
    pad[2] = True                                                 # an empty window
    pad[3, 69] = False
    lens = (~pad).sum(1)
    cu = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).to(torch.int32)
    table, pos = _rand((V, d), 18, 2.0), _rand((L, d), 19)
    return W, L, V, d, ids, pad, cu, table, pos


def _embed_ref(with_pos):
    W, L, V, d, ids, pad, cu, table, pos = _windows()
    x = table[ids.clamp(0, V - 1)]
    if with_pos:
        x = x + pos[None]
    return x[~pad]


def _make_mask_to_cu():
    def make():
        W, L, V, d, ids, pad, cu, table, pos = _windows()

        def run(p):
            with poison_allocations(p):
                out = _ops().mask_to_cu_seqlens(guarded(pad.view(torch.uint8), p))
            _sync()
            return {"cu": out}
        return Built(run, {"cu": full(W + 1)}, lambda bufs: _assert_equal(bufs["cu"], cu))
    return make


def _assert_equal(a, b):
    assert torch.equal(a, b)


def _make_embed_pack(with_pos):
    def make():
        W, L, V, d, ids, pad, cu, table, pos = _windows()
        n = int(cu[-1])

        def run(p):
            with poison_allocations(p):
                out = _ops().embed_pack(guarded(ids, p), guarded(pad.view(torch.uint8), p), guarded(cu, p), guarded(table, p),
                                        guarded(pos, p) if with_pos else None, n)
            _sync()
            return {"out": out}
        return Built(run, {"out": full(n, d)}, lambda bufs: _assert_equal(bufs["out"], _embed_ref(with_pos)))     # one fp32 add
    return make


def _make_embed_stream(dtype, need_x, need_t16, with_pos):
    def make():
        W, L, V, d, ids, pad, cu, table, pos = _windows()
        n = int(cu[-1])
        tdt = TDT[dtype]
        scale = 1.0 if dtype == "bf16" else 2.0 ** -4

        def run(p):
            ops = _ops()
            with poison_allocations(p), ops.compute_dtype(tdt):
                s = ops.embed_stream(guarded(ids, p), guarded(pad.view(torch.uint8), p), guarded(cu, p), guarded(table, p),
                                     guarded(pos, p) if with_pos else None, n, need_x=need_x, need_t16=need_t16)
            _sync()
            bufs = {"x16": s.x16, "stats": s.stats}
            if need_x:
                bufs["x"] = s.x
            if need_t16:
                bufs["t16"] = s.t16
            return bufs

        def reference(bufs):                # tests/test_ops_gpu.py::test_embed_stream_equals_embed_pack_then_stream_passes
            x = _embed_ref(with_pos)
            assert torch.equal(bufs["x16"], (x * scale).to(tdt))
            _check_stats(bufs["stats"], x, scale)
            assert not need_x or torch.equal(bufs["x"], x)
            assert not need_t16 or torch.equal(bufs["t16"], (x * 2.0 ** -4).half())
        written = {"x16": full(n, d), "stats": full(n, 2)}
        if need_x:
            written["x"] = full(n, d)
        if need_t16:
            written["t16"] = full(n, d)
        return Built(run, written, reference)
    return make


def _make_token_keys(with_pos):
    def make():
        W, L, V, d, ids, pad, cu, table, pos = _windows()
        n = int(cu[-1])
        key_L = L if with_pos else 1
        want = torch.tensor([min(max(int(ids[w, q]), 0), V - 1) * key_L + (q if with_pos else 0)
                             for w in range(W) for q in range(L) if not pad[w, q]], dtype=torch.int64)

        def run(p):
            with poison_allocations(p):
                out = _ops().token_keys(guarded(ids, p), guarded(pad.view(torch.uint8), p), guarded(cu, p), n, V, key_L)
            _sync()
            return {"keys": out}
        return Built(run, {"keys": full(n)}, lambda bufs: _assert_equal(bufs["keys"], want))
    return make


_case("mask_to_cu_seqlens", "stream", ["vf_mask_to_cu_seqlens"], ["mask_to_cu_seqlens"], _make_mask_to_cu())
for _wp in (True, False):
    _case(f"embed_pack-{'pos' if _wp else 'nopos'}", "stream", ["vf_embed_pack"], ["embed_pack"], _make_embed_pack(_wp))
    _case(f"token_keys-{'pos' if _wp else 'ids'}", "stream", ["vf_token_keys"], ["token_keys"], _make_token_keys(_wp))
for _dt in TDT:
    for _nx in (True, False):
        for _nt in (True, False):
            _case(f"embed_stream-{_dt}-{'x' if _nx else 'nox'}-{'t16' if _nt else 'not16'}", "stream", ["vf_embed_stream"],
                  ["embed_stream"], _make_embed_stream(_dt, _nx, _nt, with_pos=_nx == _nt))


# ---- segment pools ------------------------------------------------------------------------------------------------------------
SEG_LENS = [3, 1, 200, 0, 77]           # an empty window: NaN (mean: the reference's 0 / 0), -inf (max), lin_b (linear)


def _make_segment_mean(out_dtype):
    def make():
        d = 136
        cu = E.cu_of(SEG_LENS)
        x = _rand((sum(SEG_LENS), d), 51, 2.0)
        nan_ok = torch.zeros((len(SEG_LENS), d), dtype=torch.bool)
        nan_ok[3] = True                # vf_hip.h, vf_segment_mean: "NaN if the window is empty, as the reference's 0/0"

        def run(p):
            with poison_allocations(p):
                out = _ops().segment_mean(guarded(x, p), guarded(cu, p), out_dtype)
            _sync()
            return {"out": out}

        def reference(bufs):            # tests/test_ops_gpu.py::test_segment_mean
            ops = _ops()
            o32 = bufs["out"] if out_dtype == torch.float32 else ops.segment_mean(x.to(DEVICE), cu.to(DEVICE), torch.float32).cpu()
            for w, n in enumerate(SEG_LENS):
                a = int(cu[w])
                if n == 0:
                    assert torch.isnan(bufs["out"][w].float()).all()
                else:
                    np.testing.assert_allclose(o32[w].numpy(), x[a:a + n].sum(0).numpy() / n, rtol=1e-5, atol=1e-6)
            ok = ~torch.isnan(o32)
            assert torch.equal(bufs["out"][ok], o32.to(out_dtype)[ok])
        return Built(run, {"out": full(len(SEG_LENS), d)}, reference, {"out": nan_ok})
    return make


def _make_segment_mean16(dtype, split):
    def make():
        d = 136
        lens = [200, 1, 3, 0, 65, 7]
        cu = E.cu_of(lens)
        tdt = TDT[dtype]
        x = _rand((sum(lens), d), 81, 3.0).to(tdt)
        scale = 16.0
        n_cols = 2 * d if split else d
        nan_ok = torch.zeros((len(lens), n_cols), dtype=torch.bool)
        nan_ok[3] = True                # the same masked mean: an empty window is 0 / 0

        def run(p):
            with poison_allocations(p):
                out = _ops().segment_mean16(guarded(x, p, GUARD_COLS), guarded(cu, p), in_scale=scale, split=split)
            _sync()
            return {"out": out}

        def reference(bufs):            # tests/test_ops_gpu.py::test_segment_mean16_vs_float64
            out = bufs["out"]
            for w, ln in enumerate(lens):
                a = int(cu[w])
                if ln == 0:
                    assert torch.isnan(out[w].float()).all()
                    continue
                ref = x[a:a + ln].double().mean(dim=0) * scale
                tol = float(ref.abs().max())
                if split:
                    assert float((out[w, :d].double() + out[w, d:].double() - ref).abs().max()) <= 2 ** -15 * tol
                else:
                    assert float((out[w].double() - ref).abs().max()) <= 2e-6 * tol + 1e-30
        return Built(run, {"out": full(len(lens), n_cols)}, reference, {"out": nan_ok})
    return make


def _make_segment_max():
    def make():
        d = 136
        cu = E.cu_of(SEG_LENS)
        x = -(_rand((sum(SEG_LENS), d), 111).abs() * 3.0 + 0.01)

        def run(p):
            with poison_allocations(p):
                out = _ops().segment_max(guarded(x, p), guarded(cu, p))
            _sync()
            return {"out": out}

        def reference(bufs):            # tests/test_ops_edges_gpu.py::test_segment_max
            for w, n in enumerate(SEG_LENS):
                a = int(cu[w])
                assert torch.equal(bufs["out"][w], x[a:a + n].max(dim=0).values if n else torch.full((d,), float("-inf"))), w
        return Built(run, {"out": full(len(SEG_LENS), d)}, reference)
    return make


def _make_segment_linear(out_dtype, with_b):
    def make():
        W, L, V, d, ids, pad, cu, table, pos = _windows()
        n = int(cu[-1])
        x = _rand((n, d), 121, 2.0)
        lin_w, lin_b = _rand((L,), 122), torch.tensor([0.37])
        keep = ~pad
        dense = torch.zeros((W, L, d), dtype=torch.float64)
        dense[keep] = x.double()
        bias = 0.37 if with_b else 0.0
        want = torch.einsum("wld,l->wd", dense, lin_w.double()) + bias
        bound = L * 2.0 ** -24 * (torch.einsum("wld,l->wd", dense.abs(), lin_w.double().abs()) + 0.37)

        def call(ops, xx, cc, pp, ww, bb, od):
            return ops.segment_linear(xx, cc, pp, ww, bb if with_b else None, od)

        def run(p):
            with poison_allocations(p):
                out = call(_ops(), guarded(x, p), guarded(cu, p), guarded(pad.view(torch.uint8), p), guarded(lin_w, p),
                           guarded(lin_b, p), out_dtype)
            _sync()
            return {"out": out}

        def reference(bufs):            # tests/test_ops_edges_gpu.py::test_segment_linear
            o32 = bufs["out"] if out_dtype == torch.float32 else call(_ops(), x.to(DEVICE), cu.to(DEVICE), pad.to(DEVICE).view(torch.uint8),
                                                                     lin_w.to(DEVICE), lin_b.to(DEVICE), torch.float32).cpu()
            err = (o32.double() - want).abs()
            assert bool((err <= 1e-6 * want.abs() + bound).all()), float((err - bound).max())
            assert torch.equal(o32[2], torch.full((d,), bias))                    # the empty window: lin_b alone
            assert torch.equal(bufs["out"], o32.to(out_dtype))
        return Built(run, {"out": full(W, d)}, reference)
    return make


for _od in (torch.float32, torch.bfloat16, torch.float16):
    _case(f"segment_mean-{str(_od)[6:]}", "stream", ["vf_segment_mean"], ["segment_mean"], _make_segment_mean(_od))
    _case(f"segment_linear-{str(_od)[6:]}", "stream", ["vf_segment_linear"], ["segment_linear"],
          _make_segment_linear(_od, with_b=_od != torch.float16))
for _dt in TDT:
    for _sp in (False, True):
        _case(f"segment_mean16-{_dt}-{'split' if _sp else 'f32'}", "stream", ["vf_segment_mean16"], ["segment_mean16"],
              _make_segment_mean16(_dt, _sp))
_case("segment_max", "stream", ["vf_segment_max"], ["segment_max"], _make_segment_max())


# ---- row movers -----------------------------------------------------------------------------------------------------------------
def _make_gather_f32(out_dtype, d):
    def make():
        a, b = _rand((50, d), 171), _rand((9, d), 172)
        idx = torch.tensor([0, 49, -1, -9, 7, 7, -3, 48], dtype=torch.int64)
        want = torch.stack([a[i] if i >= 0 else b[-i - 1] for i in idx.tolist()]).to(out_dtype)

        def run(p):
            with poison_allocations(p):
                out = _ops().gather_rows_f32(guarded(a, p), guarded(b, p), guarded(idx, p), out_dtype)
            _sync()
            return {"out": out}
        return Built(run, {"out": full(idx.numel(), d)}, lambda bufs: _assert_equal(bufs["out"], want))
    return make


def _make_gather16(dtype):
    def make():
        d = 136
        src = _rand((9, d), 181).to(TDT[dtype])
        idx = torch.tensor([8, 0, 0, 3, 5, 8, 1], dtype=torch.int64)

        def run(p):
            ops = _ops()
            from variantformer_amd import _lib
            tab, where = spread_rows(src, p, GUARD_COLS)
            di = guarded(where[idx].contiguous(), p)
            big, out = arena(idx.numel(), d, TDT[dtype], p)
            _lib.check(_lib.load().vf_gather_rows_bf16(tab.data_ptr(), tab.stride(0), di.data_ptr(), out.data_ptr(), out.stride(0),
                                                       idx.numel(), d, _stream()), "vf_gather_rows_bf16")
            with poison_allocations(p):
                w = ops.gather_rows_bf16(tab, di)
            _sync()
            return {"out": big, "wrapper_out": w}

        def reference(bufs):
            assert torch.equal(bufs["out"][8:8 + idx.numel(), GUARD_COLS:GUARD_COLS + d], src[idx])
            assert torch.equal(bufs["wrapper_out"], src[idx])
        return Built(run, {"out": arena_mask(idx.numel(), d), "wrapper_out": full(idx.numel(), d)}, reference)
    return make


def _make_add_rows(use_a, use_b):
    def make():
        d, n = 136, 41
        ra, rb = (19 if use_a else n), (7 if use_b else n)
        a, b = _rand((ra, d), 141, 2.0), _rand((rb, d), 142, 2.0)
        ia = torch.randint(0, ra, (n,), generator=torch.Generator().manual_seed(143)) if use_a else None
        ib = torch.randint(0, rb, (n,), generator=torch.Generator().manual_seed(144)) if use_b else None
        want = (a[ia] if use_a else a) + (b[ib] if use_b else b)

        def run(p):
            with poison_allocations(p):
                out = _ops().add_rows(guarded(a, p), guarded(b, p), None if ia is None else guarded(ia, p),
                                      None if ib is None else guarded(ib, p))
            _sync()
            return {"out": out}
        return Built(run, {"out": full(n, d)}, lambda bufs: _assert_equal(bufs["out"], want))     # one fp32 add
    return make


def _make_affine_rows(use_scale, use_shift):
    def make():
        d, n, rows = 136, 37, 23
        src = _rand((rows, d), 131, 2.0)
        idx = torch.randint(0, rows, (n,), generator=torch.Generator().manual_seed(132))
        scale = _rand((n,), 133, 3.0) if use_scale else None
        shift = _rand((n,), 134, 3.0) if use_shift else None

        def run(p):
            with poison_allocations(p):
                out = _ops().affine_rows(guarded(src, p), guarded(idx, p), None if scale is None else guarded(scale, p),
                                         None if shift is None else guarded(shift, p))
            _sync()
            return {"out": out}

        def reference(bufs):            # tests/test_ops_edges_gpu.py::test_affine_rows
            g = src[idx]
            if use_scale and use_shift:
                want = g.double() * scale.double()[:, None] + shift.double()[:, None]
                ulp = torch.from_numpy(np.spacing(np.abs(want.float().numpy()))).double()
                assert bool(((bufs["out"].double() - want).abs() <= ulp).all())
            else:
                assert torch.equal(bufs["out"], g * scale[:, None] if use_scale else (g + shift[:, None] if use_shift else g))
        return Built(run, {"out": full(n, d)}, reference)
    return make


def _make_rowdot(softplus, use_b):
    def make():
        n, d = 5, 136
        x = _rand((n, d), 151, 0.5)
        x[3] *= 30
        w, b = _rand((d,), 152, 0.05), torch.tensor([0.25])
        y = x.double() @ w.double() + (0.25 if use_b else 0.0)
        want = F.softplus(y) if softplus else y

        def run(p):
            with poison_allocations(p):
                out = _ops().rowdot_softplus(guarded(x, p), guarded(w, p), guarded(b, p) if use_b else None, softplus=softplus)
            _sync()
            return {"out": out}
        return Built(run, {"out": full(n, 1)},              # tests/test_ops_gpu.py::test_rowdot_softplus
                     lambda bufs: _close(bufs["out"][:, 0], want, rtol=1e-5, atol=1e-5))
    return make


for _od in (torch.float32, torch.bfloat16, torch.float16):
    _case(f"gather_rows_f32-{str(_od)[6:]}", "stream", ["vf_gather_rows_f32"], ["gather_rows_f32"], _make_gather_f32(_od, 136))
_case("gather_rows_f32-narrow", "stream", ["vf_gather_rows_f32"], ["gather_rows_f32"], _make_gather_f32(torch.float32, 2))
for _dt in TDT:
    _case(f"gather_rows16-{_dt}", "stream", ["vf_gather_rows_bf16"], ["gather_rows_bf16"], _make_gather16(_dt))
for _a, _b in ((False, False), (True, False), (False, True), (True, True)):
    _case(f"add_rows-{int(_a)}{int(_b)}", "stream", ["vf_add_rows_f32"], ["add_rows"], _make_add_rows(_a, _b))
    _case(f"affine_rows-{int(_a)}{int(_b)}", "stream", ["vf_affine_rows_f32"], ["affine_rows"], _make_affine_rows(_a, _b))
    _case(f"rowdot_softplus-{int(_a)}{int(_b)}", "stream", ["vf_rowdot_softplus"], ["rowdot_softplus"], _make_rowdot(_a, _b))


# ---------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------
# Entries that take a `stream` argument and have no case, with the reason.  (The host-side entries -- BPE, VCF, vf_narrow_ids --
# take no stream and are out of scope by construction.)
ABI_EXCLUSIONS: dict = {}
# Functions of variantformer_amd/ops.py whose source mentions `empty` without allocating an output.
WRAPPER_EXCLUSIONS: dict = {}


def stream_entries(header_text: str) -> list:
    """Every entry of the header that takes a `stream` argument (comments stripped as tests/test_abi_cpu.py::_declared does)."""
    src = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    return sorted(set(m.group(1) for m in re.finditer(r"\b(vf_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
                      if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2))))


def uncovered_entries(header_text: str, cases=None) -> list:
    cases = CASES if cases is None else cases
    covered = {e for c in cases for e in c.entries}
    return [e for e in stream_entries(header_text) if e not in covered and e not in ABI_EXCLUSIONS]


def allocating_wrappers() -> list:
    """Every function of variantformer_amd/ops.py whose source allocates with `empty`."""
    import inspect
    from variantformer_amd import ops
    names = []
    for name, fn in inspect.getmembers(ops, inspect.isfunction):
        if fn.__module__ == ops.__name__ and re.search(r"\btorch\.empty(_like)?\(", inspect.getsource(fn)):
            names.append(name)
    return sorted(names)


def uncovered_wrappers(cases=None) -> list:
    cases = CASES if cases is None else cases
    covered = {w for c in cases for w in c.wrappers}
    return [w for w in allocating_wrappers() if w not in covered and w not in WRAPPER_EXCLUSIONS]

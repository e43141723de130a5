"""The mutation argument of tests/test_large_offsets_gpu.py, made on the CPU from tests/large_offset_cases.py alone: every big
operand of every case really crosses element 2^31 (and byte 2^32), an element or byte offset narrowed to int32 or uint32
differs from the true one exactly where the GPU test looks, and even the narrowed ADDRESS lies inside the arena -- a kernel
that dropped a 64-bit cast would fail the GPU test with a wrong bit or a disturbed 0xFF, not fault the machine.  Deliberately
narrowed kernels are never run.

Huge-stride operands: at least a quarter of the rows and the last row start beyond element 2^31 (4-byte operands: also beyond
byte 2^32).  Natural operands (no stride argument; rows x width just above 2^31) cross in their last rows only: there the last
row, and the row the GPU test's middle slice is built around, are checked.

One narrowing cannot be told apart at these sizes and is not a fault at them either: an UNSIGNED 32-bit ELEMENT index is exact
up to 2^32 elements, and no operand here reaches that (a 4-byte operand of 2^32 elements is the whole 16 GiB behind the
headroom).  Its signed form, and both byte forms, differ from the true offset at every probe beyond the threshold."""
import pytest

from tests import large_offset_cases as C

T31, T32 = C.T31, C.T32


def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def _u32(x):
    return x & 0xFFFFFFFF


def _probe_elements(b):
    """Element offsets of the first and the last touched element and of the first touched element of the first row beyond
    element 2^31 (and, for 4-byte operands, beyond byte 2^32)."""
    first_row31 = -(-T31 // b.ld)
    probes = {"first": 0, "last": (b.rows - 1) * b.ld + b.cols - 1, "first_beyond_elem_2^31": first_row31 * b.ld}
    if b.esize == 4:
        probes["first_beyond_byte_2^32"] = -(-(T32 // 4) // b.ld) * b.ld
    return probes


@pytest.mark.parametrize("cid", [c.id for c in C.CASES])
def test_case_crosses_discriminates_and_stays_inside_the_arena(cid):
    case = C.BY_ID[cid]
    offs = C.layout(case.bigs)
    assert offs[0] == C.HEADROOM and C.ARENA_BYTES <= 24 * C.GiB and C.HEADROOM == 8 * C.GiB
    for b, base in zip(case.bigs, offs):
        assert base % C.ALIGN == 0 and base + b.nbytes <= C.ARENA_BYTES and b.ld >= b.cols
        assert b.nbytes > T32, "an operand larger than 2^32 bytes: a uint32-wrapped offset stays inside it"
        starts = [r * b.ld for r in (range(b.rows) if b.rows <= 100000 else (0, b.rows - 1))]
        assert starts[-1] >= T31, "the last row starts beyond element 2^31"
        if b.esize == 4:
            assert starts[-1] * 4 >= T32
        if not b.natural:
            assert 4 * sum(s >= T31 for s in starts) >= b.rows, (b, "a quarter of the rows beyond element 2^31")
            if b.esize == 4:
                assert 4 * sum(s * 4 >= T32 for s in starts) >= b.rows
        probes = _probe_elements(b)
        assert probes["first_beyond_elem_2^31"] <= probes["last"]
        for what, e in probes.items():
            byte = e * b.esize
            narrowed = {"elem_i32": _i32(e) * b.esize, "elem_u32": _u32(e) * b.esize, "byte_i32": _i32(byte), "byte_u32": _u32(byte)}
            for form, nb in narrowed.items():
                addr = base + nb
                assert 0 <= addr < C.ARENA_BYTES, (cid, b.name, what, form, addr)          # inside the arena: no fault
                if form == "elem_u32":
                    assert (nb != byte) == (e >= T32)                                      # (see the module docstring)
                elif what in ("last", "first_beyond_elem_2^31") or (what == "first_beyond_byte_2^32" and form.startswith("byte")):
                    assert nb != byte, (cid, b.name, what, form)                           # other memory: the GPU test sees it
                if nb != byte and nb >= 0 and form.endswith("u32"):
                    assert nb < b.nbytes                                                  # wrapped, still inside the operand
                if nb < 0:
                    assert -nb <= C.HEADROOM                                              # negative: in the headroom
        # the extreme narrowed values, whatever element a kernel addresses: never outside the arena
        assert base - (1 << 31) * b.esize >= 0


def test_attention_key_strides_respect_the_24_bit_guard():
    """K / V of every attention case: stride < 2^24 and max_seqlen_k * stride < 2^31 (vf_attn_varlen_fwd's guard accepts them)."""
    specs = C.attn_specs()
    n = 0
    for case in C.family("attn"):
        if case.p["big"] == "kv":
            spec, (b,) = specs[case.p["spec"]], case.bigs
            assert b.ld < (1 << 24) and max(spec.kl) * b.ld < T31 and b.ld % 8 == 0, case.id
            n += 1
    for case, spec in zip(C.family("attn_kv24"), C.KV24_SPECS):
        (b,) = case.bigs
        assert b.ld == 1 << 23 and max(spec.kl) * b.ld < T31 <= (max(spec.kl) + 1) * b.ld
        # the second sequence starts one row (16 MiB) short of byte 2^32: every key of it but the first lies beyond
        assert (spec.kl[0] + 1) * b.ld * b.esize >= T32 > spec.kl[0] * b.ld * b.esize
        n += 1
    assert n == len(C.attn_specs()) + len(C.FP16_NAMES) + 4
    assert (1 << 24) < C.LONGK * C.LONGK_STRIDE < T31            # past what a 24-bit PRODUCT would hold, inside the guard


def test_the_table_covers_every_family_and_kernel():
    fams = {c.family for c in C.CASES}
    assert fams >= {"gemm", "ln_producer", "ln_consumer", "gemm_wqkv", "attn", "attn_rows", "counted_keys", "softmax_counted",
                    "attn_probs", "attn_kv24", "attn_gene", "layernorm", "row_stats_cast2", "embed_pack", "embed_stream",
                    "segment", "rowdot", "cast", "rows_source", "rows_out", "segment_mean16", "gather16"}
    kernels = {s.kernel for s in C.attn_specs().values()}
    assert kernels >= {C.FWD64, C.FWD128, C.X32_32, C.X32_64, "attn_short2_kernel<1 pass>", "attn_short2_kernel<2 passes>",
                       "attn_short_kernel"}
    assert {s.kernel for s in C.KV24_SPECS} == {s.kernel for s in C.LONGK_SPECS} == {C.FWD64, C.FWD128, C.X32_32, C.X32_64}
    a, m, e = C.WQKV_SLICES
    assert m[0] <= C.straddle_row(C.WQKV_N) < m[1] and C.straddle_row(C.WQKV_N) == 466033
    for (sa, se) in C.gene_seq_slices():
        assert 0 <= sa < se <= C.GENE_SEQS
    mid = C.gene_seq_slices()[1]
    assert mid[0] * C.GENE_LEN <= 466033 < mid[1] * C.GENE_LEN

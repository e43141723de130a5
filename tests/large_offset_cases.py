"""The case table of the large-offset tests: which operand of which entry is made BIG (a view into one arena whose element
and byte offsets pass 2^31 / 2^32), with what shape and row stride, and where it lies in the arena.  Pure Python: no GPU, no
library.  tests/test_large_offsets_cpu.py proves from this table alone that every case crosses the thresholds, that an offset
narrowed to 32 bits would differ from the true one (so a narrowed kernel fails the GPU test) and that even the narrowed
address stays inside the arena (so it fails as a wrong bit, not as a fault); tests/test_large_offsets_gpu.py builds its
operands from the same table.

Arena: one uint8 buffer of ARENA_BYTES.  The first HEADROOM bytes hold no operand; every big operand of a case is placed
behind them, 256-byte aligned, in table order (an earlier operand is headroom for a later one).

Two ways to make an operand big:
  huge stride   a few hundred rows, LD_HUGE = 2^22 + 64 elements apart (only the touched columns of a row hold data).  Where an
                operand has too few (or too many) rows for a quarter of them to start beyond element 2^31 at LD_HUGE within the
                arena, its stride is chosen instead so that 30 % of the rows do (huge_ld).
  natural       the entry has no stride argument (or the shape is a product shape): the smallest row count with
                rows x width > 2^31, plus one ragged tile."""
from typing import NamedTuple

GiB = 1 << 30
T31, T32 = 1 << 31, 1 << 32
ARENA_BYTES = 24 * GiB
HEADROOM = 8 * GiB
ALIGN = 256
LD_HUGE = 2 ** 22 + 64
ESIZE = {"bf16": 2, "fp16": 2, "f32": 4}


class Big(NamedTuple):
    name: str            # the argument(s) of the entry this operand is
    esize: int           # bytes per element
    rows: int
    cols: int            # touched columns of every row
    ld: int              # row stride in elements (== cols: natural)
    natural: bool = False

    @property
    def n_elems(self):
        return (self.rows - 1) * self.ld + self.cols

    @property
    def nbytes(self):
        return self.n_elems * self.esize


class Case(NamedTuple):
    id: str
    family: str          # which GPU test runs it
    p: dict              # parameters of that test
    bigs: tuple          # the big operands, in arena order


def huge_ld(rows: int, esize: int) -> int:
    """Row stride (elements, a multiple of 64 plus 64) of a huge-stride operand of `rows` rows."""
    room = ARENA_BYTES - HEADROOM
    first = -(-T31 // LD_HUGE)                            # first row that starts beyond element 2^31
    if rows - first >= (rows + 3) // 4 and ((rows - 1) * LD_HUGE + LD_HUGE) * esize <= room:
        return LD_HUGE
    assert rows >= 4, rows
    ld = -(-T31 // (rows * 7 // 10))
    return (ld + 63) // 64 * 64 + 64


def huge(name, dtype, rows, cols):
    es = ESIZE[dtype]
    return Big(name, es, rows, cols, huge_ld(rows, es))


def natural(name, dtype, rows, cols):
    return Big(name, ESIZE[dtype], rows, cols, cols, True)


def layout(bigs):
    """Byte offset of every big operand inside the arena."""
    off, out = HEADROOM, []
    for b in bigs:
        out.append(off)
        off = (off + b.nbytes + ALIGN - 1) // ALIGN * ALIGN
    assert off <= ARENA_BYTES, (bigs, off)
    return out


# ---------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------
# M = 700: ragged against every tile (64, 128, 256) like the 515 rows of tests/test_ops_edges_gpu.py, and enough rows for a
# quarter of them (188 of 700) to start beyond element 2^31 at LD_HUGE, where row 512 is the first to do so (600 rows leave 88)
GEMM_M = 700
# (variant 22, the persistent 256x256 kernel, needs K % 128 == 0 and is variant 20's kernel at K = 192: "22-K256" is the path
# that really runs gemm8x_kernel)
GEMM_PATHS = (1, 5, 20, 22, "22-K256", "generic")
GEMM_KERNEL = {1: "gemm_mfma_kernel<128x128>", 5: "gemm_mfma_kernel<64x64>", 20: "gemm8_kernel", 22: "gemm8_kernel",
               "22-K256": "gemm8x_kernel", "generic": "gemm_generic_kernel"}
GEMM_VARIANT = {"gemm_mfma_kernel<128x128>": 1, "gemm_mfma_kernel<64x64>": 5, "gemm8_kernel": 20, "gemm8x_kernel": 22}
GEMM_BIGS = (("bf16", "A"), ("bf16", "out"), ("f32", "out"), ("res", "out"), ("res", "residual"), ("geglu", "out"))


def gemm_shape(path, epi):
    if path == "generic":
        return GEMM_M, (64 if epi == "geglu" else 40), 72
    return GEMM_M, (800 if epi == "geglu" else 776), (256 if path == "22-K256" else 192)


def _gemm_cases():
    out = []
    for dtype in ("bf16", "fp16"):
        for path in GEMM_PATHS:
            for epi, which in GEMM_BIGS:
                M, N, K = gemm_shape(path, epi)
                n_out = N // 2 if epi == "geglu" else N
                if which == "A":
                    big = huge("A", dtype, M, K)
                elif which == "out":
                    big = huge("out", "f32" if epi in ("f32", "res") else dtype, M, n_out)
                else:
                    big = huge("residual", "f32", M, N)
                out.append(Case(f"gemm-{dtype}-{path}-{epi}-{which}", "gemm", dict(dtype=dtype, path=path, epi=epi, big=which,
                                                                                   M=M, N=N, K=K), (big,)))
    return out


LN_M, LN_N, LN_K = GEMM_M, 1536, 512
# (form, big operand): the producer with an fp32 residual (out16 / out), with the 16-bit residual copy (R16), with the fp16 trunk
# (T16: residual in, t16_out out); the consumer (A = out16 of a producer, out) with the 16-bit and the GEGLU epilogue
LN_PRODUCER = (("f32", "out16"), ("f32", "out"), ("r16", "residual"), ("t16", "residual"), ("t16", "t16_out"))
LN_CONSUMER = (("bf16", "A"), ("bf16", "out"), ("geglu", "A"), ("geglu", "out"))


def _gemm_ln_cases():
    out = []
    for dtype in ("bf16", "fp16"):
        for form, which in LN_PRODUCER:
            bdt = {"out16": dtype, "out": "f32", "t16_out": "fp16", "residual": dtype if form == "r16" else "fp16"}[which]
            out.append(Case(f"ln_producer-{dtype}-{form}-{which}", "ln_producer", dict(dtype=dtype, form=form, big=which),
                            (huge(which, bdt, LN_M, LN_N),)))
        for epi, which in LN_CONSUMER:
            N = 2048 if epi == "geglu" else LN_N
            cols = LN_K if which == "A" else (N // 2 if epi == "geglu" else N)
            out.append(Case(f"ln_consumer-{dtype}-{epi}-{which}", "ln_consumer", dict(dtype=dtype, epi=epi, big=which, N=N),
                            (huge(which, dtype, LN_M, cols),)))
    return out


# the 44-gene Wqkv: 44 x 54 x 201 gene-stream tokens, out bf16 [M, 4608] = 2.2e9 elements
WQKV_M, WQKV_N, WQKV_K = 44 * 10854, 4608, 64
SLICE_ROWS = 256
WQKV_SLICES = ((0, 256), (465900, 466156), (WQKV_M - 256, WQKV_M))       # element 2^31 of out falls in row 466 033


def straddle_row(width):
    """The row of a natural [rows, width] buffer that holds element 2^31."""
    return T31 // width


def row_slices(rows, width, n=SLICE_ROWS, extra=()):
    """Row ranges [a, e) compared with small-buffer twins: the first n rows, n rows around element 2^31 (and around any row of
    `extra`), the last n rows."""
    mids = [straddle_row(width)] + list(extra)
    out = [(0, min(n, rows))]
    for m in mids:
        a = max(0, min(m - n // 2, rows - n))
        out.append((a, a + n))
    out.append((rows - n, rows))
    return out


def _natural_gemm_cases():
    return [Case(f"gemm_wqkv-v{v}", "gemm_wqkv", dict(variant=v), (natural("out", "bf16", WQKV_M, WQKV_N),)) for v in (0, 1)]


# ---------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------
class AttnSpec(NamedTuple):
    name: str
    dh: int
    H: int
    ql: tuple
    kl: tuple
    kernel: str
    q_log2: bool
    alibi: bool
    seed: int
    edge_case: str = ""        # the entry of tests/attn_edge_cases.py whose operands these are (repeated `rep` times)
    rep: int = 1


X32_32, X32_64 = "attn_x32_kernel<32 queries per wave>", "attn_x32_kernel<64 queries per wave>"
FWD64, FWD128 = "attn_fwd_kernel<64-query blocks>", "attn_fwd_kernel<128-query blocks>"
EDGE_NAMES = ("registry", "fwd64_dh48", "fwd64_dh128", "fwd128_dh48", "fwd128_dh96", "short2_2pass_dh48", "short2_1pass_dh64",
              "short2_2pass_dh64", "short_3groups", "short_4groups", "short2_2pass_dh40")
FP16_NAMES = ("fwd64_dh48", "short2_2pass_dh48")          # one tiled and one short case also run with fp16 operands


def _x32_specs():
    # dh 48 without ALiBi is attn_x32_kernel: 64 queries per wave once n_seq * H * ceil(max_q / 256) >= 2048, else 32
    import numpy as np
    rng = np.random.default_rng(1220)
    ql = (40, 1, 17, 33) + tuple(int(x) for x in rng.integers(1, 41, 60))
    kl = (9, 70, 17, 34) + tuple(int(x) for x in rng.integers(1, 71, 60))
    a = AttnSpec("x32_32_dh48", 48, 4, (10, 50, 7, 128, 1, 20, 33, 70) * 3, (9, 300, 64, 1, 77, 21, 33, 200) * 3, X32_32, True,
                 False, 1230)
    b = AttnSpec("x32_64_dh48", 48, 32, ql, kl, X32_64, True, False, 1240)
    assert len(a.ql) * a.H * -(-max(a.ql) // 256) < 2048 <= len(b.ql) * b.H * -(-max(b.ql) // 256)
    return [a, b]


def edge_spec(name) -> AttnSpec:
    """An entry of tests/attn_edge_cases.py with its sequence list repeated until both token counts reach about 700 (at most 8
    times: the rest is the stride's business), its first q_log2 setting, ALiBi."""
    from tests import attn_edge_cases as E
    c = E.CASES_BY_NAME[name]
    rep = max(1, min(8, -(-700 // max(1, min(sum(c.ql), sum(c.kl))))))
    return AttnSpec(name, c.dh, c.H, tuple(c.ql) * rep, tuple(c.kl) * rep, c.kernel, c.q_log2[0], True, c.seed, name, rep)


def attn_specs():
    return {s.name: s for s in [edge_spec(n) for n in EDGE_NAMES] + _x32_specs()}


def attn_bigs(spec: AttnSpec, dtype: str):
    D = spec.H * spec.dh
    return {"q": huge("q", dtype, sum(spec.ql), D), "kv": huge("k,v", dtype, sum(spec.kl), 2 * D),
            "out": huge("out", dtype, sum(spec.ql), D)}


def _attn_cases():
    out = []
    for name, spec in attn_specs().items():
        for dtype in ("bf16", "fp16") if name in FP16_NAMES else ("bf16",):
            bigs = attn_bigs(spec, dtype)
            for which in ("q", "kv", "out"):
                out.append(Case(f"attn-{name}-{dtype}-{which}", "attn", dict(spec=name, dtype=dtype, big=which), (bigs[which],)))
    return out


ROWMAP_TABLE_ROWS = 700
ROWMAP_GEOMS = {"seq2reg_windows": (64, 8, False), "gene_self": (48, 32, True)}      # dh, H, alibi (tests/test_ops_gpu.py)


def _rowmap_cases():
    return [Case(f"attn_rows-{g}", "attn_rows", dict(geom=g), (huge("q,k,v", "bf16", ROWMAP_TABLE_ROWS, 3 * H * dh),))
            for g, (dh, H, _) in ROWMAP_GEOMS.items()]


COUNTED = dict(dh=48, H=32, C=9, lens=(300, 1, 0, 77, 1024, 5))                   # tests/test_ops_gpu.py's geometry
SOFTMAX_COUNTED = dict(H=32, Cp=10, C=9, lens=(700, 1, 0, 33, 1300))


def _counted_cases():
    T, D = sum(COUNTED["lens"]), COUNTED["H"] * COUNTED["dh"]
    out = [Case(f"attn_counted_keys-{w}", "counted_keys", dict(big=w), (huge(w, "bf16", T, D),)) for w in ("q", "out")]
    T, W = sum(SOFTMAX_COUNTED["lens"]), SOFTMAX_COUNTED["H"] * SOFTMAX_COUNTED["Cp"]
    out += [Case("softmax_counted-scores", "softmax_counted", dict(big="scores"), (huge("scores", "f32", T, W),)),
            Case("softmax_counted-out", "softmax_counted", dict(big="out"), (huge("out", "bf16", T, W),))]
    return out


# vf_attn_probs_v2: H 4, dh 32; (keys, selected rows) per sequence -- R = 180 selected rows, R * H = 720 per-head output rows
PROBS_H, PROBS_DH = 4, 32
PROBS_SEQS = ((300, 54), (33, 3), (0, 3), (1, 1), (31, 65), (64, 54))
PROBS_R = sum(s[1] for s in PROBS_SEQS)
PROBS_TK = sum(s[0] for s in PROBS_SEQS)
PROBS_MAX_K = max(s[0] for s in PROBS_SEQS)


def _probs_cases():
    out = []
    D = PROBS_H * PROBS_DH
    for alibi in (True, False):
        for per_head in (0, 1):
            bigs = {"q": huge("q", "bf16", PROBS_R + 7, D), "k": huge("k", "bf16", PROBS_TK, D),
                    "out": huge("out", "f32", PROBS_R * (PROBS_H if per_head else 1), PROBS_MAX_K)}
            for which in ("q", "k", "out"):
                out.append(Case(f"attn_probs-{'alibi' if alibi else 'nobias'}-ph{per_head}-{which}", "attn_probs",
                                dict(alibi=alibi, per_head=per_head, big=which), (bigs[which],)))
    return out


# the 24-bit key offset of the tiled kernels.  At the guard: K | V slices of one buffer with row stride exactly 2^23, two sequences
# of 255 keys (255 * 2^23 < 2^31 is accepted; the second sequence starts beyond 2^32 bytes).  The queries (and H) are what sends
# the geometry to each kernel form.
KV24_STRIDE = 1 << 23
KV24_KL = (255, 255)
KV24_SPECS = [
    AttnSpec("kv24_fwd64", 48, 4, (20, 33), KV24_KL, FWD64, True, True, 1250),
    AttnSpec("kv24_fwd128", 48, 128, (600, 257), KV24_KL, FWD128, True, True, 1260),        # 2 * 128 * ceil(600 / 128) >= 1024
    AttnSpec("kv24_x32_32", 48, 4, (20, 33), KV24_KL, X32_32, True, False, 1270),
    AttnSpec("kv24_x32_64", 48, 256, (1024, 130), KV24_KL, X32_64, True, False, 1280),      # 2 * 256 * ceil(1024 / 256) >= 2048
]
# past 2^24 at a natural stride: one sequence of 6000 keys x stride 4608 (key * stride reaches 2.8e7), 600 queries, ordinary memory.
# H 4 and one sequence reach the 64-query-block and the 32-queries-per-wave forms; the two other forms need more blocks: H 32 (a
# packed [.., 3 * 32 * 48] row IS 4608 wide) and short sequences behind the long one.
LONGK, LONGK_STRIDE, LONGK_Q = 6000, 4608, 600
LONGK_SPECS = [
    AttnSpec("longk_fwd64", 48, 4, (LONGK_Q,), (LONGK,), FWD64, True, True, 1290),
    AttnSpec("longk_fwd128", 48, 32, (LONGK_Q,) + (3,) * 6, (LONGK,) + (5,) * 6, FWD128, True, True, 1300),
    AttnSpec("longk_x32_32", 48, 4, (LONGK_Q,), (LONGK,), X32_32, True, False, 1310),
    AttnSpec("longk_x32_64", 48, 32, (LONGK_Q,) + (3,) * 21, (LONGK,) + (5,) * 21, X32_64, True, False, 1320),
]


def _kv24_cases():
    out = []
    for s in KV24_SPECS:
        big = Big("k,v", 2, sum(s.kl), 2 * s.H * s.dh, KV24_STRIDE)
        out.append(Case(f"attn_kv24-{s.name}", "attn_kv24", dict(spec=s.name), (big,)))
    return out


# the 44-gene gene-stream self attention: 2376 sequences of 201 tokens, packed QKV [477 576, 4608] bf16
GENE_SEQS, GENE_LEN, GENE_H, GENE_DH = 44 * 54, 201, 32, 48
GENE_SLICE_SEQS = 54


def gene_seq_slices():
    """Sequence ranges compared with small twins: the first 54, the 54 around the token that holds element 2^31, the last 54."""
    mid = straddle_row(3 * GENE_H * GENE_DH) // GENE_LEN
    a = mid - GENE_SLICE_SEQS // 2
    return [(0, GENE_SLICE_SEQS), (a, a + GENE_SLICE_SEQS), (GENE_SEQS - GENE_SLICE_SEQS, GENE_SEQS)]


def _gene_attn_case():
    return [Case("attn_gene_self_44", "attn_gene", {}, (natural("qkv", "bf16", GENE_SEQS * GENE_LEN, 3 * GENE_H * GENE_DH),))]


# ---------------------------------------------------------------------------------------------
# streaming kernels
# ---------------------------------------------------------------------------------------------
LN_ROWS, LN_D = 524288 + 37, 4096                      # 2^31 elements fall on row 524 288, byte 2^32 of the fp32 rows on 262 144
EMB_W, EMB_L, EMB_D, EMB_V = 8200, 128, 2048, 500      # 1 049 600 tokens x 2048: element 2^31 is the first of window 8192
SEG_ROWS, SEG_D, SEG_WIN = EMB_W * EMB_L, 2048, 128
CAST_N = T31 + 4100                                    # (the table counts the flat buffer as rows of 4 elements)
assert CAST_N % 4 == 0
ROWS_D, ROWS_N = 2048, SEG_ROWS
MEAN16_LENS = (200, 1, 3, 0, 64, 65, 7, 130, 97, 2) * 2
MEAN16_D = 512
GATHER16_ROWS, GATHER16_D = 700, 384


def _stream_cases():
    x = natural("x", "f32", SEG_ROWS, SEG_D)
    out = [
        Case("layernorm", "layernorm", {}, (natural("x", "f32", LN_ROWS, LN_D), natural("out", "bf16", LN_ROWS, LN_D))),
        Case("row_stats_cast2", "row_stats_cast2", {}, (natural("x", "f32", LN_ROWS, LN_D), natural("out16", "fp16", LN_ROWS, LN_D))),
        Case("embed_pack", "embed_pack", {}, (natural("out", "f32", SEG_ROWS, EMB_D),)),
        Case("embed_stream", "embed_stream", {}, (natural("out16", "bf16", SEG_ROWS, EMB_D), natural("t16", "fp16", SEG_ROWS, EMB_D))),
        Case("segment_mean", "segment", dict(op="mean"), (x,)),
        Case("segment_max", "segment", dict(op="max"), (x,)),
        Case("segment_linear", "segment", dict(op="linear"), (x,)),
        Case("rowdot_softplus", "rowdot", {}, (x,)),
        Case("cast_f32_bf16", "cast", dict(dtype="bf16"), (natural("x", "f32", CAST_N // 4, 4), natural("out", "bf16", CAST_N // 4, 4))),
        Case("cast_f32_f16", "cast", dict(dtype="fp16"), (natural("x", "f32", CAST_N // 4, 4), natural("out", "fp16", CAST_N // 4, 4))),
    ]
    for op in ("gather", "add", "affine"):
        out.append(Case(f"{op}_rows-source", "rows_source", dict(op=op), (natural("src", "f32", ROWS_N, ROWS_D),)))
        out.append(Case(f"{op}_rows-out", "rows_out", dict(op=op, out="f32"), (natural("out", "f32", ROWS_N, ROWS_D),)))
    out.append(Case("gather_rows-out-bf16", "rows_out", dict(op="gather", out="bf16"), (natural("out", "bf16", ROWS_N, ROWS_D),)))
    for dtype in ("bf16", "fp16"):
        out.append(Case(f"segment_mean16-{dtype}", "segment_mean16", dict(dtype=dtype),
                        (huge("x", dtype, sum(MEAN16_LENS), MEAN16_D),)))
    out.append(Case("gather_rows_bf16-src", "gather16", dict(big="src"), (huge("src", "bf16", GATHER16_ROWS, GATHER16_D),)))
    out.append(Case("gather_rows_bf16-out", "gather16", dict(big="out"), (huge("out", "bf16", GATHER16_ROWS, GATHER16_D),)))
    return out


CASES = (_gemm_cases() + _gemm_ln_cases() + _natural_gemm_cases() + _attn_cases() + _rowmap_cases() + _counted_cases()
         + _probs_cases() + _kv24_cases() + _gene_attn_case() + _stream_cases())
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def family(name):
    return [c for c in CASES if c.family == name]


def ids(name):
    return [c.id for c in family(name)]

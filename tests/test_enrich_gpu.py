"""vf_enrich_counts and vf_hypergeom_tail on the GPU (include/vf_hip_enrich.h) through their ops wrappers, against
tests/enrich_cases.py: the counts exactly equal numpy; `tail` and `steps` equal the restatement bit for bit (they need only
+ * / and comparisons) and log_p is within LOG_P_ULPS ulp of the restatement's, the ulp taken at max(1, |log_p|) (the device's
log, exp and log1p), each figure printed before it is asserted.  Operands sit in guarded buffers, outputs are poisoned with
padding columns behind them: nothing outside the write set changes.  Then determinism and splits, the Benjamini-Hochberg step on
the device, and enrichment.enrich end to end on the planted case."""
import math

import numpy as np
import pytest
import torch

from tests import enrich_cases as E
from tests import write_set_cases as W

pytestmark = pytest.mark.gpu

GUARD = 64                      # guard rows either side of an output
EXTRA_LD = 5                    # padding columns behind an output's k


def _ops():
    from variantformer_amd import _lib, ops
    _lib.load()
    return ops


def _matrix_out(rows: int, cols: int, dtype, pattern: int, extra: int = EXTRA_LD):
    big = W.poisoned((rows + 2 * GUARD, cols + extra), dtype, W.DEVICE, pattern)
    return big, big[GUARD:GUARD + rows, :cols]


def _check_matrix(name: str, big: torch.Tensor, rows: int, cols: int, pattern: int):
    size = big.element_size()
    h = big.cpu().numpy().view(np.uint8).reshape(rows + 2 * GUARD, -1, size)
    assert (h[:GUARD] == pattern).all() and (h[GUARD + rows:] == pattern).all(), f"{name}: guard rows were written"
    assert (h[GUARD:GUARD + rows, cols:] == pattern).all(), f"{name}: the padding columns were written"


def _vector(n: int, dtype, pattern: int):
    big = W.poisoned((n + 2 * GUARD,), dtype, W.DEVICE, pattern)
    return big, big[GUARD:GUARD + n]


def _check_vector(name: str, big: torch.Tensor, n: int, pattern: int):
    h = big.cpu().numpy().view(np.uint8)
    size = big.element_size()
    assert (h[:size * GUARD] == pattern).all() and (h[size * (GUARD + n):] == pattern).all(), f"{name}: guard elements were written"


def _in(x: np.ndarray, pattern: int) -> torch.Tensor:
    return W.guarded(torch.from_numpy(x), pattern, rows=GUARD)


def _same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- counts --------------------------------------------------------------------------------------------------------------------------
def _counts(termptr, gene, labels, k, pattern):
    ops = _ops()
    T = termptr.shape[0] - 1
    tp, ge, la = _in(termptr, pattern), _in(gene, pattern), _in(labels, pattern)
    big, count = _matrix_out(T, k, torch.int32, pattern)
    assert count.stride(0) == k + EXTRA_LD
    bs, size = _vector(T, torch.int32, pattern)
    out = ops.enrich_counts(tp, ge, la, k, count=count, size=size)
    torch.cuda.synchronize()
    assert out[0] is count and out[1] is size
    _check_matrix("count", big, T, k, pattern)
    _check_vector("size", bs, T, pattern)
    assert np.array_equal(tp.cpu().numpy(), termptr) and np.array_equal(ge.cpu().numpy(), gene) and np.array_equal(la.cpu().numpy(), labels), \
        "termptr, gene and labels are only read"
    return count.cpu().numpy(), size.cpu().numpy()


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, E.MAX_K])
def test_counts_equal_numpy_exactly(k):
    G, T = 300, 40
    termptr, gene, labels = E.counts_case(G, k, T)
    sizes = np.diff(termptr)
    assert sizes[:5].tolist() == list(E.TERM_SIZES) and sizes[5] == G and {-1, G} <= set(gene[termptr[6]:termptr[7]].tolist())
    assert sizes.max() > 2 * E.THREADS or G < 2 * E.THREADS, "a term longer than two passes of the block, where the universe allows"
    assert -1 in labels and k in labels, "labels that name no cluster"
    want_count, want_size = E.counts(termptr, gene, labels, k)
    assert want_size[5] == G and want_size[6] == sizes[6] - 3 and want_count.sum(1).max() < want_size.max(), "entries outside the universe and genes in no cluster"
    for pattern in W.PATTERNS[:2]:
        count, size = _counts(termptr, gene, labels, k, pattern)
        assert _same_bits(count, want_count) and _same_bits(size, want_size), (k, pattern)
    # the cluster sizes: the same entry with the one term that lists every gene
    csize, whole = _counts(np.array([0, G], dtype=np.int64), np.arange(G, dtype=np.int32), labels, k, 0xFF)
    assert whole.tolist() == [G] and _same_bits(csize[0], np.bincount(labels[(labels >= 0) & (labels < k)], minlength=k).astype(np.int32))
    # rows [0, T) equal [0, a) + [a, T), called separately (a term-pointer slice keeps its offsets into gene)
    a = 7
    first, first_size = _counts(termptr[:a + 1], gene, labels, k, 0x3C)
    rest, rest_size = _counts(termptr[a:], gene, labels, k, 0x3C)
    assert _same_bits(np.concatenate((first, rest)), want_count) and _same_bits(np.concatenate((first_size, rest_size)), want_size)


def test_counts_past_max_k_are_refused_and_empty_inputs_write_zeros():
    from variantformer_amd import _lib
    ops = _ops()
    lib = _lib.load()
    dev = torch.device("cuda")
    k = E.MAX_K + 1
    count = torch.zeros((2, k), dtype=torch.int32, device=dev)
    size = torch.zeros(2, dtype=torch.int32, device=dev)
    termptr, gene, labels = torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    with pytest.raises(AssertionError, match="k="):
        ops.enrich_counts(termptr, gene, labels, k, count=count, size=size)
    rc = lib.vf_enrich_counts(termptr.data_ptr(), gene.data_ptr(), 1, 2, labels.data_ptr(), 4, k, count.data_ptr(), k, size.data_ptr(), 0)
    assert rc == 1 and lib.vf_last_error().decode().split(": ")[1].startswith("k="), "a larger k is refused, not served in panels"
    # no entries at all, and an empty universe
    c, s = _counts(np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32), np.array([0, 1, 2], dtype=np.int32), 3, 0xFF)
    assert not c.any() and not s.any()
    c, s = _counts(np.array([0, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32), np.zeros(0, dtype=np.int32), 3, 0xFF)
    assert not c.any() and not s.any(), "G = 0: every entry is outside the universe"


# ---- tail ----------------------------------------------------------------------------------------------------------------------------
def _tail(count, size, csize, N, alternative, lf, pattern, extra=EXTRA_LD):
    ops = _ops()
    T, k = count.shape
    wide = np.zeros((T, k + 3), dtype=np.int32)
    wide.view(np.uint8)[:] = pattern
    wide[:, :k] = count
    cnt = W.guarded(torch.from_numpy(wide), pattern, rows=GUARD)[:, :k]
    sz, cs, table = _in(size, pattern), _in(csize, pattern), _in(lf, pattern)
    outs = [_matrix_out(T, k, dtype, pattern, extra) for dtype in (torch.float64, torch.float64, torch.int32)]
    got = ops.hypergeom_tail(cnt, sz, cs, N, table, alternative, log_p=outs[0][1], tail=outs[1][1], steps=outs[2][1])
    torch.cuda.synchronize()
    assert got[0] is outs[0][1]
    for name, (big, _) in zip(("log_p", "tail", "steps"), outs):
        _check_matrix(name, big, T, k, pattern)
    assert np.array_equal(cnt.cpu().numpy(), count) and np.array_equal(sz.cpu().numpy(), size) and _same_bits(table.cpu().numpy(), lf)
    return tuple(v.cpu().numpy() for _, v in outs)


def _ulps(got, want):
    """|got - want| in ulp at max(1, |want|), over the finite cells; the others must agree exactly."""
    finite = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), finite) and _same_bits(got[~finite], want[~finite]), "-Inf exactly where the restatement has it"
    unit = np.spacing(np.maximum(1.0, np.abs(want[finite])))
    return np.abs(got[finite] - want[finite]) / unit


def _held(what, got, ref):
    log_p, tail, steps = got
    assert _same_bits(steps, ref["steps"]), f"{what}: steps equal the restatement"
    assert _same_bits(tail, ref["tail"]), f"{what}: tail equals the restatement bit for bit"
    u = _ulps(log_p, ref["log_p"])
    worst = float(u.max()) if u.size else 0.0
    print(f"[enrich tail] {what}: {steps.size} cells, longest sum {int(steps.max())} steps; log_p from the restatement by at most {worst:.2f} ulp "
          f"at max(1, |log_p|) (allowed {E.LOG_P_ULPS}); {int((u > 0).sum())} cells differ at all")
    assert worst <= E.LOG_P_ULPS
    for kind, value in (("zero", 0.0), ("-inf", -math.inf)):
        where = ref["kind"] == kind
        assert _same_bits(log_p[where], np.full(int(where.sum()), value)), f"{what}: exactly {value} where the contract says so"
        assert not tail[where].any() and not steps[where].any()
    return worst


@pytest.mark.parametrize("alternative", [E.GREATER, E.LESS])
def test_tail_equals_the_restatement_on_the_exhaustive_grid(alternative):
    kinds = set()
    for N in range(E.GRID_MAX_N + 1):
        count, size, csize = E.grid(N)
        lf = E.log_factorials(N)
        ref = E.tail_cells(count, size, csize, N, alternative, lf)
        kinds |= set(ref["kind"].ravel().tolist())
        _held(f"N={N} alternative={alternative}", _tail(count, size, csize, N, alternative, lf, W.PATTERNS[N % 3]), ref)
    assert kinds == {"zero", "-inf", "direct", "complement"}


@pytest.mark.parametrize("alternative", [E.GREATER, E.LESS])
def test_tail_equals_the_restatement_at_the_notebooks_universe(alternative):
    N = E.BIG_N
    count, size, csize = E.big_table()
    assert count.size == 2000 and 0 in size and 0 in csize, "K = 0 and n = 0 among the cells"
    lf = E.log_factorials(N)
    ref = E.tail_cells(count, size, csize, N, alternative, lf)
    lo, hi, mode = E.support(N, int(size[10]), int(csize[10]))        # cell (10, 10) is the first of ten picks: x = lo; then hi, the mode, ..
    assert count[10, 10:15].tolist() == [E.support(N, int(size[10]), int(csize[c]))[j] + d for c, j, d in ((10, 0, 0), (11, 1, 0), (12, 2, 0), (13, 2, -1), (14, 2, 1))]
    assert {"zero", "-inf", "direct", "complement"} == set(ref["kind"].ravel().tolist())
    got = _tail(count, size, csize, N, alternative, lf, 0xFF)
    _held(f"N={N} alternative={alternative}", got, ref)
    again = _tail(count, size, csize, N, alternative, lf, 0x00, extra=0)
    assert all(_same_bits(a, b) for a, b in zip(got, again)), "two runs are equal bit for bit, whatever the memory held and whatever ldo is"
    a = 17
    first = _tail(count[:a], size[:a], csize, N, alternative, lf, 0x3C)
    rest = _tail(count[a:], size[a:], csize, N, alternative, lf, 0x3C)
    assert all(_same_bits(np.concatenate((f, r)), g) for f, r, g in zip(first, rest, got)), "rows [0, T) equal [0, a) + [a, T)"
    steps = got[2][ref["kind"] != "zero"]
    print(f"[enrich tail] N={N}: steps per cell with a sum: median {int(np.median(steps))}, 90 % {int(np.percentile(steps, 90))}, max {int(steps.max())}")


def test_tail_keeps_invalid_sizes_inside_the_buffers():
    N = 20
    lf = E.log_factorials(N)
    count = np.array([[3, 3, 3], [3, 3, 3], [3, 3, 3]], dtype=np.int32)
    size, csize = np.array([-1, N + 1, 7], dtype=np.int32), np.array([5, -2, N + 3], dtype=np.int32)
    log_p, tail, steps = _tail(count, size, csize, N, E.GREATER, lf, 0xFF)
    want = E.tail_cells(count, size, csize, N, E.GREATER, lf)
    assert np.isnan(log_p).sum() == 8 and np.array_equal(np.isnan(log_p), np.isnan(want["log_p"])) and np.array_equal(np.isnan(tail), np.isnan(log_p))
    assert not steps[np.isnan(log_p)].any() and log_p[2, 0] == want["log_p"][2, 0] and np.isfinite(log_p[2, 0])


# ---- q and the whole -------------------------------------------------------------------------------------------------------------------
def test_q_on_the_device_equals_the_restatement_bit_for_bit():
    from variantformer_amd import enrichment
    rng = np.random.default_rng(11)
    for shape in ((1, 1), (30, 6), (257, 65)):
        p = rng.random(shape) ** 5
        p[rng.random(shape) < 0.3] = 1.0
        got = enrichment._bh(torch.from_numpy(p).cuda()).cpu().numpy()
        assert _same_bits(got, E.bh(p)), shape


def test_enrich_finds_the_planted_pairs():
    from variantformer_amd import enrichment
    labels, ann, universe = E.planted()
    out = enrichment.enrich(labels, ann, universe)
    T, k = E.PLANTED_TERMS, E.PLANTED_CLUSTERS
    assert out["terms"][:k] == [f"planted_{c}" for c in range(k)] and len(out["terms"]) == T
    for key, dtype in (("count", np.int32), ("log_p", np.float64), ("p", np.float64), ("fold", np.float64), ("q", np.float64)):
        assert out[key].shape == (T, k) and out[key].dtype == dtype, key
    m = enrichment.membership(ann, universe, min_size=5, max_size=500)
    count, size = E.counts(m.termptr, m.gene, labels, k)
    csize = np.bincount(labels, minlength=k).astype(np.int32)
    assert _same_bits(out["count"], count) and _same_bits(out["term_size"], size) and _same_bits(out["cluster_size"], csize)
    ref = E.tail_cells(count, size, csize, len(universe), E.GREATER)
    assert float(_ulps(out["log_p"], ref["log_p"]).max()) <= E.LOG_P_ULPS
    assert _same_bits(out["q"], E.bh(out["p"])), "q is Benjamini-Hochberg over all T * k cells of the device's p"
    assert np.allclose(out["p"], np.exp(out["log_p"]), rtol=1e-14, atol=0) and np.allclose(out["fold"], (count / csize[None, :]) / (size[:, None] / 600.0), rtol=1e-14)
    smallest = np.argsort(out["q"].ravel(), kind="stable")[:k]
    assert sorted(smallest.tolist()) == [c * k + c for c in range(k)], "the six planted pairs have the six smallest q"
    assert out["q"].ravel()[smallest].max() < 0.05
    frame = out["frame"]
    assert list(frame.columns) == ["cluster", "term", "count", "term_size", "cluster_size", "fold", "log_p", "p", "q"]
    assert len(frame) == k and sorted(zip(frame["cluster"], frame["term"])) == [(c, f"planted_{c}") for c in range(k)]
    assert (np.diff(frame["q"].to_numpy()) >= 0).all() and (frame["count"] == 40).all() and (frame["fold"] > 5).all()
    # the stages by themselves, a Membership in place of the annotation, names for the clusters, and the other tail
    h = enrichment.hypergeom(labels, m, return_steps=True)
    assert _same_bits(h["log_p"], out["log_p"]) and _same_bits(h["count"], count) and _same_bits(h["steps"], ref["steps"]) and _same_bits(h["tail"], ref["tail"])
    named = enrichment.enrich(labels, m, cluster_names=list("abcdef"), fdr=1.0)
    assert _same_bits(named["q"], out["q"]) and len(named["frame"]) == T * k and set(named["frame"]["cluster"]) == set("abcdef")
    less = enrichment.hypergeom(labels, m, alternative="less")
    both = np.exp(less["log_p"]) + out["p"] - np.exp([[E.log_pmf(E.log_factorials(600), int(count[t, c]), int(size[t]), int(csize[c]), 600) for c in range(k)] for t in range(T)])
    assert np.abs(both - 1.0).max() < 1e-12, "P[X <= x] + P[X >= x] - P[X = x] = 1"
    wider = enrichment.hypergeom(np.where(labels == 5, -1, labels), m, n_clusters=8)
    assert wider["count"].shape == (T, 8) and not wider["count"][:, 5:].any() and _same_bits(wider["count"][:, :5], count[:, :5])
    assert (wider["log_p"][:, 5:] == 0).all() and _same_bits(wider["term_size"], size), "a gene in no cluster stays in the universe; an empty cluster has p = 1"

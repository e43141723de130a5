"""vf_tsne_perplexity, vf_tsne_joint, vf_tsne_repulsion and vf_tsne_descent on the GPU (include/vf_hip_tsne.h) through their ops
wrappers, against the numpy restatements of tests/tsne_cases.py: selections, integers and every sum without exp / log / sqrt /
reciprocal exactly; the rest against the fp64 restatement within FACTOR times the case's yardstick (the fp32 restatement's own
deviation from the fp64 one, tests/tsne_cases.py), each figure printed before it is asserted.  Operands sit in guarded buffers
with odd row strides, outputs are poisoned and guarded: nothing outside the write set changes and nothing inside it keeps the
pattern.  Then a row stride past 2^31 elements, manifold.tsne end to end on the two fixtures against the three CPU references,
and VCFProcessor.expression_tsne."""
import numpy as np
import pandas as pd
import pytest
import torch

from tests import tsne_cases as T
from tests import write_set_cases as W

pytestmark = pytest.mark.gpu

GUARD = 64                      # guard elements / rows either side of an output
EXTRA_LD = 5                    # columns behind the matrix, in operands and outputs alike
_WORST = dict.fromkeys(T.MEASURED, 0.0)


@pytest.fixture(scope="module", autouse=True)
def _report_the_measured_deviations():
    """After the module's tests: what they measured as device deviation over yardstick, beside what tests/tsne_cases.py records."""
    yield
    for key, worst in _WORST.items():
        print(f"[tsne measured] {key}: largest device deviation / yardstick {worst:.2f}; recorded {T.MEASURED[key]}; allowed {T.FACTOR:g}")


def _ops():
    from variantformer_amd import _lib, ops
    _lib.load()
    return ops


def _vector(n: int, dtype, pattern: int):
    big = W.poisoned((n + 2 * GUARD,), dtype, W.DEVICE, pattern)
    return big, big[GUARD:GUARD + n]


def _check_vector(name: str, big: torch.Tensor, n: int, pattern: int):
    h = big.cpu().numpy().view(np.uint8)
    size = big.element_size()
    assert (h[:size * GUARD] == pattern).all() and (h[size * (GUARD + n):] == pattern).all(), f"{name}: guard elements were written"


def _matrix_out(rows: int, cols: int, pattern: int, extra: int = EXTRA_LD):
    big = W.poisoned((rows + 2 * GUARD, cols + extra), torch.float32, W.DEVICE, pattern)
    return big, big[GUARD:GUARD + rows, :cols]


def _check_matrix(name: str, big: torch.Tensor, rows: int, cols: int, pattern: int):
    h = big.cpu().numpy().view(np.uint8).reshape(rows + 2 * GUARD, -1, 4)
    assert (h[:GUARD] == pattern).all() and (h[GUARD + rows:] == pattern).all(), f"{name}: guard rows were written"
    assert (h[GUARD:GUARD + rows, cols:] == pattern).all(), f"{name}: columns past the write set were written"


def _operand(x: np.ndarray, pattern: int, extra: int = EXTRA_LD) -> torch.Tensor:
    """The matrix as a [rows, cols] view of rows cols + extra apart, the pattern behind the columns and in guard rows around."""
    rows, cols = x.shape
    wide = np.zeros((rows, cols + extra), dtype=x.dtype)
    wide.view(np.uint8)[:] = pattern
    wide[:, :cols] = x
    return W.guarded(torch.from_numpy(wide), pattern, rows=GUARD)[:, :cols]


def _same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _held(name: str, what: str, got, want64, ref32):
    """The device's `got` against the fp64 restatement within FACTOR yardsticks; yardstick = the fp32 restatement's deviation.
    A yardstick of 0 must be met exactly.  Prints before it asserts; returns deviation / yardstick."""
    with np.errstate(invalid="ignore"):
        nan = np.isnan(want64)
        assert np.array_equal(np.isnan(got), nan), f"{what}: NaN exactly where the restatement has it"
        yard = float(np.abs(ref32.astype(np.float64) - want64)[~nan].max()) if (~nan).any() else 0.0
        dev = float(np.abs(got.astype(np.float64) - want64)[~nan].max()) if (~nan).any() else 0.0
    ratio = dev / yard if yard > 0 else (0.0 if dev == 0 else np.inf)
    print(f"[tsne {name}] {what}: device from fp64 by {dev:.3e}, yardstick (fp32 restatement from fp64) {yard:.3e}, ratio {ratio:.2f} "
          f"(allowed {T.FACTOR:g})")
    _WORST[name] = max(_WORST[name], ratio if np.isfinite(ratio) else 1e30)
    if yard == 0:
        assert _same_bits(got[~nan], ref32[~nan]), f"{what}: a yardstick of 0 is met exactly"
    else:
        assert dev <= T.FACTOR * yard, (what, dev, yard)
    return ratio


# ---- perplexity ----------------------------------------------------------------------------------------------------------------------
def _perplexity(idx, d2, perplexity, pattern):
    ops = _ops()
    R, m = idx.shape
    idx_d, d2_d = _operand(idx, pattern), _operand(d2, pattern)
    assert idx_d.stride(0) == d2_d.stride(0) == m + EXTRA_LD
    bb, beta = _vector(R, torch.float32, pattern)
    bp, p_cond = _matrix_out(R, m, pattern)
    ops.tsne_perplexity(idx_d, d2_d, perplexity, beta=beta, p_cond=p_cond)
    torch.cuda.synchronize()
    _check_vector("beta", bb, R, pattern)
    _check_matrix("p_cond", bp, R, m, pattern)
    assert np.array_equal(idx_d.cpu().numpy(), idx) and _same_bits(d2_d.cpu().numpy(), d2), "idx and d2 are only read"
    return beta.cpu().numpy(), p_cond.cpu().numpy()


@pytest.mark.parametrize("m", T.PERPLEXITY_MS)
@pytest.mark.parametrize("R", T.PERPLEXITY_RS)
def test_perplexity_equals_the_reference(R, m):
    from variantformer_amd import _lib
    if m == 1:                                                        # perplexity >= 1 and < m: a list of one admits none
        idx, d2 = T.perplexity_case("random", R, m)
        with pytest.raises(_lib.VFError, match="perplexity="):
            _perplexity(idx, d2, 1.0, 0xFF)
        return
    perplexity = T.perplexity_of(m)
    target = np.float64(np.float32(np.log(perplexity)))
    for kind in T.PERPLEXITY_KINDS:
        idx, d2 = T.perplexity_case(kind, R, m)
        beta32, p32, conv32 = T.perplexity_search(idx, d2, perplexity, T.F32)
        _, _, conv64 = T.perplexity_search(idx, d2, perplexity, T.F64)
        x64, pres = T.shifted(idx, d2, T.F64)
        p_at32, _, h_at32 = T.evaluate(x64, pres, beta32.astype(np.float64), T.F64)
        x32, _ = T.shifted(idx, d2, T.F32)
        _, _, h32 = T.evaluate(x32, pres, beta32, T.F32)
        for pattern in (W.PATTERNS if kind in ("random", "absent") else W.PATTERNS[:1]):
            beta, p = _perplexity(idx, d2, perplexity, pattern)
            some = pres.any(1)
            # selections, exactly: what is not present gets +0, a row with nothing present beta = +0 and all +0
            assert _same_bits(p[~pres], np.zeros(int((~pres).sum()), dtype=np.float32)), (kind, "an absent entry, or idx == i, gets +0")
            assert _same_bits(beta[~some], np.zeros(int((~some).sum()), dtype=np.float32)) and (beta[some] > 0).all() and np.isfinite(beta).all()
            assert np.isfinite(p).all() and (p >= 0).all() and np.allclose(p[some].sum(1), 1.0, atol=1e-5), kind
            # the probabilities at the beta the search ended at
            p_at, _, h_at = T.evaluate(x64, pres, beta.astype(np.float64), T.F64)
            p_at, p_ref = np.where(pres, p_at, 0), np.where(pres, p_at32, 0)
            yard = float(np.abs(p32.astype(np.float64) - p_ref).max())
            dev = float(np.abs(p.astype(np.float64) - p_at).max())
            ratio = dev / yard if yard > 0 else (0.0 if dev == 0 else np.inf)
            _WORST["p_cond"] = max(_WORST["p_cond"], ratio if np.isfinite(ratio) else 1e30)
            print(f"[tsne p_cond] R={R} m={m} {kind} pattern={pattern:#x}: device P from the fp64 P at its beta by {dev:.3e}, yardstick {yard:.3e}, "
                  f"ratio {ratio:.2f} (allowed {T.FACTOR:g})")
            assert dev <= T.FACTOR * yard if yard > 0 else dev == 0, (kind, dev, yard)
            # beta by its equation, on the rows both restatements solved
            solved = some & conv32 & conv64
            if solved.any():
                yard_h = float(np.abs(h32.astype(np.float64) - h_at32)[solved].max())
                res = float(np.abs(h_at - target)[solved].max())
                excess = max(res - float(np.float32(T.TOL)), 0.0)
                ratio_h = excess / yard_h if yard_h > 0 else (0.0 if excess == 0 else np.inf)
                _WORST["entropy"] = max(_WORST["entropy"], ratio_h if np.isfinite(ratio_h) else 1e30)
                print(f"[tsne entropy] R={R} m={m} {kind}: |H(beta) - log perplexity| in fp64 {res:.3e} (tolerance {T.TOL:g}), beyond it "
                      f"{excess:.3e}, yardstick {yard_h:.3e}, ratio {ratio_h:.2f}")
                assert excess <= T.FACTOR * yard_h, (kind, res, yard_h)
            # a row the search cannot solve ends finite after all its steps, where the restatement ends: every branch is exact
            flat = some & ~conv32 & ~conv64 & ((x64 == 0) | ~pres).all(1)
            assert _same_bits(beta[flat], beta32[flat]) and _same_bits(p[flat], p32[flat]), (kind, "equal distances: beta = 2^+-99, P uniform")
            assert np.isin(beta[flat], (np.float32(2.0 ** 99), np.float32(2.0 ** -99))).all()
            if kind == "flat" and m >= 63:                               # (a short list may hold the row itself and one other: solved at once)
                assert flat[0] and (R == 1 or flat[1]), "the rows of duplicates and of equal distances are such rows"


# ---- joint ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,m", [(1, 2), (3, 2), (63, 2), (64, 29), (65, 64), (257, 5), (70, 255)])
def test_joint_equals_the_reference_and_is_symmetric_bit_for_bit(R, m):
    ops = _ops()
    rng = np.random.default_rng(R * 1000 + m)
    idx, d2 = T.perplexity_case("absent", R, m)
    idx = np.where(idx >= 0, idx % R, idx).astype(np.int32)           # rows of the graph: one-way and mutual edges, rows that list themselves
    if R > 8:
        idx[7], d2[7] = -1, np.inf                                    # lists nobody; others may list it
        five = idx == 5
        idx[five], d2[five] = -1, np.inf
        idx[5], d2[5] = -1, np.inf                                    # no edge at all
        idx[3, 0] = 3                                                 # a row that lists itself
    p_cond = np.where(T.present(idx, d2), rng.random((R, m), dtype=np.float32), 0).astype(np.float32)
    rowptr, col = T.csr(idx, d2)
    nnz = col.shape[0]
    want = T.joint(idx, p_cond, rowptr, col)
    for pattern in W.PATTERNS[:2]:
        idx_d, pc_d = _operand(idx, pattern), _operand(p_cond, pattern)
        big, p = _vector(nnz, torch.float32, pattern)
        rp, cl = W.guarded(torch.from_numpy(rowptr), pattern, rows=GUARD), W.guarded(torch.from_numpy(col), pattern, rows=GUARD)
        assert ops.tsne_joint(idx_d, pc_d, rp, cl, p=p) is p
        torch.cuda.synchronize()
        _check_vector("p", big, nnz, pattern)
        got = p.cpu().numpy()
        assert _same_bits(got, want), "a + b, rounded once: exact"
        assert np.array_equal(idx_d.cpu().numpy(), idx) and _same_bits(pc_d.cpu().numpy(), p_cond) and np.array_equal(cl.cpu().numpy(), col)
        full = T.dense(rowptr, col, got)
        assert _same_bits(full, full.T.copy()), "(i, j) and (j, i) get the same bits"
    if R == 1:
        assert nnz == 0, "R = 1 has no edge: nnz = 0 launches nothing and writes nothing"


# ---- repulsion -----------------------------------------------------------------------------------------------------------------------
def _repulsion(Y, dof, splits, pattern, extra=EXTRA_LD):
    ops = _ops()
    R, dim = Y.shape
    y_d = _operand(Y, pattern, extra) if extra else W.guarded(torch.from_numpy(Y), pattern, rows=GUARD)
    big = W.poisoned((splits * R * (dim + 1) + 2 * GUARD,), torch.float32, W.DEVICE, pattern)
    part = big[GUARD:GUARD + splits * R * (dim + 1)].view(splits, R, dim + 1)
    assert ops.tsne_repulsion(y_d, dof=dof, splits=splits, part=part) is part
    torch.cuda.synchronize()
    _check_vector("part", big, splits * R * (dim + 1), pattern)
    assert _same_bits(y_d.cpu().numpy(), Y), "Y is only read"
    return part.cpu().numpy()


@pytest.mark.parametrize("R", [1, 2, 63, 64, 65, 257])
def test_repulsion_equals_the_reference(R):
    for dim in (1, 2, 3, 4):
        Y = T.embedding(R, dim, scale=1.5)
        if R > 8:
            Y[4] = Y[2]                                               # coincident points
        for dof in (1, 2, 3):
            for splits in sorted({1, 2, 3, 7, R + 1}):
                want64, ref32 = T.repulsion(Y, dof, splits, T.F64), T.repulsion(Y, dof, splits, T.F32)
                pattern = W.PATTERNS[(dim + dof + splits) % 3]
                got = _repulsion(Y, dof, splits, pattern)
                assert not np.isnan(got).any()
                what = f"R={R} dim={dim} dof={dof} splits={splits}"
                _held("repulsion", what + " forces", got[:, :, :dim], want64[:, :, :dim], ref32[:, :, :dim])
                _held("repulsion", what + " weights", got[:, :, dim], want64[:, :, dim], ref32[:, :, dim])
                for s in range(splits):
                    lo, hi = T.split_range(R, splits, s)
                    if lo == hi:
                        assert _same_bits(got[s], np.zeros((R, dim + 1), dtype=np.float32)), "an empty range writes +0"
                if R > 8 and splits == 1:
                    alone = _repulsion(Y[[2, 4]], dof, 1, pattern)
                    assert (alone[0, :, :dim] == 0).all() and (alone[0, :, dim] == 1).all(), "coincident: w = 1 exactly and no force"


def test_repulsion_rows_do_not_depend_on_the_stride_and_a_nan_row_poisons_what_reads_it():
    R, dim, dof, splits = 300, 2, 1, 3
    Y = T.embedding(R, dim)
    base = _repulsion(Y, dof, splits, 0xFF)
    for extra in (0, 1, 11):
        assert _same_bits(_repulsion(Y, dof, splits, 0x3C, extra), base), "the same bits whatever ld is, whatever stands behind the columns"
    # more rows behind: the vertices of the first split read the same rows in the same order
    more = np.concatenate((Y, T.embedding(100, dim, seed=1)))
    assert [T.split_range(R + 100, splits + 1, s) for s in range(splits)] == [T.split_range(R, splits, s) for s in range(splits)]
    wide = _repulsion(more, dof, splits + 1, 0x00)
    assert _same_bits(wide[:splits, :R], base), "a vertex's row depends on the rows of its range alone: not on how many vertices or splits there are"
    bad = Y.copy()
    bad[131, 1] = np.nan                                              # in split 1 (rows 100 .. 199)
    got = _repulsion(bad, dof, splits, 0xFF)
    nan = np.isnan(got).any(2)
    want = np.zeros((splits, R), dtype=bool)
    want[1, :] = True
    want[:, 131] = True
    assert np.array_equal(nan, want), "NaN in exactly the rows that read the NaN row"
    clean = ~want
    assert _same_bits(got[clean], base[clean]), "and nothing else changes"


# ---- descent -------------------------------------------------------------------------------------------------------------------------
def _descent(graph, Y, update, gains, begin, end, pattern, exaggeration=12.0, momentum=0.5, learning_rate=T.STEPS_LEARNING_RATE, min_gain=0.01, splits=3):
    ops = _ops()
    rowptr, col, p = graph
    R, dim = Y.shape
    state = [_operand(a.astype(np.float32), pattern) for a in (Y, update, gains)]
    need = ops.tsne_work_bytes(R, dim, splits)
    work_big = W.poisoned((need + 2 * 8 * GUARD,), torch.uint8, W.DEVICE, pattern)
    work = work_big[8 * GUARD:8 * GUARD + need]
    zb, zsum = _vector(end - begin, torch.float64, pattern)
    g = [W.guarded(torch.from_numpy(a), pattern, rows=GUARD) for a in (rowptr, col, p)]
    out = ops.tsne_descent(*g, *state, iter_begin=begin, iter_end=end, exaggeration=exaggeration, momentum=momentum,
                           learning_rate=learning_rate, min_gain=min_gain, dof=max(dim - 1, 1), splits=splits, work=work, zsum=zsum)
    torch.cuda.synchronize()
    assert out[0] is state[0] and out[3] is zsum
    _check_vector("zsum", zb, end - begin, pattern)
    h = work_big.cpu().numpy()
    assert (h[:8 * GUARD] == pattern).all() and (h[8 * GUARD + need:] == pattern).all(), "work: bytes outside VF_TSNE_WORK_BYTES were written"
    for name, s in zip(("Y", "update", "gains"), state):
        wide = torch.as_strided(s, (R + 2 * GUARD, dim + EXTRA_LD), (dim + EXTRA_LD, 1), s.storage_offset() - GUARD * (dim + EXTRA_LD))
        _check_matrix(name, wide, R, dim, pattern)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(g, (rowptr, col, p))), "the graph is only read"
    return tuple(s.cpu().numpy() for s in state) + (zsum.cpu().numpy(),)


@pytest.mark.parametrize("R,m,dim", [(70, 9, 2), (130, 20, 3), (65, 6, 1), (257, 4, 4)])
def test_descent_equals_the_reference_and_can_be_split(R, m, dim):
    _, _, rowptr, col, p = T.small_graph(R, m)
    graph = (rowptr, col, p)
    Y0 = T.embedding(R, dim, scale=1e-4)
    zero, one = np.zeros((R, dim), dtype=np.float32), np.ones((R, dim), dtype=np.float32)
    whole = _descent(graph, Y0, zero, one, 0, 20, 0xFF)
    again = _descent(graph, Y0, zero, one, 0, 20, 0x00)
    assert all(_same_bits(a, b) for a, b in zip(whole, again)), "two runs are equal bit for bit, whatever the memory held"
    first = _descent(graph, Y0, zero, one, 0, 7, 0x3C)
    rest = _descent(graph, *first[:3], 7, 20, 0xFF)
    assert all(_same_bits(a, b) for a, b in zip(whole[:3], rest[:3])), "[0, 7) then [7, 20) equals [0, 20), state included"
    assert _same_bits(np.concatenate((first[3], rest[3])), whole[3]), "and so does every iteration's Z"
    assert np.isfinite(whole[0]).all() and (whole[2] >= np.float32(0.01)).all()
    want64 = T.descent(rowptr, col, p, Y0, zero, one, 20, 12.0, 0.5, T.STEPS_LEARNING_RATE, 0.01, 3, T.F64)
    ref32 = T.descent(rowptr, col, p, Y0, zero, one, 20, 12.0, 0.5, T.STEPS_LEARNING_RATE, 0.01, 3, T.F32)
    what = f"R={R} dim={dim}"
    _held("positions", what + " positions after 20 iterations", whole[0], want64[0], ref32[0])
    _held("positions", what + " updates after 20 iterations", whole[1], want64[1], ref32[1])
    _held("zsum", what + " Z of 20 iterations", whole[3], want64[3], ref32[3])
    # the first iteration alone: update = 0, so update * grad == 0 for every element and all go to dec; then the floor
    one_step = _descent(graph, Y0, zero, one, 0, 1, 0xFF)
    assert _same_bits(one_step[2], np.full((R, dim), np.float32(1.0) * np.float32(0.8), dtype=np.float32)), "update * grad == 0 goes to dec"
    floored = _descent(graph, Y0, zero, one, 0, 1, 0xFF, min_gain=0.9)
    assert _same_bits(floored[2], np.full((R, dim), np.float32(0.9), dtype=np.float32)), "gains below min_gain are raised to it"
    ref1 = T.descent(rowptr, col, p, Y0, zero, one, 1, 12.0, 0.5, T.STEPS_LEARNING_RATE, 0.9, 3, T.F32)
    assert np.array_equal(floored[2], ref1[2])
    print(f"[tsne descent] {what}: {int((whole[2] > 1).sum())} of {whole[2].size} gains above 1 after 20 iterations (the inc branch)")


def test_descent_without_edges_and_without_iterations():
    ops = _ops()
    R, dim = 5, 2
    graph = (np.zeros(R + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
    Y0 = T.embedding(R, dim)
    zero, one = np.zeros((R, dim), dtype=np.float32), np.ones((R, dim), dtype=np.float32)
    none = _descent(graph, Y0, zero, one, 4, 4, 0xFF)
    assert _same_bits(none[0], Y0) and _same_bits(none[1], zero) and _same_bits(none[2], one) and none[3].shape == (0,), "an empty range writes nothing"
    got = _descent(graph, Y0, zero, one, 0, 3, 0xFF, exaggeration=1.0, momentum=0.8, splits=2)
    want = T.descent(*graph, Y0, zero, one, 3, 1.0, 0.8, T.STEPS_LEARNING_RATE, 0.01, 2, T.F64)
    ref = T.descent(*graph, Y0, zero, one, 3, 1.0, 0.8, T.STEPS_LEARNING_RATE, 0.01, 2, T.F32)
    _held("positions", "nnz = 0: repulsion alone", got[0], want[0], ref[0])
    del ops


def test_a_row_stride_past_2_31_elements():
    """R = 3 with the rows of p_cond 2^30 + 8 elements apart: the third row starts past 2^31 elements and 8 GiB.  Only the used
    elements are written before the call."""
    ops = _ops()
    R, m, ld = 3, 2, 2 ** 30 + 8
    assert (R - 1) * ld > 2 ** 31
    idx = np.array([[1, 2], [2, 0], [0, 1]], dtype=np.int32)
    d2 = np.array([[0.25, 0.5], [0.125, 0.75], [0.5, 0.5625]], dtype=np.float32)
    buf = torch.empty(2 * ld + 8, dtype=torch.float32, device="cuda")
    p_cond = buf.as_strided((R, m), (ld, 1))
    p_cond.fill_(7.0)
    assert p_cond[2].data_ptr() - buf.data_ptr() > 2 ** 33
    _, beta = _vector(R, torch.float32, 0xFF)
    idx_d = torch.from_numpy(idx).cuda()
    ops.tsne_perplexity(idx_d, torch.from_numpy(d2).cuda(), 1.5, beta=beta, p_cond=p_cond)
    torch.cuda.synchronize()
    got = p_cond.cpu().numpy()
    beta32, p32, _ = T.perplexity_search(idx, d2, 1.5, T.F32)
    x64, pres = T.shifted(idx, d2, T.F64)
    p_at, _, _ = T.evaluate(x64, pres, beta.cpu().numpy().astype(np.float64), T.F64)
    p_ref, _, _ = T.evaluate(x64, pres, beta32.astype(np.float64), T.F64)
    yard = float(np.abs(p32 - p_ref).max())
    dev = float(np.abs(got - p_at).max())
    print(f"[tsne p_cond] ld = 2^30 + 8: device from the fp64 P at its beta by {dev:.3e}, yardstick {yard:.3e}")
    assert dev <= T.FACTOR * yard and np.allclose(got.sum(1), 1.0, atol=1e-6)
    rowptr, col = T.csr(idx, d2)
    p = torch.empty(col.shape[0], dtype=torch.float32, device="cuda")
    ops.tsne_joint(idx_d, p_cond, torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), p=p)      # row 2 of p_cond is read where it is
    torch.cuda.synchronize()
    assert _same_bits(p.cpu().numpy(), T.joint(idx, got, rowptr, col))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(T.FIXTURES))
def test_tsne_end_to_end_against_the_three_references(name):
    from variantformer_amd import manifold, neighbors
    pytest.importorskip("sklearn.manifold", reason="the references need scikit-learn")
    R, perplexity, m = T.FIXTURES[name]
    ref = T.fixture_references(name)
    for key, Y in ref["embeddings"].items():
        assert T.nearest_in_group(Y, ref["labels"]), f"the {key} reference holds condition (a) itself"
    kw = dict(perplexity=perplexity, n_neighbors=m, n_iter=T.N_ITER, exaggeration_iter=T.EXAGGERATION_ITER,
              early_exaggeration=T.EARLY_EXAGGERATION, init=ref["init"])
    y, kl_dev = manifold.tsne(ref["x"], return_kl=True, **kw)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == (R, 2) and np.isfinite(y).all()
    assert _same_bits(manifold.tsne(ref["x"], **kw), y), "two runs are equal bit for bit"
    # the pieces, as the whole puts them together
    t = torch.from_numpy(ref["x"]).cuda()
    idx, dist = neighbors.knn(t, k=m) if m <= 63 else manifold._knn_panels(t, m, "correlation")
    if m > 63:
        i63, d63 = neighbors.knn(t, k=63)
        assert torch.equal(idx[:, :63], i63) and torch.equal(dist[:, :63], d63), "the panel path lists in vf_knn_dot's order, bit for bit"
    graph = manifold.tsne_affinities(idx, dist, perplexity)
    assert int(graph[0][-1]) == R * (R - 1), "m = R - 1: the sparse P is the dense P"
    p_dense = T.dense(graph[0].cpu().numpy(), graph[1].cpu().numpy(), graph[2].cpu().numpy())
    p_ref = T.dense(*ref["graph"])
    print(f"[tsne fixture {name}] device P from the CPU's fp32 P by {np.abs(p_dense - p_ref).max():.2e} (largest {p_ref.max():.2e}): "
          f"the device's own fp32 correlations stand behind it")
    assert np.abs(p_dense - p_ref).max() <= 1e-3 * p_ref.max()
    lr = max(R / T.EARLY_EXAGGERATION / 4.0, 50.0)
    y1 = manifold.tsne_descent(graph, torch.from_numpy(ref["init"]).cuda(), 0, T.EXAGGERATION_ITER, exaggeration=T.EARLY_EXAGGERATION, momentum=0.5, learning_rate=lr)
    y2 = manifold.tsne_descent(graph, y1, T.EXAGGERATION_ITER, T.N_ITER, exaggeration=1.0, momentum=0.8, learning_rate=lr)
    assert _same_bits(y2.cpu().numpy(), y), "tsne is tsne_affinities and two tsne_descent calls"
    assert manifold.tsne_kl(graph, y2) == kl_dev
    kl_cpu = T.kl(graph[0].cpu().numpy(), graph[1].cpu().numpy(), graph[2].cpu().numpy(), y)
    assert abs(kl_cpu - kl_dev) <= 1e-6 * kl_cpu, "tsne_kl is the fp64 divergence over the device's P"
    # condition (a)
    assert T.nearest_in_group(y, ref["labels"]), f"every row's {T.NEAREST} nearest rows in the device embedding belong to its own group"
    # condition (b): g is the largest relative gap among the three references' KL
    kls = list(ref["kl"].values())
    g = max(abs(a - b) / min(a, b) for a in kls for b in kls)
    print(f"[tsne fixture {name}] KL: device {kl_dev:.5f}; references {', '.join(f'{k} {v:.5f}' for k, v in ref['kl'].items())}; g = {g:.4f}; "
          f"bound {max(kls) * (1 + g):.5f}")
    assert kl_dev <= max(kls) * (1 + g)


def test_expression_tsne_adds_columns_and_equals_manifold_tsne():
    from variantformer_amd import manifold
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    x, _ = T.clusters(48, d=6)
    frame = pd.DataFrame({"gene_id": [f"G{i}" for i in range(48)], "tissues": [list(range(6))] * 48,
                          "tissue_names": [[f"t{j}" for j in range(6)]] * 48, "predicted_expression": list(x)})
    kw = dict(perplexity=8.0, n_iter=60, exaggeration_iter=20, seed=3)
    out = VCFProcessor.expression_tsne(VCFProcessor.__new__(VCFProcessor), frame, **kw)
    want = manifold.tsne(np.stack(list(frame["predicted_expression"])), **kw)
    assert _same_bits(out["coords"], want), "the processor's call is manifold.tsne on the same matrix"
    assert list(frame.columns[-2:]) == ["tsne_1", "tsne_2"] and frame["tsne_1"].dtype == np.float32
    assert _same_bits(frame[["tsne_1", "tsne_2"]].to_numpy(), want), "the columns are in row order"
    assert len(out["labels"]) == 48
    three = manifold.tsne(x, n_components=3, init="random", **kw)
    assert three.shape == (48, 3) and np.isfinite(three).all()
    called = manifold.tsne(x, init=lambda graph, n, seed: manifold.random_init(48, n, seed) * 1e-4, **kw)
    assert called.shape == (48, 2) and np.isfinite(called).all()
    with pytest.raises(ValueError, match="no finite spread"):
        manifold.tsne(np.ones((48, 6), dtype=np.float32), **kw)      # identical rows: the PCA start is all zero, nothing to scale

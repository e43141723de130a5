"""vf_umap_smooth_knn, vf_umap_union and vf_umap_layout on the GPU (include/vf_hip_umap.h) through their ops wrappers, against the
fp64 numpy references of tests/umap_cases.py: selections and integers (rho, the CSR arrays, the due sets and negative vertices
through the positions they produce) exactly, the rest within the bounds recorded there, each printed before it is asserted.
Operands sit in guarded buffers with odd row strides, outputs are poisoned and guarded: nothing outside the write set changes
and nothing inside it keeps the pattern.  Then rows that start past 2^31 elements."""
import numpy as np
import pytest
import torch

from tests import umap_cases as U
from tests import write_set_cases as W

pytestmark = pytest.mark.gpu

GUARD = 64                      # guard elements / rows either side of an output
EXTRA_LD = 5                    # columns behind the matrix, in operands and outputs alike: m + 5 and dim + 5 are odd strides for the table


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


def _matrix_out(rows: int, cols: int, pattern: int):
    big = W.poisoned((rows + 2 * GUARD, cols + EXTRA_LD), torch.float32, W.DEVICE, pattern)
    return big, big[GUARD:GUARD + rows, :cols]


def _check_matrix(name: str, big: torch.Tensor, rows: int, cols: int, pattern: int):
    h = big.cpu().numpy().view(np.uint8).reshape(rows + 2 * GUARD, -1, 4)
    assert (h[:GUARD] == pattern).all() and (h[GUARD + rows:] == pattern).all(), f"{name}: guard rows were written"
    assert (h[GUARD:GUARD + rows, cols:] == pattern).all(), f"{name}: columns past the write set were written"


def _operand(x: np.ndarray, pattern: int) -> torch.Tensor:
    """The matrix as a [rows, cols] view of rows cols + EXTRA_LD apart, the pattern behind the columns and in guard rows around."""
    rows, cols = x.shape
    wide = np.zeros((rows, cols + EXTRA_LD), dtype=x.dtype)
    wide.view(np.uint8)[:] = pattern
    wide[:, :cols] = x
    return W.guarded(torch.from_numpy(wide), pattern, rows=GUARD)[:, :cols]


def _same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- smooth_knn ----------------------------------------------------------------------------------------------------------------------
def _smooth(idx, dist, mean_dist, pattern):
    ops = _ops()
    R, m = idx.shape
    idx_d, dist_d = _operand(idx, pattern), _operand(dist, pattern)
    assert idx_d.stride(0) == dist_d.stride(0) == m + EXTRA_LD
    br, rho = _vector(R, torch.float32, pattern)
    bs, sigma = _vector(R, torch.float32, pattern)
    bt, strength = _matrix_out(R, m, pattern)
    ops.umap_smooth_knn(idx_d, dist_d, mean_dist, rho=rho, sigma=sigma, strength=strength)
    torch.cuda.synchronize()
    _check_vector("rho", br, R, pattern)
    _check_vector("sigma", bs, R, pattern)
    _check_matrix("strength", bt, R, m, pattern)
    assert np.array_equal(idx_d.cpu().numpy(), idx) and _same_bits(dist_d.cpu().numpy(), dist), "idx and dist are only read"
    return rho.cpu().numpy(), sigma.cpu().numpy(), strength.cpu().numpy()


_WORST = {"sigma": 0.0, "strength": 0.0, "residual": 0.0}


@pytest.mark.parametrize("m", U.MS)
@pytest.mark.parametrize("R", U.RS)
def test_smooth_knn_equals_the_reference(R, m):
    worst = dict.fromkeys(_WORST, 0.0)
    for kind in U.SMOOTH_KINDS:
        idx, dist = U.smooth_case(kind, R, m)
        mean_dist = U.mean_distance(idx, dist)
        rho_ref, sigma_ref, strength_ref, converged, floored = U.smooth_knn(idx, dist, mean_dist)
        for pattern in (W.PATTERNS if kind in ("random", "nonfinite") else W.PATTERNS[:1]):
            rho, sigma, strength = _smooth(idx, dist, mean_dist, pattern)
            assert _same_bits(rho, rho_ref), (kind, "rho is a selection", np.flatnonzero(rho != rho_ref)[:4].tolist())
            assert np.isfinite(sigma).all() and np.isfinite(strength).all() and (sigma >= 0).all(), kind
            present = U.present(idx, dist)
            own = idx == np.arange(R)[:, None]
            assert (strength[~present | own] == 0).all() and ((strength >= 0) & (strength <= 1)).all(), kind
            none = ~present.any(1)
            assert (sigma[none] == 0).all() and (sigma[~none] > 0).all(), kind
            live = sigma_ref > 0
            # a row whose bisection ran all 64 steps without converging and whose floor does not bind ends at 2^-64 or so in
            # both; there the last bits of the sums decide the steps, and the strengths (all 1 or 0) are what is compared
            compare = live & (converged | floored)
            rel = float((np.abs(sigma[compare] - sigma_ref[compare]) / sigma_ref[compare]).max()) if compare.any() else 0.0
            err = float(np.abs(strength - strength_ref).max())
            solved = converged & ~floored
            res = float(U.smooth_residual(idx, dist, rho, sigma)[solved].max()) if solved.any() else 0.0
            worst = {"sigma": max(worst["sigma"], rel), "strength": max(worst["strength"], err), "residual": max(worst["residual"], res)}
            print(f"[umap smooth_knn] R={R} m={m} {kind} pattern={pattern:#x}: sigma rel {rel:.2e}, strength abs {err:.2e}, residual {res:.2e}")
            assert rel <= U.SIGMA_RTOL and err <= U.STRENGTH_ATOL and res <= U.RESIDUAL_ATOL, (kind, rel, err, res)
    for key in _WORST:
        _WORST[key] = max(_WORST[key], worst[key])
    print(f"[umap smooth_knn] so far: sigma rel {_WORST['sigma']:.3e} (recorded {U.SIGMA_MEASURED:.1e}), strength abs {_WORST['strength']:.3e} "
          f"(recorded {U.STRENGTH_MEASURED:.1e}), residual {_WORST['residual']:.3e} (recorded {U.RESIDUAL_MEASURED:.1e}); asserted at 8x")
    assert U.SIGMA_RTOL == 8 * U.SIGMA_MEASURED and U.STRENGTH_ATOL == 8 * U.STRENGTH_MEASURED and U.RESIDUAL_ATOL == 8 * U.RESIDUAL_MEASURED


# ---- union ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,m", [(1, 1), (63, 2), (64, 29), (65, 63), (257, 5), (257, 29)])
def test_union_equals_the_reference_and_is_symmetric_bit_for_bit(R, m):
    from variantformer_amd import manifold
    ops = _ops()
    idx, dist = U.smooth_case("absent-tails", R, m)
    if R > 8:
        idx[7], dist[7] = -1, np.inf                                  # lists nobody; others may list it
        five = idx == 5
        idx[five], dist[five] = -1, np.inf
        idx[5], dist[5] = -1, np.inf                                  # no edge at all
    _, _, strength64, _, _ = U.smooth_knn(idx, dist, U.mean_distance(idx, dist))
    strength = strength64.astype(np.float32)
    rowptr, col = U.csr(idx, dist)
    nnz = col.shape[0]
    want = U.union(idx, strength, rowptr, col)
    i, j = U.entry_rows(rowptr), col.astype(np.int64)
    if R > 8:
        assert rowptr[5] == rowptr[6] and nnz > 0
    if R > 8 and m >= 5:
        listed = {(r, int(c)) for r in range(R) for c in idx[r] if c >= 0}
        assert any((b, a) in listed for a, b in listed) and any((b, a) not in listed for a, b in listed), "mutual and one-way edges"
    for pattern in W.PATTERNS:
        idx_d, strength_d = _operand(idx, pattern), _operand(strength, pattern)
        rowptr_d = W.guarded(torch.from_numpy(rowptr), pattern, rows=GUARD)
        col_d = W.guarded(torch.from_numpy(col), pattern, rows=GUARD)
        bw, w = _vector(nnz, torch.float32, pattern)
        ops.umap_union(idx_d, strength_d, rowptr_d, col_d, w=w)
        torch.cuda.synchronize()
        _check_vector("w", bw, nnz, pattern)
        got = w.cpu().numpy()
        err = float(np.abs(got - want).max()) if nnz else 0.0
        print(f"[umap union] R={R} m={m} nnz={nnz} pattern={pattern:#x}: w abs {err:.2e} (recorded {U.UNION_MEASURED:.1e}, asserted {U.UNION_ATOL:.1e})")
        assert U.UNION_ATOL == 8 * U.UNION_MEASURED and err <= U.UNION_ATOL
        back = np.zeros((R, R), dtype=np.uint32)
        back[i, j] = got.view(np.uint32)
        assert np.array_equal(back, back.T), "w[i -> j] and w[j -> i] have the same bits"
        assert np.array_equal(idx_d.cpu().numpy(), idx) and _same_bits(strength_d.cpu().numpy(), strength)
        assert np.array_equal(rowptr_d.cpu().numpy(), rowptr) and np.array_equal(col_d.cpu().numpy(), col)
    # the library's own graph: CSR integer-equal to the reference, rho exact, the rest within the bounds
    g_rowptr, g_col, g_w, g_rho, g_sigma = manifold.fuzzy_graph(idx, dist)
    assert g_rowptr.dtype == np.int64 and g_col.dtype == np.int32 and g_w.dtype == np.float32
    assert np.array_equal(g_rowptr, rowptr) and np.array_equal(g_col, col), "the CSR structure"
    rho_ref, sigma_ref, _, converged, floored = U.smooth_knn(idx, dist, U.mean_distance(idx, dist))
    assert _same_bits(g_rho, rho_ref)
    err = float(np.abs(g_w - U.union(idx, strength64, rowptr, col)).max()) if nnz else 0.0
    print(f"[umap union] R={R} m={m}: fuzzy_graph's w against the all-fp64 chain abs {err:.2e}")
    assert err <= 2 * U.STRENGTH_ATOL + U.UNION_ATOL, "d(a + b - a b) <= da + db"
    t = manifold.fuzzy_graph(torch.from_numpy(idx).cuda(), torch.from_numpy(dist).cuda())
    assert all(v.is_cuda for v in t) and _same_bits(t[2].cpu().numpy(), g_w), "tensors in, tensors out, the same graph"


# ---- layout --------------------------------------------------------------------------------------------------------------------------
def _run_layout(case, begin, end, pattern=0xFF, Y=None, rate=None, lr=1.0):
    """(result fp32 [R, dim], the other buffer) of ops.umap_layout on poisoned, guarded position buffers; the write set asserted."""
    ops = _ops()
    Y = case.Y if Y is None else Y
    R, dim = Y.shape
    rowptr, col, samples = torch.from_numpy(case.rowptr).cuda(), torch.from_numpy(case.col).cuda(), torch.from_numpy(case.samples).cuda()
    b0, y0 = _matrix_out(R, dim, pattern)
    b1, y1 = _matrix_out(R, dim, pattern)
    y0.copy_(torch.from_numpy(Y))
    out = ops.umap_layout(rowptr, col, samples, y0, y1, epoch_begin=begin, epoch_end=end, n_epochs=case.N, a=case.a, b=case.b, learning_rate=lr,
                          negative_sample_rate=case.rate if rate is None else rate, seed=case.seed)
    torch.cuda.synchronize()
    assert out is (y0 if (end - begin) % 2 == 0 else y1), "the parity of the epoch count names the buffer"
    _check_matrix("Y0", b0, R, dim, pattern)
    _check_matrix("Y1", b1, R, dim, pattern)
    other = y1 if out is y0 else y0
    return out.cpu().numpy(), other.cpu().numpy()


def _reference(case, begin, end, Y=None, rate=None, lr=1.0):
    return U.layout(case.rowptr, case.col, case.samples, case.Y if Y is None else Y, begin, end, case.N, case.a, case.b, 1.0, lr,
                    case.rate if rate is None else rate, case.seed)


@pytest.mark.parametrize("R,dim", [(1, 2), (63, 1), (64, 2), (65, 3), (257, 2), (257, 8)])
def test_layout_equals_the_reference(R, dim):
    case = U.layout_case(R, dim)
    if R >= 63:
        deg = np.diff(case.rowptr)
        assert deg[case.isolated] == 0 and deg[case.idle] > 0 and (case.samples[case.rowptr[case.idle]:case.rowptr[case.idle + 1]] == 0).all()
        assert (case.samples == case.N).any() and ((case.samples > 0) & (case.samples < case.N)).any()
    for n in (0, 3, case.N - 1):                                       # one epoch from a given state: the due sets and the negative vertices
        for pattern in (W.PATTERNS if n == 3 else W.PATTERNS[:1]):
            got, before = _run_layout(case, n, n + 1, pattern)
            want = _reference(case, n, n + 1)
            err = float(np.abs(got - want).max())
            print(f"[umap layout] R={R} dim={dim} epoch {n} pattern={pattern:#x}: abs {err:.2e} (recorded {U.LAYOUT_1_MEASURED:.1e}, asserted {U.LAYOUT_1_ATOL:.1e})")
            assert U.LAYOUT_1_ATOL == 8 * U.LAYOUT_1_MEASURED and err <= U.LAYOUT_1_ATOL
            assert _same_bits(before, case.Y), "the input buffer of the last epoch is unchanged"
            if R >= 63:
                for v in (case.isolated, case.idle):
                    assert _same_bits(got[v], case.Y[v]), "a vertex without entries, and one with nothing due, are copied through"
                if n == 3:                                            # at epoch 0 only the entries with samples == N are due
                    assert (got != case.Y).any(1).sum() > R // 2, "the others move"
    # ten epochs against fp64 at the gentle step U.LAYOUT_10_LR (why: tests/umap_cases.py); everything bit-exact below at step 1
    slow, _ = _run_layout(case, 0, case.N, lr=U.LAYOUT_10_LR)
    want = _reference(case, 0, case.N, lr=U.LAYOUT_10_LR)
    err = float(np.abs(slow - want).max())
    if R > 1:
        assert np.abs(want - case.Y).max() > 0.5, "ten epochs at this step still move the vertices"
    print(f"[umap layout] R={R} dim={dim} epochs 0..{case.N} at learning_rate {U.LAYOUT_10_LR}: abs {err:.2e} (recorded {U.LAYOUT_10_MEASURED:.1e}, asserted {U.LAYOUT_10_ATOL:.1e})")
    assert U.LAYOUT_10_ATOL == 8 * U.LAYOUT_10_MEASURED and err <= U.LAYOUT_10_ATOL
    got, before = _run_layout(case, 0, case.N)
    assert np.isfinite(got).all() and np.isfinite(slow).all()
    again, _ = _run_layout(case, 0, case.N, 0x3C)
    assert _same_bits(again, got), "two runs are equal bit for bit"
    half, _ = _run_layout(case, 0, case.N // 2)
    rest, previous = _run_layout(case, case.N // 2, case.N, Y=half)
    assert _same_bits(rest, got), "[0, 10) equals [0, 5) then [5, 10) bit for bit"
    assert case.N == 10 and (case.N - case.N // 2) % 2 == 1 and _same_bits(_run_layout(case, case.N // 2, case.N - 1, Y=half)[0], previous), \
        "the other buffer holds the positions one epoch earlier"
    none, _ = _run_layout(case, 4, 4)
    assert _same_bits(none, case.Y), "an empty range launches nothing"


def test_layout_without_negatives_and_with_another_rate():
    case = U.layout_case(65, 2)
    for rate in (0, 1, 2):
        got, _ = _run_layout(case, 3, 4, rate=rate)
        err = float(np.abs(got - _reference(case, 3, 4, rate=rate)).max())
        print(f"[umap layout] rate={rate}, epoch 3: abs {err:.2e} (recorded {U.LAYOUT_1_MEASURED:.1e}, asserted {U.LAYOUT_1_ATOL:.1e})")
        assert err <= U.LAYOUT_1_ATOL
        assert (got != case.Y).any(1).sum() > 32
    assert not _same_bits(_run_layout(case, 3, 4, rate=0)[0], _run_layout(case, 3, 4, rate=1)[0]), "the repulsions count"


def test_coincident_points_do_not_move_and_make_no_nan():
    case = U.layout_case(65, 3)
    Y = np.tile(np.array([[2.5, 7.0, 0.0]], dtype=np.float32), (65, 1))
    got, _ = _run_layout(case, 0, 3, Y=Y)
    assert _same_bits(got, Y), "every d2 is 0: no attraction, no repulsion, no NaN"
    Y2 = case.Y.copy()
    Y2[20] = Y2[int(case.col[case.rowptr[20]])]                        # one vertex on top of its first neighbour
    got, _ = _run_layout(case, 0, 1, Y=Y2)
    assert np.isfinite(got).all()
    err = float(np.abs(got - _reference(case, 0, 1, Y=Y2)).max())
    print(f"[umap layout] one vertex on its neighbour, epoch 0: abs {err:.2e}")
    assert err <= U.LAYOUT_1_ATOL


def test_rows_that_start_past_2_31_elements():
    """R = 3 with rows 2^30 + 8 elements apart: the third row starts past 2^31 elements and 8 GiB, in dist, in strength and in
    both position buffers.  Only the used elements are written before the calls."""
    ops = _ops()
    R, m, ld = 3, 2, 2 ** 30 + 8
    assert (R - 1) * ld > 2 ** 31
    idx = np.array([[1, 2], [2, 0], [0, -1]], dtype=np.int32)
    dist = np.array([[0.25, 0.5], [0.125, 0.75], [0.5, np.inf]], dtype=np.float32)
    bufs = [torch.empty(2 * ld + 8, dtype=torch.float32, device="cuda") for _ in range(2)]
    dist_d, strength = (b.as_strided((R, m), (ld, 1)) for b in bufs)
    dist_d.copy_(torch.from_numpy(dist).cuda())
    strength.fill_(7.0)
    assert dist_d[2].data_ptr() - bufs[0].data_ptr() > 2 ** 33
    _, rho = _vector(R, torch.float32, 0xFF)
    _, sigma = _vector(R, torch.float32, 0xFF)
    mean_dist = U.mean_distance(idx, dist)
    idx_d = torch.from_numpy(idx).cuda()
    ops.umap_smooth_knn(idx_d, dist_d, mean_dist, rho=rho, sigma=sigma, strength=strength)
    torch.cuda.synchronize()
    rho_ref, sigma_ref, strength_ref, _, _ = U.smooth_knn(idx, dist, mean_dist)
    assert _same_bits(rho.cpu().numpy(), rho_ref) and rho_ref.tolist() == [0.25, 0.125, 0.5]
    assert np.abs(sigma.cpu().numpy() - sigma_ref).max() <= U.SIGMA_RTOL * sigma_ref.max()
    got = strength.cpu().numpy()
    assert np.abs(got - strength_ref).max() <= U.STRENGTH_ATOL and got[2, 1] == 0 and got[2, 0] == 1
    rowptr, col = U.csr(idx, dist)
    w = torch.empty(col.shape[0], dtype=torch.float32, device="cuda")
    ops.umap_union(idx_d, strength, torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), w=w)      # row 2 of strength is read where it is
    torch.cuda.synchronize()
    assert np.abs(w.cpu().numpy() - U.union(idx, got, rowptr, col)).max() <= U.UNION_ATOL
    # the layout with both position buffers strided the same way (the two buffers of this test are reused)
    del dist_d, strength
    y0, y1 = (b.as_strided((R, 2), (ld, 1)) for b in bufs)
    Y = np.array([[0.0, 0.0], [10.0, 1.0], [4.0, 9.0]], dtype=np.float32)
    y0.copy_(torch.from_numpy(Y).cuda())
    y1.fill_(-1.0)
    samples = np.full(col.shape[0], 4, dtype=np.int32)
    out = ops.umap_layout(torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(samples).cuda(), y0, y1,
                          epoch_begin=0, epoch_end=3, n_epochs=4, a=1.577, b=0.895, seed=1)
    torch.cuda.synchronize()
    assert out is y1
    want = U.layout(rowptr, col, samples, Y, 0, 3, 4, 1.577, 0.895, 1.0, 1.0, 5, 1)
    got = out.cpu().numpy()
    print(f"[umap layout] rows 2^30 + 8 apart, three epochs: abs {np.abs(got - want).max():.2e}")
    assert np.abs(got - want).max() <= U.LAYOUT_10_ATOL and (got != Y).any(1).all(), "every vertex moved, the third among them"
    del y0, y1, out, bufs
    torch.cuda.empty_cache()

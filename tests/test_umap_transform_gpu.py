"""vf_umap_smooth_knn_query, vf_umap_init_transform and vf_umap_layout_transform on the GPU (include/vf_hip_umap_transform.h)
through their ops wrappers, against the numpy restatements of tests/umap_transform_cases.py, and manifold.fit /
UMAPModel.transform as a whole.  Selections, integers and the start are held exactly (the due sets and the negative vertices
through the positions one epoch produces from a given state: a wrong vertex moves a query by thousands of times the bound), the
rest within the bounds recorded there, each printed before it is asserted.  Operands sit in guarded buffers with odd row
strides, outputs are poisoned and guarded: nothing outside the write set changes.  Then rows 2^30 + 8 elements apart."""
import numpy as np
import pytest
import torch

from tests import umap_cases as U
from tests import umap_transform_cases as T
from tests import write_set_cases as W

pytestmark = pytest.mark.gpu

GUARD = 64                      # guard rows either side of a buffer
EXTRA_LD = 5                    # columns behind the matrix, in operands and outputs alike: m + 5 and dim + 5


def _ops():
    from variantformer_amd import _lib, ops
    _lib.load()
    return ops


def _vector(n: int, pattern: int):
    big = W.poisoned((n + 2 * GUARD,), torch.float32, W.DEVICE, pattern)
    return big, big[GUARD:GUARD + n]


def _check_vector(name: str, big: torch.Tensor, n: int, pattern: int):
    h = big.cpu().numpy().view(np.uint8)
    assert (h[:4 * GUARD] == pattern).all() and (h[4 * (GUARD + n):] == pattern).all(), f"{name}: guard elements were written"


def _matrix_out(rows: int, cols: int, pattern: int):
    big = W.poisoned((rows + 2 * GUARD, cols + EXTRA_LD), torch.float32, W.DEVICE, pattern)
    return big, big[GUARD:GUARD + rows, :cols]


def _check_matrix(name: str, big: torch.Tensor, rows: int, cols: int, pattern: int):
    h = big.cpu().numpy().view(np.uint8).reshape(rows + 2 * GUARD, -1, 4)
    assert (h[:GUARD] == pattern).all() and (h[GUARD + rows:] == pattern).all(), f"{name}: guard rows were written"
    assert (h[GUARD:GUARD + rows, cols:] == pattern).all(), f"{name}: columns past the write set were written"


def _operand(x: np.ndarray, pattern: int):
    """(the whole buffer, the matrix as a [rows, cols] view of rows cols + EXTRA_LD apart): the pattern behind the columns (a NaN
    for 0xFF) and in guard rows around."""
    rows, cols = x.shape
    wide = np.zeros((rows, cols + EXTRA_LD), dtype=x.dtype)
    wide.view(np.uint8)[:] = pattern
    wide[:, :cols] = x
    view = W.guarded(torch.from_numpy(wide), pattern, rows=GUARD)
    return view, view[:, :cols]


def _unchanged(name: str, whole: torch.Tensor, x: np.ndarray, pattern: int):
    """An operand is only read: its matrix keeps its bits and the gap columns keep the pattern."""
    h = whole.cpu().numpy()
    assert _same_bits(h[:, :x.shape[1]], x), f"{name} is only read"
    assert (np.ascontiguousarray(h[:, x.shape[1]:]).view(np.uint8) == pattern).all(), f"{name}: gap columns were written"


def _same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- smooth_knn_query ------------------------------------------------------------------------------------------------------------------
def _smooth(idx, dist, mean_dist, pattern):
    ops = _ops()
    Rq, m = idx.shape
    (wi, idx_d), (wd, dist_d) = _operand(idx, pattern), _operand(dist, pattern)
    assert idx_d.stride(0) == dist_d.stride(0) == m + EXTRA_LD
    bs, sigma = _vector(Rq, pattern)
    bt, strength = _matrix_out(Rq, m, pattern)
    ops.umap_smooth_knn_query(idx_d, dist_d, mean_dist, sigma=sigma, strength=strength)
    torch.cuda.synchronize()
    _check_vector("sigma", bs, Rq, pattern)
    _check_matrix("strength", bt, Rq, m, pattern)
    _unchanged("idx", wi, idx, pattern)
    _unchanged("dist", wd, dist, pattern)
    return sigma.cpu().numpy(), strength.cpu().numpy()


_WORST = {"sigma": 0.0, "strength": 0.0, "layout_1": 0.0, "layout_10": 0.0}


@pytest.mark.parametrize("m", T.SMOOTH_MS)
@pytest.mark.parametrize("Rq", T.RQS)
def test_smooth_knn_query_equals_the_restatement(Rq, m):
    worst = {"sigma": 0.0, "strength": 0.0}
    for kind in T.SMOOTH_KINDS:
        idx, dist = T.smooth_case(kind, Rq, m)
        for mean_dist in ((0.7, float("nan"), float("inf")) if kind == "random" else (0.7,)):
            sigma_ref, strength_ref, converged, floored, open_ended = T.smooth_knn_query(idx, dist, mean_dist)
            for pattern in (W.PATTERNS if kind in ("random", "nonfinite") and mean_dist == 0.7 else W.PATTERNS[:1]):
                sigma, strength = _smooth(idx, dist, mean_dist, pattern)
                present = U.present(idx, dist)
                assert not np.isnan(sigma).any() and not np.isnan(strength).any() and (sigma >= 0).all(), kind
                assert _same_bits(strength[~present], np.zeros((~present).sum(), dtype=np.float32)), (kind, "an absent entry has strength +0")
                assert ((strength >= 0) & (strength <= 1)).all(), kind
                assert (strength[present & (dist <= 0)] == 1).all(), (kind, "a distance of zero or below has strength 1")
                # (a present entry far out may underflow to 0 in fp32 alone, and one very near may round to 1 in fp32 alone)
                assert (strength[strength_ref == 1] == 1).all() and (strength[strength_ref == 0] == 0).all(), (kind, "the ones and the zeros")
                none = ~present.any(1)
                assert (sigma[none] == 0).all() and (sigma[~none] > 0).all(), kind
                if kind == "own-row":
                    assert (idx[:, 0] == np.arange(Rq)).all() and (dist[:, 0] > 0).all() and (strength[:, 0] > 0).all(), \
                        "an index equal to the row's own number names a training row: its strength is not zeroed"
                if np.isinf(mean_dist):
                    assert (sigma[~none] == np.inf).all() and (strength[present] == 1).all()
                    continue
                # a row whose bisection ran all 64 steps without converging and whose floor does not bind ends near 2^-64 in
                # both; there the last bits of the sums decide the steps, and the strengths (all 1 or 0) are what is compared
                # A row that converges while the search is still open-ended (as many present entries as log2(m): one of m = 2,
                # two of m = 4; or m = 1) doubles or halves mid per step, and |sum - target| passes 1e-5 within fp32's
                # resolution of the sum: the device may stop one step from the restatement, a factor of exactly two in sigma
                # and at most the tolerance in the strengths.  Such a row is held to the nearest of sigma / 2, sigma, 2 sigma.
                compare = (sigma_ref > 0) & (converged | floored)
                rel = float(T.sigma_deviation(sigma, sigma_ref, open_ended & ~floored)[compare].max()) if compare.any() else 0.0
                err = float(np.abs(strength - strength_ref).max())
                worst = {"sigma": max(worst["sigma"], rel), "strength": max(worst["strength"], err)}
                print(f"[umap transform smooth] Rq={Rq} m={m} {kind} mean_dist={mean_dist} pattern={pattern:#x}: sigma rel {rel:.2e}, strength abs {err:.2e}")
                assert rel <= T.SIGMA_RTOL and err <= T.STRENGTH_ATOL, (kind, rel, err)
    for key in worst:
        _WORST[key] = max(_WORST[key], worst[key])
    print(f"[umap transform smooth] so far: sigma rel {_WORST['sigma']:.3e} (recorded {T.SIGMA_MEASURED:.1e}), strength abs {_WORST['strength']:.3e} "
          f"(recorded {T.STRENGTH_MEASURED:.1e}); asserted at 8x")
    assert T.SIGMA_RTOL == 8 * T.SIGMA_MEASURED and T.STRENGTH_ATOL == 8 * T.STRENGTH_MEASURED


# ---- init_transform --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Rq,m,R,dim", [(1, 1, 1, 1), (2, 2, 2, 2), (63, 15, 65, 3), (64, 30, 1000, 8), (65, 63, 1000, 2), (257, 64, 65, 2),
                                        (257, 2, 2, 8), (65, 64, 1, 3)])
def test_init_transform_equals_the_fp32_restatement_bit_for_bit(Rq, m, R, dim):
    ops = _ops()
    g = np.random.default_rng(31 * Rq + m + R + dim)
    idx = g.integers(-1, R + 1, (Rq, m)).astype(np.int32)             # -1 and R among them: skipped
    w = g.uniform(0.001, 1.0, (Rq, m)).astype(np.float32)
    w[g.uniform(size=w.shape) < 0.1] = 0                               # absent entries carry +0
    w[g.uniform(size=w.shape) < 0.1] = 1
    Y = U.rescale(U.random_init(R, dim, 5 + R)) if R > 1 else np.full((1, dim), 3.25, dtype=np.float32)
    if Rq >= 63:
        idx[3] = np.where(np.arange(m) % 2 == 0, -1, R)                # no usable neighbour
        w[7] = 0                                                       # usable neighbours, S == 0
        idx[7] = 0
    want = T.init_transform(idx, w, Y)
    if Rq >= 63:
        assert np.isnan(want[3]).all() and np.isnan(want[7]).all() and np.isfinite(want).any()
        assert (idx == -1).any() and (idx == R).any()
    for pattern in W.PATTERNS:
        (wi, idx_d), (ww, w_d), (wy, Y_d) = _operand(idx, pattern), _operand(w, pattern), _operand(Y, pattern)
        bq, yq = _matrix_out(Rq, dim, pattern)
        ops.umap_init_transform(idx_d, w_d, Y_d, out=yq)
        torch.cuda.synchronize()
        _check_matrix("Yq", bq, Rq, dim, pattern)
        _unchanged("idx", wi, idx, pattern)
        _unchanged("strength", ww, w, pattern)
        _unchanged("Y", wy, Y, pattern)
        got = yq.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)), "a row without a usable neighbour, or with S == 0, is NaN; no other is"
        assert np.array_equal(got, want, equal_nan=True), (np.abs(got - want)[~np.isnan(want)].max(), "every operation is rounded once, in order")


# ---- layout_transform ------------------------------------------------------------------------------------------------------------------
LAYOUT_TABLE = [  # Rq, R, dim, m, rate, N, first_row
    (1, 1, 1, 1, 0, 1, 0), (2, 2, 2, 2, 1, 2, 5), (63, 3, 3, 30, 5, 10, 0), (64, 100, 8, 64, 7, 33, 5), (65, 1000, 2, 30, 5, 10, 2 ** 32 - 65),
    (257, 1000, 2, 64, 5, 33, 0), (257, 100, 3, 2, 1, 10, 5), (65, 1, 2, 30, 5, 10, 0)]


class _Layout:
    """One case on the device: the operands in guarded buffers, uploaded once per pattern."""

    def __init__(self, case, rate, N, first_row, pattern=0xFF):
        self.idx, self.cnt, self.Y, self.Yq = case
        self.rate, self.N, self.first_row, self.pattern = rate, N, first_row, pattern
        (self.wi, self.idx_d), (self.wc, self.cnt_d), (self.wy, self.Y_d) = (_operand(v, pattern) for v in (self.idx, self.cnt, self.Y))

    def run(self, begin, end, Yq=None, lr=1.0, rows=None, first_row=None):
        """fp32 positions after the epochs [begin, end) from Yq, on a poisoned, guarded buffer; the write set asserted."""
        ops = _ops()
        Yq = self.Yq if Yq is None else Yq
        rows = slice(0, Yq.shape[0]) if rows is None else rows
        bq, yq = _matrix_out(Yq.shape[0], Yq.shape[1], self.pattern)
        yq.copy_(torch.from_numpy(Yq))
        out = ops.umap_layout_transform(self.idx_d[rows], self.cnt_d[rows], self.Y_d, yq, epoch_begin=begin, epoch_end=end, n_epochs=self.N,
                                        a=T.AB[0], b=T.AB[1], learning_rate=lr, negative_sample_rate=self.rate, seed=7,
                                        first_row=self.first_row if first_row is None else first_row)
        torch.cuda.synchronize()
        assert out is yq, "in place"
        _check_matrix("Yq", bq, Yq.shape[0], Yq.shape[1], self.pattern)
        return yq.cpu().numpy()

    def operands_unchanged(self):
        _unchanged("idx", self.wi, self.idx, self.pattern)
        _unchanged("samples", self.wc, self.cnt, self.pattern)
        _unchanged("Y", self.wy, self.Y, self.pattern)

    def reference(self, begin, end, Yq=None, lr=1.0):
        return T.layout_transform(self.idx, self.cnt, self.Y, self.Yq if Yq is None else Yq, begin, end, self.N, *T.AB, 1.0, lr, self.rate, 7,
                                  self.first_row)


@pytest.mark.parametrize("Rq,R,dim,m,rate,N,first_row", LAYOUT_TABLE)
def test_layout_transform_equals_the_restatement(Rq, R, dim, m, rate, N, first_row):
    case = T.layout_case(Rq, R, dim, m, N)
    dev = _Layout(case, rate, N, first_row)
    idx, cnt, Y, Yq = case
    nan_rows = np.isnan(Yq).any(1)
    assert nan_rows.sum() == (1 if Rq >= 63 else 0)
    if Rq >= 63:
        assert (cnt == 0).any() and (cnt == N).any() and (cnt == N + 1).any() and (cnt == -1).any() and (idx == -1).any() and (idx == R).any()
    ok = ~nan_rows
    # one epoch from a given state: which entries are due and which vertices repel, through the positions they produce
    for n in sorted({0, N // 3, N - 1}):
        for pattern in (W.PATTERNS if n == N // 3 else W.PATTERNS[:1]):
            d = dev if pattern == dev.pattern else _Layout(case, rate, N, first_row, pattern)
            got, want = d.run(n, n + 1), d.reference(n, n + 1)
            d.operands_unchanged()
            err = float(np.abs(got - want)[ok].max())
            _WORST["layout_1"] = max(_WORST["layout_1"], err)
            print(f"[umap transform layout] Rq={Rq} R={R} dim={dim} m={m} rate={rate} N={N} epoch {n} pattern={pattern:#x}: abs {err:.2e} "
                  f"(recorded {T.LAYOUT_1_MEASURED:.1e}, asserted {T.LAYOUT_1_ATOL:.1e})")
            assert T.LAYOUT_1_ATOL == 8 * T.LAYOUT_1_MEASURED and err <= T.LAYOUT_1_ATOL
            assert np.isnan(got[nan_rows]).all() and np.isnan(want[nan_rows]).all() and np.isfinite(got[ok]).all(), "a NaN query stays NaN and touches no other row"
    if Rq >= 63 and R > 1:
        trace = []
        T.layout_transform(idx, cnt, Y, Yq, 0, 1, N, *T.AB, rate=rate, seed=7, first_row=first_row, trace=trace)
        moved = np.zeros(Rq, dtype=bool)
        for _, _, rows, _ in trace:
            moved[rows] = True
        first = dev.run(0, 1)
        assert _same_bits(first[~moved & ok], Yq[~moved & ok]) and moved.sum() > 1, "a query with nothing due in the epoch keeps its bits"
        assert (first[moved & ok] != Yq[moved & ok]).any(1).sum() >= (moved & ok).sum() - 1, "the others move (one stands on its neighbour)"
    # up to ten epochs against fp64 at the gentle step (why: tests/umap_cases.py); more than one launch when N allows
    span = min(N, 10)
    slow, want = dev.run(0, span, lr=T.LAYOUT_10_LR), dev.reference(0, span, lr=T.LAYOUT_10_LR)
    err = float(np.abs(slow - want)[ok].max())
    _WORST["layout_10"] = max(_WORST["layout_10"], err)
    print(f"[umap transform layout] Rq={Rq} R={R} dim={dim} m={m} rate={rate} N={N} epochs 0..{span} at learning_rate {T.LAYOUT_10_LR}: abs {err:.2e} "
          f"(recorded {T.LAYOUT_10_MEASURED:.1e}, asserted {T.LAYOUT_10_ATOL:.1e})")
    assert T.LAYOUT_10_ATOL == 8 * T.LAYOUT_10_MEASURED and err <= T.LAYOUT_10_ATOL
    # everything below is bit-exact, at learning_rate 1
    whole = dev.run(0, N)
    assert np.isfinite(whole[ok]).all() and np.isnan(whole[nan_rows]).all()
    assert _same_bits(_Layout(case, rate, N, first_row, 0x3C).run(0, N), whole), "two runs are equal bit for bit"
    step = Yq
    for n in range(N):
        step = dev.run(n, n + 1, Yq=step)
    assert _same_bits(step, whole), "a run split at every epoch boundary equals the one call"
    if N > T.EPOCHS_PER_LAUNCH:
        cut = dev.run(T.EPOCHS_PER_LAUNCH, N, Yq=dev.run(0, T.EPOCHS_PER_LAUNCH))
        assert _same_bits(cut, whole), "and so does one split where the library's loop starts its second launch"
    assert _same_bits(dev.run(N // 2, N // 2), Yq), "an empty range launches nothing"
    for a, b in ((0, 1), (Rq // 3, Rq // 3 + 1), (Rq // 2, Rq), (Rq - 1, Rq)):
        if a < b <= Rq:
            part = dev.run(0, N, Yq=np.ascontiguousarray(Yq[a:b]), rows=slice(a, b), first_row=first_row + a)
            assert _same_bits(part, whole[a:b]), f"the rows [{a}, {b}) alone with first_row + {a} equal those rows of the whole run"
    if Rq > 1 and R > 1 and rate > 0:
        other = dev.run(0, N, first_row=first_row + 1 if first_row + Rq < 2 ** 32 else first_row - 1)
        assert not _same_bits(other[ok], whole[ok]), "the row number is in the hash"
    if R == 1 and Rq >= 63:
        assert _same_bits(whole[5], Yq[5]), "a query on the one training point: every d2 is 0, no move, no NaN"
    dev.operands_unchanged()
    print(f"[umap transform layout] so far: one epoch abs {_WORST['layout_1']:.3e} (recorded {T.LAYOUT_1_MEASURED:.1e}), ten epochs abs "
          f"{_WORST['layout_10']:.3e} (recorded {T.LAYOUT_10_MEASURED:.1e}); asserted at 8x")


REVEAL_ATOL = 0.05


@pytest.mark.parametrize("first_row", [0, 5, 2 ** 32 - 65])
def test_the_due_sets_and_the_negative_vertices_are_the_restatements(first_row):
    """A run whose result reveals the integers.  64 training rows stand at (+-1000, ..) in 8 coordinates, coordinate c < 6 of row k
    on the side that bit c of k names (6 and 7 mirror 0 and 1), and the queries start within [-1, 1]^8.  With gamma = 1e15 every
    repulsion is clipped: it moves the query by exactly 4 alpha per coordinate, AWAY from vertex k, so the signs spell k's six
    bits; the sides are balanced, so a query's walk stays far inside the box (asserted on the restatement: |y| < 128).  With
    a = b = 1 an attraction moves it by less than 1e-3 alpha.  One wrong bit of one negative vertex in the last of N = 10 epochs
    (alpha = 0.025) changes a coordinate by 8 alpha = 0.2, and a wrong due set changes an odd number of clipped moves per
    coordinate; fp32 rounding of the at most 1800 moves of a query at |y| < 128 is below 1800 * 2^-18 = 7e-3.  REVEAL_ATOL = 0.05
    lies between."""
    Rq, R, m, N, rate = 65, 64, 30, 10, 5
    idx, cnt, _, _ = T.layout_case(Rq, R, 8, m, N)
    k = np.arange(R)
    Y = np.where((k[:, None] >> np.arange(8)[None, :]) & 1, 1000.0, -1000.0).astype(np.float32)
    Y[:, 6:] = -Y[:, :2]
    Yq = (2.0 * U.random_init(Rq, 8, 77) - 1.0).astype(np.float32)
    ops = _ops()
    (_, idx_d), (_, cnt_d), (_, Y_d) = (_operand(v, 0xFF) for v in (idx, cnt, Y))
    bq, yq = _matrix_out(Rq, 8, 0xFF)
    yq.copy_(torch.from_numpy(Yq))
    ops.umap_layout_transform(idx_d, cnt_d, Y_d, yq, epoch_begin=0, epoch_end=N, n_epochs=N, a=1.0, b=1.0, gamma=1e15, negative_sample_rate=rate,
                              seed=11, first_row=first_row)
    torch.cuda.synchronize()
    _check_matrix("Yq", bq, Rq, 8, 0xFF)
    got = yq.cpu().numpy()
    trace = []
    want = T.layout_transform(idx, cnt, Y, Yq, 0, N, N, 1.0, 1.0, 1e15, 1.0, rate, 11, first_row, trace=trace)
    err = float(np.abs(got - want).max())
    vertices = np.concatenate([ks.reshape(-1) for _, _, _, ks in trace])
    print(f"[umap transform layout] revealing run, first_row={first_row}: abs {err:.2e} (asserted {REVEAL_ATOL}); {len(trace)} (epoch, entry) pairs due, "
          f"{np.unique(vertices).size} distinct negative vertices, the queries moved by up to {np.abs(want - Yq).max():.1f}")
    assert np.unique(vertices).size == R and np.abs(want - Yq).max() > 5 and np.abs(want).max() < 128
    assert err <= REVEAL_ATOL
    wrong = T.layout_transform(idx, cnt, Y, Yq, 0, N, N, 1.0, 1.0, 1e15, 1.0, rate, 12, first_row)
    assert np.abs(wrong - want).max() > 1.0, "another seed's vertices are far outside the bound"


def test_rates_zero_and_seven_and_a_query_on_its_negative():
    case = T.layout_case(65, 3, 2, 15, 10)
    idx, cnt, Y, Yq = case
    results = {}
    for rate in (0, 1, 5, 7):
        dev = _Layout(case, rate, 10, 0)
        got, want = dev.run(3, 4), dev.reference(3, 4)
        ok = ~np.isnan(Yq).any(1)
        err = float(np.abs(got - want)[ok].max())
        print(f"[umap transform layout] rate={rate}, epoch 3, R=3: abs {err:.2e} (recorded {T.LAYOUT_1_MEASURED:.1e}, asserted {T.LAYOUT_1_ATOL:.1e})")
        assert err <= T.LAYOUT_1_ATOL
        results[rate] = got
    assert not _same_bits(results[0], results[1]) and not _same_bits(results[5], results[7]), "the repulsions count"
    # row 5 stands on Y[0], its neighbour; with three training rows a third of its negatives are Y[0] too: d2 == 0, no move, no NaN
    assert _same_bits(Yq[5], Y[0]) and np.isfinite(results[7][5]).all()


def test_rows_that_start_past_2_31_elements():
    """Rq = 3 and R = 3 with rows 2^30 + 8 elements apart: the third row starts past 2^31 elements and 8 GiB in dist and strength,
    then in Y and Yq.  Only the used elements are written before the calls."""
    ops = _ops()
    Rq, m, ld = 3, 2, 2 ** 30 + 8
    assert (Rq - 1) * ld > 2 ** 31
    idx = np.array([[1, 2], [2, 0], [0, -1]], dtype=np.int32)
    dist = np.array([[0.25, 0.5], [0.125, 0.75], [0.5, np.inf]], dtype=np.float32)
    bufs = [torch.empty(2 * ld + 8, dtype=torch.float32, device="cuda") for _ in range(2)]
    dist_d, strength = (b.as_strided((Rq, m), (ld, 1)) for b in bufs)
    dist_d.copy_(torch.from_numpy(dist).cuda())
    strength.fill_(7.0)
    assert dist_d[2].data_ptr() - bufs[0].data_ptr() > 2 ** 33
    _, sigma = _vector(Rq, 0xFF)
    idx_d = torch.from_numpy(idx).cuda()
    ops.umap_smooth_knn_query(idx_d, dist_d, 0.4, sigma=sigma, strength=strength)
    torch.cuda.synchronize()
    sigma_ref, strength_ref = T.smooth_knn_query(idx, dist, 0.4)[:2]
    assert np.abs(sigma.cpu().numpy() - sigma_ref).max() <= T.SIGMA_RTOL * sigma_ref.max()
    w = strength.cpu().numpy()
    assert np.abs(w - strength_ref).max() <= T.STRENGTH_ATOL and w[2, 1] == 0 and (w[:, 0] > 0).all()
    del dist_d, strength
    # the training positions and the queries' positions strided the same way (the two buffers are reused)
    Y_d, yq = (b.as_strided((3, 2), (ld, 1)) for b in bufs)
    Y = np.array([[0.0, 0.0], [10.0, 1.0], [4.0, 9.0]], dtype=np.float32)
    Y_d.copy_(torch.from_numpy(Y).cuda())
    yq.fill_(-1.0)
    w_d = torch.from_numpy(w).cuda()
    ops.umap_init_transform(idx_d, w_d, Y_d, out=yq)
    torch.cuda.synchronize()
    y0 = yq.cpu().numpy()
    assert np.array_equal(y0, T.init_transform(idx, w, Y)) and np.isfinite(y0).all()
    cnt = np.array([[4, 2], [4, 3], [4, 4]], dtype=np.int32)
    out = ops.umap_layout_transform(idx_d, torch.from_numpy(cnt).cuda(), Y_d, yq, epoch_begin=0, epoch_end=3, n_epochs=4, a=1.577, b=0.895, seed=1)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = T.layout_transform(idx, cnt, Y, y0, 0, 3, 4, 1.577, 0.895, 1.0, 1.0, 5, 1)
    print(f"[umap transform layout] rows 2^30 + 8 apart, three epochs: abs {np.abs(got - want).max():.2e}")
    assert np.abs(got - want).max() <= T.LAYOUT_10_ATOL and (got != y0).any(1).all(), "every query moved, the third among them"
    assert np.array_equal(Y_d.cpu().numpy(), Y), "Y is never written"
    del Y_d, yq, out, bufs
    torch.cuda.empty_cache()


# ---- the whole -------------------------------------------------------------------------------------------------------------------------
def test_the_blob_queries_land_in_their_blobs_like_the_restatement():
    from variantformer_amd import manifold, neighbors
    x, lx, Y, q, lq = T.blobs()
    ref, ref0, mean_dist = T.blobs_reference()
    model = manifold.UMAPModel.from_state(T.blobs_state(x, Y, mean_dist))          # no fit is in the way
    N = T.BLOBS["n_epochs"]
    y = model.transform(q, n_epochs=N)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == (60, 2) and np.isfinite(y).all()
    found = T.nearest_training_label(Y, lx, y)
    print(f"[umap transform blobs] device: {(found == lq).sum()} of 60 queries nearest to a training point of their own blob")
    assert (found == lq).all(), "every query's nearest training point in the embedding has the query's blob label"
    idx, dist = neighbors.knn(x, k=15, queries=q)
    same, _ = T.transform(x, Y, q, 15, mean_dist, N, *T.AB, lists=(idx, dist))     # the restatement on the device's own lists
    err = float(np.abs(y - same).max())
    print(f"[umap transform blobs] {N} epochs, device against the restatement: abs {err:.2e} (recorded {T.WHOLE_MEASURED:.1e}, asserted {T.WHOLE_ATOL:.1e}); "
          f"against the restatement with its own fp64 search {np.abs(y - ref).max():.2e}")
    assert T.WHOLE_ATOL == 8 * T.WHOLE_MEASURED and err <= T.WHOLE_ATOL
    t_dev, t_ref = T.trust(x, q, Y, y), T.trust(x, q, Y, ref)
    print(f"[umap transform blobs] trustworthiness of [Y; transform(q)]: device {t_dev:.4f}, restatement {t_ref:.4f}; margin {T.TRUST_MARGIN}")
    assert t_dev >= t_ref - T.TRUST_MARGIN
    # determinism, types, chunks, the function form
    assert np.array_equal(model.transform(q, n_epochs=N), y) and np.array_equal(manifold.transform(model, q, n_epochs=N), y)
    t = model.transform(torch.from_numpy(q).cuda(), n_epochs=N)
    assert isinstance(t, torch.Tensor) and t.is_cuda and np.array_equal(t.cpu().numpy(), y), "torch in, torch out, the same bits"
    big = np.concatenate([q, q[::-1], q, q[::-1], q[:17]])            # 257 rows
    whole = model.transform(big, n_epochs=20, first_row=3)
    for size in (7, 64, 129):
        parts = [model.transform(big[at:at + size], n_epochs=20, first_row=3 + at) for at in range(0, len(big), size)]
        assert np.array_equal(np.concatenate(parts), whole), f"chunks of {size} rows with first_row equal the transform at once"
    order = np.random.default_rng(0).permutation(len(big))
    for i in (0, 100, 256):                                            # the other rows permuted: row i alone, its number kept
        assert np.array_equal(model.transform(big[order][np.flatnonzero(order == i)], n_epochs=20, first_row=3 + i)[0], whole[i])
    assert not np.array_equal(model.transform(big, n_epochs=20, first_row=4), whole)
    restored = manifold.UMAPModel.from_state(model.state())
    assert np.array_equal(restored.transform(q, n_epochs=N), y), "a model restored from its state transforms to the same bits"


def test_fit_is_umap_kept_and_its_state_restores_it():
    from variantformer_amd import manifold
    g = np.random.default_rng(12)
    x = (4.0 * g.standard_normal((5, 12))[np.arange(500) % 5] + g.standard_normal((500, 12))).astype(np.float32)
    q = (x[:40] * (1 + 0.05 * g.standard_normal((40, 12)))).astype(np.float32)
    kw = dict(n_neighbors=15, n_epochs=50, init="random", seed=3)
    model = manifold.fit(x, **kw)
    assert isinstance(model.embedding, np.ndarray) and np.array_equal(model.embedding, manifold.umap(x, **kw)), "fit(x).embedding equals umap(x)"
    assert (model.rows, model.columns, model.n_components, model.n_neighbors, model.metric, model.n_epochs, model.seed) == (500, 12, 2, 15, "correlation", 50, 3)
    assert 0 < model.mean_dist < 2 and (model.a, model.b) == manifold.find_ab(0.1)
    y = model.transform(q, n_epochs=30)
    assert y.shape == (40, 2) and y.dtype == np.float32 and np.isfinite(y).all()
    near = ((y[:, None, :] - model.embedding[None, :, :]) ** 2).sum(2).argmin(1)
    assert (near % 5 == np.arange(40) % 5).mean() > 0.9, "a slightly perturbed training row lands among its own blob"
    state = model.state()
    assert set(state) == {"embedding", "z", "n_neighbors", "metric", "a", "b", "n_epochs", "seed", "negative_sample_rate", "repulsion_strength",
                          "learning_rate", "mean_dist"} and state["z"].shape == (500, 12) and state["z"].dtype == np.float32
    assert np.array_equal(manifold.UMAPModel.from_state(state).transform(q, n_epochs=30), y), "transform through fit equals transform through its state"
    t = manifold.fit(torch.from_numpy(x).cuda(), **kw)
    assert t.embedding.is_cuda and np.array_equal(t.embedding.cpu().numpy(), model.embedding) and np.array_equal(t.transform(q, n_epochs=30), y)
    few = manifold.fit(x[:10], n_neighbors=15, n_epochs=10, init="random")         # n_neighbors above the training rows: -1 / +Inf, absent
    assert np.isfinite(few.transform(q, n_epochs=10)).all()

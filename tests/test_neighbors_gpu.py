"""vf_rows_standardize, vf_knn_dot and vf_pairwise_dot on the GPU (include/vf_hip_neighbors.h) through ops.rows_standardize,
ops.knn_dot and ops.pairwise_dot: every geometry and data kind of tests/neighbors_cases.py on guarded and poisoned buffers --
the operands sit between poisoned guard rows with 0xFF (NaN, which would rank first) in the columns behind d, the outputs hold
the pattern and keep it outside the write set.  Exact-arithmetic cases are compared bit for bit against the one ranking
reference; random cases through the derived bound tau; then the two entries against each other on the device, the
independence of a row from everything around it, the prefix property, repeatability, and rows that start past 2^31 elements."""
import numpy as np
import pytest
import torch

from tests import neighbors_cases as N
from tests import topk_cases as T
from tests import write_set_cases as W

pytestmark = pytest.mark.gpu

GUARD = 16                      # guard rows either side of the outputs
GEOMETRIES = N.geometries()


def _ops():
    from variantformer_amd import _lib, ops
    _lib.load()
    return ops


def _outputs(rows: int, ldo: int, pattern: int):
    bv = W.poisoned((rows + 2 * GUARD, ldo), torch.float32, W.DEVICE, pattern)
    bi = W.poisoned((rows + 2 * GUARD, ldo), torch.int32, W.DEVICE, pattern)
    return bv, bv[GUARD:GUARD + rows], bi, bi[GUARD:GUARD + rows]


def _check_frame(name: str, big: torch.Tensor, rows: int, width: int, pattern: int, what: str):
    h = big.cpu().numpy().view(np.uint8).reshape(rows + 2 * GUARD, -1, 4)
    assert (h[:GUARD] == pattern).all() and (h[GUARD + rows:] == pattern).all(), f"{what}: {name} guard rows were written"
    assert (h[GUARD:GUARD + rows, width:] == pattern).all(), f"{what}: {name} columns past the write set were written"


def _knn(q, y, k, self_offset, pattern, what):
    """One vf_knn_dot call on poisoned outputs with ldo = k + 3; asserts the write set; (values fp32, indices int32) [Rq, k]."""
    ops = _ops()
    rows = q.shape[0]
    bv, values, bi, indices = _outputs(rows, k + N.EXTRA_LDO, pattern)
    ops.knn_dot(q, y, k, self_offset=self_offset, values=values, indices=indices)
    torch.cuda.synchronize()
    _check_frame("values", bv, rows, k, pattern, what)
    _check_frame("indices", bi, rows, k, pattern, what)
    return values[:, :k].cpu().numpy(), indices[:, :k].cpu().numpy()


def _operands(c, pattern: int):
    """(q, y) on the device, [., d] views of rows d + 5 apart between poisoned guard rows; in "slice" mode q is rows of y itself."""
    y = W.guarded(torch.from_numpy(c.y), pattern)
    q = y[N.SLICE_AT:N.SLICE_AT + c.Rq] if c.mode == "slice" else W.guarded(torch.from_numpy(c.q), pattern)
    assert y.stride(0) == c.d + N.EXTRA_LD and q.stride(0) == c.d + N.EXTRA_LD
    return q[:, :c.d], y[:, :c.d]


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "Rq%d-Ry%d-d%d-k%d-%s" % g)
def test_every_geometry_and_kind_equals_the_reference(geometry):
    for n, kind in enumerate(N.EXACT_KINDS):
        c = N.exact_case(geometry, kind)
        pattern = W.PATTERNS[(n + geometry[0] + geometry[1]) % len(W.PATTERNS)]
        q, y = _operands(c, pattern)
        got_v, got_i = _knn(q, y, c.k, c.self_offset, pattern, c.name)
        want_v, want_i = N.expected(c)
        assert np.array_equal(got_i, want_i), (c.name, pattern, np.argwhere(got_i != want_i)[:4].tolist())
        assert N.same_bits(got_v, want_v), (c.name, pattern)


PAIRWISE = [g for g in GEOMETRIES if g[1] <= 3 * N.BN + 2 and g[3] in (30, 31)]


@pytest.mark.parametrize("geometry", PAIRWISE, ids=lambda g: "Rq%d-Ry%d-d%d-%s" % (g[0], g[1], g[2], g[4]))
def test_pairwise_dot_has_the_bits_of_the_chain_and_one_minus_them(geometry):
    ops = _ops()
    for n, kind in enumerate(("dense", "nonfinite", "ties")):
        c = N.exact_case(geometry, kind)
        want = N.chain(c.q[:, :c.d], c.y[:, :c.d])
        with np.errstate(invalid="ignore"):
            dist = np.float32(1.0) - want
        for r in range(c.Rq):
            if 0 <= c.self_offset and r + c.self_offset < c.Ry:
                dist[r, r + c.self_offset] = 0.0
        for mode, ref in ((0, want), (1, dist)):
            pattern = W.PATTERNS[(n + mode) % len(W.PATTERNS)]
            q, y = _operands(c, pattern)
            big = W.poisoned((c.Rq + 2 * GUARD, c.Ry + N.EXTRA_LDO), torch.float32, W.DEVICE, pattern)
            out = big[GUARD:GUARD + c.Rq, :c.Ry]
            ops.pairwise_dot(q, y, mode=mode, self_offset=c.self_offset, out=out)
            torch.cuda.synchronize()
            _check_frame("out", big, c.Rq, c.Ry, pattern, c.name)
            got = out.cpu().numpy()
            assert N.same_bits(got, ref), (c.name, mode, pattern)
            if mode == 1 and c.self_offset >= 0:
                diag = [T.bits(got[r, r + c.self_offset:r + c.self_offset + 1])[0] for r in range(c.Rq) if r + c.self_offset < c.Ry]
                assert all(b == 0 for b in diag), "the self element of mode 1 is +0.0f"


@pytest.mark.parametrize("Rq", (1, N.BM + 1))
def test_no_candidates_at_all_is_padding_and_reads_nothing(Rq):
    """Ry == 0 with Rq > 0: a launch with no tile.  Every rank of every row is -1 / +0.0f for each k, the pattern stays
    everywhere else, and y -- zero rows inside a poisoned buffer -- keeps its bytes."""
    ops = _ops()
    d = 7
    for n, k in enumerate(N.KS):
        pattern = W.PATTERNS[n % len(W.PATTERNS)]
        q = W.guarded(torch.randn((Rq, d + N.EXTRA_LD), generator=torch.Generator().manual_seed(k)), pattern)[:, :d]
        ybig = W.poisoned((2 * GUARD, d + N.EXTRA_LD), torch.float32, W.DEVICE, pattern)
        y = ybig[GUARD:GUARD, :d]
        assert y.shape == (0, d)
        for self_offset in (-1, 0, 5):
            v, i = _knn(q, y, k, self_offset, pattern, f"Ry=0 Rq={Rq} k={k}")
            assert (i == -1).all() and (T.bits(v) == 0).all(), (Rq, k, self_offset)
        assert (ybig.cpu().numpy().view(np.uint8) == pattern).all(), "y was written"
        out = W.poisoned((Rq, 4), torch.float32, W.DEVICE, pattern)
        ops.pairwise_dot(q, y, mode=1, self_offset=0, out=out[:, :0])   # nothing to write: VF_OK, nothing launched
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint8) == pattern).all()


@pytest.mark.parametrize("shape", N.RANDOM_SHAPES, ids=lambda s: "%dx%d" % s)
def test_random_rows_meet_the_four_checks_and_the_decided_ranks(shape):
    c = N.random_case(*shape)
    z = W.guarded(torch.from_numpy(c.z.copy()), 0xFF)[:, :c.d]
    v, i = _knn(z, z, N.RANDOM_K, 0, 0x3C, c.name)
    frac = N.check_random(c, v, i)
    print(f"[neighbors] {c.name}: all four checks on every row; {100 * frac:.2f} % of ranks decided and equal")
    assert frac >= 0.99
    v2, i2 = _knn(z, z, N.RANDOM_K, 0, 0x00, c.name)                  # a second launch, other poison: the same bits
    assert np.array_equal(i, i2) and np.array_equal(T.bits(v), T.bits(v2))
    vn, inn = _knn(z, z, N.RANDOM_K, -1, 0xFF, c.name)                # self not excluded: it comes first, at similarity ~1
    assert (inn[:, 0] == np.arange(c.rows)).all()
    N.check_random(c, vn, inn, self_excluded=False)
    assert np.array_equal(inn[:, 1:], i[:, :-1]) and np.array_equal(T.bits(vn[:, 1:]), T.bits(v[:, :-1]))


@pytest.mark.parametrize("Rq,Ry,d,k", [(N.BM + 1, 1000, 49, 30), (7, T.MAX_N, 33, 64), (N.BM - 1, 2 * N.BN + 1, 200, 31)])
def test_knn_dot_equals_topk_rows_of_pairwise_dot_on_the_device(Rq, Ry, d, k):
    """Random (inexact) data: both entries run the same chain, so the ranking of the matrix is the fused ranking, bit for bit."""
    ops = _ops()
    g = torch.Generator().manual_seed(Ry + d)
    y = W.guarded(torch.randn((Ry, d + N.EXTRA_LD), generator=g), 0xFF)[:, :d]
    q = W.guarded(torch.randn((Rq, d + N.EXTRA_LD), generator=g), 0xFF)[:, :d]
    v, i = _knn(q, y, k, -1, 0x3C, f"cross {Rq} {Ry} {d}")
    sim = W.poisoned((Rq, Ry), torch.float32, W.DEVICE, 0xFF)
    ops.pairwise_dot(q, y, out=sim)
    tv = W.poisoned((Rq, k), torch.float32, W.DEVICE, 0xFF)
    ti = W.poisoned((Rq, k), torch.int32, W.DEVICE, 0xFF)
    ops.topk_rows(sim, k, values=tv, indices=ti)
    torch.cuda.synchronize()
    assert np.array_equal(i, ti.cpu().numpy()) and np.array_equal(T.bits(v), T.bits(tv.cpu().numpy()))
    ref = q.double().cpu().numpy() @ y.double().cpu().numpy().T
    assert (np.abs(sim.cpu().numpy() - ref) <= N.tau(q.cpu().numpy(), y.cpu().numpy())).all()


def test_a_row_does_not_depend_on_what_is_around_it():
    """Its result under another Rq, ldq, ldo and place in the block, between NaN query rows; and the prefix property."""
    ops = _ops()
    c = N.random_case(333, 33)
    d = c.d
    y = W.guarded(torch.from_numpy(c.z.copy()), 0x3C)[:, :d]
    full = {k: _knn(y, y, k, 0, 0x00, c.name) for k in (1, 31, 64)}
    for k in (1, 31):
        assert np.array_equal(full[64][1][:, :k], full[k][1]) and np.array_equal(T.bits(full[64][0][:, :k]), T.bits(full[k][0])), k
    want_v, want_i = full[31]
    for r, before, after, ldq, ldo in ((0, 0, 0, d, 31), (63, 5, 0, d + 1, 32), (64, 64, 3, d + 64, 40), (65, 1, 130, d + 7, 31),
                                        (200, 63, 1, d + 2, 97), (332, 127, 0, d + 3, 33)):
        rows = before + 1 + after
        host = np.full((rows, ldq), np.nan, dtype=np.float32)
        host[before, :d] = c.z[r, :d]
        q = torch.from_numpy(host).cuda()[:, :d]
        values = torch.full((rows, ldo), 7.0, dtype=torch.float32, device="cuda")
        indices = torch.full((rows, ldo), 7, dtype=torch.int32, device="cuda")
        assert r - before >= 0
        ops.knn_dot(q, y, 31, self_offset=r - before, values=values, indices=indices)
        assert np.array_equal(indices[before, :31].cpu().numpy(), want_i[r]), (r, before, after)
        assert np.array_equal(T.bits(values[before, :31].cpu().numpy()), T.bits(want_v[r])), (r, before, after)
        if after:                                                    # a NaN query: every similarity NaN, ranked in row order
            other = indices[before + 1, :31].cpu().numpy()
            self_row = before + 1 + r - before
            assert other.tolist() == [j for j in range(33) if j != self_row][:31] and torch.isnan(values[before + 1, :31]).all()


def test_rows_that_start_past_2_31_elements():
    """Three rows 2^30 + 8 elements apart, q and y alike: the last row of each starts past 2^31 elements and 8 GiB."""
    ops = _ops()
    d, ld, k = N.BK + 1, 2 ** 30 + 8, 3
    try:
        buf = torch.empty(2 * ld + d, dtype=torch.float32, device="cuda")
    except RuntimeError as e:                                        # torch.OutOfMemoryError is one
        pytest.skip(f"no room for {(2 * ld + d) * 4 / 2 ** 30:.1f} GiB on this device: {str(e).splitlines()[0]}")
    x = buf.as_strided((3, d), (ld, 1))
    host = np.random.default_rng(31).integers(-8, 9, (3, d)).astype(np.float32)
    x.copy_(torch.from_numpy(host).cuda())
    assert x[2].data_ptr() - buf.data_ptr() > 2 ** 33
    v, i = _knn(x, x, k, 0, 0xFF, "past 2^31")
    want_v, want_i = N.rank(N.chain(host, host), k, 0)
    assert np.array_equal(i, want_i) and N.same_bits(v, want_v) and (i[:, 2] == -1).all()
    out = W.poisoned((3, 3), torch.float32, W.DEVICE, 0xFF)
    ops.pairwise_dot(x, x, out=out)
    assert np.array_equal(out.cpu().numpy(), N.chain(host, host))
    z = x
    norm = W.poisoned((3,), torch.float32, W.DEVICE, 0xFF)
    ops.rows_standardize(x, z=z, norm=norm)                           # in place: the rows past 2^31 are read and written where they are
    torch.cuda.synchronize()
    ref_z, ref_n = N.std_reference(host, True)
    tol_z, tol_n = N.std_bound(host, True)
    assert (np.abs(z.cpu().numpy() - ref_z) <= tol_z).all() and (np.abs(norm.cpu().numpy() - ref_n) <= tol_n).all()
    del x, z, buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("center", (True, False), ids=("correlation", "cosine"))
@pytest.mark.parametrize("d", N.STD_DS)
def test_rows_standardize_meets_the_two_pass_bound_on_every_kind(d, center):
    ops = _ops()
    host = N.std_case(d)
    R = host.shape[0]
    ref_z, ref_n = N.std_reference(host[:, :d], center)
    tol_z, tol_n = N.std_bound(host[:, :d], center)
    got = {}
    for pattern in W.PATTERNS:
        x = W.guarded(torch.from_numpy(host), pattern)[:, :d]
        bz = W.poisoned((R + 2 * GUARD, d + N.EXTRA_LDO), torch.float32, W.DEVICE, pattern)
        bn = W.poisoned((R + 2 * GUARD,), torch.float32, W.DEVICE, pattern)
        z, norm = bz[GUARD:GUARD + R, :d], bn[GUARD:GUARD + R]
        ops.rows_standardize(x, center=center, z=z, norm=norm)
        torch.cuda.synchronize()
        _check_frame("z", bz, R, d, pattern, f"standardize d={d}")
        hn = bn.cpu().numpy().view(np.uint8).reshape(-1, 4)
        assert (hn[:GUARD] == pattern).all() and (hn[GUARD + R:] == pattern).all(), "norm guard elements were written"
        assert np.array_equal(x.cpu().numpy().view(np.int32), host[:, :d].view(np.int32)), "x is only read"
        got[pattern] = (z.cpu().numpy(), norm.cpu().numpy())
    gz, gn = got[0x00]
    for p in W.PATTERNS:
        assert N.same_bits(got[p][0], gz) and N.same_bits(got[p][1], gn), "the result depends on the poison"
    finite = np.isfinite(host[:, :d]).all(axis=1)
    assert np.isnan(gz[~finite]).all() and np.isnan(gn[~finite]).all(), "a NaN or Inf makes the whole row and its norm NaN"
    err = np.abs(gz[finite].astype(np.float64) - ref_z[finite])
    assert (err <= tol_z[finite]).all(), f"d={d}: z is {(err / np.maximum(tol_z[finite], 1e-300)).max():.2f} of its bound off"
    assert (np.abs(gn[finite].astype(np.float64) - ref_n[finite]) <= tol_n[finite]).all()
    flat = ref_n == 0
    assert flat[N.STD_KINDS.index("constant_inexact")] == center, "centred, the constant whose fp32 mean is off is flat all the same"
    assert flat[N.STD_KINDS.index("zero")] and (T.bits(gz[flat]) == 0).all() and (T.bits(gn[flat]) == 0).all(), "norm 0: +0.0f throughout"
    # a row's result depends on its d values alone: the same rows in another call, other strides, other neighbours
    wide = np.full((2 * R + 3, d + 11), np.nan, dtype=np.float32)
    wide[3:3 + 2 * R:2, :d] = host[:, :d]
    xw = torch.from_numpy(wide).cuda()
    zw = torch.full((2 * R + 3, d + 1), 7.0, device="cuda")
    ops.rows_standardize(xw[:, :d], center=center, z=zw[:, :d])
    assert N.same_bits(zw[3:3 + 2 * R:2, :d].cpu().numpy(), gz) and (zw[:, d] == 7).all()

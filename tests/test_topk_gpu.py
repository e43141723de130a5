"""vf_topk_rows on the GPU (include/vf_hip_topk.h) through ops.topk_rows: every geometry and data kind of tests/topk_cases.py
against the numpy reference, bit for bit, on guarded and poisoned buffers -- x sits between poisoned guard rows with 0xFF
(NaN, which would rank first) in every column at or past len(r), the outputs hold the pattern and keep it outside the write
set -- then the independence of a row from everything around it, the prefix property, and a row that starts past 2^31
elements.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

from tests import topk_cases as T
from tests import write_set_cases as W

pytestmark = pytest.mark.gpu

GUARD = 16                      # guard rows either side of the outputs


def _ops():
    from variantformer_amd import _lib, ops
    _lib.load()
    return ops


def _outputs(rows: int, ldo: int, pattern: int):
    """(big, view) for values and indices: [rows, ldo] between GUARD poisoned rows, every byte the pattern."""
    bv = W.poisoned((rows + 2 * GUARD, ldo), torch.float32, W.DEVICE, pattern)
    bi = W.poisoned((rows + 2 * GUARD, ldo), torch.int32, W.DEVICE, pattern)
    return bv, bv[GUARD:GUARD + rows], bi, bi[GUARD:GUARD + rows]


def _run(c: T.Case, pattern: int):
    """One call on guarded buffers; asserts the write set and returns (values bits, indices) [R, k] on the host."""
    ops = _ops()
    x = W.guarded(torch.from_numpy(c.x), pattern)                     # [R, n + 5] between poisoned guard rows: ldx = n + 5
    ldo = c.k + T.EXTRA_LDO
    bv, values, bi, indices = _outputs(T.R, ldo, pattern)
    row_len = None if c.row_len is None else W.guarded(torch.from_numpy(c.row_len), pattern)
    assert x.stride(0) == c.n + T.EXTRA_LDX and values.stride(0) == ldo
    ops.topk_rows(x[:, :c.n], c.k, row_len=row_len, values=values, indices=indices)
    torch.cuda.synchronize()
    hv, hi = bv.cpu().numpy().view(np.uint8), bi.cpu().numpy().view(np.uint8)
    for name, h in (("values", hv), ("indices", hi)):
        h = h.reshape(T.R + 2 * GUARD, ldo, 4)
        assert (h[:GUARD] == pattern).all() and (h[GUARD + T.R:] == pattern).all(), f"{c.name}: {name} guard rows were written"
        assert (h[GUARD:GUARD + T.R, c.k:] == pattern).all(), f"{c.name}: {name} columns at or past k were written"
    return values[:, :c.k].cpu().numpy().view(np.int32), indices[:, :c.k].cpu().numpy()


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("n", T.NS)
def test_every_geometry_and_kind_equals_the_reference(n, kind):
    count = 0
    for k in T.KS:
        for form in T.FORMS:
            c = T.case(n, k, form, kind)
            pattern = W.PATTERNS[count % len(W.PATTERNS)]
            count += 1
            got_v, got_i = _run(c, pattern)
            want_v, want_i = T.expected(c)
            assert np.array_equal(got_i, want_i), (c.name, pattern, got_i.tolist(), want_i.tolist())
            assert np.array_equal(got_v, T.bits(want_v)), (c.name, pattern)


def _alone(ops, row: np.ndarray, length: int, k: int, ldx: int, ldo: int, rows_before: int, rows_after: int, use_len: bool):
    """One row ranked inside another call: at position rows_before of R = rows_before + 1 + rows_after, other strides; the
    neighbours are NaN rows of full length."""
    R = rows_before + 1 + rows_after
    n = len(row)
    host = np.full((R, ldx), np.nan, dtype=np.float32)
    host[rows_before, :n] = row
    x = torch.from_numpy(host).cuda()
    lens = np.full(R, n, dtype=np.int32)
    lens[rows_before] = length
    values = torch.full((R, ldo), 7.0, dtype=torch.float32, device="cuda")
    indices = torch.full((R, ldo), 7, dtype=torch.int32, device="cuda")
    ops.topk_rows(x[:, :n], k, row_len=torch.from_numpy(lens).cuda() if use_len else None, values=values, indices=indices)
    return values[rows_before, :k].cpu().numpy().view(np.int32), indices[rows_before, :k].cpu().numpy()


@pytest.mark.parametrize("kind", ("nonfinite", "ties3", "softmax"))
def test_a_row_does_not_depend_on_what_is_around_it(kind):
    ops = _ops()
    n, k = 1025, 31
    c = T.case(n, k, "ragged", kind)
    got_v, got_i = _run(c, 0x3C)
    for r, length in enumerate(T.clamped(n, c.row_len)):
        length = int(length)
        row = c.x[r, :n].copy()
        for ldx, ldo, before, after in ((n, k, 0, 0), (n + 64, k + 1, 3, 0), (n + 1, k + 9, 0, 70)):
            v, i = _alone(ops, row, length, k, ldx, ldo, before, after, True)
            assert np.array_equal(i, got_i[r]) and np.array_equal(v, got_v[r]), (kind, r, ldx, ldo, before, after)
        if length:                                                   # the same columns as a whole row of a narrower call
            v, i = _alone(ops, row[:length].copy(), length, k, length + 2, k, 1, 1, False)
            assert np.array_equal(i, got_i[r]) and np.array_equal(v, got_v[r]), (kind, r, "as n")


@pytest.mark.parametrize("kind", T.KINDS)
def test_the_result_for_k_is_a_prefix_of_the_result_for_a_larger_k(kind):
    for n in (65, 4097):
        for form in T.FORMS:
            small, large = T.case(n, 31, form, kind), T.case(n, 64, form, kind)
            large = large._replace(x=small.x, row_len=small.row_len)                  # the same rows under both k
            v31, i31 = _run(small, 0x00)
            v64, i64 = _run(large, 0xFF)
            assert np.array_equal(i64[:, :31], i31) and np.array_equal(v64[:, :31], v31), (kind, n, form)
            v1, i1 = _run(large._replace(k=1), 0x3C)
            assert np.array_equal(i64[:, :1], i1) and np.array_equal(v64[:, :1], v1), (kind, n, form)


def test_a_row_that_starts_past_2_31_elements():
    """Three rows 2^30 + 8 elements apart: the last one starts past 2^31 elements and 8 GiB.  Only the rows are written."""
    ops = _ops()
    n, k, ldx = 200, 31, 2 ** 30 + 8
    try:
        buf = torch.empty(2 * ldx + n, dtype=torch.float32, device="cuda")
    except RuntimeError as e:                                        # torch.OutOfMemoryError is one
        pytest.skip(f"no room for {(2 * ldx + n) * 4 / 2 ** 30:.1f} GiB on this device: {str(e).splitlines()[0]}")
    x = buf.as_strided((3, n), (ldx, 1))
    g = np.random.default_rng(31)
    host = np.stack([T.make_row(kind, n, g) for kind in ("nonfinite", "distinct", "softmax")])
    x.copy_(torch.from_numpy(host).cuda())
    assert x[2].data_ptr() - buf.data_ptr() > 2 ** 33
    row_len = np.array([n, 17, n - 1], dtype=np.int32)
    values = W.poisoned((3, k), torch.float32, W.DEVICE, 0xFF)
    indices = W.poisoned((3, k), torch.int32, W.DEVICE, 0xFF)
    ops.topk_rows(x, k, row_len=torch.from_numpy(row_len).cuda(), values=values, indices=indices)
    torch.cuda.synchronize()
    want_v, want_i = T.reference(host, k, row_len)
    assert np.array_equal(indices.cpu().numpy(), want_i)
    assert np.array_equal(values.cpu().numpy().view(np.int32), T.bits(want_v))
    del x, buf
    torch.cuda.empty_cache()

"""vf_linkage_nearest and vf_linkage_contract on the GPU (include/vf_hip_linkage.h) through ops.linkage_nearest and
ops.linkage_contract, and linkage.ward on top of them, against the fp32 numpy reference of tests/linkage_cases.py bit for bit:
every fp32 operation of the device code is individually rounded IEEE, as numpy's are.  The operands sit in guarded buffers with
the pattern behind their columns, the outputs are poisoned and guarded: nothing outside the write set changes and nothing inside
it keeps the pattern.  Then rows that start past 2^31 elements, the whole case table end to end, ward_of_rows against scipy on
numpy's own fp64 1 - corrcoef, and VCFProcessor.expression_dendrogram on a synthetic frame."""
import numpy as np
import pandas as pd
import pytest
import torch

from tests import linkage_cases as L
from tests import write_set_cases as W

pytestmark = pytest.mark.gpu

GUARD = 64                      # guard elements / rows either side of an output
EXTRA_LD = 5                    # columns behind the matrix, in operands and outputs alike


def _ops():
    from variantformer_amd import _lib, ops
    _lib.load()
    return ops


def _vector(n: int, dtype, pattern: int):
    big = W.poisoned((n + 2 * GUARD,), dtype, W.DEVICE, pattern)
    return big, big[GUARD:GUARD + n]


def _check_vector(name: str, big: torch.Tensor, n: int, pattern: int):
    h = big.cpu().numpy().view(np.uint8)
    assert (h[:4 * GUARD] == pattern).all() and (h[4 * (GUARD + n):] == pattern).all(), f"{name}: guard elements were written"


def _matrix_out(m: int, pattern: int):
    big = W.poisoned((m + 2 * GUARD, m + EXTRA_LD), torch.float32, W.DEVICE, pattern)
    return big, big[GUARD:GUARD + m, :m]


def _check_matrix(name: str, big: torch.Tensor, m: int, pattern: int):
    h = big.cpu().numpy().view(np.uint8).reshape(m + 2 * GUARD, -1, 4)
    assert (h[:GUARD] == pattern).all() and (h[GUARD + m:] == pattern).all(), f"{name}: guard rows were written"
    assert (h[GUARD:GUARD + m, m:] == pattern).all(), f"{name}: columns past the write set were written"


def _operand(D: np.ndarray, pattern: int) -> torch.Tensor:
    """The square matrix as a [m, m] view of rows m + EXTRA_LD apart, the pattern behind the columns and in guard rows around."""
    m = D.shape[0]
    wide = np.full((m, m + EXTRA_LD), 0, dtype=np.float32)
    wide.view(np.uint8)[:] = pattern
    wide[:, :m] = D
    return W.guarded(torch.from_numpy(wide), pattern, rows=GUARD)[:, :m]


@pytest.mark.parametrize("m", (1, 2, 3, 63, 64, 65, 257))
def test_nearest_equals_the_reference_row_minimum(m):
    ops = _ops()
    host = L.nearest_case(m)
    want_v, want_i = L.nearest(host)
    for pattern in W.PATTERNS:
        D = _operand(host, pattern)
        assert D.stride(0) == m + EXTRA_LD > m
        bv, nn_val = _vector(m, torch.float32, pattern)
        bi, nn_idx = _vector(m, torch.int32, pattern)
        ops.linkage_nearest(D, nn_val=nn_val, nn_idx=nn_idx)
        torch.cuda.synchronize()
        _check_vector("nn_val", bv, m, pattern)
        _check_vector("nn_idx", bi, m, pattern)
        got_v, got_i = nn_val.cpu().numpy(), nn_idx.cpu().numpy()
        assert np.array_equal(got_i, want_i), (m, pattern, np.flatnonzero(got_i != want_i)[:4].tolist())
        assert L.same_bits(got_v, want_v), (m, pattern)
        assert L.same_bits(D.cpu().numpy(), host), "D is only read"
    if m == 1:
        assert want_i.tolist() == [-1] and np.isposinf(want_v[0])


def _contract(D_host, size, first, second, upper_only, pattern):
    """One vf_linkage_contract call on guarded operands and poisoned, guarded outputs; asserts the write set and that the inputs
    keep their bytes; (D_out, size_out, pair_dist) on the host."""
    ops = _ops()
    m, m_out = D_host.shape[0], first.shape[0]
    D = _operand(D_host, pattern)
    size_d = W.guarded(torch.from_numpy(size), pattern, rows=GUARD)
    first_d = W.guarded(torch.from_numpy(first), pattern, rows=GUARD)
    second_d = W.guarded(torch.from_numpy(second), pattern, rows=GUARD)
    bo, out = _matrix_out(m_out, pattern)
    bs, size_out = _vector(m_out, torch.int32, pattern)
    bp, pair_dist = _vector(m_out, torch.float32, pattern)
    ops.linkage_contract(D, size_d, first_d, second_d, upper_only=upper_only, out=out, size_out=size_out, pair_dist=pair_dist)
    torch.cuda.synchronize()
    _check_matrix("D_out", bo, m_out, pattern)
    _check_vector("size_out", bs, m_out, pattern)
    _check_vector("pair_dist", bp, m_out, pattern)
    assert L.same_bits(D.cpu().numpy(), D_host), "D is only read"
    assert np.array_equal(size_d.cpu().numpy(), size) and np.array_equal(first_d.cpu().numpy(), first) and np.array_equal(second_d.cpu().numpy(), second)
    return out.cpu().numpy(), size_out.cpu().numpy(), pair_dist.cpu().numpy()


@pytest.mark.parametrize("kind", ("none", "single", "all", "mixed"))
def test_contract_equals_one_reference_round(kind):
    D, size, first, second = L.contract_case(kind)
    m = D.shape[0]
    want = L.contract_round(D, size, first, second, False)
    if kind == "all":
        assert m % 2 == 0 and first.shape[0] == m // 2 and (second >= 0).all()
    if kind == "none":
        assert (second < 0).all() and L.same_bits(want[0], D)
    for pattern in W.PATTERNS:
        for upper_only in ((True,) if kind == "none" else (False, True)):
            host = D.copy()
            if upper_only:                                            # the lower triangle and the diagonal hold the pattern: never read
                low = np.tril_indices(m)
                host.view(np.uint32)[low] = pattern * 0x01010101
            got = _contract(host, size, first, second, upper_only, pattern)
            assert L.same_bits(got[0], want[0]), (kind, pattern, upper_only, np.argwhere(got[0].view(np.uint32) != want[0].view(np.uint32))[:4].tolist())
            assert np.array_equal(got[1], want[1]) and L.same_bits(got[2], want[2]), (kind, pattern, upper_only)
            assert L.same_bits(got[0], got[0].T) and (got[0].diagonal().view(np.uint32) == 0).all(), "symmetric bit for bit, diagonal +0"


def test_rows_that_start_past_2_31_elements():
    """m = 3 with rows 2^30 + 8 elements apart: the third row starts past 2^31 elements and 8 GiB, in D and in D_out.  Only the
    used elements are written before the calls."""
    ops = _ops()
    m, ld = 3, 2 ** 30 + 8
    assert (m - 1) * ld > 2 ** 31
    host = L.upper(np.array([[0, 3, 1], [0, 0, 2.5], [0, 0, 0]], dtype=np.float32))
    buf = torch.empty(2 * ld + m, dtype=torch.float32, device="cuda")
    D = buf.as_strided((m, m), (ld, 1))
    D.copy_(torch.from_numpy(host).cuda())
    assert D[2].data_ptr() - buf.data_ptr() > 2 ** 33
    bv, nn_val = _vector(m, torch.float32, 0xFF)
    bi, nn_idx = _vector(m, torch.int32, 0xFF)
    ops.linkage_nearest(D, nn_val=nn_val, nn_idx=nn_idx)
    torch.cuda.synchronize()
    want_v, want_i = L.nearest(host)
    assert want_i.tolist() == [2, 2, 0]
    assert np.array_equal(nn_idx.cpu().numpy(), want_i) and L.same_bits(nn_val.cpu().numpy(), want_v)
    size = torch.tensor([2, 1, 3], dtype=torch.int32, device="cuda")
    # the merge of slots 0 and 2 beside slot 1: row 2 of D is read where it is
    first, second = np.array([0, 1], dtype=np.int32), np.array([2, -1], dtype=np.int32)
    want = L.contract_round(host, size.cpu().numpy(), first, second, False)
    bo, out = _matrix_out(2, 0x3C)
    bs, size_out = _vector(2, torch.int32, 0x3C)
    bp, pair_dist = _vector(2, torch.float32, 0x3C)
    ops.linkage_contract(D, size, torch.from_numpy(first).cuda(), torch.from_numpy(second).cuda(), out=out, size_out=size_out, pair_dist=pair_dist)
    torch.cuda.synchronize()
    _check_matrix("D_out", bo, 2, 0x3C)
    assert L.same_bits(out.cpu().numpy(), want[0]) and np.array_equal(size_out.cpu().numpy(), want[1]) and L.same_bits(pair_dist.cpu().numpy(), want[2])
    assert want[1].tolist() == [5, 1] and want[2].tolist() == [1.0, 0.0]
    # no merge, into an output whose third row starts past 2^31 elements as well
    obuf = torch.empty(2 * ld + m, dtype=torch.float32, device="cuda")
    big_out = obuf.as_strided((m, m), (ld, 1))
    ident, alone = torch.arange(3, dtype=torch.int32, device="cuda"), torch.full((3,), -1, dtype=torch.int32, device="cuda")
    for upper_only in (False, True):
        big_out.fill_(7.0)
        _, size_out3 = _vector(3, torch.int32, 0x3C)
        _, pair_dist3 = _vector(3, torch.float32, 0x3C)
        ops.linkage_contract(D, size, ident, alone, upper_only=upper_only, out=big_out, size_out=size_out3, pair_dist=pair_dist3)
        torch.cuda.synchronize()
        assert L.same_bits(big_out.cpu().numpy(), host) and size_out3.cpu().tolist() == [2, 1, 3] and pair_dist3.cpu().tolist() == [0, 0, 0]
    assert L.same_bits(D.cpu().numpy(), host)
    del D, big_out, buf, obuf
    torch.cuda.empty_cache()


CASES = L.cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_ward_equals_the_reference_on_every_case(case):
    from variantformer_amd import linkage
    Z_ref, rounds_ref = L.reference(case)
    whole = torch.from_numpy(case.D).cuda()
    D = whole[:, :case.n]                                              # ld > n where the case has it
    Z, info = linkage.ward(D, return_info=True)
    assert Z.dtype == np.float64 and Z.shape == (case.n - 1, 4)
    assert np.array_equal(Z[:, :2], Z_ref[:, :2]) and np.array_equal(Z[:, 3], Z_ref[:, 3]), case.name
    assert np.array_equal(Z[:, 2], Z_ref[:, 2]), (case.name, np.abs(Z[:, 2] - Z_ref[:, 2]).max())
    assert info == {"rounds": rounds_ref}
    assert np.array_equal(whole.cpu().numpy().view(np.uint32), case.D.view(np.uint32)), "the caller's matrix is never written"
    if case.n in (5, 65):                                             # a numpy matrix in, the same tree out
        assert np.array_equal(linkage.ward(np.ascontiguousarray(case.matrix)), Z)
    if case.name == "garbage-lower-65":
        bad = case.D.copy()
        bad[2, 9] = np.inf
        with pytest.raises(ValueError, match="finite"):
            linkage.ward(torch.from_numpy(bad).cuda())
        Zn, _ = linkage.ward(torch.from_numpy(bad).cuda(), check_finite=False, return_info=True)
        assert Zn.shape == Z.shape and not np.isfinite(Zn[-1, 2]), "unchecked, an Inf distance reaches the root"


def test_ward_of_rows_builds_scipys_tree_of_numpys_own_distances():
    from scipy.cluster.hierarchy import leaves_list, linkage as scipy_linkage
    from scipy.spatial.distance import squareform
    from variantformer_amd import linkage
    x = L.rows_case()
    assert x.shape == (54, 300)
    ref = 1.0 - np.corrcoef(np.nan_to_num(x, nan=0.0).astype(np.float64))
    np.fill_diagonal(ref, 0.0)
    Zs = scipy_linkage(squareform(ref, checks=False), method="ward")
    Z, info = linkage.ward_of_rows(x, return_info=True)
    assert np.array_equal(Z[:, :2], Zs[:, :2]) and np.array_equal(Z[:, 3], Zs[:, 3])
    assert np.array_equal(linkage.leaves_list(Z), leaves_list(Zs))
    rel = (np.abs(Z[:, 2] - Zs[:, 2]) / Zs[:, 2]).max()
    print(f"[linkage] ward_of_rows 54 x 300: {info['rounds']} rounds, heights within {rel:.3e} of scipy on fp64 1 - corrcoef; "
          f"recorded {L.ROWS_HEIGHT_MEASURED:.1e}, asserted {L.ROWS_HEIGHT_RTOL:.1e}")
    assert L.ROWS_HEIGHT_RTOL == 8 * L.ROWS_HEIGHT_MEASURED and rel <= L.ROWS_HEIGHT_RTOL
    Zt = linkage.ward_of_rows(torch.from_numpy(x).cuda())             # a tensor on the device in: the same tree
    assert np.array_equal(Zt, Z)


def test_expression_dendrogram_of_tissues_and_of_genes():
    from scipy.cluster.hierarchy import is_valid_linkage
    from variantformer_amd import linkage, neighbors
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    genes, tissues = 40, 54
    g = np.random.default_rng(20261020)
    names = [f"tissue{t:02d}" for t in range(tissues)]
    programme = g.standard_normal((6, tissues))
    expr = (g.standard_normal((genes, 6)) @ programme + 0.5 * g.standard_normal((genes, tissues)) + 5.0).astype(np.float32)
    df = pd.DataFrame({"gene_id": [f"ENSG{i:05d}" for i in range(genes)], "tissues": [list(range(tissues))] * genes,
                       "tissue_names": [names] * genes, "predicted_expression": [e.reshape(tissues, 1) for e in expr]})
    vp = VCFProcessor()
    for axis, labels in (("tissues", names), ("genes", list(df["gene_id"]))):
        out = vp.expression_dendrogram(df, axis=axis)
        assert set(out) == {"Z", "leaves", "labels", "ordered_labels"} and out["labels"] == labels
        n = len(labels)
        assert out["Z"].shape == (n - 1, 4) and is_valid_linkage(out["Z"])
        assert sorted(out["leaves"].tolist()) == list(range(n))
        assert out["ordered_labels"] == [labels[i] for i in out["leaves"]]
        m, _ = neighbors.from_predictions(df, axis=axis)
        assert np.array_equal(out["Z"], linkage.ward_of_rows(m)) and np.array_equal(out["leaves"], linkage.leaves_list(out["Z"]))
    assert vp.expression_dendrogram(df)["labels"] == names, "the tissue dendrogram is the default"

"""The Ward linkage without a GPU: the boundary of include/vf_hip_linkage.h (it parses, its two names are exported and bound
through _lib.ENTRIES), every refusal with its argument named, the fp32 numpy
reference of tests/linkage_cases.py against scipy -- equal trees on the no-tie cases, heights within the recorded bound, valid
linkages on the tie cases -- leaves_list against scipy's, and the argument checks of linkage.ward and
VCFProcessor.expression_dendrogram."""
import inspect
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests import linkage_cases as L
from tests import write_set_cases as W
from tests.conftest import REPO

NAMES = ["vf_linkage_contract", "vf_linkage_nearest"]
ARGS = {"vf_linkage_nearest": 6, "vf_linkage_contract": 13}


def _header(name="vf_hip_linkage.h") -> str:
    with open(os.path.join(REPO, "include", name)) as f:
        return f.read()


# ---- 1. header and binding ---------------------------------------------------------------------------------------------------------
def test_header_parses_and_its_names_are_exported_and_bound():
    from variantformer_amd import _lib
    from variantformer_amd.csrc import build as B
    text = _header()
    assert W.stream_entries(text) == NAMES
    assert sorted(_lib.ENTRIES["vf_hip_linkage.h"]) == NAMES, "ctypes binding and vf_hip_linkage.h disagree"
    assert "vf_linkage.hip" in B.SOURCES and any(h.endswith("vf_hip_linkage.h") for h in B.HEADERS)
    assert "vf_linkage.hip" not in B.EXTRA_FLAGS                      # the order of nearest is defined for NaN: no -fno-honor-nans
    with open(os.path.join(REPO, "variantformer_amd", "csrc", "vf_linkage.hip")) as f:
        assert "#pragma clang fp contract(off)" in f.read(), "every fp32 operation is rounded on its own"
    bound = _lib.load()
    assert {name: len(_lib.SIGNATURES[name]) for name in NAMES} == ARGS
    assert _lib.ABI_VERSION == 13 and bound.vf_version() == 13
    assert "eight headers" in text
    for word in ("Arguments", "Write set", "Arithmetic", "Non-finite operands", "Refused before anything is launched"):
        assert text.count(word) >= 2, f"an entry's comment contract has no `{word}` part"
    assert "Not checked" in text and int(re.search(r"#define\s+VF_LINKAGE_MAX_M\s+\(1 << (\d+)\)", text).group(1)) == 24


def _err(lib):
    return lib.vf_last_error().decode()


P = 4096                                                 # a non-null, aligned address; never dereferenced
INVALID = 1


def test_nearest_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(D=P, ld=60, m=0, nn_val=P, nn_idx=P):
        return lib.vf_linkage_nearest(D, ld, m, nn_val, nn_idx, 0)
    assert call() == 0 and call(ld=0) == 0                            # m = 0: nothing launched
    for name in ("D", "nn_val", "nn_idx"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        assert call(**{name: P + 2}) == INVALID and re.search(rf"\b{name} must be 4-byte aligned", _err(lib)), _err(lib)
    assert call(m=-1) == INVALID and "m=" in _err(lib)
    assert call(m=2 ** 24 + 1, ld=2 ** 25) == INVALID and "m=" in _err(lib) and "2^24" in _err(lib)
    assert call(m=61) == INVALID and "ld=" in _err(lib)
    assert call(m=2 ** 40, ld=2 ** 41) == INVALID and "m=" in _err(lib)


def test_contract_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(D=P, ld=60, m=54, size=P, first=P, second=P, m_out=0, D_out=P, ld_out=60, size_out=P, pair_dist=P, upper_only=0):
        return lib.vf_linkage_contract(D, ld, m, size, first, second, m_out, D_out, ld_out, size_out, pair_dist, upper_only, 0)
    assert call() == 0 and call(upper_only=1) == 0 and call(m=0, ld=0, ld_out=0) == 0      # m_out = 0: nothing launched
    for name in ("D", "size", "first", "second", "D_out", "size_out", "pair_dist"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        assert call(**{name: P + 2}) == INVALID and re.search(rf"\b{name} must be 4-byte aligned", _err(lib)), _err(lib)
    assert call(m=-1) == INVALID and "m=" in _err(lib)
    assert call(m=2 ** 24 + 1, ld=2 ** 25) == INVALID and "m=" in _err(lib) and "2^24" in _err(lib)
    assert call(ld=53) == INVALID and _err(lib).split(": ")[1].startswith("ld=")
    assert call(m_out=-1) == INVALID and "m_out=" in _err(lib)
    assert call(m=0, ld=0, m_out=1) == INVALID and "m_out=" in _err(lib)
    assert call(m=54, m_out=55, ld_out=55) == INVALID and "m_out=" in _err(lib)
    assert call(ld_out=-1) == INVALID and "ld_out=" in _err(lib)
    for u in (-1, 2):
        assert call(upper_only=u) == INVALID and "upper_only=" in _err(lib)


def test_the_wrappers_allocate_nothing_and_refuse_cpu_tensors():
    from variantformer_amd import ops
    for fn, outs in ((ops.linkage_nearest, ("nn_val", "nn_idx")), (ops.linkage_contract, ("out", "size_out", "pair_dist"))):
        src = inspect.getsource(fn)
        assert not re.search(r"\b(empty|empty_like|zeros|zeros_like|ones|full|new_empty|new_zeros|new_full|tensor|arange|clone|contiguous)\s*\(", src)
        assert 'family="linkage"' not in src and "family or _SCOPE" in src
        prm = inspect.signature(fn).parameters
        for o in outs:
            assert prm[o].kind is inspect.Parameter.KEYWORD_ONLY and prm[o].default is inspect.Parameter.empty
        assert fn.__name__ not in W.allocating_wrappers()
    assert W.uncovered_wrappers() == []
    D = torch.zeros(4, 4)
    i = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(Exception, match="GPU"):
        ops.linkage_nearest(D, nn_val=torch.zeros(4), nn_idx=i)
    with pytest.raises(Exception, match="GPU"):
        ops.linkage_contract(D, i, i, i, out=torch.zeros(4, 4), size_out=i.clone(), pair_dist=torch.zeros(4))
    from variantformer_amd import linkage
    assert inspect.getsource(linkage).count('family="linkage"') == 3, "every launch of the driver is recorded under the family"


# ---- 2. the reference against scipy ------------------------------------------------------------------------------------------------
def _scipy_Z(case):
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    return linkage(squareform(L.upper(case.matrix).astype(np.float64), checks=False), method="ward")


def test_the_case_table_is_what_the_contract_asks_for():
    cases = L.cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for n in L.NS:
        assert sum(c.n == n and not c.ties for c in cases if c.name.startswith(("random", "clustered"))) == 2, n
    assert L.NS == (2, 3, 5, 54, 63, 64, 65, 200, 257) and any(c.n == 1000 for c in cases)
    by = {c.name: c for c in cases}
    assert {c.name for c in cases if c.ties} == {"chain-12", "constant-54", "duplicates-60"}
    const = by["constant-54"].matrix
    assert (const[~np.eye(54, dtype=bool)] == 1).all(), "constant rows: every distance equal"
    dup = by["duplicates-60"].matrix
    assert ((dup == 0).sum(axis=1) == 3).all(), "every row has two duplicates at distance exactly 0"
    g = by["garbage-lower-65"]
    assert np.isnan(np.diag(g.D)).all() and (g.D[np.tril_indices(65, -1)] < 0).mean() > 0.9 and not np.allclose(g.D, g.D.T, equal_nan=True)
    w = by["ld-above-n-63"]
    assert w.D.shape == (63, 74) and np.isnan(w.D[:, 63:]).all()
    for c in cases:
        assert c.D.dtype == np.float32 and np.isfinite(c.matrix[np.triu_indices(c.n, 1)]).all() and (L.upper(c.matrix) >= 0).all()
    assert L.reference(by["chain-12"])[1] == 11, "the chain merges one pair per round"
    assert L.reference(cases[0])[0] is L.reference(cases[0])[0], "a reference is computed once"


def test_the_reference_builds_scipys_tree_on_the_no_tie_cases():
    from scipy.cluster.hierarchy import is_valid_linkage, leaves_list
    from variantformer_amd import linkage
    worst = 0.0
    for c in L.cases():
        if c.ties:
            continue
        Z, rounds = L.reference(c)
        Zs = _scipy_Z(c)
        assert is_valid_linkage(Z) and Z.dtype == np.float64 and Z.shape == (c.n - 1, 4)
        assert np.array_equal(Z[:, :2], Zs[:, :2]) and np.array_equal(Z[:, 3], Zs[:, 3]), c.name
        assert (Z[:, 0] < Z[:, 1]).all() and (np.diff(Z[:, 2]) >= 0).all()
        assert np.array_equal(linkage.leaves_list(Z), leaves_list(Zs)), c.name
        rel = (np.abs(Z[:, 2] - Zs[:, 2]) / Zs[:, 2]).max()
        worst = max(worst, rel)
        print(f"[linkage cases] {c.name}: {rounds} rounds, heights within {rel:.2e} of scipy's")
        assert 1 <= rounds <= c.n - 1
    print(f"[linkage cases] largest relative height deviation {worst:.3e}; recorded {L.REF_HEIGHT_MEASURED:.1e}, asserted {L.REF_HEIGHT_RTOL:.1e}")
    assert L.REF_HEIGHT_RTOL == 8 * L.REF_HEIGHT_MEASURED
    assert worst <= L.REF_HEIGHT_RTOL


def test_the_reference_gives_a_valid_linkage_on_the_tie_cases():
    from scipy.cluster.hierarchy import is_valid_linkage
    from variantformer_amd import linkage
    for c in L.cases():
        if not c.ties:
            continue
        Z, rounds = L.reference(c)
        assert is_valid_linkage(Z), c.name
        assert (np.diff(Z[:, 2]) >= 0).all(), "monotone heights"
        assert sorted(linkage.leaves_list(Z).tolist()) == list(range(c.n)), "every leaf exactly once"
        assert Z[-1, 3] == c.n and 1 <= rounds <= c.n - 1


def test_nearest_reference_follows_the_order():
    D = L.nearest_case(65)
    v, i = L.nearest(D)
    assert i[0] == 1 and np.isnan(v[0]), "a row of NaNs finds its lowest j != i"
    assert i[1] == 0 and np.isposinf(v[1])
    assert i[2] == 64 and v[2] == 0 and np.signbit(v[2]), "-0 is returned with its bits"
    assert i[5] == 63 and np.isneginf(v[5])
    assert i[6] == 64 and np.isposinf(v[6]), "+Inf ranks before NaN"
    for r in range(7, 65):
        row = np.delete(D[r], r)
        if not np.isnan(row).all():
            assert v[r] == np.nanmin(row) and i[r] == min(j for j in range(65) if j != r and D[r, j] == v[r])
    zero = np.zeros((3, 3), dtype=np.float32)
    zero[0, 1] = -0.0
    assert L.nearest(zero)[1].tolist() == [1, 0, 0], "+0 and -0 tie: the lower j"
    assert L.nearest(np.zeros((1, 1), dtype=np.float32))[1].tolist() == [-1]


def test_contract_reference_is_symmetric_and_is_wards_update():
    for kind in ("none", "single", "all", "mixed"):
        D, size, first, second = L.contract_case(kind)
        out, size_out, pd = L.contract_round(D, size, first, second, False)
        assert L.same_bits(out, out.T) and (np.diag(out) == 0).all(), kind
        assert size_out.sum() == size.sum() and ((pd == 0) == (second < 0)).all()
        # against the update in fp64 from cluster pairs: d(X u Y, I)^2 = ((sx+si) dxi^2 + (sy+si) dyi^2 - si dxy^2) / (sx+sy+si)
        m_out = first.shape[0]
        D64 = D.astype(np.float64)
        groups = [[f] if s < 0 else [f, s] for f, s in zip(first.tolist(), second.tolist())]
        g = np.random.default_rng(m_out)
        for a, b in g.integers(0, m_out, (200, 2)):
            if a == b:
                continue
            lo, hi = groups[min(a, b)], groups[max(a, b)]

            def lw(dxi, dyi, dxy, sx, sy, si):
                with np.errstate(invalid="ignore"):
                    return np.sqrt(((sx + si) * dxi ** 2 + (sy + si) * dyi ** 2 - si * dxy ** 2) / (sx + sy + si))
            if len(lo) == 1 and len(hi) == 1:
                want = D64[lo[0], hi[0]]
            elif len(hi) == 1:
                want = lw(D64[lo[0], hi[0]], D64[lo[1], hi[0]], D64[lo[0], lo[1]], size[lo[0]], size[lo[1]], size[hi[0]])
            elif len(lo) == 1:
                want = lw(D64[lo[0], hi[0]], D64[lo[0], hi[1]], D64[hi[0], hi[1]], size[hi[0]], size[hi[1]], size[lo[0]])
            else:
                u = lw(D64[lo[0], hi[0]], D64[lo[1], hi[0]], D64[lo[0], lo[1]], size[lo[0]], size[lo[1]], size[hi[0]])
                v = lw(D64[lo[0], hi[1]], D64[lo[1], hi[1]], D64[lo[0], lo[1]], size[lo[0]], size[lo[1]], size[hi[1]])
                want = lw(u, v, D64[hi[0], hi[1]], size[hi[0]], size[hi[1]], size[lo[0]] + size[lo[1]])
            if np.isfinite(want):                                     # random "distances" are no metric: a radicand may be negative
                assert abs(out[a, b] - want) <= 1e-5 * max(want, 1.0), (kind, a, b)
    D, size, first, second = L.contract_case("mixed")
    merged = second >= 0
    assert (merged[:, None] & merged[None, :]).sum() > 1000 and (size > 1).any(), "the both-merged branch is reached, with sizes above 1"
    poisoned = D.copy()
    poisoned[np.tril_indices(D.shape[0])] = np.nan
    ident = np.arange(D.shape[0], dtype=np.int32)
    out, _, _ = L.contract_round(poisoned, np.ones_like(size), ident, np.full_like(ident, -1), True)
    assert L.same_bits(out, D), "upper_only: the symmetric copy of the upper triangle"


def test_leaves_list_equals_scipys_on_scipys_own_Z():
    from scipy.cluster.hierarchy import leaves_list
    from variantformer_amd import linkage
    for c in L.cases():
        if c.ties:
            continue
        Zs = _scipy_Z(c)
        got = linkage.leaves_list(Zs)
        assert got.dtype == np.int32 and np.array_equal(got, leaves_list(Zs)), c.name
    for bad in (np.zeros((3, 3)), np.zeros(4), np.array([[0.0, 5.0, 1.0, 2.0]]), np.array([[0.0, 1.0, 1.0, 2.0], [0.0, 3.0, 2.0, 3.0]])):
        with pytest.raises(ValueError, match="linkage"):
            linkage.leaves_list(bad)
    src = inspect.getsource(linkage)
    assert not re.search(r"^\s*(import|from)\s+scipy", src, flags=re.M), "the product does not import scipy"


# ---- 3. argument checks --------------------------------------------------------------------------------------------------------------
def test_ward_checks_its_arguments_before_the_device():
    from variantformer_amd import linkage
    for bad in (np.zeros((4, 5), dtype=np.float32), np.zeros(4, dtype=np.float32), torch.zeros(3, 4)):
        with pytest.raises(ValueError, match="square"):
            linkage.ward(bad)
    for bad in (np.zeros((1, 1), dtype=np.float32), np.zeros((0, 0), dtype=np.float32)):
        with pytest.raises(ValueError, match="at least 2"):
            linkage.ward(bad)
    with pytest.raises(TypeError, match="numpy array or a torch tensor"):
        linkage.ward([[0.0, 1.0], [1.0, 0.0]])
    D = L.cases()[4].matrix.copy()
    for value in (np.nan, np.inf, -np.inf):
        E = D.copy()
        E[1, 3] = value
        with pytest.raises(ValueError, match="finite"):
            linkage.ward(E)
        with pytest.raises(ValueError, match="finite"):
            linkage.ward(torch.from_numpy(E))
    with pytest.raises(ValueError, match="at least 2 rows"):
        linkage.ward_of_rows(np.zeros((1, 7), dtype=np.float32))
    with pytest.raises(ValueError, match="matrix"):
        linkage.ward_of_rows(np.zeros(7, dtype=np.float32))
    prm = inspect.signature(linkage.ward).parameters
    assert [(n, p.default) for n, p in prm.items()] == [("D", inspect.Parameter.empty), ("check_finite", True), ("return_info", False)]
    assert inspect.signature(linkage.ward_of_rows).parameters["nan_to_zero"].default is True
    if not torch.cuda.is_available():
        E = D.copy()
        E[3, 1] = np.nan                                              # the lower triangle is not used: this gets as far as the device
        with pytest.raises(Exception, match="GPU"):
            linkage.ward(E)
        with pytest.raises(Exception, match="GPU"):
            linkage.ward_of_rows(np.random.default_rng(0).standard_normal((5, 7)).astype(np.float32))


def test_expression_dendrogram_checks_the_frame():
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    prm = inspect.signature(VCFProcessor.expression_dendrogram).parameters
    assert [(n, p.default) for n, p in prm.items()][1:] == [("df", inspect.Parameter.empty), ("on", "predicted_expression"),
                                                           ("axis", "tissues"), ("tissue", None)]
    vp = VCFProcessor(require_gpu=False)
    names = [f"tissue{t}" for t in range(4)]
    df = pd.DataFrame({"gene_id": [f"ENSG{i:03d}" for i in range(6)], "tissues": [list(range(4))] * 6, "tissue_names": [names] * 6,
                       "predicted_expression": [np.arange(4, dtype=np.float32).reshape(4, 1) * (i + 1) for i in range(6)]})
    with pytest.raises(ValueError, match="format_output"):
        vp.expression_dendrogram(df.drop(columns=["predicted_expression"]))
    with pytest.raises(ValueError, match="format_output"):
        vp.expression_dendrogram(df.drop(columns=["gene_id"]))
    with pytest.raises(ValueError, match="format_output"):
        vp.expression_dendrogram(df, on="embeddings")
    with pytest.raises(ValueError, match="axis"):
        vp.expression_dendrogram(df, axis="rows")
    with pytest.raises(ValueError, match="at least 2"):
        vp.expression_dendrogram(df.iloc[:1], axis="genes")
    if not torch.cuda.is_available():
        with pytest.raises(Exception, match="GPU"):
            vp.expression_dendrogram(df)

"""The ranked cCREs without a GPU: the vf_topk_rows boundary (include/vf_hip_topk.h parses, its one name is exported and bound
through _lib.ENTRIES), every refusal of the entry with the argument named, the
wrapper that allocates nothing, `top_k` in the three signatures and its validation before a batch is read -- and, on the
reference alone, that the case table of tests/topk_cases.py tells every plausible mistake from the contract."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import topk_cases as T
from tests import write_set_cases as W
from tests.conftest import REPO

NAME = "vf_topk_rows"


def _header(name="vf_hip_topk.h") -> str:
    with open(os.path.join(REPO, "include", name)) as f:
        return f.read()


# ---- 1. header and binding ---------------------------------------------------------------------------------------------------------
def test_header_parses_and_its_name_is_exported_and_bound():
    """What is this header's own; the boundary every header shares is tests/test_abi_cpu.py's."""
    from variantformer_amd import _lib
    from variantformer_amd.csrc import build as B
    text = _header()
    assert W.stream_entries(text) == [NAME]
    assert sorted(_lib.ENTRIES["vf_hip_topk.h"]) == [NAME], "ctypes binding and vf_hip_topk.h disagree"
    assert "vf_topk.hip" in B.SOURCES and any(h.endswith("vf_hip_topk.h") for h in B.HEADERS)
    assert "vf_topk.hip" not in B.EXTRA_FLAGS                         # the NaN order needs NaNs honoured: no -fno-honor-nans
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert len(_lib.SIGNATURES[NAME]) == 10
    assert _lib.ABI_VERSION == 13 and _lib.load().vf_version() == 13
    for word in ("Arguments", "Write set", "Arithmetic", "Non-finite operands", "Refused before anything is launched", "Order"):
        assert word in text, f"the comment contract of {NAME} has no `{word}` part"
    limits = {k: int(v) for k, v in re.findall(r"#define\s+(VF_TOPK_MAX_[NK])\s+(\d+)", src)}
    assert limits == {"VF_TOPK_MAX_N": T.MAX_N, "VF_TOPK_MAX_K": T.MAX_K}
    from variantformer_amd import attn_maps
    assert (attn_maps.TOP_K_MAX, attn_maps.TOP_K_MAX_WIDTH) == (T.MAX_K, T.MAX_N)


def test_argument_validation_without_gpu():
    """Refused before anything is launched (no GPU here: a launch would fail differently), the argument named."""
    from variantformer_amd import _lib
    lib = _lib.load()
    p = 4096                                             # a non-null, aligned address; never dereferenced
    INVALID = 1

    def call(x=p, ldx=200, R=0, n=200, row_len=0, k=32, values=p, indices=p, ldo=32):
        return lib.vf_topk_rows(x, ldx, R, n, row_len, k, values, indices, ldo, 0)

    def err():
        return lib.vf_last_error().decode()
    assert call() == 0 and call(row_len=p) == 0                                         # the base call is valid (R = 0)
    for name in ("x", "values", "indices"):
        assert call(**{name: 0}) == INVALID and err().endswith(f"null pointer {name}"), err()
    for name in ("x", "row_len", "values", "indices"):
        assert call(**{name: p + 2}) == INVALID and re.search(rf"\b{name} must be 4-byte aligned", err()), err()
    for n in (-1, 16385):
        assert call(n=n, ldx=20000) == INVALID and "n=" in err() and "16384" in err()
    assert call(n=0) == 0 and call(n=16384, ldx=16384) == 0                             # n == 0 is VF_OK
    for k in (0, -1, 65):
        assert call(k=k, ldo=128) == INVALID and "k=" in err()
    assert call(k=1) == 0 and call(k=64, ldo=64) == 0
    assert call(ldx=199) == INVALID and "ldx" in err()
    assert call(ldo=31) == INVALID and "ldo" in err()
    assert call(R=-1) == INVALID and "R=" in err()
    assert call(R=2 ** 31) == INVALID and "grid" in err()
    assert call(R=0) == 0                                                               # nothing to do: VF_OK, no launch


def test_the_wrapper_allocates_nothing():
    """As forest_predict (tests/test_forest_cpu.py): the caller owns every buffer, so `values` and `indices` are required and
    keyword-only and no allocating call of any spelling stands in the wrapper."""
    from variantformer_amd import ops
    src = inspect.getsource(ops.topk_rows)
    assert not re.search(r"\b(empty|empty_like|zeros|zeros_like|ones|full|new_empty|new_zeros|new_full|tensor|arange|clone|contiguous)\s*\(", src)
    prm = inspect.signature(ops.topk_rows).parameters
    assert list(prm) == ["x", "k", "row_len", "values", "indices", "family"]
    assert all(prm[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("row_len", "values", "indices", "family"))
    assert prm["values"].default is inspect.Parameter.empty and prm["indices"].default is inspect.Parameter.empty
    assert prm["row_len"].default is None
    assert "topk_rows" not in W.allocating_wrappers() and W.uncovered_wrappers() == []
    with pytest.raises(Exception, match="GPU"):                      # no CPU fallback
        ops.topk_rows(torch.zeros(2, 8), 2, values=torch.zeros(2, 2), indices=torch.zeros(2, 2, dtype=torch.int32))


# ---- 2. top_k in the model and the processor ---------------------------------------------------------------------------------------
def test_top_k_defaults_to_none_and_is_the_last_keyword():
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    from variantformer_amd.seq2gene.model_combined_modulator import Seq2GenePredictorCombinedModulator as M
    for fn in (M.predict_step_with_attention, M.variant_prediction_with_attention, VCFProcessor.predict_with_attention):
        prm = inspect.signature(fn).parameters
        assert list(prm)[-1] == "top_k" and prm["top_k"].default is None, fn.__qualname__


def _small_model(**extra):
    from tests.helpers import SEQ2REG_512, build_model, seq2gene_kw
    small = dict(SEQ2REG_512, embedding_dim=64, num_heads=2, num_layers=1)
    kw = seq2gene_kw(emb_dim=64, heads=2, layers=3, token_dim=64, gene_emb_dim=64)
    return build_model(small, dict(kw, **extra), seed=1)


def test_top_k_is_validated_before_the_batch_is_read():
    model = _small_model()
    for bad in (0, 65, 2.5, -1, True, "8"):
        with pytest.raises(ValueError, match="top_k"):
            model.predict_step_with_attention({}, 0, top_k=bad)      # an empty dict: reading the batch would be a KeyError
    model.vep = True
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError, match="top_k"):
            model.variant_prediction_with_attention({}, top_k=bad)
    from variantformer_amd import attn_maps
    assert attn_maps.select_top_k(None) is None and attn_maps.select_top_k(1) == 1 and attn_maps.select_top_k(np.int64(64)) == 64


def test_unsupported_options_still_raise_by_name_with_top_k():
    model = _small_model()
    with pytest.raises(ValueError, match="out of range"):
        model.predict_step_with_attention({}, 0, layers=[3], top_k=8)
    model.vep = True
    with pytest.raises(NotImplementedError, match="vep"):
        model.predict_step_with_attention({}, 0, top_k=8)
    for extra, word in ((dict(cross_alibi=True), "cross_alibi"), (dict(gene_pooling="max"), "gene_pooling")):
        other = _small_model(**extra)
        with pytest.raises(NotImplementedError, match=word):
            other.predict_step_with_attention({}, 0, top_k=8)
        other.vep = True
        with pytest.raises(NotImplementedError, match=word):
            other.variant_prediction_with_attention({}, top_k=8)


# ---- 3. the reference and the case table -------------------------------------------------------------------------------------------
def test_the_reference_on_a_handwritten_row():
    f = np.float32
    nan_a, nan_b = np.array([0x7FC00001, 0xFFC00002], dtype=np.uint32).view(np.float32)
    row = np.array([[1.0, nan_a, -0.0, np.inf, 0.0, 1.0, nan_b, -np.inf, f(1e-42)]], dtype=np.float32)
    v, i = T.reference(row, 12)
    assert i.tolist() == [[1, 6, 3, 0, 5, 8, 2, 4, 7, -1, -1, -1]]
    want = np.concatenate([row[0, [1, 6, 3, 0, 5, 8, 2, 4, 7]], np.zeros(3, dtype=np.float32)])
    assert np.array_equal(T.bits(v[0]), T.bits(want))                # the NaN payloads, -0 before +0 (its column is lower), +0.0 pads
    v3, i3 = T.reference(row, 3)
    assert np.array_equal(i3, i[:, :3]) and np.array_equal(T.bits(v3), T.bits(v[:, :3]))          # a prefix
    v, i = T.reference(row, 4, row_len=np.array([3]))
    assert i.tolist() == [[1, 0, 2, -1]]
    v, i = T.reference(row, 2, row_len=np.array([-5]))
    assert i.tolist() == [[-1, -1]] and T.bits(v).tolist() == [[0, 0]]
    # torch.topk agrees wherever it is defined: NaN first, then descending (its tie order is not defined: distinct values)
    c = T.case(200, 31, "full", "distinct")
    tv, ti = torch.topk(torch.from_numpy(c.x[:, :c.n].copy()), 31, dim=1)
    v, i = T.expected(c)
    assert np.array_equal(tv.numpy(), v) and np.array_equal(ti.numpy(), i)


def test_the_case_table_is_what_the_contract_asks_for():
    assert T.NS == (0, 1, 2, 63, 64, 65, 200, 1024, 1025, 4097, 16384) and T.KS == (1, 2, 31, 64) and T.R == 7
    c = T.case(1025, 31, "ragged", "nonfinite")
    assert c.x.shape == (7, 1030) and c.row_len.tolist() == [0, 1, 30, 1025, 1026, -3, 513]
    lens = T.clamped(c.n, c.row_len)
    assert lens.tolist() == [0, 1, 30, 1025, 1025, 0, 513]
    for r, length in enumerate(lens):                                # 0xFF bytes in every column at or past len(r)
        assert (c.x[r, length:].view(np.uint8) == 0xFF).all()
    row = c.x[3, :1025]
    assert np.isnan(row).sum() == 3 and len(set(row.view(np.uint32)[np.isnan(row)].tolist())) == 3          # three payloads
    assert np.isposinf(row).sum() == 1 and np.isneginf(row).sum() == 1
    zeros = np.flatnonzero(row == 0)
    assert len(zeros) >= 2 and np.signbit(row[zeros[0]]) and not np.signbit(row[zeros[1]])
    soft = T.case(1024, 31, "full", "softmax").x[:, :1024]
    assert (soft == 0).sum() > 1000 and ((soft > 0) & (soft < np.finfo(np.float32).tiny)).sum() > 500 and np.isfinite(soft).all()
    assert len(np.unique(T.case(1024, 31, "full", "ties3").x[:, :1024])) == 3
    d = T.case(4097, 64, "full", "distinct").x[:, :4097]
    assert all(len(np.unique(r)) == 4097 for r in d)
    assert T.case(64, 2, "full", "ties3").x.tobytes() == T.case(64, 2, "full", "ties3").x.tobytes()         # seeded


@pytest.mark.parametrize("mistake", list(T.MUTATIONS))
def test_the_cases_tell_every_mistake_from_the_contract(mistake):
    """A condition on the inputs, asserted: in the data kind that goes with a mistake, in every geometry wide enough to hold it
    (n >= 63 and k >= 31: a NaN, an Inf and two zeros need six ranks) and in every row_len form in which it can show, the wrong
    implementation's output differs from the contract's in at least a quarter of the rows."""
    kind, forms = T.MUTATIONS[mistake]
    least = T.R
    for n in T.NS:
        for k in T.KS:
            for form in forms:
                if n < 63 or k < 31:
                    continue
                changed = T.rows_changed(T.case(n, k, form, kind), mistake)
                least = min(least, changed)
                assert 4 * changed >= T.R, (mistake, n, k, form, changed)
    print(f"[topk cases] {mistake}: at least {least} of {T.R} rows change in every geometry with n >= 63 and k >= 31")


def test_a_mistake_is_not_the_contract():
    """Every mistake is a different function: none of them equals the reference on the whole table of its kind."""
    for mistake, (kind, forms) in T.MUTATIONS.items():
        assert any(T.rows_changed(T.case(n, k, form, kind), mistake) for n in (63, 200) for k in T.KS for form in forms), mistake
    c = T.case(200, 31, "ragged", "distinct")
    assert T.rows_changed(c, None) == 0

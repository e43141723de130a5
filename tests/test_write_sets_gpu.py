"""Write set and read set of every C-ABI entry on a real MI355X (tests/write_set_cases.py): each case runs three times, its
outputs, workspaces and operand guards filled with 0xFF, 0x00 and 0x3C, and check_write_set holds the documented output set
to bit identity across the three, every other byte to the poison, and the 0x00 run to the case's existing reference.  Then the
whole model under the poisoning allocator, caches included."""
import numpy as np
import pytest
import torch

from tests import write_set_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from variantformer_amd import _lib as lib
    lib.load()      # must be the in-tree HIP library; raises if missing


def _drive(case):
    built = case.make()
    try:
        W.check_write_set(built.run, built.written, built.reference, built.nan_ok)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):       # a faulted device: launch nothing more on it
            pytest.exit(f"GPU fault in {case.name}: {e}", returncode=3)
        raise


def _params(family):
    return pytest.mark.parametrize("case", W.cases_of(family), ids=lambda c: c.name)


@_params("gemm")
def test_gemm_write_sets(case):
    """vf_gemm_bf16 / _f16 and their _ex forms: variants 0, 1, 5, 20, 22 at M = 515, N = 776 (800 for GEGLU), K = 192 -- ragged
    against every tile -- and the generic path at 77 x 40 x 72; every epilogue; a, residual and out row-strided inside poison."""
    _drive(case)


@_params("gemm_ln")
def test_gemm_ln_write_sets(case):
    """vf_gemm_ln as consumer and as producer (no / fp32 / 16-bit residual, with and without the fp32 rows), vf_gemm_ln_t16 (with
    and without t16_out and out), vf_gemm_ln_bf16; part_stats is returned too: vf_ln_finalize2 reads all of it."""
    _drive(case)


@_params("stats")
def test_row_statistics_write_sets(case):
    _drive(case)


@_params("attn")
def test_forward_attention_write_sets(case):
    """One case per kernel family of the edge table (the kernel's name is asserted), both operand types, both ALiBi alignments,
    the four pre-ABI-4 entries, the row-map form, vf_attn_counted_keys and vf_softmax_counted.  Every forward case holds a
    sequence without queries, one without keys and query / output rows past cu_seqlens_q[n_seq], and every family runs once
    more at a padded head dim (dh - 8 through vf_attn_varlen_fwd_v3) against the class-dh call on zero-padded operands."""
    _drive(case)


@_params("attn_probs")
def test_attention_probabilities_write_sets(case):
    """vf_attn_probs and _v2: head mean and per head, out wider than max_seqlen_k, stats poisoned, a sequence without selected
    rows and one without keys; with ALiBi the keys come through a row map over a table with poisoned rows."""
    _drive(case)


@_params("stream")
def test_streaming_kernels_write_sets(case):
    _drive(case)


# ---------------------------------------------------------------------------------------------
# the whole model
# ---------------------------------------------------------------------------------------------
MODEL_KEYS = ("pred_gene_exp", "embeddings", "cre_attention", "gene_attention")


def _model_results(precision, pattern):
    """A fresh model from the fixed seed, warmed and run -- under the poisoning allocator from its first forward on when a
    pattern is given, so the weight-derived caches are built under poison too."""
    from tests.helpers import SEQ2REG_512, build_model, seq2gene_kw
    from variantformer_amd.utils.synthetic import TISSUES_54, make_batch
    batch = make_batch(31, [280, 64], [120, 30], [TISSUES_54[:9], TISSUES_54[3:8]], 200)

    def go():
        model = build_model(SEQ2REG_512, seq2gene_kw(layers=3), seed=21).cuda()
        model.precision = precision
        model.predict_step(batch, 0)                          # (the cache-building first forward)
        plain = model.predict_step(batch, 0)
        maps = model.predict_step_with_attention(batch, 0, gene_body=True)
        torch.cuda.synchronize()
        return plain, maps
    if pattern is None:
        return go()
    with W.poison_allocations(pattern, keep=False) as px:
        out = go()
    assert px.count > 100, "the forward did not allocate through the patched modules"
    return out


@pytest.mark.parametrize("precision", ["bf16-mixed", "16-mixed"])
def test_whole_model_under_poisoned_allocations(precision):
    """predict_step and predict_step_with_attention(gene_body=True) on the default two-stream path: expressions, embeddings and
    both kinds of attention map are finite and bit-identical whether torch.empty hands out whatever the allocator holds, NaN
    bytes or small finite values -- no kernel of the forward leaves part of a buffer the model reads unwritten, and none
    reads a workspace before writing it."""
    base_plain, base_maps = _model_results(precision, None)
    for key in MODEL_KEYS:
        for a in base_maps[key]:
            assert np.isfinite(np.asarray(a)).all(), key
    for pattern in (0xFF, 0x3C):
        plain, maps = _model_results(precision, pattern)
        for key in MODEL_KEYS[:2]:
            assert len(plain[key]) == len(base_plain[key]) == 2
            for g, (a, b) in enumerate(zip(plain[key], base_plain[key])):
                np.testing.assert_array_equal(a, b, err_msg=f"predict_step {key}[{g}] under {pattern:#04x}")
        for key in MODEL_KEYS:
            assert len(maps[key]) == len(base_maps[key]) == 2
            for g, (a, b) in enumerate(zip(maps[key], base_maps[key])):
                np.testing.assert_array_equal(a, b, err_msg=f"predict_step_with_attention {key}[{g}] under {pattern:#04x}")

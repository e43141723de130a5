"""cCRE contribution maps without a GPU: the vf_attn_contrib boundary (include/vf_hip_attn_contrib.h parses, every name in it is
exported and bound through _lib.ENTRIES, every stream-taking declaration has a write-set case in the parallel net, the
wrapper allocates nothing), every refusal of the entry with the argument named, and -- on the references alone -- that the
operands of tests/attn_contrib_cases.py tell the contribution norm from four cheaper quantities by far more than the GPU limit."""
import inspect
import os
import re

import pytest
import torch

from tests import attn_contrib_cases as A
from tests import write_set_cases as W
from tests.conftest import REPO


def _next_header() -> str:
    with open(os.path.join(REPO, "include", "vf_hip_attn_contrib.h")) as f:
        return f.read()


def test_next_header_parses_and_every_name_is_exported_and_bound():
    """What is this header's own; the boundary every header shares is tests/test_abi_cpu.py's."""
    from variantformer_amd import _lib
    assert sorted(_lib.ENTRIES["vf_hip_attn_contrib.h"]) == ["vf_attn_contrib"], "ctypes binding and vf_hip_attn_contrib.h disagree"
    assert _lib.ABI_VERSION == 13 and _lib.load().vf_version() == 13


def test_every_stream_entry_of_the_next_header_has_a_write_set_case():
    entries = W.stream_entries(_next_header())
    assert entries == ["vf_attn_contrib"]
    cases = A.ws_cases()
    assert set(entries) <= {e for c in cases for e in c.entries}
    assert {e for c in cases for e in c.entries} <= set(entries)    # no case names an entry the header does not declare
    assert len({c.name for c in cases}) == len(cases)
    # entry and wrapper, head-summed and per head, every geometry
    for H, dh in A.GEOMETRIES:
        for ph in ("summed", "per_head"):
            for how in ("entry", "wrapper"):
                assert any(c.name.startswith(f"attn_contrib-H{H}-dh{dh}-") and c.name.endswith(f"{ph}-{how}") for c in cases)
    assert all(c.wrappers == (("attn_contrib",) if c.name.endswith("wrapper") else ()) for c in cases)


def test_the_wrapper_allocates_nothing():
    from variantformer_amd import ops
    src = inspect.getsource(ops.attn_contrib)
    assert not re.search(r"\b(empty|empty_like|zeros|zeros_like|ones|full|new_empty|new_zeros|clone|contiguous)\s*\(", src)
    assert "attn_contrib" not in W.allocating_wrappers()


def test_argument_validation_without_gpu():
    """Refused before anything is launched (no GPU here: a launch would fail differently), the argument named."""
    from variantformer_amd import _lib
    lib = _lib.load()
    p = 4096                                             # a non-null, 16-byte aligned address; never dereferenced
    INVALID = 1

    def call(v=p, v_stride=128, s_gram=p, probs=p, ldp=8, cu_rows=p, cu_k=p, n_seq=1, max_rows=4, max_k=8, H=2, dh=32,
             dtype=_lib.VF_BF16, per_head=0, gram=p, out=p, ldo=8):
        return lib.vf_attn_contrib(v, v_stride, s_gram, probs, ldp, cu_rows, cu_k, n_seq, max_rows, max_k, H, dh, dtype,
                                   per_head, gram, out, ldo, 0)

    def err():
        return lib.vf_last_error().decode()
    for name, word in (("v", "v"), ("s_gram", "s_gram"), ("probs", "probs"), ("cu_rows", "cu_rows"), ("cu_k", "cu_seqlens_k"),
                       ("gram", "gram"), ("out", "out")):
        assert call(**{name: 0}) == INVALID, name
        assert err().endswith(f"null pointer {word}"), err()
    for dh in (0, 16, 40, 56, 80, 256):                  # the maps' own set: 32 / 48 / 64 / 96 / 128
        assert call(dh=dh, v_stride=1024) == INVALID and "head_dim" in err()
    for dh in (32, 48, 64, 96, 128):
        assert call(dh=dh, v_stride=1024, n_seq=0) == 0
    assert call(ldo=7) == INVALID and "ldo" in err()
    assert call(ldp=7) == INVALID and "ldp" in err()
    assert call(v_stride=56) == INVALID and "v_stride" in err()                       # below H * dh = 64
    assert call(v=p + 8) == INVALID and "v" in err() and "16-byte" in err()
    assert call(v_stride=68) == INVALID and "v_stride" in err()                       # not a multiple of 8
    assert call(s_gram=p + 4) == INVALID and "s_gram" in err()
    for name in ("probs", "gram", "out"):
        assert call(**{name: p + 2}) == INVALID and name in err()
    assert call(dtype=_lib.VF_F32) == INVALID and "operand_dtype" in err()
    assert call(dtype=7) == INVALID and "operand_dtype" in err()
    assert call(n_seq=-1) == INVALID and "n_seq" in err()
    assert call(max_rows=-1) == INVALID and "max_rows" in err()
    assert call(max_k=-1) == INVALID and "max_seqlen_k" in err()
    assert call(H=0) == INVALID and "H=" in err()
    assert call(H=33, v_stride=33 * 32 + 8) == INVALID and "H=33" in err()            # what the norm kernel cannot hold
    assert call(H=32, v_stride=1024, n_seq=0) == 0                                    # H <= 32 is taken
    # the grid limits: vf_attn_probs's (sequences, row tiles) and the Gram grid
    assert call(n_seq=65536) == INVALID and "grid" in err()
    assert call(max_rows=64 * 65535 + 1) == INVALID and "grid" in err()
    assert call(H=32, v_stride=1024, n_seq=65535, max_k=2 ** 25, ldo=2 ** 25, ldp=2 ** 25) == INVALID and "grid" in err()
    assert call(n_seq=0) == 0 and call(max_rows=0) == 0                               # nothing selected: VF_OK, no launch


def test_capture_takes_contributions_and_defaults_to_off():
    from variantformer_amd import attn_maps
    with attn_maps.capture([0]) as cap:
        assert cap.contributions is False and cap.contrib is None
    with attn_maps.capture([1, 0], per_head=True, contributions=True) as cap:
        assert cap.contributions is True and cap.per_head is True and cap.contrib is None
        cap.begin(torch.arange(3), torch.tensor([0, 3], dtype=torch.int32), 3, torch.tensor([0, 5], dtype=torch.int32), 5)
        assert cap.contrib is None and cap._scratch is None
    for fn in ("predict_step_with_attention", "variant_prediction_with_attention"):
        from variantformer_amd.seq2gene.model_combined_modulator import Seq2GenePredictorCombinedModulator as M
        assert inspect.signature(getattr(M, fn)).parameters["contributions"].default is False
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    assert inspect.signature(VCFProcessor.predict_with_attention).parameters["contributions"].default is False


def test_unsupported_options_still_raise_by_name_with_contributions():
    from tests.helpers import SEQ2REG_512, build_model, seq2gene_kw
    small = dict(SEQ2REG_512, embedding_dim=64, num_heads=2, num_layers=1)
    kw = seq2gene_kw(emb_dim=64, heads=2, layers=3, token_dim=64, gene_emb_dim=64)
    model = build_model(small, kw, seed=1)
    with pytest.raises(ValueError, match="out of range"):
        model.predict_step_with_attention({}, 0, layers=[3], contributions=True)
    model.vep = True
    with pytest.raises(NotImplementedError, match="vep"):
        model.predict_step_with_attention({}, 0, contributions=True)
    for extra, word in ((dict(cross_alibi=True), "cross_alibi"), (dict(gene_pooling="max"), "gene_pooling")):
        other = build_model(small, dict(kw, **extra), seed=1)
        with pytest.raises(NotImplementedError, match=word):
            other.predict_step_with_attention({}, 0, contributions=True)
        other.vep = True
        with pytest.raises(NotImplementedError, match=word):
            other.variant_prediction_with_attention({}, contributions=True)


def test_contrib_gram_of_a_module_is_the_gram_matrix_of_the_packed_weight():
    """MHA.contrib_gram's arithmetic, restated on the CPU (the method itself packs through a GPU kernel): S[h, h'] = Wo_h^T Wo_h'
    of the 16-bit weight, symmetric under (h, e) <-> (h', e'), and v^T S v the squared norm of Wo v."""
    c = A.case(4, 32, "bf16")
    S = c.s_gram
    assert S.shape == (4, 4, 32, 32) and S.dtype == torch.float32
    assert torch.equal(S, S.permute(1, 0, 3, 2))
    v = c.v16.double().reshape(c.tk, 4, 32)
    g = torch.einsum("jhe,hgef,jgf->jhg", v, S.double(), v)
    want = A.reference(4, 32, "bf16")["gram"]
    assert float((g - want).abs().max() / want.abs().max()) < 1e-6


@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("H,dh", A.GEOMETRIES)
def test_the_operands_tell_the_norm_from_cheaper_quantities(H, dh, dtype):
    """A condition on the inputs, not a measurement: in at least a quarter of the (row, key) entries of every geometry the
    reference differs from each wrong quantity by more than 10 x the GPU limit, relative to the row maximum.  (And the GPU
    limits stay 4 x the measured maxima: the separation is bought with the operands, never with the limit.)"""
    assert A.OUT_TOL == 4.0 * A.MEASURED_OUT and A.GRAM_TOL == 4.0 * A.MEASURED_GRAM and 0 < A.OUT_TOL < 1e-5
    c, ref = A.case(H, dh, dtype), A.reference(H, dh, dtype)
    valid = c.valid()
    assert int(valid.sum()) == sum(r * k for r, k in zip(c.rl, c.kl))
    top = ref["n"].amax(dim=-1, keepdim=True)
    for name, wrong in A.wrong_quantities(H, dh, dtype).items():
        rel = ((ref["n"] - wrong).abs() / top.clamp_min(1e-300))[valid]
        share = float((rel > 10.0 * A.OUT_TOL).double().mean())
        print(f"[attn_contrib operands H={H} dh={dh} {dtype}] {name}: {share:.3f} of the entries differ by more than {10 * A.OUT_TOL:.1e}")
        assert share >= 0.25, (name, share)
    # per head the wrong quantity is the attention weight itself scaled to the same row maximum
    ph, P = ref["per_head"], c.P.double()
    scaled = P * (ph.amax(dim=-1, keepdim=True) / P.amax(dim=-1, keepdim=True).clamp_min(1e-300))
    rel = ((ph - scaled).abs() / ph.amax(dim=-1, keepdim=True).clamp_min(1e-300))[valid[:, None, :].expand_as(ph)]
    assert float((rel > 10.0 * A.OUT_TOL).double().mean()) >= 0.25


def test_reference_is_formed_from_vectors_and_matches_the_gram_form():
    """The float64 reference (vectors) and the Gram form (what the kernel evaluates) are the same number: the formula of the
    header, checked on the CPU to 1e-12 of the row maximum; zero past a sequence's keys and for the sequence without keys."""
    H, dh = 4, 32
    c, ref = A.case(H, dh, "bf16"), A.reference(H, dh, "bf16")
    P = c.P.double()
    for _, r, n_rows, k, n_keys in c.sequences():
        if n_rows and n_keys:
            p = P[r:r + n_rows, :, :n_keys]
            n2 = torch.einsum("rhj,rgj,jhg->rj", p, p, ref["gram"][k:k + n_keys])
            want = ref["n"][r:r + n_rows, :n_keys]
            assert float((n2.sqrt() - want).abs().max() / want.max()) < 1e-12
        assert bool((ref["n"][r:r + n_rows, n_keys:] == 0).all())
    assert A.out_err(ref["n"].float(), ref["n"]) < 1e-7

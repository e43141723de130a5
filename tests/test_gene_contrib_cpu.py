"""Gene-body contribution maps without a GPU: the vf_attn_contrib_self boundary (include/vf_hip_gene_contrib.h parses, its one
name is exported and bound through _lib.ENTRIES, every stream-taking
declaration has a write-set case in the parallel net, the wrapper allocates nothing), every refusal of the entry with the
argument named, the new keyword of the capture and of the public interface, and -- on the references alone -- that the operands
of tests/gene_contrib_cases.py tell the contribution norm from three cheaper quantities by far more than the GPU limit."""
import inspect
import os
import re

import pytest
import torch

from tests import gene_contrib_cases as G
from tests import write_set_cases as W
from tests.conftest import REPO

NAME = "vf_attn_contrib_self"


def _header(name="vf_hip_gene_contrib.h") -> str:
    with open(os.path.join(REPO, "include", name)) as f:
        return f.read()


def test_header_parses_and_its_name_is_exported_and_bound():
    """What is this header's own; the boundary every header shares is tests/test_abi_cpu.py's."""
    from variantformer_amd import _lib
    assert sorted(_lib.ENTRIES["vf_hip_gene_contrib.h"]) == [NAME], "ctypes binding and vf_hip_gene_contrib.h disagree"
    assert _lib.ABI_VERSION == 13 and _lib.load().vf_version() == 13


def test_every_stream_entry_of_the_header_has_a_write_set_case():
    """The rule of tests/test_attn_contrib_cpu.py for this header: entry and wrapper, head-summed and per head."""
    entries = W.stream_entries(_header())
    assert entries == [NAME]
    cases = G.ws_cases()
    assert {e for c in cases for e in c.entries} == set(entries)
    assert len({c.name for c in cases}) == len(cases)
    for H, dh, Do, dtype in G.WS_GEOMETRIES:
        for ph in ("summed", "per_head"):
            for how in ("entry", "wrapper"):
                assert any(c.name == f"attn_contrib_self-H{H}-dh{dh}-Do{Do}-{dtype}-{ph}-{how}" for c in cases)
    assert all(c.wrappers == (("attn_contrib_self",) if c.name.endswith("wrapper") else ()) for c in cases)


def test_the_wrapper_allocates_nothing():
    from variantformer_amd import ops
    src = inspect.getsource(ops.attn_contrib_self)
    assert not re.search(r"\b(empty|empty_like|zeros|zeros_like|ones|full|new_empty|new_zeros|clone|contiguous)\s*\(", src)
    assert "attn_contrib_self" not in W.allocating_wrappers()


def test_argument_validation_without_gpu():
    """Refused before anything is launched (no GPU here: a launch would fail differently), the argument named."""
    from variantformer_amd import _lib
    lib = _lib.load()
    p = 4096                                             # a non-null, 16-byte aligned address; never dereferenced
    INVALID = 1

    def call(v=p, v_stride=128, v_rows=0, wo=p, ldw=64, probs=p, ldp=8, cu_k=p, n_seq=1, max_k=8, H=2, dh=32, Do=96,
             dtype=_lib.VF_BF16, per_head=0, out=p, ldo=8):
        return lib.vf_attn_contrib_self(v, v_stride, v_rows, wo, ldw, probs, ldp, cu_k, n_seq, max_k, H, dh, Do, dtype, per_head,
                                        out, ldo, 0)

    def err():
        return lib.vf_last_error().decode()
    for name, word in (("v", "v"), ("wo", "wo"), ("probs", "probs"), ("cu_k", "cu_seqlens_k"), ("out", "out")):
        assert call(**{name: 0}) == INVALID, name
        assert err().endswith(f"null pointer {word}"), err()
    assert call(v_rows=0, n_seq=0) == 0 and call(v_rows=p, n_seq=0) == 0               # v_rows may be null
    for dh in (0, 16, 40, 56, 80, 256):
        assert call(dh=dh, v_stride=1024, ldw=1024) == INVALID and "dh=" in err()
    for dh in (32, 48, 64, 96, 128):
        assert call(dh=dh, v_stride=1024, ldw=1024, n_seq=0) == 0
    for Do in (0, -32, 16, 100):
        assert call(Do=Do) == INVALID and "Do=" in err()
    assert call(Do=32, n_seq=0) == 0 and call(Do=1536, n_seq=0) == 0
    assert call(H=0) == INVALID and "H=0" in err()
    assert call(H=1025, v_stride=1025 * 32, ldw=1025 * 32) == INVALID and "H=1025" in err()
    assert call(H=1024, v_stride=1024 * 32, ldw=1024 * 32, n_seq=0) == 0
    assert call(ldo=7) == INVALID and "ldo" in err()
    assert call(ldp=7) == INVALID and "ldp" in err()
    assert call(v_stride=56) == INVALID and "v_stride" in err()                        # below H * dh = 64
    assert call(v_stride=68) == INVALID and "v_stride" in err()                        # not a multiple of 8
    assert call(ldw=56) == INVALID and "ldw" in err()
    assert call(ldw=68) == INVALID and "ldw" in err()
    assert call(v=p + 8) == INVALID and re.search(r"\bv must be 16-byte", err())
    assert call(wo=p + 8) == INVALID and re.search(r"\bwo must be 16-byte", err())
    assert call(v_rows=p + 4) == INVALID and "v_rows" in err()
    for name, word in (("probs", "probs"), ("out", "out"), ("cu_k", "cu_seqlens_k")):
        assert call(**{name: p + 2}) == INVALID and word in err()
    assert call(dtype=_lib.VF_F32) == INVALID and "operand_dtype" in err()
    assert call(dtype=7) == INVALID and "operand_dtype" in err()
    assert call(n_seq=-1) == INVALID and "n_seq" in err()
    assert call(max_k=-1) == INVALID and "max_seqlen_k" in err()
    assert call(n_seq=2 ** 31 - 1, max_k=512, ldo=512, ldp=512) == INVALID and "grid" in err()
    assert call(n_seq=0) == 0 and call(max_k=0) == 0                                   # nothing to do: VF_OK, no launch
    assert lib.vf_last_kernel(1).decode() == "attn_contrib_self_kernel"


def test_capture_takes_gene_contributions_and_defaults_to_off():
    from variantformer_amd import attn_maps
    params = list(inspect.signature(attn_maps.capture.__init__).parameters)
    assert params == ["self", "layers", "per_head", "gene_body", "contributions", "gene_contributions"]     # the fifth keyword
    with attn_maps.capture([0]) as cap:
        assert cap.gene_contributions is False and cap.gene_contrib is None
    cu = torch.tensor([0, 1, 2, 3], dtype=torch.int32)
    for gene_body in (False, True):                                  # independent of gene_body: running_self answers for either
        with attn_maps.capture([1, 0], per_head=True, gene_body=gene_body, gene_contributions=True) as cap:
            assert cap.gene_contributions is True and cap.gene_body is gene_body and cap.contributions is False
            cap.begin(torch.arange(3), torch.tensor([0, 3], dtype=torch.int32), 3, torch.tensor([0, 5], dtype=torch.int32), 5,
                      gene_self=(cu, torch.tensor([0, 4, 8, 12], dtype=torch.int32), 4))
            assert cap.gene_contrib is None and cap._self_scratch is None
            assert attn_maps.running_self() is None                  # no gene layer is running
            with cap.layer(1):
                assert attn_maps.running_self() is cap
            with cap.layer(2):                                       # not a requested layer
                assert attn_maps.running_self() is None
    with attn_maps.capture([0], contributions=True) as cap:
        cap.begin(torch.arange(3), torch.tensor([0, 3], dtype=torch.int32), 3, torch.tensor([0, 5], dtype=torch.int32), 5,
                  gene_self=(cu, torch.tensor([0, 4, 8, 12], dtype=torch.int32), 4))
        with cap.layer(0):
            assert attn_maps.running_self() is None and attn_maps.running() is cap
    from variantformer_amd.seq2gene.model_combined_modulator import Seq2GenePredictorCombinedModulator as M
    for fn in ("predict_step_with_attention", "variant_prediction_with_attention"):
        assert inspect.signature(getattr(M, fn)).parameters["gene_contributions"].default is False
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    assert inspect.signature(VCFProcessor.predict_with_attention).parameters["gene_contributions"].default is False


def test_unsupported_options_still_raise_by_name_with_gene_contributions():
    from tests.helpers import SEQ2REG_512, build_model, seq2gene_kw
    small = dict(SEQ2REG_512, embedding_dim=64, num_heads=2, num_layers=1)
    kw = seq2gene_kw(emb_dim=64, heads=2, layers=3, token_dim=64, gene_emb_dim=64)
    model = build_model(small, kw, seed=1)
    with pytest.raises(ValueError, match="out of range"):
        model.predict_step_with_attention({}, 0, layers=[3], gene_contributions=True)
    model.vep = True
    with pytest.raises(NotImplementedError, match="vep"):
        model.predict_step_with_attention({}, 0, gene_contributions=True)
    for extra, word in ((dict(cross_alibi=True), "cross_alibi"), (dict(gene_pooling="max"), "gene_pooling")):
        other = build_model(small, dict(kw, **extra), seed=1)
        with pytest.raises(NotImplementedError, match=word):
            other.predict_step_with_attention({}, 0, gene_contributions=True)
        other.vep = True
        with pytest.raises(NotImplementedError, match=word):
            other.variant_prediction_with_attention({}, gene_contributions=True)


@pytest.mark.parametrize("H,dh,Do,dtype", G.ALL, ids=[f"H{H}-dh{dh}-Do{Do}-{dt}" for H, dh, Do, dt in G.ALL])
def test_the_operands_tell_the_norm_from_cheaper_quantities(H, dh, Do, dtype):
    """A condition on the inputs, not a measurement: each wrong quantity's largest per-row error, relative to the row maximum,
    is at least 1000 x the GPU limit.  (`weight` coincides with the truth on the one-key sequence by construction -- one key,
    P = 1 in every head -- which is why the maximum over the call is the criterion.)  The smallest over all geometries and
    types, computed here: 0.092 (`diagonal`, H = 2, dh = 96)."""
    assert G.OUT_TOL == 4.0 * G.MEASURED_OUT and 0 < G.OUT_TOL < 1e-5
    c, ref = G.case(H, dh, Do, dtype), G.reference(H, dh, Do, dtype)
    assert int(c.valid().sum()) == c.tk and c.n_seq == len(G.KEY_LENS)
    assert bool((ref["n"][~c.valid()] == 0).all()) and bool((ref["n"][c.valid()] > 0).all())
    for name, wrong in G.wrong_quantities(H, dh, Do, dtype).items():
        e = G.out_err(wrong, ref["n"])
        print(f"[attn_contrib_self operands H={H} dh={dh} Do={Do} {dtype}] {name}: {e:.3f} of the row maximum")
        assert e >= 1000.0 * G.OUT_TOL, (name, e)
    # the triangle inequality between the two references
    assert bool((ref["n"] <= ref["per_head"].sum(dim=1) * (1 + 1e-12)).all())


def test_reference_is_formed_from_vectors():
    """The float64 reference against the definition, term by term, on the smallest geometry; zero for the sequence without keys."""
    H, dh, Do = 4, 32, 96
    c, ref = G.case(H, dh, Do, "bf16"), G.reference(H, dh, Do, "bf16")
    wo = c.wo16.double().view(Do, H, dh)
    v = c.v16.double().view(c.tk, H, dh)
    for s in (2, 6):
        k0, n = int(c.cu_k[s]), c.kl[s]
        for j in (0, n - 1):
            vec = sum(float(c.P[s, h, j]) * (wo[:, h] @ v[k0 + j, h]) for h in range(H))
            assert abs(float(vec.norm()) - float(ref["n"][s, j])) <= 1e-12 * float(ref["n"][s].max())
            for h in range(H):
                want = float(c.P[s, h, j]) * float((wo[:, h] @ v[k0 + j, h]).norm())
                assert abs(want - float(ref["per_head"][s, h, j])) <= 1e-12 * float(ref["per_head"][s, h].max())
    assert c.kl[4] == 0 and bool((ref["n"][4] == 0).all()) and bool((ref["per_head"][4] == 0).all())

"""Attention maps of a vep model: variant_prediction_with_attention returns variant_prediction's dict bit for bit plus the
gene -> cCRE and gene-body maps of the three genotypes (ref, het, hom), on the ref / het / hom batch construction of
tests/test_configs_gpu.py's VEP tests and a calibrated (sequence-sensitive) model.  predict_step_with_attention keeps refusing
vep models (it returns predict_step's dict; tests/test_attn_maps_gpu.py pins that)."""
import numpy as np
import pytest
import torch

from oracle import vf_oracle as O
from tests.attn_map_cases import oracle_registry_maps, total_variation
from tests.attn_self_map_cases import oracle_gene_body_maps
from tests.helpers import SEQ2REG_512, build_model, seq2gene_kw, state_dict_cpu
from variantformer_amd.utils.synthetic import TISSUES_54, calibrate_sequence_sensitivity, make_vep_batch

pytestmark = pytest.mark.gpu

N_CRE, N_CHUNKS, CRE_INDEX, GENE_INDEX = 9, 6, 4, (2, 2, 3)
TISSUES = TISSUES_54[:3]
VEP_KEYS = ("pred_gene_exp", "embd", "gene_token_embedding", "cre_token_embedding")


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    kw = seq2gene_kw(layers=3)
    model = build_model(SEQ2REG_512, kw, seed=77).cuda()
    calibrate_sequence_sensitivity(model)
    model.vep = True
    vb = make_vep_batch(515, N_CRE, N_CHUNKS, TISSUES, 200, cre_index=CRE_INDEX, gene_index=GENE_INDEX)
    plain = model.predict_step(vb, 0)
    att = model.variant_prediction_with_attention(vb, gene_body=True)
    return model, kw, vb, plain, att


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def test_the_five_outputs_are_variant_predictions(setup):
    model, _, vb, plain, att = setup
    for key in VEP_KEYS:
        assert _same(att[key], plain[key]), key
    assert att["variant_type"] == plain["variant_type"]
    again = model.variant_prediction_with_attention(vb, gene_body=True)
    for key in VEP_KEYS + ("cre_attention", "gene_attention"):
        assert _same(again[key], att[key]), key
    cross_only = model.variant_prediction_with_attention(vb)
    assert "gene_attention" not in cross_only and _same(cross_only["cre_attention"], att["cre_attention"])
    with pytest.raises(NotImplementedError, match="vep"):
        model.predict_step_with_attention(vb, 0)


def test_three_maps_of_each_kind(setup):
    _, _, _, _, att = setup
    assert att["cre_attention_layers"] == [0, 1, 2]
    assert len(att["cre_attention"]) == len(att["gene_attention"]) == 3               # ref, het, hom
    for g in range(3):
        c, b = att["cre_attention"][g], att["gene_attention"][g]
        assert c.shape == (3, len(TISSUES), N_CRE) and b.shape == (3, len(TISSUES), 1 + N_CHUNKS)
        for m in (c, b):
            assert m.dtype == np.float32 and np.isfinite(m).all() and (m >= 0).all()
            assert np.abs(m.astype(np.float64).sum(axis=-1) - 1.0).max() < 1e-5
    ph = setup[0].variant_prediction_with_attention(setup[2], layers=[-1], per_head=True, gene_body=True)
    for g in range(3):
        assert ph["gene_attention"][g].shape == (1, len(TISSUES), 32, 1 + N_CHUNKS)
        assert np.abs(ph["gene_attention"][g].astype(np.float64).mean(axis=2) - att["gene_attention"][g][2:3]).max() <= 32 * 2.0 ** -24
        assert np.abs(ph["cre_attention"][g].astype(np.float64).mean(axis=2) - att["cre_attention"][g][2:3]).max() <= 32 * 2.0 ** -24


def test_the_ref_map_is_the_plain_models_map_and_the_variant_moves_it(setup):
    """The ref genotype through the VEP forward (full last gene layer, every layer through the row map) against the same
    sample through the plain forward (registry-rows form of the last layer: another kernel form, so no bit-identity): within
    the limit of the oracle comparisons, 2 x the bf16 oracle's distance from the fp32 oracle.  And the het genotype's maps
    differ from the ref's in the column of the window / chunk the variant was planted in."""
    model, kw, vb, _, att = setup
    one = {"cre_sequences": vb["cre_sequences"][:1], "cre_attention_masks": vb["cre_attention_masks"][:1],
           "tissue_context": vb["tissue_context"][:1], "ref_cre_labels": vb["ref_labels"][:1], "strand_val": vb["strand"][:1],
           "gene_embeddings": vb["gene_embeddings"][:1], "gene_attention_masks": vb["gene_attention_masks"][:1]}
    model.vep = False
    try:
        plain = model.predict_step_with_attention(one, 0, gene_body=True)
    finally:
        model.vep = True
    sd = state_dict_cpu(model)
    shp, ghp = O.Seq2RegHP.from_hparams(SEQ2REG_512), O.Seq2GeneHP.from_kwargs(kw)
    mp = pytest.MonkeyPatch()
    try:
        body = {mode: oracle_gene_body_maps(mp, one, sd, shp, shp, ghp, mode)[1]["mean"][0] for mode in (None, "bf16")}
        cross = {mode: oracle_registry_maps(mp, one, sd, shp, shp, ghp, mode)[1][0] for mode in (None, "bf16")}
    finally:
        mp.undo()
    for name, key, orc in (("gene body", "gene_attention", body), ("cCRE", "cre_attention", cross)):
        limit = 2.0 * total_variation(orc["bf16"], orc[None])
        got = total_variation(att[key][0], plain[key][0])
        moved = total_variation(att[key][1], att[key][0])
        print(f"[vep maps, {name}] TV(ref through the VEP forward, plain forward) {got:.3e}; limit {limit:.3e}; "
              f"TV(het, ref) {moved:.3e}")
        assert got <= limit
    assert not np.array_equal(att["cre_attention"][1][..., CRE_INDEX], att["cre_attention"][0][..., CRE_INDEX])
    assert not np.array_equal(att["gene_attention"][1][..., 1 + GENE_INDEX[1]], att["gene_attention"][0][..., 1 + GENE_INDEX[1]])


def test_unsupported_options_refuse_the_capture_and_still_predict():
    vb = make_vep_batch(8, 6, 3, [7, 8], 200)
    for extra, word in ((dict(cross_alibi=True), "cross_alibi"), (dict(gene_pooling="max"), "gene_pooling")):
        model = build_model(SEQ2REG_512, dict(seq2gene_kw(layers=2), **extra), seed=11).cuda()
        model.vep = True
        with pytest.raises(NotImplementedError, match=word):
            model.variant_prediction_with_attention(vb)
        assert len(model.predict_step(vb, 0)["pred_gene_exp"]) == 3

"""Gene-body contribution maps end to end: predict_step_with_attention(gene_contributions=True) -- the norm of what the registry
token's own value and every gene-body chunk add to the token through the SELF attention's out_proj, beside the attention maps
-- against predict_step and the captures without it (same bits), against the oracle-side recorder of
tests/gene_contrib_cases.py (which forms the contribution vectors directly at the oracle's rounding points), on the calibrated
3-layer model and batch of tests/test_contribution_maps_gpu.py with the self attention's value third conditioned
(condition_self_value_side); a healed batch; the dataframe column of VCFProcessor.predict_with_attention; and the three
genotypes of a vep model.  The comparison with the oracle is only worth something if a contribution is not simply the ALiBi
attention weight rescaled: the test asserts that distance."""
import numpy as np
import pandas as pd
import pytest
import torch
import torch.nn.functional as F
import yaml

from oracle import vf_oracle as O
from tests.conftest import load_fixture
from tests.gene_contrib_cases import oracle_gene_contributions, row_err
from tests.helpers import SEQ2REG_512, build_model, seq2gene_kw, state_dict_cpu
from tests.test_attn_maps_gpu import N_CHUNKS, N_CRES, TISSUES, _same
from variantformer_amd.utils.synthetic import TISSUES_54, calibrate_sequence_sensitivity, make_batch, make_vep_batch

pytestmark = pytest.mark.gpu

OTHERS = ("pred_gene_exp", "embeddings", "cre_attention", "gene_attention", "cre_contribution")
H = 32


def _oracle(batch, sd, kw, modes):
    shp, ghp = O.Seq2RegHP.from_hparams(SEQ2REG_512), O.Seq2GeneHP.from_kwargs(kw)
    threads = torch.get_num_threads()
    torch.set_num_threads(16)
    mp = pytest.MonkeyPatch()
    try:
        return {mode: oracle_gene_contributions(mp, batch, sd, shp, shp, ghp, mode) for mode in modes}
    finally:
        mp.undo()
        torch.set_num_threads(threads)


def condition_self_value_side(model, tissues, keep: float = 0.1) -> None:
    """In place, on the VALUE third of every gene layer's Wqkv -- what this comparison needs from the operands: the component of
    a value along the registry tokens in use (the span of the layer's LayerNorm of their embeddings) is scaled to `keep`.  The
    registry token then hands itself a tenth of what its attention weight suggests, while ALiBi gives position 0 the largest
    weight of every row: the rows' maxima are gene-body chunks, and the map scaled to the same maximum is far from the
    contributions in column 0.
    What tests/test_contribution_maps_gpu.py::condition_value_side does for Wkv (a rank-one component along a seeded input
    direction) does not work here: the chunk rows come out of the 16-bit tokenizer, re-centred and rescaled by the calibration,
    so a value that follows one direction of them carries the tokenizer's rounding, amplified -- the bf16 oracle then sits 0.06
    from the fp32 oracle (against 0.004 without) and no 10 x separation fits below 1.  The registry embeddings are parameters,
    the same in every rounding mode.  Tuned on the CPU oracle alone, before any GPU run: limit 1.1e-2, separation 0.84."""
    ts = sorted({int(t) for row in tissues for t in row})
    with torch.no_grad():
        reg = model.start_tkn.registry_tokens.weight[ts].float()
        for layer in model.combined_modulator.gene_layers:
            w = layer.mixer.MHA.Wqkv.weight
            D = w.shape[1]
            q, _ = torch.linalg.qr(F.layer_norm(reg, (D,), layer.norm1.weight.float(), layer.norm1.bias.float()).t())
            w[2 * D:] -= (1.0 - keep) * (w[2 * D:] @ q) @ q.t()


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    kw = seq2gene_kw(layers=3)
    model = build_model(SEQ2REG_512, kw, seed=4242).cuda()
    calibrate_sequence_sensitivity(model)
    condition_self_value_side(model, TISSUES)
    batch = make_batch(99, N_CRES, N_CHUNKS, TISSUES, 200)
    oracle = _oracle(batch, state_dict_cpu(model), kw, (None, "bf16"))
    plain = model.predict_step(batch, 0)
    att = model.predict_step_with_attention(batch, 0, gene_body=True, contributions=True)
    con = model.predict_step_with_attention(batch, 0, gene_body=True, contributions=True, gene_contributions=True)
    return model, batch, plain, att, con, oracle


def _feature_launches(model, batch, **kw):
    from variantformer_amd import ops
    ops.TIMER = ops.KernelTimer(detail=True)
    try:
        model.predict_step_with_attention(batch, 0, **kw)
        order = list(ops.TIMER.order)
    finally:
        ops.TIMER = None
    return [(name, family) for name, _, family, _, _ in order if family.endswith("_gene_contrib")]


def test_gene_contributions_change_nothing_else_and_are_reproducible(setup):
    from variantformer_amd import runtime
    model, batch, plain, att, con, _ = setup
    assert "gene_contribution" not in att and con["cre_attention_layers"] == [0, 1, 2]
    assert set(con) == set(att) | {"gene_contribution"}
    for key in ("pred_gene_exp", "embeddings"):
        assert _same(con[key], plain[key]), key
    for key in OTHERS:
        assert _same(con[key], att[key]), key
    again = model.predict_step_with_attention(batch, 0, gene_body=True, contributions=True, gene_contributions=True)
    for key in OTHERS + ("gene_contribution",):
        assert _same(again[key], con[key]), key                                    # run to run
    with runtime.override(overlap_cre_stream=False):
        one_plain = model.predict_step(batch, 0)
        one = model.predict_step_with_attention(batch, 0, gene_body=True, contributions=True, gene_contributions=True)
    for key in ("pred_gene_exp", "embeddings"):
        assert _same(one[key], one_plain[key]) and _same(one[key], plain[key]), key
    for key in OTHERS[2:] + ("gene_contribution",):
        assert _same(one[key], con[key]), key                                      # the two stream orders
    # without gene_body only the contributions are returned, with the same bits (the per-head P then goes to the scratch)
    alone = model.predict_step_with_attention(batch, 0, gene_contributions=True)
    assert "gene_attention" not in alone and "cre_contribution" not in alone
    assert _same(alone["gene_contribution"], con["gene_contribution"]) and _same(alone["pred_gene_exp"], plain["pred_gene_exp"])
    # off: not one launch of the feature; on: one per-head probabilities launch and one contribution launch per layer
    assert _feature_launches(model, batch, gene_body=True, contributions=True) == []
    mine = _feature_launches(model, batch, gene_body=True, gene_contributions=True)
    assert [name for name, _ in mine] == ["attn_probs_alibi", "attn_contrib_self"] * 3, mine
    assert all("self" in family for _, family in mine), mine
    # per head with gene_body the gene map itself is the per-head P: no second probabilities launch
    mine = _feature_launches(model, batch, gene_body=True, gene_contributions=True, per_head=True)
    assert [name for name, _ in mine] == ["attn_contrib_self"] * 3, mine


def test_shapes_and_layer_selection(setup):
    model, batch, plain, att, con, _ = setup
    for i, m in enumerate(con["gene_contribution"]):
        assert m.shape == att["gene_attention"][i].shape == (3, len(TISSUES[i]), 1 + N_CHUNKS[i]) and m.dtype == np.float32
        assert np.isfinite(m).all() and (m > 0).all()
    last = model.predict_step_with_attention(batch, 0, layers=[-1], gene_contributions=True)      # the registry-rows form
    first = model.predict_step_with_attention(batch, 0, layers=[0], gene_contributions=True)      # through the row map
    two = model.predict_step_with_attention(batch, 0, layers=[2, 0], gene_body=True, gene_contributions=True)
    assert last["cre_attention_layers"] == [2] and first["cre_attention_layers"] == [0] and two["cre_attention_layers"] == [2, 0]
    for i in range(3):
        assert np.array_equal(last["gene_contribution"][i], con["gene_contribution"][i][2:3])
        assert np.array_equal(first["gene_contribution"][i], con["gene_contribution"][i][0:1])
        for key in ("gene_contribution", "gene_attention"):
            assert np.array_equal(two[key][i], con[key][i][[2, 0]]), key
        assert np.array_equal(last["pred_gene_exp"][i], plain["pred_gene_exp"][i])


def test_gene_contributions_against_the_oracle(setup):
    """Per-row error relative to the row maximum, against the pure-fp32 oracle: at most 2 x the same-rounding (bf16) oracle's own
    distance from it (the rule of tests/test_contribution_maps_gpu.py::test_contributions_against_the_oracle) -- and the fp32
    reference at least 10 x that limit away from the gene-body attention map scaled to the same row maximum, or the test could
    not tell a contribution from an ALiBi weight.  The limit and the separation come from the CPU oracle alone (limit 1.1e-2,
    separation 0.84 with the calibration run through the oracle's tokenizer).
    Measured on MI355X (bf16 operands): the product 5.61e-3 from the fp32 oracle (5.2e-4 from the bf16 oracle) against a limit
    of 1.17e-2; the fp32 oracle's contributions sit 0.845 of the row maximum from the gene-body map scaled to it."""
    _, _, _, _, con, oracle = setup
    ref, same, maps32 = oracle[None]["n"], oracle["bf16"]["n"], oracle[None]["mean"]
    limit = 2.0 * max(row_err(same[i], ref[i]) for i in range(3))
    got = max(row_err(con["gene_contribution"][i], ref[i]) for i in range(3))
    got_same = max(row_err(con["gene_contribution"][i], same[i]) for i in range(3))
    scaled = [maps32[i] * (ref[i].max(axis=-1, keepdims=True) / maps32[i].max(axis=-1, keepdims=True)) for i in range(3)]
    apart = min(row_err(scaled[i], ref[i]) for i in range(3))
    print(f"[gene contribution maps] err(product, fp32 oracle) {got:.3e}; err(product, bf16 oracle) {got_same:.3e}; limit 2 x "
          f"err(bf16 oracle, fp32 oracle) = {limit:.3e}; err(gene-body map scaled to the row maximum, fp32 oracle) {apart:.3e}")
    assert apart >= 10.0 * limit, "a contribution is the attention weight rescaled to within the limit: this would pass vacuously"
    assert got <= limit


def test_per_head_gene_contributions(setup):
    """Shape, the triangle inequality against the head-summed norm, and the oracle rule per head.  Measured on MI355X:
    4.55e-2 against a limit of 8.98e-2."""
    model, batch, _, att, con, oracle = setup
    ph = model.predict_step_with_attention(batch, 0, per_head=True, gene_body=True, gene_contributions=True)
    limit = 2.0 * max(row_err(oracle["bf16"]["per_head"][i], oracle[None]["per_head"][i]) for i in range(3))
    for i in range(3):
        m = ph["gene_contribution"][i]
        assert m.shape == ph["gene_attention"][i].shape == (3, len(TISSUES[i]), H, 1 + N_CHUNKS[i]) and m.dtype == np.float32
        # the triangle inequality: the norm of the sum is at most the sum of the heads' norms
        assert (con["gene_contribution"][i] <= m.astype(np.float64).sum(axis=2) * (1 + 1e-5)).all()
    got = max(row_err(ph["gene_contribution"][i], oracle[None]["per_head"][i]) for i in range(3))
    print(f"[gene contribution maps, per head] err(product, fp32 oracle) {got:.3e}; limit {limit:.3e}")
    assert got <= limit
    plain_ph = model.predict_step_with_attention(batch, 0, per_head=True, gene_body=True)
    assert _same(ph["gene_attention"], plain_ph["gene_attention"]) and _same(ph["pred_gene_exp"], plain_ph["pred_gene_exp"])
    alone = model.predict_step_with_attention(batch, 0, per_head=True, gene_contributions=True)       # P through the scratch
    assert _same(alone["gene_contribution"], ph["gene_contribution"])


def test_a_healed_batch_returns_the_recomputations_gene_contributions(monkeypatch):
    """As tests/test_contribution_maps_gpu.py::test_a_healed_batch_returns_the_recomputations_contributions."""
    from variantformer_amd import ops
    from variantformer_amd.seq2gene.modules import layers as L
    monkeypatch.delenv("VF_LN_FOLD", raising=False)
    monkeypatch.delenv("VF_TRUNK16", raising=False)
    monkeypatch.setattr(L, "_LN_FOLD_DISABLED", False)
    tissues = [TISSUES_54[:3], [9]]
    model = build_model(SEQ2REG_512, seq2gene_kw(layers=2), seed=4242).cuda()
    batch = make_batch(99, [12, 5], [5, 3], tissues, 200)
    ops.ln_fold_alert(torch.device("cuda", torch.cuda.current_device()))
    with torch.no_grad():                                  # registry rows in use get a mean of 20 standard deviations
        w = model.start_tkn.registry_tokens.weight
        for t in sorted({t for ts in tissues for t in ts}):
            w[t] += 20.0 * w[t].std()
    monkeypatch.setenv("VF_LN_FOLD", "0")
    plain = model.predict_step_with_attention(batch, 0, gene_body=True, gene_contributions=True)
    maps_only = model.predict_step_with_attention(batch, 0, gene_body=True)
    monkeypatch.delenv("VF_LN_FOLD")
    healed = model.predict_step_with_attention(batch, 0, gene_body=True, gene_contributions=True)
    assert model.ln_fold_state()["batches_recomputed"] == 1
    keys = ("pred_gene_exp", "embeddings", "cre_attention", "gene_attention")
    for key in keys + ("gene_contribution",):
        assert _same(healed[key], plain[key]), key
    for key in keys:
        assert _same(plain[key], maps_only[key]), key
    for i, m in enumerate(healed["gene_contribution"]):
        assert m.shape == (2, len(tissues[i]), 1 + [5, 3][i]) and np.isfinite(m).all()


def test_vcfprocessor_column(tmp_path):
    """The genome files of tests/test_contribution_maps_gpu.py::test_vcfprocessor_column: the gene_contribution column beside
    unchanged predictions and maps, split and shaped like gene_attention, its columns named by gene_chunk_table."""
    from tests.test_consensus_cpu import make_genome, write_fasta
    from tests.test_processors_gpu import _write_artifacts
    from variantformer_amd.datasets.vepdataset import LocalManifest
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    meta, arrays, sd, _ = load_fixture("small_sin")
    cfg_dir = _write_artifacts(tmp_path, meta, sd)
    fasta = str(tmp_path / "genome.fa")
    write_fasta(fasta, {"chr1": make_genome(99), "chr2": make_genome(100, 5000)})
    genes = pd.DataFrame([
        {"gene_id": "ENSG_A", "gene_name": "a", "chromosome": "chr1", "start": 1000, "end": 6000, "strand": "+"},
        {"gene_id": "ENSG_B", "gene_name": "b", "chromosome": "chr2", "start": 500, "end": 4000, "strand": "-"}])
    genes.to_csv(tmp_path / "genes.csv", index=False)
    cres = {"ENSG_A": [(2030, 2080, "dELS"), (1040, 1110, "PLS"), (5000, 5100, "dELS"), (1490, 1560, "pELS")],
            "ENSG_B": [(300, 390, "CTCF-only,CTCF-bound"), (1300, 1345, "DNase-H3K4me3"), (4400, 4460, "PLS")]}
    paths = {}
    for g, rows in cres.items():
        chrom = genes.set_index("gene_id").loc[g, "chromosome"]
        paths[g] = str(tmp_path / f"{g}.csv")
        pd.DataFrame([{"chromosome": chrom, "start_cre": a, "end_cre": b, "cre_name": n} for a, b, n in rows]).to_csv(paths[g], index=False)
    with open(cfg_dir / "vcfloader.yaml") as f:
        loader_cfg = yaml.safe_load(f)
    loader_cfg["fasta_path"] = fasta
    with open(cfg_dir / "vcfloader.yaml", "w") as f:
        yaml.safe_dump(loader_cfg, f)
    with open(cfg_dir / "vf_model.yaml") as f:
        model_cfg = yaml.safe_load(f)
    for blk in model_cfg.values():
        blk["dataset"].update(max_chunks=8, cre_neighbour_hood=15, gene_upstream_neighbour_hood=100,
                              gene_downstream_neighbour_hood=3000)
    with open(cfg_dir / "vf_model.yaml", "w") as f:
        yaml.safe_dump(model_cfg, f)
    vp = VCFProcessor(config_dir=str(cfg_dir), gene_cre_manifest=LocalManifest(paths))
    query = pd.DataFrame({"gene_id": ["ENSG_A", "ENSG_B"], "tissues": ["whole blood,thyroid", "liver"]})
    model, ckpt, trainer = vp.load_model()
    dataset, loader = vp.create_data(None, query.copy())
    body = vp.predict_with_attention(model, ckpt, trainer, loader, dataset, layers=[0, -1], gene_body=True)
    dataset, loader = vp.create_data(None, query.copy())
    out = vp.predict_with_attention(model, ckpt, trainer, loader, dataset, layers=[0, -1], gene_body=True, gene_contributions=True)
    assert sorted(out.columns) == sorted(list(body.columns) + ["gene_contribution"])
    for i in range(2):
        for col in ("predicted_expression", "embeddings", "cre_attention", "gene_attention", "gene_chunk_seq_start"):
            assert np.array_equal(out[col][i], body[col][i]), col
        m = out["gene_contribution"][i]
        assert m.shape == out["gene_attention"][i].shape and m.shape[:2] == (2, len(out["tissues"][i]))
        assert m.dtype == np.float32 and np.isfinite(m).all() and (m > 0).all()
        assert len(out["gene_chunk_seq_start"][i]) == m.shape[-1] - 1
    dataset, loader = vp.create_data(None, query.copy())
    alone = vp.predict_with_attention(model, ckpt, trainer, loader, dataset, layers=[-1], per_head=True, gene_contributions=True)
    heads = model.combined_modulator.num_heads
    assert "gene_attention" not in alone.columns and "gene_chunk_seq_start" in alone.columns
    for i in range(2):
        assert alone["gene_contribution"][i].shape == (1, len(out["tissues"][i]), heads, out["gene_contribution"][i].shape[-1])


def test_vep_model_one_entry_per_genotype():
    """variant_prediction_with_attention(gene_contributions=True) on the batch of tests/test_vep_attention_maps_gpu.py: the outputs
    and the other maps keep their bits, one map per genotype; the ref genotype through the VEP forward against the same sample
    through the plain forward within the oracle limit (another kernel form of the last layer, so no bit identity is asked).
    Measured on MI355X: ref through the VEP forward against the plain forward 0 (bit for bit), limit 6.99e-3; het against ref
    5.72e-3."""
    from tests.test_vep_attention_maps_gpu import CRE_INDEX, GENE_INDEX, N_CRE, VEP_KEYS
    from tests.test_vep_attention_maps_gpu import N_CHUNKS as VEP_CHUNKS
    from tests.test_vep_attention_maps_gpu import TISSUES as VEP_TISSUES
    kw = seq2gene_kw(layers=3)
    model = build_model(SEQ2REG_512, kw, seed=77).cuda()
    calibrate_sequence_sensitivity(model)
    model.vep = True
    vb = make_vep_batch(515, N_CRE, VEP_CHUNKS, VEP_TISSUES, 200, cre_index=CRE_INDEX, gene_index=GENE_INDEX)
    plain = model.predict_step(vb, 0)
    att = model.variant_prediction_with_attention(vb, gene_body=True)
    con = model.variant_prediction_with_attention(vb, gene_body=True, gene_contributions=True)
    for key in VEP_KEYS + ("cre_attention", "gene_attention"):
        assert _same(con[key], att[key]), key
    for key in VEP_KEYS:
        assert _same(con[key], plain[key]), key
    assert "gene_contribution" not in att and len(con["gene_contribution"]) == 3            # ref, het, hom
    for g in range(3):
        m = con["gene_contribution"][g]
        assert m.shape == (3, len(VEP_TISSUES), 1 + VEP_CHUNKS) and m.dtype == np.float32 and np.isfinite(m).all() and (m > 0).all()
    one = {"cre_sequences": vb["cre_sequences"][:1], "cre_attention_masks": vb["cre_attention_masks"][:1],
           "tissue_context": vb["tissue_context"][:1], "ref_cre_labels": vb["ref_labels"][:1], "strand_val": vb["strand"][:1],
           "gene_embeddings": vb["gene_embeddings"][:1], "gene_attention_masks": vb["gene_attention_masks"][:1]}
    model.vep = False
    try:
        forward = model.predict_step_with_attention(one, 0, gene_contributions=True)
    finally:
        model.vep = True
    oracle = _oracle(one, state_dict_cpu(model), kw, (None, "bf16"))
    limit = 2.0 * row_err(oracle["bf16"]["n"][0], oracle[None]["n"][0])
    got = row_err(con["gene_contribution"][0], forward["gene_contribution"][0])
    moved = row_err(con["gene_contribution"][1], con["gene_contribution"][0])
    print(f"[vep gene contribution maps] err(ref through the VEP forward, plain forward) {got:.3e}; limit {limit:.3e}; "
          f"err(het, ref) {moved:.3e}")
    assert got <= limit
    with pytest.raises(NotImplementedError, match="vep"):
        model.predict_step_with_attention(vb, 0, gene_contributions=True)

"""cCRE contribution maps end to end: predict_step_with_attention(contributions=True) -- the norm of what every cCRE adds to
the registry token through the cross attention's out_proj, beside the attention maps -- against predict_step and the capture
without it (same bits), against the oracle-side recorder of tests/attn_contrib_cases.py (which forms the contribution vectors
directly at the oracle's rounding points), on the calibrated 3-layer model and batch of tests/test_attn_maps_gpu.py with the
value side conditioned (condition_value_side); the
dataframe column of VCFProcessor.predict_with_attention; and the three genotypes of a vep model.  The comparison with the
oracle is only worth something if a contribution is not simply the attention weight rescaled: the test asserts that distance."""
import numpy as np
import pandas as pd
import pytest
import torch
import yaml

from oracle import vf_oracle as O
from tests.attn_contrib_cases import oracle_registry_contributions, row_err
from tests.conftest import load_fixture
from tests.helpers import SEQ2REG_512, build_model, seq2gene_kw, state_dict_cpu
from tests.test_attn_maps_gpu import N_CHUNKS, N_CRES, TISSUES, _same
from variantformer_amd.utils.synthetic import TISSUES_54, calibrate_sequence_sensitivity, make_batch, make_vep_batch

pytestmark = pytest.mark.gpu

KEYS = ("pred_gene_exp", "embeddings", "cre_attention")
H = 32


def _oracle(batch, sd, kw, modes):
    shp, ghp = O.Seq2RegHP.from_hparams(SEQ2REG_512), O.Seq2GeneHP.from_kwargs(kw)
    threads = torch.get_num_threads()
    torch.set_num_threads(16)
    mp = pytest.MonkeyPatch()
    try:
        return {mode: oracle_registry_contributions(mp, batch, sd, shp, shp, ghp, mode) for mode in modes}
    finally:
        mp.undo()
        torch.set_num_threads(threads)


def condition_value_side(model, gain: float = 4.0, k_scale: float = 0.25, seed: int = 5) -> None:
    """In place, on every gene layer's cross attention -- what this comparison needs from the operands and the attention-map
    tests do not:
      - a rank-one component in the VALUE half of Wkv, gain x the Frobenius norm of that half, along a seeded input direction d:
        v_j gains gain * |Wv| * (x_j . d) u.  The calibrated cCRE rows are centred, so x_j . d changes sign and size from window
        to window and the value norms spread from near zero to several times their mean.  With plain seeded weights every
        window's value has much the same norm and a contribution is little more than the attention weight rescaled;
      - the KEY half (weight and bias) scaled by k_scale.  The calibration makes the logits large so that the MAPS are selective;
        the 16-bit rounding of q and k then moves a probability by a few percent of the row maximum, and twice that -- the
        limit below -- leaves no room for a 10 x separation on a scale that ends at 1.
    Measured on MI355X without either: the attention map scaled to the row maximum sits 0.39 from the fp32 reference against a
    limit of 0.056; with the value component alone 0.51 against 0.087."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in model.combined_modulator.gene_layers:
            wkv = layer.crossMHA.MHA.Wkv
            D = wkv.weight.shape[1]
            u, d = torch.randn(D, generator=g), torch.randn(D, generator=g)
            rank_one = torch.outer(u / u.norm(), d / d.norm()).to(wkv.weight.device)
            wkv.weight[D:] += gain * float(wkv.weight[D:].norm()) * rank_one
            wkv.weight[:D] *= k_scale
            wkv.bias[:D] *= k_scale


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    kw = seq2gene_kw(layers=3)
    model = build_model(SEQ2REG_512, kw, seed=4242).cuda()
    calibrate_sequence_sensitivity(model)
    condition_value_side(model)
    batch = make_batch(99, N_CRES, N_CHUNKS, TISSUES, 200)
    oracle = _oracle(batch, state_dict_cpu(model), kw, (None, "bf16"))
    plain = model.predict_step(batch, 0)
    att = model.predict_step_with_attention(batch, 0)
    con = model.predict_step_with_attention(batch, 0, contributions=True)
    return model, batch, plain, att, con, oracle


def test_contributions_change_nothing_else_and_are_reproducible(setup):
    from variantformer_amd import ops, runtime
    model, batch, plain, att, con, _ = setup
    assert "cre_contribution" not in att and con["cre_attention_layers"] == [0, 1, 2]
    for key in ("pred_gene_exp", "embeddings"):
        assert _same(con[key], plain[key]), key
    assert _same(con["cre_attention"], att["cre_attention"])
    again = model.predict_step_with_attention(batch, 0, contributions=True)
    for key in KEYS + ("cre_contribution",):
        assert _same(again[key], con[key]), key                                    # run to run
    with runtime.override(overlap_cre_stream=False):
        one_plain = model.predict_step(batch, 0)
        one = model.predict_step_with_attention(batch, 0, contributions=True)
    for key in ("pred_gene_exp", "embeddings"):
        assert _same(one[key], one_plain[key]) and _same(one[key], plain[key]), key
    for key in ("cre_attention", "cre_contribution"):
        assert _same(one[key], con[key]), key                                      # the two stream orders
    # off: not one launch of the feature; on: one contribution launch and one per-head probabilities launch per layer
    for on in (False, True):
        ops.TIMER = ops.KernelTimer(detail=True)
        try:
            model.predict_step_with_attention(batch, 0, contributions=on)
            order = list(ops.TIMER.order)
        finally:
            ops.TIMER = None
        mine = [name for name, _, family, _, _ in order if name.endswith("_contrib") or family.endswith("_contrib")]
        assert mine == (["attn_probs", "attn_contrib"] * 3 if on else []), mine
        assert all(family.endswith("cross_contrib") for name, _, family, _, _ in order if name == "attn_contrib")


def test_shapes_and_layer_selection(setup):
    model, batch, plain, att, con, _ = setup
    for i, m in enumerate(con["cre_contribution"]):
        assert m.shape == att["cre_attention"][i].shape == (3, len(TISSUES[i]), N_CRES[i]) and m.dtype == np.float32
        assert np.isfinite(m).all() and (m >= 0).all() and (m > 0).any()
    last = model.predict_step_with_attention(batch, 0, layers=[-1], contributions=True)
    two = model.predict_step_with_attention(batch, 0, layers=[0, 2], contributions=True)
    assert last["cre_attention_layers"] == [2] and two["cre_attention_layers"] == [0, 2]
    for i in range(3):
        for key in ("cre_contribution", "cre_attention"):
            assert np.array_equal(last[key][i], con[key][i][2:3]), key
            assert np.array_equal(two[key][i], con[key][i][[0, 2]]), key
        assert np.array_equal(last["pred_gene_exp"][i], plain["pred_gene_exp"][i])


def test_contributions_against_the_oracle(setup):
    """Per-row error relative to the row maximum, against the pure-fp32 oracle: at most 2 x the same-rounding (bf16) oracle's own
    distance from it (the rule of tests/test_attn_maps_gpu.py::test_maps_against_the_oracle) -- and the fp32 reference at least
    10 x that limit away from the attention map scaled to the same row maximum, or the test could not tell a contribution from
    a weight.  Measured on MI355X (bf16 operands): the product 2.09e-2 from the fp32 oracle (5.4e-3 from the bf16 oracle) against
    a limit of 4.54e-2; the fp32 oracle's contributions sit 0.85 of the row maximum from the attention map scaled to it.  All
    three quantities of the first assert come from the CPU oracle alone."""
    _, _, _, _, con, oracle = setup
    maps32, ref, _ = oracle[None]
    _, same, _ = oracle["bf16"]
    limit = 2.0 * max(row_err(same[i], ref[i]) for i in range(3))
    got = max(row_err(con["cre_contribution"][i], ref[i]) for i in range(3))
    got_same = max(row_err(con["cre_contribution"][i], same[i]) for i in range(3))
    scaled = [maps32[i] * (ref[i].max(axis=-1, keepdims=True) / maps32[i].max(axis=-1, keepdims=True)) for i in (0, 1)]
    apart = min(row_err(scaled[i], ref[i]) for i in (0, 1))
    print(f"[contribution maps] err(product, fp32 oracle) {got:.3e}; err(product, bf16 oracle) {got_same:.3e}; limit 2 x "
          f"err(bf16 oracle, fp32 oracle) = {limit:.3e}; err(attention map scaled to the row maximum, fp32 oracle) {apart:.3e}")
    assert apart >= 10.0 * limit, "a contribution is the attention weight rescaled to within the limit: this would pass vacuously"
    assert got <= limit


def test_per_head_contributions(setup):
    """Shape, the triangle inequality against the head-summed norm, and the oracle rule per head.  Measured on MI355X: 4.83e-2
    against a limit of 1.02e-1."""
    model, batch, _, att, con, oracle = setup
    ph = model.predict_step_with_attention(batch, 0, per_head=True, contributions=True)
    limit = 2.0 * max(row_err(oracle["bf16"][2][i], oracle[None][2][i]) for i in range(3))
    for i in range(3):
        m = ph["cre_contribution"][i]
        assert m.shape == ph["cre_attention"][i].shape == (3, len(TISSUES[i]), H, N_CRES[i]) and m.dtype == np.float32
        # the triangle inequality: the norm of the sum is at most the sum of the heads' norms
        assert (con["cre_contribution"][i] <= m.astype(np.float64).sum(axis=2) * (1 + 1e-5)).all()
    got = max(row_err(ph["cre_contribution"][i], oracle[None][2][i]) for i in range(3))
    print(f"[contribution maps, per head] err(product, fp32 oracle) {got:.3e}; limit {limit:.3e}")
    assert got <= limit
    plain_ph = model.predict_step_with_attention(batch, 0, per_head=True)
    assert _same(ph["cre_attention"], plain_ph["cre_attention"]) and _same(ph["pred_gene_exp"], plain_ph["pred_gene_exp"])


def test_a_healed_batch_returns_the_recomputations_contributions(monkeypatch):
    """As tests/test_attn_maps_gpu.py::test_a_healed_batch_returns_the_recomputations_maps, with contributions."""
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
    plain = model.predict_step_with_attention(batch, 0, contributions=True)
    maps_only = model.predict_step_with_attention(batch, 0)
    monkeypatch.delenv("VF_LN_FOLD")
    healed = model.predict_step_with_attention(batch, 0, contributions=True)
    assert model.ln_fold_state()["batches_recomputed"] == 1
    for key in KEYS + ("cre_contribution",):
        assert _same(healed[key], plain[key]), key
    for key in KEYS:
        assert _same(plain[key], maps_only[key]), key
    for i, m in enumerate(healed["cre_contribution"]):
        assert m.shape == (2, len(tissues[i]), [12, 5][i]) and np.isfinite(m).all()


def test_vcfprocessor_column(tmp_path):
    """The genome files of tests/test_attn_maps_gpu.py::test_vcfprocessor_predict_with_attention: the cre_contribution column
    beside unchanged predictions and maps, split and shaped like cre_attention."""
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
    cross = vp.predict_with_attention(model, ckpt, trainer, loader, dataset, layers=[0, -1])
    dataset, loader = vp.create_data(None, query.copy())
    out = vp.predict_with_attention(model, ckpt, trainer, loader, dataset, layers=[0, -1], contributions=True)
    assert list(out.columns) == list(cross.columns) + ["cre_contribution"]
    for i in range(2):
        for col in ("predicted_expression", "embeddings", "cre_attention"):
            assert np.array_equal(out[col][i], cross[col][i]), col
        m = out["cre_contribution"][i]
        assert m.shape == out["cre_attention"][i].shape == (2, len(out["tissues"][i]), len(cres[out["gene_id"][i]]))
        assert m.dtype == np.float32 and np.isfinite(m).all() and (m > 0).all() and len(out["cre_names"][i]) == m.shape[-1]
    dataset, loader = vp.create_data(None, query.copy())
    ph = vp.predict_with_attention(model, ckpt, trainer, loader, dataset, layers=[-1], per_head=True, contributions=True)
    heads = model.combined_modulator.num_heads
    for i in range(2):
        assert ph["cre_contribution"][i].shape == (1, len(out["tissues"][i]), heads, len(cres[out["gene_id"][i]]))


def test_vep_model_one_entry_per_genotype():
    """variant_prediction_with_attention(contributions=True) on the batch of tests/test_vep_attention_maps_gpu.py: the five outputs
    and the maps keep their bits, one contribution map per genotype; the ref genotype through the VEP forward against the same
    sample through the plain forward within the oracle limit (another kernel form of the last layer, so no bit identity); the
    het genotype's contributions differ from the ref's in the column of the window the variant was planted in.  Measured on
    MI355X: ref through the VEP forward against the plain forward 0 (bit for bit), limit 1.80e-2; het against ref 1.03e-2."""
    from tests.test_vep_attention_maps_gpu import CRE_INDEX, GENE_INDEX, N_CRE, VEP_KEYS
    from tests.test_vep_attention_maps_gpu import N_CHUNKS as VEP_CHUNKS
    from tests.test_vep_attention_maps_gpu import TISSUES as VEP_TISSUES
    kw = seq2gene_kw(layers=3)
    model = build_model(SEQ2REG_512, kw, seed=77).cuda()
    calibrate_sequence_sensitivity(model)
    model.vep = True
    vb = make_vep_batch(515, N_CRE, VEP_CHUNKS, VEP_TISSUES, 200, cre_index=CRE_INDEX, gene_index=GENE_INDEX)
    plain = model.predict_step(vb, 0)
    att = model.variant_prediction_with_attention(vb)
    con = model.variant_prediction_with_attention(vb, contributions=True)
    for key in VEP_KEYS + ("cre_attention",):
        assert _same(con[key], att[key]), key
    for key in VEP_KEYS:
        assert _same(con[key], plain[key]), key
    assert "cre_contribution" not in att and len(con["cre_contribution"]) == 3             # ref, het, hom
    for g in range(3):
        m = con["cre_contribution"][g]
        assert m.shape == (3, len(VEP_TISSUES), N_CRE) and m.dtype == np.float32 and np.isfinite(m).all() and (m > 0).all()
    one = {"cre_sequences": vb["cre_sequences"][:1], "cre_attention_masks": vb["cre_attention_masks"][:1],
           "tissue_context": vb["tissue_context"][:1], "ref_cre_labels": vb["ref_labels"][:1], "strand_val": vb["strand"][:1],
           "gene_embeddings": vb["gene_embeddings"][:1], "gene_attention_masks": vb["gene_attention_masks"][:1]}
    model.vep = False
    try:
        forward = model.predict_step_with_attention(one, 0, contributions=True)
    finally:
        model.vep = True
    oracle = _oracle(one, state_dict_cpu(model), kw, (None, "bf16"))
    limit = 2.0 * row_err(oracle["bf16"][1][0], oracle[None][1][0])
    got = row_err(con["cre_contribution"][0], forward["cre_contribution"][0])
    moved = row_err(con["cre_contribution"][1], con["cre_contribution"][0])
    print(f"[vep contribution maps] err(ref through the VEP forward, plain forward) {got:.3e}; limit {limit:.3e}; "
          f"err(het, ref) {moved:.3e}")
    assert got <= limit
    assert not np.array_equal(con["cre_contribution"][1][..., CRE_INDEX], con["cre_contribution"][0][..., CRE_INDEX])
    with pytest.raises(NotImplementedError, match="vep"):
        model.predict_step_with_attention(vb, 0, contributions=True)

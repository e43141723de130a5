"""Gene-body attention maps end to end: predict_step_with_attention(gene_body=True) -- the registry tokens' SELF attention
over their own sequence (the token itself, then the gene-body chunks, with ALiBi) beside the gene -> cCRE maps -- against
predict_step and the capture without gene_body (same bits) and against the oracle-side helper tests/attn_self_map_cases.py, on
the calibrated 3-layer model and batch of tests/test_attn_maps_gpu.py; and VCFProcessor.predict_with_attention(gene_body=True)
on genome files.  The comparison is only worth something if the reference map is neither the bias alone nor the bias-free
softmax: the test asserts both distances."""
import numpy as np
import pandas as pd
import pytest
import torch
import yaml

from oracle import vf_oracle as O
from tests.attn_map_cases import total_variation
from tests.attn_self_map_cases import oracle_gene_body_maps
from tests.conftest import load_fixture
from tests.helpers import SEQ2REG_512, build_model, seq2gene_kw, state_dict_cpu
from variantformer_amd.utils.synthetic import TISSUES_54, calibrate_sequence_sensitivity, make_batch

pytestmark = pytest.mark.gpu

N_CRES, N_CHUNKS = [7, 40, 1], [3, 9, 2]
TISSUES = [[7], TISSUES_54[:5], [62, 10]]
KEYS = ("pred_gene_exp", "embeddings", "cre_attention")


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    kw = seq2gene_kw(layers=3)
    model = build_model(SEQ2REG_512, kw, seed=4242).cuda()
    calibrate_sequence_sensitivity(model)
    batch = make_batch(99, N_CRES, N_CHUNKS, TISSUES, 200)
    sd = state_dict_cpu(model)                            # with the calibrated cre_map / gene_map
    shp, ghp = O.Seq2RegHP.from_hparams(SEQ2REG_512), O.Seq2GeneHP.from_kwargs(kw)
    threads = torch.get_num_threads()
    torch.set_num_threads(16)
    mp = pytest.MonkeyPatch()
    try:
        oracle = {mode: oracle_gene_body_maps(mp, batch, sd, shp, shp, ghp, mode)[1] for mode in (None, "bf16", "fp16")}
    finally:
        mp.undo()
        torch.set_num_threads(threads)
    plain = model.predict_step(batch, 0)
    cross = model.predict_step_with_attention(batch, 0)
    both = model.predict_step_with_attention(batch, 0, gene_body=True)
    return model, batch, plain, cross, both, oracle


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def test_gene_body_changes_nothing_else_and_is_reproducible(setup):
    from variantformer_amd import runtime
    model, batch, plain, cross, both, _ = setup
    assert "gene_attention" not in cross
    for key in ("pred_gene_exp", "embeddings"):
        assert _same(both[key], plain[key]), key
    assert _same(both["cre_attention"], cross["cre_attention"]) and both["cre_attention_layers"] == [0, 1, 2]
    again = model.predict_step_with_attention(batch, 0, gene_body=True)
    for key in KEYS + ("gene_attention",):
        assert _same(again[key], both[key]), key                                   # run to run
    with runtime.override(overlap_cre_stream=False):
        one = model.predict_step_with_attention(batch, 0, gene_body=True)
    for key in KEYS + ("gene_attention",):
        assert _same(one[key], both[key]), key                                     # the two stream orders


def test_shapes_and_row_sums(setup):
    _, _, _, _, both, _ = setup
    for i, m in enumerate(both["gene_attention"]):
        assert m.shape == (3, len(TISSUES[i]), 1 + N_CHUNKS[i]) and m.dtype == np.float32       # registry token + C chunks
        assert np.isfinite(m).all() and (m >= 0).all()
        assert np.abs(m.astype(np.float64).sum(axis=-1) - 1.0).max() < 1e-5


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_maps_against_the_oracle(setup, mode):
    """The rule of tests/test_attn_maps_gpu.py::test_maps_against_the_oracle: per-row total variation from the fp32 oracle at
    most 2 x the same-rounding oracle's own distance from it -- and that limit at least 10 x smaller than the fp32 oracle map's
    distance from the two maps a wrong bias would give: the bias alone (head mean of softmax_j(-slope_h log2(e) j)) and the
    oracle's logits with the slopes removed (both on the nine-chunk gene).
    Measured on MI355X with the default calibration (gene_std = 1): bf16 operands 7.6e-4 against a limit of 1.52e-3, fp16
    1.2e-4 against 2.5e-4; the fp32 oracle's nine-chunk maps sit 1.62e-2 from the bias alone and 1.62e-1 from the map without
    slopes.  The first of the two is 10.6 x the bf16 limit: close to the bar, and scaling the mixer's Q / K rows would not move
    it (the distance from the bias alone and the 16-bit rounding of q and k both grow with the logits); the quantities on both
    sides of that assert come from the CPU oracle alone."""
    model, batch, _, _, both, oracle = setup
    if mode == "fp16":
        keep = model.precision
        model.precision = "16-mixed"
        try:
            both = model.predict_step_with_attention(batch, 0, gene_body=True)
        finally:
            model.precision = keep
    ref = oracle[None]
    limit = 2.0 * max(total_variation(oracle[mode]["mean"][i], ref["mean"][i]) for i in range(3))
    got = max(total_variation(both["gene_attention"][i], ref["mean"][i]) for i in range(3))
    from_bias = total_variation(ref["mean"][1], ref["bias_only"][1])
    from_no_slopes = total_variation(ref["mean"][1], ref["no_slopes"][1])
    print(f"[gene-body maps, {mode}] TV(product, fp32 oracle) {got:.3e}; limit 2 x TV({mode} oracle, fp32 oracle) = {limit:.3e}; "
          f"TV(fp32 oracle, bias alone) {from_bias:.3e}; TV(fp32 oracle, slopes removed) {from_no_slopes:.3e}")
    assert from_bias >= 10.0 * limit, "the map is the bias alone to within the limit: this comparison would pass vacuously"
    assert from_no_slopes >= 10.0 * limit, "the slopes do not show in the map: this comparison would pass vacuously"
    assert got <= limit


def test_layer_selection(setup):
    model, batch, plain, _, both, _ = setup
    last = model.predict_step_with_attention(batch, 0, layers=[-1], gene_body=True)
    two = model.predict_step_with_attention(batch, 0, layers=[0, 2], gene_body=True)
    assert last["cre_attention_layers"] == [2] and two["cre_attention_layers"] == [0, 2]
    for i in range(3):
        for key in ("gene_attention", "cre_attention"):
            assert np.array_equal(last[key][i], both[key][i][2:3]), key
            assert np.array_equal(two[key][i], both[key][i][[0, 2]]), key
        assert np.array_equal(last["pred_gene_exp"][i], plain["pred_gene_exp"][i])


def test_per_head_maps_average_to_the_head_mean(setup):
    model, batch, _, _, both, oracle = setup
    ph = model.predict_step_with_attention(batch, 0, per_head=True, gene_body=True)
    H = 32
    for i in range(3):
        m = ph["gene_attention"][i]
        assert m.shape == (3, len(TISSUES[i]), H, 1 + N_CHUNKS[i])
        assert np.abs(m.astype(np.float64).mean(axis=2) - both["gene_attention"][i]).max() <= H * 2.0 ** -24
        assert np.abs(m.astype(np.float64).sum(axis=-1) - 1.0).max() < 1e-5
    # every head is its own head (each has its own slope): the rule of test_maps_against_the_oracle, per head
    limit = 2.0 * max(total_variation(oracle["bf16"]["per_head"][i], oracle[None]["per_head"][i]) for i in range(3))
    got = max(total_variation(ph["gene_attention"][i], oracle[None]["per_head"][i]) for i in range(3))
    print(f"[gene-body maps, per head] TV(product, fp32 oracle) {got:.3e}; limit {limit:.3e}")
    assert got <= limit


def test_a_model_without_alibi_records_the_bias_free_map():
    kw = dict(seq2gene_kw(layers=2), use_alibi=False)
    model = build_model(SEQ2REG_512, kw, seed=4242).cuda()
    calibrate_sequence_sensitivity(model)
    batch = make_batch(99, N_CRES, N_CHUNKS, TISSUES, 200)
    shp, ghp = O.Seq2RegHP.from_hparams(SEQ2REG_512), O.Seq2GeneHP.from_kwargs(kw)
    mp = pytest.MonkeyPatch()
    try:
        oracle = {mode: oracle_gene_body_maps(mp, batch, state_dict_cpu(model), shp, shp, ghp, mode)[1] for mode in (None, "bf16")}
    finally:
        mp.undo()
    got = model.predict_step_with_attention(batch, 0, gene_body=True)
    for i in range(3):
        assert np.array_equal(oracle[None]["mean"][i], oracle[None]["no_slopes"][i])          # the oracle had no slopes either
    limit = 2.0 * max(total_variation(oracle["bf16"]["mean"][i], oracle[None]["mean"][i]) for i in range(3))
    assert max(total_variation(got["gene_attention"][i], oracle[None]["mean"][i]) for i in range(3)) <= limit


def test_a_healed_batch_returns_the_recomputations_maps(monkeypatch):
    """As tests/test_attn_maps_gpu.py::test_a_healed_batch_returns_the_recomputations_maps, for both kinds of map."""
    from variantformer_amd import ops
    from variantformer_amd.seq2gene.modules import layers as L
    monkeypatch.delenv("VF_LN_FOLD", raising=False)
    monkeypatch.delenv("VF_TRUNK16", raising=False)
    monkeypatch.setattr(L, "_LN_FOLD_DISABLED", False)
    tissues = [TISSUES_54[:3], [9]]
    model = build_model(SEQ2REG_512, seq2gene_kw(layers=2), seed=4242).cuda()
    batch = make_batch(99, [12, 5], [5, 3], tissues, 200)
    dev = torch.device("cuda", torch.cuda.current_device())
    ops.ln_fold_alert(dev)
    with torch.no_grad():                                  # registry rows in use get a mean of 20 standard deviations
        w = model.start_tkn.registry_tokens.weight
        for t in sorted({t for ts in tissues for t in ts}):
            w[t] += 20.0 * w[t].std()
    calls = {"n": 0}
    orig = model.forward_prepared

    def counted(*a, **k):
        calls["n"] += 1
        return orig(*a, **k)
    monkeypatch.setattr(model, "forward_prepared", counted)
    monkeypatch.setenv("VF_LN_FOLD", "0")
    plain = model.predict_step_with_attention(batch, 0, gene_body=True)
    assert calls["n"] == 1
    monkeypatch.delenv("VF_LN_FOLD")
    calls["n"] = 0
    healed = model.predict_step_with_attention(batch, 0, gene_body=True)
    assert calls["n"] == 2 and model.ln_fold_state()["batches_recomputed"] == 1
    for key in KEYS + ("gene_attention",):
        assert _same(healed[key], plain[key]), key
    for i, m in enumerate(healed["gene_attention"]):
        assert m.shape == (2, len(tissues[i]), 1 + [5, 3][i]) and np.abs(m.astype(np.float64).sum(axis=-1) - 1.0).max() < 1e-5


def test_vcfprocessor_predict_with_attention_gene_body(tmp_path):
    """The genome files of tests/test_attn_maps_gpu.py::test_vcfprocessor_predict_with_attention: the gene-body column beside
    unchanged predictions and cCRE maps, and a chunk table row per map column behind the registry token's."""
    from tests.test_consensus_cpu import make_genome, write_fasta
    from tests.test_processors_gpu import _write_artifacts
    from variantformer_amd.datasets.vepdataset import LocalManifest
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    meta, arrays, sd, _ = load_fixture("small_sin")
    cfg_dir = _write_artifacts(tmp_path, meta, sd)
    g1, g2 = make_genome(99), make_genome(100, 5000)
    fasta = str(tmp_path / "genome.fa")
    write_fasta(fasta, {"chr1": g1, "chr2": g2})
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
    out = vp.predict_with_attention(model, ckpt, trainer, loader, dataset, layers=[0, -1], gene_body=True)
    new = ["gene_attention", "gene_chunk_seq_start", "gene_chunk_seq_end", "gene_chunk_start", "gene_chunk_end"]
    assert list(out.columns) == list(cross.columns) + new
    for i in range(2):
        for col in ("predicted_expression", "embeddings", "cre_attention"):
            assert np.array_equal(out[col][i], cross[col][i]), col
        m = out["gene_attention"][i]
        table = dataset.gene_chunk_table(out["gene_id"][i])
        assert m.shape == (2, len(out["tissues"][i]), 1 + len(table)) and len(table) > 1
        assert np.abs(m.astype(np.float64).sum(axis=-1) - 1.0).max() < 1e-5
        assert out["gene_chunk_seq_start"][i] == table["seq_start"].tolist() and out["gene_chunk_end"][i] == table["end"].tolist()
        assert all(v is not None for v in out["gene_chunk_start"][i])             # no VCF: the reference itself, bounds known
    assert out["gene_chunk_start"][0] == sorted(out["gene_chunk_start"][0])
    assert out["gene_chunk_start"][1] == sorted(out["gene_chunk_start"][1], reverse=True)      # minus strand: 5' end first

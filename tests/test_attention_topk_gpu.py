"""Ranked cCREs end to end: predict_step_with_attention(top_k=K) against the same call without top_k -- predictions and
embeddings bit for bit, and every `*_top_value` / `*_top_index` array equal, bit for bit, to the numpy reference of
tests/topk_cases.py applied to the corresponding full map (the maps are deterministic: no atomics) -- on two ragged genes whose
widths straddle K, with and without per_head; the three genotypes of a vep model; and the columns of
VCFProcessor.predict_with_attention with the names looked up in cre_table."""
import numpy as np
import pandas as pd
import pytest
import torch
import yaml

from tests import topk_cases as T
from tests.conftest import load_fixture
from tests.helpers import SEQ2REG_512, build_model, seq2gene_kw
from variantformer_amd.utils.synthetic import TISSUES_54, calibrate_sequence_sensitivity, make_batch, make_vep_batch

pytestmark = pytest.mark.gpu

K = 8
N_CRES, N_CHUNKS = [5, 40], [3, 12]                 # cCRE maps 5 and 40 wide, gene-body maps 4 and 13: one below K, one above
TISSUES = [[7], TISSUES_54[:5]]
MAPS = ("cre_attention", "gene_attention", "cre_contribution", "gene_contribution")
ALL = dict(gene_body=True, contributions=True, gene_contributions=True)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    model = build_model(SEQ2REG_512, seq2gene_kw(layers=3), seed=4242).cuda()
    calibrate_sequence_sensitivity(model)
    batch = make_batch(99, N_CRES, N_CHUNKS, TISSUES, 200)
    return model, batch, model.predict_step(batch, 0)


def _check_against_the_full_maps(full: dict, top: dict, k: int, widths: dict) -> int:
    """Every ranked array of `top` against the reference applied to the full map of `full`; returns how many -1 it saw."""
    padded = 0
    for name in MAPS:
        assert name not in top and len(top[name + "_top_value"]) == len(top[name + "_top_index"]) == len(full[name])
        for i, m in enumerate(full[name]):
            w = m.shape[-1]
            assert w == widths[name][i]
            want_v, want_i = T.reference(m.reshape(-1, w), k)
            got_v, got_i = top[name + "_top_value"][i], top[name + "_top_index"][i]
            assert got_v.dtype == np.float32 and got_i.dtype == np.int32
            assert got_v.shape == got_i.shape == m.shape[:-1] + (k,), (name, i, got_v.shape)
            assert np.array_equal(got_i.reshape(-1, k), want_i), (name, i)
            assert np.array_equal(T.bits(got_v).reshape(-1, k), T.bits(want_v)), (name, i)
            # -1 / +0.0 exactly where the gene has fewer than k columns
            assert (got_i[..., :min(w, k)] >= 0).all() and (got_i[..., min(w, k):] == -1).all()
            assert (T.bits(got_v)[..., min(w, k):] == 0).all()
            padded += int((got_i == -1).sum())
    return padded


@pytest.mark.parametrize("per_head", (False, True), ids=("head_mean", "per_head"))
def test_rankings_equal_the_reference_on_the_full_maps(setup, per_head):
    model, batch, plain = setup
    full = model.predict_step_with_attention(batch, 0, per_head=per_head, **ALL)
    top = model.predict_step_with_attention(batch, 0, per_head=per_head, top_k=K, **ALL)
    for key in ("pred_gene_exp", "embeddings"):
        assert _same(top[key], full[key]) and _same(top[key], plain[key]), key
    assert top["cre_attention_layers"] == full["cre_attention_layers"] == [0, 1, 2]
    assert set(top) == (set(full) - set(MAPS)) | {n + s for n in MAPS for s in ("_top_value", "_top_index")} | {"cre_map_width", "gene_map_width"}
    assert top["cre_map_width"] == N_CRES and top["gene_map_width"] == [1 + c for c in N_CHUNKS]
    widths = {n: (N_CRES if n.startswith("cre") else [1 + c for c in N_CHUNKS]) for n in MAPS}
    padded = _check_against_the_full_maps(full, top, K, widths)
    H = model.combined_modulator.num_heads if per_head else 1
    assert padded == 3 * len(TISSUES[0]) * H * 2 * ((K - N_CRES[0]) + (K - 1 - N_CHUNKS[0]))          # gene 0 alone, both kinds of map
    for i in range(2):                                                                     # a ranking: descending, distinct columns
        v, ix = top["cre_attention_top_value"][i], top["cre_attention_top_index"][i]
        n = min(K, N_CRES[i])
        assert (np.diff(v[..., :n], axis=-1) <= 0).all()
        assert all(len(set(r[:n].tolist())) == n for r in ix.reshape(-1, K))
    again = model.predict_step_with_attention(batch, 0, per_head=per_head, top_k=K, **ALL)
    for name in MAPS:
        for s in ("_top_value", "_top_index"):
            assert _same(again[name + s], top[name + s]), name + s                         # run to run


def _launches(model, batch, **kw):
    from variantformer_amd import ops
    ops.TIMER = ops.KernelTimer(detail=True)
    try:
        model.predict_step_with_attention(batch, 0, **kw)
        order = list(ops.TIMER.order)
        summary = ops.TIMER.summary()
    finally:
        ops.TIMER = None
    return [(name, family) for name, _, family, _, _ in order if name == "topk_rows"], summary


def test_one_launch_per_requested_map_and_none_without_top_k(setup):
    model, batch, _ = setup
    assert _launches(model, batch, **ALL)[0] == []
    mine, summary = _launches(model, batch, top_k=K, **ALL)
    assert sorted(f for _, f in mine) == sorted(n + "_topk" for n in MAPS) and len(mine) == 4
    rows = 3 * sum(len(t) for t in TISSUES)
    valid = 3 * sum(len(t) * w for t, w in zip(TISSUES, N_CRES)), 3 * sum(len(t) * (1 + c) for t, c in zip(TISSUES, N_CHUNKS))
    assert summary["topk_rows"]["launches"] == 4
    assert summary["topk_rows"]["bytes"] == 4.0 * (2 * valid[0] + 2 * valid[1] + 4 * 2 * rows * K)        # valid values once + outputs
    only, _ = _launches(model, batch, top_k=3, layers=[-1])
    assert only == [("topk_rows", "cre_attention_topk")]
    sub = model.predict_step_with_attention(batch, 0, top_k=3, layers=[2, 0], contributions=True)
    ref = model.predict_step_with_attention(batch, 0, top_k=K, **ALL)
    for name in ("cre_attention", "cre_contribution"):                                     # another k, other layers: a prefix of the same rows
        for i in range(2):
            assert np.array_equal(sub[name + "_top_index"][i], ref[name + "_top_index"][i][[2, 0]][..., :3])
            assert np.array_equal(T.bits(sub[name + "_top_value"][i]), T.bits(ref[name + "_top_value"][i][[2, 0]][..., :3]))
    assert "gene_map_width" not in sub and "gene_attention_top_index" not in sub


def test_vep_model_one_entry_per_genotype():
    from tests.test_vep_attention_maps_gpu import CRE_INDEX, GENE_INDEX, N_CRE, VEP_KEYS
    from tests.test_vep_attention_maps_gpu import N_CHUNKS as VEP_CHUNKS
    from tests.test_vep_attention_maps_gpu import TISSUES as VEP_TISSUES
    assert 1 + VEP_CHUNKS < K < N_CRE                                                      # the widths straddle K here too
    model = build_model(SEQ2REG_512, seq2gene_kw(layers=3), seed=77).cuda()
    calibrate_sequence_sensitivity(model)
    model.vep = True
    vb = make_vep_batch(515, N_CRE, VEP_CHUNKS, VEP_TISSUES, 200, cre_index=CRE_INDEX, gene_index=GENE_INDEX)
    plain = model.predict_step(vb, 0)
    full = model.variant_prediction_with_attention(vb, **ALL)
    top = model.variant_prediction_with_attention(vb, top_k=K, **ALL)
    for key in VEP_KEYS:
        assert _same(top[key], full[key]) and _same(top[key], plain[key]), key
    assert len(top["cre_attention_top_index"]) == 3                                        # ref, het, hom
    widths = {n: ([N_CRE] * 3 if n.startswith("cre") else [1 + VEP_CHUNKS] * 3) for n in MAPS}
    assert _check_against_the_full_maps(full, top, K, widths) > 0
    with pytest.raises(NotImplementedError, match="vep"):
        model.predict_step_with_attention(vb, 0, top_k=K)


def test_vcfprocessor_columns(tmp_path):
    """The genome files of tests/test_gene_contribution_maps_gpu.py::test_vcfprocessor_column: genes of 4 and 3 cCRE windows
    under top_k = 4."""
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
    kw = dict(layers=[0, -1], gene_body=True, contributions=True)
    dataset, loader = vp.create_data(None, query.copy())
    full = vp.predict_with_attention(model, ckpt, trainer, loader, dataset, **kw)
    dataset, loader = vp.create_data(None, query.copy())
    out = vp.predict_with_attention(model, ckpt, trainer, loader, dataset, top_k=4, **kw)
    maps = ("cre_attention", "gene_attention", "cre_contribution")
    new = [n + s for n in maps for s in ("_top_value", "_top_index")] + ["cre_attention_top_names", "cre_contribution_top_names"]
    assert sorted(out.columns) == sorted([c for c in full.columns if c not in maps] + new)
    for i in range(2):
        for col in ("predicted_expression", "embeddings", "cre_names", "cre_start", "cre_end", "gene_chunk_seq_start", "cre_attention_layers"):
            assert np.array_equal(out[col][i], full[col][i]), col
        for name in maps:
            m = full[name][i]
            want_v, want_i = T.reference(m.reshape(-1, m.shape[-1]), 4)
            assert np.array_equal(out[name + "_top_index"][i].reshape(-1, 4), want_i), name
            assert np.array_equal(T.bits(out[name + "_top_value"][i]).reshape(-1, 4), T.bits(want_v)), name
            assert out[name + "_top_index"][i].shape == m.shape[:-1] + (4,)
        for name in ("cre_attention", "cre_contribution"):
            ix, names = out[name + "_top_index"][i], out[name + "_top_names"][i]
            assert names.shape == ix.shape
            table = out["cre_names"][i]
            assert all((nm is None and j == -1) or (j >= 0 and nm == table[j]) for nm, j in zip(names.reshape(-1), ix.reshape(-1)))
    assert [len(t) for t in out["cre_names"]] == [4, 3]                                   # one gene fills K = 4, one does not
    assert (out["cre_attention_top_index"][0] >= 0).all()
    assert (out["cre_attention_top_index"][1][..., 3] == -1).all() and (out["cre_attention_top_names"][1][..., 3] == None).all()  # noqa: E711
    assert (out["cre_attention_top_index"][1][..., :3] >= 0).all()

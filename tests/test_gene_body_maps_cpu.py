"""Gene-body attention maps without a GPU: the capture sink's second buffer, VCFDataset.gene_chunk_table against the sample
builder's own chunks (and against the genome where it names genomic bounds), and the oracle-side self-map helper."""
import numpy as np
import pytest
import torch

from tests.conftest import load_fixture
from tests.test_attn_maps_cpu import _vcf_dataset


def test_capture_names_the_self_attention_grouping_only_when_asked():
    from variantformer_amd import attn_maps
    rows, cu_r, cu_k = torch.arange(3), torch.tensor([0, 3], dtype=torch.int32), torch.tensor([0, 5], dtype=torch.int32)
    cu_one, cu_self = torch.arange(4, dtype=torch.int32), torch.tensor([0, 4, 8, 12], dtype=torch.int32)
    with attn_maps.capture([1]) as cap:                   # the default: the cross maps alone
        cap.begin(rows, cu_r, 3, cu_k, 5, gene_self=(cu_one, cu_self, 4))
        with attn_maps.gene_layer(1):
            assert attn_maps.running() is cap and attn_maps.running_self() is None
    with attn_maps.capture([1], gene_body=True) as cap:
        assert cap.gene_body and cap.gene_maps is None
        with attn_maps.gene_layer(1):
            assert attn_maps.running_self() is None      # no forward has begun
        cap.begin(rows, cu_r, 3, cu_k, 5, gene_self=(cu_one, cu_self, 4), shape=([3], [5], [3]))
        with attn_maps.gene_layer(0):
            assert attn_maps.running_self() is None      # not a requested layer
        with attn_maps.gene_layer(1, compact=True):
            assert attn_maps.running_self() is cap and cap._running == (0, True)
        cap.gene_maps = torch.zeros(1)
        cap.begin(rows, cu_r, 3, cu_k, 5, gene_self=(cu_one, cu_self, 4))
        assert cap.gene_maps is None and cap.maps is None         # a second forward starts afresh
    assert attn_maps.active() is None


def _oriented_reference(ds, info, start, end):
    from variantformer_amd.utils.data_process import open_fasta
    from variantformer_amd.utils.functions import reverse_complement
    ref = open_fasta(ds.fasta_path).fetch(info["chromosome"], int(start), int(end)).upper()
    return ref if info["strand"] == "+" else reverse_complement(ref)


@pytest.mark.parametrize("gene_id", ["ENSG_PLUS", "ENSG_MINUS"])
def test_gene_chunk_table_rows_are_the_chunks_of_the_sample(tmp_path, gene_id):
    ds, _ = _vcf_dataset(tmp_path)
    info = ds._get_gene_info(gene_id)
    chunks, masks = ds._get_gene(gene_id, info, None)
    table = ds.gene_chunk_table(gene_id)
    assert list(table.columns) == ["chunk", "tokens", "seq_start", "seq_end", "start", "end"]
    assert len(table) == chunks.shape[0] > 1 and table["chunk"].tolist() == list(range(len(table)))
    assert table["tokens"].tolist() == (~masks[:, 0, :]).sum(dim=1).tolist()
    assert (table["seq_start"].to_numpy()[1:] >= table["seq_end"].to_numpy()[:-1]).all() and table["seq_start"][0] >= 0
    # no variants: the consensus is the reference, so every chunk has genomic bounds, and the bases between them (read on the
    # gene's strand) spell the chunk's tokens -- up to the characters the encoder drops (N)
    for k in range(len(table)):
        n = int(table["tokens"][k])
        text = "".join(ds.bpe.id_to_token[int(t)] for t in chunks[k, 0, :n])
        span = _oriented_reference(ds, info, table["start"][k], table["end"][k])
        assert len(span) == table["seq_end"][k] - table["seq_start"][k]
        assert "".join(c for c in span if c != "N") == text
    if info["strand"] == "+":
        assert (np.diff(table["start"].to_numpy()) > 0).all()
    else:
        assert (np.diff(table["start"].to_numpy()) < 0).all()        # chunk 0 starts at the gene's 5' end: the highest coordinates


def test_gene_chunk_table_names_genomic_bounds_only_without_indels(tmp_path):
    from tests import vep_artifacts as va
    from tests.test_consensus_cpu import write_vcf
    ds, _ = _vcf_dataset(tmp_path)
    genome = va.make_spec()["genome"]
    info = ds._get_gene_info("ENSG_PLUS")
    lo = ds._extractor(ds.gene_downstream_neighbour_hood, ds.gene_upstream_neighbour_hood).gene_region(
        info["strand"], info["start"], int(info["end"]))[0]
    pos = lo + 40                                         # 1-based position of a base inside the first chunk
    ref = genome[pos - 1].upper()
    assert ref in "ACGT"
    snp, indel = str(tmp_path / "snp.vcf"), str(tmp_path / "indel.vcf")
    write_vcf(snp, {"chr1": [(pos, ref, ["A" if ref != "A" else "C"], "1/1")]})
    write_vcf(indel, {"chr1": [(pos, ref, [ref + "TT"], "1/1")]})
    plain, with_snp, with_indel = ds.gene_chunk_table("ENSG_PLUS"), ds.gene_chunk_table("ENSG_PLUS", snp), \
        ds.gene_chunk_table("ENSG_PLUS", indel)
    # a SNP keeps every base where it was (the tokens around it may change, and the chunk boundaries with them)
    assert with_snp["start"].notna().all() and with_snp["end"].notna().all() and with_snp["start"][0] == plain["start"][0]
    assert ((with_snp["end"] - with_snp["start"]) == (with_snp["seq_end"] - with_snp["seq_start"])).all()
    assert (with_snp["start"] - with_snp["seq_start"]).nunique() == 1
    assert with_indel["start"].isna().all() and with_indel["end"].isna().all()
    assert len(with_indel) == len(ds._get_gene("ENSG_PLUS", info, indel)[0])
    assert with_indel["seq_end"].iloc[-1] != plain["seq_end"].iloc[-1] or len(with_indel) != len(plain) or \
        with_indel["seq_start"].tolist() != plain["seq_start"].tolist()                   # the insertion moved the tokens


def test_oracle_self_map_helper_leaves_the_oracle_alone_and_rows_sum_to_one(monkeypatch):
    from oracle import vf_oracle as O
    from tests.attn_self_map_cases import oracle_gene_body_maps
    meta, arrays, sd, batch = load_fixture("small_alibi")
    hp = O.Seq2RegHP.from_hparams(meta["seq2reg"])
    ghp = O.Seq2GeneHP.from_kwargs(meta["seq2gene"])
    plain = O.predict_step(batch, sd, hp, hp, ghp, rounding="bf16", share_cre_stream=True)
    original = O.mha_self
    out, maps = oracle_gene_body_maps(monkeypatch, batch, sd, hp, hp, ghp, "bf16")
    assert O.mha_self is original                        # the patch ends with the helper
    for key in ("pred_gene_exp", "embeddings"):
        for a, b in zip(plain[key], out[key]):
            assert np.array_equal(a, b)                  # bit-identical predictions with the recorder in place
    _, picked = oracle_gene_body_maps(monkeypatch, batch, sd, hp, hp, ghp, "bf16", layers=[-1, 0])
    for i in range(len(batch["cre_sequences"])):
        T, G = len(batch["tissue_context"][i]), int(batch["gene_embeddings"][i].shape[0]) + 1
        for kind in ("mean", "no_slopes", "bias_only"):
            m = maps[kind][i]
            assert m.shape == (ghp.num_layers, T, G) and np.abs(m.sum(axis=-1) - 1.0).max() < 1e-12 and (m >= 0).all()
        assert np.allclose(maps["per_head"][i].mean(axis=2), maps["mean"][i], atol=1e-15)
        assert np.array_equal(picked["mean"][i], maps["mean"][i][[ghp.num_layers - 1, 0]])
        if G > 1:                                        # the bias alone decays with the distance from the registry token
            assert (np.diff(maps["bias_only"][i], axis=-1) < 0).all()

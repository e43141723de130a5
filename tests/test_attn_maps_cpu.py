"""Attention maps without a GPU: the vf_attn_probs boundary (declared, bound, exported, argument validation), the capture
sink's context handling, VCFDataset.cre_table against the sample builder's own row order, and the oracle-side map helper."""
import numpy as np
import pandas as pd
import pytest
import torch

from tests.conftest import REPO, load_fixture


def test_symbol_is_declared_bound_and_exported_under_abi_13():
    import ctypes
    import os
    import re
    from variantformer_amd import _lib
    from variantformer_amd.csrc.build import build_lib
    with open(os.path.join(REPO, "include", "vf_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+vf_attn_probs\s*\(", header)
    assert re.search(r"#define\s+VF_ABI_VERSION\s+13\b", header)
    assert len(_lib.SIGNATURES["vf_attn_probs"]) == 20
    assert hasattr(ctypes.CDLL(build_lib()), "vf_attn_probs")
    assert _lib.ABI_VERSION == 13 and _lib.load().vf_version() == 13


def test_argument_validation_without_gpu():
    """Refused before anything is launched (no GPU here: a launch would fail differently)."""
    from variantformer_amd import _lib
    lib = _lib.load()
    p = 4096                                             # a non-null, 16-byte aligned address; never dereferenced

    def call(q=p, k=p, q_rows=0, cu_rows=p, cu_k=p, n_seq=1, max_rows=4, max_k=8, H=2, dh=32, flags=2, stats=p, out=p, ldo=8,
             q_stride=64, k_stride=128, dtype=_lib.VF_BF16):
        return lib.vf_attn_probs(q, q_stride, k, k_stride, q_rows, cu_rows, cu_k, n_seq, max_rows, max_k, H, dh, 1.0, dtype,
                                 flags, 0, stats, out, ldo, 0)
    for name in ("q", "k", "out", "stats", "cu_rows", "cu_k"):
        assert call(**{name: 0}) == 1, name
        assert b"null" in lib.vf_last_error()
    assert call(dh=40) == 1 and b"head_dim" in lib.vf_last_error()
    assert call(ldo=7) == 1 and b"ldo" in lib.vf_last_error()
    assert call(flags=1) == 1 and call(flags=3) == 1 and call(flags=4) == 1          # VF_ATTN_Q_AT_START, unknown bits
    assert b"flags" in lib.vf_last_error()
    assert call(n_seq=-1) == 1 and call(max_rows=-1) == 1
    assert call(q_stride=56) == 1 and call(k_stride=32) == 1                          # below H * dh = 64
    assert call(dtype=_lib.VF_F32) == 1 and b"operand_dtype" in lib.vf_last_error()
    assert call(n_seq=0) == 0 and call(max_rows=0) == 0                               # nothing selected: VF_OK, no launch


def test_capture_is_a_context_variable_that_nests_and_restores():
    import threading
    from variantformer_amd import attn_maps
    assert attn_maps.active() is None and attn_maps.running() is None
    with attn_maps.gene_layer(0):                        # no capture open: a no-op
        assert attn_maps.running() is None
    with attn_maps.capture([2, 0]) as outer:
        assert attn_maps.active() is outer and attn_maps.running() is None
        outer.begin(torch.arange(3), torch.tensor([0, 3], dtype=torch.int32), 3, torch.tensor([0, 5], dtype=torch.int32), 5)
        with attn_maps.gene_layer(1):
            assert attn_maps.running() is None           # not a requested layer
        with attn_maps.gene_layer(0):
            assert attn_maps.running() is outer and outer._running == (1, False)
            with attn_maps.capture([0], per_head=True) as inner:
                assert attn_maps.active() is inner and attn_maps.running() is None
            assert attn_maps.running() is outer
        assert attn_maps.running() is None               # a CRE layer between two gene layers sees no running layer
        seen = []
        t = threading.Thread(target=lambda: seen.append(attn_maps.active()))
        t.start()
        t.join()
        assert seen == [None]                            # another thread starts without a capture
    assert attn_maps.active() is None


def test_layer_selection_and_refusals_without_gpu():
    from tests.helpers import SEQ2REG_512, build_model, seq2gene_kw
    small = dict(SEQ2REG_512, embedding_dim=64, num_heads=2, num_layers=1)
    kw = seq2gene_kw(emb_dim=64, heads=2, layers=3, token_dim=64, gene_emb_dim=64)
    model = build_model(small, kw, seed=1)
    with pytest.raises(ValueError, match="out of range"):
        model.predict_step_with_attention({}, 0, layers=[3])
    with pytest.raises(ValueError, match="out of range"):
        model.predict_step_with_attention({}, 0, layers=[-4])
    with pytest.raises(ValueError, match="no gene layer"):
        model.predict_step_with_attention({}, 0, layers=[])
    for twice in ([0, 0], [-1, 2], [1, 0, -2]):          # every slot of the result is one layer's map: no layer twice
        with pytest.raises(ValueError, match="twice"):
            model.predict_step_with_attention({}, 0, layers=twice)
    from variantformer_amd import attn_maps
    assert attn_maps.select_layers(3, None) == [0, 1, 2] and attn_maps.select_layers(3, [-1, 0]) == [2, 0]
    with pytest.raises(ValueError):
        attn_maps.capture([1, 1])
    model.vep = True
    with pytest.raises(NotImplementedError, match="vep"):
        model.predict_step_with_attention({}, 0)
    for extra, word in ((dict(cross_alibi=True), "cross_alibi"), (dict(gene_pooling="max"), "gene_pooling")):
        other = build_model(small, dict(kw, **extra), seed=1)
        with pytest.raises(NotImplementedError, match=word):
            other.predict_step_with_attention({}, 0)


# ---- VCFDataset.cre_table -------------------------------------------------------------------------------------------
def _vcf_dataset(tmp_path):
    """The synthetic genome of tests/vep_artifacts.py as FASTA + per-gene cCRE manifests: its plus- and its minus-strand gene,
    the plus gene once more with the manifest rows out of order, and once with a window past the chromosome end (empty)."""
    from tests import vep_artifacts as va
    from tests.test_consensus_cpu import write_fasta
    from variantformer_amd.datasets.vcfdataset import VCFDataset
    from variantformer_amd.datasets.vepdataset import LocalManifest
    spec = va.make_spec()
    fasta = str(tmp_path / "genome.fa")
    write_fasta(fasta, {"chr1": spec["genome"]})
    genes = [dict(g) for g in spec["genes"]]
    genes += [dict(genes[0], gene_id="ENSG_UNSORTED"), dict(genes[0], gene_id="ENSG_EMPTYWIN")]
    known = lambda n: "PLS" if n == "not-a-class" else n                             # noqa: E731
    rows = {g: [(a, b, known(n)) for a, b, n in v] for g, v in spec["cres"].items()}
    plus = rows["ENSG_PLUS"]
    rows["ENSG_UNSORTED"] = [plus[3], plus[0], plus[4], plus[2], plus[1]]
    rows["ENSG_EMPTYWIN"] = [plus[2], (len(spec["genome"]) + 1000, len(spec["genome"]) + 1050, "dELS"), plus[0]]
    paths = {}
    for g, v in rows.items():
        paths[g] = str(tmp_path / f"{g}.csv")
        pd.DataFrame([{"chromosome": "chr1", "start_cre": a, "end_cre": b, "cre_name": n} for a, b, n in v]).to_csv(paths[g], index=False)
    query = pd.DataFrame({"gene_id": list(rows), "tissues": ["liver"] * len(rows)})
    s = spec["settings"]
    ds = VCFDataset(max_length=s["max_length"], max_chunks=4, cre_neighbour_hood=s["cre_neighbour_hood"],
                    gencode_v24=pd.DataFrame(genes), gene_cre_manifest=LocalManifest(paths),
                    gene_upstream_neighbour_hood=s["gene_upstream_neighbour_hood"],
                    gene_downstream_neighbour_hood=s["gene_downstream_neighbour_hood"], query_df=query, fasta_path=fasta)
    return ds, rows


@pytest.mark.parametrize("path", ["batched", "per_window"])
def test_cre_table_is_the_row_order_of_cre_sequences(tmp_path, monkeypatch, path):
    ds, rows = _vcf_dataset(tmp_path)
    if path == "per_window":
        monkeypatch.setattr(type(ds), "_get_cres_batched", lambda self, *a, **k: None)
    for gene_id, manifest in rows.items():
        if path == "per_window" and gene_id == "ENSG_EMPTYWIN":
            continue                                     # (a window outside the genome is the batched builder's case)
        info = ds._get_gene_info(gene_id)
        X, mask, ref_labels, labels = ds._get_cres(gene_id, info, None)
        table = ds.cre_table(gene_id)
        assert list(table.columns) == ["chromosome", "start_cre", "end_cre", "cre_name"]
        assert len(table) == X.shape[0]
        assert [ds.ref_cre_to_idx[n] for n in table["cre_name"]] == ref_labels.tolist()
        starts = table["start_cre"].tolist()
        assert starts == sorted(starts, reverse=info["strand"] == "-")
        inside = sorted((a, b, n) for a, b, n in manifest if a < 6000)
        assert sorted(zip(table["start_cre"], table["end_cre"], table["cre_name"])) == inside
        # the rows really are these windows: row k holds the tokens of window k of the table, built on its own
        one = type(ds)._get_cres
        for k in (0, len(table) - 1):
            single = pd.DataFrame([table.iloc[k]])
            p = tmp_path / f"one_{path}_{gene_id}_{k}.csv"
            single.to_csv(p, index=False)
            monkeypatch.setattr(ds.gene_cre_manifest, "table", dict(ds.gene_cre_manifest.table, ONE=str(p)))
            Xk = one(ds, "ONE", info, None)[0]
            assert torch.equal(Xk[0], X[k])
    assert len(ds.cre_table("ENSG_EMPTYWIN")) == 2 and len(rows["ENSG_EMPTYWIN"]) == 3


def test_cre_table_follows_the_per_window_path_where_the_batched_builder_steps_aside(tmp_path):
    """Manifests the batched builder does not serve -- windows on several chromosomes, a chromosome the genome lacks -- are
    built window by window: process_subject keeps the manifest order when the padded starts already ascend, sorts by
    (chromosome, start) otherwise, and drops a window that yields no sequence.  cre_table must name exactly those rows."""
    from tests import vep_artifacts as va
    from tests.test_consensus_cpu import make_genome, write_fasta
    from variantformer_amd.datasets.vcfdataset import VCFDataset
    from variantformer_amd.datasets.vepdataset import LocalManifest
    spec = va.make_spec()
    fasta = str(tmp_path / "genome.fa")
    write_fasta(fasta, {"chr1": spec["genome"], "chr2": make_genome(100, 5000)})
    manifests = {
        # starts ascend across chromosomes: the manifest order is kept (chr2 first)
        "G_KEEP": [("chr2", 100, 160, "dELS"), ("chr1", 1040, 1110, "PLS"), ("chr1", 2030, 2080, "pELS")],
        # starts do not ascend: sorted by (chromosome, start)
        "G_SORT": [("chr2", 3000, 3060, "dELS"), ("chr1", 2030, 2080, "pELS"), ("chr2", 100, 160, "CTCF-only,CTCF-bound"),
                   ("chr1", 1040, 1110, "PLS")],
        # a chromosome the genome lacks: its window yields no sequence and is dropped, in both orders
        "G_DROP": [("chr1", 1040, 1110, "PLS"), ("chrZ", 1500, 1560, "dELS"), ("chr1", 2030, 2080, "pELS")],
        "G_DROP_SORT": [("chr1", 2030, 2080, "pELS"), ("chrZ", 1500, 1560, "dELS"), ("chr1", 1040, 1110, "PLS"),
                        ("chr1", 1490, 1560, "DNase-H3K4me3")],
    }
    want = {"G_KEEP": ["dELS", "PLS", "pELS"], "G_SORT": ["PLS", "pELS", "CTCF-only,CTCF-bound", "dELS"],
            "G_DROP": ["PLS", "pELS"], "G_DROP_SORT": ["PLS", "DNase-H3K4me3", "pELS"]}
    genes, paths = [], {}
    for g, rows in manifests.items():
        for strand in "+-":
            gid = f"{g}_{'P' if strand == '+' else 'M'}"
            genes.append({"gene_id": gid, "chromosome": "chr1", "start": 1000, "end": 2600, "strand": strand})
            paths[gid] = str(tmp_path / f"{gid}.csv")
            pd.DataFrame([{"chromosome": c, "start_cre": a, "end_cre": b, "cre_name": n} for c, a, b, n in rows]).to_csv(paths[gid], index=False)
    s = spec["settings"]
    ds = VCFDataset(max_length=s["max_length"], max_chunks=4, cre_neighbour_hood=s["cre_neighbour_hood"],
                    gencode_v24=pd.DataFrame(genes), gene_cre_manifest=LocalManifest(paths),
                    gene_upstream_neighbour_hood=s["gene_upstream_neighbour_hood"],
                    gene_downstream_neighbour_hood=s["gene_downstream_neighbour_hood"],
                    query_df=pd.DataFrame({"gene_id": list(paths), "tissues": ["liver"] * len(paths)}), fasta_path=fasta)
    for gid in paths:
        info = ds._get_gene_info(gid)
        table_in = pd.read_csv(paths[gid])
        assert ds._batched_windows(table_in) is None                       # these are the per-window path's manifests
        X, mask, ref_labels, labels = ds._get_cres(gid, info, None)
        table = ds.cre_table(gid)
        assert len(table) == X.shape[0]
        assert [ds.ref_cre_to_idx[n] for n in table["cre_name"]] == ref_labels.tolist()
        names = want[gid[:-2]]
        assert table["cre_name"].tolist() == (names if info["strand"] == "+" else names[::-1])
        # coordinates travel with the names
        by_name = {n: (c, a, b) for c, a, b, n in manifests[gid[:-2]]}
        assert [(c, a, b) for c, a, b in zip(table["chromosome"], table["start_cre"], table["end_cre"])] == \
            [by_name[n] for n in table["cre_name"]]


# ---- the oracle-side map helper -------------------------------------------------------------------------------------
def test_oracle_map_helper_leaves_the_oracle_alone_and_rows_sum_to_one(monkeypatch):
    from oracle import vf_oracle as O
    from tests.attn_map_cases import oracle_registry_maps, record_oracle_maps, total_variation
    meta, arrays, sd, batch = load_fixture("small_sin")
    hp = O.Seq2RegHP.from_hparams(meta["seq2reg"])
    ghp = O.Seq2GeneHP.from_kwargs(meta["seq2gene"])
    plain = O.predict_step(batch, sd, hp, hp, ghp, rounding="bf16", share_cre_stream=True)
    original = O.mha_cross
    out, maps = oracle_registry_maps(monkeypatch, batch, sd, hp, hp, ghp, "bf16")
    assert O.mha_cross is original                       # the patch ends with the helper
    for key in ("pred_gene_exp", "embeddings"):
        for a, b in zip(plain[key], out[key]):
            assert np.array_equal(a, b)                  # bit-identical predictions with the recorder in place
    assert len(maps) == len(meta["n_cres"])
    _, picked = oracle_registry_maps(monkeypatch, batch, sd, hp, hp, ghp, "bf16", layers=[-1, 0])     # the product's layer convention
    assert all(np.array_equal(p, m[[ghp.num_layers - 1, 0]]) for p, m in zip(picked, maps))
    with pytest.raises(ValueError):
        oracle_registry_maps(monkeypatch, batch, sd, hp, hp, ghp, "bf16", layers=[ghp.num_layers])
    for i, m in enumerate(maps):
        assert m.shape == (ghp.num_layers, len(batch["tissue_context"][i]), meta["n_cres"][i]) and m.dtype == np.float64
        assert np.abs(m.sum(axis=-1) - 1.0).max() < 1e-12 and (m >= 0).all()
    # every record of a forward: one [T * G, N] block per (gene, gene layer), rows summing to 1 per head as well
    with monkeypatch.context() as mp:
        records = record_oracle_maps(mp)
        O.predict_step(batch, sd, hp, hp, ghp, rounding=None, share_cre_stream=True)
    assert [r["layer"] for r in records] == list(range(ghp.num_layers)) * len(meta["n_cres"])
    for r in records:
        assert float((r["per_head"].sum(dim=-1) - 1.0).abs().max()) < 1e-12
        assert torch.allclose(r["mean"], r["per_head"].mean(dim=1))
    assert total_variation(maps[0], maps[0]) == 0.0

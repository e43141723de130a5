"""VCFProcessor: the vcf2exp API surface (reference processors/vcfprocessor.py:23-277) over the HIP model.

Kept: constructor(model_class), create_vcf_from_variant, get_tissues, get_genes, create_data, load_model, predict,
format_output with the same return types.  `create_data` builds the in-tree `VCFDataset` (FASTA + VCF + per-gene
cCRE manifest -> IUPAC consensus -> BPE, all in process: no samtools / bcftools subprocesses); the per-gene cCRE
manifest lookup (S3 + duckdb in the reference, utils/assets.py:307-368) is duck-typed: pass anything with
`get_file_path(gene_id)` as `gene_cre_manifest`.  A `dataset_factory` may replace the dataset (e.g.
datasets.SyntheticGeneDataset where no genome is available)."""
from __future__ import annotations

import gzip
import os
from pathlib import Path

import numpy as np
import pandas as pd
import torch
import yaml
from torch.utils.data import DataLoader

from ..datasets.vcfdataset import VCFDataset, collate_fn_batching
from ..utils.config import Config, load_yaml
from .model_manager import ModelManager
from .trainer import Trainer


def cre_class_names(num_classes: int) -> list:
    """The names of a tokenizer's classes: utils.constants.CREs when its heads have exactly that many, else the indices."""
    from ..utils.constants import CREs
    return list(CREs) if num_classes == len(CREs) else list(range(num_classes))


class VCFProcessor:
    def __init__(self, model_class: str = "v4_pcg", config_dir: str | None = None, require_gpu: bool = True,
                 gene_cre_manifest=None, indel_policy: str = "bcftools"):
        base_dir = Path(__file__).parent.parent.resolve()
        self.config_location = Path(config_dir) if config_dir else base_dir / "configs"
        self.model_config = load_yaml(str(self.config_location / "vf_model.yaml"))[model_class]
        with open(base_dir / "vocabs" / "tissue_vocab.yaml") as f:
            self.tissue_vocab = yaml.safe_load(f)
        self.vcf_loader_config = load_yaml(str(self.config_location / "vcfloader.yaml"))
        root = self.config_location.parent
        for node, key in ((self.model_config.dataset, "gencode_v24"), (self.model_config.model, "checkpoint_path"),
                          (self.model_config.model.cre_tokenizer, "path"), (self.model_config.model.gene_tokenizer, "path")):
            if not os.path.isabs(node[key]):
                node[key] = str(root / node[key])
        if not os.path.isabs(self.vcf_loader_config.fasta_path):
            self.vcf_loader_config.fasta_path = str(root / self.vcf_loader_config.fasta_path)
        self.gene_cre_manifest = gene_cre_manifest
        self.indel_policy = indel_policy        # insertions / deletions in the consensus: see utils/data_process.py
        if require_gpu:
            assert torch.cuda.is_available(), "GPU is not available"          # reference :60
        self.accelerator = "gpu"

    def create_vcf_from_variant(self, variant_df: pd.DataFrame, output_path: str, vcf_path: str = None):
        """Write (or merge into a copy of `vcf_path`) a single-sample VCF from rows chrom, pos, ref, alt, GT after
        checking every REF against the genome (reference :62-219, which shells out to samtools / bgzip / tabix /
        bcftools sort + concat -a -D).  Output is gzip text sorted by contig order of first appearance and position;
        a record already present (same chrom, pos, ref, alt) is kept once, the existing file's line first.  No
        tabix index is written: the in-process reader does not need one."""
        from ..utils.data_process import open_fasta
        for col in ("chrom", "pos", "ref", "alt", "GT"):
            assert col in variant_df.columns, f"{col} column is required"
        if len(variant_df) == 0:
            raise ValueError("variant_df is empty")
        fasta = open_fasta(self.vcf_loader_config.fasta_path)
        for _, row in variant_df.iterrows():
            pos, ref = int(row["pos"]), row["ref"]
            try:
                found = fasta.fetch(row["chrom"], pos - 1, pos - 1 + len(ref)).upper()
            except KeyError as e:
                raise ValueError(f"Failed to extract reference at {row['chrom']}:{pos}-{pos + len(ref) - 1}: {e}")
            if found != ref.upper():
                raise ValueError(f"Reference mismatch at {row['chrom']}:{pos}: expected '{ref}' but found '{found}' "
                                 f"in reference genome")
        sample, header, body = "SAMPLE", None, []
        if vcf_path is not None:
            opener = gzip.open if open(vcf_path, "rb").read(2) == b"\x1f\x8b" else open
            with opener(vcf_path, "rt") as f:
                lines = f.read().splitlines()
            header = [ln for ln in lines if ln.startswith("#")]
            body = [ln for ln in lines if ln and not ln.startswith("#")]
            names = header[-1].split("\t")[9:]
            assert len(names) == 1, "merging needs a single-sample VCF"
            sample = names[0]
        if header is None:
            header = ["##fileformat=VCFv4.2", f"##reference={self.vcf_loader_config.fasta_path}"]
            header += [f"##contig=<ID={c}>" for c in sorted(variant_df["chrom"].unique())]
            header += ['##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
                       f"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t{sample}"]
        new = [f"{r['chrom']}\t{int(r['pos'])}\t.\t{r['ref']}\t{r['alt']}\t.\tPASS\t.\tGT\t{r['GT']}"
               for _, r in variant_df.sort_values(by=["chrom", "pos"]).iterrows()]
        order, seen, records = {}, set(), []
        for ln in body + new:
            f = ln.split("\t", 5)
            key = (f[0], int(f[1]), f[3], f[4])
            if key in seen:
                continue
            seen.add(key)
            order.setdefault(f[0], len(order))
            records.append((order[f[0]], int(f[1]), len(records), ln))
        records.sort()
        final_path = output_path if output_path.endswith(".vcf.gz") else f"{output_path}.vcf.gz"
        Path(final_path).parent.mkdir(parents=True, exist_ok=True)
        with gzip.open(final_path, "wt") as f:
            f.write("\n".join(header + [r[3] for r in records]) + "\n")
        return final_path

    def get_tissues(self):
        return self.tissue_vocab.keys()

    def get_genes(self):
        return pd.read_csv(self.model_config.dataset.gencode_v24)

    def create_data(self, vcf_path, query_df: pd.DataFrame, dataset_factory=None, **kwargs):
        cfg = Config(dict(self.vcf_loader_config.dataloader))
        cfg.update(kwargs)
        if dataset_factory is None:
            if self.gene_cre_manifest is None:
                raise ValueError("VCFProcessor needs gene_cre_manifest (get_file_path(gene_id) -> per-gene cCRE CSV) to "
                                 "build samples from a VCF; the reference resolves it from S3 (utils/assets.py:307-368)")
            d = self.model_config.dataset
            dataset = VCFDataset(max_length=d.max_length, max_chunks=d.max_chunks, cre_neighbour_hood=d.cre_neighbour_hood,
                                 gencode_v24=d.gencode_v24, gene_cre_manifest=self.gene_cre_manifest,
                                 gene_upstream_neighbour_hood=d.gene_upstream_neighbour_hood,
                                 gene_downstream_neighbour_hood=d.gene_downstream_neighbour_hood, query_df=query_df,
                                 fasta_path=self.vcf_loader_config.fasta_path, vcf_path=vcf_path,
                                 indel_policy=self.indel_policy)
        else:
            dataset = dataset_factory(vcf_path=vcf_path, query_df=query_df, tissue_vocab=self.tissue_vocab,
                                      dataset_config=self.model_config.dataset)
        if cfg.get("num_workers", 0) == 0:
            cfg.pop("prefetch_factor", None)
        return dataset, DataLoader(dataset, collate_fn=collate_fn_batching, **cfg)

    def load_model(self):
        model, checkpoint_path = ModelManager(self.model_config.model).load_model()
        trainer = Trainer(accelerator=self.accelerator, devices=1, logger=False,
                          precision=self.model_config.model.precision, enable_checkpointing=False)
        return model, checkpoint_path, trainer

    def predict(self, model, checkpoint_path, trainer, dataloader, vcf_dataset):
        predictions = trainer.predict(model, dataloader, ckpt_path=checkpoint_path)
        return self.format_output(vcf_dataset.query_df, predictions)

    def predict_with_attention(self, model, checkpoint_path, trainer, dataloader, vcf_dataset, layers=None, per_head=False,
                               gene_body=False, contributions=False, gene_contributions=False, top_k=None):
        """`predict`'s frame plus the gene -> cCRE attention maps of the same forwards (no reference counterpart: flash-attn
        returns no probabilities).  New columns, one entry per gene:
          cre_attention         fp32 [len(layers), tissues, cCREs] (per_head: [len(layers), tissues, heads, cCREs]) -- how much the
                                registry token of each requested tissue attends to each of the gene's cCRE windows in gene
                                layer layers[k]; tissues in the order of the query, cCREs in the order of cre_names;
          cre_attention_layers  the gene-layer indices (layers=None: all; negative: from the end);
          cre_names, cre_start, cre_end   the manifest rows of the windows, where the dataset can name them (cre_table).
        gene_body=True adds
          gene_attention        fp32 [len(layers), tissues, 1 + chunks] (per_head: [len(layers), tissues, heads, 1 + chunks]) -- the
                                same registry tokens' self attention over their own sequence: column 0 the token itself, column
                                1 + c gene-body chunk c;
          gene_chunk_seq_start, gene_chunk_seq_end, gene_chunk_start, gene_chunk_end   where each chunk lies in the encoded
                                consensus sequence and (SNPs only, else null) on the genome, where the dataset can say
                                (gene_chunk_table).
        contributions=True adds
          cre_contribution      fp32, shaped and ordered like cre_attention -- the norm of what each cCRE window adds to the
                                registry token through the cross attention's output projection (value-weighted: a window with
                                a large weight and a value near zero moves the token less than its weight suggests); the
                                quantity to rank cCREs by.
        gene_contributions=True adds (with or without gene_body)
          gene_contribution     fp32, shaped and ordered like gene_attention -- the same norm through the SELF attention's output
                                projection: column 0 is what the registry token's own value adds, column 1 + c what gene-body
                                chunk c (gene_chunk_table) adds; the quantity to rank chunks by, comparable with cre_contribution.
        top_k=K (1 .. 64) returns rankings instead of maps: the selection runs on the device behind each forward and only K
        values and K indices per row are read back.  In place of every map column above the frame holds
          <name>_top_value      fp32 [len(layers), tissues, K] (per_head: [len(layers), tissues, heads, K]) -- the K largest
                                entries of each row of the map, descending;
          <name>_top_index      int32, the same shape -- their columns in the full map (a row of cre_names / 1 + a row of
                                gene_chunk_table; 0 in a gene-body map is the token itself), -1 where the gene has fewer than K;
          cre_attention_top_names, cre_contribution_top_names   the cre_name of every index (None for -1), where the dataset
                                has cre_table.
        A plain loop over the loader (the maps or the rankings are read back per batch)."""
        model.trainer = trainer
        model.eval()
        kw = {"gene_body": True} if gene_body else {}
        if contributions:
            kw["contributions"] = True
        if gene_contributions:
            kw["gene_contributions"] = True
        if top_k is not None:
            kw["top_k"] = top_k
        predictions = [model.predict_step_with_attention(batch, i, layers=layers, per_head=per_head, **kw)
                       for i, batch in enumerate(dataloader)]
        try:       # as Trainer.predict: what the self-healing LayerNorm fold did during this pass
            from ..seq2gene.model_combined_modulator import ln_fold_state
            trainer.ln_fold_state = ln_fold_state(model)
        except Exception:                                     # a model class without the fold
            trainer.ln_fold_state = None
        df = self.format_output(vcf_dataset.query_df, predictions)
        suffixes = ("",) if top_k is None else ("_top_value", "_top_index")

        def column(key):
            for sfx in suffixes:
                df[key + sfx] = pd.Series([m for p in predictions for m in p[key + sfx]], index=df.index, dtype=object)

        def widths(kind):                                            # the gene's columns in the full map, from the prediction
            if top_k is not None:
                return [w for p in predictions for w in p[kind + "_map_width"]]
            key = {"cre": "cre_attention", "gene": "gene_attention" if gene_body else "gene_contribution"}[kind]
            return [m.shape[-1] for p in predictions for m in p[key]]
        column("cre_attention")
        df["cre_attention_layers"] = pd.Series([list(p["cre_attention_layers"]) for p in predictions for _ in p["pred_gene_exp"]],
                                               index=df.index, dtype=object)
        if hasattr(vcf_dataset, "cre_table"):
            tables = [vcf_dataset.cre_table(g) for g in df["gene_id"]]
            for g, t, w in zip(df["gene_id"], tables, widths("cre")):     # a name per map column, or no names at all
                assert len(t) == w, f"{g}: cre_table names {len(t)} windows, the map has {w} columns"
            for col, src in (("cre_names", "cre_name"), ("cre_start", "start_cre"), ("cre_end", "end_cre")):
                df[col] = pd.Series([t[src].tolist() for t in tables], index=df.index, dtype=object)
            if top_k is not None:
                for key in ("cre_attention",) + (("cre_contribution",) if contributions else ()):
                    idx = [m for p in predictions for m in p[key + "_top_index"]]
                    names = []
                    for t, ix in zip(tables, idx):
                        lut = np.array(t["cre_name"].tolist() + [None], dtype=object)       # -1 finds the None at the end
                        names.append(lut[ix])
                    df[key + "_top_names"] = pd.Series(names, index=df.index, dtype=object)
        if contributions:
            column("cre_contribution")
        if gene_body or gene_contributions:
            for key, on in (("gene_attention", gene_body), ("gene_contribution", gene_contributions)):
                if on:
                    column(key)
            if hasattr(vcf_dataset, "gene_chunk_table"):
                tables = [vcf_dataset.gene_chunk_table(g) for g in df["gene_id"]]
                for g, t, w in zip(df["gene_id"], tables, widths("gene")):    # a row per map column behind the registry token's
                    assert len(t) == w - 1, f"{g}: gene_chunk_table has {len(t)} chunks, the map {w - 1}"
                for col, src in (("gene_chunk_seq_start", "seq_start"), ("gene_chunk_seq_end", "seq_end"),
                                 ("gene_chunk_start", "start"), ("gene_chunk_end", "end")):
                    df[col] = pd.Series([[None if pd.isna(v) else int(v) for v in t[src]] for t in tables], index=df.index,
                                        dtype=object)
        return df

    def predict_cre_activity(self, tokenizer, dataloader, vcf_dataset, tissues=None):
        """What the cCRE tokenizer takes each of a gene's cCRE windows to BE in each of its tissues, for this individual's
        sequence: the class probabilities of the tokenizer's per-tissue classifier heads.  `tokenizer` is
        ModelManager.load_tokenizer("cre") -- the pretrained pair of encoder and heads, not the tokenizer inside the expression
        model, whose encoder was fine-tuned away from its heads.  `tissues`: head indices (default: all).  Returns the query
        frame with, one entry per gene:
          cre_class_probabilities   fp32 [cCREs, len(tissues), classes];
          cre_class                 int [cCREs, len(tissues)]: the most probable class (-1 where a logit is NaN);
          cre_activity_tissues      the heads' names (the tokenizer's `tissues` hyper-parameter) where it has them, else their
                                    indices, in the order of axis 1;
          cre_class_names           the names of the classes (utils.constants.CREs when the heads have that many), else indices;
          cre_names, cre_start, cre_end   the manifest rows of the windows, where the dataset can name them (cre_table).
        A plain loop over the loader; the window's reference label is the context of a use_context tokenizer and unused
        otherwise."""
        tokenizer.eval()
        n_heads = len(tokenizer.tissue_classifiers)
        sel = list(range(n_heads)) if tissues is None else [int(t) for t in tissues]
        probs, classes = [], []
        with torch.no_grad():
            for batch in dataloader:
                for i, ids in enumerate(batch["cre_sequences"]):
                    p, c = tokenizer.classify(ids, batch["cre_attention_masks"][i], context=batch["ref_cre_labels"][i],
                                              tissues=None if tissues is None else sel, probabilities=True)
                    probs.append(p.cpu().numpy())
                    classes.append(c.cpu().numpy())
        df = vcf_dataset.query_df
        assert len(df) == len(probs), "DataFrame and predictions length mismatch"
        df["cre_class_probabilities"] = pd.Series(probs, index=df.index, dtype=object)
        df["cre_class"] = pd.Series(classes, index=df.index, dtype=object)
        names = getattr(tokenizer, "tissues", None)
        head_names = [names[t] for t in sel] if names is not None and len(names) == n_heads else list(sel)
        df["cre_activity_tissues"] = pd.Series([list(head_names) for _ in probs], index=df.index, dtype=object)
        class_names = cre_class_names(tokenizer.num_classes)
        df["cre_class_names"] = pd.Series([list(class_names) for _ in probs], index=df.index, dtype=object)
        if hasattr(vcf_dataset, "cre_table"):
            tables = [vcf_dataset.cre_table(g) for g in df["gene_id"]]
            for g, t, p in zip(df["gene_id"], tables, probs):           # a name per window, or no names at all
                assert len(t) == p.shape[0], f"{g}: cre_table names {len(t)} windows, {p.shape[0]} were classified"
            for col, src in (("cre_names", "cre_name"), ("cre_start", "start_cre"), ("cre_end", "end_cre")):
                df[col] = pd.Series([t[src].tolist() for t in tables], index=df.index, dtype=object)
        return df

    def expression_neighbors(self, df, k: int = 30, on: str = "predicted_expression", axis: str = "genes", tissue=None,
                             metric: str = "correlation"):
        """The correlation k-nearest neighbours among the rows of a finished prediction: `df` is what
        format_output returned; the matrix is neighbors.from_predictions(df, on, axis, tissue) and the search runs on the
        device (neighbors.knn: rows standardised in fp32, similarities on the f32 MFMA, no rows x rows buffer).  No model and
        no checkpoint are involved.  Per row of the matrix:
          neighbor_ids         the labels of its k nearest rows, nearest first (None where the matrix has fewer than k others);
          neighbor_distance    fp32 [k], 1 - correlation, ascending (+Inf beside a None);
          neighbor_degenerate  True for a row without variation (its norm is 0): it is at distance 1 from everything.
        Rows that are genes (axis="genes" with expression, or embeddings of one `tissue`) get these as three columns of `df`,
        which is returned.  Embeddings with tissue=None have (gene, tissue) rows: each gene's cell then holds its tissues'
        results, [tissues, k] / [tissues].  axis="tissues" has no gene rows: a new frame is returned, one row per tissue
        under the column `tissue`."""
        from .. import neighbors
        m, labels = neighbors.from_predictions(df, on=on, axis=axis, tissue=tissue)
        idx, dist, norm = neighbors._knn(m, k, metric, None, False, False)
        idx, dist, flat = idx.cpu().numpy(), dist.cpu().numpy(), (norm == 0).cpu().numpy()
        lut = np.empty(len(labels) + 1, dtype=object)                    # -1 finds the None at the end
        for i, label in enumerate(labels):                               # one by one: a (gene, tissue) label stays one object
            lut[i] = label
        lut[len(labels)] = None
        ids = lut[idx]
        if axis == "tissues":
            return pd.DataFrame({"tissue": labels, "neighbor_ids": list(ids), "neighbor_distance": list(dist),
                                 "neighbor_degenerate": flat})
        per = len(labels) // len(df)                                     # 1, or the tissues of a (gene, tissue) row set
        if per > 1:
            ids, dist, flat = ids.reshape(len(df), per, -1), dist.reshape(len(df), per, -1), flat.reshape(len(df), per)
        df["neighbor_ids"] = pd.Series(list(ids), index=df.index, dtype=object)
        df["neighbor_distance"] = pd.Series(list(dist), index=df.index, dtype=object)
        df["neighbor_degenerate"] = pd.Series(list(flat), index=df.index, dtype=object if per > 1 else bool)
        return df

    def expression_dendrogram(self, df, on: str = "predicted_expression", axis: str = "tissues", tissue=None):
        """The Ward tree over the rows of a finished prediction, what vcf2exp's compute_ordered_leaves
        computes with scipy: `df` is what format_output returned; the matrix is neighbors.from_predictions(df, on, axis, tissue),
        its correlation distances and their linkage are formed on the device (linkage.ward_of_rows).  axis="tissues" is the
        notebook's tissue dendrogram, axis="genes" the row order of its heatmap.  No model and no checkpoint are involved.
        Returns a dict:
          Z               float64 [rows - 1, 4], scipy's linkage format (scipy.cluster.hierarchy.dendrogram takes it);
          leaves          int32 [rows], the rows from left to right;
          labels          what names each row of the matrix;  ordered_labels  the labels in `leaves` order."""
        from .. import linkage, neighbors
        m, labels = neighbors.from_predictions(df, on=on, axis=axis, tissue=tissue)
        Z = linkage.ward_of_rows(m)
        leaves = linkage.leaves_list(Z)
        return {"Z": Z, "leaves": leaves, "labels": labels, "ordered_labels": [labels[i] for i in leaves]}

    def expression_umap(self, df, on: str = "predicted_expression", axis: str = "genes", tissue=None, return_model: bool = False,
                        **umap_kwargs):
        """The UMAP picture of a finished prediction, what the reference's vcf2embed notebook draws with
        umap-learn: `df` is what format_output returned; the matrix is neighbors.from_predictions(df, on, axis, tissue) and the
        k-NN graph, the fuzzy simplicial set and the layout run on the device (manifold.umap, which takes `umap_kwargs`:
        n_neighbors=30, min_dist=0.1, metric="correlation", n_components=2, n_epochs, init="pca", seed=42, ...; init=manifold.spectral_init
        starts from the eigenvectors of the fuzzy graph's normalised Laplacian, umap-learn's default, DESIGN.md section 5i;
        init=manifold.spectral_init_components keeps that start where separated clusters disconnect the graph, section 5k).  No
        model and no checkpoint are involved.  Returns a dict:
          coords   fp32 [rows, n_components], one row per row of the matrix;
          labels   what names each row of the matrix.
        Rows that are genes (axis="genes" with expression, or embeddings of one `tissue`) also get the columns umap_1 ..
        umap_n of `df`, one number per gene.  Embeddings with tissue=None have (gene, tissue) rows: each gene's cell then holds
        its tissues' coordinates, fp32 [tissues].  axis="tissues" has no gene rows and adds no column.
        return_model=True adds `model`, the manifold.UMAPModel of the fit (the same embedding, bit for bit), which
        expression_umap_transform takes to place a second prediction in these coordinates."""
        from .. import manifold, neighbors
        m, labels = neighbors.from_predictions(df, on=on, axis=axis, tissue=tissue)
        model = manifold.fit(m, **umap_kwargs) if return_model else None
        coords = model.embedding if return_model else manifold.umap(m, **umap_kwargs)
        self._umap_columns(df, coords, labels, axis)
        return {"coords": coords, "labels": labels, "model": model} if return_model else {"coords": coords, "labels": labels}

    def expression_tsne(self, df, on: str = "predicted_expression", axis: str = "genes", tissue=None, **tsne_kwargs):
        """The t-SNE picture of a finished prediction, the first of the "alternative methods" the
        reference's vcf2embed notebook lists as next steps: the twin of expression_umap.  `df` is what format_output returned;
        the matrix is neighbors.from_predictions(df, on, axis, tissue), and the neighbour lists, the perplexity search and the
        descent with the exact all-pairs gradient run on the device (manifold.tsne, which takes `tsne_kwargs`: perplexity=30,
        metric="correlation", n_components=2, n_iter=1000, early_exaggeration=12, exaggeration_iter=250, learning_rate="auto",
        init="pca", seed=42, n_neighbors=None).  No model and no checkpoint are involved.  Returns a dict:
          coords   fp32 [rows, n_components], one row per row of the matrix;
          labels   what names each row of the matrix.
        The columns tsne_1 .. tsne_n are added to `df` under expression_umap's rules."""
        from .. import manifold, neighbors
        if "return_kl" in tsne_kwargs:
            raise ValueError("expression_tsne returns coordinates: ask manifold.tsne(..., return_kl=True) for the divergence")
        m, labels = neighbors.from_predictions(df, on=on, axis=axis, tissue=tissue)
        coords = manifold.tsne(m, **tsne_kwargs)
        self._umap_columns(df, coords, labels, axis, prefix="tsne")
        return {"coords": coords, "labels": labels}

    def expression_enrichment(self, df, annotations, labels=None, n_clusters=None, on: str = "predicted_expression", axis: str = "genes",
                              tissue=None, **enrich_kwargs):
        """Which annotation terms are over-represented in which cluster of genes: the "pathway enrichment"
        the reference's vcf2embed notebook lists as a next step, over its gene -> GO term lists.  `df` is what format_output
        returned; its genes are the universe.  `annotations` is a dict or a two-column frame, gene id -> list of terms.  `labels`
        says how the genes are clustered:
          a column name of `df`   its values, numbered in sorted order (a column of integers is taken as it is, negative = none);
          an array                one integer per gene, 0 .. k - 1, any other value = in no cluster;
          "max_tissue"            every gene's tissue of highest predicted expression (the notebook's Step 6);
          None                    the Ward tree of the matrix neighbors.from_predictions(df, on, axis, tissue), cut into
                                  `n_clusters` (linkage.ward_of_rows on the device, linkage.cut on the host).
        The overlap counts and the hypergeometric tests run on the device (enrichment.enrich, which takes `enrich_kwargs`:
        fdr=0.05, alternative="greater", min_size=5, max_size=500).  No model and no checkpoint are involved.  Adds the column
        `enrichment_cluster` to `df` (the cluster's name: a number, a value of the column, a tissue) and returns enrich's dict,
        with `cluster_names` and the tidy `frame` of significant (cluster, term) rows."""
        from .. import enrichment, linkage, neighbors
        if axis != "genes":
            raise ValueError("enrichment tests clusters of genes: axis must be 'genes'")
        for key in ("universe", "cluster_names", "n_clusters"):
            if key in enrich_kwargs:
                raise ValueError(f"expression_enrichment sets {key} itself")
        if "gene_id" not in df.columns or len(df) == 0:
            raise ValueError("the frame has no `gene_id` column or no rows: pass what format_output returned")
        genes = list(df["gene_id"])
        names = None
        if labels is None:
            if n_clusters is None:
                raise ValueError("labels=None cuts the Ward tree of the genes: say into how many with n_clusters")
            m, rows = neighbors.from_predictions(df, on=on, axis=axis, tissue=tissue)
            if len(rows) != len(genes):
                raise ValueError("embeddings of every tissue have (gene, tissue) rows: choose one `tissue` to cluster genes")
            if isinstance(n_clusters, bool) or not isinstance(n_clusters, (int, np.integer)) or not 1 <= n_clusters <= min(len(genes), enrichment.MAX_K):
                raise ValueError(f"n_clusters must be an integer in 1 .. {min(len(genes), enrichment.MAX_K)}, not {n_clusters!r}")
            lab = linkage.cut(linkage.ward_of_rows(m), int(n_clusters))
            k = int(n_clusters)
        elif isinstance(labels, str) and labels == "max_tissue":
            m, _ = neighbors.from_predictions(df, on="predicted_expression", axis="genes")
            lab = np.argmax(m, axis=1).astype(np.int32)
            names = list(neighbors._tissue_names(df))
            k = len(names)
        elif isinstance(labels, str):
            if labels not in df.columns:
                raise ValueError(f"labels={labels!r} is neither a column of the frame nor 'max_tissue'")
            values = df[labels].to_numpy()
            if values.dtype != np.bool_ and np.issubdtype(values.dtype, np.integer):
                lab, k = values.astype(np.int64), n_clusters
            else:
                missing = pd.isna(values)
                names = sorted(set(values[~missing].tolist()))
                lut = {v: i for i, v in enumerate(names)}
                lab = np.array([-1 if miss else lut[v] for v, miss in zip(values.tolist(), missing)], dtype=np.int32)
                k = len(names)
        else:
            lab, k = (np.asarray(labels) if isinstance(labels, (list, tuple)) else labels), n_clusters
        out =enrichment.enrich(lab, annotations, genes, n_clusters=k, cluster_names=names, **enrich_kwargs)
        k = out["cluster_size"].shape[0]
        lab = np.asarray(lab.cpu() if isinstance(lab, torch.Tensor) else lab)
        inside = (lab >= 0) & (lab < k)
        shown = np.arange(k) if names is None else np.array(list(names), dtype=object)
        column = np.where(inside, shown[np.where(inside, lab, 0)], -1 if names is None else None)
        df["enrichment_cluster"] = pd.Series(column if names is not None else column.astype(np.int64), index=df.index,
                                             dtype=object if names is not None else np.int64)
        out["cluster_names"] = list(shown)
        out["labels"] = lab.astype(np.int32)
        return out

    @staticmethod
    def _kmeans_matrix(df, on, axis, tissue):
        """(matrix, labels, metric forced or None) of expression_kmeans: a from_predictions matrix, or the frame's own umap_1 ..
        / tsne_1 .. columns."""
        import re
        from .. import neighbors
        if on in ("umap", "tsne"):
            if axis != "genes" or tissue is not None:
                raise ValueError(f"on={on!r} clusters the frame's {on}_1 .. columns: one row per gene, no tissue")
            cols = sorted((c for c in df.columns if isinstance(c, str) and re.fullmatch(rf"{on}_[1-9]\d*", c)), key=lambda c: int(c.split("_")[1]))
            if not cols or "gene_id" not in df.columns or len(df) == 0:
                raise ValueError(f"the frame has no {on}_1 .. columns (run expression_{on} first), no `gene_id` column or no rows")
            try:
                m = np.ascontiguousarray(df[cols].to_numpy(dtype=np.float32))
            except (TypeError, ValueError) as e:
                raise ValueError(f"the {on}_1 .. columns hold one array per gene ((gene, tissue) rows): they cannot be clustered as genes") from e
            return m, list(df["gene_id"]), "euclidean"
        m, labels = neighbors.from_predictions(df, on=on, axis=axis, tissue=tissue)
        return m, labels, None

    def expression_kmeans(self, df, n_clusters, on: str = "predicted_expression", axis: str = "genes", tissue=None, **kmeans_kwargs):
        """Flat clusters of a finished prediction: the k-means the vcf2embed notebook's "GO term enrichment
        within UMAP clusters" needs.  `df` is what format_output returned.  on="predicted_expression" / "embeddings" cluster the
        matrix neighbors.from_predictions(df, on, axis, tissue); on="umap" / "tsne" cluster the frame's umap_1 .. / tsne_1 ..
        columns with metric="euclidean".  Lloyd's loop and the seeding run on the device (kmeans.kmeans, which takes
        `kmeans_kwargs`: metric="correlation", init="k-means++", n_init=1, max_iter=300, tol=1e-4, seed=0).  No model and no
        checkpoint are involved.  Returns a dict: labels int32 [rows], centers fp32 [k, columns], inertia, n_iter, and `model`, the
        kmeans.KMeansModel that expression_kmeans_assign takes.  Where the rows are genes the integer column `kmeans_cluster` is
        added to `df`: expression_enrichment(df, annotations, labels="kmeans_cluster", n_clusters=k) takes it as it is."""
        from .. import kmeans
        m, labels, metric = self._kmeans_matrix(df, on, axis, tissue)
        if metric is not None:
            if kmeans_kwargs.get("metric", metric) != metric:
                raise ValueError(f"on={on!r} clusters coordinates: metric must be {metric!r}")
            kmeans_kwargs["metric"] = metric
        model = kmeans.kmeans(m, n_clusters, **kmeans_kwargs)
        if axis == "genes" and len(labels) == len(df):
            df["kmeans_cluster"] = pd.Series(np.asarray(model.labels, dtype=np.int64), index=df.index, dtype=np.int64)
        return {"labels": model.labels, "centers": model.centers, "inertia": model.inertia, "n_iter": model.n_iter, "model": model,
                "row_labels": labels}

    def expression_kmeans_assign(self, model, df, on: str = "predicted_expression", axis: str = "genes", tissue=None):
        """The clusters of a first prediction for the rows of a second: `model` is what expression_kmeans
        returned under "model", `df` what format_output returned for another individual (with its umap_1 .. columns from
        expression_umap_transform for on="umap").  Every row gets its nearest fitted centre (model.predict: an assignment alone).
        Returns {"labels": int32 [rows], "distance": fp32 [rows], "row_labels"} and adds the column `kmeans_cluster` to `df`
        under expression_kmeans's rule."""
        from .. import kmeans
        if not isinstance(model, kmeans.KMeansModel):
            raise TypeError(f"model must be a kmeans.KMeansModel (expression_kmeans(...)['model']), not {type(model).__name__}")
        m, labels, metric = self._kmeans_matrix(df, on, axis, tissue)
        if metric is not None and model.metric != metric:
            raise ValueError(f"on={on!r} assigns coordinates: the model was fitted with metric={model.metric!r}")
        if m.shape[1] != model.columns:
            raise ValueError(f"the frame's matrix has {m.shape[1]} columns, the model was fitted on {model.columns}")
        lab, dist = model.predict(m, return_distance=True)
        if axis == "genes" and len(labels) == len(df):
            df["kmeans_cluster"] = pd.Series(np.asarray(lab, dtype=np.int64), index=df.index, dtype=np.int64)
        return {"labels": lab, "distance": dist, "row_labels": labels}

    def expression_silhouette(self, df, labels="kmeans_cluster", on: str = "predicted_expression", axis: str = "genes", tissue=None,
                              metric=None, standardize=None, max_bytes=None):
        """How well a flat clustering of a finished prediction separates: the silhouette coefficient,
        scikit-learn's silhouette_samples, on the device (validation.silhouette_samples).  `df` is what format_output returned;
        the matrix is expression_kmeans's: neighbors.from_predictions(df, on, axis, tissue), or the frame's umap_1 .. / tsne_1 ..
        columns for on="umap" / "tsne".  `labels` names a column of `df` (the default is expression_kmeans's `kmeans_cluster`;
        `enrichment_cluster` and any column of one's own serve too) or is an array with one label per row of the matrix; a
        negative label is no label.  metric: "correlation" (the default for a matrix; linear in the rows), "cosine" or
        "euclidean" (the default, and the only one, for coordinates); standardize as in validation.silhouette_samples.  Where the
        rows are genes the columns `silhouette` (NaN for a gene without a label) and `silhouette_neighbor_cluster` (the label of
        the nearest other cluster: where the gene would go next) are added to `df`.  Returns the score, the mean over the
        labelled rows."""
        from .. import validation
        m, row_labels, forced = self._kmeans_matrix(df, on, axis, tissue)
        if forced is not None and metric not in (None, forced):
            raise ValueError(f"on={on!r} scores coordinates: metric must be {forced!r}")
        metric = forced or metric or "correlation"
        if isinstance(labels, str):
            if labels not in df.columns:
                raise ValueError(f"the frame has no `{labels}` column: run expression_kmeans first, or pass the labels themselves")
            if len(row_labels) != len(df):
                raise ValueError(f"the column `{labels}` has one label per gene, the matrix has {len(row_labels)} rows: pass an array")
            labels = df[labels].to_numpy()
        kwargs = {} if max_bytes is None else {"max_bytes": max_bytes}
        res = validation.silhouette_samples(m, labels, metric=metric, standardize=standardize, **kwargs)
        if axis == "genes" and len(row_labels) == len(df):
            df["silhouette"] = pd.Series(np.asarray(res.samples, dtype=np.float64), index=df.index, dtype=np.float64)
            df["silhouette_neighbor_cluster"] = pd.Series(res.nearest, index=df.index)
        return res.score

    def expression_silhouette_sweep(self, df, ks, method: str = "kmeans", on: str = "predicted_expression", axis: str = "genes", tissue=None,
                                    metric=None, **kwargs):
        """Which number of clusters?  Clusters the matrix of expression_silhouette at every k of `ks`
        (validation.silhouette_sweep: method="kmeans", which takes kmeans.kmeans's `kwargs`, or method="ward", one tree cut once
        per k) and scores each clustering by its silhouette.  Returns a small frame, one row per k: `k`, `silhouette_score` and,
        for k-means, `inertia`; frame.attrs["best_k"] is the k of the largest score and frame.attrs["labels"] maps every k to its
        int32 labels."""
        from .. import validation
        m, _, forced = self._kmeans_matrix(df, on, axis, tissue)
        if forced is not None and metric not in (None, forced):
            raise ValueError(f"on={on!r} scores coordinates: metric must be {forced!r}")
        res = validation.silhouette_sweep(m, ks, method=method, metric=forced or metric or "correlation", **kwargs)
        out = pd.DataFrame({"k": np.asarray(res.ks, dtype=np.int64), "silhouette_score": np.asarray(res.scores, dtype=np.float64)})
        if res.inertia is not None:
            out["inertia"] = np.asarray(res.inertia, dtype=np.float64)
        out.attrs["best_k"] = res.best_k
        out.attrs["labels"] = dict(zip(res.ks, res.labels))
        return out

    @staticmethod
    def _umap_columns(df, coords, labels, axis, prefix: str = "umap"):
        if axis != "tissues":
            per = len(labels) // len(df)                                 # 1, or the tissues of a (gene, tissue) row set
            for c in range(coords.shape[1]):
                column = coords[:, c] if per == 1 else list(coords[:, c].reshape(len(df), per))
                df[f"{prefix}_{c + 1}"] = pd.Series(column, index=df.index, dtype=np.float32 if per == 1 else object)

    def expression_umap_transform(self, model, df, on: str = "predicted_expression", axis: str = "genes", tissue=None, n_epochs=None):
        """A second prediction in the coordinates of a first: `model` is what
        expression_umap(first, ..., return_model=True) returned under "model" (or any manifold.UMAPModel), `df` what format_output
        returned for another individual, cohort or set of alleles.  The matrix is neighbors.from_predictions(df, on, axis, tissue),
        as in expression_umap, and must have the model's column count (the same tissues, or the same embedding width): another
        count is refused with both stated.  Every row is placed by model.transform(matrix, n_epochs) among the first frame's
        points, which do not move, so the two pictures can be compared.  Returns {"coords": fp32 [rows, n_components],
        "labels"} and adds the columns umap_1 .. umap_n to `df` under expression_umap's rules."""
        from .. import manifold, neighbors
        if not isinstance(model, manifold.UMAPModel):
            raise TypeError(f"model must be a manifold.UMAPModel (expression_umap(..., return_model=True)['model']), not {type(model).__name__}")
        m, labels = neighbors.from_predictions(df, on=on, axis=axis, tissue=tissue)
        if m.shape[1] != model.columns:
            raise ValueError(f"the frame's matrix has {m.shape[1]} columns, the model was fitted on {model.columns}: the two predictions "
                             f"must cover the same tissues (or embedding width)")
        coords = model.transform(m, n_epochs=n_epochs)
        self._umap_columns(df, coords, labels, axis)
        return {"coords": coords, "labels": labels}

    def predict_distributed(self, model, checkpoint_path, trainer, vcf_dataset, batch_size: int | None = None, costs=None,
                            **loader_kwargs):
        """Multi-GPU vcf2exp (the reference is single-device, vcfprocessor.py:252-258): call from every rank
        of a torch.distributed job (one process per GPU, launched with `python -m torch.distributed.run` BEFORE anything
        touches the GPU; scripts/vcf2exp_dist.py shows the launcher).  The rows of `vcf_dataset.query_df` are dealt to
        the ranks by LPT on `costs` (default: `vcf_dataset.gene_costs()` when the dataset offers it, else equal),
        every rank runs the single-GPU path over its rows, and one padded all-gather per output (RCCL over xGMI)
        returns the complete frame, in query order, on every rank."""
        from ..dist import predict_sharded
        model.trainer = trainer
        model.eval()
        if costs is None and hasattr(vcf_dataset, "gene_costs"):
            costs = vcf_dataset.gene_costs()
        bs = batch_size or int(self.vcf_loader_config.dataloader.get("batch_size", 8))

        def run(batch, i):
            with torch.no_grad():
                return model.predict_step(batch, i)
        results, busy = predict_sharded(run, vcf_dataset, collate_fn_batching, costs=costs, batch_size=bs,
                                        device=model.device, loader_kwargs=loader_kwargs)
        self.last_busy_seconds = busy
        return self.format_output(vcf_dataset.query_df, [results])

    def format_output(self, df, predictions):
        pred_exp, embd = [], []
        for p in predictions:
            pred_exp.extend(p["pred_gene_exp"])
            embd.extend(p["embeddings"])
        pred_df = pd.DataFrame({"predicted_expression": pred_exp, "embeddings": embd})
        assert len(df) == len(pred_df), "DataFrame and predictions length mismatch"
        df["predicted_expression"] = pred_df["predicted_expression"]
        df["embeddings"] = pred_df["embeddings"]
        return df

"""ADrisk / ADriskFromVCF: the vcf2risk API surface (reference processors/ad_risk.py) over the HIP forest evaluator.

Each (gene, tissue) pair has one forest on the registry-token embedding; the result is its second output, the reference's
predict_proba[:, 1].  Kept: the class names, constructor and call signatures, the asserts and the returned types.  The
reference deserialises a treelite model and predicts per DataFrame row on the host; here the distinct forests of a query are
packed into one forest.ForestBank and every row goes through its own in ONE launch (ops.forest_predict, row form), and
ADrisk.__call__ sends a cohort through one forest (cohort form).

`predictors` stands where the reference resolves files from S3 (utils/assets.py GeneTissueManifestLookup): anything with
get_file_path(gene_id, tissue_id) -> str | None, or a directory, read by LocalPredictorStore.  The files are what forest.load
reads: `.npz` (packed), `.json` (a treelite dump) or, where treelite is installed, `.tl` -- the last two unpinned, see
forest.py."""
from __future__ import annotations

import os
from typing import List

import numpy as np
import pandas as pd
import torch

from .. import forest as _forest
from .. import ops
from . import vcfprocessor

MODEL_CLASSES = ("v4_ag", "v4_pcg")


def normalize_tissue_id(tissue_id) -> int:
    """7, "7", "model_7" and "tissue_7" all name tissue 7 (the reference's manifest lookup accepts the same spellings)."""
    if isinstance(tissue_id, (int, np.integer)):
        return int(tissue_id)
    s = str(tissue_id)
    for prefix in ("model_", "tissue_"):
        if s.startswith(prefix):
            s = s[len(prefix):]
    return int(s)


class LocalPredictorStore:
    """Predictor files under a directory: root/manifest.csv with the columns gene_id, tissue_id, file_path (relative paths are
    taken from root)."""

    def __init__(self, root: str):
        self.root = str(root)
        table = pd.read_csv(os.path.join(self.root, "manifest.csv"), dtype={"gene_id": str, "file_path": str})
        missing = {"gene_id", "tissue_id", "file_path"} - set(table.columns)
        if missing:
            raise ValueError(f"manifest.csv lacks the columns {sorted(missing)}")
        self._paths = {(g, normalize_tissue_id(t)): p for g, t, p in zip(table["gene_id"], table["tissue_id"], table["file_path"])}

    def exists(self, gene_id: str, tissue_id) -> bool:
        return (gene_id, normalize_tissue_id(tissue_id)) in self._paths

    def get_file_path(self, gene_id: str, tissue_id):
        p = self._paths.get((gene_id, normalize_tissue_id(tissue_id)))
        if p is None:
            return None
        return p if os.path.isabs(p) else os.path.join(self.root, p)


def _store(predictors):
    if predictors is None:
        raise ValueError("the AD-risk predictors need `predictors`: a directory with manifest.csv (LocalPredictorStore) or "
                         "anything with get_file_path(gene_id, tissue_id); the reference resolves them from S3 "
                         "(utils/assets.py GeneTissueManifestLookup)")
    return LocalPredictorStore(predictors) if isinstance(predictors, (str, os.PathLike)) else predictors


def _predictor_path(store, gene_id, tissue_id) -> str:
    path = store.get_file_path(gene_id, tissue_id)
    if path is None:
        raise FileNotFoundError(f"AD predictor not found for gene {gene_id} and tissue {tissue_id}")
    return path


def _check_model(model, what: str):
    if model.n_outputs < 2:
        raise ValueError(f"{what}: the AD risk is a model's second output, and this one has {model.n_outputs}")
    return model


class ADrisk:
    def __init__(self, gene_id: str, tissue_id: int, model_class: str = "v4_pcg", predictors=None):
        assert model_class in MODEL_CLASSES, "model_class should be either 'v4_ag' or 'v4_pcg'"
        assert type(tissue_id) is int, "tissue_id should be an integer"
        assert type(gene_id) is str, "gene_id should be a string"
        self.gene_id, self.tissue_id, self.model_class = gene_id, tissue_id, model_class
        self.gene_tissue_manifest = _store(predictors)
        self.ad_preds = self._load_ad_predictor()

    def _load_ad_predictor(self):
        path = _predictor_path(self.gene_tissue_manifest, self.gene_id, self.tissue_id)
        self.predictor = _check_model(_forest.load(path), path)
        self.bank = _forest.ForestBank([self.predictor])

    def __call__(self, gene_tissue_embeds) -> np.ndarray:
        """gene_tissue_embeds ndarray or tensor [num_samples, embedding_dim] -> ndarray [num_samples]: the AD risk of every
        sample under this (gene, tissue) forest."""
        x = torch.as_tensor(gene_tissue_embeds)
        assert x.dim() == 2 and x.shape[1] == self.bank.n_features, \
            f"embeddings should be [num_samples, {self.bank.n_features}], not {tuple(x.shape)}"
        x = x.to(device="cuda", dtype=torch.float32)
        if x.stride(1) != 1:
            x = x.contiguous()
        out = torch.empty((x.shape[0], self.bank.n_outputs), dtype=torch.float32, device=x.device)
        ops.forest_predict(x, self.bank.to(x.device), model=0, out=out)
        return out[:, 1].contiguous().cpu().numpy()


class ADriskFromVCF:
    def __init__(self, model_class: str = "v4_pcg", predictors=None, config_dir=None, **vcfprocessor_kwargs):
        self.model_class = model_class
        self.ad_preds = _store(predictors)
        self._config_dir, self._vcf_kwargs = config_dir, vcfprocessor_kwargs
        self._models, self._bank = {}, (None, None)
        self._init_model()

    def _init_model(self):
        self.vcf_processor = vcfprocessor.VCFProcessor(model_class=self.model_class, config_dir=self._config_dir, **self._vcf_kwargs)
        vocab = self.vcf_processor.tissue_vocab
        self.tissue_map = pd.DataFrame({"tissue": list(vocab.keys())}, index=pd.Index(list(vocab.values()), name="tissue_id"))
        self.genes_map = self.vcf_processor.get_genes().set_index("gene_id")
        self.model, self.checkpoint_path, self.trainer = self.vcf_processor.load_model()

    def _format_query(self, gene_ids: List[str], tissue_ids: List[int]) -> pd.DataFrame:
        assert len(gene_ids) == len(tissue_ids), "Please map gene ids to tissue ids, there should be 2 lists of the same length"
        for gene_id, tissue_id in zip(gene_ids, tissue_ids):
            assert type(tissue_id) is int, "tissue_id should be an integer"
            assert type(gene_id) is str, "gene_id should be a string"
        return pd.DataFrame({"gene_id": list(gene_ids), "tissues": self.tissue_map.loc[list(tissue_ids), "tissue"].tolist()})

    def _init_dataloader(self, vcf_path: str, gene_ids: List[str], tissue_ids: List[int], dataset_factory=None):
        return self.vcf_processor.create_data(vcf_path, self._format_query(gene_ids, tissue_ids), dataset_factory=dataset_factory)

    def __call__(self, vcf_file: str, gene_ids: List[str], tissue_ids: List[int], dataset_factory=None) -> pd.DataFrame:
        """One row per (gene, tissue) of the query, in query order: gene_id, tissue_id, tissue_name, predicted_expression,
        embedding, ad_risk, gene_name."""
        vcf_dataset, dataloader = self._init_dataloader(vcf_file, gene_ids, tissue_ids, dataset_factory)
        preds_df = self.vcf_processor.predict(self.model, self.checkpoint_path, self.trainer, dataloader, vcf_dataset)
        return self._predict_ad_risk(self._reformat_predictions(preds_df))

    def _reformat_predictions(self, preds_df: pd.DataFrame) -> pd.DataFrame:
        preds_df.rename(columns={"tissues": "tissue_id", "tissue_names": "tissue_name", "embeddings": "embedding"}, inplace=True)
        assert preds_df.tissue_id.apply(lambda ids: len(ids) == 1).all()
        for col in ("tissue_id", "tissue_name"):
            preds_df[col] = preds_df[col].apply(lambda v: v[0])
        preds_df["predicted_expression"] = preds_df["predicted_expression"].apply(lambda v: v[0][0])
        return preds_df

    def _bank_for(self, pairs):
        """The bank of the query's distinct forests, in order of first appearance; files are read once per processor and the
        last query's bank (and its device copy) is kept."""
        paths = tuple(_predictor_path(self.ad_preds, g, t) for g, t in pairs)
        if self._bank[0] != paths:
            for p in paths:
                if p not in self._models:
                    self._models[p] = _check_model(_forest.load(p), p)
            self._bank = (paths, _forest.ForestBank([self._models[p] for p in paths]))
        return self._bank[1]

    def _predict_ad_risk(self, preds_df: pd.DataFrame) -> pd.DataFrame:
        keys = list(zip(preds_df["gene_id"], preds_df["tissue_id"]))
        index = {}
        for k in keys:
            index.setdefault(k, len(index))
        if keys:
            bank = self._bank_for(list(index))
            emb = np.stack([np.asarray(e, dtype=np.float32).reshape(-1) for e in preds_df["embedding"]])
            assert emb.shape[1] == bank.n_features, f"the predictors take {bank.n_features} features, the embeddings have {emb.shape[1]}"
            x = torch.from_numpy(emb).cuda()
            rows = torch.tensor([index[k] for k in keys], dtype=torch.int32, device=x.device)
            out = torch.empty((len(keys), bank.n_outputs), dtype=torch.float32, device=x.device)
            ops.forest_predict(x, bank.to(x.device), model_of_row=rows, out=out)           # one launch for the whole query
            preds_df["ad_risk"] = out[:, 1].contiguous().cpu().numpy()
        else:
            preds_df["ad_risk"] = np.zeros(0, dtype=np.float32)
        preds_df["gene_name"] = preds_df["gene_id"].map(self.genes_map["gene_name"])
        return preds_df

"""The vcf2risk surface without a GPU (variantformer_amd/processors/ad_risk.py): the reference's names and signatures, the local
predictor store with the reference's tissue-id spellings, the missing pair, and the reference's asserts -- all of which fire
before anything touches a device."""
import inspect

import numpy as np
import pandas as pd
import pytest

from tests import forest_cases as FC
from variantformer_amd.processors import ad_risk as A


def _store(tmp_path):
    m = FC.make_forest(40, 5, 8, 2, depth=3)
    (tmp_path / "models").mkdir()
    m.save(str(tmp_path / "models" / "a_7.npz"))
    m.save(str(tmp_path / "abs.npz"))
    pd.DataFrame({"gene_id": ["ENSG_A", "ENSG_B"], "tissue_id": [7, 12], "file_path": ["models/a_7.npz", str(tmp_path / "abs.npz")]}
                 ).to_csv(tmp_path / "manifest.csv", index=False)
    return A.LocalPredictorStore(str(tmp_path))


def test_public_signatures():
    assert list(inspect.signature(A.ADrisk.__init__).parameters) == ["self", "gene_id", "tissue_id", "model_class", "predictors"]
    assert inspect.signature(A.ADrisk.__init__).parameters["model_class"].default == "v4_pcg"
    assert list(inspect.signature(A.ADrisk.__call__).parameters) == ["self", "gene_tissue_embeds"]
    sig = inspect.signature(A.ADriskFromVCF.__init__)
    assert list(sig.parameters) == ["self", "model_class", "predictors", "config_dir", "vcfprocessor_kwargs"]
    assert sig.parameters["vcfprocessor_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert sig.parameters["model_class"].default == "v4_pcg" and sig.parameters["predictors"].default is None
    call = inspect.signature(A.ADriskFromVCF.__call__)
    assert list(call.parameters) == ["self", "vcf_file", "gene_ids", "tissue_ids", "dataset_factory"]
    assert call.parameters["dataset_factory"].default is None
    for name in ("_init_model", "_init_dataloader", "_format_query", "_predict_ad_risk", "_reformat_predictions"):
        assert callable(getattr(A.ADriskFromVCF, name))                 # the reference's method names
    assert callable(A.ADrisk._load_ad_predictor)


def test_local_predictor_store(tmp_path):
    s = _store(tmp_path)
    want = str(tmp_path / "models" / "a_7.npz")
    for tid in (7, "7", "model_7", "tissue_7", np.int64(7)):
        assert s.get_file_path("ENSG_A", tid) == want and s.exists("ENSG_A", tid)
    assert s.get_file_path("ENSG_B", 12) == str(tmp_path / "abs.npz")
    assert s.get_file_path("ENSG_A", 12) is None and s.get_file_path("ENSG_C", 7) is None and not s.exists("ENSG_C", "model_7")
    with pytest.raises(ValueError):
        s.get_file_path("ENSG_A", "liver")
    pd.DataFrame({"gene_id": ["g"], "tissue_id": [1]}).to_csv(tmp_path / "manifest.csv", index=False)
    with pytest.raises(ValueError, match="file_path"):
        A.LocalPredictorStore(str(tmp_path))


def test_adrisk_asserts_and_the_missing_pair(tmp_path):
    s = _store(tmp_path)
    with pytest.raises(AssertionError, match="model_class should be either"):
        A.ADrisk("ENSG_A", 7, model_class="v3", predictors=s)
    with pytest.raises(AssertionError, match="tissue_id should be an integer"):
        A.ADrisk("ENSG_A", "7", predictors=s)
    with pytest.raises(AssertionError, match="gene_id should be a string"):
        A.ADrisk(17, 7, predictors=s)
    with pytest.raises(FileNotFoundError, match="AD predictor not found for gene ENSG_C and tissue 7"):
        A.ADrisk("ENSG_C", 7, predictors=s)
    with pytest.raises(ValueError, match="predictors"):
        A.ADrisk("ENSG_A", 7)
    r = A.ADrisk("ENSG_A", 7, predictors=str(tmp_path))                 # a directory is read as a LocalPredictorStore
    assert (r.gene_id, r.tissue_id, r.model_class) == ("ENSG_A", 7, "v4_pcg")
    assert r.predictor.n_trees == 5 and r.bank.n_models == 1 and r.bank.n_features == 8
    with pytest.raises(AssertionError, match="embeddings should be"):
        r(np.zeros((3, 9), dtype=np.float32))
    one = FC.make_forest(41, 2, 8, 1, depth=2)
    one.save(str(tmp_path / "abs.npz"))
    with pytest.raises(ValueError, match="second output"):
        A.ADrisk("ENSG_B", 12, predictors=s)


def test_query_asserts_and_the_reformatting():
    r = object.__new__(A.ADriskFromVCF)                                 # no model is loaded: these run before any of it is used
    vocab = {"liver": 3, "lung": 5}
    r.tissue_map = pd.DataFrame({"tissue": list(vocab)}, index=pd.Index(list(vocab.values()), name="tissue_id"))
    q = r._format_query(["g1", "g2", "g1"], [5, 3, 3])
    assert list(q.columns) == ["gene_id", "tissues"] and q["tissues"].tolist() == ["lung", "liver", "liver"]
    with pytest.raises(AssertionError, match="2 lists of the same length"):
        r._format_query(["g1", "g2"], [5])
    with pytest.raises(AssertionError, match="tissue_id should be an integer"):
        r._format_query(["g1"], ["5"])
    with pytest.raises(AssertionError, match="gene_id should be a string"):
        r._format_query([1], [5])
    emb = [np.ones((1, 4), dtype=np.float32), np.zeros((1, 4), dtype=np.float32)]
    df = pd.DataFrame({"gene_id": ["g1", "g2"], "tissues": [[5], [3]], "tissue_names": [["lung"], ["liver"]],
                       "predicted_expression": [np.array([[1.5]]), np.array([[2.5]])], "embeddings": emb})
    out = r._reformat_predictions(df)
    assert list(out.columns) == ["gene_id", "tissue_id", "tissue_name", "predicted_expression", "embedding"]
    assert out["tissue_id"].tolist() == [5, 3] and out["tissue_name"].tolist() == ["lung", "liver"]
    assert out["predicted_expression"].tolist() == [1.5, 2.5] and out["embedding"][0].shape == (1, 4)
    two = pd.DataFrame({"gene_id": ["g1"], "tissues": [[5, 3]], "tissue_names": [["lung", "liver"]],
                        "predicted_expression": [np.zeros((2, 1))], "embeddings": [np.zeros((2, 4))]})
    with pytest.raises(AssertionError):
        r._reformat_predictions(two)                                    # one tissue per row

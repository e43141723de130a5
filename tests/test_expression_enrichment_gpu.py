"""VCFProcessor.expression_enrichment on the GPU, on a synthetic format_output frame: every kind of `labels` (a column of the
frame, an array, "max_tissue", None with n_clusters) gives the columns and shapes promised, and equals enrichment.enrich on the
labels it stands for."""
import numpy as np
import pandas as pd
import pytest

from tests import enrich_cases as E

pytestmark = pytest.mark.gpu

GENES, TISSUES, GROUPS = 120, 6, 4


def _frame():
    """(frame, annotations, group [GENES]): four groups of genes, each with its own expression profile peaking in its own tissue,
    a column `go_broad` naming the group (None for a few genes), and annotations with one term per group plus random ones."""
    rng = np.random.default_rng(21)
    group = np.arange(GENES) % GROUPS
    profile = rng.standard_normal((GROUPS, TISSUES))
    profile[np.arange(GROUPS), np.arange(GROUPS)] += 6.0              # group g peaks in tissue g
    x = (profile[group] + 0.3 * rng.standard_normal((GENES, TISSUES))).astype(np.float32)
    genes = [f"ENSG{i:05d}" for i in range(GENES)]
    broad = np.array([f"category_{g}" for g in group], dtype=object)
    broad[[5, 77]] = None
    frame = pd.DataFrame({"gene_id": genes, "tissues": [list(range(TISSUES))] * GENES, "tissue_names": [[f"tissue_{j}" for j in range(TISSUES)]] * GENES,
                          "predicted_expression": list(x), "go_broad": broad, "cluster_id": group.astype(np.int64)})
    ann = {g: [] for g in genes}
    for i, g in enumerate(genes):
        if i % 3:                                                     # two thirds of every group carry its term
            ann[g].append(f"GO:group_{group[i]}")
        for j in range(8):
            if rng.random() < 0.2:
                ann[g].append(f"GO:random_{j}")
    ann["ENSG_elsewhere"] = ["GO:group_0"]
    return frame, ann, group


def _proc():
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    return VCFProcessor.__new__(VCFProcessor)


def _check(out, frame, k, terms):
    for key, dtype in (("count", np.int32), ("log_p", np.float64), ("p", np.float64), ("fold", np.float64), ("q", np.float64)):
        assert out[key].shape == (terms, k) and out[key].dtype == dtype, key
    assert out["term_size"].shape == (terms,) and out["cluster_size"].shape == (k,) and len(out["terms"]) == terms and len(out["cluster_names"]) == k
    assert out["labels"].shape == (GENES,) and out["labels"].dtype == np.int32
    assert list(out["frame"].columns) == ["cluster", "term", "count", "term_size", "cluster_size", "fold", "log_p", "p", "q"]
    assert frame.columns[-1] == "enrichment_cluster" and len(frame["enrichment_cluster"]) == GENES
    assert (out["frame"]["q"] <= 0.05).all() and set(out["frame"]["cluster"]) <= set(out["cluster_names"])


def test_every_kind_of_labels_gives_the_promised_columns():
    from variantformer_amd import enrichment
    proc = _proc()
    frame, ann, group = _frame()
    universe = list(frame["gene_id"])
    terms = len(enrichment.membership(ann, universe, min_size=5, max_size=500).terms)
    assert terms == GROUPS + 8
    direct = enrichment.enrich(group.astype(np.int32), ann, universe)
    found = sorted(zip(direct["frame"]["cluster"], direct["frame"]["term"]))
    assert [(g, f"GO:group_{g}") for g in range(GROUPS)] == [f for f in found if "group" in f[1]], "every group's own term is significant in it"

    # an array, and a column of integers: the labels as they are
    f1 = frame.copy()
    out = proc.expression_enrichment(f1, ann, labels=group)
    _check(out, f1, GROUPS, terms)
    assert np.array_equal(out["q"].view(np.uint64), direct["q"].view(np.uint64)) and f1["enrichment_cluster"].tolist() == group.tolist()
    f2 = frame.copy()
    out2 = proc.expression_enrichment(f2, ann, labels="cluster_id")
    assert np.array_equal(out2["q"].view(np.uint64), direct["q"].view(np.uint64)) and f2["enrichment_cluster"].dtype == np.int64

    # a column of names: numbered in sorted order, a missing value is no cluster but stays in the universe
    f3 = frame.copy()
    out3 = proc.expression_enrichment(f3, ann, labels="go_broad")
    _check(out3, f3, GROUPS, terms)
    assert out3["cluster_names"] == [f"category_{g}" for g in range(GROUPS)] and out3["labels"][[5, 77]].tolist() == [-1, -1]
    assert f3["enrichment_cluster"][5] is None and f3["enrichment_cluster"][6] == "category_2"
    assert out3["cluster_size"].sum() == GENES - 2 and out3["term_size"].tolist() == direct["term_size"].tolist()
    assert ("category_1", "GO:group_1") in set(zip(out3["frame"]["cluster"], out3["frame"]["term"]))

    # the tissue of highest expression: group g peaks in tissue g, tissues 4 and 5 stay empty
    f4 = frame.copy()
    out4 = proc.expression_enrichment(f4, ann, labels="max_tissue")
    _check(out4, f4, TISSUES, terms)
    assert out4["cluster_names"] == [f"tissue_{j}" for j in range(TISSUES)] and out4["labels"].tolist() == group.tolist()
    assert out4["cluster_size"].tolist() == [GENES // GROUPS] * GROUPS + [0, 0] and (out4["log_p"][:, GROUPS:] == 0).all()
    assert f4["enrichment_cluster"].tolist() == [f"tissue_{g}" for g in group]
    assert np.array_equal(out4["log_p"][:, :GROUPS].view(np.uint64), direct["log_p"].view(np.uint64))

    # None: the Ward tree of the genes' expression, cut into n_clusters
    f5 = frame.copy()
    out5 = proc.expression_enrichment(f5, ann, n_clusters=GROUPS, fdr=0.01)
    _check({**out5, "frame": out5["frame"][out5["frame"]["q"] <= 0.05]}, f5, GROUPS, terms)
    pairs = set(zip(out5["labels"].tolist(), group.tolist()))
    assert len(pairs) == GROUPS, "four well separated profiles: the cut finds the groups"
    assert (out5["frame"]["q"] <= 0.01).all() and len(out5["frame"]) >= GROUPS
    first = [int(np.flatnonzero(out5["labels"] == c)[0]) for c in range(GROUPS)]
    assert first == sorted(first) and f5["enrichment_cluster"].tolist() == out5["labels"].tolist()
    assert E.PLANTED_GENES == 600

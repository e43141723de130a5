"""VCFProcessor.expression_umap(..., return_model=True) and VCFProcessor.expression_umap_transform on synthetic format_output
frames: a second prediction placed in the coordinates of a first, per gene and per (gene, tissue), through manifold.fit and
UMAPModel.transform."""
import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

GENES, TISSUES, EMB = 60, 12, 8
NAMES = [f"tissue{t:02d}" for t in range(TISSUES)]


def _frames():
    g = np.random.default_rng(20261021)
    programme = g.standard_normal((4, TISSUES))
    load = g.standard_normal((GENES, 4))
    own = 0.5 * g.standard_normal((GENES, TISSUES))
    embeddings = g.standard_normal((GENES, TISSUES, EMB)).astype(np.float32)
    frames = []
    for noise in (0.0, 0.05):                                          # the second individual: the first's genes, slightly changed
        expr = (load + noise * g.standard_normal(load.shape)) @ programme + own + 5.0
        emb = embeddings * (1 + noise * g.standard_normal(embeddings.shape)).astype(np.float32)
        frames.append(pd.DataFrame({"gene_id": [f"ENSG{i:05d}" for i in range(GENES)], "tissues": [list(range(TISSUES))] * GENES,
                                    "tissue_names": [NAMES] * GENES, "predicted_expression": [e.reshape(TISSUES, 1) for e in expr.astype(np.float32)],
                                    "embeddings": list(emb.astype(np.float32))}))
    return frames


def test_a_second_frame_is_placed_in_the_first_frames_coordinates():
    from variantformer_amd import manifold, neighbors
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    first, second = _frames()
    vp = VCFProcessor()
    kw = dict(n_neighbors=10, n_epochs=30)
    plain = vp.expression_umap(first.copy(), **kw)
    assert set(plain) == {"coords", "labels"}, "the default is unchanged"
    out = vp.expression_umap(first, return_model=True, **kw)
    assert set(out) == {"coords", "labels", "model"} and isinstance(out["model"], manifold.UMAPModel)
    assert np.array_equal(out["coords"], plain["coords"]) and np.array_equal(out["model"].embedding, plain["coords"]), "the same embedding, bit for bit"
    assert np.array_equal(np.stack((first["umap_1"], first["umap_2"]), 1), out["coords"]) and first["umap_1"].dtype == np.float32
    model = out["model"]
    assert (model.rows, model.columns, model.n_neighbors, model.n_epochs) == (GENES, TISSUES, 10, 30)
    placed = vp.expression_umap_transform(model, second, n_epochs=20)
    assert set(placed) == {"coords", "labels"} and placed["labels"] == list(first["gene_id"]), "the first frame's labels, in its order"
    assert placed["coords"].shape == (GENES, 2) and placed["coords"].dtype == np.float32 and np.isfinite(placed["coords"]).all()
    assert [c for c in second.columns if c.startswith("umap_")] == ["umap_1", "umap_2"] and second["umap_1"].dtype == np.float32 and second["umap_2"].dtype == np.float32
    assert np.array_equal(np.stack((second["umap_1"], second["umap_2"]), 1), placed["coords"])
    m, _ = neighbors.from_predictions(second)
    assert np.array_equal(placed["coords"], model.transform(m, n_epochs=20)), "the frame's matrix through UMAPModel.transform"
    assert np.array_equal(vp.expression_umap_transform(model, second.copy(), n_epochs=20)["coords"], placed["coords"]), "deterministic"
    assert np.array_equal(np.stack((first["umap_1"], first["umap_2"]), 1), out["coords"]), "the first frame's points did not move"
    # a slightly changed gene lands near where the gene stood: nearer than the typical distance between two genes
    moved = np.linalg.norm(placed["coords"] - out["coords"], axis=1)
    spread = np.linalg.norm(out["coords"] - out["coords"][::-1], axis=1)
    print(f"[expression umap transform] median distance of a placed gene from its own fitted position {np.median(moved):.3f}; "
          f"between two different genes {np.median(spread):.3f}")
    assert np.median(moved) < np.median(spread)
    # another tissue count is refused, with both counts stated
    fewer = second.drop(columns=["umap_1", "umap_2"]).copy()
    fewer["tissue_names"] = [NAMES[:-1]] * GENES
    fewer["tissues"] = [list(range(TISSUES - 1))] * GENES
    fewer["predicted_expression"] = [np.asarray(v)[:-1] for v in fewer["predicted_expression"]]
    fewer = fewer.drop(columns=["embeddings"])
    with pytest.raises(ValueError, match=rf"{TISSUES - 1} columns.*fitted on {TISSUES}"):
        vp.expression_umap_transform(model, fewer)
    assert not [c for c in fewer.columns if c.startswith("umap_")], "a refused call leaves the frame as it was"


def test_embeddings_per_gene_and_per_gene_and_tissue():
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    first, second = _frames()
    vp = VCFProcessor()
    kw = dict(n_neighbors=10, n_epochs=30)
    one = vp.expression_umap(first, on="embeddings", tissue="tissue03", return_model=True, **kw)
    o = vp.expression_umap_transform(one["model"], second, on="embeddings", tissue="tissue03", n_epochs=20)
    assert o["coords"].shape == (GENES, 2) and o["labels"] == list(first["gene_id"]) and second["umap_2"].dtype == np.float32
    with pytest.raises(ValueError, match=rf"{TISSUES} columns.*fitted on {EMB}"):
        vp.expression_umap_transform(one["model"], second, on="predicted_expression")
    # all tissues: (gene, tissue) rows, a cell per gene holding its tissues' coordinates
    a, b = (f.drop(columns=[c for c in f.columns if c.startswith("umap_")]) for f in (first, second))
    both = vp.expression_umap(a, on="embeddings", return_model=True, **kw)
    assert both["model"].rows == GENES * TISSUES and both["model"].columns == EMB
    p = vp.expression_umap_transform(both["model"], b, on="embeddings", tissue=None, n_epochs=20)
    assert p["coords"].shape == (GENES * TISSUES, 2) and p["labels"][:2] == [("ENSG00000", "tissue00"), ("ENSG00000", "tissue01")]
    assert p["labels"] == both["labels"] and np.isfinite(p["coords"]).all()
    assert b["umap_1"].dtype == object and b["umap_1"].iloc[5].shape == (TISSUES,) and b["umap_1"].iloc[5].dtype == np.float32
    assert np.array_equal(np.stack(list(b["umap_2"])).reshape(-1), p["coords"][:, 1])
    # tissues as rows: no gene rows, no column
    t = vp.expression_umap(first.drop(columns=[c for c in first.columns if c.startswith("umap_")]), axis="tissues", n_neighbors=5, n_epochs=30, return_model=True)
    by_tissue = second.drop(columns=[c for c in second.columns if c.startswith("umap_")])
    q = vp.expression_umap_transform(t["model"], by_tissue, axis="tissues", n_epochs=20)
    assert q["labels"] == NAMES and q["coords"].shape == (TISSUES, 2) and not [c for c in by_tissue.columns if c.startswith("umap_")]

"""manifold.umap end to end on the GPU, and VCFProcessor.expression_umap on a synthetic format_output frame.  The embedding of
four Gaussian blobs is held to the fp64 numpy reference of tests/umap_cases.py run with the same seed: its trustworthiness
(scikit-learn's, by correlation distance) may fall below the reference's by no more than the reference's own spread over five
seeds, which is recorded there."""
import numpy as np
import pandas as pd
import pytest
import torch

from tests import umap_cases as U

pytestmark = pytest.mark.gpu


def test_the_blobs_embed_as_well_as_the_reference():
    from variantformer_amd import manifold
    x = U.blobs()
    kwargs = dict(n_neighbors=U.BLOBS["n_neighbors"], min_dist=U.BLOBS["min_dist"], n_epochs=U.BLOBS["n_epochs"], init="random", seed=42)
    y = manifold.umap(x, **kwargs)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == (400, 2) and np.isfinite(y).all()
    ref = U.blobs_reference(42)
    t_dev, t_ref = U.trust(x, y), U.trust(x, ref)
    t_start = U.trust(x, U.rescale(U.random_init(400, 2, 42)))
    print(f"[umap blobs] trustworthiness: device {t_dev:.4f}, fp64 reference {t_ref:.4f}, random initialisation {t_start:.4f}; "
          f"margin {U.TRUST_MARGIN} (the reference's spread over five seeds); largest coordinate difference {np.abs(y - ref).max():.2e}")
    assert t_dev >= t_ref - U.TRUST_MARGIN
    assert np.array_equal(manifold.umap(x, **kwargs), y), "two runs are equal bit for bit"
    t = manifold.umap(torch.from_numpy(x).cuda(), **kwargs)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), y), "a tensor on the device in, a tensor out, the same embedding"
    assert not np.array_equal(manifold.umap(x, **{**kwargs, "seed": 43}), y)
    # the stages by hand give the same: fuzzy_graph + layout from the same start, split at an epoch
    from variantformer_amd import neighbors
    idx, dist = neighbors.knn(x, k=14)
    graph = manifold.fuzzy_graph(idx, dist)
    a, b = manifold.find_ab(0.1)
    start = manifold.rescale(manifold.random_init(400, 2, 42)).cpu().numpy()
    assert np.array_equal(manifold.random_init(400, 2, 42).cpu().numpy(), U.random_init(400, 2, 42)), "the counter-based start, restated in numpy"
    first = manifold.layout(graph, start, 100, a, b, seed=42, epoch_end=37)
    assert np.array_equal(manifold.layout(graph, first, 100, a, b, seed=42, epoch_begin=37), y)
    # the other initialisations: pca (deterministic), an array, other dimensions
    p = manifold.umap(x, n_neighbors=15, n_epochs=100, init="pca")
    assert np.isfinite(p).all() and np.array_equal(p, manifold.umap(x, n_neighbors=15, n_epochs=100, init="pca"))
    print(f"[umap blobs] trustworthiness with init='pca': {U.trust(x, p):.4f}")
    assert U.trust(x, p) > t_start + 0.2, "far better than a random scatter; the reference's margin is for its own initialisation"
    assert np.array_equal(manifold.umap(x, **{**kwargs, "init": U.random_init(400, 2, 42)}), y), "an array is rescaled like any init"
    for dim in (1, 3, 8):
        z = manifold.umap(x, n_neighbors=15, n_epochs=20, init="random", n_components=dim)
        assert z.shape == (400, dim) and np.isfinite(z).all()


def test_expression_umap_on_a_synthetic_frame():
    from variantformer_amd import manifold, neighbors
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    genes, tissues, emb = 60, 12, 8
    g = np.random.default_rng(20261020)
    names = [f"tissue{t:02d}" for t in range(tissues)]
    programme = g.standard_normal((4, tissues))
    expr = (g.standard_normal((genes, 4)) @ programme + 0.5 * g.standard_normal((genes, tissues)) + 5.0).astype(np.float32)
    embeddings = g.standard_normal((genes, tissues, emb)).astype(np.float32)
    df = pd.DataFrame({"gene_id": [f"ENSG{i:05d}" for i in range(genes)], "tissues": [list(range(tissues))] * genes,
                       "tissue_names": [names] * genes, "predicted_expression": [e.reshape(tissues, 1) for e in expr],
                       "embeddings": list(embeddings)})
    vp = VCFProcessor()
    kw = dict(n_neighbors=10, n_epochs=30)
    out = vp.expression_umap(df, **kw)
    assert set(out) == {"coords", "labels"} and out["labels"] == list(df["gene_id"]), "label order is the frame's"
    assert out["coords"].shape == (genes, 2) and out["coords"].dtype == np.float32 and np.isfinite(out["coords"]).all()
    assert [c for c in df.columns if c.startswith("umap_")] == ["umap_1", "umap_2"] and df["umap_1"].dtype == np.float32
    assert np.array_equal(np.stack((df["umap_1"], df["umap_2"]), 1), out["coords"])
    m, _ = neighbors.from_predictions(df)
    assert np.array_equal(out["coords"], manifold.umap(m, **kw)), "the frame's matrix through manifold.umap"
    assert np.array_equal(vp.expression_umap(df.copy(), **kw)["coords"], out["coords"]), "deterministic"
    three = vp.expression_umap(df, n_components=3, init="random", **kw)
    assert three["coords"].shape == (genes, 3) and "umap_3" in df.columns
    # one tissue's embeddings: gene rows again; all tissues: (gene, tissue) rows, a cell per gene holding its tissues' coordinates
    one = df.drop(columns=["umap_1", "umap_2", "umap_3"])
    o = vp.expression_umap(one, on="embeddings", tissue="tissue03", **kw)
    assert o["coords"].shape == (genes, 2) and o["labels"] == list(df["gene_id"]) and one["umap_2"].dtype == np.float32
    both = df.drop(columns=["umap_1", "umap_2", "umap_3"])
    b = vp.expression_umap(both, on="embeddings", **kw)
    assert b["coords"].shape == (genes * tissues, 2) and b["labels"][:2] == [("ENSG00000", "tissue00"), ("ENSG00000", "tissue01")]
    assert both["umap_1"].dtype == object and both["umap_1"].iloc[5].shape == (tissues,)
    assert np.array_equal(np.stack(list(both["umap_2"])).reshape(-1), b["coords"][:, 1])
    # tissues as rows: no gene rows, no column
    by_tissue = df.drop(columns=["umap_1", "umap_2", "umap_3"])
    t = vp.expression_umap(by_tissue, axis="tissues", n_neighbors=5, n_epochs=30)
    assert t["labels"] == names and t["coords"].shape == (tissues, 2) and not [c for c in by_tissue.columns if c.startswith("umap_")]

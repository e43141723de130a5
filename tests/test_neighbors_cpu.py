"""The expression and embedding neighbours without a GPU: the boundary of include/vf_hip_neighbors.h (it parses, its three names
are exported and bound through _lib.ENTRIES), every refusal with its argument
named, the conditions the case table of tests/neighbors_cases.py rests on, its references against scipy and scikit-learn, and
the host side of variantformer_amd/neighbors.py: matrix building, labels and argument checks."""
import inspect
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests import neighbors_cases as N
from tests import topk_cases as T
from tests import write_set_cases as W
from tests.conftest import REPO

NAMES = ["vf_knn_dot", "vf_pairwise_dot", "vf_rows_standardize"]
ARGS = {"vf_rows_standardize": 9, "vf_knn_dot": 13, "vf_pairwise_dot": 12}


def _header(name="vf_hip_neighbors.h") -> str:
    with open(os.path.join(REPO, "include", name)) as f:
        return f.read()


# ---- 1. header and binding ---------------------------------------------------------------------------------------------------------
def test_header_parses_and_its_names_are_exported_and_bound():
    from variantformer_amd import _lib
    from variantformer_amd.csrc import build as B
    text = _header()
    assert W.stream_entries(text) == NAMES
    assert sorted(_lib.ENTRIES["vf_hip_neighbors.h"]) == NAMES, "ctypes binding and vf_hip_neighbors.h disagree"
    assert "vf_neighbors.hip" in B.SOURCES and any(h.endswith("vf_hip_neighbors.h") for h in B.HEADERS)
    assert "vf_neighbors.hip" not in B.EXTRA_FLAGS                    # the NaN order needs NaNs honoured: no -fno-honor-nans
    bound = _lib.load()
    assert {name: len(_lib.SIGNATURES[name]) for name in NAMES} == ARGS
    assert _lib.ABI_VERSION == 13 and bound.vf_version() == 13
    assert "seven headers" in text
    for word in ("Arguments", "Write set", "Arithmetic", "Non-finite operands", "Refused before anything is launched", "Order"):
        assert text.count(word) >= (1 if word == "Order" else 3), f"an entry's comment contract has no `{word}` part"
    assert N.tile_constants() == {"BM": N.BM, "BN": N.BN, "BK": N.BK} and min(N.BM, N.BN, N.BK) >= 2
    from variantformer_amd import neighbors
    assert neighbors.K_MAX == T.MAX_K


def _err(lib):
    return lib.vf_last_error().decode()


P = 4096                                                 # a non-null, aligned address; never dereferenced
INVALID = 1


def test_knn_dot_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(q=P, ldq=50, Rq=0, y=P, ldy=50, Ry=100, d=49, self_offset=-1, k=30, values=P, indices=P, ldo=30):
        return lib.vf_knn_dot(q, ldq, Rq, y, ldy, Ry, d, self_offset, k, values, indices, ldo, 0)
    assert call() == 0 and call(self_offset=0) == 0 and call(self_offset=2 ** 40) == 0 and call(Ry=0) == 0      # Rq = 0: nothing launched
    for name in ("q", "y", "values", "indices"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        assert call(**{name: P + 2}) == INVALID and re.search(rf"\b{name} must be 4-byte aligned", _err(lib)), _err(lib)
    for d in (0, -1):
        assert call(d=d) == INVALID and "d=" in _err(lib)
    assert call(d=1) == 0
    assert call(ldq=48) == INVALID and "ldq" in _err(lib)
    assert call(ldy=48) == INVALID and "ldy" in _err(lib)
    assert call(ldo=29) == INVALID and "ldo" in _err(lib)
    for k in (0, -1, 65):
        assert call(k=k, ldo=128) == INVALID and "k=" in _err(lib)
    assert call(k=1) == 0 and call(k=64, ldo=64) == 0
    assert call(Rq=-1) == INVALID and "Rq=" in _err(lib)
    assert call(Ry=-1) == INVALID and "Ry=" in _err(lib)
    assert call(Ry=2 ** 31) == INVALID and "Ry=" in _err(lib) and "2^31" in _err(lib)
    assert call(Ry=2 ** 31 - 1) == 0
    assert call(Rq=2 ** 36) == INVALID and "grid" in _err(lib)
    for so in (-2, -2 ** 40):
        assert call(self_offset=so) == INVALID and "self_offset" in _err(lib)


def test_pairwise_dot_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(q=P, ldq=50, Rq=0, y=P, ldy=50, Ry=100, d=49, self_offset=-1, mode=0, out=P, ldo=100):
        return lib.vf_pairwise_dot(q, ldq, Rq, y, ldy, Ry, d, self_offset, mode, out, ldo, 0)
    assert call() == 0 and call(mode=1, self_offset=0) == 0 and call(Rq=5, Ry=0, ldo=0) == 0
    for name in ("q", "y", "out"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        assert call(**{name: P + 2}) == INVALID and re.search(rf"\b{name} must be 4-byte aligned", _err(lib)), _err(lib)
    assert call(d=0) == INVALID and "d=" in _err(lib)
    assert call(ldq=48) == INVALID and "ldq" in _err(lib)
    assert call(ldy=48) == INVALID and "ldy" in _err(lib)
    assert call(ldo=99) == INVALID and "ldo" in _err(lib)
    for mode in (-1, 2):
        assert call(mode=mode) == INVALID and "mode=" in _err(lib)
    assert call(Rq=-1) == INVALID and "Rq=" in _err(lib)
    assert call(Ry=-1) == INVALID and "Ry=" in _err(lib)
    assert call(Ry=2 ** 31, ldo=2 ** 31) == INVALID and "Ry=" in _err(lib)
    assert call(self_offset=-2) == INVALID and "self_offset" in _err(lib)
    assert call(Rq=2 ** 40, Ry=2 ** 30, ldo=2 ** 30) == INVALID and "grid" in _err(lib)


def test_rows_standardize_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(x=P, ldx=50, R=0, d=49, center=1, z=P, ldz=50, norm=P):
        return lib.vf_rows_standardize(x, ldx, R, d, center, z, ldz, norm, 0)
    assert call() == 0 and call(norm=0) == 0 and call(center=0) == 0
    for name in ("x", "z"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
    for name in ("x", "z", "norm"):
        assert call(**{name: P + 2}) == INVALID and re.search(rf"\b{name} must be 4-byte aligned", _err(lib)), _err(lib)
    assert call(d=0) == INVALID and "d=" in _err(lib)
    assert call(ldx=48) == INVALID and "ldx" in _err(lib)
    assert call(ldz=48) == INVALID and "ldz" in _err(lib)
    for center in (-1, 2):
        assert call(center=center) == INVALID and "center=" in _err(lib)
    assert call(R=-1) == INVALID and "R=" in _err(lib)
    assert call(R=2 ** 33) == INVALID and "grid" in _err(lib)


def test_the_wrappers_allocate_nothing_and_refuse_cpu_tensors():
    from variantformer_amd import ops
    for fn, outs in ((ops.rows_standardize, ("z",)), (ops.knn_dot, ("values", "indices")), (ops.pairwise_dot, ("out",))):
        src = inspect.getsource(fn)
        assert not re.search(r"\b(empty|empty_like|zeros|zeros_like|ones|full|new_empty|new_zeros|new_full|tensor|arange|clone|contiguous)\s*\(", src)
        prm = inspect.signature(fn).parameters
        for o in outs:
            assert prm[o].kind is inspect.Parameter.KEYWORD_ONLY and prm[o].default is inspect.Parameter.empty
        assert fn.__name__ not in W.allocating_wrappers()
    assert W.uncovered_wrappers() == []
    x = torch.zeros(4, 8)
    i = torch.zeros(4, 2, dtype=torch.int32)
    with pytest.raises(Exception, match="GPU"):
        ops.rows_standardize(x, z=torch.zeros(4, 8))
    with pytest.raises(Exception, match="GPU"):
        ops.knn_dot(x, x, 2, values=torch.zeros(4, 2), indices=i)
    with pytest.raises(Exception, match="GPU"):
        ops.pairwise_dot(x, x, out=torch.zeros(4, 4))


# ---- 2. the case table ---------------------------------------------------------------------------------------------------------------
def test_the_geometries_are_what_the_contract_asks_for():
    G = N.geometries()
    base = (N.BM + 1, 2 * N.BN + 1, N.BK + 1)
    for axis, tile in ((0, N.BM), (1, N.BN), (2, N.BK)):
        for size in (1, tile - 1, tile, tile + 1, 2 * tile + 1):
            assert any(g[axis] == size and all(g[a] == base[a] for a in range(3) if a != axis) for g in G), (axis, size)
    assert {g[3] for g in G} == set(N.KS) == {1, 30, 31, 64}
    for k in N.KS:
        assert {k - 1, k, k + 1} <= {g[1] for g in G if g[3] == k}
    assert (5, 0, 7, 1) in {g[:4] for g in G}, "Ry == 0: no candidate, every rank is padding"
    assert any(g[1] == T.MAX_N + N.BN + 1 for g in G) and any(g[2] == 1536 for g in G)
    assert {g[4] for g in G} == set(N.SELF_MODES)
    big = [g for g in G if g[1] == 3 * N.BN + 2]
    assert {g[4] for g in big} == set(N.SELF_MODES)
    assert len(G) == len(set(G)) and len(G) <= 48


def test_exact_data_is_exact_and_leading_dimensions_are_odd():
    g = (N.BM + 1, 2 * N.BN + 1, 1536, 30, "zero")
    assert g in N.geometries()
    c = N.exact_case(g, "dense")
    assert c.q.shape == (g[0], 1536 + N.EXTRA_LD) and (1536 + N.EXTRA_LD) % 2 == 1 and c.self_offset == 0
    assert (c.q[:, 1536:].view(np.uint8) == 0xFF).all() and (c.y[:, 1536:].view(np.uint8) == 0xFF).all()
    q, y = c.q[:, :1536].astype(np.float64), c.y[:, :1536].astype(np.float64)
    assert np.abs(q).max() <= 8 and np.abs(y).max() <= 8 and (q == np.round(q)).all()
    partial = np.abs(np.cumsum(q[:5, None, :] * y[None, :7, :], axis=2)).max()
    assert partial <= 64 * 1536 < 2 ** 24
    # so every summation order gives the bits of the chain: fp64 matmul rounded once, and the reversed chain
    assert np.array_equal(N.chain(c.q[:, :1536], c.y[:, :1536]), (q @ y.T).astype(np.float32))
    assert np.array_equal(N.chain(c.q[:, 1535::-1], c.y[:, 1535::-1]), (q @ y.T).astype(np.float32))
    ties = N.exact_case((N.BM + 1, 2 * N.BN + 1, N.BK + 1, 30, "none"), "ties")
    v, i = N.expected(ties)
    assert (v[:, :-1] == v[:, 1:]).mean() > 0.5, "ties are plentiful"
    assert ((v[:, :-1] > v[:, 1:]) | (i[:, :-1] < i[:, 1:])).all()
    assert N.exact_case(g, "ties").y.tobytes() == N.exact_case(g, "ties").y.tobytes()         # seeded


def test_planted_winners_are_where_the_kind_says():
    g = (N.BM + 1, 3 * N.BN + 2, N.BK + 1, 31, "none")
    assert g in N.geometries()
    tiles = 4
    for kind in ("first_tile", "last_tile", "per_tile", "edges"):
        c = N.exact_case(g, kind)
        rows = N.planted(kind, g[1], g[3])
        v, i = N.expected(c)
        n = min(len(rows), g[3])
        assert all(set(r[:n]) <= set(rows) for r in i.tolist()), kind
        assert (i[:, :n] == np.array(rows[:n])).all(), "equal winners rank by row: the tie rule"
    assert N.planted("first_tile", g[1], 31) == list(range(31))
    assert min(N.planted("last_tile", g[1], 31)) == 3 * N.BN and max(N.planted("last_tile", g[1], 31)) == g[1] - 1
    assert [j // N.BN for j in N.planted("per_tile", g[1], 31)] == list(range(tiles))
    assert {N.BN - 1, N.BN, 2 * N.BN - 1, 2 * N.BN, 0, g[1] - 1} <= set(N.planted("edges", g[1], 31))


def test_nonfinite_and_zero_rows_and_self_modes():
    g = (N.BM + 1, 3 * N.BN + 2, N.BK + 1, 31, "slice")
    c = N.exact_case(g, "nonfinite")
    assert c.self_offset == N.SLICE_AT and np.array_equal(c.q.view(np.uint32), c.y[N.SLICE_AT:N.SLICE_AT + g[0]].view(np.uint32))
    y = c.y[:, :c.d]
    assert np.isnan(y).any() and np.isposinf(y).any() and np.isneginf(y).any() and (np.signbit(y) & (y == 0)).any()
    v, i = N.expected(c)
    nan_cols = np.flatnonzero(np.isnan(N.chain(c.q[:1, :c.d], y))[0])
    first = [j for j in nan_cols if j != N.SLICE_AT][:len(i[0])]
    assert len(first) >= 1 and i[0, :len(first)].tolist() == first, "NaN similarities rank first, in row order"
    assert (i != (np.arange(g[0])[:, None] + N.SLICE_AT)).all(), "self is no candidate"
    z = N.exact_case(g[:4] + ("outside",), "zero_row")
    assert z.self_offset == g[1] and (z.y[:, :z.d] == 0).all(axis=1).sum() >= 1 and (z.q[:, :z.d] == 0).all(axis=1).sum() >= 1
    zi = N.expected(z)[1]
    r = int(np.flatnonzero((z.q[:, :z.d] == 0).all(axis=1))[0])
    assert zi[r].tolist() == list(range(31)), "an all-zero query ties with everything: row order"
    short = N.exact_case((5, 30, 7, 31, "zero"), "dense")
    sv, si = N.expected(short)
    assert (si[:, 29:] == -1).all() and (si[:, :29] >= 0).all() and (T.bits(sv[:, 29:]) == 0).all()
    assert N.self_offset_of("none", 3, 9) == -1 and N.self_offset_of("zero", 3, 9) == 0


def test_random_cases_decide_their_ranks():
    """The condition the random cases rest on, asserted on the reference alone: at least 99 % of the (row, rank) pairs have fp64
    gaps to both neighbouring ranks above the sum of their bounds, so exact index equality is asked for almost everywhere."""
    assert {d for _, d in N.RANDOM_SHAPES} == {5, 33, 49, 64} and max(r for r, _ in N.RANDOM_SHAPES) == 1000
    for rows, d in N.RANDOM_SHAPES:
        c = N.random_case(rows, d)
        z = c.z[:, :d].astype(np.float64)
        assert np.abs(z.sum(axis=1)).max() < 1e-5 and np.abs((z * z).sum(axis=1) - 1).max() < 1e-5
        assert c.tau.max() <= (d + 4) * N.U * 1.0001, "Cauchy-Schwarz: sum |q y| <= 1 for unit rows"
        frac = N.decided(c).mean()
        print(f"[neighbors cases] {c.name}: {100 * frac:.2f} % of (row, rank) pairs decided")
        assert frac >= 0.99, (c.name, frac)
        # the fp64 ranking itself passes the checks it is used for
        order, s, _ = N.fp64_ranking(c)
        assert N.check_random(c, s[:, :N.RANDOM_K].astype(np.float32), order[:, :N.RANDOM_K].astype(np.int32)) == frac


def test_the_reference_agrees_with_scipy_and_sklearn():
    from scipy.spatial.distance import cdist
    from sklearn.neighbors import NearestNeighbors
    for rows, d in N.RANDOM_SHAPES:
        c = N.random_case(rows, d)
        x = c.z[:, :d].astype(np.float64)
        dist = cdist(x, x, metric="correlation")
        assert (np.abs((1.0 - dist) - c.sim) <= c.tau).all()
        nn = NearestNeighbors(n_neighbors=N.RANDOM_K + 1, algorithm="brute", metric="correlation").fit(x)
        nd, ni = nn.kneighbors(x)
        order, s, t = N.fp64_ranking(c)
        dec = N.decided(c)
        rowsel = ni[:, 0] == np.arange(rows)                         # sklearn returns the row itself first (distance 0) but for exact duplicates
        assert rowsel.all()
        assert np.array_equal(ni[:, 1:][dec], order[:, :N.RANDOM_K][dec])
        assert (np.abs((1.0 - nd[:, 1:]) - s[:, :N.RANDOM_K]) <= t[:, :N.RANDOM_K] + t[:, 1:N.RANDOM_K + 1]).all()
    # and the chain reference on exact data is the matrix product
    e = N.exact_case((N.BM + 1, 2 * N.BN + 1, N.BK + 1, 30, "none"), "dense")
    assert np.array_equal(N.chain(e.q[:, :e.d], e.y[:, :e.d]), (e.q[:, :e.d].astype(np.float64) @ e.y[:, :e.d].astype(np.float64).T).astype(np.float32))


def test_the_standardize_bound_is_not_vacuous():
    """The forbidden one-pass formula, in fp32, misses the bound on the offset row (x = 1000 + noise) at every d that has a
    variance; the two-pass algorithm in fp32 numpy meets it on every finite row."""
    offset = N.STD_KINDS.index("offset")
    for d in N.STD_DS:
        x = N.std_case(d)[:, :d]
        z, n = N.std_reference(x, True)
        tol_z, tol_n = N.std_bound(x, True)
        finite = np.isfinite(x).all(axis=1)
        assert finite.tolist() == [True, True, True, True, False, False, False, True]
        assert np.isnan(z[~finite]).all() and np.isnan(n[~finite]).all()
        assert (z[2] == 0).all() and n[2] == 0 and (z[3] == 0).all() and n[3] == 0
        if d >= 5:
            err = np.abs(N.one_pass_fp32(x[offset:offset + 1])[0].astype(np.float64) - z[offset])
            assert not (err <= tol_z[offset]).all(), f"d={d}: the one-pass formula passes, the bound is too wide"
            assert 1e-7 < tol_z[offset].max() < 2e-3
        inexact = N.STD_KINDS.index("constant_inexact")
        assert (x[inexact] == N.INEXACT).all() and (z[inexact] == 0).all() and n[inexact] == 0 and (tol_z[inexact] == 0).all()
        plain = finite.copy()
        plain[inexact] = False                                       # plain two-pass arithmetic is not enough for that row: below
        x32 = x[plain].astype(np.float32)
        m = (x32.sum(axis=1, dtype=np.float32) / np.float32(d))[:, None]
        t = x32 - m
        nn = np.sqrt((t * t).sum(axis=1, dtype=np.float32))
        two = t / np.where(nn == 0, np.float32(1), nn)[:, None]
        assert (np.abs(two.astype(np.float64) - z[plain]) <= tol_z[plain] + (nn == 0)[:, None]).all(), d
    # the constant row that needs the header's "all values compare equal" rule: in the kernel's own summation order its fp32
    # mean is not its value at these d, so x - mean is a non-zero constant and norm == 0 alone would not catch the row
    for d in (49, 200):
        assert N.device_mean(np.full(d, N.INEXACT)) != N.INEXACT, d
    assert N.device_mean(np.full(49, 3.0, dtype=np.float32)) == 3.0   # where the other constant row's mean is exact
    zc, nc = N.std_reference(N.std_case(49)[:, :49], False)
    assert abs(np.linalg.norm(zc[2]) - 1) < 1e-12 and nc[3] == 0                       # without centring a constant row is a direction


# ---- 3. the host side of variantformer_amd/neighbors.py ----------------------------------------------------------------------------
def _frame(genes=6, tissues=4, emb=3):
    g = np.random.default_rng(5)
    names = [f"tissue{t}" for t in range(tissues)]
    return pd.DataFrame({"gene_id": [f"ENSG{i:03d}" for i in range(genes)], "tissues": [list(range(tissues))] * genes,
                         "tissue_names": [names] * genes,
                         "predicted_expression": [g.standard_normal((tissues, 1)).astype(np.float32) for _ in range(genes)],
                         "embeddings": [g.standard_normal((tissues, emb)).astype(np.float32) for _ in range(genes)]}), names


def test_from_predictions_builds_the_matrix_and_its_labels():
    from variantformer_amd import neighbors
    df, names = _frame()
    expr = np.stack([np.asarray(v).reshape(-1) for v in df["predicted_expression"]])
    emb = np.stack(list(df["embeddings"]))
    m, labels = neighbors.from_predictions(df)
    assert m.dtype == np.float32 and np.array_equal(m, expr) and labels == list(df["gene_id"])
    m, labels = neighbors.from_predictions(df, axis="tissues")
    assert np.array_equal(m, expr.T) and labels == names and m.flags.c_contiguous
    m, labels = neighbors.from_predictions(df, on="embeddings", tissue="tissue2")
    assert np.array_equal(m, emb[:, 2]) and labels == list(df["gene_id"])
    assert np.array_equal(neighbors.from_predictions(df, on="embeddings", tissue=2)[0], m)
    m, labels = neighbors.from_predictions(df, on="embeddings")
    assert m.shape == (24, 3) and np.array_equal(m, emb.reshape(24, 3)) and labels[5] == ("ENSG001", "tissue1") and len(labels) == 24
    df.at[1, "predicted_expression"] = np.array([1.0, np.nan, 2.0, np.nan], dtype=np.float32)
    assert neighbors.from_predictions(df)[0][1].tolist() == [1.0, 0.0, 2.0, 0.0]
    assert np.isnan(neighbors.from_predictions(df, nan_to_zero=False)[0][1]).sum() == 2
    plain = df.drop(columns=["tissue_names"]).assign(tissues=["a,b,c,d"] * len(df))      # a frame that names its tissues in `tissues`
    assert neighbors.from_predictions(plain, axis="tissues")[1] == ["a", "b", "c", "d"]
    for kw, word in ((dict(on="expression"), "on"), (dict(axis="rows"), "axis"), (dict(tissue="tissue1"), "tissue"),
                     (dict(on="embeddings", axis="tissues"), "axis"), (dict(on="embeddings", tissue="liver"), "liver"),
                     (dict(on="embeddings", tissue=4), "position")):
        with pytest.raises(ValueError, match=word):
            neighbors.from_predictions(df, **kw)
    ragged = df.copy()
    ragged.at[2, "tissue_names"] = names[:3]
    with pytest.raises(ValueError, match="same tissues"):
        neighbors.from_predictions(ragged)
    with pytest.raises(ValueError, match="format_output"):
        neighbors.from_predictions(df.drop(columns=["embeddings"]), on="embeddings")


def test_knn_and_correlation_distance_check_their_arguments_before_the_device():
    from variantformer_amd import neighbors
    x = np.zeros((10, 4), dtype=np.float32)
    for kw, word in ((dict(metric="euclidean"), "metric"), (dict(k=0), "k must"), (dict(k=65), "k must"), (dict(k=2.5), "k must"),
                     (dict(k=True), "k must"), (dict(queries=np.zeros((3, 5), dtype=np.float32)), "columns"),
                     (dict(queries=x[:3], include_self=True), "include_self")):
        with pytest.raises(ValueError, match=word):
            neighbors.knn(x, **kw)
    for bad in (np.zeros(4, dtype=np.float32), np.zeros((4, 0), dtype=np.float32)):
        with pytest.raises(ValueError, match="matrix"):
            neighbors.knn(bad)
        with pytest.raises(ValueError, match="matrix"):
            neighbors.correlation_distance(bad)
    with pytest.raises(TypeError, match="numpy array or a torch tensor"):
        neighbors.knn([[1.0, 2.0]])
    prm = inspect.signature(neighbors.knn).parameters
    assert [(n, p.default) for n, p in prm.items()] == [("x", inspect.Parameter.empty), ("k", 30), ("metric", "correlation"), ("queries", None),
                                                       ("include_self", False), ("nan_to_zero", True)]
    assert "NOT pinned" in neighbors.knn.__doc__ and "umap" in neighbors.knn.__doc__.lower()
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    prm = inspect.signature(VCFProcessor.expression_neighbors).parameters
    assert list(prm)[:6] == ["self", "df", "k", "on", "axis", "tissue"] and prm["k"].default == 30
    if not torch.cuda.is_available():
        with pytest.raises(Exception, match="GPU"):
            neighbors.knn(x, k=3)

"""The forest evaluator without a GPU: the vf_forest_predict boundary (include/vf_hip_forest.h parses, its one name is exported and
bound through _lib.ENTRIES, it has write-set cases in the parallel net), every
refusal of the entry with the argument named, the wrapper that allocates nothing, the converters of variantformer_amd/forest.py
against scikit-learn, and -- on the references alone -- that the float64 restatement of tests/forest_cases.py reproduces the
fixture's scikit-learn probabilities and that the fixture tells right from wrong."""
import inspect
import json
import os
import re

import numpy as np
import pytest

from tests import forest_cases as FC
from tests import write_set_cases as W
from tests.conftest import REPO
from variantformer_amd import forest as Fo

NAME = "vf_forest_predict"


def _header(name="vf_hip_forest.h") -> str:
    with open(os.path.join(REPO, "include", name)) as f:
        return f.read()


# ---- 1. header and binding ---------------------------------------------------------------------------------------------------------
def test_header_parses_and_its_name_is_exported_and_bound():
    """What is this header's own; the boundary every header shares is tests/test_abi_cpu.py's."""
    from variantformer_amd import _lib
    from variantformer_amd.csrc import build as B
    text = _header()
    assert sorted(_lib.ENTRIES["vf_hip_forest.h"]) == [NAME], "ctypes binding and vf_hip_forest.h disagree"
    assert "vf_forest.hip" in B.SOURCES and any(h.endswith("vf_hip_forest.h") for h in B.HEADERS)
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert _lib.ABI_VERSION == 13 and _lib.load().vf_version() == 13
    for word in ("Arguments", "Write set", "Arithmetic", "Non-finite operands", "Refused before anything is launched"):
        assert word in text, f"the comment contract of {NAME} has no `{word}` part"
    assert {f"VF_FOREST_{k.upper()}": v for k, v in Fo.POSTPROCESSORS.items()} == {
        k: int(v) for k, v in re.findall(r"#define\s+(VF_FOREST_[A-Z]+)\s+(\d+)", src)}


def test_the_entry_has_write_set_cases():
    entries = W.stream_entries(_header())
    assert entries == [NAME]
    cases = FC.ws_cases()
    assert {e for c in cases for e in c.entries} == set(entries)
    assert len({c.name for c in cases}) == len(cases)
    for name in FC.WS_GEOMETRIES:
        for form in ("row", "cohort"):
            for how in ("entry", "wrapper"):
                assert any(c.name == FC.ws_name(name, form, how) for c in cases)
    assert all(c.wrappers == (("forest_predict",) if c.name.endswith("wrapper") else ()) for c in cases)
    assert {FC.case(n).bank.postprocessor for n in FC.WS_GEOMETRIES} == set(Fo.POSTPROCESSORS)


def test_the_wrapper_allocates_nothing():
    """As tissue_heads (tests/test_cre_heads_cpu.py): the caller owns every buffer, so `out` is required and keyword-only and no
    allocating call of any spelling stands in the wrapper."""
    from variantformer_amd import ops
    src = inspect.getsource(ops.forest_predict)
    assert not re.search(r"\b(empty|empty_like|zeros|zeros_like|ones|full|new_empty|new_zeros|new_full|tensor|arange|clone|contiguous)\s*\(", src)
    prm = inspect.signature(ops.forest_predict).parameters
    assert list(prm) == ["x", "bank", "model_of_row", "model", "out", "family"]
    assert all(prm[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("model_of_row", "model", "out", "family"))
    assert prm["out"].default is inspect.Parameter.empty
    assert "forest_predict" not in W.allocating_wrappers() and W.uncovered_wrappers() == []


def test_argument_validation_without_gpu():
    """Refused before anything is launched (no GPU here: a launch would fail differently), the argument named."""
    from variantformer_amd import _lib
    lib = _lib.load()
    p = 4096                                             # a non-null, 16-byte aligned address; never dereferenced
    INVALID = 1
    ptrs = ("x", "nodes", "tree_root", "leaf_values", "base_scores", "model_node_base", "model_tree_base", "model_leaf_base",
            "model_n_trees", "out")

    def call(ldx=96, R=0, F=96, M=3, K=2, average=1, post=0, model_of_row=p, model=-1, ldo=2, **kw):
        a = {n: kw.pop(n, p) for n in ptrs}
        assert not kw
        return lib.vf_forest_predict(a["x"], ldx, R, F, a["nodes"], a["tree_root"], a["leaf_values"], a["base_scores"],
                                     a["model_node_base"], a["model_tree_base"], a["model_leaf_base"], a["model_n_trees"], M, K,
                                     average, post, model_of_row, model, a["out"], ldo, 0)

    def err():
        return lib.vf_last_error().decode()
    assert call() == 0                                                                  # the base call is valid (R = 0)
    assert call(model_of_row=0, model=2) == 0                                            # so is the cohort form
    for name in ptrs:
        assert call(**{name: 0}) == INVALID, name
        assert err().endswith(f"null pointer {name}"), err()
        assert call(**{name: p + 2}) == INVALID and re.search(rf"\b{name} must be", err()), err()
    assert call(nodes=p + 4) == INVALID and "nodes must be 16-byte" in err()
    assert call(model_of_row=p + 2) == INVALID and "model_of_row" in err()
    for F in (0, -1, 4097):
        assert call(F=F, ldx=8192) == INVALID and "F=" in err()
    assert call(F=1) == 0 and call(F=4096, ldx=4096) == 0
    for K in (0, -1, 9):
        assert call(K=K, ldo=16) == INVALID and "K=" in err()
    assert call(K=1) == 0 and call(K=8, ldo=8) == 0
    assert call(M=0) == INVALID and "n_models" in err()
    for average in (-1, 2):
        assert call(average=average) == INVALID and "average" in err()
    for post in (-1, 3):
        assert call(post=post) == INVALID and "postprocessor" in err()
    assert call(ldx=95) == INVALID and "ldx" in err()
    assert call(ldo=1) == INVALID and "ldo" in err()
    assert call(model_of_row=p, model=0) == INVALID and "model_of_row" in err() and "both" in err()
    assert call(model_of_row=0, model=-1) == INVALID and "model_of_row" in err() and "neither" in err()
    assert call(R=-1) == INVALID and "R=" in err()
    assert call(R=2 ** 31) == INVALID and "grid" in err()
    assert call(R=0) == 0                                                               # nothing to do: VF_OK, no launch


# ---- 2. the packed format and its converters ---------------------------------------------------------------------------------------
def test_threshold_rounding_decides_like_float64():
    g = np.random.default_rng(5)
    t = np.concatenate([g.normal(size=2000) * 10.0 ** g.integers(-30, 30, 2000), [0.0, -0.0, 1.0, 1e300, -1e300, 1e-60, -1e-60,
                                                                                   np.inf, -np.inf, 0.1, float(np.float32(0.1))]])
    le = Fo.f32_at_or_below(t)
    with pytest.raises(ValueError, match="-inf"):
        Fo.f32_at_or_below(t, strict=True)
    ts = np.where(np.isneginf(t), -1.0, t)                             # the strict rule, on the same values without -inf
    lt = Fo.f32_at_or_below(ts, strict=True)
    assert le.dtype == lt.dtype == np.float32
    up = np.nextafter(le, np.float32(np.inf))
    assert (le.astype(np.float64) <= t).all() and ((up.astype(np.float64) > t) | np.isposinf(le)).all()
    assert (lt.astype(np.float64) < ts).all() and (np.nextafter(lt, np.float32(np.inf)).astype(np.float64) >= ts).all()
    # for float32 x around the threshold: x <= le  <=>  x <= t (float64), x <= lt  <=>  x < t
    for k in (-2, -1, 0, 1, 2):
        x = le.copy()
        for _ in range(abs(k)):
            x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
        assert np.array_equal(x <= le, x.astype(np.float64) <= t)
        x = lt.copy()
        for _ in range(abs(k)):
            x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
        assert np.array_equal(x <= lt, x.astype(np.float64) < ts)
    changed = (t.astype(np.float32).astype(np.float64) > t).sum()
    assert changed > 500                                               # round-to-nearest would have gone above these
    with pytest.raises(ValueError, match="NaN"):
        Fo.f32_at_or_below([0.0, np.nan])


def test_packed_forest_refuses_what_a_walk_cannot_survive():
    m = FC.make_forest(1, 3, 4, 2, depth=3)
    kw = {k: getattr(m, k).copy() for k in Fo.PackedForest.ARRAYS}
    inner = int(np.flatnonzero(m.feature >= 0)[0])

    def build(**over):
        return Fo.PackedForest(**{**kw, **over}, n_features=4, average=True)
    build()
    bad = kw["left"].copy()
    bad[inner] = inner                                                 # a node that is its own child: the walk would not end
    with pytest.raises(ValueError, match="above the node's own index"):
        build(left=bad)
    bad = kw["right"].copy()
    bad[inner] = m.n_nodes
    with pytest.raises(ValueError, match="inside the model"):
        build(right=bad)
    bad = kw["feature"].copy()
    bad[inner] = 4
    with pytest.raises(ValueError, match="feature"):
        build(feature=bad)
    bad = kw["left"].copy()
    bad[m.feature < 0] = m.leaf_values.shape[0]
    with pytest.raises(ValueError, match="row of leaf_values"):
        build(left=bad)
    with pytest.raises(ValueError, match="tree_root"):
        build(tree_root=np.array([m.n_nodes]))
    with pytest.raises(ValueError, match="K in 1 .. 8"):
        build(leaf_values=np.zeros((m.leaf_values.shape[0], 9)), base_scores=np.zeros(9))
    with pytest.raises(ValueError, match="postprocessor"):
        Fo.PackedForest(**kw, n_features=4, average=True, postprocessor="exp")
    with pytest.raises(ValueError, match="n_features"):
        Fo.PackedForest(**kw, n_features=4097, average=True)


def test_npz_round_trip_and_load(tmp_path):
    m = FC.make_forest(2, 5, 16, 3, depth=4, average=False, postprocessor="softmax")
    m.save(str(tmp_path / "m.npz"))
    back = Fo.load(str(tmp_path / "m.npz"))
    for k in Fo.PackedForest.ARRAYS:
        assert np.array_equal(getattr(m, k), getattr(back, k)) and getattr(m, k).dtype == getattr(back, k).dtype
    assert (back.n_features, back.average, back.postprocessor) == (16, False, "softmax")
    nodes = m.nodes16()
    assert nodes.dtype == np.int32 and nodes.shape == (m.n_nodes, 4) and nodes.flags.c_contiguous
    inner = m.feature >= 0
    assert (nodes[~inner, 0] == -1).all() and np.array_equal(nodes[inner, 0] & 0xFFFF, m.feature[inner])
    assert np.array_equal((nodes[inner, 0] >> 16) & 1, m.default_left[inner]) and np.array_equal(nodes[:, 1].view(np.float32), m.threshold)
    wide = m.with_n_features(1536)
    x = FC.make_rows(3, 9, 16)
    assert wide.n_features == 1536 and np.array_equal(wide.predict_host(np.pad(x, ((0, 0), (0, 1520)))), m.predict_host(x))
    with pytest.raises(ValueError, match="not a .npz, .json or .tl"):
        Fo.load(str(tmp_path / "m.bin"))


def test_load_tl_without_treelite_names_what_is_missing(tmp_path):
    try:
        import treelite  # noqa: F401
        pytest.skip("treelite is installed: the .tl branch would run")
    except ImportError:
        pass
    (tmp_path / "m.tl").write_bytes(b"")
    with pytest.raises(ImportError) as e:
        Fo.load(str(tmp_path / "m.tl"))
    msg = str(e.value)
    assert "treelite" in msg and ".json" in msg and ".npz" in msg
    doc = " ".join(Fo.__doc__.split())
    assert "UNPINNED" in doc and "AS REMEMBERED" in doc and "UNPINNED" in Fo.from_treelite_json.__doc__ and "UNPINNED" in Fo.load.__doc__


TREELITE_JSON = {
    "num_feature": 3, "average_tree_output": True, "postprocessor": "identity_multiclass", "num_class": [2],
    "leaf_vector_shape": [1, 2], "base_scores": [0.0, 0.0],
    "trees": [
        {"nodes": [                                                     # numbered breadth first: renumbered in preorder
            {"node_id": 0, "split_feature_id": 0, "default_left": True, "comparison_op": "<", "threshold": 0.5, "left_child": 1,
             "right_child": 2},
            {"node_id": 1, "split_feature_id": 1, "default_left": False, "comparison_op": "<=", "threshold": 0.1, "left_child": 3,
             "right_child": 4},
            {"node_id": 2, "leaf_value": [0.25, 0.75]},
            {"node_id": 3, "leaf_value": [1.0, 0.0]},
            {"node_id": 4, "leaf_value": [0.5, 0.5]}]},
        {"nodes": [
            {"node_id": 0, "split_feature_id": 2, "default_left": True, "comparison_op": ">=", "threshold": 2.0, "left_child": 1,
             "right_child": 2},
            {"node_id": 1, "leaf_value": [0.0, 1.0]},
            {"node_id": 2, "leaf_value": [0.75, 0.25]}]}]}


def test_from_treelite_json_on_a_handwritten_model(tmp_path):
    m = Fo.from_treelite_json(TREELITE_JSON)
    assert (m.n_trees, m.n_features, m.n_outputs, m.average, m.postprocessor) == (2, 3, 2, True, "identity")
    assert m.tree_root.tolist() == [0, 5] and m.feature.tolist() == [0, 1, -1, -1, -1, 2, -1, -1]
    # `< 0.5`: the largest float32 below 0.5;  `<= 0.1`: the largest float32 at or below the float64 0.1;  `>= 2`: children swapped
    # and the threshold as for `<`, default_left flipped with them
    assert m.threshold[0] == np.nextafter(np.float32(0.5), np.float32(0)) and m.threshold[1] == np.nextafter(np.float32(0.1), np.float32(0))
    assert float(np.float32(0.1)) > 0.1 and m.threshold[5] == np.nextafter(np.float32(2.0), np.float32(0))
    assert m.default_left.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    f32 = np.float32
    x = np.array([[0.4, 0.0, 3.0], [0.5, 0.0, 2.0], [np.nextafter(f32(0.5), f32(0)), f32(0.1), np.nextafter(f32(2), f32(0))],
                  [np.nan, np.nan, np.nan], [0.0, np.nextafter(f32(0.1), f32(0)), np.nan]], dtype=np.float32)

    def tree0(a, b):                                                   # the handwritten semantics, in float64
        if np.isnan(a) or float(a) < 0.5:
            return [0.5, 0.5] if (np.isnan(b) or not float(b) <= 0.1) else [1.0, 0.0]
        return [0.25, 0.75]

    def tree1(c):
        return [0.0, 1.0] if (np.isnan(c) or float(c) >= 2.0) else [0.75, 0.25]
    want = np.array([(np.array(tree0(r[0], r[1])) + np.array(tree1(r[2]))) / 2 for r in x])
    assert np.array_equal(m.predict_host(x), want) and np.array_equal(FC.predict64(m, x)[0], want)
    with open(tmp_path / "m.json", "w") as f:
        json.dump(TREELITE_JSON, f)
    assert np.array_equal(Fo.load(str(tmp_path / "m.json")).nodes16(), m.nodes16())
    loop = json.loads(json.dumps(TREELITE_JSON))
    loop["trees"][0]["nodes"][1]["left_child"] = 0
    with pytest.raises(ValueError, match="reached twice"):
        Fo.from_treelite_json(loop)
    # one scalar tree per class: K-vectors that are zero outside the tree's class
    ova = {"num_feature": 1, "average_tree_output": False, "postprocessor": "softmax", "num_class": [3], "leaf_vector_shape": [1, 1],
           "base_scores": [0.5], "class_id": [0, 2],
           "trees": [{"nodes": [{"node_id": 0, "leaf_value": 1.5}]}, {"nodes": [{"node_id": 0, "leaf_value": -2.0}]}]}
    m3 = Fo.from_treelite_json(ova)
    assert m3.leaf_values.tolist() == [[1.5, 0.0, 0.0], [0.0, 0.0, -2.0]] and m3.base_scores.tolist() == [0.5, 0.5, 0.5]


def test_forest_bank_concatenates_and_refuses(monkeypatch):
    ms = [FC.make_forest(10 + i, T, 8, 2, depth=3) for i, T in enumerate((3, 1, 7))]
    b = Fo.ForestBank(ms)
    assert b.n_models == 3 and b.model_n_trees.tolist() == [3, 1, 7]
    assert b.model_node_base.tolist() == [0, ms[0].n_nodes, ms[0].n_nodes + ms[1].n_nodes]
    assert b.model_tree_base.tolist() == [0, 3, 4] and b.model_leaf_base.tolist()[1] == ms[0].leaf_values.shape[0]
    assert b.nodes.shape == (sum(m.n_nodes for m in ms), 4) and b.base_scores.shape == (3, 2)
    for a in (getattr(b, k) for k in Fo.ForestBank.ARRAYS):
        assert a.dtype in (np.int32, np.float32)
    for other, word in ((FC.make_forest(1, 2, 8, 3), "n_outputs"), (FC.make_forest(1, 2, 9, 2), "n_features"),
                        (FC.make_forest(1, 2, 8, 2, average=False), "average"),
                        (FC.make_forest(1, 2, 8, 2, postprocessor="sigmoid"), "postprocessor")):
        with pytest.raises(ValueError, match=word):
            Fo.ForestBank([ms[0], other])
    with pytest.raises(ValueError, match="at least one"):
        Fo.ForestBank([])
    assert Fo.MAX_BANK_NODES == 2 ** 31 - 1
    monkeypatch.setattr(Fo, "MAX_BANK_NODES", b.nodes.shape[0] - 1)    # (a bank of 2^31 nodes is 32 GiB: the rule, at a size a test can hold)
    with pytest.raises(ValueError, match="int32 indices"):
        Fo.ForestBank(ms)


def _fit(kind):
    from sklearn.ensemble import ExtraTreesClassifier, GradientBoostingClassifier, RandomForestClassifier
    g = np.random.default_rng({"rf": 1, "et": 2, "gb": 3}[kind])
    x = g.normal(size=(300, 20)).astype(np.float32)
    x[:, ::2] = np.round(x[:, ::2] * 4) / 4
    score = x[:, 0] + x[:, 1] * x[:, 2]
    n_classes = 3 if kind == "et" else 2
    y = np.digitize(score, np.quantile(score, np.arange(1, n_classes) / n_classes))
    est = {"rf": RandomForestClassifier(24, max_depth=6, random_state=0), "et": ExtraTreesClassifier(12, max_depth=5, random_state=0),
           "gb": GradientBoostingClassifier(n_estimators=20, max_depth=3, random_state=0)}[kind].fit(x, y)
    xt = g.normal(size=(400, 20)).astype(np.float32)
    xt[:, ::2] = np.round(xt[:, ::2] * 4) / 4
    return est, xt


@pytest.mark.parametrize("kind", ["rf", "et", "gb"])
def test_from_sklearn_reproduces_apply_and_predict_proba(kind):
    pytest.importorskip("sklearn")
    est, x = _fit(kind)
    m = Fo.from_sklearn(est)
    trees = est.estimators_[:, 0] if kind == "gb" else est.estimators_
    thr64 = np.concatenate([np.where(t.tree_.children_left < 0, 0.0, t.tree_.threshold) for t in trees])
    inner = m.feature >= 0
    # rows ON every threshold that rounding to nearest would move up: the float32 above the threshold goes right in scikit-learn
    near = thr64.astype(np.float32)
    up = np.flatnonzero(inner & (near.astype(np.float64) > thr64))
    on = x[np.arange(len(up)) % len(x)].copy()
    on[np.arange(len(up)), m.feature[up]] = near[up]
    x = np.concatenate([x, on])
    if kind != "gb":                                                   # scikit-learn's boosted model takes no NaN
        x[::7, ::3] = np.nan
    print(f"[forest sklearn {kind}] {int((m.threshold[inner].astype(np.float64) != thr64[inner]).sum())} of {int(inner.sum())} thresholds "
          f"change under the rule, {len(up)} of them would round up")
    assert np.array_equal(m.leaves_of(x) - m.tree_root[None], est.apply(x).reshape(len(x), -1))
    assert np.array_equal(FC.walk(m, x[:40]), m.leaves_of(x[:40]))                        # the two host walks agree
    want = est.predict_proba(x)
    out, bound = FC.predict64(m, x[:120])
    assert (np.abs(out - want[:120]) <= bound).all()
    assert (m.n_outputs, m.average, m.postprocessor) == ((3, True, "identity") if kind == "et" else (2, True, "identity") if kind == "rf"
                                                         else (2, False, "sigmoid"))
    assert np.abs(m.predict_host(x) - want).max() < 1e-6
    if len(up):
        wrong = FC.walk(m, on[:40], "nearest", thr64)
        assert not np.array_equal(wrong, m.leaves_of(on[:40]))          # rounding to nearest is caught on these rows


def test_from_sklearn_refuses_what_it_does_not_know():
    pytest.importorskip("sklearn")
    from sklearn.ensemble import GradientBoostingClassifier
    from sklearn.tree import DecisionTreeClassifier
    g = np.random.default_rng(0)
    x, y = g.normal(size=(60, 4)), g.integers(0, 3, 60)
    with pytest.raises(TypeError, match="DecisionTreeClassifier"):
        Fo.from_sklearn(DecisionTreeClassifier().fit(x, y))
    with pytest.raises(ValueError, match="binary"):
        Fo.from_sklearn(GradientBoostingClassifier(n_estimators=2).fit(x, y))


# ---- 3. the fixture ----------------------------------------------------------------------------------------------------------------
def test_fixture_covers_what_it_should():
    fx = FC.load_ad_risk()
    assert tuple(fx) == FC.FIXTURE_MODELS
    want = {"rf": (2, True, "identity"), "et": (3, True, "identity"), "gb": (2, False, "sigmoid")}
    for name, f in fx.items():
        m = f["model"]
        assert (m.n_outputs, m.average, m.postprocessor) == want[name]
        assert m.n_trees <= 32 and m.n_features <= 96 and f["x"].dtype == np.float32 and f["proba"].dtype == np.float64
        assert f["proba"].shape == (f["x"].shape[0], m.n_outputs) and np.isfinite(f["proba"]).all()
        inner = m.feature >= 0
        assert np.array_equal(m.threshold[inner], Fo.f32_at_or_below(f["thr64"][inner]))
        # rows fall exactly on thresholds, and every threshold that rounds UP to its nearest float32 has a row on that float32
        on = sum(int((f["x"][:, m.feature[n]] == m.threshold[n]).any()) for n in np.flatnonzero(inner))
        assert on >= m.n_trees // 2
        near = f["thr64"].astype(np.float32)
        up = np.flatnonzero(inner & (near.astype(np.float64) > f["thr64"]))
        assert len(up) >= 20 and all((f["x"][:, m.feature[n]] == near[n]).any() for n in up)
        assert bool(np.isnan(f["x"]).any()) == (name != "gb")
    assert os.path.getsize(os.path.join(FC.GOLDEN, "ad_risk.npz")) < 200_000


@pytest.mark.parametrize("name", FC.FIXTURE_MODELS)
def test_float64_restatement_reproduces_the_fixture(name):
    f = FC.load_ad_risk()[name]
    out, bound = FC.predict64(f["model"], f["x"])
    assert float(bound.min()) > 0
    err = np.abs(out - f["proba"])
    print(f"[forest fixture {name}] largest error {float((err / bound).max()):.4f} of the bound")
    assert bool((err <= bound).all())
    assert np.array_equal(f["model"].leaves_of(f["x"]), FC.walk(f["model"], f["x"]))


@pytest.mark.parametrize("name", FC.FIXTURE_MODELS)
def test_the_fixture_tells_right_from_wrong(name):
    """A condition on the references: each wrong variant differs from scikit-learn's probabilities by more than 100 bounds in at
    least three quarters of the rows -- `nearest` in at least 8 rows, `no_default` in every row that holds a NaN."""
    f = FC.load_ad_risk()[name]
    _, bound = FC.predict64(f["model"], f["x"])
    variants = FC.wrong_variants(f)
    assert tuple(variants) == FC.VARIANTS
    assert (variants["no_average"] is not None) == f["model"].average and (variants["no_default"] is not None) == (name != "gb")
    for kind, wrong in variants.items():
        if wrong is None:
            continue
        off = FC.rows_off(wrong, f, bound)
        rows, need = FC.variant_need(kind, f)
        got = int(off.sum() if rows is None else (off & rows).sum())
        print(f"[forest fixture {name}] {kind}: {got} of {off.size} rows differ by more than 100 bounds (needed: {need})")
        assert need >= (8 if kind == "nearest" else 1) and got >= need, (kind, got, need)


def test_the_geometries_cover_the_kernel_paths():
    seen = {k: set() for k in ("T", "F", "K", "R", "M", "post")}
    for name, trees, F, K, R, average, post, depth in FC.GEOMETRIES:
        seen["T"].update(trees), seen["F"].add(F), seen["K"].add(K), seen["R"].add(R), seen["M"].add(len(trees)), seen["post"].add(post)
    assert seen == {"T": {1, 5, 64, 65, 130}, "F": {4, 96, 1536}, "K": {1, 2, 3, 8}, "R": {1, 5, 67}, "M": {1, 2, 4},
                    "post": {"identity", "sigmoid", "softmax"}}
    leaf = FC.case("leaf")
    m = leaf.models[0]
    assert m.feature[m.tree_root[2]] == -1 and (m.feature[m.tree_root[[0, 1, 3, 4]]] >= 0).all()   # a tree that is a single leaf
    assert len(set(next(g for g in FC.GEOMETRIES if g[0] == "bank4")[1])) == 4 and FC.EXTRA_LDX > 0 and FC.EXTRA_LDO > 0
    c = FC.case("bank4")
    assert len(set(c.model_of_row.tolist())) == 4 and np.isnan(c.x).any()
    on = sum(int((c.x[:, m.feature[n]] == m.threshold[n]).any()) for m in c.models for n in np.flatnonzero(m.feature >= 0))
    assert on > 20                                                      # seeded rows sit on seeded thresholds (the 1/4 grid)

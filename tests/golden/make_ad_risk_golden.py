"""Writes tests/golden/ad_risk.npz / .json: three small scikit-learn models in the packed form of variantformer_amd/forest.py,
test rows, and scikit-learn's own predict_proba on those rows.  Needs scikit-learn (the tests that read the fixture do not).

    python -m tests.golden.make_ad_risk_golden

Models (<= 32 trees, depth <= 7, F <= 96): `rf` RandomForestClassifier, 2 classes; `et` ExtraTreesClassifier, 3 classes; `gb`
GradientBoostingClassifier, binary.  Half the features of the training data lie on a 1/4 grid, half are continuous, so a good
part of the thresholds (midpoints of two float32 values, held in float64) are no float32.

Rows, per model:
  * seeded rows like the training data;
  * for EVERY threshold whose round-to-nearest float32 lies above it, one row holds that float32 in the threshold's feature
    (scikit-learn sends it right; a converter that rounds to nearest sends it left).  The rows are shared: a row takes one such
    value per feature.  The shallowest of these nodes also get a row of their own, steered down the path to the node (each
    ancestor's feature on its threshold, or on the next float32 above it), so that a converter that rounds to nearest shows
    in enough rows;
  * rf / et: rows with NaN in the features of tree roots (scikit-learn's missing_go_to_left decides them; its boosted model
    takes no NaN);
  * every row then gets the (rounded-down) threshold of the roots of the first trees in the roots' features, where the row
    has nothing placed yet: the walk is decided by `<=` against `<` at the first node.
The fixture is written only if the wrong variants of tests/forest_cases.py are told from scikit-learn's values as
tests/test_forest_cpu.py demands.
"""
import json
import os

import numpy as np

from tests import forest_cases as FC
from variantformer_amd import forest as Fo

HERE = os.path.dirname(os.path.abspath(__file__))
N_TRAIN, N_BASE, N_NAN, N_ROOTS, N_STEERED = 400, 24, 12, 6, 16


def _data(g, n, F):
    x = g.normal(size=(n, F)).astype(np.float32)
    x[:, ::2] = np.round(x[:, ::2] * 4) / 4
    return x


def _thr64(est, kind) -> np.ndarray:
    trees = est.estimators_[:, 0] if kind == "gb" else est.estimators_
    return np.concatenate([np.where(t.tree_.children_left < 0, 0.0, t.tree_.threshold) for t in trees])


def _depths(m) -> np.ndarray:
    d = np.zeros(m.n_nodes, dtype=np.int64)
    for n in range(m.n_nodes):                                  # children lie above their parent
        if m.feature[n] >= 0:
            d[m.left[n]] = d[m.right[n]] = d[n] + 1
    return d


def _rows(g, m, thr64, F, with_nan):
    base = _data(g, N_BASE, F)
    taken = np.zeros(base.shape, dtype=bool)
    inner = np.flatnonzero(m.feature >= 0)
    near = thr64.astype(np.float32)
    up = inner[near[inner].astype(np.float64) > thr64[inner]]            # nearest float32 above the threshold
    up = up[np.argsort(_depths(m)[up], kind="stable")]
    rows, marks = [], []
    parent = {}
    for n in inner:
        parent[m.left[n]], parent[m.right[n]] = (n, True), (n, False)
    for n in up[:N_STEERED]:                                    # a row of its own, steered down the path to the node
        x, t = _data(g, 1, F)[0], np.zeros(F, dtype=bool)
        x[m.feature[n]], t[m.feature[n]] = near[n], True
        c = n
        while c in parent:
            c, go_left = parent[c]
            f = m.feature[c]
            if not t[f]:
                x[f], t[f] = (m.threshold[c] if go_left else np.nextafter(m.threshold[c], np.float32(np.inf))), True
        rows.append(x), marks.append(t)
    for n in up:
        f = m.feature[n]
        for x, t in zip(rows, marks):
            if not t[f]:
                break
        else:
            x, t = _data(g, 1, F)[0], np.zeros(F, dtype=bool)
            rows.append(x), marks.append(t)
        x[f], t[f] = near[n], True
    x = np.concatenate([base, np.array(rows).reshape(-1, F)])
    taken = np.concatenate([taken, np.array(marks).reshape(-1, F)])
    if with_nan:
        nan_rows = _data(g, N_NAN, F)
        nan_taken = np.zeros(nan_rows.shape, dtype=bool)
        roots_dl = [r for r in m.tree_root if m.feature[r] >= 0 and m.default_left[r]]
        for i in range(N_NAN):
            for r in (roots_dl[(3 * i + j) % len(roots_dl)] for j in range(3)):
                nan_rows[i, m.feature[r]] = np.nan
                nan_taken[i, m.feature[r]] = True
        x, taken = np.concatenate([x, nan_rows]), np.concatenate([taken, nan_taken])
    for i in range(x.shape[0]):
        for r in m.tree_root[(np.arange(N_ROOTS) + i) % m.n_trees]:
            f = m.feature[r]
            if f >= 0 and not taken[i, f]:
                x[i, f], taken[i, f] = m.threshold[r], True
    return np.ascontiguousarray(x, dtype=np.float32), int(len(up))


def main():
    import sklearn
    from sklearn.ensemble import ExtraTreesClassifier, GradientBoostingClassifier, RandomForestClassifier
    specs = {"rf": (RandomForestClassifier(n_estimators=24, max_depth=6, random_state=11), 24, 2),
             "et": (ExtraTreesClassifier(n_estimators=16, max_depth=5, random_state=12), 96, 3),
             "gb": (GradientBoostingClassifier(n_estimators=32, max_depth=3, random_state=13), 16, 2)}
    arrays, meta = {}, {"sklearn": sklearn.__version__, "models": {}}
    for seed, (name, (est, F, n_classes)) in enumerate(specs.items()):
        g = np.random.default_rng(4100 + seed)
        xt = _data(g, N_TRAIN, F)
        score = xt[:, 0] + xt[:, 1] * xt[:, 2] - 0.5 * xt[:, 3] + 0.3 * g.normal(size=N_TRAIN)
        y = np.digitize(score, np.quantile(score, np.arange(1, n_classes) / n_classes))
        est.fit(xt, y)
        m = Fo.from_sklearn(est)
        thr64 = _thr64(est, name)
        x, n_up = _rows(g, m, thr64, F, with_nan=name != "gb")
        proba = est.predict_proba(x)
        f = dict(model=m, thr64=thr64, x=x, proba=proba)
        # the conditions of tests/test_forest_cpu.py, before anything is written
        apply_ = est.apply(x).reshape(len(x), -1)
        assert np.array_equal(m.leaves_of(x) - m.tree_root[None], apply_), "a leaf differs from estimator.apply"
        out, bound = FC.predict64(m, x)
        assert (np.abs(out - proba) <= bound).all(), "the float64 restatement misses scikit-learn's probabilities"
        inner = m.feature >= 0
        near = thr64.astype(np.float32)
        for n in np.flatnonzero(inner & (near.astype(np.float64) > thr64)):
            assert (x[:, m.feature[n]] == near[n]).any(), "a threshold that rounds up has no row on its float32"
        told = {}
        for kind, wrong in FC.wrong_variants(f).items():
            if wrong is None:
                continue
            off = FC.rows_off(wrong, f, bound)
            rows, need = FC.variant_need(kind, f)
            got = int(off.sum() if rows is None else (off & rows).sum())
            assert got >= need, (name, kind, got, need)
            told[kind] = got
        arrays.update(m.to_arrays(f"{name}."))
        arrays.update({f"{name}.thr64": thr64, f"{name}.x": x, f"{name}.proba": proba})
        meta["models"][name] = dict(estimator=type(est).__name__, params={k: v for k, v in est.get_params().items()
                                                                           if k in ("n_estimators", "max_depth", "random_state")},
                                    n_features=F, n_classes=n_classes, n_trees=m.n_trees, n_nodes=m.n_nodes, n_rows=int(len(x)),
                                    n_rows_with_nan=int(np.isnan(x).any(axis=1).sum()), thresholds_changed=int(
                                        (m.threshold[inner].astype(np.float64) != thr64[inner]).sum()),
                                    thresholds_nearest_above=n_up, rows_told_from_variant=told)
        print(name, meta["models"][name])
    np.savez_compressed(os.path.join(HERE, "ad_risk.npz"), **arrays)
    with open(os.path.join(HERE, "ad_risk.json"), "w") as fjson:
        json.dump(meta, fjson, indent=1)
    print(os.path.getsize(os.path.join(HERE, "ad_risk.npz")), "bytes")


if __name__ == "__main__":
    main()

"""Decision forests on embeddings: the packed format behind ops.forest_predict (vf_forest_predict, include/vf_hip_forest.h),
its converters and the bank that holds many models on the device.  Host code; only ForestBank.to() touches a device.

The reference (processors/ad_risk.py) keeps one treelite model per (gene, tissue) and calls treelite.gtil.predict per row.
Here a model is a PackedForest -- flat arrays, one comparison -- and M of them are concatenated into a ForestBank whose
device image one launch evaluates.

ONE COMPARISON: a walk goes left iff x <= threshold, both fp32.  The converters make that exact instead of approximate: a
float64 threshold t with operator `<=` becomes the largest float32 <= t, with `<` the largest float32 < t.  For a float32 x,
x <= t (in float64, what scikit-learn and treelite evaluate) holds exactly when x <= that float32, so every decision, and
with it every leaf, is the source model's bit for bit.  Rounding t to the NEAREST float32 does not have this property: where
the nearest float32 lies above t, a feature equal to it goes left here and right in the source.

What is pinned and what is not: the packed semantics are pinned to scikit-learn (tests/golden/ad_risk.*,
tests/test_forest_cpu.py).  treelite is not a dependency and no treelite file was available when this was written:
`from_treelite_json` reads the field names of treelite 4.x's Model.dump_as_json() AS REMEMBERED (num_feature,
average_tree_output, postprocessor, base_scores, num_class, leaf_vector_shape, class_id; per tree `nodes` with node_id,
split_feature_id, threshold, comparison_op, default_left, left_child, right_child, leaf_value) and is tested on a handwritten
JSON only; the `.tl` branch of `load` (treelite.Model.deserialize(path).dump_as_json()) has never run.  Both are UNPINNED.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass

import numpy as np

POSTPROCESSORS = {"identity": 0, "sigmoid": 1, "softmax": 2}        # VF_FOREST_* of include/vf_hip_forest.h
MAX_FEATURES, MAX_OUTPUTS = 4096, 8
MAX_BANK_NODES = 2 ** 31 - 1


def f32_at_or_below(t, strict: bool = False) -> np.ndarray:
    """The largest float32 <= t (strict: < t) of float64 thresholds: x <= result, in fp32, is x <= t (x < t) in float64 for
    every float32 x.  A threshold below every finite float32 gives -inf (nothing but -inf goes left)."""
    t = np.asarray(t, dtype=np.float64)
    if np.isnan(t).any():
        raise ValueError("a NaN threshold has no float32 that decides like it")
    if strict and np.isneginf(t).any():
        raise ValueError("`x < -inf` holds for no x: no float32 threshold decides like it")
    with np.errstate(over="ignore"):
        c = t.astype(np.float32)
    above = (c.astype(np.float64) >= t) if strict else (c.astype(np.float64) > t)
    return np.where(above, np.nextafter(c, np.float32(-np.inf)), c).astype(np.float32)


@dataclass
class PackedForest:
    """One model as flat arrays.  Per node: feature int32 (-1: a leaf), threshold fp32, left / right int32 (node indices
    inside this model; a leaf's `left` is its row in leaf_values), default_left uint8 (where a NaN feature goes).  tree_root
    int32 [T]; leaf_values fp32 [n_leaves, K]; base_scores fp32 [K].  Output k of a row = postprocessor((sum over the trees
    of the row's leaf, divided by T if `average`) + base_scores[k]).  Every child index is above its parent's, so a walk
    ends: validate() refuses anything else."""
    feature: np.ndarray
    threshold: np.ndarray
    left: np.ndarray
    right: np.ndarray
    default_left: np.ndarray
    tree_root: np.ndarray
    leaf_values: np.ndarray
    base_scores: np.ndarray
    n_features: int
    average: bool
    postprocessor: str = "identity"

    def __post_init__(self):
        self.feature = np.ascontiguousarray(self.feature, dtype=np.int32)
        self.threshold = np.ascontiguousarray(self.threshold, dtype=np.float32)
        self.left = np.ascontiguousarray(self.left, dtype=np.int32)
        self.right = np.ascontiguousarray(self.right, dtype=np.int32)
        self.default_left = np.ascontiguousarray(self.default_left, dtype=np.uint8)
        self.tree_root = np.ascontiguousarray(self.tree_root, dtype=np.int32)
        self.leaf_values = np.ascontiguousarray(self.leaf_values, dtype=np.float32)
        self.base_scores = np.ascontiguousarray(self.base_scores, dtype=np.float32)
        self.n_features, self.average = int(self.n_features), bool(self.average)
        self.validate()

    @property
    def n_nodes(self) -> int:
        return int(self.feature.shape[0])

    @property
    def n_trees(self) -> int:
        return int(self.tree_root.shape[0])

    @property
    def n_outputs(self) -> int:
        return int(self.leaf_values.shape[1])

    def validate(self) -> "PackedForest":
        n, K = self.n_nodes, self.leaf_values.shape[1] if self.leaf_values.ndim == 2 else -1
        if self.postprocessor not in POSTPROCESSORS:
            raise ValueError(f"postprocessor {self.postprocessor!r} is not one of {sorted(POSTPROCESSORS)}")
        if not 1 <= self.n_features <= MAX_FEATURES:
            raise ValueError(f"n_features={self.n_features} outside 1 .. {MAX_FEATURES}")
        if not 1 <= K <= MAX_OUTPUTS:
            raise ValueError(f"leaf_values must be [n_leaves, K] with K in 1 .. {MAX_OUTPUTS}, not {self.leaf_values.shape}")
        if self.base_scores.shape != (K,):
            raise ValueError(f"base_scores must be [{K}], not {self.base_scores.shape}")
        for name in ("threshold", "left", "right", "default_left"):
            if getattr(self, name).shape != (n,):
                raise ValueError(f"{name} must have one entry per node ({n}), not {getattr(self, name).shape}")
        if self.n_trees < 1 or n < 1:
            raise ValueError("a forest has at least one tree")
        if self.tree_root.min() < 0 or self.tree_root.max() >= n:
            raise ValueError("tree_root names a node outside the model")
        leaf = self.feature < 0
        inner = ~leaf
        if (self.feature[inner] >= self.n_features).any() or (self.feature[leaf] != -1).any():
            raise ValueError("feature must be -1 (a leaf) or lie in 0 .. n_features-1")
        idx = np.arange(n)
        for name in ("left", "right"):
            c = getattr(self, name)[inner]
            if (c <= idx[inner]).any() or (c >= n).any():
                raise ValueError(f"`{name}` of an inner node must lie above the node's own index and inside the model")
        if np.isnan(self.threshold[inner]).any():
            raise ValueError("a NaN threshold")
        if leaf.any() and (self.left[leaf].min() < 0 or self.left[leaf].max() >= self.leaf_values.shape[0]):
            raise ValueError("a leaf's `left` must be a row of leaf_values")
        if (self.default_left > 1).any():
            raise ValueError("default_left must be 0 or 1")
        return self

    def nodes16(self) -> np.ndarray:
        """int32 [n_nodes, 4]: the 16-byte nodes of include/vf_hip_forest.h."""
        w0 = np.where(self.feature < 0, np.int32(-1), self.feature | (self.default_left.astype(np.int32) << 16)).astype(np.int32)
        return np.ascontiguousarray(np.stack([w0, self.threshold.view(np.int32), self.left, self.right], axis=1))

    def leaves_of(self, X: np.ndarray) -> np.ndarray:
        """int64 [n, T]: the node at which each row's walk of each tree ends (host; the kernel's decisions on float32 X)."""
        X = np.ascontiguousarray(X, dtype=np.float32)
        assert X.ndim == 2 and X.shape[1] >= self.n_features
        n = X.shape[0]
        node = np.broadcast_to(self.tree_root.astype(np.int64), (n, self.n_trees)).copy()
        rows = np.arange(n)[:, None]
        while True:
            f = self.feature[node]
            live = f >= 0
            if not live.any():
                return node
            v = X[rows, np.where(live, f, 0)]
            go_left = np.where(np.isnan(v), self.default_left[node] != 0, v <= self.threshold[node])
            node = np.where(live, np.where(go_left, self.left[node], self.right[node]), node)

    def predict_host(self, X: np.ndarray) -> np.ndarray:
        """float64 [n, K]: the packed semantics on the host (decisions in fp32 as on the device, sums in float64)."""
        leaves = self.left[self.leaves_of(X)]
        v = self.leaf_values.astype(np.float64)[leaves].sum(axis=1)
        if self.average:
            v = v / self.n_trees
        v = v + self.base_scores.astype(np.float64)
        if self.postprocessor == "sigmoid":
            return 1.0 / (1.0 + np.exp(-v))
        if self.postprocessor == "softmax":
            e = np.exp(v - v.max(axis=1, keepdims=True))
            return e / e.sum(axis=1, keepdims=True)
        return v

    def with_n_features(self, n_features: int) -> "PackedForest":
        """The same model declared for wider rows (the features it tests keep their columns)."""
        return PackedForest(self.feature, self.threshold, self.left, self.right, self.default_left, self.tree_root,
                            self.leaf_values, self.base_scores, n_features, self.average, self.postprocessor)

    ARRAYS = ("feature", "threshold", "left", "right", "default_left", "tree_root", "leaf_values", "base_scores")

    def to_arrays(self, prefix: str = "") -> dict:
        out = {prefix + k: getattr(self, k) for k in self.ARRAYS}
        out[prefix + "meta"] = np.array([self.n_features, int(self.average), POSTPROCESSORS[self.postprocessor]], dtype=np.int32)
        return out

    @classmethod
    def from_arrays(cls, arrays, prefix: str = "") -> "PackedForest":
        nf, avg, post = (int(v) for v in arrays[prefix + "meta"])
        name = {v: k for k, v in POSTPROCESSORS.items()}[post]
        return cls(*(arrays[prefix + k] for k in cls.ARRAYS), nf, bool(avg), name)

    def save(self, path: str) -> None:
        np.savez(path, **self.to_arrays())


# ---- converters --------------------------------------------------------------------------------------------------------------------
def _from_sklearn_trees(trees, n_features: int, leaf_of, K: int, base, average: bool, postprocessor: str) -> PackedForest:
    feat, thr, left, right, dl, roots, leaves = [], [], [], [], [], [], []
    node_base = leaf_base = 0
    for t in trees:
        tr = t.tree_
        is_leaf = tr.children_left < 0
        n = tr.node_count
        leaf_row = np.cumsum(is_leaf) - 1 + leaf_base
        feat.append(np.where(is_leaf, -1, tr.feature))
        thr.append(np.where(is_leaf, np.float32(0), f32_at_or_below(np.where(is_leaf, 0.0, tr.threshold))))
        left.append(np.where(is_leaf, leaf_row, tr.children_left + node_base))
        right.append(np.where(is_leaf, 0, tr.children_right + node_base))
        go_left = getattr(tr, "missing_go_to_left", None)
        dl.append(np.where(is_leaf, 0, go_left if go_left is not None else 0))
        roots.append(node_base)
        leaves.append(leaf_of(tr.value[is_leaf]))
        node_base += n
        leaf_base += int(is_leaf.sum())
    return PackedForest(np.concatenate(feat), np.concatenate(thr), np.concatenate(left), np.concatenate(right), np.concatenate(dl),
                        np.array(roots), np.concatenate(leaves).reshape(-1, K), np.asarray(base), n_features, average, postprocessor)


def from_sklearn(estimator) -> PackedForest:
    """RandomForestClassifier / ExtraTreesClassifier (leaf = tree_.value / its row sum, mean over the trees, identity: the
    columns are predict_proba) or a binary GradientBoostingClassifier (sum of the trees with the learning rate folded into
    the leaves, the init prior as base score, sigmoid; K = 2 with leaves (-v, +v), so the columns are [1 - p, p]).  Node i of
    tree j keeps scikit-learn's numbering: it is node tree_root[j] + i, which makes leaves_of comparable with `apply`.
    scikit-learn tests `float32(x) <= float64 threshold`; the thresholds are rounded DOWN to float32 (module docstring)."""
    from sklearn.ensemble import ExtraTreesClassifier, GradientBoostingClassifier, RandomForestClassifier   # lazily: not a dependency
    F = int(estimator.n_features_in_)
    if isinstance(estimator, (RandomForestClassifier, ExtraTreesClassifier)):
        if getattr(estimator, "n_outputs_", 1) != 1:
            raise ValueError("multi-output forests are not supported")
        K = int(estimator.n_classes_)

        def fractions(value):                                   # [n_leaves, 1, K] counts or fractions -> fractions
            v = value[:, 0, :].astype(np.float64)
            return v / v.sum(axis=1, keepdims=True)
        return _from_sklearn_trees(estimator.estimators_, F, fractions, K, np.zeros(K), True, "identity")
    if isinstance(estimator, GradientBoostingClassifier):
        if int(estimator.n_classes_) != 2:
            raise ValueError("only the binary GradientBoostingClassifier is supported")
        init = estimator.init_
        if isinstance(init, str):
            b = 0.0
        else:
            from sklearn.dummy import DummyClassifier
            if not isinstance(init, DummyClassifier):
                raise ValueError("a GradientBoostingClassifier whose init is an estimator has no constant base score")
            b = float(np.ravel(estimator._raw_predict_init(np.zeros((1, F))))[0])
        lr = float(estimator.learning_rate)

        def signed(value):
            v = lr * value[:, 0, 0].astype(np.float64)
            return np.stack([-v, v], axis=1)
        return _from_sklearn_trees(list(estimator.estimators_[:, 0]), F, signed, 2, np.array([-b, b]), False, "sigmoid")
    raise TypeError(f"from_sklearn does not know {type(estimator).__name__}")


_TL_POST = {"identity": "identity", "identity_multiclass": "identity", "sigmoid": "sigmoid", "softmax": "softmax"}


def from_treelite_json(obj: dict) -> PackedForest:
    """The dict of treelite.Model.dump_as_json().  UNPINNED: the field names are treelite 4.x's as remembered (module
    docstring).  A node goes left iff `x comparison_op threshold`; `<` and `<=` become the one comparison by rounding the
    threshold down, `>` and `>=` by swapping the children as well.  Nodes are renumbered in preorder (a node seen twice, a
    cycle, is refused).  A scalar leaf of a model with K > 1 outputs lands in the column `class_id` of its tree."""
    F = int(obj["num_feature"])
    num_class = obj.get("num_class", [1])
    K = int(num_class[0] if isinstance(num_class, (list, tuple)) else num_class)
    shape = obj.get("leaf_vector_shape", [1, 1])
    K = max(K, int(shape[-1]))
    post = _TL_POST.get(obj.get("postprocessor", "identity"))
    if post is None:
        raise ValueError(f"postprocessor {obj.get('postprocessor')!r} is not supported")
    base = np.zeros(K)
    bs = np.ravel(np.asarray(obj.get("base_scores", [0.0]), dtype=np.float64))
    base[:] = bs[:K] if bs.size >= K else bs[0]
    class_id = obj.get("class_id")
    feat, thr, left, right, dl, roots, leaves = [], [], [], [], [], [], []
    for ti, tree in enumerate(obj["trees"]):
        nodes = {int(n.get("node_id", i)): n for i, n in enumerate(tree["nodes"])}
        roots.append(len(feat))
        seen = set()
        stack = [(0, None, None)]                               # node 0 is the root
        while stack:                                            # preorder; the parent's child slot is patched on arrival
            nid, parent, side = stack.pop()
            if nid in seen:
                raise ValueError(f"tree {ti}: node {nid} is reached twice")
            seen.add(nid)
            me = len(feat)
            if parent is not None:
                (left if side == 0 else right)[parent] = me
            n = nodes[nid]
            if "leaf_value" in n:
                v = np.zeros(K)
                lv = np.ravel(np.asarray(n["leaf_value"], dtype=np.float64))
                if lv.size == K:
                    v[:] = lv
                elif lv.size == 1:
                    c = int(class_id[ti]) if class_id is not None else 0
                    v[c if c >= 0 else slice(None)] = lv[0]
                else:
                    raise ValueError(f"tree {ti}: a leaf of {lv.size} values in a model of {K} outputs")
                feat.append(-1), thr.append(np.float32(0)), left.append(len(leaves)), right.append(0), dl.append(0)
                leaves.append(v)
                continue
            op = n.get("comparison_op", "<")
            if op not in ("<", "<=", ">", ">="):
                raise ValueError(f"tree {ti}: comparison_op {op!r}")
            swap = op in (">", ">=")
            # x > t is not(x <= t): children swapped, threshold as for `<=`;  x >= t is not(x < t): swapped, as for `<`
            strict = op in ("<", ">=")
            feat.append(int(n["split_feature_id"]))
            thr.append(f32_at_or_below(float(n["threshold"]), strict=strict)[()])
            left.append(-1), right.append(-1)
            dl.append(int(bool(n.get("default_left", False)) != swap))
            a, b = int(n["left_child"]), int(n["right_child"])
            if swap:
                a, b = b, a
            stack.append((b, me, 1))
            stack.append((a, me, 0))                            # the left subtree first
    return PackedForest(np.array(feat), np.array(thr, dtype=np.float32), np.array(left), np.array(right), np.array(dl),
                        np.array(roots), np.array(leaves).reshape(-1, K), base, F, bool(obj.get("average_tree_output", False)), post)


def load(path: str) -> PackedForest:
    """`.npz`: the packed form (PackedForest.save).  `.json`: a treelite JSON dump.  `.tl`: a treelite checkpoint, only where
    the treelite package imports (UNPINNED, never run: module docstring)."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npz":
        with np.load(path) as z:
            return PackedForest.from_arrays(z)
    if ext == ".json":
        with open(path) as f:
            return from_treelite_json(json.load(f))
    if ext == ".tl":
        try:
            import treelite
        except ImportError as e:
            raise ImportError(f"{path}: reading a .tl checkpoint needs the treelite package, which is not installed; "
                              "convert it once where treelite is (Model.deserialize(path).dump_as_json() -> .json, or "
                              "forest.load(...).save(...) -> .npz): .json and .npz need nothing") from e
        dump = treelite.Model.deserialize(path).dump_as_json()
        return from_treelite_json(json.loads(dump) if isinstance(dump, str) else dump)
    raise ValueError(f"{path}: not a .npz, .json or .tl file")


# ---- the bank ----------------------------------------------------------------------------------------------------------------------
@dataclass
class DeviceBank:
    """The operands of ops.forest_predict on one device (ForestBank.to)."""
    nodes: object
    tree_root: object
    leaf_values: object
    base_scores: object
    model_node_base: object
    model_tree_base: object
    model_leaf_base: object
    model_n_trees: object
    n_models: int
    n_outputs: int
    n_features: int
    average: bool
    postprocessor: str


class ForestBank:
    """M models end to end: the arrays of include/vf_hip_forest.h on the host, and per device one uploaded copy, made on the
    first to(device) and kept (a weight-derived operand like the others: built once, never per call)."""

    def __init__(self, models):
        models = list(models)
        if not models:
            raise ValueError("a bank holds at least one model")
        first = models[0]
        for name in ("n_outputs", "n_features", "postprocessor", "average"):
            vals = {getattr(m, name) for m in models}
            if len(vals) != 1:
                raise ValueError(f"the models of a bank must share {name}; got {sorted(vals, key=str)}")
        counts = np.array([[m.n_nodes, m.n_trees, m.leaf_values.shape[0]] for m in models], dtype=np.int64)
        if int(counts[:, 0].sum()) > MAX_BANK_NODES:
            raise ValueError(f"a bank of {int(counts[:, 0].sum())} nodes is past the {MAX_BANK_NODES} that int32 indices reach")
        bases = np.concatenate([np.zeros((1, 3), dtype=np.int64), np.cumsum(counts, axis=0)[:-1]])
        self.n_models, self.n_outputs, self.n_features = len(models), first.n_outputs, first.n_features
        self.average, self.postprocessor = first.average, first.postprocessor
        self.nodes = np.concatenate([m.nodes16() for m in models])
        self.tree_root = np.concatenate([m.tree_root for m in models])
        self.leaf_values = np.concatenate([m.leaf_values for m in models])
        self.base_scores = np.stack([m.base_scores for m in models])
        self.model_node_base, self.model_tree_base, self.model_leaf_base = (bases[:, i].astype(np.int32) for i in range(3))
        self.model_n_trees = counts[:, 1].astype(np.int32)
        self._device = {}

    ARRAYS = ("nodes", "tree_root", "leaf_values", "base_scores", "model_node_base", "model_tree_base", "model_leaf_base",
              "model_n_trees")

    def to(self, device) -> DeviceBank:
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        hit = self._device.get(device)
        if hit is None:
            arrays = [torch.from_numpy(np.ascontiguousarray(getattr(self, k))).to(device) for k in self.ARRAYS]
            hit = self._device[device] = DeviceBank(*arrays, self.n_models, self.n_outputs, self.n_features, self.average,
                                                    self.postprocessor)
        return hit

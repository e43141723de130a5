"""Operands, float64 restatement, error bound, fixture loader and write-set cases of the forest evaluator (vf_forest_predict,
include/vf_hip_forest.h), shared by tests/test_forest_cpu.py, tests/test_forest_gpu.py, tests/test_ad_risk_gpu.py and
tests/golden/make_ad_risk_golden.py.  Importing this module needs no GPU.

The restatement is the header's semantics with the sums in float64: every tree walked from its root (left iff x <= threshold,
both fp32; a NaN feature by default_left), the leaf rows of all trees added, divided by T where the model averages, the base
score added, the postprocessor applied.

Beside every output stands its a-priori error bound.  Before the postprocessor,
    delta[k] = (T + 2) * 2^-24 * (sum_t |leaf_t[k]| / (T if average else 1) + |base[k]|):
an fp32 sum of T terms loses at most (T - 1) * 2^-24 * sum |terms| in ANY order (Higham 3.5: every partial sum is at most
sum |terms|, each of the T - 1 additions rounds once), and three more roundings of values no larger follow or precede: the
fp32 storage of a leaf the converter computed in float64 (which is how this bound also covers scikit-learn's own float64
probabilities), the division by T and the addition of the base score.  After it,
    identity  delta;
    sigmoid   delta / 4 + 3 * 2^-24:     |s'| <= 1/4;  s = 1 / (1 + e), e = expf(-v): an error of U_EXP ulps in e (relative
              U_EXP * 2^-23) moves s by e / (1 + e)^2 <= 1/4 of it, i.e. U_EXP/2 * 2^-24; the addition and the division round s
              (<= 1) once each: (U_EXP/2 + 2) * 2^-24, rounded up to 3;
    softmax   delta_max + (2 U_EXP + K + 4) * 2^-24, delta_max the largest delta of the row: |dp_k| <= 2 p_k (1 - p_k) *
              delta_max <= delta_max / 2 for a perturbation of the logits, and as much again for the subtraction v - max,
              which rounds an exponent d to within 2^-24 |d| while p falls like exp(-|d|) (|d| exp(-|d|) < 1/2); each e_j carries
              U_EXP ulps (2 U_EXP * 2^-24 relative, on numerator and denominator: at most that on p <= 1), the K - 1 additions
              of the denominator and the division at most K * 2^-24, the rest is slack of four roundings.
U_EXP = 1: the HIP math API documents expf with a maximum error of 1 ulp.  Nothing in the bounds is measured.
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np
import torch

from variantformer_amd import forest as Fo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U24 = 2.0 ** -24
U_EXP = 1                                              # ulps of the device expf (HIP math API: 1)
POST = {"identity": 0, "sigmoid": 1, "softmax": 2}
EXTRA_LDX, EXTRA_LDO = 7, 3                            # ldx > F and ldo > K (no multiple of anything: the entry asks for none)
FIXTURE_MODELS = ("rf", "et", "gb")
VARIANTS = ("lt", "nearest", "swapped", "no_average", "no_default")


# ---- float64 restatement -----------------------------------------------------------------------------------------------------------
def walk(m, X: np.ndarray, variant: str | None = None, thr64=None) -> np.ndarray:
    """int64 [n, T]: the node each walk ends in.  variant (a plausible mistake, for the references' own test):
      lt          `<` where `<=` belongs;
      nearest     the float64 thresholds `thr64` rounded to the NEAREST float32 instead of down;
      swapped     the children swapped;
      no_default  default_left ignored: a NaN feature fails the comparison and goes right."""
    X = np.asarray(X, dtype=np.float32)
    thr = m.threshold if variant != "nearest" else np.asarray(thr64, dtype=np.float64).astype(np.float32)
    left, right = (m.right, m.left) if variant == "swapped" else (m.left, m.right)
    leaf = m.feature < 0
    ends = np.empty((X.shape[0], m.n_trees), dtype=np.int64)
    for r in range(X.shape[0]):
        x = X[r]
        for t, n in enumerate(m.tree_root):
            while not leaf[n]:
                v = x[m.feature[n]]
                if np.isnan(v):
                    go_left = bool(m.default_left[n]) and variant != "no_default"
                else:
                    go_left = v < thr[n] if variant == "lt" else v <= thr[n]
                n = left[n] if go_left else right[n]
            ends[r, t] = n
    return ends


def post64(v: np.ndarray, postprocessor: str) -> np.ndarray:
    if postprocessor == "sigmoid":
        return 1.0 / (1.0 + np.exp(-v))
    if postprocessor == "softmax":
        e = np.exp(v - v.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)
    return v


def predict64(m, X: np.ndarray, variant: str | None = None, thr64=None):
    """(out, bound) float64 [n, K] each: the packed semantics and the a-priori bound of the module docstring."""
    ends = walk(m, X, variant, thr64)
    lv = m.leaf_values.astype(np.float64)[m.left[ends]]                   # [n, T, K]
    T = m.n_trees
    div = T if (m.average and variant != "no_average") else 1
    base = m.base_scores.astype(np.float64)
    v = lv.sum(axis=1) / div + base
    delta = (T + 2) * U24 * (np.abs(lv).sum(axis=1) / div + np.abs(base))
    K = v.shape[1]
    if m.postprocessor == "sigmoid":
        delta = delta / 4 + 3 * U24
    elif m.postprocessor == "softmax":
        delta = np.broadcast_to(delta.max(axis=1, keepdims=True) + (2 * U_EXP + K + 4) * U24, v.shape).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        return post64(v, m.postprocessor), delta


# ---- seeded forests ----------------------------------------------------------------------------------------------------------------
def make_forest(seed: int, T: int, F: int, K: int, depth: int = 5, average: bool = True, postprocessor: str = "identity",
                leaf_only=()) -> Fo.PackedForest:
    """A seeded forest of T random trees, nodes in preorder (children above their parent).  A node at depth < `depth` splits
    with probability 0.8 (the root always, except in the trees `leaf_only`, which are a single leaf).  Thresholds are fp32
    normals, every fourth on a 1/4 grid (where the seeded rows put values too); leaves are uniform in [0, 1) for identity
    models and normal otherwise."""
    g = np.random.default_rng(9000 + seed)
    feat, thr, left, right, dl, roots, leaves = [], [], [], [], [], [], []

    def grow(d, root, single):
        me = len(feat)
        if single or d == depth or (not root and g.random() > 0.8):
            feat.append(-1), thr.append(0.0), left.append(len(leaves)), right.append(0), dl.append(0)
            leaves.append(g.random(K) if postprocessor == "identity" else g.normal(size=K))
            return me
        t = g.normal()
        feat.append(int(g.integers(F))), thr.append(np.round(t * 4) / 4 if g.integers(4) == 0 else t)
        left.append(-1), right.append(-1), dl.append(int(g.integers(2)))
        left[me] = grow(d + 1, False, False)
        right[me] = grow(d + 1, False, False)
        return me
    for t in range(T):
        roots.append(grow(0, True, t in leaf_only))
    return Fo.PackedForest(np.array(feat), np.array(thr, dtype=np.float32), np.array(left), np.array(right), np.array(dl),
                           np.array(roots), np.array(leaves), g.normal(size=K) * 0.1, F, average, postprocessor)


def make_rows(seed: int, R: int, F: int, nan_fraction: float = 0.05) -> np.ndarray:
    """fp32 [R, F]: normals, a quarter of them on the 1/4 grid of the seeded thresholds, `nan_fraction` of them NaN."""
    g = np.random.default_rng(7000 + seed)
    x = g.normal(size=(R, F))
    x = np.where(g.random((R, F)) < 0.25, np.round(x * 4) / 4, x)
    x[g.random((R, F)) < nan_fraction] = np.nan
    return x.astype(np.float32)


# (name, trees of each model of the bank, F, K, R, average, postprocessor, depth): every T, F, K and R of the kernel's paths --
# T 1 / 5: one lane, a few; 64 / 65: a full wave of walks and one lane's second; 130: three rounds; `leaf` holds a tree that is a
# single leaf; R 1 / 5 / 67 blocks; banks of one model and of four with different T; the three postprocessors
GEOMETRIES = (
    ("t1", (1,), 4, 1, 1, True, "identity", 3),
    ("t5", (5,), 4, 2, 5, True, "identity", 4),
    ("t64", (64,), 96, 3, 67, True, "identity", 5),
    ("t65", (65,), 96, 8, 5, False, "identity", 5),
    ("t130", (130,), 1536, 2, 5, True, "identity", 6),
    ("leaf", (5,), 96, 2, 5, True, "identity", 4),
    ("bank4", (1, 64, 5, 130), 96, 2, 67, True, "identity", 5),
    ("bank4_sum", (65, 5, 1, 64), 1536, 3, 67, False, "identity", 5),
    ("sigmoid", (65, 5), 96, 2, 67, False, "sigmoid", 4),
    ("sigmoid1", (5,), 4, 1, 5, False, "sigmoid", 3),
    ("softmax", (5, 130), 1536, 8, 5, False, "softmax", 5),
    ("softmax3", (64,), 96, 3, 67, True, "softmax", 5),
)
GEOMETRY_IDS = [g[0] for g in GEOMETRIES]


class Case:
    def __init__(self, name, trees, F, K, R, average, postprocessor, depth, seed=0):
        self.name, self.F, self.K, self.R = name, F, K, R
        base = 100 * GEOMETRY_IDS.index(name) + 17 * seed
        self.models = [make_forest(base + i, T, F, K, depth, average, postprocessor, leaf_only=(2,) if name == "leaf" else ())
                       for i, T in enumerate(trees)]
        self.bank = Fo.ForestBank(self.models)
        self.x = make_rows(base, R, F)
        self.model_of_row = np.random.default_rng(base).integers(0, len(trees), R).astype(np.int32)
        self.ldx, self.ldo = F + EXTRA_LDX, K + EXTRA_LDO


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    return Case(*next(g for g in GEOMETRIES if g[0] == name))


@functools.lru_cache(maxsize=None)
def reference(name) -> dict:
    """float64, computed once per geometry: `all` / `all_bound` [M, R, K], every row through every model of the bank."""
    c = case(name)
    both = [predict64(m, c.x) for m in c.models]
    return {"all": np.stack([b[0] for b in both]), "all_bound": np.stack([b[1] for b in both])}


def row_form(ref: dict, model_of_row) -> tuple:
    idx = np.arange(len(model_of_row))
    return ref["all"][model_of_row, idx], ref["all_bound"][model_of_row, idx]


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def load_ad_risk() -> dict:
    """{name: dict(model, thr64, x, proba, kind)} of tests/golden/ad_risk.*: three scikit-learn models in packed form, the test
    rows and scikit-learn's own predict_proba on them."""
    with open(os.path.join(GOLDEN, "ad_risk.json")) as f:
        meta = json.load(f)
    out = {}
    with np.load(os.path.join(GOLDEN, "ad_risk.npz")) as z:
        for name in FIXTURE_MODELS:
            out[name] = dict(model=Fo.PackedForest.from_arrays(z, f"{name}."), thr64=z[f"{name}.thr64"], x=z[f"{name}.x"],
                             proba=z[f"{name}.proba"], meta=meta["models"][name])
    return out


def wrong_variants(f: dict) -> dict:
    """What a plausible mistake computes instead of the fixture's probabilities, float64 [n, K] each (None: the model leaves no
    room for it -- a boosted model does not average, and scikit-learn's takes no NaN so its rows hold none)."""
    m = f["model"]
    out = {v: predict64(m, f["x"], v, f["thr64"])[0] for v in ("lt", "nearest", "swapped")}
    out["no_average"] = predict64(m, f["x"], "no_average")[0] if m.average else None
    out["no_default"] = predict64(m, f["x"], "no_default")[0] if np.isnan(f["x"]).any() else None
    return out


def rows_off(wrong: np.ndarray, f: dict, bound: np.ndarray) -> np.ndarray:
    """bool [n]: the rows in which a variant is further than 100 bounds from the golden values."""
    return (np.abs(wrong - f["proba"]) > 100.0 * bound).any(axis=1)


def variant_need(kind: str, f: dict) -> tuple:
    """(rows that must differ or None, how many must differ): three quarters of the rows; `nearest` 8 rows; `no_default` every
    row that holds a NaN."""
    n = f["x"].shape[0]
    if kind == "nearest":
        return None, 8
    if kind == "no_default":
        has_nan = np.isnan(f["x"]).any(axis=1)
        return has_nan, int(has_nan.sum())
    return None, -(-3 * n // 4)


# ---- the parallel write-set net: one case list for the entry of include/vf_hip_forest.h --------------------------------------------
# tests/write_set_cases.py's machinery on vf_forest_predict, beside the lists of tests/attn_contrib_cases.py,
# tests/gene_contrib_cases.py and tests/cre_heads_cases.py.  Every input is an interior slice of a poisoned buffer (x with guard
# columns: ldx > F), out is an arena with padding columns and rows; after the call the inputs' whole buffers, guards included, are
# compared with a copy taken before it.
WS_GEOMETRIES = ("bank4", "sigmoid", "softmax", "t1")


def ws_name(name, form, how):
    return f"forest_predict-{name}-{form}-{how}"


def _make_ws(name, row_form_, wrapper):
    def make():
        from tests import write_set_cases as W
        c = Case(*next(g for g in GEOMETRIES if g[0] == name), seed=1)
        K, R = c.K, c.R
        which = len(c.models) - 1                                     # the cohort form's model: the last of the bank
        both = [predict64(m, c.x) for m in c.models]
        if row_form_:
            idx = np.arange(R)
            want = np.stack([b[0] for b in both])[c.model_of_row, idx]
            bound = np.stack([b[1] for b in both])[c.model_of_row, idx]
        else:
            want, bound = both[which]
        cols = K + EXTRA_LDO

        def run(p):
            from variantformer_amd import _lib
            ops = W._ops()
            b = c.bank
            x = W.guarded(torch.from_numpy(c.x), p, W.GUARD_COLS)
            dev = {k: W.guarded(torch.from_numpy(np.ascontiguousarray(getattr(b, k))), p) for k in Fo.ForestBank.ARRAYS}
            mor = W.guarded(torch.from_numpy(c.model_of_row), p) if row_form_ else None
            inputs = [x] + list(dev.values()) + ([mor] if mor is not None else [])
            bases = [t._base if t._base is not None else t for t in inputs]
            before = [t.clone() for t in bases]
            big, out = W.arena(R, cols, torch.float32, p)
            if wrapper:
                bank = Fo.DeviceBank(*(dev[k] for k in Fo.ForestBank.ARRAYS), b.n_models, b.n_outputs, b.n_features, b.average,
                                     b.postprocessor)
                with W.poison_allocations(p) as proxy:
                    ops.forest_predict(x, bank, model_of_row=mor, model=None if row_form_ else which, out=out)
                assert proxy.count == 0, "ops.forest_predict makes nothing: every buffer is the caller's"
            else:
                _lib.check(_lib.load().vf_forest_predict(x.data_ptr(), x.stride(0), R, c.F, *(dev[k].data_ptr() for k in Fo.ForestBank.ARRAYS),
                                                         b.n_models, K, int(b.average), POST[b.postprocessor],
                                                         0 if mor is None else mor.data_ptr(), -1 if row_form_ else which,
                                                         out.data_ptr(), out.stride(0), W._stream()), "vf_forest_predict")
            W._sync()
            for t, was in zip(bases, before):
                assert torch.equal(t.view(torch.uint8), was.view(torch.uint8)), "an input, or the memory around it, was written"
            return {"out": big}

        def check(bufs):
            body = bufs["out"][8:8 + R, W.GUARD_COLS:W.GUARD_COLS + K].double().numpy()
            assert bool((np.abs(body - want) <= bound).all())
        inner = torch.zeros((R, cols), dtype=torch.bool)
        inner[:, :K] = True                                           # the padding columns of a row keep the poison
        return W.Built(run, {"out": W.arena_mask(R, cols, inner)}, check)
    return make


def ws_cases() -> list:
    from tests import write_set_cases as W
    out = []
    for name in WS_GEOMETRIES:
        for row_form_ in (True, False):
            for wrapper in (False, True):
                out.append(W.WSCase(ws_name(name, "row" if row_form_ else "cohort", "wrapper" if wrapper else "entry"),
                                    "forest_predict", ("vf_forest_predict",), ("forest_predict",) if wrapper else (),
                                    _make_ws(name, row_form_, wrapper)))
    return out

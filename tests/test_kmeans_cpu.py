"""k-means without a GPU: the boundary of include/vf_hip_kmeans.h (it parses, its four names are exported and bound through
_lib.ENTRIES), every refusal of every entry and of the Python functions, the
numpy restatements of tests/kmeans_cases.py against exhaustive small cases (the tie and NaN rule, the integer sampling), and the
restatements pinned to scikit-learn's KMeans(algorithm="lloyd") on the fixtures, whose condition is checked first."""
import inspect
import itertools
import math
import os
import re
import warnings

import numpy as np
import pytest
import torch

from tests import kmeans_cases as K
from tests import write_set_cases as W
from tests.conftest import REPO

NAMES = ["vf_kmeans_assign", "vf_kmeans_lloyd", "vf_kmeans_seed", "vf_kmeans_update"]
ARGS = {"vf_kmeans_assign": 10, "vf_kmeans_update": 12, "vf_kmeans_lloyd": 20, "vf_kmeans_seed": 13}


def _header(name="vf_hip_kmeans.h") -> str:
    with open(os.path.join(REPO, "include", name)) as f:
        return f.read()


# ---- 1. header, constants and build lists ------------------------------------------------------------------------------------------
def test_header_parses_and_its_names_are_exported_and_bound():
    from variantformer_amd import _lib, ops
    from variantformer_amd.csrc import build as B
    text = _header()
    assert W.stream_entries(text) == NAMES
    assert sorted(_lib.ENTRIES["vf_hip_kmeans.h"]) == NAMES, "ctypes binding and vf_hip_kmeans.h disagree"
    assert "vf_kmeans.hip" in B.SOURCES and any(h.endswith("vf_hip_kmeans.h") for h in B.HEADERS)
    assert "vf_kmeans.hip" not in B.EXTRA_FLAGS                       # a NaN distance is recognised as such: no -fno-honor-nans
    with open(os.path.join(REPO, "variantformer_amd", "csrc", "vf_kmeans.hip")) as f:
        source = f.read()
    assert "#pragma clang fp contract(off)" in source, "the distance's bits hold only without an fma"
    assert "hipDeviceSynchronize" not in source and "hipStreamSynchronize" not in source and "hipMemcpy" not in source, \
        "no entry synchronises the stream or reads anything back"
    assert not re.search(r"\b_*(hip_)?atomic\w*\s*\(", source, flags=re.I), "no atomic: every sum has a stated order"
    bound = _lib.load()
    assert {name: len(_lib.SIGNATURES[name]) for name in NAMES} == ARGS
    assert _lib.ABI_VERSION == 13 and bound.vf_version() == 13
    for word in ("Arguments", "Write set", "Arithmetic", "Non-finite operands", "Refused before anything is launched", "Not checked"):
        assert text.count(word) >= 4, f"an entry's comment contract has no `{word}` part"
    for phrase in ("t = x[r, c] - cen[j, c];   p = t * t;   acc = acc + p", "NO fused multiply-add", "ties to the lower j",
                   "a NaN distance never", "label -1 and dist NaN", "NOT scikit-learn's greedy k-means++", "0x7FEB352D", "0x846CA68B"):
        assert phrase in text, phrase
    for macro, value in (("VF_KMEANS_MAX_K", K.MAX_K), ("VF_KMEANS_MAX_R", "(1 << 24)"), ("VF_KMEANS_MAX_D", K.MAX_D), ("VF_KMEANS_ROWS", K.ROWS),
                         ("VF_KMEANS_SPLITS", K.SPLITS), ("VF_KMEANS_JT", K.JT), ("VF_KMEANS_DC", K.DC), ("VF_KMEANS_DC_SMALL", K.DC_SMALL),
                         ("VF_KMEANS_UPDATE_WAVES", K.UPDATE_WAVES), ("VF_KMEANS_UPDATE_COLS", K.UPDATE_COLS),
                         ("VF_KMEANS_RED_THREADS", K.RED_THREADS)):
        assert re.search(rf"#define\s+{macro}\s+{re.escape(str(value))}\s", text), macro
    assert re.search(r"#define\s+VF_ENRICH_MAX_K\s+4096\s", _header("vf_hip_enrich.h")) and K.MAX_K == 4096     # the labels' consumer
    # the Python mirrors of the constants and of the two workspace formulas
    assert (ops.KMEANS_MAX_K, ops.KMEANS_MAX_R, ops.KMEANS_MAX_D) == (K.MAX_K, K.MAX_R, K.MAX_D)
    for R, d, k in ((1, 1, 1), (64, 64, 3), (65, 65, 4096), (18000, 49, 50), (262144, 64, 1024)):
        assert ops.kmeans_lloyd_work_bytes(R, d, k) == K.lloyd_work_bytes(R, d, k) == 8 + 8 * k * -(-d // 64) + 4 * -(-R // 64)
        assert ops.kmeans_seed_work_bytes(R) == K.seed_work_bytes(R) == 16 + 12 * -(-R // 256)
    assert "8 + 8 * (int64_t)(k)" in text and "16 + 12 *" in text


def test_the_wrappers_allocate_nothing():
    from variantformer_amd import ops
    for name in ("kmeans_assign", "kmeans_update", "kmeans_lloyd", "kmeans_seed"):
        src = inspect.getsource(getattr(ops, name))
        assert not re.search(r"torch\.(empty|zeros|ones|full|tensor|arange)", src), name
        assert "nothing is made here" in src


P = 4096                                                 # a non-null, aligned address; never dereferenced
INVALID = 1


def _err(lib):
    return lib.vf_last_error().decode()


def check_refusals():
    """Every refusal of every entry, its argument named; nothing is launched (tests/test_kmeans_gpu.py runs it on the device too)."""
    from variantformer_amd import _lib
    lib = _lib.load()

    def common(call, cen="cen", aligned4=(), aligned8=(), k_max=K.MAX_K):
        for name in ("x", cen) + tuple(aligned4) + tuple(aligned8):
            assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), (name, _err(lib))
            align = 8 if name in aligned8 else 4
            assert call(**{name: P + align // 2}) == INVALID and re.search(rf"\b{name} must be {align}-byte aligned", _err(lib)), (name, _err(lib))
        for d in (0, -1, K.MAX_D + 1):
            assert call(d=d, ldx=1 << 20, ldc=1 << 20) == INVALID and _err(lib).split(": ")[1].startswith("d="), _err(lib)
        for name in ("ldx", "ldc"):
            assert call(**{name: 11}) == INVALID and _err(lib).split(": ")[1].startswith(f"{name}="), _err(lib)
        for k in (0, -1, k_max + 1):
            assert call(k=k) == INVALID and _err(lib).split(": ")[1].startswith("k="), _err(lib)
        assert call(R=-1) == INVALID and "R=" in _err(lib)
        assert call(R=2 ** 24 + 1) == INVALID and "R=" in _err(lib)

    def assign(x=P, ldx=12, R=0, d=12, cen=P, ldc=12, k=5, labels=P, dist=P):
        return lib.vf_kmeans_assign(x, ldx, R, d, cen, ldc, k, labels, dist, 0)
    assert assign() == 0 and assign(k=K.MAX_K, d=K.MAX_D, ldx=K.MAX_D, ldc=K.MAX_D) == 0                     # R = 0: nothing launched
    common(assign, aligned4=("labels", "dist"))

    def update(x=P, ldx=12, R=5, d=12, labels=P, cen_old=P, ldc=12, k=5, cen_new=P, ldn=12, counts=P):
        return lib.vf_kmeans_update(x, ldx, R, d, labels, cen_old, ldc, k, cen_new, ldn, counts, 0)
    common(update, cen="cen_old", aligned4=("labels", "cen_new", "counts"))
    assert update(ldn=11) == INVALID and _err(lib).split(": ")[1].startswith("ldn="), _err(lib)

    def lloyd(x=P, ldx=12, R=0, d=12, cen=P, ldc=12, k=5, max_iter=3, tol_abs=0.0, resume=0, labels=P, dist=P, prev_labels=P, counts=P,
              n_iter=P, shift=P, changed=P, work=P, work_bytes=1 << 40):
        return lib.vf_kmeans_lloyd(x, ldx, R, d, cen, ldc, k, max_iter, tol_abs, resume, labels, dist, prev_labels, counts, n_iter, shift,
                                   changed, work, work_bytes, 0)
    assert lloyd() == 0 and lloyd(max_iter=0, shift=0, changed=0) == 0 and lloyd(resume=1, tol_abs=1e300) == 0
    common(lloyd, aligned4=("labels", "dist", "prev_labels", "counts", "n_iter"), aligned8=("shift", "changed", "work"))
    assert lloyd(max_iter=-1) == INVALID and "max_iter=" in _err(lib)
    for bad in (float("nan"), -1e-300, -float("inf")):
        assert lloyd(tol_abs=bad) == INVALID and "tol_abs=" in _err(lib), bad
    for bad in (-1, 2):
        assert lloyd(resume=bad) == INVALID and "resume=" in _err(lib)
    need = K.lloyd_work_bytes(1000, 12, 5)
    assert lloyd(R=1000, work_bytes=need - 1) == INVALID and "work_bytes=" in _err(lib) and str(need) in _err(lib)

    def seed(x=P, ldx=12, R=100, d=12, k=5, seed=0, rows=P, cen=P, ldc=12, mind=P, work=P, work_bytes=1 << 40):
        return lib.vf_kmeans_seed(x, ldx, R, d, k, seed, rows, cen, ldc, mind, work, work_bytes, 0)
    common(seed, aligned4=("rows", "mind"), aligned8=("work",))
    assert seed(R=0) == INVALID and "R=" in _err(lib)
    assert seed(R=4, k=5) == INVALID and _err(lib).split(": ")[1].startswith("k="), _err(lib)
    assert seed(work_bytes=K.seed_work_bytes(100) - 1) == INVALID and "work_bytes=" in _err(lib)


def test_refusals_without_gpu():
    check_refusals()


def test_python_refusals_without_gpu():
    from variantformer_amd import kmeans
    x = np.zeros((10, 3), np.float32)
    for kwargs, word in ((dict(n_clusters=11), "above the 10 rows"), (dict(n_clusters=0), "n_clusters"), (dict(n_clusters=True), "n_clusters"),
                         (dict(n_clusters=2, metric="manhattan"), "metric"), (dict(n_clusters=2, init="pca"), "init"),
                         (dict(n_clusters=2, init=np.zeros((3, 3), np.float32)), "init array"), (dict(n_clusters=2, n_init=0), "n_init"),
                         (dict(n_clusters=2, max_iter=0), "max_iter"), (dict(n_clusters=2, tol=-1.0), "tol"),
                         (dict(n_clusters=2, tol=float("nan")), "tol"), (dict(n_clusters=2, seed=-1), "seed"), (dict(n_clusters=2, seed=1.5), "seed")):
        with pytest.raises(ValueError, match=word):
            kmeans.kmeans(x, **kwargs)
    with pytest.raises(ValueError, match="above 4096"):
        kmeans.kmeans(np.zeros((5000, 2), np.float32), 4097)
    with pytest.raises(ValueError, match="matrix"):
        kmeans.kmeans(np.zeros(7, np.float32), 2)
    with pytest.raises(ValueError, match="metric"):
        kmeans.KMeansModel.from_state({"metric": "l1", "centers": np.zeros((2, 2)), "labels": [0], "inertia": 0, "n_iter": 1, "counts": [1, 0],
                                       "nan_to_zero": True})
    model = kmeans.KMeansModel.from_state(kmeans.KMeansModel(np.array([0, 1], np.int32), np.eye(2, dtype=np.float32), 0.5, 3, np.array([1, 1]),
                                                             "euclidean").state())
    assert model.n_clusters == 2 and model.columns == 2 and model.n_iter == 3 and model.inertia == 0.5 and model.metric == "euclidean"
    with pytest.raises(ValueError, match="columns"):
        model.predict(np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError, match="chunk_rows"):
        model.predict(np.zeros((4, 2), np.float32), chunk_rows=0)
    # the two hashes are one: the pipeline's (random starts) and the case module's (the seeding's restatement)
    for seed, t in itertools.product((0, 1, 42, 2 ** 40 + 5), (0, 1, 7, 4095)):
        assert kmeans.hash64(seed, t) == K.hash64(seed, t) < 1 << 64
    for R, k, seed in ((1, 1, 0), (5, 5, 3), (130, 50, 9), (18000, 50, 0)):
        rows = kmeans.random_rows(R, k, seed)
        assert rows.dtype == np.int32 and len(set(rows.tolist())) == k and rows.min() >= 0 and rows.max() < R
        assert np.array_equal(rows, kmeans.random_rows(R, k, seed))
    assert not np.array_equal(kmeans.random_rows(130, 50, 9), kmeans.random_rows(130, 50, 10))


# ---- 2. the restatement against exhaustive small cases -----------------------------------------------------------------------------
def test_the_tie_and_nan_rule_on_integer_valued_data():
    """Every row of {0, 1, 2, NaN, Inf}^2 against every pair of centres from the same set: integer-valued distances are exact, so
    ties are real ties; the vectorised winner equals the rule applied one comparison at a time."""
    vals = np.array([0.0, 1.0, 2.0, np.nan, np.inf], np.float32)
    pts = np.array(list(itertools.product(vals, repeat=2)), np.float32)                 # 25 points
    for a, b, c in itertools.product(range(len(pts)), repeat=3):
        if a % 3 or b % 2:                                                              # a third of the triples: 1 875 centre sets
            continue
        cen = pts[[a, b, c]]
        D = K.distances(pts, cen)
        lab, dist = K.winners(D)
        lab2, dist2 = K.winners_brute(D)
        assert np.array_equal(lab, lab2) and np.array_equal(np.isnan(dist), lab < 0)
        assert np.array_equal(dist[lab >= 0], dist2[lab >= 0]) and not np.signbit(dist[lab >= 0]).any()
    # the rule itself, spelled out
    D = np.array([[4, 1, 1, 9], [np.nan, 3, np.nan, 3], [np.nan, np.nan, np.nan, np.nan], [np.inf, np.inf, np.nan, np.inf],
                  [np.nan, np.inf, 5, 5], [0, 0, 0, 0]], np.float32)
    lab, dist = K.winners(D)
    assert lab.tolist() == [1, 1, -1, 0, 2, 0]
    assert dist.view(np.uint32).tolist() == np.array([1, 3, np.nan, np.inf, 5, 0], np.float32).view(np.uint32).tolist()
    assert dist.view(np.uint32)[2] == K.NAN_BITS
    # the fp32 chain is a chain: three columns whose sum depends on the order
    x = np.array([[1.0, 2.0 ** -12, 2.0 ** -12]], np.float32)
    assert K.distances(x, np.zeros((1, 3), np.float32))[0, 0] == np.float32(1.0)        # 1 + 2^-24 is a tie and rounds to the even 1, twice
    assert K.distances(x[:, ::-1], np.zeros((1, 3), np.float32))[0, 0] == np.float32(1.0 + 2.0 ** -23)


def test_the_integer_sampling_against_a_brute_force_prefix():
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 64, 300):
        for trial in range(6):
            mind = rng.random(n).astype(np.float32) * np.float32(10.0 ** rng.integers(-3, 4))
            if trial % 2 and n > 2:
                mind[rng.integers(0, n, 2)] = [np.nan, np.inf]
                mind[rng.integers(0, n)] = 0.0
            q, m = K.quanta(mind)
            fin = np.isfinite(mind)
            assert q.dtype == np.uint64 and (q[~fin] == 0).all() and q.max() <= 1 << 32
            if fin.any() and m > 0:
                assert q[fin].max() == 1 << 32 and m == mind[fin].max()
                for i in np.nonzero(fin)[0]:
                    assert int(q[i]) == int(float(mind[i]) / float(m) * 4294967296.0)   # the header's expression in Python floats
            total = int(q.astype(object).sum())
            assert total < 1 << 56
            if total == 0:
                continue
            targets = {0, total - 1, total // 2} | {K.mulhi64(K.hash64(n, t), total) for t in range(8)}
            csum = np.cumsum(q.astype(object))
            targets |= {int(c) for c in csum[:5]} | {int(c) - 1 for c in csum[:5] if c > 0}          # the boundaries themselves
            for target in sorted(t for t in targets if 0 <= t < total):
                r = K.pick(q, target)
                assert r == K.pick_brute(q, target) and q[r] > 0
    assert K.mulhi64((1 << 64) - 1, 10) == 9 and K.mulhi64(0, 10) == 0 and K.mulhi64(1 << 63, 7) == 3
    # the whole seeding: distinct rows, reproducible, exhausted distinct rows fall back to the lowest row not yet chosen
    x = K.blobs(130, 2, 5, 1.2, 7, scale=4.0)
    rows, mind = K.seed_rows(x, 20, 5)
    assert len(set(rows.tolist())) == 20 and np.array_equal(rows, K.seed_rows(x, 20, 5)[0]) and (mind[rows[:-1]] == 0).all()
    dup = np.repeat(np.array([[0.0, 0.0], [3.0, 4.0]], np.float32), 3, axis=0)           # two distinct rows, six rows
    rows, _ = K.seed_rows(dup, 5, 1)
    assert len(set(rows.tolist())) == 5 and {tuple(dup[r]) for r in rows[:2]} == {(0.0, 0.0), (3.0, 4.0)}
    first = int(rows[0])
    other = int(rows[1])
    assert rows[2:].tolist() == sorted(set(range(6)) - {first, other})[:3]


def test_update_and_shift_orders():
    """The stated orders are orders: the ranges' partial sums differ from one running sum, and the restatement follows the header."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((200, 3)) * 10.0 ** rng.integers(-6, 7, (200, 1))).astype(np.float32)
    labels = rng.integers(-1, 4, 200).astype(np.int32)                                   # -1 and 3: in no centre of k = 3
    old = rng.standard_normal((3, 3)).astype(np.float32)
    new, counts = K.update(x, labels, old)
    assert counts.tolist() == [int((labels == j).sum()) for j in range(3)]
    one, _ = K.update(x, labels, old, waves=1)
    exact = np.array([[math.fsum(x[labels == j, c].tolist()) / int(counts[j]) for c in range(3)] for j in range(3)])
    assert np.abs(new.astype(np.float64) - exact).max() <= np.abs(exact).max() * 2.0 ** -23
    assert np.abs(one.astype(np.float64) - exact).max() <= np.abs(exact).max() * 2.0 ** -23
    labels[:] = 1
    new, counts = K.update(x, labels, old)
    assert counts.tolist() == [0, 200, 0] and new[0].tobytes() == old[0].tobytes() and new[2].tobytes() == old[2].tobytes()
    plain = float(np.sum((new.astype(np.float64) - old) ** 2))
    assert abs(K.shift_of(new, old) - plain) <= 4 * np.spacing(plain) and plain > 0
    assert K.shift_of(old, old) == 0.0


# ---- 3. pinned to scikit-learn ---------------------------------------------------------------------------------------------------------
_RUNS = {}


def _runs(f, tol):
    """(x, start, fp64 run, fp32 run) of a fixture at a tolerance: computed once, shared and left unchanged."""
    if (f.name, tol) not in _RUNS:
        x = f.make()
        start = x[list(f.start)]
        ta = K.tol_abs_of(x, tol)
        _RUNS[f.name, tol] = (x, start, K.lloyd(x.astype(np.float64), start.astype(np.float64), 300, ta, dtype=np.float64), K.lloyd(x, start, 300, ta))
    return _RUNS[f.name, tol]


@pytest.mark.parametrize("f", K.FIXTURES, ids=lambda f: f.name)
def test_fixture_condition_on_the_fp64_restatement(f):
    """In every iteration every row's relative gap between its best and second-best distance is >= 32 d 2^-24, and no cluster is
    ever empty: then the fp32 chain, whose relative error d 2^-24 bounds, takes the same labels."""
    for tol in K.TOLS:
        x, _, r64, _ = _runs(f, tol)
        print(f"[kmeans] {f.name} tol {tol}: n_iter {r64.n_iter}, gap {r64.min_gap:.3e}, condition {K.gap_condition(x.shape[1]):.3e}")
        assert r64.min_gap >= K.gap_condition(x.shape[1]) and not r64.any_empty and r64.stopped
        assert r64.n_iter == f.n_iter[tol]
    assert abs(_runs(f, 0.0)[2].min_gap / f.min_gap - 1) < 1e-3                           # the number written into the case module


@pytest.mark.parametrize("f", K.FIXTURES, ids=lambda f: f.name)
def test_restatements_equal_scikit_learn(f):
    """scikit-learn 1.7.2 KMeans(algorithm="lloyd") on the fp64 copy of the fp32 rows, from the same start array: equal labels and
    n_iter_; fp64 centres within 64 ulp of fp64 at the data's largest magnitude (scikit-learn subtracts the column means before
    it iterates and adds them back, so that is the scale its rounding lives on); the fp32 restatement takes the same labels and
    n_iter and its centres equal the rounded fp64 ones within 1 fp32 ulp."""
    sklearn = pytest.importorskip("sklearn", reason="scikit-learn is the reference of this test")
    from sklearn.cluster import KMeans
    assert sklearn.__version__ == "1.7.2"
    for tol in K.TOLS:
        x, start, r64, r32 = _runs(f, tol)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sk = KMeans(n_clusters=len(f.start), init=start.astype(np.float64), n_init=1, algorithm="lloyd", tol=tol, max_iter=300).fit(x.astype(np.float64))
        assert np.array_equal(sk.labels_, r64.labels) and sk.n_iter_ == r64.n_iter == f.n_iter[tol], (tol, sk.n_iter_, r64.n_iter)
        err = np.abs(sk.cluster_centers_ - r64.cen).max()
        print(f"[kmeans] {f.name} tol {tol}: centres differ by {err:.2e}")
        assert err <= 64 * np.spacing(np.float64(np.abs(x).max()))
        assert abs(sk.inertia_ - float(r64.dist.sum())) <= 1e-12 * sk.inertia_
        assert np.array_equal(r32.labels, r64.labels) and r32.n_iter == r64.n_iter and r32.changed == r64.changed
        rounded = r64.cen.astype(np.float32)
        assert np.abs(r32.cen.view(np.int32).astype(np.int64) - rounded.view(np.int32).astype(np.int64)).max() <= 1


def test_split_and_resume_of_the_restatement():
    f = K.fixture("C-k7")
    x, start, _, whole = _runs(f, 0.0)
    a = K.lloyd(x, start, 4, 0.0)
    assert not a.stopped and a.n_iter == 4
    b = K.lloyd(x, a.cen, 300, 0.0, resume=True, prev=a.prev)
    assert a.n_iter + b.n_iter == whole.n_iter and a.changed + b.changed == whole.changed and a.shift + b.shift == whole.shift
    assert b.cen.tobytes() == whole.cen.tobytes() and np.array_equal(b.labels, whole.labels) and b.dist.tobytes() == whole.dist.tobytes()
    # once changed == 0, further iterations reproduce the state
    again = K.lloyd(x, whole.cen, 3, -1.0, resume=True, prev=whole.prev)
    assert again.changed[0] == 0 and again.cen.tobytes() == whole.cen.tobytes() and np.array_equal(again.prev, whole.prev)

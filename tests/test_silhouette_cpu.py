"""The silhouette entries without a GPU: the boundary of include/vf_hip_silhouette.h (it parses, its three names are exported and
bound type by type through _lib.ENTRIES), every refusal of every entry and of the Python functions, the numpy restatement of tests/silhouette_cases.py against the
definition on exhaustive tiny cases, and the restatement pinned to scikit-learn's silhouette_samples on the fixtures, whose
condition for `nearest` is checked first."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest

from tests import kmeans_cases as K
from tests import silhouette_cases as C
from tests import write_set_cases as W
from tests.conftest import REPO
from tests.test_abi_cpu import _binding_mismatches, _prototypes

ARGS = {"vf_silhouette_sums_l2": 13, "vf_silhouette_sums_dot": 16, "vf_silhouette_finish": 13}
CSRC = os.path.join(REPO, "variantformer_amd", "csrc")


def _header() -> str:
    with open(os.path.join(REPO, "include", "vf_hip_silhouette.h")) as f:
        return f.read()


# ---- 1. header, constants and build lists ------------------------------------------------------------------------------------------
def test_header_parses_and_its_names_are_exported_and_bound_type_by_type():
    from variantformer_amd import _lib, ops
    from variantformer_amd.csrc import build as B
    text = _header()
    declared = _prototypes(text)
    assert sorted(declared) == C.NAMES == W.stream_entries(text)
    assert sorted(_lib.ENTRIES["vf_hip_silhouette.h"]) == C.NAMES, "ctypes binding and vf_hip_silhouette.h disagree"
    assert "vf_silhouette.hip" in B.SOURCES and "vf_silhouette.hip" not in B.EXTRA_FLAGS
    with open(os.path.join(CSRC, "vf_silhouette.hip")) as f:
        source = f.read()
    assert "#pragma clang fp contract(off)" in source, "the sums' bits hold only without an fma"
    assert "hipDeviceSynchronize" not in source and "hipStreamSynchronize" not in source and "hipMemcpy" not in source, \
        "no entry synchronises the stream or reads anything back"
    assert not re.search(r"\b_*(hip_)?atomic\w*\s*\(", source, flags=re.I), "no atomic: every sum has a stated order"
    bound = _lib.load()
    got = {}
    for name in C.NAMES:
        fn = getattr(bound, name)
        assert list(fn.argtypes) == list(_lib.SIGNATURES[name]) and len(fn.argtypes) == ARGS[name], name
        got[name] = (fn.restype, list(fn.argtypes))
    assert _binding_mismatches(declared, got) == []
    # the comparison does notice: an int64_t stride bound as int
    broken = dict(got, vf_silhouette_finish=(ctypes.c_int, [ctypes.c_void_p, ctypes.c_int] + got["vf_silhouette_finish"][1][2:]))
    assert [m.split(":")[0] for m in _binding_mismatches(declared, broken)] == ["vf_silhouette_finish"]
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert _lib.ABI_VERSION == 13 and bound.vf_version() == 13
    for word in ("Arguments", "Write set", "Arithmetic", "Non-finite operands", "Refused before anything is launched", "Not checked"):
        assert text.count(word) >= 3, f"an entry's comment contract has no `{word}` part"
    for phrase in ("t = x[i, c] - x[j, c];  p = t * t;  acc = acc + p", "NO fused", "(((p_0 + p_1) + p_2) .. + p_{W-1})", "ties to the lower c",
                   "a NaN mean never wins", "only constant of this header that enters any bit"):
        assert phrase in text, phrase
    # every macro has its Python mirror
    macros = dict(re.findall(r"#define\s+(VF_SILHOUETTE_[A-Z_]+)\s+([A-Z_0-9]+)\s", src))
    mirror = {"VF_SILHOUETTE_MAX_K": ("VF_KMEANS_MAX_K", C.MAX_K, ops.SILHOUETTE_MAX_K), "VF_SILHOUETTE_MAX_R": ("VF_KMEANS_MAX_R", C.MAX_R, ops.SILHOUETTE_MAX_R),
              "VF_SILHOUETTE_MAX_D": ("VF_KMEANS_MAX_D", C.MAX_D, ops.SILHOUETTE_MAX_D), "VF_SILHOUETTE_RANGES": ("4", C.RANGES, ops.SILHOUETTE_RANGES),
              "VF_SILHOUETTE_ROWS": ("64", C.ROWS, None), "VF_SILHOUETTE_JT": ("8", C.JT, None), "VF_SILHOUETTE_DC_SMALL": ("4", C.DC_SMALL, None),
              "VF_SILHOUETTE_DC": ("32", C.DC, None), "VF_SILHOUETTE_DC_WIDE": ("64", C.DC_WIDE, None)}
    assert set(macros) == set(mirror), sorted(set(macros) ^ set(mirror))
    for macro, (value, case_value, ops_value) in mirror.items():
        assert macros[macro] == value, macro
        expected = {"VF_KMEANS_MAX_K": K.MAX_K, "VF_KMEANS_MAX_R": K.MAX_R, "VF_KMEANS_MAX_D": K.MAX_D}.get(value) or int(value)
        assert case_value == expected and ops_value in (None, expected), macro
    assert re.search(r"#define\s+VF_SILHOUETTE_DOT_WORK_BYTES\(d, k\)\s+\(8 \* \(int64_t\)\(k\) \* \(int64_t\)\(d\)\)", text)
    for d, k in ((1, 1), (49, 50), (64, 1024), (65536, 4096)):
        assert ops.silhouette_dot_work_bytes(d, k) == C.dot_work_bytes(d, k) == 8 * d * k


def test_the_wrappers_allocate_nothing():
    from variantformer_amd import ops
    for name in ("silhouette_sums_l2", "silhouette_sums_dot", "silhouette_finish"):
        src = inspect.getsource(getattr(ops, name))
        assert not re.search(r"torch\.(empty|zeros|ones|full|tensor|arange)", src), name
        assert "nothing is made here" in src


# ---- 2. refusals -------------------------------------------------------------------------------------------------------------------
P = 4096                                                 # a non-null, aligned address; never dereferenced
INVALID = 1


def _err(lib):
    return lib.vf_last_error().decode()


def check_refusals():
    """Every refusal of every entry, its argument named; nothing is launched (tests/test_silhouette_gpu.py runs it on the device too)."""
    from variantformer_amd import _lib
    lib = _lib.load()

    def named(rc, word):
        assert rc == INVALID and _err(lib).split(": ")[1].startswith(word), (word, _err(lib))

    def pointers(call, aligned4, aligned8):
        for name in aligned4 + aligned8:
            assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), (name, _err(lib))
            align = 8 if name in aligned8 else 4
            assert call(**{name: P + align // 2}) == INVALID and re.search(rf"\b{name} must be {align}-byte aligned", _err(lib)), (name, _err(lib))

    def ranges(call):
        for k in (0, -1, C.MAX_K + 1):
            named(call(k=k), "k=")
        named(call(R=-1, row0=0, rows=0), "R=")
        named(call(R=2 ** 24 + 1), "R=")
        named(call(row0=-1), "row0=")
        named(call(rows=-1), "rows=")
        named(call(R=100, row0=60, rows=41, lds=64), "rows=")
        named(call(R=100, row0=101, rows=0), "rows=")
        named(call(rows=40, lds=39), "lds=")

    def sums(call, x, ldx):
        for d in (0, -1, C.MAX_D + 1):
            named(call(d=d, **{ldx: 1 << 20}), "d=")
        named(call(**{ldx: 11}), f"{ldx}=")
        named(call(n=-1), "n=")
        named(call(R=100, n=101), "n=")
        ranges(call)

    def l2(x=P, ldx=12, R=100, d=12, order=P, n=90, seg=P, k=5, row0=0, rows=0, S=P, lds=64):
        return lib.vf_silhouette_sums_l2(x, ldx, R, d, order, n, seg, k, row0, rows, S, lds, 0)
    assert l2() == 0 and l2(R=0, n=0) == 0 and l2(k=C.MAX_K, d=C.MAX_D, ldx=C.MAX_D, R=2 ** 24, row0=2 ** 24) == 0    # rows = 0: nothing launched
    pointers(l2, ("x", "order"), ("seg", "S"))
    sums(l2, "x", "ldx")

    def dot(z=P, ldz=12, R=100, d=12, order=P, n=90, seg=P, k=5, labels=P, row0=0, rows=0, S=P, lds=64, work=P, work_bytes=1 << 40):
        return lib.vf_silhouette_sums_dot(z, ldz, R, d, order, n, seg, k, labels, row0, rows, S, lds, work, work_bytes, 0)
    assert dot() == 0 and dot(work_bytes=C.dot_work_bytes(12, 5)) == 0
    pointers(dot, ("z", "order", "labels"), ("seg", "S", "work"))
    sums(dot, "z", "ldz")
    named(dot(work_bytes=C.dot_work_bytes(12, 5) - 1), "work_bytes=")
    assert str(C.dot_work_bytes(12, 5)) in _err(lib)

    def finish(S=P, lds=64, labels=P, R=100, seg=P, k=5, row0=0, rows=0, a=P, b=P, s=P, nearest=P):
        return lib.vf_silhouette_finish(S, lds, labels, R, seg, k, row0, rows, a, b, s, nearest, 0)
    assert finish() == 0 and finish(R=0) == 0
    pointers(finish, ("labels", "nearest"), ("S", "seg", "a", "b", "s"))
    ranges(finish)


def test_refusals_without_gpu():
    check_refusals()


def test_python_refusals_and_label_encoding_without_gpu():
    from variantformer_amd import validation as V
    x = np.zeros((10, 3), np.float32)
    lab = np.arange(10) % 3
    for kwargs, word in ((dict(metric="manhattan"), "metric"), (dict(standardize="pearson"), "standardize"),
                         (dict(metric="correlation", standardize="cosine"), "goes with metric='euclidean'"), (dict(max_bytes=0), "max_bytes"),
                         (dict(max_bytes=True), "max_bytes"), (dict(max_bytes=1.5), "max_bytes")):
        with pytest.raises(ValueError, match=word):
            V.silhouette_samples(x, lab, **kwargs)
    with pytest.raises(ValueError, match="one per row"):
        V.silhouette_samples(x, lab[:9])
    with pytest.raises(ValueError, match="at least 2"):
        V.silhouette_samples(x, np.zeros(10, int))
    with pytest.raises(ValueError, match="at least 2"):
        V.silhouette_score(x, np.where(lab == 0, 4, -1))                 # the negative labels are no labels: one cluster is left
    with pytest.raises(ValueError, match="at most 4096"):
        V.silhouette_samples(np.zeros((5000, 2), np.float32), np.arange(5000))
    with pytest.raises(ValueError, match="matrix"):
        V.silhouette_samples(np.zeros(7, np.float32), np.arange(7))
    with pytest.raises(TypeError, match="numpy array or a torch tensor"):
        V.silhouette_samples([[0.0, 1.0]], [0])
    for kwargs, word in ((dict(method="dbscan"), "method"), (dict(metric="l1"), "metric"), (dict(method="ward", metric="euclidean"), "correlation"),
                         (dict(method="ward", seed=3), "no further arguments"), (dict(ks=[]), "no cluster count"), (dict(ks=[1]), "2 .. rows - 1"),
                         (dict(ks=[10]), "2 .. rows - 1"), (dict(ks=[2.5]), "2 .. rows - 1"), (dict(ks=[True]), "2 .. rows - 1"), (dict(max_bytes=-1), "max_bytes")):
        with pytest.raises(ValueError, match=word):
            V.silhouette_sweep(x, **{"ks": [2, 3], **kwargs})
    # labels of any dtype go through np.unique; a negative number or a NaN is no label
    codes, classes = V.encode_labels(np.array([7, -1, 3, 7, 10, -5]), 6)
    assert codes.tolist() == [1, -1, 0, 1, 2, -1] and classes.tolist() == [3, 7, 10] and codes.dtype == np.int32
    codes, classes = V.encode_labels(np.array([2.0, np.nan, 0.5, -1.0]), 4)
    assert codes.tolist() == [1, -1, 0, -1] and classes.tolist() == [0.5, 2.0]
    codes, classes = V.encode_labels(np.array(["b", "a", "b", "c"]), 4)
    assert codes.tolist() == [1, 0, 1, 2] and classes.tolist() == ["a", "b", "c"]
    codes, classes = V.encode_labels(np.array(["b", -1, "a", None], dtype=object)[:3], 3)
    assert codes.tolist() == [1, -1, 0] and classes.tolist() == ["a", "b"]
    import torch
    assert V.encode_labels(torch.tensor([4, 4, -1, 9]), 4)[0].tolist() == [0, 0, -1, 1]
    # the chunks follow max_bytes and always advance
    assert V.chunk_rows(18000, 50, 1 << 28) == 18000 and V.chunk_rows(262144, 1024, 1 << 28) == 32768
    assert V.chunk_rows(100, 50, 1) == 1 and V.chunk_rows(100, 2, 8 * 2 * 37) == 37
    codes = C.csr(np.array([1, -1, 0, 1, 2, 0], np.int32), 4)
    assert codes[0].tolist() == [2, 5, 0, 3, 4] and codes[1].tolist() == [0, 2, 4, 5, 5]


# ---- 3. the restatement against the definition ---------------------------------------------------------------------------------------
def _same_rows(got, want):
    for g, w in zip(zip(*got), want):
        for u, v in zip(g[:3], w[:3]):
            assert (np.isnan(u) and np.isnan(v)) or (u == v and np.signbit(u) == np.signbit(v)), (g, w)
        assert int(g[3]) == w[3], (g, w)


def test_exhaustive_tiny_cases_against_the_definition():
    """Five points on the integer line (two of them identical), every labelling from {-1, 0, 1, 2, 3} with k = 4: integer
    distances and sums are exact, so the restatement must equal the definition exactly.  That covers singleton clusters, empty
    cluster ids, rows without a label, identical rows, ties for `nearest` and the labellings with no other cluster."""
    pts = np.array([[0.0], [3.0], [3.0], [6.0], [10.0]], np.float32)
    D = np.abs(pts - pts.T).astype(np.float64).tolist()
    seen = {"singleton": 0, "empty": 0, "tie": 0, "none": 0, "unlabelled": 0}
    for lab in itertools.product((-1, 0, 1, 2, 3), repeat=5):
        lab = np.array(lab, np.int32)
        order, seg = C.csr(lab, 4)
        S = C.sums_l2(pts, order, seg)
        got = C.finish(S, lab, seg)
        want = C.brute(D, lab.tolist(), 4)
        _same_rows(got, want)
        n = np.diff(seg)
        seen["singleton"] += int((n == 1).any())
        seen["empty"] += int((n == 0).any())
        seen["unlabelled"] += int((lab < 0).any())
        seen["none"] += int((got[3] < 0).any())
        means = [[S[c, i] / n[c] for c in range(4) if n[c] and c != lab[i]] for i in range(5)]
        seen["tie"] += int(any(len(m) > 1 and sorted(m)[0] == sorted(m)[1] for m in means))
    assert all(v > 50 for v in seen.values()), seen
    # all rows identical: every distance 0, max(a, b) == 0 and s = +0.0; through the dot family too, on exact rows
    same = np.ones((6, 2), np.float32)
    lab = np.array([0, 0, 1, 1, 1, -1], np.int32)
    r = C.restate(same, lab, 2)
    assert r.a[:5].tolist() == [0.0] * 5 and r.b.tolist() == [0.0] * 6 and r.s[:5].tolist() == [0.0] * 5 and not np.signbit(r.s[:5]).any()
    assert np.isnan(r.s[5]) and np.isnan(r.a[5]) and r.nearest.tolist() == [1, 1, 0, 0, 0, 0]
    z = np.array([[1, 0], [1, 0], [0, 1], [0, 1], [-1, 0], [0, -1]], np.float32)          # unit rows: 1 - z.z' is 0, 1 or 2 exactly
    lab = np.array([0, 0, 1, 1, 2, 5], np.int32)
    order, seg = C.csr(lab, 4)
    S, M = C.sums_dot(z, order, seg, lab)
    assert M.tolist() == [[2, 0], [0, 2], [-1, 0], [0, 0]]
    Dz = (1.0 - z.astype(np.float64) @ z.T.astype(np.float64)).tolist()
    _same_rows(C.finish(S, lab, seg), C.brute(Dz, lab.tolist(), 4))
    assert S[:, 0].tolist() == [0.0, 2.0, 2.0, 0.0] and S[:, 5].tolist() == [2.0, 4.0, 1.0, 0.0]


def test_the_ranges_are_an_order_and_non_finite_operands_follow_ieee():
    rng = np.random.default_rng(5)
    v = (rng.standard_normal(37) * 10.0 ** rng.integers(-8, 9, 37)).astype(np.float64)
    got = C.ranged_sum(v)
    parts = [v[i:i + 10] for i in range(0, 40, 10)]                     # L = ceil(37 / 4) = 10: ranges of 10, 10, 10, 7
    want = 0.0
    for i, p in enumerate(parts):
        acc = 0.0
        for e in p.tolist():
            acc = acc + e
        want = acc if i == 0 else want + acc
    assert got == want and C.ranged_sum(np.zeros(0)) == 0.0 and not np.signbit(C.ranged_sum(np.array([-0.0])))
    assert C.ranged_sum(np.array([1.0, 2.0, 3.0, 4.0, 5.0])) == 15.0    # L = 2: ranges of 2, 2, 1 and an empty one
    assert len({got, float(np.sum(v)), float(np.cumsum(v)[-1])}) > 1, "on this data the order shows"
    x, lab = C.device_case(40, 3, 4, 1, nonfinite=True)
    r = C.restate(x, lab, 4)
    members = np.diff(C.csr(lab, 4)[1]) > 0
    assert not members[3] and (r.S[3] == 0).all() and not np.signbit(r.S[3]).any()                  # an empty cluster id: +0.0
    assert np.isnan(r.s[2]) and np.isnan(r.S[members, 2]).all() and np.isnan(r.S[lab[2]]).all()    # a NaN row: its sums, and its cluster's
    finite = np.isfinite(x).all(axis=1)
    assert 0 <= lab[4] < 4 and not np.isfinite(r.S[lab[4]][finite]).any()                          # an Inf row: +Inf (or the NaN row's NaN) in its cluster's sums
    other = [c for c in range(3) if members[c] and c not in (lab[2], lab[4], lab[39])]
    assert other and np.isfinite(r.S[other][:, finite]).all()


def test_a_row_range_of_the_restatement_is_a_slice_of_the_whole():
    for family in ("l2", "dot"):
        x, lab = C.device_case(130, 5, 3, 2)
        order, seg = C.csr(lab, 3)
        whole = C.sums_l2(x, order, seg) if family == "l2" else C.sums_dot(x, order, seg, lab)[0]
        for row0, rows in ((0, 64), (1, 64), (63, 67), (129, 1)):
            part = C.sums_l2(x, order, seg, row0, rows) if family == "l2" else C.sums_dot(x, order, seg, lab, row0, rows)[0]
            assert C.same_bits(part, whole[:, row0:row0 + rows])
            for g, w in zip(C.finish(part, lab, seg, row0), C.finish(whole, lab, seg)):
                assert C.same_bits(g, w[row0:row0 + rows])


# ---- 4. pinned to scikit-learn ---------------------------------------------------------------------------------------------------------
_RUNS = {}


def _run(f):
    """(restatement, scikit-learn's s, its nearest, the relative gap of its two smallest means): computed once, shared, left unchanged."""
    if f.name not in _RUNS:
        rows, lab, k, _ = f.make()
        _RUNS[f.name] = (C.restate(rows, lab, k, f.family), *C.sklearn_reference(f), lab, k)
    return _RUNS[f.name]


@pytest.mark.parametrize("f", C.FIXTURES, ids=lambda f: f.name)
def test_restatement_equals_scikit_learn(f):
    """scikit-learn 1.7.2 silhouette_samples on the fp64 copy of the same fp32 rows (before standardisation for the dot family,
    with its own metric="correlation" / "cosine"): s within 4 x the measured error; `nearest` equals its argmin, on fixtures on
    which every row's two smallest cluster means differ by more than that tolerance, which is checked first."""
    sklearn = pytest.importorskip("sklearn", reason="scikit-learn is the reference of this test")
    assert sklearn.__version__ == "1.7.2"
    r, s, nearest, gap, lab, k = _run(f)
    keep = lab >= 0
    assert keep.sum() >= 100 and gap[keep].min() > C.TOLERANCE, (f.name, gap[keep].min())       # the condition, on every labelled row
    err = float(np.abs(r.s[keep] - s[keep]).max())
    print(f"[silhouette] {f.name}: largest |s - scikit-learn's| {err:.3e}, smallest relative gap of two means {gap[keep].min():.3e}")
    assert err <= C.TOLERANCE
    assert np.array_equal(r.nearest[keep], nearest[keep])
    assert np.isnan(r.s[~keep]).all() and (r.nearest[~keep] >= 0).all()
    from sklearn.metrics import silhouette_score
    _, _, _, ref = f.make()
    assert abs(C.score_of(r.s, lab, k) - silhouette_score(ref[keep].astype(np.float64), lab[keep], metric=f.metric)) <= C.TOLERANCE


def test_the_measured_error_is_the_largest_of_the_fixtures():
    pytest.importorskip("sklearn", reason="scikit-learn is the reference of this test")
    worst = max(float(np.abs(_run(f)[0].s[_run(f)[4] >= 0] - _run(f)[1][_run(f)[4] >= 0]).max()) for f in C.FIXTURES)
    assert 0.9 * C.MEASURED_ERROR <= worst <= C.MEASURED_ERROR and C.TOLERANCE == 4 * C.MEASURED_ERROR, worst


# ---- 5. the sweep ------------------------------------------------------------------------------------------------------------------------
def test_sweep_on_separated_blobs_peaks_at_the_planted_count():
    """5 well-separated clusters, 300 x 7: the restated chain -- D^2 seeding and Lloyd's loop of tests/kmeans_cases.py scored by the
    Euclidean sums, and a Ward tree on correlation distances scored by the linear sums -- has its largest score at k = 5
    (tests/test_silhouette_gpu.py holds validation.silhouette_sweep to the same on the device)."""
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import pdist
    x = C.sweep_blobs()
    ks = list(range(2, 9))
    scores = []
    for k in ks:
        rows, _ = K.seed_rows(x, k, 0)
        run = K.lloyd(x, x[rows], 300, K.tol_abs_of(x, 1e-4))
        scores.append(C.score_of(C.restate(x, run.labels, k).s, run.labels, k))
    print("[silhouette] k-means sweep:", [f"{s:.3f}" for s in scores])
    assert ks[int(np.argmax(scores))] == 5
    z = C.standardize32(x)
    Z = hierarchy.linkage(pdist(x.astype(np.float64), metric="correlation"), method="ward")
    scores = []
    for k in ks:
        lab = (hierarchy.fcluster(Z, k, criterion="maxclust") - 1).astype(np.int32)
        scores.append(C.score_of(C.restate(z, lab, k, "dot").s, lab, k))
    print("[silhouette] Ward sweep:", [f"{s:.3f}" for s in scores])
    assert ks[int(np.argmax(scores))] == 5

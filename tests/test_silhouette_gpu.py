"""The silhouette entries on the GPU against the numpy restatement of tests/silhouette_cases.py, BIT FOR BIT (a NaN equals any
NaN): the sums of both families, the clusters' column sums, a, b, s and nearest; on both sides of every tile constant, with
strided operands, a cluster larger than a staged tile, a singleton, an empty cluster id, rows without a label, NaN and Inf rows;
row ranges that start off a multiple of 64 against the whole call, two runs, every refusal; and the pipeline end to end against
scikit-learn, through the sweep and through VCFProcessor.expression_silhouette.  The restatement itself is pinned to scikit-learn
in tests/test_silhouette_cpu.py."""
import numpy as np
import pytest
import torch

from tests import silhouette_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from variantformer_amd import _lib as lib
    lib.load()      # must be the in-tree HIP library; raises if missing


def _ops():
    from variantformer_amd import ops
    return ops


def _dev(a, pad=0):
    """The array on the device; pad > 0: as the first columns of a wider buffer whose other columns are NaN (a strided operand)."""
    a = np.ascontiguousarray(a)
    if not pad:
        return torch.from_numpy(a).cuda()
    wide = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return wide[:, :a.shape[1]]


def _empty(shape, dtype):
    """A buffer of the shape whose every byte is the sentinel: what an entry does not write keeps it."""
    shape = shape if isinstance(shape, tuple) else (shape,)
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda").view(dtype).reshape(shape)


def _untouched(t) -> bool:
    return bool((t.contiguous().view(torch.uint8) == SENTINEL).all())


def run_entries(x, lab, k, family, row0=0, rows=None, xpad=0, spad=0):
    """The sums entry of the family and vf_silhouette_finish over [row0, row0 + rows) into sentinel-filled buffers: numpy arrays
    S [k, rows], M (dot), and a, b, s, nearest [R] whole."""
    ops = _ops()
    R, d = x.shape
    rows = R - row0 if rows is None else rows
    order, seg = C.csr(lab, k)
    xd, od, sd, ld = _dev(x, xpad), _dev(order), _dev(seg), _dev(np.asarray(lab, np.int32))
    wide = _empty((k, rows + spad), torch.float64)
    S = wide[:, :rows]
    out = {}
    if family == "l2":
        ops.silhouette_sums_l2(xd, od, sd, row0, rows, S=S)
    else:
        work = _empty(C.dot_work_bytes(d, k) // 8 + 3, torch.float64)
        ops.silhouette_sums_dot(xd, od, sd, ld, row0, rows, S=S, work=work)
        out["M"] = work[:k * d].reshape(k, d).cpu().numpy()
        assert rows == 0 or _untouched(work[k * d:])
    a, b, s, nearest = _empty(R, torch.float64), _empty(R, torch.float64), _empty(R, torch.float64), _empty(R, torch.int32)
    ops.silhouette_finish(S, ld, sd, row0, rows, a=a, b=b, s=s, nearest=nearest)
    assert spad == 0 or _untouched(wide[:, rows:])
    for t in (a, b, s, nearest):
        assert _untouched(t[:row0]) and _untouched(t[row0 + rows:])
    out.update(S=S.cpu().numpy(), a=a.cpu().numpy(), b=b.cpu().numpy(), s=s.cpu().numpy(), nearest=nearest.cpu().numpy())
    return out


def _check(got, x, lab, k, family, what, row0=0, rows=None):
    rows = x.shape[0] - row0 if rows is None else rows
    order, seg = C.csr(lab, k)
    if family == "l2":
        S = C.sums_l2(x, order, seg, row0, rows)
    else:
        S, M = C.sums_dot(x, order, seg, lab, row0, rows)
        assert C.same_bits(got["M"], M), (what, "M")
    assert C.same_bits(got["S"], S), (what, "S", np.argwhere(got["S"] != S)[:4].tolist())
    for name, want in zip(("a", "b", "s", "nearest"), C.finish(S, lab, seg, row0)):
        assert C.same_bits(got[name][row0:row0 + rows], want), (what, name)


# d on both sides of the three column chunks (4, 32, 64) and of two wide chunks; k below, at and past a staged tile of 32 clusters
DS = (1, 2, 3, 4, 5, 33, 49, 70)
KS = (2, 3, 70)


@pytest.mark.parametrize("R", (1, 2, 63, 64, 65, 130, 600))
def test_every_entry_equals_the_restatement_bit_for_bit(R):
    """R on both sides of a block of 64 query rows and past several; every d and k of the table; ld > d and lds > rows on every
    other case; NaN and Inf rows on every other case; rows without a label, a singleton, an empty id and (R >= 100) a cluster of
    R / 2 rows, more than the 32 members of a staged tile, in every case with R >= 8."""
    for d in DS:
        for k in KS:
            odd = (d + k) % 2 == 1
            x, lab = C.device_case(R, d, k, 1000 * R + 10 * d + k, nonfinite=odd)
            for family in ("l2", "dot"):
                got = run_entries(x, lab, k, family, xpad=3 if odd else 0, spad=5 if odd else 0)
                _check(got, x, lab, k, family, (R, d, k, family))
    if R >= 100:
        assert np.bincount(lab[lab >= 0], minlength=k)[0] > C.RANGES * C.JT and (np.bincount(lab[(lab >= 0) & (lab < k)], minlength=k) == 1).any()


@pytest.mark.parametrize("d", (32, 64, 65, 129))
def test_the_chunk_boundaries_themselves(d):
    x, lab = C.device_case(130, d, 5, d, nonfinite=d == 65)
    for family in ("l2", "dot"):
        _check(run_entries(x, lab, 5, family, xpad=1), x, lab, 5, family, (d, family))


def test_row_ranges_equal_the_whole_call_and_two_runs_are_equal():
    for d, k in ((5, 3), (70, 33), (2, 70)):
        x, lab = C.device_case(600, d, k, d + k)
        for family in ("l2", "dot"):
            whole = run_entries(x, lab, k, family)
            _check(whole, x, lab, k, family, (d, k, family))
            again = run_entries(x, lab, k, family)
            assert all(C.same_bits(again[key], whole[key]) for key in whole), (d, k, family)
            for row0, rows in ((1, 64), (63, 130), (37, 500), (599, 1), (64, 0)):
                part = run_entries(x, lab, k, family, row0, rows, spad=2)
                assert C.same_bits(part["S"], whole["S"][:, row0:row0 + rows]), (d, k, family, row0, rows)
                for key in ("a", "b", "s", "nearest"):
                    assert C.same_bits(part[key][row0:row0 + rows], whole[key][row0:row0 + rows]), (key, row0, rows)


def test_special_cases_of_the_definition_on_the_device():
    """All rows identical (max(a, b) == 0: s = +0.0), ties for nearest to the lower cluster, no other non-empty cluster (b and s
    NaN, nearest -1), a singleton (a = s = +0.0), a row whose label is outside 0 .. k - 1 (a and s NaN, b over all clusters)."""
    same = np.ones((70, 2), np.float32)
    lab = (np.arange(70) % 3).astype(np.int32)
    lab[69] = -1
    got = run_entries(same, lab, 4, "l2")
    _check(got, same, lab, 4, "l2", "identical")
    assert (got["s"][:69] == 0).all() and not np.signbit(got["s"][:69]).any() and np.isnan(got["s"][69]) and np.isnan(got["a"][69])
    assert got["nearest"].tolist() == [1 if l == 0 else 0 for l in lab.tolist()] and (got["b"] == 0).all()
    x, _ = C.device_case(40, 3, 2, 7)
    lone = np.zeros(40, np.int32)
    lone[11] = 5
    for family in ("l2", "dot"):
        got = run_entries(x, lone, 3, family)
        _check(got, x, lone, 3, family, "one cluster")
        keep = np.arange(40) != 11
        assert np.isnan(got["b"][keep]).all() and np.isnan(got["s"][keep]).all() and (got["nearest"][keep] == -1).all()
        assert got["nearest"][11] == 0 and np.isnan(got["a"][11]) and np.isfinite(got["b"][11])
    lone[11] = 2                                                          # a singleton beside the large cluster
    got = run_entries(x, lone, 3, "l2")
    _check(got, x, lone, 3, "l2", "singleton")
    assert got["a"][11] == 0 and got["s"][11] == 0 and got["nearest"][11] == 0 and (got["nearest"][np.arange(40) != 11] == 2).all()


def test_refusals_on_the_device():
    from tests.test_silhouette_cpu import check_refusals
    check_refusals()
    ops = _ops()
    x, lab = C.device_case(20, 3, 2, 1)
    order, seg = C.csr(lab, 2)
    xd, od, sd, ld = _dev(x), _dev(order), _dev(seg), _dev(lab)
    with pytest.raises(AssertionError):
        ops.silhouette_sums_l2(xd, od, sd, 0, 20, S=_empty((2, 19), torch.float64))
    with pytest.raises(AssertionError):
        ops.silhouette_sums_l2(xd, od, sd, 5, 16, S=_empty((2, 16), torch.float64))
    with pytest.raises(AssertionError):
        ops.silhouette_finish(_empty((2, 20), torch.float64), ld, sd, 0, 20, a=_empty(20, torch.float64), b=_empty(20, torch.float64),
                              s=_empty(19, torch.float64), nearest=_empty(20, torch.int32))
    with pytest.raises(ops._lib.VFError, match="work_bytes"):
        ops.silhouette_sums_dot(xd, od, sd, ld, 0, 20, S=_empty((2, 20), torch.float64), work=_empty(5, torch.float64))
    with pytest.raises(ops._lib.VFError):
        ops.silhouette_sums_l2(torch.from_numpy(x), od, sd, 0, 20, S=_empty((2, 20), torch.float64))


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------
def _blobs(R, d, g, seed):
    from tests import kmeans_cases as K
    return K.blobs(R, d, g, 0.8, seed, scale=2.0), (np.arange(R) % g).astype(np.int64)


@pytest.mark.parametrize("shape", [(600, 49, "correlation"), (600, 49, "euclidean"), (600, 2, "euclidean"), (600, 49, "cosine")], ids=str)
def test_silhouette_samples_against_scikit_learn(shape):
    """validation.silhouette_samples against scikit-learn 1.7.2 on the fp64 copy of the same fp32 rows, within the tolerance
    measured on the CPU (tests/silhouette_cases.py); labels that are no 0 .. k - 1, rows without a label, chunks of any size."""
    from sklearn.metrics import silhouette_samples, silhouette_score
    from variantformer_amd import validation as V
    R, d, metric = shape
    x, true = _blobs(R, d, 6, R + d)
    labels = np.array([3, 8, 15, 16, 23, 42])[true]
    labels[::41] = -1
    keep = labels >= 0
    want = silhouette_samples(x[keep].astype(np.float64), labels[keep], metric=metric)
    res = V.silhouette_samples(x, labels, metric=metric, nan_to_zero=False)
    err = float(np.abs(res.samples[keep] - want).max())
    print(f"[silhouette] {shape}: largest |s - scikit-learn's| {err:.3e} (tolerance {C.TOLERANCE:.3e}), score {res.score:.6f}")
    assert err <= C.TOLERANCE
    assert isinstance(res.samples, np.ndarray) and res.samples.dtype == np.float64 and np.isnan(res.samples[~keep]).all() and np.isnan(res.a[~keep]).all()
    assert abs(res.score - silhouette_score(x[keep].astype(np.float64), labels[keep], metric=metric)) <= C.TOLERANCE
    assert res.classes.tolist() == [3, 8, 15, 16, 23, 42] and res.cluster_sizes.sum() == keep.sum() and set(res.nearest.tolist()) <= set(res.classes.tolist())
    assert (res.nearest[keep] != labels[keep]).all() and np.array_equal(res.classes[res.nearest_index], res.nearest)
    assert abs(float(np.average(res.cluster_means, weights=res.cluster_sizes)) - res.score) < 1e-12
    # the chunks do not enter the result; tensors in, tensors out
    for max_bytes in (8 * 6 * 64, 8 * 6 * 37, 1):
        again = V.silhouette_samples(x, labels, metric=metric, nan_to_zero=False, max_bytes=max_bytes)
        assert all(C.same_bits(getattr(again, f), getattr(res, f)) for f in ("samples", "a", "b", "nearest_index")) and again.score == res.score
    t = V.silhouette_samples(torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda(), metric=metric, nan_to_zero=False)
    assert isinstance(t.samples, torch.Tensor) and t.samples.is_cuda and C.same_bits(t.samples.cpu().numpy(), res.samples)
    assert V.silhouette_score(x, labels, metric=metric, nan_to_zero=False) == res.score


def test_the_pipeline_equals_the_restatement_and_standardize_is_kmeans_space():
    from variantformer_amd import neighbors, validation as V
    x, true = _blobs(300, 12, 5, 4)
    lab = true.astype(np.int32)
    z = neighbors.standardize(x, "correlation")[0].cpu().numpy()
    for metric, standardize, rows, family in (("euclidean", None, x, "l2"), ("euclidean", "correlation", z, "l2"), ("correlation", None, z, "dot")):
        res = V.silhouette_samples(x, lab, metric=metric, standardize=standardize)
        want = C.restate(rows, lab, 5, family)
        for got, ref in ((res.samples, want.s), (res.a, want.a), (res.b, want.b), (res.nearest_index, want.nearest)):
            assert C.same_bits(got, ref), (metric, standardize)
        assert res.score == C.score_of(want.s, lab, 5)
    # on standardised rows |a - b|^2 = 2 (1 - corr): the two scores rank alike but are not the same number
    assert V.silhouette_score(x, lab, "euclidean", "correlation") != V.silhouette_score(x, lab, "correlation")
    with pytest.raises(ValueError, match="at least 2"):
        V.silhouette_samples(x, np.zeros(300, int))


def test_sweep_on_separated_blobs_peaks_at_the_planted_count():
    from variantformer_amd import validation as V
    x = C.sweep_blobs()
    ks = list(range(2, 9))
    for method, metric in (("kmeans", "euclidean"), ("kmeans", "correlation"), ("ward", "correlation")):
        res = V.silhouette_sweep(x, ks, method=method, metric=metric)
        print(f"[silhouette] sweep {method} {metric}:", [f"{s:.3f}" for s in res.scores])
        assert res.ks == ks and res.best_k == 5 == ks[int(np.argmax(res.scores))], (method, metric, res.scores)
        assert len(res.labels) == len(ks) and all(l.shape == (300,) and l.dtype == np.int32 for l in res.labels)
        assert (res.inertia is None) == (method == "ward") and (method == "ward" or len(res.inertia) == len(ks))
    one = V.silhouette_sweep(x, 5, method="kmeans", metric="euclidean", seed=3)
    assert one.ks == [5] and one.best_k == 5


def test_expression_silhouette_on_a_frame_after_expression_kmeans():
    from tests.test_expression_enrichment_gpu import GROUPS, _frame, _proc
    from variantformer_amd import validation as V
    proc = _proc()
    frame, _, group = _frame()
    proc.expression_kmeans(frame, GROUPS, seed=1)
    score = proc.expression_silhouette(frame)
    x = np.stack(list(frame["predicted_expression"])).astype(np.float32)
    direct = V.silhouette_samples(x, frame["kmeans_cluster"].to_numpy(), metric="correlation")
    assert isinstance(score, float) and score == direct.score and score > 0.5
    assert list(frame.columns[-2:]) == ["silhouette", "silhouette_neighbor_cluster"] and frame["silhouette"].dtype == np.float64
    assert C.same_bits(frame["silhouette"].to_numpy(), direct.samples) and frame["silhouette_neighbor_cluster"].tolist() == direct.nearest.tolist()
    assert (frame["silhouette_neighbor_cluster"] != frame["kmeans_cluster"]).all()
    # an array of labels, a negative one among them; another metric; coordinates
    lab = group.astype(np.int64).copy()
    lab[0] = -1
    again = proc.expression_silhouette(frame, labels=lab, metric="euclidean", standardize="correlation")
    assert np.isnan(frame["silhouette"].iloc[0]) and again == V.silhouette_score(x, lab, "euclidean", "correlation")
    frame["umap_1"], frame["umap_2"] = x[:, 0], x[:, 1]
    on_umap = proc.expression_silhouette(frame, on="umap")
    assert on_umap == V.silhouette_score(np.ascontiguousarray(x[:, :2]), frame["kmeans_cluster"].to_numpy(), "euclidean")
    with pytest.raises(ValueError, match="metric"):
        proc.expression_silhouette(frame, on="umap", metric="correlation")
    with pytest.raises(ValueError, match="no `clusters` column"):
        proc.expression_silhouette(frame, labels="clusters")
    sweep = proc.expression_silhouette_sweep(frame, [2, 3, GROUPS, GROUPS + 2], seed=1)
    assert list(sweep.columns) == ["k", "silhouette_score", "inertia"] and sweep["k"].tolist() == [2, 3, GROUPS, GROUPS + 2]
    assert sweep.attrs["best_k"] == GROUPS and sweep.attrs["labels"][GROUPS].shape == (len(frame),)
    ward = proc.expression_silhouette_sweep(frame, [2, GROUPS, GROUPS + 3], method="ward")
    assert list(ward.columns) == ["k", "silhouette_score"] and ward.attrs["best_k"] == GROUPS

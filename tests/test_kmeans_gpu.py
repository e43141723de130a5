"""The k-means entries on the GPU against the fp32 restatement of tests/kmeans_cases.py, BIT FOR BIT: labels, distance bits,
centre bits, counts, changed, shift, n_iter and the seeded rows; on both sides of every tile constant, with strided operands,
ties, NaN and Inf rows, a NaN centre and an empty cluster; the stops at the restatement's n_iter with the buffers past them
untouched, split and resume, two runs, chunked predict, every refusal; and the pipeline end to end on the three fixtures, through
VCFProcessor.expression_kmeans and on into expression_enrichment.  The restatement itself is pinned to scikit-learn in
tests/test_kmeans_cpu.py."""
import warnings

import numpy as np
import pytest
import torch

from tests import kmeans_cases as K

pytestmark = pytest.mark.gpu


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


def _empty(shape, dtype, byte=0xA5):
    """A buffer of the shape whose every byte is the sentinel: what an entry does not write keeps it."""
    shape = shape if isinstance(shape, tuple) else (shape,)
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((n,), byte, dtype=torch.uint8, device="cuda").view(dtype).reshape(shape)


def _bits(t):
    t = t.detach().cpu().contiguous() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return (t.numpy() if isinstance(t, torch.Tensor) else t).tobytes()


def _data(R, d, k, seed, spread=3.0):
    rng = np.random.default_rng(seed)
    cen = (rng.standard_normal((k, d)) * spread).astype(np.float32)
    x = (cen[rng.integers(0, k, R)] + rng.standard_normal((R, d))).astype(np.float32)
    return x, cen


def _assign(x, cen, xpad=0, cpad=0):
    R = x.shape[0]
    labels, dist = _empty(R, torch.int32), _empty(R, torch.float32)
    _ops().kmeans_assign(_dev(x, xpad), _dev(cen, cpad), labels=labels, dist=dist)
    return labels.cpu().numpy(), dist.cpu().numpy()


# R on both sides of a block (64) and past one; d on both sides of both column chunks (4, 32) and of two chunks (64); k on both sides
# of a wavefront's tile (8), of a staged tile (32) and past several (257)
ASSIGN_SHAPES = [(1, 1, 1), (63, 2, 2), (64, 3, 7), (65, 4, 8), (257, 5, 9), (65, 31, 31), (64, 32, 32), (63, 33, 33), (257, 49, 50),
                 (1025, 65, 257), (130, 64, 5), (1025, 2, 257)]


@pytest.mark.parametrize("shape", ASSIGN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_assign_equals_the_restatement_bit_for_bit(shape):
    R, d, k = shape
    x, cen = _data(R, d, k, sum(shape))
    want_l, want_d = K.assign(x, cen)
    for xpad, cpad in ((0, 0), (3, 5)):
        got_l, got_d = _assign(x, cen, xpad, cpad)
        assert np.array_equal(got_l, want_l) and _bits(got_d) == _bits(want_d), (shape, xpad, cpad)
    assert k == 1 or len(set(want_l.tolist())) > 1


def test_assign_ties_and_non_finite_operands():
    """Integer-valued rows and duplicate centres: real ties, to the lower j, across wavefronts' tiles and staged tiles; a NaN row has
    no winner, an Inf row takes the lowest finite centre at +Inf, a NaN centre is never chosen."""
    rng = np.random.default_rng(11)
    base = rng.integers(-3, 4, (12, 3)).astype(np.float32)
    cen = base[rng.integers(0, 12, 70)]                                   # 70 centres, many of them equal: ties 8, 32 and more apart
    cen[[0, 9, 33]] = np.nan
    cen[40, 1] = np.inf
    x = rng.integers(-3, 4, (200, 3)).astype(np.float32)
    x[:70] = np.nan_to_num(cen, nan=1.0, posinf=2.0)                      # duplicate rows, each on top of a centre
    x[5] = np.nan
    x[6, 2] = np.nan
    x[7, 0] = np.inf
    x[8] = -np.inf
    want_l, want_d = K.assign(x, cen)
    got_l, got_d = _assign(x, cen)
    assert np.array_equal(got_l, want_l) and _bits(got_d) == _bits(want_d)
    assert want_l[5] == want_l[6] == -1 and got_d.view(np.uint32)[5] == K.NAN_BITS and want_l[7] == 1 and np.isinf(got_d[7])
    assert not np.isin(want_l, [0, 9, 33]).any() and (want_d[10:33] == 0).all()                    # rows on top of finite centres
    lone = np.full((1, 3), np.nan, np.float32)                            # every centre NaN: no row has a winner
    got_l, got_d = _assign(x, lone)
    assert (got_l == -1).all() and (got_d.view(np.uint32) == K.NAN_BITS).all()


UPDATE_SHAPES = [(1, 1, 1), (5, 2, 2), (63, 33, 7), (64, 64, 9), (65, 65, 33), (257, 49, 50), (1025, 129, 257)]


@pytest.mark.parametrize("shape", UPDATE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_update_equals_the_restatement_bit_for_bit(shape):
    """R below the sixteen row ranges and past them; d on both sides of a column tile and of two; labels outside 0 .. k - 1 in no
    centre; an empty cluster keeps its bits; in place equals out of place."""
    R, d, k = shape
    rng = np.random.default_rng(sum(shape))
    x = (rng.standard_normal((R, d)) * 10.0 ** rng.integers(-3, 4, (R, 1))).astype(np.float32)
    labels = rng.integers(-1, k + 1, R).astype(np.int32)                  # -1 and k: in no centre
    if k > 2:
        labels[labels == 1] = 0                                           # cluster 1 is empty
    old = rng.standard_normal((k, d)).astype(np.float32)
    want_c, want_n = K.update(x, labels, old)
    for xpad, cpad in ((0, 0), (2, 7)):
        new, counts = _dev(np.full((k, d), 7.0, np.float32), cpad), _empty(k, torch.int32)
        _ops().kmeans_update(_dev(x, xpad), _dev(labels), _dev(old, cpad), cen_new=new, counts=counts)
        assert _bits(new) == _bits(want_c) and np.array_equal(counts.cpu().numpy(), want_n), (shape, xpad, cpad)
    inplace, counts = _dev(old, 1), _empty(k, torch.int32)
    _ops().kmeans_update(_dev(x), _dev(labels), inplace, cen_new=inplace, counts=counts)
    assert _bits(inplace) == _bits(want_c) and np.array_equal(counts.cpu().numpy(), want_n)
    if k > 2:
        assert want_n[1] == 0 and _bits(want_c[1]) == _bits(old[1])


def _lloyd(x, cen, max_iter, tol_abs, resume=False, prev=None, xpad=0, cpad=0):
    """vf_kmeans_lloyd into sentinel-filled buffers: a dict of numpy arrays."""
    ops = _ops()
    R, d = x.shape
    k = cen.shape[0]
    c = _dev(cen, cpad)
    out = dict(labels=_empty(R, torch.int32), dist=_empty(R, torch.float32), prev=_dev(prev) if resume else _empty(R, torch.int32),
               counts=_empty(k, torch.int32), n_iter=_empty(1, torch.int32), shift=_empty(max_iter, torch.float64),
               changed=_empty(max_iter, torch.int64))
    work = _empty((ops.kmeans_lloyd_work_bytes(R, d, k) + 7) // 8, torch.int64)
    ops.kmeans_lloyd(_dev(x, xpad), c, max_iter=max_iter, tol_abs=tol_abs, resume=resume, labels=out["labels"], dist=out["dist"],
                     prev_labels=out["prev"], counts=out["counts"], n_iter=out["n_iter"], shift=out["shift"], changed=out["changed"], work=work)
    res = {key: v.cpu().numpy() for key, v in out.items()}
    res["cen"] = c.cpu().numpy().copy()
    return res


SENTINEL64 = np.frombuffer(bytes([0xA5] * 8), dtype=np.int64)[0]


def _check_run(got, want, max_iter, what):
    n = int(got["n_iter"][0])
    assert n == want.n_iter, (what, n, want.n_iter)
    assert got["changed"][:n].tolist() == want.changed and _bits(got["shift"][:n]) == _bits(np.array(want.shift, np.float64)), what
    # past the stop nothing was written
    assert (got["changed"][n:] == SENTINEL64).all() and (got["shift"][n:].view(np.int64) == SENTINEL64).all(), what
    assert _bits(got["cen"]) == _bits(want.cen), what
    assert np.array_equal(got["labels"], want.labels) and _bits(got["dist"]) == _bits(want.dist), what
    assert np.array_equal(got["prev"], want.prev) and np.array_equal(got["counts"], want.counts), what


@pytest.mark.parametrize("f", K.FIXTURES, ids=lambda f: f.name)
def test_lloyd_equals_the_restatement_and_stops_where_it_stops(f):
    """Stop by labels (tol 0) and by tolerance, max_iter well above both; the iterations scikit-learn takes (the numbers of the
    case module, pinned in tests/test_kmeans_cpu.py); max_iter below convergence; a then b equals a + b; two runs are equal."""
    x = f.make()
    start = x[list(f.start)]
    runs = {}
    for tol in (0.0, 1e-2, 1e-1):
        ta = K.tol_abs_of(x, tol)
        want = K.lloyd(x, start, 40, ta)
        got = runs[tol] = _lloyd(x, start, 40, ta)
        _check_run(got, want, 40, (f.name, tol))
        assert want.stopped and want.n_iter == f.n_iter[tol] < 40
    whole = K.lloyd(x, start, 40, 0.0)
    assert whole.changed[-1] == 0 and np.array_equal(runs[0.0]["labels"], runs[0.0]["prev"])       # a stop by labels: the same bits again
    assert f.n_iter[1e-1] < f.n_iter[0.0] and K.lloyd(x, start, 40, K.tol_abs_of(x, 1e-1)).changed[-1] > 0   # a stop by tolerance
    again = _lloyd(x, start, 40, 0.0)
    assert all(_bits(again[key]) == _bits(runs[0.0][key]) for key in again)
    a = 2
    first = _lloyd(x, start, a, 0.0, xpad=1, cpad=3)
    _check_run(first, K.lloyd(x, start, a, 0.0), a, (f.name, "max_iter below convergence"))
    assert int(first["n_iter"][0]) == a < whole.n_iter
    second = _lloyd(x, first["cen"], 40, 0.0, resume=True, prev=first["prev"])
    n = int(second["n_iter"][0])
    assert a + n == whole.n_iter and first["changed"][:a].tolist() + second["changed"][:n].tolist() == whole.changed
    assert _bits(np.concatenate([first["shift"][:a], second["shift"][:n]])) == _bits(np.array(whole.shift))
    for key in ("cen", "labels", "dist", "prev", "counts"):
        assert _bits(second[key]) == _bits(runs[0.0][key]), key


def test_lloyd_with_a_nan_row_an_empty_cluster_and_no_iterations():
    x, _ = _data(300, 33, 6, 4)
    x[17, 5] = np.nan
    start = x[[0, 1, 2, 3, 4, 19]].copy()
    start[5] += 1000.0                                                    # nobody's nearest centre: it keeps its bits
    want = K.lloyd(x, start, 30, 0.0)
    got = _lloyd(x, start, 30, 0.0)
    _check_run(got, want, 30, "nan-row")
    assert want.labels[17] == -1 and want.counts[5] == 0 and _bits(want.cen[5]) == _bits(start[5]) and want.stopped
    none = _lloyd(x, start, 0, 0.0)
    assert int(none["n_iter"][0]) == 0 and _bits(none["cen"]) == _bits(start)
    first = K.assign(x, start)
    assert np.array_equal(none["labels"], first[0]) and _bits(none["dist"]) == _bits(first[1])


SEED_SHAPES = [(1, 1, 1, 0), (65, 2, 9, 1), (257, 33, 33, 2), (1025, 5, 64, 3), (300, 49, 50, 42), (513, 65, 8, 2 ** 40 + 7)]


def _seed(x, k, seed, xpad=0, cpad=0):
    ops = _ops()
    R, d = x.shape
    rows, mind = _empty(k, torch.int32), _empty(R, torch.float32)
    cen = _dev(np.zeros((k, d), np.float32), cpad)
    work = _empty((ops.kmeans_seed_work_bytes(R) + 7) // 8, torch.int64)
    ops.kmeans_seed(_dev(x, xpad), k, seed, rows=rows, cen=cen, mind=mind, work=work)
    return rows.cpu().numpy(), cen.cpu().numpy(), mind.cpu().numpy()


@pytest.mark.parametrize("shape", SEED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_seeding_equals_the_restatement_bit_for_bit(shape):
    R, d, k, seed = shape
    x, _ = _data(R, d, max(k // 2, 1), R + k)
    want_rows, want_mind = K.seed_rows(x, k, seed)
    for xpad, cpad in ((0, 0), (5, 2)):
        rows, cen, mind = _seed(x, k, seed, xpad, cpad)
        assert np.array_equal(rows, want_rows), (shape, rows, want_rows)
        assert _bits(cen) == _bits(x[want_rows]) and (k == 1 or _bits(mind) == _bits(want_mind))
    assert len(set(want_rows.tolist())) == k


def test_seeding_with_duplicate_and_non_finite_rows():
    """Fewer distinct finite rows than k: once every mind is 0 the lowest row not yet chosen is taken; NaN and Inf rows have q = 0."""
    x = np.repeat(np.array([[0.0, 0.0], [3.0, 4.0], [-6.0, 8.0]], np.float32), 4, axis=0)
    x[5] = np.nan
    x[10, 1] = np.inf
    for seed in (0, 1, 2):
        want_rows, want_mind = K.seed_rows(x, 9, seed)
        rows, cen, mind = _seed(x, 9, seed)
        assert np.array_equal(rows, want_rows) and _bits(mind) == _bits(want_mind) and _bits(cen) == _bits(x[want_rows])
        assert len(set(rows.tolist())) == 9


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", K.FIXTURES, ids=lambda f: f.name)
def test_kmeans_end_to_end_equals_scikit_learn_on_the_fixtures(f):
    from variantformer_amd import kmeans
    x = f.make()
    start = x[list(f.start)]
    for tol in (0.0, 1e-4, 1e-2, 1e-1):
        with warnings.catch_warnings():
            warnings.simplefilter("error")                                # no cluster ends empty
            model = kmeans.kmeans(x, len(f.start), metric="euclidean", init=start, tol=tol, nan_to_zero=False)
        want = K.lloyd(x, start, 300, K.tol_abs_of(x, tol))
        assert model.n_iter == want.n_iter == f.n_iter[tol], (tol, model.n_iter)
        assert isinstance(model.labels, np.ndarray) and np.array_equal(model.labels, want.labels) and _bits(model.centers) == _bits(want.cen)
        assert model.inertia == float(want.dist.astype(np.float64).sum()) or abs(model.inertia / float(want.dist.astype(np.float64).sum()) - 1) < 1e-12
        assert np.array_equal(model.counts, np.bincount(want.labels, minlength=len(f.start)))
        try:
            from sklearn.cluster import KMeans
        except ImportError:
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sk = KMeans(n_clusters=len(f.start), init=start.astype(np.float64), n_init=1, algorithm="lloyd", tol=tol).fit(x.astype(np.float64))
        assert np.array_equal(model.labels, sk.labels_) and model.n_iter == sk.n_iter_
    # predict: an assignment alone, in chunks or whole, from a restored model
    q, _ = _data(301, x.shape[1], 3, 9)
    whole, dist = model.predict(q, return_distance=True)
    want_l, want_d = K.assign(q, model.centers)
    assert np.array_equal(whole, want_l) and _bits(dist) == _bits(want_d)
    restored = kmeans.KMeansModel.from_state(model.state())
    for chunk in (1000, 64, 37):
        assert np.array_equal(restored.predict(q, chunk_rows=chunk), whole)
    assert np.array_equal(model.predict(x), model.labels)


def test_kmeans_starts_metrics_and_n_init():
    from variantformer_amd import kmeans, neighbors
    x = K.blobs(400, 12, 5, 0.5, 3)
    z = neighbors.standardize(x, "correlation")[0].cpu().numpy()
    m = kmeans.kmeans(x, 5, metric="correlation", init="k-means++", seed=4)
    rows, _ = K.seed_rows(z, 5, 4)
    want = K.lloyd(z, z[rows], 300, K.tol_abs_of(z, 1e-4))
    assert np.array_equal(m.labels, want.labels) and _bits(m.centers) == _bits(want.cen) and m.n_iter == want.n_iter and m.metric == "correlation"
    assert np.array_equal(m.predict(x), m.labels)                         # queries are standardised like the fit's rows
    r = kmeans.kmeans(x, 5, metric="euclidean", init="random", seed=4)
    want = K.lloyd(x, x[kmeans.random_rows(400, 5, 4)], 300, K.tol_abs_of(x, 1e-4))
    assert np.array_equal(r.labels, want.labels) and _bits(r.centers) == _bits(want.cen)
    # n_init: the seeds seed, seed + 1, ..; the lowest inertia, ties to the first
    singles = [kmeans.kmeans(x, 5, metric="euclidean", init="random", seed=s) for s in (4, 5, 6)]
    best = kmeans.kmeans(x, 5, metric="euclidean", init="random", seed=4, n_init=3)
    pick = min(range(3), key=lambda i: (singles[i].inertia, i))
    assert best.inertia == singles[pick].inertia and np.array_equal(best.labels, singles[pick].labels)
    # tensors in, tensors out; a cluster that ends empty warns and keeps its centre
    t = kmeans.kmeans(torch.from_numpy(x).cuda(), 5, metric="euclidean", init="random", seed=4)
    assert isinstance(t.labels, torch.Tensor) and t.labels.is_cuda and np.array_equal(t.labels.cpu().numpy(), r.labels)
    far = np.vstack([x[:4], np.full((1, 12), 1e3, np.float32)])
    with pytest.warns(RuntimeWarning, match="ended without rows"):
        e = kmeans.kmeans(x, 5, metric="euclidean", init=far)
    assert e.counts[4] == 0 and _bits(e.centers[4]) == _bits(far[4])


def test_refusals_on_the_device():
    from tests.test_kmeans_cpu import check_refusals
    check_refusals()
    ops = _ops()
    x, cen = _dev(np.zeros((4, 3), np.float32)), _dev(np.zeros((2, 3), np.float32))
    with pytest.raises(AssertionError):
        ops.kmeans_assign(x, cen, labels=_empty(3, torch.int32), dist=_empty(4, torch.float32))
    with pytest.raises(AssertionError):
        ops.kmeans_seed(x, 5, 0, rows=_empty(5, torch.int32), cen=_dev(np.zeros((5, 3), np.float32)), mind=_empty(4, torch.float32),
                        work=_empty(8, torch.int64))
    with pytest.raises(ops._lib.VFError, match="work_bytes"):
        ops.kmeans_lloyd(x, cen, max_iter=1, tol_abs=0.0, labels=_empty(4, torch.int32), dist=_empty(4, torch.float32),
                         prev_labels=_empty(4, torch.int32), counts=_empty(2, torch.int32), n_iter=_empty(1, torch.int32),
                         shift=_empty(1, torch.float64), changed=_empty(1, torch.int64), work=_empty(1, torch.int64))


def test_expression_kmeans_and_its_column_through_expression_enrichment():
    from tests.test_expression_enrichment_gpu import GROUPS, _frame, _proc
    from variantformer_amd import kmeans
    proc = _proc()
    frame, ann, group = _frame()
    out = proc.expression_kmeans(frame, GROUPS, seed=1)
    assert set(out) == {"labels", "centers", "inertia", "n_iter", "model", "row_labels"} and isinstance(out["model"], kmeans.KMeansModel)
    assert frame.columns[-1] == "kmeans_cluster" and frame["kmeans_cluster"].dtype == np.int64
    assert frame["kmeans_cluster"].tolist() == out["labels"].tolist() and out["centers"].shape == (GROUPS, 6)
    # the four planted groups are the four clusters, up to their numbering
    pairs = set(zip(group.tolist(), out["labels"].tolist()))
    assert len(pairs) == GROUPS and len({g for g, _ in pairs}) == len({c for _, c in pairs}) == GROUPS
    enriched = proc.expression_enrichment(frame, ann, labels="kmeans_cluster", n_clusters=GROUPS)
    lut = dict(pairs)
    found = {(c, t) for c, t in zip(enriched["frame"]["cluster"], enriched["frame"]["term"]) if "group" in t}
    assert found == {(lut[g], f"GO:group_{g}") for g in range(GROUPS)}, "every group's own term is significant in its cluster"
    # a second frame gets the first one's clusters; coordinates are clustered with the Euclidean metric
    second = frame.drop(columns=["kmeans_cluster", "enrichment_cluster"]).iloc[::-1].reset_index(drop=True)
    assigned = proc.expression_kmeans_assign(out["model"], second)
    assert second["kmeans_cluster"].tolist() == out["labels"][::-1].tolist() == assigned["labels"].tolist()
    x = np.stack(list(frame["predicted_expression"]))
    frame["umap_1"], frame["umap_2"] = x[:, 0].astype(np.float32), x[:, 1].astype(np.float32)
    on_umap = proc.expression_kmeans(frame, 3, on="umap", init="random", seed=2)
    direct = kmeans.kmeans(np.ascontiguousarray(x[:, :2]), 3, metric="euclidean", init="random", seed=2)
    assert on_umap["model"].metric == "euclidean" and np.array_equal(on_umap["labels"], direct.labels)
    with pytest.raises(ValueError, match="metric"):
        proc.expression_kmeans(frame, 3, on="umap", metric="correlation")
    with pytest.raises(ValueError, match="tsne_1"):
        proc.expression_kmeans(frame, 3, on="tsne")
    with pytest.raises(TypeError, match="KMeansModel"):
        proc.expression_kmeans_assign(object(), frame)

"""vf_graph_components_rounds, vf_csr_components and vf_segment_mean_gather on the GPU (include/vf_hip_components.h) through
their ops wrappers, against the numpy restatements of tests/components_cases.py bit for bit, inside poisoned, guarded buffers;
then manifold.spectral_init_components on the composite graph -- every solved component against the device's own solver on the
sub-graph extracted in numpy, the small ones against their formula --, the two small meta branches, a connected graph, and
umap / VCFProcessor.expression_umap with init=manifold.spectral_init_components on separated clusters."""
import warnings

import numpy as np
import pandas as pd
import pytest
import torch

from tests import components_cases as C
from tests import spectral_cases as S
from tests import umap_cases as U
from tests import write_set_cases as W

pytestmark = pytest.mark.gpu

GUARD = 64
NAN = 0xFF                      # the byte pattern of a NaN in fp32, of -1 in the integers


def _ops():
    from variantformer_amd import _lib, ops
    _lib.load()
    return ops


def _bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _vector(n: int, dtype, values=None):
    big = W.poisoned((n + 2 * GUARD,), dtype, W.DEVICE, NAN)
    view = big[GUARD:GUARD + n]
    if values is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(values)))
    return big, view


def _guards_hold(big: torch.Tensor, n: int) -> bool:
    h = big.cpu().numpy().view(np.uint8)
    size = big.element_size()
    return bool((h[:size * GUARD] == NAN).all() and (h[size * (GUARD + n):] == NAN).all())


def _graph(rowptr, col, w):
    return torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(w).cuda()


# ---- the rounds entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", C.RS)
def test_rounds_equal_their_restatement(R):
    from variantformer_amd import manifold
    ops = _ops()
    for name, graph in C.search_graphs(R).items():
        n = graph[0].shape[0] - 1
        g = _graph(*graph)
        identity = np.arange(n, dtype=np.int32)
        labels, settled_after = C.fixed_point(*graph)
        for rounds in C.ROUNDS + (settled_after + 1, settled_after + 3):
            bp, P = _vector(n, torch.int32, identity)
            bg, gg = _vector(n, torch.int32)
            bm, mm = _vector(n, torch.int32)
            bc, changed = _vector(1, torch.int32)
            assert ops.graph_components_rounds(*g, P, gg, mm, changed, rounds=rounds) is P
            torch.cuda.synchronize()
            want, want_changed = C.rounds(*graph, identity, rounds)
            assert np.array_equal(P.cpu().numpy(), want), f"{name} R={n}: the state after {rounds} rounds"
            assert _guards_hold(bp, n) and _guards_hold(bg, n) and _guards_hold(bm, n) and _guards_hold(bc, 1), f"{name}: a write outside the buffers"
            got_changed = int(changed.cpu()[0])
            if rounds == 0:
                assert got_changed == -1 and (gg.cpu().numpy() == -1).all() and (mm.cpu().numpy() == -1).all(), "no round: nothing is written"
            else:
                assert got_changed == want_changed == int(rounds <= settled_after), f"{name}: changed after {rounds} rounds (settled after {settled_after})"
                assert np.array_equal(mm.cpu().numpy(), want), "m holds the round's result"
            assert (P.cpu().numpy() <= identity).all()
        # the fixed point: scipy's components (of the edges alone), the torch search and the driver
        count, ref = S.components(*C.clean(*graph))
        assert np.array_equal(labels, ref) and np.array_equal(want, labels), f"{name}: the fixed point is the smallest vertex of the component"
        got, k = manifold._components(*g)
        old, k_old = manifold._components_torch(*g)
        assert got.dtype == torch.int32 and k == k_old == count and np.array_equal(got.cpu().numpy(), ref) and np.array_equal(old.cpu().numpy(), ref), name
        assert np.array_equal(g[0].cpu().numpy(), graph[0]) and np.array_equal(g[1].cpu().numpy(), graph[1]), "the graph is only read"


def test_rounds_continue_from_a_state_and_refuse_bad_buffers():
    ops = _ops()
    from variantformer_amd._lib import VFError
    graph = C.random_path(1000)
    g = _graph(*graph)
    n = 1000
    P = torch.arange(n, dtype=torch.int32, device="cuda")
    work = [torch.empty_like(P) for _ in range(2)]
    changed = torch.empty(1, dtype=torch.int32, device="cuda")
    for step in (1, 2, 3):                                                 # 6 rounds in three calls are 6 rounds
        ops.graph_components_rounds(*g, P, *work, changed, rounds=step)
    assert np.array_equal(P.cpu().numpy(), C.rounds(*graph, np.arange(n), 6)[0])
    with pytest.raises(VFError, match="three buffers"):
        ops.graph_components_rounds(*g, P, P, work[0], changed, rounds=1)
    with pytest.raises(AssertionError):
        ops.graph_components_rounds(*g, P[:-1], *work, changed, rounds=1)
    # garbage in the state stays inside the buffers: a parent outside [0, i] is read as i
    bad = np.arange(n, dtype=np.int32)
    bad[[3, 500, 999]] = (7, -4, 2 ** 30)
    bp, Pb = _vector(n, torch.int32, bad)
    ops.graph_components_rounds(*g, Pb, *work, changed, rounds=2)
    torch.cuda.synchronize()
    assert np.array_equal(Pb.cpu().numpy(), C.rounds(*graph, np.arange(n), 2)[0]) and _guards_hold(bp, n)


# ---- the permute entry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("composite", "kernel-spoiled"))
def test_csr_components_equal_their_restatement(name):
    ops = _ops()
    graph = C.composite() if name == "composite" else C.spoiled_kernel_graph()
    R, nnz = graph[0].shape[0] - 1, graph[1].shape[0]
    labels, _ = C.fixed_point(*graph)
    order, rank, comp, starts, rowptr_new = C.permutation(labels, graph[0])
    g = _graph(*graph)
    bc, col_new = _vector(nnz, torch.int32)
    bw, w_new = _vector(nnz, torch.float32)
    dev = [torch.from_numpy(a).cuda() for a in (order, rank, comp, starts, rowptr_new)]
    ops.csr_components(*g, *dev, col_new=col_new, w_new=w_new)
    torch.cuda.synchronize()
    want_col, want_w = C.csr_components(*graph, order, rank, comp, starts, rowptr_new)
    got_col, got_w = col_new.cpu().numpy(), w_new.cpu().numpy()
    assert np.array_equal(got_col, want_col) and _bits(got_w, want_w)
    assert _guards_hold(bc, nnz) and _guards_hold(bw, nnz)
    sizes = np.diff(starts)
    for r in range(R):
        row = got_col[rowptr_new[r]:rowptr_new[r + 1]]
        assert ((row == -1) | ((row >= 0) & (row < sizes[comp[r]]))).all(), "a local column lies in [0, size) or is -1"
        if name == "composite":
            assert (np.diff(row) > 0).all() and (row >= 0).all(), "ascending columns stay ascending"
    assert (got_w[got_col == -1] == 0).all() and not np.signbit(got_w[got_col == -1]).any(), "no edge: column -1 with weight +0"
    if name == "composite":
        assert sorted(sizes.tolist()) == [1, 3, 65, 257, 400]
        for k in range(starts.shape[0] - 1):
            sub = C.extract(*graph, order[starts[k]:starts[k + 1]].astype(np.int64))
            for a, b in zip(C.component_slice(rowptr_new, got_col, got_w, starts, k), sub):
                assert _bits(a, b), "a component's slice is the sub-graph extracted on its own"
    else:
        assert (got_col == -1).sum() >= 3 + 2 * 36, "the spoiled entries are no edges"


# ---- the segment mean ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", C.SEGMENT_DS)
def test_segment_mean_equals_its_restatement(d):
    ops = _ops()
    order, starts = C.segments(C.SEGMENT_LENGTHS, seed=d)
    R, n_seg, ld = order.shape[0], starts.shape[0] - 1, d + 5
    x = np.random.default_rng(d).standard_normal((R, d)).astype(np.float32)
    x[order[starts[2]]] = -0.0                                             # a segment whose first partial starts from a -0
    big = W.poisoned((R + 2 * GUARD, ld), torch.float32, W.DEVICE, NAN)      # NaN in the gap and around
    xd = big[GUARD:GUARD + R, :d]
    xd.copy_(torch.from_numpy(x))
    bo = W.poisoned((n_seg + 2 * GUARD, ld), torch.float32, W.DEVICE, NAN)
    out = bo[GUARD:GUARD + n_seg, :d]
    ops.segment_mean_gather(xd, torch.from_numpy(order).cuda(), torch.from_numpy(starts).cuda(), out=out)
    torch.cuda.synchronize()
    got, want = out.cpu().numpy(), C.segment_mean(x, order, starts)
    assert _bits(got, want), f"d={d}"
    h = bo.cpu().numpy().view(np.uint8).reshape(n_seg + 2 * GUARD, ld, 4)
    assert (h[:GUARD] == NAN).all() and (h[GUARD + n_seg:] == NAN).all() and (h[GUARD:GUARD + n_seg, d:] == NAN).all(), "only out[C, d] is written"
    exact = np.stack([x[order[starts[k]:starts[k + 1]]].astype(np.float64).mean(0) for k in range(n_seg)])
    assert np.abs(got - exact).max() <= 2.0 ** -23 * np.abs(exact).max() + 1e-12, "it is the mean"
    again = torch.empty((n_seg, d), dtype=torch.float32, device="cuda")
    assert _bits(ops.segment_mean_gather(xd, torch.from_numpy(order).cuda(), torch.from_numpy(starts).cuda(), out=again).cpu().numpy(), got)


def test_segment_mean_of_rows_that_start_past_2_31_elements():
    """Three rows 2^30 + 8 elements apart: the third starts past 2^31 elements and 8 GiB.  Only the used elements are written."""
    ops = _ops()
    R, d, ld = 3, 2, 2 ** 30 + 8
    buf = torch.empty(2 * ld + 8, dtype=torch.float32, device="cuda")
    view = buf.as_strided((R, d), (ld, 1))
    assert view[2].data_ptr() - buf.data_ptr() > 2 ** 33
    x = np.random.default_rng(31).standard_normal((R, d)).astype(np.float32)
    view.copy_(torch.from_numpy(x).cuda())
    order, starts = np.array([2, 0, 1], dtype=np.int32), np.array([0, 1, 3], dtype=np.int32)
    out = torch.empty((2, d), dtype=torch.float32, device="cuda")
    ops.segment_mean_gather(view, torch.from_numpy(order).cuda(), torch.from_numpy(starts).cuda(), out=out)
    torch.cuda.synchronize()
    want = C.segment_mean(x, order, starts)
    assert _bits(out.cpu().numpy(), want) and _bits(want[0], x[2])
    del view, buf
    torch.cuda.empty_cache()


# ---- the layout ----------------------------------------------------------------------------------------------------------------------
def _device_solver(seed):
    from variantformer_amd import manifold

    def solve(sub, k):
        g = _graph(*sub)
        deg, dinv = manifold._degrees(*g)
        y, info = manifold._spectral(*g, deg, dinv, k, 16, 40, 1e-4, 50, seed)
        return y.cpu().numpy(), info
    return solve


def _ulp(x) -> float:
    return float(np.spacing(np.float32(x)))


def test_the_layout_of_the_composite_graph():
    """The largest |position - meta| of a solved component is its data_range to within one unit of fp32's precision: with
    e = fl(data_range / max|y|) the farthest coordinate is fl(max|y| e) = data_range (1 + a)(1 + b), |a|, |b| <= 2^-24, so it is
    off by at most 2^-23 data_range, and adding meta rounds once more, by half an ulp of |meta| + data_range.  A small component
    has |2 u - 1| < 1, so it stays within data_range but for that last rounding."""
    from variantformer_amd import manifold
    graph, rows, dim, seed = C.composite(), C.composite_rows(), 2, 42
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = manifold.spectral_init_components(graph, dim, seed, rows=rows)
        want, parts = C.layout(*graph, dim, seed, rows=rows, solver=_device_solver(seed))
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (726, 2)
    y = got.cpu().numpy()
    order, starts, meta, spread = parts["order"], parts["starts"], parts["meta"].astype(np.float32), parts["data_range"]
    assert starts.shape[0] - 1 == 5 and parts["solved"].sum() == 3
    for k in range(5):
        members = order[starts[k]:starts[k + 1]]
        far = np.abs(y[members].astype(np.float64) - meta[k].astype(np.float64)).max()
        if parts["solved"][k]:
            assert _bits(y[members], want[members]), f"component {k}: fl(fl(y expansion) + meta) of the device's solver on the extracted sub-graph"
            assert abs(far - spread[k]) <= 2.0 ** -23 * spread[k] + _ulp(np.abs(meta[k]).max() + spread[k]) / 2, f"component {k} reaches its data_range"
            info = parts["infos"][k]
            sub = C.extract(*graph, members.astype(np.int64))
            truth = S.dense_truth(*sub)
            vectors = _device_solver(seed)(sub, dim)[0]
            eig, vec, dev_sub = S.deviations(vectors, info["eigenvalues"], truth)
            print(f"[components layout] component {k} of {members.shape[0]} vertices: {info['iterations']} outer iterations, eigenvalues {eig:.2e}, "
                  f"vectors {vec:.2e}, subspaces {dev_sub:.2e}")
            assert info["converged"] and eig <= S.GPU_EIG_ATOL and vec <= S.GPU_VEC_ATOL and dev_sub <= S.GPU_SUB_ATOL
        else:
            assert _bits(y[members], C.small(U.random_init(726, dim, seed)[members], spread[k], parts["meta"][k])), f"small component {k}"
            assert far <= spread[k] + _ulp(np.abs(meta[k]).max() + spread[k]) / 2
    assert _bits(y, want)
    again = manifold.spectral_init_components(_graph(*graph), dim, seed, rows=torch.from_numpy(rows).cuda(), metric="correlation")
    assert _bits(again.cpu().numpy(), y), "two runs are equal bit for bit, tensors or arrays in"
    with pytest.raises(ValueError, match="rows"):
        manifold.spectral_init_components(graph, dim, seed)
    assert not _bits(manifold.spectral_init_components(graph, dim, seed, rows=rows, metric="cosine").cpu().numpy(), y), "the metric standardises the centroids"


def test_the_small_meta_branches_and_a_connected_graph():
    from variantformer_amd import manifold
    with warnings.catch_warnings():
        # a blob is a complete graph: its second and third eigenvalues lie among 38 nearly equal ones (tests/spectral_cases.py),
        # so the solver may stop at max_iter with its warning; the placement is what is asserted
        warnings.simplefilter("ignore", RuntimeWarning)
        two = manifold.spectral_init_components(S.blobs(False), 2, 42).cpu().numpy()
        want, parts = C.layout(*S.blobs(False), 2, 42, solver=_device_solver(42))
    assert np.array_equal(parts["meta"], [[1, 0], [-1, 0]]) and (parts["data_range"] == 1).all() and _bits(two, want)
    assert (two[:40, 0] >= 0).all() and (two[40:, 0] <= 0).all() and np.abs(two - np.repeat(parts["meta"], 40, 0)).max() <= 1, \
        "C = 2: the components sit around +e1 and -e1, within data_range = 1"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        four = manifold.spectral_init_components(C.composite(True), 2, 7).cpu().numpy()          # C = 4 = 2 dim: no rows needed
        want, parts = C.layout(*C.composite(True), 2, 7, solver=_device_solver(7))
        assert np.array_equal(parts["meta"], [[1, 0], [0, 1], [-1, 0], [0, -1]]) and _bits(four, want)
        strip = manifold.spectral_init_components(S.strip(), 2, 42)
        assert _bits(strip.cpu().numpy(), manifold.spectral_init(S.strip(), 2, 42).cpu().numpy()), "a connected graph: spectral_init, bit for bit"
    with pytest.warns(RuntimeWarning, match="2 vertices"):
        y = manifold.spectral_init_components(S.path(2), 2, 42)
    assert np.array_equal(y.cpu().numpy(), U.random_init(2, 2, 42))
    many = S.from_edges(2 * C.COMPONENTS_MAX + 2, np.arange(0, 2 * C.COMPONENTS_MAX + 2, 2), np.arange(1, 2 * C.COMPONENTS_MAX + 2, 2),
                        np.ones(C.COMPONENTS_MAX + 1))
    with pytest.warns(RuntimeWarning, match=f"{C.COMPONENTS_MAX + 1} components"):
        y = manifold.spectral_init_components(many, 2, 3, rows=np.zeros((2 * C.COMPONENTS_MAX + 2, 3), dtype=np.float32))
    assert np.array_equal(y.cpu().numpy(), U.random_init(2 * C.COMPONENTS_MAX + 2, 2, 3)), "past the cap: the random fallback"


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_clusters,n", ((3, 40), (7, 24)))
def test_umap_from_the_per_component_start(n_clusters, n):
    from variantformer_amd import manifold, neighbors
    x = C.clusters(n_clusters, n)
    R = x.shape[0]
    kw = dict(n_neighbors=11, n_epochs=50)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        y = manifold.umap(x, init=manifold.spectral_init_components, **kw)
    assert y.shape == (R, 2) and y.dtype == np.float32 and np.isfinite(y).all()
    assert np.array_equal(manifold.umap(x, init=manifold.spectral_init_components, **kw), y), "two runs are equal bit for bit"
    idx, dist = neighbors.knn(x, k=10)
    graph = manifold.fuzzy_graph(idx, dist)
    assert manifold.graph_components(graph)[1] == n_clusters
    start = manifold.rescale(manifold.spectral_init_components(graph, 2, 42, rows=x, metric="correlation"))
    a, b = manifold.find_ab(0.1)
    assert np.array_equal(manifold.layout(graph, start.cpu().numpy(), 50, a, b, seed=42), y), "the stages composed by hand"
    with pytest.warns(RuntimeWarning, match=f"{n_clusters} components"):
        fallback = manifold.umap(x, init=manifold.spectral_init, **kw)
    assert not np.array_equal(fallback, y)
    seen = []

    def plain(*args, **kwargs):
        seen.append((len(args), sorted(kwargs)))
        return U.random_init(R, args[1], args[2])
    manifold.umap(x, init=plain, **kw)
    assert seen == [(3, [])], "a callable without wants_rows sees exactly the three arguments"

    def asking(graph, n_components, seed, rows=None, metric=None):
        seen.append((tuple(rows.shape), rows.is_cuda, metric))
        return U.random_init(R, n_components, seed)
    asking.wants_rows = True
    manifold.umap(x, init=asking, metric="cosine", **kw)
    assert seen[-1] == ((R, 10), True, "cosine"), "a callable that asks gets the rows on the device and the metric"


def test_expression_umap_from_the_per_component_start():
    from variantformer_amd import manifold, neighbors
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    x = C.clusters(3, 40)
    genes, tissues = x.shape
    names = [f"tissue{t:02d}" for t in range(tissues)]
    df = pd.DataFrame({"gene_id": [f"ENSG{i:05d}" for i in range(genes)], "tissues": [list(range(tissues))] * genes,
                       "tissue_names": [names] * genes, "predicted_expression": [e.reshape(tissues, 1) for e in x]})
    kw = dict(n_neighbors=11, n_epochs=30, init=manifold.spectral_init_components)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        out = VCFProcessor().expression_umap(df, **kw)
        m, _ = neighbors.from_predictions(df)
        assert np.array_equal(out["coords"], manifold.umap(m, **kw)), "the frame's matrix through manifold.umap"
    assert out["coords"].shape == (genes, 2) and out["coords"].dtype == np.float32 and np.isfinite(out["coords"]).all()
    assert np.array_equal(np.stack((df["umap_1"], df["umap_2"]), 1), out["coords"]) and out["labels"] == list(df["gene_id"])

"""References and the case table of the component entries (include/vf_hip_components.h) and of the per-component spectral start
(manifold.spectral_init_components).

The references are numpy restatements with the header's operation order.  `one_round` is a round of vf_graph_components_rounds
as the header writes it -- integers only, the hook an integer minimum whose result does not depend on order -- so the device's
state is compared with array_equal after every number of rounds.  `csr_components` is vf_csr_components (copies and one integer
subtraction).  `segment_mean` is vf_segment_mean_gather: four interleaved fp64 partials, each summed in ascending order from +0,
added as ((p0 + p1) + p2) + p3, one fp64 division, rounded once to fp32; bit for bit.  `extract` takes a component's sub-graph
out of a graph on its own, in numpy, and `layout` is spectral_init_components over these restatements with the eigensolver
handed in (tests/spectral_cases.spectral_reference on the host, the device's own on the GPU): the meta positions restated here
from the docstring's formulas, not imported.

Bounds.  Everything about the entries is bit equality.  The meta positions of more than 2 dim components are compared with
scikit-learn's SpectralEmbedding(affinity="precomputed") per column after both are normalised and signed alike: two fp64
eigensolvers of one symmetric C x C matrix of norm <= 2 differ in an eigenvector by about u ||L|| / gap (u = 2^-53, gap the
distance to the nearest other eigenvalue), and the division by the degrees' roots and the normalisation add a few u more; the
bound asserted is META_FACTOR u / gap with META_FACTOR = 64 C for the C-term sums, gap measured on the matrix.  The solved
components of the layout are held to the GPU_*_ATOL of tests/spectral_cases.py: the same solver, the same bounds.
"""
from __future__ import annotations

import numpy as np

from tests import spectral_cases as S
from tests import umap_cases as U

F32, F64, I32, I64 = np.float32, np.float64, np.int32, np.int64

ROUNDS = (0, 1, 2, 3, 8)
RS = (1, 2, 63, 64, 65, 257, 1000)
SEGMENT_DS = (1, 49, 64, 65)
SEGMENT_LENGTHS = (1, 3, 4, 5, 255, 256, 257)
COMPONENTS_MAX = 2048
META_FACTOR = 64


# ---- the component search -----------------------------------------------------------------------------------------------------------
def edges(rowptr, col, w):
    """(rows, cols) int64 of the entries that are edges: w > 0 and 0 <= col < R."""
    R = rowptr.shape[0] - 1
    c = col.astype(I64)
    with np.errstate(invalid="ignore"):
        ok = (np.asarray(w, dtype=F32) > 0) & (c >= 0) & (c < R)
    return U.entry_rows(rowptr)[ok], c[ok]


def one_round(P: np.ndarray, r: np.ndarray, c: np.ndarray):
    """(the next state, changed) as the header states a round."""
    g = P[P]
    m = g.copy()
    np.minimum.at(m, r, g[c])
    Pn = np.minimum(g, m)
    np.minimum.at(Pn, P, m)
    return Pn, int((Pn != P).any())


def rounds(rowptr, col, w, P: np.ndarray, n: int):
    """(state int32, changed of the last round or None without one) after n rounds from P."""
    r, c = edges(rowptr, col, w)
    P, changed = np.array(P, dtype=I64), None
    for _ in range(n):
        P, changed = one_round(P, r, c)
    return P.astype(I32), changed


def fixed_point(rowptr, col, w):
    """(labels int32, the rounds that changed something)."""
    r, c = edges(rowptr, col, w)
    P, n = np.arange(rowptr.shape[0] - 1, dtype=I64), 0
    while True:
        P, changed = one_round(P, r, c)
        if not changed:
            return P.astype(I32), n
        n += 1


# ---- the renumbered graph -----------------------------------------------------------------------------------------------------------
def permutation(labels: np.ndarray, rowptr: np.ndarray):
    """(order, rank, comp, starts int32; rowptr_new int64) as manifold.spectral_init_components hands them to vf_csr_components."""
    R = labels.shape[0]
    order = np.argsort(labels, kind="stable")
    rank = np.empty(R, dtype=I64)
    rank[order] = np.arange(R)
    sorted_labels = labels[order]
    first = np.ones(R, dtype=bool)
    first[1:] = sorted_labels[1:] != sorted_labels[:-1]
    comp = np.cumsum(first) - 1
    starts = np.append(np.nonzero(first)[0], R)
    rowptr_new = np.zeros(R + 1, dtype=I64)
    rowptr_new[1:] = np.cumsum(np.diff(rowptr)[order])
    return order.astype(I32), rank.astype(I32), comp.astype(I32), starts.astype(I32), rowptr_new


def csr_components(rowptr, col, w, order, rank, comp, starts, rowptr_new):
    """(col_new int32, w_new fp32) as vf_csr_components writes them (valid arrays)."""
    R, nnz = rowptr.shape[0] - 1, col.shape[0]
    col_new, w_new = np.full(nnz, -1, dtype=I32), np.zeros(nnz, dtype=F32)
    w = np.asarray(w, dtype=F32)
    for r in range(R):
        i, lo, hi = int(order[r]), int(starts[comp[r]]), int(starts[comp[r] + 1])
        for t in range(int(rowptr_new[r + 1] - rowptr_new[r])):
            e = int(rowptr[i]) + t
            j = int(col[e])
            if w[e] > 0 and 0 <= j < R and lo <= rank[j] < hi:
                col_new[rowptr_new[r] + t], w_new[rowptr_new[r] + t] = rank[j] - lo, w[e]
    return col_new, w_new


def extract(rowptr, col, w, members: np.ndarray):
    """The sub-graph of the vertices `members` (ascending) on its own: (rowptr int64 from 0, col int32 local, w fp32), a row's
    entries in their order; an entry that is no edge of the sub-graph stays as column -1 with weight +0."""
    R = rowptr.shape[0] - 1
    local = np.full(R, -1, dtype=I64)
    local[members] = np.arange(members.shape[0])
    w = np.asarray(w, dtype=F32)
    rp, cols, ws = [0], [], []
    for i in members:
        for e in range(int(rowptr[i]), int(rowptr[i + 1])):
            j = int(col[e])
            edge = w[e] > 0 and 0 <= j < R and local[j] >= 0
            cols.append(local[j] if edge else -1)
            ws.append(w[e] if edge else F32(0))
        rp.append(len(cols))
    return np.array(rp, dtype=I64), np.array(cols, dtype=I32), np.array(ws, dtype=F32)


def component_slice(rowptr_new, col_new, w_new, starts, k: int):
    """Component k's slice of the renumbered graph with its rowptr rebased to 0."""
    s, e = int(starts[k]), int(starts[k + 1])
    a, b = int(rowptr_new[s]), int(rowptr_new[e])
    return rowptr_new[s:e + 1] - a, col_new[a:b], w_new[a:b]


# ---- the centroids ------------------------------------------------------------------------------------------------------------------
def segment_mean(x: np.ndarray, order: np.ndarray, starts: np.ndarray) -> np.ndarray:
    """fp32 [C, d] as vf_segment_mean_gather forms it."""
    C, d = starts.shape[0] - 1, x.shape[1]
    out = np.zeros((C, d), dtype=F32)
    with np.errstate(all="ignore"):
        for k in range(C):
            s, e = int(starts[k]), int(starts[k + 1])
            part = []
            for v in range(4):
                rows = x[order[s + v:e:4]].astype(F64)
                part.append(np.cumsum(np.concatenate((np.zeros((1, d)), rows)), axis=0)[-1])      # ascending, from +0
            total = ((part[0] + part[1]) + part[2]) + part[3]
            out[k] = (total / F64(e - s)).astype(F32)
    return out


def segments(lengths, seed: int = 0):
    """(order int32 a permutation of the rows, starts int32) for segments of the given lengths."""
    R = int(sum(lengths))
    return np.random.default_rng(seed).permutation(R).astype(I32), np.concatenate(([0], np.cumsum(lengths))).astype(I32)


# ---- the layout, restated -----------------------------------------------------------------------------------------------------------
def standardise(z: np.ndarray, metric: str) -> np.ndarray:
    z = np.array(z, dtype=F64)
    if metric == "correlation":
        z = z - z.mean(1, keepdims=True)
    norm = np.sqrt((z * z).sum(1, keepdims=True))
    return np.where(norm > 0, z / np.where(norm > 0, norm, 1.0), 0.0)


def meta_laplacian(centroids: np.ndarray, metric: str):
    """(L fp64 [C, C], the inverse roots of the affinity's degrees) of the components' centroids."""
    z = standardise(centroids, metric)
    D = 1.0 - z @ z.T
    np.fill_diagonal(D, 0.0)
    A = np.exp(-D * D)
    np.fill_diagonal(A, 0.0)
    dinv = 1.0 / np.sqrt(A.sum(1))
    L = np.eye(A.shape[0]) - A * np.outer(dinv, dinv)
    return (L + L.T) / 2.0, dinv, A


def meta_positions(count: int, dim: int, centroids=None, metric: str = "correlation") -> np.ndarray:
    if count <= 2 * dim:
        k = -(-count // 2)
        base = np.eye(k, dim)
        return np.concatenate((base, -base))[:count]
    L, dinv, _ = meta_laplacian(centroids, metric)
    _, vec = np.linalg.eigh(L)
    y = vec[:, 1:dim + 1] * dinv[:, None]
    big = np.abs(y).argmax(0)
    y = y * np.where(y[big, np.arange(dim)] < 0, -1.0, 1.0)[None, :]
    return y / np.abs(y).max()


def data_ranges(meta: np.ndarray) -> np.ndarray:
    d = np.sqrt(((meta[:, None, :] - meta[None, :, :]) ** 2).sum(-1))
    return np.where(d > 0, d, np.inf).min(1) / 2.0


def place(y: np.ndarray, data_range, meta_row: np.ndarray) -> np.ndarray:
    """fl(fl(y * expansion) + meta) in fp32 with expansion = fl(data_range / max|y|)."""
    expansion = F32(data_range) / np.abs(y).max()
    return ((y * expansion).astype(F32) + meta_row.astype(F32)[None, :]).astype(F32)


def small(u: np.ndarray, data_range, meta_row: np.ndarray) -> np.ndarray:
    """fl(fl((2 u - 1) * data_range) + meta) in fp32 (2 u - 1 is exact)."""
    t = (F32(2) * u - F32(1)).astype(F32)
    return ((t * F32(data_range)).astype(F32) + meta_row.astype(F32)[None, :]).astype(F32)


def layout(rowptr, col, w, dim: int, seed: int, rows=None, metric: str = "correlation", solver=None):
    """(positions fp32 [R, dim], parts) as manifold.spectral_init_components places a DISCONNECTED graph.  solver(sub-graph, k)
    -> (vectors fp32, info); default tests/spectral_cases.spectral_reference.  parts: labels, order, starts, meta, data_range
    (fp32), solved (bool per component), infos (per solved component)."""
    R = rowptr.shape[0] - 1
    solver = solver or (lambda g, k: S.spectral_reference(*g, k=k, seed=seed))
    labels, _ = fixed_point(rowptr, col, w)
    order, rank, comp, starts, rowptr_new = permutation(labels, rowptr)
    count = starts.shape[0] - 1
    centroids = segment_mean(np.asarray(rows, dtype=F32), order, starts) if count > 2 * dim else None
    meta = meta_positions(count, dim, centroids, metric)
    spread = data_ranges(meta).astype(F32)
    u = U.random_init(R, dim, seed)
    out = np.zeros((R, dim), dtype=F32)
    solved, infos = np.diff(starts) >= max(2 * dim, dim + 2), {}
    for k in range(count):
        members = order[starts[k]:starts[k + 1]].astype(I64)
        if solved[k]:
            y, infos[k] = solver(extract(rowptr, col, w, members), dim)
            out[members] = place(y, spread[k], meta[k])
        else:
            out[members] = small(u[members], spread[k], meta[k])
    return out, dict(labels=labels, order=order, starts=starts, meta=meta, data_range=spread, solved=solved, infos=infos)


# ---- the graphs ---------------------------------------------------------------------------------------------------------------------
def from_entries(R: int, rows, cols, wt):
    """The CSR graph of the directed entries (row, col, w), columns ascending within a row."""
    rows, cols = np.asarray(rows, dtype=I64), np.asarray(cols, dtype=I64)
    o = np.lexsort((cols, rows))
    rowptr = np.zeros(R + 1, dtype=I64)
    rowptr[1:] = np.cumsum(np.bincount(rows, minlength=R))
    return rowptr, cols[o].astype(I32), np.asarray(wt, dtype=F32)[o]


def random_path(R: int, seed: int = 9):
    """A path through the vertices in a random order."""
    g = np.random.default_rng(seed + R)
    p = g.permutation(R)
    return S.from_edges(R, p[:-1], p[1:], g.uniform(0.2, 1.0, max(R - 1, 0)))


def long_row(R: int = 257, n: int = 200):
    """A star: row 0 has n entries."""
    return S.from_edges(R, np.zeros(n, dtype=I64), np.arange(1, n + 1), np.ones(n))


def spoiled_kernel_graph(R: int = 257):
    """The pairs of S.kernel_graph(R) as a graph of symmetric structure, with 12 pairs each of weight 0, -1 and NaN (in both
    directions) and three more entries that name the columns -1, R and R + 5: an entry is an edge only with a positive weight
    and a column inside [0, R)."""
    rowptr, col, w = S.kernel_graph(R)
    rows, c = U.entry_rows(rowptr), col.astype(I64)
    inside = (c >= 0) & (c < R) & (c != rows)
    lo, hi = np.minimum(rows[inside], c[inside]), np.maximum(rows[inside], c[inside])
    pairs, at = np.unique(lo * R + hi, return_index=True)
    i, j, wt = pairs // R, pairs % R, w[inside][at].copy()
    g = np.random.default_rng(77)
    for n, value in enumerate((0.0, -1.0, np.nan)):
        wt[g.choice(wt.shape[0], 36, replace=False)[12 * n:12 * n + 12]] = value
    junk_rows, junk_cols = g.integers(0, R, 3), np.array([-1, R, R + 5])
    return from_entries(R, np.concatenate((i, j, junk_rows)), np.concatenate((j, i, junk_cols)), np.concatenate((wt, wt, np.ones(3))))


def clean(rowptr, col, w):
    """The graph with its edges alone (for scipy, which takes every stored entry)."""
    r, c = edges(rowptr, col, w)
    return from_entries(rowptr.shape[0] - 1, r, c, np.ones(r.shape[0]))


def search_graphs(R: int):
    """name -> graph, the graphs of the search at size R (the fixed ones where R is theirs)."""
    out = {"path": S.path(R), "random-path": random_path(R), "random-path-b": random_path(R, seed=10)}
    if R == 64:
        out["ring"] = S.ring()
    if R == 65:
        out["isolated"] = S.isolated()
    if R == 257:
        out.update({"blobs-apart": S.blobs(False), "strip": S.strip(), "kernel-spoiled": spoiled_kernel_graph(), "long-row": long_row()})
    return out


COMPOSITE_PARTS = ("path65", "strip400", "path257", "path3", "single")
_COMPOSITE = {}


def composite(drop_strip: bool = False):
    """The disjoint union of path(65), strip(), path(257), a 3-vertex path and a vertex without an entry, its vertices renumbered
    by a fixed random permutation: 726 vertices and 5 components (326 and 4 without the strip).  Computed once."""
    if drop_strip not in _COMPOSITE:
        parts = [S.path(65)] + ([] if drop_strip else [S.strip()]) + [S.path(257), S.path(3, seed=4), (np.zeros(2, dtype=I64), np.zeros(0, dtype=I32), np.zeros(0, dtype=F32))]
        R = sum(p[0].shape[0] - 1 for p in parts)
        perm = np.random.default_rng(20 + drop_strip).permutation(R)
        rows, cols, ws, at = [], [], [], 0
        for rowptr, col, w in parts:
            rows.append(perm[U.entry_rows(rowptr) + at])
            cols.append(perm[col.astype(I64) + at])
            ws.append(w)
            at += rowptr.shape[0] - 1
        _COMPOSITE[drop_strip] = from_entries(R, np.concatenate(rows), np.concatenate(cols), np.concatenate(ws))
    return _COMPOSITE[drop_strip]


def composite_rows(R: int = 726, d: int = 7) -> np.ndarray:
    """fp32 [R, d]: data rows for the composite's centroids (any rows do: the meta positions need C distinct centroids)."""
    return np.random.default_rng(21).standard_normal((R, d)).astype(F32)


def clusters(n_clusters: int, n: int, d: int = 10) -> np.ndarray:
    """fp32 [n_clusters n, d]: well-separated clusters, np.repeat(base, n, 0) + 0.05 noise, generator seed 11."""
    g = np.random.default_rng(11)
    base = g.standard_normal((n_clusters, d))
    return (np.repeat(base, n, 0) + 0.05 * g.standard_normal((n_clusters * n, d))).astype(F32)

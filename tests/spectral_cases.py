"""References and the case table of the spectral embedding (include/vf_hip_spectral.h, variantformer_amd/manifold.py).

The references are numpy restatements with the header's operation order: `degree` is vf_graph_degree and `spmm_recur` is
vf_spmm_recur, in fp32 with every operation rounded once and the header's lane / group order, so the device's results are
compared with array_equal; `tall_gram` is vf_tall_gram (fp64, per-chunk partials, then the partials in order) and `tall_mul` is
vf_tall_mul (fp64 sum over k ascending, rounded once to fp32).  `spectral_reference` is manifold._spectral over those
restatements: the same start (the counter-based hash), the locked trivial vector, the orthonormalisation through the
column-scaled Gram matrix twice, Rayleigh-Ritz, the Chebyshev coefficients (restated here from the formulas of
manifold.chebyshev_coefficients' docstring, not imported).  `dense_truth` is numpy.linalg.eigh of the fp64 normalised Laplacian.

A computed vector y_j is compared with the truth through dev = 1 - ||P y_j||_2, where P projects on the true eigenvectors of the
CLUSTER of j: the consecutive eigenvalues around the j-th whose neighbouring gaps are at most GAP = 1e-3 (the trivial one
included).  For a vector alone in its cluster that is 1 - |cos| (VEC); otherwise it is the distance from the invariant
subspace (SUB): inside a cluster of nearly equal eigenvalues the single vectors are not determined to fp32's precision.
Eigenvalues are compared absolutely (EIG).  Measured once, asserted at 8 times the measurement:

  the numpy restatement on the host (python -m pytest tests/test_spectral_cpu.py -s prints every figure), over the connected
  graphs of the table at degree 20 and 40:       EIG 1.79e-7  VEC 5.8e-9   SUB 1.77e-6, at most 4 outer iterations (SUB is
      path257's at degree 20, which stops with a residual of 3.3e-5: the figure is the stopping rule's, not the arithmetic's;
      at degree 40 it is 1.5e-8);
  an MI355X (python -m pytest tests/test_spectral_gpu.py -s), degree 40:   EIG 1.79e-7  VEC 5.8e-9   SUB 1.5e-8.
"""
from __future__ import annotations

import numpy as np

from tests import umap_cases as U

F32, F64 = np.float32, np.float64

GAP = 1e-3
EIG_MEASURED, VEC_MEASURED, SUB_MEASURED = 1.79e-7, 5.8e-9, 1.77e-6          # the numpy restatement, on the host
GPU_EIG_MEASURED, GPU_VEC_MEASURED, GPU_SUB_MEASURED = 1.79e-7, 5.8e-9, 1.5e-8  # an MI355X
EIG_ATOL, VEC_ATOL, SUB_ATOL = 8 * EIG_MEASURED, 8 * VEC_MEASURED, 8 * SUB_MEASURED
GPU_EIG_ATOL, GPU_VEC_ATOL, GPU_SUB_ATOL = 8 * GPU_EIG_MEASURED, 8 * GPU_VEC_MEASURED, 8 * GPU_SUB_MEASURED
ITERATIONS_CAP = 10                         # a table graph that needs more outer iterations is replaced, not the cap

KERNEL_RS = (1, 2, 63, 64, 65, 257)
KERNEL_PS = (1, 3, 16, 17, 32)
KERNEL_STEPS = (0, 1, 2, 3, 4, 7)
ROW_LENGTHS = (0, 1, 63, 64, 65, 200)
MAX_P, TILE, MAX_BLOCKS = 32, 64, 1024
FILTER_LOW, FILTER_HIGH, ORTH_FLOOR = -0.99, 1.0 - 1e-7, 1e-14


# ---- the three entries (and the fourth), restated -----------------------------------------------------------------------------------
def _butterfly(v: np.ndarray, axis_len: int) -> np.ndarray:
    """v[..., g, ...] = v[g] + v[g ^ off] for off = axis_len / 2 .. 1 along axis 1, in v's type."""
    lanes = np.arange(axis_len)
    off = axis_len // 2
    while off >= 1:
        v = v + v[:, lanes ^ off]
        off //= 2
    return v


def _plan(rowptr: np.ndarray, nnz: int, G: int):
    """(entry index [R, steps, G], valid [R, steps, G]): group g of row i takes rowptr[i] + g, + G, ...; entries outside [0, nnz) are skipped."""
    begin, end = np.clip(rowptr[:-1], 0, None), np.clip(rowptr[1:], None, nnz)
    lens = np.maximum(end - begin, 0)
    steps = max(1, int(-(-int(lens.max(initial=0)) // G)))
    t = np.arange(steps * G, dtype=np.int64).reshape(steps, G)
    E = begin[:, None, None] + t[None]
    return np.where(t[None] < lens[:, None, None], E, 0), t[None] < lens[:, None, None]


def degree(rowptr: np.ndarray, w: np.ndarray):
    """(deg fp32 [R], dinv_sqrt fp32 [R]) as vf_graph_degree forms them."""
    w = np.asarray(w, dtype=F32)
    E, valid = _plan(rowptr, w.shape[0], 64)
    v = np.zeros((rowptr.shape[0] - 1, 64), dtype=F32)
    for s in range(E.shape[1]):
        v = v + np.where(valid[:, s], w[E[:, s]] if w.size else F32(0), F32(0))
    deg = _butterfly(v, 64)[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        dinv = np.where(deg > 0, F32(1) / np.sqrt(deg, dtype=F32), F32(0)).astype(F32)
    return deg, dinv


def product(rowptr, col, w, dinv, Y: np.ndarray, p: int) -> np.ndarray:
    """(S Y)[:, :p] fp32 as vf_spmm_recur forms it."""
    R, nnz = rowptr.shape[0] - 1, col.shape[0]
    C = 1
    while C < p:
        C *= 2
    G = 64 // C
    E, valid = _plan(rowptr, nnz, G)
    acc = np.zeros((R, G, p), dtype=F32)
    if nnz:
        j = col.astype(np.int64)
        inside = (j >= 0) & (j < R)
        j = np.where(inside, j, 0)
        with np.errstate(all="ignore"):
            scale = (np.asarray(w, dtype=F32) * dinv[j]).astype(F32)
            for s in range(E.shape[1]):
                e = E[:, s]
                term = (scale[e][:, :, None] * Y[j[e]][:, :, :p]).astype(F32)
                acc = acc + np.where((valid[:, s] & inside[e])[:, :, None], term, F32(0))
    with np.errstate(all="ignore"):
        return (dinv[:, None] * _butterfly(acc, G)[:, 0]).astype(F32)


def spmm_recur(rowptr, col, w, dinv, X0, X1, X2, p: int, coef: np.ndarray):
    """The three buffers after coef.shape[0] steps (copies; columns at or past p untouched); the result is [steps % 3]."""
    X = [np.array(X0, dtype=F32), np.array(X1, dtype=F32), np.array(X2, dtype=F32)]
    for t, (c0, c1, c2) in enumerate(np.asarray(coef, dtype=F32)):
        Y, W = X[t % 3], X[(t + 2) % 3]
        z, have = np.zeros((Y.shape[0], p), dtype=F32), False
        with np.errstate(all="ignore"):
            if c0 != 0:
                z, have = (c0 * product(rowptr, col, w, dinv, Y, p)).astype(F32), True
            if c1 != 0:
                term = (c1 * Y[:, :p]).astype(F32)
                z, have = ((z + term).astype(F32) if have else term), True
            if c2 != 0:
                term = (c2 * W[:, :p]).astype(F32)
                z = (z + term).astype(F32) if have else term
        X[(t + 1) % 3][:, :p] = z
    return X


def gram_blocks(R: int):
    """(chunk, nb) of vf_tall_gram."""
    if R == 0:
        return 0, 0
    chunk = TILE * (-(-R // (TILE * MAX_BLOCKS)))
    return chunk, -(-R // chunk)


def tall_gram(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    """A^T B fp64 in vf_tall_gram's order: rows ascending within a chunk, then the chunks ascending."""
    R = A.shape[0]
    chunk, nb = gram_blocks(R)
    G = np.zeros((A.shape[1], B.shape[1]), dtype=F64)
    with np.errstate(all="ignore"):
        for k in range(nb):
            a, b = A[k * chunk:(k + 1) * chunk].astype(F64), B[k * chunk:(k + 1) * chunk].astype(F64)
            G = G + np.cumsum(a[:, :, None] * b[:, None, :], axis=0)[-1]        # cumsum adds in order
    return G


def tall_mul(X: np.ndarray, T: np.ndarray) -> np.ndarray:
    """X T as vf_tall_mul forms it: fp64, k ascending, rounded once to fp32."""
    s = np.zeros((X.shape[0], T.shape[1]), dtype=F64)
    with np.errstate(all="ignore"):
        for k in range(T.shape[0]):
            s = s + X[:, k].astype(F64)[:, None] * T[k][None, :]
        return s.astype(F32)


# ---- the solver, restated -----------------------------------------------------------------------------------------------------------
def chebyshev(bound: float, degree_: int) -> np.ndarray:
    c, e = (bound - 1.0) / 2.0, (bound + 1.0) / 2.0
    sigma1 = e / (1.0 - c)
    sigma, out = sigma1, [(sigma1 / e, -c * sigma1 / e, 0.0)]
    for _ in range(1, degree_):
        nxt = 1.0 / (2.0 / sigma1 - sigma)
        out.append((2.0 * nxt / e, -2.0 * nxt * c / e, -sigma * nxt))
        sigma = nxt
    return np.array(out, dtype=F64).astype(F32)


def orth_matrix(G: np.ndarray) -> np.ndarray:
    p = G.shape[0]
    T = np.zeros((p, p))
    T[0, 0] = 1.0
    if p == 1:
        return T
    c = G[0, 1:] / G[0, 0]
    Gp = G[1:, 1:] - G[0, 0] * np.outer(c, c)
    Gp = (Gp + Gp.T) / 2.0
    d = np.sqrt(np.where(np.diag(Gp) > 0, np.diag(Gp), 1.0))
    lam, V = np.linalg.eigh(Gp / np.outer(d, d))
    lam = np.maximum(lam, ORTH_FLOOR * max(lam.max(), np.finfo(F64).tiny))
    M = (V / np.sqrt(lam)[None, :]) / d[:, None]
    T[0, 1:], T[1:, 1:] = -c @ M, M
    return T


ONE_STEP = np.array([[1.0, 0.0, 0.0]], dtype=F32)


def spectral_reference(rowptr, col, w, k: int = 2, block: int = 16, degree_: int = 40, tol: float = 1e-4, max_iter: int = 50, seed: int = 42):
    """(vectors fp32 [R, k], info) as manifold.spectral_embedding(..., return_info=True) computes them, on a connected graph."""
    R = rowptr.shape[0] - 1
    p = min(block, R)
    deg, dinv = degree(rowptr, w)
    products = 0

    def recur(x, coef):
        nonlocal products
        products += coef.shape[0]
        return spmm_recur(rowptr, col, w, dinv, x, np.zeros_like(x), np.zeros_like(x), p, coef)[coef.shape[0] % 3]

    def orthonormalise(x):
        for _ in range(2):
            x = tall_mul(x, orth_matrix(tall_gram(x, x)))
        return x

    def rayleigh_ritz(x):
        H = tall_gram(x, recur(x, ONE_STEP))
        H = (H + H.T) / 2.0
        lam, Q = np.linalg.eigh(H[1:, 1:]) if p > 1 else (np.zeros(0), np.zeros((0, 0)))
        T = np.zeros((p, p))
        T[0, 0] = 1.0
        T[1:, 1:] = Q[:, ::-1]
        theta = np.concatenate(([H[0, 0]], lam[::-1]))
        x = tall_mul(x, T)
        sx = recur(x, ONE_STEP)
        r = (sx[:, :k + 1] - (x[:, :k + 1] * theta[:k + 1].astype(F32)[None, :]).astype(F32)).astype(F32)
        return x, theta, np.sqrt(np.diag(tall_gram(r, r)))

    x = (U.random_init(R, p, seed) - F32(0.5)).astype(F32)
    v0 = np.sqrt(deg, dtype=F32)
    v0 = (v0 * F32(1.0 / np.sqrt(tall_gram(v0[:, None], v0[:, None])[0, 0]))).astype(F32)
    x[:, 0] = v0
    x, theta, res = rayleigh_ritz(orthonormalise(x))
    iterations = 0
    while res[1:k + 1].max() >= tol and iterations < max_iter:
        iterations += 1
        x = recur(x, chebyshev(min(max(float(theta[-1]), FILTER_LOW), FILTER_HIGH), degree_))
        x[:, 0] = v0
        x, theta, res = rayleigh_ritz(orthonormalise(x))
    y = x[:, 1:k + 1]
    y = (y * (1.0 / np.sqrt(np.diag(tall_gram(y, y)))).astype(F32)[None, :]).astype(F32)
    big = np.abs(y).argmax(0)
    y = y * np.where(y[big, np.arange(k)] < 0, F32(-1), F32(1))[None, :]
    return y, dict(eigenvalues=1.0 - theta[:k + 1], residuals=res[:k + 1].copy(), iterations=iterations, products=products,
                   converged=bool(res[1:k + 1].max() < tol))


# ---- the truth, and the comparison --------------------------------------------------------------------------------------------------
def dense(rowptr, col, w) -> np.ndarray:
    R = rowptr.shape[0] - 1
    A = np.zeros((R, R), dtype=F64)
    A[U.entry_rows(rowptr), col.astype(np.int64)] = np.asarray(w, dtype=F64)
    return A


def dense_truth(rowptr, col, w):
    """(eigenvalues ascending, eigenvectors in columns, S) of L = I - D^-1/2 W D^-1/2 in fp64."""
    A = dense(rowptr, col, w)
    d = 1.0 / np.sqrt(A.sum(1))
    S = A * np.outer(d, d)
    S = (S + S.T) / 2.0
    lam, V = np.linalg.eigh(np.eye(A.shape[0]) - S)
    return lam, V, S


def cluster(lam: np.ndarray, j: int):
    lo = hi = j
    while lo > 0 and lam[lo] - lam[lo - 1] <= GAP:
        lo -= 1
    while hi + 1 < lam.shape[0] and lam[hi + 1] - lam[hi] <= GAP:
        hi += 1
    return lo, hi


def deviations(y: np.ndarray, eigenvalues: np.ndarray, truth):
    """(eig, vec, sub): the largest |eigenvalue - true| over the k + 1 values, the largest dev over the vectors alone in their
    cluster and over the others (0.0 where there is none of the kind)."""
    lam, V, _ = truth
    k = y.shape[1]
    eig = float(np.abs(np.asarray(eigenvalues) - lam[:k + 1]).max())
    vec = sub = 0.0
    for j in range(1, k + 1):
        lo, hi = cluster(lam, j)
        dev = abs(1.0 - float(np.linalg.norm(V[:, lo:hi + 1].T @ y[:, j - 1].astype(F64))))
        if lo == hi:
            vec = max(vec, dev)
        else:
            sub = max(sub, dev)
    return eig, vec, sub


def residuals64(y: np.ndarray, truth) -> np.ndarray:
    """||S y_j - (y_j^T S y_j) y_j||_2 in fp64, for unit y_j."""
    S = truth[2]
    y = y.astype(F64)
    sy = S @ y
    return np.linalg.norm(sy - y * (y * sy).sum(0)[None, :], axis=0)


def sign_rule_holds(y: np.ndarray) -> bool:
    big = np.abs(y).argmax(0)                                             # numpy: the first of equal ones
    return bool((y[big, np.arange(y.shape[1])] > 0).all())


# ---- the graphs ---------------------------------------------------------------------------------------------------------------------
def from_edges(R: int, i, j, wt):
    """The symmetric CSR graph (rowptr int64, col int32 ascending, w fp32) of the undirected edges {i, j} with weights wt."""
    i, j, wt = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64), np.asarray(wt, dtype=F32)
    rows, cols, ws = np.concatenate((i, j)), np.concatenate((j, i)), np.concatenate((wt, wt))
    order = np.lexsort((cols, rows))
    rowptr = np.zeros(R + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rows, minlength=R))
    return rowptr, cols[order].astype(np.int32), ws[order]


def path(R: int, seed: int = 1):
    g = np.random.default_rng(seed)
    return from_edges(R, np.arange(R - 1), np.arange(1, R), g.uniform(0.2, 1.0, max(R - 1, 0)))


def ring(R: int = 64):
    return from_edges(R, np.arange(R), (np.arange(R) + 1) % R, np.ones(R))


def blobs(bridge: bool = True, n: int = 40, seed: int = 2):
    g = np.random.default_rng(seed)
    a, b = np.triu_indices(n, 1)
    i, j = np.concatenate((a, a + n)), np.concatenate((b, b + n))
    wt = g.uniform(0.5, 1.0, i.shape[0])
    if bridge:
        i, j, wt = np.append(i, n - 1), np.append(j, n), np.append(wt, 1e-3)
    return from_edges(2 * n, i, j, wt)


STRIP = dict(R=400, d=10, m=10, seed=3)


def strip_points() -> np.ndarray:
    """fp32 [400, 10]: a 20:1 strip carried into 10 dimensions by two random directions, with a little noise."""
    g = np.random.default_rng(STRIP["seed"])
    u, v = g.uniform(0, 20, STRIP["R"]), g.uniform(0, 1, STRIP["R"])
    a, b = g.standard_normal(STRIP["d"]), g.standard_normal(STRIP["d"])
    return (np.outer(u, a) + np.outer(v, b) + 5.0 * g.standard_normal(STRIP["d"])[None, :] +
            0.01 * g.standard_normal((STRIP["R"], STRIP["d"]))).astype(F32)


_STRIP = {}


def strip():
    """The fuzzy graph of the strip through the numpy knn / smooth_knn / csr / union of tests/umap_cases.py; computed once."""
    if "g" not in _STRIP:
        idx, dist = U.knn(strip_points(), STRIP["m"])
        _, _, strength, _, _ = U.smooth_knn(idx, dist, U.mean_distance(idx, dist))
        rowptr, col = U.csr(idx, dist)
        _STRIP["g"] = (rowptr, col, U.union(idx, strength.astype(F32), rowptr, col).astype(F32))
    return _STRIP["g"]


def isolated():
    """path(64) and a 65th vertex without an entry."""
    rowptr, col, w = path(64)
    return np.append(rowptr, rowptr[-1]), col, w


# name -> (graph, n_components); every one connected.  The bridged blobs are asked for the Fiedler vector alone: their third
# eigenvalue lies among 78 nearly equal ones, which no filter of a useful degree separates.
CONNECTED = {"path65": (lambda: path(65), 2), "path257": (lambda: path(257), 2), "ring64": (ring, 2), "blobs-bridged": (blobs, 1),
             "strip400": (strip, 3)}
DISCONNECTED = {"blobs-apart": (lambda: blobs(False), 2), "isolated": (isolated, 2)}
SMALL = (1, 2, 3)                          # R of the size fallback, at n_components = 2: paths


def components(rowptr, col, w):
    """(count, labels) with scipy; a label is renumbered to the smallest vertex of its component."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    R = rowptr.shape[0] - 1
    count, lab = connected_components(csr_matrix((np.asarray(w, dtype=F64), col, rowptr), shape=(R, R)), directed=False)
    first = np.full(count, R, dtype=np.int64)
    np.minimum.at(first, lab, np.arange(R))
    return int(count), first[lab].astype(np.int32)


_TRUTH, _REFERENCE = {}, {}


def truth(name: str):
    if name not in _TRUTH:
        _TRUTH[name] = dense_truth(*CONNECTED[name][0]())
    return _TRUTH[name]


def reference(name: str, degree_: int = 40):
    """spectral_reference of a connected table graph, computed once per (graph, degree) and shared; callers do not write to it."""
    if (name, degree_) not in _REFERENCE:
        make, k = CONNECTED[name]
        y, info = spectral_reference(*make(), k=k, degree_=degree_)
        y.setflags(write=False)
        _REFERENCE[(name, degree_)] = (y, info)
    return _REFERENCE[(name, degree_)]


def kernel_graph(R: int, seed: int = 5):
    """A directed CSR graph for the kernels (they need no symmetry): at R = 257 the rows 0 .. 5 have the lengths ROW_LENGTHS, the
    others 0 .. 20 entries; columns ascending and distinct; from R = 63 on one entry names column -1 and one column R."""
    g = np.random.default_rng(seed + R)
    lens = g.integers(0, min(R, 20) + 1, R)
    if R >= 257:
        lens[:len(ROW_LENGTHS)] = ROW_LENGTHS
    cols = [np.sort(g.choice(R, int(n), replace=False)) for n in lens]
    rowptr = np.zeros(R + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(lens)
    col = (np.concatenate(cols) if rowptr[-1] else np.zeros(0)).astype(np.int32)
    if R >= 63 and col.shape[0] >= 2:
        col[g.integers(0, col.shape[0])] = -1
        col[g.integers(0, col.shape[0])] = R
    return rowptr, col, g.uniform(0.1, 1.0, col.shape[0]).astype(F32)

"""UMAP on the device: what vcf2embed's umap.UMAP(n_neighbors=30, min_dist=0.05, metric='correlation').fit_transform does over
~18 000 genes x 49 tissues, and what the same picture needs over the registry-token embeddings.

  find_ab(min_dist, spread)        the a, b of the curve 1 / (1 + a x^(2b)) that umap-learn fits with scipy, in plain numpy;
  fuzzy_graph(indices, distances)  the fuzzy simplicial set of a k-NN graph: (rowptr, col, w, rho, sigma);
  layout(graph, init, n_epochs, a, b, ...)   the SGD epochs over that graph from the positions `init`;
  umap(x, ...)                     neighbors.knn, fuzzy_graph, an initialisation and layout, on the device throughout;
  spectral_embedding(graph, n)     the eigenvectors of the graph's normalised Laplacian for its smallest non-trivial eigenvalues, by
                                   Chebyshev-filtered subspace iteration on the device (include/vf_hip_spectral.h);
  spectral_init                    that embedding as a callable `init` of umap: umap-learn's default init="spectral";
  spectral_init_components         the same start, and on a disconnected graph umap-learn's per-component layout: every component
                                   solved on its own and placed around a meta position (include/vf_hip_components.h);
  graph_components(graph)          the graph's connected components (labels, count), by a search on the device.

Three entries of include/vf_hip_umap.h do the work: ops.umap_smooth_knn (rho, sigma, directed strengths),
ops.umap_union (the fuzzy union over the symmetric graph, whose CSR arrays are built here with torch: index plumbing) and
ops.umap_layout (all epochs of a call from one loop inside the library).  The layout is a gather: a vertex reads the others where
they stood when the epoch began and writes only its own row, so a run has one result, bit for bit, whatever the hardware does,
and can be split at any epoch.  Two deliberate differences from umap-learn follow from that and are stated in DESIGN.md 5h: others
are read at epoch-start positions (umap-learn reads and writes them concurrently), and every drawn edge gets exactly
negative_sample_rate repulsions (umap-learn keeps a float schedule).  init is "pca", "random", an array or a callable
f(graph, n_components, seed) -> positions; umap-learn's default start is init=spectral_init (the string "spectral" stays refused
and names it).  On a disconnected graph spectral_init falls back to the random initialisation with a warning;
init=spectral_init_components lays every component out on its own instead, as umap-learn does.  There is no CPU path: without
a GPU the calls raise, after their arguments have been checked.  scipy, umap-learn, numba and pynndescent are not imported.

  fit(x, ...)                      umap(x, ...) kept as a UMAPModel: the embedding, the standardised rows, the fit's arguments;
  UMAPModel.transform(queries)     new rows placed in the fitted embedding, which stands still (transform(model, queries) is the
                                   same as a function); UMAPModel.state() / UMAPModel.from_state(dict) store and restore a model.

The transform runs through three entries of include/vf_hip_umap_transform.h: ops.umap_smooth_knn_query (the strengths
of a query's training neighbours), ops.umap_init_transform (its start among them) and ops.umap_layout_transform (all its epochs in
one kernel: a query depends on nothing that moves except itself).  A query's result depends on that row, the model, the epoch
count and its row number alone, so a cohort can be transformed in chunks, bit for bit.

  tsne(x, ...)                     t-SNE with the EXACT gradient, pinned stage by stage to scikit-learn's method="exact";
  tsne_affinities / tsne_descent / tsne_kl   its stages: the joint probabilities P over the k-NN graph, the iterations of the
                                   descent from given positions (a run can be split), the KL divergence of an embedding.

Four entries of include/vf_hip_tsne.h do that work: ops.tsne_perplexity (scikit-learn's binary search of every
row's beta), ops.tsne_joint (P = p_cond + p_cond^T over the symmetric CSR graph), ops.tsne_repulsion (one all-pairs pass over the
embedding, a gather with a stated summation order) and ops.tsne_descent (all iterations of a call from one loop inside the
library).  scikit-learn is not imported here: tests/tsne_cases.py holds the two together.
"""
from __future__ import annotations

import contextvars
import warnings

import numpy as np
import torch

from . import neighbors, ops

N_NEIGHBORS_MAX = neighbors.K_MAX          # n_neighbors counts the row itself: m = n_neighbors - 1 <= 63 others, one wavefront
DIM_MAX = 8                                # VF_UMAP_MAX_DIM
INITS = ("pca", "random")
_MASK = 0xFFFFFFFF


# ---- the curve -------------------------------------------------------------------------------------------------------------------
def find_ab(min_dist: float, spread: float = 1.0):
    """(a, b) of 1 / (1 + a x^(2b)) fitted to umap-learn's target -- 1 below min_dist, exp(-(x - min_dist) / spread) above, at
    300 points on [0, 3 spread] -- by least squares: a Levenberg-Marquardt iteration in fp64 numpy from a = b = 1, where
    umap-learn calls scipy.optimize.curve_fit (tests/test_umap_cpu.py holds the two together)."""
    min_dist, spread = float(min_dist), float(spread)
    if not (np.isfinite(spread) and spread > 0):
        raise ValueError(f"spread must be a positive number, not {spread!r}")
    if not (np.isfinite(min_dist) and 0 <= min_dist <= spread):
        raise ValueError(f"min_dist must lie in 0 .. spread={spread}, not {min_dist!r}")
    x = np.linspace(0.0, 3.0 * spread, 300)
    t = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    xs, ts = x[1:], t[1:]                                             # at x = 0 the curve is 1 whatever a and b are
    lx = np.log(xs)

    def residual(p):
        return 1.0 / (1.0 + p[0] * np.exp(2.0 * p[1] * lx)) - ts
    p = np.array([1.0, 1.0])
    r = residual(p)
    cost = float(r @ r)
    lam = 1e-3
    for _ in range(500):
        u = np.exp(2.0 * p[1] * lx)
        f = 1.0 / (1.0 + p[0] * u)
        J = np.stack((-f * f * u, -f * f * p[0] * u * 2.0 * lx), 1)
        A, g = J.T @ J, J.T @ r
        step = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
        q = p + step
        rq = residual(q) if q[0] > 0 and q[1] > 0 else None
        cq = float(rq @ rq) if rq is not None else np.inf
        if cq < cost:
            done = np.abs(step).max() <= 1e-14 * np.abs(p).max()
            p, r, cost, lam = q, rq, cq, max(lam / 10.0, 1e-12)
            if done:
                break
        else:
            if lam > 1e12:
                break
            lam *= 10.0
    return float(p[0]), float(p[1])


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def _int_in(value, name: str, lo: int, hi: int | None) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < lo or (hi is not None and value > hi):
        raise ValueError(f"{name} must be an integer in {lo} .. {hi if hi is not None else 'any'}, not {value!r}")
    return int(value)


def _number(value, name: str, lo: float, strict: bool) -> float:
    ok = isinstance(value, (int, float, np.integer, np.floating)) and not isinstance(value, bool) and np.isfinite(value) and \
        (value > lo if strict else value >= lo)
    if not ok:
        raise ValueError(f"{name} must be a finite number {'>' if strict else '>='} {lo}, not {value!r}")
    return float(value)


def _need_gpu():
    if not torch.cuda.is_available():
        raise ops._lib.VFError("variantformer_amd.manifold needs a GPU (no CPU fallback)")


def _tensor(t, dtype):
    t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
    return t.to(device="cuda", dtype=dtype)


def _check_graph_lists(indices, distances):
    for v, name in ((indices, "indices"), (distances, "distances")):
        if not isinstance(v, (np.ndarray, torch.Tensor)):
            raise TypeError(f"{name} must be a numpy array or a torch tensor, not {type(v).__name__}")
        if v.ndim != 2:
            raise ValueError(f"{name} must be a matrix [rows, neighbours], not {tuple(v.shape)}")
    if tuple(indices.shape) != tuple(distances.shape):
        raise ValueError(f"indices {tuple(indices.shape)} and distances {tuple(distances.shape)} must have one shape")
    if not 1 <= indices.shape[1] <= N_NEIGHBORS_MAX - 1:
        raise ValueError(f"the lists must hold 1 .. {N_NEIGHBORS_MAX - 1} neighbours per row (the row itself not among them), not {indices.shape[1]}")
    if indices.shape[0] > 1 << 24:
        raise ValueError(f"at most 2^24 rows, not {indices.shape[0]}")


# ---- the fuzzy simplicial set ------------------------------------------------------------------------------------------------------
def _mean_dist(idx: torch.Tensor, dist: torch.Tensor) -> float:
    """The fp64 mean of the present distances of a k-NN graph, 0 without one: the floor of sigma where rho == 0."""
    listed = (idx >= 0) & torch.isfinite(dist)
    return float(dist[listed].to(torch.float64).mean()) if bool(listed.any()) else 0.0


def _symmetric_csr(idx: torch.Tensor, listed: torch.Tensor):
    """(rowptr int64 [R + 1], col int32 [nnz]): the symmetric graph of the neighbour lists in CSR: every listed pair in both
    directions, once, columns ascending within a row; a row that lists itself makes no edge."""
    R, m = idx.shape
    dev = idx.device
    rows = torch.arange(R, dtype=torch.int64, device=dev)[:, None].expand(R, m)
    edge = listed & (idx != rows)
    i, j = rows[edge], idx[edge].to(torch.int64)
    keys = torch.unique(torch.cat((i * R + j, j * R + i)))             # sorted
    row = torch.div(keys, R, rounding_mode="floor")
    col = (keys - row * R).to(torch.int32)
    rowptr = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    if R:
        rowptr[1:] = torch.cumsum(torch.bincount(row, minlength=R), 0)
    return rowptr, col


def _fuzzy_graph(idx: torch.Tensor, dist: torch.Tensor):
    R, m = idx.shape
    dev = idx.device
    listed = (idx >= 0) & torch.isfinite(dist)                          # the header's "present"
    if bool((idx >= R).any()):
        raise ValueError(f"indices must name rows below {R}")
    mean_dist = _mean_dist(idx, dist)
    rho = torch.empty(R, dtype=torch.float32, device=dev)
    sigma = torch.empty(R, dtype=torch.float32, device=dev)
    strength = torch.empty((R, m), dtype=torch.float32, device=dev)
    ops.umap_smooth_knn(idx, dist, mean_dist, rho=rho, sigma=sigma, strength=strength, family="umap")
    rowptr, col = _symmetric_csr(idx, listed)
    w = torch.empty(col.shape[0], dtype=torch.float32, device=dev)
    ops.umap_union(idx, strength, rowptr, col, w=w, family="umap")
    return rowptr, col, w, rho, sigma


def fuzzy_graph(indices, distances):
    """The fuzzy simplicial set of a k-NN graph.  indices int [R, m] and distances [R, m]: the m <= 63 OTHER rows nearest to each
    row, as neighbors.knn(x, k=m) returns them (-1 / +Inf where a row has fewer; an entry with a NaN or infinite distance counts
    as not there).  Returns (rowptr int64 [R + 1], col int32 [nnz], w fp32 [nnz], rho fp32 [R], sigma fp32 [R]), of the type of
    `indices` (numpy arrays, or tensors on the device): the symmetric graph in CSR -- {i, j} is an edge if either lists the
    other, stored in both directions, columns ascending -- with the fuzzy union w = a + b - a b of the two directed membership
    strengths, the same bits in both directions; rho is each row's nearest positive distance and sigma solves
    sum_t exp(-max(0, d_t - rho) / sigma) = log2(m + 1), as in umap-learn with local_connectivity = 1."""
    _check_graph_lists(indices, distances)
    _need_gpu()
    out = _fuzzy_graph(_tensor(indices, torch.int32).contiguous(), _tensor(distances, torch.float32).contiguous())
    return neighbors._back(indices, *out)


def edge_samples(w: torch.Tensor, n_epochs: int) -> torch.Tensor:
    """int32 [nnz]: how often each entry is drawn in n_epochs epochs, floor(fl(fl(w / w_max) * n_epochs)) in individually rounded
    fp32; 0 for an entry with w < w_max / n_epochs, umap-learn's cut."""
    if w.numel() == 0:
        return torch.zeros(0, dtype=torch.int32, device=w.device)
    w_max = w.max()
    ratio = torch.where(w_max > 0, w / w_max, torch.zeros_like(w))
    return torch.floor(ratio * torch.tensor(float(n_epochs), dtype=torch.float32, device=w.device)).clamp_(0, n_epochs).to(torch.int32)


# ---- the layout --------------------------------------------------------------------------------------------------------------------
def _check_layout_args(n_epochs, a, b, gamma, learning_rate, negative_sample_rate, seed):
    n_epochs = _int_in(n_epochs, "n_epochs", 1, 2 ** 31 - 1)
    return (n_epochs, _number(a, "a", 0.0, True), _number(b, "b", 0.0, True), _number(gamma, "repulsion_strength", 0.0, False),
            _number(learning_rate, "learning_rate", 0.0, True), _int_in(negative_sample_rate, "negative_sample_rate", 0, 1 << 20),
            _int_in(seed, "seed", 0, 2 ** 32 - 1))


def _layout(rowptr, col, w, y, n_epochs, a, b, gamma, learning_rate, negative_sample_rate, seed, epoch_begin=0, epoch_end=None):
    epoch_end = n_epochs if epoch_end is None else epoch_end
    samples = edge_samples(w, n_epochs)
    y0 = y.clone()
    y1 = torch.empty_like(y0)
    return ops.umap_layout(rowptr, col, samples, y0, y1, epoch_begin=epoch_begin, epoch_end=epoch_end, n_epochs=n_epochs, a=a, b=b,
                           gamma=gamma, learning_rate=learning_rate, negative_sample_rate=negative_sample_rate, seed=seed, family="umap")


def layout(graph, init, n_epochs: int, a: float, b: float, repulsion_strength: float = 1.0, learning_rate: float = 1.0,
           negative_sample_rate: int = 5, seed: int = 42, epoch_begin: int = 0, epoch_end: int | None = None):
    """The epochs [epoch_begin, epoch_end) (default: all n_epochs) of the layout over `graph` -- what fuzzy_graph returned, or
    its first three members (rowptr, col, w) -- from the positions init [R, 1 .. 8], which are not written.  Returns fp32
    [R, dim] of the type of init.  Entry e is drawn floor(w[e] / w_max * n_epochs) times, spread evenly over the epochs by a
    stateless rule; the step shrinks linearly from learning_rate to 0 at epoch n_epochs; a and b are find_ab's.  The result
    depends on the arguments alone: two runs are equal bit for bit, and so is a run split at any epoch."""
    if not isinstance(graph, (tuple, list)) or len(graph) < 3:
        raise ValueError("graph must be what fuzzy_graph returned: (rowptr, col, w, ...)")
    if not isinstance(init, (np.ndarray, torch.Tensor)):
        raise TypeError(f"init must be a numpy array or a torch tensor, not {type(init).__name__}")
    if init.ndim != 2 or not 1 <= init.shape[1] <= DIM_MAX:
        raise ValueError(f"init must be positions [rows, 1 .. {DIM_MAX}], not {tuple(init.shape)}")
    if graph[0].shape[0] != init.shape[0] + 1:
        raise ValueError(f"the graph has {graph[0].shape[0] - 1} rows, init has {init.shape[0]}")
    n_epochs, a, b, gamma, learning_rate, negative_sample_rate, seed = _check_layout_args(
        n_epochs, a, b, repulsion_strength, learning_rate, negative_sample_rate, seed)
    epoch_end = n_epochs if epoch_end is None else epoch_end
    epoch_begin, epoch_end = _int_in(epoch_begin, "epoch_begin", 0, n_epochs), _int_in(epoch_end, "epoch_end", 0, n_epochs)
    if epoch_begin > epoch_end:
        raise ValueError(f"epoch_begin={epoch_begin} must not be above epoch_end={epoch_end}")
    _need_gpu()
    rowptr, col, w = _tensor(graph[0], torch.int64).contiguous(), _tensor(graph[1], torch.int32).contiguous(), _tensor(graph[2], torch.float32).contiguous()
    y = _layout(rowptr, col, w, _tensor(init, torch.float32).contiguous(), n_epochs, a, b, gamma, learning_rate, negative_sample_rate,
                seed, epoch_begin, epoch_end)
    return neighbors._back(init, y)[0]


# ---- initialisations ---------------------------------------------------------------------------------------------------------------
def _mix32(x: torch.Tensor) -> torch.Tensor:
    """The 32-bit mixer of include/vf_hip_umap.h on int64 tensors that hold uint32 values (products wrap; the low 32 bits are kept)."""
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _MASK
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _MASK
    return x ^ (x >> 16)


def random_init(rows: int, dim: int, seed: int, device="cuda") -> torch.Tensor:
    """fp32 [rows, dim] in [0, 1): element (i, c) is mix(mix(mix(seed + 0x85EBCA6B) ^ i) ^ c) >> 8 over 2^24 -- counter-based, so
    numpy restates it (tests/umap_cases.py) and it does not depend on the device's generator."""
    s = _mix32(torch.tensor([(int(seed) + 0x85EBCA6B) & _MASK], dtype=torch.int64, device=device))
    hi = _mix32(s ^ torch.arange(rows, dtype=torch.int64, device=device))[:, None]
    h = _mix32(hi ^ torch.arange(dim, dtype=torch.int64, device=device)[None, :])
    return (h >> 8).to(torch.float32) * (1.0 / (1 << 24))


def pca_init(x: torch.Tensor, dim: int) -> torch.Tensor:
    """fp32 [R, dim]: the rows of x on their first `dim` principal axes.  The d x d covariance is formed on the device, its
    eigenvectors are taken with numpy on the host in fp64, every axis is signed so that its largest-magnitude component is
    positive, and the projection runs on the device."""
    xc = x - x.mean(0, keepdim=True)
    cov = (xc.T @ xc).to(torch.float64).cpu().numpy() / max(x.shape[0] - 1, 1)
    _, vec = np.linalg.eigh((cov + cov.T) / 2.0)
    axes = vec[:, ::-1][:, :dim].copy()                                # descending eigenvalue
    big = np.abs(axes).argmax(0)
    axes *= np.where(axes[big, np.arange(axes.shape[1])] < 0, -1.0, 1.0)[None, :]
    return xc @ torch.from_numpy(axes.astype(np.float32)).to(x.device)


def rescale(y: torch.Tensor) -> torch.Tensor:
    """Every coordinate to [0, 10], as umap-learn scales an initialisation; a coordinate without spread becomes 0.  No noise."""
    lo, hi = y.amin(0, keepdim=True), y.amax(0, keepdim=True)
    span = hi - lo
    return torch.where(span > 0, 10.0 * (y - lo) / torch.where(span > 0, span, torch.ones_like(span)), torch.zeros_like(y))


# ---- the spectral embedding ----------------------------------------------------------------------------------------------------------
SPECTRAL_BLOCK_MAX = 32                    # VF_SPECTRAL_MAX_P
FILTER_LOW, FILTER_HIGH = -0.99, 1.0 - 1e-7   # where the upper end of the damped interval is held
ORTH_FLOOR = 1e-14                         # eigenvalues of the scaled Gram matrix below this share of the largest are raised to it
_ONE_STEP = np.array([[1.0, 0.0, 0.0]], dtype=np.float32)


def _graph_members(graph):
    if not isinstance(graph, (tuple, list)) or len(graph) < 3:
        raise ValueError("graph must be what fuzzy_graph returned: (rowptr, col, w, ...)")
    for v, name in zip(graph[:3], ("rowptr", "col", "w")):
        if not isinstance(v, (np.ndarray, torch.Tensor)) or v.ndim != 1:
            raise ValueError(f"graph: {name} must be a vector (numpy or torch)")
    R = graph[0].shape[0] - 1
    if R < 0 or R > 1 << 24 or graph[1].shape[0] != graph[2].shape[0]:
        raise ValueError("graph: rowptr must hold 1 .. 2^24 + 1 offsets, and col and w one entry each per edge")
    return R


def _graph_tensors(graph):
    return (_tensor(graph[0], torch.int64).contiguous(), _tensor(graph[1], torch.int32).contiguous(), _tensor(graph[2], torch.float32).contiguous())


COMPONENT_ROUNDS = 8                       # rounds of the component search per call: one scalar is read back per batch


def _components(rowptr: torch.Tensor, col: torch.Tensor, w: torch.Tensor):
    """(labels int32 [R] on the device, count): batches of COMPONENT_ROUNDS rounds of ops.graph_components_rounds from the
    identity until a batch's last round changed nothing.  The rounds are bounded by R + 1."""
    R = rowptr.shape[0] - 1
    dev = rowptr.device
    parent = torch.arange(R, dtype=torch.int32, device=dev)
    if R == 0:
        return parent, 0
    g, m = torch.empty_like(parent), torch.empty_like(parent)
    changed = torch.empty(1, dtype=torch.int32, device=dev)
    for _ in range(-(-(R + 1) // COMPONENT_ROUNDS)):
        ops.graph_components_rounds(rowptr, col, w, parent, g, m, changed, rounds=COMPONENT_ROUNDS, family="components")
        if int(changed) == 0:                                             # the batch's one scalar
            return parent, int((parent == torch.arange(R, dtype=torch.int32, device=dev)).sum())
    raise RuntimeError(f"graph_components did not settle in {R + 1} rounds")


def _components_torch(rowptr: torch.Tensor, col: torch.Tensor, w: torch.Tensor):
    """_components as torch index plumbing: min-label propagation over the edges with a full pointer-jumping sweep and one
    scalar read back per round.  A second reference of the search and the baseline of scripts/components_bench.py."""
    R = rowptr.shape[0] - 1
    dev = rowptr.device
    labels = torch.arange(R, dtype=torch.int64, device=dev)
    if R == 0:
        return labels.to(torch.int32), 0
    rows = torch.repeat_interleave(torch.arange(R, dtype=torch.int64, device=dev), rowptr[1:] - rowptr[:-1])
    cols = col.to(torch.int64)
    edge = (w > 0) & (cols >= 0) & (cols < R)                             # an entry without a positive weight is no edge
    rows, cols = rows[edge], cols[edge]
    jumps = max(int(R - 1).bit_length(), 1)
    for _ in range(R + 1):
        new = labels.scatter_reduce(0, rows, labels[cols], "amin", include_self=True)       # an integer minimum: one result
        for _ in range(jumps):                                            # pointer jumping: a label is a vertex of the component
            new = new[new]
        if not bool((new != labels).any()):                               # the round's one scalar
            return labels.to(torch.int32), int((labels == torch.arange(R, dtype=torch.int64, device=dev)).sum())
        labels = new
    raise RuntimeError(f"graph_components did not settle in {R + 1} rounds")


def graph_components(graph):
    """(labels int32 [R], count): the connected components of `graph` -- what fuzzy_graph returned, or (rowptr, col, w) -- by
    rounds of shortcut, gather and hook-onto-the-parent on the device (ops.graph_components_rounds,
    include/vf_hip_components.h); a batch of COMPONENT_ROUNDS rounds reads one scalar back, rounds are bounded by R + 1.  A
    label is the smallest vertex of its component; a vertex without an edge is a component of its own; an entry whose weight
    is not positive is no edge.  labels has the type of the graph's members."""
    _graph_members(graph)
    _need_gpu()
    labels, count = _components(*_graph_tensors(graph))
    return neighbors._back(graph[0], labels)[0], count


def chebyshev_coefficients(bound: float, degree: int) -> np.ndarray:
    """fp32 [degree, 3]: the coefficients ops.spmm_recur takes for the degree-`degree` Chebyshev filter p(S) that damps the
    eigenvalues in [-1, bound] (|p| <= p(bound)) and has p(1) = 1.  In fp64, rounded once: with c = (bound - 1) / 2,
    e = (bound + 1) / 2, sigma_1 = e / (1 - c): step 0 is (sigma_1 / e, -c sigma_1 / e, 0); step t >= 1 has
    sigma' = 1 / (2 / sigma_1 - sigma) and is (2 sigma' / e, -2 sigma' c / e, -sigma sigma'), then sigma = sigma'."""
    c, e = (bound - 1.0) / 2.0, (bound + 1.0) / 2.0
    sigma1 = e / (1.0 - c)
    sigma = sigma1
    coef = np.zeros((degree, 3), dtype=np.float64)
    coef[0] = (sigma1 / e, -c * sigma1 / e, 0.0)
    for t in range(1, degree):
        nxt = 1.0 / (2.0 / sigma1 - sigma)
        coef[t] = (2.0 * nxt / e, -2.0 * nxt * c / e, -sigma * nxt)
        sigma = nxt
    return coef.astype(np.float32)


def orthonormalising_matrix(G: np.ndarray) -> np.ndarray:
    """fp64 [p, p] T with X T orthonormal, from G = X^T X, for a block whose column 0 is the locked trivial eigenvector: column 0
    of T is the unit vector (X T keeps it bit for bit); the other columns are first made orthogonal to it (c = G[0, 1:] / G[0, 0],
    G' = G[1:, 1:] - G[0, 0] c c^T), then G' is scaled to a unit diagonal by d = sqrt(diag G'), decomposed as V diag(lam) V^T
    (lam raised to ORTH_FLOOR max(lam) at least), and M = diag(1 / d) V diag(lam^-1/2); T[0, 1:] = -c M, T[1:, 1:] = M.  No
    Cholesky factor: a filtered block is too ill-conditioned for one.  Applied twice."""
    p = G.shape[0]
    T = np.zeros((p, p), dtype=np.float64)
    T[0, 0] = 1.0
    if p == 1:
        return T
    c = G[0, 1:] / G[0, 0]
    Gp = G[1:, 1:] - G[0, 0] * np.outer(c, c)
    Gp = (Gp + Gp.T) / 2.0
    d = np.sqrt(np.where(np.diag(Gp) > 0, np.diag(Gp), 1.0))
    lam, V = np.linalg.eigh(Gp / np.outer(d, d))
    lam = np.maximum(lam, ORTH_FLOOR * max(lam.max(), np.finfo(np.float64).tiny))
    M = (V / np.sqrt(lam)[None, :]) / d[:, None]
    T[0, 1:] = -c @ M
    T[1:, 1:] = M
    return T


def _spectral(rowptr, col, w, deg, dinv, k: int, block: int, degree: int, tol: float, max_iter: int, seed: int):
    """The eigensolver on a connected graph with positive degrees: (vectors fp32 [R, k] on the device, info)."""
    R = rowptr.shape[0] - 1
    dev = rowptr.device
    p = min(block, R)
    bufs = [torch.empty((R, p), dtype=torch.float32, device=dev) for _ in range(3)]
    work = torch.empty(ops.TALL_GRAM_MAX_BLOCKS * p * p, dtype=torch.float64, device=dev)
    products = 0

    def gram(a, b):
        out = torch.empty((a.shape[1], b.shape[1]), dtype=torch.float64, device=dev)
        return ops.tall_gram(a, b, out=out, work=work, family="spectral").cpu().numpy()

    def others(x):
        return [b for b in bufs if b is not x]

    def recur(x, coef):
        nonlocal products
        o = others(x)
        products += coef.shape[0]
        return ops.spmm_recur(rowptr, col, w, dinv, x, o[0], o[1], coef, family="spectral")

    def times(x, T):
        return ops.tall_mul(x, torch.from_numpy(np.ascontiguousarray(T)).to(dev), out=others(x)[0], family="spectral")

    def orthonormalise(x):
        for _ in range(2):
            x = times(x, orthonormalising_matrix(gram(x, x)))
        return x

    def rayleigh_ritz(x):
        H = gram(x, recur(x, _ONE_STEP))
        H = (H + H.T) / 2.0
        lam, Q = np.linalg.eigh(H[1:, 1:]) if p > 1 else (np.zeros(0), np.zeros((0, 0)))
        lam, Q = lam[::-1], Q[:, ::-1]                                  # descending in S: ascending in L = I - S
        T = np.zeros((p, p), dtype=np.float64)
        T[0, 0] = 1.0
        T[1:, 1:] = Q
        theta = np.concatenate(([H[0, 0]], lam))
        x = times(x, T)
        sx = recur(x, _ONE_STEP)
        th = torch.from_numpy(theta[:k + 1].astype(np.float32)).to(dev)
        r = sx[:, :k + 1] - x[:, :k + 1] * th[None, :]
        return x, theta, np.sqrt(np.diag(gram(r, r)))

    # the trivial eigenvector sqrt(deg) / ||sqrt(deg)|| is locked as column 0; the other columns start from the hash
    x = bufs[0]
    x.copy_(random_init(R, p, seed, dev) - 0.5)
    v0 = torch.sqrt(deg)
    v0 = v0 * float(1.0 / np.sqrt(gram(v0[:, None], v0[:, None])[0, 0]))
    x[:, 0] = v0
    x, theta, res = rayleigh_ritz(orthonormalise(x))
    iterations = 0
    while res[1:k + 1].max() >= tol and iterations < max_iter:
        iterations += 1
        bound = min(max(float(theta[-1]), FILTER_LOW), FILTER_HIGH)      # the block's smallest Ritz value
        x = recur(x, chebyshev_coefficients(bound, degree))
        x[:, 0] = v0
        x, theta, res = rayleigh_ritz(orthonormalise(x))
    converged = bool(res[1:k + 1].max() < tol)
    if not converged:
        warnings.warn(f"spectral_embedding stopped at max_iter={max_iter} with a residual of {res[1:k + 1].max():.3e} (tol={tol:g})",
                      RuntimeWarning, stacklevel=3)
    y = x[:, 1:k + 1]
    y = y * torch.from_numpy((1.0 / np.sqrt(np.diag(gram(y, y)))).astype(np.float32)).to(dev)[None, :]
    big = y.abs().argmax(0)                                               # the first of equal magnitudes
    y = y * torch.where(y[big, torch.arange(k, device=dev)] < 0, -1.0, 1.0)[None, :]
    info = dict(eigenvalues=1.0 - theta[:k + 1], residuals=res[:k + 1].copy(), iterations=iterations, products=products, converged=converged)
    return y.contiguous(), info


def _check_spectral_args(n_components, block, degree, tol, max_iter, seed):
    n_components = _int_in(n_components, "n_components", 1, DIM_MAX)
    block = _int_in(block, "block", n_components + 1, SPECTRAL_BLOCK_MAX)
    return (n_components, block, _int_in(degree, "degree", 2, 1 << 16), _number(tol, "tol", 0.0, True),
            _int_in(max_iter, "max_iter", 0, 1 << 20), _int_in(seed, "seed", 0, 2 ** 32 - 1))


def _degrees(rowptr, col, w):
    R = rowptr.shape[0] - 1
    deg = torch.empty(R, dtype=torch.float32, device=rowptr.device)
    dinv = torch.empty(R, dtype=torch.float32, device=rowptr.device)
    return ops.graph_degree(rowptr, col, w, deg=deg, dinv_sqrt=dinv, family="spectral")


def spectral_embedding(graph, n_components: int = 2, *, block: int = 16, degree: int = 40, tol: float = 1e-4, max_iter: int = 50,
                       seed: int = 42, return_info: bool = False):
    """fp32 [R, n_components], of the type of the graph's members: the eigenvectors of the normalised Laplacian
    L = I - D^-1/2 W D^-1/2 of `graph` -- what fuzzy_graph returned, or (rowptr, col, w) -- for its 2nd .. (n_components + 1)-th
    smallest eigenvalues, ascending: what umap-learn's spectral_layout takes.  Each has unit norm and is signed so that its
    largest-magnitude component is positive (the first of equal ones), pca_init's rule.

    Chebyshev-filtered subspace iteration on the device (include/vf_hip_spectral.h) in S = D^-1/2 W D^-1/2, whose
    largest eigenvalues are L's smallest.  The block has p = min(block, R) columns.  Column 0 is LOCKED to the known trivial
    eigenvector sqrt(deg) / ||sqrt(deg)||: it is set, never iterated, and every orthonormalisation projects the others against
    it.  The others start from random_init(R, p, seed) - 0.5.  Orthonormalisation is X <- X T with T from the eigen-decomposition
    of the column-scaled fp64 Gram matrix (orthonormalising_matrix), applied twice; Rayleigh-Ritz takes H = X^T (S X) through
    ops.tall_gram, numpy's eigh of the symmetrised matrix in fp64 on the host, X <- X Q, and the residuals ||S x - theta x||_2 of
    the rotated columns from a fresh product.  Every outer iteration applies chebyshev_coefficients(bound, degree) through one
    ops.spmm_recur call, bound the block's smallest Ritz value held in [-0.99, 1 - 1e-7], then orthonormalises and rotates again;
    it stops when the wanted residuals are below tol, or at max_iter with a RuntimeWarning that states the worst residual (the
    current vectors are returned).  X Q and X T are ops.tall_mul, the library's own kernel: nothing of the solver's arithmetic
    is torch's but elementwise operations, so two runs are equal bit for bit.

    return_info=True: (vectors, dict) with `eigenvalues` (of L, fp64, n_components + 1 of them: the trivial one first),
    `residuals` (likewise), `iterations` (outer), `products` (sparse block products S Y) and `converged`.
    ValueError before the device is touched: n_components outside 1 .. 8, block outside n_components + 1 .. 32, degree < 2,
    tol <= 0.  ValueError after the degrees and components have been computed on the device: R < n_components + 2; a graph of
    more than one component (isolated vertices count; the message states how many)."""
    R = _graph_members(graph)
    k, block, degree, tol, max_iter, seed = _check_spectral_args(n_components, block, degree, tol, max_iter, seed)
    _need_gpu()
    rowptr, col, w = _graph_tensors(graph)
    deg, dinv = _degrees(rowptr, col, w)
    _, count = _components(rowptr, col, w)
    if R < k + 2:
        raise ValueError(f"spectral_embedding needs at least n_components + 2 = {k + 2} vertices, the graph has {R}")
    if count != 1:
        raise ValueError(f"spectral_embedding needs a connected graph, this one has {count} components (isolated vertices count)")
    if not bool((deg > 0).all()):
        raise ValueError("spectral_embedding needs positive degrees: the weights of some vertex do not sum to a positive number")
    y, info = _spectral(rowptr, col, w, deg, dinv, k, block, degree, tol, max_iter, seed)
    y = neighbors._back(graph[0], y)[0]
    return (y, info) if return_info else y


def spectral_init(graph, n_components: int, seed: int):
    """An `init` for umap: spectral_embedding(graph, n_components, seed=seed) on a connected graph of at least n_components + 2
    vertices.  Otherwise a RuntimeWarning that names the number of components or the size, and random_init(R, n_components,
    seed): umap-learn's own fallback when its eigensolver fails (its per-component layout of a disconnected graph is
    spectral_init_components).  Well-separated clusters do disconnect a k-NN graph, so the fallback is no rarity.  Returns a
    tensor on the device."""
    R = _graph_members(graph)
    k, _, _, _, _, seed = _check_spectral_args(n_components, SPECTRAL_BLOCK_MAX, 40, 1e-4, 50, seed)
    _need_gpu()
    rowptr, col, w = _graph_tensors(graph)
    if R < k + 2:
        warnings.warn(f"spectral_init: {R} vertices are fewer than n_components + 2 = {k + 2}; the random initialisation is used", RuntimeWarning, stacklevel=2)
        return random_init(R, k, seed, rowptr.device)
    deg, dinv = _degrees(rowptr, col, w)
    _, count = _components(rowptr, col, w)
    if count != 1 or not bool((deg > 0).all()):
        warnings.warn(f"spectral_init: the graph has {count} components (isolated vertices count); the random initialisation is used",
                      RuntimeWarning, stacklevel=2)
        return random_init(R, k, seed, rowptr.device)
    return _spectral(rowptr, col, w, deg, dinv, k, 16, 40, 1e-4, 50, seed)[0]


# ---- the spectral start of a disconnected graph --------------------------------------------------------------------------------------
COMPONENTS_MAX = 2048                      # more components than this take the random fallback: the solver loop is the host's


def meta_positions(count: int, dim: int, centroids=None, metric: str = "correlation") -> np.ndarray:
    """fp64 [count, dim]: where umap-learn's multi_component_layout puts `count` components, in label order, on the host.
    count <= 2 dim: the rows of [I_k | 0] and then of -[I_k | 0] with k = ceil(count / 2), cut to count.  Otherwise the spectral
    embedding of the components' `centroids` [count, d]: the rows standardised for `metric` (a correlation centres them, a
    cosine does not; a row without spread becomes 0), D = 1 - z z^T with a zero diagonal, the affinity A = exp(-D^2) with its
    diagonal dropped, the eigenvectors 2 .. dim + 1 of I - D_A^-1/2 A D_A^-1/2 (numpy's eigh) scaled by D_A^-1/2, every one
    signed so that its largest-magnitude component is positive (the solver's rule), all divided by the largest magnitude
    overall: scikit-learn's SpectralEmbedding(affinity="precomputed") up to sign and a scale per column.  umap-learn divides
    by the signed maximum instead."""
    if count <= 2 * dim:
        k = -(-count // 2)
        base = np.zeros((k, dim), dtype=np.float64)
        base[np.arange(k), np.arange(k)] = 1.0
        return np.concatenate((base, -base))[:count]
    if centroids is None:
        raise ValueError(f"{count} components are more than 2 n_components = {2 * dim}: their meta positions need the data, pass `rows`")
    z = np.array(centroids, dtype=np.float64)
    if metric == "correlation":
        z = z - z.mean(1, keepdims=True)
    norm = np.sqrt((z * z).sum(1, keepdims=True))
    z = np.where(norm > 0, z / np.where(norm > 0, norm, 1.0), 0.0)
    D = 1.0 - z @ z.T
    np.fill_diagonal(D, 0.0)
    A = np.exp(-D * D)
    np.fill_diagonal(A, 0.0)
    dinv = 1.0 / np.sqrt(A.sum(1))
    L = np.eye(count) - A * np.outer(dinv, dinv)
    _, vec = np.linalg.eigh((L + L.T) / 2.0)
    y = vec[:, 1:dim + 1] * dinv[:, None]
    big = np.abs(y).argmax(0)
    y = y * np.where(y[big, np.arange(dim)] < 0, -1.0, 1.0)[None, :]
    return y / np.abs(y).max()


def data_ranges(meta: np.ndarray) -> np.ndarray:
    """fp64 [count]: half the smallest positive Euclidean distance from each meta position to another (+Inf without one)."""
    d2 = np.zeros((meta.shape[0], meta.shape[0]), dtype=np.float64)
    for c in range(meta.shape[1]):
        d2 += (meta[:, None, c] - meta[None, :, c]) ** 2
    d = np.sqrt(d2)
    return np.where(d > 0, d, np.inf).min(1) / 2.0


def _random_fallback(count: int, why: str, R: int, k: int, seed: int, device):
    warnings.warn(f"spectral_init_components: the graph has {count} components ({why}); the random initialisation is used",
                  RuntimeWarning, stacklevel=3)
    return random_init(R, k, seed, device)


def spectral_init_components(graph, n_components: int, seed: int, rows=None, metric: str = "correlation"):
    """An `init` for umap that keeps the spectral start on a DISCONNECTED graph: umap-learn's multi_component_layout.  On a
    connected graph it is spectral_init, bit for bit (the size fallback included).  Otherwise, with C components in label
    order (a label is the component's smallest vertex) and dim = n_components:

      the graph is renumbered on the device so that every component is a contiguous range of rows with local columns
      (a stable torch sort of the labels, then ops.csr_components), and its degrees are taken again;
      meta_positions(C, dim, centroids, metric) places the components: for C > 2 dim from the centroids of `rows` [R, d] (the
      data the graph was built from; ops.segment_mean_gather on the device, the C x C eigenproblem in fp64 on the host), which
      are then required -- ValueError that names `rows` without them;
      data_range(c) is half the smallest positive distance from meta position c to another, rounded to fp32;
      a component of fewer than max(2 dim, dim + 2) vertices gets (2 u - 1) data_range + meta with u its vertices' OWN rows of
      random_init(R, dim, seed): counter-based, so no order enters;
      any other component is solved by the eigensolver with spectral_init's arguments on its slice of the renumbered graph,
      y, and placed as y * (data_range / max|y|) + meta.

    All of that is fp32 with every operation rounded once, so the result is a function of the arguments, bit for bit.  More
    than COMPONENTS_MAX = 2048 components, meta positions that do not separate, or a solved component with a vertex whose
    degree is not positive, take spectral_init's fallback: a RuntimeWarning that states the count, and random_init.  The
    components are solved one after another from the host (umap-learn loops too).  umap passes `rows` and `metric` itself: the
    callable carries wants_rows = True.  Returns a tensor on the device."""
    R = _graph_members(graph)
    k, _, _, _, _, seed = _check_spectral_args(n_components, SPECTRAL_BLOCK_MAX, 40, 1e-4, 50, seed)
    if metric not in neighbors.METRICS:
        raise ValueError(f"metric must be one of {neighbors.METRICS}, not {metric!r}")
    if rows is not None:
        neighbors._check_matrix(rows, "rows")
        if rows.shape[0] != R:
            raise ValueError(f"rows has {rows.shape[0]} rows, the graph has {R} vertices")
    _need_gpu()
    rowptr, col, w = _graph_tensors(graph)
    dev = rowptr.device
    if R < k + 2:
        warnings.warn(f"spectral_init_components: {R} vertices are fewer than n_components + 2 = {k + 2}; the random initialisation is used",
                      RuntimeWarning, stacklevel=2)
        return random_init(R, k, seed, dev)
    deg, dinv = _degrees(rowptr, col, w)
    labels, count = _components(rowptr, col, w)
    if count == 1:
        if not bool((deg > 0).all()):
            return _random_fallback(count, "and a vertex whose degree is not positive", R, k, seed, dev)
        return _spectral(rowptr, col, w, deg, dinv, k, 16, 40, 1e-4, 50, seed)[0]
    if count > COMPONENTS_MAX:
        return _random_fallback(count, f"more than {COMPONENTS_MAX}", R, k, seed, dev)
    if count > 2 * k and rows is None:
        raise ValueError(f"spectral_init_components: {count} components are more than 2 n_components = {2 * k}: their meta positions "
                         "need the data the graph was built from, pass `rows`")
    # the graph renumbered by components: index plumbing in torch, the entries in HIP
    sorted_labels, order64 = torch.sort(labels, stable=True)
    order = order64.to(torch.int32)
    rank = torch.empty_like(order)
    rank[order64] = torch.arange(R, dtype=torch.int32, device=dev)
    first = torch.ones(R, dtype=torch.bool, device=dev)
    first[1:] = sorted_labels[1:] != sorted_labels[:-1]
    comp = (torch.cumsum(first, 0) - 1).to(torch.int32)
    starts = torch.cat((torch.nonzero(first)[:, 0], torch.tensor([R], dtype=torch.int64, device=dev))).to(torch.int32)
    rowptr_new = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    rowptr_new[1:] = torch.cumsum((rowptr[1:] - rowptr[:-1])[order64], 0)
    col_new, w_new = torch.empty_like(col), torch.empty_like(w)
    ops.csr_components(rowptr, col, w, order, rank, comp, starts, rowptr_new, col_new=col_new, w_new=w_new, family="components")
    deg_new, dinv_new = _degrees(rowptr_new, col_new, w_new)
    starts_h = starts.cpu().numpy().astype(np.int64)
    entries_h = rowptr_new[starts.to(torch.int64)].cpu().numpy()
    solved = np.diff(starts_h) >= max(2 * k, k + 2)
    if bool((torch.from_numpy(solved).to(dev)[comp.to(torch.int64)] & ~(deg_new > 0)).any()):
        return _random_fallback(count, "and a vertex whose degree is not positive", R, k, seed, dev)
    # where the components go
    centroids = None
    if count > 2 * k:
        x = _tensor(rows, torch.float32)
        x = x if x.stride(1) == 1 or x.shape[1] <= 1 else x.contiguous()
        centroids = torch.empty((count, x.shape[1]), dtype=torch.float32, device=dev)
        centroids = ops.segment_mean_gather(x, order, starts, out=centroids, family="components").cpu().numpy()
    meta = meta_positions(count, k, centroids, metric)
    spread = data_ranges(meta)
    if not (np.isfinite(meta).all() and np.isfinite(spread).all()):
        return _random_fallback(count, "whose meta positions do not separate", R, k, seed, dev)
    meta32 = torch.from_numpy(meta.astype(np.float32)).to(dev)
    spread32 = torch.from_numpy(spread.astype(np.float32)).to(dev)
    # every vertex as in a small component, from its own row of the hash; the solved components are then written over
    of_vertex = comp[rank.to(torch.int64)].to(torch.int64)
    y = (2.0 * random_init(R, k, seed, dev) - 1.0) * spread32[of_vertex][:, None]
    y = y + meta32[of_vertex]
    for c in np.nonzero(solved)[0]:
        s, e, a, b = int(starts_h[c]), int(starts_h[c + 1]), int(entries_h[c]), int(entries_h[c + 1])
        v = _spectral(rowptr_new[s:e + 1] - a, col_new[a:b], w_new[a:b], deg_new[s:e], dinv_new[s:e], k, 16, 40, 1e-4, 50, seed)[0]
        placed = v * (spread32[c] / v.abs().max())
        y[order64[s:e]] = placed + meta32[c]
    return y


spectral_init_components.wants_rows = True


# ---- the whole ---------------------------------------------------------------------------------------------------------------------
def _called_init(init, graph, R: int, n_components: int, seed: int):
    """What the callable `init` returns for (graph, n_components, seed), refused unless it is positions [R, n_components]."""
    y = init(graph, n_components, seed)
    if not isinstance(y, (np.ndarray, torch.Tensor)) or tuple(y.shape) != (R, n_components):
        raise ValueError(f"init: the callable must return positions [{R}, {n_components}] (numpy or torch), not "
                         f"{tuple(y.shape) if hasattr(y, 'shape') else type(y).__name__}")
    return y


def _with_rows(init, rows, metric: str):
    """The callable `init` as one of three arguments, with rows= and metric= handed on."""
    return lambda graph, n_components, seed: init(graph, n_components, seed, rows=rows, metric=metric)


def umap(x, n_neighbors: int = 30, min_dist: float = 0.1, metric: str = "correlation", n_components: int = 2, n_epochs=None,
         init="pca", seed: int = 42, negative_sample_rate: int = 5, repulsion_strength: float = 1.0, learning_rate: float = 1.0):
    """The UMAP embedding of the rows of x [R, d] (numpy or torch): fp32 [R, n_components] of the type of x.

    n_neighbors 2 .. 64 counts the row itself as umap-learn does: the graph is neighbors.knn(x, n_neighbors - 1, metric).
    min_dist 0 .. 1 gives the curve through find_ab (spread 1).  n_epochs None: 500 for R <= 10000, else 200.  init: "pca"
    (d >= n_components), "random" (counter-based from `seed`), an array [R, n_components] or a callable
    f(graph, n_components, seed) -> positions [R, n_components] (numpy or torch; graph = (rowptr, col, w), the device tensors of
    the fuzzy graph; a result of another shape is refused); every init is rescaled per coordinate to [0, 10] and no noise is
    added.  init=manifold.spectral_init is umap-learn's default spectral start (the string "spectral" is refused and names it);
    init=manifold.spectral_init_components keeps that start on a disconnected graph, every component laid out on its own.  A
    callable that carries wants_rows = True is called as f(graph, n_components, seed, rows=x on the device, metric=metric).
    New points are placed in a finished embedding by fit(x, ...).transform(queries): fit takes these arguments and keeps what a
    transform needs.  seed also fixes the negative samples: the result is a function of the arguments, bit for bit.
    Differences from umap-learn, deliberate: other vertices are read where they stood when the epoch began, and
    every drawn edge gets exactly negative_sample_rate repulsions."""
    neighbors._check_matrix(x, "x")
    if metric not in neighbors.METRICS:
        raise ValueError(f"metric must be one of {neighbors.METRICS}, not {metric!r}")
    n_neighbors = _int_in(n_neighbors, "n_neighbors", 2, N_NEIGHBORS_MAX)
    n_components = _int_in(n_components, "n_components", 1, DIM_MAX)
    min_dist = _number(min_dist, "min_dist", 0.0, False)
    if min_dist > 1.0:
        raise ValueError(f"min_dist must lie in 0 .. 1 (the spread), not {min_dist!r}")
    R = x.shape[0]
    if R < 1 or R > 1 << 24:
        raise ValueError(f"x must hold 1 .. 2^24 rows, not {R}")
    if n_epochs is None:
        n_epochs = 500 if R <= 10000 else 200
    if isinstance(init, str):
        if init == "spectral":
            raise ValueError("init='spectral' is not a name here: pass init=manifold.spectral_init, the callable")
        if init not in INITS:
            raise ValueError(f"init must be one of {INITS}, an array [rows, n_components] or a callable such as manifold.spectral_init, not {init!r}")
        if init == "pca" and x.shape[1] < n_components:
            raise ValueError(f"init='pca' needs at least n_components={n_components} columns, x has {x.shape[1]}")
    elif callable(init):
        pass                                                              # its result is checked when it has been called
    elif not isinstance(init, (np.ndarray, torch.Tensor)) or tuple(init.shape) != (R, n_components):
        raise ValueError(f"init must be one of {INITS}, a callable or an array [{R}, {n_components}]")
    a, b = find_ab(min_dist)
    n_epochs, a, b, gamma, learning_rate, negative_sample_rate, seed = _check_layout_args(
        n_epochs, a, b, repulsion_strength, learning_rate, negative_sample_rate, seed)
    t = neighbors._to_device(x, True)
    idx, dist = neighbors.knn(t, k=n_neighbors - 1, metric=metric)
    rowptr, col, w, _, _ = _fuzzy_graph(idx, dist)
    if isinstance(init, str):
        y = pca_init(t, n_components) if init == "pca" else random_init(R, n_components, seed, t.device)
    elif callable(init):
        if getattr(init, "wants_rows", False):                            # it asks for the data: spectral_init_components does
            init = _with_rows(init, t, metric)
        y = _tensor(_called_init(init, (rowptr, col, w), R, n_components, seed), torch.float32)
    else:
        y = _tensor(init, torch.float32)
    y = _layout(rowptr, col, w, rescale(y).contiguous(), n_epochs, a, b, gamma, learning_rate, negative_sample_rate, seed)
    fitted = _FITTED.get()
    if fitted is not None:                                                # fit() is asking: what a transform needs beside the embedding
        fitted.update(rows=t, embedding=y, mean_dist=_mean_dist(idx, dist), n_neighbors=n_neighbors, metric=metric, a=a, b=b,
                      n_epochs=n_epochs, seed=seed, negative_sample_rate=negative_sample_rate, repulsion_strength=gamma,
                      learning_rate=learning_rate)
    return neighbors._back(x, y)[0]


# ---- a fitted model and the transform of new rows ------------------------------------------------------------------------------------
_FITTED: contextvars.ContextVar = contextvars.ContextVar("variantformer_amd_manifold_fitted", default=None)
QUERIES_MAX = 1 << 24                      # VF_UMAP_MAX_R
_STATE_SCALARS = ("n_neighbors", "metric", "a", "b", "n_epochs", "seed", "negative_sample_rate", "repulsion_strength", "learning_rate",
                  "mean_dist")


def transform_samples(strength: torch.Tensor, n_epochs: int) -> torch.Tensor:
    """int32 like strength: how often each entry of a query's list is drawn in n_epochs epochs,
    floor(fl(fl(strength / rowmax) * n_epochs)) in individually rounded fp32 with rowmax the ROW's largest strength (umap-learn
    divides by the batch's: DESIGN.md 5j); 0 in a row whose largest strength is 0."""
    if strength.numel() == 0:
        return torch.zeros(strength.shape, dtype=torch.int32, device=strength.device)
    rowmax = strength.amax(1, keepdim=True)
    ratio = torch.where(rowmax > 0, strength / rowmax, torch.zeros_like(strength))
    return torch.floor(ratio * torch.tensor(float(n_epochs), dtype=torch.float32, device=strength.device)).clamp_(0, n_epochs).to(torch.int32)


class UMAPModel:
    """A fitted UMAP: what manifold.fit returns and UMAPModel.from_state restores.  Attributes: `embedding` fp32
    [rows, n_components] (of the type of the fitted x), `rows`, `n_components`, `n_neighbors`, `metric`, `a`, `b`, `n_epochs`,
    `seed`, `negative_sample_rate`, `repulsion_strength`, `learning_rate` (all as the fit used them) and `mean_dist`, the fp64
    mean of the fit's present k-NN distances.  The model also keeps the STANDARDISED training rows (zero mean for a correlation,
    unit norm), on the device once a transform has run, so that a transform standardises only its queries."""

    def __init__(self, embedding, *, z=None, x=None, n_neighbors, metric, a, b, n_epochs, seed, negative_sample_rate, repulsion_strength,
                 learning_rate, mean_dist):
        if not isinstance(embedding, (np.ndarray, torch.Tensor)):
            raise TypeError(f"embedding must be a numpy array or a torch tensor, not {type(embedding).__name__}")
        if embedding.ndim != 2 or not 1 <= embedding.shape[1] <= DIM_MAX:
            raise ValueError(f"embedding must be positions [rows, 1 .. {DIM_MAX}], not {tuple(embedding.shape)}")
        rows = z if z is not None else x
        if rows is None:
            raise ValueError("a model needs its training rows: `z` (standardised, as state() returns them) or `x` (as fitted)")
        neighbors._check_matrix(rows, "z" if z is not None else "x")
        if rows.shape[0] != embedding.shape[0]:
            raise ValueError(f"embedding has {embedding.shape[0]} rows, the training rows are {rows.shape[0]}")
        if not 1 <= rows.shape[0] <= 1 << 24:
            raise ValueError(f"a model holds 1 .. 2^24 training rows, not {rows.shape[0]}")
        if metric not in neighbors.METRICS:
            raise ValueError(f"metric must be one of {neighbors.METRICS}, not {metric!r}")
        self.embedding = embedding
        self.rows, self.columns, self.n_components = int(rows.shape[0]), int(rows.shape[1]), int(embedding.shape[1])
        self.metric = str(metric)
        self.n_neighbors = _int_in(n_neighbors, "n_neighbors", 1, N_NEIGHBORS_MAX)
        (self.n_epochs, self.a, self.b, self.repulsion_strength, self.learning_rate, self.negative_sample_rate, self.seed) = \
            _check_layout_args(n_epochs, a, b, repulsion_strength, learning_rate, negative_sample_rate, seed)
        if isinstance(mean_dist, bool) or not isinstance(mean_dist, (int, float, np.integer, np.floating)):
            raise ValueError(f"mean_dist must be a number, not {mean_dist!r}")
        self.mean_dist = float(mean_dist)
        self._z, self._standardised = rows, z is not None
        self._y = None

    # -- persistence
    def state(self) -> dict:
        """Everything a transform needs, as numpy arrays and scalars (np.savez(path, **model.state()) stores it):
        `embedding` fp32 [rows, n_components], `z` fp32 [rows, columns] -- the standardised training rows, bit for bit what the
        transform multiplies by --, and the scalars.  A model restored with from_state transforms to the same bits."""
        if not self._standardised:
            self._on_device()

        def host(t):
            return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)
        out = {"embedding": host(self.embedding if self._y is None else self._y), "z": host(self._z)}
        out.update({name: getattr(self, name) for name in _STATE_SCALARS})
        return out

    @classmethod
    def from_state(cls, state) -> "UMAPModel":
        """The model of a state(): a dict (or an opened .npz) with `embedding` [rows, 1 .. 8], the training rows -- `z`,
        standardised as state() returns them and used as they are, or else `x`, raw rows [rows, columns] that are standardised
        for `metric` on the device (NaN -> 0 first, as in a fit) -- and the scalars n_neighbors (1 .. 64: the training rows a
        query is attached to), metric, a, b, n_epochs, seed, negative_sample_rate, repulsion_strength, learning_rate, mean_dist.
        Any embedding of the training rows is accepted, not only a fit's.  Nothing touches the device before a transform."""
        missing = [k for k in ("embedding",) + _STATE_SCALARS if k not in state]
        if missing or ("z" not in state and "x" not in state):
            raise ValueError(f"state lacks {missing + ([] if 'z' in state or 'x' in state else ['z (or x)'])}")

        def scalar(v):
            v = v.item() if isinstance(v, np.ndarray) and v.ndim == 0 else v
            return str(v) if isinstance(v, (str, np.str_)) else v
        return cls(np.asarray(state["embedding"], dtype=np.float32), z=np.asarray(state["z"], dtype=np.float32) if "z" in state else None,
                   x=None if "z" in state else np.asarray(state["x"], dtype=np.float32), **{k: scalar(state[k]) for k in _STATE_SCALARS})

    def _on_device(self):
        """The standardised training rows and the embedding as contiguous fp32 tensors on the device, made once."""
        _need_gpu()
        if not self._standardised:
            self._z, self._standardised = neighbors.standardize(self._z, self.metric, True)[0], True
        if not (isinstance(self._z, torch.Tensor) and self._z.is_cuda and self._z.is_contiguous()):
            self._z = _tensor(self._z, torch.float32).contiguous()
        if self._y is None:
            self._y = _tensor(self.embedding, torch.float32).contiguous()
        return self._z, self._y

    # -- the transform
    def transform(self, queries, n_epochs=None, first_row: int = 0):
        """Place new rows in the fitted embedding, which does not move: fp32 [Rq, n_components] of the type of `queries`
        [Rq, columns of the fit] (umap-learn's transform).  Each query is attached to its n_neighbors nearest
        TRAINING rows (neighbors.knn(x, n_neighbors, metric, queries=queries), bit for bit), gets membership strengths with
        rho = 0 and the model's mean distance as the floor of sigma, starts at the strength-weighted mean of those rows'
        positions and then runs n_epochs epochs of the layout (None: 100 for up to 10 000 queries, else 30) at a quarter of the
        fit's learning rate, attracted to its neighbours and repelled from hashed training rows.

        A query's coordinates are a function of that row, the model, n_epochs and its row number first_row + i alone: a cohort
        transformed in chunks with first_row equals the cohort transformed at once, bit for bit (with n_epochs given: the default
        depends on the chunk's size), and adding rows to a batch moves nobody else.  A query without a usable neighbour (every
        similarity NaN) comes out NaN: this row cannot be placed.  ValueError / TypeError before the device is touched: queries
        of another column count, n_epochs outside 1 .. 2^31 - 1, a negative first_row or one with first_row + Rq > 2^32, more
        than 2^24 queries.  No queries give an empty [0, n_components]."""
        neighbors._check_matrix(queries, "queries")
        if queries.shape[1] != self.columns:
            raise ValueError(f"queries have {queries.shape[1]} columns, the model was fitted on {self.columns}")
        Rq = int(queries.shape[0])
        if Rq > QUERIES_MAX:
            raise ValueError(f"queries: at most 2^24 rows per call, not {Rq} (transform in chunks with first_row)")
        if n_epochs is None:
            n_epochs = 100 if Rq <= 10000 else 30
        n_epochs = _int_in(n_epochs, "n_epochs", 1, 2 ** 31 - 1)
        first_row = _int_in(first_row, "first_row", 0, 2 ** 32 - Rq)
        if Rq == 0:
            empty = np.zeros((0, self.n_components), dtype=np.float32)
            return empty if isinstance(queries, np.ndarray) else torch.from_numpy(empty).to(queries.device)
        z, y = self._on_device()
        m, dev = self.n_neighbors, z.device
        zq, _ = neighbors.standardize(queries, self.metric, True)
        idx = torch.empty((Rq, m), dtype=torch.int32, device=dev)
        dist = torch.empty((Rq, m), dtype=torch.float32, device=dev)
        ops.knn_dot(zq, z, m, self_offset=-1, values=dist, indices=idx, family="umap_transform")      # as neighbors.knn does it
        dist.neg_().add_(1.0)
        dist.masked_fill_(idx < 0, float("inf"))
        sigma = torch.empty(Rq, dtype=torch.float32, device=dev)
        strength = torch.empty((Rq, m), dtype=torch.float32, device=dev)
        ops.umap_smooth_knn_query(idx, dist, self.mean_dist, sigma=sigma, strength=strength, family="umap_transform")
        yq = torch.empty((Rq, self.n_components), dtype=torch.float32, device=dev)
        ops.umap_init_transform(idx, strength, y, out=yq, family="umap_transform")
        ops.umap_layout_transform(idx, transform_samples(strength, n_epochs), y, yq, epoch_begin=0, epoch_end=n_epochs, n_epochs=n_epochs,
                                  a=self.a, b=self.b, gamma=self.repulsion_strength, learning_rate=self.learning_rate,
                                  negative_sample_rate=self.negative_sample_rate, seed=self.seed, first_row=first_row,
                                  family="umap_transform")
        return neighbors._back(queries, yq)[0]


def fit(x, n_neighbors: int = 30, min_dist: float = 0.1, metric: str = "correlation", n_components: int = 2, n_epochs=None,
        init="pca", seed: int = 42, negative_sample_rate: int = 5, repulsion_strength: float = 1.0, learning_rate: float = 1.0) -> UMAPModel:
    """umap(x, ...) with the same arguments (init=spectral_init_components among them: umap hands it the rows), kept as a
    UMAPModel: model.embedding is what umap returns, bit for bit, and model.transform(queries) places new rows in it."""
    fitted = {}
    token = _FITTED.set(fitted)
    try:
        embedding = umap(x, n_neighbors=n_neighbors, min_dist=min_dist, metric=metric, n_components=n_components, n_epochs=n_epochs,
                         init=init, seed=seed, negative_sample_rate=negative_sample_rate, repulsion_strength=repulsion_strength,
                         learning_rate=learning_rate)
    finally:
        _FITTED.reset(token)
    rows, y = fitted.pop("rows"), fitted.pop("embedding")
    model = UMAPModel(embedding, x=rows, **fitted)
    model._y = y.contiguous()
    model._on_device()                                                    # the rows are on the device already: standardise them now
    return model


def transform(model: UMAPModel, queries, n_epochs=None, first_row: int = 0):
    """model.transform(queries, n_epochs, first_row) as a function."""
    if not isinstance(model, UMAPModel):
        raise TypeError(f"model must be a UMAPModel (manifold.fit returns one), not {type(model).__name__}")
    return model.transform(queries, n_epochs=n_epochs, first_row=first_row)


# ---- t-SNE with the exact gradient -----------------------------------------------------------------------------------------------------
TSNE_M_MAX = ops.TSNE_MAX_M                # VF_TSNE_MAX_M: the longest neighbour list of the perplexity search
TSNE_DIM_MAX = ops.TSNE_MAX_DIM            # VF_TSNE_MAX_DIM
TSNE_EPS = float(np.finfo(np.float64).eps)  # scikit-learn's MACHINE_EPSILON
TSNE_BLOCKS = 2048                         # blocks the all-pairs pass is cut into at least, where the rows allow: 8 per CU of 256
TSNE_SPLIT_ROWS = 64                       # a split covers at least this many rows
TSNE_PANEL_ELEMENTS = 1 << 26              # similarities the panel path of the neighbour lists holds at a time


def tsne_splits(R: int) -> int:
    """How many contiguous ranges of rows the all-pairs pass sums separately at R vertices: a function of R alone, since the
    result's bits depend on it.  With 256 vertices per block, enough splits for TSNE_BLOCKS blocks, each of at least
    TSNE_SPLIT_ROWS rows: 29 at 18 000 vertices (71 x 29 = 2059 blocks), 1 up to 64."""
    tiles = max(-(-R // 256), 1)
    return max(1, min(-(-TSNE_BLOCKS // tiles), -(-R // TSNE_SPLIT_ROWS)))


def _check_tsne_lists(indices, distances, perplexity):
    for v, name in ((indices, "indices"), (distances, "distances")):
        if not isinstance(v, (np.ndarray, torch.Tensor)):
            raise TypeError(f"{name} must be a numpy array or a torch tensor, not {type(v).__name__}")
        if v.ndim != 2:
            raise ValueError(f"{name} must be a matrix [rows, neighbours], not {tuple(v.shape)}")
    if tuple(indices.shape) != tuple(distances.shape):
        raise ValueError(f"indices {tuple(indices.shape)} and distances {tuple(distances.shape)} must have one shape")
    if not 1 <= indices.shape[1] <= TSNE_M_MAX:
        raise ValueError(f"the lists must hold 1 .. {TSNE_M_MAX} neighbours per row (the row itself not among them), not {indices.shape[1]}")
    if indices.shape[0] > 1 << 24:
        raise ValueError(f"at most 2^24 rows, not {indices.shape[0]}")
    perplexity = _number(perplexity, "perplexity", 0.0, True)
    if perplexity < 1.0 or perplexity >= indices.shape[1]:
        raise ValueError(f"perplexity must lie in 1 .. the {indices.shape[1]} neighbours of a list (below them), not {perplexity!r}")
    return perplexity


def _tsne_affinities(idx: torch.Tensor, dist: torch.Tensor, perplexity: float):
    R, m = idx.shape
    dev = idx.device
    if bool((idx >= R).any()):
        raise ValueError(f"indices must name rows below {R}")
    d2 = dist * dist                                                      # scikit-learn squares a metric that is not Euclidean
    listed = (idx >= 0) & torch.isfinite(d2)                              # the header's "present", the row itself aside
    beta = torch.empty(R, dtype=torch.float32, device=dev)
    p_cond = torch.empty((R, m), dtype=torch.float32, device=dev)
    ops.tsne_perplexity(idx, d2, perplexity, beta=beta, p_cond=p_cond, family="tsne")
    rowptr, col = _symmetric_csr(idx, listed)
    p = torch.empty(col.shape[0], dtype=torch.float32, device=dev)
    ops.tsne_joint(idx, p_cond, rowptr, col, p=p, family="tsne")
    # P /= max(sum P, eps): the sum in fp64, one fp32 division per entry (not part of vf_tsne_joint's contract)
    total = max(float(p.to(torch.float64).sum()), TSNE_EPS) if p.numel() else 1.0
    p = p / torch.tensor(total, dtype=torch.float64).to(device=dev, dtype=torch.float32)
    return rowptr, col, p, beta


def tsne_affinities(indices, distances, perplexity: float = 30.0):
    """The joint probabilities P of t-SNE over a k-NN graph: (rowptr int64 [R + 1], col int32 [nnz], p fp32 [nnz], beta fp32 [R]),
    of the type of `indices`.  indices int [R, m] and distances [R, m]: the m <= 255 OTHER rows nearest to each row and their
    METRIC distances, as neighbors.knn returns them (1 - s; -1 / +Inf where a row has fewer; a NaN or infinite distance counts
    as not there).  For a metric that is not Euclidean scikit-learn squares the metric distance before the search; so does this
    function, with one torch multiply.  Every row's beta is found by scikit-learn's binary search for the given perplexity
    (1 <= perplexity < m) on the device (ops.tsne_perplexity), p_cond is summed over the symmetric graph (ops.tsne_joint: {i, j}
    is an edge if either lists the other, stored in both directions, columns ascending, the same bits both ways) and divided
    by max(sum, eps), the sum in fp64: with m = R - 1 this is scikit-learn's dense P."""
    perplexity = _check_tsne_lists(indices, distances, perplexity)
    _need_gpu()
    out = _tsne_affinities(_tensor(indices, torch.int32).contiguous(), _tensor(distances, torch.float32).contiguous(), perplexity)
    return neighbors._back(indices, *out)


def _tsne_dof(dim: int) -> int:
    return max(dim - 1, 1)                                                # scikit-learn's degrees_of_freedom


def _tsne_run(rowptr, col, p, y, update, gains, iter_begin, iter_end, exaggeration, momentum, learning_rate, min_gain, splits):
    """Iterations [iter_begin, iter_end) in place on the contiguous device state; returns zsum fp64 [iter_end - iter_begin]."""
    R, dim = y.shape
    work = torch.empty(ops.tsne_work_bytes(R, dim, splits) // 8 + 1, dtype=torch.float64, device=y.device)
    zsum = torch.empty(iter_end - iter_begin, dtype=torch.float64, device=y.device)
    ops.tsne_descent(rowptr, col, p, y, update, gains, iter_begin=iter_begin, iter_end=iter_end, exaggeration=exaggeration,
                     momentum=momentum, learning_rate=learning_rate, min_gain=min_gain, dof=_tsne_dof(dim), splits=splits, work=work,
                     zsum=zsum, family="tsne")
    return zsum


def _check_tsne_graph(graph, y, name: str):
    _graph_members(graph)
    if not isinstance(y, (np.ndarray, torch.Tensor)):
        raise TypeError(f"{name} must be a numpy array or a torch tensor, not {type(y).__name__}")
    if y.ndim != 2 or not 1 <= y.shape[1] <= TSNE_DIM_MAX:
        raise ValueError(f"{name} must be positions [rows, 1 .. {TSNE_DIM_MAX}], not {tuple(y.shape)}")
    if graph[0].shape[0] != y.shape[0] + 1:
        raise ValueError(f"the graph has {graph[0].shape[0] - 1} rows, {name} has {y.shape[0]}")


def tsne_descent(graph, init, iter_begin: int = 0, iter_end: int = 250, exaggeration: float = 1.0, momentum: float = 0.8,
                 learning_rate: float = 200.0, min_gain: float = 0.01, state=None, return_state: bool = False, splits=None):
    """The iterations [iter_begin, iter_end) of t-SNE's gradient descent over `graph` -- what tsne_affinities returned, or its
    first three members (rowptr, col, p) -- from the positions init [R, 1 .. 4], which are not written: scikit-learn's
    _gradient_descent with its exact _kl_divergence gradient, on the device (ops.tsne_descent).  exaggeration multiplies the
    attraction (12 in the early phase), momentum and learning_rate are scikit-learn's; the degrees of freedom are
    max(dim - 1, 1).  state: None for update = 0 and gains = 1 (a fresh _gradient_descent call), or the (update, gains) of an
    earlier call.  splits: the ranges the all-pairs sum is cut into, default tsne_splits(R).  Returns fp32 [R, dim] of the type
    of init; return_state=True: (positions, update, gains, zsum) with zsum fp64 [iterations] the normaliser Z of each
    iteration.  The result depends on the arguments alone: two runs are equal bit for bit, and so is a run split at any
    iteration with its state carried over."""
    _check_tsne_graph(graph, init, "init")
    iter_begin, iter_end = _int_in(iter_begin, "iter_begin", 0, 2 ** 31 - 1), _int_in(iter_end, "iter_end", 0, 2 ** 31 - 1)
    if iter_begin > iter_end:
        raise ValueError(f"iter_begin={iter_begin} must not be above iter_end={iter_end}")
    exaggeration = _number(exaggeration, "exaggeration", 0.0, True)
    momentum = _number(momentum, "momentum", 0.0, False)
    learning_rate = _number(learning_rate, "learning_rate", 0.0, True)
    min_gain = _number(min_gain, "min_gain", 0.0, False)
    R, dim = init.shape
    splits = tsne_splits(R) if splits is None else _int_in(splits, "splits", 1, 65535)
    if state is not None:
        if not isinstance(state, (tuple, list)) or len(state) != 2 or any(
                not isinstance(s, (np.ndarray, torch.Tensor)) or tuple(s.shape) != (R, dim) for s in state):
            raise ValueError(f"state must be (update, gains), each [{R}, {dim}]")
    _need_gpu()
    rowptr, col, p = _graph_tensors(graph)
    y = _tensor(init, torch.float32).contiguous().clone()
    update = torch.zeros_like(y) if state is None else _tensor(state[0], torch.float32).contiguous().clone()
    gains = torch.ones_like(y) if state is None else _tensor(state[1], torch.float32).contiguous().clone()
    zsum = _tsne_run(rowptr, col, p, y, update, gains, iter_begin, iter_end, exaggeration, momentum, learning_rate, min_gain, splits)
    return neighbors._back(init, y, update, gains, zsum) if return_state else neighbors._back(init, y)[0]


def _tsne_kl(rowptr, col, p, y, splits: int) -> float:
    R, dim = y.shape
    if R == 0 or p.numel() == 0:
        return 0.0
    dof = _tsne_dof(dim)
    part = torch.empty((splits, R, dim + 1), dtype=torch.float32, device=y.device)
    ops.tsne_repulsion(y, dof=dof, splits=splits, part=part, family="tsne")
    z = part[:, :, dim].to(torch.float64).sum()
    rows = torch.repeat_interleave(torch.arange(R, dtype=torch.int64, device=y.device), rowptr[1:] - rowptr[:-1])
    y64 = y.to(torch.float64)
    d2 = ((y64[rows] - y64[col.to(torch.int64)]) ** 2).sum(1)
    w = (1.0 + d2 / dof) ** (-(dof + 1.0) / 2.0)
    q = torch.clamp(w / z, min=TSNE_EPS)
    p64 = p.to(torch.float64)
    return float((p64 * torch.log(torch.clamp(p64, min=TSNE_EPS) / q)).sum())


def tsne_kl(graph, y, splits=None) -> float:
    """The Kullback-Leibler divergence KL(P || Q) of the embedding y [R, 1 .. 4] over `graph` (tsne_affinities's result):
    scikit-learn's kl_divergence_ where the graph holds every pair.  Z comes from one all-pairs pass on the device
    (ops.tsne_repulsion, its column of sums added in fp64), the rest is fp64 torch over the nnz entries:
    sum_e p_e log(max(p_e, eps) / max(w_e / Z, eps)), every pair counted in both directions as P's normalisation does."""
    _check_tsne_graph(graph, y, "y")
    splits = tsne_splits(y.shape[0]) if splits is None else _int_in(splits, "splits", 1, 65535)
    _need_gpu()
    return _tsne_kl(*_graph_tensors(graph), _tensor(y, torch.float32).contiguous(), splits)


def _knn_panels(t: torch.Tensor, m: int, metric: str):
    """neighbors.knn's (indices, distances) for lists longer than its 63: ops.pairwise_dot over panels of rows and a stable torch
    sort, in vf_knn_dot's order (NaN first, descending similarity, ties to the lower column).  One-off plumbing, not a kernel
    of its own."""
    z, _ = neighbors.standardize(t, metric, nan_to_zero=False)
    R = z.shape[0]
    dev = z.device
    idx = torch.empty((R, m), dtype=torch.int32, device=dev)
    dist = torch.empty((R, m), dtype=torch.float32, device=dev)
    panel = max(1, min(R, TSNE_PANEL_ELEMENTS // max(R, 1)))
    for r0 in range(0, R, panel):
        n = min(panel, R - r0)
        s = torch.empty((n, R), dtype=torch.float32, device=dev)
        ops.pairwise_dot(z[r0:r0 + n], z, mode=0, out=s, family="tsne")
        own = torch.arange(n, device=dev)
        s[own, own + r0] = float("-inf")                                  # the row itself is no neighbour of itself
        val, order = torch.sort(s, dim=1, descending=True, stable=True)
        idx[r0:r0 + n] = order[:, :m].to(torch.int32)
        dist[r0:r0 + n] = 1.0 - val[:, :m]                                # 1 - s: the negation is exact
    return idx, dist


def tsne(x, perplexity: float = 30.0, metric: str = "correlation", n_components: int = 2, n_iter: int = 1000,
         early_exaggeration: float = 12.0, exaggeration_iter: int = 250, learning_rate="auto", init="pca", seed: int = 42,
         n_neighbors=None, return_kl: bool = False):
    """The t-SNE embedding of the rows of x [R, d] (numpy or torch) with the EXACT gradient: fp32 [R, n_components] of the type
    of x, or (embedding, KL divergence) with return_kl=True.

    The affinities are tsne_affinities of the n_neighbors nearest rows under `metric` (default min(R - 1, int(3 perplexity + 1)),
    at most 255; perplexity must stay below it): neighbors.knn up to 63 neighbours, and beyond that (the default perplexity's 91
    among them) lists built from ops.pairwise_dot row panels and a stable torch sort, in the same order.  With
    n_neighbors = R - 1 P is scikit-learn's dense P.  The descent is scikit-learn's: exaggeration_iter iterations with P
    multiplied by early_exaggeration at momentum 0.5, then the rest up to n_iter at momentum 0.8, update and gains starting
    afresh in each phase as its two _gradient_descent calls do; min_gain 0.01; learning_rate "auto" = max(R / early_exaggeration
    / 4, 50).  Every iteration sums the repulsion over ALL pairs on the device: no Barnes-Hut tree, no interpolation grid.
    init: "pca" (pca_init, d >= n_components) or "random" (random_init from `seed`), both scaled so that the first column's
    standard deviation is 1e-4 as scikit-learn scales its PCA start (a start whose first coordinate has no finite spread, as
    identical rows give under "pca", is refused with a ValueError where scikit-learn would divide by zero); an array [R, n_components], taken as it is; or a callable
    f(graph, n_components, seed) -> positions as in umap, taken as it is.
    Differences from scikit-learn, deliberate: the iteration count is fixed (its early stopping on the error's
    progress and the gradient norm is left out), the arithmetic is fp32 with stated summation orders (its is fp64), and P is
    sparse unless n_neighbors = R - 1.  The result is a function of the arguments, bit for bit."""
    neighbors._check_matrix(x, "x")
    if metric not in neighbors.METRICS:
        raise ValueError(f"metric must be one of {neighbors.METRICS}, not {metric!r}")
    n_components = _int_in(n_components, "n_components", 1, TSNE_DIM_MAX)
    R = x.shape[0]
    if R < 3 or R > 1 << 24:
        raise ValueError(f"x must hold 3 .. 2^24 rows, not {R}")
    perplexity = _number(perplexity, "perplexity", 0.0, True)
    if n_neighbors is None:
        n_neighbors = min(R - 1, int(3.0 * perplexity + 1.0))
    n_neighbors = _int_in(n_neighbors, "n_neighbors", 2, min(R - 1, TSNE_M_MAX))
    if perplexity < 1.0 or perplexity >= n_neighbors:
        raise ValueError(f"perplexity must lie in 1 .. n_neighbors={n_neighbors} (below it), not {perplexity!r}")
    n_iter = _int_in(n_iter, "n_iter", 0, 2 ** 31 - 1)
    exaggeration_iter = _int_in(exaggeration_iter, "exaggeration_iter", 0, 2 ** 31 - 1)
    early_exaggeration = _number(early_exaggeration, "early_exaggeration", 0.0, True)
    if isinstance(learning_rate, str):
        if learning_rate != "auto":
            raise ValueError(f"learning_rate must be 'auto' or a positive number, not {learning_rate!r}")
        learning_rate = max(R / early_exaggeration / 4.0, 50.0)
    learning_rate = _number(learning_rate, "learning_rate", 0.0, True)
    seed = _int_in(seed, "seed", 0, 2 ** 32 - 1)
    if isinstance(init, str):
        if init not in INITS:
            raise ValueError(f"init must be one of {INITS}, an array [rows, n_components] or a callable, not {init!r}")
        if init == "pca" and x.shape[1] < n_components:
            raise ValueError(f"init='pca' needs at least n_components={n_components} columns, x has {x.shape[1]}")
    elif callable(init):
        pass                                                              # its result is checked when it has been called
    elif not isinstance(init, (np.ndarray, torch.Tensor)) or tuple(init.shape) != (R, n_components):
        raise ValueError(f"init must be one of {INITS}, a callable or an array [{R}, {n_components}]")
    t = neighbors._to_device(x, True)
    y = None
    if isinstance(init, str):                                             # before the graph: a start without spread is refused early
        y = pca_init(t, n_components) if init == "pca" else random_init(R, n_components, seed, t.device)
        spread = float(y[:, 0].std(unbiased=False))
        if not (np.isfinite(spread) and spread > 0.0):
            raise ValueError(f"init={init!r}: the start's first coordinate has no finite spread (standard deviation {spread!r}; identical "
                             "or non-finite rows?), so it cannot be scaled to 1e-4: pass init='random' or an array")
        y = y / spread * 1e-4
    if n_neighbors <= N_NEIGHBORS_MAX - 1:
        idx, dist = neighbors.knn(t, k=n_neighbors, metric=metric)
    else:
        idx, dist = _knn_panels(t, n_neighbors, metric)
    rowptr, col, p, _ = _tsne_affinities(idx, dist, perplexity)
    if callable(init):
        y = _tensor(_called_init(init, (rowptr, col, p), R, n_components, seed), torch.float32)
    elif y is None:
        y = _tensor(init, torch.float32)
    y = y.contiguous().clone()
    splits = tsne_splits(R)
    early = min(exaggeration_iter, n_iter)
    for begin, end, exaggeration, momentum in ((0, early, early_exaggeration, 0.5), (early, n_iter, 1.0, 0.8)):
        if end > begin:
            _tsne_run(rowptr, col, p, y, torch.zeros_like(y), torch.ones_like(y), begin, end, exaggeration, momentum, learning_rate,
                      0.01, splits)
    if return_kl:
        return neighbors._back(x, y)[0], _tsne_kl(rowptr, col, p, y, splits)
    return neighbors._back(x, y)[0]

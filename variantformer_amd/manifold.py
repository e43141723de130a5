"""UMAP on the device: what vcf2embed's umap.UMAP(n_neighbors=30, min_dist=0.05, metric='correlation').fit_transform does over
~18 000 genes x 49 tissues, and what the same picture needs over the registry-token embeddings.

  find_ab(min_dist, spread)        the a, b of the curve 1 / (1 + a x^(2b)) that umap-learn fits with scipy, in plain numpy;
  fuzzy_graph(indices, distances)  the fuzzy simplicial set of a k-NN graph: (rowptr, col, w, rho, sigma);
  layout(graph, init, n_epochs, a, b, ...)   the SGD epochs over that graph from the positions `init`;
  umap(x, ...)                     neighbors.knn, fuzzy_graph, an initialisation and layout, on the device throughout.

Three entries of include/vf_hip_umap.h do the work: ops.umap_smooth_knn (rho, sigma, directed strengths),
ops.umap_union (the fuzzy union over the symmetric graph, whose CSR arrays are built here with torch: index plumbing) and
ops.umap_layout (all epochs of a call from one loop inside the library).  The layout is a gather: a vertex reads the others where
they stood when the epoch began and writes only its own row, so a run has one result, bit for bit, whatever the hardware does,
and can be split at any epoch.  Two deliberate differences from umap-learn follow from that and are stated in DESIGN.md 5h: others
are read at epoch-start positions (umap-learn reads and writes them concurrently), and every drawn edge gets exactly
negative_sample_rate repulsions (umap-learn keeps a float schedule).  Spectral initialisation is out of scope (it needs a sparse
eigensolver): init is "pca", "random" or an array.  transform() of new points is out of scope too.  There is no CPU path: without
a GPU the calls raise, after their arguments have been checked.  scipy, umap-learn, numba and pynndescent are not imported.
"""
from __future__ import annotations

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
def _fuzzy_graph(idx: torch.Tensor, dist: torch.Tensor):
    R, m = idx.shape
    dev = idx.device
    listed = (idx >= 0) & torch.isfinite(dist)                          # the header's "present"
    if bool((idx >= R).any()):
        raise ValueError(f"indices must name rows below {R}")
    mean_dist = float(dist[listed].to(torch.float64).mean()) if bool(listed.any()) else 0.0
    rho = torch.empty(R, dtype=torch.float32, device=dev)
    sigma = torch.empty(R, dtype=torch.float32, device=dev)
    strength = torch.empty((R, m), dtype=torch.float32, device=dev)
    ops.umap_smooth_knn(idx, dist, mean_dist, rho=rho, sigma=sigma, strength=strength, family="umap")
    # the symmetric graph in CSR: every listed pair in both directions, once, columns ascending within a row; a row that lists
    # itself makes no edge
    rows = torch.arange(R, dtype=torch.int64, device=dev)[:, None].expand(R, m)
    edge = listed & (idx != rows)
    i, j = rows[edge], idx[edge].to(torch.int64)
    keys = torch.unique(torch.cat((i * R + j, j * R + i)))             # sorted
    row = torch.div(keys, R, rounding_mode="floor")
    col = (keys - row * R).to(torch.int32)
    rowptr = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    if R:
        rowptr[1:] = torch.cumsum(torch.bincount(row, minlength=R), 0)
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


# ---- the whole ---------------------------------------------------------------------------------------------------------------------
def umap(x, n_neighbors: int = 30, min_dist: float = 0.1, metric: str = "correlation", n_components: int = 2, n_epochs=None,
         init="pca", seed: int = 42, negative_sample_rate: int = 5, repulsion_strength: float = 1.0, learning_rate: float = 1.0):
    """The UMAP embedding of the rows of x [R, d] (numpy or torch): fp32 [R, n_components] of the type of x.

    n_neighbors 2 .. 64 counts the row itself as umap-learn does: the graph is neighbors.knn(x, n_neighbors - 1, metric).
    min_dist 0 .. 1 gives the curve through find_ab (spread 1).  n_epochs None: 500 for R <= 10000, else 200.  init: "pca"
    (d >= n_components), "random" (counter-based from `seed`) or an array [R, n_components]; every init is rescaled per coordinate
    to [0, 10] and no noise is added.  Spectral initialisation is out of scope (it needs a sparse eigensolver), and so is
    transform() of new points.  seed also fixes the negative samples: the result is a function of the arguments, bit for bit.
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
        if init not in INITS:
            raise ValueError(f"init must be one of {INITS} or an array [rows, n_components], not {init!r}")
        if init == "pca" and x.shape[1] < n_components:
            raise ValueError(f"init='pca' needs at least n_components={n_components} columns, x has {x.shape[1]}")
    elif not isinstance(init, (np.ndarray, torch.Tensor)) or tuple(init.shape) != (R, n_components):
        raise ValueError(f"init must be one of {INITS} or an array [{R}, {n_components}]")
    a, b = find_ab(min_dist)
    n_epochs, a, b, gamma, learning_rate, negative_sample_rate, seed = _check_layout_args(
        n_epochs, a, b, repulsion_strength, learning_rate, negative_sample_rate, seed)
    t = neighbors._to_device(x, True)
    idx, dist = neighbors.knn(t, k=n_neighbors - 1, metric=metric)
    rowptr, col, w, _, _ = _fuzzy_graph(idx, dist)
    if isinstance(init, str):
        y = pca_init(t, n_components) if init == "pca" else random_init(R, n_components, seed, t.device)
    else:
        y = _tensor(init, torch.float32)
    y = _layout(rowptr, col, w, rescale(y).contiguous(), n_epochs, a, b, gamma, learning_rate, negative_sample_rate, seed)
    return neighbors._back(x, y)[0]

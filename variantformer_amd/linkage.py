"""Hierarchical clustering on the device: Ward linkage of a distance matrix, the step vcf2exp's compute_ordered_leaves hands to
scipy.cluster.hierarchy.linkage(squareform(1 - corrcoef), method="ward") -- once over the ~54 tissues for the dendrogram, once
over the ~18 000 genes for the row order of the heatmap.

  ward(D)            Z in scipy's format from a square distance matrix (its upper triangle), numpy or torch;
  ward_of_rows(x)    neighbors.correlation_distance(x) followed by ward, on the device throughout;
  leaves_list(Z)     the left-to-right leaf order of Z, as scipy.cluster.hierarchy.leaves_list;
  cut(Z, n_clusters) the flat clusters of Z, the partition of scipy.cluster.hierarchy.cut_tree, on the host.

Ward is a reducible linkage: every pair of mutually nearest clusters belongs to the final tree, so all such pairs merge at once.
A round is two entries of include/vf_hip_linkage.h: ops.linkage_nearest finds every row's nearest row,
ops.linkage_contract writes the Lance-Williams distances between the merged clusters into the other of two working matrices;
between them a few torch calls pick the mutual pairs and compact the slots, with one scalar read back per round.  A tree over
n rows takes a few dozen rounds, not n - 1 dependent steps.  Every fp32 operation is individually rounded, so
tests/linkage_cases.py restates the algorithm in numpy bit for bit.  On tied distances the result is a valid linkage but may be
another, equally valid tree than scipy's.  Peak device memory: the caller's matrix plus two working copies, 12 n^2 bytes.  There
is no CPU path: without a GPU the calls raise, after their arguments have been checked.  scipy is not imported.
"""
from __future__ import annotations

import numpy as np
import torch

from . import neighbors, ops


def _check_square(D):
    if not isinstance(D, (np.ndarray, torch.Tensor)):
        raise TypeError(f"D must be a numpy array or a torch tensor, not {type(D).__name__}")
    if D.ndim != 2 or D.shape[0] != D.shape[1]:
        raise ValueError(f"D must be a square distance matrix, not {tuple(D.shape)}")
    if D.shape[0] < 2:
        raise ValueError(f"D must hold at least 2 observations, not {D.shape[0]}")


_NOT_FINITE = "the distance matrix must contain only finite values (its upper triangle is what is used)"


def ward(D, check_finite: bool = True, return_info: bool = False):
    """Ward linkage of the square distance matrix D [n, n], n >= 2: a numpy array, or a torch tensor (fp32 on the device is used
    where it lies, with any row stride, and is never written).  Only the upper triangle is read, as by squareform.  Returns Z,
    float64 numpy [n - 1, 4] in scipy's format: the two ids of a row ascending, rows sorted by height, the cluster made by row
    i has id n + i, the last column its size.  Heights are fp32 values: the Lance-Williams update in individually rounded fp32
    (include/vf_hip_linkage.h), a parent never below its children.  Non-finite input raises ValueError as scipy does, unless
    check_finite=False.  return_info=True returns (Z, {"rounds": the rounds the tree took})."""
    _check_square(D)
    n = D.shape[0]
    on_device = isinstance(D, torch.Tensor) and D.is_cuda
    if not on_device:
        host = D.detach().numpy() if isinstance(D, torch.Tensor) else D
        host = np.ascontiguousarray(host, dtype=np.float32)
        if check_finite and not np.isfinite(host[np.triu_indices(n, 1)]).all():
            raise ValueError(_NOT_FINITE)
        if not torch.cuda.is_available():
            raise ops._lib.VFError("variantformer_amd.linkage needs a GPU (no CPU fallback)")
        D = torch.from_numpy(host).cuda()
    elif D.dtype != torch.float32 or D.stride(1) != 1:
        D = D.to(torch.float32).contiguous()
    dev = D.device
    work = [torch.empty(n * n, dtype=torch.float32, device=dev) for _ in range(2)]

    def matrix(k, m):
        return work[k][:m * m].view(m, m)
    arange = torch.arange(n + 1, dtype=torch.int64, device=dev)
    nn_val = torch.empty(n, dtype=torch.float32, device=dev)
    nn_idx = torch.empty(n, dtype=torch.int32, device=dev)
    sizes = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
    pair_dist = torch.empty(n, dtype=torch.float32, device=dev)
    slots = torch.empty((2, n + 1), dtype=torch.int32, device=dev)     # first, second of a round; column m_out takes what is dropped
    # the merge records in creation order; row n - 1 takes the writes of the slots that did not merge
    rec_left = torch.empty(n, dtype=torch.int64, device=dev)
    rec_right = torch.empty(n, dtype=torch.int64, device=dev)
    rec_height = torch.empty(n, dtype=torch.float32, device=dev)
    rec_size = torch.empty(n, dtype=torch.int32, device=dev)

    # round 0 merges nothing: the symmetric working copy out of the caller's upper triangle
    ones = torch.ones(n, dtype=torch.int32, device=dev)
    alone = torch.full((n,), -1, dtype=torch.int32, device=dev)
    cur = 0
    ops.linkage_contract(D, ones, arange[:n].to(torch.int32), alone, upper_only=True, out=matrix(cur, n), size_out=sizes[cur],
                         pair_dist=pair_dist, family="linkage")
    if on_device and check_finite:
        lo, hi = torch.aminmax(matrix(cur, n))                          # a NaN comes out of both; no n x n temporary, as isfinite would make
        if not bool(torch.isfinite(lo) & torch.isfinite(hi)):
            raise ValueError(_NOT_FINITE)
    node = arange[:n].clone()                                           # the tree node every slot stands for: leaves first
    height = torch.zeros(n, dtype=torch.float32, device=dev)
    m, made, rounds = n, 0, 0
    while m > 1:
        W = matrix(cur, m)
        ops.linkage_nearest(W, nn_val=nn_val[:m], nn_idx=nn_idx[:m], family="linkage")
        ar = arange[:m]
        nn = nn_idx[:m].to(torch.int64)
        mutual = nn[nn] == ar
        lower, upper = mutual & (ar < nn), mutual & (ar > nn)
        pos = torch.cumsum(~upper, 0) - 1                               # a pair takes the place of its lower slot, order preserved
        m_out = int(pos[-1]) + 1                                        # the round's one read-back
        if not m_out < m:
            raise RuntimeError(f"Ward linkage made no progress at {m} clusters (round {rounds}): no mutually nearest pair")
        target = torch.where(upper, m_out, pos)
        slots[0].scatter_(0, target, ar.to(torch.int32))
        slots[1].scatter_(0, target, torch.where(lower, nn, -1).to(torch.int32))
        first, second = slots[0, :m_out], slots[1, :m_out]
        ops.linkage_contract(W, sizes[cur][:m], first, second, out=matrix(1 - cur, m_out), size_out=sizes[1 - cur][:m_out],
                             pair_dist=pair_dist[:m_out], family="linkage")
        # the round's merge records, in order of the lower slot
        f, s = first.to(torch.int64), second.to(torch.int64).clamp(min=0)
        merged = second >= 0
        h = torch.maximum(pair_dist[:m_out], torch.maximum(height[f], height[s]))      # monotone under rounding
        k = made + torch.cumsum(merged, 0) - 1
        row = torch.where(merged, k, n - 1)
        rec_left.scatter_(0, row, node[f])
        rec_right.scatter_(0, row, node[s])
        rec_height.scatter_(0, row, h)
        rec_size.scatter_(0, row, sizes[1 - cur][:m_out])
        node = torch.where(merged, n + k, node[f])
        height = torch.where(merged, h, height[f])
        made += m - m_out
        m, cur, rounds = m_out, 1 - cur, rounds + 1
    assert made == n - 1
    Z = _to_scipy(torch.stack((rec_left[:n - 1], rec_right[:n - 1]), 1).cpu().numpy(), rec_height[:n - 1].cpu().numpy(), rec_size[:n - 1].cpu().numpy(), n)
    return (Z, {"rounds": rounds}) if return_info else Z


def _to_scipy(child: np.ndarray, height: np.ndarray, size: np.ndarray, n: int) -> np.ndarray:
    """Merge records in creation order (children made before their parents, node n + k made by record k) to scipy's Z: a stable
    sort by height -- which keeps children before parents, a parent being no lower -- and the relabelling that goes with it."""
    order = np.argsort(height, kind="stable")
    new_id = np.arange(2 * n - 1, dtype=np.int64)
    new_id[n + order] = n + np.arange(n - 1)
    ids = np.sort(new_id[child[order]], axis=1)
    Z = np.empty((n - 1, 4), dtype=np.float64)
    Z[:, :2] = ids
    Z[:, 2] = height[order]
    Z[:, 3] = size[order]
    return Z


def ward_of_rows(x, nan_to_zero: bool = True, return_info: bool = False):
    """ward(neighbors.correlation_distance(x)) without leaving the device: x [R >= 2, d] numpy or torch, NaN -> 0 first as the
    notebooks' np.nan_to_num does.  A constant row is at distance 1 from every row (numpy has NaN there); a row with an Inf
    makes its distances NaN, which raises ValueError."""
    neighbors._check_matrix(x, "x")
    if x.shape[0] < 2:
        raise ValueError(f"x must hold at least 2 rows, not {x.shape[0]}")
    D = neighbors.correlation_distance(neighbors._to_device(x, nan_to_zero), nan_to_zero=False)
    return ward(D, return_info=return_info)


def leaves_list(Z) -> np.ndarray:
    """The leaves of the tree Z from left to right, int32 [n]: scipy.cluster.hierarchy.leaves_list in plain numpy (the first
    id of a row is its left child)."""
    Z = np.asarray(Z)
    if Z.ndim != 2 or Z.shape[1] != 4 or Z.shape[0] < 1:
        raise ValueError(f"Z must be a linkage matrix [n - 1, 4], not {tuple(Z.shape)}")
    n = Z.shape[0] + 1
    children = Z[:, :2].astype(np.int64)
    if children.min() < 0 or (children >= n + np.arange(n - 1)[:, None]).any():
        raise ValueError("Z is no linkage: a row names a cluster that is not made before it")
    if (np.bincount(children.ravel(), minlength=2 * n - 2) != 1).any():
        raise ValueError("Z is no linkage: every leaf and every cluster but the last is merged exactly once")
    out = np.empty(n, dtype=np.int32)
    filled = 0
    stack = [2 * n - 2]
    while stack:
        node = stack.pop()
        if node < n:
            out[filled] = node
            filled += 1
        else:
            left, right = children[node - n]
            stack.append(int(right))
            stack.append(int(left))
    return out


def cut(Z, n_clusters) -> np.ndarray:
    """The flat clusters of the tree Z: the partition of scipy.cluster.hierarchy.cut_tree(Z, n_clusters=...) for a monotone Z (a
    parent never below its children, which ward returns), on the host in plain numpy.  n_clusters: an integer in 1 .. rows, or
    a list of them.  The first rows - n_clusters merges of Z are applied; the clusters are numbered 0, 1, .. by their lowest
    row.  Returns int32 [rows], or [rows, len(n_clusters)] for a list: the step between ward / ward_of_rows and labels."""
    Z = np.asarray(Z)
    if Z.ndim != 2 or Z.shape[1] != 4 or Z.shape[0] < 1:
        raise ValueError(f"Z must be a linkage matrix [n - 1, 4], not {tuple(Z.shape)}")
    n = Z.shape[0] + 1
    children = Z[:, :2].astype(np.int64)
    if children.min() < 0 or (children >= n + np.arange(n - 1)[:, None]).any():
        raise ValueError("Z is no linkage: a row names a cluster that is not made before it")
    if (np.bincount(children.ravel(), minlength=2 * n - 2) != 1).any():
        raise ValueError("Z is no linkage: every leaf and every cluster but the last is merged exactly once")
    if (np.diff(Z[:, 2]) < 0).any():
        raise ValueError("Z is not monotone: its heights must not fall from one row to the next")
    many = isinstance(n_clusters, (list, tuple, np.ndarray))
    wanted = list(n_clusters) if many else [n_clusters]
    if many and not wanted:
        raise ValueError("n_clusters must name at least one number of clusters")
    for c in wanted:
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 1 <= c <= n:
            raise ValueError(f"n_clusters must be an integer in 1 .. {n}, not {c!r}")
    out = np.empty((n, len(wanted)), dtype=np.int32)
    for col, c in enumerate(wanted):
        parent = np.arange(2 * n - 1, dtype=np.int64)
        done = n - int(c)                                                # the merges applied
        parent[children[:done].ravel()] = np.repeat(n + np.arange(done), 2)
        while True:                                                       # pointer doubling: every node to the top of its tree
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
        root = parent[:n]
        _, first, inverse = np.unique(root, return_index=True, return_inverse=True)
        rank = np.empty(first.shape[0], dtype=np.int32)
        rank[np.argsort(first, kind="stable")] = np.arange(first.shape[0], dtype=np.int32)
        out[:, col] = rank[inverse.reshape(-1)]
    return out if many else out[:, 0]

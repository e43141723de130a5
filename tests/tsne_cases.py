"""References and the case table of the t-SNE entries (include/vf_hip_tsne.h): numpy restatements of every stage, each in two
precisions -- fp64, and INDIVIDUALLY ROUNDED fp32 in the device's stated summation orders -- beside the scikit-learn functions
they restate (sklearn.manifold._utils._binary_search_perplexity, _t_sne._joint_probabilities, _kl_divergence, _gradient_descent).

How the non-exact quantities are bounded (the probabilities, the forces, twenty iterations of positions): for every case the
YARDSTICK is the deviation of the fp32 restatement from the fp64 one on that case, both computed on the CPU; the device may
deviate from the fp64 restatement by FACTOR times the yardstick, and a case whose yardstick is 0 must be met exactly.  numpy's
fp32 exp / log / sqrt and its correctly rounded division stand where the device has its own exp / log / sqrt and a 1-ulp
reciprocal: that is what the factor covers.  FACTOR was chosen on the first run on the GPU and is at most 8; the device
deviations measured then are recorded beside it (MEASURED).

The perplexity search is a bisection, so its trajectory is not continuous in its sums: a sum that differs in its last bit can
take the other branch and end at another beta within the tolerance.  The probabilities are therefore compared AT THE BETA A
SEARCH ENDED AT (device P against the fp64 P of the device's beta; yardstick: fp32 P against the fp64 P of the fp32 search's
beta), and beta itself is held by its equation: the fp64 entropy at the returned beta is within the search's tolerance of the
target, plus FACTOR times the fp32 restatement's own entropy deviation."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
EPS = float(np.finfo(np.float64).eps)      # scikit-learn's MACHINE_EPSILON
STEPS, TOL = 100, 1e-5                     # VF_TSNE_PERPLEXITY_STEPS, VF_TSNE_PERPLEXITY_TOL
MAX_M, MAX_DIM, Z_BLOCKS, Z_THREADS, TILE = 255, 4, 64, 256, 256

# The multiple of the yardstick the device is allowed (at most 8), chosen on the first GPU run: the largest device deviation
# over yardstick measured then, per quantity, is recorded below (tests/test_tsne_gpu.py prints them again on every run).  The
# worst is 1.87, on a force; positions and Z came out AT the yardstick, i.e. at the fp32 restatement's own value.  A device whose
# exp, log, sqrt and reciprocal are each 1 ulp where numpy's are 0.5 can at most double an individually rounded deviation, so
# the factor is 4: twice what was seen, half of what was allowed.
FACTOR = 4.0
MEASURED = {"p_cond": 1.51, "entropy": 0.57, "repulsion": 1.87, "positions": 1.00, "zsum": 1.00}


# ---- the perplexity search -----------------------------------------------------------------------------------------------------------
def present(idx, d2):
    return (idx >= 0) & np.isfinite(d2) & (idx != np.arange(idx.shape[0])[:, None])


def lane_sum(v):
    """Row sums of v [R, m] in the device's order: entry t on lane t mod 64, each lane adds its entries in ascending t, then a
    butterfly over the lanes (xor 32 .. 1).  In v's dtype."""
    R, m = v.shape
    pad = np.zeros((R, 4 * 64), dtype=v.dtype)
    pad[:, :m] = v
    q = pad.reshape(R, 4, 64)
    a = ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        a = a + a[:, lanes ^ off]
    return a[:, 0]


def shifted(idx, d2, dtype):
    """(x = d2 - the row's smallest present d2, 0 where not present; present)."""
    pres = present(idx, d2)
    dmin = np.where(pres, d2, np.inf).astype(F32).min(1)
    dmin = np.where(pres.any(1), dmin, 0).astype(F32)
    with np.errstate(invalid="ignore"):
        x = np.where(pres, d2.astype(dtype) - dmin.astype(dtype)[:, None], 0).astype(dtype)
    return x, pres


def evaluate(x, pres, beta, dtype):
    """(P, S, H) at the given betas: e = exp(-(x beta)), S = sum e, P = e / S, H = log S + beta sum x P, in dtype."""
    beta = beta.astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = np.where(pres, np.exp(-(x * beta[:, None])), 0).astype(dtype)
        S = lane_sum(e)
        P = (e / S[:, None]).astype(dtype)
        D = lane_sum((x * P).astype(dtype))
        H = (np.log(S) + beta * D).astype(dtype)
    return P, S, H


def perplexity_search(idx, d2, perplexity, dtype=F64, target=None):
    """The header's search in `dtype`: (beta, P, converged).  target: log(perplexity), by default the fp32 nearest to it as the
    device takes it."""
    R, m = idx.shape
    x, pres = shifted(idx, d2, dtype)
    target = dtype(F32(np.log(F64(perplexity)))) if target is None else dtype(target)
    tol = dtype(F32(TOL))
    beta = np.ones(R, dtype=dtype)
    lo, hi = np.full(R, -np.inf, dtype=dtype), np.full(R, np.inf, dtype=dtype)
    active = pres.any(1)
    P = np.zeros((R, m), dtype=dtype)
    for step in range(STEPS):
        if not active.any():
            break
        Pn, _, H = evaluate(x, pres, beta, dtype)
        P[active] = Pn[active]
        diff = (H - target).astype(dtype)
        active = active & ~(np.abs(diff) <= tol)
        if step == STEPS - 1:
            break
        up, down = active & (diff > 0), active & ~(diff > 0)
        lo[up] = beta[up]
        hi[down] = beta[down]
        with np.errstate(invalid="ignore", over="ignore"):
            nxt_up = np.where(np.isinf(hi), beta * dtype(2), (beta + hi) / dtype(2)).astype(dtype)
            nxt_down = np.where(np.isinf(lo), beta / dtype(2), (beta + lo) / dtype(2)).astype(dtype)
        beta = np.where(up, nxt_up, np.where(down, nxt_down, beta)).astype(dtype)
    converged = pres.any(1) & ~active
    beta[~pres.any(1)] = 0
    return beta, np.where(pres, P, 0).astype(dtype), converged


def perplexity_case(kind: str, R: int, m: int, seed: int = 0):
    """(idx int32 [R, m], d2 fp32 [R, m]) of one kind: random squared distances; absent entries (-1, NaN, +Inf, -Inf) in every
    lane class; rows that list themselves; a row of duplicates (all 0), a row of equal distances."""
    rng = np.random.default_rng(1000 * R + m + seed)
    idx = np.stack([rng.permutation(max(R + m, 2 * m))[:m] for _ in range(R)]).astype(np.int32)
    d2 = np.sort(rng.random((R, m), dtype=F32) * F32(2.0), axis=1).astype(F32) ** 2
    if kind == "random":
        return idx, d2
    if kind == "absent":
        for i in range(R):
            for k, t in enumerate(range(i % 3, m, 3)):                     # every third entry: lanes and lane classes alike
                if k % 4 == 0:
                    idx[i, t] = -1
                else:
                    d2[i, t] = (np.nan, np.inf, -np.inf)[k % 4 - 1]
        if R > 1:
            idx[R - 1], d2[R - 1] = -1, np.inf                             # a row with nothing present
        return idx, d2
    if kind == "self":
        for i in range(R):
            idx[i, i % m] = i
            d2[i, i % m] = 0
        return idx, d2
    if kind == "flat":
        d2[0] = 0                                                         # duplicates
        if R > 1:
            d2[1] = F32(0.37)                                             # equal distances
        return idx, d2
    raise ValueError(kind)


PERPLEXITY_KINDS = ("random", "absent", "self", "flat")
PERPLEXITY_MS = (1, 2, 63, 64, 65, 128, 255)
PERPLEXITY_RS = (1, 3, 65)


def perplexity_of(m: int) -> float:
    """A perplexity valid for lists of m: m = 1 admits none (perplexity >= 1 and < m), so the case is its refusal."""
    return float(min(max(m / 3.0, 1.0), 30.0))


# ---- the symmetric graph ---------------------------------------------------------------------------------------------------------------
def csr(idx, d2):
    """(rowptr int64 [R + 1], col int32 [nnz]): every listed pair in both directions, once, columns ascending."""
    R = idx.shape[0]
    pres = present(idx, d2)
    i, j = np.nonzero(pres)[0], idx[pres].astype(np.int64)
    keys = np.unique(np.concatenate((i * R + j, j * R + i))) if i.size else np.zeros(0, dtype=np.int64)
    row = keys // max(R, 1)
    rowptr = np.zeros(R + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(row, minlength=R))
    return rowptr, (keys - row * R).astype(np.int32)


def joint(idx, p_cond, rowptr, col):
    """p[e] = a + b in p_cond's dtype: the first match of j in row i's list, of i in row j's, +0 without one."""
    R, m = idx.shape
    p = np.zeros(col.shape[0], dtype=p_cond.dtype)

    def first(row, other):
        hit = np.flatnonzero(idx[row] == other)
        return p_cond[row, hit[0]] if hit.size else p_cond.dtype.type(0)
    for i in range(R):
        for e in range(rowptr[i], rowptr[i + 1]):
            j = col[e]
            p[e] = first(i, j) + (first(j, i) if 0 <= j < R else 0)
    return p


def normalised(p, dtype):
    """P / max(sum P, eps): the sum in fp64, one division per entry in dtype."""
    total = max(float(p.astype(F64).sum()), EPS)
    return (p.astype(dtype) / dtype(total)).astype(dtype)


def dense(rowptr, col, p):
    R = rowptr.shape[0] - 1
    out = np.zeros((R, R), dtype=p.dtype)
    out[np.repeat(np.arange(R), np.diff(rowptr)), col] = p
    return out


def full_lists(D2):
    """(idx int32 [R, R - 1], d2 fp32 [R, R - 1]): every other row, ascending by squared distance (stable), from a dense matrix."""
    R = D2.shape[0]
    masked = D2.astype(F64).copy()
    np.fill_diagonal(masked, np.inf)
    order = np.argsort(masked, axis=1, kind="stable")[:, :R - 1]
    return order.astype(np.int32), np.take_along_axis(D2.astype(F32), order, 1)


# ---- the forces ------------------------------------------------------------------------------------------------------------------------
def split_range(R: int, splits: int, s: int):
    L = -(-R // splits)
    return min(s * L, R), min((s + 1) * L, R)


def weight(d2, dof: int, dtype):
    """w = t^((dof + 1) / 2) with t = 1 / (1 + q), q = d2, d2 * 0.5, d2 * fl(1 / 3): the header's forms, in dtype."""
    third = dtype(F32(1.0) / F32(3.0)) if dtype is F32 else dtype(1.0) / dtype(3.0)
    q = d2 if dof == 1 else ((d2 * dtype(0.5)) if dof == 2 else (d2 * third))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = (dtype(1) / (dtype(1) + q.astype(dtype))).astype(dtype)
        return t if dof == 1 else ((t * np.sqrt(t)).astype(dtype) if dof == 2 else (t * t).astype(dtype))


def sq_dist(a, b, dtype):
    """(differences, sum of their squares over c ascending from +0), in dtype."""
    with np.errstate(invalid="ignore", over="ignore"):
        diff = (a.astype(dtype) - b.astype(dtype)).astype(dtype)
        d2 = np.zeros(diff.shape[:-1], dtype=dtype)
        for c in range(diff.shape[-1]):
            d2 = (d2 + (diff[..., c] * diff[..., c]).astype(dtype)).astype(dtype)
    return diff, d2


def repulsion(Y, dof: int, splits: int, dtype=F64):
    """part [splits, R, dim + 1] in dtype: for vertex i and split s one running sum over j ascending in the split's range,
    j == i skipped by index."""
    R, dim = Y.shape
    Y = Y.astype(dtype)
    part = np.zeros((splits, R, dim + 1), dtype=dtype)
    rows = np.arange(R)
    for s in range(splits):
        lo, hi = split_range(R, splits, s)
        for j in range(lo, hi):
            diff, d2 = sq_dist(Y, Y[j][None, :], dtype)
            w = weight(d2, dof, dtype)
            with np.errstate(invalid="ignore", over="ignore"):
                ww = (w * w).astype(dtype)
                new = part[s].copy()
                new[:, :dim] = (part[s][:, :dim] + (ww[:, None] * diff).astype(dtype)).astype(dtype)
                new[:, dim] = (part[s][:, dim] + w).astype(dtype)
            keep = rows == j
            part[s] = np.where(keep[:, None], part[s], new)
    return part


def attraction(rowptr, col, p, Y, dof: int, dtype=F64):
    """attr [R, dim] in dtype: the CSR row in entry order, one running sum of (p w) (y_i - y_j)."""
    R, dim = Y.shape
    Y = Y.astype(dtype)
    attr = np.zeros((R, dim), dtype=dtype)
    deg = np.diff(rowptr)
    for k in range(int(deg.max()) if R else 0):
        rows = np.flatnonzero(deg > k)
        e = rowptr[rows] + k
        j = col[e]
        ok = (j >= 0) & (j < R)
        rows, e, j = rows[ok], e[ok], j[ok]
        diff, d2 = sq_dist(Y[rows], Y[j], dtype)
        w = weight(d2, dof, dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            pw = (p[e].astype(dtype) * w).astype(dtype)
            attr[rows] = (attr[rows] + (pw[:, None] * diff).astype(dtype)).astype(dtype)
    return attr


def z_sum(part) -> float:
    """Z in fp64 in the device's order: chunks of C consecutive k = s R + i, thread u adds k = b C + u, + 256, ..; a tree; the
    chunks in ascending b."""
    v = part[:, :, -1].astype(F64).ravel()
    total = v.shape[0]
    C = -(-total // Z_BLOCKS)
    Z = 0.0
    for b in range(Z_BLOCKS):
        chunk = v[b * C:min((b + 1) * C, total)]
        x = np.zeros(Z_THREADS, dtype=F64)
        for u0 in range(0, chunk.shape[0], Z_THREADS):
            seg = chunk[u0:u0 + Z_THREADS]
            x[:seg.shape[0]] += seg
        stride = Z_THREADS // 2
        while stride:
            x[:stride] += x[stride:2 * stride]
            stride //= 2
        Z += x[0]
    return float(Z)


def descent(rowptr, col, p, Y, update, gains, iters: int, exaggeration, momentum, learning_rate, min_gain, splits: int, dtype=F64):
    """`iters` iterations of the header's step 1 .. 4 in dtype (Z always in fp64): (Y, update, gains, zsum fp64 [iters])."""
    R, dim = Y.shape
    dof = max(dim - 1, 1)
    Y, update, gains = Y.astype(dtype).copy(), update.astype(dtype).copy(), gains.astype(dtype).copy()
    G = dtype(2.0 * (dof + 1) / dof)
    ex, mo, lr, mg = dtype(exaggeration), dtype(momentum), dtype(learning_rate), dtype(min_gain)
    zs = np.zeros(iters, dtype=F64)
    for n in range(iters):
        part = repulsion(Y, dof, splits, dtype)
        attr = attraction(rowptr, col, p, Y, dof, dtype)
        Z = z_sum(part)
        zs[n] = Z
        rep = np.zeros((R, dim), dtype=dtype)
        for s in range(splits):
            rep = (rep + part[s][:, :dim]).astype(dtype)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            grad = (G * ((ex * attr).astype(dtype) - (rep / dtype(Z)).astype(dtype)).astype(dtype)).astype(dtype)
            inc = (update * grad).astype(dtype) < 0
            gains = np.where(inc, (gains + dtype(0.2)).astype(dtype), (gains * dtype(0.8)).astype(dtype))
            gains = np.where(gains < mg, mg, gains).astype(dtype)
            grad = (grad * gains).astype(dtype)
            update = ((mo * update).astype(dtype) - (lr * grad).astype(dtype)).astype(dtype)
            Y = (Y + update).astype(dtype)
    return Y, update, gains, zs


def gradient(rowptr, col, p, Y, exaggeration=1.0, splits: int = 1, dtype=F64):
    """The gradient the update sees, before the gains: G (exaggeration attr - rep / Z)."""
    R, dim = Y.shape
    dof = max(dim - 1, 1)
    part = repulsion(Y, dof, splits, dtype)
    attr = attraction(rowptr, col, p, Y, dof, dtype)
    rep = part[:, :, :dim].sum(0)
    return dtype(2.0 * (dof + 1) / dof) * (dtype(exaggeration) * attr - rep / dtype(z_sum(part)))


def kl(rowptr, col, p, Y) -> float:
    """KL(P || Q) in fp64 over the entries: sum p log(max(p, eps) / max(w / Z, eps)), as manifold.tsne_kl."""
    R, dim = Y.shape
    dof = max(dim - 1, 1)
    Y = Y.astype(F64)
    D2 = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    W = (1.0 + D2 / dof) ** (-(dof + 1.0) / 2.0)
    np.fill_diagonal(W, 0.0)
    rows = np.repeat(np.arange(R), np.diff(rowptr))
    q = np.maximum(W[rows, col] / W.sum(), EPS)
    p = p.astype(F64)
    return float((p * np.log(np.maximum(p, EPS) / q)).sum())


# The learning rate of the twenty-step comparisons.  scikit-learn's "auto" would be 50 at these few rows; at 12x exaggeration
# that oscillates, every inc / dec decision near update * grad = 0 is a discontinuity, and twenty steps then multiply a rounding
# difference by 1e5 .. 1e7 (measured on the CPU: the fp32 restatement ends O(1) from the fp64 one, and a yardstick of O(1) holds
# nothing).  At 2 the same steps keep a deviation near the rounding that made it (fp32 from fp64 by 3e-7 of the span), and
# they still take both branches of the gains.
STEPS_LEARNING_RATE = 2.0


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------
def embedding(R: int, dim: int, seed: int = 0, scale: float = 1.0):
    return (np.random.default_rng(77 * R + dim + seed).standard_normal((R, dim)) * scale).astype(F32)


def small_graph(R: int, m: int, seed: int = 0):
    """(idx, d2, rowptr, col, p fp32 normalised) of random lists at perplexity perplexity_of(m): the graph of the descent cases."""
    idx, d2 = perplexity_case("random", R, m, seed)
    idx = (idx % R).astype(np.int32)
    _, p_cond, _ = perplexity_search(idx, d2, perplexity_of(m), F32)
    rowptr, col = csr(idx, d2)
    return idx, d2, rowptr, col, normalised(joint(idx, p_cond, rowptr, col), F32)


def clusters(R: int, d: int = 24, groups: int = 4, noise: float = 0.8, seed: int = 5):
    """(x fp32 [R, d], labels [R]): `groups` distinct random profiles plus noise, rows interleaved.  The noise was chosen on the
    CPU references alone: at 0.35 the three end at one KL to three digits (a gap g of 0.1 %), at 1.2 none of them keeps every
    row's 5 nearest in its group; at 0.8 all three do, with KLs of 0.120 .. 0.135 that differ by 1 .. 1.5 %."""
    rng = np.random.default_rng(seed)
    profiles = rng.standard_normal((groups, d))
    labels = np.arange(R) % groups
    return (profiles[labels] + noise * rng.standard_normal((R, d))).astype(F32), labels


# name -> (R, perplexity, m): m = R - 1, so the sparse P is scikit-learn's dense P
FIXTURES = {"A": (64, 21.0, 63), "B": (128, 42.0, 127)}
N_ITER, EXAGGERATION_ITER, EARLY_EXAGGERATION, NEAREST = 1000, 250, 12.0, 5


def correlation_distance(x):
    z = x.astype(F64) - x.astype(F64).mean(1, keepdims=True)
    z /= np.sqrt((z * z).sum(1, keepdims=True))
    D = 1.0 - z @ z.T
    np.fill_diagonal(D, 0.0)
    return np.maximum(D, 0.0)


def fixture_init(R: int, dim: int = 2):
    y = np.random.default_rng(R).standard_normal((R, dim))
    return (y / y[:, 0].std() * 1e-4).astype(F32)


def nearest_in_group(Y, labels, k: int = NEAREST) -> bool:
    """Condition (a): every row's k nearest rows in the embedding belong to its own group."""
    Y = np.asarray(Y, dtype=F64)
    D2 = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(D2, np.inf)
    near = np.argsort(D2, axis=1, kind="stable")[:, :k]
    return bool((labels[near] == labels[:, None]).all())


def descent_dense(P, Y, iters: int, exaggeration, momentum, learning_rate, min_gain, dtype):
    """descent() from update = 0, gains = 1 over a dense P, every operation in dtype but the sums in numpy's own order: a thousand
    iterations in a fraction of a second.  For the end-to-end references alone: trajectories are chaotic, no coordinate of
    theirs is compared, so the order of a sum is not what they pin."""
    R, dim = Y.shape
    dof = max(dim - 1, 1)
    Y, P = Y.astype(dtype).copy(), P.astype(dtype)
    update, gains = np.zeros_like(Y), np.ones_like(Y)
    G = dtype(2.0 * (dof + 1) / dof)
    ex, mo, lr, mg = dtype(exaggeration), dtype(momentum), dtype(learning_rate), dtype(min_gain)
    for _ in range(iters):
        diff = Y[:, None, :] - Y[None, :, :]
        W = weight((diff * diff).sum(-1, dtype=dtype), dof, dtype)
        np.fill_diagonal(W, 0)
        Z = dtype(W.astype(F64).sum())
        attr = ((P * W)[:, :, None] * diff).sum(1, dtype=dtype)
        rep = ((W * W)[:, :, None] * diff).sum(1, dtype=dtype)
        grad = G * (ex * attr - rep / Z)
        inc = update * grad < 0
        gains = np.where(inc, gains + dtype(0.2), gains * dtype(0.8))
        gains = np.where(gains < mg, mg, gains).astype(dtype)
        update = (mo * update - lr * (grad * gains)).astype(dtype)
        Y = (Y + update).astype(dtype)
    return Y


def run_restatement(rowptr, col, p, init, R: int, dtype):
    """manifold.tsne's two phases on the CPU: scikit-learn's schedule, update and gains afresh in each."""
    lr = max(R / EARLY_EXAGGERATION / 4.0, 50.0)
    P = dense(rowptr, col, p)
    y = descent_dense(P, init, EXAGGERATION_ITER, EARLY_EXAGGERATION, 0.5, lr, 0.01, dtype)
    return descent_dense(P, y, N_ITER - EXAGGERATION_ITER, 1.0, 0.8, lr, 0.01, dtype)


@functools.lru_cache(maxsize=None)
def fixture_references(name: str):
    """The three CPU references of a fixture from one init: scikit-learn's TSNE(method="exact", metric="precomputed") on the
    1 - corr matrix, the fp64 restatement and the fp32 one.  Returns a dict: x, labels, init, graph = (rowptr, col, p fp32),
    embeddings {name: Y} and kl {name: KL}; the KL of every embedding is taken over the same fp64 P by kl()."""
    from sklearn.manifold import TSNE
    R, perplexity, m = FIXTURES[name]
    x, labels = clusters(R)
    D = correlation_distance(x)
    init = fixture_init(R)
    idx, d2 = full_lists((D * D).astype(F32))
    out = {"x": x, "labels": labels, "init": init}
    emb = {}
    sk = TSNE(n_components=2, perplexity=perplexity, early_exaggeration=EARLY_EXAGGERATION, learning_rate="auto", max_iter=N_ITER,
              n_iter_without_progress=N_ITER, min_grad_norm=0.0, metric="precomputed", init=init.astype(F64), method="exact")
    emb["sklearn"] = sk.fit_transform(D.copy())                           # it squares a metric that is not Euclidean, in place
    graphs = {}
    for dtype, key in ((F64, "fp64"), (F32, "fp32")):
        _, p_cond, _ = perplexity_search(idx, d2, perplexity, dtype)
        rowptr, col = csr(idx, d2)
        p = normalised(joint(idx, p_cond, rowptr, col), dtype)
        graphs[key] = (rowptr, col, p)
        emb[key] = run_restatement(rowptr, col, p, init, R, dtype)
    out["graph"] = graphs["fp32"]
    out["embeddings"] = emb
    out["kl"] = {k: kl(*graphs["fp64"], v) for k, v in emb.items()}
    out["kl_sklearn_own"] = float(sk.kl_divergence_)
    return out

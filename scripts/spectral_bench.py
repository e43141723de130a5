"""What the spectral initialisation of UMAP costs on the device, at the two shapes of scripts/umap_bench.py and one more:

    18000 x 49      genes x tissues with n_neighbors=30, min_dist=0.05, 200 epochs: the call of the reference's vcf2embed notebook;
    262144 x 64     synthetic rows, the same arguments;
    18000 x 49      points on a 20:1 strip carried into 49 dimensions (not a shape of umap_bench.py): a graph whose Laplacian has
                    small eigengaps, where the solver needs more than two filters and a host eigensolver seconds.

Per shape, one process, on the fuzzy graph manifold.umap builds:

    components      manifold._components (torch: min-label propagation with pointer jumping): wall time and the count;
    degree          ops.graph_degree: wall time;
    solver          manifold._spectral with spectral_init's arguments (block 16, degree 40, tol 1e-4): wall time over several
                    passes, outer iterations, sparse block products, residuals; and from one further pass under ops.KernelTimer
                    (HIP events on the launch stream) the kernels' own times: the filter calls of ops.spmm_recur (degree steps
                    under one pair of events) with their achieved bytes/s against the bytes the algorithm needs (per step every
                    entry's column, weight and neighbour scale, a row of p values gathered per entry, the block read twice and
                    written once), the one-step products, ops.tall_gram and ops.tall_mul; the rest of the solver's wall time is
                    the host's: the p x p eigenproblems, the read-backs of the Gram matrices, torch's elementwise work;
    umap            manifold.umap end to end with init="pca" and with init=manifold.spectral_init: wall time, and scikit-learn's
                    trustworthiness (correlation distance, 30 neighbours) of both layouts on a fixed sample of 4000 rows: reported,
                    not asserted;
    eigsh           scipy.sparse.linalg.eigsh on the same normalised adjacency on the host, once (only at 18000 rows), with
                    1 - |cos| between its vectors and the device's.

A graph of more than one component has no spectral start (spectral_init falls back to the random one): the count is recorded
and the solver's entries are left out.  Wall times are a host clock around a synchronised window.  One JSON line, also written
to profiles/spectral_bench.json.

    python scripts/spectral_bench.py [--rounds 3] [--warmup 1] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from scripts.umap_bench import MIN_DIST, N_EPOCHS, N_NEIGHBORS, SHAPES, rows_of  # noqa: E402

BLOCK, DEGREE, TOL, MAX_ITER, SEED, DIM = 16, 40, 1e-4, 50, 42, 2
TRUST_ROWS, EIGSH_ROWS = 4000, 20000


def strip_rows(rows: int, d: int) -> np.ndarray:
    """Points on a 20:1 strip carried into d dimensions by two random directions, with a little noise."""
    g = np.random.default_rng(rows + d + 1)
    u, v = g.uniform(0, 20, rows), g.uniform(0, 1, rows)
    a, b = g.standard_normal(d), g.standard_normal(d)
    return (np.outer(u, a) + np.outer(v, b) + 5.0 * g.standard_normal(d)[None, :] + 0.01 * g.standard_normal((rows, d))).astype(np.float32)


CASES = tuple(("expression-like", rows, d, rows_of) for rows, d in SHAPES) + (("strip 20:1", 18000, 49, strip_rows),)


def trust(x: np.ndarray, y: np.ndarray) -> float:
    from sklearn.manifold import trustworthiness
    pick = np.random.default_rng(7).choice(x.shape[0], min(TRUST_ROWS, x.shape[0]), replace=False)
    return float(trustworthiness(x[pick].astype(np.float64), y[pick].astype(np.float64), n_neighbors=N_NEIGHBORS, metric="correlation"))


def host_eigsh(rowptr, col, w, ours: np.ndarray):
    from scipy.sparse import csr_matrix, diags
    from scipy.sparse.linalg import eigsh
    R = rowptr.shape[0] - 1
    A = csr_matrix((w.astype(np.float64), col, rowptr), shape=(R, R))
    d = 1.0 / np.sqrt(np.asarray(A.sum(1)).ravel())
    S = diags(d) @ A @ diags(d)
    t0 = time.perf_counter()
    lam, vec = eigsh(S, k=ours.shape[1] + 1, which="LA")
    seconds = time.perf_counter() - t0
    vec = vec[:, np.argsort(-lam)][:, 1:]
    cos = np.abs((vec * ours.astype(np.float64)).sum(0)) / np.linalg.norm(vec, axis=0) / np.linalg.norm(ours.astype(np.float64), axis=0)
    return {"seconds": round(seconds, 3), "eigenvalues_of_L": [float(v) for v in 1.0 - np.sort(lam)[::-1]], "one_minus_abs_cos": [float(v) for v in 1.0 - cos]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "spectral_bench.json"))
    args = ap.parse_args()

    import bench
    from variantformer_amd import _lib, manifold, neighbors, ops
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("spectral_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def mean(values):
        return round(sum(values) / len(values), 3)

    shapes = []
    for kind, rows, d, make in CASES:
        x_host = make(rows, d)
        x = torch.from_numpy(x_host).to(dev)
        idx, dist = neighbors.knn(x, k=N_NEIGHBORS - 1)
        rowptr, col, w = manifold._fuzzy_graph(idx, dist)[:3]
        entry = {"data": kind, "rows": rows, "d": d, "n_neighbors": N_NEIGHBORS, "entries": int(col.shape[0]), "block": BLOCK, "filter_degree": DEGREE, "tol": TOL}
        for _ in range(args.warmup):
            manifold._components(rowptr, col, w)
            manifold._degrees(rowptr, col, w)
        comp = [timed(lambda: manifold._components(rowptr, col, w)) for _ in range(args.rounds)]
        count = comp[0][0][1]
        degs = [timed(lambda: manifold._degrees(rowptr, col, w)) for _ in range(args.rounds)]
        deg, dinv = degs[0][0]
        entry["components"] = {"count": int(count), "wall_ms": [round(ms, 3) for _, ms in comp], "mean_ms": mean([ms for _, ms in comp])}
        entry["degree"] = {"wall_ms": [round(ms, 3) for _, ms in degs], "mean_ms": mean([ms for _, ms in degs])}
        connected = count == 1 and bool((deg > 0).all())
        if connected:
            def solve():
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)
                    return manifold._spectral(rowptr, col, w, deg, dinv, DIM, BLOCK, DEGREE, TOL, MAX_ITER, SEED)
            for _ in range(args.warmup):
                solve()
            passes = [timed(solve) for _ in range(args.rounds)]
            (y, info), _ = passes[0]
            ops.TIMER = ops.KernelTimer(detail=True)
            try:
                _, timer_wall = timed(solve)
                summ = ops.TIMER.summary()
            finally:
                ops.TIMER = None
            p = min(BLOCK, rows)
            filt = [v for k, v in summ.items() if k.startswith("spmm_recur[") and f"steps={DEGREE}" in k]
            ones = [v for k, v in summ.items() if k.startswith("spmm_recur[") and "steps=1" in k.split(" ")[-1]]
            filter_ms, filter_bytes = sum(v["total_ms"] for v in filt), sum(v["bytes"] for v in filt)
            kernels_ms = sum(summ[n]["total_ms"] for n in ("spmm_recur", "tall_gram", "tall_mul") if n in summ)
            wall = mean([ms for _, ms in passes])
            entry["solver"] = {
                "wall_ms": [round(ms, 3) for _, ms in passes], "mean_ms": wall, "iterations": int(info["iterations"]), "products": int(info["products"]),
                "converged": bool(info["converged"]), "residuals": [float(v) for v in info["residuals"]],
                "eigenvalues_of_L": [float(v) for v in info["eigenvalues"]], "block_columns": p,
                "filter": {"calls": sum(v["launches"] for v in filt), "steps_per_call": DEGREE, "total_ms": round(filter_ms, 4),
                           "ms_per_step": round(filter_ms / max(sum(v["launches"] for v in filt) * DEGREE, 1), 5),
                           "algorithmic_bytes": filter_bytes, "achieved_GBps": round(filter_bytes / max(filter_ms, 1e-9) / 1e6, 1)},
                "one_step_products": {"calls": sum(v["launches"] for v in ones), "total_ms": round(sum(v["total_ms"] for v in ones), 4)},
                "gram": {"calls": summ["tall_gram"]["launches"], "total_ms": round(summ["tall_gram"]["total_ms"], 4)},
                "tall_mul": {"calls": summ["tall_mul"]["launches"], "total_ms": round(summ["tall_mul"]["total_ms"], 4)},
                "kernels_ms": round(kernels_ms, 4), "timed_pass_wall_ms": round(timer_wall, 3),
                "host_rayleigh_ritz_and_readbacks_ms": round(timer_wall - kernels_ms, 3)}
            entry["spectral_init_mean_ms"] = round(entry["components"]["mean_ms"] + entry["degree"]["mean_ms"] + wall, 3)
            if rows <= EIGSH_ROWS:
                entry["host_eigsh"] = host_eigsh(rowptr.cpu().numpy(), col.cpu().numpy(), w.cpu().numpy(), y.cpu().numpy())
        else:
            entry["solver"] = None
        kw = dict(n_neighbors=N_NEIGHBORS, min_dist=MIN_DIST, n_epochs=N_EPOCHS)
        umap = {}
        for name, init in (("pca", "pca"), ("spectral_init", manifold.spectral_init)):
            def run():
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)
                    return manifold.umap(x, init=init, **kw)
            for _ in range(args.warmup):
                run()
            runs = [timed(run) for _ in range(args.rounds)]
            layout = runs[0][0].cpu().numpy()
            umap[name] = {"wall_ms": [round(ms, 3) for _, ms in runs], "mean_ms": mean([ms for _, ms in runs]),
                          "trustworthiness": round(trust(x_host, layout), 4), "finite": bool(np.isfinite(layout).all())}
        umap["spectral_init_fell_back_to_random"] = not connected
        entry["umap"] = umap
        shapes.append(entry)
        print(json.dumps(entry), file=sys.stderr, flush=True)
        del x, rowptr, col, w
        torch.cuda.empty_cache()
    result = {"rounds": args.rounds, "warmup": args.warmup, "shapes": shapes,
              "note": "wall_ms: host clock around a synchronised window; solver kernels: HIP events around each entry of one further pass "
                      "(a filter call's 40 launches under one pair of events); achieved_GBps is algorithmic bytes over kernel time, "
                      "not a share of peak: the gathered rows are re-read from cache; trustworthiness on a fixed sample of "
                      f"{TRUST_ROWS} rows, reported, not asserted; host_eigsh ran once, on the CPU of the machine that holds the GPU",
              "source_sha": bench.source_sha()}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

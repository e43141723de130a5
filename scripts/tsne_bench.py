"""What t-SNE with the exact gradient costs on the device, at two shapes:

    18000 x 49      genes x tissues at perplexity 30 (91 neighbours), 1000 iterations: the notebook's matrix;
    65536 x 64      synthetic rows, the same arguments: 4.3e9 pair terms per iteration.

Per shape, one process, stage by stage as manifold.tsne runs them (init="pca"):

    knn63       neighbors.knn(x, 63): the k-NN kernel at its longest list, wall time (what a perplexity up to 20 uses);
    panels91    the lists of 91 from ops.pairwise_dot row panels and a stable torch sort: wall time.  One-off plumbing;
    affinities  manifold._tsne_affinities: wall time, the two kernels' own times (ops.KernelTimer: HIP events on the launch
                stream) and the rest, which is the torch plumbing of the CSR arrays and the normalisation;
    repulsion   ops.tsne_repulsion alone, 50 calls back to back under one pair of events: time per all-pairs pass and the pair
                terms per second, beside the 0.1 ms that had been estimated for 18 000 rows before anyone measured;
    iteration   ops.tsne_descent over 250 iterations under one pair of events, workspace allocated before: time per iteration;
    kernels     the four kernels of an iteration apart -- repulsion, attraction, the fp64 sum of Z, update -- as their average
                duration in a rocprofv3 --kernel-trace --stats run of its own: a child process that runs nothing but the
                stages up to the graph and 260 iterations (`--descent-only`).  launch_gaps_ms is what an iteration takes
                beyond their sum; it has come out within 0.02 ms of zero, either side: the two are taken in different
                processes, and the host enqueues ahead of the device;
    whole       manifold.tsne end to end, wall time, and its KL divergence.

Then the host, clearly apart and under a time limit each, in child processes that do not touch the GPU: scikit-learn's
Barnes-Hut TSNE at 18000 x 49 (its default method; metric="correlation", 1000 iterations) and its exact method at 2000 x 49 with
500 iterations (250 of them after the exaggeration phase), against the device at those same 2000 rows and 500 iterations.
Wall times are a host clock around a synchronised window.  One JSON line, also written to profiles/tsne_bench.json.

    python scripts/tsne_bench.py [--rounds 3] [--warmup 1] [--host-limit 300] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPES = ((18000, 49), (65536, 64))
PERPLEXITY, N_ITER, EXAGGERATION_ITER = 30.0, 1000, 250
EXACT_ROWS, EXACT_ITER = 2000, 500
ESTIMATE_MS = 0.1                          # the issue's estimate of one all-pairs pass at 18 000 rows, nobody had measured it

HOST_CHILD = r"""
import json, sys, time
import numpy as np
sys.path.insert(0, {repo!r})
from scripts.tsne_bench import rows_of
from sklearn.manifold import TSNE
x = rows_of({rows}, {d})
t0 = time.perf_counter()
model = TSNE(n_components=2, perplexity={perplexity}, metric="correlation", method={method!r}, max_iter={iters}, init="pca", random_state=0)
model.fit_transform(x)
print(json.dumps({{"seconds": round(time.perf_counter() - t0, 2), "kl": float(model.kl_divergence_), "n_iter": int(model.n_iter_)}}))
"""


def rows_of(rows: int, d: int) -> np.ndarray:
    """Expression-like rows: a mix of a dozen programmes plus noise, so that the graph has clusters and hubs."""
    g = np.random.default_rng(rows + d)
    programme = g.standard_normal((12, d))
    return (g.standard_normal((rows, 12)) @ programme + 0.5 * g.standard_normal((rows, d)) + 5.0).astype(np.float32)


def host_run(rows: int, d: int, method: str, iters: int, limit: float) -> dict:
    """scikit-learn's TSNE in a child process without the GPU, ended at the limit."""
    code = HOST_CHILD.format(repo=REPO, rows=rows, d=d, perplexity=PERPLEXITY, method=method, iters=iters)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    what = {"rows": rows, "d": d, "method": method, "max_iter": iters, "limit_s": limit}
    try:
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=limit, env=env)
    except subprocess.TimeoutExpired:
        return dict(what, result=f"not finished within {limit:g} s")
    if r.returncode != 0:
        return dict(what, result="failed: " + r.stderr.strip().splitlines()[-1][:200])
    return dict(what, **json.loads(r.stdout.strip().splitlines()[-1]))


TRACED = {"repulsion": "tsne_repulsion_kernel", "attraction": "tsne_attraction_kernel", "z": "tsne_z_kernel", "update": "tsne_update_kernel"}


def descent_only(rows: int, d: int):
    """What the kernel trace watches: the graph of one shape, then 10 + 250 iterations of the early phase, and nothing else."""
    from variantformer_amd import _lib, manifold, ops
    _lib.load()
    x = torch.from_numpy(rows_of(rows, d)).cuda()
    idx, dist = manifold._knn_panels(x, min(rows - 1, int(3 * PERPLEXITY + 1)), "correlation")
    rowptr, col, p, _ = manifold._tsne_affinities(idx, dist, PERPLEXITY)
    y = manifold.pca_init(x, 2)
    y = (y / y[:, 0].std(unbiased=False) * 1e-4).contiguous()
    update, gains = torch.zeros_like(y), torch.ones_like(y)
    splits = manifold.tsne_splits(rows)
    work = torch.empty(ops.tsne_work_bytes(rows, 2, splits) // 8 + 1, dtype=torch.float64, device=y.device)
    lr = max(rows / 12.0 / 4.0, 50.0)
    for begin, end in ((0, 10), (10, 10 + EXAGGERATION_ITER)):
        zsum = torch.empty(end - begin, dtype=torch.float64, device=y.device)
        ops.tsne_descent(rowptr, col, p, y, update, gains, iter_begin=begin, iter_end=end, exaggeration=12.0, momentum=0.5, learning_rate=lr,
                         dof=1, splits=splits, work=work, zsum=zsum)
    torch.cuda.synchronize()


def kernel_trace(rows: int, d: int, limit: float) -> dict:
    """Average duration of each of an iteration's kernels, ms, from rocprofv3's kernel statistics of a `--descent-only` child."""
    import csv
    import glob
    import shutil
    import tempfile
    tool = shutil.which("rocprofv3")
    if tool is None:
        return {"result": "not measured: no rocprofv3 on this machine"}
    out = tempfile.mkdtemp(prefix="tsne_trace_")
    try:
        cmd = [tool, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--descent-only", str(rows), str(d)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            return {"result": f"not measured: the traced run did not finish within {limit:g} s"}
        files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return {"result": f"not measured: the traced run ended with {r.returncode} and {len(files)} statistics files"}
        found = {}
        with open(files[0], newline="") as f:
            for row in csv.DictReader(f):
                for key, name in TRACED.items():
                    if name in row["Name"]:
                        found[key] = {"calls": int(row["Calls"]), "average_ms": round(float(row["AverageNs"]) * 1e-6, 5)}
        if set(found) != set(TRACED):
            return {"result": f"not measured: the statistics name only {sorted(found)}"}
        found["sum_ms"] = round(sum(v["average_ms"] for v in found.values()), 5)
        return found
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--descent-only", nargs=2, type=int, metavar=("ROWS", "D"), help="run only what the kernel trace watches, and leave")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-limit", type=float, default=300.0)
    ap.add_argument("--shapes", type=int, default=len(SHAPES), help="how many of the shapes to run")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tsne_bench.json"))
    args = ap.parse_args()

    if not torch.cuda.is_available():
        raise SystemExit("tsne_bench.py measures on the GPU: none found")
    if args.descent_only:
        return descent_only(*args.descent_only)
    import bench
    from variantformer_amd import _lib, manifold, neighbors, ops
    _lib.load()
    traces = {rows: kernel_trace(rows, d, args.host_limit) for rows, d in SHAPES[:args.shapes]}      # runs of their own, before this one
    print(json.dumps(traces), file=sys.stderr, flush=True)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def stages(x, with_timer):
        ms = {}
        R = x.shape[0]
        m = min(R - 1, int(3 * PERPLEXITY + 1))
        _, ms["knn63"] = timed(lambda: neighbors.knn(x, k=63))
        (idx, dist), ms["panels91"] = timed(lambda: manifold._knn_panels(x, m, "correlation"))
        ops.TIMER = ops.KernelTimer() if with_timer else None
        try:
            graph, ms["affinities"] = timed(lambda: manifold._tsne_affinities(idx, dist, PERPLEXITY))
            summ = ops.TIMER.summary() if with_timer else None
        finally:
            ops.TIMER = None
        rowptr, col, p, _ = graph
        y0, ms["init"] = timed(lambda: manifold.pca_init(x, 2))
        y0 = (y0 / y0[:, 0].std(unbiased=False) * 1e-4).contiguous()
        splits = manifold.tsne_splits(R)
        part = torch.empty((splits, R, 3), dtype=torch.float32, device=dev)
        passes = 50
        ms["repulsion_pass"] = events(lambda: [ops.tsne_repulsion(y0, dof=1, splits=splits, part=part) for _ in range(passes)]) / passes
        y, update, gains = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)
        lr = max(R / 12.0 / 4.0, 50.0)
        work = torch.empty(ops.tsne_work_bytes(R, 2, splits) // 8 + 1, dtype=torch.float64, device=dev)
        zsum = torch.empty(EXAGGERATION_ITER, dtype=torch.float64, device=dev)
        ms["iteration"] = events(lambda: ops.tsne_descent(rowptr, col, p, y, update, gains, iter_begin=0, iter_end=EXAGGERATION_ITER,
                                                          exaggeration=12.0, momentum=0.5, learning_rate=lr, dof=1, splits=splits,
                                                          work=work, zsum=zsum)) / EXAGGERATION_ITER
        # a spread-out embedding costs what a tight one costs: the pass has no data-dependent branch; the iteration is timed on
        # the early phase it really runs
        (emb, kl), ms["whole"] = timed(lambda: manifold.tsne(x, perplexity=PERPLEXITY, n_iter=N_ITER, return_kl=True))
        return ms, graph, emb, kl, summ, splits

    shapes = []
    for rows, d in SHAPES[:args.shapes]:
        x = torch.from_numpy(rows_of(rows, d)).to(dev)
        for _ in range(args.warmup):
            stages(x, False)
        runs = [stages(x, False)[0] for _ in range(args.rounds)]
        _, graph, emb, kl, summ, splits = stages(x, True)
        rowptr, col, p, beta = graph
        length = torch.diff(rowptr)
        kernels = {name: {"launches": summ[name]["launches"], "total_ms": round(summ[name]["total_ms"], 4)} for name in ("tsne_perplexity", "tsne_joint")}
        mean = {k: round(sum(r[k] for r in runs) / len(runs), 4) for k in runs[0]}
        pairs = float(rows) * (rows - 1)
        kernel_ms = kernels["tsne_perplexity"]["total_ms"] + kernels["tsne_joint"]["total_ms"]
        entry = {"rows": rows, "d": d, "perplexity": PERPLEXITY, "n_neighbors": min(rows - 1, int(3 * PERPLEXITY + 1)),
                 "n_iter": N_ITER, "splits": splits,
                 "wall_ms": {"passes": [{k: round(v, 4) for k, v in r.items()} for r in runs], "mean": mean},
                 "affinity_kernels_ms": round(kernel_ms, 4), "affinity_torch_plumbing_ms": round(mean["affinities"] - kernel_ms, 3),
                 "kernels": kernels,
                 "repulsion": {"ms_per_pass": mean["repulsion_pass"], "pair_terms": pairs, "pair_terms_per_s": round(pairs / (mean["repulsion_pass"] * 1e-3), 1),
                               "estimate_before_ms": ESTIMATE_MS if rows == 18000 else None},
                 "iteration": {"ms": mean["iteration"], "kernels": traces[rows],
                               "launch_gaps_ms": round(mean["iteration"] - traces[rows]["sum_ms"], 4) if "sum_ms" in traces[rows] else None},
                 "csr": {"entries": int(col.shape[0]), "mean_row": round(float(length.double().mean()), 2), "largest_row": int(length.max())},
                 "beta": {"min": float(beta.min()), "max": float(beta.max())}, "kl": round(kl, 5), "finite": bool(torch.isfinite(emb).all())}
        shapes.append(entry)
        print(json.dumps(entry), file=sys.stderr, flush=True)
        del x, graph, emb
        torch.cuda.empty_cache()

    # the host, apart: scikit-learn in child processes, and the device at the exact method's size
    xs = torch.from_numpy(rows_of(EXACT_ROWS, 49)).to(dev)
    manifold.tsne(xs, perplexity=PERPLEXITY, n_iter=EXACT_ITER)
    (_, kl_small), small_ms = timed(lambda: manifold.tsne(xs, perplexity=PERPLEXITY, n_iter=EXACT_ITER, return_kl=True))
    host = {"barnes_hut_18000": host_run(18000, 49, "barnes_hut", N_ITER, args.host_limit),
            "exact_2000": host_run(EXACT_ROWS, 49, "exact", EXACT_ITER, args.host_limit),
            "device_2000": {"rows": EXACT_ROWS, "d": 49, "n_iter": EXACT_ITER, "seconds": round(small_ms / 1e3, 4), "kl": round(kl_small, 5)},
            "note": "scikit-learn on this host's CPUs, one child process each, ended at limit_s; Barnes-Hut approximates the gradient, "
                    "the device computes it exactly; scikit-learn may stop early, n_iter says where"}
    print(json.dumps(host), file=sys.stderr, flush=True)
    result = {"rounds": args.rounds, "warmup": args.warmup, "shapes": shapes, "host": host,
              "note": "wall_ms: host clock around a synchronised window per stage of manifold.tsne (init='pca'); kernels: HIP events around "
                      "each entry of one further pass; repulsion_pass and iteration: one pair of events around 50 passes / 250 iterations; "
                      "iteration.kernels: average kernel durations from rocprofv3 --kernel-trace --stats over a child process of its own",
              "source_sha": bench.source_sha()}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

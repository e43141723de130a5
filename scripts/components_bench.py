"""What the component search and the per-component spectral start cost on the device.

Part 1, on the three fuzzy graphs of scripts/spectral_bench.py (18000 x 49 and 262144 x 64 expression-like rows, the 18000 x 49
strip), one process:

    torch           manifold._components_torch, the search as torch index plumbing (the code before the kernels): wall time;
    kernels         manifold._components over ops.graph_components_rounds: wall time, the batches (one scalar read back each) and
                    rounds run, the rounds the graph needs (single rounds until one changes nothing, that one counted), and
                    from one further pass under ops.KernelTimer (HIP events on the launch stream, a batch's launches under
                    one pair) the kernels' own time per round; both searches' labels are compared.

Part 2, on rows made of several separated clusters (18000 x 49 in 12 clusters, 262144 x 64 in 16), on the fuzzy graph
manifold.umap builds:

    components      the count found;
    init            manifold.spectral_init_components whole: wall time; from one further pass the kernels' own times of
                    ops.csr_components (permute) and ops.segment_mean_gather (centroids), and the host loop over the components
                    (every manifold._spectral call inside a synchronised host clock: its sum, the calls, their outer iterations
                    and how many converged);
    umap            manifold.umap end to end with init=manifold.spectral_init_components and with init=manifold.spectral_init,
                    which falls back to the random start on these graphs: wall time.

Wall times are a host clock around a synchronised window.  One JSON line, also written to profiles/components_bench.json.

    python scripts/components_bench.py [--rounds 3] [--warmup 1] [--part 1|2|both] [--out FILE]
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

from scripts.spectral_bench import CASES  # noqa: E402
from scripts.umap_bench import MIN_DIST, N_EPOCHS, N_NEIGHBORS  # noqa: E402

SEED, DIM = 42, 2
CLUSTERED = ((18000, 49, 12), (262144, 64, 16))


def clustered_rows(rows: int, d: int, n_clusters: int) -> np.ndarray:
    """rows x d in n_clusters separated clusters of equal size: a random centre each and a tenth of its scale as noise."""
    g = np.random.default_rng(rows + d + n_clusters)
    centre = g.standard_normal((n_clusters, d))
    return (centre[np.arange(rows) % n_clusters] + 0.1 * g.standard_normal((rows, d))).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--part", default="both", choices=("1", "2", "both"))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "components_bench.json"))
    args = ap.parse_args()

    import bench
    from variantformer_amd import _lib, manifold, neighbors, ops
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("components_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def walls(fn):
        for _ in range(args.warmup):
            fn()
        runs = [timed(fn) for _ in range(args.rounds)]
        ms = [round(t, 3) for _, t in runs]
        return runs[0][0], {"wall_ms": ms, "mean_ms": round(sum(ms) / len(ms), 3)}

    def under_timer(fn):
        ops.TIMER = ops.KernelTimer(detail=False)
        try:
            out, wall = timed(fn)
            return out, wall, ops.TIMER.summary()
        finally:
            ops.TIMER = None

    def graph_of(x):
        idx, dist = neighbors.knn(x, k=N_NEIGHBORS - 1)
        return manifold._fuzzy_graph(idx, dist)[:3]

    result = {"rounds": args.rounds, "warmup": args.warmup, "component_rounds_per_batch": manifold.COMPONENT_ROUNDS}
    if args.part in ("1", "both"):
        search = []
        for kind, rows, d, make in CASES:
            x = torch.from_numpy(make(rows, d)).to(dev)
            graph = graph_of(x)
            (old, old_count), torch_ms = walls(lambda: manifold._components_torch(*graph))
            (new, count), kernel_ms = walls(lambda: manifold._components(*graph))
            _, timer_wall, summ = under_timer(lambda: manifold._components(*graph))
            batches = summ["graph_components_rounds"]["launches"]
            # the rounds the graph needs: single rounds until one changes nothing (that last one counted)
            state = torch.arange(rows, dtype=torch.int32, device=dev)
            work, changed, needed = [torch.empty_like(state) for _ in range(2)], torch.ones(1, dtype=torch.int32, device=dev), 0
            while int(changed):
                ops.graph_components_rounds(*graph, state, *work, changed, rounds=1)
                needed += 1
            run = batches * manifold.COMPONENT_ROUNDS
            entry = {"data": kind, "rows": rows, "d": d, "entries": int(graph[1].shape[0]), "components": int(count),
                     "labels_equal": bool(torch.equal(old, new)) and old_count == count, "torch": torch_ms, "kernels": kernel_ms,
                     "batches": batches, "rounds_run": run, "rounds_needed": needed, "kernel_ms_total": round(summ["graph_components_rounds"]["total_ms"], 4),
                     "kernel_ms_per_round": round(summ["graph_components_rounds"]["total_ms"] / run, 5), "timed_pass_wall_ms": round(timer_wall, 3)}
            search.append(entry)
            print(json.dumps(entry), file=sys.stderr, flush=True)
            del x, graph
            torch.cuda.empty_cache()
        result["search"] = search
    if args.part in ("2", "both"):
        layouts = []
        solver = manifold._spectral
        for rows, d, n_clusters in CLUSTERED:
            x = torch.from_numpy(clustered_rows(rows, d, n_clusters)).to(dev)
            graph = graph_of(x)
            _, count = manifold._components(*graph)

            def init():
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)
                    return manifold.spectral_init_components(graph, DIM, SEED, rows=x)
            _, init_ms = walls(init)
            calls = []

            def clocked(*a):
                (y, info), ms = timed(lambda: solver(*a))
                calls.append((ms, int(a[0].shape[0]) - 1, int(info["iterations"]), bool(info["converged"])))
                return y, info
            manifold._spectral = clocked
            try:
                y, timer_wall, summ = under_timer(init)
            finally:
                manifold._spectral = solver
            entry = {"rows": rows, "d": d, "clusters": n_clusters, "n_neighbors": N_NEIGHBORS, "entries": int(graph[1].shape[0]),
                     "components": int(count), "finite": bool(torch.isfinite(y).all()), "spectral_init_components": init_ms,
                     "timed_pass_wall_ms": round(timer_wall, 3),
                     "search_kernels_ms": round(summ["graph_components_rounds"]["total_ms"], 4),
                     "permute_kernel_ms": round(summ["csr_components"]["total_ms"], 4) if "csr_components" in summ else None,
                     "centroid_kernel_ms": round(summ["segment_mean_gather"]["total_ms"], 4) if "segment_mean_gather" in summ else None,
                     "solver_loop": {"calls": len(calls), "wall_ms": round(sum(c[0] for c in calls), 3),
                                     "largest_component": max((c[1] for c in calls), default=0),
                                     "outer_iterations": [c[2] for c in calls], "converged": sum(c[3] for c in calls)}}
            umap = {}
            for name, start in (("spectral_init_components", manifold.spectral_init_components), ("spectral_init_random_fallback", manifold.spectral_init)):
                def run():
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore", RuntimeWarning)
                        return manifold.umap(x, init=start, n_neighbors=N_NEIGHBORS, min_dist=MIN_DIST, n_epochs=N_EPOCHS)
                out, umap[name] = walls(run)
                umap[name]["finite"] = bool(torch.isfinite(out).all())
            entry["umap"] = umap
            layouts.append(entry)
            print(json.dumps(entry), file=sys.stderr, flush=True)
            del x, graph
            torch.cuda.empty_cache()
        result["layouts"] = layouts
    result["note"] = ("wall_ms: host clock around a synchronised window; kernel times: HIP events around each entry of one further pass "
                      "(a batch's 3 x rounds launches under one pair of events); the solver loop's wall time is taken with a "
                      "synchronisation around every component's solve, which the plain call does not have")
    result["source_sha"] = bench.source_sha()
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

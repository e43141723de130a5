"""What UMAP after the k-NN graph costs on the device, at two shapes:

    18000 x 49      genes x tissues with n_neighbors=30, min_dist=0.05, 200 epochs: the call of the reference's vcf2embed notebook;
    262144 x 64     synthetic rows, the same arguments: towards the registry-token embeddings.

Per shape, one process, stage by stage as manifold.umap runs them (init="pca"):

    knn         neighbors.knn(x, 29): wall time;
    graph       manifold.fuzzy_graph's work: wall time, the two kernels' own times (ops.KernelTimer: HIP events on the launch
                stream) and the rest, which is the torch plumbing of the CSR arrays (sort / unique over 64-bit keys);
    init        the PCA initialisation (covariance and projection on the device, a d x d eigenproblem on the host);
    layout      all epochs from one call of ops.umap_layout: wall time, and the events' time over the epochs = kernel time per
                epoch (the launches of a call are back to back on one stream, nothing from the host sits between them);

with the graph's size: entries, the mean and the LARGEST CSR row -- one thread walks a row, so the largest row is the hub
imbalance -- and the entries drawn per epoch.  Wall times are a host clock around a synchronised window.  No host UMAP is
installed where this runs, so nothing is compared: the reference's notebook calls its own umap-learn step "the slow step" and
quotes 1-2 minutes, which nobody has measured here.  One JSON line, also written to profiles/umap_bench.json.

    python scripts/umap_bench.py [--rounds 3] [--warmup 1] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPES = ((18000, 49), (262144, 64))
N_NEIGHBORS, MIN_DIST, N_EPOCHS = 30, 0.05, 200


def rows_of(rows: int, d: int) -> np.ndarray:
    """Expression-like rows: a mix of a dozen programmes plus noise, so that the graph has clusters and hubs."""
    g = np.random.default_rng(rows + d)
    programme = g.standard_normal((12, d))
    return (g.standard_normal((rows, 12)) @ programme + 0.5 * g.standard_normal((rows, d)) + 5.0).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "umap_bench.json"))
    args = ap.parse_args()

    import bench
    from variantformer_amd import _lib, manifold, neighbors, ops
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("umap_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    a, b = manifold.find_ab(MIN_DIST)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def stages(x, with_timer):
        ms = {}
        (idx, dist), ms["knn"] = timed(lambda: neighbors.knn(x, k=N_NEIGHBORS - 1))
        ops.TIMER = ops.KernelTimer() if with_timer else None
        try:
            graph, ms["graph"] = timed(lambda: manifold._fuzzy_graph(idx, dist))
            y, ms["init"] = timed(lambda: manifold.rescale(manifold.pca_init(x, 2)).contiguous())
            rowptr, col, w = graph[:3]
            out, ms["layout"] = timed(lambda: manifold._layout(rowptr, col, w, y, N_EPOCHS, a, b, 1.0, 1.0, 5, 42))
            summ = ops.TIMER.summary() if with_timer else None
        finally:
            ops.TIMER = None
        return ms, graph, out, summ

    shapes = []
    for rows, d in SHAPES:
        x = torch.from_numpy(rows_of(rows, d)).to(dev)
        for _ in range(args.warmup):
            stages(x, False)
        passes = [stages(x, False)[0] for _ in range(args.rounds)]
        _, graph, out, summ = stages(x, True)
        rowptr, col, w = graph[:3]
        length = torch.diff(rowptr)
        samples = manifold.edge_samples(w, N_EPOCHS)
        kernels = {name: {"launches": summ[name]["launches"], "total_ms": round(summ[name]["total_ms"], 4)}
                   for name in ("umap_smooth_knn", "umap_union", "umap_layout")}
        mean = {k: round(sum(p[k] for p in passes) / len(passes), 3) for k in passes[0]}
        graph_kernel_ms = kernels["umap_smooth_knn"]["total_ms"] + kernels["umap_union"]["total_ms"]
        entry = {"rows": rows, "d": d, "n_neighbors": N_NEIGHBORS, "min_dist": MIN_DIST, "n_epochs": N_EPOCHS,
                 "wall_ms": {"passes": [{k: round(v, 3) for k, v in p.items()} for p in passes], "mean": mean,
                             "total_mean": round(sum(mean.values()), 3)},
                 "graph_kernels_ms": round(graph_kernel_ms, 4), "graph_torch_plumbing_ms": round(mean["graph"] - graph_kernel_ms, 3),
                 "kernels": kernels, "layout_kernel_ms_per_epoch": round(kernels["umap_layout"]["total_ms"] / N_EPOCHS, 5),
                 "csr": {"entries": int(col.shape[0]), "mean_row": round(float(length.double().mean()), 2), "largest_row": int(length.max()),
                         "entries_never_drawn": int((samples == 0).sum()), "entries_drawn_per_epoch": round(float(samples.double().sum()) / N_EPOCHS, 1)},
                 "finite": bool(torch.isfinite(out).all())}
        shapes.append(entry)
        print(json.dumps(entry), file=sys.stderr, flush=True)
        del x, graph, out
        torch.cuda.empty_cache()
    result = {"rounds": args.rounds, "warmup": args.warmup, "shapes": shapes,
              "note": "wall_ms: host clock around a synchronised window per stage of manifold.umap (init='pca'); kernels: HIP events "
                      "around each entry of one further pass, the layout's 200 launches under one pair of events; no host UMAP is "
                      "installed here, so there is no comparison: the reference notebook's '1-2 minutes' was not measured",
              "source_sha": bench.source_sha()}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

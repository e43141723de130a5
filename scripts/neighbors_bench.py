"""What the correlation k-nearest-neighbour search costs, k = 30, at the three shapes of the analysis flow:

    18000 x 49      genes x GTEx tissues: the UMAP of vcf2embed (metric="correlation", n_neighbors=30);
    18000 x 1536    one tissue's registry-token embeddings of every gene;
    54 x 18000      tissues x genes: the dendrogram's rows.

Per shape, one process, the device passes alternating round after round so that each is measured beside the other:

    fused       ops.rows_standardize + ops.knn_dot: vf_knn_dot forms the similarity tiles on the f32 MFMA and keeps the k best
                per row; nothing grows with rows x rows.  Wall time per call (host clock around a synchronised window) and the
                two kernels' own times from ops.KernelTimer (HIP events on the launch stream), with vf_knn_dot's achieved
                TFLOP/s (2 rows^2 d operations, from the shape) against the 157.3 TFLOP/s fp32 matrix peak;
    panelled    the same standardised rows through torch.matmul + torch.topk over panels of 2048 query rows: the
                bounded-memory way without the kernel (self masked to -inf before the top-k);
    cpu         sklearn.neighbors.NearestNeighbors(algorithm="brute", metric="correlation", n_jobs=16) on the host, once;
                the query (kneighbors) is timed apart from fit.

and how the three agree: the fraction of (row, rank) pairs with the same index (fp32 ties and near-ties may differ).  One JSON
line, also written to profiles/neighbors_bench.json.

    python scripts/neighbors_bench.py [--rounds 3] [--steps 5] [--warmup 2] [--min-window-ms 300] [--no-cpu]

A timed window holds at least --steps calls and at least --min-window-ms of work: the number of calls per window is set per
shape and pass from one timed call after the warm-up, and is reported.
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

FP32_MATRIX_PEAK_TFLOPS = 157.3          # MI355X, v_mfma_f32_32x32x2_f32: the fp32 vector rate
SHAPES = ((18000, 49), (18000, 1536), (54, 18000))
K = 30
PANEL = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-window-ms", type=float, default=300.0, help="a timed window holds at least this much work")
    ap.add_argument("--no-cpu", action="store_true", help="skip the scikit-learn pass")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "neighbors_bench.json"))
    args = ap.parse_args()

    import bench
    from variantformer_amd import _lib, ops
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("neighbors_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def fused(x, z, norm, values, indices):
        ops.rows_standardize(x, z=z, norm=norm)
        ops.knn_dot(z, z, min(K, x.shape[0] - 1), self_offset=0, values=values, indices=indices)

    def panelled(x, z, norm, values, indices):
        ops.rows_standardize(x, z=z, norm=norm)
        k = min(K, x.shape[0] - 1)
        for p0 in range(0, x.shape[0], PANEL):
            s = torch.matmul(z[p0:p0 + PANEL], z.T)
            n = s.shape[0]
            s[every_row[:n], every_row[p0:p0 + n]] = float("-inf")     # the index vector is made once per shape, outside the windows
            v, i = torch.topk(s, k, dim=1)
            values[p0:p0 + n], indices[p0:p0 + n] = v, i

    def window(fn, bufs, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn(*bufs)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    def timed(fn, bufs, steps):
        for _ in range(args.warmup):
            fn(*bufs)
        return window(fn, bufs, steps)

    def steps_for(fn, bufs):
        """Calls per window: --steps, or as many as --min-window-ms takes at the time of one call after the warm-up."""
        one = timed(fn, bufs, 1)
        return max(args.steps, int(args.min_window_ms / max(one, 1e-3)) + 1)

    shapes = []
    for rows, d in SHAPES:
        k = min(K, rows - 1)
        x = torch.randn((rows, d), generator=torch.Generator().manual_seed(rows + d)).to(dev)
        z, norm = torch.empty_like(x), torch.empty(rows, device=dev)
        out = {name: (torch.empty((rows, k), device=dev), torch.empty((rows, k), dtype=torch.int32 if name == "fused" else torch.int64, device=dev))
               for name in ("fused", "panelled")}
        every_row = torch.arange(rows, device=dev)
        passes = {"fused": fused, "panelled": panelled}
        times = {name: [] for name in passes}
        steps = {name: steps_for(fn, (x, z, norm) + out[name]) for name, fn in passes.items()}
        for _ in range(args.rounds):
            for name, fn in passes.items():
                times[name].append(timed(fn, (x, z, norm) + out[name], steps[name]))
        ops.TIMER = ops.KernelTimer()
        try:
            for _ in range(args.steps):
                fused(x, z, norm, *out["fused"])
            summ = ops.TIMER.summary()
        finally:
            ops.TIMER = None
        knn_ms = summ["knn_dot"]["total_ms"] / summ["knn_dot"]["launches"]
        std_ms = summ["rows_standardize"]["total_ms"] / summ["rows_standardize"]["launches"]
        tflops = 2.0 * rows * rows * d / (knn_ms * 1e-3) / 1e12
        fi, pi = out["fused"][1].cpu().numpy(), out["panelled"][1].cpu().numpy()
        entry = {
            "rows": rows, "d": d, "k": k, "calls_per_window": steps,
            "ms": {name: {"passes": [round(v, 3) for v in vs], "mean": round(sum(vs) / len(vs), 3), "spread": round(max(vs) - min(vs), 3)}
                   for name, vs in times.items()},
            "fused_over_panelled": round(sum(times["fused"]) / sum(times["panelled"]), 3),
            "kernel_ms": {"vf_rows_standardize": round(std_ms, 4), "vf_knn_dot": round(knn_ms, 4)},
            "vf_knn_dot_tflops": round(tflops, 2), "vf_knn_dot_share_of_fp32_matrix_peak": round(tflops / FP32_MATRIX_PEAK_TFLOPS, 4),
            "same_index_fused_vs_panelled": round(float((fi == pi).mean()), 6),
        }
        if not args.no_cpu:
            from sklearn.neighbors import NearestNeighbors
            host = x.cpu().numpy()
            t0 = time.perf_counter()
            nn = NearestNeighbors(n_neighbors=k + 1, algorithm="brute", metric="correlation", n_jobs=16).fit(host)
            t1 = time.perf_counter()
            ci = nn.kneighbors(host, return_distance=False)
            entry["cpu_sklearn_brute_16_threads_ms"] = round((time.perf_counter() - t1) * 1e3, 1)       # the query alone
            entry["cpu_sklearn_fit_ms"] = round((t1 - t0) * 1e3, 1)
            own = ci[:, 0] == np.arange(rows)
            entry["same_index_fused_vs_cpu"] = round(float((fi[own] == ci[own, 1:]).mean()), 6)
        shapes.append(entry)
        print(json.dumps(entry), file=sys.stderr, flush=True)
        del x, z, norm, out
        torch.cuda.empty_cache()
    result = {"k": K, "panel_rows": PANEL, "rounds": args.rounds, "steps": args.steps, "warmup": args.warmup, "min_window_ms": args.min_window_ms,
              "fp32_matrix_peak_tflops": FP32_MATRIX_PEAK_TFLOPS, "shapes": shapes,
              "note": "ms: wall time per call of standardize + search, host clock around a synchronised window; kernel_ms: HIP "
                      "events around each launch; tflops: 2 rows^2 d over vf_knn_dot's kernel time",
              "source_sha": bench.source_sha()}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

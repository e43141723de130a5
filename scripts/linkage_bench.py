"""What the Ward linkage of correlation distances costs on the device, at the two shapes of vcf2exp's
compute_ordered_leaves:

    54 x 18000      tissues x genes: the dendrogram;
    18000 x 49      genes x tissues: the row order of the heatmap (an 18000 x 18000 distance matrix).

Per shape, one process:

    device      linkage.ward_of_rows: rows standardised, the distance matrix, then rounds of ops.linkage_nearest and
                ops.linkage_contract until one cluster is left.  Wall time per call (host clock around a synchronised window; a
                call ends with its tree on the host), the kernels' own times per entry from ops.KernelTimer (HIP events on the
                launch stream) with the bytes they move (from the shapes) over that time, and the number of rounds;
    host        the notebook's own path, once: np.nan_to_num, np.corrcoef in fp64, squareform(checks=False),
                scipy.cluster.hierarchy.linkage(method="ward"), each step timed;

and how the two agree: whether leaves_list is the same, the share of rows of Z with the same two ids, and the largest relative
difference of the heights (the host path computes its distances in fp64, the device in fp32).  One JSON line, also written to
profiles/linkage_bench.json.

    python scripts/linkage_bench.py [--rounds 3] [--steps 3] [--warmup 1] [--min-window-ms 300] [--no-cpu] [--out FILE]
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

SHAPES = ((54, 18000), (18000, 49))
HBM_PEAK_GBS = 8000.0                    # MI355X


def rows_of(rows: int, d: int) -> np.ndarray:
    """Expression-like rows: a mix of a dozen programmes plus noise, so that the tree has structure at every level."""
    g = np.random.default_rng(rows + d)
    programme = g.standard_normal((12, d))
    return (g.standard_normal((rows, 12)) @ programme + 0.5 * g.standard_normal((rows, d)) + 5.0).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--min-window-ms", type=float, default=300.0, help="a timed window holds at least this much work")
    ap.add_argument("--no-cpu", action="store_true", help="skip the scipy pass")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "linkage_bench.json"))
    args = ap.parse_args()

    import bench
    from variantformer_amd import _lib, linkage, ops
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("linkage_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def window(x, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            linkage.ward_of_rows(x)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    shapes = []
    for rows, d in SHAPES:
        host = rows_of(rows, d)
        x = torch.from_numpy(host).to(dev)
        for _ in range(args.warmup):
            linkage.ward_of_rows(x)
        one = window(x, 1)
        steps = max(args.steps, int(args.min_window_ms / max(one, 1e-3)) + 1)
        times = [window(x, steps) for _ in range(args.rounds)]
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        ops.TIMER = ops.KernelTimer()
        try:
            Z, info = linkage.ward_of_rows(x, return_info=True)
            summ = ops.TIMER.summary()
        finally:
            ops.TIMER = None
        peak = torch.cuda.max_memory_allocated() - before
        kernels = {}
        for name in ("rows_standardize", "pairwise_dot", "linkage_nearest", "linkage_contract"):
            s = summ[name]
            kernels[name] = {"launches": s["launches"], "total_ms": round(s["total_ms"], 4), "gbytes": round(s["bytes"] / 1e9, 3),
                             "gbytes_per_s": round(s["bytes"] / 1e9 / (s["total_ms"] * 1e-3), 1) if s["total_ms"] > 0 else None}
        mean = sum(times) / len(times)
        kernel_ms = sum(k["total_ms"] for k in kernels.values())
        entry = {"rows": rows, "d": d, "calls_per_window": steps, "merge_rounds": info["rounds"],
                 "ms": {"passes": [round(v, 3) for v in times], "mean": round(mean, 3), "spread": round(max(times) - min(times), 3)},
                 "kernels": kernels, "kernel_ms_total": round(kernel_ms, 3), "between_kernels_ms": round(mean - kernel_ms, 3),
                 "peak_device_bytes_of_a_call": int(peak), "distance_matrix_bytes": 4 * rows * rows}
        if not args.no_cpu:
            from scipy.cluster.hierarchy import leaves_list, linkage as scipy_linkage
            from scipy.spatial.distance import squareform
            t = [time.perf_counter()]
            M = np.nan_to_num(host, nan=0.0)
            t.append(time.perf_counter())
            Dm = 1.0 - np.corrcoef(M)
            np.fill_diagonal(Dm, 0.0)
            t.append(time.perf_counter())
            y = squareform(Dm, checks=False)
            t.append(time.perf_counter())
            Zs = scipy_linkage(y, method="ward")
            t.append(time.perf_counter())
            steps_ms = [round((b - a) * 1e3, 1) for a, b in zip(t, t[1:])]
            entry["host_scipy_ms"] = {"nan_to_num": steps_ms[0], "corrcoef_fp64": steps_ms[1], "squareform": steps_ms[2],
                                      "linkage_ward": steps_ms[3], "total": round((t[-1] - t[0]) * 1e3, 1)}
            entry["host_over_device"] = round((t[-1] - t[0]) * 1e3 / mean, 2)
            entry["same_leaves_list"] = bool(np.array_equal(linkage.leaves_list(Z), leaves_list(Zs)))
            entry["same_leaf_positions"] = round(float((linkage.leaves_list(Z) == leaves_list(Zs)).mean()), 6)
            entry["same_id_rows"] = round(float((Z[:, :2] == Zs[:, :2]).all(axis=1).mean()), 6)
            entry["max_rel_height_difference"] = float((np.abs(np.sort(Z[:, 2]) - np.sort(Zs[:, 2])) / np.maximum(np.sort(Zs[:, 2]), 1e-30)).max())
            del Dm, y
        shapes.append(entry)
        print(json.dumps(entry), file=sys.stderr, flush=True)
        del x
        torch.cuda.empty_cache()
    result = {"rounds": args.rounds, "steps": args.steps, "warmup": args.warmup, "min_window_ms": args.min_window_ms,
              "hbm_peak_gbytes_per_s": HBM_PEAK_GBS, "shapes": shapes,
              "note": "ms: wall time per ward_of_rows call, host clock around a synchronised window, the tree on the host at the "
                      "end; kernels: HIP events around each launch of one further call, bytes from the shapes; host_scipy_ms: "
                      "the notebook's path on the CPU, timed once",
              "source_sha": bench.source_sha()}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

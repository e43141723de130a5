"""What k-means costs on the device, at three shapes:

    expression   18 000 x 49, metric correlation, k = 50 (the enrichment bench's cluster count);
    embedding    18 000 x 2, Euclidean, k = 50 (the coordinates of a UMAP);
    large        262 144 x 64, Euclidean, k = 1 024 (the shape every manifold bench runs; a Ward tree cannot exist there).

Per shape, after a warm-up, the median of `--rounds` runs, each under its own pair of HIP events on the launch stream:

    assign      ops.kmeans_assign (the hot kernel);
    update      ops.kmeans_update;
    iteration   ops.kmeans_lloyd with max_iter = 1: one assignment, update and finish, and the last assignment;
    seed        ops.kmeans_seed: k - 1 steps of four launches;
    whole       kmeans.kmeans(init="k-means++") end to end, a host clock around a synchronised window, and its n_iter.

Then the host, clearly apart and under a time limit, in a child process that does not touch the GPU: scikit-learn's
KMeans(init=<the same start array>, n_init=1, algorithm="lloyd") on the standardised rows, on this machine's CPUs; its n_iter_ and
the share of rows whose label equals the device's are reported (random blobs at k = 1 024 have rows within rounding of two
centres: equality is not expected there, and is pinned on conditioned fixtures by the tests instead).  One JSON line, also
written to profiles/kmeans_bench.json.

    python scripts/kmeans_bench.py [--rounds 11] [--warmup 2] [--host-limit 240] [--shapes expression,embedding,large] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# name -> (rows, columns, generating centres, noise, metric, k)
SHAPES = {"expression": (18000, 49, 50, 0.7, "correlation", 50), "embedding": (18000, 2, 50, 0.08, "euclidean", 50),
          "large": (262144, 64, 1024, 0.5, "euclidean", 1024)}

HOST_CHILD = r"""
import json, sys, time, warnings
import numpy as np
from sklearn.cluster import KMeans
d = np.load({path!r})
x = d["z"].astype(np.float64)
t0 = time.perf_counter()
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    km = KMeans(n_clusters=int(d["start"].shape[0]), init=d["start"].astype(np.float64), n_init=1, algorithm="lloyd", tol={tol!r}, max_iter={max_iter}).fit(x)
t1 = time.perf_counter()
print(json.dumps({{"sklearn_fit_s": round(t1 - t0, 3), "n_iter": int(km.n_iter_), "inertia": float(km.inertia_),
                  "labels_equal_share": float((km.labels_ == d["labels"]).mean())}}))
"""


def rows_of(name: str) -> np.ndarray:
    R, d, g, noise, _, _ = SHAPES[name]
    rng = np.random.default_rng(R + d)
    cen = rng.standard_normal((g, d)).astype(np.float32)
    return cen[rng.integers(0, g, R)] + noise * rng.standard_normal((R, d)).astype(np.float32)


def host_run(arrays: dict, tol: float, max_iter: int, limit: float) -> dict:
    with tempfile.TemporaryDirectory(prefix="kmeans_bench_") as tmp:
        path = os.path.join(tmp, "rows.npz")
        np.savez(path, **arrays)
        env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
        try:
            r = subprocess.run([sys.executable, "-c", HOST_CHILD.format(path=path, tol=tol, max_iter=max_iter)], capture_output=True, text=True,
                               timeout=limit, env=env)
        except subprocess.TimeoutExpired:
            return {"result": f"not finished within {limit:g} s"}
    if r.returncode != 0:
        return {"result": "failed: " + (r.stderr.strip().splitlines() or ["no message"])[-1][:200]}
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-limit", type=float, default=240.0)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kmeans_bench.json"))
    args = ap.parse_args()
    if args.rounds < 10:
        raise SystemExit("the medians are over at least 10 runs")
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_bench.py measures on the GPU: none found")
    import bench
    from variantformer_amd import _lib, kmeans, ops
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    tol, max_iter = 1e-4, 300

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def median(fn, timer=events):
        for _ in range(args.warmup):
            timer(fn)
        runs = [timer(fn) for _ in range(args.rounds)]
        return {"median_ms": round(statistics.median(runs), 4), "min_ms": round(min(runs), 4), "max_ms": round(max(runs), 4)}

    results, host = {}, {}
    for name in args.shapes.split(","):
        R, d, _, _, metric, k = SHAPES[name]
        x = rows_of(name)
        z = kmeans._rows_of(x, metric, True)
        rows, start = kmeans.seed_rows(z, k, 0)
        cen = start.clone()
        i32 = lambda n: torch.empty((n,), dtype=torch.int32, device=dev)
        labels, prev, counts, n_iter, dist = i32(R), i32(R), i32(k), i32(1), torch.empty((R,), dtype=torch.float32, device=dev)
        shift, changed = torch.empty((1,), dtype=torch.float64, device=dev), torch.empty((1,), dtype=torch.int64, device=dev)
        work = torch.empty((max(ops.kmeans_lloyd_work_bytes(R, d, k), ops.kmeans_seed_work_bytes(R)) + 7) // 8, dtype=torch.int64, device=dev)
        new, mind, srows, scen = torch.empty_like(cen), torch.empty((R,), dtype=torch.float32, device=dev), i32(k), torch.empty_like(cen)
        ms = {"assign": median(lambda: ops.kmeans_assign(z, start, labels=labels, dist=dist)),
              "update": median(lambda: ops.kmeans_update(z, labels, start, cen_new=new, counts=counts))}

        def iteration():
            cen.copy_(start)
            ops.kmeans_lloyd(z, cen, max_iter=1, tol_abs=0.0, labels=labels, dist=dist, prev_labels=prev, counts=counts, n_iter=n_iter,
                             shift=shift, changed=changed, work=work)
        ms["iteration"] = median(iteration)
        ms["seed"] = median(lambda: ops.kmeans_seed(z, k, 0, rows=srows, cen=scen, mind=mind, work=work))
        model = kmeans.kmeans(x, k, metric=metric, init="k-means++", seed=0, tol=tol, max_iter=max_iter)
        ms["whole"] = median(lambda: kmeans.kmeans(x, k, metric=metric, init="k-means++", seed=0, tol=tol, max_iter=max_iter), timer=wall)
        pair_ops = 3.0 * R * k * d
        results[name] = {"rows": R, "columns": d, "k": k, "metric": metric, "ms": ms, "n_iter": model.n_iter, "inertia": model.inertia,
                         "empty_clusters": int((np.asarray(model.counts) == 0).sum()),
                         "assign_gflops_fp32": round(pair_ops / (ms["assign"]["median_ms"] * 1e-3) / 1e9, 1),
                         "seed_ms_per_step": round(ms["seed"]["median_ms"] / max(k - 1, 1), 5)}
        print(json.dumps({name: results[name]}), file=sys.stderr, flush=True)
        host[name] = host_run({"z": z.cpu().numpy(), "start": start.cpu().numpy(), "labels": model.labels}, tol, max_iter, args.host_limit)
        host[name]["device_whole_ms"] = ms["whole"]["median_ms"]
        host[name]["device_n_iter"] = model.n_iter
        print(json.dumps({name: host[name]}), file=sys.stderr, flush=True)
        del x, z, start, cen, labels, prev, dist, new, mind, work, model
    result = {"rounds": args.rounds, "warmup": args.warmup, "tol": tol, "max_iter": max_iter, "shapes": results, "host": host,
              "note": "assign, update, iteration, seed: HIP events around one call, median of `rounds` runs after `warmup`; iteration: "
                      "vf_kmeans_lloyd with max_iter = 1 (begin, assignment, update, finish, last assignment); whole: host clock around a "
                      "synchronised kmeans.kmeans(init='k-means++'), seeding and read-backs included; host: scikit-learn KMeans(lloyd) from the "
                      "device's start array on this machine's CPUs in a child process of its own, one run; rows are Gaussian blobs",
              "source_sha": bench.source_sha()}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

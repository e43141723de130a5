"""What the silhouette coefficient costs on the device, at five shapes:

    expression-dot   18 000 x 49, k = 50, metric correlation: the linear path;
    expression-l2    18 000 x 49, k = 50, Euclidean on the standardised rows (k-means' space): all pairs;
    embedding-l2     18 000 x 2, k = 50, Euclidean (the coordinates of a UMAP): all pairs;
    large-dot        262 144 x 64, k = 1 024, metric correlation: the linear path, in row chunks;
    large-l2         262 144 x 2, k = 1 024, Euclidean: all pairs, 6.9e10 of them, in row chunks.

Per shape, after a warm-up, the median of `--rounds` runs, each under its own pair of HIP events on the launch stream:

    sums     ops.silhouette_sums_l2 or ops.silhouette_sums_dot over all row chunks (the hot kernel);
    finish   ops.silhouette_finish over all row chunks;
    whole    validation.silhouette_samples end to end on rows that are on the device, labels from the host: a host clock around a
             synchronised window; its score.

Then the host, clearly apart and under a time limit, in a child process that does not touch the GPU: scikit-learn's
silhouette_samples on the fp64 copy of the same rows, on this machine's CPUs, for the 18 000-row shapes (the others are not
attempted: 262 144 rows are 6.9e10 pairs in fp64 chunks); the largest difference of the two results is reported.  One JSON line,
also written to profiles/silhouette_bench.json.

    python scripts/silhouette_bench.py [--rounds 7] [--warmup 2] [--host-limit 300] [--shapes a,b,..] [--out FILE]
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

# name -> (rows, columns, clusters, noise, metric, standardize, scikit-learn on the host)
SHAPES = {"expression-dot": (18000, 49, 50, 0.7, "correlation", None, True), "expression-l2": (18000, 49, 50, 0.7, "euclidean", "correlation", True),
          "embedding-l2": (18000, 2, 50, 0.08, "euclidean", None, True), "large-dot": (262144, 64, 1024, 0.5, "correlation", None, False),
          "large-l2": (262144, 2, 1024, 0.02, "euclidean", None, False)}

HOST_CHILD = r"""
import json, sys, time
import numpy as np
from sklearn.metrics import silhouette_samples
d = np.load({path!r})
x = d["x"].astype(np.float64)
t0 = time.perf_counter()
s = silhouette_samples(x, d["labels"], metric={metric!r})
t1 = time.perf_counter()
print(json.dumps({{"sklearn_s": round(t1 - t0, 3), "largest_difference": float(np.abs(s - d["samples"]).max()), "score": float(s.mean())}}))
"""


def rows_of(name: str):
    R, d, k, noise, *_ = SHAPES[name]
    rng = np.random.default_rng(R + d + k)
    cen = rng.standard_normal((k, d))
    labels = rng.integers(0, k, R)
    return np.ascontiguousarray(cen[labels] + noise * rng.standard_normal((R, d)), dtype=np.float32), labels.astype(np.int64)


def _timed(fn, rounds: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def measure(name: str, rounds: int, warmup: int) -> dict:
    from variantformer_amd import neighbors, ops, validation as V
    R, d, k, _, metric, standardize, _ = SHAPES[name]
    x, labels = rows_of(name)
    xd = torch.from_numpy(x).cuda()
    z = xd if metric == "euclidean" and standardize is None else neighbors.standardize(xd, metric if metric != "euclidean" else standardize)[0]
    codes, _ = V.encode_labels(labels, R)
    labels32, order, seg, _ = V._clusters(codes, k, z.device)
    step = V.chunk_rows(R, k, V.DEFAULT_MAX_BYTES)
    S = torch.empty((k, step), dtype=torch.float64, device=z.device)
    work = torch.empty((k * d,), dtype=torch.float64, device=z.device)
    a, b, s = (torch.empty((R,), dtype=torch.float64, device=z.device) for _ in range(3))
    nearest = torch.empty((R,), dtype=torch.int32, device=z.device)
    chunks = [(r0, min(step, R - r0)) for r0 in range(0, R, step)]

    def sums():
        for r0, rows in chunks:
            if metric == "euclidean":
                ops.silhouette_sums_l2(z, order, seg, r0, rows, S=S[:, :rows])
            else:
                ops.silhouette_sums_dot(z, order, seg, labels32, r0, rows, S=S[:, :rows], work=work)

    def finish():
        for r0, rows in chunks:
            ops.silhouette_finish(S[:, :rows], labels32, seg, r0, rows, a=a, b=b, s=s, nearest=nearest)

    out = {"rows": R, "columns": d, "clusters": k, "metric": metric, "standardize": standardize, "path": "l2" if metric == "euclidean" else "dot",
           "row_chunks": len(chunks), "sums_ms": round(_timed(sums, rounds, warmup), 4), "finish_ms": round(_timed(finish, rounds, warmup), 4)}
    pairs = float(R) * float(R)
    if metric == "euclidean":
        out["pairs_per_s"] = round(pairs / (out["sums_ms"] * 1e-3), 1)
    whole = []
    for i in range(warmup + rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = V.silhouette_samples(xd, labels, metric=metric, standardize=standardize)
        torch.cuda.synchronize()
        if i >= warmup:
            whole.append((time.perf_counter() - t0) * 1e3)
    out["whole_ms"] = round(statistics.median(whole), 3)
    out["score"] = res.score
    out["_samples"] = res.samples.cpu().numpy()
    out["_x"], out["_labels"] = x, labels
    return out


def host(name: str, result: dict, limit: float) -> dict:
    metric, standardize = SHAPES[name][4:6]
    if standardize is not None:
        return {"skipped": "scikit-learn has no Euclidean distance on standardised rows; the dot shape of the same rows is its twin"}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "rows.npz")
        np.savez(path, x=result["_x"], labels=result["_labels"], samples=result["_samples"])
        env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
        try:
            r = subprocess.run([sys.executable, "-c", HOST_CHILD.format(path=path, metric=metric)], capture_output=True, text=True, timeout=limit, env=env)
        except subprocess.TimeoutExpired:
            return {"skipped": f"scikit-learn did not finish within {limit:.0f} s"}
    if r.returncode != 0:
        return {"skipped": "scikit-learn failed: " + (r.stderr.strip().splitlines() or ["no message"])[-1]}
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-limit", type=float, default=300.0)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "silhouette_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the bench needs a GPU"
    from variantformer_amd import ops
    report = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "ranges": ops.SILHOUETTE_RANGES, "shapes": {}}
    for name in args.shapes.split(","):
        result = measure(name, args.rounds, args.warmup)
        if SHAPES[name][6]:
            result["host"] = host(name, result, args.host_limit)
        report["shapes"][name] = {key: v for key, v in result.items() if not key.startswith("_")}
        print(f"[silhouette_bench] {name}: {report['shapes'][name]}", file=sys.stderr, flush=True)
    line = json.dumps(report)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

"""Times the forest evaluator behind the AD-risk predictors (ops.forest_predict, vf_forest_predict) on one GPU and the float64
NumPy restatement of the same work on the host:

  row form     32 genes x 45 tissues = 1440 rows, each through its own 100-tree, depth-10 forest on 1536 features -- what
               ADriskFromVCF launches once per query;
  cohort form  4096 rows through one such forest -- what ADrisk.__call__ launches.

    python scripts/ad_risk_bench.py [--out profiles/ad_risk_bench.json] [--steps 2000] [--warmup 5]

Writes one JSON record.  There is no threshold: these are the first numbers of a path the project did not have.  The forests
are seeded random trees (a node above the depth limit splits with probability 0.7: about 140 nodes a tree, the size scikit-learn
grows on a few hundred samples), not fitted ones: the work per walk is the same, the branch statistics are not."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from variantformer_amd import forest as Fo  # noqa: E402


def random_models(n_models: int, T: int, depth: int, F: int, K: int, p_split: float, seed: int) -> list:
    """n_models seeded forests of T trees each, grown level by level for all trees at once, then laid out tree by tree (a
    child's index above its parent's)."""
    g = np.random.default_rng(seed)
    n_trees = n_models * T
    tree = [np.arange(n_trees)]
    parent, side, split = [np.full(n_trees, -1)], [np.zeros(n_trees, dtype=np.int8)], []
    first = 0
    for d in range(depth + 1):
        n = tree[-1].size
        s = (g.random(n) < p_split) | (d == 0) if d < depth else np.zeros(n, dtype=bool)
        split.append(s)
        who = np.flatnonzero(s)
        if who.size == 0:
            break
        tree.append(np.repeat(tree[-1][who], 2))
        parent.append(np.repeat(first + who, 2))
        side.append(np.tile(np.array([0, 1], dtype=np.int8), who.size))
        first += n
    tree, parent, side, split = np.concatenate(tree), np.concatenate(parent), np.concatenate(side), np.concatenate(split)
    order = np.argsort(tree, kind="stable")                           # tree by tree, levels in order inside a tree
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    left = np.full(tree.size, -1, dtype=np.int64)
    right = np.full(tree.size, -1, dtype=np.int64)
    kids = np.flatnonzero(parent >= 0)
    lk, rk = kids[side[kids] == 0], kids[side[kids] == 1]
    left[rank[parent[lk]]], right[rank[parent[rk]]] = rank[lk], rank[rk]
    tree, split = tree[order], split[order]
    model = tree // T
    node_base = np.searchsorted(model, np.arange(n_models))
    is_leaf = ~split
    leaf_rank = np.cumsum(is_leaf) - 1
    leaf_base = np.concatenate([[0], np.cumsum(is_leaf)])[node_base]
    feature = np.where(split, g.integers(0, F, tree.size), -1)
    threshold = g.normal(size=tree.size).astype(np.float32)
    default_left = g.integers(0, 2, tree.size)
    leaves = g.random((int(is_leaf.sum()), K)).astype(np.float32)
    leaves /= leaves.sum(axis=1, keepdims=True)
    roots = np.flatnonzero(np.concatenate([[True], tree[1:] != tree[:-1]]))
    ends = np.append(node_base, tree.size)
    out = []
    for m in range(n_models):
        a, b = ends[m], ends[m + 1]
        lf = is_leaf[a:b]
        out.append(Fo.PackedForest(feature[a:b], threshold[a:b], np.where(lf, leaf_rank[a:b] - leaf_base[m], left[a:b] - a),
                                   np.where(lf, 0, right[a:b] - a), np.where(lf, 0, default_left[a:b]), roots[m * T:(m + 1) * T] - a,
                                   leaves[leaf_base[m]:leaf_base[m] + int(lf.sum())], np.zeros(K), F, True, "identity"))
    return out


def _time_gpu(fn, steps: int, warmup: int) -> list:
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(3):                                                 # three windows: the spread is part of the record
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / steps)
    return times


def _time_cold(fn, repeats: int = 5) -> list:
    """One launch at a time, each after a 512 MiB fill that pushes the bank out of the caches: what a query's one call sees."""
    import torch
    scratch = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    times = []
    for i in range(repeats):
        scratch.fill_(i)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ad_risk_bench.json"))
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--genes", type=int, default=32)
    ap.add_argument("--tissues", type=int, default=45)
    ap.add_argument("--cohort", type=int, default=4096)
    args = ap.parse_args()
    import torch
    from variantformer_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("ad_risk_bench needs a GPU: a host timing of the HIP path would mean nothing")
    T, depth, F, K = 100, 10, 1536, 2
    M = args.genes * args.tissues
    t0 = time.perf_counter()
    models = random_models(M, T, depth, F, K, 0.7, 20260101)
    bank = Fo.ForestBank(models)
    build_s = time.perf_counter() - t0
    g = np.random.default_rng(7)
    x_rows = g.normal(size=(M, F)).astype(np.float32)
    x_cohort = g.normal(size=(args.cohort, F)).astype(np.float32)
    t0 = time.perf_counter()
    dev = bank.to("cuda")
    torch.cuda.synchronize()
    upload_s = time.perf_counter() - t0
    xr, xc = torch.from_numpy(x_rows).cuda(), torch.from_numpy(x_cohort).cuda()
    mor = torch.arange(M, dtype=torch.int32, device="cuda")
    out_r = torch.empty((M, K), dtype=torch.float32, device="cuda")
    out_c = torch.empty((args.cohort, K), dtype=torch.float32, device="cuda")
    row, cohort = (lambda: ops.forest_predict(xr, dev, model_of_row=mor, out=out_r)), (lambda: ops.forest_predict(xc, dev, model=M // 2, out=out_c))
    row_ms, cohort_ms = _time_gpu(row, args.steps, args.warmup), _time_gpu(cohort, args.steps, args.warmup)
    row_cold_ms, cohort_cold_ms = _time_cold(row), _time_cold(cohort)
    # the same work on the host, in float64 NumPy (one vectorised walk of a forest's trees per row / of the cohort)
    t0 = time.perf_counter()
    host_r = np.concatenate([models[m].predict_host(x_rows[m:m + 1]) for m in range(M)])
    host_row_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    host_c = models[M // 2].predict_host(x_cohort)
    host_cohort_s = time.perf_counter() - t0
    err_r = float(np.abs(out_r.cpu().numpy() - host_r).max())
    err_c = float(np.abs(out_c.cpu().numpy() - host_c).max())
    assert err_r < 1e-5 and err_c < 1e-5, (err_r, err_c)               # probabilities in [0, 1], 100 fp32 additions
    sha = hashlib.sha256()
    for rel in ("variantformer_amd/csrc/vf_forest.hip", "include/vf_hip_forest.h", "variantformer_amd/forest.py"):
        with open(os.path.join(REPO, rel), "rb") as f:
            sha.update(f.read())
    rec = {"shape": {"genes": args.genes, "tissues": args.tissues, "forests": M, "trees": T, "depth": depth, "features": F, "outputs": K,
                     "cohort_rows": args.cohort, "bank_nodes": int(bank.nodes.shape[0]), "bank_bytes": int(sum(
                         getattr(bank, k).nbytes for k in Fo.ForestBank.ARRAYS))},
           "steps": args.steps, "warmup": args.warmup,
           "row_form_ms": [round(v, 4) for v in row_ms], "row_form_forests_per_s": round(M / (min(row_ms) * 1e-3)),
           "cohort_form_ms": [round(v, 4) for v in cohort_ms], "cohort_form_rows_per_s": round(args.cohort / (min(cohort_ms) * 1e-3)),
           "row_form_cold_ms": [round(v, 4) for v in row_cold_ms], "cohort_form_cold_ms": [round(v, 4) for v in cohort_cold_ms],
           "host_numpy_float64_row_form_s": round(host_row_s, 3), "host_numpy_float64_cohort_form_s": round(host_cohort_s, 3),
           "bank_build_s": round(build_s, 2), "bank_upload_s": round(upload_s, 3),
           "max_abs_difference_from_host": {"row_form": err_r, "cohort_form": err_c},
           "note": "device times are HIP events around `steps` back-to-back launches on the same rows (the nodes they walk stay in the "
                   "caches), three windows each; the cold times are single launches, each after a 512 MiB fill; the host times are one "
                   "pass of PackedForest.predict_host (float64 sums, NumPy) over the same rows; seeded random forests, not fitted "
                   "ones.  First measurement of this path: nothing to compare with.",
           "source_sha": sha.hexdigest()[:16]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

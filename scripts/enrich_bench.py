"""What the enrichment of gene clusters costs on the device, at two annotations over a universe of 18 000 genes
in 50 clusters of 50 .. 2 000 genes (the rest in no cluster):

    detailed    15 000 terms of 5 .. 500 genes: 7.5e5 cells, the notebook's go_category_detailed;
    broad       12 terms of 500 .. 5 000 genes: 600 cells, its go_category_broad.

Per annotation, after a warm-up, the median of `--rounds` runs, each under its own pair of HIP events on the launch stream:

    counts      ops.enrich_counts over the annotation (one block per term, a k-bin LDS histogram);
    csize       the same entry over the one term that lists every gene: the cluster sizes;
    tail        ops.hypergeom_tail, alternative "greater" (one thread per cell);
    bh          enrichment._bh: torch's sort, running minimum and scatter in fp64;
    whole       enrichment.enrich end to end, a host clock around a synchronised window: the above plus the table of
                log-factorials (math.lgamma on the host, 18 001 values), the uploads, exp, fold, the read-back and the frame.

Beside them the distribution of `steps`, the number of terms a cell's sum added, and what it says about divergence: a wavefront
takes as long as its longest cell, so lane_use = mean steps / mean of the wavefronts' largest steps.  Then the host, clearly
apart and under a time limit, in a child process that does not touch the GPU: scipy.stats.hypergeom.sf on the same cells, and
scipy.stats.false_discovery_control on the device's p, which the device's q must equal bit for bit.  One JSON line, also written to profiles/enrich_bench.json.

    python scripts/enrich_bench.py [--rounds 11] [--warmup 2] [--host-limit 300] [--out FILE]
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

GENES, CLUSTERS = 18000, 50
ANNOTATIONS = {"detailed": (15000, 5, 500), "broad": (12, 500, 5000)}

HOST_CHILD = r"""
import json, sys, time
import numpy as np
from scipy import stats
d = np.load({path!r})
t0 = time.perf_counter()
p = stats.hypergeom.sf(d["count"] - 1, {genes}, d["size"][:, None], d["csize"][None, :])
t1 = time.perf_counter()
q = stats.false_discovery_control(d["p"].ravel(), method="bh")
t2 = time.perf_counter()
with np.errstate(divide="ignore"):
    dev = np.abs(np.log(p) - d["log_p"])[p > 1e-280]
print(json.dumps({{"hypergeom_sf_s": round(t1 - t0, 3), "false_discovery_control_s": round(t2 - t1, 4), "cells": int(p.size),
                  "largest_log_p_difference_above_1e-280": float(dev.max()), "q_equal_bit_for_bit": bool(np.array_equal(q, d["q"].ravel()))}}))
"""


def labels_of(seed: int = 0) -> np.ndarray:
    """int32 [GENES]: CLUSTERS clusters of 50 .. 2 000 genes in random places, every other gene in no cluster (-1)."""
    g = np.random.default_rng(seed)
    while True:                                                       # 50 clusters of up to 2 000 must fit 18 000 genes: small ones are common
        sizes = np.exp(g.uniform(np.log(50.0), np.log(1000.0), size=CLUSTERS)).astype(np.int64)
        sizes[:2] = (2000, 50)
        if sizes.sum() <= GENES:
            break
    labels = np.full(GENES, -1, dtype=np.int32)
    labels[g.permutation(GENES)[:sizes.sum()]] = np.repeat(np.arange(CLUSTERS, dtype=np.int32), sizes)
    return labels


def membership_of(name: str, seed: int = 1):
    """The annotation as an enrichment.Membership, built directly: T terms of lo .. hi distinct random genes, ascending."""
    from variantformer_amd import enrichment
    T, lo, hi = ANNOTATIONS[name]
    g = np.random.default_rng(seed + T)
    sizes = g.integers(lo, hi + 1, size=T)
    termptr = np.zeros(T + 1, dtype=np.int64)
    termptr[1:] = np.cumsum(sizes)
    gene = np.concatenate([np.sort(g.choice(GENES, size=s, replace=False)) for s in sizes]).astype(np.int32)
    return enrichment.Membership(termptr, gene, [f"term_{t:05d}" for t in range(T)], GENES)


def host_run(arrays: dict, limit: float) -> dict:
    """scipy on the same cells in a child process without the GPU, ended at the limit."""
    with tempfile.TemporaryDirectory(prefix="enrich_bench_") as tmp:
        path = os.path.join(tmp, "cells.npz")
        np.savez(path, **arrays)
        env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
        try:
            r = subprocess.run([sys.executable, "-c", HOST_CHILD.format(path=path, genes=GENES)], capture_output=True, text=True, timeout=limit, env=env)
        except subprocess.TimeoutExpired:
            return {"result": f"not finished within {limit:g} s"}
    if r.returncode != 0:
        return {"result": "failed: " + (r.stderr.strip().splitlines() or ["no message"])[-1][:200]}
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-limit", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "enrich_bench.json"))
    args = ap.parse_args()
    if args.rounds < 10:
        raise SystemExit("the medians are over at least 10 runs")
    if not torch.cuda.is_available():
        raise SystemExit("enrich_bench.py measures on the GPU: none found")
    import bench
    from variantformer_amd import _lib, enrichment, ops
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

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
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def median(fn, timer=events):
        for _ in range(args.warmup):
            timer(fn)
        runs = [timer(fn) for _ in range(args.rounds)]
        runs = [r[1] if isinstance(r, tuple) else r for r in runs]
        return {"median_ms": round(statistics.median(runs), 4), "min_ms": round(min(runs), 4), "max_ms": round(max(runs), 4)}

    labels = labels_of()
    k = CLUSTERS
    lab = torch.from_numpy(labels).to(dev)
    logfact = torch.from_numpy(enrichment.log_factorials(GENES)).to(dev)
    every, whole = torch.arange(GENES, dtype=torch.int32, device=dev), torch.tensor([0, GENES], dtype=torch.int64, device=dev)
    results, host = {}, {}
    for name in ANNOTATIONS:
        m = membership_of(name)
        T = len(m.terms)
        termptr, gene = torch.from_numpy(m.termptr).to(dev), torch.from_numpy(m.gene).to(dev)
        count, size = torch.empty((T, k), dtype=torch.int32, device=dev), torch.empty(T, dtype=torch.int32, device=dev)
        csize, one = torch.empty((1, k), dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        log_p, tail = torch.empty((T, k), dtype=torch.float64, device=dev), torch.empty((T, k), dtype=torch.float64, device=dev)
        steps = torch.empty((T, k), dtype=torch.int32, device=dev)
        ms = {"counts": median(lambda: ops.enrich_counts(termptr, gene, lab, k, count=count, size=size)),
              "csize": median(lambda: ops.enrich_counts(whole, every, lab, k, count=csize, size=one)),
              "tail": median(lambda: ops.hypergeom_tail(count, size, csize[0], GENES, logfact, 0, log_p=log_p, tail=tail, steps=steps))}
        p = torch.exp(log_p)
        ms["bh"] = median(lambda: enrichment._bh(p))
        ms["whole"] = median(lambda: enrichment.enrich(labels, m), timer=wall)
        out = enrichment.enrich(labels, m)
        st = steps.cpu().numpy().ravel()
        pad = np.zeros(-(-st.size // 64) * 64, dtype=st.dtype)
        pad[:st.size] = st
        waves = pad.reshape(-1, 64).max(1)
        pct = [int(v) for v in np.percentile(st, (50, 90, 99, 100))]
        results[name] = {"terms": T, "clusters": k, "genes": GENES, "cells": T * k, "entries": int(m.gene.shape[0]),
                         "term_size": {"min": int(out["term_size"].min()), "max": int(out["term_size"].max())},
                         "cluster_size": {"min": int(out["cluster_size"].min()), "max": int(out["cluster_size"].max())},
                         "ms": ms, "cells_per_s_tail": round(T * k / (ms["tail"]["median_ms"] * 1e-3), 1),
                         "steps": {"mean": round(float(st.mean()), 2), "p50": pct[0], "p90": pct[1], "p99": pct[2], "max": pct[3],
                                   "cells_without_a_sum": int((out["log_p"] == 0).sum() + np.isneginf(out["log_p"]).sum()),
                                   "mean_of_wavefront_max": round(float(waves.mean()), 2), "lane_use": round(float(st.mean() / max(waves.mean(), 1e-9)), 3)},
                         "significant_at_0.05": int(len(out["frame"])), "smallest_log_p": float(out["log_p"].min())}
        print(json.dumps({name: results[name]}), file=sys.stderr, flush=True)
        host[name] = host_run({"count": out["count"], "size": out["term_size"], "csize": out["cluster_size"], "log_p": out["log_p"], "p": out["p"], "q": out["q"]},
                              args.host_limit)
        host[name]["device_whole_ms"] = ms["whole"]["median_ms"]
        print(json.dumps({name: host[name]}), file=sys.stderr, flush=True)
    result = {"rounds": args.rounds, "warmup": args.warmup, "annotations": results, "host": host,
              "note": "counts, csize, tail, bh: HIP events around one call, median of `rounds` runs after `warmup`; whole: host clock around a "
                      "synchronised enrichment.enrich; host: scipy.stats.hypergeom.sf and false_discovery_control on this machine's CPUs in a "
                      "child process of its own, one run, on the device's counts (sf) and on the device's p (false_discovery_control); random labels and terms: nothing is enriched, q stays near 1",
              "source_sha": bench.source_sha()}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

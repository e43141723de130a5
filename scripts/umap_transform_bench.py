"""What placing new rows in a fitted UMAP embedding costs on the device, beside what the fit cost:

    18000 x 49      genes x tissues, the notebook's arguments (n_neighbors=30, min_dist=0.05): fit, then transform 18 000 rows that
                    are the training rows times 1 + 0.05 noise (a second individual);
    262144 x 64     synthetic rows, the same arguments: fit, then transform 65 536 such rows.

Per case, one process: the fit's wall time (manifold.fit, init="pca", n_epochs by its default), then the transform stage by
stage as UMAPModel.transform runs them:

    knn         standardising the queries and the search among the standardised training rows (ops.knn_dot): wall time;
    strengths   ops.umap_smooth_knn_query and ops.umap_init_transform, the two small kernels: wall time and the events' time;
    plumbing    the draw counts, in torch: wall time;
    layout      all epochs from one call of ops.umap_layout_transform: wall time, the events' time, and that over the launches
                (VF_UMAP_TRANSFORM_EPOCHS_PER_LAUNCH epochs each, back to back on one stream);

and the whole of model.transform.  Then the layout kernel alone at its largest: ONE launch (8 epochs) for 262 144 queries with
m = 64, rate 5 and every entry due in every epoch, among 18 000 x 2 training positions (144 KB: they live in L2) and among
2^24 x 8 (512 MB: they do not).  Wall times are a host clock around a synchronised window, kernel times HIP events on the launch
stream (ops.KernelTimer).  No host UMAP is installed where this runs, so nothing external is compared.  The one expectation is
that a transform of as many rows as the fit costs less than the fit did; it is reported (`transform_below_fit`), not asserted.
One JSON line, also written to profiles/umap_transform_bench.json.

    python scripts/umap_transform_bench.py [--rounds 3] [--warmup 1] [--out FILE]
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

CASES = ((18000, 49, 18000), (262144, 64, 65536))
N_NEIGHBORS, MIN_DIST = 30, 0.05
EPOCHS_PER_LAUNCH = 8                      # VF_UMAP_TRANSFORM_EPOCHS_PER_LAUNCH
LARGEST = dict(Rq=262144, m=64, rate=5, trainings=((18000, 2), (1 << 24, 8)))


def rows_of(rows: int, d: int) -> np.ndarray:
    """Expression-like rows: a mix of a dozen programmes plus noise, so that the graph has clusters and hubs."""
    g = np.random.default_rng(rows + d)
    programme = g.standard_normal((12, d))
    return (g.standard_normal((rows, 12)) @ programme + 0.5 * g.standard_normal((rows, d)) + 5.0).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "umap_transform_bench.json"))
    args = ap.parse_args()

    import bench
    from variantformer_amd import _lib, manifold, neighbors, ops
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("umap_transform_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def stages(model, q, N, with_timer):
        z, y = model._on_device()
        m, Rq = model.n_neighbors, q.shape[0]
        ms = {}

        def search():
            zq, _ = neighbors.standardize(q, model.metric, True)
            idx = torch.empty((Rq, m), dtype=torch.int32, device=dev)
            dist = torch.empty((Rq, m), dtype=torch.float32, device=dev)
            ops.knn_dot(zq, z, m, self_offset=-1, values=dist, indices=idx)
            dist.neg_().add_(1.0)
            dist.masked_fill_(idx < 0, float("inf"))
            return idx, dist
        (idx, dist), ms["knn"] = timed(search)
        ops.TIMER = ops.KernelTimer() if with_timer else None
        try:
            sigma = torch.empty(Rq, dtype=torch.float32, device=dev)
            strength = torch.empty((Rq, m), dtype=torch.float32, device=dev)
            yq = torch.empty((Rq, model.n_components), dtype=torch.float32, device=dev)

            def small():
                ops.umap_smooth_knn_query(idx, dist, model.mean_dist, sigma=sigma, strength=strength)
                ops.umap_init_transform(idx, strength, y, out=yq)
            _, ms["strengths"] = timed(small)
            samples, ms["plumbing"] = timed(lambda: manifold.transform_samples(strength, N))
            _, ms["layout"] = timed(lambda: ops.umap_layout_transform(
                idx, samples, y, yq, epoch_begin=0, epoch_end=N, n_epochs=N, a=model.a, b=model.b, gamma=model.repulsion_strength,
                learning_rate=model.learning_rate, negative_sample_rate=model.negative_sample_rate, seed=model.seed))
            summ = ops.TIMER.summary() if with_timer else None
        finally:
            ops.TIMER = None
        return ms, samples, yq, summ

    cases = []
    for rows, d, Rq in CASES:
        x = rows_of(rows, d)
        g = np.random.default_rng(Rq)
        q = torch.from_numpy((x[:Rq] * (1.0 + 0.05 * g.standard_normal((Rq, d)))).astype(np.float32)).to(dev)
        xt = torch.from_numpy(x).to(dev)
        kw = dict(n_neighbors=N_NEIGHBORS, min_dist=MIN_DIST)
        for _ in range(args.warmup):
            manifold.fit(xt, **kw)
        fits = []
        for _ in range(args.rounds):
            model, ms = timed(lambda: manifold.fit(xt, **kw))
            fits.append(ms)
        N = 100 if Rq <= 10000 else 30
        for _ in range(args.warmup):
            stages(model, q, N, False)
        passes = [stages(model, q, N, False)[0] for _ in range(args.rounds)]
        wholes = [timed(lambda: model.transform(q))[1] for _ in range(args.rounds)]
        _, samples, yq, summ = stages(model, q, N, True)
        kernels = {name: {"launches": summ[name]["launches"], "total_ms": round(summ[name]["total_ms"], 4)}
                   for name in ("umap_smooth_knn_query", "umap_init_transform", "umap_layout_transform")}
        launches = -(-N // EPOCHS_PER_LAUNCH)
        mean = {k: round(sum(p[k] for p in passes) / len(passes), 3) for k in passes[0]}
        fit_ms, whole_ms = sum(fits) / len(fits), sum(wholes) / len(wholes)
        entry = {"training_rows": rows, "d": d, "queries": Rq, "n_neighbors": N_NEIGHBORS, "min_dist": MIN_DIST, "fit_epochs": model.n_epochs,
                 "transform_epochs": N, "fit_wall_ms": {"passes": [round(v, 3) for v in fits], "mean": round(fit_ms, 3)},
                 "transform_wall_ms": {"passes": [{k: round(v, 3) for k, v in p.items()} for p in passes], "mean": mean,
                                       "stages_total_mean": round(sum(mean.values()), 3), "model_transform_mean": round(whole_ms, 3)},
                 "kernels": kernels, "layout_kernel_launches": launches,
                 "layout_kernel_ms_per_launch": round(kernels["umap_layout_transform"]["total_ms"] / launches, 4),
                 "draws_per_epoch": round(float(samples.double().sum()) / N, 1), "finite": bool(torch.isfinite(yq).all()),
                 "transform_below_fit": bool(whole_ms < fit_ms) if Rq == rows else None,
                 "fit_ms_per_row": round(fit_ms / rows, 6), "transform_ms_per_row": round(whole_ms / Rq, 6)}
        cases.append(entry)
        print(json.dumps(entry), file=sys.stderr, flush=True)
        del x, xt, q, model, samples, yq
        torch.cuda.empty_cache()

    # the layout kernel at its largest: one launch, every entry due in every epoch
    largest = []
    Rq, m, rate = LARGEST["Rq"], LARGEST["m"], LARGEST["rate"]
    a, b = manifold.find_ab(MIN_DIST)
    for R, dim in LARGEST["trainings"]:
        gen = torch.Generator(device=dev).manual_seed(R)
        Y = torch.rand((R, dim), generator=gen, device=dev) * 10.0
        idx = torch.randint(0, R, (Rq, m), generator=gen, device=dev, dtype=torch.int32)
        samples = torch.full((Rq, m), 200, dtype=torch.int32, device=dev)
        start = torch.rand((Rq, dim), generator=gen, device=dev) * 10.0
        times = []
        for r in range(args.warmup + args.rounds):
            yq = start.clone()
            ops.TIMER = ops.KernelTimer()
            try:
                ops.umap_layout_transform(idx, samples, Y, yq, epoch_begin=0, epoch_end=EPOCHS_PER_LAUNCH, n_epochs=200, a=a, b=b,
                                          negative_sample_rate=rate, seed=42)
                ms = ops.TIMER.summary()["umap_layout_transform"]["total_ms"]
            finally:
                ops.TIMER = None
            if r >= args.warmup:
                times.append(round(ms, 3))
        moves = EPOCHS_PER_LAUNCH * Rq * m * (1 + rate)
        entry = {"queries": Rq, "m": m, "rate": rate, "training_rows": R, "dim": dim, "epochs_in_the_launch": EPOCHS_PER_LAUNCH,
                 "launch_ms": times, "moves": moves, "moves_per_s": round(moves / (min(times) * 1e-3), 1), "finite": bool(torch.isfinite(yq).all())}
        largest.append(entry)
        print(json.dumps(entry), file=sys.stderr, flush=True)
        del Y, idx, samples, start, yq
        torch.cuda.empty_cache()

    result = {"rounds": args.rounds, "warmup": args.warmup, "cases": cases, "largest_launch": largest,
              "note": "wall_ms: host clock around a synchronised window; kernels: HIP events around each entry of one further pass, the "
                      "layout's launches under one pair of events; largest_launch: one launch of the layout kernel with every entry due "
                      "in every epoch; no host UMAP is installed here, so nothing external is compared; transform_below_fit is "
                      "reported, not asserted",
              "source_sha": bench.source_sha()}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

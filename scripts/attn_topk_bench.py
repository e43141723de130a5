"""What the ranked cCREs cost at scripts/attn_maps_bench.py's shape (bench.py's model and batch: 32 genes x 54 tissues,
1024 cCREs, production depth), one process, the passes alternating round after round so that each is measured beside the
others under the same conditions:

    off              the step with the capture off;
    full             all gene layers' cCRE maps captured and copied to the host whole (cap.maps.cpu(): the path without top_k,
                     at its cheapest -- the per-gene split on the host is not counted);
    top_k            the same capture, ranked on the device and only the selections copied: the model's own _with_top_k,
                     per-gene split included;
    full_contrib / top_k_contrib   both again with contributions=True (two maps).

and the selection kernel's own time from ops.KernelTimer (HIP events around each vf_topk_rows launch) with its algorithmic
bytes / time.  One JSON line, also written to profiles/attn_topk_bench.json.

    python scripts/attn_topk_bench.py [--rounds 3] [--steps 6] [--warmup 3] [--top-k 32] [--no-top-k]

--no-top-k times `off`, `full` and `full_contrib` alone: the same script then runs on a tree from before top_k (the parent
commit), which is how the two trees are compared in one session.  A step is bench.py's step (forward_prepared + the
expression matrix copied to the host)."""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E, on paper


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--top-k", type=int, default=32)
    ap.add_argument("--no-top-k", action="store_true", help="time the passes without top_k alone (a tree from before it)")
    ap.add_argument("--genes-per-step", type=int, default=32)
    ap.add_argument("--n-cre", type=int, default=1024)
    ap.add_argument("--n-chunks", type=int, default=200)
    ap.add_argument("--tissues", type=int, default=54)
    ap.add_argument("--layers", type=int, default=None, help="override modulator depth (debug only)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "attn_topk_bench.json"))
    args = ap.parse_args()

    import bench
    from variantformer_amd import attn_maps, ops
    from variantformer_amd.utils.synthetic import TISSUES_54, make_batch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model, hp, kw = bench.build_model(dev, args.layers)
    G, tissues = args.genes_per_step, TISSUES_54[: args.tissues]
    batch = make_batch(20251205, [args.n_cre] * G, [args.n_chunks] * G, [tissues] * G, 200)
    n_layers = len(model.combined_modulator.gene_layers)
    every = list(range(n_layers))

    def step(mode, contributions):
        if mode == "off":
            model.forward_prepared(pb)[0].cpu()
            return
        with attn_maps.capture(every, contributions=contributions) as cap:
            model.forward_prepared(pb)[0].cpu()
            if mode == "full":
                cap.maps.cpu()
                if contributions:
                    cap.contrib.cpu()
            else:
                model._with_top_k({}, cap, args.top_k)

    def timed(mode, contributions=False):
        for _ in range(args.warmup):
            step(mode, contributions)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(mode, contributions)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    passes = [("off", "off", False), ("full", "full", False), ("top_k", "top_k", False), ("full_contrib", "full", True),
              ("top_k_contrib", "top_k", True)]
    if args.no_top_k:
        passes = [p for p in passes if p[1] != "top_k"]
    times = {name: [] for name, _, _ in passes}
    kernel = None
    with torch.no_grad():
        pb = model.prepare_batch(batch)
        for _ in range(args.rounds):
            for name, mode, contributions in passes:
                times[name].append(timed(mode, contributions))
        if not args.no_top_k:
            ops.TIMER = ops.KernelTimer()
            try:
                step("top_k", True)
                summ = ops.TIMER.summary()
            finally:
                ops.TIMER = None
            k = summ["topk_rows"]
            gbs = k["bytes"] / (k["total_ms"] * 1e-3) / 1e9
            kernel = {"launches": k["launches"], "total_ms": round(k["total_ms"], 4), "ms_per_launch": round(k["total_ms"] / k["launches"], 4),
                      "bytes": k["bytes"], "algorithmic_gb_per_s": round(gbs, 1),
                      "algorithmic_gb_per_s_over_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
                      "per_map_ms": {n.split(":", 1)[1]: round(v["total_ms"], 4) for n, v in summ.items() if n.startswith("topk_rows:")},
                      "note": "vf_topk_rows, one launch per captured buffer viewed as [layers * rows, max_k], bracketed by HIP "
                              "events on the launch stream; bytes = the rows' valid values once and the outputs"}
    rows = n_layers * G * len(tissues)
    result = {
        "shape": {"genes": G, "tissues": len(tissues), "n_cre": args.n_cre, "n_chunks": args.n_chunks, "gene_layers": n_layers},
        "rounds": args.rounds, "steps": args.steps, "warmup": args.warmup, "top_k": None if args.no_top_k else args.top_k,
        "ms": {name: {"passes": [round(v, 3) for v in vs], "mean": round(sum(vs) / len(vs), 3), "spread": round(max(vs) - min(vs), 3)}
               for name, vs in times.items()},
        "map_bytes": rows * args.n_cre * 4, "selection_bytes": None if args.no_top_k else rows * args.top_k * 8,
        "kernel": kernel,
        "source_sha": bench.source_sha(),
    }
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

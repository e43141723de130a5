"""What the attention maps cost at the headline shape (bench.py's model and batch: 32 genes x 54 tissues, 1024 cCREs,
production depth): step time with the capture off, with the gene -> cCRE maps of the last gene layer only and of all gene
layers, with BOTH maps (gene -> cCRE and gene body) of the last layer and of all layers, and the two probabilities kernels' own
times and algorithmic bytes / time against the HBM peak (ops.KernelTimer).  One JSON line, also written to
profiles/attn_maps_bench_gene_body.json (profiles/attn_maps_bench.json is the run before the gene-body maps existed).
Then the cCRE CONTRIBUTION maps (capture(contributions=True): a second, per-head probabilities launch and vf_attn_contrib per
captured layer): step time for the last layer and for all layers beside the capture-off step of the same run, and the
contribution launches' own ops.KernelTimer time; a second JSON line, written to profiles/attn_contrib_bench.json.
Then the GENE-BODY contribution maps (capture(gene_contributions=True): a per-head ALiBi probabilities launch and
vf_attn_contrib_self per captured layer): the same step times, the kernel's own time per layer, and -- for comparison only,
never on the product path -- the Gram route on the same operands (the value rows gathered where there is a row map, then
ops.attn_contrib with one row per sequence); a third JSON line, written to profiles/attn_gene_contrib_bench.json.

    python scripts/attn_maps_bench.py [--steps 6] [--warmup 3] [--genes-per-step 32] [--layers N]

A step is bench.py's step (forward_prepared + the expression matrix copied to the host); with a capture the maps stay on the
device (`..._ms`) or are copied to the host as predict_step_with_attention does (`..._with_d2h_ms`)."""
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
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--genes-per-step", type=int, default=32)
    ap.add_argument("--n-cre", type=int, default=1024)
    ap.add_argument("--n-chunks", type=int, default=200)
    ap.add_argument("--tissues", type=int, default=54)
    ap.add_argument("--layers", type=int, default=None, help="override modulator depth (debug only)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "attn_maps_bench_gene_body.json"))
    ap.add_argument("--contrib-out", default=os.path.join(REPO, "profiles", "attn_contrib_bench.json"))
    ap.add_argument("--gene-contrib-out", default=os.path.join(REPO, "profiles", "attn_gene_contrib_bench.json"))
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

    def timed(layers, d2h, gene_body=False, contributions=False, gene_contributions=False):
        def step():
            if layers is None:
                model.forward_prepared(pb)[0].cpu()
                return
            with attn_maps.capture(layers, gene_body=gene_body, contributions=contributions,
                                   gene_contributions=gene_contributions) as cap:
                model.forward_prepared(pb)[0].cpu()
                if d2h:
                    cap.maps.cpu()
                    if gene_body:
                        cap.gene_maps.cpu()
                    if contributions:
                        cap.contrib.cpu()
                    if gene_contributions:
                        cap.gene_contrib.cpu()
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    with torch.no_grad():
        pb = model.prepare_batch(batch)
        off = timed(None, False)
        last = timed([n_layers - 1], False)
        last_d2h = timed([n_layers - 1], True)
        every = timed(list(range(n_layers)), False)
        every_d2h = timed(list(range(n_layers)), True)
        both_last = timed([n_layers - 1], False, True)
        both_last_d2h = timed([n_layers - 1], True, True)
        both_every = timed(list(range(n_layers)), False, True)
        both_every_d2h = timed(list(range(n_layers)), True, True)
        off_again = timed(None, False)
        ops.TIMER = ops.KernelTimer()
        with attn_maps.capture(list(range(n_layers)), gene_body=True):
            model.forward_prepared(pb)[0].cpu()
        summ = ops.TIMER.summary()
        ops.TIMER = None
        con_last = timed([n_layers - 1], False, contributions=True)
        con_last_d2h = timed([n_layers - 1], True, contributions=True)
        con_every = timed(list(range(n_layers)), False, contributions=True)
        con_every_d2h = timed(list(range(n_layers)), True, contributions=True)
        off_third = timed(None, False)
        ops.TIMER = ops.KernelTimer()
        with attn_maps.capture(list(range(n_layers)), contributions=True):
            model.forward_prepared(pb)[0].cpu()
        csumm = ops.TIMER.summary()
        ops.TIMER = None
        gcon_last = timed([n_layers - 1], False, gene_contributions=True)
        gcon_last_d2h = timed([n_layers - 1], True, gene_contributions=True)
        gcon_every = timed(list(range(n_layers)), False, gene_contributions=True)
        gcon_every_d2h = timed(list(range(n_layers)), True, gene_contributions=True)
        off_fourth = timed(None, False)
        ops.TIMER = ops.KernelTimer()
        with attn_maps.capture(list(range(n_layers)), gene_contributions=True):
            model.forward_prepared(pb)[0].cpu()
        gsumm = ops.TIMER.summary()
        ops.TIMER = None
        gram_route = gram_route_times(model, G * len(tissues), 1 + args.n_chunks, dev)
    k = summ["attn_probs"]
    gbs = k["bytes"] / (k["total_ms"] * 1e-3) / 1e9
    ka = summ["attn_probs_alibi"]
    gbs_a = ka["bytes"] / (ka["total_ms"] * 1e-3) / 1e9
    result = {
        "shape": {"genes": G, "tissues": len(tissues), "n_cre": args.n_cre, "n_chunks": args.n_chunks, "gene_layers": n_layers},
        "steps": args.steps, "warmup": args.warmup,
        "capture_off_ms": round(off, 3), "capture_off_repeat_ms": round(off_again, 3),
        "last_layer_ms": round(last, 3), "last_layer_with_d2h_ms": round(last_d2h, 3),
        "all_layers_ms": round(every, 3), "all_layers_with_d2h_ms": round(every_d2h, 3),
        "both_maps_last_layer_ms": round(both_last, 3), "both_maps_last_layer_with_d2h_ms": round(both_last_d2h, 3),
        "both_maps_all_layers_ms": round(both_every, 3), "both_maps_all_layers_with_d2h_ms": round(both_every_d2h, 3),
        "kernel": {"launches": k["launches"], "total_ms": round(k["total_ms"], 3),
                   "ms_per_layer": round(k["total_ms"] / k["launches"], 4), "bytes": k["bytes"], "flops": k["flops"],
                   "algorithmic_gb_per_s": round(gbs, 1), "algorithmic_gb_per_s_over_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
                   "note": "both passes of vf_attn_probs per launch, bracketed by HIP events on the launch stream.  bytes = the "
                           "ALGORITHMIC minimum (K once per pass + the selected queries + the map and the statistics written "
                           "once), so the rate is algorithmic bytes / time, not traffic measured at the HBM: pass 1 reads K once "
                           "per 32-row tile (twice at 54 rows) and a K slab that fits the last-level cache need not come from "
                           "HBM in pass 2"},
        "kernel_alibi": {"launches": ka["launches"], "total_ms": round(ka["total_ms"], 3),
                         "ms_per_layer": round(ka["total_ms"] / ka["launches"], 4), "bytes": ka["bytes"], "flops": ka["flops"],
                         "algorithmic_gb_per_s": round(gbs_a, 1), "algorithmic_gb_per_s_over_hbm_peak": round(gbs_a / HBM_PEAK_GBS, 4),
                         "note": "the gene-body map's launches (ALiBi form of vf_attn_probs_v2, one registry row per (gene, "
                                 "tissue) against its <= 201 keys).  bytes = the selected queries twice, every sequence's K once "
                                 "per pass, the index loads (q_rows; in the first layer also the key row map), the map and the "
                                 "statistics"},
        "source_sha": bench.source_sha(),
    }
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    kc = csumm["attn_contrib"]
    kp = next(v for name, v in csumm.items() if name.startswith("attn_probs:") and name.endswith("_contrib"))
    off_mean = (off + off_again + off_third) / 3.0
    contrib = {
        "shape": result["shape"], "steps": args.steps, "warmup": args.warmup,
        "capture_off_ms": [round(off, 3), round(off_again, 3), round(off_third, 3)],
        "maps_last_layer_ms": round(last, 3), "maps_all_layers_ms": round(every, 3),
        "contributions_last_layer_ms": round(con_last, 3), "contributions_last_layer_with_d2h_ms": round(con_last_d2h, 3),
        "contributions_all_layers_ms": round(con_every, 3), "contributions_all_layers_with_d2h_ms": round(con_every_d2h, 3),
        "contributions_all_layers_over_capture_off": round(con_every / off_mean, 4),
        "kernel_contrib": {"launches": kc["launches"], "total_ms": round(kc["total_ms"], 3),
                           "ms_per_layer": round(kc["total_ms"] / kc["launches"], 4), "flops": kc["flops"], "bytes": kc["bytes"],
                           "tflops": round(kc["flops"] / (kc["total_ms"] * 1e-3) / 1e12, 2),
                           "note": "vf_attn_contrib, both kernels (the keys' Gram matrices on the fp32 MFMA, then the norms), "
                                   "bracketed by HIP events on the launch stream.  flops = the Gram stage's upper triangle of head "
                                   "pairs, 2 (dh^2 + dh) per key and pair, plus 2 H^2 per (row, key)"},
        "kernel_per_head_probs": {"launches": kp["launches"], "total_ms": round(kp["total_ms"], 3),
                                  "ms_per_layer": round(kp["total_ms"] / kp["launches"], 4),
                                  "note": "the second, per-head vf_attn_probs launch into the scratch (the head-mean map keeps "
                                          "its own call and bits)"},
        "source_sha": bench.source_sha(),
    }
    cline = json.dumps(contrib)
    print(cline)
    os.makedirs(os.path.dirname(args.contrib_out), exist_ok=True)
    with open(args.contrib_out, "w") as f:
        f.write(cline + "\n")
    gline = gene_contrib_line(args, result["shape"], [off, off_again, off_third, off_fourth],
                              (gcon_last, gcon_last_d2h, gcon_every, gcon_every_d2h), gsumm, gram_route, bench.source_sha())
    print(gline)
    os.makedirs(os.path.dirname(args.gene_contrib_out), exist_ok=True)
    with open(args.gene_contrib_out, "w") as f:
        f.write(gline + "\n")


def gram_route_times(model, n_seq: int, n_keys: int, dev, reps: int = 3) -> dict:
    """ops.attn_contrib_self against the Gram route (ops.attn_contrib with one row per sequence, the value rows gathered first
    where there is a row map) on the same operands, per call, by ops.KernelTimer: the last gene layer's packed out_proj and
    seeded value rows and probabilities of the bench shape (the time does not depend on their values), with and without the
    first layer's row map.  The Gram route's fp32 [keys, H, H] scratch is this function's own."""
    from variantformer_amd import ops
    from variantformer_amd.seq2gene.modules.layers import packed_linear
    mha = model.combined_modulator.gene_layers[-1].mixer.MHA
    H, dh, D = mha.num_heads, mha.head_dim, mha.embed_dim
    wo = packed_linear(mha.out_proj)[0]
    keys = n_seq * n_keys
    g = torch.Generator(device=dev).manual_seed(7)
    qkv = torch.randn((keys, 3 * D), generator=g, device=dev, dtype=torch.float32).to(wo.dtype)
    rows = torch.randperm(keys, generator=g, device=dev)
    probs = torch.softmax(torch.randn((n_seq * H, n_keys), generator=g, device=dev), dim=-1)
    cu_k = torch.arange(n_seq + 1, dtype=torch.int32, device=dev) * n_keys
    cu_rows = torch.arange(n_seq + 1, dtype=torch.int32, device=dev)
    out = torch.empty((n_seq, n_keys), dtype=torch.float32, device=dev)
    gram = torch.empty((keys, H, H), dtype=torch.float32, device=dev)
    s_gram = mha.contrib_gram()
    v = qkv[:, 2 * D:]

    def direct(v_rows):
        ops.attn_contrib_self(v, wo, probs, cu_k, n_keys, H, dh, out=out, v_rows=v_rows, family="direct" + ("_rows" if v_rows is not None else ""))

    def gram_route(v_rows):
        vv = v if v_rows is None else ops.gather_rows_bf16(v, v_rows)
        ops.attn_contrib(vv, s_gram, probs, cu_rows, cu_k, 1, n_keys, H, dh, gram=gram, out=out, family="gram_route")

    res = {}
    for label, v_rows in (("", None), ("_row_map", rows)):
        for name, fn in (("direct", direct), ("gram_route", gram_route)):
            fn(v_rows)                                                   # warm
            ops.TIMER = ops.KernelTimer()
            try:
                for _ in range(reps):
                    fn(v_rows)
                summ = ops.TIMER.summary()
            finally:
                ops.TIMER = None
            res[name + label + "_ms"] = round(sum(r["total_ms"] for n, r in summ.items() if ":" not in n) / reps, 4)
    res["gram_scratch_bytes"] = gram.numel() * 4
    res["note"] = ("per call at the bench shape; gram_route = ops.attn_contrib with cu_rows = arange (its Gram kernel, its norm "
                   "kernel), with a row map also the gather of the value rows in front of it; comparison only")
    return res


def gene_contrib_line(args, shape, offs, gcon, gsumm, gram_route, sha) -> str:
    kc = gsumm["attn_contrib_self"]
    kp = [v for name, v in gsumm.items() if name.startswith("attn_probs_alibi:") and name.endswith("_gene_contrib")]
    kp_ms, kp_n = sum(v["total_ms"] for v in kp), sum(v["launches"] for v in kp)
    tflops = kc["flops"] / (kc["total_ms"] * 1e-3) / 1e12
    off_mean = sum(offs) / len(offs)
    return json.dumps({
        "shape": shape, "steps": args.steps, "warmup": args.warmup,
        "capture_off_ms": [round(v, 3) for v in offs],
        "gene_contributions_last_layer_ms": round(gcon[0], 3), "gene_contributions_last_layer_with_d2h_ms": round(gcon[1], 3),
        "gene_contributions_all_layers_ms": round(gcon[2], 3), "gene_contributions_all_layers_with_d2h_ms": round(gcon[3], 3),
        "gene_contributions_last_layer_over_capture_off": round(gcon[0] / off_mean, 4),
        "gene_contributions_all_layers_over_capture_off": round(gcon[2] / off_mean, 4),
        "kernel_contrib_self": {"launches": kc["launches"], "total_ms": round(kc["total_ms"], 3),
                                "ms_per_layer": round(kc["total_ms"] / kc["launches"], 4), "flops": kc["flops"], "bytes": kc["bytes"],
                                "tflops": round(tflops, 1), "fraction_of_gemm_rate_1085_tflops": round(tflops / 1085.0, 3),
                                "note": "vf_attn_contrib_self inside the forward, bracketed by HIP events on the launch stream.  "
                                        "flops = 2 keys H dh Do; bytes = the algorithmic minimum (v, P, wo and out once)"},
        "kernel_per_head_probs": {"launches": kp_n, "total_ms": round(kp_ms, 3), "ms_per_layer": round(kp_ms / max(kp_n, 1), 4),
                                  "note": "the per-head ALiBi vf_attn_probs_v2 launch into the scratch"},
        "gram_route_comparison": gram_route,
        "source_sha": sha,
    })


if __name__ == "__main__":
    main()

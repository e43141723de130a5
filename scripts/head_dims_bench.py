"""Attention at the padded head dims (vf_attn_varlen_fwd_v3) next to their class, and the new classes 192 / 256 on the
modulator's shapes at D = 1536.  Times are per launch (CUDA events over `reps` back-to-back launches after a warm-up);
TB/s against the algorithmic bytes 2 * H * dh * (2 sq + 2 sk) of the call's own head dim.

    python scripts/head_dims_bench.py [genes]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from oracle.vf_oracle import alibi_slopes
from variantformer_amd import ops

HBM_TBS = 8.0                                  # MI355X HBM3E peak


def timed(H, dh, ql, kl, alibi, self_attn, reps=20):
    D = H * dh
    tq, tk = sum(ql), sum(kl)
    cu_q = torch.tensor([0] + list(np.cumsum(ql)), dtype=torch.int32, device="cuda")
    cu_k = torch.tensor([0] + list(np.cumsum(kl)), dtype=torch.int32, device="cuda")
    slopes = torch.tensor(alibi_slopes(H), dtype=torch.float32, device="cuda") if alibi else None
    if self_attn:
        qkv = torch.randn((tq, 3 * D), device="cuda").bfloat16()
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    else:
        q = torch.randn((tq, D), device="cuda").bfloat16()
        kv = torch.randn((tk, 2 * D), device="cuda").bfloat16()
        k, v = kv[:, :D], kv[:, D:]
    call = lambda: ops.attn_varlen(q, k, v, cu_q, cu_k, max(ql), max(kl), H, dh, slopes, q_log2=True)  # the model's call form
    for _ in range(3):
        call()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        call()
    e.record()
    torch.cuda.synchronize()
    us = s.elapsed_time(e) / reps * 1e3
    tbs = 2.0 * D * (2 * tq + 2 * tk) / us / 1e6
    return us, tbs, ops.last_kernel("attn")


def head_class(d):
    return next(c for c in (32, 48, 64, 96, 128, 192, 256) if d <= c)


def main():
    g = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    rng = np.random.default_rng(0)
    print(f"# MI355X, bf16 operands, q pre-scaled (VF_ATTN_Q_LOG2); roofline {HBM_TBS} TB/s")
    print("## seq2reg windows: N = 1024 windows of 70-200 tokens, H = 8, self attention, no bias")
    wl = [int(x) for x in rng.integers(70, 201, 1024)]
    print("%-5s %-5s %10s %8s %10s %8s %7s  %s" % ("dh", "class", "us", "TB/s", "class us", "TB/s", "ratio", "kernel"))
    for d in (8, 16, 24, 40, 56, 72, 80, 88, 104, 112, 120, 136, 160, 184, 200, 224, 248):
        c = head_class(d)
        us, tbs, kern = timed(8, d, wl, wl, False, True)
        uc, tc, kc = timed(8, c, wl, wl, False, True)
        assert kern == kc, (kern, kc)
        print("%-5d %-5d %10.1f %8.2f %10.1f %8.2f %7.3f  %s" % (d, c, us, tbs, uc, tc, us / uc, kern))
    print(f"## modulator shapes at D = 1536, {g} gene(s): gene stream 54 x 201 tokens (ALiBi), CRE stream 1024 tokens (ALiBi), "
          "gene->CRE cross attention 54 x 201 queries x 1024 keys")
    print("%-5s %-4s %-10s %10s %8s %8s  %s" % ("dh", "H", "shape", "us", "TB/s", "of HBM", "kernel"))
    for dh in (48, 128, 192, 256):
        H = 1536 // dh
        for name, ql, kl, alibi, self_attn in (("gene", [201] * (54 * g), [201] * (54 * g), True, True),
                                               ("cre", [1024] * g, [1024] * g, True, True),
                                               ("gene->cre", [54 * 201] * g, [1024] * g, False, False)):
            us, tbs, kern = timed(H, dh, ql, kl, alibi, self_attn)
            print("%-5d %-4d %-10s %10.1f %8.2f %7.1f%%  %s" % (dh, H, name, us, tbs, 100 * tbs / HBM_TBS, kern))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Golden fixture of the tokenizer's per-tissue classifier heads: the reference's own Seq2RegPredictor.forward(only_embed=False)
and predict_step (seq2reg/model.py:193-302, :440-449), fp32 on the CPU with the stand-ins of tests/golden/make_golden.py (whose
header says what is real and what is stubbed).  Runs only where the reference is present; what it writes
(tests/golden/cre_heads.npz, cre_heads.json) is data: seeds, shapes and the reference's outputs.

Every case is the `small_sin` tokenizer with a few hyper-parameters changed.  Weights are name-keyed (fill_state_dict), windows
have 3-41 valid tokens (make_gene); the second strand of a sample comes from a differently seeded make_gene call so that the
strands differ.  tests/cre_heads_cases.py rebuilds weights and inputs from the recorded seeds.

Usage:  python tests/golden/make_cre_heads_golden.py      (writes next to this file)
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG  # noqa: E402

CRE_LEN_RANGE = (3, 41)
STRAND_SEED_STEP = 5000          # strand s of a case: make_gene(seed + s * STRAND_SEED_STEP, ...)
# every tissue at least twice, not sorted
CASES = {
    "mean2": dict(seed=921, n_strands=2, tissue_vector=[2, 0, 1, 1, 2, 0, 0, 2, 1],
                  over=dict(strand_agg="mean", positional_encoding="sinusoidal", cre_type="multi", num_classes=11, num_tissues=3)),
    "concat2": dict(seed=922, n_strands=2, tissue_vector=[3, 1, 0, 2, 2, 0, 1, 3, 1],
                    over=dict(strand_agg="concat", positional_encoding="alibi", cre_type="9class", num_classes=9, num_tissues=4)),
    "ctx1": dict(seed=923, n_strands=1, tissue_vector=[1, 0, 0, 1, 1, 0, 1],
                 over=dict(use_context=True, cre_type="binary", num_classes=2, num_tissues=2)),
}


def case_inputs(seed: int, b: int, n_strands: int, token_length: int):
    """(x int64 [b, n_strands, L], padding_mask bool [b, n_strands, L], context int64 [b]) of a case."""
    from variantformer_amd.utils.synthetic import make_gene
    gs = [make_gene(seed + s * STRAND_SEED_STEP, b, 2, [7], token_length, cre_len_range=CRE_LEN_RANGE) for s in range(n_strands)]
    x = torch.cat([g["cre_sequences"] for g in gs], dim=1).contiguous()
    mask = torch.cat([g["cre_attention_masks"] for g in gs], dim=1).contiguous()
    return x, mask, gs[0]["ref_cre_labels"]


def main():
    MG.install_stubs()
    from seq2reg.model import Seq2RegPredictor
    from variantformer_amd.utils.synthetic import fill_state_dict
    base = MG.FIXTURES["small_sin"]["seq2reg"]
    arrays, meta = {}, {}
    torch.set_num_threads(4)
    for name, c in CASES.items():
        hp = dict(base, **c["over"])
        torch.manual_seed(0)
        m = Seq2RegPredictor(**hp)
        fill_state_dict(m, c["seed"])
        m.eval()
        tv = torch.tensor(c["tissue_vector"], dtype=torch.long)
        b = tv.numel()
        assert sorted(tv.tolist()) != tv.tolist() and all(int((tv == t).sum()) >= 2 for t in range(hp["num_tissues"]))
        x, mask, ctx = case_inputs(c["seed"], b, c["n_strands"], hp["token_length"])
        with torch.no_grad():
            logits, x_embed = m(x, mask, tv, context=ctx if hp["use_context"] else None, precision=None)
            pred = m.predict_step((x, mask, tv, torch.zeros(b, dtype=torch.long), ctx, None), 0)
        assert tuple(logits.shape) == (b, hp["num_classes"]) and tuple(x_embed.shape) == (b, c["n_strands"], hp["embedding_dim"])
        for key, val in (("logits", logits), ("x_embed", x_embed), ("predict_step", pred), ("tissue_vector", tv)):
            arrays[f"{name}.{key}"] = val.numpy()
        sd = m.state_dict()
        meta[name] = dict(hparams=hp, seed=c["seed"], n_strands=c["n_strands"], b=b, cre_len_range=list(CRE_LEN_RANGE),
                          strand_seed_step=STRAND_SEED_STEP, state_dict_shapes={k: list(v.shape) for k, v in sd.items()},
                          weight_abs_sum=float(sum(float(v.double().abs().sum()) for v in sd.values() if torch.is_floating_point(v))))
        print(f"[golden] cre_heads {name}: logits {tuple(logits.shape)} {logits.ravel()[:3].numpy()}")
    np.savez_compressed(os.path.join(HERE, "cre_heads.npz"), **arrays)
    with open(os.path.join(HERE, "cre_heads.json"), "w") as f:
        json.dump(dict(cases=meta, generated_by="tests/golden/make_cre_heads_golden.py: reference seq2reg.model.Seq2RegPredictor "
                                                "forward(only_embed=False) and predict_step (fp32, CPU, stubbed flash_attn)"),
                  f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()

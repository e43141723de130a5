"""Shared test helpers: build the HIP-backed model for a golden fixture or a seeded config."""
import numpy as np
import torch

from variantformer_amd.utils.synthetic import fill_state_dict


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def erel(a, b):
    """element-wise: max |a-b| / (|b| + rms(b)), so that small elements count (not the max-norm)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / (np.abs(b) + np.sqrt((b * b).mean()) + 1e-30)).max())


def prel(a, b):
    """element-wise relative error max |a-b| / |b| for the EXPRESSION output (Softplus values, never near zero): the
    north-star's "within 1e-3 relative" read literally, per element."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / (np.abs(b) + 1e-30)).max())


def signal_rel(got, want):
    """Error as a fraction of the SIGNAL: max |got - want| over every value of a list of per-gene arrays (or one array),
    divided by the standard deviation of `want` across all genes x tissues.  Random-weight expressions sit in a narrow
    band around softplus(0) ~ 0.69, so an error that is small against the VALUE (the north-star's relative tolerance) can
    still be a visible fraction of the differences between tissues; this metric says how much.  nan when `want` holds
    fewer than 3 values or its spread is below 1 % of its mean (nothing to compare with: e.g. fixture small_opts_a, whose
    start-token pooling gives every tissue of a gene the same expression)."""
    g = np.concatenate([np.asarray(x, np.float64).ravel() for x in (got if isinstance(got, (list, tuple)) else [got])])
    w = np.concatenate([np.asarray(x, np.float64).ravel() for x in (want if isinstance(want, (list, tuple)) else [want])])
    if w.size < 3 or w.std() < 1e-2 * np.abs(w).mean():
        return float("nan")          # no spread to speak of (one value, or all tissues within 1 % of each other)
    return float(np.abs(g - w).max() / w.std())


# The environment of a process whose CPU transcendentals must be bit-identical on every x86-64 host.  torch evaluates
# exp / sin / cos through MKL's vector math, whose last bits depend on the code path MKL picks for the CPU (an AVX-512
# Intel host and an AMD host disagree by up to 64 ulps in a 512 x 200 sinusoidal table); MKL's SSE4.2 path runs the same
# instructions on every such host.  Read at process start, so it applies to child processes only.
PINNED_CPU_MATH = {"MKL_ENABLE_INSTRUCTIONS": "SSE4_2", "ATEN_CPU_CAPABILITY": "default"}


SIGNAL_RTOL = 2e-2      # expression error allowed as a fraction of the across-gene / across-tissue spread (signal_rel);
                        # measured on MI355X: 5e-4 ... 1.5e-2 (profiles/r05_l_pytest_gpu_final.log; 3e-2 until round 6)


def check_signal(tag, got, want, tol=SIGNAL_RTOL):
    """Print and assert the signal-relative error next to a north-star (value-relative) assertion."""
    s = signal_rel(got, want)
    print(f"[signal] {tag}: max|err| / std(expression across genes x tissues) = {s:.2e}")
    assert not (s >= tol), f"{tag}: error is {s:.2e} of the expression spread (limit {tol:g})"
    return s


def build_model(seq2reg_hp: dict, seq2gene_kw: dict, state_dict: dict | None = None, seed: int | None = None,
                gene_seq2reg_hp: dict | None = None):
    from variantformer_amd.seq2gene.model_combined_modulator import Seq2GenePredictorCombinedModulator
    from variantformer_amd.seq2reg.model import Seq2RegPredictor
    cre_tok = Seq2RegPredictor(**seq2reg_hp)
    gene_tok = Seq2RegPredictor(**(gene_seq2reg_hp or seq2reg_hp))
    model = Seq2GenePredictorCombinedModulator(cre_tokenizer=cre_tok, gene_tokenizer=gene_tok, **seq2gene_kw)
    if state_dict is not None:
        model.load_state_dict(state_dict, strict=True)
    elif seed is not None:
        fill_state_dict(model, seed)
    model.eval()
    return model


def state_dict_cpu(model):
    return {k: v.detach().cpu().float() if torch.is_floating_point(v) else v.detach().cpu() for k, v in model.state_dict().items()}


SEQ2REG_512 = dict(vocab_size=500, embedding_dim=512, num_heads=8, num_layers=2, num_tissues=2, num_classes=2,
                   learning_rate=1e-4, loss_fn=["cross_entropy", "0"], seq_pool="mean", cre_type="binary",
                   token_length=200, use_context=False, positional_encoding="sinusoidal", use_flash=True)


def seq2gene_kw(emb_dim=1536, heads=32, layers=2, token_dim=512, gene_emb_dim=512):
    return dict(num_tissues=63, emb_dim=emb_dim, gene_emb_dim=gene_emb_dim, num_heads=heads, num_layers=layers,
                use_alibi=True, mlp_dout=0.1, use_context=True, token_dim=token_dim, gene_pooling="multi_registry",
                multi_head=False, use_bigger_head=True, only_cross_attention=False, cross_alibi=False,
                add_context_to_cres=False, use_res=False, train_gene_tokenizer=True, use_batching=True)

"""Operands, float64 restatement, fixture loader and write-set cases of the tokenizer's per-tissue classifier heads
(vf_tissue_heads, include/vf_hip_cre_heads.h), shared by tests/test_cre_heads_cpu.py and tests/test_cre_heads_gpu.py.  Importing
this module needs no GPU.

The restatement is the header's arithmetic in float64: the strands of a sample are averaged (or concatenated), and
logit[b, t, c] = bias[t, c] + sum_f xbar[b, f] * w[t, c, f].  Beside every logit stands its a-priori error bound
    bound = F * 2^-23 * (sum_f |xbar_f * w_f| + |bias|),
what an fp32 dot product of F terms can lose in ANY summation order (F * 2^-24 * sum |terms|, Higham 3.5), doubled: the second
half pays for the fp32 rounding of xbar itself (at most n_strands - 1 additions and one division, each 2^-24 relative, and
n_strands + 1 <= F at every shape used) and for the last addition of the bias.  Nothing in it is measured.
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -23
AGG = {"mean": 0, "concat": 1}
N_TISSUES = 5                                          # heads of every kernel-level case
EXTRA_LDX, EXTRA_LDO = 12, 5                           # ldx > d (a multiple of 4), ldo wider than a row's values

# (d, C, n_strands, strand_agg, B, tissues of the all form): every d, C, n_strands, B and n_sel of the kernel's paths at least
# once with either aggregation -- B 1 / 5 / 67: one wave, a partial block of four (sample, tissue) waves, many blocks; the lists
# are shuffled and two repeat a tissue
GEOMETRIES = (
    (8, 1, 1, "mean", 1, (3,)),
    (8, 2, 2, "concat", 5, (4, 0, 4)),
    (8, 11, 2, "mean", 5, (2, 3, 0, 4, 1)),
    (8, 64, 3, "mean", 67, (1, 0, 3)),
    (200, 1, 2, "concat", 67, (4, 1, 0)),
    (200, 9, 2, "mean", 67, (2, 4, 0, 1, 3)),
    (200, 11, 3, "mean", 5, (1, 3, 1)),
    (200, 64, 1, "concat", 5, (0,)),
    (520, 2, 3, "mean", 67, (2,)),
    (520, 9, 1, "mean", 1, (0, 4, 2, 3, 1)),
    (520, 11, 2, "concat", 67, (4, 2, 4)),
    (520, 64, 3, "concat", 5, (3, 0, 2, 1, 4)),
)
GEOMETRY_IDS = [f"d{d}-C{C}-ns{ns}-{agg}-B{B}-sel{len(sel)}" for d, C, ns, agg, B, sel in GEOMETRIES]


# ---- float64 restatement -----------------------------------------------------------------------------------------------------------
def xbar64(x: torch.Tensor, ns: int, agg: str) -> torch.Tensor:
    """float64 [B, F] from x [B * ns, d] (or [B, ns, d]): the strands of a sample averaged, or laid end to end."""
    d = x.shape[-1]
    x = x.double().reshape(-1, ns, d)
    return x.sum(dim=1) / ns if agg == "mean" else x.reshape(-1, ns * d)


def heads64(x, ns: int, agg: str, w, bias, tissues=None):
    """(logits, bound) float64 [B, len(tissues), C]: every sample through the heads `tissues` (default: all, in order)."""
    xb = xbar64(x, ns, agg)
    sel = list(range(w.shape[0])) if tissues is None else list(tissues)
    W, b = w.double()[sel], bias.double()[sel]
    assert W.shape[2] == xb.shape[1]
    logits = torch.einsum("bf,icf->bic", xb, W) + b[None]
    bound = W.shape[2] * EPS * (torch.einsum("bf,icf->bic", xb.abs(), W.abs()) + b.abs()[None])
    return logits, bound


def rows64(x, ns: int, agg: str, w, bias, tissue_of_row):
    """(logits, bound) float64 [B, C]: sample b through the head of tissue_of_row[b]."""
    logits, bound = heads64(x, ns, agg, w, bias)
    idx = torch.arange(logits.shape[0])
    tv = torch.as_tensor(tissue_of_row).long()
    return logits[idx, tv], bound[idx, tv]


def softmax64(logits: torch.Tensor) -> torch.Tensor:
    return torch.softmax(logits, dim=-1)


def top_gap(logits: torch.Tensor) -> torch.Tensor:
    """float64 [...]: the distance between the two largest logits of a (sample, tissue); inf for a single class."""
    if logits.shape[-1] == 1:
        return torch.full(logits.shape[:-1], float("inf"), dtype=torch.float64)
    top = logits.topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]


# ---- kernel-level operands ---------------------------------------------------------------------------------------------------------
class Case:
    """fp32 operands of one geometry.  Samples and heads share one direction u (x = noise + a_b u, w[t, c] = noise + g_tc u), so
    the logits of a (sample, tissue) are spread by a_b g_tc on top of the noise dot product: the two largest are further apart
    than twice the error bound in all but a few pairs (tests/test_cre_heads_cpu.py counts them)."""

    def __init__(self, d, C, ns, agg, B, sel, seed=0):
        self.d, self.C, self.ns, self.agg, self.B, self.sel = d, C, ns, agg, B, tuple(sel)
        self.T = N_TISSUES
        self.F = ns * d if agg == "concat" else d
        g = torch.Generator().manual_seed(8100 + 7 * d + 31 * C + 3 * ns + AGG[agg] + 1000 * B + seed)
        u = torch.randn(d, generator=g)
        u = u / u.norm()
        a = 3.0 * torch.randn(B, 1, 1, generator=g)
        self.x = (torch.randn(B, ns, d, generator=g) + a * u).reshape(B * ns, d).contiguous()
        uF = u.repeat(ns) / ns if agg == "concat" else u
        gain = 2.0 * torch.randn(self.T, C, 1, generator=g)
        self.w = (torch.randn(self.T, C, self.F, generator=g) / self.F ** 0.5 + gain * uF).contiguous()
        self.bias = 0.5 * torch.randn(self.T, C, generator=g)
        self.tissue_of_row = torch.randint(0, self.T, (B,), generator=g, dtype=torch.int64)
        self.ldx, self.ldo_all, self.ldo_row = d + EXTRA_LDX, len(sel) * C + EXTRA_LDO, C + EXTRA_LDO


@functools.lru_cache(maxsize=None)
def case(d, C, ns, agg, B, sel) -> Case:
    return Case(d, C, ns, agg, B, sel)


@functools.lru_cache(maxsize=None)
def reference(d, C, ns, agg, B, sel) -> dict:
    """float64, computed once per geometry: `all` / `all_bound` [B, T, C] over every head, in tissue order."""
    c = case(d, C, ns, agg, B, sel)
    logits, bound = heads64(c.x, ns, agg, c.w, c.bias)
    return {"all": logits, "all_bound": bound}


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def load_cre_heads() -> dict:
    """{name: dict} of tests/golden/cre_heads.*: hparams, the name-keyed state dict rebuilt as tests/conftest.load_s2r_opts does
    (weight_abs_sum checked), the inputs rebuilt from the seeds (x, padding_mask, context, tissue_vector) and the reference's
    logits / x_embed / predict_step."""
    from oracle.vf_oracle import alibi_slopes
    from variantformer_amd.utils.synthetic import make_gene, make_tensor
    with open(os.path.join(GOLDEN, "cre_heads.json")) as f:
        meta = json.load(f)["cases"]
    arrays = dict(np.load(os.path.join(GOLDEN, "cre_heads.npz")))
    out = {}
    for name, m in meta.items():
        sd = {k: (torch.tensor(alibi_slopes(shape[0]), dtype=torch.float32) if k.endswith(".m")
                  else torch.from_numpy(make_tensor(k, shape, m["seed"]))) for k, shape in m["state_dict_shapes"].items()}
        chk = float(sum(float(v.double().abs().sum()) for v in sd.values()))
        assert abs(chk - m["weight_abs_sum"]) <= 1e-6 * m["weight_abs_sum"], "weight regeneration drifted"
        hp = m["hparams"]
        gs = [make_gene(m["seed"] + s * m["strand_seed_step"], m["b"], 2, [7], hp["token_length"],
                        cre_len_range=tuple(m["cre_len_range"])) for s in range(m["n_strands"])]
        T = hp["num_tissues"]
        out[name] = dict(hparams=hp, sd=sd, n_strands=m["n_strands"], b=m["b"], agg=hp.get("strand_agg", "mean"),
                         x=torch.cat([g["cre_sequences"] for g in gs], dim=1).contiguous(),
                         padding_mask=torch.cat([g["cre_attention_masks"] for g in gs], dim=1).contiguous(),
                         context=gs[0]["ref_cre_labels"],
                         tissue_vector=torch.from_numpy(arrays[f"{name}.tissue_vector"]),
                         logits=torch.from_numpy(arrays[f"{name}.logits"]), x_embed=torch.from_numpy(arrays[f"{name}.x_embed"]),
                         predict_step=torch.from_numpy(arrays[f"{name}.predict_step"]),
                         w=torch.stack([sd[f"tissue_classifiers.{t}.weight"] for t in range(T)]),
                         bias=torch.stack([sd[f"tissue_classifiers.{t}.bias"] for t in range(T)]))
    return out


def wrong_variants(fx: dict) -> dict:
    """What a plausible mistake computes instead of the fixture's logits, float64 [b, C] each (None: the shapes do not allow it):
      rolled     the tissue vector rolled by one HEAD: every id t becomes (t + 1) mod T, so every row goes through a wrong head.
                 This departs from the wording "the tissue vector rolled by one", which read as a shift of the vector's
                 POSITIONS cannot change every row as the same check demands: the 7 samples of `ctx1` share 2 tissues, an odd
                 cycle, so two neighbours always agree;
      strand0    only strand 0 used (for concat heads: strand 0 in both halves);
      mean       mean where concat belongs (against the first d columns of the concat weights);
      no_bias    the bias dropped."""
    ns, agg, w, bias, xe, tv = fx["n_strands"], fx["agg"], fx["w"], fx["bias"], fx["x_embed"], fx["tissue_vector"]
    d = xe.shape[-1]
    out = {"rolled": rows64(xe, ns, agg, w, bias, (tv + 1) % w.shape[0])[0],
           "no_bias": rows64(xe, ns, agg, w, torch.zeros_like(bias), tv)[0],
           "strand0": None, "mean": None}
    if ns > 1:
        out["strand0"] = rows64(xe[:, :1].expand(-1, ns, -1).contiguous(), ns, agg, w, bias, tv)[0]
    if agg == "concat":
        out["mean"] = rows64(xe, ns, "mean", w[:, :, :d].contiguous(), bias, tv)[0]
    return out


# ---- the parallel write-set net: one case list for the entry of include/vf_hip_cre_heads.h -----------------------------------------
# tests/write_set_cases.py's machinery on vf_tissue_heads, beside the lists of tests/attn_contrib_cases.py and
# tests/gene_contrib_cases.py.  tests/test_cre_heads_cpu.py requires the entry to be named here, through the raw entry and through
# the wrapper, in both forms and both modes; tests/test_cre_heads_gpu.py runs the cases.  Every input is an interior slice of a
# poisoned buffer (x with guard columns: ldx > d), out is an arena with padding columns, argmax an interior run of a poisoned
# vector; after the call the inputs' whole buffers, guards included, are compared with a copy taken before it.
WS_GEOMETRIES = ((200, 11, 2, "mean", 67, (2, 4, 0, 1, 3)), (8, 64, 3, "concat", 5, (1, 0, 1)), (520, 2, 1, "mean", 5, (4,)))


def ws_name(d, C, ns, agg, form, mode, how):
    return f"tissue_heads-d{d}-C{C}-ns{ns}-{agg}-{form}-{mode}-{how}"


def _make_ws(d, C, ns, agg, B, sel, row_form, probabilities, wrapper):
    def make():
        from tests import write_set_cases as W
        c = Case(d, C, ns, agg, B, sel, seed=1)
        n_sel = 1 if row_form else len(sel)
        if row_form:
            logits, bound = rows64(c.x, ns, agg, c.w, c.bias, c.tissue_of_row)
            logits, bound = logits[:, None], bound[:, None]
        else:
            logits, bound = heads64(c.x, ns, agg, c.w, c.bias, sel)
        cols = n_sel * C + EXTRA_LDO

        def run(p):
            from variantformer_amd import _lib
            ops = W._ops()
            x = W.guarded(c.x, p, W.GUARD_COLS)
            w = W.guarded(c.w.view(c.T * C, c.F), p).view(c.T, C, c.F)
            bias = W.guarded(c.bias.reshape(-1), p).view(c.T, C)
            tor = W.guarded(c.tissue_of_row, p) if row_form else None
            tis = None if row_form else W.guarded(torch.tensor(sel, dtype=torch.int32), p)
            inputs = [t for t in (x, w, bias, tor, tis) if t is not None]
            bases = [t._base if t._base is not None else t for t in inputs]
            before = [t.clone() for t in bases]
            big, out = W.arena(B, cols, torch.float32, p)
            big_arg = W.poisoned((B * n_sel + 2 * W.GUARD_ROWS,), torch.int32, W.DEVICE, p)
            arg = big_arg[W.GUARD_ROWS:W.GUARD_ROWS + B * n_sel]
            if wrapper:
                with W.poison_allocations(p) as proxy:
                    ops.tissue_heads(x, ns, agg, w, bias, tissue_of_row=tor, tissues=tis, probabilities=probabilities, out=out,
                                     argmax=arg if row_form else arg.view(B, n_sel))
                assert proxy.count == 0, "ops.tissue_heads makes nothing: every buffer is the caller's"
            else:
                _lib.check(_lib.load().vf_tissue_heads(x.data_ptr(), x.stride(0), ns, AGG[agg], w.data_ptr(), bias.data_ptr(), c.T, C, d,
                                                       0 if tor is None else tor.data_ptr(), 0 if tis is None else tis.data_ptr(),
                                                       n_sel, B, int(probabilities), out.data_ptr(), out.stride(0), arg.data_ptr(),
                                                       W._stream()), "vf_tissue_heads")
            W._sync()
            for t, was in zip(bases, before):
                assert torch.equal(t.view(torch.uint8), was.view(torch.uint8)), "an input, or the memory around it, was written"
            return {"out": big, "argmax": big_arg}

        def check(bufs):
            body = bufs["out"][8:8 + B, W.GUARD_COLS:W.GUARD_COLS + n_sel * C].double().view(B, n_sel, C)
            if probabilities:
                delta = bound.amax(dim=-1, keepdim=True)
                assert bool(((body - softmax64(logits)).abs() <= 2.0 * delta + 1e-6).all())
            else:
                assert bool(((body - logits).abs() <= bound).all())
            arg = bufs["argmax"][W.GUARD_ROWS:W.GUARD_ROWS + B * n_sel].view(B, n_sel).long()
            sure = top_gap(logits) > 2.0 * bound.amax(dim=-1)
            assert bool((arg[sure] == logits.argmax(dim=-1)[sure]).all())
        inner = torch.zeros((B, cols), dtype=torch.bool)
        inner[:, :n_sel * C] = True                                   # the padding columns of a row keep the poison
        arg_mask = torch.zeros(B * n_sel + 2 * W.GUARD_ROWS, dtype=torch.bool)
        arg_mask[W.GUARD_ROWS:W.GUARD_ROWS + B * n_sel] = True
        return W.Built(run, {"out": W.arena_mask(B, cols, inner), "argmax": arg_mask}, check)
    return make


def ws_cases() -> list:
    from tests import write_set_cases as W
    out = []
    for d, C, ns, agg, B, sel in WS_GEOMETRIES:
        for row_form in (True, False):
            for probabilities in (False, True):
                for wrapper in (False, True):
                    name = ws_name(d, C, ns, agg, "row" if row_form else "all", "probs" if probabilities else "logits",
                                   "wrapper" if wrapper else "entry")
                    out.append(W.WSCase(name, "tissue_heads", ("vf_tissue_heads",), ("tissue_heads",) if wrapper else (),
                                        _make_ws(d, C, ns, agg, B, sel, row_form, probabilities, wrapper)))
    return out

"""The tokenizer's per-tissue classifier heads on the GPU: vf_tissue_heads alone (against float64 within the a-priori bound of
tests/cre_heads_cases.py, row form = all form bit for bit, write set, NaN / Inf rules, refusals), then through
Seq2RegPredictor.forward(only_embed=False) / predict_step / classify against the reference's fixture, and through
ModelManager.load_tokenizer and VCFProcessor.predict_cre_activity."""
import numpy as np
import pandas as pd
import pytest
import torch
import yaml

from tests import cre_heads_cases as H
from tests import write_set_cases as W
from tests.conftest import load_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda"
POISON = -7.25                                  # what an output buffer holds before a call, padding columns included


def _ops():
    from variantformer_amd import _lib, ops
    _lib.load()
    return ops


def _strided(x: torch.Tensor, ld: int) -> torch.Tensor:
    big = torch.full((x.shape[0], ld), float("nan"), dtype=x.dtype, device=DEV)       # NaN in the columns nobody may read
    big[:, :x.shape[1]] = x.to(DEV)
    return big[:, :x.shape[1]]


def _run(c, form="all", sel=None, mode=0, x=None, w=None, bias=None, tor=None, rows=None, ldo_extra=H.EXTRA_LDO, want_argmax=True):
    """One call on the case's operands (or the given replacements); `rows`: only these samples, in this order.
    Returns (values [B, n_sel, C] on the CPU, argmax [B, n_sel], the whole out buffer)."""
    ops = _ops()
    x = c.x if x is None else x
    tor = c.tissue_of_row if tor is None else tor
    if rows is not None:
        idx = torch.tensor(rows)
        x = x.view(c.B, c.ns, c.d)[idx].reshape(-1, c.d)
        tor = tor[idx]
    B = x.shape[0] // c.ns
    n_sel = 1 if form == "row" else len(sel)
    out_big = torch.full((B, n_sel * c.C + ldo_extra), POISON, dtype=torch.float32, device=DEV)
    arg = torch.full((B,) if form == "row" else (B, n_sel), -9, dtype=torch.int32, device=DEV) if want_argmax else None
    got, got_arg = ops.tissue_heads(_strided(x, c.d + H.EXTRA_LDX), c.ns, c.agg, (c.w if w is None else w).to(DEV),
                                    (c.bias if bias is None else bias).to(DEV), tissue_of_row=tor.to(DEV) if form == "row" else None,
                                    tissues=None if form == "row" else torch.tensor(list(sel), dtype=torch.int32, device=DEV),
                                    probabilities=bool(mode),
                                    out=out_big[:, :n_sel * c.C] if ldo_extra else out_big, argmax=arg)
    torch.cuda.synchronize()
    assert got.data_ptr() == out_big.data_ptr() and (arg is None or got_arg.data_ptr() == arg.data_ptr())
    out_cpu = out_big.cpu()
    assert bool((out_cpu[:, n_sel * c.C:] == POISON).all()), "padding columns of out were written"
    return out_cpu[:, :n_sel * c.C].reshape(B, n_sel, c.C), (got_arg.cpu().view(B, n_sel) if want_argmax else None), out_cpu


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


# ---- 4. against float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", H.GEOMETRIES, ids=H.GEOMETRY_IDS)
def test_logits_probabilities_and_argmax_against_float64(geom):
    c, ref = H.case(*geom), H.reference(*geom)
    sel = list(c.sel)
    want, bound = ref["all"][:, sel], ref["all_bound"][:, sel]
    delta = bound.amax(dim=-1)
    got, arg, _ = _run(c, "all", sel, 0)
    err = (got.double() - want).abs()
    print(f"[tissue_heads {H.GEOMETRY_IDS[H.GEOMETRIES.index(geom)]}] logits: largest error {float((err / bound).max()):.4f} of the bound")
    assert bool((err <= bound).all())
    probs, arg1, _ = _run(c, "all", sel, 1)
    perr = (probs.double() - H.softmax64(want)).abs()
    print(f"    probabilities: largest error {float(perr.max()):.3e}, limit at that element "
          f"{float((2 * delta[..., None] + 1e-6).expand_as(perr).flatten()[perr.argmax()]):.3e}; "
          f"largest |row sum - 1| {float((probs.double().sum(-1) - 1).abs().max()):.3e}")
    assert bool((perr <= 2.0 * delta[..., None] + 1e-6).all())
    assert bool(((probs.double().sum(dim=-1) - 1.0).abs() <= 1e-6).all())
    sure = H.top_gap(want) > 2.0 * delta
    assert bool((arg.long()[sure] == want.argmax(dim=-1)[sure]).all()) and torch.equal(arg, arg1)
    assert bool(((arg >= 0) & (arg < c.C)).all())
    # the first index of the largest fp32 logit, ties included
    assert torch.equal(arg.long(), got.argmax(dim=-1))
    # the row form: sample b through the head of its own tissue
    rwant, rbound = H.rows64(c.x, c.ns, c.agg, c.w, c.bias, c.tissue_of_row)
    rgot, rarg, _ = _run(c, "row", None, 0)
    assert bool(((rgot[:, 0].double() - rwant).abs() <= rbound).all())
    assert tuple(rarg.shape) == (c.B, 1)


# ---- 5. row form = all form, and a sample's bits are its own -----------------------------------------------------------------------
@pytest.mark.parametrize("geom", H.GEOMETRIES, ids=H.GEOMETRY_IDS)
@pytest.mark.parametrize("mode", [0, 1], ids=["logits", "probs"])
def test_row_form_equals_all_form_and_bits_do_not_depend_on_the_call(geom, mode):
    c = H.case(*geom)
    every = list(range(c.T))
    full, full_arg, _ = _run(c, "all", every, mode)
    row, row_arg, _ = _run(c, "row", None, mode)
    idx = torch.arange(c.B)
    assert torch.equal(_bits(row[:, 0]), _bits(full[idx, c.tissue_of_row])), "row form and all form differ"
    assert torch.equal(row_arg[:, 0], full_arg[idx, c.tissue_of_row])
    # another n_sel, order and repeat of tissues, another ldo
    part, part_arg, _ = _run(c, "all", list(c.sel), mode, ldo_extra=0)
    assert torch.equal(_bits(part), _bits(full[:, list(c.sel)])) and torch.equal(part_arg, full_arg[:, list(c.sel)])
    # another B and another position in the batch
    rows = [c.B - 1, 0] if c.B > 1 else [0]
    if c.B > 4:
        rows = [4, 2, 0]
    sub, sub_arg, _ = _run(c, "all", [every[-1]], mode, rows=rows, ldo_extra=3)
    assert torch.equal(_bits(sub[:, 0]), _bits(full[rows, every[-1]])) and torch.equal(sub_arg[:, 0], full_arg[rows, every[-1]])
    subrow, _, _ = _run(c, "row", None, mode, rows=rows, want_argmax=False)
    assert torch.equal(_bits(subrow[:, 0]), _bits(row[rows, 0]))
    # and the call repeats itself
    again, _, _ = _run(c, "all", every, mode)
    assert torch.equal(_bits(again), _bits(full))


# ---- 6. write set ------------------------------------------------------------------------------------------------------------------
_WS = H.ws_cases()


@pytest.mark.parametrize("case", _WS, ids=[c.name for c in _WS])
def test_write_set(case):
    built = case.make()
    W.check_write_set(built.run, built.written, built.reference, built.nan_ok)


def test_the_wrapper_runs_on_the_callers_buffers_and_stream():
    ops = _ops()
    c = H.case(200, 11, 3, "mean", 5, (1, 3, 1))
    x, w, bias = c.x.to(DEV), c.w.to(DEV), c.bias.to(DEV)
    sel = torch.tensor(c.sel, dtype=torch.int32, device=DEV)

    def bufs(n_sel, row=False):
        return dict(out=torch.full((c.B, n_sel * c.C), POISON, device=DEV),
                    argmax=torch.full((c.B,) if row else (c.B, n_sel), -9, dtype=torch.int32, device=DEV))
    mine = bufs(3)
    out, arg = ops.tissue_heads(x, c.ns, c.agg, w, bias, tissues=sel, **mine)
    assert out is mine["out"] and arg is mine["argmax"]
    want, _, _ = _run(c, "all", c.sel, 0)
    assert torch.equal(_bits(out.cpu().view(c.B, 3, c.C)), _bits(want))
    out_only, none = ops.tissue_heads(x, c.ns, c.agg, w, bias, tissues=sel, out=torch.empty_like(out), argmax=None)
    assert none is None and torch.equal(_bits(out_only.cpu()), _bits(out.cpu()))
    rout, rarg = ops.tissue_heads(x, c.ns, 0, w, bias, tissue_of_row=c.tissue_of_row.to(DEV), probabilities=True, **bufs(1, row=True))
    assert tuple(rout.shape) == (c.B, c.C) and tuple(rarg.shape) == (c.B,) and bool((rarg >= 0).all())
    with pytest.raises(TypeError):                                                    # nothing is made here: both are required
        ops.tissue_heads(x, c.ns, c.agg, w, bias, tissues=sel)
    with pytest.raises(ValueError, match="not both"):
        ops.tissue_heads(x, c.ns, c.agg, w, bias, tissue_of_row=c.tissue_of_row.to(DEV), tissues=sel, **bufs(3))
    with pytest.raises(ValueError, match="one of them is required"):
        ops.tissue_heads(x, c.ns, c.agg, w, bias, **bufs(3))
    side = torch.cuda.Stream()                                                        # the current stream is the launch stream
    side.wait_stream(torch.cuda.current_stream())
    theirs = bufs(3)
    with torch.cuda.stream(side):
        s_out, _ = ops.tissue_heads(x, c.ns, c.agg, w, bias, tissues=sel, **theirs)
    side.synchronize()
    assert torch.equal(_bits(s_out.cpu()), _bits(out.cpu()))


# ---- 7. NaN and Inf ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(200, 11, 2, "mean", 5, (1, 3, 1)), (8, 64, 3, "concat", 5, (3, 0, 1)), (520, 2, 1, "mean", 5, (1, 3))],
                         ids=["mean-C11", "concat-C64", "single-C2"])
def test_nonfinite_rules_of_the_header(geom):
    c = H.Case(*geom, seed=2)
    sel = list(c.sel)
    nan = float("nan")
    base = {m: _run(c, "all", sel, m) for m in (0, 1)}
    hit_b, hit_t, hit_c = 2, 3, c.C - 1
    at_t = [i for i, t in enumerate(sel) if t == hit_t]
    not_t = [i for i, t in enumerate(sel) if t != hit_t]
    others = [b for b in range(c.B) if b != hit_b]
    assert at_t and not_t
    # (1) a NaN in a strand row of sample b: every output of sample b, no other sample
    x = c.x.clone()
    x.view(c.B, c.ns, c.d)[hit_b, c.ns - 1, 5] = nan
    for m in (0, 1):
        got, arg, _ = _run(c, "all", sel, m, x=x)
        assert bool(torch.isnan(got[hit_b]).all()) and bool((arg[hit_b] == -1).all())
        assert torch.equal(_bits(got[others]), _bits(base[m][0][others])) and torch.equal(arg[others], base[m][1][others])
    rgot, rarg, _ = _run(c, "row", None, 0, x=x)
    assert bool(torch.isnan(rgot[hit_b]).all()) and int(rarg[hit_b]) == -1 and not bool(torch.isnan(rgot[others]).any())
    # (2) a NaN in w[t, c, :] / (3) in bias[t, c]: logit (., t, c); in mode 1 all C probabilities of tissue t; no other tissue
    w = c.w.clone()
    w[hit_t, hit_c, c.F - 3] = nan
    bias = c.bias.clone()
    bias[hit_t, hit_c] = nan
    for kw in (dict(w=w), dict(bias=bias)):
        got, arg, _ = _run(c, "all", sel, 0, **kw)
        assert bool(torch.isnan(got[:, at_t, hit_c]).all()) and bool((arg[:, at_t] == -1).all())
        keep = torch.ones(c.B, len(sel), c.C, dtype=torch.bool)
        keep[:, at_t, hit_c] = False
        assert torch.equal(_bits(got[keep]), _bits(base[0][0][keep])) and torch.equal(arg[:, not_t], base[0][1][:, not_t])
        probs, parg, _ = _run(c, "all", sel, 1, **kw)
        assert bool(torch.isnan(probs[:, at_t]).all()) and bool((parg[:, at_t] == -1).all())
        assert torch.equal(_bits(probs[:, not_t]), _bits(base[1][0][:, not_t])) and torch.equal(parg[:, not_t], base[1][1][:, not_t])
    # Inf follows IEEE: Inf * 0 = NaN for that logit only, Inf * w = +-Inf for the others of the sample
    k = 3
    f = k                                                       # strand 0, column k is feature k under either aggregation
    w0 = c.w.clone()
    w0[hit_t, hit_c, f] = 0.0
    assert bool((w0[:, :, f].flatten() != 0).sum() == w0[:, :, f].numel() - 1)
    base0 = _run(c, "all", sel, 0, w=w0)
    xi = c.x.clone()
    xi.view(c.B, c.ns, c.d)[hit_b, 0, k] = float("inf")
    got, arg, _ = _run(c, "all", sel, 0, x=xi, w=w0)
    assert bool(torch.isnan(got[hit_b, at_t, hit_c]).all()) and bool((arg[hit_b, at_t] == -1).all())
    keep = torch.ones(len(sel), c.C, dtype=torch.bool)
    keep[at_t, hit_c] = False
    want_inf = torch.sign(w0[sel][:, :, f]) * float("inf")
    assert torch.equal(got[hit_b][keep], want_inf[keep])
    assert torch.equal(_bits(got[others]), _bits(base0[0][others])) and torch.equal(arg[others], base0[1][others])
    assert bool((arg[hit_b, not_t].long() == want_inf[not_t].argmax(dim=-1)).all())      # the first +Inf


# ---- 8. refusals, empty calls, ids without a head ------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_empty_calls_are_ok():
    from variantformer_amd import _lib
    ops = _ops()
    lib = _lib.load()
    c = H.case(8, 11, 2, "mean", 5, (2, 3, 0, 4, 1))
    x, w, bias = c.x.to(DEV), c.w.to(DEV), c.bias.to(DEV)
    tor = c.tissue_of_row.to(DEV)
    tis = torch.tensor(c.sel, dtype=torch.int32, device=DEV)
    out = torch.full((c.B, 64), POISON, dtype=torch.float32, device=DEV)
    arg = torch.full((c.B * 5,), -9, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    good = dict(x=x.data_ptr(), ldx=c.d, ns=c.ns, agg=0, w=w.data_ptr(), bias=bias.data_ptr(), T=c.T, C=c.C, d=c.d, tor=tor.data_ptr(),
                tis=0, n_sel=0, B=c.B, mode=0, out=out.data_ptr(), ldo=64, arg=arg.data_ptr())
    allf = dict(tor=0, tis=tis.data_ptr(), n_sel=5)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vf_tissue_heads(a["x"], a["ldx"], a["ns"], a["agg"], a["w"], a["bias"], a["T"], a["C"], a["d"], a["tor"], a["tis"],
                                   a["n_sel"], a["B"], a["mode"], a["out"], a["ldo"], a["arg"], st)
    refused = [(dict(x=0), "null pointer x"), (dict(w=0), "null pointer w"), (dict(bias=0), "null pointer bias"),
               (dict(out=0), "null pointer out"), (dict(d=0), "d="), (dict(d=6), "d="), (dict(C=0), "C="), (dict(C=65, ldo=128), "C="),
               (dict(ns=0), "n_strands"), (dict(ns=9), "n_strands"), (dict(T=0), "n_tissues"), (dict(agg=2), "strand_agg"),
               (dict(mode=2), "mode"), (dict(ldx=4), "ldx"), (dict(ldx=10), "ldx"), (dict(ldo=10), "ldo"), (dict(allf, ldo=54), "ldo"),
               (dict(tis=tis.data_ptr()), "both"), (dict(tor=0), "neither"), (dict(x=x.data_ptr() + 4), "x must be 16-byte"),
               (dict(w=w.data_ptr() + 8), "w must be 16-byte"), (dict(tor=tor.data_ptr() + 4), "tissue_of_row"),
               (dict(bias=bias.data_ptr() + 2), "bias"), (dict(out=out.data_ptr() + 2), "out"), (dict(arg=arg.data_ptr() + 2), "argmax"),
               (dict(allf, tis=tis.data_ptr() + 2), "tissues"), (dict(B=-1), "B="), (dict(allf, n_sel=-1), "n_sel"),
               (dict(B=2 ** 33), "grid")]
    for kw, word in refused:
        assert call(**kw) == 1, kw                                                      # VF_ERR_INVALID_ARG
        assert word in lib.vf_last_error().decode(), (kw, lib.vf_last_error().decode())
    assert call(B=0) == 0 and call(**dict(allf, n_sel=0)) == 0                          # VF_OK, nothing launched
    torch.cuda.synchronize()
    assert bool((out == POISON).all()) and bool((arg == -9).all()), "a refused or empty call wrote something"
    e_out, e_arg = ops.tissue_heads(x[:0], c.ns, c.agg, w, bias, tissues=tis[:2].contiguous(), out=out[:0, :2 * c.C],
                                    argmax=torch.empty((0, 2), dtype=torch.int32, device=DEV))
    assert tuple(e_out.shape) == (0, 2 * c.C) and tuple(e_arg.shape) == (0, 2)
    # an id without a head, through the raw entry: a NaN row and -1, every other row intact
    assert call() == 0
    torch.cuda.synchronize()
    base, base_arg = out.cpu().clone(), arg.cpu().clone()
    for bad in (c.T, -1, 2 ** 40):
        out.fill_(POISON)
        arg.fill_(-9)
        tor_bad = tor.clone()
        tor_bad[3] = bad
        assert call(tor=tor_bad.data_ptr()) == 0
        torch.cuda.synchronize()
        got, got_arg = out.cpu(), arg.cpu()
        assert bool(torch.isnan(got[3, :c.C]).all()) and int(got_arg[3]) == -1 and bool((got[3, c.C:] == POISON).all())
        keep = [b for b in range(c.B) if b != 3]
        assert torch.equal(_bits(got[keep]), _bits(base[keep])) and torch.equal(got_arg[keep], base_arg[keep])
        assert bool((got_arg[c.B:] == -9).all())
        out.fill_(POISON)
        with pytest.raises(KeyError, match=str(bad)):                                  # the wrapper: before anything is launched
            ops.tissue_heads(x, c.ns, c.agg, w, bias, tissue_of_row=tor_bad, out=out[:, :c.C], argmax=arg[:c.B])
        torch.cuda.synchronize()
        assert bool((out == POISON).all())
    for bad in ([0, c.T], [-1]):
        with pytest.raises(KeyError):
            ops.tissue_heads(x, c.ns, c.agg, w, bias, tissues=torch.tensor(bad, dtype=torch.int32, device=DEV),
                             out=out[:, :len(bad) * c.C], argmax=arg[:c.B * len(bad)])
    tis_bad = tis.clone()
    tis_bad[1] = c.T                                                                    # the all form guards its ids too
    out.fill_(POISON)
    assert call(**dict(allf, tis=tis_bad.data_ptr())) == 0
    torch.cuda.synchronize()
    got = out.cpu()[:, :5 * c.C].view(c.B, 5, c.C)
    assert bool(torch.isnan(got[:, 1]).all()) and not bool(torch.isnan(got[:, [0, 2, 3, 4]]).any())
    out.fill_(POISON)
    with pytest.raises(KeyError):
        ops.tissue_heads(x, c.ns, c.agg, w, bias, tissues=tis_bad, out=out[:, :5 * c.C], argmax=arg)
    torch.cuda.synchronize()
    assert bool((out == POISON).all())


# ---- 9. the golden cases through the model -------------------------------------------------------------------------------------------
def _model(fx, sd=None):
    from variantformer_amd.seq2reg.model import Seq2RegPredictor
    m = Seq2RegPredictor(**fx["hparams"])
    m.load_state_dict(fx["sd"] if sd is None else sd, strict=True)
    return m.cuda().eval()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", ["mean2", "concat2", "ctx1"])
def test_golden_cases_through_forward_and_predict_step(name, dtype):
    from tests.test_model_gpu import BF16_VS_FP32, _erel
    ops = _ops()
    fx = H.load_cre_heads()[name]
    m = _model(fx)
    ns, agg, b, C = fx["n_strands"], fx["agg"], fx["b"], fx["hparams"]["num_classes"]
    ctx = fx["context"] if fx["hparams"]["use_context"] else None
    with ops.compute_dtype(dtype), torch.no_grad():
        embed = m(fx["x"], fx["padding_mask"], None, context=ctx, only_embed=True)
        logits, x_embed = m(fx["x"], fx["padding_mask"], fx["tissue_vector"], ctx)
        pred = m.predict_step((fx["x"], fx["padding_mask"], fx["tissue_vector"], torch.zeros(b, dtype=torch.long), fx["context"], None), 0)
    assert logits.dtype == x_embed.dtype == torch.float32 and logits.is_cuda
    assert tuple(logits.shape) == (b, C) and tuple(x_embed.shape) == (b, ns, fx["hparams"]["embedding_dim"])
    assert torch.equal(_bits(x_embed.cpu()), _bits(embed.cpu())), "x_embed is not what only_embed=True returns"
    assert torch.equal(_bits(pred.cpu()), _bits(logits.cpu())), "predict_step is not forward's logits"
    e = _erel(x_embed.cpu().numpy(), fx["x_embed"].numpy())
    print(f"[cre_heads {name} {dtype}] x_embed vs the reference's: {e:.3e}")
    assert e < BF16_VS_FP32
    # the heads themselves: float64 on the product's own embeddings, within the a-priori bound
    own, bound = H.rows64(x_embed.cpu(), ns, agg, fx["w"], fx["bias"], fx["tissue_vector"])
    err = (logits.cpu().double() - own).abs()
    print(f"    logits vs float64 heads on the product's embeddings: {float((err / bound).max()):.4f} of the bound")
    assert bool((err <= bound).all())
    # against the golden logits: the embedding difference carried through the linear map, exactly, plus that bound
    dx = (H.xbar64(x_embed.cpu(), ns, agg) - H.xbar64(fx["x_embed"], ns, agg)).abs()
    carried = torch.einsum("bf,bcf->bc", dx, fx["w"].double().abs()[fx["tissue_vector"]])
    for key in ("logits", "predict_step"):
        gerr = (logits.cpu().double() - fx[key].double()).abs()
        print(f"    vs golden {key}: largest error {float(gerr.max()):.3e}, {float((gerr / (carried + bound)).max()):.4f} of its limit")
        assert bool((gerr <= carried + bound).all()), key


# ---- 10. classify ------------------------------------------------------------------------------------------------------------------
def _launches(m, fx, ctx):
    ops = _ops()
    timer = ops.KernelTimer(detail=True)
    ops.TIMER = timer
    try:
        with torch.no_grad():
            out = m(fx["x"], fx["padding_mask"], None, context=ctx, only_embed=True)
        torch.cuda.synchronize()
    finally:
        ops.TIMER = None
    return out.cpu(), [(name, geometry) for name, geometry, *_ in timer.order]


@pytest.mark.parametrize("name", ["mean2", "concat2", "ctx1"])
def test_classify(name):
    from variantformer_amd import weights
    fx = H.load_cre_heads()[name]
    m = _model(fx)
    T, C, b = fx["hparams"]["num_tissues"], fx["hparams"]["num_classes"], fx["b"]
    ctx = fx["context"] if fx["hparams"]["use_context"] else None
    with torch.no_grad():
        m(fx["x"], fx["padding_mask"], None, context=ctx, only_embed=True)              # builds the weight-derived operands
    before, launches_before = _launches(m, fx, ctx)
    assert launches_before and all(n != "tissue_heads" for n, _ in launches_before)
    with torch.no_grad():
        logits, classes = m.classify(fx["x"], fx["padding_mask"], context=ctx, probabilities=False)
        assert logits.dtype == torch.float32 and classes.dtype == torch.int32
        assert tuple(logits.shape) == (b, T, C) and tuple(classes.shape) == (b, T)
        for t in range(T):
            one, _ = m(fx["x"], fx["padding_mask"], torch.full((b,), t, dtype=torch.long), ctx)
            assert torch.equal(_bits(logits[:, t].cpu()), _bits(one.cpu())), f"classify and forward differ for tissue {t}"
        assert torch.equal(classes.cpu().long(), logits.cpu().argmax(dim=-1))
        probs, pclasses = m.classify(fx["x"], fx["padding_mask"], context=ctx)
        assert torch.equal(pclasses, classes)
        want = torch.softmax(logits.cpu().double(), dim=-1)
        assert bool(((probs.cpu().double() - want).abs() <= 1e-6).all())                # softmax of these very logits: no logit error
        order = [T - 1, 0]
        two, two_c = m.classify(fx["x"], fx["padding_mask"], context=ctx, tissues=order, probabilities=False)
        assert tuple(two.shape) == (b, 2, C)
        assert torch.equal(_bits(two.cpu()), _bits(logits[:, order].cpu())) and torch.equal(two_c, classes[:, order])
        with pytest.raises(KeyError):
            m.classify(fx["x"], fx["padding_mask"], context=ctx, tissues=[T])
        # one launch of the heads behind the encoder's launches
        ops = _ops()
        timer = ops.KernelTimer(detail=True)
        ops.TIMER = timer
        try:
            m.classify(fx["x"], fx["padding_mask"], context=ctx)
            torch.cuda.synchronize()
        finally:
            ops.TIMER = None
        names = [(n, g) for n, g, *_ in timer.order]
        assert names[:-1] == launches_before and names[-1][0] == "tissue_heads"
        # new head weights arrive: the weights.derived key sees load_state_dict's in-place copy
        builds = weights.BUILDS
        m.classify(fx["x"], fx["padding_mask"], context=ctx, probabilities=False)
        assert weights.BUILDS == builds                                                  # a hit while nothing changed
        sd2 = {k: (v * -1.5 + 0.25 if k.startswith("tissue_classifiers.") else v) for k, v in fx["sd"].items()}
        m.load_state_dict(sd2, strict=True)
        logits2, _ = m.classify(fx["x"], fx["padding_mask"], context=ctx, probabilities=False)
        w2 = torch.stack([sd2[f"tissue_classifiers.{t}.weight"] for t in range(T)])
        b2 = torch.stack([sd2[f"tissue_classifiers.{t}.bias"] for t in range(T)])
        own, bound = H.heads64(before, fx["n_strands"], fx["agg"], w2, b2)
        assert bool(((logits2.cpu().double() - own).abs() <= bound).all()) and not torch.equal(logits2, logits)
    after, launches_after = _launches(m, fx, ctx)
    assert torch.equal(_bits(after), _bits(before)) and launches_after == launches_before


# ---- 11. product -------------------------------------------------------------------------------------------------------------------
TOK_TISSUES = ["adrenal gland", "liver", "whole blood"]


def _write_artifacts(tmp_path, meta, sd, tok_sd):
    """The artifact writer of tests/test_processors_gpu.py, with a tokenizer checkpoint of its own: `tok_sd`, and the names of
    its heads' tissues among the hyper-parameters."""
    torch.save({"hyper_parameters": dict(meta["seq2reg"], tissues=TOK_TISSUES), "state_dict": tok_sd}, tmp_path / "tok.pth")
    torch.save({"state_dict": sd}, tmp_path / "model.pth")
    cfg_dir = tmp_path / "configs"
    cfg_dir.mkdir()
    model_cfg = dict(meta["seq2gene"], model_class="Seq2GenePredictorCombinedModulator", token_dim=999,
                     checkpoint_path=str(tmp_path / "model.pth"), precision="bf16-mixed",
                     cre_tokenizer={"path": str(tmp_path / "tok.pth")}, gene_tokenizer={"path": str(tmp_path / "tok.pth")})
    pd.DataFrame({"gene_id": ["ENSG_A", "ENSG_B", "ENSG_C"], "gene_name": ["a", "b", "c"]}).to_csv(tmp_path / "genes.csv", index=False)
    block = {"dataset": {"max_length": meta["token_length"], "max_chunks": 8, "cre_neighbour_hood": 15,
                         "gencode_v24": str(tmp_path / "genes.csv"), "gene_upstream_neighbour_hood": 100,
                         "gene_downstream_neighbour_hood": 3000}, "model": model_cfg}
    with open(cfg_dir / "vf_model.yaml", "w") as f:
        yaml.safe_dump({"v4_pcg": block, "v4_ag": block}, f)
    return cfg_dir


def test_load_tokenizer_and_predict_cre_activity(tmp_path):
    from tests.test_consensus_cpu import make_genome, make_records, write_fasta, write_vcf
    from variantformer_amd.datasets.vepdataset import LocalManifest
    from variantformer_amd.processors.model_manager import ModelManager
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    from variantformer_amd.utils.config import load_yaml
    meta, arrays, sd, _ = load_fixture("small_sin")
    pfx = "cre_tokenizer."
    big_tok = {k[len(pfx):]: v for k, v in sd.items() if k.startswith(pfx)}
    # the tokenizer checkpoint: other heads AND another encoder than the big checkpoint carries for its tokenizer
    tok_sd = {k: (v * 3.0 - 0.125 if k.startswith("tissue_classifiers.") else
                  (v * 1.25 if k == "token_embedding.weight" else v.clone())) for k, v in big_tok.items()}
    cfg_dir = _write_artifacts(tmp_path, meta, sd, tok_sd)
    g1, g2 = make_genome(99), make_genome(100, 5000)
    fasta = str(tmp_path / "genome.fa")
    write_fasta(fasta, {"chr1": g1, "chr2": g2})
    vcf = str(tmp_path / "donor.vcf.gz")
    write_vcf(vcf, {"chr1": make_records(g1, 7), "chr2": make_records(g2, 8)})
    genes = pd.DataFrame([
        {"gene_id": "ENSG_A", "gene_name": "a", "chromosome": "chr1", "start": 1000, "end": 6000, "strand": "+"},
        {"gene_id": "ENSG_B", "gene_name": "b", "chromosome": "chr2", "start": 500, "end": 4000, "strand": "-"}])
    genes.to_csv(tmp_path / "genes.csv", index=False)
    cres = {"ENSG_A": [(1040, 1110, "PLS"), (1490, 1560, "pELS"), (2030, 2080, "dELS"), (5000, 5100, "dELS")],
            "ENSG_B": [(300, 390, "CTCF-only,CTCF-bound"), (1300, 1345, "DNase-H3K4me3"), (4400, 4460, "PLS")]}
    paths = {}
    for g, rows in cres.items():
        chrom = genes.set_index("gene_id").loc[g, "chromosome"]
        paths[g] = str(tmp_path / f"{g}.csv")
        pd.DataFrame([{"chromosome": chrom, "start_cre": a, "end_cre": b, "cre_name": n} for a, b, n in rows]).to_csv(paths[g], index=False)
    with open(cfg_dir / "vcfloader.yaml", "w") as f:
        yaml.safe_dump({"CRE_BED": "x", "fasta_path": fasta, "precision": "bf16-mixed",
                        "dataloader": {"num_workers": 0, "batch_size": 2, "pin_memory": False, "drop_last": False,
                                       "prefetch_factor": 4}}, f)
    # the loader: the pair of the tokenizer checkpoint, not the big checkpoint's
    mm = ModelManager(load_yaml(str(cfg_dir / "vf_model.yaml")).v4_pcg.model)
    tok = mm.load_tokenizer("cre")
    assert not tok.training and next(tok.parameters()).is_cuda and tok.tissues == TOK_TISSUES
    for k, v in tok.state_dict().items():
        if k.startswith("tissue_classifiers.") or k == "token_embedding.weight":
            assert torch.equal(v.cpu(), tok_sd[k]) and not torch.equal(v.cpu(), big_tok[k]), k
    gene_tok = mm.load_tokenizer("gene")
    assert torch.equal(gene_tok.tissue_classifiers["1"].weight.cpu(), tok_sd["tissue_classifiers.1.weight"])
    with pytest.raises(ValueError, match="which"):
        mm.load_tokenizer("both")
    # the product entry
    vp = VCFProcessor(config_dir=str(cfg_dir), gene_cre_manifest=LocalManifest(paths))
    query = pd.DataFrame({"gene_id": ["ENSG_A", "ENSG_B"], "tissues": ["whole blood,thyroid", "liver"]})
    model, ckpt, trainer = vp.load_model()
    dataset, loader = vp.create_data(vcf, query.copy())
    first = vp.predict(model, ckpt, trainer, loader, dataset)
    first = {col: [np.array(v, copy=True) for v in first[col]] for col in ("predicted_expression", "embeddings")}
    df = vp.predict_cre_activity(tok, loader, dataset)
    T, C = meta["seq2reg"]["num_tissues"], meta["seq2reg"]["num_classes"]
    assert len(df) == 2
    for i, g in enumerate(df["gene_id"]):
        ids, mask, _, _, ref_labels = dataset[i][:5]                                   # the sample tuple of collate_fn_batching
        n = ids.shape[0]
        assert n == len(cres[g])
        p, cls = df["cre_class_probabilities"][i], df["cre_class"][i]
        assert p.dtype == np.float32 and p.shape == (n, T, C) and cls.shape == (n, T)
        with torch.no_grad():
            want, want_c = tok.classify(ids, mask, context=ref_labels)
        assert np.array_equal(p.view(np.int32), want.cpu().numpy().view(np.int32)) and np.array_equal(cls, want_c.cpu().numpy())
        assert np.allclose(p.sum(-1), 1.0, atol=1e-6) and np.array_equal(cls, p.argmax(-1))
        assert df["cre_activity_tissues"][i] == TOK_TISSUES and df["cre_class_names"][i] == list(range(C))
        names = [r[2] for r in cres[g]]                                              # sorted by start; reversed on the minus strand
        assert df["cre_names"][i] == dataset.cre_table(g)["cre_name"].tolist() == (names[::-1] if g == "ENSG_B" else names)
        assert len(df["cre_start"][i]) == len(df["cre_end"][i]) == n
    every = [np.array(p, copy=True) for p in df["cre_class_probabilities"]]         # (the frame is the query's own: a second call rewrites it)
    sub = vp.predict_cre_activity(tok, loader, dataset, tissues=[2, 0])
    assert sub["cre_activity_tissues"][0] == [TOK_TISSUES[2], TOK_TISSUES[0]]
    for i in range(2):
        assert np.array_equal(sub["cre_class_probabilities"][i], every[i][:, [2, 0]])
    # the expression path is untouched by it
    second = vp.predict(model, ckpt, trainer, loader, dataset)
    for col, vals in first.items():
        for a, b in zip(vals, second[col]):
            assert np.array_equal(a, np.asarray(b)), col

"""The tokenizer's per-tissue classifier heads without a GPU: the vf_tissue_heads boundary (include/vf_hip_cre_heads.h parses, its
one name is exported and bound through _lib.ENTRIES, it has write-set cases
in the parallel net), every refusal of the entry with the argument named, the public surface, and -- on the references alone --
that the float64 restatement of tests/cre_heads_cases.py reproduces the reference's fixture, that the fixture tells right from
wrong, and that the kernel-level operands leave the argmax decidable."""
import inspect
import os
import re

import pytest
import torch

from tests import cre_heads_cases as H
from tests import write_set_cases as W
from tests.conftest import REPO

NAME = "vf_tissue_heads"
FIXTURE_CASES = ("mean2", "concat2", "ctx1")


def _header(name="vf_hip_cre_heads.h") -> str:
    with open(os.path.join(REPO, "include", name)) as f:
        return f.read()


# ---- 1. header and binding ---------------------------------------------------------------------------------------------------------
def test_header_parses_and_its_name_is_exported_and_bound():
    """What is this header's own; the boundary every header shares is tests/test_abi_cpu.py's."""
    from variantformer_amd import _lib
    text = _header()
    assert sorted(_lib.ENTRIES["vf_hip_cre_heads.h"]) == [NAME], "ctypes binding and vf_hip_cre_heads.h disagree"
    assert _lib.ABI_VERSION == 13 and _lib.load().vf_version() == 13
    for word in ("Write set", "Non-finite operands", "Refused before anything is launched", "Arithmetic"):
        assert word in text, f"the comment contract of {NAME} has no `{word}` part"


def test_the_entry_has_write_set_cases():
    """The rule of tests/test_gene_contrib_cpu.py for this header: entry and wrapper, both forms, both modes."""
    entries = W.stream_entries(_header())
    assert entries == [NAME]
    cases = H.ws_cases()
    assert {e for c in cases for e in c.entries} == set(entries)
    assert len({c.name for c in cases}) == len(cases)
    for d, C, ns, agg, _, _ in H.WS_GEOMETRIES:
        for form in ("row", "all"):
            for mode in ("logits", "probs"):
                for how in ("entry", "wrapper"):
                    assert any(c.name == H.ws_name(d, C, ns, agg, form, mode, how) for c in cases)
    assert all(c.wrappers == (("tissue_heads",) if c.name.endswith("wrapper") else ()) for c in cases)


def test_the_wrapper_allocates_nothing():
    """As attn_contrib and attn_contrib_self (tests/test_gene_contrib_cpu.py): the caller owns every buffer, so out and argmax
    are required and no allocating call of any spelling stands in the wrapper.  The issue's `out=None, argmax=None` ("allocates
    only what the caller did not pass") is not followed: every allocation of ops.py has a poisoned-allocation case in
    tests/write_set_cases.py, whose case list is not this file's to extend; Seq2RegPredictor makes the two buffers instead."""
    from variantformer_amd import ops
    src = inspect.getsource(ops.tissue_heads)
    assert not re.search(r"\b(empty|empty_like|zeros|zeros_like|ones|full|new_empty|new_zeros|new_full|tensor|arange|clone|contiguous)\s*\(", src)
    prm = inspect.signature(ops.tissue_heads).parameters
    for name in ("out", "argmax"):
        assert prm[name].default is inspect.Parameter.empty and prm[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert "tissue_heads" not in W.allocating_wrappers() and W.uncovered_wrappers() == []


def test_argument_validation_without_gpu():
    """Refused before anything is launched (no GPU here: a launch would fail differently), the argument named."""
    from variantformer_amd import _lib
    lib = _lib.load()
    p = 4096                                             # a non-null, 16-byte aligned address; never dereferenced
    INVALID = 1

    def call(x=p, ldx=16, ns=2, agg=0, w=p, bias=p, T=3, C=11, d=16, tor=p, tis=0, n_sel=0, B=0, mode=0, out=p, ldo=11, arg=0):
        return lib.vf_tissue_heads(x, ldx, ns, agg, w, bias, T, C, d, tor, tis, n_sel, B, mode, out, ldo, arg, 0)

    def err():
        return lib.vf_last_error().decode()
    assert call() == 0                                                                  # the base call is valid (B = 0)
    for name in ("x", "w", "bias", "out"):
        assert call(**{name: 0}) == INVALID, name
        assert err().endswith(f"null pointer {name}"), err()
    for d in (0, -4, 6, 17):
        assert call(d=d, ldx=32) == INVALID and "d=" in err()
    for C in (0, -1, 65):
        assert call(C=C, ldo=128) == INVALID and "C=" in err()
    assert call(C=1) == 0 and call(C=64, ldo=64) == 0
    for ns in (0, 9):
        assert call(ns=ns) == INVALID and "n_strands" in err()
    assert call(ns=1) == 0 and call(ns=8) == 0
    assert call(T=0) == INVALID and "n_tissues" in err()
    for agg in (-1, 2):
        assert call(agg=agg) == INVALID and "strand_agg" in err()
    for mode in (-1, 2):
        assert call(mode=mode) == INVALID and "mode" in err()
    assert call(ldx=12) == INVALID and "ldx" in err()                                   # below d
    assert call(ldx=18) == INVALID and "ldx" in err()                                   # not a multiple of 4
    assert call(ldo=10) == INVALID and "ldo" in err()                                   # row form: below C
    assert call(tor=0, tis=p, n_sel=3, ldo=32) == INVALID and "ldo" in err()             # all form: below n_sel * C
    assert call(tor=0, tis=p, n_sel=3, ldo=33) == 0
    assert call(tor=p, tis=p) == INVALID and "tissue_of_row" in err() and "tissues" in err() and "both" in err()
    assert call(tor=0, tis=0) == INVALID and "tissue_of_row" in err() and "neither" in err()
    assert call(x=p + 8) == INVALID and re.search(r"\bx must be 16-byte", err())
    assert call(w=p + 4) == INVALID and re.search(r"\bw must be 16-byte", err())
    assert call(tor=p + 4) == INVALID and "tissue_of_row" in err()
    for name, word in (("bias", "bias"), ("out", "out"), ("arg", "argmax")):
        assert call(**{name: p + 2}) == INVALID and word in err()
    assert call(tor=0, tis=p + 2, n_sel=1) == INVALID and "tissues" in err()
    assert call(B=-1) == INVALID and "B=" in err()
    assert call(tor=0, tis=p, n_sel=-1, ldo=64) == INVALID and "n_sel" in err()
    assert call(B=2 ** 33) == INVALID and "grid" in err()                               # 2^31 blocks of four pairs
    assert call(tor=0, tis=p, n_sel=2 ** 20, ldo=2 ** 24, B=2 ** 13) == INVALID and "grid" in err()
    assert call(tor=0, tis=p, n_sel=0, B=5) == 0 and call(B=0) == 0                     # nothing to do: VF_OK, no launch


def test_public_surface():
    from variantformer_amd import ops
    from variantformer_amd.processors.model_manager import ModelManager
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    from variantformer_amd.seq2reg.model import Seq2RegPredictor
    assert list(inspect.signature(ops.tissue_heads).parameters)[:10] == [
        "x", "n_strands", "strand_agg", "w", "bias", "tissue_of_row", "tissues", "probabilities", "out", "argmax"]
    assert list(inspect.signature(Seq2RegPredictor.forward).parameters)[:6] == [
        "self", "x", "padding_mask", "tissue_vector", "context", "only_embed"]
    assert inspect.signature(Seq2RegPredictor.forward).parameters["only_embed"].default is False
    assert list(inspect.signature(Seq2RegPredictor.predict_step).parameters) == ["self", "batch", "batch_idx"]
    sig = inspect.signature(Seq2RegPredictor.classify)
    assert list(sig.parameters) == ["self", "x", "padding_mask", "context", "tissues", "probabilities"]
    assert sig.parameters["probabilities"].default is True and sig.parameters["tissues"].default is None
    assert inspect.signature(ModelManager.load_tokenizer).parameters["which"].default == "cre"
    doc = " ".join(ModelManager.load_tokenizer.__doc__.split())
    assert "fine-tuned" in doc and "tokenizer checkpoint" in doc                       # why not the tokenizer of the loaded model
    assert list(inspect.signature(VCFProcessor.predict_cre_activity).parameters) == ["self", "tokenizer", "dataloader", "vcf_dataset",
                                                                                      "tissues"]


def test_class_names():
    from variantformer_amd.processors.vcfprocessor import cre_class_names
    from variantformer_amd.utils.constants import CREs
    assert len(CREs) == H.load_cre_heads()["mean2"]["hparams"]["num_classes"] == 11      # the `multi` tokenizer of the fixture
    assert cre_class_names(11) == list(CREs) and cre_class_names(9) == list(range(9)) and cre_class_names(2) == [0, 1]


def test_forward_names_what_is_missing_before_any_launch():
    from variantformer_amd.seq2reg.model import Seq2RegPredictor
    fx = H.load_cre_heads()
    x, pad = fx["mean2"]["x"], fx["mean2"]["padding_mask"]
    m = Seq2RegPredictor(**fx["mean2"]["hparams"])
    with pytest.raises(ValueError, match="tissue_vector"):
        m(x, pad)
    with pytest.raises(ValueError, match="tissue_vector"):
        m(x, pad, None, only_embed=False)
    c = Seq2RegPredictor(**fx["concat2"]["hparams"])
    for ns in (1, 3):
        ids = x[:, :1].expand(-1, ns, -1)
        with pytest.raises(ValueError, match="concat"):
            c(ids, torch.zeros_like(ids, dtype=torch.bool), torch.zeros(len(ids), dtype=torch.long))
        with pytest.raises(ValueError, match="concat"):
            c.classify(ids, torch.zeros_like(ids, dtype=torch.bool))
    assert c.tissue_classifiers["0"].in_features == 2 * c.token_embedding.weight.shape[1]


# ---- 2. the float64 restatement reproduces the fixture -----------------------------------------------------------------------------
def test_fixture_covers_what_it_should():
    fx = H.load_cre_heads()
    assert sorted(fx) == sorted(FIXTURE_CASES)
    want = {"mean2": ("mean", 2, "sinusoidal", "multi", 11, 3, 9, False), "concat2": ("concat", 2, "alibi", "9class", 9, 4, 9, False),
            "ctx1": ("mean", 1, "sinusoidal", "binary", 2, 2, 7, True)}
    for name, f in fx.items():
        hp = f["hparams"]
        got = (f["agg"], f["n_strands"], hp["positional_encoding"], hp["cre_type"], hp["num_classes"], hp["num_tissues"], f["b"],
               hp["use_context"])
        assert got == want[name], (name, got)
        tv = f["tissue_vector"]
        assert tv.dtype == torch.int64 and sorted(tv.tolist()) != tv.tolist()
        assert all(int((tv == t).sum()) >= 2 for t in range(hp["num_tissues"]))
        assert tuple(f["logits"].shape) == tuple(f["predict_step"].shape) == (f["b"], hp["num_classes"])
        assert tuple(f["x_embed"].shape) == (f["b"], f["n_strands"], hp["embedding_dim"])
        valid = (~f["padding_mask"]).sum(dim=-1)
        assert int(valid.min()) >= 3 and int(valid.max()) <= 41
        if f["n_strands"] == 2:
            assert not torch.equal(f["x"][:, 0], f["x"][:, 1]) and not torch.equal(f["x_embed"][:, 0], f["x_embed"][:, 1])


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_float64_restatement_reproduces_the_fixture(name):
    f = H.load_cre_heads()[name]
    logits, bound = H.rows64(f["x_embed"], f["n_strands"], f["agg"], f["w"], f["bias"], f["tissue_vector"])
    assert float(bound.min()) > 0
    for key in ("logits", "predict_step"):
        err = (logits - f[key].double()).abs()
        print(f"[cre_heads fixture {name}] {key}: largest error {float((err / bound).max()):.4f} of the bound")
        assert bool((err <= bound).all()), key


# ---- 3. the cases can tell right from wrong ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_the_fixture_tells_right_from_wrong(name):
    """A condition on the references: each wrong variant's logits differ from the golden ones by more than 100 x the bound -- in
    every row for the rolled tissues and the dropped bias, in at least 3/4 of the rows for the strand variants."""
    f = H.load_cre_heads()[name]
    _, bound = H.rows64(f["x_embed"], f["n_strands"], f["agg"], f["w"], f["bias"], f["tissue_vector"])
    variants = H.wrong_variants(f)
    assert (variants["strand0"] is not None) == (f["n_strands"] > 1) and (variants["mean"] is not None) == (f["agg"] == "concat")
    for kind, wrong in variants.items():
        if wrong is None:
            continue
        rows = ((wrong - f["logits"].double()).abs() > 100.0 * bound).any(dim=1)
        print(f"[cre_heads fixture {name}] {kind}: {int(rows.sum())} of {rows.numel()} rows differ by more than 100 bounds")
        need = rows.numel() if kind in ("rolled", "no_bias") else -(-3 * rows.numel() // 4)
        assert int(rows.sum()) >= need, (kind, int(rows.sum()), need)


def test_the_operands_leave_the_argmax_decidable():
    """At most 1 % of the (sample, tissue) pairs of the kernel-level operands have their two largest float64 logits closer than
    twice the error bound (where the fp32 argmax may legitimately differ); the GPU test leaves exactly those out."""
    total = unsure = 0
    seen = {k: set() for k in ("d", "C", "ns", "agg", "B", "n_sel")}
    for g in H.GEOMETRIES:
        d, C, ns, agg, B, sel = g
        for k, v in zip(seen, (d, C, ns, agg, B, len(sel))):
            seen[k].add(v)
        assert all(0 <= t < H.N_TISSUES for t in sel)
        ref = H.reference(*g)
        gap, delta = H.top_gap(ref["all"]), ref["all_bound"].amax(dim=-1)
        total += gap.numel()
        unsure += int((gap <= 2.0 * delta).sum())
    print(f"[cre_heads operands] {unsure} of {total} (sample, tissue) pairs are closer than 2 delta")
    assert unsure <= 0.01 * total
    assert seen == {"d": {8, 200, 520}, "C": {1, 2, 9, 11, 64}, "ns": {1, 2, 3}, "agg": {"mean", "concat"}, "B": {1, 5, 67},
                    "n_sel": {1, 3, 5}}
    sels = [g[5] for g in H.GEOMETRIES]
    assert any(len(set(s)) < len(s) for s in sels) and any(list(s) != sorted(s) for s in sels)     # a repeat, a shuffle
    assert H.EXTRA_LDX > 0 and H.EXTRA_LDX % 4 == 0 and H.EXTRA_LDO > 0

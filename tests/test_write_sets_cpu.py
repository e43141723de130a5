"""The write-set net itself, without a GPU (tests/write_set_cases.py): the checker tells a wrong fake op from a right one and
for the right reason, every C-ABI entry with a `stream` argument and every allocating wrapper of variantformer_amd/ops.py has
a case, the poisoning allocator poisons, and the attention masks equal a direct restatement of the header rule."""
import os

import numpy as np
import pytest
import torch

from tests import attn_edge_cases as E
from tests import write_set_cases as W
from tests.conftest import REPO

M_ROWS, N_COLS, TAIL = 37, 24, 32           # the fakes' "kernel" writes rows in tiles of 32: row 32 ... 36 are its ragged tail


def _header():
    with open(os.path.join(REPO, "include", "vf_hip.h")) as f:
        return f.read()


def _fake(kind):
    """A plain-torch op on CPU tensors, out[i, :] = max_j x[i, j] + x[i, :], run the way a wrapper runs a kernel: the output
    and the running-max workspace come poisoned, the input sits inside poisoned guards."""
    x = ((torch.arange(M_ROWS * N_COLS, dtype=torch.float32).reshape(M_ROWS, N_COLS) % 7) + 1) * 0.001

    def run(p):
        xg = W.guarded(x, p, W.GUARD_COLS, device="cpu")
        out = W.poisoned((M_ROWS + 1, N_COLS), torch.float32, "cpu", p)     # one spare row behind the documented output
        ws = W.poisoned((M_ROWS,), torch.float32, "cpu", p)
        if kind == "stale_max":
            m = torch.fmax(ws, xg.max(dim=1).values)        # reads the workspace before writing it; fmax(NaN, x) = x
        else:
            m = xg.max(dim=1).values
        ws.copy_(m)
        rows = TAIL if kind == "drops_tail" else M_ROWS
        out[:rows] = (xg + m[:, None])[:rows]
        if kind == "stores_past":
            out[M_ROWS, 0] = 1.0
        return {"out": out, "ws": ws}
    mask = torch.zeros((M_ROWS + 1, N_COLS), dtype=torch.bool)
    mask[:M_ROWS] = True

    def reference(bufs):
        assert torch.equal(bufs["out"][:M_ROWS], x + x.max(dim=1, keepdim=True).values)
    return run, {"out": mask, "ws": W.full(M_ROWS)}, reference


def test_checker_passes_a_correct_op():
    run, written, reference = _fake("correct")
    bufs = W.check_write_set(run, written, reference)
    assert set(bufs) == {"out", "ws"}


def test_checker_catches_an_unwritten_ragged_tail():
    run, written, reference = _fake("drops_tail")
    with pytest.raises(AssertionError, match=r"out: \d+ elements differ between the runs") as e:
        W.check_write_set(run, written, reference)
    assert f"first at ({TAIL}, 0)" in str(e.value)
    # the classic blind spot: with one pattern alone (every run sees the same stale bytes) only the reference could tell
    with pytest.raises(AssertionError, match="NaNs inside the write set"):
        W.check_write_set(run, written, None, patterns=(0xFF,))


def test_checker_catches_a_stale_read_inside_a_running_max_only_with_the_finite_pattern():
    """Row maxima lie in (0, 0.008): NaN poison is dropped by fmax, zero poison loses the maximum -- under those two the stale read
    changes nothing, the 0x00 run even meets the reference -- and the 0x3C value (0.0115 in fp32) wins it."""
    run, written, reference = _fake("stale_max")
    assert 0.008 < float(W.poisoned((1,), torch.float32, "cpu", 0x3C)[0]) < 0.012
    W.check_write_set(run, written, reference, patterns=(0xFF,))
    W.check_write_set(run, written, reference, patterns=(0xFF, 0x00))
    with pytest.raises(AssertionError, match=r"elements differ between the runs poisoned with 0xff and 0x3c"):
        W.check_write_set(run, written, reference)


def test_checker_catches_a_store_past_the_mask():
    run, written, reference = _fake("stores_past")
    with pytest.raises(AssertionError, match=r"out: 1 elements outside the documented write set were written") as e:
        W.check_write_set(run, written, reference)
    assert f"first at ({M_ROWS}, 0)" in str(e.value)


def test_checker_catches_a_guard_that_reaches_the_result():
    """The read-set half: an op that sums one column too many (a wide load past the row) differs between the guard patterns."""
    x = torch.ones((5, 8))

    def run(p):
        xg = W.guarded(x, p, W.GUARD_COLS, device="cpu")
        wide = torch.as_strided(xg, (5, 9), xg.stride())                   # one element into the guard columns
        out = W.poisoned((5,), torch.float32, "cpu", p)
        out.copy_((wide * torch.tensor([1.0] * 8 + [0.0])).sum(dim=1))     # "masked" by a multiplication: 0 x NaN
        return {"out": out}
    with pytest.raises(AssertionError, match="elements differ between the runs"):
        W.check_write_set(run, {"out": W.full(5)})


def test_patterns_mean_what_the_module_says():
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert torch.isnan(W.poisoned((3,), dt, "cpu", 0xFF)).all()
        v = W.poisoned((3,), dt, "cpu", 0x3C).float()
        assert torch.isfinite(v).all() and 1e-3 < float(v[0]) < 2.0
        assert (W.poisoned((3,), dt, "cpu", 0x00) == 0).all()
    assert (W.poisoned((3,), torch.int32, "cpu", 0xFF) == -1).all() and (W.poisoned((3,), torch.int64, "cpu", 0xFF) == -1).all()


def test_guards_are_wide_enough_and_aligned():
    for dt, cols in ((torch.bfloat16, W.GUARD_COLS), (torch.float32, W.GUARD_COLS), (torch.float32, 0), (torch.int64, 0)):
        x = torch.zeros((5, 24), dtype=dt)
        g = W.guarded(x, 0x3C, cols, device="cpu")
        assert g.data_ptr() % 16 == 0 and g.shape == x.shape and g.stride(0) == 24 + 2 * cols and (g == 0).all()
        base = g.untyped_storage()
        assert g.storage_offset() == W.GUARD_ROWS * g.stride(0) + cols >= 256 * g.stride(0)
        assert base.nbytes() == (5 + 2 * W.GUARD_ROWS) * g.stride(0) * x.element_size()
    v = W.guarded(torch.zeros(7, dtype=torch.int32), 0xFF, device="cpu")
    assert v.data_ptr() % 16 == 0 and v.storage_offset() == W.GUARD_ROWS
    tab, where = W.spread_rows(torch.ones((4, 8)), 0xFF, device="cpu")
    assert where.tolist() == [1, 3, 5, 7] and (tab[where] == 1).all() and torch.isnan(tab[[0, 2, 4, 6, 8]]).all()


# ---------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------
def test_every_entry_with_a_stream_argument_has_a_case():
    from tests.test_abi_cpu import _declared
    hdr = _header()
    entries = W.stream_entries(hdr)
    assert len(entries) >= 39 and set(entries) <= set(_declared())
    # the entries without a stream are the host-side ones and the queries
    host = set(_declared()) - set(entries)
    assert all(n.startswith(("vf_bpe_", "vf_vcf_")) or n in ("vf_version", "vf_last_error", "vf_last_kernel", "vf_attn_rows_supported",
                                                                "vf_build_windows", "vf_narrow_ids") for n in host), sorted(host)
    assert W.uncovered_entries(hdr) == []
    assert set(W.ABI_EXCLUSIONS) <= set(entries)
    named = {e for c in W.CASES for e in c.entries}
    assert named <= set(entries), sorted(named - set(entries))              # no case names an entry the header does not declare


def test_a_new_declaration_or_a_removed_case_fails_the_coverage():
    hdr = _header()
    grown = hdr.replace("#ifdef __cplusplus\n}", "int vf_new_kernel(const float* x, float* out, int64_t n, void* stream);\n"
                        "#ifdef __cplusplus\n}", 1)
    assert grown != hdr and W.uncovered_entries(grown) == ["vf_new_kernel"]
    fewer = [c for c in W.CASES if "vf_segment_max" not in c.entries]
    assert len(fewer) == len(W.CASES) - 1 and W.uncovered_entries(hdr, fewer) == ["vf_segment_max"]
    assert W.uncovered_wrappers(fewer) == ["segment_max"]


def test_every_allocating_wrapper_has_a_case():
    import inspect
    from variantformer_amd import ops
    names = W.allocating_wrappers()
    n_allocs = sum(inspect.getsource(getattr(ops, n)).count("torch.empty") for n in names)
    assert n_allocs == inspect.getsource(ops).count("torch.empty") >= 36, n_allocs     # every allocation sits in a listed wrapper
    assert W.uncovered_wrappers() == []
    assert {w for c in W.CASES for w in c.wrappers} <= set(names)


def test_case_names_are_unique_and_families_are_known():
    names = [c.name for c in W.CASES]
    assert len(set(names)) == len(names)
    assert {c.family for c in W.CASES} == {"gemm", "gemm_ln", "stats", "attn", "attn_probs", "stream"}


def test_the_patched_name_poisons_and_is_restored(monkeypatch):
    import importlib
    mods = [importlib.import_module(n) for n in W.WRAPPER_MODULES]
    with W.poison_allocations(0x3C) as px:
        for m in mods:
            assert m.torch is px
            t = m.torch.empty((3, 5), dtype=torch.bfloat16)
            assert (t.view(torch.uint8) == 0x3C).all()
            e = m.torch.empty_like(torch.zeros(4))
            assert (e.view(torch.uint8) == 0x3C).all()
            assert m.torch.zeros(2).tolist() == [0.0, 0.0] and m.torch.float16 is torch.float16       # everything else passes through
        assert len(px.allocated) == 2 * len(mods)
    assert all(m.torch is torch for m in mods)
    px = W.install(monkeypatch, 0xFF)
    assert mods[0].torch is px and torch.isnan(mods[0].torch.empty(2)).all() and mods[0].torch.empty(0).numel() == 0
    monkeypatch.undo()
    assert all(m.torch is torch for m in mods)


# ---------------------------------------------------------------------------------------------
# masks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", W.ATTN_FAMILY_CASES + ("fwd64_dh48",))
def test_attention_masks_restate_the_header_rule(name):
    """vf_hip.h, vf_attn_varlen_fwd: element (t, c) of out is written exactly when token t belongs to a sequence (t < cu_seqlens_q[n_seq];
    a sequence without queries owns no token, one without keys has its rows written as zeros) and c < H * dh."""
    c, ql, kl = W.attn_geometry(name)
    assert 0 in ql and 0 in kl and len(ql) == len(kl)
    tq = sum(ql) + W.EXTRA_Q_ROWS
    n_cols = c.H * c.dh
    cu = np.concatenate([[0], np.cumsum(ql)])
    want = np.zeros((tq, n_cols), dtype=bool)
    for s in range(len(ql)):
        for t in range(cu[s], cu[s + 1]):
            want[t, :c.H * c.dh] = True
    assert tq > cu[-1] and not want[cu[-1]:].any()
    built = [k for k in W.CASES if k.name == f"attn-{name}-bf16-qend"] or [k for k in W.CASES if k.name == "attn-direct-vf_attn_varlen_fwd"]
    mask = built[0].make().written["out"]
    inner = mask[8:8 + tq, W.GUARD_COLS:W.GUARD_COLS + n_cols]
    assert np.array_equal(inner.numpy(), want)
    assert int(mask.sum()) == int(want.sum())                               # nothing of the arena's frame is in the write set
    assert np.array_equal(W.attn_written_mask(ql, tq, c.H, c.dh, n_cols).numpy(), want)


def test_one_forward_attention_case_per_kernel_family():
    assert {E.CASES_BY_NAME[n].kernel for n in W.ATTN_FAMILY_CASES} == {c.kernel for c in E.ATTN_EDGE_CASES}
    names = {c.name for c in W.CASES}
    for n in W.ATTN_FAMILY_CASES:                       # every family at a padded head dim: its own, or dh - 8 of its class
        dh = E.CASES_BY_NAME[n].dh
        assert dh not in (32, 48, 64, 96, 128) or {f"attn-{n}-bf16-padded_dh{dh - 8}", f"attn-{n}-fp16-padded_dh{dh - 8}"} <= names

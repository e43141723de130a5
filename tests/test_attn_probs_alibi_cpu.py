"""vf_attn_probs_v2 without a GPU: the boundary (declared, bound, exported, argument refusals) and the proof that the operands
of tests/test_attn_probs_alibi_gpu.py DISCRIMINATE -- on the float64 references alone, every plausible way of getting the bias
wrong (dropped, position off by one, q_pos taken as 0, sign flipped, flash-attn's end alignment) moves more than a quarter of
the rows of every head by more than 1e-3 of the row maximum, ten times the cap on the GPU test's tolerance."""
import pytest

from tests.attn_probs_alibi_cases import GEOMETRIES, MUTATIONS, AlibiCase, moved_share, rows_with_keys
from tests.conftest import REPO


def test_v2_symbol_is_declared_bound_and_exported_under_abi_13():
    import ctypes
    import os
    import re
    from variantformer_amd import _lib
    from variantformer_amd.csrc.build import build_lib
    with open(os.path.join(REPO, "include", "vf_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+vf_attn_probs_v2\s*\(", header)
    assert re.search(r"#define\s+VF_ABI_VERSION\s+13\b", header)
    assert len(_lib.SIGNATURES["vf_attn_probs_v2"]) == len(_lib.SIGNATURES["vf_attn_probs"]) + 3 == 23
    assert hasattr(ctypes.CDLL(build_lib()), "vf_attn_probs_v2")
    assert _lib.ABI_VERSION == 13 and _lib.load().vf_version() == 13


def test_v2_argument_validation_without_gpu():
    """Refused before anything is launched (no GPU here: a launch would fail differently); each refusal names its cause."""
    from variantformer_amd import _lib
    lib = _lib.load()
    INVALID = 1                                          # VF_ERR_INVALID_ARG (include/vf_hip.h)
    p = 4096                                             # a non-null, 16-byte aligned address; never dereferenced

    def call(q=p, k=p, q_rows=0, cu_rows=p, cu_k=p, n_seq=1, max_rows=4, max_k=8, H=2, dh=32, flags=2, stats=p, out=p, ldo=8,
             q_stride=64, k_stride=128, dtype=_lib.VF_BF16, slopes=p, q_pos=p, k_rows=p):
        return lib.vf_attn_probs_v2(q, q_stride, k, k_stride, q_rows, cu_rows, cu_k, n_seq, max_rows, max_k, H, dh, 1.0, dtype,
                                    flags, 0, stats, out, ldo, slopes, q_pos, k_rows, 0)
    for name in ("q", "k", "out", "stats", "cu_rows"):
        assert call(**{name: 0}) == INVALID, name
        assert b"null" in lib.vf_last_error() and name.encode() in lib.vf_last_error()
    assert call(cu_k=0) == INVALID and b"cu_seqlens_k" in lib.vf_last_error()
    assert call(dh=40) == INVALID and b"head_dim" in lib.vf_last_error()
    assert call(ldo=7) == INVALID and b"ldo" in lib.vf_last_error()
    for flags in (1, 3, 4):                              # VF_ATTN_Q_AT_START (alone, with Q_LOG2), an unknown bit
        assert call(flags=flags) == INVALID
        assert b"VF_ATTN_Q_AT_START" in lib.vf_last_error()
    assert call(n_seq=-1) == INVALID and call(max_rows=-1) == INVALID
    assert call(q_stride=56) == INVALID and call(k_stride=32) == INVALID     # below H * dh = 64
    assert call(dtype=_lib.VF_F32) == INVALID and b"operand_dtype" in lib.vf_last_error()
    assert call(slopes=p + 2) == INVALID and call(k_rows=p + 4) == INVALID
    assert b"aligned" in lib.vf_last_error()
    assert call(n_seq=0) == 0 and call(max_rows=0) == 0                                # nothing selected: VF_OK, no launch
    assert call(n_seq=0, slopes=0, q_pos=0, k_rows=0) == 0                             # the three new pointers are optional


@pytest.mark.parametrize("H,dh", GEOMETRIES)
def test_operands_discriminate_every_wrong_bias(H, dh):
    case = AlibiCase(H, dh, "bf16", True)
    _, qsel = case.queries(True)
    P, _ = case.reference(qsel)
    has_keys = rows_with_keys(case)
    assert abs(float(P[has_keys].sum(dim=-1).min()) - 1.0) < 1e-12
    for mutation in MUTATIONS:
        P_mut, _ = case.reference(qsel, mutation=mutation)
        share = moved_share(P, P_mut, has_keys)
        print(f"[attn_probs_alibi] H={H} dh={dh} {mutation}: smallest share of moved rows over the heads {float(share.min()):.3f}")
        assert float(share.min()) > 0.25, f"{mutation}: head {int(share.argmin())} moves only {float(share.min()):.3f} of its rows"

"""Argument validation of vf_attn_varlen_fwd_v3 without a GPU: every call here is refused before any launch (non-null
placeholder pointers reach the head-dim check, which comes before anything touches them)."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from variantformer_amd import _lib
    return _lib.load()


def _args(dh, dtype=1, flags=0):
    # q, k, v, out, strides, cu_q, cu_k, n_seq, max_q, max_k, H, dh, slopes, scale, operand_dtype, flags, stream
    return (16, 16, 16, 16, 8, 8, 8, 8, 16, 16, 1, 1, 1, 1, dh, 0, 1.0, dtype, flags, 0)


@pytest.mark.parametrize("dh", [0, 4, 36, 264, -8, 12, 257])
@pytest.mark.parametrize("dtype", [1, 2])
def test_v3_refuses_unsupported_head_dims(lib, dh, dtype):
    assert lib.vf_attn_varlen_fwd_v3(*_args(dh, dtype)) == 1
    msg = lib.vf_last_error()
    assert b"head_dim" in msg and b"vf_attn_varlen_fwd_v3" in msg


def test_v3_refuses_bad_operand_type_and_flags(lib):
    assert lib.vf_attn_varlen_fwd_v3(*_args(4, 0)) == 1                 # dtype check first: not an operand type
    assert b"operand_dtype" in lib.vf_last_error()
    assert lib.vf_attn_varlen_fwd_v3(*_args(40, 1, 8)) == 1             # unknown flag bit
    assert b"flag" in lib.vf_last_error()


def test_legacy_entries_still_refuse_padded_head_dims(lib):
    args18 = (16, 16, 16, 16, 8, 8, 8, 8, 16, 16, 1, 1, 1, 1, 40, 0, 1.0, 0)
    for name in ("vf_attn_varlen_fwd", "vf_attn_varlen_fwd_qstart", "vf_attn_varlen_fwd_f16", "vf_attn_varlen_fwd_qstart_f16"):
        assert getattr(lib, name)(*args18) == 1, name
        assert b"head_dim" in lib.vf_last_error(), name
    assert lib.vf_attn_varlen_fwd_v2(*_args(40)) == 1
    assert b"head_dim" in lib.vf_last_error()
    assert lib.vf_attn_varlen_fwd_rows(*_args(40)[:-1], 16, 16, 0) == 1
    assert b"head_dim" in lib.vf_last_error()
    # counted keys: 32 / 48 / 64 only (C = 1, H = 1)
    assert lib.vf_attn_counted_keys(16, 8, 16, 16, 16, 16, 1, 1, 1, 1, 40, 16, 8, 1, 0) == 1
    assert b"dh=40" in lib.vf_last_error()


@pytest.mark.parametrize("dh", [8, 16, 40, 56, 80, 136, 192, 200, 256])
def test_padded_head_dims_have_no_row_map_form(lib, dh):
    # (vf_attn_rows_supported is a pure function of the geometry: no device memory involved)
    assert lib.vf_attn_rows_supported(dh, 0, 4096, 8, 100, 100, 2) == 0
    assert lib.vf_attn_rows_supported(dh, 1, 4096, 8, 201, 201, 2) == 0


def test_class_head_dims_keep_their_row_map_form(lib):
    assert lib.vf_attn_rows_supported(64, 0, 4096, 8, 100, 100, 2) == 1
    assert lib.vf_attn_rows_supported(48, 1, 64, 32, 201, 201, 2) == 1


def test_abi_version_and_binding(lib):
    from variantformer_amd import _lib
    assert _lib.ABI_VERSION == 13 and lib.vf_version() == 13
    assert _lib.SIGNATURES["vf_attn_varlen_fwd_v3"] == _lib.SIGNATURES["vf_attn_varlen_fwd_v2"]

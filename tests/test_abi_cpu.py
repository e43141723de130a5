"""CPU-side checks of the drop-in boundary: libvf_hip.so builds for gfx950, loads, and exports exactly
the entry points the headers under include/ declare (no compute calls: there is no GPU here).  This file owns the generic
boundary of EVERY header -- it parses, its names are those of its table in _lib.ENTRIES, each is exported, bound and matches its
prototype type by type, and is declared once; the per-family tests hold what is particular to a family."""
import ctypes
import os
import re

import pytest

from tests.conftest import REPO

HEADERS = sorted(os.listdir(os.path.join(REPO, "include")))
N_HEADERS = 16
N_ENTRIES = 89                  # 53 of vf_hip.h and 36 of the fifteen vf_hip_*.h


def _declared(header: str = "vf_hip.h"):
    with open(os.path.join(REPO, "include", header)) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vf_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_and_exports_every_declared_symbol():
    from variantformer_amd.csrc.build import build_lib
    from variantformer_amd import _lib
    path = build_lib()
    assert os.path.exists(path)
    lib = ctypes.CDLL(path)
    names = _declared()
    assert len(names) >= 12
    for n in names:
        assert hasattr(lib, n), f"{n} declared in vf_hip.h but not exported"
    assert sorted(_lib.ENTRIES["vf_hip.h"]) == names, "ctypes binding and header disagree"
    assert _lib.load().vf_version() == _lib.ABI_VERSION


# ---------------------------------------------------------------------------------------------
# the binding, type by type: every prototype of every header against the ctypes tables of _lib.py
# ---------------------------------------------------------------------------------------------
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "double": ctypes.c_double}
_PROTOTYPE = re.compile(r"((?:const\s+)?\b(?:void|char|int|int32_t|int64_t|float|double)\b[\s\*]*?)\s*\b(vf_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;")


def _header_texts() -> dict:
    inc = os.path.join(REPO, "include")
    out = {}
    for name in sorted(os.listdir(inc)):
        if name.endswith(".h"):
            with open(os.path.join(inc, name)) as f:
                out[name] = f.read()
    return out


def _ctype_of(decl: str, what: str):
    """The ctypes that may bind the C type of `decl` (a parameter with its name, or a return type): a tuple of the accepted ones."""
    decl = " ".join(decl.replace("*", " * ").split())
    if "*" in decl:
        words = [w for w in decl.split() if w not in ("const", "*")]
        return (ctypes.c_void_p, ctypes.c_char_p) if words[0] == "char" else (ctypes.c_void_p,)
    words = [w for w in decl.split() if w != "const"]
    if words == ["void"]:
        return (None,)
    assert words[0] in _SCALARS, f"{what}: a C type this test does not map: {decl!r}"
    return (_SCALARS[words[0]],)


def _prototypes(text: str) -> dict:
    """name -> (accepted restypes, [accepted argtypes per parameter]) of every vf_* prototype of a header's text; comments and
    preprocessor lines are stripped first."""
    src = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*$", " ", src, flags=re.M)
    out = {}
    for m in _PROTOTYPE.finditer(src):
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        assert name not in out, f"{name} is declared twice"
        plist = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
        out[name] = (_ctype_of(ret, name), [_ctype_of(p, f"{name}({p})") for p in plist])
    return out


def _bound() -> dict:
    """name -> (restype, argtypes) of every entry of every table of _lib.ENTRIES, read off the loaded library."""
    from variantformer_amd import _lib
    lib = _lib.load()
    out = {}
    for header, table in sorted(_lib.ENTRIES.items()):
        for name, argtypes in table.items():
            assert name not in out, f"{name} is bound by two tables"
            fn = getattr(lib, name)
            assert fn.argtypes is not None, f"_lib.load() does not bind {name} of _lib.ENTRIES[{header!r}]"
            assert list(fn.argtypes) == list(argtypes), f"{name}: load() bound other argtypes than _lib.ENTRIES[{header!r}] lists"
            out[name] = (fn.restype, list(fn.argtypes))
    return out


def _binding_mismatches(declared: dict, bound: dict) -> list:
    """One line per disagreement between the headers' prototypes and the binding, each naming its entry."""
    bad = [f"{n}: declared in a header, bound by no table" for n in sorted(set(declared) - set(bound))]
    bad += [f"{n}: bound, declared in no header" for n in sorted(set(bound) - set(declared))]
    for name in sorted(set(declared) & set(bound)):
        (ret_ok, params), (restype, argtypes) = declared[name], bound[name]
        if restype not in ret_ok:
            bad.append(f"{name}: restype {restype} where the header returns {[getattr(t, '__name__', t) for t in ret_ok]}")
        if len(params) != len(argtypes):
            bad.append(f"{name}: {len(argtypes)} argtypes for {len(params)} declared parameters")
            continue
        for i, (ok, got) in enumerate(zip(params, argtypes)):
            if got not in ok:
                bad.append(f"{name}: parameter {i} is bound as {got.__name__}, the header wants {[t.__name__ for t in ok]}")
    return bad


def _all_declared(texts: dict) -> dict:
    declared = {}
    for header, text in texts.items():
        for name, proto in _prototypes(text).items():
            assert name not in declared, f"{name} is declared in two headers"
            declared[name] = proto
    return declared


def test_every_binding_matches_its_prototype_type_by_type():
    """Parameter by parameter and the return type: a c_int for an int64_t, a c_float for a double or a missing argument would load
    and run with garbage in a register.  Every header under include/, every table of _lib.ENTRIES."""
    from variantformer_amd import _lib
    texts = _header_texts()
    assert len(texts) == N_HEADERS and "vf_hip.h" in texts
    declared, bound = _all_declared(texts), _bound()
    assert sorted(_prototypes(texts["vf_hip.h"])) == _declared()            # the parser sees what the name test sees
    assert len(declared) == N_ENTRIES
    assert _binding_mismatches(declared, bound) == []
    # load() binds every table the module defines: a table it forgot leaves ctypes' default int arguments in place
    assert len(_lib.ENTRIES) == N_HEADERS and sum(map(len, _lib.ENTRIES.values())) == len(_lib.SIGNATURES) == len(bound) == len(declared)
    assert not [n for n in vars(_lib) if n.endswith(("_SIGNATURES", "_ENTRIES"))], "one table: a family adds a key to ENTRIES"
    assert set(_lib._RESTYPES) <= set(bound)


@pytest.mark.parametrize("header", HEADERS)
def test_header_parses_and_its_names_are_exported_and_bound(header):
    """The boundary of one header, the same for all sixteen: what tests/test_<family>_cpu.py used to repeat for its own header,
    each against the headers that existed when it was written."""
    from variantformer_amd import _lib
    from variantformer_amd.csrc import build as B
    texts = _header_texts()
    assert set(texts) == set(HEADERS) == set(_lib.ENTRIES), "a header under include/ has one table in _lib.ENTRIES, and the reverse"
    protos = _prototypes(texts[header])
    names = sorted(protos)
    assert names and names == _declared(header), "the header parses: every vf_* name before a parenthesis is a prototype"
    assert sorted(_lib.ENTRIES[header]) == names, f"ctypes binding and {header} disagree"
    assert any(h.endswith(os.path.join("include", header)) for h in B.HEADERS), "a change of the header rebuilds the library"
    with open(os.path.join(REPO, "variantformer_amd", "csrc", "vf_common.h")) as f:
        assert f'#include "../../include/{header}"' in f.read(), "the sources see the prototypes they define"
    lib, bound = ctypes.CDLL(B.build_lib()), _bound()                       # _bound: load() binds each name with the listed argtypes
    for n in names:
        assert hasattr(lib, n), f"{n} declared in {header} but not exported"
        assert bound[n][1] == list(_lib.ENTRIES[header][n]) == list(_lib.SIGNATURES[n])
    assert _binding_mismatches(protos, {n: bound[n] for n in names}) == []   # type by type, the return type too
    assert set(_all_declared(texts)) >= set(names)                          # _all_declared: no name is declared in two headers
    src = re.sub(r"/\*.*?\*/", "", texts[header], flags=re.S)
    assert bool(re.search(r"#define\s+VF_ABI_VERSION", src)) == (header == "vf_hip.h"), "the version is the main header's"
    assert _lib.ABI_VERSION == 13 and _lib.load().vf_version() == 13


def test_the_type_comparison_names_a_mutated_entry():
    """On a copy of a header's text: an int64_t stride as int, a dropped parameter, a float as double -- each is reported, under
    the entry's name, and nothing else is."""
    texts = _header_texts()
    bound = _bound()
    text = texts["vf_hip_linkage.h"]
    mutations = {
        "vf_linkage_nearest": ("int vf_linkage_nearest(const float* D, int64_t ld,", "int vf_linkage_nearest(const float* D, int ld,",
                               "parameter 1 is bound as c_long"),
        "vf_linkage_contract": ("float* pair_dist, int upper_only,", "float* pair_dist,", "13 argtypes for 12 declared parameters"),
    }
    for entry, (old, new, message) in mutations.items():
        assert text.count(old) == 1
        bad = _binding_mismatches(_all_declared({**texts, "vf_hip_linkage.h": text.replace(old, new)}), bound)
        assert len(bad) == 1 and bad[0].startswith(entry + ":") and message in bad[0].replace("c_int64", "c_long"), bad
    text = texts["vf_hip_umap.h"]
    proto = re.search(r"int vf_umap_smooth_knn\([^;]*;", text).group(0)
    assert proto.count("float ") == 1                                           # its one scalar float: mean_dist
    bad = _binding_mismatches(_all_declared({**texts, "vf_hip_umap.h": text.replace(proto, proto.replace("float ", "double "))}), bound)
    assert len(bad) == 1 and bad[0].startswith("vf_umap_smooth_knn: parameter 6 is bound as c_float"), bad


def test_argument_validation_without_gpu():
    """Error behaviour of the boundary: invalid arguments are rejected before any launch."""
    from variantformer_amd import _lib
    lib = _lib.load()
    assert lib.vf_gemm_bf16(0, 64, 0, 0, 0, 0, 0, 64, 4, 8, 64, 0, 0) == 1          # null pointers
    assert b"null" in lib.vf_last_error()
    assert lib.vf_attn_varlen_fwd(16, 16, 16, 16, 8, 8, 8, 8, 16, 16, 1, 1, 1, 1, 40, 0, 1.0, 0) == 1   # dh=40
    assert b"head_dim" in lib.vf_last_error()
    assert lib.vf_layernorm(16, 16, 16, 16, 1, 6, 1e-5, 1, 0, 0) == 1                 # D % 4 != 0
    with pytest.raises(_lib.VFError):
        _lib.check(1, "demo")


def test_ops_refuse_cpu_tensors():
    import torch
    from variantformer_amd import ops
    from variantformer_amd._lib import VFError
    with pytest.raises(VFError):
        ops.layernorm(torch.zeros(2, 8), torch.ones(8), torch.zeros(8))


def test_vf_narrow_ids_clamps_narrows_and_reports_ranges():
    """vf_narrow_ids (ABI 11, host only): int64 ids -> int32, clamped to [-1, INT32_MAX] like the embedding kernels' own clamp
    would treat them, with the range flags prepare_batch keys its window de-duplication on; strided source rows."""
    import numpy as np
    from variantformer_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(0)
    src = rng.integers(0, 500, (7, 3, 40)).astype(np.int64)          # [rows, strands, L]: rows are 3 * 40 elements apart
    view = src[:, 1, :]
    dst = np.full((7, 40), -7, dtype=np.int32)
    assert lib.vf_narrow_ids(view.ctypes.data, view.strides[0] // 8, dst.ctypes.data, 7, 40) == 0
    assert np.array_equal(dst, view.astype(np.int32))
    view[2, 5], view[4, 0] = -(2 ** 40), -1
    assert lib.vf_narrow_ids(view.ctypes.data, view.strides[0] // 8, dst.ctypes.data, 7, 40) == 1
    assert dst[2, 5] == -1 and dst[4, 0] == -1
    view[2, 5], view[4, 0], view[6, 39] = 3, 4, 2 ** 31 + 9
    assert lib.vf_narrow_ids(view.ctypes.data, view.strides[0] // 8, dst.ctypes.data, 7, 40) == 2
    assert dst[6, 39] == 2 ** 31 - 1
    view[6, 39], view[0, 0] = 2 ** 30, -5
    assert lib.vf_narrow_ids(view.ctypes.data, view.strides[0] // 8, dst.ctypes.data, 7, 40) == 3 and dst[6, 39] == 2 ** 30
    view[6, 39], view[0, 0] = 2 ** 30 - 1, 0
    assert lib.vf_narrow_ids(view.ctypes.data, view.strides[0] // 8, dst.ctypes.data, 7, 40) == 0
    assert lib.vf_narrow_ids(None, 0, dst.ctypes.data, 7, 40) == -1
    assert lib.vf_narrow_ids(view.ctypes.data, view.strides[0] // 8, dst.ctypes.data, 0, 40) == 0

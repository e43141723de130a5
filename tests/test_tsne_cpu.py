"""t-SNE without a GPU: the boundary of include/vf_hip_tsne.h (it parses, its four names are exported and bound through
_lib.ENTRIES), every refusal of every entry and of the Python
functions with its argument named, and the numpy restatements of tests/tsne_cases.py, in fp64 and in individually rounded fp32,
against the scikit-learn functions they restate: _binary_search_perplexity, _joint_probabilities, _kl_divergence (dof 1, 2, 3)
and twenty steps of _gradient_descent; then the end-to-end fixtures' three CPU references against condition (a)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests import tsne_cases as T
from tests import write_set_cases as W
from tests.conftest import REPO

NAMES = ["vf_tsne_descent", "vf_tsne_joint", "vf_tsne_perplexity", "vf_tsne_repulsion"]
ARGS = {"vf_tsne_perplexity": 11, "vf_tsne_joint": 11, "vf_tsne_repulsion": 8, "vf_tsne_descent": 22}


def _header(name="vf_hip_tsne.h") -> str:
    with open(os.path.join(REPO, "include", name)) as f:
        return f.read()


# ---- 1. header and binding ---------------------------------------------------------------------------------------------------------
def test_header_parses_and_its_names_are_exported_and_bound():
    from variantformer_amd import _lib
    from variantformer_amd.csrc import build as B
    text = _header()
    assert W.stream_entries(text) == NAMES
    assert sorted(_lib.ENTRIES["vf_hip_tsne.h"]) == NAMES, "ctypes binding and vf_hip_tsne.h disagree"
    assert "vf_tsne.hip" in B.SOURCES and any(h.endswith("vf_hip_tsne.h") for h in B.HEADERS)
    assert "vf_tsne.hip" not in B.EXTRA_FLAGS                         # absent entries are recognised by NaN / Inf: no -fno-honor-nans
    with open(os.path.join(REPO, "variantformer_amd", "csrc", "vf_tsne.hip")) as f:
        source = f.read()
    assert "#pragma clang fp contract(off)" in source, "p[i->j] and p[j->i], and every stated order, hold only without an fma"
    assert "hipDeviceSynchronize" not in source and "hipStreamSynchronize" not in source, "no entry synchronises the stream"
    assert not re.search(r"\b_*(hip_)?atomic\w*\s*\(", source, flags=re.I), "no atomic: every sum has a stated order"
    bound = _lib.load()
    assert {name: len(_lib.SIGNATURES[name]) for name in NAMES} == ARGS
    assert _lib.ABI_VERSION == 13 and bound.vf_version() == 13
    assert "thirteenth header" in text
    for word in ("Arguments", "Write set", "Arithmetic", "Non-finite operands", "Refused before anything is launched", "Not checked"):
        assert text.count(word) >= 4, f"an entry's comment contract has no `{word}` part"
    for macro, value in (("VF_TSNE_MAX_M", str(T.MAX_M)), ("VF_TSNE_MAX_DIM", str(T.MAX_DIM)), ("VF_TSNE_MAX_R", "(1 << 24)"),
                         ("VF_TSNE_PERPLEXITY_STEPS", str(T.STEPS)), ("VF_TSNE_PERPLEXITY_TOL", "1e-5f"), ("VF_TSNE_TILE", str(T.TILE)),
                         ("VF_TSNE_Z_BLOCKS", str(T.Z_BLOCKS)), ("VF_TSNE_Z_THREADS", str(T.Z_THREADS))):
        assert re.search(rf"#define\s+{macro}\s+{re.escape(value)}\s", text), macro
    assert "is NOT part of this contract" in text, "the header says that the normalisation of P is torch plumbing"


def _err(lib):
    return lib.vf_last_error().decode()


P = 4096                                                 # a non-null, aligned address; never dereferenced
INVALID = 1


def test_perplexity_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(idx=P, ld_idx=255, d2=P, ld_d2=255, R=0, m=90, perplexity=30.0, beta=P, p_cond=P, ld_p=255):
        return lib.vf_tsne_perplexity(idx, ld_idx, d2, ld_d2, R, m, perplexity, beta, p_cond, ld_p, 0)
    assert call() == 0 and call(m=2, perplexity=1.0) == 0 and call(m=255, perplexity=254.5) == 0          # R = 0: nothing launched
    for name in ("idx", "d2", "beta", "p_cond"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        assert call(**{name: P + 2}) == INVALID and re.search(rf"\b{name} must be 4-byte aligned", _err(lib)), _err(lib)
    for m in (0, -1, 256):
        assert call(m=m, ld_idx=256, ld_d2=256, ld_p=256) == INVALID and _err(lib).split(": ")[1].startswith("m="), _err(lib)
    assert call(R=-1) == INVALID and "R=" in _err(lib)
    assert call(R=2 ** 24 + 1) == INVALID and "R=" in _err(lib) and "2^24" in _err(lib)
    for name in ("ld_idx", "ld_d2", "ld_p"):
        assert call(**{name: 89}) == INVALID and _err(lib).split(": ")[1].startswith(f"{name}="), _err(lib)
    for bad in (float("nan"), float("inf"), -float("inf"), 0.5, 0.0, -3.0, 90.0, 91.0):
        assert call(perplexity=bad) == INVALID and _err(lib).split(": ")[1].startswith("perplexity="), (bad, _err(lib))
    assert call(m=1, perplexity=1.0) == INVALID and "perplexity=" in _err(lib), "a list of one admits no perplexity"


def test_joint_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(idx=P, ld_idx=255, p_cond=P, ld_p=255, R=0, m=90, rowptr=P, col=P, nnz=5, p=P):
        return lib.vf_tsne_joint(idx, ld_idx, p_cond, ld_p, R, m, rowptr, col, nnz, p, 0)
    assert call() == 0 and call(R=7, nnz=0) == 0 and call(R=7, nnz=0, col=0, p=0) == 0     # nothing launched
    for name in ("idx", "p_cond", "rowptr", "col", "p"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        align = 8 if name == "rowptr" else 4
        assert call(**{name: P + align // 2}) == INVALID and re.search(rf"\b{name} must be {align}-byte aligned", _err(lib)), _err(lib)
    for m in (0, 256):
        assert call(m=m, ld_idx=256, ld_p=256) == INVALID and _err(lib).split(": ")[1].startswith("m="), _err(lib)
    assert call(R=-1) == INVALID and "R=" in _err(lib)
    assert call(R=2 ** 24 + 1) == INVALID and "R=" in _err(lib) and "2^24" in _err(lib)
    for name in ("ld_idx", "ld_p"):
        assert call(**{name: 89}) == INVALID and _err(lib).split(": ")[1].startswith(f"{name}="), _err(lib)
    assert call(nnz=-1) == INVALID and "nnz=" in _err(lib)


def test_repulsion_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(Y=P, ld=2, R=0, dim=2, dof=1, splits=3, part=P):
        return lib.vf_tsne_repulsion(Y, ld, R, dim, dof, splits, part, 0)
    assert call() == 0 and call(dim=4, ld=4, dof=3, splits=65535) == 0        # R = 0: nothing launched
    for name in ("Y", "part"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        assert call(**{name: P + 2}) == INVALID and re.search(rf"\b{name} must be 4-byte aligned", _err(lib)), _err(lib)
    assert call(R=-1) == INVALID and "R=" in _err(lib)
    assert call(R=2 ** 24 + 1) == INVALID and "R=" in _err(lib) and "2^24" in _err(lib)
    for dim in (0, 5):
        assert call(dim=dim, ld=16) == INVALID and _err(lib).split(": ")[1].startswith("dim="), _err(lib)
    assert call(dim=3) == INVALID and _err(lib).split(": ")[1].startswith("ld=")
    for dof in (0, 4, -1):
        assert call(dof=dof) == INVALID and _err(lib).split(": ")[1].startswith("dof="), _err(lib)
    for splits in (0, -2, 65536):
        assert call(splits=splits) == INVALID and _err(lib).split(": ")[1].startswith("splits="), _err(lib)


def test_descent_refusals_without_gpu():
    from variantformer_amd import _lib, ops
    lib = _lib.load()
    f = ctypes.c_float

    def call(rowptr=P, col=P, p=P, nnz=5, R=0, dim=2, Y=P, update=2 * P, gains=3 * P, ld=2, iter_begin=0, iter_end=10, dof=1, splits=3,
             work=4 * P, work_bytes=1 << 20, zsum=5 * P):
        return lib.vf_tsne_descent(rowptr, col, p, nnz, R, dim, Y, update, gains, ld, iter_begin, iter_end, f(12.0), f(0.5), f(50.0), f(0.01),
                                   dof, splits, work, work_bytes, zsum, 0)
    assert call() == 0 and call(R=9, iter_begin=4, iter_end=4) == 0 and call(nnz=0, col=0, p=0) == 0      # nothing launched
    assert call(R=9, iter_begin=4, iter_end=4, zsum=0) == 0, "an empty range needs no zsum"
    for name in ("rowptr", "col", "p", "Y", "update", "gains", "work", "zsum"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        align = 8 if name in ("rowptr", "work", "zsum") else 4
        assert call(**{name: P + align // 2}) == INVALID and re.search(rf"\b{name} must be {align}-byte aligned", _err(lib)), _err(lib)
    assert call(R=-1) == INVALID and "R=" in _err(lib)
    assert call(R=2 ** 24 + 1, work_bytes=1 << 40) == INVALID and "R=" in _err(lib) and "2^24" in _err(lib)
    assert call(nnz=-1) == INVALID and "nnz=" in _err(lib)
    for dim in (0, 5):
        assert call(dim=dim, ld=16) == INVALID and _err(lib).split(": ")[1].startswith("dim="), _err(lib)
    assert call(dim=3) == INVALID and _err(lib).split(": ")[1].startswith("ld=")
    for dof in (0, 4):
        assert call(dof=dof) == INVALID and _err(lib).split(": ")[1].startswith("dof="), _err(lib)
    for splits in (0, 65536):
        assert call(splits=splits) == INVALID and _err(lib).split(": ")[1].startswith("splits="), _err(lib)
    assert call(iter_begin=-1) == INVALID and "iter_begin=" in _err(lib)
    assert call(iter_begin=6, iter_end=5) == INVALID and _err(lib).split(": ")[1].startswith("iter_begin=")
    need = ops.tsne_work_bytes(100, 2, 3)
    assert need == 8 * 64 + 4 * (3 * 100 * 3 + 100 * 2), "VF_TSNE_WORK_BYTES, restated"
    assert call(R=100, work_bytes=need - 1, iter_end=0) == INVALID and _err(lib).split(": ")[1].startswith("work_bytes="), _err(lib)
    assert call(R=100, work_bytes=need, iter_end=0) == 0


def test_the_wrappers_allocate_nothing_and_refuse_cpu_tensors():
    from variantformer_amd import manifold, ops
    for fn, outs in ((ops.tsne_perplexity, ("beta", "p_cond")), (ops.tsne_joint, ("p",)), (ops.tsne_repulsion, ("part",)),
                     (ops.tsne_descent, ("work", "zsum"))):
        src = inspect.getsource(fn)
        assert not re.search(r"\b(empty|empty_like|zeros|zeros_like|ones|full|new_empty|new_zeros|new_full|tensor|arange|clone|contiguous)\s*\(", src)
        assert 'family="tsne"' not in src and "family or _SCOPE" in src
        prm = inspect.signature(fn).parameters
        for o in outs:
            assert prm[o].kind is inspect.Parameter.KEYWORD_ONLY and prm[o].default is inspect.Parameter.empty
        assert fn.__name__ not in W.allocating_wrappers()
    assert W.uncovered_wrappers() == []
    i, f = torch.zeros((4, 3), dtype=torch.int32), torch.zeros((4, 3))
    rowptr, col = torch.zeros(5, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(Exception, match="GPU"):
        ops.tsne_perplexity(i, f, 2.0, beta=torch.zeros(4), p_cond=f.clone())
    with pytest.raises(Exception, match="GPU"):
        ops.tsne_joint(i, f, rowptr, col, p=torch.zeros(2))
    with pytest.raises(Exception, match="GPU"):
        ops.tsne_repulsion(torch.zeros(4, 2), dof=1, splits=1, part=torch.zeros(1, 4, 3))
    with pytest.raises(Exception, match="GPU"):
        ops.tsne_descent(rowptr, col, torch.zeros(2), torch.zeros(4, 2), torch.zeros(4, 2), torch.ones(4, 2), iter_begin=0, iter_end=1,
                         exaggeration=1.0, momentum=0.8, learning_rate=50.0, dof=1, splits=1, work=torch.zeros(200, dtype=torch.float64),
                         zsum=torch.zeros(1, dtype=torch.float64))
    assert inspect.getsource(manifold).count('family="tsne"') == 5, "every launch of the driver is recorded under the family"
    assert not re.search(r"^\s*(import|from)\s+(scipy|sklearn|openTSNE)", inspect.getsource(manifold), flags=re.M)


def test_the_python_functions_check_their_arguments_before_the_device():
    from variantformer_amd import manifold
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    x = np.random.default_rng(0).standard_normal((40, 6)).astype(np.float32)
    for bad, word in ((dict(perplexity=0.5), "perplexity"), (dict(perplexity=float("nan")), "perplexity"), (dict(perplexity=39.0), "perplexity"),
                      (dict(perplexity=5.0, n_neighbors=5), "perplexity"), (dict(n_neighbors=40), "n_neighbors"), (dict(n_neighbors=1), "n_neighbors"),
                      (dict(metric="euclidean"), "metric"), (dict(n_components=0), "n_components"), (dict(n_components=5), "n_components"),
                      (dict(n_iter=-1), "n_iter"), (dict(exaggeration_iter=-1), "exaggeration_iter"), (dict(early_exaggeration=0.0), "early_exaggeration"),
                      (dict(learning_rate="fast"), "learning_rate"), (dict(learning_rate=0.0), "learning_rate"), (dict(seed=-1), "seed"),
                      (dict(init="spectral"), "init"), (dict(init=np.zeros((39, 2), dtype=np.float32)), "init")):
        kw = dict(perplexity=10.0)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            manifold.tsne(x, **kw)
    with pytest.raises(ValueError, match="init='pca'"):
        manifold.tsne(x[:, :1], perplexity=10.0)
    with pytest.raises(ValueError, match="rows"):
        manifold.tsne(x[:2], perplexity=1.0)
    with pytest.raises(TypeError, match="x must be"):
        manifold.tsne([[1.0, 2.0]])
    assert manifold.tsne_splits(18000) == 29 and manifold.tsne_splits(64) == 1 and manifold.tsne_splits(1) == 1 and manifold.tsne_splits(65) == 2
    idx, dist = np.zeros((5, 3), dtype=np.int32), np.zeros((5, 3), dtype=np.float32)
    for args, word in (((idx, dist[:, :2], 2.0), "one shape"), ((idx, dist, 3.0), "perplexity"), ((idx, dist, 0.9), "perplexity"),
                       ((np.zeros((5, 256), dtype=np.int32), np.zeros((5, 256), dtype=np.float32), 30.0), "1 .. 255"),
                       ((idx[0], dist[0], 2.0), "matrix")):
        with pytest.raises(ValueError, match=word):
            manifold.tsne_affinities(*args)
    with pytest.raises(TypeError, match="indices must be"):
        manifold.tsne_affinities([[1]], dist, 2.0)
    graph = (np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
    y = np.zeros((5, 2), dtype=np.float32)
    for kw, word in ((dict(init=np.zeros((4, 2), dtype=np.float32)), "rows"), (dict(init=np.zeros((5, 5), dtype=np.float32)), "1 .. 4"),
                     (dict(iter_begin=3, iter_end=2), "iter_begin"), (dict(iter_begin=-1), "iter_begin"), (dict(exaggeration=0.0), "exaggeration"),
                     (dict(momentum=-0.1), "momentum"), (dict(learning_rate=float("inf")), "learning_rate"), (dict(min_gain=-1.0), "min_gain"),
                     (dict(splits=0), "splits"), (dict(state=(y,)), "state"), (dict(state=(y, y[:4])), "state")):
        args = dict(init=y)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            manifold.tsne_descent(graph, **args)
    with pytest.raises(ValueError, match="graph"):
        manifold.tsne_descent((graph[0],), y)
    with pytest.raises(ValueError, match="rows"):
        manifold.tsne_kl(graph, y[:4])
    with pytest.raises(ValueError, match="splits"):
        manifold.tsne_kl(graph, y, splits=70000)
    if not torch.cuda.is_available():
        with pytest.raises(Exception, match="GPU"):
            manifold.tsne(x, perplexity=10.0)
        with pytest.raises(Exception, match="GPU"):
            manifold.tsne_affinities(idx, dist, 2.0)
        with pytest.raises(Exception, match="GPU"):
            manifold.tsne_descent(graph, y)
        with pytest.raises(Exception, match="GPU"):
            manifold.tsne_kl(graph, y)
    frame = pd.DataFrame({"gene": ["a", "b"], "predicted_expression": [np.zeros(3, dtype=np.float32)] * 2})
    with pytest.raises(ValueError, match="return_kl"):
        VCFProcessor.expression_tsne(None, frame, return_kl=True)
    assert list(inspect.signature(VCFProcessor.expression_tsne).parameters)[:5] == ["self", "df", "on", "axis", "tissue"]


# ---- 2. the restatements against scikit-learn --------------------------------------------------------------------------------------------
def _sk():
    utils = pytest.importorskip("sklearn.manifold._utils", reason="scikit-learn is not installed")
    tsne = pytest.importorskip("sklearn.manifold._t_sne", reason="scikit-learn is not installed")
    for mod, name in ((utils, "_binary_search_perplexity"), (tsne, "_joint_probabilities"), (tsne, "_kl_divergence"), (tsne, "_gradient_descent")):
        if not hasattr(mod, name):
            pytest.skip(f"this scikit-learn has no {mod.__name__}.{name}")
    return utils, tsne


def _square_case(R: int, seed: int):
    """A dense fp32 matrix of squared distances between R random points, and its full neighbour lists."""
    pts = np.random.default_rng(seed).standard_normal((R, 5))
    D2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1).astype(np.float32)
    return D2, T.full_lists(D2)


def test_the_search_restates_binary_search_perplexity():
    utils, _ = _sk()
    for R, m, perplexity in ((40, 39, 12.0), (70, 30, 9.5), (30, 29, 1.0), (200, 130, 42.0)):
        idx, d2 = T.perplexity_case("random", R, m)
        want = utils._binary_search_perplexity(d2, perplexity, 0)      # no index enters it: a list is a list
        beta, got, converged = T.perplexity_search(idx % (10 * R) + R, d2, perplexity, T.F64, target=np.log(perplexity))
        assert converged.all() and np.allclose(got.sum(1), 1.0, atol=1e-12)
        err = float(np.abs(got - want).max())
        print(f"[tsne search] R={R} m={m} perplexity={perplexity}: fp64 restatement from scikit-learn by {err:.2e}")
        assert err <= 1e-12, "the row minimum changes nothing in exact arithmetic: the same branches, the same P"
        _, got32, conv32 = T.perplexity_search(idx % (10 * R) + R, d2, perplexity, T.F32)
        err32 = float(np.abs(got32 - want).max())
        print(f"[tsne search] ... the fp32 restatement by {err32:.2e}; {int(conv32.sum())} of {R} rows converged in fp32")
        assert got32.dtype == np.float32 and err32 <= 2e-5, "fp32 sums move the entropy by ~1e-6: P stays within the search's own tolerance"
    # the dense form: scikit-learn skips the diagonal where the list is the whole row
    D2, (idx, d2) = _square_case(35, 3)
    want = utils._binary_search_perplexity(D2, 10.0, 0)
    _, got, _ = T.perplexity_search(idx, d2, 10.0, T.F64, target=np.log(10.0))
    full = np.zeros((35, 35))
    full[np.arange(35)[:, None], idx] = got
    assert np.abs(full - want).max() <= 1e-12


def test_the_joint_probabilities_restate_scikit_learn():
    _, tsne = _sk()
    from scipy.spatial.distance import squareform
    for R, perplexity, seed in ((35, 10.0, 3), (64, 21.0, 4)):
        D2, (idx, d2) = _square_case(R, seed)
        want = squareform(tsne._joint_probabilities(D2, perplexity, 0))
        rowptr, col = T.csr(idx, d2)
        assert rowptr[-1] == R * (R - 1), "m = R - 1: every pair is an edge"
        for dtype, bound in ((T.F64, 1e-13), (T.F32, 2e-7)):
            _, p_cond, _ = T.perplexity_search(idx, d2, perplexity, dtype, target=np.log(perplexity) if dtype is T.F64 else None)
            p = T.normalised(T.joint(idx, p_cond, rowptr, col), dtype)
            got = T.dense(rowptr, col, p)
            assert got.dtype == dtype and np.array_equal(got, got.T), "the same bits in both directions"
            err = float(np.abs(got - want).max())
            print(f"[tsne joint] R={R} {np.dtype(dtype).name}: from scikit-learn's P by {err:.2e} (largest P {want.max():.2e})")
            assert err <= bound


def _dense_p(R: int, seed: int):
    _, tsne = _sk()
    D2, (idx, d2) = _square_case(R, seed)
    condensed = tsne._joint_probabilities(D2, 8.0, 0)
    _, p_cond, _ = T.perplexity_search(idx, d2, 8.0, T.F64, target=np.log(8.0))
    rowptr, col = T.csr(idx, d2)
    return condensed, rowptr, col, T.normalised(T.joint(idx, p_cond, rowptr, col), T.F64)


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_the_gradient_restates_kl_divergence(dim):
    _, tsne = _sk()
    R = 30
    dof = max(dim - 1, 1)                                             # dim 1, 2 -> 1; 3 -> 2; 4 -> 3
    condensed, rowptr, col, p = _dense_p(R, 10 + dim)
    Y = T.embedding(R, dim, scale=2.0)
    kl_ref, grad_ref = tsne._kl_divergence(Y.astype(np.float64).ravel(), condensed, dof, R, dim)
    grad_ref = grad_ref.reshape(R, dim)
    for splits in (1, 3):
        got = T.gradient(rowptr, col, p, Y, 1.0, splits, T.F64)
        rel = float(np.abs(got - grad_ref).max() / np.abs(grad_ref).max())
        print(f"[tsne gradient] dim={dim} dof={dof} splits={splits}: fp64 restatement from _kl_divergence by {rel:.2e} of the largest component")
        assert rel <= 1e-12
    got32 = T.gradient(rowptr, col, p.astype(np.float32), Y, 1.0, 3, T.F32)
    rel32 = float(np.abs(got32 - grad_ref).max() / np.abs(grad_ref).max())
    print(f"[tsne gradient] ... the fp32 restatement by {rel32:.2e}")
    assert got32.dtype == np.float32 and rel32 <= 1e-5
    assert abs(T.kl(rowptr, col, p, Y) - kl_ref) <= 1e-12 * max(abs(kl_ref), 1.0), "kl() is scikit-learn's error over the same P"


LR = T.STEPS_LEARNING_RATE


@pytest.mark.parametrize("dim", [2, 3, 4])
def test_twenty_steps_restate_gradient_descent(dim):
    _, tsne = _sk()
    R = 30
    dof = max(dim - 1, 1)
    condensed, rowptr, col, p = _dense_p(R, 20 + dim)
    Y0 = T.embedding(R, dim, scale=1e-4)
    for exaggeration, momentum in ((12.0, 0.5), (1.0, 0.8)):
        ref, _, it = tsne._gradient_descent(tsne._kl_divergence, Y0.astype(np.float64).ravel(), 0, 20, n_iter_check=1000,
                                            n_iter_without_progress=1000, momentum=momentum, learning_rate=LR, min_gain=0.01, min_grad_norm=0.0,
                                            args=[condensed * exaggeration, dof, R, dim], kwargs={})
        assert it == 19, "all twenty iterations ran"
        ref = ref.reshape(R, dim)
        zero, one = np.zeros((R, dim)), np.ones((R, dim))
        got, update, gains, zs = T.descent(rowptr, col, p, Y0, zero, one, 20, exaggeration, momentum, LR, 0.01, 2, T.F64)
        scale = float(np.abs(ref).max())
        rel = float(np.abs(got - ref).max() / scale)
        print(f"[tsne descent] dim={dim} exaggeration={exaggeration}: 20 steps of the fp64 restatement from _gradient_descent by {rel:.2e} of the span {scale:.2e}")
        # the early steps at 12x multiply a difference many times over (the span grows from 1e-4 to tens): fp64 rounding of
        # 1e-16 arrives as up to 1e-9 here, and a formula that differed at all would arrive as O(1)
        assert rel <= 1e-6 and zs.shape == (20,) and (zs > 0).all() and (gains >= 0.01).all()
        got32, _, _, zs32 = T.descent(rowptr, col, p.astype(np.float32), Y0, zero, one, 20, exaggeration, momentum, LR, 0.01, 2, T.F32)
        rel32 = float(np.abs(got32 - ref).max() / scale)
        print(f"[tsne descent] ... the fp32 restatement by {rel32:.2e}, its Z by {float(np.abs(zs32 / zs - 1).max()):.2e}")
        assert got32.dtype == np.float32 and rel32 <= 1e-3
        half, u, g, z1 = T.descent(rowptr, col, p, Y0, zero, one, 7, exaggeration, momentum, LR, 0.01, 2, T.F64)
        rest, _, _, z2 = T.descent(rowptr, col, p, half, u, g, 13, exaggeration, momentum, LR, 0.01, 2, T.F64)
        assert np.array_equal(rest, got) and np.array_equal(np.concatenate((z1, z2)), zs), "the restatement itself can be split"


def test_the_orders_of_the_sums_are_what_the_header_states():
    rng = np.random.default_rng(9)
    v = rng.random((3, 200)).astype(np.float32)
    assert np.allclose(T.lane_sum(v), v.astype(np.float64).sum(1), rtol=1e-6) and T.lane_sum(v).dtype == np.float32
    one = np.zeros((1, 130), dtype=np.float32)
    one[0, [0, 64, 128]] = (1.0, 2.0 ** -24, 2.0 ** -24)             # lane 0 adds its three entries in ascending t: 1 + 2^-24 rounds to 1, twice
    assert T.lane_sum(one)[0] == 1.0
    one[0, [0, 64, 128]] = (2.0 ** -24, 2.0 ** -24, 1.0)             # (2^-24 + 2^-24) + 1 does not
    assert T.lane_sum(one)[0] == np.float32(1.0) + np.float32(2.0 ** -23)
    assert [T.split_range(10, 3, s) for s in range(3)] == [(0, 4), (4, 8), (8, 10)] and T.split_range(2, 3, 2) == (2, 2)
    part = rng.random((5, 77, 3))
    assert abs(T.z_sum(part) - part[:, :, 2].sum()) <= 1e-12 * part[:, :, 2].sum()
    Y = T.embedding(9, 2)
    Y[4] = Y[2]                                                       # coincident points: w = 1 and no force between them
    a, b = T.repulsion(Y, 1, 1, T.F32), T.repulsion(Y, 1, 4, T.F32)
    assert a.dtype == np.float32 and np.allclose(a[0], b.sum(0), rtol=1e-5, atol=1e-7)
    lone = T.repulsion(Y[[2, 4]], 1, 1, T.F32)
    assert (lone[0, :, :2] == 0).all() and (lone[0, :, 2] == 1).all()


# ---- 3. the end-to-end fixtures' references ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(T.FIXTURES))
def test_the_fixture_references_hold_condition_a(name):
    _sk()
    ref = T.fixture_references(name)
    R, perplexity, m = T.FIXTURES[name]
    assert m == R - 1 and ref["graph"][0][-1] == R * (R - 1)
    for key, Y in ref["embeddings"].items():
        ok = T.nearest_in_group(Y, ref["labels"])
        print(f"[tsne fixture {name}] {key}: KL {ref['kl'][key]:.4f}, every row's {T.NEAREST} nearest in its own group: {ok}")
        assert np.isfinite(Y).all() and ok, key
    print(f"[tsne fixture {name}] scikit-learn's own kl_divergence_ {ref['kl_sklearn_own']:.4f}")
    # scikit-learn reports the error it computed before its last update: one late iteration's progress apart
    assert abs(ref["kl"]["sklearn"] - ref["kl_sklearn_own"]) <= 1e-3 * ref["kl_sklearn_own"], "kl() over the fp64 P is scikit-learn's error"

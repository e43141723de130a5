"""The spectral embedding without a GPU: the boundary of include/vf_hip_spectral.h (it parses, its four names are exported and
bound through _lib.ENTRIES), every refusal with its argument named, the numpy
restatement of the solver against the dense fp64 truth on every connected graph of tests/spectral_cases.py, and the argument
checks of manifold.spectral_embedding and of a callable init."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import spectral_cases as S
from tests import write_set_cases as W
from tests.conftest import REPO

NAMES = ["vf_graph_degree", "vf_spmm_recur", "vf_tall_gram", "vf_tall_mul"]
ARGS = {"vf_graph_degree": 8, "vf_spmm_recur": 14, "vf_tall_gram": 10, "vf_tall_mul": 9}


def _header(name="vf_hip_spectral.h") -> str:
    with open(os.path.join(REPO, "include", name)) as f:
        return f.read()


# ---- 1. header and binding ---------------------------------------------------------------------------------------------------------
def test_header_parses_and_its_names_are_exported_and_bound():
    from variantformer_amd import _lib
    from variantformer_amd.csrc import build as B
    text = _header()
    assert W.stream_entries(text) == NAMES
    assert sorted(_lib.ENTRIES["vf_hip_spectral.h"]) == NAMES, "ctypes binding and vf_hip_spectral.h disagree"
    assert "vf_spectral.hip" in B.SOURCES and any(h.endswith("vf_hip_spectral.h") for h in B.HEADERS)
    assert "vf_spectral.hip" not in B.EXTRA_FLAGS
    with open(os.path.join(REPO, "variantformer_amd", "csrc", "vf_spectral.hip")) as f:
        assert "#pragma clang fp contract(off)" in f.read(), "every operation is rounded on its own only without an fma"
    bound = _lib.load()
    assert {name: len(_lib.SIGNATURES[name]) for name in NAMES} == ARGS
    assert _lib.ABI_VERSION == 13 and bound.vf_version() == 13
    assert "tenth header" in text
    for word in ("Arguments", "Write set", "Arithmetic", "Non-finite operands", "Refused before anything is launched", "Not checked"):
        assert text.count(word) >= 4, f"an entry's comment contract has no `{word}` part"
    for macro, value in (("VF_SPECTRAL_MAX_P", "32"), ("VF_SPECTRAL_MAX_R", "(1 << 24)"), ("VF_TALL_GRAM_MAX_BLOCKS", "1024"), ("VF_TALL_GRAM_TILE", "64")):
        assert re.search(rf"#define\s+{macro}\s+{re.escape(value)}\s", text), macro
    assert (S.MAX_P, S.MAX_BLOCKS, S.TILE) == (32, 1024, 64)
    assert "`coef` IS A HOST POINTER" in text and "X0 if\n * steps mod 3 == 0" in text, "the header says which pointer is the host's and which buffer holds the result"
    assert "IS SKIPPED" in text, "the header says how a zero coefficient is handled"


def _err(lib):
    return lib.vf_last_error().decode()


P = 4096                                                 # a non-null, aligned address; never dereferenced
INVALID = 1


def test_graph_degree_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(rowptr=P, col=P, w=P, nnz=5, R=0, deg=P, dinv_sqrt=P):
        return lib.vf_graph_degree(rowptr, col, w, nnz, R, deg, dinv_sqrt, 0)
    assert call() == 0 and call(nnz=0, col=0, w=0) == 0               # R = 0: nothing launched
    for name in ("rowptr", "col", "w", "deg", "dinv_sqrt"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        align = 8 if name == "rowptr" else 4
        assert call(**{name: P + align // 2}) == INVALID and re.search(rf"\b{name} must be {align}-byte aligned", _err(lib)), _err(lib)
    assert call(R=-1) == INVALID and "R=" in _err(lib)
    assert call(R=2 ** 24 + 1) == INVALID and "R=" in _err(lib) and "2^24" in _err(lib)
    assert call(nnz=-1) == INVALID and "nnz=" in _err(lib)


def test_spmm_recur_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()
    coef = (ctypes.c_float * 6)(1, 0, 0, 1, 0, 0)
    host = ctypes.addressof(coef)

    def call(rowptr=P, col=P, w=P, nnz=5, R=0, dinv_sqrt=P, p=16, X0=P, X1=2 * P, X2=3 * P, ld=16, steps=2, coef=host):
        return lib.vf_spmm_recur(rowptr, col, w, nnz, R, dinv_sqrt, p, X0, X1, X2, ld, steps, coef, 0)
    assert call() == 0 and call(R=9, steps=0, coef=0) == 0 and call(nnz=0, col=0, w=0) == 0      # nothing launched
    for name in ("rowptr", "col", "w", "dinv_sqrt", "X0", "X1", "X2"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        align = 8 if name == "rowptr" else 4
        assert call(**{name: P + align // 2}) == INVALID and re.search(rf"\b{name} must be {align}-byte aligned", _err(lib)), _err(lib)
    assert call(coef=0) == INVALID and _err(lib).endswith("null pointer coef")
    for same in (dict(X1=P), dict(X2=P), dict(X2=2 * P)):
        assert call(**same) == INVALID and "X0, X1 and X2" in _err(lib), _err(lib)
    assert call(R=-1) == INVALID and "R=" in _err(lib)
    assert call(R=2 ** 24 + 1) == INVALID and "R=" in _err(lib) and "2^24" in _err(lib)
    assert call(nnz=-1) == INVALID and "nnz=" in _err(lib)
    for p in (0, -1, 33):
        assert call(p=p, ld=64) == INVALID and _err(lib).split(": ")[1].startswith("p="), _err(lib)
    assert call(ld=15) == INVALID and _err(lib).split(": ")[1].startswith("ld=")
    assert call(steps=-1) == INVALID and _err(lib).split(": ")[1].startswith("steps=")


def test_tall_gram_and_tall_mul_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def gram(A=P, lda=16, B=P, ldb=16, R=-5, p=16, q=16, G=P, work=P):
        return lib.vf_tall_gram(A, lda, B, ldb, R, p, q, G, work, 0)
    base = dict(R=7)                                                   # every call below is refused: R = 7 would launch
    for name in ("A", "B", "G", "work"):
        assert gram(**base, **{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        align = 8 if name in ("G", "work") else 4
        assert gram(**base, **{name: P + align // 2}) == INVALID and re.search(rf"\b{name} must be {align}-byte aligned", _err(lib)), _err(lib)
    assert gram() == INVALID and "R=" in _err(lib)
    assert gram(R=2 ** 24 + 1) == INVALID and "R=" in _err(lib) and "2^24" in _err(lib)
    for name in ("p", "q"):
        for v in (0, 33):
            assert gram(**base, lda=64, ldb=64, **{name: v}) == INVALID and _err(lib).split(": ")[1].startswith(f"{name}="), _err(lib)
    assert gram(**base, lda=15) == INVALID and _err(lib).split(": ")[1].startswith("lda=")
    assert gram(**base, ldb=15) == INVALID and _err(lib).split(": ")[1].startswith("ldb=")

    def mul(X=P, ldx=16, R=0, p=16, T=P, q=16, Out=2 * P, ldo=16):
        return lib.vf_tall_mul(X, ldx, R, p, T, q, Out, ldo, 0)
    assert mul() == 0                                                  # R = 0: nothing launched
    for name in ("X", "T", "Out"):
        assert mul(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        align = 8 if name == "T" else 4
        assert mul(**{name: P + align // 2}) == INVALID and re.search(rf"\b{name} must be {align}-byte aligned", _err(lib)), _err(lib)
    assert mul(Out=P) == INVALID and "X and Out" in _err(lib)
    assert mul(R=-1) == INVALID and "R=" in _err(lib)
    assert mul(R=2 ** 24 + 1) == INVALID and "R=" in _err(lib) and "2^24" in _err(lib)
    for name in ("p", "q"):
        for v in (0, 33):
            assert mul(ldx=64, ldo=64, **{name: v}) == INVALID and _err(lib).split(": ")[1].startswith(f"{name}="), _err(lib)
    assert mul(ldx=15) == INVALID and _err(lib).split(": ")[1].startswith("ldx=")
    assert mul(ldo=15) == INVALID and _err(lib).split(": ")[1].startswith("ldo=")


def test_the_wrappers_allocate_nothing_and_refuse_cpu_tensors():
    from variantformer_amd import manifold, ops
    for fn, outs in ((ops.graph_degree, ("deg", "dinv_sqrt")), (ops.spmm_recur, ()), (ops.tall_gram, ("out", "work")), (ops.tall_mul, ("out",))):
        src = inspect.getsource(fn)
        assert not re.search(r"\b(empty|empty_like|zeros|zeros_like|ones|full|new_empty|new_zeros|new_full|tensor|arange|clone|contiguous)\s*\(", src)
        assert 'family="spectral"' not in src and "family or _SCOPE" in src
        prm = inspect.signature(fn).parameters
        for o in outs:
            assert prm[o].kind is inspect.Parameter.KEYWORD_ONLY and prm[o].default is inspect.Parameter.empty
        assert fn.__name__ not in W.allocating_wrappers()
    rowptr, col, w = (torch.from_numpy(a) for a in S.path(5))
    with pytest.raises(Exception, match="GPU"):
        ops.graph_degree(rowptr, col, w, deg=torch.zeros(5), dinv_sqrt=torch.zeros(5))
    with pytest.raises(Exception, match="GPU"):
        ops.spmm_recur(rowptr, col, w, torch.zeros(5), torch.zeros(5, 2), torch.zeros(5, 2), torch.zeros(5, 2), S.ONE_STEP)
    with pytest.raises(Exception, match="GPU"):
        ops.tall_gram(torch.zeros(5, 2), torch.zeros(5, 2), out=torch.zeros(2, 2, dtype=torch.float64), work=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(Exception, match="GPU"):
        ops.tall_mul(torch.zeros(5, 2), torch.zeros(2, 2, dtype=torch.float64), out=torch.zeros(5, 2))
    assert inspect.getsource(manifold).count('family="spectral"') == 4, "every launch of the solver is recorded under the family"
    assert not re.search(r"^\s*(import|from)\s+(scipy|umap|numba|pynndescent|sklearn)", inspect.getsource(manifold), flags=re.M)


# ---- 2. the reference ---------------------------------------------------------------------------------------------------------------
def test_the_restated_kernels_agree_with_plain_fp64():
    """The fixed orders change the last bits, not the values: each restatement against a plain fp64 evaluation."""
    g = np.random.default_rng(11)
    rowptr, col, w = S.kernel_graph(257)
    assert np.diff(rowptr)[:6].tolist() == list(S.ROW_LENGTHS) and (col == -1).any() and (col == 257).any()
    deg, dinv = S.degree(rowptr, w)
    plain = np.array([w[a:b].astype(np.float64).sum() for a, b in zip(rowptr[:-1], rowptr[1:])])
    assert deg.dtype == np.float32 and np.abs(deg - plain).max() <= 200 * 2.0 ** -24 * plain.max() and deg[0] == 0 and dinv[0] == 0
    some = deg > 0
    assert np.array_equal(dinv[some], (np.float32(1) / np.sqrt(deg[some])).astype(np.float32)) and (dinv[~some] == 0).all() and (~some).sum() >= 2
    ok = (col >= 0) & (col < 257)
    A = np.zeros((257, 257))
    A[S.U.entry_rows(rowptr)[ok], col[ok]] = w[ok]
    Sm = A * np.outer(dinv, dinv).astype(np.float64)
    for p in S.KERNEL_PS:
        X = [g.standard_normal((257, p + 3)).astype(np.float32) for _ in range(3)]
        assert np.abs(S.product(rowptr, col, w, dinv, X[0], p) - Sm @ X[0][:, :p]).max() < 1e-5, p
        coef = g.standard_normal((4, 3)).astype(np.float32)
        out = S.spmm_recur(rowptr, col, w, dinv, *X, p, coef)
        Y = [x.astype(np.float64) for x in X]
        for t in range(4):
            Y[(t + 1) % 3][:, :p] = coef[t, 0] * (Sm @ Y[t % 3][:, :p]) + coef[t, 1] * Y[t % 3][:, :p] + coef[t, 2] * Y[(t + 2) % 3][:, :p]
        for a, b, x in zip(out, Y, X):
            assert np.abs(a - b).max() < 1e-4 and np.array_equal(a[:, p:], x[:, p:]), "columns at or past p are not touched"
    poisoned = S.spmm_recur(rowptr, col, w, dinv, X[0], X[1], np.full_like(X[2], np.nan), 32, np.array([[1.0, 0.5, 0.0]], dtype=np.float32))
    assert np.isfinite(poisoned[1][:, :32]).all(), "a coefficient of exactly 0 skips its term"
    A_, B_ = g.standard_normal((300, 5)).astype(np.float32), g.standard_normal((300, 7)).astype(np.float32)
    assert np.abs(S.tall_gram(A_, B_) - A_.astype(np.float64).T @ B_.astype(np.float64)).max() < 1e-12
    assert S.gram_blocks(0) == (0, 0) and S.gram_blocks(64) == (64, 1) and S.gram_blocks(65) == (64, 2) and S.gram_blocks(65536) == (64, 1024)
    assert S.gram_blocks(65537) == (128, 513) and S.gram_blocks(2 ** 24) == (16384, 1024)
    T = g.standard_normal((5, 5))
    T[:, 0] = np.eye(5)[0]
    out = S.tall_mul(A_, T)
    assert np.array_equal(out[:, 0], A_[:, 0]) and np.abs(out - A_.astype(np.float64) @ T).max() < 1e-6, "a unit column copies"


def test_the_coefficients_are_the_librarys_and_the_filter_is_one_at_one():
    from variantformer_amd import manifold
    for bound in (-0.99, -0.3, 0.5, 0.98, 1.0 - 1e-7):
        for degree in (2, 20, 40, 80):
            coef = S.chebyshev(bound, degree)
            assert np.array_equal(coef, manifold.chebyshev_coefficients(bound, degree)) and coef.shape == (degree, 3) and coef[0, 2] == 0
            for x, want in ((1.0, 1.0), (bound, None), (-1.0, None), ((bound - 1) / 2, None)):
                y, prev = 1.0, 0.0
                for c0, c1, c2 in coef.astype(np.float64):
                    y, prev = c0 * x * y + c1 * y + c2 * prev, y
                if want is not None:
                    assert abs(y - want) < 1e-4, (bound, degree, y)
                else:
                    assert abs(y) < 1.0 + 1e-4, "inside [-1, bound] the filter stays below its value at 1"
    G = np.random.default_rng(3).standard_normal((50, 6))
    G = G.T @ G
    T = S.orth_matrix(G)
    assert np.array_equal(T, manifold.orthonormalising_matrix(G)) and T[0, 0] == 1 and (T[1:, 0] == 0).all()
    B = T.T @ G @ T
    assert np.abs(B[1:, 1:] - np.eye(5)).max() < 1e-12 and np.abs(B[0, 1:]).max() < 1e-12, "orthonormal, and orthogonal to the locked column"
    assert (S.FILTER_LOW, S.FILTER_HIGH, S.ORTH_FLOOR) == (manifold.FILTER_LOW, manifold.FILTER_HIGH, manifold.ORTH_FLOOR)


def test_the_table_graphs_are_what_they_are_for():
    for name, (make, k) in S.CONNECTED.items():
        rowptr, col, w = make()
        assert S.components(rowptr, col, w)[0] == 1, f"{name} is connected"
        A = S.dense(rowptr, col, w)
        assert np.array_equal(A, A.T) and (np.diag(A) == 0).all() and (w > 0).all() and rowptr.shape[0] - 1 >= k + 2
        assert all((np.diff(col[a:b]) > 0).all() for a, b in zip(rowptr[:-1], rowptr[1:])), "columns ascend within a row"
    lam = S.truth("ring64")[0]
    assert lam[2] - lam[1] < 1e-12 and lam[3] - lam[2] > 1e-2, "a degenerate pair"
    lam = S.truth("blobs-bridged")[0]
    assert 1e-6 < lam[1] < 3e-6 and lam[2] > 0.9, "an eigengap of 2e-6 between the trivial and the Fiedler vector"
    lam = S.truth("path257")[0]
    assert lam[2] - lam[1] < S.GAP and S.cluster(lam, 1)[0] == 0, "the path's lowest eigenvalues form one cluster"
    assert S.cluster(S.truth("path65")[0], 1) == (1, 1) and S.cluster(S.truth("strip400")[0], 3) == (3, 3)
    for name, want in (("blobs-apart", 2), ("isolated", 2)):
        count, labels = S.components(*S.DISCONNECTED[name][0]())
        assert count == want and labels[-1] == (40 if name == "blobs-apart" else 64)
    for R in S.SMALL:
        rowptr, col, w = S.path(R)
        assert rowptr.shape[0] == R + 1 and col.shape[0] == 2 * (R - 1) and R < 2 + 2


@pytest.mark.parametrize("name", sorted(S.CONNECTED))
def test_the_reference_converges_and_is_accurate(name):
    truth = S.truth(name)
    k = S.CONNECTED[name][1]
    for degree in (20, 40):
        y, info = S.reference(name, degree)
        eig, vec, sub = S.deviations(y, info["eigenvalues"], truth)
        res = S.residuals64(y, truth)
        print(f"[spectral reference] {name} degree {degree}: {info['iterations']} outer iterations, {info['products']} products, "
              f"residuals {np.array2string(info['residuals'], precision=2)}, in fp64 {res.max():.2e}; eigenvalues {eig:.2e}, "
              f"vectors {vec:.2e}, subspaces {sub:.2e}")
        assert info["converged"] and info["iterations"] <= S.ITERATIONS_CAP and (info["residuals"][1:] < 1e-4).all()
        assert y.shape == (truth[0].shape[0], k) and y.dtype == np.float32 and info["eigenvalues"].shape == (k + 1,)
        assert (res < 2e-4).all() and np.abs(np.linalg.norm(y.astype(np.float64), axis=0) - 1).max() < 1e-6 and S.sign_rule_holds(y)
        assert eig <= S.EIG_ATOL and vec <= S.VEC_ATOL and sub <= S.SUB_ATOL
    assert S.EIG_ATOL == 8 * S.EIG_MEASURED and S.VEC_ATOL == 8 * S.VEC_MEASURED and S.SUB_ATOL == 8 * S.SUB_MEASURED
    if name == "blobs-bridged":
        side = y[:, 0] > 0
        assert (side[:40] == side[0]).all() and (side[40:] == side[40]).all() and side[0] != side[40], "the Fiedler vector's sign separates the blobs"


# ---- 3. argument checks --------------------------------------------------------------------------------------------------------------
def test_spectral_embedding_checks_its_arguments_before_the_device():
    from variantformer_amd import manifold
    graph = S.path(65)
    prm = inspect.signature(manifold.spectral_embedding).parameters
    assert [(n, p.default) for n, p in prm.items()] == [("graph", inspect.Parameter.empty), ("n_components", 2), ("block", 16), ("degree", 40),
                                                        ("tol", 1e-4), ("max_iter", 50), ("seed", 42), ("return_info", False)]
    assert all(prm[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("block", "degree", "tol", "max_iter", "seed", "return_info"))
    assert list(inspect.signature(manifold.spectral_init).parameters) == ["graph", "n_components", "seed"]
    for kwargs, name in ((dict(n_components=0), "n_components"), (dict(n_components=9), "n_components"), (dict(n_components=2.0), "n_components"),
                         (dict(n_components=2, block=2), "block"), (dict(n_components=8, block=8), "block"), (dict(block=33), "block"),
                         (dict(degree=1), "degree"), (dict(degree=40.0), "degree"), (dict(tol=0.0), "tol"), (dict(tol=-1e-4), "tol"),
                         (dict(tol=float("nan")), "tol"), (dict(max_iter=-1), "max_iter"), (dict(seed=-1), "seed"), (dict(seed=2 ** 32), "seed")):
        with pytest.raises(ValueError, match=name):
            manifold.spectral_embedding(graph, **kwargs)
    for bad in (graph[:2], (graph[0], graph[1], graph[2][:-1]), "graph", (graph[0].reshape(-1, 1), graph[1], graph[2])):
        with pytest.raises(ValueError, match="graph"):
            manifold.spectral_embedding(bad)
        with pytest.raises(ValueError, match="graph"):
            manifold.graph_components(bad)
    with pytest.raises(ValueError, match="n_components"):
        manifold.spectral_init(graph, 0, 42)
    if not torch.cuda.is_available():
        for call in (lambda: manifold.spectral_embedding(graph), lambda: manifold.spectral_init(graph, 2, 42), lambda: manifold.graph_components(graph)):
            with pytest.raises(Exception, match="GPU"):
                call()


def test_a_callable_init_is_accepted_and_its_result_checked():
    from variantformer_amd import manifold
    x = np.random.default_rng(0).standard_normal((40, 6)).astype(np.float32)
    with pytest.raises(ValueError, match=r"init.*manifold\.spectral_init"):
        manifold.umap(x, init="spectral")
    with pytest.raises(ValueError, match="init"):
        manifold.umap(x, init="laplacian")
    with pytest.raises(ValueError, match="init"):
        manifold.umap(x, init=7)
    seen = []

    def init(graph, n_components, seed):
        seen.append((graph, n_components, seed))
        return np.zeros((40, 3), dtype=np.float32)
    for result in (lambda *a: np.zeros((40, 3), dtype=np.float32), lambda *a: torch.zeros(39, 2), lambda *a: [[0.0, 0.0]] * 40, lambda *a: None):
        with pytest.raises(ValueError, match="init"):
            manifold._called_init(result, ("rowptr", "col", "w"), 40, 2, 42)
    with pytest.raises(ValueError, match="init"):
        manifold._called_init(init, ("rowptr", "col", "w"), 40, 2, 7)
    assert seen == [(("rowptr", "col", "w"), 2, 7)], "the callable gets (graph, n_components, seed)"
    good = manifold._called_init(lambda *a: torch.ones(40, 2), None, 40, 2, 42)
    assert tuple(good.shape) == (40, 2)
    src = inspect.getsource(manifold.umap)
    assert "callable(init)" in src and "_called_init(init, (rowptr, col, w), R, n_components, seed)" in src and "rescale(y)" in src
    if not torch.cuda.is_available():
        with pytest.raises(Exception, match="GPU"):                   # a callable passes the argument checks: the device is next
            manifold.umap(x, n_neighbors=5, init=init)
        assert len(seen) == 1

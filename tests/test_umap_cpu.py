"""UMAP after the k-NN graph without a GPU: the boundary of include/vf_hip_umap.h (it parses, its three names are exported and
bound through _lib.ENTRIES), every refusal with its argument named, find_ab against
scipy's curve_fit, the exact parts of tests/umap_cases.py (due rule, hash, random initialisation), the reference's sigma against
its own equation, the reference's embedding of four blobs against the random initialisation it started from, and the argument
checks of manifold.umap and VCFProcessor.expression_umap."""
import inspect
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests import umap_cases as U
from tests import write_set_cases as W
from tests.conftest import REPO

NAMES = ["vf_umap_layout", "vf_umap_smooth_knn", "vf_umap_union"]
ARGS = {"vf_umap_smooth_knn": 12, "vf_umap_union": 11, "vf_umap_layout": 19}


def _header(name="vf_hip_umap.h") -> str:
    with open(os.path.join(REPO, "include", name)) as f:
        return f.read()


# ---- 1. header and binding ---------------------------------------------------------------------------------------------------------
def test_header_parses_and_its_names_are_exported_and_bound():
    from variantformer_amd import _lib
    from variantformer_amd.csrc import build as B
    text = _header()
    assert W.stream_entries(text) == NAMES
    assert sorted(_lib.ENTRIES["vf_hip_umap.h"]) == NAMES, "ctypes binding and vf_hip_umap.h disagree"
    assert "vf_umap.hip" in B.SOURCES and any(h.endswith("vf_hip_umap.h") for h in B.HEADERS)
    assert "vf_umap.hip" not in B.EXTRA_FLAGS                         # absent entries are recognised by NaN / Inf: no -fno-honor-nans
    with open(os.path.join(REPO, "variantformer_amd", "csrc", "vf_umap.hip")) as f:
        assert "#pragma clang fp contract(off)" in f.read(), "w[i->j] and w[j->i] have the same bits only without an fma"
    bound = _lib.load()
    assert {name: len(_lib.SIGNATURES[name]) for name in NAMES} == ARGS
    assert _lib.ABI_VERSION == 13 and bound.vf_version() == 13
    assert "nine headers" in text
    for word in ("Arguments", "Write set", "Arithmetic", "Non-finite operands", "Refused before anything is launched", "Not checked"):
        assert text.count(word) >= 3, f"an entry's comment contract has no `{word}` part"
    for macro, value in (("VF_UMAP_MAX_M", "63"), ("VF_UMAP_MAX_DIM", "8"), ("VF_UMAP_MAX_R", "(1 << 24)"), ("VF_UMAP_SMOOTH_ITERS", "64")):
        assert re.search(rf"#define\s+{macro}\s+{re.escape(value)}\s", text), macro
    assert "Y0 if epoch_end - epoch_begin is even" in text, "the header says which buffer holds the result"
    assert "0x7FEB352D" in text and "0x846CA68B" in text and "0x9E3779B9" in text, "the header states the hash"


def _err(lib):
    return lib.vf_last_error().decode()


P = 4096                                                 # a non-null, aligned address; never dereferenced
INVALID = 1


def test_smooth_knn_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(idx=P, ld_idx=63, dist=P, ld_dist=63, R=0, m=29, mean_dist=0.5, rho=P, sigma=P, strength=P, ld_strength=63):
        return lib.vf_umap_smooth_knn(idx, ld_idx, dist, ld_dist, R, m, mean_dist, rho, sigma, strength, ld_strength, 0)
    assert call() == 0 and call(m=1) == 0 and call(m=63) == 0         # R = 0: nothing launched
    for name in ("idx", "dist", "rho", "sigma", "strength"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        assert call(**{name: P + 2}) == INVALID and re.search(rf"\b{name} must be 4-byte aligned", _err(lib)), _err(lib)
    for m in (0, -1, 64):
        assert call(m=m, ld_idx=64, ld_dist=64, ld_strength=64) == INVALID and _err(lib).split(": ")[1].startswith("m="), _err(lib)
    assert call(R=-1) == INVALID and "R=" in _err(lib)
    assert call(R=2 ** 24 + 1) == INVALID and "R=" in _err(lib) and "2^24" in _err(lib)
    for name in ("ld_idx", "ld_dist", "ld_strength"):
        assert call(**{name: 28}) == INVALID and _err(lib).split(": ")[1].startswith(f"{name}="), _err(lib)


def test_union_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(idx=P, ld_idx=63, strength=P, ld_strength=63, R=0, m=29, rowptr=P, col=P, nnz=5, w=P):
        return lib.vf_umap_union(idx, ld_idx, strength, ld_strength, R, m, rowptr, col, nnz, w, 0)
    assert call() == 0 and call(R=7, nnz=0) == 0 and call(R=7, nnz=0, col=0, w=0) == 0     # nothing launched
    for name in ("idx", "strength", "rowptr", "col", "w"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        align = 8 if name == "rowptr" else 4
        assert call(**{name: P + align // 2}) == INVALID and re.search(rf"\b{name} must be {align}-byte aligned", _err(lib)), _err(lib)
    for m in (0, 64):
        assert call(m=m, ld_idx=64, ld_strength=64) == INVALID and _err(lib).split(": ")[1].startswith("m="), _err(lib)
    assert call(R=-1) == INVALID and "R=" in _err(lib)
    assert call(R=2 ** 24 + 1) == INVALID and "R=" in _err(lib) and "2^24" in _err(lib)
    for name in ("ld_idx", "ld_strength"):
        assert call(**{name: 28}) == INVALID and _err(lib).split(": ")[1].startswith(f"{name}="), _err(lib)
    assert call(nnz=-1) == INVALID and "nnz=" in _err(lib)


def test_layout_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(rowptr=P, col=P, samples=P, nnz=5, R=0, dim=2, Y0=P, Y1=2 * P, ld=2, epoch_begin=0, epoch_end=10, N=10, rate=5):
        return lib.vf_umap_layout(rowptr, col, samples, nnz, R, dim, Y0, Y1, ld, epoch_begin, epoch_end, N, 1.5, 0.9, 1.0, 1.0, rate, 42, 0)
    assert call() == 0 and call(R=9, epoch_begin=4, epoch_end=4) == 0 and call(nnz=0, col=0, samples=0) == 0      # nothing launched
    for name in ("rowptr", "col", "samples", "Y0", "Y1"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        align = 8 if name == "rowptr" else 4
        assert call(**{name: P + align // 2}) == INVALID and re.search(rf"\b{name} must be {align}-byte aligned", _err(lib)), _err(lib)
    assert call(Y1=P) == INVALID and "Y0 and Y1" in _err(lib)
    assert call(R=-1) == INVALID and "R=" in _err(lib)
    assert call(R=2 ** 24 + 1) == INVALID and "R=" in _err(lib) and "2^24" in _err(lib)
    assert call(nnz=-1) == INVALID and "nnz=" in _err(lib)
    for dim in (0, 9):
        assert call(dim=dim, ld=16) == INVALID and _err(lib).split(": ")[1].startswith("dim="), _err(lib)
    assert call(dim=3) == INVALID and _err(lib).split(": ")[1].startswith("ld=")
    assert call(N=0, epoch_end=0) == INVALID and "N=" in _err(lib)
    assert call(epoch_begin=-1) == INVALID and "epoch_begin=" in _err(lib)
    assert call(epoch_begin=6, epoch_end=5) == INVALID and _err(lib).split(": ")[1].startswith("epoch_begin=")
    assert call(epoch_end=11) == INVALID and _err(lib).split(": ")[1].startswith("epoch_end=")
    assert call(rate=-1) == INVALID and "negative_sample_rate=" in _err(lib)


def test_the_wrappers_allocate_nothing_and_refuse_cpu_tensors():
    from variantformer_amd import manifold, ops
    for fn, outs in ((ops.umap_smooth_knn, ("rho", "sigma", "strength")), (ops.umap_union, ("w",)), (ops.umap_layout, ())):
        src = inspect.getsource(fn)
        assert not re.search(r"\b(empty|empty_like|zeros|zeros_like|ones|full|new_empty|new_zeros|new_full|tensor|arange|clone|contiguous)\s*\(", src)
        assert 'family="umap"' not in src and "family or _SCOPE" in src
        prm = inspect.signature(fn).parameters
        for o in outs:
            assert prm[o].kind is inspect.Parameter.KEYWORD_ONLY and prm[o].default is inspect.Parameter.empty
        assert fn.__name__ not in W.allocating_wrappers()
    assert W.uncovered_wrappers() == []
    i, f = torch.zeros((4, 3), dtype=torch.int32), torch.zeros((4, 3))
    with pytest.raises(Exception, match="GPU"):
        ops.umap_smooth_knn(i, f, 0.5, rho=torch.zeros(4), sigma=torch.zeros(4), strength=f.clone())
    with pytest.raises(Exception, match="GPU"):
        ops.umap_union(i, f, torch.zeros(5, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), w=torch.zeros(2))
    with pytest.raises(Exception, match="GPU"):
        ops.umap_layout(torch.zeros(5, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                        torch.zeros(4, 2), torch.zeros(4, 2), epoch_begin=0, epoch_end=1, n_epochs=1, a=1.5, b=0.9)
    assert inspect.getsource(manifold).count('family="umap"') == 3, "every launch of the driver is recorded under the family"
    assert not re.search(r"^\s*(import|from)\s+(scipy|umap|numba|pynndescent|sklearn)", inspect.getsource(manifold), flags=re.M)


# ---- 2. find_ab, and the exact parts of the reference -------------------------------------------------------------------------------
def test_find_ab_equals_scipys_curve_fit():
    from scipy.optimize import curve_fit
    from variantformer_amd import manifold
    worst = 0.0
    for min_dist in (0.001, 0.05, 0.1, 0.5, 0.99):
        x = np.linspace(0, 3.0, 300)                                  # umap-learn's find_ab_params, verbatim in what it fits
        y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / 1.0))
        (a_ref, b_ref), _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), x, y)
        a, b = manifold.find_ab(min_dist)
        da, db = abs(a - a_ref) / a_ref, abs(b - b_ref) / b_ref
        print(f"[umap find_ab] min_dist={min_dist}: a={a:.10f} b={b:.10f}, from scipy's by {da:.2e} and {db:.2e}")
        worst = max(worst, da, db)
        cost = lambda a, b: float(((1.0 / (1.0 + a * x ** (2 * b)) - y) ** 2).sum())     # noqa: E731
        assert cost(a, b) <= cost(a_ref, b_ref) * (1 + 1e-9), "the fit here is no worse than scipy's"
    print(f"[umap find_ab] largest relative difference {worst:.3e}; recorded {U.AB_MEASURED:.1e}, asserted {U.AB_RTOL:.1e}")
    assert U.AB_RTOL == 8 * U.AB_MEASURED and worst <= U.AB_RTOL
    a, b = manifold.find_ab(0.1)
    assert abs(a - 1.577) < 1e-3 and abs(b - 0.8951) < 1e-4, "umap-learn's documented values at min_dist = 0.1"
    for bad in (dict(min_dist=-0.1), dict(min_dist=1.5), dict(min_dist=0.1, spread=0.0), dict(min_dist=float("nan"))):
        with pytest.raises(ValueError, match="min_dist|spread"):
            manifold.find_ab(**bad)


def test_the_due_rule_draws_an_entry_exactly_samples_times():
    for N in (1, 2, 7, 10, 200, 500, 65535, 65536, 100003):
        s = np.unique(np.concatenate((np.arange(0, min(N, 40) + 1), [N // 2, N - 1, N], np.random.default_rng(N).integers(0, N + 1, 20))))
        if N <= 500:
            drawn = sum((U.due(s, n, N).astype(np.int64) for n in range(N)), np.zeros_like(s))
            assert np.array_equal(drawn, s), N
            half = sum((U.due(s, n, N).astype(np.int64) for n in range(N // 2)), np.zeros_like(s))
            assert np.array_equal(half, (N // 2) * s // N), "a prefix of the epochs draws its share: the schedule has no state"
        for n in (0, 1, N // 3, N - 1):                               # the device's form of the rule: (n s mod N) + s >= N
            assert np.array_equal(U.due(s, n, N), (s >= 1) & ((n * s) % N + s >= N)), (N, n)
    assert not U.due(np.array([-3, 0, 11]), 4, 10).any(), "a count outside 1 .. N is never due"
    big = np.array([2 ** 31 - 1, 2 ** 30 + 12345], dtype=np.int64)
    for n in (2 ** 31 - 2, 2 ** 30):
        want = [((n + 1) * int(v)) // (2 ** 31 - 1) > (n * int(v)) // (2 ** 31 - 1) for v in big]
        assert U.due(big, n, 2 ** 31 - 1).tolist() == want, "64-bit products"


def test_the_hash_is_the_headers_and_its_vertex_stays_below_R():
    def mix(x):                                                       # the header's five lines, on python integers
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)
    g = np.random.default_rng(5)
    values = np.concatenate(([0, 1, 0xFFFFFFFF, 0x80000000], g.integers(0, 2 ** 32, 200)))
    assert U.mix32(values).tolist() == [mix(int(v)) for v in values]
    assert len(set(U.mix32(np.arange(4096)).tolist())) == 4096, "the mixer is a bijection"
    for R in (1, 2, 63, 257, 18000, 2 ** 24):
        i = g.integers(0, R, 500)
        s = g.integers(0, 3000, 500)
        for seed, n, p in ((42, 0, 0), (2 ** 32 - 1, 199, 4), (0, 2 ** 31 - 2, 63)):
            k = U.negative_vertex(seed, n, i, s, p, R)
            assert k.dtype == np.int64 and (k >= 0).all() and (k < R).all(), R
            h = mix(mix(mix(mix(mix((seed + 0x9E3779B9) & 0xFFFFFFFF) ^ n) ^ int(i[7])) ^ int(s[7])) ^ p)
            assert k[7] == (h * R) >> 32
    k = U.negative_vertex(42, 3, np.arange(20000), np.zeros(20000, dtype=np.int64), 0, 16)
    assert np.abs(np.bincount(k, minlength=16) - 1250).max() < 150, "the vertices are spread evenly"


def test_random_init_is_the_librarys_and_rescale_spans_0_to_10():
    from variantformer_amd import manifold
    for rows, dim, seed in ((1, 1, 0), (65, 2, 42), (257, 8, 2 ** 32 - 1)):
        want = U.random_init(rows, dim, seed)
        got = manifold.random_init(rows, dim, seed, device="cpu").numpy()
        assert got.dtype == np.float32 and np.array_equal(got, want) and (want >= 0).all() and (want < 1).all()
        r = U.rescale(want)
        assert np.array_equal(manifold.rescale(torch.from_numpy(want)).numpy(), r)
        if rows > 1:
            assert (r.min(0) == 0).all() and (r.max(0) == 10).all()
        else:
            assert (r == 0).all(), "a coordinate without spread becomes 0"
    assert not np.array_equal(U.random_init(65, 2, 42), U.random_init(65, 2, 43))
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((50, 6)).astype(np.float32)) * torch.tensor([5.0, 3.0, 1.0, 0.5, 0.2, 0.1])
    y = manifold.pca_init(x, 2).numpy()
    xc = (x - x.mean(0)).numpy().astype(np.float64)
    _, _, vt = np.linalg.svd(xc, full_matrices=False)
    assert np.allclose(np.abs(y), np.abs(xc @ vt[:2].T), atol=1e-4), "the projection on the first two principal axes"
    axes = np.linalg.lstsq(xc, y.astype(np.float64), rcond=None)[0]
    assert (axes[np.abs(axes).argmax(0), np.arange(2)] > 0).all(), "each axis has its largest-magnitude component positive"


def test_the_references_sigma_solves_its_own_equation():
    for kind in U.SMOOTH_KINDS:
        idx, dist = U.smooth_case(kind, 65, 29)
        rho, sigma, strength, converged, floored = U.smooth_knn(idx, dist, U.mean_distance(idx, dist))
        p = U.present(idx, dist)
        solved = converged & ~floored
        assert (U.smooth_residual(idx, dist, rho, sigma)[solved] < U.SMOOTH_TOL).all(), kind
        assert ((strength >= 0) & (strength <= 1)).all() and (strength[~p] == 0).all(), kind
        none = ~p.any(1)
        assert (rho[none] == 0).all() and (sigma[none] == 0).all() and (strength[none] == 0).all()
        if kind == "random":
            assert solved.all() and strength[1, 0] == 0 and idx[1, 0] == 1, "a row that lists itself"
            # umap-learn's loop for one row, entry by entry
            d = dist[0].astype(np.float64)
            lo, hi, mid = 0.0, np.inf, 1.0
            for _ in range(64):
                psum = sum(np.exp(-((v - rho[0]) / mid)) if v - rho[0] > 0 else 1.0 for v in d)
                if abs(psum - np.log2(30)) < 1e-5:
                    break
                if psum > np.log2(30):
                    hi = mid
                    mid = (lo + hi) / 2
                else:
                    lo = mid
                    mid = mid * 2 if hi == np.inf else (lo + hi) / 2
            assert sigma[0] == mid and rho[0] == dist[0].min()
        if kind == "zeros":
            assert (rho[::2] == 0).all() and floored[::2].all() and (strength[::2][p[::2]] == 1).all() and (rho[1::2] > 0).all()
            assert U.mean_distance(idx, dist) > 0.1 and np.allclose(sigma[::2], 1e-3 * U.mean_distance(idx, dist)), "the global mean's floor"
        if kind == "tight":
            assert floored.all() and (rho > 0).all(), "the floor binds: 1e-3 of the row's mean distance"
        if kind == "wide":
            assert solved.all() and (sigma > 2 ** 15).all(), "hi stayed infinite for many doublings"
        if kind == "absent-row":
            assert none[::3].all() and not none[1::3].any()
        if kind == "nonfinite":
            assert (~np.isfinite(dist)).any(1).all() and np.isfinite(sigma).all() and np.isfinite(strength).all()


def test_the_reference_graph_is_symmetric():
    idx, dist = U.smooth_case("absent-tails", 65, 5)
    idx[7], dist[7] = -1, np.inf                                      # a row that lists nobody may still be listed
    _, _, strength, _, _ = U.smooth_knn(idx, dist, U.mean_distance(idx, dist))
    rowptr, col = U.csr(idx, dist)
    i, j = U.entry_rows(rowptr), col.astype(np.int64)
    pairs = set(zip(i.tolist(), j.tolist()))
    assert len(pairs) == col.shape[0] and all((b, a) in pairs for a, b in pairs) and not any(a == b for a, b in pairs)
    assert all((np.diff(col[rowptr[r]:rowptr[r + 1]]) > 0).all() for r in range(65)), "columns ascend within a row"
    listed = {(r, int(c)) for r in range(65) for c, d in zip(idx[r], dist[r]) if c >= 0 and np.isfinite(d) and c != r}
    assert pairs == listed | {(b, a) for a, b in listed}
    w = U.union(idx, strength, rowptr, col)
    back = {(a, b): v for a, b, v in zip(i.tolist(), j.tolist(), w.tolist())}
    assert all(back[(a, b)] == back[(b, a)] for a, b in pairs) and ((w > 0) & (w <= 1)).all()
    one_way = [(a, b) for a, b in listed if (b, a) not in listed]
    assert one_way and all(back[ab] == strength[ab[0], list(idx[ab[0]]).index(ab[1])] for ab in one_way[:20]), "one-way: w = a"
    s = U.edge_samples(w.astype(np.float32), 10)
    assert s.max() == 10 and s.min() >= 0 and s.dtype == np.int32


def test_the_reference_embeds_the_blobs_better_than_its_random_start():
    x = U.blobs()
    assert x.shape == (U.BLOBS["R"], U.BLOBS["d"]) == (400, 10) and U.BLOBS["n_neighbors"] == 15 and U.BLOBS["n_epochs"] == 100
    y = U.blobs_reference(42)
    assert y is U.blobs_reference(42), "a reference is computed once"
    start = U.rescale(U.random_init(400, 2, 42))
    t_ref, t_start = U.trust(x, y), U.trust(x, start)
    print(f"[umap blobs] trustworthiness: the reference {t_ref:.4f}, its random initialisation {t_start:.4f}; margin {U.TRUST_MARGIN}")
    assert np.isfinite(y).all() and t_ref > t_start + 0.2, "the reference alone meets the GPU test's condition"
    assert 0 < U.TRUST_MARGIN < 0.05


# ---- 3. argument checks --------------------------------------------------------------------------------------------------------------
def test_umap_checks_its_arguments_before_the_device():
    from variantformer_amd import manifold
    x = np.random.default_rng(0).standard_normal((40, 6)).astype(np.float32)
    prm = inspect.signature(manifold.umap).parameters
    assert [(n, p.default) for n, p in prm.items()] == [
        ("x", inspect.Parameter.empty), ("n_neighbors", 30), ("min_dist", 0.1), ("metric", "correlation"), ("n_components", 2),
        ("n_epochs", None), ("init", "pca"), ("seed", 42), ("negative_sample_rate", 5), ("repulsion_strength", 1.0), ("learning_rate", 1.0)]
    with pytest.raises(TypeError, match="numpy array or a torch tensor"):
        manifold.umap([[1.0, 2.0]])
    with pytest.raises(ValueError, match="matrix"):
        manifold.umap(x[0])
    for kwargs, name in ((dict(n_neighbors=1), "n_neighbors"), (dict(n_neighbors=65), "n_neighbors"), (dict(n_neighbors=True), "n_neighbors"),
                         (dict(n_neighbors=15.0), "n_neighbors"), (dict(min_dist=-0.1), "min_dist"), (dict(min_dist=1.5), "min_dist"),
                         (dict(metric="euclidean"), "metric"), (dict(n_components=0), "n_components"), (dict(n_components=9), "n_components"),
                         (dict(n_epochs=0), "n_epochs"), (dict(n_epochs=2.5), "n_epochs"), (dict(init="spectral"), "init"),
                         (dict(init=np.zeros((40, 3), dtype=np.float32)), "init"), (dict(init="pca", n_components=7), "init='pca'"),
                         (dict(seed=-1), "seed"), (dict(seed=2 ** 32), "seed"), (dict(negative_sample_rate=-1), "negative_sample_rate"),
                         (dict(repulsion_strength=-1.0), "repulsion_strength"), (dict(learning_rate=0.0), "learning_rate"),
                         (dict(learning_rate=float("inf")), "learning_rate")):
        with pytest.raises(ValueError, match=name):
            manifold.umap(x, **kwargs)
    i, d = U.knn_lists(9, 3, 1)
    with pytest.raises(ValueError, match="one shape"):
        manifold.fuzzy_graph(i, d[:, :2])
    with pytest.raises(ValueError, match="1 .. 63"):
        manifold.fuzzy_graph(np.zeros((3, 64), dtype=np.int32), np.zeros((3, 64), dtype=np.float32))
    with pytest.raises(TypeError, match="indices"):
        manifold.fuzzy_graph(i.tolist(), d)
    graph = (np.zeros(10, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
    y = np.zeros((9, 2), dtype=np.float32)
    for args, kwargs, name in (((graph[:2], y, 10, 1.5, 0.9), {}, "fuzzy_graph"), ((graph, np.zeros((9, 9), dtype=np.float32), 10, 1.5, 0.9), {}, "init"),
                               ((graph, np.zeros((8, 2), dtype=np.float32), 10, 1.5, 0.9), {}, "rows"), ((graph, y, 0, 1.5, 0.9), {}, "n_epochs"),
                               ((graph, y, 10, 0.0, 0.9), {}, "a must"), ((graph, y, 10, 1.5, -1.0), {}, "b must"),
                               ((graph, y, 10, 1.5, 0.9), dict(epoch_begin=6, epoch_end=5), "epoch_begin"),
                               ((graph, y, 10, 1.5, 0.9), dict(epoch_end=11), "epoch_end")):
        with pytest.raises(ValueError, match=name):
            manifold.layout(*args, **kwargs)
    if not torch.cuda.is_available():
        for call in (lambda: manifold.umap(x, n_neighbors=5), lambda: manifold.fuzzy_graph(i, d), lambda: manifold.layout(graph, y, 10, 1.5, 0.9)):
            with pytest.raises(Exception, match="GPU"):
                call()


def test_expression_umap_checks_the_frame():
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    prm = inspect.signature(VCFProcessor.expression_umap).parameters
    assert [(n, p.default) for n, p in prm.items()][1:5] == [("df", inspect.Parameter.empty), ("on", "predicted_expression"),
                                                             ("axis", "genes"), ("tissue", None)]
    assert prm["umap_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    vp = VCFProcessor(require_gpu=False)
    names = [f"tissue{t}" for t in range(4)]
    df = pd.DataFrame({"gene_id": [f"ENSG{i:03d}" for i in range(6)], "tissues": [list(range(4))] * 6, "tissue_names": [names] * 6,
                       "predicted_expression": [np.arange(4, dtype=np.float32).reshape(4, 1) * (i + 1) for i in range(6)]})
    with pytest.raises(ValueError, match="format_output"):
        vp.expression_umap(df.drop(columns=["predicted_expression"]))
    with pytest.raises(ValueError, match="format_output"):
        vp.expression_umap(df, on="embeddings")
    with pytest.raises(ValueError, match="axis"):
        vp.expression_umap(df, axis="rows")
    with pytest.raises(ValueError, match="n_neighbors"):
        vp.expression_umap(df, n_neighbors=100)
    with pytest.raises(ValueError, match="init"):
        vp.expression_umap(df, init="spectral")
    assert "umap_1" not in df.columns, "a refused call leaves the frame as it was"
    if not torch.cuda.is_available():
        with pytest.raises(Exception, match="GPU"):
            vp.expression_umap(df, n_neighbors=3)

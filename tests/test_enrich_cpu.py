"""Enrichment without a GPU: the boundary of include/vf_hip_enrich.h (it parses, its two names are exported and bound through
_lib.ENTRIES), every refusal of both entries and of the Python
functions with its argument named, the restatement of the tail rule (tests/enrich_cases.py) against exact integer arithmetic on
the exhaustive grid N <= 12 and on random cells, and against scipy.stats.hypergeom at N = 18 000; Benjamini-Hochberg against
scipy.stats.false_discovery_control bit for bit; linkage.cut against scipy's cut_tree; membership on hand-made annotations; and
the planted end-to-end case by scipy alone."""
import inspect
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests import enrich_cases as E
from tests import write_set_cases as W
from tests.conftest import REPO

NAMES = ["vf_enrich_counts", "vf_hypergeom_tail"]
ARGS = {"vf_enrich_counts": 11, "vf_hypergeom_tail": 14}


def _header(name="vf_hip_enrich.h") -> str:
    with open(os.path.join(REPO, "include", name)) as f:
        return f.read()


# ---- 1. header and binding ---------------------------------------------------------------------------------------------------------
def test_header_parses_and_its_names_are_exported_and_bound():
    from variantformer_amd import _lib
    from variantformer_amd.csrc import build as B
    text = _header()
    assert W.stream_entries(text) == NAMES
    assert sorted(_lib.ENTRIES["vf_hip_enrich.h"]) == NAMES, "ctypes binding and vf_hip_enrich.h disagree"
    assert "vf_enrich.hip" in B.SOURCES and any(h.endswith("vf_hip_enrich.h") for h in B.HEADERS)
    assert "vf_enrich.hip" not in B.EXTRA_FLAGS
    with open(os.path.join(REPO, "variantformer_amd", "csrc", "vf_enrich.hip")) as f:
        source = f.read()
    assert "#pragma clang fp contract(off)" in source, "tail and steps are restated bit for bit only without an fma"
    assert "hipDeviceSynchronize" not in source and "hipStreamSynchronize" not in source, "no entry synchronises the stream"
    assert "lgamma" not in re.sub(r"//.*", "", source), "the device computes no lgamma"
    atomics = re.findall(r"\b(\w*atomic\w*)\s*\(&?\s*(\w+)", source, flags=re.I)
    assert atomics and all(fn == "atomicAdd" and arg == "bins" for fn, arg in atomics), "integer additions on the LDS bins are the only atomics"
    bound = _lib.load()
    assert {name: len(_lib.SIGNATURES[name]) for name in NAMES} == ARGS
    assert _lib.ABI_VERSION == 13 and bound.vf_version() == 13
    assert "fourteenth header" in text and "contracted into a fused multiply-add" in text
    for word in ("Arguments", "Write set", "Arithmetic", "Non-finite operands", "Refused before anything is launched", "Not checked"):
        assert text.count(word) >= 2, f"an entry's comment contract has no `{word}` part"
    for macro, value in (("VF_ENRICH_MAX_K", str(E.MAX_K)), ("VF_ENRICH_MAX_N", "(1 << 24)"), ("VF_ENRICH_THREADS", str(E.THREADS)),
                         ("VF_ENRICH_STOP", "0x1p-60")):
        assert re.search(rf"#define\s+{macro}\s+{re.escape(value)}\s", text), macro
    assert float.fromhex("0x1p-60") == E.STOP
    from variantformer_amd import enrichment, ops
    assert (ops.ENRICH_MAX_K, ops.ENRICH_MAX_N) == (E.MAX_K, E.MAX_N) == (enrichment.MAX_K, enrichment.MAX_N)


def _err(lib):
    return lib.vf_last_error().decode()


P = 4096                                                 # a non-null, aligned address; never dereferenced
INVALID = 1


def test_counts_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(termptr=P, gene=P, nnz=9, T=0, labels=P, G=300, k=50, count=P, ldc=50, size=P):
        return lib.vf_enrich_counts(termptr, gene, nnz, T, labels, G, k, count, ldc, size, 0)
    assert call() == 0 and call(nnz=0, gene=0) == 0 and call(k=1, ldc=1) == 0 and call(k=4096, ldc=4096, G=0) == 0      # T = 0: nothing launched
    for name in ("termptr", "gene", "labels", "count", "size"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        align = 8 if name == "termptr" else 4
        assert call(**{name: P + align // 2}) == INVALID and re.search(rf"\b{name} must be {align}-byte aligned", _err(lib)), _err(lib)
    assert call(nnz=-1) == INVALID and "nnz=" in _err(lib)
    assert call(T=-1) == INVALID and "T=" in _err(lib)
    assert call(T=2 ** 24 + 1) == INVALID and "T=" in _err(lib) and "2^24" in _err(lib)
    assert call(G=-1) == INVALID and "G=" in _err(lib)
    assert call(G=2 ** 24 + 1) == INVALID and "G=" in _err(lib) and "2^24" in _err(lib)
    for k in (0, -1, 4097):
        assert call(k=k, ldc=5000) == INVALID and _err(lib).split(": ")[1].startswith("k="), _err(lib)
    assert call(ldc=49) == INVALID and _err(lib).split(": ")[1].startswith("ldc="), _err(lib)


def test_tail_refusals_without_gpu():
    from variantformer_amd import _lib
    lib = _lib.load()

    def call(count=P, ldc=50, size=P, csize=P, T=0, k=50, N=18000, logfact=P, alternative=0, log_p=P, tail=2 * P, steps=3 * P, ldo=50):
        return lib.vf_hypergeom_tail(count, ldc, size, csize, T, k, N, logfact, alternative, log_p, tail, steps, ldo, 0)
    assert call() == 0 and call(alternative=1) == 0 and call(N=0) == 0 and call(N=2 ** 24, k=4096, ldc=4096, ldo=4096) == 0    # T = 0: nothing launched
    for name in ("count", "size", "csize", "logfact", "log_p", "tail", "steps"):
        assert call(**{name: 0}) == INVALID and _err(lib).endswith(f"null pointer {name}"), _err(lib)
        align = 8 if name in ("logfact", "log_p", "tail") else 4
        assert call(**{name: P + align // 2}) == INVALID and re.search(rf"\b{name} must be {align}-byte aligned", _err(lib)), _err(lib)
    assert call(T=-1) == INVALID and "T=" in _err(lib)
    assert call(T=2 ** 24 + 1) == INVALID and "T=" in _err(lib) and "2^24" in _err(lib)
    for k in (0, -3, 4097):
        assert call(k=k, ldc=5000, ldo=5000) == INVALID and _err(lib).split(": ")[1].startswith("k="), _err(lib)
    assert call(N=-1) == INVALID and "N=" in _err(lib)
    assert call(N=2 ** 24 + 1) == INVALID and "N=" in _err(lib) and "2^24" in _err(lib)
    assert call(ldc=49) == INVALID and _err(lib).split(": ")[1].startswith("ldc="), _err(lib)
    assert call(ldo=49) == INVALID and _err(lib).split(": ")[1].startswith("ldo="), _err(lib)
    for alternative in (-1, 2):
        assert call(alternative=alternative) == INVALID and _err(lib).split(": ")[1].startswith("alternative="), _err(lib)


def test_the_wrappers_allocate_nothing_and_refuse_cpu_tensors():
    from variantformer_amd import enrichment, ops
    for fn, outs in ((ops.enrich_counts, ("count", "size")), (ops.hypergeom_tail, ("log_p", "tail", "steps"))):
        src = inspect.getsource(fn)
        assert not re.search(r"\b(empty|empty_like|zeros|zeros_like|ones|full|new_empty|new_zeros|new_full|tensor|arange|clone|contiguous)\s*\(", src)
        assert "family or _SCOPE" in src
        prm = inspect.signature(fn).parameters
        for o in outs:
            assert prm[o].kind is inspect.Parameter.KEYWORD_ONLY and prm[o].default is inspect.Parameter.empty
        assert fn.__name__ not in W.allocating_wrappers()
    assert W.uncovered_wrappers() == []
    termptr, gene, labels = torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), torch.zeros(9, dtype=torch.int32)
    count, size = torch.zeros((2, 3), dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(Exception, match="GPU"):
        ops.enrich_counts(termptr, gene, labels, 3, count=count, size=size)
    with pytest.raises(Exception, match="GPU"):
        ops.hypergeom_tail(count, size, torch.zeros(3, dtype=torch.int32), 9, torch.zeros(10, dtype=torch.float64), 0,
                           log_p=torch.zeros((2, 3), dtype=torch.float64), tail=torch.zeros((2, 3), dtype=torch.float64),
                           steps=torch.zeros((2, 3), dtype=torch.int32))
    assert inspect.getsource(enrichment).count('family="enrich"') == 3, "every launch of the driver is recorded under the family"
    assert not re.search(r"^\s*(import|from)\s+(scipy|statsmodels)", inspect.getsource(enrichment), flags=re.M)
    lf = enrichment.log_factorials(50)
    assert lf.dtype == np.float64 and lf.shape == (51,) and all(lf[i] == math.lgamma(i + 1.0) for i in range(51)), "the host's math.lgamma"
    assert np.array_equal(lf, E.log_factorials(50))


def test_the_python_functions_check_their_arguments_before_the_device():
    from variantformer_amd import enrichment, linkage
    from variantformer_amd.processors.vcfprocessor import VCFProcessor
    universe = [f"g{i}" for i in range(8)]
    ann = {"g0": ["a", "b"], "g1": ["a"], "g2": ["b"], "g9": ["a"]}
    m = enrichment.membership(ann, universe)
    labels = np.array([0, 0, 1, 1, -1, 2, 2, 0])
    for bad, err, word in (((ann, "g0"), TypeError, "universe"), ((ann, 5), TypeError, "universe"), ((ann, ["g0", "g0"]), ValueError, "twice"),
                           (([1, 2], universe), TypeError, "annotations"), (({"g0": 7}, universe), TypeError, "terms of gene"),
                           ((pd.DataFrame({"a": [1], "b": [2], "c": [3]}), universe), ValueError, "two columns")):
        with pytest.raises(err, match=word):
            enrichment.membership(*bad)
    for kw, word in ((dict(min_size=-1), "min_size"), (dict(min_size=1.5), "min_size"), (dict(min_size=3, max_size=2), "max_size"), (dict(max_size=True), "max_size")):
        with pytest.raises(ValueError, match=word):
            enrichment.membership(ann, universe, **kw)
    for args, kw, err, word in (((labels, (m.termptr, m.gene)), {}, TypeError, "membership"), (([0] * 8, m), {}, TypeError, "labels must be"),
                                ((labels[:7], m), {}, ValueError, "one integer per gene"), ((labels.astype(np.float32), m), {}, ValueError, "integers"),
                                ((labels > 0, m), {}, ValueError, "integers"), ((np.full(8, -1), m), {}, ValueError, "no cluster"),
                                ((labels + 4096, m), {}, ValueError, "n_clusters"), ((labels, m), dict(n_clusters=0), ValueError, "n_clusters"),
                                ((labels, m), dict(n_clusters=4097), ValueError, "n_clusters"), ((labels, m), dict(alternative="two-sided"), ValueError, "alternative"),
                                ((labels, m._replace(termptr=m.termptr.astype(np.int32))), {}, ValueError, "termptr"),
                                ((labels, m._replace(gene=m.gene + 8)), {}, ValueError, "rows of the universe"),
                                ((labels, m._replace(termptr=m.termptr[::-1].copy())), {}, ValueError, "rise from 0")):
        with pytest.raises(err, match=word):
            enrichment.hypergeom(*args, **kw)
    for kw, word in ((dict(fdr=0.0), "fdr"), (dict(fdr=1.5), "fdr"), (dict(fdr="5%"), "fdr"), (dict(alternative="both"), "alternative"),
                     (dict(cluster_names=["x"]), "cluster_names"), (dict(min_size=-2), "min_size")):
        with pytest.raises(ValueError, match=word):
            enrichment.enrich(labels, ann, universe, **kw)
    with pytest.raises(ValueError, match="universe"):
        enrichment.enrich(labels, ann)
    with pytest.raises(ValueError, match="universe=None"):
        enrichment.enrich(labels, m, universe)
    if not torch.cuda.is_available():
        with pytest.raises(Exception, match="GPU"):
            enrichment.hypergeom(labels, m)
        with pytest.raises(Exception, match="GPU"):
            enrichment.enrich(labels, ann, universe, min_size=1)
    Z = np.array([[0, 1, 1.0, 2], [2, 3, 2.0, 2], [4, 5, 3.0, 4]])
    for bad, word in ((dict(Z=Z[:, :3], n_clusters=2), "linkage matrix"), (dict(Z=Z, n_clusters=0), "n_clusters"), (dict(Z=Z, n_clusters=5), "n_clusters"),
                      (dict(Z=Z, n_clusters=2.0), "n_clusters"), (dict(Z=Z, n_clusters=[]), "at least one"), (dict(Z=Z, n_clusters=[2, True]), "n_clusters"),
                      (dict(Z=Z[::-1].copy(), n_clusters=2), "not made before"), (dict(Z=np.array([[0, 1, 2.0, 2], [2, 3, 1.0, 2], [4, 5, 3.0, 4]]), n_clusters=2), "monotone"),
                      (dict(Z=np.array([[0, 1, 1.0, 2], [0, 3, 2.0, 2], [4, 5, 3.0, 4]]), n_clusters=2), "exactly once")):
        with pytest.raises(ValueError, match=word):
            linkage.cut(**bad)
    frame = pd.DataFrame({"gene_id": universe, "tissues": [[0, 1, 2]] * 8, "predicted_expression": [np.arange(3, dtype=np.float32)] * 8, "kind": list("aabbccdd")})
    proc = VCFProcessor.__new__(VCFProcessor)
    for kw, word in ((dict(axis="tissues"), "axis"), (dict(labels=None), "n_clusters"), (dict(labels="nothing"), "neither a column"),
                     (dict(labels="kind", universe=universe), "sets universe"), (dict(n_clusters=0), "n_clusters"), (dict(n_clusters=9), "n_clusters"),
                     (dict(labels=labels, fdr=2.0), "fdr")):
        with pytest.raises(ValueError, match=word):
            VCFProcessor.expression_enrichment(proc, frame, ann, **kw)
    assert list(inspect.signature(VCFProcessor.expression_enrichment).parameters)[:8] == ["self", "df", "annotations", "labels", "n_clusters", "on", "axis", "tissue"]


# ---- 2. the tail rule against exact arithmetic --------------------------------------------------------------------------------------
def _against_exact(cells, what):
    """cells: iterable of (x, K, n, N, alternative).  Holds every cell to exact arithmetic; returns the largest deviation / bound."""
    worst, worst_dev, most_steps, tables = 0.0, 0.0, 0, {}
    for x, K, n, N, alt in cells:
        lf = tables.setdefault(N, E.log_factorials(N))
        lp, s, steps, kind, x0 = E.tail_cell(x, K, n, N, alt, lf)
        exact = E.exact_log_tail(x, K, n, N, alt)
        if x0 is None:
            assert kind in ("-inf", "zero") and (lp == exact), ("exactly 0 or -Inf where the contract says so", x, K, n, N, alt, lp, exact)
            assert s == 0.0 and steps == 0
            continue
        assert 1.0 <= s <= steps + 1, "every ratio is at most 1: the sum runs away from the mode"
        bound = E.derived_bound(lf, x0, K, n, N, steps)
        dev = abs(lp - exact)
        most_steps = max(most_steps, steps)
        if dev / bound > worst:
            worst, worst_dev = dev / bound, dev
        assert dev <= bound, (x, K, n, N, alt, kind, lp, exact, dev, bound)
    print(f"[enrich exact] {what}: largest deviation / derived bound {worst:.3f} (deviation {worst_dev:.3e}), longest sum {most_steps} steps")
    return worst


def test_the_rule_holds_exact_arithmetic_on_the_exhaustive_grid():
    cells = ((x, K, n, N, alt) for alt in (E.GREATER, E.LESS) for N in range(E.GRID_MAX_N + 1) for K in range(N + 1) for n in range(N + 1)
             for x in range(-1, N + 2))
    assert _against_exact(cells, f"all (N, K, n, x) with N <= {E.GRID_MAX_N}, both alternatives") <= 1.0


def test_the_rule_holds_exact_arithmetic_on_random_cells():
    rng = np.random.default_rng(1)
    cells = []
    for alt in (E.GREATER, E.LESS):
        for _ in range(300):
            N = int(rng.integers(13, 1001))
            K, n = int(rng.integers(0, N + 1)), int(rng.integers(0, N + 1))
            lo, hi, mode = E.support(N, K, n)
            x = (int(rng.integers(lo, hi + 1)), lo, hi, mode, mode + 1, max(mode - 1, lo))[int(rng.integers(0, 6))]
            cells.append((min(max(x, lo), hi), K, n, N, alt))
    assert _against_exact(cells, "600 random cells with N <= 1000") <= 1.0


def test_the_rule_restates_scipy_at_the_notebooks_universe():
    stats = pytest.importorskip("scipy.stats", reason="scipy is not installed")
    N = E.BIG_N
    count, size, csize = E.big_table()
    lf = E.log_factorials(N)
    # scipy's own deviation from exact arithmetic, where exact sums are affordable: K, n <= 600
    rows, cols = np.flatnonzero(size <= 600)[:12], np.flatnonzero(csize <= 600)[:6]
    own = {E.GREATER: 0.0, E.LESS: 0.0}
    for alt in (E.GREATER, E.LESS):
        for t in rows:
            for c in cols:
                x, K, n = int(count[t, c]), int(size[t]), int(csize[c])
                ref = float(stats.hypergeom.sf(x - 1, N, K, n)) if alt == E.GREATER else float(stats.hypergeom.cdf(x, N, K, n))
                if ref <= 1e-280:
                    continue
                exact = E.exact_log_tail(x, K, n, N, alt)
                own[alt] = max(own[alt], abs(math.log(ref) - exact))
                lp, _, steps, _, x0 = E.tail_cell(x, K, n, N, alt, lf)
                if x0 is not None:
                    assert abs(lp - exact) <= E.derived_bound(lf, x0, K, n, N, steps), "the rule against exact sums at N = 18 000"
    for alt, name in ((E.GREATER, "greater / sf"), (E.LESS, "less / cdf")):
        got = E.tail_cells(count, size, csize, N, alt, lf)
        xs, Ks, ns = count.astype(np.int64), np.broadcast_to(size[:, None], count.shape), np.broadcast_to(csize[None, :], count.shape)
        ref = stats.hypergeom.sf(xs - 1, N, Ks, ns) if alt == E.GREATER else stats.hypergeom.cdf(xs, N, Ks, ns)
        held = ref > 1e-280
        with np.errstate(divide="ignore", invalid="ignore"):
            dev = np.abs(got["log_p"] - np.log(ref))
        # the derived bound of the rule, plus four times scipy's own measured deviation from exact arithmetic
        bound = got["bound"] + 4.0 * own[alt] + 2.0 ** -50
        worst = float((dev[held] / bound[held]).max())
        print(f"[enrich scipy] N={N} {name}: {int(held.sum())} of {held.size} cells above 1e-280; largest |log p - log scipy| {float(dev[held].max()):.3e}, "
              f"largest derived bound {float(got['bound'].max()):.3e}, scipy's own deviation from exact sums {own[alt]:.3e}, deviation / bound {worst:.3f}; "
              f"longest sum {int(got['steps'].max())} steps")
        assert held.sum() >= 0.6 * held.size and (dev[held] <= bound[held]).all()
        assert (got["log_p"][~held] < math.log(1e-279)).all(), "where scipy underflows the logarithm goes on"


# ---- 3. Benjamini-Hochberg ------------------------------------------------------------------------------------------------------------
def test_q_equals_false_discovery_control_bit_for_bit():
    stats = pytest.importorskip("scipy.stats", reason="scipy is not installed")
    if not hasattr(stats, "false_discovery_control"):
        pytest.skip("this scipy has no false_discovery_control")
    from variantformer_amd import enrichment
    rng = np.random.default_rng(4)
    for shape in ((1, 1), (7, 3), (50, 30), (1, 1000)):
        p = rng.random(shape) ** 4
        p[rng.random(shape) < 0.2] = 1.0                              # ties at 1, as cells without an overlap give
        p.ravel()[0] = 0.0
        if p.size > 5:
            p.ravel()[3] = p.ravel()[5]                               # a tie below 1
        want = stats.false_discovery_control(p.ravel(), method="bh").reshape(shape)
        got = E.bh(p)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), "the numpy restatement"
        dev = enrichment._bh(torch.from_numpy(p)).numpy()
        assert np.array_equal(dev.view(np.uint64), want.view(np.uint64)), "the torch form, here on the host"


# ---- 4. cut ---------------------------------------------------------------------------------------------------------------------------
def _same_partition(a, b) -> bool:
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def test_cut_gives_cut_trees_partition_on_random_ward_trees():
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy", reason="scipy is not installed")
    from variantformer_amd import linkage
    for n, seed in ((2, 0), (3, 1), (17, 2), (64, 3), (301, 4)):
        x = np.random.default_rng(seed).standard_normal((n, 5))
        Z = hierarchy.ward(x)
        wanted = sorted({1, 2, min(3, n), max(n // 2, 1), n - 1, n})
        got = linkage.cut(Z, wanted)
        # one call per count: with the list [1, 2] over two rows scipy's cut_tree returns one cluster for both
        ref = np.concatenate([hierarchy.cut_tree(Z, n_clusters=c) for c in wanted], axis=1)
        assert got.dtype == np.int32 and got.shape == (n, len(wanted))
        for j, c in enumerate(wanted):
            assert _same_partition(got[:, j], ref[:, j]) and len(set(got[:, j].tolist())) == c, (n, c)
            first = [int(np.flatnonzero(got[:, j] == v)[0]) for v in range(c)]
            assert first == sorted(first), "clusters are numbered by their lowest row"
            assert np.array_equal(linkage.cut(Z, int(c)), got[:, j]) and linkage.cut(Z, np.int64(c)).shape == (n,)
    # through the project's own record order: merge records to scipy's Z, then the cut
    Z = hierarchy.ward(np.random.default_rng(9).standard_normal((40, 3)))
    again = linkage._to_scipy(Z[:, :2].astype(np.int64), Z[:, 2], Z[:, 3], 40)
    assert np.array_equal(again, Z) and _same_partition(linkage.cut(again, 6), hierarchy.cut_tree(Z, n_clusters=6)[:, 0])


# ---- 5. membership ---------------------------------------------------------------------------------------------------------------------
def test_membership_on_hand_made_annotations():
    from variantformer_amd import enrichment
    universe = ["g0", "g1", "g2", "g3", "g4"]
    ann = {"g0": ["t_a", "t_b", "t_a"],            # a duplicate
           "g1": ["t_a"], "g2": ["t_a", "t_c"], "g3": "t_b",      # a single string is one term
           "g4": None, "outside": ["t_a", "t_b", "t_d"]}          # no term; a gene outside the universe
    m = enrichment.membership(ann, universe)
    assert m.terms == ["t_a", "t_b", "t_c"] and m.genes == 5, "t_d has no gene in the universe"
    assert m.termptr.dtype == np.int64 and m.termptr.tolist() == [0, 3, 5, 6] and m.gene.dtype == np.int32 and m.gene.tolist() == [0, 1, 2, 0, 3, 2]
    assert enrichment.membership(ann, universe, min_size=2).terms == ["t_a", "t_b"]
    assert enrichment.membership(ann, universe, min_size=2, max_size=2).terms == ["t_b"]
    assert enrichment.membership(ann, universe, max_size=1).terms == ["t_c"]
    empty = enrichment.membership(ann, universe, min_size=4)
    assert empty.terms == [] and empty.termptr.tolist() == [0] and empty.gene.shape == (0,)
    frame = pd.DataFrame({"gene_id": ["g2", "g0", "g0", "zz"], "go": [["t_c", "t_a"], ["t_b"], np.array(["t_a", "t_b"]), ["t_a"]]})
    f = enrichment.membership(frame, universe)
    assert f.terms == ["t_a", "t_b", "t_c"] and f.termptr.tolist() == [0, 2, 3, 4] and f.gene.tolist() == [0, 2, 0, 2], "a gene's rows are united"
    reordered = enrichment.membership(ann, universe[::-1])
    assert reordered.gene.tolist() == [2, 3, 4, 1, 4, 2], "rows of the universe as it was given, ascending within a term"


# ---- 6. the planted case, by scipy alone -----------------------------------------------------------------------------------------------
def test_scipy_alone_finds_the_planted_pairs():
    stats = pytest.importorskip("scipy.stats", reason="scipy is not installed")
    from variantformer_amd import enrichment
    labels, ann, universe = E.planted()
    m = enrichment.membership(ann, universe, min_size=5, max_size=500)
    assert len(m.terms) == E.PLANTED_TERMS and m.terms[:E.PLANTED_CLUSTERS] == [f"planted_{c}" for c in range(E.PLANTED_CLUSTERS)]
    count, size = E.counts(m.termptr, m.gene, labels, E.PLANTED_CLUSTERS)
    csize = np.bincount(labels, minlength=E.PLANTED_CLUSTERS)
    p = stats.hypergeom.sf(count - 1, E.PLANTED_GENES, size[:, None], csize[None, :])
    q = stats.false_discovery_control(p.ravel(), method="bh").reshape(p.shape)
    smallest = np.argsort(q.ravel(), kind="stable")[:E.PLANTED_CLUSTERS]
    assert sorted(smallest.tolist()) == [c * E.PLANTED_CLUSTERS + c for c in range(E.PLANTED_CLUSTERS)], "the six planted (term, cluster) cells"
    rest = np.delete(q.ravel(), smallest)
    print(f"[enrich planted] scipy: planted q at most {q.ravel()[smallest].max():.3e}, every other q at least {rest.min():.3e}")
    assert q.ravel()[smallest].max() < 0.05 and rest.min() > q.ravel()[smallest].max()

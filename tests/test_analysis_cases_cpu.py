"""The pipeline net itself, without a GPU (tests/analysis_pipeline_cases.py): every allocating function of the analysis modules is
reached by a case, the poisoning proxy can be installed in those modules and is taken out again, and the stream table of
tests/test_analysis_streams_gpu.py names what the headers declare."""
import importlib
import inspect
import re

import numpy as np
import torch

from tests import analysis_pipeline_cases as A
from tests import write_set_cases as W

COUNTS = {"manifold": 31, "linkage": 10, "enrichment": 8, "neighbors": 5, "ad_risk": 2}      # torch.empty / empty_like per module


def test_every_allocating_function_of_the_analysis_modules_has_a_case():
    found = A.allocating_functions()
    per_module = {}
    for qual, n in found.items():
        per_module[qual.split(".")[0]] = per_module.get(qual.split(".")[0], 0) + n
    # every allocation of a module sits in a listed function: the per-function counts add up to the module's own
    for mod in A.analysis_modules():
        in_source = len(re.findall(r"\btorch\.empty(?:_like)?\(", inspect.getsource(mod)))
        assert per_module.get(A._short(mod), 0) == in_source, (mod.__name__, per_module, in_source)
        # a new allocation belongs into the read-before-write table of the case module's docstring; then this number follows
        assert in_source == COUNTS[A._short(mod)], f"{mod.__name__} now allocates {in_source} times, the table lists {COUNTS[A._short(mod)]}"
    assert sum(per_module.values()) == 56
    assert A.uncovered_functions() == []
    assert {f for c in A.CASES for f in c.covers} <= set(found), sorted({f for c in A.CASES for f in c.covers} - set(found))
    names = [c.name for c in A.CASES]
    assert len(set(names)) == len(names)
    for c in A.CASES:
        assert c.covers and c.finite, c.name


def test_a_removed_case_is_named_by_the_coverage():
    fewer = [c for c in A.CASES if c.name != "tsne-B"]
    assert len(fewer) == len(A.CASES) - 1 and A.uncovered_functions(fewer) == ["manifold._knn_panels"]
    fewer = [c for c in A.CASES if c.name != "ad_risk-golden-rf"]
    assert A.uncovered_functions(fewer) == ["ad_risk.ADrisk.__call__", "ad_risk.ADriskFromVCF._predict_ad_risk"]
    fewer = [c for c in A.CASES if "enrichment._bh" not in c.covers]
    assert A.uncovered_functions(fewer) == ["enrichment._bh"]


def test_cases_build_their_inputs_without_a_gpu():
    for c in A.CASES:
        inputs = c.build()
        assert isinstance(inputs, dict) and inputs, c.name
        assert c.late is None or c.late in inputs, c.name


def test_the_proxy_is_installed_in_the_analysis_modules_and_restored(monkeypatch):
    mods = [importlib.import_module(n) for n in W.ANALYSIS_MODULES]
    wrappers = [importlib.import_module(n) for n in W.WRAPPER_MODULES]
    assert len(mods) == 5 and not set(W.ANALYSIS_MODULES) & set(W.WRAPPER_MODULES)
    with W.poison_allocations(0x3C, modules=W.ANALYSIS_MODULES) as px:
        for m in mods:
            assert m.torch is px
            t = m.torch.empty((3, 5), dtype=torch.int32)
            assert (t == 0x3C3C3C3C).all()
            assert (m.torch.empty_like(torch.zeros(4)).view(torch.uint8) == 0x3C).all()
            # what the pipelines ask of the name beside allocations: linkage.ward's isinstance among them
            assert isinstance(t, m.torch.Tensor) and not isinstance(t.numpy(), m.torch.Tensor)
            assert m.torch.zeros(2).tolist() == [0.0, 0.0] and m.torch.float32 is torch.float32
            assert m.torch.cuda.is_available() == torch.cuda.is_available()
        assert all(m.torch is torch for m in wrappers)                       # only the modules named
        assert px.count == len(px.allocated) == 2 * len(mods)
    assert all(m.torch is torch for m in mods)
    with W.poison_allocations(0xFF, keep=False, modules=W.WRAPPER_MODULES + W.ANALYSIS_MODULES) as px:
        assert all(m.torch is px for m in mods + wrappers)
        assert (mods[0].torch.empty(3, dtype=torch.int64) == -1).all() and px.count == 1 and px.allocated == []
    assert all(m.torch is torch for m in mods + wrappers)
    px = W.install(monkeypatch, 0xFF, modules=W.ANALYSIS_MODULES[:1])
    assert mods[0].torch is px and mods[1].torch is torch
    monkeypatch.undo()
    assert mods[0].torch is torch
    # the default is unchanged: the wrapper modules alone
    with W.poison_allocations(0x3C) as px:
        assert all(m.torch is px for m in wrappers) and all(m.torch is torch for m in mods)


# ---------------------------------------------------------------------------------------------
# the stream table of tests/test_analysis_streams_gpu.py
# ---------------------------------------------------------------------------------------------
def _side_headers() -> dict:
    import os
    from tests.conftest import REPO
    inc = os.path.join(REPO, "include")
    out = {}
    for name in sorted(os.listdir(inc)):
        if name.startswith("vf_hip_") and name.endswith(".h"):
            with open(os.path.join(inc, name)) as f:
                out[name] = f.read()
    return out


def test_the_stream_table_names_every_stream_taking_entry_of_the_side_headers():
    """The three stream tables together: the analysis table, and those the k-means and silhouette nets keep beside their cases."""
    from tests import test_analysis_streams_gpu as S
    from tests import test_kmeans_nets_gpu as KN
    from tests import test_silhouette_nets_gpu as SN
    headers = _side_headers()
    assert len(headers) == 15
    declared = sorted(e for text in headers.values() for e in W.stream_entries(text))
    assert len(declared) == len(set(declared)) == 36
    named = [c.entry for table in (S.ENTRY_CASES, KN.ENTRY_CASES, SN.ENTRY_CASES) for c in table]
    assert (len(S.ENTRY_CASES), len(KN.ENTRY_CASES), len(SN.ENTRY_CASES)) == (29, 4, 3)
    assert len(set(named)) == len(named)
    assert sorted(set(declared) - set(named)) == [], "stream-taking entries without a case"
    assert sorted(set(named) - set(declared)) == [], "cases for entries no header declares"
    # a new declaration is noticed
    grown = dict(headers, **{"vf_hip_new.h": "int vf_new_entry(const float* x, float* out, int64_t n, void* stream);"})
    assert sorted({e for t in grown.values() for e in W.stream_entries(t)} - set(named)) == ["vf_new_entry"]


def test_stream_cases_build_valid_operand_pairs_without_a_gpu():
    from tests import test_analysis_streams_gpu as S
    multi = {"vf_tsne_descent": S.DESCENT_ITERATIONS, "vf_umap_layout": S.LAYOUT_EPOCHS, "vf_umap_layout_transform": S.TRANSFORM_EPOCHS,
             "vf_graph_components_rounds": S.COMPONENT_ROUNDS, "vf_spmm_recur": S.RECUR_STEPS}
    assert all(n >= 2 for n in multi.values()) and set(multi) <= {c.entry for c in S.ENTRY_CASES}
    for c in S.ENTRY_CASES:
        built = c.make()
        assert set(built.stale) == set(built.fresh) and built.canary in built.stale, c.entry
        differs = False
        for k in built.stale:
            a, b = (np.asarray(v) if not isinstance(v, torch.Tensor) else v.view(torch.uint8).numpy() for v in (built.stale[k], built.fresh[k]))
            assert a.shape == b.shape and a.dtype == b.dtype, (c.entry, k)
            differs |= k == built.canary and a.tobytes() != b.tobytes()
        assert differs, f"{c.entry}: the canary's operand is the same in both sets"

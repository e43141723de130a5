"""The forest evaluator on the GPU (vf_forest_predict, include/vf_hip_forest.h): every geometry of tests/forest_cases.py against
the float64 restatement within the a-priori bound, in both forms; the scikit-learn fixture; the contract on bits; write and read
sets with poisoned memory; the header's rules for non-finite operands and model indices outside the bank."""
import numpy as np
import pytest
import torch

from tests import forest_cases as FC
from tests import write_set_cases as W
from variantformer_amd import forest as Fo

pytestmark = pytest.mark.gpu


def _ops():
    from variantformer_amd import _lib, ops
    _lib.load()
    return ops


def _strided(x: np.ndarray, ld: int) -> torch.Tensor:
    """x on the device as the leading columns of a [rows, ld] buffer whose other columns hold 1e30."""
    big = torch.full((x.shape[0], ld), 1e30, dtype=torch.float32, device="cuda")
    big[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    return big[:, :x.shape[1]]


def _run(bank, x: np.ndarray, model_of_row=None, model=None, ldx=None, ldo=None) -> np.ndarray:
    """float32 [R, K] from the device: x with row stride ldx, out with row stride ldo (default: both padded)."""
    K, F = bank.n_outputs, bank.n_features
    xd = _strided(x, F + FC.EXTRA_LDX if ldx is None else ldx)
    out = torch.full((x.shape[0], K + FC.EXTRA_LDO if ldo is None else ldo), -7.0, dtype=torch.float32, device="cuda")
    mor = None if model_of_row is None else torch.from_numpy(np.asarray(model_of_row, dtype=np.int32)).cuda()
    _ops().forest_predict(xd, bank.to("cuda"), model_of_row=mor, model=model, out=out[:, :K])
    torch.cuda.synchronize()
    assert bool((out[:, K:] == -7.0).all()), "columns past K were written"
    return out[:, :K].cpu().numpy()


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("name", FC.GEOMETRY_IDS)
def test_both_forms_against_float64(name):
    c, ref = FC.case(name), FC.reference(name)
    worst = 0.0
    want, bound = FC.row_form(ref, c.model_of_row)
    got = _run(c.bank, c.x, model_of_row=c.model_of_row)
    frac = np.abs(got - want) / bound
    worst = max(worst, float(frac.max()))
    print(f"[forest {name}] row form: largest error {float(frac.max()):.4f} of the bound")
    assert bool((frac <= 1.0).all())
    for m in range(len(c.models)):
        got = _run(c.bank, c.x, model=m)
        frac = np.abs(got - ref["all"][m]) / ref["all_bound"][m]
        worst = max(worst, float(frac.max()))
        assert bool((frac <= 1.0).all()), m
    print(f"[forest {name}] both forms: largest error {worst:.4f} of the bound")


@pytest.mark.parametrize("name", FC.FIXTURE_MODELS)
def test_fixture_against_sklearn(name):
    f = FC.load_ad_risk()[name]
    m = f["model"]
    _, bound = FC.predict64(m, f["x"])
    bank = Fo.ForestBank([m])
    for form, got in (("cohort", _run(bank, f["x"], model=0)),
                      ("row", _run(bank, f["x"], model_of_row=np.zeros(len(f["x"]), dtype=np.int32)))):
        frac = np.abs(got - f["proba"]) / bound
        print(f"[forest fixture {name}] {form} form: largest error {float(frac.max()):.4f} of the bound")
        assert bool((frac <= 1.0).all())
    # and what each wrong variant would give is told from the device's answer too
    for kind, wrong in FC.wrong_variants(f).items():
        if wrong is not None:
            rows, need = FC.variant_need(kind, f)
            off = (np.abs(wrong - got) > 50.0 * bound).any(axis=1)
            assert int(off.sum() if rows is None else (off & rows).sum()) >= need, kind


@pytest.mark.parametrize("name", ["bank4", "sigmoid", "softmax", "t130"])
def test_bits_depend_on_the_row_and_its_model_alone(name):
    """The same row at another R, position, ldx, ldo, form and bank composition gives equal bits."""
    c = FC.case(name)
    F, K, R = c.F, c.K, c.R
    base = _run(c.bank, c.x, model_of_row=c.model_of_row)
    # another stride of x and out (none padded), the rows reversed
    rev = _run(c.bank, c.x[::-1].copy(), model_of_row=c.model_of_row[::-1].copy(), ldx=F, ldo=K)
    assert np.array_equal(_bits(rev[::-1]), _bits(base))
    # every row alone (R = 1), in the cohort form, through a bank that holds its model alone
    for r in range(0, R, max(1, R // 5)):
        m = int(c.model_of_row[r])
        alone = _run(Fo.ForestBank([c.models[m]]), c.x[r:r + 1], model=0, ldx=F + 1)
        assert np.array_equal(_bits(alone[0]), _bits(base[r])), r
    # the cohort form over the whole bank, and a bank with the models in another order and one more in front
    for m in range(len(c.models)):
        rows = np.flatnonzero(c.model_of_row == m)
        if len(rows):
            cohort = _run(c.bank, c.x, model=m)
            assert np.array_equal(_bits(cohort[rows]), _bits(base[rows])), m
    order = list(range(len(c.models)))[::-1]
    other = Fo.ForestBank([c.models[0]] + [c.models[i] for i in order])
    remap = np.array([1 + order.index(int(m)) for m in c.model_of_row], dtype=np.int32)
    assert np.array_equal(_bits(_run(other, c.x, model_of_row=remap)), _bits(base))


_WS = FC.ws_cases()


@pytest.mark.parametrize("case", _WS, ids=[c.name for c in _WS])
def test_write_set(case):
    built = case.make()
    W.check_write_set(built.run, built.written, built.reference, built.nan_ok)


def test_rows_past_R_are_untouched_and_empty_calls_are_ok():
    ops = _ops()
    c = FC.case("t5")
    bank = c.bank.to("cuda")
    x = torch.from_numpy(c.x).cuda()
    out = torch.full((c.R + 3, c.K), -7.0, dtype=torch.float32, device="cuda")
    ops.forest_predict(x, bank, model=0, out=out[:c.R])
    ops.forest_predict(x[:0], bank, model=0, out=out[:0])
    ops.forest_predict(x[:0], bank, model_of_row=torch.zeros(0, dtype=torch.int32, device="cuda"), out=out[:0])
    torch.cuda.synchronize()
    assert bool((out[c.R:] == -7.0).all()) and bool((out[:c.R] != -7.0).all())
    with pytest.raises(ValueError, match="not both"):
        ops.forest_predict(x, bank, model=0, model_of_row=torch.zeros(c.R, dtype=torch.int32, device="cuda"), out=out[:c.R])
    with pytest.raises(ValueError, match="required"):
        ops.forest_predict(x, bank, out=out[:c.R])
    with pytest.raises(IndexError):
        ops.forest_predict(x, bank, model=1, out=out[:c.R])
    assert c.bank.to("cuda") is bank                                   # uploaded once


def _stump(feature, threshold, default_left, left_value, right_value, F=4, post="identity") -> Fo.PackedForest:
    return Fo.PackedForest([feature, -1, -1], [threshold, 0, 0], [1, 0, 1], [2, 0, 0], [default_left, 0, 0], [0],
                           [[left_value], [right_value]], [0.0], F, False, post)


def test_nonfinite_rules_of_the_header():
    nan, inf = float("nan"), float("inf")
    left_stump, right_stump = _stump(1, 0.5, 1, 10.0, 20.0), _stump(1, 0.5, 0, 10.0, 20.0)
    bank = Fo.ForestBank([left_stump, right_stump, _stump(1, inf, 0, 10.0, 20.0), _stump(1, -inf, 0, 10.0, 20.0)])
    x = np.zeros((6, 4), dtype=np.float32)
    x[:, 1] = [nan, inf, -inf, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), 0.0]
    x[:, 0] = x[:, 2] = x[:, 3] = nan                                  # features no node tests are never looked at
    got = {m: _run(bank, x, model=m)[:, 0].tolist() for m in range(4)}
    assert got[0] == [10.0, 20.0, 10.0, 10.0, 20.0, 10.0]              # a NaN feature goes left with default_left ...
    assert got[1] == [20.0, 20.0, 10.0, 10.0, 20.0, 10.0]              # ... and right without; +Inf right, -Inf left
    assert got[2] == [20.0, 10.0, 10.0, 10.0, 10.0, 10.0]              # +Inf <= +Inf: left
    assert got[3] == [20.0, 20.0, 10.0, 20.0, 20.0, 20.0]              # only -Inf <= -Inf
    # a NaN leaf reaches the rows whose walk ends in it and no other; an Inf leaf follows IEEE through the postprocessor
    c = FC.case("bank4")
    m1 = c.models[1]
    ends = m1.leaves_of(c.x)
    hit_leaf = int(m1.left[ends[0, 3]])                                # the leaf of row 0 in tree 3 of model 1
    lv = m1.leaf_values.copy()
    lv[hit_leaf, 0] = nan
    poisoned = Fo.PackedForest(m1.feature, m1.threshold, m1.left, m1.right, m1.default_left, m1.tree_root, lv, m1.base_scores,
                               m1.n_features, m1.average, m1.postprocessor)
    bank2 = Fo.ForestBank([c.models[0], poisoned] + c.models[2:])
    base = _run(c.bank, c.x, model_of_row=c.model_of_row)
    got = _run(bank2, c.x, model_of_row=c.model_of_row)
    reaches = (m1.left[ends] == hit_leaf).any(axis=1) & (c.model_of_row == 1)
    assert np.isnan(got[reaches, 0]).all() and np.array_equal(_bits(got[reaches, 1]), _bits(base[reaches, 1]))
    assert np.array_equal(_bits(got[~reaches]), _bits(base[~reaches]))
    cohort = _run(bank2, c.x, model=1)
    all_reach = (m1.left[ends] == hit_leaf).any(axis=1)
    assert all_reach[0] and np.array_equal(np.isnan(cohort[:, 0]), all_reach) and not np.isnan(cohort[:, 1]).any()
    s = Fo.ForestBank([_stump(0, 0.0, 0, inf, -inf, post="sigmoid")])
    assert _run(s, np.array([[-1.0, 0, 0, 0], [1.0, 0, 0, 0]], dtype=np.float32), model=0)[:, 0].tolist() == [1.0, 0.0]


@pytest.mark.parametrize("name", ["bank4", "softmax"])
def test_a_model_index_outside_the_bank_gives_a_nan_row_and_reads_nothing(name):
    c = FC.case(name)
    M = len(c.models)
    base = _run(c.bank, c.x, model_of_row=c.model_of_row)
    mor = c.model_of_row.copy()
    bad = {0: -1, c.R // 2: M, c.R - 1: 2 ** 31 - 1}
    for r, v in bad.items():
        mor[r] = v
    got = _run(c.bank, c.x, model_of_row=mor)
    ok = np.ones(c.R, dtype=bool)
    ok[list(bad)] = False
    assert np.isnan(got[~ok]).all() and np.array_equal(_bits(got[ok]), _bits(base[ok]))
    # the entry itself in the cohort form (the wrapper raises IndexError before it): every row NaN, nothing else written
    from variantformer_amd import _lib
    b = c.bank.to("cuda")
    x = torch.from_numpy(c.x).cuda()
    out = torch.full((c.R + 2, c.K + 2), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().vf_forest_predict(x.data_ptr(), x.stride(0), c.R, c.F, *(getattr(b, k).data_ptr() for k in Fo.ForestBank.ARRAYS),
                                             M, c.K, int(b.average), FC.POST[b.postprocessor], 0, M, out.data_ptr(), out.stride(0),
                                             torch.cuda.current_stream().cuda_stream), "vf_forest_predict")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:c.R, :c.K]).all()) and bool((out[c.R:] == -7.0).all()) and bool((out[:, c.K:] == -7.0).all())

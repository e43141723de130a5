"""The cache of weight-derived operands (variantformer_amd.weights) and the per-thread operand type (ops.compute_dtype), on CPU
tensors with a trivial build.  No kernel is launched."""
import threading

import torch

from variantformer_amd import ops, weights


def _derive(lin, form="plain", *spec):
    return weights.derived(lin, "_vf_packed", (lin.weight, lin.bias), lambda: (form, lin.weight.detach() * 2), form, *spec)


def test_hit_rebuild_on_version_and_operand_type():
    lin = torch.nn.Linear(4, 3)
    first = _derive(lin)
    n = weights.BUILDS
    assert _derive(lin) is first and weights.BUILDS == n                  # same sources: a hit
    with torch.no_grad():
        lin.weight.mul_(3.0)                                              # in place: new _version, same address
    again = _derive(lin)
    assert weights.BUILDS == n + 1 and torch.equal(again[1], lin.weight.detach() * 2)
    assert _derive(lin) is again and weights.BUILDS == n + 1
    with ops.compute_dtype(torch.float16):
        half = _derive(lin)
    assert weights.BUILDS == n + 2 and half is not again
    assert _derive(lin) is not half and weights.BUILDS == n + 3           # one entry per slot: back to bf16 rebuilds


def test_forms_sharing_a_slot_evict_each_other():
    lin = torch.nn.Linear(4, 3)
    plain = _derive(lin, "plain")
    n = weights.BUILDS
    assert _derive(lin, "ln")[0] == "ln" and weights.BUILDS == n + 1
    assert _derive(lin, "plain") is not plain and weights.BUILDS == n + 2
    _derive(lin, "plain", 0.5)                                            # a spec value is part of the key too
    assert weights.BUILDS == n + 3
    assert list(k for k in lin.__dict__ if k.startswith("_vf_")) == ["_vf_packed"]


def test_none_source_and_built_from():
    lin = torch.nn.Linear(4, 3, bias=False)
    assert lin.bias is None
    v = _derive(lin)
    n = weights.BUILDS
    assert _derive(lin) is v and weights.BUILDS == n
    assert weights.built_from(lin, "_vf_packed", (lin.weight, None), "plain")
    with ops.compute_dtype(torch.float16):                               # whichever operand type the entry was built in
        assert weights.built_from(lin, "_vf_packed", (lin.weight,), "plain")
    assert not weights.built_from(lin, "_vf_packed", (lin.weight,), "ln")
    assert not weights.built_from(lin, "_vf_absent", (lin.weight,), "plain")
    with torch.no_grad():
        lin.weight.add_(1.0)
    assert not weights.built_from(lin, "_vf_packed", (lin.weight,), "plain")


def test_compute_dtype_is_per_thread():
    seen = {}
    with ops.compute_dtype(torch.float16):
        t = threading.Thread(target=lambda: seen.update(started=ops.cdt()))
        t.start()
        t.join()
        assert ops.cdt() == torch.float16
    assert seen["started"] == torch.bfloat16 and ops.cdt() == torch.bfloat16

    inside, release = threading.Event(), threading.Event()

    def worker():
        with ops.compute_dtype(torch.float16):
            seen["worker"] = ops.cdt()
            inside.set()
            release.wait(30)
        seen["after"] = ops.cdt()
    t = threading.Thread(target=worker)
    t.start()
    try:
        assert inside.wait(30)
        assert ops.cdt() == torch.bfloat16, "a block entered in another thread changed this thread's operand type"
    finally:
        release.set()
        t.join()
    assert seen["worker"] == torch.float16 and seen["after"] == torch.bfloat16

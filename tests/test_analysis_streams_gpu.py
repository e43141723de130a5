"""The analysis entries and pipelines off the default stream and from two threads, on a real MI355X.  Nothing here is poisoned:
every operand buffer holds what a previous VALID call or copy left, so that even a launch on the wrong stream reads only
well-formed operands.

Every entry honours its stream (ENTRY_CASES: the 29 stream-taking entries of the headers beside include/vf_hip.h, each built
from the smallest builder of its own *_cases.py).  Two valid operand sets, STALE and FRESH, whose results on the default stream
differ (asserted).  The entry runs on the stale operands into its outputs and workspaces.  Then a side stream that has waited for
the current one gets a delay, the copy of the fresh operands into the same operand buffers, and the entry into the same outputs.
Right behind it a clone of one operand buffer is enqueued on the default stream: the canary.  After side.synchronize() the outputs
must equal the fresh result bit for bit, and the canary must still hold what the buffer held before: that proves the delay held,
so a launch that did not wait on the stream it was given would have computed from the stale operands.  A canary that already
holds the fresh operand fails the test's premise ("delay too short to prove anything"); it is no skip and no retry.  The entries
that launch more than once per call -- vf_tsne_descent, vf_umap_layout, vf_umap_layout_transform, vf_graph_components_rounds,
vf_spmm_recur -- run at least two iterations, epochs or rounds, all enqueued behind the delay: a later launch on another stream
would start from a stale state.  No case reads anything back between the delay and the canary.

Pipelines behind a late input (the cases of tests/analysis_pipeline_cases.py, whose `late` input may be a device tensor): the
same, with the pipeline under torch.cuda.stream(side) and its input buffer written behind the delay; the result must equal the
plain run bit for bit.  Here the canary is cloned BEFORE the pipeline is called, not after it: every pipeline reads scalars or
results back, which waits the delay out on the host, so the canary proves that the fresh input -- and every launch up to the
pipeline's first read-back -- was still held back when it was enqueued.

The side stream is probed (fixture `side`): the runtime serves its streams from a few in-order hardware queues, and a stream that
shares its queue with the default stream holds the default stream's work back too -- the first run of this module saw two of
thirteen canaries wait for the delay that way.  The fixture takes a stream behind whose delay the default stream demonstrably
goes on.

The delay is torch.cuda._sleep, calibrated once per module with events to about 100 ms.  Measured on an MI355X: 238 536 524
cycles, 99.6 ms (DELAY_MEASURED_MS); the host time between enqueueing the entry (or the copy) and the canary was 0.02 .. 0.07 ms
(HOST_MEASURED_MS, the largest).  The delay must be at least 20 times that host time, asserted per test with that run's own
times: the room for a shared machine's jitter is more than a thousandfold.

Two threads, two streams: the shape of tests/test_concurrency_gpu.py::test_two_models_in_two_threads_on_their_own_streams -- a
barrier, errors re-raised in the main thread, three repetitions per thread, everything in one process -- over pairs of pipelines
and over a pipeline beside a model forward; every result equals the one obtained alone, bit for bit."""
import threading
import time
from typing import Callable, NamedTuple

import numpy as np
import pytest
import torch

from tests import analysis_pipeline_cases as A

pytestmark = pytest.mark.gpu

DELAY_TARGET_MS = 100.0
DELAY_MEASURED_MS = 99.6         # torch.cuda._sleep of the calibrated cycle count, by events
HOST_MEASURED_MS = 0.07          # enqueueing the copy and the canary's clone, by time.perf_counter
DELAY_OVER_HOST = 20.0


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from variantformer_amd import _lib as lib
    lib.load()      # must be the in-tree HIP library; raises if missing


def _timed_sleep(cycles: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(cycles)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


@pytest.fixture(scope="module")
def delay():
    """(cycles, measured ms): a torch.cuda._sleep of about DELAY_TARGET_MS, measured once."""
    _timed_sleep(1000)                                                   # the kernel's first launch
    probe = 2_000_000
    ms = max(_timed_sleep(probe), 1e-3)
    cycles = int(probe * DELAY_TARGET_MS / ms)
    assert 0 < cycles < 1 << 40, (cycles, ms)
    measured = _timed_sleep(cycles)
    print(f"[streams] delay: {cycles} cycles measured {measured:.1f} ms (probe {probe} cycles: {ms:.3f} ms)")
    assert 0.5 * DELAY_TARGET_MS <= measured <= 4 * DELAY_TARGET_MS, measured
    return cycles, measured


@pytest.fixture(scope="module")
def side(delay):
    """A side stream that demonstrably runs BESIDE the default stream.  The runtime serves its streams from a few hardware queues
    (four by default), each in order: a stream that shares its queue with the default stream holds back everything enqueued on the
    default stream behind it, the canary included, and then no canary can tell a held-back launch from one that was not.  So
    the candidates are probed once: a short delay on the candidate, an event on the default stream behind it; the candidate
    serves if that event completes while the candidate's delay is still running.  One stream serves the whole module."""
    cycles, _ = delay
    for _ in range(16):
        candidate = torch.cuda.Stream()
        torch.cuda.synchronize()
        held, passed = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(candidate):
            torch.cuda._sleep(cycles // 4)
            held.record()
        passed.record()                                                 # the default stream
        passed.synchronize()
        beside = not held.query()
        torch.cuda.synchronize()
        if beside:
            return candidate
    pytest.fail("no stream of 16 runs beside the default stream: every canary would wait for the delay")


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _assert_equal_results(got: dict, want: dict, what: str):
    assert set(got) == set(want), what
    for key in want:
        assert _same_bits(got[key], want[key]), f"{what}: {key} differs from the run made alone on the default stream"


def _stale_of(case, fresh: np.ndarray) -> np.ndarray:
    """Another valid operand of the same shape and type as the case's late input."""
    if case.late == "D":                                                  # a distance matrix stays one: rows and columns permuted alike
        n = fresh.shape[0]
        stale = fresh.copy()
        stale[:, :n] = fresh[::-1, :n][:, ::-1]
        return stale
    if case.late == "w":                                                  # edge weights stay positive and symmetric
        return fresh * np.float32(0.5)
    return np.ascontiguousarray(fresh[::-1])                              # rows, or labels, in reverse order


LATE_CASES = [c for c in A.CASES if c.late is not None]


def test_every_pipeline_case_takes_a_device_input():
    assert len(LATE_CASES) == len(A.CASES) >= 12


@pytest.mark.parametrize("case", LATE_CASES, ids=lambda c: c.name)
def test_pipeline_behind_a_late_input_on_a_side_stream(case, delay, side):
    cycles, delay_ms = delay
    inputs = case.build()
    plain = case.run(inputs)
    fresh = np.ascontiguousarray(inputs[case.late])
    stale = _stale_of(case, fresh)
    assert stale.shape == fresh.shape and stale.dtype == fresh.dtype and not _same_bits(stale, fresh)
    buf, fresh_dev = torch.from_numpy(stale).cuda(), torch.from_numpy(fresh).cuda()
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.cuda._sleep(cycles)
        t0 = time.perf_counter()
        buf.copy_(fresh_dev)
    canary = buf.clone()                                                  # the default stream: not behind the delay
    host_ms = (time.perf_counter() - t0) * 1e3
    with torch.cuda.stream(side):
        got = case.run({**inputs, case.late: buf})
    side.synchronize()
    torch.cuda.synchronize()
    print(f"[streams] {case.name}: delay {delay_ms:.1f} ms, copy and canary enqueued in {host_ms:.3f} ms")
    assert _same_bits(canary.cpu().numpy(), stale), "delay too short to prove anything: the canary already saw the fresh input"
    assert delay_ms >= DELAY_OVER_HOST * host_ms, (delay_ms, host_ms)
    assert _same_bits(buf.cpu().numpy(), fresh)                           # an input is never written
    _assert_equal_results(got, plain, case.name)


# ---- every entry honours its stream ----------------------------------------------------------------------------------------------
class Built(NamedTuple):
    const: dict                   # operands that stay as they are: name -> numpy array / torch tensor (or any object, passed on)
    stale: dict                   # the operand buffers' first content: name -> array
    fresh: dict                   # what is copied into them behind the delay (equal to `stale` for a state that is only reset)
    outs: Callable                # () -> the outputs and workspaces, zeroed tensors on the device
    call: Callable                # (operands on the device, outs) -> {name: result tensor}; no host read-back inside
    canary: str                   # the operand whose clone on the default stream is the canary: a key of stale and fresh


class EntryCase(NamedTuple):
    entry: str                    # the C-ABI entry the case launches
    make: Callable                # () -> Built; CPU work only


ENTRY_CASES: list = []


def _entry(name):
    def deco(make):
        ENTRY_CASES.append(EntryCase(name, make))
        return make
    return deco


def _ops():
    from variantformer_amd import ops
    return ops


def _flip(a):
    return np.ascontiguousarray(np.asarray(a)[::-1])


def _zeros(shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device="cuda")


@_entry("vf_attn_contrib")
def _attn_contrib():
    from tests import attn_contrib_cases as AC
    c = AC.case(4, 32, "bf16")
    const = dict(s_gram=c.s_gram, probs=c.P.reshape(c.R * c.H, c.max_k).contiguous(), cu_rows=c.cu_rows, cu_k=c.cu_k)

    def call(b, o):
        _ops().attn_contrib(b["kv"][:, c.D:], b["s_gram"], b["probs"], b["cu_rows"], b["cu_k"], c.max_rows, c.max_k, c.H, c.dh,
                            gram=o["gram"], out=o["out"])
        return o
    return Built(const, {"kv": torch.flip(c.kv16, (0,))}, {"kv": c.kv16},
                 lambda: {"gram": _zeros((c.tk, c.H, c.H)), "out": _zeros((c.R, c.max_k))}, call, "kv")


@_entry("vf_attn_contrib_self")
def _attn_contrib_self():
    from tests import gene_contrib_cases as GC
    c = GC.case(4, 32, 96, "bf16")
    const = dict(wo=c.wo16, probs=c.P.reshape(c.n_seq * c.H, c.max_k).contiguous(), cu_k=c.cu_k)

    def call(b, o):
        _ops().attn_contrib_self(b["v"], b["wo"], b["probs"], b["cu_k"], c.max_k, c.H, c.dh, out=o["out"])
        return o
    return Built(const, {"v": torch.flip(c.v16, (0,))}, {"v": c.v16}, lambda: {"out": _zeros((c.n_seq, c.max_k))}, call, "v")


@_entry("vf_tissue_heads")
def _tissue_heads():
    from tests import cre_heads_cases as H
    c = H.case(200, 11, 3, "mean", 5, (1, 3, 1))
    const = dict(w=c.w, bias=c.bias, tissues=torch.tensor(c.sel, dtype=torch.int32))

    def call(b, o):          # checked=True: the ids are the case's own, and the check would read them back
        _ops().tissue_heads(b["x"], c.ns, c.agg, b["w"], b["bias"], tissues=b["tissues"], out=o["out"], argmax=o["argmax"], checked=True)
        return o
    return Built(const, {"x": torch.flip(c.x, (0,))}, {"x": c.x},
                 lambda: {"out": _zeros((c.B, len(c.sel) * c.C)), "argmax": _zeros((c.B, len(c.sel)), torch.int32)}, call, "x")


@_entry("vf_forest_predict")
def _forest_predict():
    from tests import forest_cases as FC
    from variantformer_amd import forest
    F, K, R = 16, 2, 67
    bank = forest.ForestBank([FC.make_forest(1, 65, F, K, depth=5)])
    x = FC.make_rows(1, R, F)

    def call(b, o):
        _ops().forest_predict(b["x"], bank.to(b["x"].device), model=0, out=o["out"])
        return o
    return Built({}, {"x": _flip(x)}, {"x": x}, lambda: {"out": _zeros((R, K))}, call, "x")


@_entry("vf_topk_rows")
def _topk_rows():
    from tests import topk_cases as T
    c = T.case(65, 31, "full", "distinct")

    def call(b, o):
        _ops().topk_rows(b["x"][:, :c.n], c.k, values=o["values"], indices=o["indices"])
        return o
    return Built({}, {"x": _flip(c.x)}, {"x": c.x},
                 lambda: {"values": _zeros((T.R, c.k)), "indices": _zeros((T.R, c.k), torch.int32)}, call, "x")


def _neighbour_rows():
    from tests import neighbors_cases as N
    c = N.random_case(200, 5)
    return np.ascontiguousarray(c.z[:, :c.d])


@_entry("vf_rows_standardize")
def _rows_standardize():
    from tests import neighbors_cases as N
    d = 5
    x = N.std_case(d)                                                       # [kinds, d + 5]: the row stride is above d

    def call(b, o):
        _ops().rows_standardize(b["x"][:, :d], center=True, z=o["z"], norm=o["norm"])
        return o
    return Built({}, {"x": _flip(x)}, {"x": x}, lambda: {"z": _zeros((x.shape[0], d)), "norm": _zeros((x.shape[0],))}, call, "x")


@_entry("vf_knn_dot")
def _knn_dot():
    z, k = _neighbour_rows(), 30

    def call(b, o):
        _ops().knn_dot(b["z"], b["z"], k, self_offset=0, values=o["values"], indices=o["indices"])
        return o
    return Built({}, {"z": _flip(z)}, {"z": z},
                 lambda: {"values": _zeros((z.shape[0], k)), "indices": _zeros((z.shape[0], k), torch.int32)}, call, "z")


@_entry("vf_pairwise_dot")
def _pairwise_dot():
    z = _neighbour_rows()

    def call(b, o):
        _ops().pairwise_dot(b["z"], b["z"], mode=1, self_offset=0, out=o["out"])
        return o
    return Built({}, {"z": _flip(z)}, {"z": z}, lambda: {"out": _zeros((z.shape[0], z.shape[0]))}, call, "z")


@_entry("vf_linkage_nearest")
def _linkage_nearest():
    from tests import linkage_cases as L
    D = L.nearest_case(65)

    def call(b, o):
        _ops().linkage_nearest(b["D"], nn_val=o["nn_val"], nn_idx=o["nn_idx"])
        return o
    return Built({}, {"D": np.ascontiguousarray(D.T)}, {"D": D},
                 lambda: {"nn_val": _zeros((65,)), "nn_idx": _zeros((65,), torch.int32)}, call, "D")


@_entry("vf_linkage_contract")
def _linkage_contract():
    from tests import linkage_cases as L
    D, size, first, second = L.contract_case("single")
    m_out = first.shape[0]

    def call(b, o):
        _ops().linkage_contract(b["D"], b["size"], b["first"], b["second"], out=o["out"], size_out=o["size_out"], pair_dist=o["pair_dist"])
        return o
    return Built(dict(size=size, first=first, second=second), {"D": D * np.float32(2.0)}, {"D": D},
                 lambda: {"out": _zeros((m_out, m_out)), "size_out": _zeros((m_out,), torch.int32), "pair_dist": _zeros((m_out,))}, call, "D")


@_entry("vf_umap_smooth_knn")
def _umap_smooth_knn():
    from tests import umap_cases as U
    idx, dist = U.smooth_case("random", 65, 29)
    mean_dist = U.mean_distance(idx, dist)

    def call(b, o):
        _ops().umap_smooth_knn(b["idx"], b["dist"], mean_dist, rho=o["rho"], sigma=o["sigma"], strength=o["strength"])
        return o
    return Built(dict(idx=idx), {"dist": dist * np.float32(1.5)}, {"dist": dist},
                 lambda: {"rho": _zeros((65,)), "sigma": _zeros((65,)), "strength": _zeros((65, 29))}, call, "dist")


@_entry("vf_umap_union")
def _umap_union():
    from tests import umap_cases as U
    idx, dist = U.smooth_case("random", 65, 29)
    strength = U.smooth_knn(idx, dist, U.mean_distance(idx, dist))[2].astype(np.float32)
    rowptr, col = U.csr(idx, dist)

    def call(b, o):
        _ops().umap_union(b["idx"], b["strength"], b["rowptr"], b["col"], w=o["w"])
        return o
    return Built(dict(idx=idx, rowptr=rowptr, col=col), {"strength": strength * np.float32(0.5)}, {"strength": strength},
                 lambda: {"w": _zeros((col.shape[0],))}, call, "strength")


LAYOUT_EPOCHS = 3                          # vf_umap_layout: one launch per epoch


@_entry("vf_umap_layout")
def _umap_layout():
    from tests import umap_cases as U
    c = U.layout_case(65, 2)

    def call(b, o):
        y = _ops().umap_layout(b["rowptr"], b["col"], b["samples"], b["y0"], o["y1"], epoch_begin=0, epoch_end=LAYOUT_EPOCHS, n_epochs=c.N,
                               a=c.a, b=c.b, negative_sample_rate=c.rate, seed=c.seed)
        return {"y": y}
    return Built(dict(rowptr=c.rowptr, col=c.col, samples=c.samples), {"y0": _flip(c.Y)}, {"y0": c.Y},
                 lambda: {"y1": _zeros(c.Y.shape)}, call, "y0")


def _spectral_graph():
    from tests import spectral_cases as S
    rowptr, col, w = S.kernel_graph(65)
    return rowptr, col, w, S.degree(rowptr, w)[1]


@_entry("vf_graph_degree")
def _graph_degree():
    rowptr, col, w, _ = _spectral_graph()

    def call(b, o):
        _ops().graph_degree(b["rowptr"], b["col"], b["w"], deg=o["deg"], dinv_sqrt=o["dinv_sqrt"])
        return o
    return Built(dict(rowptr=rowptr, col=col), {"w": _flip(w)}, {"w": w}, lambda: {"deg": _zeros((65,)), "dinv_sqrt": _zeros((65,))}, call, "w")


RECUR_STEPS = 4                            # vf_spmm_recur: one launch per step; from step 1 on the block before the newest is read


@_entry("vf_spmm_recur")
def _spmm_recur():
    from tests import spectral_cases as S
    from tests import umap_cases as U
    rowptr, col, w, dinv = _spectral_graph()
    x = U.random_init(65, 3, 11) - np.float32(0.5)
    coef = S.chebyshev(0.5, RECUR_STEPS)
    assert coef.shape == (RECUR_STEPS, 3) and coef[0, 2] == 0                # x2 is not read before step 1 has written it

    def call(b, o):
        return {"x": _ops().spmm_recur(b["rowptr"], b["col"], b["w"], b["dinv"], b["x0"], o["x1"], o["x2"], coef)}
    return Built(dict(rowptr=rowptr, col=col, w=w, dinv=dinv), {"x0": _flip(x)}, {"x0": x},
                 lambda: {"x1": _zeros(x.shape), "x2": _zeros(x.shape)}, call, "x0")


def _tall_block():
    from tests import umap_cases as U
    return U.random_init(257, 3, 12) - np.float32(0.5)


@_entry("vf_tall_gram")
def _tall_gram():
    x = _tall_block()

    def call(b, o):
        _ops().tall_gram(b["x"], b["x"], out=o["out"], work=o["work"])
        return {"out": o["out"]}
    return Built({}, {"x": x * np.float32(2.0)}, {"x": x},
                 lambda: {"out": _zeros((3, 3), torch.float64), "work": _zeros((_ops().TALL_GRAM_MAX_BLOCKS * 9,), torch.float64)}, call, "x")


@_entry("vf_tall_mul")
def _tall_mul():
    x = _tall_block()
    t = np.random.default_rng(13).standard_normal((3, 3))

    def call(b, o):
        _ops().tall_mul(b["x"], b["t"], out=o["out"])
        return o
    return Built(dict(t=t), {"x": _flip(x)}, {"x": x}, lambda: {"out": _zeros(x.shape)}, call, "x")


@_entry("vf_umap_smooth_knn_query")
def _umap_smooth_knn_query():
    from tests import umap_transform_cases as UT
    idx, dist = UT.smooth_case("random", 65, 15)

    def call(b, o):
        _ops().umap_smooth_knn_query(b["idx"], b["dist"], 0.5, sigma=o["sigma"], strength=o["strength"])
        return o
    return Built(dict(idx=idx), {"dist": dist * np.float32(1.5)}, {"dist": dist},
                 lambda: {"sigma": _zeros((65,)), "strength": _zeros((65, 15))}, call, "dist")


TRANSFORM_EPOCHS = 20                      # vf_umap_layout_transform runs 8 epochs per launch: three launches


def _transform_case():
    from tests import umap_transform_cases as UT
    assert TRANSFORM_EPOCHS > 2 * UT.EPOCHS_PER_LAUNCH
    return UT.layout_case(65, 100, 2, 15, TRANSFORM_EPOCHS)


@_entry("vf_umap_init_transform")
def _umap_init_transform():
    idx, cnt, Y, Yq = _transform_case()
    strength = (np.clip(cnt, 0, TRANSFORM_EPOCHS) / np.float32(TRANSFORM_EPOCHS)).astype(np.float32)

    def call(b, o):
        _ops().umap_init_transform(b["idx"], b["strength"], b["y"], out=o["out"])
        return o
    return Built(dict(idx=idx, strength=strength), {"y": _flip(Y)}, {"y": Y}, lambda: {"out": _zeros(Yq.shape)}, call, "y")


@_entry("vf_umap_layout_transform")
def _umap_layout_transform():
    from tests import umap_transform_cases as UT
    idx, cnt, Y, Yq = _transform_case()

    def call(b, o):
        _ops().umap_layout_transform(b["idx"], b["cnt"], b["y"], b["yq"], epoch_begin=0, epoch_end=TRANSFORM_EPOCHS, n_epochs=TRANSFORM_EPOCHS,
                                     a=UT.AB[0], b=UT.AB[1])
        return {"yq": b["yq"]}
    return Built(dict(idx=idx, cnt=cnt, y=Y), {"yq": _flip(Yq)}, {"yq": Yq}, lambda: {}, call, "yq")


COMPONENT_ROUNDS = 3                       # vf_graph_components_rounds: three launches per round


def _components_graph():
    from tests import components_cases as C
    return C.search_graphs(65)["random-path"]


@_entry("vf_graph_components_rounds")
def _graph_components_rounds():
    rowptr, col, w = _components_graph()
    identity = np.arange(65, dtype=np.int32)

    def call(b, o):          # stale: no entry has a positive weight, so no entry is an edge and the identity stays
        _ops().graph_components_rounds(b["rowptr"], b["col"], b["w"], b["parent"], o["g"], o["m"], o["changed"], rounds=COMPONENT_ROUNDS)
        return {"parent": b["parent"], "g": o["g"], "m": o["m"], "changed": o["changed"]}
    return Built(dict(rowptr=rowptr, col=col), {"w": np.zeros_like(w), "parent": identity}, {"w": w, "parent": identity},
                 lambda: {"g": _zeros((65,), torch.int32), "m": _zeros((65,), torch.int32), "changed": _zeros((1,), torch.int32)}, call, "w")


@_entry("vf_csr_components")
def _csr_components():
    from tests import components_cases as C
    rowptr, col, w = C.search_graphs(65)["isolated"]
    order, rank, comp, starts, rowptr_new = C.permutation(C.fixed_point(rowptr, col, w)[0], rowptr)

    def call(b, o):
        _ops().csr_components(b["rowptr"], b["col"], b["w"], b["order"], b["rank"], b["comp"], b["starts"], b["rowptr_new"],
                              col_new=o["col_new"], w_new=o["w_new"])
        return o
    return Built(dict(rowptr=rowptr, col=col, order=order, rank=rank, comp=comp, starts=starts, rowptr_new=rowptr_new),
                 {"w": w * np.float32(0.5)}, {"w": w},
                 lambda: {"col_new": _zeros(col.shape, torch.int32), "w_new": _zeros(w.shape)}, call, "w")


@_entry("vf_segment_mean_gather")
def _segment_mean_gather():
    from tests import components_cases as C
    order, starts = C.segments((1, 3, 4, 5, 255))
    x = np.random.default_rng(14).standard_normal((order.shape[0], 49)).astype(np.float32)

    def call(b, o):
        _ops().segment_mean_gather(b["x"], b["order"], b["starts"], out=o["out"])
        return o
    return Built(dict(order=order, starts=starts), {"x": _flip(x)}, {"x": x}, lambda: {"out": _zeros((starts.shape[0] - 1, 49))}, call, "x")


@_entry("vf_tsne_perplexity")
def _tsne_perplexity():
    from tests import tsne_cases as TS
    idx, d2 = TS.perplexity_case("random", 65, 63)

    def call(b, o):
        _ops().tsne_perplexity(b["idx"], b["d2"], TS.perplexity_of(63), beta=o["beta"], p_cond=o["p_cond"])
        return o
    return Built(dict(idx=idx), {"d2": d2 * np.float32(2.0)}, {"d2": d2}, lambda: {"beta": _zeros((65,)), "p_cond": _zeros((65, 63))}, call, "d2")


def _tsne_graph():
    from tests import tsne_cases as TS
    return TS.small_graph(65, 15)


@_entry("vf_tsne_joint")
def _tsne_joint():
    from tests import tsne_cases as TS
    idx, d2, rowptr, col, _ = _tsne_graph()
    p_cond = TS.perplexity_search(idx, d2, TS.perplexity_of(15), np.float32)[1]

    def call(b, o):
        _ops().tsne_joint(b["idx"], b["p_cond"], b["rowptr"], b["col"], p=o["p"])
        return o
    return Built(dict(idx=idx, rowptr=rowptr, col=col), {"p_cond": p_cond * np.float32(0.5)}, {"p_cond": p_cond},
                 lambda: {"p": _zeros((col.shape[0],))}, call, "p_cond")


@_entry("vf_tsne_repulsion")
def _tsne_repulsion():
    from tests import tsne_cases as TS
    y = TS.embedding(65, 2)

    def call(b, o):
        _ops().tsne_repulsion(b["y"], dof=1, splits=2, part=o["part"])
        return o
    return Built({}, {"y": _flip(y)}, {"y": y}, lambda: {"part": _zeros((2, 65, 3))}, call, "y")


DESCENT_ITERATIONS = 3                     # vf_tsne_descent: four launches per iteration


@_entry("vf_tsne_descent")
def _tsne_descent():
    from tests import tsne_cases as TS
    _, _, rowptr, col, p = _tsne_graph()
    y = TS.embedding(65, 2)
    zero, one = np.zeros_like(y), np.ones_like(y)

    def call(b, o):
        _ops().tsne_descent(b["rowptr"], b["col"], b["p"], b["y"], b["update"], b["gains"], iter_begin=0, iter_end=DESCENT_ITERATIONS,
                            exaggeration=1.0, momentum=0.5, learning_rate=TS.STEPS_LEARNING_RATE, dof=1, splits=2, work=o["work"],
                            zsum=o["zsum"])
        return {"y": b["y"], "update": b["update"], "gains": b["gains"], "zsum": o["zsum"]}
    return Built(dict(rowptr=rowptr, col=col, p=p), {"y": _flip(y), "update": zero, "gains": one}, {"y": y, "update": zero, "gains": one},
                 lambda: {"work": _zeros((_ops().tsne_work_bytes(65, 2, 2) // 8 + 1,), torch.float64),
                          "zsum": _zeros((DESCENT_ITERATIONS,), torch.float64)}, call, "y")


@_entry("vf_enrich_counts")
def _enrich_counts():
    from tests import enrich_cases as EC
    k = 7
    termptr, gene, labels = EC.counts_case(300, k)
    T = termptr.shape[0] - 1

    def call(b, o):
        _ops().enrich_counts(b["termptr"], b["gene"], b["labels"], k, count=o["count"], size=o["size"])
        return o
    return Built(dict(termptr=termptr, gene=gene), {"labels": _flip(labels)}, {"labels": labels},
                 lambda: {"count": _zeros((T, k), torch.int32), "size": _zeros((T,), torch.int32)}, call, "labels")


@_entry("vf_hypergeom_tail")
def _hypergeom_tail():
    from tests import enrich_cases as EC
    N = 6
    count, size, csize = EC.grid(N)

    def call(b, o):
        _ops().hypergeom_tail(b["count"], b["size"], b["csize"], N, b["logfact"], 0, log_p=o["log_p"], tail=o["tail"], steps=o["steps"])
        return o
    return Built(dict(size=size, csize=csize, logfact=EC.log_factorials(N)), {"count": _flip(count)}, {"count": count},
                 lambda: {"log_p": _zeros(count.shape, torch.float64), "tail": _zeros(count.shape, torch.float64),
                          "steps": _zeros(count.shape, torch.int32)}, call, "count")


def _to_device(v):
    if isinstance(v, np.ndarray):
        v = torch.from_numpy(np.ascontiguousarray(v))
    return v.contiguous().cuda() if isinstance(v, torch.Tensor) else v


def _host(results: dict) -> dict:
    return {k: v.detach().cpu().contiguous().view(torch.uint8).numpy().copy() for k, v in results.items()}


@pytest.mark.parametrize("case", ENTRY_CASES, ids=lambda c: c.entry)
def test_entry_launches_on_the_current_stream(case, delay, side):
    """Stale operands, then -- on a side stream, behind the delay -- the copy of the fresh operands and the entry into the same
    outputs; a clone of an operand buffer on the default stream right behind it is the canary."""
    cycles, delay_ms = delay
    built = case.make()
    assert set(built.stale) == set(built.fresh) and built.canary in built.stale
    const = {k: _to_device(v) for k, v in built.const.items()}
    stale = {k: _to_device(v) for k, v in built.stale.items()}
    fresh = {k: _to_device(v) for k, v in built.fresh.items()}
    for k in stale:
        assert stale[k].shape == fresh[k].shape and stale[k].dtype == fresh[k].dtype, k

    def alone(operands):
        res = _host(built.call({**const, **{k: v.clone() for k, v in operands.items()}}, built.outs()))
        torch.cuda.synchronize()
        return res
    want_stale, want_fresh = alone(stale), alone(fresh)
    assert set(want_stale) == set(want_fresh) and want_fresh
    assert any(not np.array_equal(want_stale[k], want_fresh[k]) for k in want_fresh), f"{case.entry}: stale and fresh operands give one result"
    # the entry on the stale operands, into the buffers the side stream then reuses
    bufs, outs = {k: v.clone() for k, v in stale.items()}, built.outs()
    built.call({**const, **bufs}, outs)
    torch.cuda.synchronize()
    before = bufs[built.canary].clone()                               # (an entry may have advanced a state in place)
    assert not torch.equal(before.view(torch.uint8), fresh[built.canary].view(torch.uint8))
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.cuda._sleep(cycles)
        for k in bufs:
            bufs[k].copy_(fresh[k])
        t0 = time.perf_counter()
        results = built.call({**const, **bufs}, outs)
    canary = bufs[built.canary].clone()                               # the default stream: not behind the delay
    host_ms = (time.perf_counter() - t0) * 1e3
    side.synchronize()
    torch.cuda.synchronize()
    print(f"[streams] {case.entry}: delay {delay_ms:.1f} ms, entry and canary enqueued in {host_ms:.3f} ms")
    assert torch.equal(canary.view(torch.uint8), before.view(torch.uint8)), \
        "delay too short to prove anything: the canary already saw the fresh operand"
    assert delay_ms >= DELAY_OVER_HOST * host_ms, (delay_ms, host_ms)
    got = _host(results)
    for k in want_fresh:
        assert np.array_equal(got[k], want_fresh[k]), (f"{case.entry}: {k} differs from the fresh operands' result: a launch did not "
                                                       f"wait on the stream it was given")


# ---- two threads, two streams ----------------------------------------------------------------------------------------------------
REPEATS = 3


def _in_two_threads(jobs):
    """jobs: two zero-argument callables.  Each runs REPEATS times in a thread of its own on a stream of its own, started together;
    returns the two lists of results, errors re-raised here."""
    errors, results = [], [[], []]
    gate = threading.Barrier(2)

    def work(i):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                gate.wait()
                for _ in range(REPEATS):
                    results[i].append(jobs[i]())
            stream.synchronize()
        except Exception as e:                                    # noqa: BLE001 (re-raised in the main thread)
            errors.append(e)
            gate.abort()
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    return results


@pytest.mark.parametrize("pair", [("umap-fit-transform-blobs", "tsne-B"), ("ward_of_rows-257", "enrich-planted")], ids="+".join)
def test_two_pipelines_in_two_threads_on_their_own_streams(pair):
    cases = [A.case(n) for n in pair]
    inputs = [c.build() for c in cases]
    alone = [c.run(i) for c, i in zip(cases, inputs)]
    results = _in_two_threads([lambda c=c, i=i: c.run(i) for c, i in zip(cases, inputs)])
    for c, want, outs in zip(cases, alone, results):
        assert len(outs) == REPEATS
        for out in outs:
            _assert_equal_results(out, want, f"{c.name} beside {[n for n in pair if n != c.name][0]}")


def test_a_pipeline_beside_a_model_forward_in_two_threads():
    """UMAP of the blobs (three starts, the spectral solver among them) beside predict_step of the 3-layer model that
    tests/test_write_sets_gpu.py::_model_results builds."""
    from tests.helpers import SEQ2REG_512, build_model, seq2gene_kw
    from variantformer_amd.utils.synthetic import TISSUES_54, make_batch
    case = A.case("umap-blobs")
    inputs = case.build()
    batch = make_batch(31, [280, 64], [120, 30], [TISSUES_54[:9], TISSUES_54[3:8]], 200)
    model = build_model(SEQ2REG_512, seq2gene_kw(layers=3), seed=21).cuda()
    model.precision = "bf16-mixed"
    model.predict_step(batch, 0)                                      # (the cache-building first forward)
    alone_model = model.predict_step(batch, 0)
    alone = case.run(inputs)
    torch.cuda.synchronize()
    results = _in_two_threads([lambda: case.run(inputs), lambda: model.predict_step(batch, 0)])
    assert len(results[0]) == len(results[1]) == REPEATS
    for out in results[0]:
        _assert_equal_results(out, alone, "umap-blobs beside predict_step")
    for out in results[1]:
        for key in ("pred_gene_exp", "embeddings"):
            assert len(out[key]) == len(alone_model[key]) == 2
            for g in range(2):
                np.testing.assert_array_equal(out[key][g], alone_model[key][g], err_msg=f"predict_step {key}[{g}] beside umap-blobs")

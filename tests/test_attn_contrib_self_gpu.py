"""vf_attn_contrib_self on a real MI355X (include/vf_hip_gene_contrib.h; operands and float64 references:
tests/gene_contrib_cases.py): accuracy of both outputs against the directly formed contribution vectors, agreement with the Gram
route (ops.attn_contrib with one row per sequence: a formulation with no code in common), independence of a sequence's bits
from the rest of the call, from max_seqlen_k, ldo / ldp and the row map, the write set and read set under the three poison
patterns, the three NaN rules, and one case whose value rows start past element 2^31."""
import pytest
import torch

from tests import attn_contrib_cases as A
from tests import gene_contrib_cases as G
from tests import write_set_cases as W

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from variantformer_amd import _lib
    from variantformer_amd import ops as _ops
    _lib.load()
    return _ops


def _bits(t):
    return t.contiguous().view(torch.int32)


def _cu(kl):
    return torch.tensor([0] + list(torch.tensor(kl).cumsum(0)), dtype=torch.int32, device=DEV)


def run(ops, c, per_head=False, layout="qkv", v=None, v_rows=None, P=None, wo=None, kl=None, max_k=None, extra_o=G.EXTRA_COLS,
        extra_p=G.EXTRA_COLS):
    """One call on case c's operands (or the given replacements); returns out [n_out, max_k] on the host."""
    kl = c.kl if kl is None else kl
    P = c.P if P is None else P
    n_seq = P.shape[0]
    max_k = P.shape[-1] if max_k is None else max_k
    if v is None:
        v = c.v_buffer(layout).to(DEV)[:, -c.D:]
    probs = torch.zeros((n_seq * c.H, max_k + extra_p), dtype=torch.float32, device=DEV)
    probs[:, :P.shape[-1]] = P.reshape(n_seq * c.H, -1).to(DEV)
    n_out = n_seq * (c.H if per_head else 1)
    out = torch.full((n_out, max_k + extra_o), -7.0, dtype=torch.float32, device=DEV)
    ops.attn_contrib_self(v, (c.wo16 if wo is None else wo).to(DEV), probs, _cu(kl), max_k, c.H, c.dh, out=out, per_head=per_head,
                          v_rows=v_rows)
    assert ops.last_kernel("attn") == "attn_contrib_self_kernel"
    torch.cuda.synchronize()
    assert bool((out[:, max_k:] == -7.0).all()), "columns >= max_seqlen_k were touched"
    return out[:, :max_k].cpu()


@pytest.mark.parametrize("layout", ["qkv", "kv"], ids=["v_third_of_qkv", "v_half_of_kv"])
@pytest.mark.parametrize("H,dh,Do,dtype", G.ALL, ids=[f"H{H}-dh{dh}-Do{Do}-{dt}" for H, dh, Do, dt in G.ALL])
def test_against_float64(ops, H, dh, Do, dtype, layout):
    """Both outputs against the float64 contribution vectors.  The limit is 4 x the maximum measured on MI355X over all
    geometries, operand types and value layouts (tests/gene_contrib_cases.py: MEASURED_OUT)."""
    c, ref = G.case(H, dh, Do, dtype), G.reference(H, dh, Do, dtype)
    n = run(ops, c, False, layout)
    ph = run(ops, c, True, layout).view(c.n_seq, H, -1)
    valid = c.valid()
    assert bool((n[~valid] == 0).all()) and bool((ph[~valid[:, None, :].expand_as(ph)] == 0).all())
    e_n, e_ph = G.out_err(n, ref["n"]), G.out_err(ph, ref["per_head"])
    print(f"[attn_contrib_self H={H} dh={dh} Do={Do} {dtype} {layout}] out {e_n:.3e}  per head {e_ph:.3e}  (limit {G.OUT_TOL:.3e})")
    assert e_n <= G.OUT_TOL and e_ph <= G.OUT_TOL


@pytest.mark.parametrize("H,dh,Do,dtype", G.ALL, ids=[f"H{H}-dh{dh}-Do{Do}-{dt}" for H, dh, Do, dt in G.ALL])
def test_against_the_gram_route(ops, H, dh, Do, dtype):
    """ops.attn_contrib on the same operands with cu_rows = arange (one selected row per sequence): S = Wo^T Wo in fp32, a Gram
    matrix per key on the fp32 MFMA, then the quadratic form.  Both stand within their own limit of the float64 value, so
    they agree within the sum of the limits."""
    c = G.case(H, dh, Do, dtype)
    v = c.v_buffer("qkv").to(DEV)[:, 2 * c.D:]
    probs = c.P.reshape(c.n_seq * H, c.max_k).to(DEV)
    cu_rows = torch.arange(c.n_seq + 1, dtype=torch.int32, device=DEV)
    gram = torch.empty((c.tk, H, H), dtype=torch.float32, device=DEV)
    for per_head in (False, True):
        want = torch.empty((c.n_seq * (H if per_head else 1), c.max_k), dtype=torch.float32, device=DEV)
        ops.attn_contrib(v, A.s_gram_of(c.wo16, H, dh).to(DEV), probs, cu_rows, _cu(c.kl), 1, c.max_k, H, dh, gram=gram, out=want,
                         per_head=per_head)
        got = run(ops, c, per_head)
        e = G.out_err(got, want.cpu().double())
        print(f"[attn_contrib_self vs the Gram route H={H} dh={dh} Do={Do} {dtype} {'per head' if per_head else 'summed'}] {e:.3e}")
        assert e <= A.OUT_TOL + G.OUT_TOL


@pytest.mark.parametrize("per_head", [False, True], ids=["summed", "per_head"])
@pytest.mark.parametrize("H,dh,Do", [(4, 32, 96), (32, 48, 1536)])
def test_a_sequences_bits_depend_on_its_own_operands_alone(ops, H, dh, Do, per_head):
    """Sequences 2 (33 keys), 6 (201) and 8 (257: two blocks): inside the large call, alone, alone with a larger max_seqlen_k,
    with wider ldo / ldp; and the whole call through a shuffled row map with repeated rows against the gathered copy."""
    c = G.case(H, dh, Do, "bf16")
    m = H if per_head else 1
    inside = run(ops, c, per_head)
    for s in (2, 6, 8):
        k0, n = int(c.cu_k[s]), c.kl[s]
        v = c.v_buffer("qkv").to(DEV)[k0:k0 + n, 2 * c.D:]
        P = c.P[s:s + 1, :, :n]
        alone = run(ops, c, per_head, v=v, P=P, kl=(n,))
        assert torch.equal(_bits(inside[s * m:(s + 1) * m, :n]), _bits(alone))
        wider = run(ops, c, per_head, v=v, P=P, kl=(n,), max_k=n + 300)
        assert torch.equal(_bits(wider[:, :n]), _bits(alone)) and bool((wider[:, n:] == 0).all())
        strides = run(ops, c, per_head, v=v, P=P, kl=(n,), extra_o=67, extra_p=131)
        assert torch.equal(_bits(strides), _bits(alone))
    # the row map: a table of the distinct value rows in shuffled order; keys 0 .. 99 all name the row of key 0
    g = torch.Generator().manual_seed(11)
    perm = torch.randperm(c.tk, generator=g)
    table = torch.empty(c.tk + 3, 3 * c.D, dtype=c.v16.dtype)
    table.fill_(float("nan"))
    table[perm, 2 * c.D:] = c.v16
    rows = perm.clone()
    rows[:100] = perm[0]
    mapped = run(ops, c, per_head, v=table.to(DEV)[:, 2 * c.D:], v_rows=rows.to(DEV))
    gathered = run(ops, c, per_head, v=table[rows].to(DEV)[:, 2 * c.D:])
    assert torch.equal(_bits(mapped), _bits(gathered)) and not bool(torch.isnan(mapped).any())
    assert c.cu_k[4] >= 100                                                  # sequences 4 .. hold their own rows: the clean call's bits
    assert torch.equal(_bits(mapped[4 * m:]), _bits(inside[4 * m:])) and not torch.equal(_bits(mapped[:4 * m]), _bits(inside[:4 * m]))


WS = G.ws_cases()


@pytest.mark.parametrize("case", WS, ids=[c.name for c in WS])
def test_write_set(ops, case):
    """out and the guards around v (the wrapper cases: a row-map table whose unnamed rows are poisoned), wo, probs (its columns
    past a sequence's keys poisoned) and cu_seqlens_k under 0xFF / 0x00 / 0x3C: the written bytes are exactly the header's write
    set and depend on nothing outside the documented operands (tests/write_set_cases.py::check_write_set)."""
    built = case.make()
    W.check_write_set(built.run, built.written, built.reference, built.nan_ok)


@pytest.mark.parametrize("per_head", [False, True], ids=["summed", "per_head"])
@pytest.mark.parametrize("H,dh,Do", [(4, 32, 96), (2, 48, 96), (32, 48, 1536)])
def test_nan_rules(ops, H, dh, Do, per_head):
    """A NaN in value row (t, h): column j of row s (per_head: of head h's row) and no other element; a NaN at P[s, h, j]:
    out[s, j] (per_head: out[s, h, j]) and no other element; every other element keeps the bits of the clean call.  A NaN in wo
    may reach everything: the call completes and the columns past the keys stay 0."""
    c = G.case(H, dh, Do, "fp16")
    m = H if per_head else 1
    clean = run(ops, c, per_head)
    # value row: key 5 of sequence 3 (64 keys), head h
    s, h, j = 3, H - 1, 5
    v16 = c.v16.clone()
    v16[int(c.cu_k[s]) + j, h * dh + 3] = float("nan")
    got = run(ops, c, per_head, v=torch.cat([c._other, v16], dim=1).to(DEV)[:, 2 * c.D:])
    want = torch.zeros_like(clean, dtype=torch.bool)
    want[s * m + (h if per_head else 0), j] = True
    assert torch.equal(torch.isnan(got), want), (int(torch.isnan(got).sum()), int(want.sum()))
    assert torch.equal(_bits(got[~want]), _bits(clean[~want]))
    # one probability: sequence 6 (201 keys), head 0, key 170
    s, h, j = 6, 0, 170
    P = c.P.clone()
    P[s, h, j] = float("nan")
    got = run(ops, c, per_head, P=P)
    want = torch.zeros_like(clean, dtype=torch.bool)
    want[s * m + (h if per_head else 0), j] = True
    assert torch.equal(torch.isnan(got), want), (int(torch.isnan(got).sum()), int(want.sum()))
    assert torch.equal(_bits(got[~want]), _bits(clean[~want]))
    # wo
    wo = c.wo16.clone()
    wo[1, 2] = float("nan")
    got = run(ops, c, per_head, wo=wo)
    valid = c.valid() if not per_head else c.valid()[:, None, :].expand(c.n_seq, H, c.max_k).reshape(c.n_seq * H, c.max_k)
    assert bool((got[~valid] == 0).all()) and bool(torch.isnan(got).any())


def test_value_rows_past_2_31_elements(ops):
    """v placed with a row stride of 2^24 elements: the rows from 128 on start past element 2^31 (and byte 2^32 long before).
    Bit-equal to the same call on a compact copy; the buffer is NaN everywhere else, so a narrowed offset cannot go unseen.
    Once directly and once through a row map that names the far rows in reverse."""
    H, dh, Do = 4, 32, 96
    c = G.Case(H, dh, Do, "bf16", kl=(70, 64), seed=5)
    stride = 1 << 24
    need = 2 * ((c.tk - 1) * stride + c.D)
    free = torch.cuda.mem_get_info()[0]
    if free < need + (2 << 30):
        pytest.skip(f"free device memory {free} B is below the {need} B of the strided value buffer plus 2 GiB")
    big = torch.empty((c.tk - 1) * stride + c.D, dtype=torch.int16, device=DEV)
    big.fill_(-1)
    v_far = big.view(torch.bfloat16).as_strided((c.tk, c.D), (stride, 1))
    v_far.copy_(c.v16.to(DEV))
    assert (c.tk - 1) * stride > 2 ** 31 and v_far.data_ptr() % 16 == 0
    far = run(ops, c, v=v_far)
    rev = torch.arange(c.tk - 1, -1, -1, dtype=torch.int64, device=DEV)
    v_far.copy_(c.v16.flip(0).to(DEV))
    far_rows = run(ops, c, v=v_far, v_rows=rev)
    near = run(ops, c, layout="compact")
    del v_far, big
    torch.cuda.empty_cache()
    assert torch.equal(_bits(far), _bits(near)) and torch.equal(_bits(far_rows), _bits(near))
    assert G.out_err(near, G.reference_of(c)["n"]) <= G.OUT_TOL

"""vf_attn_contrib on a real MI355X (include/vf_hip_attn_contrib.h; operands and float64 references: tests/attn_contrib_cases.py):
accuracy of both outputs and of the Gram workspace against the directly formed contribution vectors, independence of a row's
bits from the rest of the call, the write set under the three poison patterns (the parallel net of the entries declared in
vf_hip_attn_contrib.h), the four NaN rules, and one case whose value rows start past element 2^31."""
import pytest
import torch

from tests import attn_contrib_cases as A
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


def run(ops, c, per_head=False, contiguous_v=False, v=None, P=None, s_gram=None, kl=None, rl=None, max_rows=None, max_k=None,
        extra=A.EXTRA_COLS):
    """One call on case c's operands (or the given replacements); returns (out [n_out, max_k], gram [tk, H, H]) on the host."""
    kl, rl = c.kl if kl is None else kl, c.rl if rl is None else rl
    P = c.P if P is None else P
    R, tk = P.shape[0], sum(kl)
    max_rows, max_k = max(rl) if max_rows is None else max_rows, P.shape[-1] if max_k is None else max_k
    if v is None:
        v = c.v16.contiguous().to(DEV) if contiguous_v else c.kv16.to(DEV)[:, c.D:]
    probs = torch.zeros((R * c.H, max_k + extra), dtype=torch.float32, device=DEV)
    probs[:, :P.shape[-1]] = P.reshape(R * c.H, -1).to(DEV)
    n_out = R * (c.H if per_head else 1)
    out = torch.full((n_out, max_k + extra), -7.0, dtype=torch.float32, device=DEV)
    gram = torch.full((tk, c.H, c.H), -7.0, dtype=torch.float32, device=DEV)
    cu = lambda x: torch.tensor([0] + list(torch.tensor(x).cumsum(0)), dtype=torch.int32, device=DEV)      # noqa: E731
    ops.attn_contrib(v, (c.s_gram if s_gram is None else s_gram).to(DEV), probs, cu(rl), cu(kl), max_rows, max_k, c.H, c.dh,
                     gram=gram, out=out, per_head=per_head)
    assert ops.last_kernel("attn") == "attn_contrib_kernel"
    torch.cuda.synchronize()
    assert bool((out[:, max_k:] == -7.0).all()), "columns >= max_seqlen_k were touched"
    return out[:, :max_k].cpu(), gram.cpu()


@pytest.mark.parametrize("contiguous_v", [False, True], ids=["v_half_of_kv", "v_contiguous"])
@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("H,dh", A.GEOMETRIES)
def test_against_float64(ops, H, dh, dtype, contiguous_v):
    """Both outputs and the Gram matrices against the float64 contribution vectors.  Measured on MI355X, maxima over all
    geometries, operand types and value layouts: out 1.90e-7 head-summed and 1.57e-7 per head (both H 32, dh 48, fp16), gram
    1.04e-7 (H 2, dh 48, bf16); the limits are 4 x the maxima, 7.6e-7 and 4.2e-7 (tests/attn_contrib_cases.py)."""
    c, ref = A.case(H, dh, dtype), A.reference(H, dh, dtype)
    n, gram = run(ops, c, False, contiguous_v)
    ph, gram_ph = run(ops, c, True, contiguous_v)
    assert torch.equal(_bits(gram), _bits(gram_ph))
    assert torch.equal(_bits(gram), _bits(gram.transpose(1, 2)))                    # G[j, h', h] holds the bits of G[j, h, h']
    valid = c.valid()
    assert bool((n[~valid] == 0).all()) and bool((ph.view(c.R, H, -1)[~valid[:, None, :].expand(c.R, H, c.max_k)] == 0).all())
    e_n, e_ph, e_g = A.out_err(n, ref["n"]), A.out_err(ph.view(c.R, H, -1), ref["per_head"]), A.gram_err(gram, ref["gram"])
    print(f"[attn_contrib H={H} dh={dh} {dtype} {'contiguous' if contiguous_v else 'kv half'}] out {e_n:.3e}  per head {e_ph:.3e}  "
          f"gram {e_g:.3e}  (limits {A.OUT_TOL:.3e} / {A.GRAM_TOL:.3e})")
    assert e_n <= A.OUT_TOL and e_ph <= A.OUT_TOL
    assert e_g <= A.GRAM_TOL


@pytest.mark.parametrize("per_head", [False, True], ids=["summed", "per_head"])
@pytest.mark.parametrize("H,dh", A.GEOMETRIES)
def test_a_rows_bits_do_not_depend_on_the_rest_of_the_call(ops, H, dh, per_head):
    """Sequence 2 (33 rows, 33 keys): inside the large call, alone, and alone with a larger max_rows / max_seqlen_k."""
    c = A.case(H, dh, "bf16")
    _, r, n_rows, k, n_keys = list(c.sequences())[2]
    m = H if per_head else 1
    inside, gram_in = run(ops, c, per_head)
    v = c.kv16.to(DEV)[k:k + n_keys, c.D:]
    P = c.P[r:r + n_rows, :, :n_keys]
    alone, gram_alone = run(ops, c, per_head, v=v, P=P, kl=(n_keys,), rl=(n_rows,))
    wider, gram_wider = run(ops, c, per_head, v=v, P=P, kl=(n_keys,), rl=(n_rows,), max_rows=100, max_k=129)
    assert torch.equal(_bits(inside[r * m:(r + n_rows) * m, :n_keys]), _bits(alone))
    assert torch.equal(_bits(wider[:, :n_keys]), _bits(alone)) and bool((wider[:, n_keys:] == 0).all())
    assert torch.equal(_bits(gram_in[k:k + n_keys]), _bits(gram_alone)) and torch.equal(_bits(gram_wider), _bits(gram_alone))


WS = A.ws_cases()


@pytest.mark.parametrize("case", WS, ids=[c.name for c in WS])
def test_write_set(ops, case):
    """out, gram and the guards around v, probs and s_gram under 0xFF / 0x00 / 0x3C: the written bytes are exactly the header's
    write set and depend on nothing outside the documented operands (tests/write_set_cases.py::check_write_set)."""
    built = case.make()
    W.check_write_set(built.run, built.written, built.reference, built.nan_ok)


@pytest.mark.parametrize("per_head", [False, True], ids=["summed", "per_head"])
@pytest.mark.parametrize("H,dh", A.GEOMETRIES)
def test_nan_rules(ops, H, dh, per_head):
    """A NaN in value row (j, h): column j of that sequence's rows (per_head: of head h's rows) and G[j, h, :], G[j, :, h];
    a NaN probs row: that row; every other element keeps the bits of the clean call.  A NaN in s_gram may reach everything: the
    call completes and the columns past the keys stay 0."""
    c = A.case(H, dh, "fp16")
    m = H if per_head else 1
    clean, gram_clean = run(ops, c, per_head)
    seqs = list(c.sequences())
    # value row: key 5 of sequence 3 (2 rows, 64 keys), head h
    _, r, n_rows, k, n_keys = seqs[3]
    h, j = H - 1, 5
    kv = c.kv16.clone()
    kv[k + j, c.D + h * dh + 3] = float("nan")
    got, gram = run(ops, c, per_head, v=kv.to(DEV)[:, c.D:])
    want = torch.zeros_like(clean, dtype=torch.bool)
    if per_head:
        want[[(r + i) * H + h for i in range(n_rows)], j] = True
    else:
        want[r:r + n_rows, j] = True
    print(f"[attn_contrib nan, value row] NaNs in out {int(torch.isnan(got).sum())} (want {int(want.sum())}), in gram {int(torch.isnan(gram).sum())}")
    assert torch.equal(torch.isnan(got), want)
    assert torch.equal(_bits(got[~want]), _bits(clean[~want]))
    gwant = torch.zeros_like(gram_clean, dtype=torch.bool)
    gwant[k + j, h, :] = True
    gwant[k + j, :, h] = True
    assert torch.equal(torch.isnan(gram), gwant) and torch.equal(_bits(gram[~gwant]), _bits(gram_clean[~gwant]))
    # probs row: row 1 of sequence 2, head 0 (every column of the buffer row)
    _, r, n_rows, k, n_keys = seqs[2]
    P = c.P.clone()
    P[r + 1, 0, :] = float("nan")
    got, gram = run(ops, c, per_head, P=P)
    want = torch.zeros_like(clean, dtype=torch.bool)
    want[(r + 1) * m + 0, :n_keys] = True                   # per_head: head 0's row; columns past the keys are stored zeros
    assert torch.equal(torch.isnan(got), want)
    assert torch.equal(_bits(got[~want]), _bits(clean[~want])) and torch.equal(_bits(gram), _bits(gram_clean))
    # s_gram
    S = c.s_gram.clone()
    S[0, 0, 1, 2] = float("nan")                           # a diagonal block: the per-head form reads it too
    got, _ = run(ops, c, per_head, s_gram=S)
    valid = c.valid() if not per_head else c.valid()[:, None, :].expand(c.R, H, c.max_k).reshape(c.R * H, c.max_k)
    assert bool((got[~valid] == 0).all()) and bool(torch.isnan(got).any())


def test_value_rows_past_2_31_elements(ops):
    """v placed with a row stride of 2^24 elements: the rows from 128 on start past element 2^31 (and byte 2^32 long before).
    Bit-equal to the same call on a compact copy; the buffer is NaN everywhere else, so a narrowed offset cannot go unseen."""
    H, dh = 4, 32
    c = A.Case(H, dh, "bf16", kl=(70, 64), rl=(3, 2), seed=5)
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
    far, gram_far = run(ops, c, v=v_far)
    near, gram_near = run(ops, c, contiguous_v=True)
    del v_far, big
    torch.cuda.empty_cache()
    assert torch.equal(_bits(far), _bits(near)) and torch.equal(_bits(gram_far), _bits(gram_near))
    ref_n = torch.zeros(c.R, c.max_k, dtype=torch.float64)
    u = A.head_vectors(c)
    for _, r, n_rows, k, n_keys in c.sequences():
        ref_n[r:r + n_rows, :n_keys] = torch.einsum("rhj,jhd->rjd", c.P.double()[r:r + n_rows, :, :n_keys], u[k:k + n_keys]).norm(dim=-1)
    assert A.out_err(near, ref_n) <= A.OUT_TOL

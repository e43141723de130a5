"""Every head dim flash-attn takes (multiples of 8 up to 256) through vf_attn_varlen_fwd_v3: attention against the oracle,
bit-exactness of the padded classes against a zero-padded class-dh call, the five class head dims unchanged, and the models
end to end at geometries whose head dim is none of the five."""
import numpy as np
import pytest
import torch

from oracle import vf_oracle as O
from tests.helpers import build_model, check_signal, prel, seq2gene_kw, state_dict_cpu
from variantformer_amd.utils.synthetic import TISSUES_54, make_batch

pytestmark = pytest.mark.gpu

NORTH_STAR_RTOL = 1e-3                      # as tests/test_model_gpu.py
CLASS_DIMS = (32, 48, 64, 96, 128)
NEW_DIMS = [d for d in range(8, 257, 8) if d not in CLASS_DIMS]
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def head_class(d):
    return next(c for c in (32, 48, 64, 96, 128, 192, 256) if d <= c)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from variantformer_amd import ops as _ops
    return _ops


def _cu(lens):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)


def _operands(seed, ql, kl, H, d, dtype, self_attn, amp=2.0):
    """q [tq, H*d], k / v [tk, H*d] uniform in [-amp, amp) (the operands test_ops_gpu.py's attention tolerances were set
    for), rounded to the operand type: cpu fp32 copies and device 16-bit views."""
    g = torch.Generator().manual_seed(seed)
    D = H * d
    tq, tk = sum(ql), sum(kl)
    uni = lambda *shape: ((torch.rand(shape, generator=g) * 2 - 1) * amp).to(TDT[dtype])
    if self_attn:
        qkv = uni(tq, 3 * D)
        dev = qkv.cuda()
        cpu = qkv.float()
        return (cpu[:, :D], cpu[:, D:2 * D], cpu[:, 2 * D:]), (dev[:, :D], dev[:, D:2 * D], dev[:, 2 * D:])
    q = uni(tq, D)
    kv = uni(tk, 2 * D)
    dkv = kv.cuda()
    return (q.float(), kv.float()[:, :D], kv.float()[:, D:]), (q.cuda(), dkv[:, :D], dkv[:, D:])


def _attn_ref(q, k, v, cu_q, cu_k, H, d, slopes, dtype):
    rnd = O.Rounding(dtype)
    out = torch.zeros(q.shape[0], H * d)
    for b in range(len(cu_q) - 1):
        a, e = int(cu_q[b]), int(cu_q[b + 1])
        ka, ke = int(cu_k[b]), int(cu_k[b + 1])
        if e > a and ke > ka:
            out[a:e] = O.attention(q[a:e].view(-1, H, d), k[ka:ke].view(-1, H, d), v[ka:ke].view(-1, H, d),
                                   slopes, rnd).reshape(e - a, H * d)
    return out


def _vs_oracle(ops, d, H, ql, kl, alibi, dtype, seed=21):
    self_attn = kl is None
    kl = ql if self_attn else kl
    (q, k, v), (dq, dk, dv) = _operands(seed, ql, kl, H, d, dtype, self_attn)
    cu_q, cu_k = _cu(ql), _cu(kl)
    slopes = torch.tensor(O.alibi_slopes(H), dtype=torch.float32) if alibi else None
    out = ops.attn_varlen(dq, dk, dv, cu_q.cuda(), cu_k.cuda(), max(ql), max(kl), H, d, slopes.cuda() if alibi else None)
    torch.cuda.synchronize()
    kernel = ops.last_kernel("attn")
    ref = _attn_ref(q, k, v, cu_q, cu_k, H, d, slopes, dtype)
    # the tolerances of test_ops_gpu.py::test_attention_matches_oracle: 16-bit output + 16-bit P rounded at a different
    # running maximum than the oracle's final one
    want = ref.to(TDT[dtype]).float().numpy()
    np.testing.assert_allclose(out.float().cpu().numpy(), want, rtol=2 ** -7, atol=6e-3, err_msg=f"d={d} {kernel}")
    return kernel


# (H, q lens, k lens (None = self), alibi): self attention with ALiBi, cross attention without, ragged with an empty key
# sequence (zero rows) and a 1-token sequence
SWEEP = [
    (2, [70, 33, 1], None, True),
    (2, [10, 50, 130], [9, 300, 64], False),
    (3, [5, 200, 64, 1], [17, 0, 65, 129], False),
]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("d", NEW_DIMS)
def test_attention_every_head_dim_vs_oracle(ops, d, dtype):
    for i, (H, ql, kl, alibi) in enumerate(SWEEP):
        _vs_oracle(ops, d, H, ql, kl, alibi, dtype, seed=100 * d + i)


def _lens(seed, n, lo, hi):
    return [int(x) for x in np.random.default_rng(seed).integers(lo, hi + 1, n)]


# geometries that reach every kernel family a class routes to: (d, H, q lens, k lens, alibi, expected kernel prefix)
FAMILIES = [
    (16, 16, _lens(1, 64, 1, 128), None, False, "attn_short2_kernel<1 pass>"),        # class 32, <= 128 tokens
    (56, 16, _lens(2, 64, 1, 128), None, True, "attn_short2_kernel<1 pass>"),         # class 64
    (40, 4, [201, 150, 201, 129], None, True, "attn_short2_kernel<2 passes>"),        # class 48, 129-256 tokens
    (56, 8, _lens(3, 128, 129, 200), None, False, "attn_short2_kernel<2 passes>"),     # class 64, 129-256 tokens
    (24, 4, [250, 240, 3], None, True, "attn_short_kernel"),                          # class 32: the image is too large for 3
    (40, 8, [603], [1024], False, "attn_x32_kernel"),                                 # class 48 without ALiBi
    (80, 4, [300, 64], None, True, "attn_fwd_kernel<64-query blocks>"),               # class 96, > 256 tokens
    (72, 16, _lens(4, 64, 65, 128), None, False, "attn_fwd_kernel<128-query blocks>"),  # class 96, 65-128-token windows
    (8, 4, [300, 1, 77], None, False, "attn_fwd_kernel<64-query blocks>"),            # class 32, > 256 tokens
    (136, 2, [201, 70], None, True, "attn_fwd_kernel<64-query blocks>"),              # class 192
    (200, 2, [300, 9], [257, 64], False, "attn_fwd_kernel<64-query blocks>"),         # class 256
]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_every_kernel_family_reached_vs_oracle(ops, dtype):
    reached = set()
    for i, (d, H, ql, kl, alibi, want) in enumerate(FAMILIES):
        kernel = _vs_oracle(ops, d, H, ql, kl, alibi, dtype, seed=7 + i)
        assert kernel.startswith(want), (d, kernel, want)
        reached.add(kernel.split("<")[0])
    assert reached == {"attn_short2_kernel", "attn_short_kernel", "attn_x32_kernel", "attn_fwd_kernel"}


def _pad_heads(x, H, d, c):
    return torch.nn.functional.pad(x.view(-1, H, d), (0, c - d)).reshape(-1, H * c)


# per class: the geometries of its kernel families (self attention unless k lens are given)
EXACT_GEOMS = {
    32: [(16, _lens(5, 64, 1, 128), None, False), (4, [250, 240, 3], None, True), (2, [300, 33], None, True)],
    48: [(4, [201, 150, 129], None, True), (4, [603, 20], [1024, 5], False), (2, [300, 1], None, True)],
    64: [(16, _lens(6, 64, 1, 128), None, False), (8, _lens(7, 128, 129, 200), None, True), (2, [300], [100], False)],
    96: [(16, _lens(8, 64, 65, 128), None, True), (2, [300, 17], None, False)],
    128: [(2, [130, 64, 1], None, True), (2, [257], [500], False)],
    192: [(2, [201, 70, 1], None, True), (2, [130], [300], False)],
    256: [(2, [201, 70, 1], None, True), (2, [130], [300], False)],
}


@pytest.mark.parametrize("d", NEW_DIMS + [192, 256])
def test_padding_is_exact(ops, d):
    """A head dim d below its class c gives, bit for bit, the first d columns of a class-dh call on operands zero-padded per
    head (same scale 1/sqrt(d), same flags) -- through the same kernel.  192 / 256 run against their own class too."""
    c = head_class(d)
    for gi, (H, ql, kl, alibi) in enumerate(EXACT_GEOMS[c]):
        self_attn = kl is None
        kl = ql if self_attn else kl
        for dtype, q_log2, q_at_start in (("bf16", True, False), ("fp16", False, alibi)):
            (_, _, _), (dq, dk, dv) = _operands(1000 * d + gi, ql, kl, H, d, dtype, self_attn, amp=1.5)
            cq, ck = _cu(ql).cuda(), _cu(kl).cuda()
            slopes = torch.tensor(O.alibi_slopes(H), dtype=torch.float32).cuda() if alibi else None
            scale = 1.0 / float(np.sqrt(d))
            kw = dict(q_log2=q_log2, q_at_start=q_at_start, scale=scale)
            out_d = ops.attn_varlen(dq, dk, dv, cq, ck, max(ql), max(kl), H, d, slopes, **kw)
            k_d = ops.last_kernel("attn")
            pq, pk, pv = (_pad_heads(t, H, d, c) for t in (dq, dk, dv))
            # the class-dh call goes through v3 as well when c is one of the padded-only classes (192 / 256)
            out_c = ops.attn_varlen(pq, pk, pv, cq, ck, max(ql), max(kl), H, c, slopes, **kw)
            k_c = ops.last_kernel("attn")
            torch.cuda.synchronize()
            t = out_d.shape[0]
            assert k_d == k_c, (d, c, k_d, k_c)
            assert torch.equal(out_d.view(t, H, d), out_c.view(t, H, c)[..., :d]), (d, c, gi, dtype, k_d)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_v3_equals_v2_at_class_dims(ops, monkeypatch, dtype):
    geoms = [(32, 16, _lens(9, 64, 1, 128), None, False), (48, 4, [201, 129], None, True), (48, 8, [603], [1024], False),
             (64, 8, _lens(10, 128, 129, 200), None, False), (96, 2, [300, 64], None, True), (128, 2, [130], [257], False)]
    for i, (d, H, ql, kl, alibi) in enumerate(geoms):
        self_attn = kl is None
        kl = ql if self_attn else kl
        (_, _, _), (dq, dk, dv) = _operands(i, ql, kl, H, d, dtype, self_attn)
        cq, ck = _cu(ql).cuda(), _cu(kl).cuda()
        slopes = torch.tensor(O.alibi_slopes(H), dtype=torch.float32).cuda() if alibi else None
        for q_log2 in (False, True):
            v2 = ops.attn_varlen(dq, dk, dv, cq, ck, max(ql), max(kl), H, d, slopes, q_log2=q_log2)
            k2 = ops.last_kernel("attn")
            with monkeypatch.context() as m:
                m.setattr(ops, "ATTN_CLASS_DIMS", ())                 # every head dim through vf_attn_varlen_fwd_v3
                v3 = ops.attn_varlen(dq, dk, dv, cq, ck, max(ql), max(kl), H, d, slopes, q_log2=q_log2)
                k3 = ops.last_kernel("attn")
            torch.cuda.synchronize()
            assert k2 == k3 and torch.equal(v2, v3), (d, k2, k3)


def test_unsupported_head_dims_fail_with_the_library_message(ops):
    from variantformer_amd._lib import VFError
    for d in (12, 264):
        (_, _, _), (dq, dk, dv) = _operands(0, [10], [10], 2, d, "bf16", True)
        cu = _cu([10]).cuda()
        with pytest.raises(VFError, match="head_dim"):
            ops.attn_varlen(dq, dk, dv, cu, cu, 10, 10, 2, d)


# ---- models

def _s2r_hp(d, h, pe, pool):
    return dict(vocab_size=500, embedding_dim=d, num_heads=h, num_layers=2, num_tissues=2, num_classes=2,
                learning_rate=1e-4, loss_fn=["cross_entropy", "0"], seq_pool=pool, cre_type="binary",
                token_length=200, use_context=False, positional_encoding=pe, use_flash=True)


def _erel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / (np.abs(b) + np.sqrt((b * b).mean()) + 1e-30)).max())


@pytest.mark.parametrize("d,h,pe,pool,dtype", [
    (512, 32, "sinusoidal", "mean", "bf16"), (512, 32, "alibi", "max", "fp16"),
    (512, 2, "alibi", "mean", "bf16"), (512, 2, "sinusoidal", "max", "fp16"),
    (640, 8, "sinusoidal", "mean", "fp16"), (640, 8, "alibi", "max", "bf16"),
])
def test_seq2reg_new_head_dims_vs_oracle(ops, d, h, pe, pool, dtype):
    from variantformer_amd.seq2reg.model import Seq2RegPredictor
    hp = _s2r_hp(d, h, pe, pool)
    torch.manual_seed(17)
    m = Seq2RegPredictor(**hp)
    sd = state_dict_cpu(m)
    m = m.cuda().eval()
    rng = np.random.default_rng(d + h)
    W, L = 24, 200
    ids = torch.from_numpy(rng.integers(0, 500, (W, 1, L))).long()
    lens = rng.integers(1, L + 1, W)
    lens[:3] = (L, 1, 129)
    pad = torch.arange(L)[None, None, :] >= torch.from_numpy(lens)[:, None, None]
    with ops.compute_dtype(TDT[dtype]):
        got = m(ids, pad, None, only_embed=True)
    orc = O.seq2reg_embed(ids, pad, sd, "", O.Seq2RegHP.from_hparams(hp), O.Rounding(dtype))
    assert got.shape == orc.shape
    assert _erel(got.cpu().numpy(), orc.numpy()) < 1e-2, (d, h)          # as test_seq2reg_options_vs_reference_golden


@pytest.mark.parametrize("heads,tok", [(8, (512, 32)), (6, (640, 8))])
def test_predict_step_new_head_dims_vs_oracle(heads, tok):
    """Modulator D = 1536 at H = 8 (dh 192) and H = 6 (dh 256, non-power-of-two ALiBi slopes), tokenizers at dh 16 / 80."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    td, th = tok
    s2r = _s2r_hp(td, th, "sinusoidal", "mean")
    kw = seq2gene_kw(heads=heads, layers=2, token_dim=td, gene_emb_dim=td)
    model = build_model(s2r, kw, seed=4242)
    sd = state_dict_cpu(model)
    model = model.cuda()
    batch = make_batch(99, [12, 3], [5, 2], [TISSUES_54[:3], [9]], 200)
    out = model.predict_step(batch, 0)
    hp = O.Seq2RegHP.from_hparams(s2r)
    orc = O.predict_step(batch, sd, hp, hp, O.Seq2GeneHP.from_kwargs(kw), rounding="bf16", share_cre_stream=True)
    for i in range(2):
        assert prel(out["pred_gene_exp"][i], orc["pred_gene_exp"][i]) < NORTH_STAR_RTOL
        assert _erel(out["embeddings"][i], orc["embeddings"][i]) < 3 * NORTH_STAR_RTOL
    check_signal(f"D=1536 H={heads}, tokenizer {td}/{th}", out["pred_gene_exp"], orc["pred_gene_exp"])
    again = model.predict_step(batch, 0)
    for i in range(2):                                                   # run-to-run determinism
        assert np.array_equal(again["pred_gene_exp"][i], out["pred_gene_exp"][i])
        assert np.array_equal(again["embeddings"][i], out["embeddings"][i])

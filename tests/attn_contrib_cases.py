"""Operands and float64 references of vf_attn_contrib (include/vf_hip_attn_contrib.h), shared by tests/test_attn_contrib_cpu.py,
tests/test_attn_contrib_gpu.py and tests/test_contribution_maps_gpu.py.  Importing this module needs no GPU.

The reference forms the contribution VECTORS directly,
    c[r, j, :] = sum_h P[r, h, j] * Wo[:, h*dh:(h+1)*dh] @ v[j, h, :]      (float64, [rows, keys, Do])  ->  n = ||c||_2,
never the Gram form the kernel uses, so a transposed S[h, h'], a wrong head stride or a dropped cross-head term cannot cancel
between the kernel and its reference.  The kernel sees Wo only through S = Wo^T Wo (fp32, built here as MHA.contrib_gram builds
it: float64 accumulation of the 16-bit weight, one rounding), so the test's Wo is [DO, H * dh] with a small DO.

The operands are built so that the quantity cannot be mistaken for a cheaper one (tests/test_attn_contrib_cpu.py checks it on
the references alone): the value rows and the out_proj columns of different heads share a direction (the cross-head terms
P_h P_h' G[h, h'] carry a large part of the norm), the heads have different gains, the keys different value norms, and a
per-(head, head') asymmetric part keeps S[h, h'] away from S[h', h].

The limits OUT_TOL / GRAM_TOL are 4 x the maxima measured on an MI355X over all geometries below (the margin of
tests/test_attn_probs_alibi_gpu.py: one more fp32 rounding per term on another box); the measured values stand beside them.
"""
from __future__ import annotations

import functools
import math

import torch

KEY_LENS = (1, 31, 33, 64, 0, 70)          # one call: a single key, one short of / one past a 32-key step, a full 64-key tile,
ROW_LENS = (1, 3, 33, 2, 2, 0)             # no keys (rows written as zeros), 70 keys without selected rows (gram only)
GEOMETRIES = ((4, 32), (2, 48), (32, 48))  # (H, dh)
DTYPES = ("bf16", "fp16")
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
DO = 96                                    # rows of the test's Wo
EXTRA_COLS = 5                             # ldp / ldo wider than max_k

# max |n - n64| / rowmax(n64) over head-summed and per-head outputs; max |G - G64| / max_j G64[j, h, h].
# Measured on MI355X over GEOMETRIES x DTYPES x both value layouts (the layout does not change a bit):
MEASURED_OUT = 1.901e-7           # H 32, dh 48, fp16, head-summed (per head: 1.573e-7)
MEASURED_GRAM = 1.043e-7          # H 2, dh 48, bf16
OUT_TOL = 4.0 * MEASURED_OUT
GRAM_TOL = 4.0 * MEASURED_GRAM


def s_gram_of(wo16: torch.Tensor, H: int, dh: int) -> torch.Tensor:
    """fp32 [H, H, dh, dh] from the 16-bit weight [Do, H * dh]: float64 accumulation, one rounding (MHA.contrib_gram)."""
    w = wo16.double()
    return (w.t() @ w).view(H, dh, H, dh).permute(0, 2, 1, 3).float().contiguous()


class Case:
    def __init__(self, H: int, dh: int, dtype: str, kl=KEY_LENS, rl=ROW_LENS, seed: int = 0):
        self.H, self.dh, self.D, self.dtype = H, dh, H * dh, dtype
        self.kl, self.rl = tuple(kl), tuple(rl)
        self.tk, self.R, self.max_k, self.max_rows = sum(kl), sum(rl), max(kl), max(rl)
        g = torch.Generator().manual_seed(9100 + 97 * H + dh + seed)
        dt = TDT[dtype]
        # value rows: a direction shared by the heads of a key + the head's own part, the key's own scale
        scale = torch.exp(0.8 * torch.randn(self.tk, 1, 1, generator=g))
        v = (0.8 * torch.randn(self.tk, 1, dh, generator=g) + 0.6 * torch.randn(self.tk, H, dh, generator=g)) * scale
        k = torch.randn(self.tk, self.D, generator=g)                    # the K half of a [tokens, 2D] buffer: never read
        self.kv16 = torch.cat([k, v.reshape(self.tk, self.D)], dim=1).to(dt)
        # out_proj: columns shared by the heads (mixed by a matrix of the head's own, I + A_h) + own columns, a gain per head:
        # S[h, h'] is far from S[h', h]
        shared = torch.randn(DO, dh, generator=g)
        mix = torch.eye(dh)[None] + 0.5 * torch.randn(H, dh, dh, generator=g) / math.sqrt(dh)
        gain = torch.exp(0.5 * torch.randn(H, 1, 1, generator=g))
        wo = (0.8 * torch.einsum("de,hef->hdf", shared, mix) + 0.6 * torch.randn(H, DO, dh, generator=g)) * gain
        self.wo16 = (wo.permute(1, 0, 2).reshape(DO, self.D) / math.sqrt(dh)).to(dt)          # [DO, H * dh]
        self.s_gram = s_gram_of(self.wo16, H, dh)
        # per-head probabilities, fp32, exactly 0 past a sequence's keys; sharp enough that rows differ between heads
        P = torch.zeros(self.R, H, self.max_k, dtype=torch.float64)
        r = 0
        for n_rows, n_keys in zip(self.rl, self.kl):
            if n_rows and n_keys:
                P[r:r + n_rows, :, :n_keys] = torch.softmax(2.0 * torch.randn(n_rows, H, n_keys, generator=g, dtype=torch.float64), dim=-1)
            r += n_rows
        self.P = P.float()
        self.cu_rows = torch.tensor([0] + list(torch.tensor(self.rl).cumsum(0)), dtype=torch.int32)
        self.cu_k = torch.tensor([0] + list(torch.tensor(self.kl).cumsum(0)), dtype=torch.int32)

    @property
    def v16(self):
        """The value rows as the [:, D:] half of the [tokens, 2D] buffer (row stride 2D)."""
        return self.kv16[:, self.D:]

    def sequences(self):
        """(sequence, first row, rows, first key, keys)."""
        r = k = 0
        for s, (n_rows, n_keys) in enumerate(zip(self.rl, self.kl)):
            yield s, r, n_rows, k, n_keys
            r, k = r + n_rows, k + n_keys

    def valid(self) -> torch.Tensor:
        """bool [R, max_k]: column j is a key of row r's sequence."""
        m = torch.zeros(self.R, self.max_k, dtype=torch.bool)
        for _, r, n_rows, _, n_keys in self.sequences():
            m[r:r + n_rows, :n_keys] = True
        return m


@functools.lru_cache(maxsize=None)
def case(H: int, dh: int, dtype: str) -> Case:
    return Case(H, dh, dtype)


def head_vectors(c: Case) -> torch.Tensor:
    """float64 [tk, H, DO]: u[j, h] = Wo[:, h*dh:(h+1)*dh] @ v[j, h]."""
    wo = c.wo16.double().view(DO, c.H, c.dh)
    return torch.einsum("dhe,jhe->jhd", wo, c.v16.double().reshape(c.tk, c.H, c.dh))


@functools.lru_cache(maxsize=None)
def reference(H: int, dh: int, dtype: str) -> dict:
    """float64: n [R, max_k], per_head [R, H, max_k] (both 0 past a sequence's keys), gram [tk, H, H] -- all from the vectors."""
    c = case(H, dh, dtype)
    u = head_vectors(c)
    P = c.P.double()
    n = torch.zeros(c.R, c.max_k, dtype=torch.float64)
    ph = torch.zeros(c.R, c.H, c.max_k, dtype=torch.float64)
    for _, r, n_rows, k, n_keys in c.sequences():
        if n_rows and n_keys:
            p = P[r:r + n_rows, :, :n_keys]
            vec = torch.einsum("rhj,jhd->rjd", p, u[k:k + n_keys])                   # the contribution vectors themselves
            n[r:r + n_rows, :n_keys] = vec.norm(dim=-1)
            ph[r:r + n_rows, :, :n_keys] = p * u[k:k + n_keys].norm(dim=-1).t()[None]
    return {"n": n, "per_head": ph, "gram": torch.einsum("jhd,jgd->jhg", u, u)}


def wrong_quantities(H: int, dh: int, dtype: str) -> dict:
    """What a plausible mistake computes instead of n, float64 [R, max_k] each:
      diagonal   sqrt(sum_h P_h^2 G_hh): the cross-head terms dropped;
      weight     P_mean * ||Wo v_j||: the head-mean map times the norm of the key's transformed value;
      no_wo      ||sum_h P_h v[j, h]||: the value-weighted norm without out_proj;
      s_swapped  the Gram form with S[h', h] where S[h, h'] belongs."""
    c = case(H, dh, dtype)
    u = head_vectors(c)
    P = c.P.double()
    v = c.v16.double().reshape(c.tk, c.H, c.dh)
    S = c.s_gram.double()
    g_swapped = torch.einsum("jhe,ghef,jgf->jhg", v, S, v)            # v_h^T S[h', h] v_h'
    out = {name: torch.zeros(c.R, c.max_k, dtype=torch.float64) for name in ("diagonal", "weight", "no_wo", "s_swapped")}
    for _, r, n_rows, k, n_keys in c.sequences():
        if n_rows and n_keys:
            p, uu = P[r:r + n_rows, :, :n_keys], u[k:k + n_keys]
            sl = (slice(r, r + n_rows), slice(0, n_keys))
            out["diagonal"][sl] = torch.sqrt(torch.einsum("rhj,jh->rj", p * p, (uu * uu).sum(-1)))
            out["weight"][sl] = p.mean(dim=1) * uu.sum(dim=1).norm(dim=-1)[None]
            out["no_wo"][sl] = torch.einsum("rhj,jhe->rje", p, v[k:k + n_keys]).norm(dim=-1)
            out["s_swapped"][sl] = torch.sqrt(torch.einsum("rhj,rgj,jhg->rj", p, p, g_swapped[k:k + n_keys]).clamp_min(0.0))
    return out


def out_err(got: torch.Tensor, want: torch.Tensor) -> float:
    """max over rows of max_j |got - want| / rowmax(want); rows whose reference is all zero must be zero exactly."""
    got, want = got.double().reshape(-1, want.shape[-1]), want.reshape(-1, want.shape[-1])
    top = want.abs().amax(dim=-1, keepdim=True)
    assert bool((got[(top == 0).expand_as(got)] == 0).all())
    keep = top[:, 0] > 0
    return float(((got - want).abs()[keep] / top[keep]).max()) if bool(keep.any()) else 0.0


def gram_err(got: torch.Tensor, want: torch.Tensor) -> float:
    """max |G - G64| / max_j G64[j, h, h]."""
    diag = torch.diagonal(want, dim1=1, dim2=2)
    return float((got.double() - want).abs().max() / diag.max())


# ---- the oracle-side recorder (tests/test_contribution_maps_gpu.py) ---------------------------------------------------------
def record_oracle_contributions(monkeypatch):
    """tests/attn_map_cases.py::record_oracle_maps with the value side: wraps O.mha_cross (undone by `monkeypatch`) and, for
    every gene-layer call, recomputes q, K and V at the oracle's rounding points, reads out_proj.weight at the rounding the
    product packs (rnd.r: the 16-bit operand of the out_proj GEMM; fp32 in the fp32 mode), and records per (call, sequence
    pair) `layer`, `mean` float64 [rows, N] (the head-mean map), `n` float64 [rows, N] (the norm of the contribution vectors,
    formed directly) and `per_head` float64 [rows, H, N] (P_h ||Wo_h v_h||)."""
    from oracle import vf_oracle as O
    records = []
    original = O.mha_cross

    def wrapped(xq, xkv, sd, pfx, H, cu_q, cu_k, rnd, slopes=None, kv_labels=None):
        if "gene_layers." in pfx:
            assert slopes is None, "the maps are defined for a cross attention without positional bias"
            D = xq.shape[-1]
            dh = D // H
            pre = rnd.q_prescale
            q = rnd.r(O.linear(xq, sd[pfx + "Wq.weight"], sd[pfx + "Wq.bias"], rnd,
                               wscale=math.log2(math.e) / math.sqrt(dh) if pre else 1.0)).view(-1, H, dh)
            kv = rnd.r(O.linear(xkv, sd[pfx + "Wkv.weight"], sd[pfx + "Wkv.bias"], rnd)).view(-1, 2, H, dh)
            wo = rnd.r(sd[pfx + "out_proj.weight"]).double().view(D, H, dh)
            c = 1.0 if pre else math.log2(math.e) / math.sqrt(dh)
            layer = int(pfx.split("gene_layers.")[1].split(".")[0])
            for b in range(len(cu_q) - 1):
                a, e, ka, ke = int(cu_q[b]), int(cu_q[b + 1]), int(cu_k[b]), int(cu_k[b + 1])
                if e > a and ke > ka:
                    s2 = torch.einsum("rhd,jhd->rhj", q[a:e].double(), kv[ka:ke, 0].double()) * c
                    p = torch.exp2(s2 - s2.max(dim=-1, keepdim=True).values)
                    p = p / p.sum(dim=-1, keepdim=True)
                    u = torch.einsum("dhe,jhe->jhd", wo, kv[ka:ke, 1].double())
                    records.append({"layer": layer, "mean": p.mean(dim=1), "rows": p, "u": u})
        return original(xq, xkv, sd, pfx, H, cu_q, cu_k, rnd, slopes=slopes, kv_labels=kv_labels)

    monkeypatch.setattr(O, "mha_cross", wrapped)
    return records


def oracle_registry_contributions(monkeypatch, batch, sd, cre_hp, gene_hp, hp, rounding, layers=None):
    """(maps, contributions, per_head): per gene float64 [len(layers), T_i, N_i] head-mean maps and contribution norms and
    [len(layers), T_i, H, N_i] per-head norms of the registry-token rows, from one oracle forward with the given rounding mode
    (the conventions of tests/attn_map_cases.py::oracle_registry_maps)."""
    from oracle import vf_oracle as O
    from variantformer_amd.attn_maps import select_layers
    with monkeypatch.context() as mp:
        records = record_oracle_contributions(mp)
        O.predict_step(batch, sd, cre_hp, gene_hp, hp, rounding=rounding, share_cre_stream=True)
    n_layers, n_genes = hp.num_layers, len(batch["cre_sequences"])
    assert len(records) == n_genes * n_layers
    maps, contrib, per_head = [], [], []
    for i in range(n_genes):
        G = int(batch["gene_embeddings"][i].shape[0]) + 1
        recs = records[i * n_layers:(i + 1) * n_layers]
        assert [r["layer"] for r in recs] == list(range(n_layers))
        m, n, ph = [], [], []
        for l in select_layers(n_layers, layers):
            p, u = recs[l]["rows"][::G], recs[l]["u"]                                   # the registry rows: [T, H, N]
            m.append(recs[l]["mean"][::G])
            n.append(torch.einsum("rhj,jhd->rjd", p, u).norm(dim=-1))
            ph.append(p * u.norm(dim=-1).t()[None])
        maps.append(torch.stack(m).numpy())
        contrib.append(torch.stack(n).numpy())
        per_head.append(torch.stack(ph).numpy())
    return maps, contrib, per_head


def row_err(got, want) -> float:
    """max over rows (and leading axes) of max_j |got - want| / rowmax(want)."""
    import numpy as np
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want).max(axis=-1) / want.max(axis=-1)).max())


# ---- the parallel write-set net: one case list for the entries of include/vf_hip_attn_contrib.h --------------------------------------
# tests/write_set_cases.py's machinery (poison patterns, guarded operands, check_write_set) on vf_attn_contrib; its CASES table
# is a yardstick of the main header and stays as it is, so this list stands beside it.  tests/test_attn_contrib_cpu.py requires
# every stream-taking declaration of vf_hip_attn_contrib.h to be named here; tests/test_attn_contrib_gpu.py runs the cases.
GRAM_PAD = 8            # gram rows past cu_seqlens_k[n_seq] that must stay untouched


def _make_ws(H, dh, dtype, per_head, wrapper):
    def make():
        from tests import write_set_cases as W
        c = case(H, dh, dtype)
        ref = reference(H, dh, dtype)
        n_out = c.R * (H if per_head else 1)
        cols = c.max_k + EXTRA_COLS
        valid = c.valid()

        def run(p):
            from variantformer_amd import _lib
            ops = W._ops()
            v = W.guarded(c.v16.contiguous(), p, W.GUARD_COLS)
            s_gram = W.guarded(c.s_gram.reshape(-1), p).view(H, H, dh, dh)
            probs = W.guarded(c.P.reshape(c.R * H, c.max_k), p, W.GUARD_COLS)
            inval = (~valid)[:, None, :].expand(c.R, H, c.max_k).reshape(c.R * H, c.max_k).to(W.DEVICE)
            probs[inval] = W.poisoned((int(inval.sum()),), torch.float32, W.DEVICE, p)     # columns past a sequence's keys are not read
            cu_rows, cu_k = W.guarded(c.cu_rows, p), W.guarded(c.cu_k, p)
            big, out = W.arena(n_out, cols, torch.float32, p)
            gram = W.poisoned((c.tk + GRAM_PAD, H, H), torch.float32, W.DEVICE, p)
            if wrapper:
                with W.poison_allocations(p) as proxy:
                    ops.attn_contrib(v, s_gram, probs, cu_rows, cu_k, c.max_rows, c.max_k, H, dh, gram=gram, out=out,
                                     per_head=per_head)
                assert proxy.count == 0, "ops.attn_contrib allocates nothing: out, gram and probs are the caller's"
            else:
                _lib.check(_lib.load().vf_attn_contrib(v.data_ptr(), v.stride(0), s_gram.data_ptr(), probs.data_ptr(), probs.stride(0),
                                                       cu_rows.data_ptr(), cu_k.data_ptr(), len(c.kl), c.max_rows, c.max_k, H, dh,
                                                       ops._dt(TDT[dtype]), int(per_head), gram.data_ptr(), out.data_ptr(),
                                                       out.stride(0), W._stream()), "vf_attn_contrib")
            assert ops.last_kernel("attn") == "attn_contrib_kernel"
            W._sync()
            return {"out": big, "gram": gram}

        def check(bufs):
            body = bufs["out"][8:8 + n_out, W.GUARD_COLS:W.GUARD_COLS + c.max_k]
            if per_head:
                body = body.view(c.R, H, c.max_k)
                assert bool((body[~valid[:, None, :].expand_as(body)] == 0).all())
                assert out_err(body, ref["per_head"]) <= OUT_TOL
            else:
                assert bool((body[~valid] == 0).all()), "columns past a sequence's keys are not zero"
                assert out_err(body, ref["n"]) <= OUT_TOL
            assert gram_err(bufs["gram"][:c.tk], ref["gram"]) <= GRAM_TOL
        inner = torch.zeros((n_out, cols), dtype=torch.bool)
        inner[:, :c.max_k] = True           # every selected row belongs to a sequence; columns >= max_seqlen_k are not touched
        gmask = torch.zeros((c.tk + GRAM_PAD, H, H), dtype=torch.bool)
        gmask[:c.tk] = True                 # every key's G, the keys of the sequence without selected rows included
        return W.Built(run, {"out": W.arena_mask(n_out, cols, inner), "gram": gmask}, check)
    return make


def ws_cases() -> list:
    from tests import write_set_cases as W
    out = []
    for H, dh in GEOMETRIES:
        for dtype in DTYPES if (H, dh) == (4, 32) else ("bf16",):
            for per_head in (False, True):
                for wrapper in (False, True):
                    out.append(W.WSCase(f"attn_contrib-H{H}-dh{dh}-{dtype}-{'per_head' if per_head else 'summed'}-"
                                        f"{'wrapper' if wrapper else 'entry'}", "attn_contrib", ("vf_attn_contrib",),
                                        ("attn_contrib",) if wrapper else (), _make_ws(H, dh, dtype, per_head, wrapper)))
    return out

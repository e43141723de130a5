"""Operands and float64 references of vf_attn_contrib_self (include/vf_hip_gene_contrib.h), shared by
tests/test_gene_contrib_cpu.py, tests/test_attn_contrib_self_gpu.py and tests/test_gene_contribution_maps_gpu.py.  Importing this
module needs no GPU.

One selected row per sequence (the registry token of a (gene, tissue) pair over its own sequence), so row s is sequence s.  The
reference forms the contribution VECTORS directly,
    c[s, j, :] = sum_h P[s, h, j] * Wo[:, h*dh:(h+1)*dh] @ v[t, h, :],   t = cu_k[s] + j      (float64)  ->  n = ||c||_2,
as one float64 product (P (.) v) @ Wo^T; the per-head norms from one product per head.  The operands are built in the manner of
tests/attn_contrib_cases.py (a direction shared by the heads of a key and by the heads' columns of Wo, a gain per head, a scale
per key), so the quantity cannot be mistaken for a cheaper one: tests/test_gene_contrib_cpu.py checks that on the references.

OUT_TOL is 4 x the maximum measured on an MI355X over all geometries, both operand types and both value layouts (the margin
rule of tests/test_attn_probs_alibi_gpu.py); the measured value stands beside it.
"""
from __future__ import annotations

import functools
import math

import torch

from tests import attn_contrib_cases as A

KEY_TILE = 256                                       # keys per block of attn_contrib_self_kernel (CS_KEYS)
# one call: a single key, one short of / one past a wave's 32 keys, two waves, no keys (a row of zeros), 70, the bench's 201,
# one short of and one past the kernel's key tile (the second needs a second block for one key)
KEY_LENS = (1, 31, 33, 64, 0, 70, 201, KEY_TILE - 1, KEY_TILE + 1)
GEOMETRIES = ((4, 32, 96), (2, 48, 96), (32, 48, 96), (32, 48, 1536))      # (H, dh, Do); the last: every group of Wo tiles
BF16_ONLY = ((2, 64, 96), (2, 96, 96), (2, 128, 96))
DTYPES = A.DTYPES
TDT = A.TDT
EXTRA_COLS = A.EXTRA_COLS


def geometries(dtype: str):
    return GEOMETRIES + (BF16_ONLY if dtype == "bf16" else ())


ALL = tuple((H, dh, Do, dt) for dt in DTYPES for H, dh, Do in geometries(dt))

# max over rows of max_j |out - out64| / rowmax(out64), head-summed and per head.
# Measured on MI355X over ALL x both value layouts (the layout does not change a bit):
MEASURED_OUT = 5.098e-7           # H 32, dh 48, Do 1536, fp16, per head (head-summed: 2.531e-7, same geometry, bf16)
OUT_TOL = 4.0 * MEASURED_OUT


class Case:
    def __init__(self, H: int, dh: int, Do: int, dtype: str, kl=KEY_LENS, seed: int = 0):
        self.H, self.dh, self.Do, self.D, self.dtype = H, dh, Do, H * dh, dtype
        self.kl = tuple(kl)
        self.n_seq, self.tk, self.max_k = len(self.kl), sum(self.kl), max(self.kl)
        g = torch.Generator().manual_seed(7300 + 97 * H + dh + 13 * (Do // 32) + seed)
        dt = TDT[dtype]
        scale = torch.exp(0.8 * torch.randn(self.tk, 1, 1, generator=g))
        v = (0.8 * torch.randn(self.tk, 1, dh, generator=g) + 0.6 * torch.randn(self.tk, H, dh, generator=g)) * scale
        self.v16 = v.reshape(self.tk, self.D).to(dt)                     # compact [tk, D]
        self._other = torch.randn(self.tk, 2 * self.D, generator=g).to(dt)     # the Q and K thirds: never read
        shared = torch.randn(Do, dh, generator=g)
        mix = torch.eye(dh)[None] + 0.5 * torch.randn(H, dh, dh, generator=g) / math.sqrt(dh)
        gain = torch.exp(0.5 * torch.randn(H, 1, 1, generator=g))
        wo = (0.8 * torch.einsum("de,hef->hdf", shared, mix) + 0.6 * torch.randn(H, Do, dh, generator=g)) * gain
        self.wo16 = (wo.permute(1, 0, 2).reshape(Do, self.D) / math.sqrt(dh)).to(dt)          # [Do, H * dh]
        P = torch.zeros(self.n_seq, H, self.max_k, dtype=torch.float64)
        for s, n in enumerate(self.kl):
            if n:
                P[s, :, :n] = torch.softmax(2.0 * torch.randn(H, n, generator=g, dtype=torch.float64), dim=-1)
        self.P = P.float()                                               # fp32, exactly 0 past a sequence's keys
        self.cu_k = torch.tensor([0] + list(torch.tensor(self.kl).cumsum(0)), dtype=torch.int32)

    def v_buffer(self, layout: str) -> torch.Tensor:
        """The buffer whose LAST D columns are the value rows, as the attention kernel reads them: "qkv" = a [tokens, 3D]
        projection (V its [:, 2D:] third), "kv" = [tokens, 2D] (V its [:, D:] half), "compact" = [tokens, D]."""
        if layout == "compact":
            return self.v16
        return torch.cat([self._other if layout == "qkv" else self._other[:, :self.D], self.v16], dim=1)

    def valid(self) -> torch.Tensor:
        """bool [n_seq, max_k]: column j is a key of sequence s."""
        return torch.arange(self.max_k)[None, :] < torch.tensor(self.kl)[:, None]

    def key_probs(self) -> torch.Tensor:
        """float64 [tk, H]: P[s, h, j] of key t = cu_k[s] + j."""
        return torch.cat([self.P[s, :, :n].double().t() for s, n in enumerate(self.kl)], dim=0)

    def spread(self, x: torch.Tensor) -> torch.Tensor:
        """[n_seq, max_k] (or [n_seq, H, max_k]) from per-key values [tk] ([tk, H]), 0 past a sequence's keys."""
        out = torch.zeros((self.n_seq,) + tuple(x.shape[1:]) + (self.max_k,), dtype=x.dtype)
        k = 0
        for s, n in enumerate(self.kl):
            out[s, ..., :n] = x[k:k + n].movedim(0, -1)
            k += n
        return out


@functools.lru_cache(maxsize=None)
def case(H: int, dh: int, Do: int, dtype: str) -> Case:
    return Case(H, dh, Do, dtype)


def head_norms(c: Case) -> torch.Tensor:
    """float64 [tk, H]: ||Wo[:, h*dh:(h+1)*dh] @ v[t, h]||."""
    wo = c.wo16.double().view(c.Do, c.H, c.dh)
    v = c.v16.double().view(c.tk, c.H, c.dh)
    return torch.stack([(v[:, h] @ wo[:, h].t()).norm(dim=-1) for h in range(c.H)], dim=1)


def reference_of(c: Case) -> dict:
    """float64: n [n_seq, max_k], per_head [n_seq, H, max_k], both 0 past a sequence's keys -- from the vectors c themselves."""
    p = c.key_probs()                                                            # [tk, H]
    pv = (p[:, :, None] * c.v16.double().view(c.tk, c.H, c.dh)).reshape(c.tk, c.D)
    vec = pv @ c.wo16.double().t()                                               # c[t, :], [tk, Do]
    return {"n": c.spread(vec.norm(dim=-1)), "per_head": c.spread(p * head_norms(c))}


@functools.lru_cache(maxsize=None)
def reference(H: int, dh: int, Do: int, dtype: str) -> dict:
    return reference_of(case(H, dh, Do, dtype))


def wrong_quantities(H: int, dh: int, Do: int, dtype: str) -> dict:
    """What a plausible mistake computes instead of n, float64 [n_seq, max_k] each:
      diagonal   sqrt(sum_h P_h^2 ||Wo_h v_h||^2): the cross-head terms dropped;
      weight     P_mean * ||Wo v_t||: the head-mean map times the norm of the key's transformed value;
      no_wo      ||sum_h P_h v[t, h]||: the value-weighted norm without out_proj."""
    c = case(H, dh, Do, dtype)
    p, hn = c.key_probs(), head_norms(c)
    v = c.v16.double()
    return {"diagonal": c.spread(torch.sqrt((p * p * hn * hn).sum(dim=1))),
            "weight": c.spread(p.mean(dim=1) * (v @ c.wo16.double().t()).norm(dim=-1)),
            "no_wo": c.spread((p[:, :, None] * v.view(c.tk, H, dh)).sum(dim=1).norm(dim=-1))}


out_err = A.out_err
row_err = A.row_err


# ---- the oracle-side recorder (tests/test_gene_contribution_maps_gpu.py) ---------------------------------------------------------
def record_oracle_self_contributions(monkeypatch):
    """tests/attn_self_map_cases.py::record_oracle_self_maps with the value side: wraps O.mha_self (undone by `monkeypatch`) and,
    for every gene-layer call, recomputes q, K and V at the oracle's rounding point (the rounded Wqkv projection), reads
    out_proj.weight through rnd.r as tests/attn_contrib_cases.py::record_oracle_contributions does, and records per call
    `layer`, `mean` float64 [T, G] (the head-mean map of the registry token), `n` [T, G] (the norm of the contribution vectors,
    formed directly) and `per_head` [T, H, G] (P_h ||Wo_h v_h||)."""
    from oracle import vf_oracle as O
    from tests.attn_self_map_cases import LOG2E, _softmax2
    records = []
    original = O.mha_self

    def wrapped(x, sd, pfx, H, cu, slopes, rnd):
        if "gene_layers." in pfx:
            D = x.shape[-1]
            dh = D // H
            pre = rnd.q_prescale
            ws = 1.0
            if pre:
                ws = torch.ones(3 * D, 1)
                ws[:D] = LOG2E / math.sqrt(dh)
            qkv = rnd.r(O.linear(x, sd[pfx + "Wqkv.weight"], sd[pfx + "Wqkv.bias"], rnd, wscale=ws)).view(-1, 3, H, dh)
            wo = rnd.r(sd[pfx + "out_proj.weight"]).double().view(D, H, dh)
            c = 1.0 if pre else LOG2E / math.sqrt(dh)
            rec = {"layer": int(pfx.split("gene_layers.")[1].split(".")[0]), "mean": [], "n": [], "per_head": []}
            for b in range(len(cu) - 1):
                a, e = int(cu[b]), int(cu[b + 1])
                s2 = torch.einsum("hd,jhd->hj", qkv[a, 0].double(), qkv[a:e, 1].double()) * c
                if slopes is not None:
                    s2 = s2 - (slopes.double() * LOG2E)[:, None] * torch.arange(e - a, dtype=torch.float64)[None, :]
                p = _softmax2(s2)                                                       # [H, G]
                u = torch.einsum("dhe,jhe->jhd", wo, qkv[a:e, 2].double())               # [G, H, D]
                rec["mean"].append(p.mean(dim=0))
                rec["n"].append(torch.einsum("hj,jhd->jd", p, u).norm(dim=-1))
                rec["per_head"].append(p * u.norm(dim=-1).t())
            records.append({k: (torch.stack(v) if isinstance(v, list) else v) for k, v in rec.items()})
        return original(x, sd, pfx, H, cu, slopes, rnd)

    monkeypatch.setattr(O, "mha_self", wrapped)
    return records


def oracle_gene_contributions(monkeypatch, batch, sd, cre_hp, gene_hp, hp, rounding, layers=None):
    """{"mean", "n", "per_head"}: per gene float64 [len(layers), T_i, 1 + C_i] ([len(layers), T_i, H, 1 + C_i]) of the registry
    token's self attention, from one oracle forward with the given rounding mode (the conventions of
    tests/attn_self_map_cases.py::oracle_gene_body_maps)."""
    from oracle import vf_oracle as O
    from variantformer_amd.attn_maps import select_layers
    with monkeypatch.context() as mp:
        records = record_oracle_self_contributions(mp)
        O.predict_step(batch, sd, cre_hp, gene_hp, hp, rounding=rounding, share_cre_stream=True)
    n_layers, n_genes = hp.num_layers, len(batch["cre_sequences"])
    assert len(records) == n_genes * n_layers
    out = {kind: [] for kind in ("mean", "n", "per_head")}
    for i in range(n_genes):
        recs = records[i * n_layers:(i + 1) * n_layers]
        assert [r["layer"] for r in recs] == list(range(n_layers))
        for kind in out:
            out[kind].append(torch.stack([recs[l][kind] for l in select_layers(n_layers, layers)]).numpy())
    return out


# ---- the parallel write-set net: one case list for the entry of include/vf_hip_gene_contrib.h ----------------------------------
# tests/write_set_cases.py's machinery on vf_attn_contrib_self, beside tests/attn_contrib_cases.py's list for vf_hip_attn_contrib.h.
# tests/test_gene_contrib_cpu.py requires every stream-taking declaration of the header to be named here, entry and wrapper, head
# summed and per head; tests/test_attn_contrib_self_gpu.py runs the cases.  The wrapper cases read v through a row map into a
# table whose unnamed rows are poisoned (W.spread_rows); the entry cases read the [:, 2D:] third of a guarded [tokens, 3D] buffer.
WS_GEOMETRIES = ((4, 32, 96, "bf16"), (4, 32, 96, "fp16"), (2, 48, 96, "bf16"), (32, 48, 1536, "bf16"))


def _make_ws(H, dh, Do, dtype, per_head, wrapper):
    def make():
        from tests import write_set_cases as W
        c = case(H, dh, Do, dtype)
        ref = reference(H, dh, Do, dtype)
        n_out = c.n_seq * (H if per_head else 1)
        cols = c.max_k + EXTRA_COLS
        valid = c.valid()

        def run(p):
            from variantformer_amd import _lib
            ops = W._ops()
            wo = W.guarded(c.wo16, p, W.GUARD_COLS)
            probs = W.guarded(c.P.reshape(c.n_seq * H, c.max_k), p, W.GUARD_COLS)
            inval = (~valid)[:, None, :].expand(c.n_seq, H, c.max_k).reshape(c.n_seq * H, c.max_k).to(W.DEVICE)
            probs[inval] = W.poisoned((int(inval.sum()),), torch.float32, W.DEVICE, p)     # columns past a sequence's keys are not read
            cu_k = W.guarded(c.cu_k, p)
            big, out = W.arena(n_out, cols, torch.float32, p)
            if wrapper:
                tab, rows = W.spread_rows(c.v16, p, W.GUARD_COLS)
                v_rows = W.guarded(rows.to(torch.int64), p)
                with W.poison_allocations(p) as proxy:
                    ops.attn_contrib_self(tab, wo, probs, cu_k, c.max_k, H, dh, out=out, per_head=per_head, v_rows=v_rows)
                assert proxy.count == 0, "ops.attn_contrib_self allocates nothing: out and probs are the caller's"
            else:
                v = W.guarded(c.v_buffer("qkv"), p, W.GUARD_COLS)[:, 2 * c.D:]
                _lib.check(_lib.load().vf_attn_contrib_self(v.data_ptr(), v.stride(0), 0, wo.data_ptr(), wo.stride(0), probs.data_ptr(),
                                                            probs.stride(0), cu_k.data_ptr(), c.n_seq, c.max_k, H, dh, Do,
                                                            ops._dt(TDT[dtype]), int(per_head), out.data_ptr(), out.stride(0),
                                                            W._stream()), "vf_attn_contrib_self")
            assert ops.last_kernel("attn") == "attn_contrib_self_kernel"
            W._sync()
            return {"out": big}

        def check(bufs):
            body = bufs["out"][8:8 + n_out, W.GUARD_COLS:W.GUARD_COLS + c.max_k]
            if per_head:
                body = body.view(c.n_seq, H, c.max_k)
                assert bool((body[~valid[:, None, :].expand_as(body)] == 0).all())
                assert out_err(body, ref["per_head"]) <= OUT_TOL
            else:
                assert bool((body[~valid] == 0).all()), "columns past a sequence's keys are not zero"
                assert out_err(body, ref["n"]) <= OUT_TOL
        inner = torch.zeros((n_out, cols), dtype=torch.bool)
        inner[:, :c.max_k] = True           # every row is written, the sequence without keys as zeros; columns >= max_seqlen_k are not
        return W.Built(run, {"out": W.arena_mask(n_out, cols, inner)}, check)
    return make


def ws_cases() -> list:
    from tests import write_set_cases as W
    out = []
    for H, dh, Do, dtype in WS_GEOMETRIES:
        for per_head in (False, True):
            for wrapper in (False, True):
                out.append(W.WSCase(f"attn_contrib_self-H{H}-dh{dh}-Do{Do}-{dtype}-{'per_head' if per_head else 'summed'}-"
                                    f"{'wrapper' if wrapper else 'entry'}", "attn_contrib_self", ("vf_attn_contrib_self",),
                                    ("attn_contrib_self",) if wrapper else (), _make_ws(H, dh, Do, dtype, per_head, wrapper)))
    return out

"""The exact-arithmetic attention cases (tests/attn_exact_cases.py) checked on the CPU: the closed forms against the oracle,
the premises, the two fp32 identities, a tiled fp32 online softmax that must reproduce the closed form bit for bit, and the
sensitivity of the reference to the indexing errors the GPU screen is there to catch."""
import math

import numpy as np
import pytest
import torch

from oracle import vf_oracle as O
from tests import attn_exact_cases as X

IDS = lambda c: c.id          # noqa: E731


def test_scale_identity_in_fp32():
    """scale = float32(ln 2) times the kernels' fp32 log2(e) is exactly 1: P.scale_log2 == 1.0f without VF_ATTN_Q_LOG2.  Neither
    neighbouring float has the property."""
    s = X.LN2_F32
    assert float(s) == 0.6931471824645996
    assert np.float32(s * X.LOG2E_F32) == np.float32(1.0)
    for nb in (np.nextafter(s, np.float32(0)), np.nextafter(s, np.float32(1))):
        assert np.float32(nb * X.LOG2E_F32) != np.float32(1.0)
    # the fp32 product as the device forms it: one rounding of the exact product
    assert np.float32(np.float64(s) * np.float64(X.LOG2E_F32)) == np.float32(1.0)


def test_slope_identity_in_fp32():
    """slopes[h] = float32(ln 2) * 2^-k: the kernels' slope2 = slopes[h] * 1.4426950408889634f is exactly 2^-k."""
    for k in (0, 1, 2):
        slope = np.float32(X.LN2_F32 * np.float32(2.0 ** -k))
        assert np.float32(slope * X.LOG2E_F32) == np.float32(2.0 ** -k)
        assert np.float32(np.float64(slope) * np.float64(X.LOG2E_F32)) == np.float32(2.0 ** -k)


def test_case_table_reaches_every_instantiation():
    """Every kernel launch_attn can select, in q_log2 and plain-scale form, with and without the ALIBI code objects where the
    family has both, self and cross attention where it serves both; every padded class."""
    by = {}
    for c in X.FORWARD_CASES:
        by.setdefault(c.kernel, []).append(c)
    assert set(by) == set(X.KERNELS)
    for kern in (X.F64, X.F128, X.X32, X.X64, X.SHORT, X.S2_1, X.S2_2):
        cs = by[kern]
        assert {c.q_log2 for c in cs} == {True, False}, kern
        assert {c.k_lens is None for c in cs} == {True, False}, kern
        assert {c.order for c in cs} == {"random", "flagged_first"}, kern
    for kern in (X.F64, X.F128, X.SHORT, X.S2_1, X.S2_2, X.S2_2R):
        assert {"zero", "real"} <= {c.alibi for c in by[kern]}, kern
    for kern in (X.X32, X.X64):
        assert {c.off for c in by[kern]} == set(X.OFFSETS), kern
    assert {c.dh for c in X.FORWARD_CASES} >= {24, 40, 56, 80, 104, 136, 200, 32, 48, 64, 96, 128}
    assert any(c.q_at_start and max(c.q_lens) == 1 for c in X.FORWARD_CASES)
    # lengths: the edges inside the family's range, the maximum, an empty key sequence and an empty query sequence
    for c in X.FORWARD_CASES:
        kl = c.k_lens if c.k_lens is not None else c.q_lens
        assert 0 in kl and 0 in c.q_lens, c.name
        for lens in (kl, c.q_lens):
            top = max(lens)
            if top > 1:
                assert set(X.edges(1, top)) <= set(lens), c.name


def _sample_rows(b, s, rng, n_rand=6):
    lq = b.q_lens[s]
    if lq == 0:
        return np.zeros(0, np.int64)
    return np.unique(np.concatenate([[0, lq - 1], rng.integers(0, lq, n_rand)]))


@pytest.mark.parametrize("case", X.FORWARD_CASES, ids=IDS)
def test_closed_form_equals_oracle(case):
    """The closed form against oracle.vf_oracle.attention on the same operands (q_log2 as in the case), for the first, the last
    and six seeded rows of every sequence against ALL its keys (a row's expected value depends on the row only through the
    pattern it selects per head; with a real bias: the compared rows).  The oracle has no scale argument: without q_log2 its
    1 / sqrt(dh) is cancelled on q in fp32.  Tolerance = the oracle's fp32 rounding: its logits carry ~1e-5 absolute error at
    |off| = 200 (1.4e-4 where a bias of up to 256 cancels against q . k), its exponentials that much relative error; half a unit
    of the numerator, the smallest indexing error, is 1 / (4 L) >= 1e-4 absolute and >= 0.5 % of any non-zero value."""
    b = X.built(case)
    for dtype in case.dtypes:
        X.assert_premises(b, dtype)
    assert b.max_num < X.NUM_LIMIT
    H, dh = case.H, case.dh
    rng = np.random.default_rng(5)
    rnd = O.Rounding("bf16")
    real = case.alibi == "real"
    rtol = 2e-3 if real else 2e-4
    worst = 0.0
    for s in range(len(b.q_lens)):
        lq, n = b.q_lens[s], b.k_lens[s]
        qa, ka = int(b.cu_q[s]), int(b.cu_k[s])
        if lq == 0:
            continue
        if n == 0:
            assert float(b.expected[qa:qa + lq].abs().max()) == 0.0
            continue
        rows = np.arange(lq) if real else _sample_rows(b, s, rng)
        q = b.q[qa:qa + lq][rows].view(-1, H, dh)
        if not case.q_log2:
            q = q * np.float32(float(X.LN2_F32) * math.sqrt(dh))
        got = O.attention(q, b.k[ka:ka + n].view(n, H, dh), b.v[ka:ka + n].view(n, H, dh), b.slopes, rnd, q_log2=case.q_log2,
                          q_at_start=case.q_at_start).reshape(len(rows), H * dh)
        want = b.expected[qa:qa + lq][rows]
        keep = b.compare[qa:qa + lq][rows]
        assert bool(keep.any())
        err = (got[keep] - want[keep]).abs() - rtol * want[keep].abs()
        worst = max(worst, float(err.max()))
    assert worst <= 4e-6, f"{case.name}: closed form and oracle differ by {worst:.3e} beyond rtol {rtol}"


EMU_LENS = (1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 200, 201, 255, 256, 257, 300, 603, 1000, 1024, 1300, 0)


@pytest.mark.parametrize("order", ["random", "flagged_first"])
@pytest.mark.parametrize("off", X.OFFSETS)
def test_tiled_fp32_online_softmax_is_bit_equal_to_closed_form(order, off):
    """An fp32 online softmax in 32-key and in 64-key tiles (running maximum, rescaling by exp2(m - m_new), o * (1 / l)) gives the
    closed form bit for bit -- in fp32 already, before any rounding to 16 bits -- in random key order and with all flagged keys
    first (the maximum then rises in a later tile and the accumulators are rescaled by exactly 2)."""
    case = X.FwdCase(f"emu_{order}_{off}", "", 32, 3, tuple(min(n, 8) + (n == 0) for n in EMU_LENS), EMU_LENS, off=off,
                     order=order, seed=900)
    b = X.build(case)
    for tile in (32, 64):
        rows, out = X.emulate_tiled(b, tile)
        assert rows.numel() == b.q.shape[0]
        assert torch.equal(out.view(torch.int32), b.expected[rows].view(torch.int32)), f"tile {tile}"


SENS_KEYS = 6
SENS_SKIP_CAP = 0.01     # share of sampled keys whose V rows are zero in every head (probability (7/8)^(H dh) <= 2e-4 each)


@pytest.mark.parametrize("case", X.FORWARD_CASES, ids=IDS)
def test_reference_is_sensitive_to_indexing_errors(case):
    """On the reference alone: for 2 * SENS_KEYS seeded keys of every case (half drawn uniformly, half among the keys that carry a
    flag in some head, preferring a key whose successor's flag differs), removing the key, duplicating it, swapping its V row with
    the next key's and flipping its flag each change at least one bit of the expected output of its sequence (both patterns of
    every head, rounded to the operand type).  A key whose V rows are zero in every head is skipped (share capped at
    SENS_SKIP_CAP; none occurs with these seeds).  Swapping two V rows is visible only where the two keys' weights differ in a
    head in which their V rows differ -- attention is symmetric under a permutation of equal-weight keys -- so the swap is
    asserted under that precondition, which is computed from the operands, never from the output (it holds for about half of
    the sampled keys, and for at least one in every case)."""
    b = X.built(case)
    rng = np.random.default_rng(31 + case.seed)
    cand = [s for s in range(len(b.k_lens)) if b.k_lens[s] >= 2 and b.q_lens[s] > 0]
    p = np.asarray([b.k_lens[s] for s in cand], np.float64)
    skipped = swaps = 0
    sample = []
    for i in range(2 * SENS_KEYS):
        s = cand[int(rng.choice(len(cand), p=p / p.sum()))]
        j = int(rng.integers(0, b.k_lens[s]))
        if i >= SENS_KEYS and b.flags[s].any():          # the second half: keys that carry a flag in some (head, pattern)
            h, pat = int(rng.integers(0, case.H)), int(rng.integers(0, 2))
            f = b.flags[s][:, h, pat]
            nxt = np.append(f[1:], f[-2])                     # the flag of the key its V row would be swapped with
            edge = np.nonzero(f != nxt)[0]                    # (with all flagged keys first: the ends of the flagged run)
            j = int(rng.choice(edge if edge.size else np.nonzero(f)[0]))
        sample.append((s, j))
    for s, j in sample:
        n, ka = b.k_lens[s], int(b.cu_k[s])
        V, B = b.V_int[ka:ka + n].astype(np.int64), b.flags[s]
        if not V[j].any():
            skipped += 1
            continue
        j2 = j + 1 if j + 1 < n else j - 1
        keep = np.arange(n) != j
        Vs = V.copy()
        Vs[[j, j2]] = V[[j2, j]]
        Bf = B.copy()
        Bf[j] ^= 1
        variants = {"removed": (V[keep], B[keep]), "duplicated": (np.insert(V, j, V[j], axis=0), np.insert(B, j, B[j], axis=0)),
                    "flag flipped": (V, Bf)}
        # weights differ in (head, pattern) and the V rows differ in that head
        if ((B[j] != B[j2]).any(axis=1) & (V[j] != V[j2]).any(axis=1)).any():
            variants["V rows swapped"] = (Vs, B)
            swaps += 1
        for dtype in case.dtypes:
            base = X.rounded_table(V, B, dtype)
            for what, (Vp, Bp) in variants.items():
                assert not torch.equal(X.rounded_table(Vp, Bp, dtype).view(torch.int16), base.view(torch.int16)), \
                    f"{case.name}: key {j} of sequence {s} ({n} keys) {what}: no bit of the expected output moves ({dtype})"
    assert skipped <= SENS_SKIP_CAP * len(sample), f"{skipped} of {len(sample)} sampled keys have all-zero V rows"
    assert swaps >= 1, "no sampled key tests the V-row swap"


@pytest.mark.parametrize("case", X.PROBS_CASES, ids=IDS)
def test_probs_closed_form_equals_float64_softmax(case):
    """P = 2^-b_j / L and (m, l) = (off, L) against a float64 softmax of the same operands' base-2 logits (with the bias where
    the case has one), every selected row."""
    b = X.build_probs(case)
    for dtype in ("bf16", "fp16"):
        X.assert_premises(b, dtype)
    H, dh = case.H, case.dh
    c = 1.0 if case.q_log2 else float(np.float32(X.LN2_F32 * X.LOG2E_F32))
    assert c == 1.0
    slope2 = None if b.slopes is None else (b.slopes.numpy() * X.LOG2E_F32).astype(np.float64)
    for s in range(len(b.k_lens)):
        n, ka = b.k_lens[s], int(b.cu_k[s])
        for o in range(int(b.cu_rows[s]), int(b.cu_rows[s + 1])):
            if n == 0:
                assert float(b.P[o].abs().max()) == 0.0 and float(b.stats[o].abs().max()) == 0.0
                continue
            q = b.q[int(b.sel[o])].view(H, dh).double()
            s2 = torch.einsum("hd,nhd->hn", q, b.k[ka:ka + n].view(n, H, dh).double())
            if slope2 is not None:
                pos = 0 if b.q_pos is None else int(b.q_pos[o])
                s2 = s2 - torch.from_numpy(slope2)[:, None] * (pos - torch.arange(n)).abs().double()[None, :]
            m = s2.max(dim=-1).values
            p = torch.exp2(s2 - m[:, None])
            assert torch.equal(m, b.stats[o, :, 0].double()) and torch.equal(p.sum(dim=-1), b.stats[o, :, 1].double())
            assert torch.equal(p / p.sum(dim=-1, keepdim=True), b.P[o, :, :n]) and float(b.P[o, :, n:].abs().sum()) == 0.0


@pytest.mark.parametrize("case", X.COUNTED_CASES, ids=IDS)
def test_counted_closed_form_equals_oracle(case):
    """The counted-keys closed form against oracle.attention_counted (counts 2^log2_count over the rows a sequence holds), every
    row; launch_counted_keys' q_per_block for the case's batch is the one the case names."""
    b = X.build_counted(case)
    for dtype in ("bf16", "fp16"):
        X.assert_premises(b, dtype)
    assert X.counted_q_per_block(len(case.lens), b.max_q) == case.q_per_block
    C, H, dh = case.C, case.H, case.dh
    D = H * dh
    assert any((n * H) % 256 for n in case.lens if n), "len * H must not always be a multiple of the block size"
    for s in range(len(case.lens)):
        a, n = int(b.cu[s]), case.lens[s]
        if n == 0:
            continue
        lc = b.log2_count[s]
        present = torch.nonzero(torch.isfinite(lc))[:, 0]
        assert present.numel() >= 1 and set(lc[present].tolist()) <= {0.0, 1.0, 2.0}
        got = O.attention_counted(b.q[a:a + n].view(n, H, dh), b.kv[present, :D].view(-1, H, dh), b.kv[present, D:].view(-1, H, dh),
                                  torch.exp2(lc[present]), True).reshape(n, D)
        np.testing.assert_allclose(got.numpy(), b.expected[a:a + n].numpy(), rtol=1e-5, atol=1e-6)
    if C > 1:
        assert bool(torch.isinf(b.log2_count).any()), "no absent row in the case"


@pytest.mark.parametrize("case", X.SOFTMAX_CASES, ids=IDS)
def test_softmax_counted_closed_form_equals_float64_softmax(case):
    b = X.build_softmax(case)
    C, Cp, H = case.C, case.Cp, case.H
    T = b.scores.shape[0]
    sc = b.scores.view(T, H, Cp).double()
    want = torch.zeros(T, H, Cp, dtype=torch.float64)
    for s in range(len(case.lens)):
        a, e = int(b.cu[s]), int(b.cu[s + 1])
        if e > a:
            t = sc[a:e, :, :C] + b.log2_count[s].double()[None, None, :]
            p = torch.exp2(t - t.max(dim=-1, keepdim=True).values)
            want[a:e, :, :C] = p / p.sum(dim=-1, keepdim=True)
    assert torch.equal(want, b.expected.view(T, H, Cp).double())
    # the weights are powers of two (or zero): one bit pattern in either 16-bit type
    nz = want[want > 0]
    assert torch.equal(torch.exp2(torch.log2(nz).round()), nz)

/* vf_hip_attn_contrib.h -- the entry of libvf_hip.so behind the cCRE contribution maps.
 *
 * tests/write_set_cases.py holds one poisoned-memory case for every stream-taking declaration of vf_hip.h.  This entry is
 * declared here instead, bound through _lib.ENTRIES["vf_hip_attn_contrib.h"] (tests/test_abi_cpu.py holds every header to its
 * table), and covered by a parallel net of
 * its own (tests/attn_contrib_cases.py, tests/test_attn_contrib_cpu.py: every stream-taking declaration of THIS header has a
 * write-set case there).  Everything the main
 * header says holds here: the conventions at its top (device pointers owned by the caller, `stream` a hipStream_t, strides in
 * elements, 0 = ok / VF_ERR_*, vf_last_error()), the comment contract of every entry (arguments, write set, non-finite operands,
 * refusals), and VF_ABI_VERSION: a new symbol changes no existing one, so the version stays 13.
 */
#ifndef VF_HIP_ATTN_CONTRIB_H
#define VF_HIP_ATTN_CONTRIB_H

#include "vf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Value-weighted NORMS beside the attention maps (added under ABI 13): how much of key j reaches selected row r through the
 * cross attention's out_proj, not merely how much the row looked at it (Kobayashi et al. 2020, "Attention is not only a weight").
 * No reference counterpart: flash-attn [3p] keeps P in registers and out_proj (seq2gene/modules/layers.py:344-351) mixes the
 * heads in a GEMM; exists for the cCRE contribution maps.
 *   c[r, j] = sum_h P[r, h, j] * Wo[:, h*dh:(h+1)*dh] @ v[j, h, :]     (out_proj(attention)[r] = sum_j c[r, j] + bias; the bias
 *   belongs to no key and is left out),   n[r, j] = ||c[r, j]||_2, computed in Gram form without forming c:
 *     G[j, h, h'] = v[j, h, :]^T S[h, h'] v[j, h', :],      S[h, h', e, e'] = sum_d Wo[d, h*dh + e] * Wo[d, h'*dh + e']
 *     n[r, j]     = sqrt( sum_h P[r, h, j] * ( sum_h' G[j, h, h'] * P[r, h', j] ) ),   h and h' ascending, fp32 fma.
 *   v       16-bit [cu_seqlens_k[n_seq], >= H * dh] (operand_dtype VF_BF16 / VF_F16), heads packed (head, dh), rows v_stride
 *           elements apart: the value rows the attention kernel reads;
 *   s_gram  fp32 [H, H, dh, dh] = S, built by the caller once per weights;
 *   probs   fp32 [R * H, ldp]: P[r, h, j] at probs[(r * H + h) * ldp + j], as vf_attn_probs writes it with per_head = 1;
 *   cu_rows, cu_seqlens_k, n_seq, max_rows, max_seqlen_k: the row grouping of vf_attn_probs, exactly;
 *   gram    fp32 [cu_seqlens_k[n_seq], H, H], an OUTPUT: G of every key of every sequence, in full (both triangles; G[j, h', h]
 *           holds the bits of G[j, h, h']);
 *   per_head == 0: out[r * ldo + j] = n[r, j];
 *   per_head == 1: out[(r * H + h) * ldo + j] = P[r, h, j] * sqrt(G[j, h, h]), the norm of head h's own contribution.
 *   Columns len_k(s) <= j < max_seqlen_k of a written row are 0, columns >= max_seqlen_k are not touched, rows at or past
 *   R = cu_rows[n_seq] are not touched.  A sequence without selected rows writes no `out` row; its keys' gram rows are written.
 * fp32 throughout after the 16-bit loads of v (the exact fp32 MFMA for G, fp32 fma for n); no atomics; 64-bit row offsets; the
 * bits of n[r, j] depend on row r's P, key j's value row and S alone, not on the rest of the call, max_rows or max_seqlen_k.
 * A negative radicand (rounding) gives 0 through a comparison, so a NaN stays a NaN.  Non-finite operands: a NaN
 * in value row (j, h) makes column j of that sequence's rows NaN (per_head: of head h's rows) and no other column; a NaN in a
 * probs row makes that row NaN (per_head: that head's row); a NaN in s_gram may reach everything.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): dh outside
 * {32, 48, 64, 96, 128}; H outside 1 .. 32 (the norm kernel holds a row's H probabilities in registers); a null pointer;
 * ldo or ldp below max_seqlen_k; v_stride < H * dh; v not 16-byte aligned or v_stride not a multiple of 8; s_gram not 16-byte
 * aligned, probs / gram / out not 4-byte aligned; a bad dtype; n_seq, max_rows or max_seqlen_k < 0; n_seq > 65 535 or
 * max_rows > 64 * 65 535 (vf_attn_probs's limits) or ceil(n_seq * max_seqlen_k / 512) * H (H + 1) / 2 >= 2^31 (the Gram grid).
 * n_seq == 0 or max_rows == 0 is VF_OK with nothing launched.  vf_last_kernel(1) is "attn_contrib_kernel" afterwards. */
int vf_attn_contrib(const void* v, int64_t v_stride, const float* s_gram, const float* probs, int64_t ldp,
                    const int32_t* cu_rows, const int32_t* cu_seqlens_k, int n_seq, int max_rows, int max_seqlen_k,
                    int H, int dh, int operand_dtype, int per_head, float* gram, float* out, int64_t ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_ATTN_CONTRIB_H */

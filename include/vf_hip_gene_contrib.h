/* vf_hip_gene_contrib.h -- the entry of libvf_hip.so behind the gene-body contribution maps.
 *
 * tests/write_set_cases.py holds one poisoned-memory case for every stream-taking declaration of vf_hip.h;
 * tests/test_attn_contrib_cpu.py holds vf_hip_attn_contrib.h to exactly its one name.  This entry is declared here instead, bound
 * through _lib.ENTRIES["vf_hip_gene_contrib.h"] (tests/test_abi_cpu.py holds every header to its table), and covered by a parallel
 * net of its own (tests/gene_contrib_cases.py,
 * tests/test_gene_contrib_cpu.py: every stream-taking declaration of THIS header has a write-set case there).  Everything the
 * main header says holds here: the conventions at
 * its top (device pointers owned by the caller, `stream` a hipStream_t, strides in elements, 0 = ok / VF_ERR_*,
 * vf_last_error()), the comment contract of every entry (arguments, write set, non-finite operands, refusals), and
 * VF_ABI_VERSION: a new symbol changes no existing one, so the version stays 13.
 */
#ifndef VF_HIP_GENE_CONTRIB_H
#define VF_HIP_GENE_CONTRIB_H

#include "vf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Value-weighted NORMS beside the gene-body SELF attention maps (added under ABI 13): how much of key j of sequence s reaches
 * the sequence's one selected row (the registry token) through the self attention's out_proj (Kobayashi et al. 2020).  The
 * direct form of vf_attn_contrib's quantity: in a self attention every key belongs to one selected row, so a per-key Gram
 * matrix is shared by nobody; the vectors c are formed tile by tile on the 16-bit MFMA instead and never stored.  No reference
 * counterpart (flash-attn [3p] keeps P in registers; seq2gene/modules/layers.py:344-351 mixes the heads in a GEMM); exists for
 * the gene-body contribution maps.  With t = cu_seqlens_k[s] + j:
 *   c[s, j, :] = sum_h P[s, h, j] * Wo[:, h*dh:(h+1)*dh] @ v[t, h, :]
 *   per_head == 0: out[s * ldo + j]           = ||c[s, j, :]||_2
 *   per_head == 1: out[(s * H + h) * ldo + j] = P[s, h, j] * ||Wo[:, h*dh:(h+1)*dh] @ v[t, h, :]||_2
 *   v       16-bit [*, >= H * dh] (operand_dtype VF_BF16 / VF_F16), heads packed (head, dh), rows v_stride elements apart: the
 *           value rows the attention kernel reads (the [:, 2D:] third of a [tokens, 3D] projection, the [:, D:] half of 2D);
 *   v_rows  int64 [cu_seqlens_k[n_seq]] or NULL: key t is row v_rows[t] of v (a table of distinct projected rows); the result
 *           is the bits of the call on the gathered rows.  NULL: key t is row t;
 *   wo      16-bit [Do, >= H * dh], rows ldw elements apart, the type of v: out_proj's weight as the GEMM multiplies it;
 *   probs   fp32 [n_seq * H, ldp]: P[s, h, j] at probs[(s * H + h) * ldp + j], as vf_attn_probs_v2 writes it with per_head = 1
 *           and one selected row per sequence; columns at or past len_k(s) are not read;
 *   cu_seqlens_k int32 [n_seq + 1]; max_seqlen_k >= every len_k(s) (keys past it are not computed).
 *   Columns len_k(s) <= j < max_seqlen_k of a written row are 0, columns >= max_seqlen_k are not touched; a sequence without
 *   keys writes a row (per_head: H rows) of zeros.  No workspace: the squared norm is summed inside the block.
 * Arithmetic: keys on the MFMA's N dimension; per head and 32-row tile of Wo, dh / 16 v_mfma_f32_32x32x16 into a zeroed tile (the
 * exact fp32 product of the 16-bit operands), then one fp32 fma per register with the lane's own P[s, h, j] -- P * v is never
 * rounded to 16 bits.  The squared norm is summed over registers, Wo tiles (ascending) and the two lane halves in a fixed order;
 * no atomics; 64-bit row offsets.  The bits of out[s, j] depend on P[s, :, j], value row t and wo alone: not on the rest of the
 * call, on max_seqlen_k or on ldo.  Non-finite operands: a NaN in value row (t, h) makes column j of row s NaN
 * (per_head: of head h's row) and no other element; a NaN at P[s, h, j] makes out[s, j] NaN (per_head: out[s, h, j]) and no other
 * element; a NaN in wo may reach everything.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): dh outside
 * {32, 48, 64, 96, 128}; Do not a positive multiple of 32; H outside 1 .. 1024 (H * dh stays a 32-bit column offset); a null
 * pointer other than v_rows; ldo or ldp below max_seqlen_k; v_stride or ldw below H * dh or not a multiple of 8; v or wo not
 * 16-byte aligned; v_rows not 8-byte aligned; probs / out / cu_seqlens_k not 4-byte aligned; a bad dtype; n_seq or max_seqlen_k
 * < 0; n_seq * ceil(max_seqlen_k / 256) >= 2^31 (the grid: one block per sequence and 256-key tile).
 * n_seq == 0 or max_seqlen_k == 0 is VF_OK with nothing launched.  vf_last_kernel(1) is "attn_contrib_self_kernel" afterwards. */
int vf_attn_contrib_self(const void* v, int64_t v_stride, const int64_t* v_rows, const void* wo, int64_t ldw,
                         const float* probs, int64_t ldp, const int32_t* cu_seqlens_k, int n_seq, int max_seqlen_k,
                         int H, int dh, int Do, int operand_dtype, int per_head, float* out, int64_t ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_GENE_CONTRIB_H */

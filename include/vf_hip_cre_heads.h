/* vf_hip_cre_heads.h -- the entry of libvf_hip.so behind the tokenizer's per-tissue classifier heads (cCRE activity classes).
 *
 * One of six headers of the one library, beside vf_hip.h, vf_hip_attn_contrib.h, vf_hip_gene_contrib.h, vf_hip_forest.h and vf_hip_topk.h.  Its entry is bound
 * through _lib.ENTRIES["vf_hip_cre_heads.h"], which _lib.load() applies like the other five tables, and every stream-taking declaration here has
 * poisoned-memory write-set cases in tests/cre_heads_cases.py.  Everything the main header says holds here: the conventions at
 * its top (device pointers owned by the caller, `stream` a hipStream_t, strides in elements, 0 = ok / VF_ERR_*,
 * vf_last_error()), the comment contract of every entry (arguments, write set, non-finite operands, refusals), and
 * VF_ABI_VERSION: a new symbol changes no existing one, so the version stays 13.
 */
#ifndef VF_HIP_CRE_HEADS_H
#define VF_HIP_CRE_HEADS_H

#include "vf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tokenizer's per-tissue classifier heads on pooled window embeddings (added under ABI 13): the strands of a sample are
 * aggregated and the result goes through the nn.Linear of a tissue (reference seq2reg/model.py:274-302, which loops over
 * torch.unique(tissue_vector) with one GEMM per tissue).  All operands fp32: the pooled embeddings leave the encoder in fp32
 * and the reference runs the heads in fp32.
 *   x        fp32 [B * n_strands, >= d], rows ldx elements apart: pooled window embeddings, the strands of sample b adjacent
 *            (row b * n_strands + s is strand s of sample b);
 *   w        fp32 [n_tissues, C, F] contiguous, F = d (strand_agg 0 = mean) or n_strands * d (strand_agg 1 = concat): the heads'
 *            weights stacked by tissue; bias fp32 [n_tissues, C] contiguous;
 *   row form (tissue_of_row != NULL, int64 [B]; tissues must be NULL, n_sel is ignored): sample b goes through the head of ITS
 *            tissue t = tissue_of_row[b]:                        out[b * ldo + c]         = value(b, t, c)
 *   all form (tissue_of_row == NULL, tissues int32 [n_sel]): every sample goes through the heads tissues[0 .. n_sel-1], which may
 *            repeat and come in any order:                       out[b * ldo + i * C + c] = value(b, tissues[i], c)
 *   mode 0: value = logit;  mode 1: value = the probability, softmax over the C classes of (b, t) in fp32, the row maximum
 *            subtracted:  p[c] = exp(logit[c] - max) / sum_c' exp(logit[c'] - max);
 *   argmax   int32 [B] (row form) / [B, n_sel] contiguous (all form), or NULL: the first index of the largest logit of (b, t)
 *            (the same in both modes); -1 where any logit of that (b, t) is NaN.
 * Write set: out[b * ldo + 0 .. C-1] (row form) or out[b * ldo + 0 .. n_sel*C-1] (all form) for 0 <= b < B, and argmax if
 * given.  Columns of out at or past C (n_sel * C) are not touched; x, w, bias and the index arrays are only read.
 * Tissue ids lie in 0 .. n_tissues-1.  An id outside that range, in either index array, reads nothing: its C values are NaN
 * and its argmax is -1, every other (b, t) is as without it.  (`tissues` is a short list the caller can check on the host
 * before it uploads it; the Python wrapper reads back the minimum and maximum of ids it is not told were checked, and raises
 * KeyError.)
 * Arithmetic, per (b, t, c), all in fp32 and in this order:
 *   mean:   xbar[k] = (x[b,0,k] + x[b,1,k] + ... + x[b,ns-1,k]) / ns, added in ascending strand order, one IEEE division;
 *   concat: xbar[s * d + k] = x[b,s,k];
 *   acc = 0;  for f = 0 .. F-1 ascending: acc = fma(xbar[f], w[t,c,f], acc) (one v_fma_f32 per term: the product is not
 *   rounded);  logit = acc + bias[t,c].
 * A group of Cp adjacent lanes per (b, t), Cp the power of two at or above C (64 / Cp pairs per wave), lane c of the group owns
 * class c, so the maximum, the sum of the exponentials (a Cp-lane butterfly) and the argmax are taken inside the group in an
 * order fixed by C alone; no atomics, no workspace, no LDS; every row offset is 64-bit.  The bits of
 * value(b, t, :) and argmax(b, t) depend on the strand rows of sample b and on w[t], bias[t] alone: not on B, n_sel, ldo, ldx, the
 * other samples or tissues, the position of b in the call, or on which of the two forms was called.
 * Non-finite operands: a NaN in a strand row of sample b makes every value of sample b NaN and its argmax -1,
 * and reaches no other sample; a NaN in w[t,c,:] or bias[t,c] makes logit (., t, c) NaN and the argmax of every (., t) -1 -- in
 * mode 1 all C probabilities of tissue t are NaN -- and reaches no other tissue.  Inf follows IEEE term by term: Inf * 0 = NaN
 * for that logit only, Inf - Inf = NaN; in mode 1 a row whose maximum is +Inf, or whose logits are all -Inf, is NaN (exp(Inf -
 * Inf)), as torch.softmax makes it.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): d not a positive multiple of
 * 4; C outside 1 .. 64; n_strands outside 1 .. 8; n_tissues < 1; strand_agg or mode outside {0, 1}; ldx below d or not a
 * multiple of 4; ldo below C (row form) or n_sel * C (all form); a null x, w, bias or out; x or w not 16-byte aligned;
 * tissue_of_row not 8-byte aligned; bias / out / tissues / argmax not 4-byte aligned; both or neither of tissue_of_row and
 * tissues given; B < 0; n_sel < 0 (all form); ceil(B * n_sel / 4) >= 2^31 (the grid: at least four (b, t) pairs per block; n_sel =
 * 1 in the row form).  B == 0, or n_sel == 0 in the all form, is VF_OK with nothing launched. */
int vf_tissue_heads(const float* x, int64_t ldx, int n_strands, int strand_agg, const float* w, const float* bias,
                    int n_tissues, int C, int d, const int64_t* tissue_of_row, const int32_t* tissues, int n_sel, int64_t B,
                    int mode, float* out, int64_t ldo, int32_t* argmax, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_CRE_HEADS_H */

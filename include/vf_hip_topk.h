/* vf_hip_topk.h -- the entry of libvf_hip.so behind the ranked cCREs: the k largest values of every row of an attention or
 * contribution map, with their columns, selected on the device.
 *
 * One of six headers of the one library, beside vf_hip.h, vf_hip_attn_contrib.h, vf_hip_gene_contrib.h, vf_hip_cre_heads.h and
 * vf_hip_forest.h.  Its entry is bound through _lib.ENTRIES["vf_hip_topk.h"], which _lib.load() applies like the other five tables, and
 * tests/topk_cases.py holds its reference and case table (every comparison bit for bit, on poisoned and guarded buffers).
 * Everything the main header says holds here: the conventions at its top (device pointers owned by the caller, `stream` a
 * hipStream_t, strides in elements, 0 = ok / VF_ERR_*, vf_last_error()), the comment contract of every entry (arguments, write
 * set, arithmetic, non-finite operands, refusals), and VF_ABI_VERSION: a new symbol changes no existing one, so the version
 * stays 13.
 */
#ifndef VF_HIP_TOPK_H
#define VF_HIP_TOPK_H

#include "vf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* limits of vf_topk_rows: a row's 32-bit keys fit 64 KB of LDS; one lane of the row's wave holds one rank */
#define VF_TOPK_MAX_N 16384
#define VF_TOPK_MAX_K 64

/* The k first-ranked values of every row, with their columns (added under ABI 13): what a user takes from an attention or a
 * contribution map is a ranking, and this leaves k values and k indices per row to copy to the host instead of the row.
 * Arguments:
 *   x        fp32 [R, >= n], rows ldx elements apart (64-bit row offsets);
 *   n        the columns a row can have;  row_len  NULL, or int32 [R]: len(r) = n when row_len is NULL, else
 *            min(max(row_len[r], 0), n).  Columns at or past len(r) are never read;
 *   k        how many ranks are written per row;
 *   values   fp32 [R, >= k] and indices int32 [R, >= k], rows of both ldo elements apart.
 * Order: a ranks before b iff a is NaN and b is not, or neither is NaN and a > b by IEEE comparison (so +0 and -0 tie, and
 * every NaN ties with every other whatever its sign or payload); among ties the lower column comes first.  This is
 * torch.topk's order with the tie rule defined.
 * Write set: for 0 <= r < R and 0 <= i < k, indices[r * ldo + i] = the column of rank i and values[r * ldo + i] = the bits of
 * x[r, that column], copied (a NaN keeps its payload, -0 stays -0); for i >= len(r) the index is -1 and the value +0.0f.
 * Columns of the outputs at or past k and rows at or past R are not touched; x and row_len are only read.
 * Arithmetic: none; comparisons alone.  Every value becomes a 32-bit key whose unsigned order is the order above (sign bit
 * flipped for a non-negative value, all bits for a negative one, -0 folded onto +0 first, every NaN mapped to the one key
 * above +Inf), paired with VF_TOPK_MAX_N - column so that all pairs of a row are distinct; rank i is the largest pair below
 * rank i - 1's.  One block of 64 threads (one wave) per row: the keys are staged in len(r) * 4 bytes of LDS once, every round
 * is a per-lane scan and the xor butterfly 32, 16, 8, 4, 2, 1, and a row that runs out of columns stops early; the values are
 * read again from x at the selected columns.  No atomics, no workspace.  The outputs of row r depend on its first len(r)
 * values alone: not on R, ldx, ldo, the row's position or the other rows, and rank i does not depend on k (the result for k
 * is the beginning of the result for any k' > k).
 * Non-finite operands: NaNs rank first, in column order, and are returned with their bits; +Inf ranks above
 * every finite value and -Inf below; nothing is added or multiplied, so no operand reaches a rank it does not hold.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null x, values or
 * indices; x, row_len, values or indices not 4-byte aligned; n outside 0 .. 16384; k outside 1 .. 64; ldx < n; ldo < k;
 * R < 0; R >= 2^31 (the grid: one block per row).  R == 0 is VF_OK with nothing launched; so is n == 0 as far as reading
 * goes: with R > 0 every entry of the write set is then the -1 / +0.0f padding. */
int vf_topk_rows(const float* x, int64_t ldx, int64_t R, int n, const int32_t* row_len, int k, float* values, int32_t* indices,
                 int64_t ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_TOPK_H */

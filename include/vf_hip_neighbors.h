/* vf_hip_neighbors.h -- the entries of libvf_hip.so behind the expression and embedding neighbours: rows standardised on the
 * device, the k most similar rows of one matrix for every row of another (a correlation / cosine k-nearest-neighbour search
 * with no rows x rows buffer), and the dense similarity or distance matrix where it is small enough to exist.
 *
 * One of seven headers of the one library, beside vf_hip.h, vf_hip_attn_contrib.h, vf_hip_gene_contrib.h, vf_hip_cre_heads.h,
 * vf_hip_forest.h and vf_hip_topk.h.  Its entries are bound through _lib.ENTRIES["vf_hip_neighbors.h"], which _lib.load() applies like
 * the other six tables, and tests/neighbors_cases.py holds their references and case table.  Everything the main header says
 * holds here: the conventions at its top (device pointers owned by the caller, `stream` a hipStream_t, strides in elements,
 * 0 = ok / VF_ERR_*, vf_last_error()), the comment contract of every entry (arguments, write set, arithmetic, non-finite
 * operands, refusals), and VF_ABI_VERSION: a new symbol changes no existing one, so the version stays 13.
 *
 * The similarity of two rows, everywhere in this header:
 *   s(r, j) = fmaf(q[r, d-1], y[j, d-1], ... fmaf(q[r, 1], y[j, 1], fmaf(q[r, 0], y[j, 0], +0.0f)) ...)
 * one fp32 chain over the columns in ascending order, one rounding per column, one accumulator per (r, j): what the f32-input
 * MFMA (v_mfma_f32_32x32x2_f32) computes.  Its bits depend on the two rows and d alone.
 */
#ifndef VF_HIP_NEIGHBORS_H
#define VF_HIP_NEIGHBORS_H

#include "vf_hip.h"
#include "vf_hip_topk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the block tile of vf_knn_dot and vf_pairwise_dot: BM query rows x BN rows of y per block, BK columns per LDS stage.  Published
 * for the tests, which put their sizes on both sides of each; no result depends on them. */
#define VF_KNN_BM 64
#define VF_KNN_BN 64
#define VF_KNN_BK 32

/* Rows to zero mean (optionally) and unit Euclidean norm (added under ABI 13): after it the dot product of two rows is their
 * Pearson correlation (center = 1) or their cosine (center = 0).
 * Arguments:
 *   x       fp32 [R, >= d], rows ldx elements apart (64-bit row offsets);  d  the columns of a row;
 *   center  1: subtract the row's mean;  0: mean = 0.0f;
 *   z       fp32 [R, >= d], rows ldz elements apart;  norm  NULL, or fp32 [R].
 * Write set: z[r * ldz + c] for 0 <= r < R, 0 <= c < d, and norm[r] for 0 <= r < R when norm is given.  Columns of z at or
 * past d and rows at or past R are not touched; x is only read (z == x, with ldz == ldx, is allowed: a row is read whole
 * before it is written).
 * Arithmetic: fp32, two passes, one wave per row.  Pass 1 (center = 1): lane l adds the columns l, l + 64, ... in ascending
 * order from +0.0f, the 64 partial sums meet in the xor butterfly 32, 16, 8, 4, 2, 1, mean = sum / d.  Pass 2: with
 * t = x - mean, lane l accumulates fmaf(t, t, .) over the same columns in the same order, the same butterfly, norm =
 * sqrtf(sum); z = t / norm (IEEE division).  Never the one-pass sum(x^2) - sum(x)^2 / d.  A row with norm == 0 (all zero, or
 * constant under center = 1: its d values all compare equal, also where the fp32 mean of d equal values is an ulp off them)
 * gets z = +0.0f throughout and norm[r] = 0: it is then at similarity 0 from every row.  The row's results depend on its d
 * values, d and center alone: not on R, the strides or the row's position.
 * Non-finite operands: a NaN or an Inf in the row -- or a sum of squares that overflows fp32 -- makes norm non-finite; the
 * whole z row is then a quiet NaN and so is norm[r].  Other rows are not affected.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null x or z; x, z or
 * norm not 4-byte aligned; d < 1; ldx < d; ldz < d; center outside 0 .. 1; R < 0; R >= 2^33 (the grid: four rows per
 * block).  R == 0 is VF_OK with nothing launched. */
int vf_rows_standardize(const float* x, int64_t ldx, int64_t R, int d, int center, float* z, int64_t ldz, float* norm,
                        void* stream);

/* The k most similar rows of y for every row of q (added under ABI 13), by the similarity s above: with both standardised, a
 * correlation or cosine k-nearest-neighbour search.  No buffer grows with Rq * Ry.
 * Arguments:
 *   q            fp32 [Rq, >= d], rows ldq apart;  y  fp32 [Ry, >= d], rows ldy apart (64-bit row offsets; q and y may overlap);
 *   self_offset  -1: every j in [0, Ry) is a candidate of query r;  >= 0: every j but j == r + self_offset (q is the slice of y
 *                that starts at row self_offset; an r + self_offset at or past Ry excludes nothing);
 *   k            how many ranks are written per row;
 *   values       fp32 [Rq, >= k] and indices int32 [Rq, >= k], rows of both ldo elements apart.
 * Order: vf_topk_rows's.  a ranks before b iff a is NaN and b is not, or neither is NaN and a > b by IEEE comparison (so +0
 * and -0 tie, and every NaN ties with every other whatever its sign or payload); among ties the lower j comes first.
 * Write set: for 0 <= r < Rq and 0 <= i < k, indices[r * ldo + i] = the j of rank i among r's candidates and
 * values[r * ldo + i] = the bits of s(r, j); where r has fewer than k candidates the index is -1 and the value +0.0f.  Columns
 * of the outputs at or past k and rows at or past Rq are not touched; q and y are only read.
 * Arithmetic: s as above, on the f32-input MFMA: no split of the column range, one accumulator per (r, j).  A block owns
 * VF_KNN_BM query rows and sweeps y in tiles of VF_KNN_BN rows, VF_KNN_BK columns per LDS stage (a column range that ends
 * inside an MFMA step is filled with q = -0.0f, y = +0.0f, whose product -0 changes no accumulator).  Each row's running
 * best are 64 (key, 2^32 - 1 - j) pairs in LDS, sorted; a tile's scores above the row's rank k - 1 are inserted one by one.
 * Selection is comparisons alone, on vf_topk_rows's 32-bit keys.  No atomics, no workspace.  The outputs of row r depend on
 * q[r], the rows of y, d, self_offset and k alone: not on Rq, ldq, ldy, ldo, r's place in its block or the tile constants,
 * and rank i does not depend on k (the result for k is the beginning of the result for any k' > k).
 * Non-finite operands: a NaN in q[r] makes every s(r, .) NaN (they rank in j order); a NaN in y[j] makes s(., j) NaN, which
 * ranks first in every row; Inf operands follow IEEE (Inf * 0 and Inf - Inf are NaN).  A NaN value is returned with the
 * bits the accumulator holds.  Other rows' operands never reach a row's result.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null q, y, values or
 * indices; q, y, values or indices not 4-byte aligned; d < 1; ldq < d; ldy < d; ldo < k; k outside 1 .. VF_TOPK_MAX_K;
 * Rq < 0; Ry < 0; Ry >= 2^31 (indices are int32); Rq >= 2^36 (the grid: VF_KNN_BM rows per block); self_offset < -1.
 * Rq == 0 is VF_OK with nothing launched; with Ry == 0 nothing is read and every entry of the write set is the -1 / +0.0f
 * padding (y may then be any aligned non-null address). */
int vf_knn_dot(const float* q, int64_t ldq, int64_t Rq, const float* y, int64_t ldy, int64_t Ry, int d, int64_t self_offset,
               int k, float* values, int32_t* indices, int64_t ldo, void* stream);

/* The dense matrix of the same similarities, or of the distances 1 - s (added under ABI 13): for row counts at which it can
 * exist -- the 49 .. 54 tissues of a dendrogram.
 * Arguments: q, ldq, Rq, y, ldy, Ry, d, self_offset as in vf_knn_dot;
 *   mode  0: out[r, j] = s(r, j);  1: out[r, j] = 1.0f - s(r, j), and exactly +0.0f at j == r + self_offset (self_offset >= 0):
 *         1 - corrcoef with the diagonal filled with 0.  In mode 0 self_offset changes nothing;
 *   out   fp32 [Rq, >= Ry], rows ldo elements apart.
 * Write set: out[r * ldo + j] for 0 <= r < Rq, 0 <= j < Ry.  Columns at or past Ry and rows at or past Rq are not touched; q
 * and y are only read.
 * Arithmetic: the tile core of vf_knn_dot, one block per VF_KNN_BM x VF_KNN_BN tile of out, so out[r, j] in mode 0 has the
 * bits vf_knn_dot ranks; mode 1 adds one fp32 subtraction.  An element depends on q[r], y[j], d, mode and self_offset alone.
 * Non-finite operands: as s: a NaN in q[r] or y[j] makes out[r, j] NaN in both modes (the self element of mode 1 is +0.0f
 * whatever the rows hold); nothing crosses rows.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null q, y or out; q, y
 * or out not 4-byte aligned; d < 1; ldq < d; ldy < d; ldo < Ry; mode outside 0 .. 1; Rq < 0; Ry < 0; Ry >= 2^31;
 * self_offset < -1; more than 2^31 - 1 tiles (the grid).  Rq == 0 and Ry == 0 are VF_OK with nothing launched. */
int vf_pairwise_dot(const float* q, int64_t ldq, int64_t Rq, const float* y, int64_t ldy, int64_t Ry, int d, int64_t self_offset,
                    int mode, float* out, int64_t ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_NEIGHBORS_H */

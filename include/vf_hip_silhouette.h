/* vf_hip_silhouette.h -- the entries of libvf_hip.so behind the silhouette coefficient (scikit-learn's silhouette_samples): for
 * every row the sum of its distances to the members of every cluster, by all pairs for the Euclidean distance and by one fp64
 * product with the clusters' sums for the correlation and cosine distances, and the step from those sums to a, b, s and the
 * nearest other cluster.  Every sum has a stated order and there is no atomic, so two runs are equal bit for bit, a row's result
 * does not depend on the range of rows a call asks for, and numpy restates every entry bit for bit (tests/silhouette_cases.py).
 * The stages are driven by variantformer_amd/validation.py.
 *
 * A header of the one library beside vf_hip.h and the vf_hip_*.h family.  Its entries are bound through
 * _lib.ENTRIES["vf_hip_silhouette.h"], which _lib.load() applies like every other table.  Everything vf_hip.h says holds
 * here: the conventions at its top (device pointers owned by the caller, `stream` a hipStream_t, strides in elements, 0 = ok /
 * VF_ERR_*, vf_last_error()), the comment contract of every entry (arguments, write set, arithmetic and its order, non-finite
 * operands, refusals, not checked), and the ABI version: a new symbol changes no existing one, so it stays 13.
 *
 * THE CLUSTERS, stated once.  All three entries take the k clusters as a CSR of rows: `order` int32 [n] holds the n rows that
 * have a label in 0 .. k - 1, sorted by label and ascending within a label (a stable sort of the labels); `seg` int64 [k + 1]
 * holds the offsets, seg[0] = 0 and seg[k] = n: cluster c is order[seg[c] .. seg[c + 1]), n_c = seg[c + 1] - seg[c] members.
 * `labels` int32 [R] is the same partition by row: a value outside 0 .. k - 1 is a row without a label.
 * THE RANGES.  A sum over a cluster's members takes them in the order of `order` (ascending row), cut into
 * W = VF_SILHOUETTE_RANGES contiguous ranges of L = ceil(n_c / W) members, range v = [min(v L, n_c), min((v + 1) L, n_c)).
 * Each range's fp64 sum p_v runs ascending from +0.0, and the ranges are combined as (((p_0 + p_1) + p_2) .. + p_{W-1}).  W is
 * the only constant of this header that enters any bit.  An empty cluster's sum is +0.0.
 * THE QUERY ROWS.  Every entry works on the rows [row0, row0 + rows) and writes nothing for any other row; S is local to the
 * range: S[c * lds + (i - row0)] belongs to row i and cluster c (cluster-major, so that one lane per row stores and loads
 * neighbouring addresses).  A row's result depends on that row, the clusters and d alone: not on row0, rows, R's remainder, the
 * strides or a tile constant.
 * A NaN result is a NaN; its sign and payload are not part of the contract.
 */
#ifndef VF_HIP_SILHOUETTE_H
#define VF_HIP_SILHOUETTE_H

#include "vf_hip_kmeans.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the limits are k-means': its labels are what these entries take */
#define VF_SILHOUETTE_MAX_K VF_KMEANS_MAX_K
#define VF_SILHOUETTE_MAX_R VF_KMEANS_MAX_R
#define VF_SILHOUETTE_MAX_D VF_KMEANS_MAX_D
/* THE RANGES: the one constant that enters the bits; one wavefront of a block per range */
#define VF_SILHOUETTE_RANGES 4
/* query rows per block (one per lane), members whose running sums a thread holds in registers, and columns per staged chunk:
 * VF_SILHOUETTE_DC_SMALL where d <= VF_SILHOUETTE_DC_SMALL, VF_SILHOUETTE_DC where d <= VF_SILHOUETTE_DC, else
 * VF_SILHOUETTE_DC_WIDE.  A staged tile holds VF_SILHOUETTE_RANGES * VF_SILHOUETTE_JT members.  None of them enters a bit. */
#define VF_SILHOUETTE_ROWS 64
#define VF_SILHOUETTE_JT 8
#define VF_SILHOUETTE_DC_SMALL 4
#define VF_SILHOUETTE_DC 32
#define VF_SILHOUETTE_DC_WIDE 64
/* bytes of vf_silhouette_sums_dot's workspace: one fp64 per (cluster, column) */
#define VF_SILHOUETTE_DOT_WORK_BYTES(d, k) (8 * (int64_t)(k) * (int64_t)(d))

/* The summed Euclidean distance of every query row to the members of every cluster, by all pairs (added under ABI 13).
 * Arguments:
 *   x      fp32 [R, >= d], rows ldx apart (64-bit offsets);  R  rows, 0 .. VF_SILHOUETTE_MAX_R;  d  columns;
 *   order  int32 [n], seg  int64 [k + 1]: THE CLUSTERS;  n  0 .. R;  k  1 .. VF_SILHOUETTE_MAX_K;
 *   row0, rows  THE QUERY ROWS, 0 <= row0, 0 <= rows, row0 + rows <= R;
 *   S      fp64 [k, >= rows], clusters lds apart.
 * Write set, exactly: S[c * lds + q] for 0 <= c < k, 0 <= q < rows.  x, order and seg are only read, x at columns below d.
 * Arithmetic: D(i, j) is THE DISTANCE of include/vf_hip_kmeans.h between rows i and j: from +0.0f over the columns c = 0 .. d - 1
 * ascending, t = x[i, c] - x[j, c];  p = t * t;  acc = acc + p, every step one individually rounded fp32 operation, NO fused
 * multiply-add.  S[c, i] = the sum over the members j of cluster c, in the order of THE RANGES, of (double)sqrtf(D(i, j)), the
 * square root correctly rounded in fp32, the conversion exact, the additions fp64.  The pair of a row with itself contributes an
 * exact +0.0 and is not treated specially; every pair is computed from both sides, so that the sum is a gather.  One lane per
 * query row, VF_SILHOUETTE_ROWS rows per block; wavefront v of the block takes range v of every cluster; the members come
 * through LDS, gathered through `order`, a chunk of columns at a time, where all lanes read one address.
 * Non-finite operands: follow IEEE through the chain, the square root and the sums: a row with a NaN makes every sum it enters
 * NaN, its own included; +Inf is an ordinary value.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null x, order, seg or S;
 * x or order not 4-byte aligned, seg or S not 8-byte aligned; d outside 1 .. VF_SILHOUETTE_MAX_D; ldx < d; k outside
 * 1 .. VF_SILHOUETTE_MAX_K; R < 0; R > VF_SILHOUETTE_MAX_R (2^24); n outside 0 .. R; row0 < 0; rows < 0; row0 + rows > R;
 * lds < rows.  rows == 0 is VF_OK with nothing launched.
 * Not checked: that seg and order are THE CLUSTERS of any labels (they are on the device).  An offset is used clamped to
 * 0 .. n and a segment that would run backwards as empty; an element of order outside 0 .. R - 1 stands for a row of NaN: a
 * malformed CSR gives sums without meaning and reads nothing outside x, order and seg.  That S does not overlap an operand. */
int vf_silhouette_sums_l2(const float* x, int64_t ldx, int64_t R, int d, const int32_t* order, int64_t n, const int64_t* seg, int k,
                          int64_t row0, int64_t rows, double* S, int64_t lds, void* stream);

/* The summed correlation (or cosine) distance 1 - z_i . z_j of every query row to the members of every cluster, from the
 * clusters' column sums: O(R k d), not all pairs (added under ABI 13).  Two launches.
 * Arguments:
 *   z      fp32 [R, >= d], rows ldz apart: the standardised rows (vf_rows_standardize);  R, d  as above;
 *   order, n, seg, k  THE CLUSTERS;  labels  int32 [R];  row0, rows  THE QUERY ROWS;
 *   S      fp64 [k, >= rows], clusters lds apart;
 *   work   the caller's workspace, 8-byte aligned, of work_bytes >= VF_SILHOUETTE_DOT_WORK_BYTES(d, k) bytes: M fp64 [k, d].
 * Write set, exactly: S[c * lds + q] for 0 <= c < k, 0 <= q < rows; the first VF_SILHOUETTE_DOT_WORK_BYTES(d, k) bytes of work,
 * which afterwards hold M.
 * Arithmetic, first launch: M[c, col] = the sum over the members j of cluster c, in the order of THE RANGES, of (double)z[j, col].
 * Second launch, for query row i and cluster c, all in fp64, every operation rounded once, NO fused multiply-add, both sums
 * from +0.0 over col = 0 .. d - 1 ascending:
 *     t = t + (double)z[i, col] * M[c, col];      q = q + (double)z[i, col] * (double)z[i, col]
 *     own = 1 where labels[i] == c, else 0;       u = t - q where own == 1, else t
 *     S[c, i] = (double)(n_c - own) - u
 * that is the sum of 1 - z_i . z_j over the members other than i itself.  One lane per query row; the rows of M come through LDS.
 * Non-finite operands: follow IEEE; a NaN row makes the sums of its cluster NaN for every row, and all of its own sums.
 * Refused before anything is launched: a null z, order, seg, labels, S or work; z, order or labels not 4-byte aligned, seg, S or
 * work not 8-byte aligned; d outside 1 .. VF_SILHOUETTE_MAX_D; ldz < d; k outside 1 .. VF_SILHOUETTE_MAX_K; R < 0;
 * R > VF_SILHOUETTE_MAX_R; n outside 0 .. R; row0 < 0; rows < 0; row0 + rows > R; lds < rows; work_bytes below
 * VF_SILHOUETTE_DOT_WORK_BYTES(d, k).  rows == 0 is VF_OK with nothing launched and nothing written.
 * Not checked: as in vf_silhouette_sums_l2, with the same clamps; that labels agrees with order and seg; overlaps. */
int vf_silhouette_sums_dot(const float* z, int64_t ldz, int64_t R, int d, const int32_t* order, int64_t n, const int64_t* seg, int k,
                           const int32_t* labels, int64_t row0, int64_t rows, double* S, int64_t lds, void* work, int64_t work_bytes,
                           void* stream);

/* From the sums to the silhouette of every query row (added under ABI 13).
 * Arguments:
 *   S       fp64 [k, >= rows], clusters lds apart: what either entry above wrote for the same row0 and rows;
 *   labels  int32 [R];  R  0 .. VF_SILHOUETTE_MAX_R;  seg  int64 [k + 1];  k  1 .. VF_SILHOUETTE_MAX_K;  row0, rows  THE QUERY ROWS;
 *   a, b, s  fp64 [R];  nearest  int32 [R].
 * Write set, exactly: a[i], b[i], s[i] and nearest[i] for row0 <= i < row0 + rows.
 * Arithmetic, for row i with label l, in fp64 with the correctly rounded `/`; n_c = seg[c + 1] - seg[c]:
 *   b, nearest: over the clusters c = 0 .. k - 1 ascending, c != l, n_c > 0: mean_c = S[c, i] / (double)n_c; the smallest by IEEE
 *     comparison wins, ties to the lower c, a NaN mean never wins.  Without a winner b is NaN and nearest is -1.
 *   a = S[l, i] / (double)(n_l - 1);  a = +0.0 where n_l == 1;  a is NaN where l is outside 0 .. k - 1, and then b and nearest
 *     range over all clusters.
 *   s: NaN where a or b is NaN;  else +0.0 where n_l == 1;  else with m = the larger of a and b: +0.0 where m == 0, else
 *     (b - a) / m, one subtraction and one division.
 * Non-finite operands: follow IEEE: an infinite a or b gives what the formula gives.
 * Refused before anything is launched: a null S, labels, seg, a, b, s or nearest; labels or nearest not 4-byte aligned, S, seg, a,
 * b or s not 8-byte aligned; k outside 1 .. VF_SILHOUETTE_MAX_K; R < 0; R > VF_SILHOUETTE_MAX_R; row0 < 0; rows < 0;
 * row0 + rows > R; lds < rows.  rows == 0 is VF_OK with nothing launched.
 * Not checked: that seg and labels describe one partition (a segment that would run backwards counts as empty); overlaps. */
int vf_silhouette_finish(const double* S, int64_t lds, const int32_t* labels, int64_t R, const int64_t* seg, int k, int64_t row0,
                         int64_t rows, double* a, double* b, double* s, int32_t* nearest, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_SILHOUETTE_H */

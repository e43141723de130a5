/* vf_hip_linkage.h -- the entries of libvf_hip.so behind the hierarchical clustering of a distance matrix (Ward linkage, the
 * step vcf2exp's compute_ordered_leaves hands to scipy.cluster.hierarchy.linkage): the nearest other row of every row, and one
 * round of merging mutually nearest clusters -- Lance-Williams update and compaction in one gather pass.  Ward is a reducible
 * linkage: every pair of mutually nearest clusters belongs to the final tree, so all such pairs of a round merge at once and
 * the tree takes a few dozen data-parallel rounds over a shrinking matrix.  The rounds are driven by variantformer_amd/linkage.py.
 *
 * One of eight headers of the one library, beside vf_hip.h, vf_hip_attn_contrib.h, vf_hip_gene_contrib.h, vf_hip_cre_heads.h,
 * vf_hip_forest.h, vf_hip_topk.h and vf_hip_neighbors.h.  Its entries are bound through _lib.ENTRIES["vf_hip_linkage.h"], which
 * _lib.load() applies like the other seven tables, and tests/linkage_cases.py holds their reference and case table.
 * Everything the main header says holds here: the conventions at its top (device pointers owned by the caller, `stream` a
 * hipStream_t, strides in elements, 0 = ok / VF_ERR_*, vf_last_error()), the comment contract of every entry (arguments, write
 * set, arithmetic, non-finite operands, refusals), and VF_ABI_VERSION: a new symbol changes no existing one, so the version
 * stays 13.
 *
 * Every operation of this header is one individually rounded IEEE fp32 operation (round to nearest even, denormals kept):
 * nothing is contracted into a fused multiply-add, division and square root are the correctly rounded ones.  A restatement in
 * fp32 numpy with the same operation order therefore has the same bits (tests/linkage_cases.py is one).
 */
#ifndef VF_HIP_LINKAGE_H
#define VF_HIP_LINKAGE_H

#include "vf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest matrix side (and so the largest cluster size): every size and sum of sizes is then an exact fp32 */
#define VF_LINKAGE_MAX_M (1 << 24)

/* The nearest other row of every row (added under ABI 13).
 * Arguments:
 *   D       fp32 [m, >= m], rows ld elements apart (64-bit offsets);  m  its side;
 *   nn_val  fp32 [m];  nn_idx  int32 [m].
 * Order: ascending by value; a ranks before b iff better(a, b) = !isnan(a) && (isnan(b) || a < b) by IEEE comparison, so NaN
 * ranks last, above +Inf, +0 and -0 tie, and every NaN ties with every other; among ties the lower j comes first.
 * Write set: for 0 <= i < m, nn_idx[i] = the j != i whose D[i, j] ranks first among row i's m - 1 candidates and nn_val[i] =
 * the bits of that D[i, j] (a -0 and a NaN's payload survive).  With m == 1 there is no candidate: nn_idx[0] = -1 and
 * nn_val[0] = +Inf.  D is only read, and only at [i, j] with i, j < m; D[i, i] is never read.
 * Arithmetic: comparisons alone.  One block per row, the row read contiguously; the result of row i depends on its m - 1
 * values alone.
 * Non-finite operands: part of the order above; a row of NaNs finds its lowest j != i.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null D, nn_val or nn_idx;
 * D, nn_val or nn_idx not 4-byte aligned; m < 0; m > VF_LINKAGE_MAX_M (2^24); ld < m.  m == 0 is VF_OK with nothing launched. */
int vf_linkage_nearest(const float* D, int64_t ld, int64_t m, float* nn_val, int32_t* nn_idx, void* stream);

/* One round of merges (added under ABI 13): the m clusters of D become m_out.  New slot a stands for old slot first[a] alone
 * (second[a] == -1) or for the merge of old slots first[a] < second[a].
 * Arguments:
 *   D           fp32 [m, >= m], rows ld apart: the distances between the m old clusters;  size  int32 [m], their sizes (>= 1);
 *   first       int32 [m_out], second  int32 [m_out]: the constituents of every new slot, as above;
 *   D_out       fp32 [m_out, >= m_out], rows ld_out apart;  size_out  int32 [m_out];  pair_dist  fp32 [m_out];
 *   upper_only  1: every old distance d(X, Y) is read at D[min(X, Y), max(X, Y)] -- the first round, which makes the symmetric
 *               working matrix out of the caller's upper triangle as scipy's squareform does; the lower triangle and the
 *               diagonal are never read.  0: D is symmetric bit for bit (an earlier D_out) and d(X, Y) is read from the row of
 *               the constituent of the output row, as it coalesces best; the diagonal is never read.
 * Not checked (the caller guarantees; variantformer_amd/linkage.py does): first is strictly increasing, the constituents are
 * disjoint, sizes are positive and sum to at most 2^24, D_out / size_out / pair_dist do not overlap D or each other.  A
 * first[a] or second[a] outside [0, m) is no valid input but stays inside D: first is clamped into [0, m), a second >= m to
 * m - 1, and every negative second means "alone".
 * Write set, exactly: D_out[a * ld_out + b] for 0 <= a, b < m_out, the diagonal +0.0f; size_out[a] = size[first[a]]
 * (+ size[second[a]]) and pair_dist[a] = d(first[a], second[a]), the merged pair's own distance, or +0.0f for a slot that
 * stands alone, for 0 <= a < m_out.  Columns of D_out at or past m_out are not touched; D, size, first and second are only read.
 * Arithmetic: with
 *   LW(dxi, dyi, dxy, sx, sy, si) = sqrt(max0((((sx+si) * (dxi*dxi) + (sy+si) * (dyi*dyi)) - si * (dxy*dxy)) / (sx+sy+si)))
 * where every size sum is formed in integers and converted exactly, every product is float(s) * (d * d), each operation is
 * rounded once, and max0(q) = q < 0 ? +0.0f : q (a NaN passes).  For a != b let lo = min(a, b) be made of A(, B) and
 * hi = max(a, b) of C(, D):
 *   both alone        D_out[a, b] = d(A, C), copied;
 *   lo merged only    LW(d(A,C), d(B,C), d(A,B), sA, sB, sC);
 *   hi merged only    LW(d(A,C), d(A,D), d(C,D), sC, sD, sA);
 *   both merged       u = LW(d(A,C), d(B,C), d(A,B), sA, sB, sC), v = LW(d(A,D), d(B,D), d(A,B), sA, sB, sD),
 *                     LW(u, v, d(C,D), sC, sD, sA + sB).
 * The roles are those of lo and hi whichever thread computes the element, so D_out is symmetric bit for bit.  max0 is the one
 * deviation from scipy's Ward update: for mutually nearest pairs the radicand is at least min(dxi, dyi)^2 in exact arithmetic,
 * so it is negative through rounding alone.  A small first launch writes size_out and pair_dist, the gather pass reads
 * pair_dist back; one block per output row, no block waits for another.
 * Non-finite operands: follow IEEE through LW: a NaN distance makes every element it enters NaN, Inf - Inf is NaN; elements
 * it does not enter are not affected.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null D, size, first,
 * second, D_out, size_out or pair_dist; any of the seven not 4-byte aligned; m < 0; m > VF_LINKAGE_MAX_M (2^24); ld < m;
 * m_out < 0; m_out > m; ld_out < m_out; upper_only outside 0 .. 1.  m_out == 0 is VF_OK with nothing launched. */
int vf_linkage_contract(const float* D, int64_t ld, int64_t m, const int32_t* size, const int32_t* first, const int32_t* second,
                        int64_t m_out, float* D_out, int64_t ld_out, int32_t* size_out, float* pair_dist, int upper_only,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_LINKAGE_H */

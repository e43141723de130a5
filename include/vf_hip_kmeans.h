/* vf_hip_kmeans.h -- the entries of libvf_hip.so behind k-means clustering (scikit-learn's KMeans(algorithm="lloyd")): the
 * assignment of every row to its nearest centre, the fp64 means of the clusters, all iterations of Lloyd's loop with the stop
 * decided on the device, and plain D^2 seeding (Arthur-Vassilvitskii) with integer sampling.  Every sum has a stated order and
 * there is no atomic, so two runs are equal bit for bit, a run can be split at any iteration, and numpy restates every entry bit
 * for bit (tests/kmeans_cases.py).  The stages are driven by variantformer_amd/kmeans.py.
 *
 * A header of the one library beside vf_hip.h and the vf_hip_*.h family.  Its entries are bound through
 * _lib.ENTRIES["vf_hip_kmeans.h"], which _lib.load() applies like the other tables.  Everything the main header says holds here: the conventions at its top
 * (device pointers owned by the caller, `stream` a hipStream_t, strides in elements, 0 = ok / VF_ERR_*, vf_last_error()), the
 * comment contract of every entry (arguments, write set, arithmetic and its order, non-finite operands, refusals, not checked),
 * and the ABI version: a new symbol changes no existing one, so it stays 13.
 *
 * THE DISTANCE, stated once.  For row r and centre j the squared distance is formed from +0.0f over the columns
 * c = 0 .. d - 1 in ascending order:
 *     t = x[r, c] - cen[j, c];   p = t * t;   acc = acc + p
 * every step one individually rounded IEEE fp32 operation (round to nearest even, denormals kept), NO fused multiply-add, as
 * vf_linkage_contract does it.  It is not the |c|^2 - 2 x.c expansion: on 2-D coordinates and on tight clusters far from the
 * origin the expansion cancels, and its bits would depend on a tile order.  A distance is never negative and never -0.
 * THE WINNER of row r is the centre with the smallest distance by IEEE comparison, ties to the lower j; a NaN distance never
 * wins; a row whose distances are all NaN has label -1 and dist NaN (0x7FC00000).  +Inf is an ordinary value: a row with an
 * Inf has distance +Inf to every finite centre and takes the lowest of them.  The result for a row depends on that row, the
 * centres, d and k alone: not on R, the strides, the tile constants below or the split of the centres among wavefronts
 * (merging partial winners by (distance, j) is exact).
 */
#ifndef VF_HIP_KMEANS_H
#define VF_HIP_KMEANS_H

#include "vf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most centres: VF_ENRICH_MAX_K, what the labels' consumer takes */
#define VF_KMEANS_MAX_K 4096
/* the most rows: a row is an int32, and the seeding's integer total stays below 2^56 */
#define VF_KMEANS_MAX_R (1 << 24)
/* the most columns: the update's grid has one block row per 64 of them */
#define VF_KMEANS_MAX_D 65536
/* the assignment: rows per block (one per lane), splits of the centres (one per wavefront of the block), centres whose running
 * sums a thread holds in registers, and columns per staged chunk (VF_KMEANS_DC_SMALL where d <= VF_KMEANS_DC_SMALL).  A staged
 * tile holds VF_KMEANS_SPLITS * VF_KMEANS_JT centres. */
#define VF_KMEANS_ROWS 64
#define VF_KMEANS_SPLITS 4
#define VF_KMEANS_JT 8
#define VF_KMEANS_DC 32
#define VF_KMEANS_DC_SMALL 4
/* the update: contiguous row ranges (one wavefront each), and columns per block */
#define VF_KMEANS_UPDATE_WAVES 16
#define VF_KMEANS_UPDATE_COLS 64
/* threads of the single-block reductions (the shift, the changed count, the seeding's selection) and rows per seeding block */
#define VF_KMEANS_RED_THREADS 256
/* bytes of vf_kmeans_lloyd's workspace: the stop word (8), one fp64 per (centre, column tile), one int32 per assignment block */
#define VF_KMEANS_LLOYD_WORK_BYTES(R, d, k)                                                                               \
    (8 + 8 * (int64_t)(k) * (((int64_t)(d) + VF_KMEANS_UPDATE_COLS - 1) / VF_KMEANS_UPDATE_COLS) +                        \
     4 * (((int64_t)(R) + VF_KMEANS_ROWS - 1) / VF_KMEANS_ROWS))
/* bytes of vf_kmeans_seed's workspace: per block of VF_KMEANS_RED_THREADS rows one uint64 and one fp32, and 16 bytes of scalars */
#define VF_KMEANS_SEED_WORK_BYTES(R) (16 + 12 * (((int64_t)(R) + VF_KMEANS_RED_THREADS - 1) / VF_KMEANS_RED_THREADS))

/* The nearest centre of every row (added under ABI 13).
 * Arguments:
 *   x       fp32 [R, >= d], rows ldx apart (64-bit offsets);  R  rows;  d  columns;
 *   cen     fp32 [k, >= d], rows ldc apart;  k  centres, 1 .. VF_KMEANS_MAX_K;
 *   labels  int32 [R];  dist  fp32 [R].
 * Write set, exactly: labels[r] = THE WINNER of row r and dist[r] = its distance (header top), for 0 <= r < R.  x and cen are
 * only read, at columns below d.
 * Arithmetic: THE DISTANCE.  One lane per row, VF_KMEANS_ROWS rows per block; wavefront w of the block takes the centres
 * g * 32 + w * VF_KMEANS_JT + (0 .. VF_KMEANS_JT - 1) of every staged tile g, the tiles come through LDS VF_KMEANS_DC columns
 * at a time, where all lanes read one address, and wavefront 0 merges the four partial winners.  None of it enters the bits.
 * Non-finite operands: as THE WINNER says; a NaN centre is never chosen, a NaN in a row gives it label -1.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null x, cen, labels or
 * dist; any of the four not 4-byte aligned; d outside 1 .. VF_KMEANS_MAX_D; ldx or ldc < d; k outside 1 .. VF_KMEANS_MAX_K; R < 0; R > VF_KMEANS_MAX_R
 * (2^24).  R == 0 is VF_OK with nothing launched.
 * Not checked: that labels and dist do not overlap x or cen. */
int vf_kmeans_assign(const float* x, int64_t ldx, int64_t R, int d, const float* cen, int64_t ldc, int k, int32_t* labels, float* dist,
                     void* stream);

/* The mean of every cluster's rows, in fp64 (added under ABI 13).
 * Arguments:
 *   x, ldx, R, d  as above;  labels  int32 [R]: a value outside 0 .. k - 1 belongs to no centre;
 *   cen_old  fp32 [k, >= d], rows ldc apart;  k  1 .. VF_KMEANS_MAX_K;  cen_new  fp32 [k, >= d], rows ldn apart;
 *   counts   int32 [k].
 * Write set, exactly: cen_new[j * ldn + c] for 0 <= j < k, 0 <= c < d, and counts[j].  cen_new may BE cen_old (the same
 * pointer and stride): every element is then read by the one thread that writes it, before it writes.
 * Arithmetic: the rows are cut into W = VF_KMEANS_UPDATE_WAVES contiguous ranges of L = ceil(R / W) rows, range v =
 * [min(v L, R), min((v + 1) L, R)).  For centre j and column c, p_v = the sum of (double)x[r, c] over the members r of range v
 * in ascending r, from +0.0;  S = (((p_0 + p_1) + p_2) .. + p_{W-1});  n = the members;  cen_new[j, c] = (float)(S / (double)n),
 * one correctly rounded fp64 division and one rounding to fp32.  A centre without members keeps cen_old[j, c]'s bits and has
 * counts[j] = 0.  One block per (centre, VF_KMEANS_UPDATE_COLS columns), wavefront v scanning its range's labels 64 at a time
 * and walking the set bits of the ballot; the lane mapping does not enter the bits.  No sort, no atomic.
 * Non-finite operands: follow IEEE through the sums.
 * Refused before anything is launched (VF_ERR_INVALID_ARG): a null x, labels, cen_old, cen_new or counts; any of the five not 4-byte aligned; d outside 1 .. VF_KMEANS_MAX_D;
 * ldx, ldc or ldn < d; k outside 1 .. VF_KMEANS_MAX_K; R < 0; R > VF_KMEANS_MAX_R.  R == 0 runs: every centre keeps cen_old.
 * Not checked: that cen_new, where it is not cen_old, does not overlap it, and that neither overlaps x, labels or counts. */
int vf_kmeans_update(const float* x, int64_t ldx, int64_t R, int d, const int32_t* labels, const float* cen_old, int64_t ldc, int k,
                     float* cen_new, int64_t ldn, int32_t* counts, void* stream);

/* Up to max_iter iterations of Lloyd's loop and a last assignment, from one loop inside the entry (added under ABI 13):
 * scikit-learn's _kmeans_single_lloyd.  Nothing is read back by the host: the stop is a word of the workspace.
 * Arguments:
 *   x, ldx, R, d  as above;  cen  fp32 [k, >= d], rows ldc apart: in, the start; out, the result;  k  1 .. VF_KMEANS_MAX_K;
 *   max_iter  >= 0;  tol_abs  fp64, >= 0 (not NaN);  resume  0: a fresh run, prev_labels is not read;  1: prev_labels holds the
 *             labels of the iteration before;
 *   labels  int32 [R], dist  fp32 [R]: the last assignment;  prev_labels  int32 [R]: the labels of the last iteration that ran;
 *   counts  int32 [k]: the members behind the last update that ran (prev_labels', not labels');
 *   n_iter  int32 [1];  shift  fp64 [max_iter];  changed  int64 [max_iter];
 *   work    the caller's workspace, 8-byte aligned, of work_bytes >= VF_KMEANS_LLOYD_WORK_BYTES(R, d, k) bytes.
 * Arithmetic: per iteration n = 0 .. max_iter - 1, three launches, each of which reads the stop word first and returns without
 * writing once it is raised:
 *   1. prev_labels[r] = vf_kmeans_assign's label against cen, bit for bit; every block counts its rows whose label differs from
 *      the value it replaced (a -1 is a label like any other).  In iteration 0 of a call with resume == 0 the old value is not
 *      read and every row counts;
 *   2. cen = vf_kmeans_update(x, prev_labels, cen), in place, bit for bit, and counts; block (j, tile) also forms
 *      q = the sum over its columns c ascending, from +0.0, of e * e with e = (double)new - (double)old, individually rounded;
 *   3. one block of VF_KMEANS_RED_THREADS threads: changed[n] = the sum of the blocks' counts (integers: exact);
 *      shift[n] = the q, indexed i = j * tiles + tile: thread u adds i = u, u + VF_KMEANS_RED_THREADS, .. ascending from +0.0,
 *      and the threads' sums are added by a tree (stride 128, 64, .. 1: s[u] += s[u + stride]);  n_iter[0] = n + 1;  then the
 *      stop word is raised if changed[n] == 0 (not in iteration 0 of a call with resume == 0) or shift[n] <= tol_abs.
 * After the loop one vf_kmeans_assign(x, cen) into labels and dist: always, whatever the stop word says.  After a stop by
 * labels it reproduces prev_labels.
 * Write set, exactly: cen at [j * ldc + c], c < d; labels, dist, prev_labels [0, R); counts [0, k); n_iter[0] (0 when
 * max_iter == 0); shift[n] and changed[n] for n < n_iter[0] ALONE: the elements past the stop keep the caller's bytes; the
 * first VF_KMEANS_LLOYD_WORK_BYTES(R, d, k) bytes of work, whose content afterwards is not part of the contract.
 * The result depends on the arguments alone.  max_iter = a, then resume = 1 with max_iter = b on the carried cen and prev_labels,
 * equals one call with a + b whenever the first call did not stop (its n_iter == a, shift and changed continued).  Once
 * changed == 0 further iterations would reproduce cen and prev_labels bit for bit.
 * Non-finite operands: as in the two entries; a NaN shift never satisfies shift <= tol_abs.
 * Refused before anything is launched: a null x, cen, labels, dist, prev_labels, counts, n_iter or work, a null shift or
 * changed unless max_iter == 0; n_iter, x, cen, labels, dist, prev_labels or counts not 4-byte aligned, shift, changed or work
 * not 8-byte aligned; d outside 1 .. VF_KMEANS_MAX_D; ldx or ldc < d; k outside 1 .. VF_KMEANS_MAX_K; R < 0; R > VF_KMEANS_MAX_R; max_iter < 0; tol_abs
 * NaN or negative; resume outside 0 .. 1; work_bytes below VF_KMEANS_LLOYD_WORK_BYTES(R, d, k).  R == 0 is VF_OK with nothing
 * launched and nothing written.
 * Not checked: that the buffers do not overlap. */
int vf_kmeans_lloyd(const float* x, int64_t ldx, int64_t R, int d, float* cen, int64_t ldc, int k, int max_iter, double tol_abs, int resume,
                    int32_t* labels, float* dist, int32_t* prev_labels, int32_t* counts, int32_t* n_iter, double* shift, int64_t* changed,
                    void* work, int64_t work_bytes, void* stream);

/* Plain D^2 seeding (added under ABI 13): k rows of x as starting centres, all k steps from one loop inside the entry, the
 * sampling in exact integer arithmetic so that no float prefix sum needs an order.
 * Arguments:
 *   x, ldx, R, d  as above, R >= 1;  k  1 .. min(R, VF_KMEANS_MAX_K);  seed  its low 32 bits enter;
 *   rows  int32 [k]: the chosen rows;  cen  fp32 [k, >= d], rows ldc apart: copies of them;  mind  fp32 [R];
 *   work  8-byte aligned, work_bytes >= VF_KMEANS_SEED_WORK_BYTES(R).
 * Arithmetic: hash(seed, t), 64 bits from the 32-bit mixer of vf_hip_umap.h (x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B;
 * x ^= x >> 16):  a = mix((uint32)seed + 0x9E3779B9);  hash = (uint64)mix(a ^ (2 t)) << 32 | mix(a ^ (2 t + 1)).
 * mulhi64(h, n) = floor(h * n / 2^64), below n.
 * Step 0 takes row mulhi64(hash(seed, 0), R).  Step t = 1 .. k - 1, four launches:
 *   mind[r] = THE DISTANCE to centre t - 1 at t == 1 (mind is not read), else that distance where it is < the old mind by IEEE
 *     comparison (a NaN never replaces and is never replaced);
 *   m = the largest finite mind, +0 if there is none (a maximum: exact in any order);
 *   q[r] = (uint64)((double)mind[r] / (double)m * 4294967296.0), truncated, and 0 for a non-finite mind or m == 0;
 *     total = the sum of q: below 2^56, an integer sum, exact in any order;
 *   target = mulhi64(hash(seed, t), total); the chosen row is the lowest r whose inclusive prefix sum of q exceeds target.  With
 *     total == 0 (fewer distinct finite rows than k) the lowest row not yet chosen is taken.
 * Write set, exactly: rows[t], cen[t * ldc + c] for t < k, c < d; mind [0, R) if k >= 2 (the state before the last choice);
 * the first VF_KMEANS_SEED_WORK_BYTES(R) bytes of work.  A chosen row has mind 0 and q 0: no row is chosen twice.
 * Non-finite operands: a row with a NaN or an Inf has a NaN or infinite mind and q = 0: it is drawn by the fallback alone; the
 * distance to such a centre is NaN or +Inf for every row and replaces no mind.
 * This is NOT scikit-learn's greedy k-means++, which tries 2 + log k candidates per step from its own generator.
 * Refused before anything is launched: a null x, rows, cen, mind or work; x, rows, cen or mind not 4-byte aligned, work not
 * 8-byte aligned; d outside 1 .. VF_KMEANS_MAX_D; ldx or ldc < d; R < 1; R > VF_KMEANS_MAX_R; k outside 1 .. min(R, VF_KMEANS_MAX_K); work_bytes below
 * VF_KMEANS_SEED_WORK_BYTES(R).
 * Not checked: that the buffers do not overlap. */
int vf_kmeans_seed(const float* x, int64_t ldx, int64_t R, int d, int k, int64_t seed, int32_t* rows, float* cen, int64_t ldc, float* mind,
                   void* work, int64_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_KMEANS_H */

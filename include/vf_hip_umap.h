/* vf_hip_umap.h -- the entries of libvf_hip.so behind UMAP's two stages after the k-nearest-neighbour graph (what vcf2embed's
 * umap.UMAP(n_neighbors=30, min_dist=0.05, metric='correlation').fit_transform does once neighbors.knn has answered): the fuzzy
 * simplicial set -- every row's rho and sigma with its directed membership strengths, and their fuzzy union over the symmetric
 * graph -- and the epochs of the SGD layout, in a gather formulation: every vertex reads the others where they stood when the
 * epoch began and writes its own row alone, so an epoch has no race, no atomic and one result.  The stages are driven by
 * variantformer_amd/manifold.py, which also builds the symmetric graph's CSR arrays with torch.
 *
 * One of nine headers of the one library, beside vf_hip.h, vf_hip_attn_contrib.h, vf_hip_gene_contrib.h, vf_hip_cre_heads.h,
 * vf_hip_forest.h, vf_hip_topk.h, vf_hip_neighbors.h and vf_hip_linkage.h.  Its entries are bound through _lib.ENTRIES["vf_hip_umap.h"],
 * which _lib.load() applies like the other eight tables, and tests/umap_cases.py holds their references and case table.
 * Everything the main header says holds here: the conventions at its top (device pointers owned by the caller, `stream` a
 * hipStream_t, strides in elements, 0 = ok / VF_ERR_*, vf_last_error()), the comment contract of every entry (arguments, write
 * set, arithmetic, non-finite operands, refusals), and VF_ABI_VERSION: a new symbol changes no existing one, so the version
 * stays 13.
 *
 * Nothing in this header's code is contracted into a fused multiply-add; exp and pow are the compiler's fp32 library functions,
 * so results are held to fp64 restatements within measured bounds (tests/umap_cases.py), and every selection, every integer
 * (the due rule, the hash, the negative vertex) exactly.
 */
#ifndef VF_HIP_UMAP_H
#define VF_HIP_UMAP_H

#include "vf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the longest neighbour list: n_neighbors = m + 1 <= 64, one lane of a wavefront per neighbour */
#define VF_UMAP_MAX_M 63
/* the most rows: a vertex is an int32 and the negative vertex (h * R) >> 32 an exact product */
#define VF_UMAP_MAX_R (1 << 24)
/* the most output coordinates: a vertex's position is held in registers */
#define VF_UMAP_MAX_DIM 8
/* the bisection of sigma: iterations at most, the tolerance on the sum, and the floor's factor (umap-learn's constants) */
#define VF_UMAP_SMOOTH_ITERS 64
#define VF_UMAP_SMOOTH_TOL 1e-5f
#define VF_UMAP_MIN_SCALE 1e-3f

/* rho, sigma and the directed membership strengths of every row's neighbour list (added under ABI 13): umap-learn's
 * smooth_knn_dist with local_connectivity = 1, bandwidth = 1, followed by its compute_membership_strengths.
 * Arguments:
 *   idx        int32 [R, >= m], rows ld_idx apart, and  dist  fp32 [R, >= m], rows ld_dist apart (64-bit offsets): the m other
 *              rows nearest to each row and their distances, as neighbors.knn(include_self=False) returns them;  R  rows;
 *              m  entries per row, 1 .. VF_UMAP_MAX_M;
 *   mean_dist  fp32: the mean of all present distances (the floor of sigma where rho == 0);
 *   rho, sigma fp32 [R];  strength  fp32 [R, >= m], rows ld_strength apart.
 * An entry is ABSENT if its index is negative or its distance is NaN, +Inf or -Inf; every other entry is present.  An absent
 * entry contributes to nothing below.
 * Write set, exactly: rho[i], sigma[i] and strength[i * ld_strength + t] for 0 <= i < R, 0 <= t < m.  idx and dist are only
 * read, at [i, t] with t < m.
 * Arithmetic, per row, in fp32:
 *   rho    = the smallest present distance > 0, or +0 if there is none: a selection, its bits those of the operand;
 *   sigma  by bisection with lo = 0, hi = Inf, mid = 1 and target = log2(m + 1) (the fp32 nearest to the fp64 value), for at
 *          most VF_UMAP_SMOOTH_ITERS iterations: sum = over the present entries, in a butterfly over the lanes, of
 *          (d - rho > 0 ? exp(-((d - rho) / mid)) : 1); stop if |sum - target| < VF_UMAP_SMOOTH_TOL; if sum > target then
 *          hi = mid, mid = (lo + hi) / 2; else lo = mid and mid = (hi == Inf ? mid * 2 : (lo + hi) / 2).  sigma = mid, then
 *          the floor: sigma = max(sigma, VF_UMAP_MIN_SCALE * (rho > 0 ? the mean of the row's present distances : mean_dist));
 *   a row with no present entry: rho = +0, sigma = +0, every strength +0;
 *   strength[i, t] = +0 if the entry is absent or idx == i; 1 if d - rho <= 0 or sigma == 0; exp(-((d - rho) / sigma)) otherwise.
 * One wavefront per row, one lane per entry.
 * Non-finite operands: a NaN or infinite distance makes its entry absent, and the row is computed from the rest.  A NaN or
 * infinite mean_dist reaches sigma only through the floor of a row whose rho is 0 (a NaN never raises the floor).
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null idx, dist, rho, sigma
 * or strength; any of the five not 4-byte aligned; m outside 1 .. VF_UMAP_MAX_M; R < 0; R > VF_UMAP_MAX_R (2^24); ld_idx,
 * ld_dist or ld_strength < m.  R == 0 is VF_OK with nothing launched.
 * Not checked: that the lists are ascending (nothing here needs it) and that an index is below R (no index is used as an
 * address here). */
int vf_umap_smooth_knn(const int32_t* idx, int64_t ld_idx, const float* dist, int64_t ld_dist, int64_t R, int m, float mean_dist,
                       float* rho, float* sigma, float* strength, int64_t ld_strength, void* stream);

/* The fuzzy union over the symmetric graph (added under ABI 13): umap-learn's set_op_mix_ratio = 1.  The graph is given in CSR:
 * rowptr int64 [R + 1], col int32 [nnz]; entry e of row i (rowptr[i] <= e < rowptr[i + 1]) is the edge from i to j = col[e].
 * Arguments:
 *   idx       int32 [R, >= m], rows ld_idx apart;  strength  fp32 [R, >= m], rows ld_strength apart (what vf_umap_smooth_knn
 *             wrote);  R, m  as there;
 *   rowptr    int64 [R + 1];  col  int32 [nnz];  nnz  the entries;  w  fp32 [nnz].
 * Write set, exactly: w[e] for every e in [rowptr[i], rowptr[i + 1]) of every row i < R, clipped to [0, nnz).  Everything else
 * is only read.
 * Arithmetic: a = strength[i, t] at the first t < m with idx[i, t] == j, or +0 if there is none; b = strength[j, u] at the
 * first u < m with idx[j, u] == i, or +0; w[e] = (a + b) - a * b, each operation rounded once.  The entries (i, j) and (j, i)
 * see the same a and b with the names exchanged, and + and * commute: their w have the same bits.  One wavefront per row.
 * Non-finite operands: follow IEEE through the expression.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null idx, strength or
 * rowptr, a null col or w unless nnz == 0; idx, strength, col or w not 4-byte aligned, rowptr not 8-byte aligned; m outside
 * 1 .. VF_UMAP_MAX_M; R < 0; R > VF_UMAP_MAX_R; ld_idx or ld_strength < m; nnz < 0.  R == 0 or nnz == 0 is VF_OK with nothing
 * launched.
 * Not checked (the caller guarantees; variantformer_amd/manifold.py does): rowptr is non-decreasing from 0 to nnz, col holds
 * rows of the graph.  Input that is not valid stays inside the buffers: an e outside [0, nnz) is skipped, and a col[e] outside
 * [0, R) has b = +0. */
int vf_umap_union(const int32_t* idx, int64_t ld_idx, const float* strength, int64_t ld_strength, int64_t R, int m,
                  const int64_t* rowptr, const int32_t* col, int64_t nnz, float* w, void* stream);

/* The epochs [epoch_begin, epoch_end) of the layout (added under ABI 13), one kernel launch per epoch from a loop inside the
 * entry, the two position buffers exchanging roles: epoch epoch_begin reads Y0 and writes Y1, the next reads Y1 and writes Y0.
 * THE RESULT is in Y0 if epoch_end - epoch_begin is even and in Y1 if it is odd; the other buffer holds the positions one
 * epoch earlier.
 * Arguments:
 *   rowptr, col, nnz  the symmetric graph as in vf_umap_union;  samples  int32 [nnz]: how often entry e is drawn in N epochs,
 *                0 .. N (manifold.py: floor(fl(fl(w / w_max) * N)); the same for (i, j) and (j, i));
 *   R            vertices;  dim  coordinates, 1 .. VF_UMAP_MAX_DIM;  Y0, Y1  fp32 [R, >= dim], rows ld apart (64-bit offsets);
 *   epoch_begin, epoch_end, N   0 <= epoch_begin <= epoch_end <= N;
 *   a, b         the curve 1 / (1 + a * x^(2b));  gamma  the repulsion strength;  learning_rate  the first epoch's step;
 *   negative_sample_rate  repulsions per drawn entry, >= 0;  seed  of the negative vertices, its low 32 bits.
 * Write set, exactly: per epoch the output buffer's [i * ld + c] for 0 <= i < R, 0 <= c < dim: a vertex with nothing due, or
 * with no entry at all, has its row copied.  The input buffer of an epoch is only read during it; columns at or past dim are
 * never touched; rowptr, col and samples are only read.
 * Arithmetic: in epoch n vertex i starts from y = Yin[i] and walks its entries in order, s = e - rowptr[i] = 0, 1, ...; every
 * OTHER vertex is read from Yin, where it stood when the epoch began.  Entry e, to j = col[e], is DUE iff
 *   floor((n + 1) * samples[e] / N) > floor(n * samples[e] / N)      in 64-bit integers,
 * which draws it exactly samples[e] times in N epochs and needs no state.  With alpha = learning_rate * (1 - n / N) in fp32 and
 * clip(v) = v > 4 ? 4 : (v < -4 ? -4 : v), a due entry does, in this order:
 *   1. attraction:  d2 = sum_c (y[c] - Yin[j][c])^2 (c ascending);  g = d2 > 0 ? ((-2 * a * b) * (p / d2)) / (a * p + 1) : 0 with
 *      p = pow(d2, b);  y[c] += alpha * clip(g * (y[c] - Yin[j][c]));
 *   2. for p_ = 0 .. negative_sample_rate - 1:  k = (uint64(h) * R) >> 32 with
 *        h = mix(mix(mix(mix(mix(seed + 0x9E3779B9) ^ n) ^ i) ^ s) ^ p_),   all in uint32, and
 *        mix(x): x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16;
 *      d2 as above against Yin[k];  no move if d2 == 0 (k == i included, while y still stands on Yin[i]);  otherwise
 *      g = ((2 * gamma) * b) / ((0.001 + d2) * (a * pow(d2, b) + 1)) and y[c] += alpha * clip(g * (y[c] - Yin[k][c]));
 *   3. the attraction of step 1 once more, recomputed at the current y: vertex i's share as the tail of the mirrored entry
 *      (j, i), which has the same samples and is due in the same epochs.
 * Then Yout[i] = y.  One thread per vertex; no thread waits for another.
 * Non-finite operands: follow IEEE: a NaN coordinate of a vertex makes NaN whatever reads it (clip passes a NaN), and that
 * vertex's own row.  Finite positions stay finite: every move is at most 4 * alpha per coordinate.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null rowptr, Y0 or Y1, a
 * null col or samples unless nnz == 0; rowptr not 8-byte aligned, any other not 4-byte aligned; Y0 == Y1; R < 0;
 * R > VF_UMAP_MAX_R; nnz < 0; dim outside 1 .. VF_UMAP_MAX_DIM; ld < dim; N < 1; epoch_begin < 0; epoch_begin > epoch_end;
 * epoch_end > N; negative_sample_rate < 0.  R == 0 or an empty epoch range is VF_OK with nothing launched.
 * Not checked (the caller guarantees): rowptr is non-decreasing from 0 to nnz, samples are symmetric and in 0 .. N, Y0 and Y1
 * do not overlap.  Input that is not valid stays inside the buffers: an e outside [0, nnz), a col[e] outside [0, R) or a
 * samples[e] outside 1 .. N is never due. */
int vf_umap_layout(const int64_t* rowptr, const int32_t* col, const int32_t* samples, int64_t nnz, int64_t R, int dim, float* Y0,
                   float* Y1, int64_t ld, int epoch_begin, int epoch_end, int N, float a, float b, float gamma, float learning_rate,
                   int negative_sample_rate, int64_t seed, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_UMAP_H */

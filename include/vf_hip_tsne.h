/* vf_hip_tsne.h -- the entries of libvf_hip.so behind t-SNE with the EXACT gradient (what scikit-learn's
 * TSNE(method="exact") computes at O(R^2) memory on the host): the conditional probabilities of every row's neighbour list by
 * the perplexity search, their symmetric sum over the CSR graph, one all-pairs pass of the repulsive force over the embedding,
 * and the iterations of the descent.  Every sum has a stated order and there is no atomic, so two runs are equal bit for bit
 * and a run can be split at any iteration.  The stages are driven by variantformer_amd/manifold.py (tsne_affinities,
 * tsne_descent, tsne_kl, tsne), which also builds the symmetric graph's CSR arrays and normalises P with torch.
 *
 * The thirteenth header of the one library, beside vf_hip.h, vf_hip_attn_contrib.h, vf_hip_gene_contrib.h, vf_hip_cre_heads.h,
 * vf_hip_forest.h, vf_hip_topk.h, vf_hip_neighbors.h, vf_hip_linkage.h, vf_hip_umap.h, vf_hip_spectral.h,
 * vf_hip_umap_transform.h and vf_hip_components.h.  Its entries are bound through _lib.ENTRIES["vf_hip_tsne.h"], which _lib.load()
 * applies like the other twelve tables, and tests/tsne_cases.py holds their references and case table.  Everything the main
 * header says holds here: the conventions at its top (device pointers owned by the caller, `stream` a hipStream_t, strides in
 * elements, 0 = ok / VF_ERR_*, vf_last_error()), the comment contract of every entry (arguments, write set, arithmetic and its
 * order, non-finite operands, refusals, not checked), and the ABI version: a new symbol changes no existing one, so it stays 13.
 *
 * Nothing in this header's code is contracted into a fused multiply-add.  exp, log and sqrt are the compiler's fp32 library
 * functions and the pair kernel's reciprocal is the hardware's (1 ulp), so sums that go through them are held to fp64
 * restatements within bounds derived per case from an individually rounded fp32 restatement (tests/tsne_cases.py); every
 * selection (presence, the row minimum, the search's branch given its sum, inc / dec given its operands) and every integer is
 * exact, bit for bit.
 */
#ifndef VF_HIP_TSNE_H
#define VF_HIP_TSNE_H

#include "vf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the longest neighbour list: entry t lives on lane t mod 64 of one wavefront, at most four entries per lane */
#define VF_TSNE_MAX_M 255
/* the most rows: a vertex is an int32 and every fp32 count of rows is exact */
#define VF_TSNE_MAX_R (1 << 24)
/* the most output coordinates: a vertex's position and sums are held in registers */
#define VF_TSNE_MAX_DIM 4
/* the most splits of the all-pairs pass: the grid's second dimension */
#define VF_TSNE_MAX_SPLITS 65535
/* the perplexity search: scikit-learn's _binary_search_perplexity constants */
#define VF_TSNE_PERPLEXITY_STEPS 100
#define VF_TSNE_PERPLEXITY_TOL 1e-5f
/* rows of the embedding per block of the all-pairs pass, and per staged tile */
#define VF_TSNE_TILE 256
/* blocks, and threads per block, of the fp64 sum of Z */
#define VF_TSNE_Z_BLOCKS 64
#define VF_TSNE_Z_THREADS 256
/* bytes of vf_tsne_descent's workspace: VF_TSNE_Z_BLOCKS fp64, then part fp32 [splits, R, dim + 1], then attr fp32 [R, dim] */
#define VF_TSNE_WORK_BYTES(R, dim, splits) \
    (8 * (int64_t)VF_TSNE_Z_BLOCKS + 4 * ((int64_t)(splits) * (int64_t)(R) * ((dim) + 1) + (int64_t)(R) * (dim)))

/* Conditional probabilities of every row's neighbour list (added under ABI 13): scikit-learn's _binary_search_perplexity.
 * Arguments:
 *   idx         int32 [R, >= m], rows ld_idx apart, and  d2  fp32 [R, >= m], rows ld_d2 apart (64-bit offsets): the m rows
 *               nearest to each row and their SQUARED distances;  R  rows;  m  entries per row, 1 .. VF_TSNE_MAX_M;
 *   perplexity  fp32, 1 <= perplexity < m;
 *   beta        fp32 [R];  p_cond  fp32 [R, >= m], rows ld_p apart.
 * An entry is ABSENT if its index is negative or its distance is NaN, +Inf or -Inf (vf_umap_smooth_knn's rule); an entry with
 * idx == i is left out as well (scikit-learn skips the diagonal).  Every other entry is present.  An entry that is not
 * present contributes to nothing below and gets p_cond = +0.
 * Write set, exactly: beta[i] and p_cond[i * ld_p + t] for 0 <= i < R, 0 <= t < m.  idx and d2 are only read, once, at [i, t]
 * with t < m.
 * Arithmetic, per row, in fp32, every operation rounded once:
 *   dmin = the smallest present d2: a selection;  x_t = d2_t - dmin.  THE ONE DEVIATION from scikit-learn: in exact arithmetic
 *   it changes neither P nor the entropy, and it keeps exp from underflowing in fp32;
 *   target = log(perplexity), the fp32 nearest to the fp64 value;  beta = 1, beta_min = -Inf, beta_max = +Inf;
 *   for at most VF_TSNE_PERPLEXITY_STEPS steps:  e_t = exp(-(x_t * beta));  S = sum e_t;  P_t = e_t / S;  D = sum x_t * P_t;
 *     H = log(S) + beta * D;  diff = H - target;  stop if |diff| <= VF_TSNE_PERPLEXITY_TOL;  after the last step stop too;
 *     if diff > 0: beta_min = beta, beta = (beta_max == +Inf ? beta * 2 : (beta + beta_max) / 2);
 *     else:        beta_max = beta, beta = (beta_min == -Inf ? beta / 2 : (beta + beta_min) / 2);
 *   beta[i] = the beta of the last evaluation and p_cond[i, t] = its P_t (scikit-learn leaves P there, too).
 *   Order of both sums: one wavefront per row, entry t on lane t mod 64, held in registers across the search; each lane adds
 *   its entries in ascending t from +0, then a butterfly over the lanes (xor 32, 16, .. 1), so every lane holds the same bits
 *   and the branches are uniform.  S >= 1 always: the row's minimum has e = 1.
 *   A row with no present entry: beta = +0 and every p_cond +0.  A row whose present d2 are all equal has H = log(count)
 *   whatever beta is: the search runs all its steps, beta ends at 2^99 or 2^-99, finite, and P is uniform.
 * Non-finite operands: a NaN or infinite distance makes its entry absent, and the row is computed from the rest.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null idx, d2, beta or
 * p_cond; any of the four not 4-byte aligned; m outside 1 .. VF_TSNE_MAX_M; R < 0; R > VF_TSNE_MAX_R (2^24); ld_idx, ld_d2 or
 * ld_p < m; perplexity not finite, < 1 or >= m (the entropy target would be unreachable).  R == 0 is VF_OK with nothing
 * launched.
 * Not checked: that the lists are ascending (nothing here needs it), that an index is below R (no index is used as an address
 * here), that d2 >= 0. */
int vf_tsne_perplexity(const int32_t* idx, int64_t ld_idx, const float* d2, int64_t ld_d2, int64_t R, int m, float perplexity,
                       float* beta, float* p_cond, int64_t ld_p, void* stream);

/* The symmetric sum over the graph (added under ABI 13): scikit-learn's P = conditional_P + conditional_P.T, before its
 * normalisation.  The sibling of vf_umap_union: the graph is given in CSR, rowptr int64 [R + 1], col int32 [nnz]; entry e of
 * row i (rowptr[i] <= e < rowptr[i + 1]) is the edge from i to j = col[e].
 * Arguments:
 *   idx       int32 [R, >= m], rows ld_idx apart;  p_cond  fp32 [R, >= m], rows ld_p apart (what vf_tsne_perplexity wrote);
 *             R, m  as there;
 *   rowptr    int64 [R + 1];  col  int32 [nnz];  nnz  the entries;  p  fp32 [nnz].
 * Write set, exactly: p[e] for every e in [rowptr[i], rowptr[i + 1]) of every row i < R, clipped to [0, nnz).  Everything else
 * is only read.
 * Arithmetic: a = p_cond[i, t] at the first t < m with idx[i, t] == j, or +0 if there is none; b = p_cond[j, u] at the first
 * u < m with idx[j, u] == i, or +0; p[e] = a + b, rounded once.  The entries (i, j) and (j, i) see the same a and b with the
 * names exchanged, and + commutes: their p have the same bits.  One wavefront per row.
 * The normalisation P /= max(sum P, eps) is NOT part of this contract: manifold.py does it with torch, the sum in fp64 and one
 * fp32 division per entry.
 * Non-finite operands: follow IEEE through the expression.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null idx, p_cond or
 * rowptr, a null col or p unless nnz == 0; idx, p_cond, col or p not 4-byte aligned, rowptr not 8-byte aligned; m outside
 * 1 .. VF_TSNE_MAX_M; R < 0; R > VF_TSNE_MAX_R; ld_idx or ld_p < m; nnz < 0.  R == 0 or nnz == 0 is VF_OK with nothing
 * launched.
 * Not checked (the caller guarantees; variantformer_amd/manifold.py does): rowptr is non-decreasing from 0 to nnz, col holds
 * rows of the graph.  Input that is not valid stays inside the buffers: an e outside [0, nnz) is skipped, and a col[e] outside
 * [0, R) has b = +0. */
int vf_tsne_joint(const int32_t* idx, int64_t ld_idx, const float* p_cond, int64_t ld_p, int64_t R, int m, const int64_t* rowptr,
                  const int32_t* col, int64_t nnz, float* p, void* stream);

/* One all-pairs pass of the repulsive force over the embedding (added under ABI 13): the Q side of scikit-learn's exact
 * gradient in its (P - Q) * dist form, without the R x R matrix.
 * Arguments:
 *   Y       fp32 [R, >= dim], rows ld apart (64-bit offsets);  R  vertices;  dim  coordinates, 1 .. VF_TSNE_MAX_DIM;
 *   dof     1, 2 or 3: scikit-learn's max(n_components - 1, 1);  splits  1 .. VF_TSNE_MAX_SPLITS;
 *   part    fp32 [splits, R, dim + 1], contiguous.
 * Write set, exactly: part[(s * R + i) * (dim + 1) + c] for 0 <= s < splits, 0 <= i < R, 0 <= c <= dim.  Y is only read, at
 * [j, c] with c < dim.
 * Arithmetic: split s covers the rows j in [min(s * L, R), min((s + 1) * L, R)) with L = ceil(R / splits): a function of
 * (R, splits) alone.  For vertex i and split s, over j ascending in that range, j == i skipped BY INDEX (not by distance),
 * every sum one running fp32 sum from +0 and every operation rounded once:
 *   d2 = sum_c (y_i[c] - y_j[c])^2 (c ascending);  q = d2 for dof 1, d2 * 0.5 for dof 2, d2 * fl(1 / 3) for dof 3;
 *   t = rcp(1 + q), the hardware reciprocal (1 ulp);  w = t, t * sqrt(t), t * t for dof 1, 2, 3: t^((dof + 1) / 2), no pow;
 *   part[s, i, c] += (w * w) * (y_i[c] - y_j[c]) for c < dim;  part[s, i, dim] += w.
 * A split with an empty range writes +0.  Coincident points have d2 = 0, t = 1 exactly, w = 1 and a zero force.  A vertex's
 * row depends on Y[0 .. R), R and splits alone: not on the grid, on ld or on its place in a block.  One thread per vertex and
 * split, VF_TSNE_TILE vertices per block; the rows j come VF_TSNE_TILE at a time through LDS, where every lane reads the same
 * address (a broadcast).  No atomic.
 * Non-finite operands: follow IEEE: a NaN coordinate of row j makes NaN the row [s, i, :] of every i whose split s holds j,
 * and all of vertex j's own rows; nothing else.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null Y or part; either not
 * 4-byte aligned; R < 0; R > VF_TSNE_MAX_R; dim outside 1 .. VF_TSNE_MAX_DIM; ld < dim; dof outside 1 .. 3; splits outside
 * 1 .. VF_TSNE_MAX_SPLITS.  R == 0 is VF_OK with nothing launched.
 * Not checked: that Y and part do not overlap. */
int vf_tsne_repulsion(const float* Y, int64_t ld, int64_t R, int dim, int dof, int splits, float* part, void* stream);

/* The iterations [iter_begin, iter_end) of the descent (added under ABI 13): scikit-learn's _gradient_descent over its
 * _kl_divergence, from one loop inside the entry, four kernel launches per iteration.
 * Arguments:
 *   rowptr, col, nnz  the symmetric graph as in vf_tsne_joint;  p  fp32 [nnz]: the NORMALISED joint probabilities;
 *   R  vertices;  dim  1 .. VF_TSNE_MAX_DIM;  Y, update, gains  fp32 [R, >= dim], all three with rows ld apart: the state;
 *   iter_begin, iter_end  0 <= iter_begin <= iter_end (only their difference enters the arithmetic);
 *   exaggeration, momentum, learning_rate, min_gain  fp32, per call;  dof  1 .. 3;  splits  as in vf_tsne_repulsion;
 *   work  the caller's workspace, 8-byte aligned, of work_bytes >= VF_TSNE_WORK_BYTES(R, dim, splits) bytes;
 *   zsum  fp64 [iter_end - iter_begin]: the Z of each iteration, returned.
 * Write set, exactly: Y, update and gains at [i * ld + c] for 0 <= i < R, 0 <= c < dim; zsum[n - iter_begin] for every
 * iteration n; the first VF_TSNE_WORK_BYTES(R, dim, splits) bytes of work, whose content afterwards is not part of the
 * contract.  rowptr, col and p are only read; columns at or past dim are never touched.
 * Arithmetic, per iteration, fp32 with every operation rounded once unless fp64 is named:
 *   1. part = vf_tsne_repulsion(Y, dof, splits), bit for bit;
 *   2. attr[i, c] = sum over the entries e of row i IN ENTRY ORDER, one running sum from +0, of (p[e] * w_e) * (y_i[c] - y_j[c])
 *      with j = col[e] and w_e as in vf_tsne_repulsion (an entry with j == i contributes like any other: its difference is 0);
 *      an e outside [0, nnz) or a col[e] outside [0, R) is skipped;
 *   3. Z in fp64: the column-dim values of part, k = s * R + i, are cut into VF_TSNE_Z_BLOCKS chunks of
 *      C = ceil(splits * R / VF_TSNE_Z_BLOCKS) consecutive k; in chunk b thread u of VF_TSNE_Z_THREADS adds k = b * C + u,
 *      + VF_TSNE_Z_THREADS, .. ascending from +0, the threads' sums are added by a tree (stride 128, 64, .. 1: x[u] += x[u + stride]),
 *      and Z = the chunks' sums added in ascending b from +0.  zsum[n - iter_begin] = Z;
 *   4. element-wise, the only step that writes Y, every thread reading its own element alone:
 *      rep = sum_s part[s, i, c] in ascending s from +0;  grad = G * (exaggeration * attr - rep / fl(Z)) with
 *      G = fl(2 (dof + 1) / dof) and fl(Z) the fp32 nearest to Z;  then scikit-learn's _gradient_descent:
 *      inc = update * grad < 0;  gains = inc ? gains + 0.2f : gains * 0.8f;  gains = gains < min_gain ? min_gain : gains;
 *      grad = grad * gains;  update = momentum * update - learning_rate * grad;  Y = Y + update.
 *      update * grad == 0 (or NaN) goes to dec, as numpy's invert of the comparison does.
 * No kernel reads a position that another thread of the same launch writes: steps 1 to 3 write the workspace and zsum only.
 * The result depends on the arguments alone: [0, 20) equals [0, 7) then [7, 20) on the carried state, bit for bit.
 * Non-finite operands: follow IEEE through the expressions (a NaN gain is not floored).  R == 1 has Z = 0 and rep / Z = NaN.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null rowptr, Y, update,
 * gains, work or zsum (zsum may be null if the iteration range is empty), a null col or p unless nnz == 0; rowptr, work or zsum
 * not 8-byte aligned, any other not 4-byte aligned; R < 0; R > VF_TSNE_MAX_R; nnz < 0; dim outside 1 .. VF_TSNE_MAX_DIM;
 * ld < dim; dof outside 1 .. 3; splits outside 1 .. VF_TSNE_MAX_SPLITS; iter_begin < 0; iter_begin > iter_end; work_bytes
 * below VF_TSNE_WORK_BYTES(R, dim, splits).  R == 0 or an empty iteration range is VF_OK with nothing launched and nothing
 * written; nnz == 0 runs with attr = +0.
 * Not checked (the caller guarantees): rowptr is non-decreasing from 0 to nnz, p is symmetric, Y, update, gains, work and
 * zsum do not overlap. */
int vf_tsne_descent(const int64_t* rowptr, const int32_t* col, const float* p, int64_t nnz, int64_t R, int dim, float* Y,
                    float* update, float* gains, int64_t ld, int iter_begin, int iter_end, float exaggeration, float momentum,
                    float learning_rate, float min_gain, int dof, int splits, void* work, int64_t work_bytes, double* zsum,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_TSNE_H */

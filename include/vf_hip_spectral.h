/* vf_hip_spectral.h -- the entries of libvf_hip.so behind the spectral embedding of a symmetric graph (what umap-learn's default
 * init="spectral" starts from): the eigenvectors of the normalised Laplacian L = I - D^-1/2 W D^-1/2 for its smallest eigenvalues,
 * found by Chebyshev-filtered subspace iteration in the normalised adjacency S = D^-1/2 W D^-1/2.  The graph is the CSR graph of
 * vf_hip_umap.h (rowptr int64 [R + 1], col int32 [nnz], w fp32 [nnz]).  Four entries: the degrees, `steps` steps of a three-term
 * recurrence in S over a block of vectors (the filter, and with one step the plain product S Y), the fp64 Gram matrix of two
 * tall blocks, and a tall block times a small fp64 matrix.  They are driven by variantformer_amd/manifold.py (spectral_embedding),
 * which does the p x p eigenproblems in fp64 on the host.
 *
 * The tenth header of the one library, beside vf_hip.h, vf_hip_attn_contrib.h, vf_hip_gene_contrib.h, vf_hip_cre_heads.h,
 * vf_hip_forest.h, vf_hip_topk.h, vf_hip_neighbors.h, vf_hip_linkage.h and vf_hip_umap.h.  Its entries are bound through
 * _lib.ENTRIES["vf_hip_spectral.h"], which _lib.load() applies like the other nine tables, and tests/spectral_cases.py holds their
 * references and case table.  Everything the main header says holds here: the conventions at its top (device pointers owned by
 * the caller, `stream` a hipStream_t, strides in elements, 0 = ok / VF_ERR_*, vf_last_error()), the comment contract of every
 * entry (arguments, write set, arithmetic, non-finite operands, refusals), and VF_ABI_VERSION: a new symbol changes no existing
 * one, so the version stays 13.
 *
 * Nothing in this header's code is contracted into a fused multiply-add: every fp32 and fp64 operation below is rounded once, on
 * its own, `/` and sqrt are the correctly rounded ones, and every sum has the order stated with its entry.  No entry uses an
 * atomic and no block waits for another, so two runs give the same bits and numpy restates them (tests/spectral_cases.py).
 */
#ifndef VF_HIP_SPECTRAL_H
#define VF_HIP_SPECTRAL_H

#include "vf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most vertices, as VF_UMAP_MAX_R */
#define VF_SPECTRAL_MAX_R (1 << 24)
/* the widest block of vectors */
#define VF_SPECTRAL_MAX_P 32
/* vf_tall_gram: the most per-block partials, and the rows of one LDS tile; its workspace holds at most
 * VF_TALL_GRAM_MAX_BLOCKS * p * q doubles */
#define VF_TALL_GRAM_MAX_BLOCKS 1024
#define VF_TALL_GRAM_TILE 64

/* The weighted degree of every vertex and its inverse square root (added under ABI 13).
 * Arguments:
 *   rowptr int64 [R + 1], col int32 [nnz], w fp32 [nnz]   the graph in CSR (col is not read: the degree needs the weights alone);
 *   nnz  the entries;  R  the vertices;  deg, dinv_sqrt  fp32 [R].
 * Write set, exactly: deg[i] and dinv_sqrt[i] for 0 <= i < R.  rowptr and w are only read.
 * Arithmetic, per row i, in fp32: one wavefront per row; lane l (0 .. 63) starts from +0 and adds w[e] for
 * e = rowptr[i] + l, rowptr[i] + l + 64, ... below rowptr[i + 1], ascending; the 64 lane sums v are then combined in a butterfly,
 * v[l] = v[l] + v[l ^ off] for off = 32, 16, 8, 4, 2, 1 in this order (every lane ends with the same bits); deg[i] is that sum.
 *   dinv_sqrt[i] = deg[i] > 0 ? 1 / sqrt(deg[i]) : +0     (two correctly rounded operations).
 * A row without entries gets +0 and +0.
 * Non-finite operands: follow IEEE through the sum; a NaN or non-positive degree has dinv_sqrt +0, a degree of +Inf has +0 too
 * (1 / Inf).
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null rowptr, deg or
 * dinv_sqrt, a null col or w unless nnz == 0; rowptr not 8-byte aligned, any other not 4-byte aligned; R < 0;
 * R > VF_SPECTRAL_MAX_R (2^24); nnz < 0.  R == 0 is VF_OK with nothing launched.
 * Not checked (the caller guarantees): rowptr is non-decreasing from 0 to nnz.  Input that is not valid stays inside the
 * buffers: an e outside [0, nnz) is skipped. */
int vf_graph_degree(const int64_t* rowptr, const int32_t* col, const float* w, int64_t nnz, int64_t R, float* deg, float* dinv_sqrt,
                    void* stream);

/* `steps` steps of a three-term recurrence in S = D^-1/2 W D^-1/2 over a block of p vectors (added under ABI 13), one kernel
 * launch per step from a loop inside the entry, three buffers exchanging roles.
 *
 * >>> `coef` IS A HOST POINTER -- the one host pointer among this header's device pointers: steps x 3 floats in host memory,   <<<
 * >>> read completely before the entry returns (each step's three values travel as kernel arguments), so the caller may free  <<<
 * >>> or overwrite it as soon as the call is back.  Passing a device pointer here is a fault on the host.                      <<<
 *
 * Arguments:
 *   rowptr, col, w, nnz, R   the graph as in vf_graph_degree;  dinv_sqrt  fp32 [R], what vf_graph_degree wrote;
 *   p            the vectors of the block, 1 .. VF_SPECTRAL_MAX_P;
 *   X0, X1, X2   fp32 [R, >= p], rows ld apart (64-bit offsets), pairwise distinct and not overlapping;
 *   steps        >= 0;  coef  HOST fp32 [steps, 3].
 * Step t = 0 .. steps - 1 reads Y = X[t mod 3] (the newest block) and W = X[(t + 2) mod 3] (the one before it) and overwrites
 * the oldest, Z = X[(t + 1) mod 3]:
 *   Z = coef[t][0] * (S Y) + coef[t][1] * Y + coef[t][2] * W.
 * On entry X0 holds the newest block and X2 the one before it (read only if coef[0][2] != 0).  THE RESULT is in X0 if
 * steps mod 3 == 0, in X1 if steps mod 3 == 1 and in X2 if steps mod 3 == 2; steps == 0 launches nothing.  Coefficients
 * (1, 0, 0) with steps = 1 give the plain product X1 = S X0.
 * Write set, exactly: per step Z[i * ld + c] for 0 <= i < R, 0 <= c < p.  Columns at or past p are never touched; a step's Y
 * and W are only read during it; rowptr, col, w and dinv_sqrt are only read.
 * Arithmetic, per row i, in fp32, every operation rounded once.  Let C be the smallest power of two >= p and G = 64 / C.  One
 * wavefront per row; lane l holds column c = l mod C for the entry group g = l / C (lanes with c >= p idle).  Group g starts
 * from +0 and takes the entries e = rowptr[i] + g, rowptr[i] + g + G, ... below rowptr[i + 1], ascending:
 *   acc = acc + (w[e] * dinv_sqrt[col[e]]) * Y[col[e], c];
 * the G group sums of a column are then combined in a butterfly, v[g] = v[g] + v[g ^ off] for off = G / 2, G / 4, ..., 1 in this
 * order, and (S Y)[i, c] = dinv_sqrt[i] * v.  Then, with a = coef[t][0] * (S Y)[i, c], b = coef[t][1] * Y[i, c] and
 * d = coef[t][2] * W[i, c]:  Z[i, c] = (a + b) + d, in which A TERM WHOSE COEFFICIENT IS EXACTLY 0 (+0 or -0) IS SKIPPED, not
 * multiplied: its operand is not read and cannot bring a NaN or an Inf into the result (with coef[t][0] == 0 the row's entries
 * are not walked at all); the remaining terms are added in the same order, and with all three skipped Z[i, c] = +0.
 * Non-finite operands: follow IEEE through the terms that are not skipped; a NaN coefficient is not 0, so its term is NaN.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null rowptr, dinv_sqrt,
 * X0, X1 or X2, a null col or w unless nnz == 0, a null coef unless steps == 0; rowptr not 8-byte aligned, any other device
 * pointer not 4-byte aligned; X0, X1, X2 not pairwise distinct; R < 0; R > VF_SPECTRAL_MAX_R; nnz < 0; p outside
 * 1 .. VF_SPECTRAL_MAX_P; ld < p; steps < 0.  R == 0 or steps == 0 is VF_OK with nothing launched.
 * Not checked (the caller guarantees): rowptr is non-decreasing from 0 to nnz, the three buffers do not overlap.  Input that is
 * not valid stays inside the buffers: an e outside [0, nnz) or a col[e] outside [0, R) is skipped. */
int vf_spmm_recur(const int64_t* rowptr, const int32_t* col, const float* w, int64_t nnz, int64_t R, const float* dinv_sqrt, int p,
                  float* X0, float* X1, float* X2, int64_t ld, int steps, const float* coef, void* stream);

/* G = A^T B in fp64 for two tall fp32 blocks (added under ABI 13): X^T X, X^T (S X) and the residual norms of the solver.
 * Arguments:
 *   A  fp32 [R, >= p], rows lda apart;  B  fp32 [R, >= q], rows ldb apart (64-bit offsets; A and B may be one buffer);
 *   R  rows;  p, q  1 .. VF_SPECTRAL_MAX_P;  G  fp64 [p, q], row-major, contiguous;
 *   work  fp64 workspace of the caller's, at least nb * p * q doubles with nb = ceil(R / chunk),
 *         chunk = VF_TALL_GRAM_TILE * ceil(R / (VF_TALL_GRAM_TILE * VF_TALL_GRAM_MAX_BLOCKS)) rows (nb = 0 for R == 0);
 *         VF_TALL_GRAM_MAX_BLOCKS * p * q doubles always suffice.
 * Write set, exactly: G[a * q + b] for a < p, b < q, and work[0 .. nb * p * q).  A and B are only read.
 * Arithmetic, in fp64, two stages of fixed order: block k forms, for every (a, b), the partial
 *   work[(k * p + a) * q + b] = sum over its rows r = k * chunk .. min(R, (k + 1) * chunk) - 1, ascending, from +0, of
 *   (double)A[r, a] * (double)B[r, b]        (the product of two fp32 values is exact in fp64; each addition is rounded once);
 * then one block sums the partials of every (a, b) over k = 0 .. nb - 1, ascending, from +0, into G.  R == 0 gives G = +0.
 * Non-finite operands: follow IEEE through the sums.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null A, B, G or work; A or B
 * not 4-byte aligned, G or work not 8-byte aligned; R < 0; R > VF_SPECTRAL_MAX_R; p or q outside 1 .. VF_SPECTRAL_MAX_P;
 * lda < p; ldb < q.
 * Not checked (the caller guarantees): work is as large as stated, G and work overlap nothing else. */
int vf_tall_gram(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t R, int p, int q, double* G, double* work,
                 void* stream);

/* Out = X T for a tall fp32 block and a small fp64 matrix (added under ABI 13): the rotation X Q of Rayleigh-Ritz and the
 * orthonormalisation X T of the solver, with the sum held in fp64.
 * Arguments:
 *   X  fp32 [R, >= p], rows ldx apart;  T  fp64 [p, q], row-major, contiguous, on the device;  p, q  1 .. VF_SPECTRAL_MAX_P;
 *   Out  fp32 [R, >= q], rows ldo apart (64-bit offsets), not overlapping X.
 * Write set, exactly: Out[i * ldo + c] for 0 <= i < R, 0 <= c < q.  X and T are only read.
 * Arithmetic: one thread per output element; s = +0 in fp64, then s = s + (double)X[i, k] * T[k, c] for k = 0 .. p - 1 ascending
 * (the product and the sum each rounded once, in fp64); Out[i, c] = (float)s, rounded to nearest even.  A column of T that is a
 * unit vector therefore copies a column of X bit for bit (as long as the other columns of X are finite).
 * Non-finite operands: follow IEEE: 0 * Inf and 0 * NaN are NaN, so a non-finite X[i, k] reaches every column of row i.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null X, T or Out; X or Out
 * not 4-byte aligned, T not 8-byte aligned; Out == X; R < 0; R > VF_SPECTRAL_MAX_R; p or q outside 1 .. VF_SPECTRAL_MAX_P;
 * ldx < p; ldo < q.  R == 0 is VF_OK with nothing launched.
 * Not checked (the caller guarantees): Out and X do not overlap. */
int vf_tall_mul(const float* X, int64_t ldx, int64_t R, int p, const double* T, int q, float* Out, int64_t ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_SPECTRAL_H */

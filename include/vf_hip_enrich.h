/* vf_hip_enrich.h -- the entries of libvf_hip.so behind the enrichment of gene clusters in annotation terms (GO terms within the
 * clusters of a UMAP picture or of a cut Ward tree): for every (term, cluster) pair the size of their overlap, and the tail of
 * the hypergeometric distribution at that overlap -- what scipy.stats.hypergeom.sf(x - 1, N, K, n) / .cdf(x, N, K, n) computes
 * on the host, one cell at a time.  The counts are integers and the tail is a sum with a stated order in fp64 + * / alone, so
 * two runs are equal bit for bit and a call can be split at any term.  The stages are driven by variantformer_amd/enrichment.py
 * (membership, hypergeom, enrich), which builds the CSR arrays and the table of log-factorials on the host and does the
 * Benjamini-Hochberg step with torch.
 *
 * The fourteenth header of the one library, beside vf_hip.h, vf_hip_attn_contrib.h, vf_hip_gene_contrib.h, vf_hip_cre_heads.h,
 * vf_hip_forest.h, vf_hip_topk.h, vf_hip_neighbors.h, vf_hip_linkage.h, vf_hip_umap.h, vf_hip_spectral.h,
 * vf_hip_umap_transform.h, vf_hip_components.h and vf_hip_tsne.h.  Its entries are bound through _lib.ENTRIES["vf_hip_enrich.h"], which
 * _lib.load() applies like the other thirteen tables, and tests/enrich_cases.py holds their references and case table.
 * Everything the main header says holds here: the conventions at its top (device pointers owned by the caller, `stream` a
 * hipStream_t, strides in elements, 0 = ok / VF_ERR_*, vf_last_error()), the comment contract of every entry (arguments, write
 * set, arithmetic and its order, non-finite operands, refusals, not checked), and the ABI version: a new symbol changes no
 * existing one, so it stays 13.
 *
 * Nothing in this header's code is contracted into a fused multiply-add.  The device computes no lgamma: the host hands it
 * logfact[i] = lgamma(i + 1).  Up to the last step every operation is an fp64 + * / (each correctly rounded) or a comparison on
 * values numpy holds too, so `tail` and `steps` are restated bit for bit; log, exp and log1p are the compiler's fp64 library
 * functions, and log_p is held to the restatement within a few ulp (tests/enrich_cases.py).  The only atomics are integer
 * additions on LDS words in vf_enrich_counts: integer addition is associative, so the counts do not depend on their order.
 */
#ifndef VF_HIP_ENRICH_H
#define VF_HIP_ENRICH_H

#include "vf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most clusters: one int32 LDS bin per cluster and block, 16 KiB.  A larger k is refused, not served in panels */
#define VF_ENRICH_MAX_K 4096
/* the largest universe: every product of two counts is below 2^48 and an exact fp64 integer */
#define VF_ENRICH_MAX_N (1 << 24)
/* the most terms of one call: the grid's first dimension, one block per term */
#define VF_ENRICH_MAX_T (1 << 24)
/* threads per block of vf_enrich_counts (one block per term) and of vf_hypergeom_tail (one thread per cell) */
#define VF_ENRICH_THREADS 256
/* a sum stops after the term t with t < s * VF_ENRICH_STOP: 2^-60 */
#define VF_ENRICH_STOP 0x1p-60

/* Overlap counts of every (term, cluster) pair, and every term's size inside the universe (added under ABI 13).
 * The annotation is term-major CSR: termptr int64 [T + 1], gene int32 [nnz]; entry e of term t (termptr[t] <= e <
 * termptr[t + 1]) is the universe row gene[e].  The clustering is labels int32 [G]: a value in 0 .. k - 1 names a cluster, any
 * other value means "in the universe, in no cluster".
 * Arguments:
 *   termptr, gene, nnz  as above;  T  terms;  labels, G  as above;  k  clusters, 1 .. VF_ENRICH_MAX_K;
 *   count   int32 [T, >= k], rows ldc apart (64-bit offsets);  size  int32 [T].
 * Write set, exactly: count[t * ldc + c] for 0 <= t < T, 0 <= c < k, and size[t] for 0 <= t < T.  termptr, gene and labels are
 * only read; columns of count at or past k are never touched.
 * Arithmetic: integers.  size[t] = the number of entries e of term t, clipped to [0, nnz), with 0 <= gene[e] < G: an entry
 * outside the universe is skipped, which is how genes outside it are dropped.  count[t, c] = the number of those entries with
 * labels[gene[e]] == c.  A gene whose label is outside 0 .. k - 1 counts towards size[t] and towards no cluster.  A term
 * without entries writes zeros.  One block of VF_ENRICH_THREADS threads per term: the threads take the term's entries
 * VF_ENRICH_THREADS at a time and add 1 to the cluster's bin of a k-bin histogram in LDS with an integer LDS atomic; each
 * thread counts its in-universe entries in a register and adds them to one more LDS word with one integer atomic; after a
 * barrier the bins are stored.  No global atomic, no floating-point atomic: the result is exact whatever the order.
 * The cluster sizes are this entry called with T = 1 and one term that lists every gene: termptr = {0, G}, gene = 0 .. G - 1.
 * Non-finite operands: there are none: every operand is an integer.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null termptr, labels,
 * count or size, a null gene unless nnz == 0; termptr not 8-byte aligned, gene, labels, count or size not 4-byte aligned;
 * nnz < 0; T < 0; T > VF_ENRICH_MAX_T (2^24); G < 0; G > VF_ENRICH_MAX_N (2^24); k outside 1 .. VF_ENRICH_MAX_K; ldc < k.
 * T == 0 is VF_OK with nothing launched.  (labels may be any non-null aligned address when G == 0: nothing reads it.)
 * Not checked (the caller guarantees; variantformer_amd/enrichment.py does): termptr is non-decreasing from 0 to nnz; a term
 * lists a gene once (a gene listed twice is counted twice).  Input that is not valid stays inside the buffers: an e outside
 * [0, nnz) is skipped. */
int vf_enrich_counts(const int64_t* termptr, const int32_t* gene, int64_t nnz, int64_t T, const int32_t* labels, int64_t G, int k,
                     int32_t* count, int64_t ldc, int32_t* size, void* stream);

/* The hypergeometric tail of every cell (added under ABI 13): for x = count[t, c], K = size[t], n = csize[c] and the universe
 * N, the natural logarithm of P[X >= x] (alternative 0, "greater": scipy's hypergeom.sf(x - 1, N, K, n)) or of P[X <= x]
 * (alternative 1, "less": hypergeom.cdf(x, N, K, n)), X the overlap of n genes drawn without replacement from N of which K
 * belong to the term.  The logarithm never underflows.
 * Arguments:
 *   count    int32 [T, >= k], rows ldc apart;  size  int32 [T];  csize  int32 [k];  T, k  as in vf_enrich_counts;
 *   N        the universe, 0 .. VF_ENRICH_MAX_N;  logfact  fp64 [N + 1], logfact[i] = lgamma(i + 1), computed by the host;
 *   alternative  0 or 1;
 *   log_p, tail  fp64 [T, >= k] and  steps  int32 [T, >= k], all three with rows ldo apart.
 * Write set, exactly: log_p, tail and steps at [t * ldo + c] for 0 <= t < T, 0 <= c < k.  count, size, csize and logfact are
 * only read: count at [t, c] with c < k, logfact at the nine places below.
 * Arithmetic, per cell, one thread each; int64 for the integers, fp64 with every operation rounded once for the rest:
 *   lo = max(0, n - (N - K));  hi = min(K, n);  mode = ((n + 1) * (K + 1)) div (N + 2).
 *   sum_up(x0):    t = s = 1, steps = 0;  for i = x0, x0 + 1, .. while i < hi:
 *                    t = (t * double((K - i) * (n - i))) / double((i + 1) * (N - K - n + i + 1));  s = s + t;  steps += 1;
 *                    stop after the term with t < s * VF_ENRICH_STOP.
 *   sum_down(x0):  the same for i = x0, x0 - 1, .. while i > lo with
 *                    t = (t * double(i * (N - K - n + i))) / double((K - i + 1) * (n - i + 1)).
 *   Both integer products are formed in int64 (exact, below 2^48) and converted exactly.  A sum always runs AWAY from the mode:
 *   the distribution is unimodal, every ratio is <= 1, s <= steps + 1, nothing overflows and no divisor is 0.
 *   L(x0) = (a + b) - c with  a = (logfact[K] - logfact[x0]) - logfact[K - x0],
 *                             b = (logfact[N - K] - logfact[n - x0]) - logfact[N - K - n + x0],
 *                             c = (logfact[N] - logfact[n]) - logfact[N - n]:  the log of the probability of x0.
 *   "greater":  x > hi: log_p = -Inf;  else x <= lo: log_p = +0 exactly (p = 1);  else x > mode: log_p = L(x) + log(sum_up(x));
 *               else log_p = log1p(-exp(L(x - 1) + log(sum_down(x - 1)))).
 *   "less":     x < lo: log_p = -Inf;  else x >= hi: log_p = +0 exactly;  else x < mode: log_p = L(x) + log(sum_down(x));
 *               else log_p = log1p(-exp(L(x + 1) + log(sum_up(x + 1)))).
 *   The first matching case holds.  tail = the s of the cell's sum and steps its count of added terms; a cell without a sum
 *   (the -Inf and +0 cases) has tail = +0 and steps = 0.  K == 0 or n == 0 has lo = hi = 0 and falls under these cases:
 *   p = 1 at x = 0.  A complement's argument is at most 1 - 1 / (hi - lo + 1): the side that holds the mode is left out.
 * Non-finite operands: logfact is read as it is and a NaN or Inf in one of the nine places follows IEEE into log_p; tail and
 * steps do not depend on logfact.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null count, size, csize,
 * logfact, log_p, tail or steps; logfact, log_p or tail not 8-byte aligned, count, size, csize or steps not 4-byte aligned;
 * T < 0; T > VF_ENRICH_MAX_T; k outside 1 .. VF_ENRICH_MAX_K; N < 0; N > VF_ENRICH_MAX_N (2^24); ldc < k; ldo < k; alternative
 * not 0 or 1.  T == 0 is VF_OK with nothing launched.
 * Not checked (the caller guarantees; vf_enrich_counts delivers it): 0 <= K <= N, 0 <= n <= N.  Input that is not valid stays
 * inside the buffers: a cell whose K or n is outside 0 .. N gets log_p = tail = NaN and steps = 0 and reads nothing of logfact;
 * x may be any int32 (x < 0 is below the support, x > hi above it).  That logfact holds lgamma(i + 1), and that the outputs do
 * not overlap each other or the operands. */
int vf_hypergeom_tail(const int32_t* count, int64_t ldc, const int32_t* size, const int32_t* csize, int64_t T, int k, int64_t N,
                      const double* logfact, int alternative, double* log_p, double* tail, int32_t* steps, int64_t ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_ENRICH_H */

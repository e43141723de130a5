/* vf_hip_components.h -- the entries of libvf_hip.so behind the spectral start of a DISCONNECTED graph (umap-learn's
 * multi_component_layout): the connected components of the CSR graph of vf_hip_umap.h (rowptr int64 [R + 1], col int32 [nnz],
 * w fp32 [nnz]), the graph renumbered so that every component is a contiguous range of rows with local columns, and the centroid
 * of each component's rows of a matrix.  Three entries, driven by variantformer_amd/manifold.py (_components,
 * spectral_init_components), which sorts the labels with torch and solves every component with the entries of vf_hip_spectral.h.
 *
 * The twelfth header of the one library, beside vf_hip.h, vf_hip_attn_contrib.h, vf_hip_gene_contrib.h, vf_hip_cre_heads.h,
 * vf_hip_forest.h, vf_hip_topk.h, vf_hip_neighbors.h, vf_hip_linkage.h, vf_hip_umap.h, vf_hip_spectral.h and
 * vf_hip_umap_transform.h.  Its entries are bound through _lib.ENTRIES["vf_hip_components.h"], which _lib.load() applies like the other
 * eleven tables, and tests/components_cases.py holds their references and case table.  Everything the main header says holds
 * here: the conventions at its top (device pointers owned by the caller, `stream` a hipStream_t, strides in elements, 0 = ok /
 * VF_ERR_*, vf_last_error()), the comment contract of every entry (arguments, write set, arithmetic, refusals), and
 * VF_ABI_VERSION: a new symbol changes no existing one, so the version stays 13.  No entry synchronises the stream.
 *
 * vf_graph_components_rounds is THE ONE PLACE IN THESE HEADERS THAT USES AN ATOMIC: a vector integer minimum on global memory
 * (atomicMin on an int32), whose result does not depend on the order in which the lanes arrive.  A round therefore has one
 * result, two runs give the same bits and numpy restates a round bit for bit (tests/components_cases.py).  The other two entries
 * use no atomic.  No block waits for another anywhere: no grid-wide barrier, no spinning; the kernel boundary is the barrier.
 */
#ifndef VF_HIP_COMPONENTS_H
#define VF_HIP_COMPONENTS_H

#include "vf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most vertices, as VF_UMAP_MAX_R */
#define VF_COMPONENTS_MAX_R (1 << 24)
/* vf_segment_mean_gather: the columns of one block's tile, and the waves that share a segment's positions */
#define VF_SEGMENT_MEAN_TILE 64
#define VF_SEGMENT_MEAN_WAVES 4
/* vf_segment_mean_gather: the most columns (65 535 tiles) */
#define VF_SEGMENT_MEAN_MAX_D (64 * 65535)

/* `rounds` rounds of the component search (added under ABI 13), three kernel launches per round from one loop inside the entry.
 * An entry e of row i is an EDGE only if w[e] > 0 (a NaN is not) and 0 <= col[e] < R.
 * Arguments:
 *   rowptr, col, w, nnz, R   the graph in CSR;
 *   P        int32 [R]: the state, a parent per vertex with 0 <= P[i] <= i; the caller starts it as the identity;
 *   g, m     int32 [R]: two work vectors (what they hold on entry is not read);
 *   changed  int32 [1];  rounds >= 0.
 * One round, as numpy (r, c the rows and columns of the edges):
 *   g  = P[P]                                   the shortcut
 *   m  = g.copy(); np.minimum.at(m, r, g[c])    the gather: a row reads its neighbours' g
 *   Pn = np.minimum(g, m)
 *   np.minimum.at(Pn, P, m)                     the hook onto the parent: an integer minimum
 *   changed = any(Pn != P); P = Pn
 * Staged so that every value is formed from a buffer that no thread of that launch writes: launch 1 writes g[i] = P[P[i]] and
 * m[i] = g[i] (and changed[0] = 0); launch 2 gives a row to a thread, which forms its minimum over g in a register and lowers
 * m[i] and m[P[i]] to it with the atomic integer minimum (skipped where the minimum is not below g[i], g[P[i]]; the lanes of a
 * wavefront that all hook onto one parent are combined into one atomic first) -- g and P are only read in it; launch 3 writes
 * P[i] = m[i] where they differ and then changed[0] = 1.  Integers only: numpy restates a round bit for bit.
 * Write set, exactly, for rounds >= 1: g[i] and m[i] for 0 <= i < R, changed[0], and P[i] where a round lowers it.  changed[0]
 * describes the LAST round run: 1 if it lowered any P[i], else 0 -- written with plain stores of one value.  rounds == 0 or
 * R == 0 launches nothing and writes nothing, changed included.  rowptr, col and w are only read.
 * A settled state is a fixed point: a further round changes nothing and leaves changed[0] = 0.  On a graph of symmetric
 * structure (j is an edge of row i whenever i is one of row j) the fixed point reached from the identity is P[i] = the smallest
 * vertex of i's component; a vertex without an edge is its own component.  On any other input the entry promises only that
 * everything stays inside the buffers, that 0 <= P[i] <= i holds after every round and that no P[i] ever grows: an e outside
 * [0, nnz) is skipped, and a P[i] outside [0, i] on entry is read as i.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null rowptr, P, g, m or
 * changed, a null col or w unless nnz == 0; rowptr not 8-byte aligned, any other not 4-byte aligned; P, g and m not pairwise
 * distinct; R < 0; R > VF_COMPONENTS_MAX_R (2^24); nnz < 0; rounds < 0.
 * Not checked (the caller guarantees): rowptr is non-decreasing from 0 to nnz; P, g, m and changed do not overlap. */
int vf_graph_components_rounds(const int64_t* rowptr, const int32_t* col, const float* w, int64_t nnz, int64_t R, int32_t* P,
                               int32_t* g, int32_t* m, int32_t* changed, int rounds, void* stream);

/* The graph renumbered by components (added under ABI 13): new row r is old row order[r], and the new rows of one component
 * are the contiguous range [starts[k], starts[k + 1]) with columns counted from starts[k].
 * Arguments:
 *   rowptr, col, w, nnz, R   the graph in CSR;
 *   order    int32 [R]: the old vertex of every new row (the vertices in a stable sort on their label);
 *   rank     int32 [R]: its inverse, the new row of every old vertex;
 *   comp     int32 [R]: the component k of every NEW row, 0 <= k < C;   starts  int32 [C + 1]: the first new row of every
 *            component, starts[C] = R;   C  the components, 1 <= C <= R;
 *   rowptr_new  int64 [R + 1]: the cumulative sum of the permuted row lengths, rowptr_new[r + 1] - rowptr_new[r] =
 *            rowptr[order[r] + 1] - rowptr[order[r]];
 *   col_new  int32 [nnz];  w_new  fp32 [nnz].
 * Write set, exactly: col_new[e'] and w_new[e'] for rowptr_new[r] <= e' < rowptr_new[r + 1], 0 <= r < R (every element of both
 * when rowptr_new is as stated).  Everything else is only read.
 * One wavefront per new row r; with i = order[r], k = comp[r], lo = starts[k], hi = starts[k + 1], the t-th entry of the new row
 * is the t-th entry e of the old row, in its order: with j = col[e] it is written as
 *   col_new = rank[j] - lo, w_new = w[e]     if w[e] > 0, 0 <= j < R and lo <= rank[j] < hi (an edge inside the component);
 *   col_new = -1, w_new = +0                 otherwise (no edge: the row keeps its length, and the degree and product kernels
 *                                            of vf_hip_spectral.h skip a column of -1 or add +0).
 * No arithmetic but the integer subtraction; weights are copied bit for bit.  With labels that are constant on components and a
 * stable sort, a row's ascending columns stay ascending, so a component's slice with its rowptr rebased to 0 is exactly the
 * sub-graph extracted on its own.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null rowptr, order, rank,
 * comp, starts or rowptr_new, a null col, w, col_new or w_new unless nnz == 0; rowptr or rowptr_new not 8-byte aligned, any other
 * not 4-byte aligned; col_new == col or w_new == w; R < 0; R > VF_COMPONENTS_MAX_R; nnz < 0; C outside 1 .. R unless R == 0.
 * R == 0 is VF_OK with nothing launched.
 * Not checked (the caller guarantees): the arrays are as stated.  Input that is not valid stays inside the buffers: an order[r]
 * outside [0, R) or a comp[r] outside [0, C) writes the whole new row as no edges; an e or e' outside [0, nnz) is skipped; a new
 * row longer than the old one is filled up with no edges, a shorter one is cut. */
int vf_csr_components(const int64_t* rowptr, const int32_t* col, const float* w, int64_t nnz, int64_t R, const int32_t* order,
                      const int32_t* rank, const int32_t* comp, const int32_t* starts, int64_t C, const int64_t* rowptr_new,
                      int32_t* col_new, float* w_new, void* stream);

/* The mean of each segment's rows of x, gathered through `order` (added under ABI 13): the centroid of every component.
 * (The name says what vf_segment_mean of vf_hip.h is not: that one averages contiguous token rows in fp32.)
 * Arguments:
 *   x       fp32 [R, >= d], rows ldx apart (64-bit offsets);  R  its rows;  d  the columns, >= 1;
 *   order   int32 [R]: position -> row of x;   starts  int32 [C + 1], non-decreasing from 0 to R: segment k is the positions
 *           [starts[k], starts[k + 1]);   C  the segments, >= 0;
 *   out     fp32 [C, >= d], rows ldo apart (64-bit offsets).
 * Write set, exactly: out[k * ldo + c] for 0 <= k < C, 0 <= c < d.  x, order and starts are only read.
 * Arithmetic, in fp64, in a fixed order: one block per (segment, tile of VF_SEGMENT_MEAN_TILE = 64 columns), a lane per column.
 * With s = starts[k], n = starts[k + 1] - s, wavefront v (0 .. 3) starts from +0 and adds (double)x[order[q], c] for the
 * positions q = s + v, s + v + 4, ... below s + n, ascending; then S = ((p0 + p1) + p2) + p3 over the four partials, and
 * out[k, c] = (float)(S / (double)n): one fp64 division, rounded once to fp32.  No atomics: numpy restates it bit for bit.
 * A segment without positions gets NaN (0 / 0).
 * Non-finite operands: follow IEEE through the sums.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null x, order, starts or
 * out; any not 4-byte aligned; R < 0; R > VF_COMPONENTS_MAX_R; d outside 1 .. VF_SEGMENT_MEAN_MAX_D; ldx < d; ldo < d; C < 0; C > VF_COMPONENTS_MAX_R.
 * C == 0 is VF_OK with nothing launched.
 * Not checked (the caller guarantees): starts is non-decreasing from 0 to R.  Input that is not valid stays inside the buffers:
 * a position outside [0, R) or an order[q] outside [0, R) adds nothing (n is still starts[k + 1] - starts[k]). */
int vf_segment_mean_gather(const float* x, int64_t ldx, int64_t R, int d, const int32_t* order, const int32_t* starts, int64_t C,
                           float* out, int64_t ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_COMPONENTS_H */

// The device work behind the spectral start of a disconnected graph (include/vf_hip_components.h): rounds of the component
// search (shortcut, gather, hook onto the parent), the graph renumbered by components, and the centroid of each component's
// rows.  The hook is the library's one atomic: an integer minimum on global memory, whose result does not depend on arrival
// order, so a round has one result.  No block waits for another: every stage of a round is a launch of its own.  The centroid
// sums in fp64 in the header's order; nothing here may contract into an fma (the pragma below).
#include "vf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int ROWS_PER_BLOCK = THREADS / VF_WAVE;                        // where a wavefront takes a row
constexpr int NONE = 0x7FFFFFFF;
static_assert(THREADS == VF_SEGMENT_MEAN_WAVES * VF_WAVE && VF_SEGMENT_MEAN_TILE == VF_WAVE, "a lane per column, four wavefronts per segment");

// A parent outside [0, i] is read as i.
__device__ __forceinline__ int parent_of(const int32_t* __restrict__ P, int i) {
    const int p = P[i];
    return (unsigned)p > (unsigned)i ? i : p;
}

// Launch 1 of a round: g = P[P], m = g, changed = 0.
__global__ __launch_bounds__(THREADS) void components_shortcut_kernel(const int32_t* __restrict__ P, int R, int32_t* __restrict__ g,
                                                                      int32_t* __restrict__ m, int32_t* __restrict__ changed) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i == 0) changed[0] = 0;
    if (i >= R) return;
    const int q = parent_of(P, parent_of(P, i));
    g[i] = q;
    m[i] = q;
}

// Launch 2: a thread per row.  Its minimum over g (its own and its neighbours') stays in a register; m[i] and m[P[i]] are
// lowered to it.  g and P are only read here, m is only touched by the atomic minimum.
__global__ __launch_bounds__(THREADS) void components_hook_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                  const float* __restrict__ w, int64_t nnz, int R,
                                                                  const int32_t* __restrict__ P, const int32_t* __restrict__ g,
                                                                  int32_t* __restrict__ m) {
    const int lane = threadIdx.x & (VF_WAVE - 1);
    const int i = blockIdx.x * THREADS + threadIdx.x;
    int mi = NONE, t = 0;
    bool want = false;
    if (i < R) {
        const int gi = g[i];
        mi = gi;
        int64_t begin = rowptr[i], end = rowptr[i + 1];
        begin = begin < 0 ? 0 : begin;
        end = end > nnz ? nnz : end;
        for (int64_t e = begin; e < end; ++e) {
            const int j = col[e];
            if (!(w[e] > 0.f) || j < 0 || j >= R) continue;               // no edge
            const int gj = g[j];
            mi = gj < mi ? gj : mi;
        }
        if (mi < gi) atomicMin(&m[i], mi);
        t = parent_of(P, i);
        want = mi < g[t];                                                 // m[t] started as g[t]: otherwise the hook changes nothing
    }
    // the hook: lanes that all name one parent (the root of a large component) go as one atomic
    const unsigned long long wanting = __ballot(want);
    if (wanting == 0) return;                                             // the whole wavefront
    const int leader = __ffsll(wanting) - 1;
    const int t0 = __shfl(t, leader);
    if (__all(!want || t == t0)) {
        int v = want ? mi : NONE;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int o = __shfl_xor(v, off);
            v = o < v ? o : v;
        }
        if (lane == leader) atomicMin(&m[t0], v);
    } else if (want) {
        atomicMin(&m[t], mi);
    }
}

// Launch 3: P = m where they differ; changed = 1 then (every writer stores the same value).
__global__ __launch_bounds__(THREADS) void components_commit_kernel(const int32_t* __restrict__ m, int R, int32_t* __restrict__ P,
                                                                    int32_t* __restrict__ changed) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= R) return;
    const int v = m[i];
    if (v != P[i]) {
        P[i] = v;
        changed[0] = 1;
    }
}

// One wavefront per new row: the old row's entries in their order, columns through rank and rebased to the component.
__global__ __launch_bounds__(THREADS) void csr_components_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                 const float* __restrict__ w, int64_t nnz, int R,
                                                                 const int32_t* __restrict__ order, const int32_t* __restrict__ rank,
                                                                 const int32_t* __restrict__ comp, const int32_t* __restrict__ starts, int C,
                                                                 const int64_t* __restrict__ rowptr_new, int32_t* __restrict__ col_new,
                                                                 float* __restrict__ w_new) {
    const int lane = threadIdx.x & (VF_WAVE - 1);
    const int r = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (r >= R) return;
    int64_t nb = rowptr_new[r], ne = rowptr_new[r + 1];
    nb = nb < 0 ? 0 : nb;
    ne = ne > nnz ? nnz : ne;
    const int i = order[r], k = comp[r];
    const bool valid = i >= 0 && i < R && k >= 0 && k < C;
    const int lo = valid ? starts[k] : 0, hi = valid ? starts[k + 1] : 0;
    int64_t ob = valid ? rowptr[i] : 0, oe = valid ? rowptr[i + 1] : 0;
    ob = ob < 0 ? 0 : ob;
    oe = oe > nnz ? nnz : oe;
    for (int64_t t = lane; nb + t < ne; t += VF_WAVE) {
        const int64_t e = ob + t;
        int c = -1;
        float v = 0.f;
        if (e < oe) {
            const int j = col[e];
            const float we = w[e];
            if (we > 0.f && j >= 0 && j < R) {
                const int rk = rank[j];
                if (rk >= lo && rk < hi) {
                    c = rk - lo;
                    v = we;
                }
            }
        }
        col_new[nb + t] = c;
        w_new[nb + t] = v;
    }
}

// One block per (segment, 64-column tile): wavefront v sums the positions s + v, s + v + 4, ... in fp64, a lane per column.
__global__ __launch_bounds__(THREADS) void segment_mean_gather_kernel(const float* __restrict__ x, int64_t ldx, int R, int d,
                                                                      const int32_t* __restrict__ order, const int32_t* __restrict__ starts,
                                                                      float* __restrict__ out, int64_t ldo) {
    __shared__ double part[VF_SEGMENT_MEAN_WAVES][VF_SEGMENT_MEAN_TILE];
    const int lane = threadIdx.x & (VF_WAVE - 1), v = threadIdx.x >> 6;
    const int64_t k = blockIdx.x;
    const int c = blockIdx.y * VF_SEGMENT_MEAN_TILE + lane;
    const int64_t s = starts[k], e = starts[k + 1];
    double acc = 0.0;
    if (c < d) {
        const int64_t stop = e < R ? e : R;                                // positions outside [0, R) add nothing
        for (int64_t q = (s < 0 ? 0 : s) + v; q < stop; q += VF_SEGMENT_MEAN_WAVES) {
            const int row = order[q];
            if (row < 0 || row >= R) continue;
            acc = acc + (double)x[(int64_t)row * ldx + c];
        }
    }
    part[v][lane] = acc;
    __syncthreads();
    if (v == 0 && c < d) {
        const double sum = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
        out[k * ldo + c] = (float)(sum / (double)(e - s));
    }
}


}  // namespace

extern "C" int vf_graph_components_rounds(const int64_t* rowptr, const int32_t* col, const float* w, int64_t nnz, int64_t R, int32_t* P,
                                          int32_t* g, int32_t* m, int32_t* changed, int rounds, void* stream) {
    VF_REQUIRE(rowptr, "vf_graph_components_rounds: null pointer rowptr");
    VF_REQUIRE(col || nnz == 0, "vf_graph_components_rounds: null pointer col");
    VF_REQUIRE(w || nnz == 0, "vf_graph_components_rounds: null pointer w");
    VF_REQUIRE(P, "vf_graph_components_rounds: null pointer P");
    VF_REQUIRE(g, "vf_graph_components_rounds: null pointer g");
    VF_REQUIRE(m, "vf_graph_components_rounds: null pointer m");
    VF_REQUIRE(changed, "vf_graph_components_rounds: null pointer changed");
    VF_REQUIRE(VF_ALIGNED8(rowptr), "vf_graph_components_rounds: rowptr must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(col), "vf_graph_components_rounds: col must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(w), "vf_graph_components_rounds: w must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(P), "vf_graph_components_rounds: P must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(g), "vf_graph_components_rounds: g must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(m), "vf_graph_components_rounds: m must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(changed), "vf_graph_components_rounds: changed must be 4-byte aligned");
    VF_REQUIRE(P != g && P != m && g != m, "vf_graph_components_rounds: P, g and m must be three buffers");
    VF_REQUIRE(R >= 0, "vf_graph_components_rounds: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R <= VF_COMPONENTS_MAX_R, "vf_graph_components_rounds: R=%ld is above 2^24", (long)R);
    VF_REQUIRE(nnz >= 0, "vf_graph_components_rounds: nnz=%ld must not be negative", (long)nnz);
    VF_REQUIRE(rounds >= 0, "vf_graph_components_rounds: rounds=%d must not be negative", rounds);
    if (R == 0 || rounds == 0) return VF_OK;
    const dim3 grid((unsigned)((R + THREADS - 1) / THREADS)), block(THREADS);
    for (int t = 0; t < rounds; ++t) {
        hipLaunchKernelGGL(components_shortcut_kernel, grid, block, 0, (hipStream_t)stream, (const int32_t*)P, (int)R, g, m, changed);
        VF_CHECK_LAUNCH("vf_graph_components_rounds");
        hipLaunchKernelGGL(components_hook_kernel, grid, block, 0, (hipStream_t)stream, rowptr, col, w, nnz, (int)R, (const int32_t*)P,
                           (const int32_t*)g, m);
        VF_CHECK_LAUNCH("vf_graph_components_rounds");
        hipLaunchKernelGGL(components_commit_kernel, grid, block, 0, (hipStream_t)stream, (const int32_t*)m, (int)R, P, changed);
        VF_CHECK_LAUNCH("vf_graph_components_rounds");
    }
    return VF_OK;
}

extern "C" int vf_csr_components(const int64_t* rowptr, const int32_t* col, const float* w, int64_t nnz, int64_t R, const int32_t* order,
                                 const int32_t* rank, const int32_t* comp, const int32_t* starts, int64_t C, const int64_t* rowptr_new,
                                 int32_t* col_new, float* w_new, void* stream) {
    VF_REQUIRE(rowptr, "vf_csr_components: null pointer rowptr");
    VF_REQUIRE(col || nnz == 0, "vf_csr_components: null pointer col");
    VF_REQUIRE(w || nnz == 0, "vf_csr_components: null pointer w");
    VF_REQUIRE(order, "vf_csr_components: null pointer order");
    VF_REQUIRE(rank, "vf_csr_components: null pointer rank");
    VF_REQUIRE(comp, "vf_csr_components: null pointer comp");
    VF_REQUIRE(starts, "vf_csr_components: null pointer starts");
    VF_REQUIRE(rowptr_new, "vf_csr_components: null pointer rowptr_new");
    VF_REQUIRE(col_new || nnz == 0, "vf_csr_components: null pointer col_new");
    VF_REQUIRE(w_new || nnz == 0, "vf_csr_components: null pointer w_new");
    VF_REQUIRE(VF_ALIGNED8(rowptr), "vf_csr_components: rowptr must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(rowptr_new), "vf_csr_components: rowptr_new must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(col), "vf_csr_components: col must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(w), "vf_csr_components: w must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(order), "vf_csr_components: order must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(rank), "vf_csr_components: rank must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(comp), "vf_csr_components: comp must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(starts), "vf_csr_components: starts must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(col_new), "vf_csr_components: col_new must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(w_new), "vf_csr_components: w_new must be 4-byte aligned");
    VF_REQUIRE(nnz == 0 || (col_new != col && (const float*)w_new != w), "vf_csr_components: col_new and w_new must not be col and w");
    VF_REQUIRE(R >= 0, "vf_csr_components: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R <= VF_COMPONENTS_MAX_R, "vf_csr_components: R=%ld is above 2^24", (long)R);
    VF_REQUIRE(nnz >= 0, "vf_csr_components: nnz=%ld must not be negative", (long)nnz);
    if (R == 0) return VF_OK;
    VF_REQUIRE(C >= 1 && C <= R, "vf_csr_components: C=%ld outside 1 .. R=%ld", (long)C, (long)R);
    hipLaunchKernelGGL(csr_components_kernel, dim3((unsigned)((R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), dim3(THREADS), 0,
                       (hipStream_t)stream, rowptr, col, w, nnz, (int)R, order, rank, comp, starts, (int)C, rowptr_new, col_new, w_new);
    VF_CHECK_LAUNCH("vf_csr_components");
    return VF_OK;
}

extern "C" int vf_segment_mean_gather(const float* x, int64_t ldx, int64_t R, int d, const int32_t* order, const int32_t* starts, int64_t C,
                                      float* out, int64_t ldo, void* stream) {
    VF_REQUIRE(x, "vf_segment_mean_gather: null pointer x");
    VF_REQUIRE(order, "vf_segment_mean_gather: null pointer order");
    VF_REQUIRE(starts, "vf_segment_mean_gather: null pointer starts");
    VF_REQUIRE(out, "vf_segment_mean_gather: null pointer out");
    VF_REQUIRE(VF_ALIGNED4(x), "vf_segment_mean_gather: x must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(order), "vf_segment_mean_gather: order must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(starts), "vf_segment_mean_gather: starts must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(out), "vf_segment_mean_gather: out must be 4-byte aligned");
    VF_REQUIRE(R >= 0, "vf_segment_mean_gather: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R <= VF_COMPONENTS_MAX_R, "vf_segment_mean_gather: R=%ld is above 2^24", (long)R);
    VF_REQUIRE(d >= 1 && d <= VF_SEGMENT_MEAN_MAX_D, "vf_segment_mean_gather: d=%d outside 1 .. %d", d, VF_SEGMENT_MEAN_MAX_D);
    VF_REQUIRE(ldx >= d, "vf_segment_mean_gather: ldx=%ld is below d=%d", (long)ldx, d);
    VF_REQUIRE(ldo >= d, "vf_segment_mean_gather: ldo=%ld is below d=%d", (long)ldo, d);
    VF_REQUIRE(C >= 0 && C <= VF_COMPONENTS_MAX_R, "vf_segment_mean_gather: C=%ld outside 0 .. 2^24", (long)C);
    if (C == 0) return VF_OK;
    hipLaunchKernelGGL(segment_mean_gather_kernel, dim3((unsigned)C, (unsigned)((d + VF_SEGMENT_MEAN_TILE - 1) / VF_SEGMENT_MEAN_TILE)),
                       dim3(THREADS), 0, (hipStream_t)stream, x, ldx, (int)R, d, order, starts, out, ldo);
    VF_CHECK_LAUNCH("vf_segment_mean_gather");
    return VF_OK;
}

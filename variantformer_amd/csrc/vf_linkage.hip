// Ward linkage on the device (include/vf_hip_linkage.h): the nearest other row of every row, and one round of merging mutually
// nearest clusters -- Lance-Williams update and compaction in one gather pass.  Both are bound by memory traffic: a round reads
// the working matrix twice and writes the smaller one once.  The arithmetic is fixed operation by operation so that fp32 numpy
// restates it bit for bit: nothing in this file may contract into an fma (the pragma below), `/` and __builtin_sqrtf are hipcc's
// correctly rounded fp32 division and square root, and the file is built without -fno-honor-nans (csrc/build.py: that flag is
// vf_attn.hip's) because the order of vf_linkage_nearest is defined for NaN.
#include "vf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr unsigned long long NONE = ~0ull;      // no candidate: above every (key, j), as j < 2^24

// One block per row: thread t takes the columns t, t + 256, ...; the smallest (key, j) wins, so ties go to the lower j.
__global__ __launch_bounds__(THREADS) void linkage_nearest_kernel(const float* __restrict__ D, int64_t ld, int m,
                                                                  float* __restrict__ nn_val, int32_t* __restrict__ nn_idx) {
    __shared__ unsigned long long part[THREADS / VF_WAVE];
    const int i = blockIdx.x;
    const uint32_t* row = reinterpret_cast<const uint32_t*>(D) + (int64_t)i * ld;
    unsigned long long best = NONE;
    for (int j = threadIdx.x; j < m; j += THREADS) {
        if (j == i) continue;
        const unsigned long long c = ((unsigned long long)order_key(row[j]) << 32) | (uint32_t)j;
        best = c < best ? c : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o < best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < THREADS / VF_WAVE; ++w) best = part[w] < best ? part[w] : best;
        const bool none = best == NONE;                                  // m == 1
        const int j = (int)(uint32_t)best;
        nn_idx[i] = none ? -1 : j;
        reinterpret_cast<uint32_t*>(nn_val)[i] = none ? 0x7F800000u : row[j];
    }
}

// first clamped into [0, m), second into [-1, m): what the header promises for constituents that are no valid input.
__device__ __forceinline__ int clamp_first(int f, int m) { return min(max(f, 0), m - 1); }
__device__ __forceinline__ int clamp_second(int s, int m) { return s < 0 ? -1 : min(s, m - 1); }

// d(p, q) with p a constituent of the output row's slot and q of the output column's: row p of D is the block's own.
__device__ __forceinline__ float old_distance(const float* __restrict__ D, int64_t ld, int p, int q, int upper_only) {
    const int r = upper_only ? min(p, q) : p, c = upper_only ? max(p, q) : q;
    return D[(int64_t)r * ld + c];
}

__device__ __forceinline__ float lance_williams(float dxi, float dyi, float dxy, int sx, int sy, int si) {
    const float t1 = (float)(sx + si) * (dxi * dxi);
    const float t2 = (float)(sy + si) * (dyi * dyi);
    const float t3 = (float)si * (dxy * dxy);
    const float q = ((t1 + t2) - t3) / (float)(sx + sy + si);
    return __builtin_sqrtf(q < 0.f ? 0.f : q);
}

// size_out and pair_dist: one thread per new slot.
__global__ __launch_bounds__(THREADS) void linkage_slots_kernel(const float* __restrict__ D, int64_t ld, int m,
                                                                const int32_t* __restrict__ size, const int32_t* __restrict__ first,
                                                                const int32_t* __restrict__ second, int m_out,
                                                                int32_t* __restrict__ size_out, float* __restrict__ pair_dist,
                                                                int upper_only) {
    const int a = blockIdx.x * THREADS + threadIdx.x;
    if (a >= m_out) return;
    const int f = clamp_first(first[a], m), s = clamp_second(second[a], m);
    size_out[a] = size[f] + (s >= 0 ? size[s] : 0);
    pair_dist[a] = s >= 0 ? old_distance(D, ld, f, s, upper_only) : 0.f;
}

// One block per output row a; thread t takes the columns t, t + 256, ...  An element reads the rows of a's constituents at the
// columns of b's constituents (first is increasing, so the reads of a row run forward through it), and takes the roles of the
// header's lo and hi from min(a, b) and max(a, b).
__global__ __launch_bounds__(THREADS) void linkage_contract_kernel(const float* __restrict__ D, int64_t ld, int m,
                                                                   const int32_t* __restrict__ size, const int32_t* __restrict__ first,
                                                                   const int32_t* __restrict__ second, int m_out,
                                                                   float* __restrict__ D_out, int64_t ld_out,
                                                                   const float* __restrict__ pair_dist, int upper_only) {
    const int a = blockIdx.x;
    const int fa = clamp_first(first[a], m), sa = clamp_second(second[a], m);
    const int size_fa = size[fa], size_sa = sa >= 0 ? size[sa] : 0;
    const float pd_a = pair_dist[a];
    float* out = D_out + (int64_t)a * ld_out;
    for (int b = threadIdx.x; b < m_out; b += THREADS) {
        if (b == a) {
            out[b] = 0.f;
            continue;
        }
        const int fb = clamp_first(first[b], m), sb = clamp_second(second[b], m);
        const float d_ff = old_distance(D, ld, fa, fb, upper_only);
        float r;
        if (sa < 0 && sb < 0) {
            r = d_ff;
        } else {
            const int size_fb = size[fb];
            if (sb < 0) {                                                 // a merged, b alone
                const float d_sf = old_distance(D, ld, sa, fb, upper_only);
                // a is lo: LW(d_AC, d_BC, d_AB, sA, sB, sC); a is hi: LW(d_AC, d_AD, d_CD, sC, sD, sA).  The same expression.
                r = lance_williams(d_ff, d_sf, pd_a, size_fa, size_sa, size_fb);
            } else if (sa < 0) {                                          // b merged, a alone
                const float d_fs = old_distance(D, ld, fa, sb, upper_only);
                r = lance_williams(d_ff, d_fs, pair_dist[b], size_fb, size[sb], size_fa);
            } else {                                                      // both merged: here the roles differ
                const int size_sb = size[sb];
                const float pd_b = pair_dist[b];
                const float d_fs = old_distance(D, ld, fa, sb, upper_only);
                const float d_sf = old_distance(D, ld, sa, fb, upper_only);
                const float d_ss = old_distance(D, ld, sa, sb, upper_only);
                if (a < b) {                                              // lo = a = (A, B), hi = b = (C, D)
                    const float u = lance_williams(d_ff, d_sf, pd_a, size_fa, size_sa, size_fb);
                    const float v = lance_williams(d_fs, d_ss, pd_a, size_fa, size_sa, size_sb);
                    r = lance_williams(u, v, pd_b, size_fb, size_sb, size_fa + size_sa);
                } else {                                                  // lo = b = (A, B), hi = a = (C, D)
                    const float u = lance_williams(d_ff, d_fs, pd_b, size_fb, size_sb, size_fa);
                    const float v = lance_williams(d_sf, d_ss, pd_b, size_fb, size_sb, size_sa);
                    r = lance_williams(u, v, pd_a, size_fa, size_sa, size_fb + size_sb);
                }
            }
        }
        out[b] = r;
    }
}


}  // namespace

extern "C" int vf_linkage_nearest(const float* D, int64_t ld, int64_t m, float* nn_val, int32_t* nn_idx, void* stream) {
    VF_REQUIRE(D, "vf_linkage_nearest: null pointer D");
    VF_REQUIRE(nn_val, "vf_linkage_nearest: null pointer nn_val");
    VF_REQUIRE(nn_idx, "vf_linkage_nearest: null pointer nn_idx");
    VF_REQUIRE(VF_ALIGNED4(D), "vf_linkage_nearest: D must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(nn_val), "vf_linkage_nearest: nn_val must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(nn_idx), "vf_linkage_nearest: nn_idx must be 4-byte aligned");
    VF_REQUIRE(m >= 0, "vf_linkage_nearest: m=%ld must not be negative", (long)m);
    VF_REQUIRE(m <= VF_LINKAGE_MAX_M, "vf_linkage_nearest: m=%ld is above 2^24", (long)m);
    VF_REQUIRE(ld >= m, "vf_linkage_nearest: ld=%ld is below m=%ld", (long)ld, (long)m);
    if (m == 0) return VF_OK;
    hipLaunchKernelGGL(linkage_nearest_kernel, dim3((unsigned)m), dim3(THREADS), 0, (hipStream_t)stream, D, ld, (int)m, nn_val, nn_idx);
    VF_CHECK_LAUNCH("vf_linkage_nearest");
    return VF_OK;
}

extern "C" int vf_linkage_contract(const float* D, int64_t ld, int64_t m, const int32_t* size, const int32_t* first,
                                   const int32_t* second, int64_t m_out, float* D_out, int64_t ld_out, int32_t* size_out,
                                   float* pair_dist, int upper_only, void* stream) {
    VF_REQUIRE(D, "vf_linkage_contract: null pointer D");
    VF_REQUIRE(size, "vf_linkage_contract: null pointer size");
    VF_REQUIRE(first, "vf_linkage_contract: null pointer first");
    VF_REQUIRE(second, "vf_linkage_contract: null pointer second");
    VF_REQUIRE(D_out, "vf_linkage_contract: null pointer D_out");
    VF_REQUIRE(size_out, "vf_linkage_contract: null pointer size_out");
    VF_REQUIRE(pair_dist, "vf_linkage_contract: null pointer pair_dist");
    VF_REQUIRE(VF_ALIGNED4(D), "vf_linkage_contract: D must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(size), "vf_linkage_contract: size must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(first), "vf_linkage_contract: first must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(second), "vf_linkage_contract: second must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(D_out), "vf_linkage_contract: D_out must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(size_out), "vf_linkage_contract: size_out must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(pair_dist), "vf_linkage_contract: pair_dist must be 4-byte aligned");
    VF_REQUIRE(m >= 0, "vf_linkage_contract: m=%ld must not be negative", (long)m);
    VF_REQUIRE(m <= VF_LINKAGE_MAX_M, "vf_linkage_contract: m=%ld is above 2^24", (long)m);
    VF_REQUIRE(ld >= m, "vf_linkage_contract: ld=%ld is below m=%ld", (long)ld, (long)m);
    VF_REQUIRE(m_out >= 0, "vf_linkage_contract: m_out=%ld must not be negative", (long)m_out);
    VF_REQUIRE(m_out <= m, "vf_linkage_contract: m_out=%ld is above m=%ld", (long)m_out, (long)m);
    VF_REQUIRE(ld_out >= m_out, "vf_linkage_contract: ld_out=%ld is below m_out=%ld", (long)ld_out, (long)m_out);
    VF_REQUIRE(upper_only == 0 || upper_only == 1, "vf_linkage_contract: upper_only=%d must be 0 or 1", upper_only);
    if (m_out == 0) return VF_OK;
    hipLaunchKernelGGL(linkage_slots_kernel, dim3((unsigned)((m_out + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream,
                       D, ld, (int)m, size, first, second, (int)m_out, size_out, pair_dist, upper_only);
    VF_CHECK_LAUNCH("vf_linkage_contract");
    hipLaunchKernelGGL(linkage_contract_kernel, dim3((unsigned)m_out), dim3(THREADS), 0, (hipStream_t)stream, D, ld, (int)m, size,
                       first, second, (int)m_out, D_out, ld_out, (const float*)pair_dist, upper_only);
    VF_CHECK_LAUNCH("vf_linkage_contract");
    return VF_OK;
}

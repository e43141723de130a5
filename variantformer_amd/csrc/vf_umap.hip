// UMAP after the k-NN graph (include/vf_hip_umap.h): rho / sigma / directed strengths of every neighbour list, their fuzzy union
// over the symmetric CSR graph, and the epochs of the SGD layout as a gather: a vertex reads the others at their epoch-start
// positions and writes its own row alone, so there is no race and no atomic, and the result is defined by the header's order.
// Nothing here may contract into an fma (the pragma below): the union's w[i->j] and w[j->i] have the same bits because + and *
// commute, which an fma would break.  expf / powf are hipcc's library functions; the file is built without -fno-honor-nans
// (csrc/build.py: that flag is vf_attn.hip's) because absent entries are recognised by their NaN / Inf.
#include "vf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int ROWS_PER_BLOCK = THREADS / VF_WAVE;
constexpr int WALK = 8;                    // entries whose sample counts are loaded together
constexpr int NEG = 5;                     // negative vertices whose positions are loaded together: the default rate
constexpr int LAYOUT_THREADS = 64;          // one vertex per thread: small blocks spread a few thousand vertices over the CUs

// One wavefront per row, lane t holds entry t.
__global__ __launch_bounds__(THREADS) void umap_smooth_knn_kernel(const int32_t* __restrict__ idx, int64_t ld_idx,
                                                                  const float* __restrict__ dist, int64_t ld_dist, int R, int m,
                                                                  float mean_dist, float target, float* __restrict__ rho_out,
                                                                  float* __restrict__ sigma_out, float* __restrict__ strength,
                                                                  int64_t ld_strength) {
    const int lane = threadIdx.x & (VF_WAVE - 1);
    const int i = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= R) return;                                                   // the whole wavefront leaves
    const bool in_row = lane < m;
    const int j = in_row ? idx[(int64_t)i * ld_idx + lane] : -1;
    const float d = in_row ? dist[(int64_t)i * ld_dist + lane] : 0.f;
    const bool present = in_row && j >= 0 && finite_bits(d);

    float r = (present && d > 0.f) ? d : __builtin_inff();
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) r = fminf(r, __shfl_xor(r, off));
    const float rho = r == __builtin_inff() ? 0.f : r;
    const float count = wave_sum(present ? 1.f : 0.f);
    const float total = wave_sum(present ? d : 0.f);

    const float x = d - rho;
    float lo = 0.f, hi = __builtin_inff(), mid = 1.f;
    for (int it = 0; it < VF_UMAP_SMOOTH_ITERS; ++it) {
        const float term = present ? (x > 0.f ? expf(-(x / mid)) : 1.f) : 0.f;
        const float sum = wave_sum(term);
        if (fabsf(sum - target) < VF_UMAP_SMOOTH_TOL) break;             // the same bits in every lane: a uniform branch
        if (sum > target) {
            hi = mid;
            mid = (lo + hi) / 2.f;
        } else {
            lo = mid;
            mid = hi == __builtin_inff() ? mid * 2.f : (lo + hi) / 2.f;
        }
    }
    float sigma = mid;
    const float floor_ = VF_UMAP_MIN_SCALE * (rho > 0.f ? total / count : mean_dist);
    if (sigma < floor_) sigma = floor_;                                   // a NaN floor never binds
    if (count == 0.f) sigma = 0.f;
    if (lane == 0) {
        rho_out[i] = rho;
        sigma_out[i] = sigma;
    }
    if (in_row) {
        float s = 0.f;
        if (present && j != i) s = (x <= 0.f || sigma == 0.f) ? 1.f : expf(-(x / sigma));
        strength[(int64_t)i * ld_strength + lane] = s;
    }
}

// strength of `other` in row `row`'s list: the first match among m entries, +0 without one.
__device__ __forceinline__ float list_strength(const int32_t* __restrict__ idx, int64_t ld_idx, const float* __restrict__ strength,
                                               int64_t ld_strength, int m, int row, int other) {
    const int32_t* list = idx + (int64_t)row * ld_idx;
    for (int t = 0; t < m; ++t)
        if (list[t] == other) return strength[(int64_t)row * ld_strength + t];
    return 0.f;
}

// One wavefront per CSR row; its lanes take the row's entries 64 at a time.
__global__ __launch_bounds__(THREADS) void umap_union_kernel(const int32_t* __restrict__ idx, int64_t ld_idx,
                                                             const float* __restrict__ strength, int64_t ld_strength, int R, int m,
                                                             const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                             int64_t nnz, float* __restrict__ w) {
    const int lane = threadIdx.x & (VF_WAVE - 1);
    const int i = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= R) return;
    int64_t begin = rowptr[i], end = rowptr[i + 1];
    begin = begin < 0 ? 0 : begin;
    end = end > nnz ? nnz : end;
    for (int64_t e = begin + lane; e < end; e += VF_WAVE) {
        const int j = col[e];
        const float a = list_strength(idx, ld_idx, strength, ld_strength, m, i, j);
        const float b = (j >= 0 && j < R) ? list_strength(idx, ld_idx, strength, ld_strength, m, j, i) : 0.f;
        w[e] = (a + b) - a * b;
    }
}

template <int DIM>
__device__ __forceinline__ float dist2(const float (&y)[DIM], const float (&o)[DIM]) {
    float d2 = 0.f;
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
        const float t = y[c] - o[c];
        d2 += t * t;
    }
    return d2;
}

template <int DIM>
__device__ __forceinline__ void attract(float (&y)[DIM], const float (&o)[DIM], float a, float b, float alpha) {
    const float d2 = dist2<DIM>(y, o);
    float g = 0.f;
    if (d2 > 0.f) {
        const float p = powf(d2, b);
        g = ((-2.f * a * b) * (p / d2)) / (a * p + 1.f);
    }
#pragma unroll
    for (int c = 0; c < DIM; ++c) y[c] += alpha * clip4(g * (y[c] - o[c]));
}

// One thread per vertex.
template <int DIM>
__global__ __launch_bounds__(LAYOUT_THREADS) void umap_layout_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                     const int32_t* __restrict__ samples, int64_t nnz, int R,
                                                                     const float* __restrict__ Yin, float* __restrict__ Yout, int64_t ld,
                                                                     int n, int N, float a, float b, float gamma, float alpha, int rate,
                                                                     uint32_t seed_n) {
    const int i = blockIdx.x * LAYOUT_THREADS + threadIdx.x;
    if (i >= R) return;
    float y[DIM], o[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) y[c] = Yin[(int64_t)i * ld + c];
    int64_t begin = rowptr[i], end = rowptr[i + 1];
    begin = begin < 0 ? 0 : begin;
    end = end > nnz ? nnz : end;
    const uint32_t seed_i = mix32(seed_n ^ (uint32_t)i);
    const bool narrow = N <= 65535;                                       // n * s < 2^32: the due rule in 32-bit integers, same result
    // The walk is a chain of dependent loads, so its latency is what an epoch costs.  Two things shorten it without changing the
    // order of any arithmetic: the sample counts of WALK entries are loaded together and reduced to a mask of the due ones, and
    // the positions of a due entry's negative vertices (which depend on the hash alone, not on y) are loaded NEG at a time
    // before the moves that use them.
    for (int64_t e0 = begin; e0 < end; e0 += WALK) {
        int cnt[WALK];
#pragma unroll
        for (int u = 0; u < WALK; ++u) cnt[u] = e0 + u < end ? samples[e0 + u] : 0;
        uint32_t due = 0;
#pragma unroll
        for (int u = 0; u < WALK; ++u) {
            const int s = cnt[u];
            if (s < 1 || s > N) continue;
            // floor((n + 1) s / N) > floor(n s / N)  <=>  (n s mod N) + s >= N
            const uint32_t rem = narrow ? ((uint32_t)n * (uint32_t)s) % (uint32_t)N : (uint32_t)(((uint64_t)n * (uint64_t)s) % (uint64_t)N);
            if ((uint64_t)rem + (uint64_t)s >= (uint64_t)N) due |= 1u << u;
        }
        while (due) {
            const int u = __ffs(due) - 1;
            due &= due - 1;
            const int64_t e = e0 + u;
            const int j = col[e];
            if (j < 0 || j >= R) continue;
#pragma unroll
            for (int c = 0; c < DIM; ++c) o[c] = Yin[(int64_t)j * ld + c];
            attract<DIM>(y, o, a, b, alpha);
            const uint32_t seed_s = mix32(seed_i ^ (uint32_t)(e - begin));
            for (int p0 = 0; p0 < rate; p0 += NEG) {
                float q[NEG][DIM];
#pragma unroll
                for (int v = 0; v < NEG; ++v) {
                    const uint32_t h = mix32(seed_s ^ (uint32_t)(p0 + v));
                    const int k = (int)(((uint64_t)h * (uint64_t)(uint32_t)R) >> 32);        // below R whatever p0 + v is
#pragma unroll
                    for (int c = 0; c < DIM; ++c) q[v][c] = p0 + v < rate ? Yin[(int64_t)k * ld + c] : 0.f;
                }
#pragma unroll
                for (int v = 0; v < NEG; ++v) {
                    if (p0 + v >= rate) break;
                    const float d2 = dist2<DIM>(y, q[v]);
                    if (d2 == 0.f) continue;
                    const float g = ((2.f * gamma) * b) / ((0.001f + d2) * (a * powf(d2, b) + 1.f));
#pragma unroll
                    for (int c = 0; c < DIM; ++c) y[c] += alpha * clip4(g * (y[c] - q[v][c]));
                }
            }
            attract<DIM>(y, o, a, b, alpha);
        }
    }
#pragma unroll
    for (int c = 0; c < DIM; ++c) Yout[(int64_t)i * ld + c] = y[c];
}

template <int DIM>
void launch_layout(const int64_t* rowptr, const int32_t* col, const int32_t* samples, int64_t nnz, int R, const float* Yin, float* Yout,
                   int64_t ld, int n, int N, float a, float b, float gamma, float alpha, int rate, uint32_t seed_n, hipStream_t stream) {
    hipLaunchKernelGGL(umap_layout_kernel<DIM>, dim3((unsigned)((R + LAYOUT_THREADS - 1) / LAYOUT_THREADS)), dim3(LAYOUT_THREADS), 0,
                       stream, rowptr, col, samples, nnz, R, Yin, Yout, ld, n, N, a, b, gamma, alpha, rate, seed_n);
}


}  // namespace

extern "C" int vf_umap_smooth_knn(const int32_t* idx, int64_t ld_idx, const float* dist, int64_t ld_dist, int64_t R, int m,
                                  float mean_dist, float* rho, float* sigma, float* strength, int64_t ld_strength, void* stream) {
    VF_REQUIRE(idx, "vf_umap_smooth_knn: null pointer idx");
    VF_REQUIRE(dist, "vf_umap_smooth_knn: null pointer dist");
    VF_REQUIRE(rho, "vf_umap_smooth_knn: null pointer rho");
    VF_REQUIRE(sigma, "vf_umap_smooth_knn: null pointer sigma");
    VF_REQUIRE(strength, "vf_umap_smooth_knn: null pointer strength");
    VF_REQUIRE(VF_ALIGNED4(idx), "vf_umap_smooth_knn: idx must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(dist), "vf_umap_smooth_knn: dist must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(rho), "vf_umap_smooth_knn: rho must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(sigma), "vf_umap_smooth_knn: sigma must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(strength), "vf_umap_smooth_knn: strength must be 4-byte aligned");
    VF_REQUIRE(m >= 1 && m <= VF_UMAP_MAX_M, "vf_umap_smooth_knn: m=%d outside 1 .. %d", m, VF_UMAP_MAX_M);
    VF_REQUIRE(R >= 0, "vf_umap_smooth_knn: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R <= VF_UMAP_MAX_R, "vf_umap_smooth_knn: R=%ld is above 2^24", (long)R);
    VF_REQUIRE(ld_idx >= m, "vf_umap_smooth_knn: ld_idx=%ld is below m=%d", (long)ld_idx, m);
    VF_REQUIRE(ld_dist >= m, "vf_umap_smooth_knn: ld_dist=%ld is below m=%d", (long)ld_dist, m);
    VF_REQUIRE(ld_strength >= m, "vf_umap_smooth_knn: ld_strength=%ld is below m=%d", (long)ld_strength, m);
    if (R == 0) return VF_OK;
    const float target = (float)__builtin_log2((double)(m + 1));
    hipLaunchKernelGGL(umap_smooth_knn_kernel, dim3((unsigned)((R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), dim3(THREADS), 0,
                       (hipStream_t)stream, idx, ld_idx, dist, ld_dist, (int)R, m, mean_dist, target, rho, sigma, strength, ld_strength);
    VF_CHECK_LAUNCH("vf_umap_smooth_knn");
    return VF_OK;
}

extern "C" int vf_umap_union(const int32_t* idx, int64_t ld_idx, const float* strength, int64_t ld_strength, int64_t R, int m,
                             const int64_t* rowptr, const int32_t* col, int64_t nnz, float* w, void* stream) {
    VF_REQUIRE(idx, "vf_umap_union: null pointer idx");
    VF_REQUIRE(strength, "vf_umap_union: null pointer strength");
    VF_REQUIRE(rowptr, "vf_umap_union: null pointer rowptr");
    VF_REQUIRE(col || nnz == 0, "vf_umap_union: null pointer col");
    VF_REQUIRE(w || nnz == 0, "vf_umap_union: null pointer w");
    VF_REQUIRE(VF_ALIGNED4(idx), "vf_umap_union: idx must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(strength), "vf_umap_union: strength must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(rowptr), "vf_umap_union: rowptr must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(col), "vf_umap_union: col must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(w), "vf_umap_union: w must be 4-byte aligned");
    VF_REQUIRE(m >= 1 && m <= VF_UMAP_MAX_M, "vf_umap_union: m=%d outside 1 .. %d", m, VF_UMAP_MAX_M);
    VF_REQUIRE(R >= 0, "vf_umap_union: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R <= VF_UMAP_MAX_R, "vf_umap_union: R=%ld is above 2^24", (long)R);
    VF_REQUIRE(ld_idx >= m, "vf_umap_union: ld_idx=%ld is below m=%d", (long)ld_idx, m);
    VF_REQUIRE(ld_strength >= m, "vf_umap_union: ld_strength=%ld is below m=%d", (long)ld_strength, m);
    VF_REQUIRE(nnz >= 0, "vf_umap_union: nnz=%ld must not be negative", (long)nnz);
    if (R == 0 || nnz == 0) return VF_OK;
    hipLaunchKernelGGL(umap_union_kernel, dim3((unsigned)((R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), dim3(THREADS), 0,
                       (hipStream_t)stream, idx, ld_idx, strength, ld_strength, (int)R, m, rowptr, col, nnz, w);
    VF_CHECK_LAUNCH("vf_umap_union");
    return VF_OK;
}

extern "C" int vf_umap_layout(const int64_t* rowptr, const int32_t* col, const int32_t* samples, int64_t nnz, int64_t R, int dim,
                              float* Y0, float* Y1, int64_t ld, int epoch_begin, int epoch_end, int N, float a, float b, float gamma,
                              float learning_rate, int negative_sample_rate, int64_t seed, void* stream) {
    VF_REQUIRE(rowptr, "vf_umap_layout: null pointer rowptr");
    VF_REQUIRE(col || nnz == 0, "vf_umap_layout: null pointer col");
    VF_REQUIRE(samples || nnz == 0, "vf_umap_layout: null pointer samples");
    VF_REQUIRE(Y0, "vf_umap_layout: null pointer Y0");
    VF_REQUIRE(Y1, "vf_umap_layout: null pointer Y1");
    VF_REQUIRE(VF_ALIGNED8(rowptr), "vf_umap_layout: rowptr must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(col), "vf_umap_layout: col must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(samples), "vf_umap_layout: samples must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(Y0), "vf_umap_layout: Y0 must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(Y1), "vf_umap_layout: Y1 must be 4-byte aligned");
    VF_REQUIRE(Y0 != Y1, "vf_umap_layout: Y0 and Y1 must be two buffers");
    VF_REQUIRE(R >= 0, "vf_umap_layout: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R <= VF_UMAP_MAX_R, "vf_umap_layout: R=%ld is above 2^24", (long)R);
    VF_REQUIRE(nnz >= 0, "vf_umap_layout: nnz=%ld must not be negative", (long)nnz);
    VF_REQUIRE(dim >= 1 && dim <= VF_UMAP_MAX_DIM, "vf_umap_layout: dim=%d outside 1 .. %d", dim, VF_UMAP_MAX_DIM);
    VF_REQUIRE(ld >= dim, "vf_umap_layout: ld=%ld is below dim=%d", (long)ld, dim);
    VF_REQUIRE(N >= 1, "vf_umap_layout: N=%d must be at least 1", N);
    VF_REQUIRE(epoch_begin >= 0, "vf_umap_layout: epoch_begin=%d must not be negative", epoch_begin);
    VF_REQUIRE(epoch_begin <= epoch_end, "vf_umap_layout: epoch_begin=%d is above epoch_end=%d", epoch_begin, epoch_end);
    VF_REQUIRE(epoch_end <= N, "vf_umap_layout: epoch_end=%d is above N=%d", epoch_end, N);
    VF_REQUIRE(negative_sample_rate >= 0, "vf_umap_layout: negative_sample_rate=%d must not be negative", negative_sample_rate);
    if (R == 0 || epoch_begin == epoch_end) return VF_OK;
    const uint32_t seed0 = mix32((uint32_t)(uint64_t)seed + 0x9E3779B9u);
    for (int n = epoch_begin; n < epoch_end; ++n) {
        const bool even = ((n - epoch_begin) & 1) == 0;
        const float* Yin = even ? Y0 : Y1;
        float* Yout = even ? Y1 : Y0;
        const float alpha = learning_rate * (1.f - (float)n / (float)N);
        const uint32_t seed_n = mix32(seed0 ^ (uint32_t)n);
#define VF_UMAP_DIM(D)                                                                                                              \
    case D:                                                                                                                         \
        launch_layout<D>(rowptr, col, samples, nnz, (int)R, Yin, Yout, ld, n, N, a, b, gamma, alpha, negative_sample_rate, seed_n, \
                         (hipStream_t)stream);                                                                                      \
        break;
        switch (dim) {
            VF_UMAP_DIM(1) VF_UMAP_DIM(2) VF_UMAP_DIM(3) VF_UMAP_DIM(4) VF_UMAP_DIM(5) VF_UMAP_DIM(6) VF_UMAP_DIM(7) VF_UMAP_DIM(8)
        }
#undef VF_UMAP_DIM
        VF_CHECK_LAUNCH("vf_umap_layout");
    }
    return VF_OK;
}

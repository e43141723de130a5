// UMAP transform (include/vf_hip_umap_transform.h): new rows placed in a fitted embedding.  The training points stand still, so
// a query depends on nothing that moves except itself: one wavefront takes one query through all the epochs of a launch, lane t
// holding entry t of its neighbour list and that neighbour's position in registers, every lane holding the query's own position
// (the chain of moves is serial, and the same in all 64 lanes).  What the chain reads from memory are the negative vertices
// alone, and their addresses depend on (seed, epoch, row, entry, draw), not on a position: the lanes hash and gather 64 of them
// at once, the first 64 of an epoch while the chain of the epoch before is still running, and the chain takes each position out
// of its lane with a cross-lane read.  Nothing here may contract into an fma (the pragma below): the start is compared bit for
// bit with its fp32 restatement.  expf / powf are hipcc's library functions; the file is built without -fno-honor-nans
// (csrc/build.py) because absent entries are recognised by their NaN / Inf.
#include "vf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int ROWS_PER_BLOCK = THREADS / VF_WAVE;

// the value lane `src` holds, in every lane; src is the same in every lane
__device__ __forceinline__ float from_lane(float v, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), __builtin_amdgcn_readfirstlane(src)));
}
__device__ __forceinline__ int from_lane(int v, int src) { return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(src)); }

// One wavefront per row, lane t holds entry t.
__global__ __launch_bounds__(THREADS) void umap_smooth_knn_query_kernel(const int32_t* __restrict__ idx, int64_t ld_idx,
                                                                        const float* __restrict__ dist, int64_t ld_dist, int Rq, int m,
                                                                        float mean_dist, float target, float* __restrict__ sigma_out,
                                                                        float* __restrict__ strength, int64_t ld_strength) {
    const int lane = threadIdx.x & (VF_WAVE - 1);
    const int i = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= Rq) return;                                                  // the whole wavefront leaves
    const bool in_row = lane < m;
    const int j = in_row ? idx[(int64_t)i * ld_idx + lane] : -1;
    const float d = in_row ? dist[(int64_t)i * ld_dist + lane] : 0.f;
    const bool present = in_row && j >= 0 && finite_bits(d);
    const float count = wave_sum(present ? 1.f : 0.f);

    float lo = 0.f, hi = __builtin_inff(), mid = 1.f;
    for (int it = 0; it < VF_UMAP_SMOOTH_ITERS; ++it) {
        const float term = present ? (d > 0.f ? expf(-(d / mid)) : 1.f) : 0.f;
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
    const float floor_ = VF_UMAP_MIN_SCALE * mean_dist;
    if (sigma < floor_) sigma = floor_;                                   // a NaN floor never binds
    if (count == 0.f) sigma = 0.f;
    if (lane == 0) sigma_out[i] = sigma;
    if (in_row) {
        float s = 0.f;
        if (present) s = (d <= 0.f || sigma == 0.f) ? 1.f : expf(-(d / sigma));
        strength[(int64_t)i * ld_strength + lane] = s;
    }
}

// One wavefront per row, lane t holds entry t; the two sums walk the usable lanes in order.
__global__ __launch_bounds__(THREADS) void umap_init_transform_kernel(const int32_t* __restrict__ idx, int64_t ld_idx,
                                                                      const float* __restrict__ strength, int64_t ld_strength, int Rq,
                                                                      int m, const float* __restrict__ Y, int64_t ldy, int R, int dim,
                                                                      float* __restrict__ Yq, int64_t ldq) {
    const int lane = threadIdx.x & (VF_WAVE - 1);
    const int i = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= Rq) return;
    const bool in_row = lane < m;
    const int j = in_row ? idx[(int64_t)i * ld_idx + lane] : -1;
    const bool usable = in_row && j >= 0 && j < R;
    const float w = usable ? strength[(int64_t)i * ld_strength + lane] : 0.f;
    float v[VF_UMAP_MAX_DIM];
#pragma unroll
    for (int c = 0; c < VF_UMAP_MAX_DIM; ++c) v[c] = (usable && c < dim) ? Y[(int64_t)j * ldy + c] : 0.f;
    const uint64_t mask = __ballot(usable);
    float S = 0.f;
    for (uint64_t rest = mask; rest; rest &= rest - 1) S += from_lane(w, __ffsll((unsigned long long)rest) - 1);
    const float q = w / S;
#pragma unroll
    for (int c = 0; c < VF_UMAP_MAX_DIM; ++c) {
        if (c >= dim) break;
        const float prod = q * v[c];
        float acc = 0.f;
        for (uint64_t rest = mask; rest; rest &= rest - 1) acc += from_lane(prod, __ffsll((unsigned long long)rest) - 1);
        if (S == 0.f) acc = __builtin_nanf("");                           // no usable neighbour: this row cannot be placed
        if (lane == 0) Yq[(int64_t)i * ldq + c] = acc;
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

// What one epoch of one query needs before its chain of moves starts: which lanes' entries are due, the due lanes in order,
// and the positions of the epoch's first 64 negative vertices.
template <int DIM>
struct Epoch {
    int ndue;             // due entries
    int order;            // lane r: the lane of the r-th due entry (r < ndue)
    float q[DIM];         // lane l: the position of the negative vertex of flat draw number base + l
};

// The negative vertices of the flat draws [base, base + 64) of an epoch: draw f belongs to the (f / rate)-th due entry and is
// its (f % rate)-th repulsion.  k < R whatever the hash is, so every address is inside Y.
template <int DIM>
__device__ __forceinline__ void gather_negatives(float (&q)[DIM], int lane, int base, int ndue, int rate, int order, uint32_t seed_i,
                                                 const float* __restrict__ Y, int64_t ldy, uint32_t R) {
    const int f = base + lane;
    const bool live = f < ndue * rate;                                    // ndue <= 64, rate <= 2^20: no overflow
    const int e = live ? f / rate : 0;
    const int p = f - e * rate;
    const int s = __builtin_amdgcn_ds_bpermute(e << 2, order);
    const uint32_t h = mix32(mix32(seed_i ^ (uint32_t)s) ^ (uint32_t)p);
    const int64_t k = (int64_t)(((uint64_t)h * (uint64_t)R) >> 32);
#pragma unroll
    for (int c = 0; c < DIM; ++c) q[c] = live ? Y[k * ldy + c] : 0.f;
}

// One wavefront per query.
template <int DIM>
__global__ __launch_bounds__(THREADS) void umap_layout_transform_kernel(const int32_t* __restrict__ idx, int64_t ld_idx,
                                                                        const int32_t* __restrict__ samples, int64_t ld_samples, int Rq,
                                                                        int m, uint32_t row0, const float* __restrict__ Y, int64_t ldy,
                                                                        uint32_t R, float* __restrict__ Yq, int64_t ldq, int n0, int n1,
                                                                        int N, float a, float b, float gamma, float lr4, int rate,
                                                                        uint32_t seed0) {
    const int lane = threadIdx.x & (VF_WAVE - 1);
    const int i = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= Rq) return;                                                  // the whole wavefront leaves
    const bool in_row = lane < m;
    const int j = in_row ? idx[(int64_t)i * ld_idx + lane] : -1;
    const int cnt = in_row ? samples[(int64_t)i * ld_samples + lane] : 0;
    const bool usable = j >= 0 && (uint32_t)j < R && cnt >= 1 && cnt <= N;                 // everything else is never due
    float o[DIM], y[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) o[c] = usable ? Y[(int64_t)j * ldy + c] : 0.f;            // held for every epoch of the launch
#pragma unroll
    for (int c = 0; c < DIM; ++c) y[c] = Yq[(int64_t)i * ldq + c];
    const uint32_t row = row0 + (uint32_t)i;
    const uint32_t s_ = usable ? (uint32_t)cnt : 0u;
    // floor((n + 1) s / N) > floor(n s / N)  <=>  (n s mod N) + s >= N; the remainder is carried from epoch to epoch:
    // rem < N and s <= N <= 2^31 - 1, so rem + s fits 32 bits and one subtraction reduces it
    uint32_t rem = (uint32_t)(((uint64_t)(uint32_t)n0 * (uint64_t)s_) % (uint64_t)(uint32_t)N);
    const float ab = -2.f * a * b, gb = (2.f * gamma) * b;

    Epoch<DIM> next;
    auto prepare = [&](int n) {
        const bool due = usable && rem + s_ >= (uint32_t)N;
        rem = rem + s_ - (due ? (uint32_t)N : 0u);
        const uint64_t mask = __ballot(due);
        const int before = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        next.ndue = __popcll((unsigned long long)mask);
        // a permutation of the lanes: the due ones to the front in order, the others behind them
        next.order = __builtin_amdgcn_ds_permute((due ? before : next.ndue + (lane - before)) << 2, lane);
        gather_negatives<DIM>(next.q, lane, 0, next.ndue, rate, next.order, mix32(mix32(seed0 ^ (uint32_t)n) ^ row), Y, ldy, R);
    };
    prepare(n0);
    for (int n = n0; n < n1; ++n) {
        Epoch<DIM> cur = next;
        if (n + 1 < n1) prepare(n + 1);                                   // its gathers fly while this epoch's chain runs
        const float alpha = lr4 * (1.f - (float)n / (float)N);
        const uint32_t seed_i = mix32(mix32(seed0 ^ (uint32_t)n) ^ row);
        int base = 0;
        for (int e = 0; e < cur.ndue; ++e) {
            const int s = from_lane(cur.order, e);
            float t[DIM];
#pragma unroll
            for (int c = 0; c < DIM; ++c) t[c] = from_lane(o[c], s);
            {
                const float d2 = dist2<DIM>(y, t);
                float g = 0.f;
                if (d2 > 0.f) {
                    const float p = powf(d2, b);
                    g = (ab * (p / d2)) / (a * p + 1.f);
                }
#pragma unroll
                for (int c = 0; c < DIM; ++c) y[c] += alpha * clip4(g * (y[c] - t[c]));
            }
            for (int p_ = 0; p_ < rate; ++p_) {
                const int f = e * rate + p_;
                if (f - base == VF_WAVE) {
                    base += VF_WAVE;
                    gather_negatives<DIM>(cur.q, lane, base, cur.ndue, rate, cur.order, seed_i, Y, ldy, R);
                }
#pragma unroll
                for (int c = 0; c < DIM; ++c) t[c] = from_lane(cur.q[c], f - base);
                const float d2 = dist2<DIM>(y, t);
                if (d2 == 0.f) continue;
                const float g = gb / ((0.001f + d2) * (a * powf(d2, b) + 1.f));
#pragma unroll
                for (int c = 0; c < DIM; ++c) y[c] += alpha * clip4(g * (y[c] - t[c]));
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < DIM; ++c) Yq[(int64_t)i * ldq + c] = y[c];
    }
}


}  // namespace

extern "C" int vf_umap_smooth_knn_query(const int32_t* idx, int64_t ld_idx, const float* dist, int64_t ld_dist, int64_t Rq, int m,
                                        float mean_dist, float* sigma, float* strength, int64_t ld_strength, void* stream) {
    VF_REQUIRE(idx, "vf_umap_smooth_knn_query: null pointer idx");
    VF_REQUIRE(dist, "vf_umap_smooth_knn_query: null pointer dist");
    VF_REQUIRE(sigma, "vf_umap_smooth_knn_query: null pointer sigma");
    VF_REQUIRE(strength, "vf_umap_smooth_knn_query: null pointer strength");
    VF_REQUIRE(VF_ALIGNED4(idx), "vf_umap_smooth_knn_query: idx must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(dist), "vf_umap_smooth_knn_query: dist must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(sigma), "vf_umap_smooth_knn_query: sigma must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(strength), "vf_umap_smooth_knn_query: strength must be 4-byte aligned");
    VF_REQUIRE(m >= 1 && m <= VF_UMAP_TRANSFORM_MAX_M, "vf_umap_smooth_knn_query: m=%d outside 1 .. %d", m, VF_UMAP_TRANSFORM_MAX_M);
    VF_REQUIRE(Rq >= 0, "vf_umap_smooth_knn_query: Rq=%ld must not be negative", (long)Rq);
    VF_REQUIRE(Rq <= VF_UMAP_MAX_R, "vf_umap_smooth_knn_query: Rq=%ld is above 2^24", (long)Rq);
    VF_REQUIRE(ld_idx >= m, "vf_umap_smooth_knn_query: ld_idx=%ld is below m=%d", (long)ld_idx, m);
    VF_REQUIRE(ld_dist >= m, "vf_umap_smooth_knn_query: ld_dist=%ld is below m=%d", (long)ld_dist, m);
    VF_REQUIRE(ld_strength >= m, "vf_umap_smooth_knn_query: ld_strength=%ld is below m=%d", (long)ld_strength, m);
    if (Rq == 0) return VF_OK;
    const float target = (float)__builtin_log2((double)m);
    hipLaunchKernelGGL(umap_smooth_knn_query_kernel, dim3((unsigned)((Rq + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), dim3(THREADS), 0,
                       (hipStream_t)stream, idx, ld_idx, dist, ld_dist, (int)Rq, m, mean_dist, target, sigma, strength, ld_strength);
    VF_CHECK_LAUNCH("vf_umap_smooth_knn_query");
    return VF_OK;
}

extern "C" int vf_umap_init_transform(const int32_t* idx, int64_t ld_idx, const float* strength, int64_t ld_strength, int64_t Rq, int m,
                                      const float* Y, int64_t ldy, int64_t R, int dim, float* Yq, int64_t ldq, void* stream) {
    VF_REQUIRE(idx, "vf_umap_init_transform: null pointer idx");
    VF_REQUIRE(strength, "vf_umap_init_transform: null pointer strength");
    VF_REQUIRE(Y, "vf_umap_init_transform: null pointer Y");
    VF_REQUIRE(Yq, "vf_umap_init_transform: null pointer Yq");
    VF_REQUIRE(VF_ALIGNED4(idx), "vf_umap_init_transform: idx must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(strength), "vf_umap_init_transform: strength must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(Y), "vf_umap_init_transform: Y must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(Yq), "vf_umap_init_transform: Yq must be 4-byte aligned");
    VF_REQUIRE(Y != Yq, "vf_umap_init_transform: Y and Yq must be two buffers");
    VF_REQUIRE(m >= 1 && m <= VF_UMAP_TRANSFORM_MAX_M, "vf_umap_init_transform: m=%d outside 1 .. %d", m, VF_UMAP_TRANSFORM_MAX_M);
    VF_REQUIRE(Rq >= 0, "vf_umap_init_transform: Rq=%ld must not be negative", (long)Rq);
    VF_REQUIRE(Rq <= VF_UMAP_MAX_R, "vf_umap_init_transform: Rq=%ld is above 2^24", (long)Rq);
    VF_REQUIRE(R >= 0, "vf_umap_init_transform: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R <= VF_UMAP_MAX_R, "vf_umap_init_transform: R=%ld is above 2^24", (long)R);
    VF_REQUIRE(dim >= 1 && dim <= VF_UMAP_MAX_DIM, "vf_umap_init_transform: dim=%d outside 1 .. %d", dim, VF_UMAP_MAX_DIM);
    VF_REQUIRE(ld_idx >= m, "vf_umap_init_transform: ld_idx=%ld is below m=%d", (long)ld_idx, m);
    VF_REQUIRE(ld_strength >= m, "vf_umap_init_transform: ld_strength=%ld is below m=%d", (long)ld_strength, m);
    VF_REQUIRE(ldy >= dim, "vf_umap_init_transform: ldy=%ld is below dim=%d", (long)ldy, dim);
    VF_REQUIRE(ldq >= dim, "vf_umap_init_transform: ldq=%ld is below dim=%d", (long)ldq, dim);
    if (Rq == 0) return VF_OK;
    hipLaunchKernelGGL(umap_init_transform_kernel, dim3((unsigned)((Rq + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), dim3(THREADS), 0,
                       (hipStream_t)stream, idx, ld_idx, strength, ld_strength, (int)Rq, m, Y, ldy, (int)R, dim, Yq, ldq);
    VF_CHECK_LAUNCH("vf_umap_init_transform");
    return VF_OK;
}

extern "C" int vf_umap_layout_transform(const int32_t* idx, int64_t ld_idx, const int32_t* samples, int64_t ld_samples, int64_t Rq,
                                        int m, int64_t first_row, const float* Y, int64_t ldy, int64_t R, int dim, float* Yq,
                                        int64_t ldq, int epoch_begin, int epoch_end, int N, float a, float b, float gamma,
                                        float learning_rate, int negative_sample_rate, int64_t seed, void* stream) {
    VF_REQUIRE(idx, "vf_umap_layout_transform: null pointer idx");
    VF_REQUIRE(samples, "vf_umap_layout_transform: null pointer samples");
    VF_REQUIRE(Y, "vf_umap_layout_transform: null pointer Y");
    VF_REQUIRE(Yq, "vf_umap_layout_transform: null pointer Yq");
    VF_REQUIRE(VF_ALIGNED4(idx), "vf_umap_layout_transform: idx must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(samples), "vf_umap_layout_transform: samples must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(Y), "vf_umap_layout_transform: Y must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(Yq), "vf_umap_layout_transform: Yq must be 4-byte aligned");
    VF_REQUIRE(Y != Yq, "vf_umap_layout_transform: Y and Yq must be two buffers");
    VF_REQUIRE(m >= 1 && m <= VF_UMAP_TRANSFORM_MAX_M, "vf_umap_layout_transform: m=%d outside 1 .. %d", m, VF_UMAP_TRANSFORM_MAX_M);
    VF_REQUIRE(Rq >= 0, "vf_umap_layout_transform: Rq=%ld must not be negative", (long)Rq);
    VF_REQUIRE(Rq <= VF_UMAP_MAX_R, "vf_umap_layout_transform: Rq=%ld is above 2^24", (long)Rq);
    VF_REQUIRE(first_row >= 0, "vf_umap_layout_transform: first_row=%ld must not be negative", (long)first_row);
    VF_REQUIRE(first_row <= ((int64_t)1 << 32) - Rq, "vf_umap_layout_transform: first_row=%ld + Rq=%ld is above 2^32", (long)first_row, (long)Rq);
    VF_REQUIRE(R >= 0, "vf_umap_layout_transform: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R <= VF_UMAP_MAX_R, "vf_umap_layout_transform: R=%ld is above 2^24", (long)R);
    VF_REQUIRE(dim >= 1 && dim <= VF_UMAP_MAX_DIM, "vf_umap_layout_transform: dim=%d outside 1 .. %d", dim, VF_UMAP_MAX_DIM);
    VF_REQUIRE(ld_idx >= m, "vf_umap_layout_transform: ld_idx=%ld is below m=%d", (long)ld_idx, m);
    VF_REQUIRE(ld_samples >= m, "vf_umap_layout_transform: ld_samples=%ld is below m=%d", (long)ld_samples, m);
    VF_REQUIRE(ldy >= dim, "vf_umap_layout_transform: ldy=%ld is below dim=%d", (long)ldy, dim);
    VF_REQUIRE(ldq >= dim, "vf_umap_layout_transform: ldq=%ld is below dim=%d", (long)ldq, dim);
    VF_REQUIRE(N >= 1, "vf_umap_layout_transform: N=%d must be at least 1", N);
    VF_REQUIRE(epoch_begin >= 0, "vf_umap_layout_transform: epoch_begin=%d must not be negative", epoch_begin);
    VF_REQUIRE(epoch_begin <= epoch_end, "vf_umap_layout_transform: epoch_begin=%d is above epoch_end=%d", epoch_begin, epoch_end);
    VF_REQUIRE(epoch_end <= N, "vf_umap_layout_transform: epoch_end=%d is above N=%d", epoch_end, N);
    VF_REQUIRE(negative_sample_rate >= 0, "vf_umap_layout_transform: negative_sample_rate=%d must not be negative", negative_sample_rate);
    VF_REQUIRE(negative_sample_rate <= (1 << 20), "vf_umap_layout_transform: negative_sample_rate=%d is above 2^20", negative_sample_rate);
    if (Rq == 0 || epoch_begin == epoch_end) return VF_OK;
    VF_REQUIRE(R >= 1, "vf_umap_layout_transform: R=%ld training rows: the queries have nothing to be placed among", (long)R);
    const uint32_t seed0 = mix32((uint32_t)(uint64_t)seed + 0x9E3779B9u);
    const float lr4 = learning_rate / 4.f;
    const dim3 grid((unsigned)((Rq + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK));
    for (int n0 = epoch_begin; n0 < epoch_end; n0 += VF_UMAP_TRANSFORM_EPOCHS_PER_LAUNCH) {
        const int n1 = epoch_end - n0 > VF_UMAP_TRANSFORM_EPOCHS_PER_LAUNCH ? n0 + VF_UMAP_TRANSFORM_EPOCHS_PER_LAUNCH : epoch_end;
#define VF_UMAP_DIM(D)                                                                                                             \
    case D:                                                                                                                        \
        hipLaunchKernelGGL(umap_layout_transform_kernel<D>, grid, dim3(THREADS), 0, (hipStream_t)stream, idx, ld_idx, samples,     \
                           ld_samples, (int)Rq, m, (uint32_t)first_row, Y, ldy, (uint32_t)R, Yq, ldq, n0, n1, N, a, b, gamma, lr4, \
                           negative_sample_rate, seed0);                                                                           \
        break;
        switch (dim) {
            VF_UMAP_DIM(1) VF_UMAP_DIM(2) VF_UMAP_DIM(3) VF_UMAP_DIM(4) VF_UMAP_DIM(5) VF_UMAP_DIM(6) VF_UMAP_DIM(7) VF_UMAP_DIM(8)
        }
#undef VF_UMAP_DIM
        VF_CHECK_LAUNCH("vf_umap_layout_transform");
    }
    return VF_OK;
}

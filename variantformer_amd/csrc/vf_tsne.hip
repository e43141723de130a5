// t-SNE with the exact gradient (include/vf_hip_tsne.h): the perplexity search of every neighbour list, the symmetric sum over
// the CSR graph, the all-pairs repulsion pass and the iterations of the descent.  Every sum has the order the header states and
// there is no atomic, so a run has one result, bit for bit, and can be split at any iteration.  Nothing here may contract into
// an fma (the pragma below).  expf / logf / sqrtf and the divisions are hipcc's fp32 library forms; the pair kernel's 1 / (1 + q)
// is the hardware reciprocal.  The file is built without -fno-honor-nans (csrc/build.py: that flag is vf_attn.hip's) because
// absent entries are recognised by their NaN / Inf.
#include "vf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int ROWS_PER_BLOCK = THREADS / VF_WAVE;
constexpr int PER_LANE = (VF_TSNE_MAX_M + VF_WAVE) / VF_WAVE;       // 4 entries of a list per lane
constexpr int TILE = VF_TSNE_TILE;
constexpr int ATTR_THREADS = 64;           // one vertex per thread: small blocks spread a few thousand vertices over the CUs


// One wavefront per row; entry t lives on lane t mod 64 and stays in registers across the search.
__global__ __launch_bounds__(THREADS) void tsne_perplexity_kernel(const int32_t* __restrict__ idx, int64_t ld_idx,
                                                                  const float* __restrict__ d2, int64_t ld_d2, int R, int m, float target,
                                                                  float* __restrict__ beta_out, float* __restrict__ p_cond, int64_t ld_p) {
    const int lane = threadIdx.x & (VF_WAVE - 1);
    const int i = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= R) return;                                                   // the whole wavefront leaves
    float x[PER_LANE], P[PER_LANE];
    bool present[PER_LANE];
    float lo = __builtin_inff();
#pragma unroll
    for (int q = 0; q < PER_LANE; ++q) {
        const int t = lane + q * VF_WAVE;
        const bool in_row = t < m;
        const int j = in_row ? idx[(int64_t)i * ld_idx + t] : -1;
        const float d = in_row ? d2[(int64_t)i * ld_d2 + t] : 0.f;
        present[q] = in_row && j >= 0 && j != i && finite_bits(d);
        x[q] = present[q] ? d : 0.f;
        P[q] = 0.f;
        if (present[q]) lo = fminf(lo, d);
    }
    float any = 0.f;
#pragma unroll
    for (int q = 0; q < PER_LANE; ++q) any += present[q] ? 1.f : 0.f;
    any = wave_sum(any);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) lo = fminf(lo, __shfl_xor(lo, off));
#pragma unroll
    for (int q = 0; q < PER_LANE; ++q) x[q] = present[q] ? x[q] - lo : 0.f;

    float beta = 1.f, beta_min = -__builtin_inff(), beta_max = __builtin_inff();
    if (any > 0.f) {
        for (int step = 0; step < VF_TSNE_PERPLEXITY_STEPS; ++step) {
            float e[PER_LANE], s = 0.f;
#pragma unroll
            for (int q = 0; q < PER_LANE; ++q) {
                e[q] = present[q] ? expf(-(x[q] * beta)) : 0.f;
                s += e[q];
            }
            const float S = wave_sum(s);                                  // the same bits in every lane
            float dp = 0.f;
#pragma unroll
            for (int q = 0; q < PER_LANE; ++q) {
                P[q] = e[q] / S;
                dp += x[q] * P[q];
            }
            const float D = wave_sum(dp);
            const float H = logf(S) + beta * D;
            const float diff = H - target;
            if (fabsf(diff) <= VF_TSNE_PERPLEXITY_TOL) break;             // uniform branches from here on
            if (step == VF_TSNE_PERPLEXITY_STEPS - 1) break;
            if (diff > 0.f) {
                beta_min = beta;
                beta = beta_max == __builtin_inff() ? beta * 2.f : (beta + beta_max) / 2.f;
            } else {
                beta_max = beta;
                beta = beta_min == -__builtin_inff() ? beta / 2.f : (beta + beta_min) / 2.f;
            }
        }
    } else {
        beta = 0.f;
    }
    if (lane == 0) beta_out[i] = beta;
#pragma unroll
    for (int q = 0; q < PER_LANE; ++q) {
        const int t = lane + q * VF_WAVE;
        if (t < m) p_cond[(int64_t)i * ld_p + t] = present[q] ? P[q] : 0.f;
    }
}

// p_cond of `other` in row `row`'s list: the first match among m entries, +0 without one.
__device__ __forceinline__ float list_value(const int32_t* __restrict__ idx, int64_t ld_idx, const float* __restrict__ val, int64_t ld_val,
                                            int m, int row, int other) {
    const int32_t* list = idx + (int64_t)row * ld_idx;
    for (int t = 0; t < m; ++t)
        if (list[t] == other) return val[(int64_t)row * ld_val + t];
    return 0.f;
}

// One wavefront per CSR row; its lanes take the row's entries 64 at a time.
__global__ __launch_bounds__(THREADS) void tsne_joint_kernel(const int32_t* __restrict__ idx, int64_t ld_idx, const float* __restrict__ p_cond,
                                                             int64_t ld_p, int R, int m, const int64_t* __restrict__ rowptr,
                                                             const int32_t* __restrict__ col, int64_t nnz, float* __restrict__ p) {
    const int lane = threadIdx.x & (VF_WAVE - 1);
    const int i = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= R) return;
    int64_t begin = rowptr[i], end = rowptr[i + 1];
    begin = begin < 0 ? 0 : begin;
    end = end > nnz ? nnz : end;
    for (int64_t e = begin + lane; e < end; e += VF_WAVE) {
        const int j = col[e];
        const float a = list_value(idx, ld_idx, p_cond, ld_p, m, i, j);
        const float b = (j >= 0 && j < R) ? list_value(idx, ld_idx, p_cond, ld_p, m, j, i) : 0.f;
        p[e] = a + b;
    }
}

// w = t^((dof + 1) / 2) of one pair from its squared distance, and the differences
template <int DIM, int DOF>
__device__ __forceinline__ float pair_weight(const float (&y)[DIM], const float (&o)[DIM], float (&diff)[DIM]) {
    float d2 = 0.f;
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
        diff[c] = y[c] - o[c];
        d2 += diff[c] * diff[c];
    }
    const float q = DOF == 1 ? d2 : (DOF == 2 ? d2 * 0.5f : d2 * (1.f / 3.f));
    const float t = __builtin_amdgcn_rcpf(1.f + q);
    return DOF == 1 ? t : (DOF == 2 ? t * sqrtf(t) : t * t);
}

template <int DIM, int DOF, bool CHECK>
__device__ __forceinline__ void tile_pairs(const float* __restrict__ tile, int n, int j0, int i, const float (&y)[DIM], float (&acc)[DIM + 1]) {
#pragma unroll 4
    for (int jj = 0; jj < n; ++jj) {
        float o[DIM], diff[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) o[c] = tile[jj * DIM + c];          // one address for the whole wavefront: a broadcast
        const float w = pair_weight<DIM, DOF>(y, o, diff);
        const float ww = w * w;
        if (!CHECK || j0 + jj != i) {
#pragma unroll
            for (int c = 0; c < DIM; ++c) acc[c] += ww * diff[c];
            acc[DIM] += w;
        }
    }
}

// One thread per (vertex, split); blockIdx.y is the split.  The rows j of the split come TILE at a time through LDS.
template <int DIM, int DOF>
__global__ __launch_bounds__(TILE) void tsne_repulsion_kernel(const float* __restrict__ Y, int64_t ld, int R, int L, float* __restrict__ part) {
    __shared__ float tile[TILE * DIM];
    const int i0 = blockIdx.x * TILE;
    const int i = i0 + threadIdx.x;
    const int s = blockIdx.y;
    const int64_t lo64 = (int64_t)s * L, hi64 = lo64 + L;
    const int jbegin = (int)(lo64 < R ? lo64 : R), jend = (int)(hi64 < R ? hi64 : R);
    float y[DIM], acc[DIM + 1];
#pragma unroll
    for (int c = 0; c < DIM; ++c) y[c] = i < R ? Y[(int64_t)i * ld + c] : 0.f;
#pragma unroll
    for (int c = 0; c <= DIM; ++c) acc[c] = 0.f;
    for (int j0 = jbegin; j0 < jend; j0 += TILE) {
        const int n = jend - j0 < TILE ? jend - j0 : TILE;
        __syncthreads();                                                  // the tile before is no longer read
        if ((int)threadIdx.x < n) {
#pragma unroll
            for (int c = 0; c < DIM; ++c) tile[threadIdx.x * DIM + c] = Y[(int64_t)(j0 + (int)threadIdx.x) * ld + c];
        }
        __syncthreads();
        if (j0 < i0 + TILE && j0 + n > i0)                                // the tile may hold a vertex of this block: uniform
            tile_pairs<DIM, DOF, true>(tile, n, j0, i, y, acc);
        else
            tile_pairs<DIM, DOF, false>(tile, n, j0, i, y, acc);
    }
    if (i < R) {
        float* out = part + ((int64_t)s * R + i) * (DIM + 1);
#pragma unroll
        for (int c = 0; c <= DIM; ++c) out[c] = acc[c];
    }
}

// One thread per vertex: the CSR row in entry order.  Reads Y only.
template <int DIM, int DOF>
__global__ __launch_bounds__(ATTR_THREADS) void tsne_attraction_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                       const float* __restrict__ p, int64_t nnz, int R,
                                                                       const float* __restrict__ Y, int64_t ld, float* __restrict__ attr) {
    const int i = blockIdx.x * ATTR_THREADS + threadIdx.x;
    if (i >= R) return;
    float y[DIM], acc[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
        y[c] = Y[(int64_t)i * ld + c];
        acc[c] = 0.f;
    }
    int64_t begin = rowptr[i], end = rowptr[i + 1];
    begin = begin < 0 ? 0 : begin;
    end = end > nnz ? nnz : end;
#pragma unroll 4
    for (int64_t e = begin; e < end; ++e) {
        const int j = col[e];
        if (j < 0 || j >= R) continue;
        float o[DIM], diff[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) o[c] = Y[(int64_t)j * ld + c];
        const float w = pair_weight<DIM, DOF>(y, o, diff);
        const float pw = p[e] * w;
#pragma unroll
        for (int c = 0; c < DIM; ++c) acc[c] += pw * diff[c];
    }
#pragma unroll
    for (int c = 0; c < DIM; ++c) attr[(int64_t)i * DIM + c] = acc[c];
}

// Chunk b of the column-dim values of part, in fp64: thread u adds k = b * C + u, + Z_THREADS, ..; then the tree.
__global__ __launch_bounds__(VF_TSNE_Z_THREADS) void tsne_z_kernel(const float* __restrict__ part, int64_t total, int64_t C, int width,
                                                                   double* __restrict__ zpart) {
    __shared__ double x[VF_TSNE_Z_THREADS];
    const int u = threadIdx.x;
    const int64_t begin = (int64_t)blockIdx.x * C;
    int64_t end = begin + C;
    end = end > total ? total : end;
    double s = 0.0;
    for (int64_t k = begin + u; k < end; k += VF_TSNE_Z_THREADS) s += (double)part[k * width + (width - 1)];
    x[u] = s;
    __syncthreads();
    for (int stride = VF_TSNE_Z_THREADS / 2; stride > 0; stride >>= 1) {
        if (u < stride) x[u] += x[u + stride];
        __syncthreads();
    }
    if (u == 0) zpart[blockIdx.x] = x[0];
}

// One thread per vertex: the only kernel that writes Y, and every thread reads its own row alone.
template <int DIM>
__global__ __launch_bounds__(THREADS) void tsne_update_kernel(const float* __restrict__ part, const float* __restrict__ attr,
                                                              const double* __restrict__ zpart, int R, int splits, float* __restrict__ Y,
                                                              float* __restrict__ update, float* __restrict__ gains, int64_t ld, float G,
                                                              float exaggeration, float momentum, float learning_rate, float min_gain,
                                                              double* __restrict__ zsum) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    double Z = 0.0;
    for (int b = 0; b < VF_TSNE_Z_BLOCKS; ++b) Z += zpart[b];
    if (blockIdx.x == 0 && threadIdx.x == 0) *zsum = Z;
    if (i >= R) return;
    const float Zf = (float)Z;
    float rep[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) rep[c] = 0.f;
    for (int s = 0; s < splits; ++s) {
        const float* row = part + ((int64_t)s * R + i) * (DIM + 1);
#pragma unroll
        for (int c = 0; c < DIM; ++c) rep[c] += row[c];
    }
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
        const int64_t at = (int64_t)i * ld + c;
        float grad = G * (exaggeration * attr[(int64_t)i * DIM + c] - rep[c] / Zf);
        const float u = update[at];
        float g = gains[at];
        g = (u * grad < 0.f) ? g + 0.2f : g * 0.8f;
        g = g < min_gain ? min_gain : g;
        grad = grad * g;
        const float un = momentum * u - learning_rate * grad;
        gains[at] = g;
        update[at] = un;
        Y[at] = Y[at] + un;
    }
}

template <int DIM, int DOF>
void launch_repulsion(const float* Y, int64_t ld, int R, int splits, float* part, hipStream_t stream) {
    const int L = (int)(((int64_t)R + splits - 1) / splits);
    hipLaunchKernelGGL((tsne_repulsion_kernel<DIM, DOF>), dim3((unsigned)((R + TILE - 1) / TILE), (unsigned)splits), dim3(TILE), 0, stream,
                       Y, ld, R, L, part);
}

template <int DIM, int DOF>
void launch_attraction(const int64_t* rowptr, const int32_t* col, const float* p, int64_t nnz, int R, const float* Y, int64_t ld,
                       float* attr, hipStream_t stream) {
    hipLaunchKernelGGL((tsne_attraction_kernel<DIM, DOF>), dim3((unsigned)((R + ATTR_THREADS - 1) / ATTR_THREADS)), dim3(ATTR_THREADS), 0,
                       stream, rowptr, col, p, nnz, R, Y, ld, attr);
}

// every (dim, dof) of the two pair kernels
#define VF_TSNE_DISPATCH(CALL)                          \
    switch (dim * 4 + dof) {                            \
        case 1 * 4 + 1: CALL(1, 1); break;              \
        case 1 * 4 + 2: CALL(1, 2); break;              \
        case 1 * 4 + 3: CALL(1, 3); break;              \
        case 2 * 4 + 1: CALL(2, 1); break;              \
        case 2 * 4 + 2: CALL(2, 2); break;              \
        case 2 * 4 + 3: CALL(2, 3); break;              \
        case 3 * 4 + 1: CALL(3, 1); break;              \
        case 3 * 4 + 2: CALL(3, 2); break;              \
        case 3 * 4 + 3: CALL(3, 3); break;              \
        case 4 * 4 + 1: CALL(4, 1); break;              \
        case 4 * 4 + 2: CALL(4, 2); break;              \
        case 4 * 4 + 3: CALL(4, 3); break;              \
    }


}  // namespace

extern "C" int vf_tsne_perplexity(const int32_t* idx, int64_t ld_idx, const float* d2, int64_t ld_d2, int64_t R, int m, float perplexity,
                                  float* beta, float* p_cond, int64_t ld_p, void* stream) {
    VF_REQUIRE(idx, "vf_tsne_perplexity: null pointer idx");
    VF_REQUIRE(d2, "vf_tsne_perplexity: null pointer d2");
    VF_REQUIRE(beta, "vf_tsne_perplexity: null pointer beta");
    VF_REQUIRE(p_cond, "vf_tsne_perplexity: null pointer p_cond");
    VF_REQUIRE(VF_ALIGNED4(idx), "vf_tsne_perplexity: idx must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(d2), "vf_tsne_perplexity: d2 must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(beta), "vf_tsne_perplexity: beta must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(p_cond), "vf_tsne_perplexity: p_cond must be 4-byte aligned");
    VF_REQUIRE(m >= 1 && m <= VF_TSNE_MAX_M, "vf_tsne_perplexity: m=%d outside 1 .. %d", m, VF_TSNE_MAX_M);
    VF_REQUIRE(R >= 0, "vf_tsne_perplexity: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R <= VF_TSNE_MAX_R, "vf_tsne_perplexity: R=%ld is above 2^24", (long)R);
    VF_REQUIRE(ld_idx >= m, "vf_tsne_perplexity: ld_idx=%ld is below m=%d", (long)ld_idx, m);
    VF_REQUIRE(ld_d2 >= m, "vf_tsne_perplexity: ld_d2=%ld is below m=%d", (long)ld_d2, m);
    VF_REQUIRE(ld_p >= m, "vf_tsne_perplexity: ld_p=%ld is below m=%d", (long)ld_p, m);
    VF_REQUIRE(perplexity == perplexity && perplexity >= 1.f && perplexity < (float)m,
               "vf_tsne_perplexity: perplexity=%g must be a finite number in [1, m=%d)", (double)perplexity, m);
    if (R == 0) return VF_OK;
    const float target = (float)__builtin_log((double)perplexity);
    hipLaunchKernelGGL(tsne_perplexity_kernel, dim3((unsigned)((R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), dim3(THREADS), 0,
                       (hipStream_t)stream, idx, ld_idx, d2, ld_d2, (int)R, m, target, beta, p_cond, ld_p);
    VF_CHECK_LAUNCH("vf_tsne_perplexity");
    return VF_OK;
}

extern "C" int vf_tsne_joint(const int32_t* idx, int64_t ld_idx, const float* p_cond, int64_t ld_p, int64_t R, int m, const int64_t* rowptr,
                             const int32_t* col, int64_t nnz, float* p, void* stream) {
    VF_REQUIRE(idx, "vf_tsne_joint: null pointer idx");
    VF_REQUIRE(p_cond, "vf_tsne_joint: null pointer p_cond");
    VF_REQUIRE(rowptr, "vf_tsne_joint: null pointer rowptr");
    VF_REQUIRE(col || nnz == 0, "vf_tsne_joint: null pointer col");
    VF_REQUIRE(p || nnz == 0, "vf_tsne_joint: null pointer p");
    VF_REQUIRE(VF_ALIGNED4(idx), "vf_tsne_joint: idx must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(p_cond), "vf_tsne_joint: p_cond must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(rowptr), "vf_tsne_joint: rowptr must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(col), "vf_tsne_joint: col must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(p), "vf_tsne_joint: p must be 4-byte aligned");
    VF_REQUIRE(m >= 1 && m <= VF_TSNE_MAX_M, "vf_tsne_joint: m=%d outside 1 .. %d", m, VF_TSNE_MAX_M);
    VF_REQUIRE(R >= 0, "vf_tsne_joint: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R <= VF_TSNE_MAX_R, "vf_tsne_joint: R=%ld is above 2^24", (long)R);
    VF_REQUIRE(ld_idx >= m, "vf_tsne_joint: ld_idx=%ld is below m=%d", (long)ld_idx, m);
    VF_REQUIRE(ld_p >= m, "vf_tsne_joint: ld_p=%ld is below m=%d", (long)ld_p, m);
    VF_REQUIRE(nnz >= 0, "vf_tsne_joint: nnz=%ld must not be negative", (long)nnz);
    if (R == 0 || nnz == 0) return VF_OK;
    hipLaunchKernelGGL(tsne_joint_kernel, dim3((unsigned)((R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), dim3(THREADS), 0, (hipStream_t)stream,
                       idx, ld_idx, p_cond, ld_p, (int)R, m, rowptr, col, nnz, p);
    VF_CHECK_LAUNCH("vf_tsne_joint");
    return VF_OK;
}

extern "C" int vf_tsne_repulsion(const float* Y, int64_t ld, int64_t R, int dim, int dof, int splits, float* part, void* stream) {
    VF_REQUIRE(Y, "vf_tsne_repulsion: null pointer Y");
    VF_REQUIRE(part, "vf_tsne_repulsion: null pointer part");
    VF_REQUIRE(VF_ALIGNED4(Y), "vf_tsne_repulsion: Y must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(part), "vf_tsne_repulsion: part must be 4-byte aligned");
    VF_REQUIRE(R >= 0, "vf_tsne_repulsion: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R <= VF_TSNE_MAX_R, "vf_tsne_repulsion: R=%ld is above 2^24", (long)R);
    VF_REQUIRE(dim >= 1 && dim <= VF_TSNE_MAX_DIM, "vf_tsne_repulsion: dim=%d outside 1 .. %d", dim, VF_TSNE_MAX_DIM);
    VF_REQUIRE(ld >= dim, "vf_tsne_repulsion: ld=%ld is below dim=%d", (long)ld, dim);
    VF_REQUIRE(dof >= 1 && dof <= 3, "vf_tsne_repulsion: dof=%d outside 1 .. 3", dof);
    VF_REQUIRE(splits >= 1 && splits <= VF_TSNE_MAX_SPLITS, "vf_tsne_repulsion: splits=%d outside 1 .. %d", splits, VF_TSNE_MAX_SPLITS);
    if (R == 0) return VF_OK;
#define VF_TSNE_REP(D, F) launch_repulsion<D, F>(Y, ld, (int)R, splits, part, (hipStream_t)stream)
    VF_TSNE_DISPATCH(VF_TSNE_REP)
#undef VF_TSNE_REP
    VF_CHECK_LAUNCH("vf_tsne_repulsion");
    return VF_OK;
}

extern "C" int vf_tsne_descent(const int64_t* rowptr, const int32_t* col, const float* p, int64_t nnz, int64_t R, int dim, float* Y,
                               float* update, float* gains, int64_t ld, int iter_begin, int iter_end, float exaggeration, float momentum,
                               float learning_rate, float min_gain, int dof, int splits, void* work, int64_t work_bytes, double* zsum,
                               void* stream) {
    VF_REQUIRE(rowptr, "vf_tsne_descent: null pointer rowptr");
    VF_REQUIRE(col || nnz == 0, "vf_tsne_descent: null pointer col");
    VF_REQUIRE(p || nnz == 0, "vf_tsne_descent: null pointer p");
    VF_REQUIRE(Y, "vf_tsne_descent: null pointer Y");
    VF_REQUIRE(update, "vf_tsne_descent: null pointer update");
    VF_REQUIRE(gains, "vf_tsne_descent: null pointer gains");
    VF_REQUIRE(work, "vf_tsne_descent: null pointer work");
    VF_REQUIRE(zsum || iter_begin == iter_end, "vf_tsne_descent: null pointer zsum");
    VF_REQUIRE(VF_ALIGNED8(rowptr), "vf_tsne_descent: rowptr must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(col), "vf_tsne_descent: col must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(p), "vf_tsne_descent: p must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(Y), "vf_tsne_descent: Y must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(update), "vf_tsne_descent: update must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(gains), "vf_tsne_descent: gains must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(work), "vf_tsne_descent: work must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(zsum), "vf_tsne_descent: zsum must be 8-byte aligned");
    VF_REQUIRE(R >= 0, "vf_tsne_descent: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R <= VF_TSNE_MAX_R, "vf_tsne_descent: R=%ld is above 2^24", (long)R);
    VF_REQUIRE(nnz >= 0, "vf_tsne_descent: nnz=%ld must not be negative", (long)nnz);
    VF_REQUIRE(dim >= 1 && dim <= VF_TSNE_MAX_DIM, "vf_tsne_descent: dim=%d outside 1 .. %d", dim, VF_TSNE_MAX_DIM);
    VF_REQUIRE(ld >= dim, "vf_tsne_descent: ld=%ld is below dim=%d", (long)ld, dim);
    VF_REQUIRE(dof >= 1 && dof <= 3, "vf_tsne_descent: dof=%d outside 1 .. 3", dof);
    VF_REQUIRE(splits >= 1 && splits <= VF_TSNE_MAX_SPLITS, "vf_tsne_descent: splits=%d outside 1 .. %d", splits, VF_TSNE_MAX_SPLITS);
    VF_REQUIRE(iter_begin >= 0, "vf_tsne_descent: iter_begin=%d must not be negative", iter_begin);
    VF_REQUIRE(iter_begin <= iter_end, "vf_tsne_descent: iter_begin=%d is above iter_end=%d", iter_begin, iter_end);
    VF_REQUIRE(work_bytes >= VF_TSNE_WORK_BYTES(R, dim, splits), "vf_tsne_descent: work_bytes=%ld is below the %ld this call needs",
               (long)work_bytes, (long)VF_TSNE_WORK_BYTES(R, dim, splits));
    if (R == 0 || iter_begin == iter_end) return VF_OK;
    hipStream_t st = (hipStream_t)stream;
    double* zpart = (double*)work;
    float* part = (float*)((char*)work + 8 * VF_TSNE_Z_BLOCKS);
    float* attr = part + (int64_t)splits * R * (dim + 1);
    const int64_t total = (int64_t)splits * R;
    const int64_t C = (total + VF_TSNE_Z_BLOCKS - 1) / VF_TSNE_Z_BLOCKS;
    const float G = (float)(2.0 * (dof + 1) / dof);
    const unsigned rows = (unsigned)((R + THREADS - 1) / THREADS);
    for (int n = iter_begin; n < iter_end; ++n) {
#define VF_TSNE_REP(D, F) launch_repulsion<D, F>(Y, ld, (int)R, splits, part, st)
        VF_TSNE_DISPATCH(VF_TSNE_REP)
#undef VF_TSNE_REP
#define VF_TSNE_ATT(D, F) launch_attraction<D, F>(rowptr, col, p, nnz, (int)R, Y, ld, attr, st)
        VF_TSNE_DISPATCH(VF_TSNE_ATT)
#undef VF_TSNE_ATT
        hipLaunchKernelGGL(tsne_z_kernel, dim3(VF_TSNE_Z_BLOCKS), dim3(VF_TSNE_Z_THREADS), 0, st, part, total, C, dim + 1, zpart);
#define VF_TSNE_UPD(D)                                                                                                                  \
    case D:                                                                                                                             \
        hipLaunchKernelGGL(tsne_update_kernel<D>, dim3(rows), dim3(THREADS), 0, st, part, attr, zpart, (int)R, splits, Y, update, gains, ld, \
                           G, exaggeration, momentum, learning_rate, min_gain, zsum + (n - iter_begin));                                 \
        break;
        switch (dim) { VF_TSNE_UPD(1) VF_TSNE_UPD(2) VF_TSNE_UPD(3) VF_TSNE_UPD(4) }
#undef VF_TSNE_UPD
        VF_CHECK_LAUNCH("vf_tsne_descent");
    }
    return VF_OK;
}

// The spectral embedding's device work (include/vf_hip_spectral.h): weighted degrees, the three-term recurrence in the normalised
// adjacency S = D^-1/2 W D^-1/2 over a block of vectors (the Chebyshev filter; one step with (1, 0, 0) is S Y), the fp64 Gram
// matrix of two tall blocks and a tall block times a small fp64 matrix.  Every sum has the order the header states, nothing is
// atomic and no block waits for another, so numpy restates the results bit for bit.  Nothing here may contract into an fma (the
// pragma below); `/` and __builtin_sqrtf are hipcc's correctly rounded ones, as in vf_linkage.hip.
#include "vf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int ROWS_PER_BLOCK = THREADS / VF_WAVE;
constexpr int TILE = VF_TALL_GRAM_TILE;
constexpr int GRAM_OUTS = (VF_SPECTRAL_MAX_P * VF_SPECTRAL_MAX_P + THREADS - 1) / THREADS;      // outputs of one thread at most

// One wavefront per row, lane l takes the entries l, l + 64, ...
__global__ __launch_bounds__(THREADS) void graph_degree_kernel(const int64_t* __restrict__ rowptr, const float* __restrict__ w, int64_t nnz,
                                                               int R, float* __restrict__ deg, float* __restrict__ dinv_sqrt) {
    const int lane = threadIdx.x & (VF_WAVE - 1);
    const int i = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= R) return;                                                   // the whole wavefront leaves
    int64_t begin = rowptr[i], end = rowptr[i + 1];
    begin = begin < 0 ? 0 : begin;
    end = end > nnz ? nnz : end;
    float v = 0.f;
    for (int64_t e = begin + lane; e < end; e += VF_WAVE) v = v + w[e];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
    if (lane == 0) {
        deg[i] = v;
        dinv_sqrt[i] = v > 0.f ? 1.f / __builtin_sqrtf(v) : 0.f;
    }
}

// One wavefront per row: C = 1 << log_c columns x 64 / C entry groups.
__global__ __launch_bounds__(THREADS) void spmm_recur_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                             const float* __restrict__ w, int64_t nnz, int R,
                                                             const float* __restrict__ dinv_sqrt, int p, int log_c,
                                                             const float* __restrict__ Y, const float* __restrict__ W,
                                                             float* __restrict__ Z, int64_t ld, float c0, float c1, float c2) {
    const int lane = threadIdx.x & (VF_WAVE - 1);
    const int i = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= R) return;
    const int C = 1 << log_c, G = VF_WAVE >> log_c;
    const int c = lane & (C - 1), g = lane >> log_c;
    const bool active = c < p;
    float v = 0.f;
    if (c0 != 0.f) {                                                      // the same in every lane; a NaN coefficient is not 0
        int64_t begin = rowptr[i], end = rowptr[i + 1];
        begin = begin < 0 ? 0 : begin;
        end = end > nnz ? nnz : end;
        for (int64_t e = begin + g; e < end; e += G) {
            const int j = col[e];
            if (j < 0 || j >= R || !active) continue;
            const float s = w[e] * dinv_sqrt[j];
            v = v + s * Y[(int64_t)j * ld + c];
        }
        for (int off = 32; off >= C; off >>= 1) v = v + __shfl_xor(v, off);       // lanes of one column, groups g and g ^ (off / C)
        v = dinv_sqrt[i] * v;
    }
    if (g != 0 || !active) return;
    const int64_t at = (int64_t)i * ld + c;
    float z = 0.f;
    bool have = false;
    if (c0 != 0.f) {
        z = c0 * v;
        have = true;
    }
    if (c1 != 0.f) {
        const float t = c1 * Y[at];
        z = have ? z + t : t;
        have = true;
    }
    if (c2 != 0.f) {
        const float t = c2 * W[at];
        z = have ? z + t : t;
    }
    Z[at] = z;
}

// Block k: the partial sums of rows [k * chunk, (k + 1) * chunk), tiles of TILE rows staged in LDS, rows ascending.
__global__ __launch_bounds__(THREADS) void tall_gram_partial_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
                                                                    int64_t ldb, int64_t R, int p, int q, int64_t chunk,
                                                                    double* __restrict__ work) {
    __shared__ float sA[TILE * VF_SPECTRAL_MAX_P];
    __shared__ float sB[TILE * VF_SPECTRAL_MAX_P];
    const int tid = threadIdx.x;
    const int pq = p * q;
    const int64_t r0 = (int64_t)blockIdx.x * chunk;
    const int64_t r1 = r0 + chunk < R ? r0 + chunk : R;
    double acc[GRAM_OUTS];
    int ia[GRAM_OUTS], ib[GRAM_OUTS];
#pragma unroll
    for (int u = 0; u < GRAM_OUTS; ++u) {
        const int o = tid + u * THREADS;
        acc[u] = 0.0;
        ia[u] = o < pq ? o / q : 0;
        ib[u] = o < pq ? o - (o / q) * q : 0;
    }
    for (int64_t t0 = r0; t0 < r1; t0 += TILE) {
        const int n = (int)(r1 - t0 < TILE ? r1 - t0 : TILE);
        __syncthreads();                                                   // the tile before this one has been used
        for (int x = tid; x < n * p; x += THREADS) {
            const int r = x / p;
            sA[x] = A[(t0 + r) * lda + (x - r * p)];
        }
        for (int x = tid; x < n * q; x += THREADS) {
            const int r = x / q;
            sB[x] = B[(t0 + r) * ldb + (x - r * q)];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < GRAM_OUTS; ++u) {
            if (tid + u * THREADS >= pq) continue;
            double s = acc[u];
            for (int r = 0; r < n; ++r) s = s + (double)sA[r * p + ia[u]] * (double)sB[r * q + ib[u]];
            acc[u] = s;
        }
    }
#pragma unroll
    for (int u = 0; u < GRAM_OUTS; ++u) {
        const int o = tid + u * THREADS;
        if (o < pq) work[(int64_t)blockIdx.x * pq + o] = acc[u];
    }
}

// One block: every output's partials in block order.
__global__ __launch_bounds__(THREADS) void tall_gram_sum_kernel(const double* __restrict__ work, int nb, int pq, double* __restrict__ G) {
    for (int o = threadIdx.x; o < pq; o += THREADS) {
        double s = 0.0;
        for (int k = 0; k < nb; ++k) s = s + work[(int64_t)k * pq + o];
        G[o] = s;
    }
}

// One thread per output element.
__global__ __launch_bounds__(THREADS) void tall_mul_kernel(const float* __restrict__ X, int64_t ldx, int64_t R, int p,
                                                           const double* __restrict__ T, int q, float* __restrict__ Out, int64_t ldo) {
    const int64_t x = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (x >= R * q) return;
    const int64_t i = x / q;
    const int c = (int)(x - i * q);
    double s = 0.0;
    for (int k = 0; k < p; ++k) s = s + (double)X[i * ldx + k] * T[k * q + c];
    Out[i * ldo + c] = (float)s;
}


int64_t gram_chunk(int64_t R) {
    const int64_t span = (int64_t)TILE * VF_TALL_GRAM_MAX_BLOCKS;
    return TILE * ((R + span - 1) / span);
}

}  // namespace

extern "C" int vf_graph_degree(const int64_t* rowptr, const int32_t* col, const float* w, int64_t nnz, int64_t R, float* deg,
                               float* dinv_sqrt, void* stream) {
    VF_REQUIRE(rowptr, "vf_graph_degree: null pointer rowptr");
    VF_REQUIRE(col || nnz == 0, "vf_graph_degree: null pointer col");
    VF_REQUIRE(w || nnz == 0, "vf_graph_degree: null pointer w");
    VF_REQUIRE(deg, "vf_graph_degree: null pointer deg");
    VF_REQUIRE(dinv_sqrt, "vf_graph_degree: null pointer dinv_sqrt");
    VF_REQUIRE(VF_ALIGNED8(rowptr), "vf_graph_degree: rowptr must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(col), "vf_graph_degree: col must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(w), "vf_graph_degree: w must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(deg), "vf_graph_degree: deg must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(dinv_sqrt), "vf_graph_degree: dinv_sqrt must be 4-byte aligned");
    VF_REQUIRE(R >= 0, "vf_graph_degree: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R <= VF_SPECTRAL_MAX_R, "vf_graph_degree: R=%ld is above 2^24", (long)R);
    VF_REQUIRE(nnz >= 0, "vf_graph_degree: nnz=%ld must not be negative", (long)nnz);
    if (R == 0) return VF_OK;
    hipLaunchKernelGGL(graph_degree_kernel, dim3((unsigned)((R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), dim3(THREADS), 0,
                       (hipStream_t)stream, rowptr, w, nnz, (int)R, deg, dinv_sqrt);
    VF_CHECK_LAUNCH("vf_graph_degree");
    return VF_OK;
}

extern "C" int vf_spmm_recur(const int64_t* rowptr, const int32_t* col, const float* w, int64_t nnz, int64_t R, const float* dinv_sqrt,
                             int p, float* X0, float* X1, float* X2, int64_t ld, int steps, const float* coef, void* stream) {
    VF_REQUIRE(rowptr, "vf_spmm_recur: null pointer rowptr");
    VF_REQUIRE(col || nnz == 0, "vf_spmm_recur: null pointer col");
    VF_REQUIRE(w || nnz == 0, "vf_spmm_recur: null pointer w");
    VF_REQUIRE(dinv_sqrt, "vf_spmm_recur: null pointer dinv_sqrt");
    VF_REQUIRE(X0, "vf_spmm_recur: null pointer X0");
    VF_REQUIRE(X1, "vf_spmm_recur: null pointer X1");
    VF_REQUIRE(X2, "vf_spmm_recur: null pointer X2");
    VF_REQUIRE(coef || steps <= 0, "vf_spmm_recur: null pointer coef");
    VF_REQUIRE(VF_ALIGNED8(rowptr), "vf_spmm_recur: rowptr must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(col), "vf_spmm_recur: col must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(w), "vf_spmm_recur: w must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(dinv_sqrt), "vf_spmm_recur: dinv_sqrt must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(X0), "vf_spmm_recur: X0 must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(X1), "vf_spmm_recur: X1 must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(X2), "vf_spmm_recur: X2 must be 4-byte aligned");
    VF_REQUIRE(X0 != X1 && X0 != X2 && X1 != X2, "vf_spmm_recur: X0, X1 and X2 must be three buffers");
    VF_REQUIRE(R >= 0, "vf_spmm_recur: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R <= VF_SPECTRAL_MAX_R, "vf_spmm_recur: R=%ld is above 2^24", (long)R);
    VF_REQUIRE(nnz >= 0, "vf_spmm_recur: nnz=%ld must not be negative", (long)nnz);
    VF_REQUIRE(p >= 1 && p <= VF_SPECTRAL_MAX_P, "vf_spmm_recur: p=%d outside 1 .. %d", p, VF_SPECTRAL_MAX_P);
    VF_REQUIRE(ld >= p, "vf_spmm_recur: ld=%ld is below p=%d", (long)ld, p);
    VF_REQUIRE(steps >= 0, "vf_spmm_recur: steps=%d must not be negative", steps);
    if (R == 0 || steps == 0) return VF_OK;
    int log_c = 0;
    while ((1 << log_c) < p) ++log_c;
    float* X[3] = {X0, X1, X2};
    for (int t = 0; t < steps; ++t) {
        hipLaunchKernelGGL(spmm_recur_kernel, dim3((unsigned)((R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), dim3(THREADS), 0,
                           (hipStream_t)stream, rowptr, col, w, nnz, (int)R, dinv_sqrt, p, log_c, (const float*)X[t % 3],
                           (const float*)X[(t + 2) % 3], X[(t + 1) % 3], ld, coef[3 * t], coef[3 * t + 1], coef[3 * t + 2]);
        VF_CHECK_LAUNCH("vf_spmm_recur");
    }
    return VF_OK;
}

extern "C" int vf_tall_gram(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t R, int p, int q, double* G, double* work,
                            void* stream) {
    VF_REQUIRE(A, "vf_tall_gram: null pointer A");
    VF_REQUIRE(B, "vf_tall_gram: null pointer B");
    VF_REQUIRE(G, "vf_tall_gram: null pointer G");
    VF_REQUIRE(work, "vf_tall_gram: null pointer work");
    VF_REQUIRE(VF_ALIGNED4(A), "vf_tall_gram: A must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(B), "vf_tall_gram: B must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(G), "vf_tall_gram: G must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(work), "vf_tall_gram: work must be 8-byte aligned");
    VF_REQUIRE(R >= 0, "vf_tall_gram: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R <= VF_SPECTRAL_MAX_R, "vf_tall_gram: R=%ld is above 2^24", (long)R);
    VF_REQUIRE(p >= 1 && p <= VF_SPECTRAL_MAX_P, "vf_tall_gram: p=%d outside 1 .. %d", p, VF_SPECTRAL_MAX_P);
    VF_REQUIRE(q >= 1 && q <= VF_SPECTRAL_MAX_P, "vf_tall_gram: q=%d outside 1 .. %d", q, VF_SPECTRAL_MAX_P);
    VF_REQUIRE(lda >= p, "vf_tall_gram: lda=%ld is below p=%d", (long)lda, p);
    VF_REQUIRE(ldb >= q, "vf_tall_gram: ldb=%ld is below q=%d", (long)ldb, q);
    int nb = 0;
    if (R > 0) {
        const int64_t chunk = gram_chunk(R);
        nb = (int)((R + chunk - 1) / chunk);
        hipLaunchKernelGGL(tall_gram_partial_kernel, dim3((unsigned)nb), dim3(THREADS), 0, (hipStream_t)stream, A, lda, B, ldb, R, p, q,
                           chunk, work);
        VF_CHECK_LAUNCH("vf_tall_gram");
    }
    hipLaunchKernelGGL(tall_gram_sum_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, (const double*)work, nb, p * q, G);
    VF_CHECK_LAUNCH("vf_tall_gram");
    return VF_OK;
}

extern "C" int vf_tall_mul(const float* X, int64_t ldx, int64_t R, int p, const double* T, int q, float* Out, int64_t ldo, void* stream) {
    VF_REQUIRE(X, "vf_tall_mul: null pointer X");
    VF_REQUIRE(T, "vf_tall_mul: null pointer T");
    VF_REQUIRE(Out, "vf_tall_mul: null pointer Out");
    VF_REQUIRE(VF_ALIGNED4(X), "vf_tall_mul: X must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(T), "vf_tall_mul: T must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(Out), "vf_tall_mul: Out must be 4-byte aligned");
    VF_REQUIRE(Out != X, "vf_tall_mul: X and Out must be two buffers");
    VF_REQUIRE(R >= 0, "vf_tall_mul: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R <= VF_SPECTRAL_MAX_R, "vf_tall_mul: R=%ld is above 2^24", (long)R);
    VF_REQUIRE(p >= 1 && p <= VF_SPECTRAL_MAX_P, "vf_tall_mul: p=%d outside 1 .. %d", p, VF_SPECTRAL_MAX_P);
    VF_REQUIRE(q >= 1 && q <= VF_SPECTRAL_MAX_P, "vf_tall_mul: q=%d outside 1 .. %d", q, VF_SPECTRAL_MAX_P);
    VF_REQUIRE(ldx >= p, "vf_tall_mul: ldx=%ld is below p=%d", (long)ldx, p);
    VF_REQUIRE(ldo >= q, "vf_tall_mul: ldo=%ld is below q=%d", (long)ldo, q);
    if (R == 0) return VF_OK;
    hipLaunchKernelGGL(tall_mul_kernel, dim3((unsigned)((R * q + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, X, ldx, R, p,
                       T, q, Out, ldo);
    VF_CHECK_LAUNCH("vf_tall_mul");
    return VF_OK;
}

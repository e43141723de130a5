// Enrichment of gene clusters in annotation terms (include/vf_hip_enrich.h): the overlap counts of every (term, cluster) pair
// from the term-major CSR annotation, and the hypergeometric tail of every cell.  The counts are integers (LDS integer atomics
// alone, no global and no floating-point atomic); the tail is a running fp64 sum of + * / in the order the header states, so a
// run has one result, bit for bit, and can be split at any term.  Nothing here may contract into an fma (the pragma below).
// log, exp and log1p are hipcc's fp64 library forms; the device computes no lgamma.
#include "vf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = VF_ENRICH_THREADS;

// One block per term: a k-bin histogram in LDS, and one more word for the entries inside the universe.
__global__ __launch_bounds__(THREADS) void enrich_counts_kernel(const int64_t* __restrict__ termptr, const int32_t* __restrict__ gene,
                                                                int64_t nnz, const int32_t* __restrict__ labels, int G, int k,
                                                                int32_t* __restrict__ count, int64_t ldc, int32_t* __restrict__ size) {
    extern __shared__ int32_t bins[];                                     // k + 1 words
    const int t = blockIdx.x;
    for (int c = threadIdx.x; c <= k; c += THREADS) bins[c] = 0;
    __syncthreads();
    int64_t begin = termptr[t], end = termptr[t + 1];
    begin = begin < 0 ? 0 : begin;
    end = end > nnz ? nnz : end;
    int inside = 0;
    for (int64_t e = begin + threadIdx.x; e < end; e += THREADS) {
        const int g = gene[e];
        if (g < 0 || g >= G) continue;
        ++inside;
        const int c = labels[g];
        if (c >= 0 && c < k) atomicAdd(&bins[c], 1);
    }
    if (inside) atomicAdd(&bins[k], inside);
    __syncthreads();
    for (int c = threadIdx.x; c < k; c += THREADS) count[(int64_t)t * ldc + c] = bins[c];
    if (threadIdx.x == 0) size[t] = bins[k];
}

struct Sum {
    double s;
    int steps;
};

// t = s = 1 at x0, then the terms above it up to hi: every ratio is <= 1 when x0 is above the mode
__device__ __forceinline__ Sum sum_up(int64_t x0, int64_t hi, int64_t K, int64_t n, int64_t N) {
    double t = 1.0, s = 1.0;
    int steps = 0;
    for (int64_t i = x0; i < hi; ++i) {
        t = (t * (double)((K - i) * (n - i))) / (double)((i + 1) * (N - K - n + i + 1));
        s = s + t;
        ++steps;
        if (t < s * VF_ENRICH_STOP) break;
    }
    return {s, steps};
}

// the mirror image: the terms below x0 down to lo
__device__ __forceinline__ Sum sum_down(int64_t x0, int64_t lo, int64_t K, int64_t n, int64_t N) {
    double t = 1.0, s = 1.0;
    int steps = 0;
    for (int64_t i = x0; i > lo; --i) {
        t = (t * (double)(i * (N - K - n + i))) / (double)((K - i + 1) * (n - i + 1));
        s = s + t;
        ++steps;
        if (t < s * VF_ENRICH_STOP) break;
    }
    return {s, steps};
}

// the log of the probability of x0, lo <= x0 <= hi: every index lies in [0, N]
__device__ __forceinline__ double log_pmf(const double* __restrict__ lf, int64_t x0, int64_t K, int64_t n, int64_t N) {
    const double a = (lf[K] - lf[x0]) - lf[K - x0];
    const double b = (lf[N - K] - lf[n - x0]) - lf[N - K - n + x0];
    const double c = (lf[N] - lf[n]) - lf[N - n];
    return (a + b) - c;
}

// One thread per cell (t, c).
__global__ __launch_bounds__(THREADS) void hypergeom_tail_kernel(const int32_t* __restrict__ count, int64_t ldc, const int32_t* __restrict__ size,
                                                                 const int32_t* __restrict__ csize, int64_t cells, int k, int64_t N,
                                                                 const double* __restrict__ lf, int less, double* __restrict__ log_p,
                                                                 double* __restrict__ tail, int32_t* __restrict__ steps, int64_t ldo) {
    const int64_t cell = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (cell >= cells) return;
    const int64_t row = cell / k;
    const int c = (int)(cell - row * k);
    const int64_t x = count[row * ldc + c], K = size[row], n = csize[c];
    const int64_t at = row * ldo + c;
    if (K < 0 || K > N || n < 0 || n > N) {                               // not a distribution: nothing of logfact is read
        log_p[at] = __builtin_nan("");
        tail[at] = __builtin_nan("");
        steps[at] = 0;
        return;
    }
    const int64_t lo = n - (N - K) > 0 ? n - (N - K) : 0;
    const int64_t hi = K < n ? K : n;
    const int64_t mode = ((n + 1) * (K + 1)) / (N + 2);
    double lp;
    Sum r = {0.0, 0};
    if (!less) {
        if (x > hi) {
            lp = -__builtin_inf();
        } else if (x <= lo) {
            lp = 0.0;
        } else if (x > mode) {
            r = sum_up(x, hi, K, n, N);
            lp = log_pmf(lf, x, K, n, N) + log(r.s);
        } else {
            r = sum_down(x - 1, lo, K, n, N);
            lp = log1p(-exp(log_pmf(lf, x - 1, K, n, N) + log(r.s)));
        }
    } else {
        if (x < lo) {
            lp = -__builtin_inf();
        } else if (x >= hi) {
            lp = 0.0;
        } else if (x < mode) {
            r = sum_down(x, lo, K, n, N);
            lp = log_pmf(lf, x, K, n, N) + log(r.s);
        } else {
            r = sum_up(x + 1, hi, K, n, N);
            lp = log1p(-exp(log_pmf(lf, x + 1, K, n, N) + log(r.s)));
        }
    }
    log_p[at] = lp;
    tail[at] = r.s;
    steps[at] = r.steps;
}


}  // namespace

extern "C" int vf_enrich_counts(const int64_t* termptr, const int32_t* gene, int64_t nnz, int64_t T, const int32_t* labels, int64_t G, int k,
                                int32_t* count, int64_t ldc, int32_t* size, void* stream) {
    VF_REQUIRE(termptr, "vf_enrich_counts: null pointer termptr");
    VF_REQUIRE(gene || nnz == 0, "vf_enrich_counts: null pointer gene");
    VF_REQUIRE(labels, "vf_enrich_counts: null pointer labels");
    VF_REQUIRE(count, "vf_enrich_counts: null pointer count");
    VF_REQUIRE(size, "vf_enrich_counts: null pointer size");
    VF_REQUIRE(VF_ALIGNED8(termptr), "vf_enrich_counts: termptr must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(gene), "vf_enrich_counts: gene must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(labels), "vf_enrich_counts: labels must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(count), "vf_enrich_counts: count must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(size), "vf_enrich_counts: size must be 4-byte aligned");
    VF_REQUIRE(nnz >= 0, "vf_enrich_counts: nnz=%ld must not be negative", (long)nnz);
    VF_REQUIRE(T >= 0, "vf_enrich_counts: T=%ld must not be negative", (long)T);
    VF_REQUIRE(T <= VF_ENRICH_MAX_T, "vf_enrich_counts: T=%ld is above 2^24", (long)T);
    VF_REQUIRE(G >= 0, "vf_enrich_counts: G=%ld must not be negative", (long)G);
    VF_REQUIRE(G <= VF_ENRICH_MAX_N, "vf_enrich_counts: G=%ld is above 2^24", (long)G);
    VF_REQUIRE(k >= 1 && k <= VF_ENRICH_MAX_K, "vf_enrich_counts: k=%d outside 1 .. %d", k, VF_ENRICH_MAX_K);
    VF_REQUIRE(ldc >= k, "vf_enrich_counts: ldc=%ld is below k=%d", (long)ldc, k);
    if (T == 0) return VF_OK;
    hipLaunchKernelGGL(enrich_counts_kernel, dim3((unsigned)T), dim3(THREADS), (size_t)(k + 1) * sizeof(int32_t), (hipStream_t)stream, termptr,
                       gene, nnz, labels, (int)G, k, count, ldc, size);
    VF_CHECK_LAUNCH("vf_enrich_counts");
    return VF_OK;
}

extern "C" int vf_hypergeom_tail(const int32_t* count, int64_t ldc, const int32_t* size, const int32_t* csize, int64_t T, int k, int64_t N,
                                 const double* logfact, int alternative, double* log_p, double* tail, int32_t* steps, int64_t ldo,
                                 void* stream) {
    VF_REQUIRE(count, "vf_hypergeom_tail: null pointer count");
    VF_REQUIRE(size, "vf_hypergeom_tail: null pointer size");
    VF_REQUIRE(csize, "vf_hypergeom_tail: null pointer csize");
    VF_REQUIRE(logfact, "vf_hypergeom_tail: null pointer logfact");
    VF_REQUIRE(log_p, "vf_hypergeom_tail: null pointer log_p");
    VF_REQUIRE(tail, "vf_hypergeom_tail: null pointer tail");
    VF_REQUIRE(steps, "vf_hypergeom_tail: null pointer steps");
    VF_REQUIRE(VF_ALIGNED4(count), "vf_hypergeom_tail: count must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(size), "vf_hypergeom_tail: size must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(csize), "vf_hypergeom_tail: csize must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(logfact), "vf_hypergeom_tail: logfact must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(log_p), "vf_hypergeom_tail: log_p must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(tail), "vf_hypergeom_tail: tail must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(steps), "vf_hypergeom_tail: steps must be 4-byte aligned");
    VF_REQUIRE(T >= 0, "vf_hypergeom_tail: T=%ld must not be negative", (long)T);
    VF_REQUIRE(T <= VF_ENRICH_MAX_T, "vf_hypergeom_tail: T=%ld is above 2^24", (long)T);
    VF_REQUIRE(k >= 1 && k <= VF_ENRICH_MAX_K, "vf_hypergeom_tail: k=%d outside 1 .. %d", k, VF_ENRICH_MAX_K);
    VF_REQUIRE(N >= 0, "vf_hypergeom_tail: N=%ld must not be negative", (long)N);
    VF_REQUIRE(N <= VF_ENRICH_MAX_N, "vf_hypergeom_tail: N=%ld is above 2^24", (long)N);
    VF_REQUIRE(ldc >= k, "vf_hypergeom_tail: ldc=%ld is below k=%d", (long)ldc, k);
    VF_REQUIRE(ldo >= k, "vf_hypergeom_tail: ldo=%ld is below k=%d", (long)ldo, k);
    VF_REQUIRE(alternative == 0 || alternative == 1, "vf_hypergeom_tail: alternative=%d is neither 0 (greater) nor 1 (less)", alternative);
    if (T == 0) return VF_OK;
    const int64_t cells = T * k;
    hipLaunchKernelGGL(hypergeom_tail_kernel, dim3((unsigned)((cells + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, count,
                       ldc, size, csize, cells, k, N, logfact, alternative, log_p, tail, steps, ldo);
    VF_CHECK_LAUNCH("vf_hypergeom_tail");
    return VF_OK;
}

// Silhouette sums (vf_hip_silhouette.h): every query row's summed distance to the members of every cluster, by all pairs for the
// Euclidean distance and through the clusters' fp64 column sums for the correlation and cosine distances, and the step from the
// sums to a, b, s and the nearest other cluster.  Every sum has the order the header states and there is no atomic, so a run has
// one result, bit for bit.  Nothing here may contract into an fma (the pragma below); __builtin_sqrtf and the fp64 divisions are
// hipcc's correctly rounded ones, as in vf_linkage.hip.  The file is built without -fno-honor-nans (csrc/build.py).
#include "vf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int ROWS = VF_SILHOUETTE_ROWS;                   // == VF_WAVE: one query row per lane
constexpr int W = VF_SILHOUETTE_RANGES;                    // one wavefront per range
constexpr int JT = VF_SILHOUETTE_JT;
constexpr int GROUP = W * JT;                              // members (or clusters) per staged tile
constexpr int THREADS = ROWS * W;
static_assert(ROWS == VF_WAVE && THREADS <= 1024 && W >= 1, "the lane mappings below");


// the segment of cluster c, clamped to 0 .. n and never backwards: a malformed CSR reads nothing outside `order`
__device__ __forceinline__ void segment(const int64_t* __restrict__ seg, int c, int n, int& lo, int& nc) {
    int64_t a = seg[c], b = seg[c + 1];
    a = a < 0 ? 0 : (a > n ? n : a);
    b = b < a ? a : (b > n ? n : b);
    lo = (int)a;
    nc = (int)(b - a);
}

// One lane per query row, one wavefront per range of the cluster's members; the tiles of GROUP members x DC columns are gathered
// through `order` into LDS, where a wavefront reads one address.  blockIdx.y strides over the clusters.
template <int DC>
__global__ __launch_bounds__(THREADS) void silhouette_l2_kernel(const float* __restrict__ x, int64_t ldx, int R, int d,
                                                                const int32_t* __restrict__ order, int n, const int64_t* __restrict__ seg,
                                                                int k, int row0, int rows, double* __restrict__ S, int64_t lds) {
    __shared__ __attribute__((aligned(16))) float tile[GROUP * DC];
    __shared__ double part[W][ROWS];
    const int lane = threadIdx.x & (VF_WAVE - 1), w = threadIdx.x >> 6;
    const int q = blockIdx.x * ROWS + lane;
    const bool valid = q < rows;
    const float* xr = x + (int64_t)(row0 + (valid ? q : 0)) * ldx;        // a lane past the end computes the first row and writes nothing
    const bool one = d <= DC;
    float xc[DC];
    if (one) {
#pragma unroll
        for (int i = 0; i < DC; ++i) xc[i] = i < d ? xr[i] : 0.f;
    }
    for (int c = blockIdx.y; c < k; c += gridDim.y) {
        int lo, nc;
        segment(seg, c, n, lo, nc);
        if (nc == 0) {                                                    // uniform: the whole block goes on
            if (w == 0 && valid) S[(int64_t)c * lds + q] = 0.0;
            continue;
        }
        const int L = (nc + W - 1) / W;
        const int mine = min((w + 1) * L, nc) - min(w * L, nc);           // the members of range w
        double sum = 0.0;
        for (int t0 = 0; t0 < L; t0 += JT) {
            float acc[JT];
#pragma unroll
            for (int j = 0; j < JT; ++j) acc[j] = 0.f;
            for (int c0 = 0; c0 < d; c0 += DC) {
                __syncthreads();                                          // the tile before is no longer read
                for (int i = threadIdx.x; i < GROUP * DC; i += THREADS) {
                    const int g = i / DC, col = c0 + i % DC;
                    const int t = t0 + g % JT, m = (g / JT) * L + t;      // position in its range, and in the cluster
                    // a column past d adds t = 0 - 0, p = +0, acc + 0 = acc: nothing; a member past its range is never added
                    float v = 0.f;
                    if (t < L && m < nc && col < d) {
                        const int row = order[lo + m];
                        v = (unsigned)row < (unsigned)R ? x[(int64_t)row * ldx + col] : quiet_nan();
                    }
                    tile[i] = v;
                }
                __syncthreads();
                if (!one) {
#pragma unroll
                    for (int i = 0; i < DC; ++i) xc[i] = c0 + i < d ? xr[c0 + i] : 0.f;
                }
#pragma unroll
                for (int cc = 0; cc < DC; cc += 4) {
#pragma unroll
                    for (int j = 0; j < JT; ++j) {
                        const f32x4_t mv = *reinterpret_cast<const f32x4_t*>(&tile[(w * JT + j) * DC + cc]);   // a broadcast
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float t = xc[cc + i] - mv[i];
                            const float p = t * t;
                            acc[j] = acc[j] + p;
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < JT; ++j)                                  // ascending members; uniform in the wavefront
                if (t0 + j < mine) sum = sum + (double)__builtin_sqrtf(acc[j]);
        }
        part[w][lane] = sum;
        __syncthreads();                                                  // the next write of part lies behind a tile's barriers
        if (w == 0) {
            double s = part[0][lane];
#pragma unroll
            for (int u = 1; u < W; ++u) s = s + part[u][lane];
            if (valid) S[(int64_t)c * lds + q] = s;
        }
    }
}

// One block per (cluster, 64 columns); wavefront v adds the rows of range v in ascending order, lane c the column c0 + c.
__global__ __launch_bounds__(THREADS) void silhouette_colsum_kernel(const float* __restrict__ z, int64_t ldz, int R, int d,
                                                                    const int32_t* __restrict__ order, int n, const int64_t* __restrict__ seg,
                                                                    double* __restrict__ M) {
    __shared__ double part[W][ROWS];
    const int lane = threadIdx.x & (VF_WAVE - 1), w = threadIdx.x >> 6;
    const int c = blockIdx.x, col = blockIdx.y * VF_WAVE + lane;
    int lo, nc;
    segment(seg, c, n, lo, nc);
    const int L = (nc + W - 1) / W;
    const int begin = min(w * L, nc), end = min((w + 1) * L, nc);
    double s = 0.0;
    if (col < d) {
#pragma unroll 4
        for (int m = begin; m < end; ++m) {
            const int row = order[lo + m];
            s = s + (double)((unsigned)row < (unsigned)R ? z[(int64_t)row * ldz + col] : quiet_nan());
        }
    }
    part[w][lane] = s;
    __syncthreads();
    if (w != 0) return;
    double sum = part[0][lane];
#pragma unroll
    for (int u = 1; u < W; ++u) sum = sum + part[u][lane];
    if (col < d) M[(int64_t)c * d + col] = sum;
}

constexpr int DOT_DC = VF_SILHOUETTE_DC;

// One lane per query row, one wavefront per JT clusters of a staged tile of GROUP rows of M x DOT_DC columns.
__global__ __launch_bounds__(THREADS) void silhouette_dot_kernel(const float* __restrict__ z, int64_t ldz, int d, int n,
                                                                 const int64_t* __restrict__ seg, int k, const int32_t* __restrict__ labels,
                                                                 int row0, int rows, const double* __restrict__ M, double* __restrict__ S,
                                                                 int64_t lds) {
    __shared__ __attribute__((aligned(16))) double tile[GROUP * DOT_DC];
    const int lane = threadIdx.x & (VF_WAVE - 1), w = threadIdx.x >> 6;
    const int q = blockIdx.x * ROWS + lane;
    const bool valid = q < rows;
    const int r = row0 + (valid ? q : 0);
    const float* zr = z + (int64_t)r * ldz;
    const int label = labels[r];
    const bool one = d <= DOT_DC;
    float zc[DOT_DC];
    double qq = 0.0;
    for (int c0 = 0; c0 < d; c0 += DOT_DC) {
#pragma unroll
        for (int i = 0; i < DOT_DC; ++i) {
            zc[i] = c0 + i < d ? zr[c0 + i] : 0.f;                        // a column past d adds +0.0 to a sum that is never -0.0
            const double v = (double)zc[i];
            const double p = v * v;
            qq = qq + p;
        }
    }
    for (int g0 = blockIdx.y * GROUP; g0 < k; g0 += gridDim.y * GROUP) {
        double t[JT];
#pragma unroll
        for (int j = 0; j < JT; ++j) t[j] = 0.0;
        for (int c0 = 0; c0 < d; c0 += DOT_DC) {
            __syncthreads();                                              // the tile before is no longer read
            for (int i = threadIdx.x; i < GROUP * DOT_DC; i += THREADS) {
                const int c = g0 + i / DOT_DC, col = c0 + i % DOT_DC;
                tile[i] = c < k && col < d ? M[(int64_t)c * d + col] : 0.0;
            }
            __syncthreads();
            if (!one) {
#pragma unroll
                for (int i = 0; i < DOT_DC; ++i) zc[i] = c0 + i < d ? zr[c0 + i] : 0.f;
            }
#pragma unroll
            for (int cc = 0; cc < DOT_DC; ++cc) {
                const double v = (double)zc[cc];
#pragma unroll
                for (int j = 0; j < JT; ++j) {
                    const double p = v * tile[(w * JT + j) * DOT_DC + cc];   // a broadcast
                    t[j] = t[j] + p;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const int c = g0 + w * JT + j;
            if (c < k && valid) {
                int lo, nc;
                segment(seg, c, n, lo, nc);
                const bool own = label == c;
                const double u = own ? t[j] - qq : t[j];
                S[(int64_t)c * lds + q] = (double)(nc - (own ? 1 : 0)) - u;
            }
        }
    }
}

// One thread per query row; the clusters ascending, S read along the rows.
__global__ __launch_bounds__(256) void silhouette_finish_kernel(const double* __restrict__ S, int64_t lds, const int32_t* __restrict__ labels,
                                                                const int64_t* __restrict__ seg, int k, int row0, int rows,
                                                                double* __restrict__ a, double* __restrict__ b, double* __restrict__ s,
                                                                int32_t* __restrict__ nearest) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= rows) return;
    const int i = row0 + q;
    const int l = labels[i];
    const bool labelled = l >= 0 && l < k;
    double best = quiet_nan64(), own = 0.0;
    int bestc = -1, nl = 0;
    for (int c = 0; c < k; ++c) {
        const int64_t n64 = seg[c + 1] - seg[c];
        const int nc = n64 < 0 ? 0 : (int)n64;
        if (c == l) {
            own = S[(int64_t)c * lds + q];
            nl = nc;
            continue;
        }
        if (nc == 0) continue;
        const double mean = S[(int64_t)c * lds + q] / (double)nc;
        if (mean == mean && (bestc < 0 || mean < best)) {                 // strict <: ties to the lower c
            best = mean;
            bestc = c;
        }
    }
    double av, sv;
    if (!labelled) av = quiet_nan64();
    else if (nl <= 1) av = 0.0;
    else av = own / (double)(nl - 1);
    if (av != av) av = quiet_nan64();
    if (av != av || bestc < 0) sv = quiet_nan64();
    else if (nl <= 1) sv = 0.0;
    else {
        const double m = av < best ? best : av;
        sv = m == 0.0 ? 0.0 : (best - av) / m;
        if (sv != sv) sv = quiet_nan64();
    }
    a[i] = av;
    b[i] = best;
    s[i] = sv;
    nearest[i] = bestc;
}

// the second grid dimension: enough blocks to fill the device where the query rows alone do not
int spread(int row_blocks, int units) {
    const int want = (2048 + row_blocks - 1) / row_blocks;
    return want < 1 ? 1 : (want > units ? units : want);
}

// the row range every entry shares
#define VF_SILHOUETTE_RANGE(NAME)                                                                                                          \
    VF_REQUIRE(k >= 1 && k <= VF_SILHOUETTE_MAX_K, NAME ": k=%d outside 1 .. %d", k, VF_SILHOUETTE_MAX_K);                                  \
    VF_REQUIRE(R >= 0, NAME ": R=%ld must not be negative", (long)R);                                                                      \
    VF_REQUIRE(R <= VF_SILHOUETTE_MAX_R, NAME ": R=%ld is above 2^24", (long)R);                                                           \
    VF_REQUIRE(row0 >= 0, NAME ": row0=%ld must not be negative", (long)row0);                                                             \
    VF_REQUIRE(rows >= 0, NAME ": rows=%ld must not be negative", (long)rows);                                                             \
    VF_REQUIRE(row0 <= R && rows <= R - row0, NAME ": rows=%ld from row0=%ld end above R=%ld", (long)rows, (long)row0, (long)R);           \
    VF_REQUIRE(lds >= rows, NAME ": lds=%ld is below rows=%ld", (long)lds, (long)rows)
// the rows and the CSR of the two sums
#define VF_SILHOUETTE_SUMS(NAME, X, LDX)                                                                                                   \
    VF_REQUIRE(X, NAME ": null pointer " #X);                                                                                              \
    VF_REQUIRE(order, NAME ": null pointer order");                                                                                        \
    VF_REQUIRE(seg, NAME ": null pointer seg");                                                                                            \
    VF_REQUIRE(S, NAME ": null pointer S");                                                                                                \
    VF_REQUIRE(VF_ALIGNED4(X), NAME ": " #X " must be 4-byte aligned");                                                                    \
    VF_REQUIRE(VF_ALIGNED4(order), NAME ": order must be 4-byte aligned");                                                                 \
    VF_REQUIRE(VF_ALIGNED8(seg), NAME ": seg must be 8-byte aligned");                                                                     \
    VF_REQUIRE(VF_ALIGNED8(S), NAME ": S must be 8-byte aligned");                                                                         \
    VF_REQUIRE(d >= 1 && d <= VF_SILHOUETTE_MAX_D, NAME ": d=%d outside 1 .. %d", d, VF_SILHOUETTE_MAX_D);                                  \
    VF_REQUIRE(LDX >= d, NAME ": " #LDX "=%ld is below d=%d", (long)LDX, d);                                                               \
    VF_SILHOUETTE_RANGE(NAME);                                                                                                             \
    VF_REQUIRE(n >= 0 && n <= R, NAME ": n=%ld outside 0 .. R=%ld", (long)n, (long)R)

}  // namespace

extern "C" int vf_silhouette_sums_l2(const float* x, int64_t ldx, int64_t R, int d, const int32_t* order, int64_t n, const int64_t* seg, int k,
                                     int64_t row0, int64_t rows, double* S, int64_t lds, void* stream) {
    VF_SILHOUETTE_SUMS("vf_silhouette_sums_l2", x, ldx);
    if (rows == 0) return VF_OK;
    const int row_blocks = (int)((rows + ROWS - 1) / ROWS);
    const dim3 grid((unsigned)row_blocks, (unsigned)spread(row_blocks, k)), block(THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (d <= VF_SILHOUETTE_DC_SMALL)
        hipLaunchKernelGGL(silhouette_l2_kernel<VF_SILHOUETTE_DC_SMALL>, grid, block, 0, st, x, ldx, (int)R, d, order, (int)n, seg, k, (int)row0,
                           (int)rows, S, lds);
    else if (d <= VF_SILHOUETTE_DC)
        hipLaunchKernelGGL(silhouette_l2_kernel<VF_SILHOUETTE_DC>, grid, block, 0, st, x, ldx, (int)R, d, order, (int)n, seg, k, (int)row0,
                           (int)rows, S, lds);
    else
        hipLaunchKernelGGL(silhouette_l2_kernel<VF_SILHOUETTE_DC_WIDE>, grid, block, 0, st, x, ldx, (int)R, d, order, (int)n, seg, k, (int)row0,
                           (int)rows, S, lds);
    VF_CHECK_LAUNCH("vf_silhouette_sums_l2");
    return VF_OK;
}

extern "C" int vf_silhouette_sums_dot(const float* z, int64_t ldz, int64_t R, int d, const int32_t* order, int64_t n, const int64_t* seg, int k,
                                      const int32_t* labels, int64_t row0, int64_t rows, double* S, int64_t lds, void* work, int64_t work_bytes,
                                      void* stream) {
    VF_SILHOUETTE_SUMS("vf_silhouette_sums_dot", z, ldz);
    VF_REQUIRE(labels, "vf_silhouette_sums_dot: null pointer labels");
    VF_REQUIRE(work, "vf_silhouette_sums_dot: null pointer work");
    VF_REQUIRE(VF_ALIGNED4(labels), "vf_silhouette_sums_dot: labels must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(work), "vf_silhouette_sums_dot: work must be 8-byte aligned");
    VF_REQUIRE(work_bytes >= VF_SILHOUETTE_DOT_WORK_BYTES(d, k), "vf_silhouette_sums_dot: work_bytes=%ld is below the %ld this call needs",
               (long)work_bytes, (long)VF_SILHOUETTE_DOT_WORK_BYTES(d, k));
    if (rows == 0) return VF_OK;
    hipStream_t st = (hipStream_t)stream;
    double* M = (double*)work;
    hipLaunchKernelGGL(silhouette_colsum_kernel, dim3((unsigned)k, (unsigned)((d + VF_WAVE - 1) / VF_WAVE)), dim3(THREADS), 0, st, z, ldz, (int)R, d,
                       order, (int)n, seg, M);
    const int row_blocks = (int)((rows + ROWS - 1) / ROWS);
    hipLaunchKernelGGL(silhouette_dot_kernel, dim3((unsigned)row_blocks, (unsigned)spread(row_blocks, (k + GROUP - 1) / GROUP)), dim3(THREADS), 0, st,
                       z, ldz, d, (int)n, seg, k, labels, (int)row0, (int)rows, (const double*)M, S, lds);
    VF_CHECK_LAUNCH("vf_silhouette_sums_dot");
    return VF_OK;
}

extern "C" int vf_silhouette_finish(const double* S, int64_t lds, const int32_t* labels, int64_t R, const int64_t* seg, int k, int64_t row0,
                                    int64_t rows, double* a, double* b, double* s, int32_t* nearest, void* stream) {
    VF_REQUIRE(S, "vf_silhouette_finish: null pointer S");
    VF_REQUIRE(labels, "vf_silhouette_finish: null pointer labels");
    VF_REQUIRE(seg, "vf_silhouette_finish: null pointer seg");
    VF_REQUIRE(a, "vf_silhouette_finish: null pointer a");
    VF_REQUIRE(b, "vf_silhouette_finish: null pointer b");
    VF_REQUIRE(s, "vf_silhouette_finish: null pointer s");
    VF_REQUIRE(nearest, "vf_silhouette_finish: null pointer nearest");
    VF_REQUIRE(VF_ALIGNED8(S), "vf_silhouette_finish: S must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(labels), "vf_silhouette_finish: labels must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(seg), "vf_silhouette_finish: seg must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(a), "vf_silhouette_finish: a must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(b), "vf_silhouette_finish: b must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(s), "vf_silhouette_finish: s must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(nearest), "vf_silhouette_finish: nearest must be 4-byte aligned");
    VF_SILHOUETTE_RANGE("vf_silhouette_finish");
    if (rows == 0) return VF_OK;
    hipLaunchKernelGGL(silhouette_finish_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, S, lds, labels, seg, k,
                       (int)row0, (int)rows, a, b, s, nearest);
    VF_CHECK_LAUNCH("vf_silhouette_finish");
    return VF_OK;
}

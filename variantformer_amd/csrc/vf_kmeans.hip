// k-means clustering (include/vf_hip_kmeans.h): the assignment to the nearest centre, the fp64 means, Lloyd's loop with its stop
// decided on the device, and D^2 seeding with integer sampling.  Every sum has the order the header states and there is no
// atomic, so a run has one result, bit for bit.  Nothing here may contract into an fma (the pragma below); the fp64 divisions
// are the correctly rounded ones.  The file is built without -fno-honor-nans (csrc/build.py: that flag is vf_attn.hip's): a NaN
// distance is recognised as such.
#include "vf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int ROWS = VF_KMEANS_ROWS;                       // == VF_WAVE: one row per lane
constexpr int SPLITS = VF_KMEANS_SPLITS;
constexpr int JT = VF_KMEANS_JT;
constexpr int GROUP = SPLITS * JT;                         // centres per staged tile
constexpr int ASSIGN_THREADS = ROWS * SPLITS;
constexpr int UW = VF_KMEANS_UPDATE_WAVES;
constexpr int UCOLS = VF_KMEANS_UPDATE_COLS;               // == VF_WAVE: one column per lane
constexpr int RED = VF_KMEANS_RED_THREADS;
static_assert(ROWS == VF_WAVE && UCOLS == VF_WAVE && ASSIGN_THREADS == 256 && UW * VF_WAVE <= 1024, "the lane mappings below");

// One lane per row, one wavefront per split of the centres; the tiles of GROUP centres x DC columns come through LDS, where a
// wavefront reads one address.  `labels` may be `prev` (Lloyd's loop): a row's old label is read by the lane that replaces it.
template <int DC>
__global__ __launch_bounds__(ASSIGN_THREADS) void kmeans_assign_kernel(const float* __restrict__ x, int64_t ldx, int R, int d,
                                                                       const float* __restrict__ cen, int64_t ldc, int k, int32_t* labels,
                                                                       float* __restrict__ dist, const int32_t* prev, int first,
                                                                       int32_t* __restrict__ block_changed, const int32_t* __restrict__ stop) {
    if (stop && *stop) return;                                            // uniform: the whole grid leaves
    __shared__ __attribute__((aligned(16))) float tile[GROUP * DC];
    __shared__ float wd[SPLITS][ROWS];
    __shared__ int wj[SPLITS][ROWS];
    const int lane = threadIdx.x & (VF_WAVE - 1), w = threadIdx.x >> 6;
    const int r = blockIdx.x * ROWS + lane;
    const bool valid = r < R;
    const float* xr = x + (int64_t)(valid ? r : 0) * ldx;                 // a lane past the end computes row 0 and writes nothing
    const bool one = d <= DC;
    float xc[DC];
    if (one) {
#pragma unroll
        for (int i = 0; i < DC; ++i) xc[i] = i < d ? xr[i] : 0.f;
    }
    float bestd = quiet_nan();
    int bestj = -1;
    for (int g0 = 0; g0 < k; g0 += GROUP) {
        float acc[JT];
#pragma unroll
        for (int j = 0; j < JT; ++j) acc[j] = 0.f;
        for (int c0 = 0; c0 < d; c0 += DC) {
            __syncthreads();                                              // the tile before is no longer read
            for (int i = threadIdx.x; i < GROUP * DC; i += ASSIGN_THREADS) {
                const int j = g0 + i / DC, c = c0 + i % DC;
                // a column past d adds t = 0 - 0, p = +0, acc + 0 = acc: nothing; a centre past k is NaN and never wins
                tile[i] = j < k ? (c < d ? cen[(int64_t)j * ldc + c] : 0.f) : quiet_nan();
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
                    const f32x4_t cv = *reinterpret_cast<const f32x4_t*>(&tile[(w * JT + j) * DC + cc]);   // a broadcast
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float t = xc[cc + i] - cv[i];
                        const float p = t * t;
                        acc[j] = acc[j] + p;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < JT; ++j) {                                    // ascending j: a strict < keeps the lower one
            const float dj = acc[j];
            if (dj == dj && (bestj < 0 || dj < bestd)) {
                bestd = dj;
                bestj = g0 + w * JT + j;
            }
        }
    }
    wd[w][lane] = bestd;
    wj[w][lane] = bestj;
    __syncthreads();
    if (w != 0) return;
#pragma unroll
    for (int s = 1; s < SPLITS; ++s) {
        const float od = wd[s][lane];
        const int oj = wj[s][lane];
        if (oj >= 0 && (bestj < 0 || od < bestd || (od == bestd && oj < bestj))) {
            bestd = od;
            bestj = oj;
        }
    }
    bool differs = false;
    if (valid) {
        differs = first || !prev || prev[r] != bestj;
        labels[r] = bestj;
        if (dist) dist[r] = bestj < 0 ? quiet_nan() : bestd;
    }
    if (block_changed) {
        const unsigned long long b = __ballot(differs);
        if (lane == 0) block_changed[blockIdx.x] = __popcll(b);
    }
}

// One block per (centre, 64 columns); wavefront v scans the labels of row range v, 64 at a time, and walks the ballot's set
// bits in ascending order, lane c adding column c0 + c.  cen_new may be cen_old: a thread reads its own element before writing it.
__global__ __launch_bounds__(UW * VF_WAVE) void kmeans_update_kernel(const float* __restrict__ x, int64_t ldx, int R, int d,
                                                                     const int32_t* __restrict__ labels, const float* cen_old, int64_t ldc,
                                                                     float* cen_new, int64_t ldn, int32_t* __restrict__ counts,
                                                                     double* __restrict__ shift_part, const int32_t* __restrict__ stop) {
    if (stop && *stop) return;
    __shared__ double part[UW][UCOLS];
    __shared__ int members[UW];
    const int lane = threadIdx.x & (VF_WAVE - 1), v = threadIdx.x >> 6;
    const int j = blockIdx.x, c = blockIdx.y * UCOLS + lane;
    const int L = (R + UW - 1) / UW;
    const int64_t lo64 = (int64_t)v * L, hi64 = lo64 + L;
    const int begin = (int)(lo64 < R ? lo64 : R), end = (int)(hi64 < R ? hi64 : R);
    double s = 0.0;
    int n = 0;
    for (int r0 = begin; r0 < end; r0 += VF_WAVE) {
        const int r = r0 + lane;
        unsigned long long bits = __ballot(r < end && labels[r] == j);
        n += __popcll(bits);
        while (bits) {                                                    // uniform: every lane holds the same bits
            const int rr = r0 + __builtin_ctzll(bits);
            bits &= bits - 1;
            if (c < d) s = s + (double)x[(int64_t)rr * ldx + c];
        }
    }
    part[v][lane] = s;
    if (lane == 0) members[v] = n;
    __syncthreads();
    if (v != 0) return;
    double S = part[0][lane];
    int total = members[0];
#pragma unroll
    for (int u = 1; u < UW; ++u) {
        S = S + part[u][lane];
        total += members[u];
    }
    double e2 = 0.0;
    if (c < d) {
        const float old = cen_old[(int64_t)j * ldc + c];
        const float now = total > 0 ? (float)(S / (double)total) : old;
        cen_new[(int64_t)j * ldn + c] = now;
        const double e = (double)now - (double)old;
        e2 = e * e;
    }
    if (blockIdx.y == 0 && lane == 0) counts[j] = total;
    if (shift_part) {                                                     // wavefront 0 alone is left: no barrier from here on
        double q = 0.0;
        for (int i = 0; i < UCOLS; ++i) q = q + __shfl(e2, i);            // columns ascending; those past d hold +0
        if (lane == 0) shift_part[(int64_t)j * gridDim.y + blockIdx.y] = q;
    }
}

__global__ void kmeans_begin_kernel(int32_t* __restrict__ stop, int32_t* __restrict__ n_iter) {
    stop[0] = 0;
    stop[1] = 0;
    n_iter[0] = 0;
}

// One block: the changed count, the shift in its stated order, n_iter and the stop word of iteration n.
__global__ __launch_bounds__(RED) void kmeans_finish_kernel(int32_t* __restrict__ stop, const int32_t* __restrict__ block_changed, int nblocks,
                                                            const double* __restrict__ shift_part, int nparts, int n, int first,
                                                            double tol_abs, int64_t* __restrict__ changed, double* __restrict__ shift,
                                                            int32_t* __restrict__ n_iter) {
    if (*stop) return;
    __shared__ double sd[RED];
    __shared__ long long sc[RED];
    const int u = threadIdx.x;
    double s = 0.0;
    for (int i = u; i < nparts; i += RED) s = s + shift_part[i];
    long long cnt = 0;
    for (int i = u; i < nblocks; i += RED) cnt += block_changed[i];
    sd[u] = s;
    sc[u] = cnt;
    __syncthreads();
    for (int stride = RED / 2; stride > 0; stride >>= 1) {
        if (u < stride) {
            sd[u] = sd[u] + sd[u + stride];
            sc[u] += sc[u + stride];
        }
        __syncthreads();
    }
    if (u == 0) {
        changed[n] = sc[0];
        shift[n] = sd[0];
        n_iter[0] = n + 1;
        if ((sc[0] == 0 && !first) || sd[0] <= tol_abs) stop[0] = 1;
    }
}

// ---- seeding -----------------------------------------------------------------------------------------------------------------------
struct SeedWork {                                                         // the workspace of vf_kmeans_seed
    unsigned long long* blocksum;                                         // [nb]
    float* m;                                                             // [1] (8 bytes kept)
    float* blockmax;                                                      // [nb]
};

__device__ __forceinline__ unsigned long long quantum(float mind, float m) {
    if (!finite_bits(mind) || !(m > 0.f)) return 0ull;
    return (unsigned long long)((double)mind / (double)m * 4294967296.0);
}

// rows[t] = row and cen[t] = x[row]
__global__ __launch_bounds__(RED) void kmeans_take_kernel(const float* __restrict__ x, int64_t ldx, int d, int row, int t, int32_t* __restrict__ rows,
                                                          float* __restrict__ cen, int64_t ldc) {
    for (int c = threadIdx.x; c < d; c += RED) cen[(int64_t)t * ldc + c] = x[(int64_t)row * ldx + c];
    if (threadIdx.x == 0) rows[t] = row;
}

// One thread per row: mind against centre `t - 1`, and the block's largest finite mind.
__global__ __launch_bounds__(RED) void kmeans_mind_kernel(const float* __restrict__ x, int64_t ldx, int R, int d, const float* __restrict__ centre,
                                                          int first, float* __restrict__ mind, float* __restrict__ blockmax) {
    __shared__ float sm[RED];
    const int r = blockIdx.x * RED + threadIdx.x;
    float big = 0.f;
    if (r < R) {
        const float* xr = x + (int64_t)r * ldx;
        float acc = 0.f;
        for (int c = 0; c < d; ++c) {
            const float t = xr[c] - centre[c];
            const float p = t * t;
            acc = acc + p;
        }
        float now = acc;
        if (!first) {
            const float old = mind[r];
            now = acc < old ? acc : old;
        }
        mind[r] = now;
        if (finite_bits(now)) big = now;
    }
    sm[threadIdx.x] = big;
    __syncthreads();
    for (int stride = RED / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) sm[threadIdx.x] = fmaxf(sm[threadIdx.x], sm[threadIdx.x + stride]);
        __syncthreads();
    }
    if (threadIdx.x == 0) blockmax[blockIdx.x] = sm[0];
}

__global__ __launch_bounds__(RED) void kmeans_max_kernel(const float* __restrict__ blockmax, int nb, float* __restrict__ m) {
    __shared__ float sm[RED];
    float big = 0.f;
    for (int i = threadIdx.x; i < nb; i += RED) big = fmaxf(big, blockmax[i]);
    sm[threadIdx.x] = big;
    __syncthreads();
    for (int stride = RED / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) sm[threadIdx.x] = fmaxf(sm[threadIdx.x], sm[threadIdx.x + stride]);
        __syncthreads();
    }
    if (threadIdx.x == 0) m[0] = sm[0];
}

__global__ __launch_bounds__(RED) void kmeans_qsum_kernel(const float* __restrict__ mind, int R, const float* __restrict__ m,
                                                          unsigned long long* __restrict__ blocksum) {
    __shared__ unsigned long long sq[RED];
    const int r = blockIdx.x * RED + threadIdx.x;
    sq[threadIdx.x] = r < R ? quantum(mind[r], m[0]) : 0ull;
    __syncthreads();
    for (int stride = RED / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) sq[threadIdx.x] += sq[threadIdx.x + stride];
        __syncthreads();
    }
    if (threadIdx.x == 0) blocksum[blockIdx.x] = sq[0];
}

// One block: the total, the target, the block of rows and the row whose inclusive prefix first exceeds it; then the copy.
__global__ __launch_bounds__(RED) void kmeans_select_kernel(const float* __restrict__ x, int64_t ldx, int R, int d, const float* __restrict__ mind,
                                                            const float* __restrict__ m, const unsigned long long* __restrict__ blocksum, int nb,
                                                            unsigned long long hash, int t, int32_t* __restrict__ rows, float* __restrict__ cen,
                                                            int64_t ldc) {
    __shared__ unsigned long long sq[RED];
    __shared__ int chosen;
    const int u = threadIdx.x;
    const int per = (nb + RED - 1) / RED;                                 // thread u owns the blocks [u * per, (u + 1) * per)
    unsigned long long mine = 0ull;
    for (int i = u * per; i < nb && i < (u + 1) * per; ++i) mine += blocksum[i];
    sq[u] = mine;
    __syncthreads();
    if (u == 0) {
        unsigned long long total = 0ull;
        for (int i = 0; i < RED; ++i) total += sq[i];
        int row = -1;
        if (total > 0ull) {
            const unsigned long long target = __umul64hi(hash, total);    // below total
            unsigned long long before = 0ull;
            int owner = 0;
            while (owner < RED - 1 && before + sq[owner] <= target) before += sq[owner++];   // target < total: ends inside
            int b = owner * per;
            while (b < nb - 1 && before + blocksum[b] <= target) before += blocksum[b++];
            const float mm = m[0];
            int r = b * RED;
            for (; r < R - 1; ++r) {
                before += quantum(mind[r], mm);
                if (before > target) break;
            }
            row = r;
        }
        chosen = row;
    }
    __syncthreads();
    if (chosen < 0) {                                                     // the lowest row not yet chosen: it is at most t
        __shared__ int lowest[RED];
        int best = R;
        for (int cand = u; cand <= t && cand < R; cand += RED) {
            bool taken = false;
            for (int i = 0; i < t; ++i) taken |= rows[i] == cand;
            if (!taken && cand < best) best = cand;
        }
        lowest[u] = best;
        __syncthreads();
        for (int stride = RED / 2; stride > 0; stride >>= 1) {
            if (u < stride) lowest[u] = lowest[u + stride] < lowest[u] ? lowest[u + stride] : lowest[u];
            __syncthreads();
        }
        if (u == 0) chosen = lowest[0];
        __syncthreads();
    }
    const int row = chosen;
    __syncthreads();                                                      // rows[t] is written after every read of rows
    for (int c = u; c < d; c += RED) cen[(int64_t)t * ldc + c] = x[(int64_t)row * ldx + c];
    if (u == 0) rows[t] = row;
}

uint64_t host_hash(int64_t seed, uint32_t t) {
    const uint32_t a = mix32((uint32_t)(uint64_t)seed + 0x9E3779B9u);
    return ((uint64_t)mix32(a ^ (2u * t)) << 32) | (uint64_t)mix32(a ^ (2u * t + 1u));
}

void launch_assign(const float* x, int64_t ldx, int R, int d, const float* cen, int64_t ldc, int k, int32_t* labels, float* dist,
                   const int32_t* prev, int first, int32_t* block_changed, const int32_t* stop, hipStream_t st) {
    const dim3 grid((unsigned)((R + ROWS - 1) / ROWS)), block(ASSIGN_THREADS);
    if (d <= VF_KMEANS_DC_SMALL)
        hipLaunchKernelGGL(kmeans_assign_kernel<VF_KMEANS_DC_SMALL>, grid, block, 0, st, x, ldx, R, d, cen, ldc, k, labels, dist, prev, first,
                           block_changed, stop);
    else
        hipLaunchKernelGGL(kmeans_assign_kernel<VF_KMEANS_DC>, grid, block, 0, st, x, ldx, R, d, cen, ldc, k, labels, dist, prev, first,
                           block_changed, stop);
}

void launch_update(const float* x, int64_t ldx, int R, int d, const int32_t* labels, const float* cen_old, int64_t ldc, int k, float* cen_new,
                   int64_t ldn, int32_t* counts, double* shift_part, const int32_t* stop, hipStream_t st) {
    hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)k, (unsigned)((d + UCOLS - 1) / UCOLS)), dim3(UW * VF_WAVE), 0, st, x, ldx, R, d,
                       labels, cen_old, ldc, cen_new, ldn, counts, shift_part, stop);
}

// the operands every entry shares
#define VF_KMEANS_COMMON(NAME, CEN)                                                                                       \
    VF_REQUIRE(x, NAME ": null pointer x");                                                                               \
    VF_REQUIRE(CEN, NAME ": null pointer " #CEN);                                                                         \
    VF_REQUIRE(VF_ALIGNED4(x), NAME ": x must be 4-byte aligned");                                                        \
    VF_REQUIRE(VF_ALIGNED4(CEN), NAME ": " #CEN " must be 4-byte aligned");                                               \
    VF_REQUIRE(d >= 1 && d <= VF_KMEANS_MAX_D, NAME ": d=%d outside 1 .. %d", d, VF_KMEANS_MAX_D);                                                            \
    VF_REQUIRE(ldx >= d, NAME ": ldx=%ld is below d=%d", (long)ldx, d);                                                   \
    VF_REQUIRE(ldc >= d, NAME ": ldc=%ld is below d=%d", (long)ldc, d);                                                   \
    VF_REQUIRE(R >= 0, NAME ": R=%ld must not be negative", (long)R);                                                     \
    VF_REQUIRE(R <= VF_KMEANS_MAX_R, NAME ": R=%ld is above 2^24", (long)R)

}  // namespace

extern "C" int vf_kmeans_assign(const float* x, int64_t ldx, int64_t R, int d, const float* cen, int64_t ldc, int k, int32_t* labels,
                                float* dist, void* stream) {
    VF_KMEANS_COMMON("vf_kmeans_assign", cen);
    VF_REQUIRE(labels, "vf_kmeans_assign: null pointer labels");
    VF_REQUIRE(dist, "vf_kmeans_assign: null pointer dist");
    VF_REQUIRE(VF_ALIGNED4(labels), "vf_kmeans_assign: labels must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(dist), "vf_kmeans_assign: dist must be 4-byte aligned");
    VF_REQUIRE(k >= 1 && k <= VF_KMEANS_MAX_K, "vf_kmeans_assign: k=%d outside 1 .. %d", k, VF_KMEANS_MAX_K);
    if (R == 0) return VF_OK;
    launch_assign(x, ldx, (int)R, d, cen, ldc, k, labels, dist, nullptr, 1, nullptr, nullptr, (hipStream_t)stream);
    VF_CHECK_LAUNCH("vf_kmeans_assign");
    return VF_OK;
}

extern "C" int vf_kmeans_update(const float* x, int64_t ldx, int64_t R, int d, const int32_t* labels, const float* cen_old, int64_t ldc, int k,
                                float* cen_new, int64_t ldn, int32_t* counts, void* stream) {
    VF_KMEANS_COMMON("vf_kmeans_update", cen_old);
    VF_REQUIRE(labels, "vf_kmeans_update: null pointer labels");
    VF_REQUIRE(cen_new, "vf_kmeans_update: null pointer cen_new");
    VF_REQUIRE(counts, "vf_kmeans_update: null pointer counts");
    VF_REQUIRE(VF_ALIGNED4(labels), "vf_kmeans_update: labels must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(cen_new), "vf_kmeans_update: cen_new must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(counts), "vf_kmeans_update: counts must be 4-byte aligned");
    VF_REQUIRE(ldn >= d, "vf_kmeans_update: ldn=%ld is below d=%d", (long)ldn, d);
    VF_REQUIRE(k >= 1 && k <= VF_KMEANS_MAX_K, "vf_kmeans_update: k=%d outside 1 .. %d", k, VF_KMEANS_MAX_K);
    launch_update(x, ldx, (int)R, d, labels, cen_old, ldc, k, cen_new, ldn, counts, nullptr, nullptr, (hipStream_t)stream);
    VF_CHECK_LAUNCH("vf_kmeans_update");
    return VF_OK;
}

extern "C" int vf_kmeans_lloyd(const float* x, int64_t ldx, int64_t R, int d, float* cen, int64_t ldc, int k, int max_iter, double tol_abs,
                               int resume, int32_t* labels, float* dist, int32_t* prev_labels, int32_t* counts, int32_t* n_iter, double* shift,
                               int64_t* changed, void* work, int64_t work_bytes, void* stream) {
    VF_KMEANS_COMMON("vf_kmeans_lloyd", cen);
    VF_REQUIRE(labels, "vf_kmeans_lloyd: null pointer labels");
    VF_REQUIRE(dist, "vf_kmeans_lloyd: null pointer dist");
    VF_REQUIRE(prev_labels, "vf_kmeans_lloyd: null pointer prev_labels");
    VF_REQUIRE(counts, "vf_kmeans_lloyd: null pointer counts");
    VF_REQUIRE(n_iter, "vf_kmeans_lloyd: null pointer n_iter");
    VF_REQUIRE(work, "vf_kmeans_lloyd: null pointer work");
    VF_REQUIRE(shift || max_iter == 0, "vf_kmeans_lloyd: null pointer shift");
    VF_REQUIRE(changed || max_iter == 0, "vf_kmeans_lloyd: null pointer changed");
    VF_REQUIRE(VF_ALIGNED4(labels), "vf_kmeans_lloyd: labels must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(dist), "vf_kmeans_lloyd: dist must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(prev_labels), "vf_kmeans_lloyd: prev_labels must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(counts), "vf_kmeans_lloyd: counts must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(n_iter), "vf_kmeans_lloyd: n_iter must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(shift), "vf_kmeans_lloyd: shift must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(changed), "vf_kmeans_lloyd: changed must be 8-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(work), "vf_kmeans_lloyd: work must be 8-byte aligned");
    VF_REQUIRE(k >= 1 && k <= VF_KMEANS_MAX_K, "vf_kmeans_lloyd: k=%d outside 1 .. %d", k, VF_KMEANS_MAX_K);
    VF_REQUIRE(max_iter >= 0, "vf_kmeans_lloyd: max_iter=%d must not be negative", max_iter);
    VF_REQUIRE(tol_abs >= 0.0, "vf_kmeans_lloyd: tol_abs=%g must be a number >= 0", tol_abs);
    VF_REQUIRE(resume == 0 || resume == 1, "vf_kmeans_lloyd: resume=%d outside 0 .. 1", resume);
    VF_REQUIRE(work_bytes >= VF_KMEANS_LLOYD_WORK_BYTES(R, d, k), "vf_kmeans_lloyd: work_bytes=%ld is below the %ld this call needs",
               (long)work_bytes, (long)VF_KMEANS_LLOYD_WORK_BYTES(R, d, k));
    if (R == 0) return VF_OK;
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (d + UCOLS - 1) / UCOLS, nblocks = (int)((R + ROWS - 1) / ROWS);
    int32_t* stop = (int32_t*)work;
    double* shift_part = (double*)((char*)work + 8);
    int32_t* block_changed = (int32_t*)(shift_part + (int64_t)k * tiles);
    hipLaunchKernelGGL(kmeans_begin_kernel, dim3(1), dim3(1), 0, st, stop, n_iter);
    for (int n = 0; n < max_iter; ++n) {
        const int first = n == 0 && !resume;
        launch_assign(x, ldx, (int)R, d, cen, ldc, k, prev_labels, nullptr, prev_labels, first, block_changed, stop, st);
        launch_update(x, ldx, (int)R, d, prev_labels, cen, ldc, k, cen, ldc, counts, shift_part, stop, st);
        hipLaunchKernelGGL(kmeans_finish_kernel, dim3(1), dim3(RED), 0, st, stop, block_changed, nblocks, shift_part, k * tiles, n, first,
                           tol_abs, changed, shift, n_iter);
        VF_CHECK_LAUNCH("vf_kmeans_lloyd");
    }
    launch_assign(x, ldx, (int)R, d, cen, ldc, k, labels, dist, nullptr, 1, nullptr, nullptr, st);
    VF_CHECK_LAUNCH("vf_kmeans_lloyd");
    return VF_OK;
}

extern "C" int vf_kmeans_seed(const float* x, int64_t ldx, int64_t R, int d, int k, int64_t seed, int32_t* rows, float* cen, int64_t ldc,
                              float* mind, void* work, int64_t work_bytes, void* stream) {
    VF_KMEANS_COMMON("vf_kmeans_seed", cen);
    VF_REQUIRE(rows, "vf_kmeans_seed: null pointer rows");
    VF_REQUIRE(mind, "vf_kmeans_seed: null pointer mind");
    VF_REQUIRE(work, "vf_kmeans_seed: null pointer work");
    VF_REQUIRE(VF_ALIGNED4(rows), "vf_kmeans_seed: rows must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(mind), "vf_kmeans_seed: mind must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED8(work), "vf_kmeans_seed: work must be 8-byte aligned");
    VF_REQUIRE(R >= 1, "vf_kmeans_seed: R=%ld must be at least 1", (long)R);
    VF_REQUIRE(k >= 1 && k <= VF_KMEANS_MAX_K && k <= R, "vf_kmeans_seed: k=%d outside 1 .. min(R=%ld, %d)", k, (long)R, VF_KMEANS_MAX_K);
    VF_REQUIRE(work_bytes >= VF_KMEANS_SEED_WORK_BYTES(R), "vf_kmeans_seed: work_bytes=%ld is below the %ld this call needs", (long)work_bytes,
               (long)VF_KMEANS_SEED_WORK_BYTES(R));
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)((R + RED - 1) / RED);
    SeedWork w;
    w.blocksum = (unsigned long long*)work;
    w.m = (float*)(w.blocksum + nb);
    w.blockmax = w.m + 4;
    const uint64_t h0 = host_hash(seed, 0);                               // mulhi64(h0, R) with R <= 2^24: two 32-bit halves
    const uint64_t first_row = ((h0 >> 32) * (uint64_t)R + (((h0 & 0xFFFFFFFFull) * (uint64_t)R) >> 32)) >> 32;
    hipLaunchKernelGGL(kmeans_take_kernel, dim3(1), dim3(RED), 0, st, x, ldx, d, (int)first_row, 0, rows, cen, ldc);
    for (int t = 1; t < k; ++t) {
        hipLaunchKernelGGL(kmeans_mind_kernel, dim3((unsigned)nb), dim3(RED), 0, st, x, ldx, (int)R, d, cen + (int64_t)(t - 1) * ldc, t == 1 ? 1 : 0,
                           mind, w.blockmax);
        hipLaunchKernelGGL(kmeans_max_kernel, dim3(1), dim3(RED), 0, st, w.blockmax, nb, w.m);
        hipLaunchKernelGGL(kmeans_qsum_kernel, dim3((unsigned)nb), dim3(RED), 0, st, mind, (int)R, w.m, w.blocksum);
        hipLaunchKernelGGL(kmeans_select_kernel, dim3(1), dim3(RED), 0, st, x, ldx, (int)R, d, mind, w.m, w.blocksum, nb,
                           (unsigned long long)host_hash(seed, (uint32_t)t), t, rows, cen, ldc);
        VF_CHECK_LAUNCH("vf_kmeans_seed");
    }
    VF_CHECK_LAUNCH("vf_kmeans_seed");
    return VF_OK;
}

// Expression and embedding neighbours (include/vf_hip_neighbors.h): rows standardised so that a dot product is a correlation or
// a cosine, the k most similar rows by that dot product without a rows x rows buffer, and the dense similarity / distance
// matrix.  fp32 end to end: the similarity is the f32-input MFMA's k-ordered fmaf chain, one accumulator per element, so its
// bits depend on the two rows alone.  The order is vf_topk_rows's and is defined for NaN, which is why this file is built
// without -fno-honor-nans (csrc/build.py: that flag is vf_attn.hip's).
#include "vf_common.h"

namespace {

constexpr int BM = VF_KNN_BM, BN = VF_KNN_BN, BK = VF_KNN_BK;
constexpr int LDT = BK + 1;                    // LDS row stride of an operand tile, in words: odd, so a column of rows spreads over the banks
constexpr int THREADS = 256;                   // 4 waves, 2 x 2, one 32 x 32 MFMA accumulator each
static_assert(BM == 64 && BN == 64 && BK % 2 == 0 && THREADS % BK == 0, "the wave layout below is for a 64 x 64 tile");
static_assert(BN == VF_WAVE && VF_TOPK_MAX_K <= VF_WAVE, "one lane per tile column and per rank");
static_assert((BM + BN) * LDT >= BM * BN, "the score tile reuses the operand tiles' LDS");

// (key, 2^32 - 1 - j): larger = ranks first, the lower j among equal keys.  nj == 0 marks an empty slot (j < 2^31, so no row has it).
__device__ __forceinline__ unsigned long long rank_pair(uint32_t vbits, uint32_t nj) {
    return nj ? ((unsigned long long)order_key(vbits) << 32) | nj : 0ull;
}

// The 64 x 64 tile of s(q0 + ., j0 + .) into S (row-major, BN words per row; S overlays the operand tiles).  Every thread of
// the block calls it; it ends behind a barrier, with S complete.  Rows at or past Rq / Ry are computed from zeros and are the
// caller's to ignore.  The column range is walked in MFMA steps of 2: lane half h takes column kk + h, so the accumulator of
// (r, j) sees the columns in ascending order, and a step that straddles d is padded with (-0) * (+0) = -0, the one addend
// that leaves every accumulator as it is, -0 and NaN payloads included.
__device__ __forceinline__ void tile_scores(const float* __restrict__ q, int64_t ldq, int64_t q0, int64_t Rq,
                                            const float* __restrict__ y, int64_t ldy, int64_t j0, int64_t Ry, int d, float* tiles) {
    float* As = tiles;
    float* Bs = tiles + BM * LDT;
    float* S = tiles;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lrow = tid / BK, lcol = tid % BK;
    constexpr int NLOAD = BM / (THREADS / BK);                          // rows of each operand tile a thread stages per step
    // Every load is unconditional and lands inside the operands: a row past the end reads the last row, a column past d reads
    // column d - 1, and the value is replaced by the padding on its way to LDS.  The loads of stage s + 1 are issued before the
    // MFMAs of stage s and waited for after them.
    const float* pa[NLOAD];
    const float* pb[NLOAD];
    unsigned in_a = 0, in_b = 0;
#pragma unroll
    for (int i = 0; i < NLOAD; ++i) {
        const int64_t qr = q0 + i * (THREADS / BK) + lrow, yr = j0 + i * (THREADS / BK) + lrow;
        pa[i] = q + (qr < Rq ? qr : Rq - 1) * ldq;
        pb[i] = y + (yr < Ry ? yr : Ry - 1) * ldy;
        in_a |= (unsigned)(qr < Rq) << i;
        in_b |= (unsigned)(yr < Ry) << i;
    }
    float ra[NLOAD], rb[NLOAD];
    auto fetch = [&](int kk0) {
        const int c = min(kk0 + lcol, d - 1);
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) {
            ra[i] = pa[i][c];
            rb[i] = pb[i][c];
        }
    };
    f32x16_t acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const float* ap = As + (wm * 32 + (lane & 31)) * LDT + (lane >> 5);
    const float* bp = Bs + (wn * 32 + (lane & 31)) * LDT + (lane >> 5);
    fetch(0);
    for (int kk0 = 0; kk0 < d; kk0 += BK) {
        const bool col_in = kk0 + lcol < d;
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) {
            const int row = i * (THREADS / BK) + lrow;
            As[row * LDT + lcol] = (col_in && (in_a >> i & 1u)) ? ra[i] : -0.0f;
            Bs[row * LDT + lcol] = (col_in && (in_b >> i & 1u)) ? rb[i] : 0.0f;
        }
        __syncthreads();
        if (kk0 + BK < d) fetch(kk0 + BK);                             // block-uniform
        const int steps = d - kk0;                                     // block-uniform
        if (steps >= BK) {
#pragma unroll
            for (int k2 = 0; k2 < BK; k2 += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k2], bp[k2], acc, 0, 0, 0);
        } else {
            for (int k2 = 0; k2 < steps; k2 += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k2], bp[k2], acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = wm * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
        S[row * BN + wn * 32 + (lane & 31)] = acc[reg];
    }
    __syncthreads();
}

// One block = BM query rows; wave w keeps the running best of rows 16 w .. 16 w + 15 in LDS (value bits and 2^32 - 1 - j, rank i
// in slot i) and, after every tile, takes the row's 64 new scores one per lane: those above the row's rank k - 1 are inserted
// in lane order.  Slots at or past k hold candidates that fell out of the first k; they are never written out.
__global__ __launch_bounds__(THREADS) void knn_dot_kernel(const float* __restrict__ q, int64_t ldq, int64_t Rq,
                                                          const float* __restrict__ y, int64_t ldy, int64_t Ry, int d,
                                                          int64_t self_offset, int k, float* __restrict__ values,
                                                          int32_t* __restrict__ indices, int64_t ldo) {
    __shared__ __attribute__((aligned(16))) float tiles[(BM + BN) * LDT];
    __shared__ uint32_t best_v[BM * 64];
    __shared__ uint32_t best_nj[BM * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q0 = (int64_t)blockIdx.x * BM;
    for (int i = tid; i < BM * 64; i += THREADS) {
        best_v[i] = 0u;
        best_nj[i] = 0u;
    }
    // Thread t initialises slots t, t + 256, ...: the rows a wave reads later are written by all four waves.  The first barrier of
    // tile_scores orders these stores before the merge's reads; with Ry == 0 there is no tile, and the barrier behind the loop
    // is what orders them before the final read-out.  It must stay.
    for (int64_t j0 = 0; j0 < Ry; j0 += BN) {
        tile_scores(q, ldq, q0, Rq, y, ldy, j0, Ry, d, tiles);
        const float* S = tiles;
        const int64_t j = j0 + lane;
        for (int rr = 0; rr < BM / 4; ++rr) {
            const int row = wave * (BM / 4) + rr;
            const int64_t r = q0 + row;
            if (r >= Rq) break;                                           // wave-uniform
            const bool valid = j < Ry && !(self_offset >= 0 && j - r == self_offset);     // j - r cannot overflow: j < 2^31, r < 2^36
            const uint32_t cv = __float_as_uint(S[row * BN + lane]);
            const uint32_t cnj = valid ? 0xFFFFFFFFu - (uint32_t)j : 0u;
            const unsigned long long c = rank_pair(cv, cnj);
            unsigned long long thr = rank_pair(best_v[row * 64 + k - 1], best_nj[row * 64 + k - 1]);
            unsigned long long todo = __ballot(c > thr);
            if (todo == 0ull) continue;                                   // wave-uniform
            uint32_t mv = best_v[row * 64 + lane], mnj = best_nj[row * 64 + lane];
            unsigned long long mine = rank_pair(mv, mnj);
            while (todo) {
                const int src = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const unsigned long long nc = __shfl(c, src);
                if (nc <= __shfl(mine, k - 1)) continue;                  // rank k - 1 has risen above it meanwhile
                const uint32_t nv = __shfl(cv, src), nnj = __shfl(cnj, src);
                const int pos = __popcll(__ballot(mine > nc));            // the ranks before it; pairs are distinct
                const unsigned long long up = __shfl_up(mine, 1);
                const uint32_t upv = __shfl_up(mv, 1), upnj = __shfl_up(mnj, 1);
                if (lane == pos) {
                    mine = nc; mv = nv; mnj = nnj;
                } else if (lane > pos) {
                    mine = up; mv = upv; mnj = upnj;
                }
            }
            best_v[row * 64 + lane] = mv;
            best_nj[row * 64 + lane] = mnj;
        }
        __syncthreads();                                                  // S is the next tile's operand space
    }
    __syncthreads();
    for (int rr = 0; rr < BM / 4; ++rr) {
        const int row = wave * (BM / 4) + rr;
        const int64_t r = q0 + row;
        if (r >= Rq) break;
        if (lane < k) {
            const uint32_t nj = best_nj[row * 64 + lane];
            const int64_t o = r * ldo + lane;
            indices[o] = nj ? (int32_t)(0xFFFFFFFFu - nj) : -1;
            reinterpret_cast<uint32_t*>(values)[o] = nj ? best_v[row * 64 + lane] : 0u;   // the accumulator's bits: payloads and -0 survive
        }
    }
}

// One block = one BM x BN tile of out; tile t of panel p is block p * tiles_n + t.
__global__ __launch_bounds__(THREADS) void pairwise_dot_kernel(const float* __restrict__ q, int64_t ldq, int64_t Rq,
                                                               const float* __restrict__ y, int64_t ldy, int64_t Ry, int d,
                                                               int64_t self_offset, int mode, float* __restrict__ out, int64_t ldo,
                                                               unsigned tiles_n) {
    __shared__ __attribute__((aligned(16))) float tiles[(BM + BN) * LDT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q0 = (int64_t)(blockIdx.x / tiles_n) * BM, j0 = (int64_t)(blockIdx.x % tiles_n) * BN;
    tile_scores(q, ldq, q0, Rq, y, ldy, j0, Ry, d, tiles);
    const float* S = tiles;
    const int64_t j = j0 + lane;
    if (j >= Ry) return;
    for (int row = wave; row < BM; row += THREADS / 64) {
        const int64_t r = q0 + row;
        if (r >= Rq) break;
        float s = S[row * BN + lane];
        if (mode == 1) s = (self_offset >= 0 && j - r == self_offset) ? 0.f : 1.0f - s;          // j - r cannot overflow
        out[r * ldo + j] = s;
    }
}

// One wave per row, 4 rows per block.  No __restrict__: z may be x.
__global__ __launch_bounds__(THREADS) void rows_standardize_kernel(const float* x, int64_t ldx, int64_t R, int d, int center,
                                                                   float* z, int64_t ldz, float* norm) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (r >= R) return;                                                   // wave-uniform
    const float* xr = x + r * ldx;
    float mean = 0.f;
    bool same = false;                                                    // center: every value equals the first (a NaN equals nothing)
    if (center) {
        float s = 0.f;
        const float first = xr[0];
        int differ = 0;
        for (int c = lane; c < d; c += 64) {
            const float v = xr[c];
            s += v;
            differ |= !(v == first);
        }
        mean = wave_sum(s) / (float)d;
        same = __ballot(differ) == 0ull;
    }
    float ss = 0.f;
    for (int c = lane; c < d; c += 64) {
        const float t = xr[c] - mean;
        ss = fmaf(t, t, ss);
    }
    float nrm = sqrtf(wave_sum(ss));
    const bool bad = !(nrm < __builtin_inff());                           // NaN or +Inf
    const bool flat = !bad && (nrm == 0.f || same);                       // a constant row whose fp32 mean is off by an ulp is still constant
    if (bad) nrm = __builtin_nanf("");
    float* zr = z + r * ldz;
    for (int c = lane; c < d; c += 64) {
        const float t = xr[c] - mean;
        zr[c] = bad ? nrm : (flat ? 0.f : t / nrm);
    }
    if (norm && lane == 0) norm[r] = flat ? 0.f : nrm;
}


// The checks vf_knn_dot and vf_pairwise_dot share; `out` is the name of the width ldo is held against.
int check_operands(const char* fn, const float* q, int64_t ldq, int64_t Rq, const float* y, int64_t ldy, int64_t Ry, int d,
                   int64_t self_offset) {
    VF_REQUIRE(q, "%s: null pointer q", fn);
    VF_REQUIRE(y, "%s: null pointer y", fn);
    VF_REQUIRE(VF_ALIGNED4(q), "%s: q must be 4-byte aligned", fn);
    VF_REQUIRE(VF_ALIGNED4(y), "%s: y must be 4-byte aligned", fn);
    VF_REQUIRE(d >= 1, "%s: d=%d must be at least 1", fn, d);
    VF_REQUIRE(ldq >= d, "%s: ldq=%ld is below d=%d", fn, (long)ldq, d);
    VF_REQUIRE(ldy >= d, "%s: ldy=%ld is below d=%d", fn, (long)ldy, d);
    VF_REQUIRE(Rq >= 0, "%s: Rq=%ld must not be negative", fn, (long)Rq);
    VF_REQUIRE(Ry >= 0, "%s: Ry=%ld must not be negative", fn, (long)Ry);
    VF_REQUIRE(Ry < ((int64_t)1 << 31), "%s: Ry=%ld does not fit an int32 index (2^31)", fn, (long)Ry);
    VF_REQUIRE(self_offset >= -1, "%s: self_offset=%ld must be -1 (none) or a row of y", fn, (long)self_offset);
    return VF_OK;
}

}  // namespace

extern "C" int vf_rows_standardize(const float* x, int64_t ldx, int64_t R, int d, int center, float* z, int64_t ldz, float* norm,
                                   void* stream) {
    VF_REQUIRE(x, "vf_rows_standardize: null pointer x");
    VF_REQUIRE(z, "vf_rows_standardize: null pointer z");
    VF_REQUIRE(VF_ALIGNED4(x), "vf_rows_standardize: x must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(z), "vf_rows_standardize: z must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(norm), "vf_rows_standardize: norm must be 4-byte aligned");
    VF_REQUIRE(d >= 1, "vf_rows_standardize: d=%d must be at least 1", d);
    VF_REQUIRE(ldx >= d, "vf_rows_standardize: ldx=%ld is below d=%d", (long)ldx, d);
    VF_REQUIRE(ldz >= d, "vf_rows_standardize: ldz=%ld is below d=%d", (long)ldz, d);
    VF_REQUIRE(center == 0 || center == 1, "vf_rows_standardize: center=%d must be 0 or 1", center);
    VF_REQUIRE(R >= 0, "vf_rows_standardize: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R < ((int64_t)1 << 33), "vf_rows_standardize: grid of R=%ld rows (four per block) does not fit 2^31 blocks", (long)R);
    if (R == 0) return VF_OK;
    const unsigned blocks = (unsigned)((R + THREADS / 64 - 1) / (THREADS / 64));
    hipLaunchKernelGGL(rows_standardize_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, x, ldx, R, d, center, z, ldz,
                       norm);
    VF_CHECK_LAUNCH("vf_rows_standardize");
    return VF_OK;
}

extern "C" int vf_knn_dot(const float* q, int64_t ldq, int64_t Rq, const float* y, int64_t ldy, int64_t Ry, int d,
                          int64_t self_offset, int k, float* values, int32_t* indices, int64_t ldo, void* stream) {
    if (int rc = check_operands("vf_knn_dot", q, ldq, Rq, y, ldy, Ry, d, self_offset)) return rc;
    VF_REQUIRE(values, "vf_knn_dot: null pointer values");
    VF_REQUIRE(indices, "vf_knn_dot: null pointer indices");
    VF_REQUIRE(VF_ALIGNED4(values), "vf_knn_dot: values must be 4-byte aligned");
    VF_REQUIRE(VF_ALIGNED4(indices), "vf_knn_dot: indices must be 4-byte aligned");
    VF_REQUIRE(k >= 1 && k <= VF_TOPK_MAX_K, "vf_knn_dot: k=%d must lie in 1 .. %d", k, VF_TOPK_MAX_K);
    VF_REQUIRE(ldo >= k, "vf_knn_dot: ldo=%ld is below k=%d", (long)ldo, k);
    VF_REQUIRE(Rq < ((int64_t)1 << 36), "vf_knn_dot: grid of Rq=%ld rows (%d per block) does not fit 2^31 blocks", (long)Rq, BM);
    if (Rq == 0) return VF_OK;
    const unsigned blocks = (unsigned)((Rq + BM - 1) / BM);
    hipLaunchKernelGGL(knn_dot_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, q, ldq, Rq, y, ldy, Ry, d, self_offset,
                       k, values, indices, ldo);
    VF_CHECK_LAUNCH("vf_knn_dot");
    return VF_OK;
}

extern "C" int vf_pairwise_dot(const float* q, int64_t ldq, int64_t Rq, const float* y, int64_t ldy, int64_t Ry, int d,
                               int64_t self_offset, int mode, float* out, int64_t ldo, void* stream) {
    if (int rc = check_operands("vf_pairwise_dot", q, ldq, Rq, y, ldy, Ry, d, self_offset)) return rc;
    VF_REQUIRE(out, "vf_pairwise_dot: null pointer out");
    VF_REQUIRE(VF_ALIGNED4(out), "vf_pairwise_dot: out must be 4-byte aligned");
    VF_REQUIRE(mode == 0 || mode == 1, "vf_pairwise_dot: mode=%d must be 0 (similarity) or 1 (1 - similarity)", mode);
    VF_REQUIRE(ldo >= Ry, "vf_pairwise_dot: ldo=%ld is below Ry=%ld", (long)ldo, (long)Ry);
    const int64_t tiles_m = (Rq + BM - 1) / BM, tiles_n = (Ry + BN - 1) / BN;
    VF_REQUIRE(tiles_n == 0 || tiles_m <= (((int64_t)1 << 31) - 1) / tiles_n,
               "vf_pairwise_dot: grid of %ld x %ld tiles does not fit 2^31 blocks", (long)tiles_m, (long)tiles_n);
    if (Rq == 0 || Ry == 0) return VF_OK;
    hipLaunchKernelGGL(pairwise_dot_kernel, dim3((unsigned)(tiles_m * tiles_n)), dim3(THREADS), 0, (hipStream_t)stream, q, ldq, Rq,
                       y, ldy, Ry, d, self_offset, mode, out, ldo, (unsigned)tiles_n);
    VF_CHECK_LAUNCH("vf_pairwise_dot");
    return VF_OK;
}

// Row-wise top-k of the attention and contribution maps (include/vf_hip_topk.h): the k first-ranked values of every row and
// their columns, so that a ranking crosses to the host instead of the map.  Comparisons only; the order is total and defined
// for NaN, +-0 and ties, which is why this file is built without -fno-honor-nans (csrc/build.py: that flag is vf_attn.hip's).
#include "vf_common.h"

namespace {

// order_key (vf_common.h): the smallest key is -Inf's 0x007FFFFF, so a pair (key << 32 | VF_TOPK_MAX_N - column) is never 0: 0 = no column.

// One block = one wave = one row.  Round i finds the largest pair below round i - 1's: lane l scans the columns l, l + 64, ...
// of the staged keys, the butterfly leaves the winner in every lane, and lane i keeps it.  The pairs of a row are distinct,
// so "below the last winner" removes exactly the columns already ranked, with no store to LDS between the rounds.
__global__ __launch_bounds__(64) void topk_rows_kernel(const float* __restrict__ x, int64_t ldx, int n,
                                                      const int32_t* __restrict__ row_len, int k, float* __restrict__ values,
                                                      int32_t* __restrict__ indices, int64_t ldo) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t* keys = reinterpret_cast<uint32_t*>(smem);
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    int len = n;
    if (row_len) {                                                    // block-uniform
        len = row_len[r];
        len = len < 0 ? 0 : (len > n ? n : len);
    }
    const uint32_t* xr = reinterpret_cast<const uint32_t*>(x) + r * ldx;
    for (int c = lane; c < len; c += 64) keys[c] = order_key(xr[c]);
    __syncthreads();
    unsigned long long prev = ~0ull, mine = 0ull;                     // every pair is below ~0: its low word is at most 16384
    for (int i = 0; i < k; ++i) {
        unsigned long long best = 0ull;
        for (int c = lane; c < len; c += 64) {
            const unsigned long long p = ((unsigned long long)keys[c] << 32) | (uint32_t)(VF_TOPK_MAX_N - c);
            if (p < prev && p > best) best = p;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off);
            best = o > best ? o : best;
        }
        if (best == 0ull) break;                                      // wave-uniform: the row has no column left, the rest is padding
        if (lane == i) mine = best;
        prev = best;
    }
    if (lane >= k) return;
    const int64_t o = r * ldo + lane;
    if (mine != 0ull) {
        const int col = VF_TOPK_MAX_N - (int)(uint32_t)mine;
        indices[o] = col;
        reinterpret_cast<uint32_t*>(values)[o] = xr[col];             // the bits of x, not of the key: NaN payloads and -0 survive
    } else {
        indices[o] = -1;
        values[o] = 0.f;
    }
}

}  // namespace

extern "C" int vf_topk_rows(const float* x, int64_t ldx, int64_t R, int n, const int32_t* row_len, int k, float* values,
                            int32_t* indices, int64_t ldo, void* stream) {
    VF_REQUIRE(x, "vf_topk_rows: null pointer x");
    VF_REQUIRE(values, "vf_topk_rows: null pointer values");
    VF_REQUIRE(indices, "vf_topk_rows: null pointer indices");
    VF_REQUIRE((uintptr_t)x % 4 == 0, "vf_topk_rows: x must be 4-byte aligned");
    VF_REQUIRE((uintptr_t)row_len % 4 == 0, "vf_topk_rows: row_len must be 4-byte aligned");
    VF_REQUIRE((uintptr_t)values % 4 == 0, "vf_topk_rows: values must be 4-byte aligned");
    VF_REQUIRE((uintptr_t)indices % 4 == 0, "vf_topk_rows: indices must be 4-byte aligned");
    VF_REQUIRE(n >= 0 && n <= VF_TOPK_MAX_N, "vf_topk_rows: n=%d must lie in 0 .. %d (a row's keys fit 64 KB of LDS)", n, VF_TOPK_MAX_N);
    VF_REQUIRE(k >= 1 && k <= VF_TOPK_MAX_K, "vf_topk_rows: k=%d must lie in 1 .. %d", k, VF_TOPK_MAX_K);
    VF_REQUIRE(ldx >= n, "vf_topk_rows: ldx=%ld is below n=%d", (long)ldx, n);
    VF_REQUIRE(ldo >= k, "vf_topk_rows: ldo=%ld is below k=%d", (long)ldo, k);
    VF_REQUIRE(R >= 0, "vf_topk_rows: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R < ((int64_t)1 << 31), "vf_topk_rows: grid of R=%ld blocks (one per row) does not fit 2^31", (long)R);
    if (R == 0) return VF_OK;
    const size_t lds = (size_t)n * sizeof(uint32_t);
    hipLaunchKernelGGL(topk_rows_kernel, dim3((unsigned)R), dim3(64), lds, (hipStream_t)stream, x, ldx, n, row_len, k, values,
                       indices, ldo);
    VF_CHECK_LAUNCH("vf_topk_rows");
    return VF_OK;
}

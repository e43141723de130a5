// Decision-forest evaluation on embeddings (include/vf_hip_forest.h): a bank of packed forests, one row through its forest
// per wave.  Gather-bound: every step of a walk is one 16-byte node load that depends on the one before, so the work is
// spread as trees over lanes (64 walks in flight per row) and rows over blocks; the row itself sits in LDS.
#include "vf_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4_t;

#define VF_FOREST_MAX_K 8

// One block = one wave = one row.  Lane l walks the trees l, l + 64, ... of the row's model and keeps K partial sums; the
// butterfly leaves the K totals in every lane, lane 0 finishes and stores them.
__global__ __launch_bounds__(64) void forest_predict_kernel(const float* __restrict__ x, int64_t ldx, int F,
                                                           const i32x4_t* __restrict__ nodes, const int32_t* __restrict__ tree_root,
                                                           const float* __restrict__ leaf_values, const float* __restrict__ base_scores,
                                                           const int32_t* __restrict__ model_node_base,
                                                           const int32_t* __restrict__ model_tree_base,
                                                           const int32_t* __restrict__ model_leaf_base,
                                                           const int32_t* __restrict__ model_n_trees, int n_models, int K, int average,
                                                           int postprocessor, const int32_t* __restrict__ model_of_row, int model,
                                                           float* __restrict__ out, int64_t ldo) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* xs = reinterpret_cast<float*>(smem);
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int m = model_of_row ? model_of_row[r] : model;           // block-uniform
    float* orow = out + r * ldo;
    if (m < 0 || m >= n_models) {                                    // no such forest: nothing is read, the row is NaN
        if (lane < K) orow[lane] = __uint_as_float(0x7FC00000u);
        return;
    }
    const float* xr = x + r * ldx;
    for (int f = lane; f < F; f += 64) xs[f] = xr[f];
    __syncthreads();
    const i32x4_t* nd = nodes + model_node_base[m];
    const int32_t* roots = tree_root + model_tree_base[m];
    const float* leaves = leaf_values + (int64_t)model_leaf_base[m] * K;
    const int T = model_n_trees[m];
    float acc[VF_FOREST_MAX_K];
#pragma unroll
    for (int k = 0; k < VF_FOREST_MAX_K; ++k) acc[k] = 0.f;
    for (int t = lane; t < T; t += 64) {
        i32x4_t n = nd[roots[t]];
        while (n[0] >= 0) {
            const float v = xs[n[0] & 0xFFFF];
            const bool left = (v != v) ? ((n[0] >> 16) & 1) != 0 : v <= __int_as_float(n[1]);
            n = nd[left ? n[2] : n[3]];
        }
        const float* lv = leaves + (int64_t)n[2] * K;
#pragma unroll
        for (int k = 0; k < VF_FOREST_MAX_K; ++k)
            if (k < K) acc[k] += lv[k];
    }
#pragma unroll
    for (int k = 0; k < VF_FOREST_MAX_K; ++k)
        if (k < K) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off);
        }
    if (lane != 0) return;
    const float fT = (float)T;
    const float* base = base_scores + (int64_t)m * K;
#pragma unroll
    for (int k = 0; k < VF_FOREST_MAX_K; ++k)
        if (k < K) acc[k] = (average ? acc[k] / fT : acc[k]) + base[k];
    if (postprocessor == VF_FOREST_SIGMOID) {
#pragma unroll
        for (int k = 0; k < VF_FOREST_MAX_K; ++k)
            if (k < K) acc[k] = 1.0f / (1.0f + expf(-acc[k]));
    } else if (postprocessor == VF_FOREST_SOFTMAX) {
        float mx = acc[0];
#pragma unroll
        for (int k = 1; k < VF_FOREST_MAX_K; ++k)
            if (k < K) mx = fmaxf(mx, acc[k]);
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < VF_FOREST_MAX_K; ++k)
            if (k < K) { acc[k] = expf(acc[k] - mx); sum += acc[k]; }
#pragma unroll
        for (int k = 0; k < VF_FOREST_MAX_K; ++k)
            if (k < K) acc[k] = acc[k] / sum;
    }
#pragma unroll
    for (int k = 0; k < VF_FOREST_MAX_K; ++k)
        if (k < K) orow[k] = acc[k];
}

}  // namespace

extern "C" int vf_forest_predict(const float* x, int64_t ldx, int64_t R, int F, const int32_t* nodes, const int32_t* tree_root,
                                 const float* leaf_values, const float* base_scores, const int32_t* model_node_base,
                                 const int32_t* model_tree_base, const int32_t* model_leaf_base, const int32_t* model_n_trees,
                                 int n_models, int K, int average, int postprocessor, const int32_t* model_of_row, int model,
                                 float* out, int64_t ldo, void* stream) {
    VF_REQUIRE(x, "vf_forest_predict: null pointer x");
    VF_REQUIRE(nodes, "vf_forest_predict: null pointer nodes");
    VF_REQUIRE(tree_root, "vf_forest_predict: null pointer tree_root");
    VF_REQUIRE(leaf_values, "vf_forest_predict: null pointer leaf_values");
    VF_REQUIRE(base_scores, "vf_forest_predict: null pointer base_scores");
    VF_REQUIRE(model_node_base, "vf_forest_predict: null pointer model_node_base");
    VF_REQUIRE(model_tree_base, "vf_forest_predict: null pointer model_tree_base");
    VF_REQUIRE(model_leaf_base, "vf_forest_predict: null pointer model_leaf_base");
    VF_REQUIRE(model_n_trees, "vf_forest_predict: null pointer model_n_trees");
    VF_REQUIRE(out, "vf_forest_predict: null pointer out");
    VF_REQUIRE(F >= 1 && F <= 4096, "vf_forest_predict: F=%d must lie in 1 .. 4096", F);
    VF_REQUIRE(K >= 1 && K <= VF_FOREST_MAX_K, "vf_forest_predict: K=%d must lie in 1 .. %d", K, VF_FOREST_MAX_K);
    VF_REQUIRE(n_models >= 1, "vf_forest_predict: n_models=%d must be positive", n_models);
    VF_REQUIRE(average == 0 || average == 1, "vf_forest_predict: bad average %d (0 = sum, 1 = mean of the trees)", average);
    VF_REQUIRE(postprocessor >= VF_FOREST_IDENTITY && postprocessor <= VF_FOREST_SOFTMAX,
               "vf_forest_predict: bad postprocessor %d (0 = identity, 1 = sigmoid, 2 = softmax)", postprocessor);
    VF_REQUIRE(ldx >= F, "vf_forest_predict: ldx=%ld is below F=%d", (long)ldx, F);
    VF_REQUIRE(ldo >= K, "vf_forest_predict: ldo=%ld is below K=%d", (long)ldo, K);
    VF_REQUIRE((model_of_row != nullptr) != (model >= 0),
               "vf_forest_predict: exactly one of model_of_row and model must be given (%s)", model_of_row ? "both are" : "neither is");
    VF_REQUIRE((uintptr_t)nodes % 16 == 0, "vf_forest_predict: nodes must be 16-byte aligned");
    VF_REQUIRE((uintptr_t)x % 4 == 0, "vf_forest_predict: x must be 4-byte aligned");
    VF_REQUIRE((uintptr_t)tree_root % 4 == 0, "vf_forest_predict: tree_root must be 4-byte aligned");
    VF_REQUIRE((uintptr_t)leaf_values % 4 == 0, "vf_forest_predict: leaf_values must be 4-byte aligned");
    VF_REQUIRE((uintptr_t)base_scores % 4 == 0, "vf_forest_predict: base_scores must be 4-byte aligned");
    VF_REQUIRE((uintptr_t)model_node_base % 4 == 0, "vf_forest_predict: model_node_base must be 4-byte aligned");
    VF_REQUIRE((uintptr_t)model_tree_base % 4 == 0, "vf_forest_predict: model_tree_base must be 4-byte aligned");
    VF_REQUIRE((uintptr_t)model_leaf_base % 4 == 0, "vf_forest_predict: model_leaf_base must be 4-byte aligned");
    VF_REQUIRE((uintptr_t)model_n_trees % 4 == 0, "vf_forest_predict: model_n_trees must be 4-byte aligned");
    VF_REQUIRE((uintptr_t)model_of_row % 4 == 0, "vf_forest_predict: model_of_row must be 4-byte aligned");
    VF_REQUIRE((uintptr_t)out % 4 == 0, "vf_forest_predict: out must be 4-byte aligned");
    VF_REQUIRE(R >= 0, "vf_forest_predict: R=%ld must not be negative", (long)R);
    VF_REQUIRE(R < ((int64_t)1 << 31), "vf_forest_predict: grid of R=%ld blocks (one per row) does not fit 2^31", (long)R);
    if (R == 0) return VF_OK;
    const size_t lds = ((size_t)F * sizeof(float) + 15) & ~(size_t)15;
    hipLaunchKernelGGL(forest_predict_kernel, dim3((unsigned)R), dim3(64), lds, (hipStream_t)stream, x, ldx, F,
                       reinterpret_cast<const i32x4_t*>(nodes), tree_root, leaf_values, base_scores, model_node_base, model_tree_base,
                       model_leaf_base, model_n_trees, n_models, K, average, postprocessor, model_of_row, model, out, ldo);
    VF_CHECK_LAUNCH("vf_forest_predict");
    return VF_OK;
}

/* vf_hip_forest.h -- the entry of libvf_hip.so behind the per-(gene, tissue) forest predictors on embeddings (AD risk).
 *
 * One of six headers of the one library, beside vf_hip.h, vf_hip_attn_contrib.h, vf_hip_gene_contrib.h, vf_hip_cre_heads.h and vf_hip_topk.h.  Its
 * entry is bound through _lib.ENTRIES["vf_hip_forest.h"], which _lib.load() applies like the other five tables, and every stream-taking
 * declaration here has poisoned-memory write-set cases in tests/forest_cases.py.  Everything the main header says holds here:
 * the conventions at its top (device pointers owned by the caller, `stream` a hipStream_t, strides in elements, 0 = ok /
 * VF_ERR_*, vf_last_error()), the comment contract of every entry (arguments, write set, arithmetic, non-finite operands,
 * refusals), and VF_ABI_VERSION: a new symbol changes no existing one, so the version stays 13.
 */
#ifndef VF_HIP_FOREST_H
#define VF_HIP_FOREST_H

#include "vf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* postprocessor of vf_forest_predict */
#define VF_FOREST_IDENTITY 0
#define VF_FOREST_SIGMOID 1
#define VF_FOREST_SOFTMAX 2

/* A bank of decision forests evaluated on fp32 rows (added under ABI 13): the reference's processors/ad_risk.py calls
 * treelite.gtil.predict once per DataFrame row on the host; here every row of a call goes through its forest in one launch.
 * The bank is what variantformer_amd/forest.py (ForestBank) packs and uploads; its arrays are trusted (the host validates
 * them: every index in range and every child index above its parent's, so a walk ends).
 * Arguments:
 *   x          fp32 [R, >= F], rows ldx elements apart (64-bit row offsets): one feature vector per row;
 *   nodes      int32 [n_nodes, 4], 16 bytes per node, all models' nodes end to end:
 *                word 0  -1 for a leaf, else feature | default_left << 16 (feature in 0 .. F-1, default_left 0 / 1);
 *                word 1  the bits of the fp32 threshold;
 *                word 2  the left child, or for a leaf its row in the model's leaf values;
 *                word 3  the right child;
 *              child indices, tree roots and leaf rows are relative to the model: the kernel adds the model's base;
 *   tree_root  int32 [n_trees_total]: the root node of every tree, models end to end;
 *   leaf_values fp32 [n_leaves_total, K] contiguous;  base_scores fp32 [n_models, K] contiguous;
 *   model_node_base / model_tree_base / model_leaf_base / model_n_trees  int32 [n_models]: where model m's nodes, trees
 *              and leaf rows begin, and its tree count T;
 *   average    0 / 1: divide the sum of the trees by T;  postprocessor: VF_FOREST_IDENTITY / _SIGMOID / _SOFTMAX;
 *   row form    (model_of_row != NULL, int32 [R]; model must be -1): row r goes through the forest model_of_row[r];
 *   cohort form (model_of_row == NULL, model >= 0): every row goes through the forest `model`;
 *   out        fp32 [R, >= K], rows ldo elements apart.
 * Write set: out[r * ldo + 0 .. K-1] for 0 <= r < R.  Columns of out at or past K and rows at or past R are not touched; x,
 * the bank and model_of_row are only read.  A model index outside 0 .. n_models-1, in either form, reads nothing (not the
 * row of x either): the K values of that row are NaN, every other row is as without it.
 * Arithmetic, per row, all in fp32:
 *   every tree is walked from its root: at an inner node with feature f and threshold t the walk goes LEFT iff
 *   x[r, f] <= t (one fp32 comparison; the converter has rounded t so that this is the model's own decision), and a NaN
 *   x[r, f] goes left iff default_left;
 *   s[k] = the sum over the trees of leaf_values[leaf, k]: lane l of the row's one wave adds the trees l, l + 64, l + 128, ...
 *   in ascending order starting from +0, then the 64 partial sums are combined by the xor butterfly 32, 16, 8, 4, 2, 1 -- an
 *   order fixed by T alone; no atomics, no workspace;
 *   v[k] = (average ? s[k] / (float)T : s[k]) + base_scores[m, k]  (one IEEE division, one addition);
 *   identity: out = v[k];  sigmoid: out = 1 / (1 + expf(-v[k]));  softmax: out = e[k] / (e[0] + e[1] + ... + e[K-1]) with
 *   e[k] = expf(v[k] - max_k v[k]), added in ascending k.
 * One block of 64 threads per row; the row is staged in F * 4 bytes of LDS once.  The bits of out[r, :] depend on row r
 * of x and on its model alone: not on R, ldx, ldo, the row's position, which other models the bank holds, or on which of the
 * two forms was called.
 * Non-finite operands: a NaN feature follows default_left at every node that tests it; +Inf goes right
 * unless the threshold is +Inf, -Inf goes left; features no node tests are never looked at.  A NaN or Inf leaf value or
 * base score reaches the outputs of the rows whose walk ends in it (IEEE sums: Inf - Inf = NaN), and no other row; under
 * softmax a row whose maximum is +Inf is NaN, as torch.softmax makes it.
 * Refused before anything is launched (VF_ERR_INVALID_ARG, the argument named in vf_last_error()): a null x, nodes, tree_root,
 * leaf_values, base_scores, model_node_base, model_tree_base, model_leaf_base, model_n_trees or out; nodes not 16-byte
 * aligned; any other pointer not 4-byte aligned; F outside 1 .. 4096; K outside 1 .. 8; n_models < 1; average outside
 * {0, 1}; postprocessor outside 0 .. 2; ldx < F; ldo < K; both or neither of model_of_row and model given (model >= 0 beside
 * model_of_row, or model < 0 without it); R < 0; R >= 2^31 (the grid: one block per row).  R == 0 is VF_OK with nothing
 * launched. */
int vf_forest_predict(const float* x, int64_t ldx, int64_t R, int F, const int32_t* nodes, const int32_t* tree_root,
                      const float* leaf_values, const float* base_scores, const int32_t* model_node_base,
                      const int32_t* model_tree_base, const int32_t* model_leaf_base, const int32_t* model_n_trees,
                      int n_models, int K, int average, int postprocessor, const int32_t* model_of_row, int model,
                      float* out, int64_t ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_FOREST_H */

/*
 * hipac_mil_levels.h -- C ABI of multiscale attention pooling for the MIL head of libhipac_hip.so (gfx950).
 *
 * A bag holds the feature rows of several pyramid levels of one slide.  Every level has its own attention branch over
 * the shared hidden layer and its own softmax over that level's rows of the bag; the per-level pooled vectors are
 * concatenated level-major in front of the classifier.  With L = levels, F = feature_dim, A = attn_dim, for one bag
 * x [N][F] and lev(i) in 0..L-1 the level slot of row i:
 *     H = tanh(attn_V(x)) [N][A]      s_i = U[lev(i)] . H_i + b_U[lev(i)]
 *     a_i = softmax of s over the rows j of the bag with lev(j) = lev(i)
 *     M[k] = sum_{lev(i) = k} a_i x_i [L][F]  (all zeros where the bag has no row of level k, never NaN)
 *     pooled = M reshaped to [L F], level-major      logits = classifier(pooled)
 * This is the model of include/hipac_mil_heads.h with heads = L and the scores of every row at minus infinity in the
 * heads of the other levels.  The parameters are those of hipac_mil_params_t (include/hipac.h) in the shapes of that
 * model:
 *     attn_V_w [attn_dim][feature_dim], attn_V_b [attn_dim]           shared by the levels
 *     attn_U_w [levels][attn_dim],      attn_U_b [levels]
 *     fc1_w    [hidden_dim][levels * feature_dim], fc1_b [hidden_dim]
 *     fc2_w    [num_classes][hidden_dim], fc2_b [num_classes]
 *
 * A row belongs to one level, so its score, its pooling multiply-add, the row dot product of the softmax backward and
 * its ds U product are formed once, not once per level.  The step reads X for X V^T, for the pooled vectors, for the
 * row dot products and for dV = dH^T X -- four times, as the single-head step does.
 * These entry points live in the same shared library as include/hipac.h and include/hipac_mil_heads.h but carry
 * their own version number.
 *
 * Conventions: those of include/hipac.h.  Data pointers are DEVICE memory; all work is enqueued asynchronously on
 * `stream` (hipStream_t as void*, NULL = default stream); nothing synchronises the device; the caller owns every
 * buffer, the workspace included; 0 on success, otherwise a hipError_t value or a HIPAC_E* code with the message in
 * hipac_last_error().  float32 throughout.  Bitwise reproducible: no floating-point atomics, every cross-tile and
 * cross-bag sum goes through partial slabs added in a fixed order.
 *
 * level_of is uint8[n], indexed by BATCH row (like attn, not by feature row): the level slot of row i.  The rows of a
 * bag may come in any level order; a result is defined by the row order inside each (bag, level).  A value >= levels
 * marks a row of no level: its attention is 0, it contributes to nothing, and neither U nor g is indexed with it.
 *
 * Limits: levels in 1..4; feature_dim a multiple of 4 in 4..2048, attn_dim in 1..256, hidden_dim in 1..256,
 * num_classes in 1..16, 1 <= n_bags <= n <= 2^24 (those of hipac_mil_train_workspace_bytes).  The workspace queries
 * are functions of the dims in `params` (pointers are not read), levels, n and n_bags only, and return 0 for sizes
 * the calls refuse.
 */
#ifndef HIPAC_MIL_LEVELS_H_
#define HIPAC_MIL_LEVELS_H_

#include <stddef.h>
#include <stdint.h>

#include "hipac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_MIL_LEVELS_ABI_VERSION 1
#define HIPAC_MIL_MAX_LEVELS 4

int hipac_mil_levels_abi_version(void);

/* Inference.  feats [n][feature_dim], 16-byte aligned, rows of one bag contiguous; bag b = rows bag_offsets[b] ..
 * bag_offsets[b+1]-1 (int32[n_bags+1], 0 first, n last, strictly increasing -- the caller checks).  Outputs:
 * logits [n_bags][num_classes]; attn [n] softmax weights (0 for a row of no level), may be NULL;
 * pooled [n_bags][levels * feature_dim], may be NULL. */
size_t hipac_mil_levels_forward_workspace_bytes(const hipac_mil_params_t* params, int levels, int n, int n_bags);
int hipac_mil_levels_forward(const hipac_mil_params_t* params, int levels, const float* feats, const uint8_t* level_of,
                             const int32_t* bag_offsets, int n, int n_bags, float* logits, float* attn, float* pooled,
                             void* workspace, size_t workspace_bytes, void* stream);

/* One forward + backward under nn.CrossEntropyLoss(weight = class_w): hipac_mil_heads_train_fwd_bwd's arguments (see
 * include/hipac_mil_train.h: feats stays in place and is read through `rows`, NULL = identity; grads holds the
 * gradient buffers in the shapes above; accumulate != 0 adds to them) with `levels` in place of `heads`, and level_of.
 * Outputs: loss [1], logits [n_bags][num_classes], attn [n] (may be NULL).  With g[k] = dL/dM[k], c[k] = M[k] . g[k]:
 *     ds_i = a_i (x_i . g[lev(i)] - c[lev(i)])      dH_i = ds_i U[lev(i)] (1 - H_i^2)      dV = dH^T X
 *     db_V = sum_i dH_i      dU[k] = sum_{lev(i) = k} ds_i H_i      db_U[k] = sum_{lev(i) = k} ds_i */
size_t hipac_mil_levels_train_workspace_bytes(const hipac_mil_params_t* params, int levels, int n, int n_bags);
int hipac_mil_levels_train_fwd_bwd(const hipac_mil_params_t* params, int levels, const float* feats, int n_feat_rows,
                                   const int32_t* rows, const uint8_t* level_of, const int32_t* bag_offsets, int n,
                                   int n_bags, const int64_t* labels, const float* class_w,
                                   const hipac_mil_params_t* grads, float* loss, float* logits, float* attn,
                                   void* workspace, size_t workspace_bytes, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_MIL_LEVELS_H_ */

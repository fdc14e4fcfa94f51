/*
 * hipac_mil_heads.h -- C ABI of multi-head attention pooling for the MIL head of libhipac_hip.so (gfx950).
 *
 * experiments/experiment_configs.yaml asks for `pooling: attention_heads: 8`: K attention branches over one shared
 * hidden layer (ATTENTION_BRANCHES of Ilse et al.'s ABMIL).  With K = heads, F = feature_dim, A = attn_dim, for one
 * bag x [N][F]:
 *     H = tanh(attn_V(x)) [N][A]      S = attn_U(H) [N][K]      a[:, k] = softmax of S[:, k] over the bag
 *     M[k] = sum_i a[i][k] x[i] [K][F]      pooled = M reshaped to [K F], head-major      logits = classifier(pooled)
 * The parameters are those of hipac_mil_params_t (include/hipac.h) under the same names, with grown shapes:
 *     attn_V_w [attn_dim][feature_dim], attn_V_b [attn_dim]           shared by the heads, unchanged
 *     attn_U_w [heads][attn_dim],       attn_U_b [heads]
 *     fc1_w    [hidden_dim][heads * feature_dim], fc1_b [hidden_dim]
 *     fc2_w    [num_classes][hidden_dim], fc2_b [num_classes]          unchanged
 * heads = 1 is the model of hipac_mil_forward / hipac_mil_train_fwd_bwd with attention pooling.
 *
 * Every sweep over the feature rows serves all heads: the step reads X for X V^T, for the K pooled vectors, for the
 * K row dot products of the softmax backward and for dV = dH^T X -- four times, as the single-head step does.
 * These entry points live in the same shared library as include/hipac.h and include/hipac_mil_train.h but carry
 * their own version number.
 *
 * Conventions: those of include/hipac.h.  Data pointers are DEVICE memory; all work is enqueued asynchronously on
 * `stream` (hipStream_t as void*, NULL = default stream); nothing synchronises the device; the caller owns every
 * buffer, the workspace included; 0 on success, otherwise a hipError_t value or a HIPAC_E* code with the message in
 * hipac_last_error().  float32 throughout.  Bitwise reproducible: no floating-point atomics, every cross-tile and
 * cross-bag sum goes through partial slabs added in a fixed order.
 *
 * Limits: heads in 1..8; feature_dim a multiple of 4 in 4..2048, attn_dim in 1..256, hidden_dim in 1..256,
 * num_classes in 1..16, 1 <= n_bags <= n <= 2^24 (those of hipac_mil_train_workspace_bytes).  The workspace queries
 * are functions of the dims in `params` (pointers are not read), heads, n and n_bags only, and return 0 for sizes
 * the calls refuse.
 */
#ifndef HIPAC_MIL_HEADS_H_
#define HIPAC_MIL_HEADS_H_

#include <stddef.h>
#include <stdint.h>

#include "hipac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_MIL_HEADS_ABI_VERSION 1
#define HIPAC_MIL_MAX_HEADS 8

int hipac_mil_heads_abi_version(void);

/* Inference.  feats [n][feature_dim], 16-byte aligned, rows of one bag contiguous; bag b = rows bag_offsets[b] ..
 * bag_offsets[b+1]-1 (int32[n_bags+1], 0 first, n last, strictly increasing -- the caller checks).  Outputs:
 * logits [n_bags][num_classes]; attn [n][heads] softmax weights, may be NULL; pooled [n_bags][heads * feature_dim],
 * may be NULL. */
size_t hipac_mil_heads_forward_workspace_bytes(const hipac_mil_params_t* params, int heads, int n, int n_bags);
int hipac_mil_heads_forward(const hipac_mil_params_t* params, int heads, const float* feats,
                            const int32_t* bag_offsets, int n, int n_bags, float* logits, float* attn, float* pooled,
                            void* workspace, size_t workspace_bytes, void* stream);

/* One forward + backward under nn.CrossEntropyLoss(weight = class_w): hipac_mil_train_fwd_bwd's arguments (see
 * include/hipac_mil_train.h: feats stays in place and is read through `rows`, NULL = identity; grads holds the
 * gradient buffers in the shapes above; accumulate != 0 adds to them) with `heads` in place of `pooling`.
 * Outputs: loss [1], logits [n_bags][num_classes], attn [n][heads] (may be NULL).  With g[k] = dL/dM[k]:
 *     c[k] = M[k] . g[k]      ds[i][k] = a[i][k] (x_i . g[k] - c[k])      dH_i = (sum_k ds[i][k] U[k]) (1 - H_i^2)
 *     dV = dH^T X      db_V = sum_i dH_i      dU[k] = sum_i ds[i][k] H_i      db_U[k] = sum_i ds[i][k] */
size_t hipac_mil_heads_train_workspace_bytes(const hipac_mil_params_t* params, int heads, int n, int n_bags);
int hipac_mil_heads_train_fwd_bwd(const hipac_mil_params_t* params, int heads, const float* feats, int n_feat_rows,
                                  const int32_t* rows, const int32_t* bag_offsets, int n, int n_bags,
                                  const int64_t* labels, const float* class_w, const hipac_mil_params_t* grads,
                                  float* loss, float* logits, float* attn, void* workspace, size_t workspace_bytes,
                                  int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_MIL_HEADS_H_ */

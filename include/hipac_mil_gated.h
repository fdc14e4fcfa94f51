/*
 * hipac_mil_gated.h -- C ABI of gated attention pooling for the MIL head of libhipac_hip.so (gfx950).
 *
 * The gated attention mechanism of Ilse et al. 2018 (ABMIL, eq. 9; the form CLAM uses): a learned sigmoid gate over the
 * hidden units of the attention.  With K = heads, F = feature_dim, A = attn_dim, for one bag x [N][F]:
 *     T = tanh(attn_V(x)) [N][A]      G = sigmoid(attn_G(x)) [N][A]      S = attn_U(T o G) [N][K]
 *     a[:, k] = softmax of S[:, k] over the bag      M[k] = sum_i a[i][k] x[i] [K][F]
 *     pooled = M reshaped to [K F], head-major       logits = classifier(pooled)
 * The parameters are those of hipac_mil_heads.h (hipac_mil_params_t with the grown shapes: attn_U_w [heads][attn_dim],
 * attn_U_b [heads], fc1_w [hidden_dim][heads * feature_dim]) and the gate's
 *     attn_G_w [attn_dim][feature_dim], attn_G_b [attn_dim]
 * hipac_mil_params_t (include/hipac.h) itself does not change: hipac_mil_gated_params_t below wraps it.
 *
 * X V^T and X G_w^T are formed in one sweep of the feature rows, and so are dV = dT^T X and dG_w = dG^T X: the step reads
 * X four times whatever K is (hidden layer, pooling, row dot products, weight gradients), as the ungated steps do.
 * These entry points live in the same shared library as include/hipac.h and include/hipac_mil_heads.h but carry their
 * own version number.
 *
 * Conventions: those of include/hipac.h.  Data pointers are DEVICE memory; all work is enqueued asynchronously on
 * `stream` (hipStream_t as void*, NULL = default stream); nothing synchronises the device; the caller owns every
 * buffer, the workspace included; 0 on success, otherwise a hipError_t value or a HIPAC_E* code with the message in
 * hipac_last_error().  float32 throughout.  Bitwise reproducible: no floating-point atomics, every cross-tile and
 * cross-bag sum goes through partial slabs added in a fixed order.
 *
 * Limits: heads in 1..8; feature_dim a multiple of 4 in 4..2048, attn_dim in 1..256, hidden_dim in 1..256,
 * num_classes in 1..16, 1 <= n_bags <= n <= 2^24 (those of hipac_mil_heads.h).  The workspace queries are functions of
 * the dims in `params` (pointers are not read), heads, n and n_bags only, and return 0 for sizes the calls refuse.
 */
#ifndef HIPAC_MIL_GATED_H_
#define HIPAC_MIL_GATED_H_

#include <stddef.h>
#include <stdint.h>

#include "hipac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_MIL_GATED_ABI_VERSION 1

/* The parameters of a gated model, or its gradient buffers in the same shapes. */
typedef struct {
  hipac_mil_params_t base;
  const float* attn_G_w;
  const float* attn_G_b;
} hipac_mil_gated_params_t;

int hipac_mil_gated_abi_version(void);

/* Inference.  feats [n][feature_dim], 16-byte aligned, rows of one bag contiguous; bag b = rows bag_offsets[b] ..
 * bag_offsets[b+1]-1 (int32[n_bags+1], 0 first, n last, strictly increasing -- the caller checks).  Outputs:
 * logits [n_bags][num_classes]; attn [n][heads] softmax weights, may be NULL; pooled [n_bags][heads * feature_dim],
 * may be NULL. */
size_t hipac_mil_gated_forward_workspace_bytes(const hipac_mil_gated_params_t* params, int heads, int n, int n_bags);
int hipac_mil_gated_forward(const hipac_mil_gated_params_t* params, int heads, const float* feats,
                            const int32_t* bag_offsets, int n, int n_bags, float* logits, float* attn, float* pooled,
                            void* workspace, size_t workspace_bytes, void* stream);

/* One forward + backward under nn.CrossEntropyLoss(weight = class_w): hipac_mil_heads_train_fwd_bwd's arguments (see
 * include/hipac_mil_heads.h and include/hipac_mil_train.h: feats stays in place and is read through `rows`, NULL =
 * identity; grads holds the gradient buffers in the shapes above; accumulate != 0 adds to them).
 * Outputs: loss [1], logits [n_bags][num_classes], attn [n][heads] (may be NULL).  With g[k] = dL/dM[k], and c and ds as in
 * include/hipac_mil_heads.h:
 *     c[k] = M[k] . g[k]      ds[i][k] = a[i][k] (x_i . g[k] - c[k])      e_i = sum_k ds[i][k] U[k]
 *     dT_i = e_i o G_i o (1 - T_i^2)            dG_i = e_i o T_i o G_i o (1 - G_i)
 *     dV = dT^T X      db_V = sum_i dT_i        dG_w = dG^T X      db_G = sum_i dG_i
 *     dU[k] = sum_i ds[i][k] (T_i o G_i)        db_U[k] = sum_i ds[i][k] */
size_t hipac_mil_gated_train_workspace_bytes(const hipac_mil_gated_params_t* params, int heads, int n, int n_bags);
int hipac_mil_gated_train_fwd_bwd(const hipac_mil_gated_params_t* params, int heads, const float* feats, int n_feat_rows,
                                  const int32_t* rows, const int32_t* bag_offsets, int n, int n_bags,
                                  const int64_t* labels, const float* class_w, const hipac_mil_gated_params_t* grads,
                                  float* loss, float* logits, float* attn, void* workspace, size_t workspace_bytes,
                                  int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_MIL_GATED_H_ */

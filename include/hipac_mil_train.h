/*
 * hipac_mil_train.h -- C ABI of the MIL training step of libhipac_hip.so (gfx950).
 *
 * One forward + backward of the reference's MILClassifier (src/models/mil_classifier.py:5-45) over a batch
 * of ragged bags, under nn.CrossEntropyLoss(weight = class_w): the loss, the logits and the gradient of every
 * parameter.  The loop it serves is the one experiments/experiment_configs.yaml describes (Adam, lr 1e-3,
 * weight decay 1e-4, 32 bags per step).  These entry points live in the same shared library as include/hipac.h
 * but carry their own version number, so adding them leaves hipac.h's ABI untouched.
 *
 * Conventions: those of include/hipac.h.  Plain pointers and sizes; data pointers are DEVICE memory; all work
 * is enqueued asynchronously on `stream` (hipStream_t as void*, NULL = default stream); nothing synchronises
 * the device; the caller owns every buffer; 0 on success, otherwise a hipError_t value or a HIPAC_E* code,
 * with the message in the thread-local last-error string of hipac.h.  float32 throughout.
 */
#ifndef HIPAC_MIL_TRAIN_H_
#define HIPAC_MIL_TRAIN_H_

#include <stddef.h>
#include <stdint.h>

#include "hipac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_MIL_TRAIN_ABI_VERSION 1

int hipac_mil_train_abi_version(void);

/* Bytes of workspace hipac_mil_train_fwd_bwd needs for n rows in n_bags bags; a function of the dims in
 * `params` (pointers are not read), the pooling, n and n_bags only.  0 for sizes it refuses: n <= 0,
 * n_bags <= 0, n_bags > n, n > 2^24, feature_dim not a multiple of 4 in 4..2048, hidden_dim outside 1..256,
 * num_classes outside 1..16, a bad pooling, and for attention pooling attn_dim outside 1..256. */
size_t hipac_mil_train_workspace_bytes(const hipac_mil_params_t* params, int pooling, int n, int n_bags);

/* feats [n_feat_rows][feature_dim], 16-byte aligned, stays where it is: row i of the batch is
 * feats[rows[i]] (rows int32[n], every value in [0, n_feat_rows) -- the caller checks; NULL = identity, then
 * n <= n_feat_rows).  Bag b = batch rows bag_offsets[b] .. bag_offsets[b+1]-1 (int32[n_bags+1], 0 first,
 * n last, strictly increasing -- the caller checks).  labels int64[n_bags]; class_w [num_classes] or NULL.
 * grads: a hipac_mil_params_t whose pointers are the gradient buffers (same shapes as the parameters;
 * written through, the `const` of the type notwithstanding; the attn_* ones are needed for attention pooling
 * only); accumulate != 0 adds to them instead of overwriting.  Outputs: loss [1] (the weighted mean, as
 * torch), logits [n_bags][num_classes], attn [n] softmax weights (attention only, may be NULL).
 * Bitwise reproducible: every cross-tile sum goes through per-tile partial slabs added in a fixed order. */
int hipac_mil_train_fwd_bwd(const hipac_mil_params_t* params, int pooling, const float* feats, int n_feat_rows,
                            const int32_t* rows, const int32_t* bag_offsets, int n, int n_bags,
                            const int64_t* labels, const float* class_w, const hipac_mil_params_t* grads,
                            float* loss, float* logits, float* attn, void* workspace, size_t workspace_bytes,
                            int accumulate, void* stream);

/* torch.optim.Adam's weight decay (L2 form): grads[i] += wd * params[i], before hipac_adam_step. */
int hipac_mil_train_l2_add(float* grads, const float* params, int64_t n, float wd, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_MIL_TRAIN_H_ */

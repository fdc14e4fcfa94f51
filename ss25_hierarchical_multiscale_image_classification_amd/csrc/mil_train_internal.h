// mil_train.hip's step for the other translation units of the library (mil_dropout.hip).
#pragma once
#include "common.h"

namespace hipac {

// Called on a [n_bags][hidden] buffer of the classifier between two of the step's launches; returns 0 or an error code.
typedef int (*MilHiddenHook)(float* buf, int n_bags, int hidden, void* ctx, hipStream_t s);

// hipac_mil_train_fwd_bwd (include/hipac_mil_train.h) with a hook: called on hid after classifier.0 + ReLU (before
// classifier.2 reads it) and on dhid after classifier.2's backward (before classifier.0's backward reads it).
// hook = nullptr is hipac_mil_train_fwd_bwd itself.
int mil_train_run(const hipac_mil_params_t* p, int pooling, const float* feats, int n_feat_rows, const int32_t* rows,
                  const int32_t* bag_offsets, int n, int n_bags, const int64_t* labels, const float* class_w,
                  const hipac_mil_params_t* grads, float* loss, float* logits, float* attn, void* workspace, size_t workspace_bytes,
                  int accumulate, void* stream, MilHiddenHook hook, void* hook_ctx);

}  // namespace hipac

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

// The pieces of the step that do not depend on the number of attention heads, launched as mil_train_run launches them
// (mil_heads.hip).  Rows are tiled 64 at a time; segment (tile t, bag b) has the id t + b.
bool mil_train_sizes_ok(const hipac_mil_params_t* p, int n, int n_bags);  // the limits of hipac_mil_train_workspace_bytes, attention
void mil_train_dv_slices(int n, int F, int* chunk, int* slices);         // the row slices of the dV product
// bag_of[i] = the bag of batch row i
void mil_train_launch_bag_of(const int32_t* offs, int n_bags, int n, int32_t* bag_of, hipStream_t s);
// H[n][A_pad] = tanh(X V^T + b_V), columns A .. A_pad - 1 zero; A_pad = A rounded up to 32
void mil_train_launch_h(const float* feats, const int32_t* rows, int n, int F, const float* Vw, const float* Vb, int A, int A_pad,
                        float* H, hipStream_t s);
// pooled[b][F] = the segments part[t + b][F] of bag b added in a fixed order
void mil_train_launch_pool_combine(const float* part, const int32_t* offs, int n_bags, int F, float* pooled, hipStream_t s);
// cdot[b] = pooled[b] . g[b], b < B
void mil_train_launch_cdot(const float* pooled, const float* g, int F, int B, float* cdot, hipStream_t s);
// dst[e] (+)= sum over k < slices of part[k * per_slice + off + e], e < count, in a fixed order
void mil_train_launch_slab_reduce(const float* part, int slices, size_t per_slice, size_t off, long long count, float* dst,
                                  int accumulate, hipStream_t s);
// slab[slice][A][F] = dH^T X over the slice's rows
void mil_train_launch_dv(const float* dH, const float* feats, const int32_t* rows, int n, int F, int A, int A_pad, int chunk,
                         int slices, float* slab, hipStream_t s);
// mil_heads.hip's pooling partials for mil_gated.hip: tile t of 64 rows -> part[t + b][K][F] for every bag b it holds, from the
// attention a [n][K]; K in 1..8, ntiles = ceil(n / 64)
void mil_heads_launch_pool(const float* feats, const int32_t* rows, const int32_t* bag_of, const float* a, int n, int F, int K,
                           int ntiles, float* part, hipStream_t s);

}  // namespace hipac

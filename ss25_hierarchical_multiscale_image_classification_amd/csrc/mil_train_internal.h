// What the translation units of the MIL head share on the host, defined in mil_train.hip: the single-head step with a hook
// (mil_dropout.hip), and for the K-head steps (mil_heads.hip, mil_gated.hip, mil_levels.hip) the workspace plan, the argument
// checks, the classifier chain, the K dispatch and the launches that do not depend on K.  Device helpers: mil_device.h.
#pragma once
#include <type_traits>

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

// fn(std::integral_constant<int, K>{}) with K = k, for k in 1..MAX (a k above MAX takes MAX; the entry points refuse it first)
template <int MAX, class Fn>
inline void mil_for_count(int k, Fn&& fn) {
  if constexpr (MAX > 1) {
    if (k < MAX) return mil_for_count<MAX - 1>(k, fn);
  }
  fn(std::integral_constant<int, MAX>{});
}

// Byte offsets into the workspace of a step (or, train = false, of an inference forward) with K attention branches over
// `planes` hidden planes of [n][A_pad] floats (H; T and G with the gate).  The single-head step lays out the same buffers
// in an order of its own (mil_train.hip).
struct MilHeadPlan {
  int A_pad, ntiles, nseg, chunk, slices;
  size_t P2;  // floats of one tile's column sums: planes x [A_pad] | sum ds[i][k] H_i [K][A] | sum ds[i][k] [K]
  size_t bag_of, pooled, hid, dhid, dym, dlogits, g, ce, cdot, part, scores, attn, H, G, part2, slab, total;
};
// attn_cols: the width of scores / attn, K (a softmax per head) or 1 (mil_levels.hip: a row has one level).
// slab holds `planes` products [A][F] per row slice
MilHeadPlan make_mil_head_plan(const hipac_mil_params_t* p, int K, int n, int n_bags, int planes, int attn_cols, bool train);

// The checks of an entry point in front of its workspace check, in one order for every entry point; 0, or the error code
// after set_error("<who>: ...").  ptrs: the entry point's own pointer arguments are all there.  count_name ("heads",
// "levels"): count must be in 1..max_count; nullptr: no such argument.  attention: the attention weights (and, train, their
// gradient buffers) must be there (false: mean / max pooling).  gate: the variant's further attention tensors are there.
int mil_check_forward_args(const char* who, bool ptrs, const char* count_name, int count, int max_count, const hipac_mil_params_t* p,
                           bool gate, int n, int n_bags, const void* feats, const void* workspace);
int mil_check_train_args(const char* who, bool ptrs, const char* count_name, int count, int max_count, const hipac_mil_params_t* p,
                         const hipac_mil_params_t* grads, bool attention, bool gate, int n, int n_bags, int n_feat_rows, bool has_rows,
                         const void* feats, const void* workspace);

// classifier.0 over `cols` pooled columns + ReLU, classifier.2: hipac.h's entry points as they are
int mil_classifier_forward(const hipac_mil_params_t* p, const float* pooled, int cols, int B, float* hid, float* logits, void* stream);
// The same on the plan's pooled buffer, then the cross-entropy and the backward of both layers; want_g: dL/dpooled goes to
// the plan's g.  hook (may be nullptr): as in mil_train_run
int mil_classifier_fwd_bwd(const hipac_mil_params_t* p, const hipac_mil_params_t* grads, int cols, int B, const int64_t* labels,
                           const float* class_w, float* loss, float* logits, const MilHeadPlan& q, char* ws, bool want_g, int accumulate,
                           void* stream, MilHiddenHook hook, void* hook_ctx);

// The pieces of the step that do not depend on the number of attention heads, launched as mil_train_run launches them.
// Rows are tiled 64 at a time; segment (tile t, bag b) has the id t + b.
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
// The end of an ungated K-branch step: db_V | dU | db_U from the plan's part2, dV = dH^T X through the plan's slab
void mil_head_launch_grads(const hipac_mil_params_t* grads, int K, const float* feats, const int32_t* rows, int n, int F, int A,
                           const MilHeadPlan& q, char* ws, int accumulate, hipStream_t s);
// mil_heads.hip's pooling partials for mil_gated.hip: tile t of 64 rows -> part[t + b][K][F] for every bag b it holds, from the
// attention a [n][K]; K in 1..8, ntiles = ceil(n / 64)
void mil_heads_launch_pool(const float* feats, const int32_t* rows, const int32_t* bag_of, const float* a, int n, int F, int K,
                           int ntiles, float* part, hipStream_t s);

}  // namespace hipac

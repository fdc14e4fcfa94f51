/*
 * hipac_mil_dropout.h -- C ABI of dropout and Monte-Carlo dropout for the MIL head of libhipac_hip.so (gfx950).
 *
 * experiments/experiment_configs.yaml asks for dropout_rate 0.5 and uncertainty_estimation {monte_carlo_dropout,
 * num_samples 100}; src/utils/uncertainty.py's monte_carlo_dropout returns the mean and the torch.var of the
 * softmax outputs of num_samples stochastic forwards.  These entry points live in the same shared library as
 * include/hipac.h and include/hipac_mil_train.h but carry their own version number.
 *
 * The mask.  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85):
 *   key     = (low word, high word) of the 64-bit seed
 *   counter = (column / 4, row, sample, site); output word column % 4 belongs to the column
 *   site 0  = the feature rows: row = the row's position in the call (batch row i), column in [0, feature_dim)
 *   site 1  = the classifier's hidden activation after the ReLU: row = the bag index, column in [0, hidden_dim)
 *   sample  = the Monte-Carlo sample index (prediction) or the trainer's step number (training)
 *   an element is kept iff its word >= thr, thr = (uint32) floor(p * 2^32) in double, 0 <= p < 1;
 *   a kept element becomes fl32(x * scale), scale = (float)(1.0 / (1.0 - p)); a dropped one becomes 0.
 * The attention branch and the pooling see the same masked rows; mean and max pooling pool the masked rows.
 *
 * Conventions: those of include/hipac.h.  Data pointers are DEVICE memory; all work is enqueued asynchronously
 * on `stream`; nothing synchronises the device; the caller owns every buffer; 0 on success, otherwise a
 * hipError_t value or a HIPAC_E* code with the message in hipac_last_error().
 */
#ifndef HIPAC_MIL_DROPOUT_H_
#define HIPAC_MIL_DROPOUT_H_

#include <stddef.h>
#include <stdint.h>

#include "hipac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_MIL_DROPOUT_ABI_VERSION 1

int hipac_mil_dropout_abi_version(void);

/* The mask itself, for tests and debugging: keep[r][c] = 1 if element (row r, column c) of (sample, site) is
 * kept, else 0; uint8[n_rows][n_cols].  n_rows, n_cols >= 1, n_rows * n_cols < 2^31. */
int hipac_mil_dropout_mask(double p, uint64_t seed, uint32_t sample, uint32_t site, int n_rows, int n_cols,
                           uint8_t* keep, void* stream);

/* hipac_mil_train_fwd_bwd (include/hipac_mil_train.h; same arguments, same limits) under dropout p with the
 * masks of sample = step: the batch rows are gathered through `rows`, masked and scaled into the workspace, the
 * step runs on that copy, and the hidden mask (site 1) is applied to the hidden activation and to its gradient.
 * p == 0 is hipac_mil_train_fwd_bwd itself, bit for bit.  The workspace is that of
 * hipac_mil_train_workspace_bytes plus n * feature_dim * 4 bytes for the masked copy: with whole bags (no
 * --mil_bag_size) a step of 32 slides of 40 000 patches needs 2.6 GB for it. */
size_t hipac_mil_dropout_train_workspace_bytes(const hipac_mil_params_t* params, int pooling, int n, int n_bags);
int hipac_mil_dropout_train_fwd_bwd(const hipac_mil_params_t* params, int pooling, const float* feats,
                                    int n_feat_rows, const int32_t* rows, const int32_t* bag_offsets, int n,
                                    int n_bags, const int64_t* labels, const float* class_w,
                                    const hipac_mil_params_t* grads, float* loss, float* logits, float* attn,
                                    void* workspace, size_t workspace_bytes, int accumulate, double p,
                                    uint64_t seed, uint32_t step, void* stream);

/* Monte-Carlo dropout: n_samples stochastic forwards (samples first_sample .. first_sample + n_samples - 1) of
 * every bag, and their statistics.  feats [n][feature_dim] with the rows of a bag contiguous (row i is mask row
 * i), bag_offsets int32[n_bags + 1] as for hipac_mil_train_fwd_bwd.  Limits: those of
 * hipac_mil_train_workspace_bytes, 0 <= p < 1 and 1 <= n_samples <= 4096; the workspace query returns 0 for a
 * size it refuses.  Outputs:
 *   logits           float [n_samples][n_bags][num_classes], may be NULL
 *   mean_prob        double[n_bags][num_classes]  mean over the samples of probs_t = softmax(logits_t)
 *   var_prob         double[n_bags][num_classes]  variance with divisor n_samples - 1 (torch.var); 0 for one sample
 *   entropy          double[n_bags]  -sum_c m_c ln m_c of mean_prob
 *   expected_entropy double[n_bags]  mean over the samples of the entropy of probs_t
 *   mutual_info      double[n_bags]  max(entropy - expected_entropy, 0)
 *   attn_mean        float [n] mean over the samples of the softmax weights (attention pooling only), may be NULL
 * The statistics are IEEE double, one operation at a time, the samples added in order.  Bitwise reproducible:
 * no floating-point atomics, every cross-tile sum goes through partial slabs added in a fixed order. */
size_t hipac_mil_mc_workspace_bytes(const hipac_mil_params_t* params, int pooling, int n, int n_bags, int n_samples);
int hipac_mil_mc_forward(const hipac_mil_params_t* params, int pooling, const float* feats,
                         const int32_t* bag_offsets, int n, int n_bags, double p, uint64_t seed,
                         uint32_t first_sample, int n_samples, float* logits, double* mean_prob, double* var_prob,
                         double* entropy, double* expected_entropy, double* mutual_info, float* attn_mean,
                         void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_MIL_DROPOUT_H_ */

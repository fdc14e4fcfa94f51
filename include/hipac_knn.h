/*
 * hipac_knn.h -- C ABI of the weighted k-nearest-neighbour probe (--validate --validate_knn K) of libhipac_hip.so
 * (gfx950): the classifier of Wu et al. 2018 ("Unsupervised feature learning via non-parametric instance
 * discrimination") that SimCLR, MoCo and DINO report next to the linear probe.
 *
 *     hipac_knn_inv_norms   out[i] = 1 / max(|x_i|, 1e-12)                                    (the cosine scales)
 *     hipac_knn_topk        for every query row the K bank rows of largest similarity          v_mfma_f32_32x32x2_f32
 *     hipac_knn_vote        scores[i][c] = class_w[c] sum_{t: label_t = c} exp((s_t - s_0) / T) and the prediction
 *
 * The similarity matrix [n_q][n_b] is never written: the selection runs behind the MFMAs and keeps K numbers per query.
 *
 * Rows: x_i is row rows[i] of the feature matrix X [n_feat_rows][F], which stays in place: an index list is int32[n]
 * (NULL = identity, repeats allowed; the caller checks 0 <= rows[i] < n_feat_rows, and n <= n_feat_rows when the list is
 * NULL).  Everything else a call reads or writes per row (scales, outputs, bank_labels) is indexed by the POSITION in
 * the list, not by the row number.
 *
 * Conventions: those of include/hipac.h and include/hipac_validate.h.  Data pointers are DEVICE memory, X and the
 * workspace 16-byte aligned; all work is enqueued asynchronously on `stream` (hipStream_t as void*, NULL = default
 * stream); nothing synchronises the device; the caller owns every buffer, the workspace included; 0 on success,
 * otherwise a hipError_t value or HIPAC_EINVAL (sizes, null pointers, alignment, a short workspace) with the message in
 * hipac_last_error().  Bitwise reproducible: no floating-point atomics, no sum across workgroups.
 *
 * Limits: F a multiple of 4 in 4..2048, 1 <= n_q <= 2^24, 1 <= K <= 256, K <= n_b <= 2^24 (a bank of fewer than K rows is
 * refused, not padded).  The queries are functions of their arguments only and return 0 for sizes the calls refuse.
 */
#ifndef HIPAC_KNN_H_
#define HIPAC_KNN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_KNN_ABI_VERSION 1
#define HIPAC_KNN_MAX_K 256

int hipac_knn_abi_version(void);

/* out[i] = 1 / max(sqrt(sum_f x_i[f]^2), 1e-12f), float32, i = 0..n-1.  The sum has a fixed order (lane l of a wave adds
 * the float4 columns l, l + 64, .. in turn, then a 64-lane butterfly), so out[i] depends on the row alone.  A zero row
 * gets 1e12: its similarity to everything is 0. */
int hipac_knn_inv_norms(const float* X, int n_feat_rows, const int32_t* rows, int n, int F, float* out, void* stream);

/* How many column groups the bank is cut into so that few queries still fill the device; 0 for refused sizes.  A group
 * is a run of consecutive bank positions, a multiple of 128 long (the last may be shorter). */
int hipac_knn_bank_splits(int n_q, int n_b, int F, int K);
size_t hipac_knn_topk_workspace_bytes(int n_q, int n_b, int F, int K);

/* sim(i, j) = fl32(fl32(d_ij * q_scale[i]) * b_scale[j]), d_ij the float32 dot product of query row i (q_rows) and bank
 * row j (b_rows) on v_mfma_f32_32x32x2_f32.  A NULL scale means 1 and no multiplication.  d_ij is a function of the two
 * rows and F alone: one accumulator chain over the whole of F in a fixed feature order, the same bits wherever the rows
 * sit in their lists, whatever n_q, n_b and K are and however the bank is split.
 *
 * sim_out float[n_q][K], idx_out int32[n_q][K]: for every query the K bank POSITIONS (0..n_b-1, not row numbers) of
 * largest similarity, in descending similarity.  The order is total:
 *   1. a larger similarity comes first (-0 and +0 are equal; -0 is returned as +0);
 *   2. equal similarities go to the lower position;
 *   3. a NaN similarity ranks below -inf, NaNs among themselves again by position: a NaN is returned only when fewer
 *      than K other rows exist.
 * Every group keeps its own K-list per query; a second kernel merges the groups by the same order, so the result does
 * not depend on the split. */
int hipac_knn_topk(const float* X, int n_feat_rows, int F, const int32_t* q_rows, int n_q, const float* q_scale,
                   const int32_t* b_rows, int n_b, const float* b_scale, int K, float* sim_out, int32_t* idx_out,
                   void* workspace, size_t workspace_bytes, void* stream);

/* The weighted vote over the lists of hipac_knn_topk.  bank_labels int32[n_b] (0 or 1, by bank position; the caller
 * checks), class_w double[2], scores double[n_q][2], pred int32[n_q].  IEEE double, one rounding per operation.  For the
 * neighbours t = 0..K-1 in list order
 *     w_t = exp(((double)sim_t - (double)sim_0) * inv_T)            (<= 1: nothing overflows)
 *     scores[i][c] = class_w[c] * sum_{t: label_t = c} w_t          (added in list order)
 *     pred[i] = scores[i][1] > scores[i][0]                         (a tie goes to class 0)
 * A row whose top similarity is NaN gets NaN scores and pred 0. */
int hipac_knn_vote(const float* sim, const int32_t* idx, const int32_t* bank_labels, int n_q, int K, double inv_T,
                   const double* class_w, double* scores, int32_t* pred, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_KNN_H_ */

/*
 * hipac_validate.h -- C ABI of the feature sanity check (--validate) of libhipac_hip.so (gfx950): the device side of a
 * two-component PCA and of a class-weighted logistic-regression probe fitted with Newton's method.
 *
 * The reference's validate_resnet_classifier (src/main.py:1017-1070) takes the matrix --extract_features wrote to
 * scikit-learn.  Both numbers it reports are defined without an algorithm (the leading eigenpairs of a covariance
 * matrix, the minimiser of a strictly convex objective), so what runs here are the sweeps over the [N][F] matrix; the
 * F x F eigen-decomposition and the (F + 1) x (F + 1) Newton solve stay on the host (validate.py).
 *
 *     hipac_validate_colsum           out[f]  = sum_i w_i x_i[f]                                    (the mean)
 *     hipac_validate_gram             G[a][b] = sum_i w_i (x_i[a] - c[a]) (x_i[b] - c[b])           (covariance, Hessian)
 *     hipac_validate_logistic_sweep   margins, loss, gradient sums and curvature of the probe in one read of X
 *     hipac_validate_project          Z[i][k] = (x_i - c) . W[k], per-class sums of Z and class counts
 *
 * x_i is row rows[i] of the feature matrix X [n_feat_rows][F], which stays in place: `rows` is int32[n] (NULL =
 * identity, repeats allowed; the caller checks 0 <= rows[i] < n_feat_rows, and n <= n_feat_rows when rows is NULL).
 * Per-row inputs and outputs that are not X (w, d, margins, Z) are indexed by i; `labels` (int64, 0 or 1 -- the caller
 * checks) belongs to the matrix and is read as labels[rows[i]].
 *
 * Conventions: those of include/hipac.h.  Data pointers are DEVICE memory, 16-byte aligned where they hold F-vectors
 * or the matrix; all work is enqueued asynchronously on `stream` (hipStream_t as void*, NULL = default stream); nothing
 * synchronises the device; the caller owns every buffer, the workspace included; 0 on success, otherwise a hipError_t
 * value or a HIPAC_E* code with the message in hipac_last_error().  float32 throughout.  Bitwise reproducible: no
 * floating-point atomics, every sum that crosses a workgroup goes through partial slabs added in a fixed order.
 *
 * Limits: F a multiple of 4 in 4..2048, 1 <= n <= 2^24, 1 <= K <= 4.  The workspace queries are functions of their
 * arguments only and return 0 for sizes the calls refuse.
 */
#ifndef HIPAC_VALIDATE_H_
#define HIPAC_VALIDATE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_VALIDATE_ABI_VERSION 1
#define HIPAC_VALIDATE_MAX_COMPONENTS 4

int hipac_validate_abi_version(void);

/* out[F] = sum_i w[i] x_i; w float[n], NULL = 1. */
size_t hipac_validate_colsum_workspace_bytes(int n, int F);
int hipac_validate_colsum(const float* X, int n_feat_rows, const int32_t* rows, int n, int F, const float* w, float* out,
                          void* workspace, size_t workspace_bytes, void* stream);

/* G[F][F] = sum_i w[i] (x_i - c) (x_i - c)^T on v_mfma_f32_32x32x2_f32; w float[n], NULL = 1; c float[F], NULL = 0.  The
 * centre is subtracted as the rows are staged.  Only elements on or above the diagonal are computed, each is written to
 * both places: G == G^T bit for bit.  The rows are split over hipac_validate_gram_slices(n, F) slices of a multiple of
 * 128 rows (the last one may be shorter); one slice's partial G is F * F floats of the workspace. */
int hipac_validate_gram_slices(int n, int F); /* 0 for sizes the call refuses */
size_t hipac_validate_gram_workspace_bytes(int n, int F);
int hipac_validate_gram(const float* X, int n_feat_rows, const int32_t* rows, int n, int F, const float* w, const float* c,
                        float* G, void* workspace, size_t workspace_bytes, void* stream);

/* One sweep of the probe.  coef float[F], intercept float[1], class_w float[2] (s of label 0, of label 1).  With
 * m_i = x_i . coef + intercept, y_i = labels[rows[i]], s_i = class_w[y_i], p_i = 1 / (1 + exp(-m_i)):
 *     r_i = s_i (p_i - y_i)      d_i = s_i p_i (1 - p_i)      l_i = s_i (log(1 + exp(m_i)) - y_i m_i)
 * (formed from exp(-|m_i|): finite for every finite m_i).  Outputs:
 *     sums float[2 F + 3] = sum r_i x_i [F] | sum d_i x_i [F] | sum r_i | sum d_i | sum l_i
 *     d float[n] (the weights of the Hessian's hipac_validate_gram call); margins float[n], may be NULL. */
size_t hipac_validate_logistic_workspace_bytes(int n, int F);
int hipac_validate_logistic_sweep(const float* X, int n_feat_rows, const int32_t* rows, int n, int F, const float* coef,
                                  const float* intercept, const int64_t* labels, const float* class_w, float* sums, float* d,
                                  float* margins, void* workspace, size_t workspace_bytes, void* stream);

/* Z[n][K] = (x_i - c) . W[k]; c float[F], NULL = 0; W float[K][F].  labels may be NULL; otherwise class_sums float[2][K]
 * = the sums of Z over the rows of label 0 and of label 1, class_counts float[2] = how many rows each has (exact:
 * n <= 2^24), both required. */
size_t hipac_validate_project_workspace_bytes(int n, int F, int K);
int hipac_validate_project(const float* X, int n_feat_rows, const int32_t* rows, int n, int F, const float* c, const float* W,
                           int K, const int64_t* labels, float* Z, float* class_sums, float* class_counts, void* workspace,
                           size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_VALIDATE_H_ */

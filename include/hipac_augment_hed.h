/*
 * hipac_augment_hed.h -- C ABI of the HED stain augmentation of libhipac_hip.so (gfx950): the opt-in stage of `--aug_hed SIGMA`
 * in the device input pipelines of the training loops (augment.DeviceSimCLRLoader, augment.DeviceClassifierLoader).  Every
 * training view gets an affine map of its own in optical-density space that scales and shifts the concentrations of haematoxylin,
 * eosin and DAB (Tellez et al. 2018 / 2019 on the Ruifrok-Johnston basis).  The reference has no such stage; this is the project's
 * addition and is off by default.
 *
 * These entry points live in the same shared library as include/hipac.h but carry their own version number, so adding them
 * leaves hipac.h's ABI untouched.
 *
 * Conventions: those of include/hipac.h.  Plain pointers and sizes; every data pointer is DEVICE memory unless its comment says
 * HOST; all work is enqueued asynchronously on `stream` (hipStream_t as void*, NULL = default stream); nothing synchronises the
 * device; the caller owns every buffer; 0 on success, otherwise a hipError_t value or a HIPAC_E* code, with the message in the
 * thread-local last-error string of hipac.h.  Every argument check answers before the first launch.
 *
 * Definition.  tests/augment_hed_cpu.py is the numpy restatement of every formula below; the device equals it bit for bit.
 *
 *   Stain basis.  R = rows H, E, D = [[0.65, 0.70, 0.29], [0.07, 0.99, 0.11], [0.27, 0.57, 0.78]] (Ruifrok and Johnston 2001);
 *   Rinv = its inverse, a literal table of doubles (augment_hed.HED_FROM_RGB).
 *
 *   The view's map, made on the HOST in IEEE double, one rounding per operation, in this order (alpha[3] scales and beta[3] shifts
 *   the concentrations of H, E, D):
 *       T[i][j] = Rinv[i][j] alpha[j]
 *       A[c][k] = (T[k][0] R[0][c] + T[k][1] R[1][c]) + T[k][2] R[2][c]          (od' = od Rinv diag(alpha) R, column form)
 *       bq[c]   = 4096.0 ((beta[0] R[0][c] + beta[1] R[1][c]) + beta[2] R[2][c])  (the shift in the table's units of 2^-12)
 *   One view's payload is double[HIPAC_AUGMENT_HED_PAYLOAD] = A row-major, then bq.  The identity payload is A = I, bq = 0; views
 *   that are not to be augmented carry it.
 *
 *   Per pixel.  o_k = (double) od[v_k] with the optical-density table of include/hipac_stain.h (od[v] = rint(2^12 ln(256 / (v + 1))),
 *   od[0] = HIPAC_STAIN_OD_MAX = 22713):
 *       t_c  = rint(((A[c][0] o_0 + A[c][1] o_1) + A[c][2] o_2) + bq[c]), clamped to [0, 22713]
 *       v'_c = inv[t_c], inv[q] = the v whose od[v] is nearest to q, ties to the larger v       (hipac_stain_apply's rule)
 *   IEEE double, one rounding per operation (the library is compiled without floating-point contraction).  The table is strictly
 *   decreasing and inv[od[v]] = v for all 256 values, so the identity payload leaves every byte unchanged.  (A sum that is not a
 *   number, which only payload entries beyond 1e300 can produce, counts as 0.)
 *
 *   Position.  The stage acts on the whole 224 x 224 view AFTER the geometric stage (crop + resize + flip, or flips + rotation)
 *   and BEFORE the ColorJitter operations and the grayscale step.  That includes the black corners a rotation fills in: they are
 *   pixels of the view like any other (black has the largest optical density, so a map may lighten them).
 */
#ifndef HIPAC_AUGMENT_HED_H_
#define HIPAC_AUGMENT_HED_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_AUGMENT_HED_ABI_VERSION 1

#define HIPAC_AUGMENT_HED_PAYLOAD 12  /* doubles per view: A[3][3] row-major, then bq[3] */

int hipac_augment_hed_abi_version(void);

/* hipac_augment_views (include/hipac.h; the same arguments, the same checks) with the stage between the geometric stage and the
 * colour operations.  hed_host: HOST double[n_views][12], read by an asynchronous copy on `stream`: keep it unchanged until that
 * copy has run (pinned memory, or the host waits).  hed_dev: double[n_views][12] scratch.  Every payload entry must be finite.
 * hed_host == NULL (hed_dev is then not read) is hipac_augment_views itself, bit for bit.  The stage is part of the colour
 * kernel's load of the view into LDS: this route makes no pass over HBM that hipac_augment_views does not make. */
int hipac_augment_views_hed(const uint8_t* pool, int64_t n_pool, int P, int geometry, const int32_t* params_host, int32_t* params_dev,
                            int n_views, const int32_t* tab_bounds, const int32_t* tab_kk, int ksize, const float* lut, uint8_t* tmp,
                            uint8_t* crops, float* out, uint8_t* out_u8, const double* hed_host, double* hed_dev, void* stream);

/* The stage alone, in place on images: uint8[n_views][224][224][3] (4-byte aligned), view i under payload i.  hed_host and hed_dev
 * as above, 1 <= n_views <= 65535. */
int hipac_augment_hed_apply(uint8_t* images, int n_views, const double* hed_host, double* hed_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_AUGMENT_HED_H_ */

/*
 * hipac_tta.h -- C ABI of the test-time augmentation of the detector in libhipac_hip.so (gfx950): the eight views of a
 * square patch (the dihedral group: four rotations by 90 degrees, each with and without a mirror), made on the device
 * from the uint8 patch buffer the slide scan fills, and the reduction of the per-view logits to one tumour probability
 * per window (`--detect_tta`, tta.py).
 *
 * These entry points live in the same shared library as include/hipac.h but carry their own version number, so
 * adding them leaves hipac.h's and hipac_detect.h's ABI untouched.
 *
 * Conventions: those of include/hipac_detect.h.  Data pointers are DEVICE memory; all work is enqueued asynchronously
 * on `stream` (hipStream_t as void*, NULL = default stream); nothing synchronises the device; the caller owns every
 * buffer; 0 on success, otherwise a hipError_t value or a HIPAC_E* code, with the message in the thread-local
 * last-error string of hipac.h.  Every argument check answers before the first launch.
 *
 * Reproducibility: the view is a permutation of bytes.  The reduction uses no floating-point atomics, adds in a fixed
 * order, and the library is compiled without floating-point contraction, so its outputs are bitwise identical from
 * run to run and equal to a float32 restatement fed the same per-view probabilities (tests/tta_cpu.py).
 */
#ifndef HIPAC_TTA_H_
#define HIPAC_TTA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_TTA_ABI_VERSION 1

#define HIPAC_TTA_SIDE 224 /* the trunk takes nothing else */
#define HIPAC_TTA_VIEWS 8

int hipac_tta_abi_version(void);

/* View `view` of n patches.  in, out: uint8[n][224][224][3] (rows, columns, RGB), 4-byte aligned, byte ranges that do
 * not intersect.  view = r + 4 f, f in {0, 1}, r in {0 .. 3}: mirror the columns first if f, then rotate r quarter
 * turns counter-clockwise -- numpy's rot90(x[:, :, ::-1] if f else x, r, axes=(1, 2)).  With S = 224 and
 * z[a][b] = x[a][S - 1 - b] if f, else x[a][b]:
 *     r = 0   out[i][j] = z[i][j]
 *     r = 1   out[i][j] = z[j][S - 1 - i]
 *     r = 2   out[i][j] = z[S - 1 - i][S - 1 - j]
 *     r = 3   out[i][j] = z[S - 1 - j][i]
 * The inverse of view v is view {0, 3, 2, 1, 4, 5, 6, 7}[v].  View 0 is a copy.  n >= 0 (n = 0 succeeds without a
 * launch); every offset is 64-bit (n * 150 528 passes 2^31 at n = 14 267).
 * Refused with HIPAC_EINVAL: a null or misaligned pointer, n < 0 or n >= 2^28, view outside 0 .. 7, ranges that
 * intersect. */
int hipac_tta_view(const uint8_t* in, int n, int view, uint8_t* out, void* stream);

/* Mean tumour probability over the views of every window, and how far the views disagree.
 * logits: float32[views][n][2], 1 <= views <= HIPAC_TTA_VIEWS; tumor_class 0 or 1; n >= 0.  With
 *     p_v[i] = 1 / (1 + exp(logits[v][i][1 - tumor_class] - logits[v][i][tumor_class]))
 * evaluated by the very device function hipac_detect_probs uses:
 *     p[i]     = (p_0[i] + p_1[i] + ...) / (float)views    added in ascending v in float32 from the first term,
 *                                                          divided once                               float32[n]
 *     range[i] = max_v p_v[i] - min_v p_v[i]               NULL = not wanted                          float32[n]
 * With views = 1, p equals hipac_detect_probs bit for bit and range is 0.  A NaN logit in any view of a window gives
 * NaN p[i] and NaN range[i] (`--detect` treats NaN as "never a detection"). */
int hipac_tta_reduce(const float* logits, int views, int n, int tumor_class, float* p, float* range, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_TTA_H_ */

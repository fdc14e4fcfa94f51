/*
 * hipac_tissue.h -- C ABI of the Otsu tissue mask of libhipac_hip.so (gfx950): the opt-in window filter of
 * `--tissue_filter otsu`.  The coarsest resident level of a slide is reduced to a thumbnail with one pixel per 32 x 32
 * nominal level-0 pixels, the thumbnail's HSV saturation is thresholded with Otsu's method, the mask is cleaned up
 * (3 x 3 opening, dilation) and summed into an area table from which every window of every level is decided with four
 * reads -- before any of the window's pixels is touched.  The reference has no such stage (its rule is `mean > 240`,
 * which stays the default); this is the project's addition and is off in parity runs.
 *
 * These entry points live in the same shared library as include/hipac.h but carry their own version number, so
 * adding them leaves hipac.h's ABI untouched.
 *
 * Conventions: those of include/hipac.h.  Plain pointers and sizes; every data pointer is DEVICE memory; all work is
 * enqueued asynchronously on `stream` (hipStream_t as void*, NULL = default stream); nothing synchronises the device;
 * the caller owns every buffer; 0 on success, otherwise a hipError_t value or a HIPAC_E* code, with the message in the
 * thread-local last-error string of hipac.h.  Every argument check answers before the first launch.
 *
 * Arithmetic: integers throughout, except the Otsu score (IEEE double, one rounding per operation; the library is
 * compiled without floating-point contraction).  The only atomics are integer adds, which commute: every output is
 * bitwise identical from run to run and equal to the numpy restatement tests/tissue_cpu.py.
 *
 * Sizes: a mask is mw x mh pixels with mw, mh >= 1 and mw * mh < 2^24 (HIPAC_TISSUE_MAX_PIXELS), which keeps every
 * product below inside int64 and every count inside int32.
 */
#ifndef HIPAC_TISSUE_H_
#define HIPAC_TISSUE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_TISSUE_ABI_VERSION 1

#define HIPAC_TISSUE_MAX_PIXELS (1 << 24) /* mw * mh stays below this */
#define HIPAC_TISSUE_MAX_DILATE 8         /* radius D of the final dilation */
#define HIPAC_TISSUE_CELL 32              /* nominal level-0 pixels under one mask pixel */
#define HIPAC_TISSUE_WINDOW 1792          /* nominal level-0 pixels under a window of any level */

int hipac_tissue_abi_version(void);

/* Thumbnail, saturation and saturation histogram of one level image in a single pass.
 *     img: uint8[height][pitch bytes], RGB pixels, `width` of them per row; 16-byte aligned, pitch a multiple of 48
 *          bytes and at least 3 * 16 * ceil(width / 16).  Bytes of a row behind pixel `width` are never used as pixels.
 *     f:   level pixels per mask pixel side, 4, 8, 16 or 32 (= 32 >> level).  mw = ceil(width / f), mh = ceil(height / f).
 *     thumb[j][i][c] = (2 * sum + n) / (2 * n), sum over the level pixels [i f, (i + 1) f) x [j f, (j + 1) f) clipped to
 *                      width x height, n their number (the mean, rounded half up)                     uint8[mh][mw][3]
 *     sat[j][i]      = mx == 0 ? 0 : (2 * 255 * (mx - mn) + mx) / (2 * mx), mx / mn the largest / smallest channel of
 *                      thumb[j][i] (HSV saturation scaled to 255, rounded half up)                    uint8[mh][mw]
 *     hist[s]        = number of mask pixels with sat == s; zeroed by this call                       uint32[256]
 * Rows are read with 16-byte loads; a workgroup counts into a histogram in LDS and adds its non-empty bins to `hist`
 * with one integer atomic each. */
int hipac_tissue_thumbnail(const uint8_t* img, int width, int height, size_t pitch, int f, uint8_t* thumb, uint8_t* sat,
                           uint32_t* hist, void* stream);

/* Otsu's threshold of a histogram, on the device.  N = sum h, M = sum i h[i]; for t = 0 .. 254 with w0 = sum_{i <= t} h[i]
 * and m0 = sum_{i <= t} i h[i], t is a candidate iff 0 < w0 < N, and its score is
 *     d = (double)(M * w0 - N * m0)   (the difference exact in int64),   v = (d * d) / (double)(w0 * (N - w0)).
 * thresholds[0] = the candidate with the largest v, ties to the lowest t; 255 when there is no candidate (fewer than two
 * non-empty bins).  thresholds[1] = max(thresholds[0], floor), the threshold hipac_tissue_mask applies.
 * hist: uint32[256] with sum h < 2^24; 0 <= floor <= 255; thresholds: int32[2]. */
int hipac_tissue_otsu(const uint32_t* hist, int floor, int32_t* thresholds, void* stream);

/* The mask: raw = sat > thresholds[1] (read from DEVICE memory: the host never waits for the threshold), then, if
 * `opening`, an erosion and a dilation with a 3 x 3 square, then a dilation with a (2 dilate + 1)^2 square; everything
 * outside the mask counts as background.  Separable min / max passes; tmp: uint8[mh][mw] scratch, distinct from mask
 * and sat.  mask: uint8[mh][mw] of 0 / 1.  0 <= dilate <= HIPAC_TISSUE_MAX_DILATE. */
int hipac_tissue_mask(const uint8_t* sat, int mw, int mh, const int32_t* thresholds, int opening, int dilate, uint8_t* tmp,
                      uint8_t* mask, void* stream);

/* Summed-area table: table[j][i] = number of set mask pixels in [0, i) x [0, j).  int32[mh + 1][mw + 1]; a row scan, then a
 * column scan. */
int hipac_tissue_integral(const uint8_t* mask, int mw, int mh, int32_t* table, void* stream);

/* Window decisions.  A window with origin xy[k] = (x, y) in pixels of `level` (0 .. 3; negative origins allowed) has the
 * level-0 origin X = x * 2^level, Y = y * 2^level and the mask rectangle
 *     [X >> 5, (X + 1792 + 31) >> 5) x [Y >> 5, (Y + 1792 + 31) >> 5)           (arithmetic shifts)
 * n_rect = its unclipped area, c = the table's count over the rectangle clipped to the mask.
 *     keep[k] = c >= 1 && 1000 * c >= min_permille * n_rect      uint8[n]
 *     count[k] = c                                                int32[n]
 * One thread per window, four table reads.  0 <= min_permille <= 1000; n >= 0. */
int hipac_tissue_window_keep(const int32_t* table, int mw, int mh, const int32_t* xy, int n, int level, int min_permille,
                             uint8_t* keep, int32_t* count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_TISSUE_H_ */

/*
 * hipac_eval.h -- C ABI of the CAMELYON16 FROC evaluation stage of libhipac_hip.so (gfx950).
 *
 * The reference scores its per-slide detections with the official challenge script
 * (src/utils/evaluation_FROC.py, reached through `--run_evaluation`, src/main.py:1168-1225).  The image work of
 * that script -- the evaluation mask of a tumour slide, the region moments behind its ITC list and the label
 * under every detection -- runs here.  These entry points live in the same shared library as include/hipac.h
 * but carry their own version number, so adding them leaves hipac.h's ABI untouched.
 *
 * Conventions: those of include/hipac.h.  Plain pointers and sizes; data pointers are DEVICE memory unless
 * marked "host"; all work is enqueued asynchronously on `stream` (hipStream_t as void*, NULL = default
 * stream); nothing synchronises the device; the caller owns every buffer; 0 on success, otherwise a
 * hipError_t value or a HIPAC_E* code, with the message in the thread-local last-error string of hipac.h.
 */
#ifndef HIPAC_EVAL_H_
#define HIPAC_EVAL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_EVAL_ABI_VERSION 1

int hipac_eval_abi_version(void);

/* Bytes of workspace hipac_eval_mask needs for a W x H mask; 0 for sizes it refuses
 * (W or H < 1, W * H >= 2^31). */
size_t hipac_eval_workspace_bytes(int W, int H);

/* computeEvaluationMask (evaluation_FROC.py:14-35) of one mask level, bit for bit:
 *     d       = distance_transform_edt(255 - mask)       exact Euclidean distance to the nearest byte == 255
 *     binary  = sqrt((double)d^2) < threshold            threshold = 75 / (resolution * 2^level * 2)
 *     filled  = binary_fill_holes(binary)                background not 4-connected to the border -> 1
 *     labels  = label(filled, connectivity = 2)          8-connected, numbered 1..n in raster order of
 *                                                        each component's first pixel, background 0
 * mask: uint8, W x H, row pitch `pitch` bytes (>= W).  When no byte equals 255 the distance is taken to a
 * virtual zero at (row -1, column 0), as scipy's transform does.  labels: int32[H][W] (contiguous);
 * n_labels: one device int32, the number of components.  0 < threshold < 46340.
 * workspace: at least hipac_eval_workspace_bytes(W, H) bytes.  Deterministic: labels and n_labels do not
 * depend on the schedule. */
int hipac_eval_mask(const uint8_t* mask, int W, int H, int64_t pitch, double threshold, int32_t* labels,
                    int32_t* n_labels, void* workspace, size_t workspace_bytes, void* stream);

/* Integer region moments of a label map (the inputs of regionprops' major_axis_length, :38-62):
 * moments int64[n_labels][6] = (count, sum r, sum c, sum r^2, sum c^2, sum r*c) of every label 1..n_labels,
 * r = row, c = column.  Overwritten (zeroed first); labels outside 1..n_labels are ignored.  Integer
 * atomics only: the result is bitwise reproducible.  W, H <= 65536, so that no sum leaves int64. */
int hipac_eval_region_moments(const int32_t* labels, int W, int H, int n_labels, int64_t* moments, void* stream);

/* The label under every detection (compute_FP_TP_Probs, :131-132): out[i] = labels[y_i / 2^level][x_i / 2^level]
 * with the quotient truncated toward zero (Python's int(y / 2**level)); a point outside the label map gives 0.
 * xy: int64[n][2] level-0 (x, y); out: int32[n]; 0 <= level <= 30. */
int hipac_eval_lookup(const int32_t* labels, int W, int H, int level, const int64_t* xy, int n, int32_t* out,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_EVAL_H_ */

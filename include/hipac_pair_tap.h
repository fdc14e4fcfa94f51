/*
 * hipac_pair_tap.h -- raw taps of the pair modes (precision fp16x3, fp16q8) of the ResNet18 trunk in libhipac_hip.so.
 *
 * TEST SUPPORT.  hipac_resnet18_tap (include/hipac.h) returns (float)hi + (float)lo transposed to NCHW: it drops
 * the e4m3 byte tensor of fp16q8, and a block's inner map has no tap.  The conv-by-conv float64 replay
 * (oracle/pair_replay.py) needs the operands exactly as the kernels read them, so this entry point copies STORED
 * BYTES, device to device: no arithmetic and no layout change, so the exporter cannot hide a layout fault.  These
 * entry points live in the same shared library as include/hipac.h but carry their own version number; hipac.h's
 * ABI is untouched.
 *
 * Maps (of the workspace the last hipac_resnet18_forward of `batch` images left behind):
 *     1          the pooled map                  [batch][56][56]   C = 64
 *     2 .. 9     the output of block 0 .. 7      layer1: 56 x 56 x 64, layer2: 28 x 28 x 128, layer3: 14 x 14 x 256,
 *                                                layer4: 7 x 7 x 512
 *     10 .. 17   the INNER map of block 0 .. 7 (the output of its first conv), same geometry as the block's output.
 *                The blocks share one buffer: it holds block b's inner map only right after
 *                hipac_resnet18_run_ops(first_op = last_op = the first conv of block b) on the same workspace
 *                (op 2 / 4 for layer1, 6 + 5 (s - 1) / + 3 for stage s = 1 .. 3).  In the pair modes every conv is
 *                its own launch and the block outputs survive the forward, so that re-run reproduces the
 *                forward's inner map.  The caller orders the two calls on one stream; nothing here can tell
 *                which block's map the buffer holds.
 * Planes:
 *     0   the pair tensor as stored: fp16 [pixel][hi: C | lo: C], 4 C bytes per pixel.  Map 9, the last block's
 *         output, is the fp32 map float[pixel][512] instead; with the pooled head (the default) the forward left
 *         only partial sums, and the last conv runs once more with its fp32-map epilogue, as tap 9 of
 *         hipac_resnet18_tap does.  In fp16q8 the lo half of an inner map is never written (nothing reads it):
 *         those bytes are whatever the buffer held.
 *     1   fp16q8 only: the byte tensor [pixel][C / 64][lo8: 64 | hi8: 64] of OCP e4m3 values, 2 C bytes per
 *         pixel.  Map 9 has none.
 *
 * Conventions: those of include/hipac.h (device pointers, asynchronous on `stream`, 0 or an error code with the
 * message in hipac_last_error()).  Every refusal happens before any launch.
 */
#ifndef HIPAC_PAIR_TAP_H_
#define HIPAC_PAIR_TAP_H_

#include <stddef.h>

#include "hipac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_PAIR_TAP_ABI_VERSION 1

#define HIPAC_PAIR_TAP_POOL 1
#define HIPAC_PAIR_TAP_BLOCK0 2   /* + b: the output of block b */
#define HIPAC_PAIR_TAP_INNER0 10  /* + b: the inner map of block b */
#define HIPAC_PAIR_TAP_PLANE_PAIRS 0
#define HIPAC_PAIR_TAP_PLANE_Q8 1

int hipac_pair_tap_abi_version(void);

/* Bytes hipac_pair_tap_copy writes for these arguments; 0 for a combination it refuses (batch < 1, a precision that
 * is no pair mode, an unknown map or plane, plane 1 outside fp16q8 or of map 9).  Host only. */
size_t hipac_pair_tap_bytes(int batch, int precision, int map, int plane);

/* Copies the stored bytes of (map, plane) for images 0 .. batch - 1 to dst.  `batch` must be the batch of the last
 * forward on `workspace` and fit one sub-batch; `w` must be a pair-mode handle; dst_bytes must equal
 * hipac_pair_tap_bytes.  The workspace is written only for map 9 with the pooled head (see above). */
int hipac_pair_tap_copy(const hipac_weights_t* w, void* workspace, int batch, int map, int plane, void* dst,
                        size_t dst_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_PAIR_TAP_H_ */

/*
 * hipac_detect.h -- C ABI of the lesion detection stage of libhipac_hip.so (gfx950): everything between the patch
 * classifier's logits and the per-slide detection list that `--run_evaluation` (include/hipac_eval.h) scores.
 *
 * The standard CAMELYON16 post-processing: tumour probability per scored window -> probability map over a grid of
 * square cells -> (the project's addition) fusion of the maps of several pyramid levels -> Gaussian smoothing ->
 * non-maximum suppression -> one (probability, cell) per detection.  The reference never finished this stage
 * (src/preprocessing/pre_patches.py is a heat-map stub).  A window is 1792 level-0 pixels wide at every level (1792 /
 * 896 / 448 / 224 pixels at levels 0..3), so with a cell of C level-0 pixels a window of any level covers K x K cells,
 * K = 1792 / C, and one cell grid gw x gh = ceil(W0 / C) x ceil(H0 / C) serves all levels.
 *
 * These entry points live in the same shared library as include/hipac.h but carry their own version number, so
 * adding them leaves hipac.h's ABI untouched.
 *
 * Conventions: those of include/hipac.h.  Plain pointers and sizes; data pointers are DEVICE memory unless marked
 * "host"; all work is enqueued asynchronously on `stream` (hipStream_t as void*, NULL = default stream); nothing
 * synchronises the device; the caller owns every buffer; 0 on success, otherwise a hipError_t value or a HIPAC_E*
 * code, with the message in the thread-local last-error string of hipac.h.  Every argument check answers before the
 * first launch.
 *
 * Reproducibility: no floating-point atomics anywhere; every sum has a fixed order, and the library is compiled
 * without floating-point contraction, so every output below is bitwise identical from run to run and equal to a plain
 * float32 restatement that performs the same operations in the same order (tests/detect_cpu.py).
 */
#ifndef HIPAC_DETECT_H_
#define HIPAC_DETECT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_DETECT_ABI_VERSION 1

#define HIPAC_DETECT_MAX_K 56       /* cells per window side: C >= 32 */
#define HIPAC_DETECT_MAX_LEVELS 4   /* level maps one hipac_detect_fuse call combines */
#define HIPAC_DETECT_MAX_TAPS_R 32  /* radius of the Gaussian taps */
#define HIPAC_DETECT_MAX_NMS_R 64   /* suppression radius in cells */

#define HIPAC_DETECT_FUSE_MEAN 0
#define HIPAC_DETECT_FUSE_MAX 1

int hipac_detect_abi_version(void);

/* Tumour probability of every scored window from two-class logits, in float32:
 *     p[i] = 1 / (1 + exp(logits[i][1 - tumor_class] - logits[i][tumor_class]))
 * (the softmax of two classes).  logits: float32[n][2]; p: float32[n]; tumor_class 0 or 1; n >= 0. */
int hipac_detect_probs(const float* logits, int n, int tumor_class, float* p, void* stream);

/* Probability map of ONE level.  meta: int32[n][4] = (level, x, y, label) rows as the slide scan emits them, (x, y) the
 * window origin in pixels of its level; rows whose level differs from `level` are skipped, so the rows of all levels can
 * be passed as they are.  A window has cell origin (x / stride, y / stride), `stride` = C >> level pixels of that level,
 * and covers the K x K cells from there; cells outside the grid are dropped, and a window whose cell origin is outside
 * [0, gw) x [0, gh) is ignored.
 *     map[j][i]   = mean of p over the windows that cover cell (i, j), 0 where there is none      float32[gh][gw]
 *     count[j][i] = number of those windows                                                       int32[gh][gw]
 * Computed as a gather: every window's row index is stored at its cell origin in `origin` (int32[gh][gw], scratch,
 * -1 = none), then every cell adds p over its K x K candidate origins in raster order (origin rows from top to bottom,
 * within a row from left to right) in float32 and divides once.  Two windows of one level must not share a cell origin
 * (the scan's origins are distinct multiples of the stride); if they do, which one counts is unspecified.
 * 1 <= K <= HIPAC_DETECT_MAX_K; stride >= 1; gw, gh >= 1, gw * gh < 2^31; n >= 0. */
int hipac_detect_level_map(const float* p, const int32_t* meta, int n, int level, int stride, int K, int gw, int gh,
                           int32_t* origin, float* map, int32_t* count, void* stream);

/* Fuse the maps of n_levels levels (1 .. HIPAC_DETECT_MAX_LEVELS) cell by cell.  maps: float32[n_levels][gh][gw],
 * counts: int32[n_levels][gh][gw] as hipac_detect_level_map wrote them, in ascending level order.  A level has data
 * at a cell where its count is positive.
 *     HIPAC_DETECT_FUSE_MEAN  out = (sum over the levels with data, added in the order given) / (their number)
 *     HIPAC_DETECT_FUSE_MAX   out = the largest value over the levels with data
 * and 0 where no level has data.  out: float32[gh][gw]. */
int hipac_detect_fuse(const float* maps, const int32_t* counts, int n_levels, int gw, int gh, int mode, float* out,
                      void* stream);

/* Separable Gaussian smoothing with zeros outside the map.  taps: HOST float32[2 * radius + 1], read before the call
 * returns (the caller makes them in float64 as scipy's gaussian_filter does -- exp(-k^2 / (2 sigma^2)), radius =
 * int(4 sigma + 0.5), normalised -- and rounds them to float32).  Rows first, then columns:
 *     tmp[y][x] = sum_{k = -radius .. +radius} taps[k + radius] * in[y][x + k]
 *     out[y][x] = sum_{k = -radius .. +radius} taps[k + radius] * tmp[y + k][x]
 * each accumulated in float32 from 0 in the order written, the multiplication and the addition rounded separately.
 * tmp, out: float32[gh][gw], distinct from `in` and from each other.  0 <= radius <= HIPAC_DETECT_MAX_TAPS_R. */
int hipac_detect_smooth(const float* in, int gw, int gh, const float* taps, int radius, float* tmp, float* out,
                        void* stream);

/* Bytes of workspace hipac_detect_nms needs for a gw x gh map; 0 for sizes it refuses (gw or gh < 1,
 * gw * gh >= 2^31). */
size_t hipac_detect_nms_workspace_bytes(int gw, int gh);

/* Greedy non-maximum suppression.  The result equals this procedure exactly, values and order:
 *     1. take the largest cell of the map; among equal values the LOWEST RASTER INDEX (j * gw + i) wins;
 *     2. stop if it is below `threshold` (a cell is a detection only if value >= threshold; NaN never is);
 *     3. emit it;
 *     4. clear every cell (i', j') with (i' - i)^2 + (j' - j)^2 <= radius^2;
 *     5. repeat until max_detections have been emitted.
 * The tie rule is part of the contract: on a flat plateau the first cell in raster order wins, then the first cell
 * in raster order that the suppression left, and so on.
 * It does not run as dependent arg-max launches: in every round each live cell that is the largest of its own
 * neighbourhood under the total order (value descending, raster index ascending) is selected at once and the
 * neighbourhoods of the selected cells are cleared; the survivors are sorted by the same order and truncated.  That
 * yields the greedy result (tests/detect_cpu.py proves the two forms against each other on random and tied maps).
 *     p[k], ij[k] = (i, j)   value and cell of detection k, k < *count       float32[max_detections], int32[max_detections][2]
 *     *count                 min(number of detections, max_detections)       one device int32
 * Entries at and after *count are not written.  0 <= radius <= HIPAC_DETECT_MAX_NMS_R; max_detections >= 1;
 * workspace: at least hipac_detect_nms_workspace_bytes(gw, gh) bytes. */
int hipac_detect_nms(const float* map, int gw, int gh, int radius, float threshold, int max_detections, float* p,
                     int32_t* ij, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_DETECT_H_ */

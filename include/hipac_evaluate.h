/*
 * hipac_evaluate.h -- C ABI of the patch-level evaluation stage of libhipac_hip.so (gfx950): everything between the
 * patch classifier's tumour probabilities and the figures `--eval_patches` reports (the reference's `--evaluate`,
 * src/main.py:974-1015, with the quantities of src/utils/metrics.py, a ROC / AUC, and a bootstrap over slides).
 *
 * Two steps, integers only.  `hipac_evaluate_accumulate` adds one batch of scored patches to three running tables:
 * per slide and true class a histogram of the tumour probability over HIPAC_EVALUATE_BINS equal bins, per slide the
 * confusion counts of the caller's decision, and a count of rows that could not be tallied.  The tables are sums of
 * ones, so a set of rows gives the same tables however it is cut into batches.  `hipac_evaluate_bootstrap` resamples
 * the SLIDES (patches of one slide are not independent) and returns, per replicate, the weighted confusion counts and
 * twice the Mann-Whitney U of the weighted histograms.  The probabilities themselves come from hipac_detect_probs
 * (include/hipac_detect.h); this header has no softmax of its own.
 *
 * The bin of a probability p (float32, 0 <= p <= 1) is min(4095, (int)(p * 4096.0f)): the product is exact (a power
 * of two), the conversion truncates, and p = 1 joins the last bin.
 *
 * The draws.  Replicate r draws G slides out of G with replacement, with exactly the draws of
 * hipac_eval_ci_counts(seed, r, ..., S = G) (include/hipac_eval_ci.h: Philox counter (d / 4, r, 0, 2), slide
 * (word * G) >> 32); r is the absolute index first_replicate + i, so a replicate depends neither on B nor on where a
 * call starts.  With c[g] = how often slide g is drawn:
 *     H[t][b]   = sum_g c[g] * hist[g][t][b]
 *     conf_w[k] = sum_g c[g] * conf[g][k]
 *     n_pos     = sum_b H[1][b],   n_neg = sum_b H[0][b]
 *     u2        = sum_b H[1][b] * (2 * sum_{b' < b} H[0][b'] + H[0][b])
 * u2 is twice the Mann-Whitney U of the binned scores with ties inside a bin counted half: auc = u2 / (2 n_pos n_neg).
 * H never exists in memory: one workgroup per replicate keeps it in registers (256 threads x 16 bins x 2 classes).
 *
 * The caller's contract: G * (the largest number of rows of one slide) < 2^31, so that every H[t][b] and both class
 * totals fit 32 bits and u2 fits 64.  The library cannot see the row counts without reading the tables back; the
 * Python wrapper (evaluate.py) checks the contract and raises.
 *
 * Conventions: those of include/hipac_detect.h.  Plain pointers and sizes; data pointers are DEVICE memory; all work is
 * enqueued asynchronously on `stream` (hipStream_t as void*, NULL = default stream); nothing synchronises the device;
 * the caller owns every buffer; 0 on success, otherwise a hipError_t value or a HIPAC_E* code, with the message in the
 * thread-local last-error string of hipac.h.  Every argument check answers before the first launch.  No floating-point
 * sums anywhere; hipac_evaluate_accumulate uses integer atomics (order-independent), hipac_evaluate_bootstrap no global
 * atomics at all: every output is bitwise reproducible and equal to the numpy restatement tests/eval_patches_cpu.py.
 */
#ifndef HIPAC_EVALUATE_H_
#define HIPAC_EVALUATE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_EVALUATE_ABI_VERSION 1

#define HIPAC_EVALUATE_BINS 4096             /* bins of the probability histogram (the width of hipac_stain.h's) */
#define HIPAC_EVALUATE_MAX_GROUPS 4096       /* G, = HIPAC_EVAL_CI_MAX_CASES */
#define HIPAC_EVALUATE_MAX_REPLICATES 65536  /* B */

int hipac_evaluate_abi_version(void);

/* Add n rows to the running tables (which the caller zeroes once, before the first batch).
 *   p      float32[n]   tumour probability (hipac_detect_probs)
 *   pred   uint8[n]     the caller's decision, 0 or 1
 *   label  uint8[n]     the true class, 0 or 1
 *   group  int32[n]     the row's slide, 0 <= group < G
 *   hist   uint32[G][2][4096]   [slide][true class][bin], 16-byte aligned
 *   conf   uint32[G][4]         (TN, FP, FN, TP) of pred against label
 *   n_bad  one uint32           rows with p NaN or outside [0, 1], label or pred above 1, or group outside [0, G);
 *                               such a row is counted here and touches nothing else
 * 1 <= G <= HIPAC_EVALUATE_MAX_GROUPS; n >= 0, and n == 0 launches nothing (p, pred, label, group may then be NULL).
 * A workgroup takes a run of consecutive rows, tallies the confusion counts of the run's first slide locally and
 * flushes them once: rows of one slide arrive together and do not serialise on four addresses. */
int hipac_evaluate_accumulate(const float* p, const uint8_t* pred, const uint8_t* label, const int32_t* group, int n, int G,
                              uint32_t* hist, uint32_t* conf, uint32_t* n_bad, void* stream);

/* B replicates, first_replicate .. first_replicate + B - 1, of the tables above (hist 16-byte aligned).
 * Outputs, row i = replicate first_replicate + i:  conf_w int64[B][4];  u2, n_pos, n_neg int64[B].
 * 1 <= G <= HIPAC_EVALUATE_MAX_GROUPS, 1 <= B <= HIPAC_EVALUATE_MAX_REPLICATES, 0 <= first_replicate,
 * first_replicate + B <= 2^32; the caller's contract above holds for the tables. */
int hipac_evaluate_bootstrap(const uint32_t* hist, const uint32_t* conf, int G, uint64_t seed, int64_t first_replicate, int B,
                             int64_t* conf_w, int64_t* u2, int64_t* n_pos, int64_t* n_neg, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_EVALUATE_H_ */

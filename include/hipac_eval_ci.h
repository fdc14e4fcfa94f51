/*
 * hipac_eval_ci.h -- C ABI of the bootstrap stage of the CAMELYON16 evaluation in libhipac_hip.so (gfx950).
 *
 * `--run_evaluation --eval_bootstrap B` resamples the evaluated cases B times (S draws out of S cases, with
 * replacement) and reports percentile intervals of the FROC score, of the six sensitivities behind it and of
 * the slide-level ROC AUC.  Every replicate is a weighted scan over one shared event table; that scan runs
 * here, one workgroup per replicate, in integers only.  Everything float stays with the caller: it turns the
 * per-case probability lists into the rank tables below once (froc_ci.build_tables), with the comparisons of
 * froc.computeFROC (false positives as float64, true-positive slots as float32 against the thresholds rounded
 * to float32), and divides the integers that come back.  These entry points live in the same shared library
 * as include/hipac.h but carry their own version number; hipac.h's and hipac_eval.h's ABIs are untouched.
 *
 * The draws.  Draw d (0 <= d < S) of replicate r takes word d % 4 of
 *     philox4x32_10(counter = (d / 4, r, 0, 2), key = (seed & 0xffffffff, seed >> 32))
 * and picks case (word * S) >> 32.  r is the absolute replicate index first_replicate + i, so a replicate
 * depends neither on B nor on where a call starts; counter word 3 = 2 keeps the draws apart from the dropout
 * masks (sites 0 and 1 of include/hipac_mil_dropout.h) under the same seed.  counts[s] = how often case s is
 * drawn, built with LDS integer atomics (order-independent).
 *
 * The tables.  T_0 < T_1 < ... are the distinct values (as float64) of every FP probability and every TP
 * slot of the full table.  Event k (one FP probability or one TP slot of one case) carries
 *     ev_case[k] = 2 * case + (1 for a TP slot, 0 for an FP)
 *     ev_hi[k]   = the highest i at which the event is counted: value >= T_i (FP, float64; this is the index
 *                  of its own value) or slot >= (float)T_i (TP, float32; never below the index of its own value)
 *     ev_own[k]  = the i with T_i == its own value
 * sorted by ev_hi, descending (ties in any order).  case_tumours[s] = the case's number of tumours,
 * case_min_own[s] = the smallest ev_own among the case's events (INT32_MAX for a case without events).
 * The slides: slide_case[p] = 2 * case + label (1 = tumour) for p = 0..S-1 in ascending order of the slide
 * score, and slide_tie[p] = {first position of p's group of equal scores, one past its last}.
 *
 * The replicate.  With w_k = counts[case of k]: FP(i) = sum of w_k over FP events with ev_hi >= i, TP(i)
 * likewise over TP events; i is present when some event with w_k > 0 has ev_own == i.  For rate R (the
 * integer 4 * rate: 1, 2, 4, ... 32 for 1/4 ... 8 false positives per slide)
 *     tp_at_rate = TP(i*) at the lowest i* that is present, is not the smallest present i (computeFROC drops
 *                  the smallest value from its thresholds) and has 4 * FP(i*) <= R * S;  0 when there is none
 *                  (the curve's closing (0, 0) point)
 * which is the numerator of froc_score's sensitivity at that rate: FP and TP only grow towards lower i, so
 * the lowest admissible threshold has the largest TP count, and count / S <= rate in float64 is the integer
 * test above for every S below 2^40.  The kernel walks the event table in chunks of HIPAC_EVAL_CI_CHUNK
 * events (256 threads x 4 consecutive events, a workgroup-wide prefix sum of the weighted FP counts per
 * chunk, the running total carried in 64 bits), so the table may be far larger than LDS; it stops at the
 * first chunk past the last threshold any rate can still use.
 *
 * Conventions: those of include/hipac.h.  Plain pointers and sizes; data pointers are DEVICE memory unless
 * marked "host"; all work is enqueued asynchronously on `stream` (hipStream_t as void*, NULL = default
 * stream); nothing synchronises the device; the caller owns every buffer; 0 on success, otherwise a
 * hipError_t value or a HIPAC_E* code, with the message in the thread-local last-error string of hipac.h.
 * A null argument or an out-of-range size is refused before any launch.  No floating point, no global
 * atomics: every output is bitwise reproducible and independent of the schedule.
 */
#ifndef HIPAC_EVAL_CI_H_
#define HIPAC_EVAL_CI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_EVAL_CI_ABI_VERSION 1

#define HIPAC_EVAL_CI_MAX_CASES 4096         /* S */
#define HIPAC_EVAL_CI_MAX_EVENTS (1 << 24)   /* n_events */
#define HIPAC_EVAL_CI_MAX_REPLICATES 65536   /* B */
#define HIPAC_EVAL_CI_MAX_RATES 8
#define HIPAC_EVAL_CI_CHUNK 1024             /* events per step of the walk over the event table */

int hipac_eval_ci_abi_version(void);

/* The draws alone: counts int32[B][S], row i = the counts of replicate first_replicate + i.
 * 1 <= S <= 4096, 1 <= B <= 65536, 0 <= first_replicate, first_replicate + B <= 2^32. */
int hipac_eval_ci_counts(uint64_t seed, int64_t first_replicate, int B, int S, int32_t* counts, void* stream);

/* The kernel keeps a replicate's working set -- the count table and the prefix of the negatives' weights over
 * the slides -- in LDS and takes no device workspace.  This is the size of that working set in bytes (what
 * one workgroup requests as dynamic LDS); 0 for sizes hipac_eval_ci_bootstrap refuses (S < 1 or > 4096,
 * n_events < 0 or > 2^24, B < 1 or > 65536). */
size_t hipac_eval_ci_workspace_bytes(int S, int n_events, int B);

/* B replicates, first_replicate .. first_replicate + B - 1, of the tables above.
 * ev_case, ev_hi, ev_own: int32[n_events], 16-byte aligned (may be NULL when n_events == 0).
 * case_tumours, case_min_own, slide_case: int32[S]; slide_tie: int32[S][2].
 * rates4: host, int32[n_rates], 1 <= n_rates <= 8, every entry in 1 .. 2^20.
 * Outputs, row i = replicate first_replicate + i:
 *   tp_at_rate int64[B][n_rates]   as defined above
 *   tumours    int64[B]            sum of counts[s] * case_tumours[s] (the sensitivity's denominator)
 *   u2         int64[B]            twice the Mann-Whitney U of the drawn slides, ties counted half:
 *                                  sum over drawn tumour i, normal j of (2 if score_i > score_j, 1 if equal)
 *   n_pos, n_neg int32[B]          drawn tumour and normal slides (n_pos + n_neg == S) */
int hipac_eval_ci_bootstrap(const int32_t* ev_case, const int32_t* ev_hi, const int32_t* ev_own, int n_events,
                            const int32_t* case_tumours, const int32_t* case_min_own, const int32_t* slide_case,
                            const int32_t* slide_tie, int S, uint64_t seed, int64_t first_replicate, int B,
                            const int32_t* rates4, int n_rates, int64_t* tp_at_rate, int64_t* tumours, int64_t* u2,
                            int32_t* n_pos, int32_t* n_neg, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_EVAL_CI_H_ */

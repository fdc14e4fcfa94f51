// Bootstrap replicates of the CAMELYON16 evaluation (include/hipac_eval_ci.h has the definitions; tests/eval_ci_cpu.py
// restates them in numpy): one workgroup per replicate, integers only.
//
// A replicate
//   1. draws its S case indices with Philox into the count table cnt[S] in LDS (integer atomics: order-independent;
//      ci_draws.h, shared with evaluate.hip);
//   2. reduces over the cases: the tumour total, the drawn positives / negatives, the smallest present threshold index
//      minP (from the per-case minima the host supplies), and twice the Mann-Whitney U from an exclusive prefix of the
//      negatives' weights over the slides in score order (negpre[], LDS) and the host's tie groups;
//   3. pass A walks the event table (sorted by ev_hi, descending) in chunks of kCiChunk = 1024 events -- 256 threads x 4
//      consecutive events -- with a workgroup-wide prefix sum F of the weighted FP counts, the total carried in 64 bits.
//      F only grows along the walk and ev_hi only falls, so for rate R the first event k with 4 F_k > R S has
//      FP(ev_hi[k]) > the limit and FP(ev_hi[k] + 1) <= it: jstar[R] = ev_hi[k] + 1 is the lowest index whose FP count
//      passes (0 when the walk ends below the limit).  Exactly one thread sees a rate's crossing; it stores jstar[R].
//      The walk stops once every rate has crossed;
//   4. pass B: jr[R] = the smallest ev_own >= jstar[R] among events with a drawn case, minP excluded (a min reduction);
//      only events with ev_hi >= min jstar can qualify (ev_own <= ev_hi), a prefix of the table;
//   5. pass C: tp[R] = the weighted number of TP events with ev_hi >= jr[R] (a sum reduction), again over a prefix.
// The table is shared by all replicates and is read from L2; LDS holds 2 S + a few words per workgroup (at most 33 KiB, so
// four or more workgroups per CU at every S), all of it in the dynamic region with 32-bit accesses only.
#include "common.h"

#include <limits.h>

#include "../../include/hipac_eval_ci.h"
#include "ci_draws.h"
#include "wave_reduce.h"

namespace hipac {

constexpr int kCiPerThread = 4;
constexpr int kCiChunk = kCiThreads * kCiPerThread;  // events per step of every walk over the table
constexpr int kCiWaves = kCiThreads / 64;
constexpr int kCiScratch = 64;  // words of reduction scratch and per-rate results behind the two tables
static_assert(kCiChunk == HIPAC_EVAL_CI_CHUNK, "the header states the chunk");

struct CiRates {
  int n;
  int r4[HIPAC_EVAL_CI_MAX_RATES];
};

static inline int ci_pad4(int S) { return (S + 3) & ~3; }
static inline size_t ci_lds_bytes(int S) { return (size_t)(2 * ci_pad4(S) + 4 + kCiScratch) * sizeof(int32_t); }

// four consecutive entries a[k .. k + 3] of an event array, `fill` past its end
__device__ __forceinline__ void ci_load4(const int32_t* __restrict__ a, int k, int n, int fill, int (&out)[kCiPerThread]) {
  if (k + kCiPerThread <= n) {
    const int4 v = *reinterpret_cast<const int4*>(a + k);  // k is a multiple of 4, the array 16-byte aligned
    out[0] = v.x, out[1] = v.y, out[2] = v.z, out[3] = v.w;
  } else {
#pragma unroll
    for (int i = 0; i < kCiPerThread; ++i) out[i] = k + i < n ? a[k + i] : fill;
  }
}

// the weight of an event's case; a case index outside the table (a malformed table, or the fill -1) weighs nothing
__device__ __forceinline__ int ci_weight(const int* cnt, int case_word, int S) {
  const unsigned s = (unsigned)(case_word >> 1);
  return case_word >= 0 && s < (unsigned)S ? cnt[s] : 0;
}

__global__ __launch_bounds__(kCiThreads) void eval_ci_counts_kernel(int S, uint32_t first, uint32_t k0, uint32_t k1,
                                                                     int32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) int32_t ci_lds[];
  ci_draw_counts(ci_lds, S, first + blockIdx.x, k0, k1);
  for (int s = threadIdx.x; s < S; s += kCiThreads) counts[(size_t)blockIdx.x * S + s] = ci_lds[s];
}

__global__ __launch_bounds__(kCiThreads) void eval_ci_bootstrap_kernel(
    const int32_t* __restrict__ ev_case, const int32_t* __restrict__ ev_hi, const int32_t* __restrict__ ev_own, int n,
    const int32_t* __restrict__ case_tumours, const int32_t* __restrict__ case_min_own, const int32_t* __restrict__ slide_case,
    const int32_t* __restrict__ slide_tie, int S, uint32_t first, uint32_t k0, uint32_t k1, CiRates rates,
    int64_t* __restrict__ tp_at_rate, int64_t* __restrict__ tumours, int64_t* __restrict__ u2_out, int32_t* __restrict__ n_pos,
    int32_t* __restrict__ n_neg) {
  extern __shared__ __attribute__((aligned(16))) int32_t ci_lds[];
  const int Sp = (S + 3) & ~3;
  int* cnt = ci_lds;               // [Sp]
  int* negpre = ci_lds + Sp;       // [S + 1] (<= Sp + 4)
  int* scratch = negpre + Sp + 4;  // [16] reductions, then jstar[8], jr[8]
  int* jstar = scratch + 16;
  int* jr = scratch + 24;
  const int t = threadIdx.x;

  ci_draw_counts(cnt, S, first + blockIdx.x, k0, k1);

  // ---- the cases: tumour total, smallest present index ----
  long long tum = 0;
  int min_p = INT_MAX;
  for (int s = t; s < S; s += kCiThreads) {
    const int c = cnt[s];
    tum += (long long)c * case_tumours[s];
    if (c > 0) min_p = min(min_p, case_min_own[s]);
  }
  tum = block_sum<kCiWaves>(tum, scratch);
  min_p = block_min<kCiWaves>(min_p, scratch);

  // ---- the slides in score order: exclusive prefix of the negatives' weights, then 2 U over the tie groups ----
  const int per = (S + kCiThreads - 1) / kCiThreads;  // <= 16 consecutive positions per thread
  int neg_local = 0, pos_local = 0;
  for (int i = 0; i < per; ++i) {
    const int p = t * per + i;
    if (p < S) {
      const int w = ci_weight(cnt, slide_case[p], S);
      if (slide_case[p] & 1) pos_local += w;
      else neg_local += w;
    }
  }
  int neg_total;
  int run = block_scan_excl<kCiWaves>(neg_local, scratch, neg_total);
  for (int i = 0; i < per; ++i) {
    const int p = t * per + i;
    if (p < S) {
      negpre[p] = run;
      if (!(slide_case[p] & 1)) run += ci_weight(cnt, slide_case[p], S);
    }
  }
  if (t == 0) negpre[S] = neg_total;
  __syncthreads();
  long long u2 = 0;
  for (int p = t; p < S; p += kCiThreads) {
    const int sc = slide_case[p];
    if (sc & 1) {
      const int a = min(max(slide_tie[2 * p], 0), S), b = min(max(slide_tie[2 * p + 1], 0), S);
      const int below = negpre[a], tied = negpre[b] - below;
      u2 += (long long)ci_weight(cnt, sc, S) * (2 * below + tied);
    }
  }
  u2 = block_sum<kCiWaves>(u2, scratch);
  const long long pos_total = block_sum<kCiWaves>((long long)pos_local, scratch);

  // ---- pass A: where each rate's FP limit is crossed ----
  long long lim[HIPAC_EVAL_CI_MAX_RATES], lim_max = 0;
#pragma unroll
  for (int R = 0; R < HIPAC_EVAL_CI_MAX_RATES; ++R) {
    lim[R] = R < rates.n ? (long long)rates.r4[R] * S : 0;
    lim_max = lim[R] > lim_max ? lim[R] : lim_max;
  }
  if (t < 8) jstar[t] = 0;
  if (t >= 8 && t < 16) jr[t - 8] = INT_MAX;
  __syncthreads();
  long long carry = 0;
  for (int base = 0; base < n && 4 * carry <= lim_max; base += kCiChunk) {
    const int k = base + t * kCiPerThread;
    int cw[kCiPerThread], hi[kCiPerThread], w[kCiPerThread];
    ci_load4(ev_case, k, n, -1, cw);
    ci_load4(ev_hi, k, n, 0, hi);
    int local = 0;
#pragma unroll
    for (int i = 0; i < kCiPerThread; ++i) {
      w[i] = (cw[i] & 1) ? 0 : ci_weight(cnt, cw[i], S);  // FP events only
      local += w[i];
    }
    int total;
    const long long before = carry + block_scan_excl<kCiWaves>(local, scratch, total);
    const long long after = before + local;
#pragma unroll
    for (int R = 0; R < HIPAC_EVAL_CI_MAX_RATES; ++R) {
      if (R < rates.n && 4 * before <= lim[R] && 4 * after > lim[R]) {  // this thread holds rate R's crossing
        long long f = before;
        int j = -1;
#pragma unroll
        for (int i = 0; i < kCiPerThread; ++i) {  // the first event whose inclusive prefix exceeds the limit
          f += w[i];
          if (j < 0 && 4 * f > lim[R]) j = hi[i] + 1;
        }
        jstar[R] = j;
      }
    }
    carry += total;
  }
  __syncthreads();

  // ---- pass B: the lowest admissible present threshold of each rate ----
  int js[HIPAC_EVAL_CI_MAX_RATES], js_min = INT_MAX;
#pragma unroll
  for (int R = 0; R < HIPAC_EVAL_CI_MAX_RATES; ++R) {
    js[R] = R < rates.n ? jstar[R] : INT_MAX;
    js_min = min(js_min, js[R]);
  }
  int best[HIPAC_EVAL_CI_MAX_RATES];
#pragma unroll
  for (int R = 0; R < HIPAC_EVAL_CI_MAX_RATES; ++R) best[R] = INT_MAX;
  for (int base = 0; base < n && ev_hi[base] >= js_min; base += kCiChunk) {
    const int k = base + t * kCiPerThread;
    int cw[kCiPerThread], own[kCiPerThread];
    ci_load4(ev_case, k, n, -1, cw);
    ci_load4(ev_own, k, n, 0, own);
#pragma unroll
    for (int i = 0; i < kCiPerThread; ++i) {
      if (ci_weight(cnt, cw[i], S) > 0 && own[i] != min_p) {
#pragma unroll
        for (int R = 0; R < HIPAC_EVAL_CI_MAX_RATES; ++R)
          if (own[i] >= js[R]) best[R] = min(best[R], own[i]);
      }
    }
  }
#pragma unroll
  for (int R = 0; R < HIPAC_EVAL_CI_MAX_RATES; ++R)
    if (best[R] != INT_MAX) atomicMin(&jr[R], best[R]);
  __syncthreads();

  // ---- pass C: the weighted TP count at that threshold ----
  int jt[HIPAC_EVAL_CI_MAX_RATES], jt_min = INT_MAX;
#pragma unroll
  for (int R = 0; R < HIPAC_EVAL_CI_MAX_RATES; ++R) {
    jt[R] = R < rates.n ? jr[R] : INT_MAX;
    jt_min = min(jt_min, jt[R]);
  }
  long long tp[HIPAC_EVAL_CI_MAX_RATES];
#pragma unroll
  for (int R = 0; R < HIPAC_EVAL_CI_MAX_RATES; ++R) tp[R] = 0;
  for (int base = 0; base < n && jt_min != INT_MAX && ev_hi[base] >= jt_min; base += kCiChunk) {
    const int k = base + t * kCiPerThread;
    int cw[kCiPerThread], hi[kCiPerThread];
    ci_load4(ev_case, k, n, -1, cw);
    ci_load4(ev_hi, k, n, -1, hi);
#pragma unroll
    for (int i = 0; i < kCiPerThread; ++i) {
      const int w = (cw[i] & 1) ? ci_weight(cnt, cw[i], S) : 0;  // TP events only
#pragma unroll
      for (int R = 0; R < HIPAC_EVAL_CI_MAX_RATES; ++R)
        if (hi[i] >= jt[R]) tp[R] += w;
    }
  }
#pragma unroll
  for (int R = 0; R < HIPAC_EVAL_CI_MAX_RATES; ++R) {
    if (R < rates.n) {  // uniform: every thread takes part in the reduction
      const long long v = block_sum<kCiWaves>(tp[R], scratch);
      if (t == 0) tp_at_rate[(size_t)blockIdx.x * rates.n + R] = v;
    }
  }
  if (t == 0) {
    tumours[blockIdx.x] = tum;
    u2_out[blockIdx.x] = u2;
    n_pos[blockIdx.x] = (int32_t)pos_total;
    n_neg[blockIdx.x] = neg_total;
  }
}

static bool ci_sizes_ok(int S, int n_events, int B) {
  return S >= 1 && S <= HIPAC_EVAL_CI_MAX_CASES && n_events >= 0 && n_events <= HIPAC_EVAL_CI_MAX_EVENTS && B >= 1 &&
         B <= HIPAC_EVAL_CI_MAX_REPLICATES;
}

static bool ci_replicates_ok(int64_t first, int B) { return first >= 0 && first + B <= ((int64_t)1 << 32); }

}  // namespace hipac

extern "C" int hipac_eval_ci_abi_version(void) { return HIPAC_EVAL_CI_ABI_VERSION; }

extern "C" size_t hipac_eval_ci_workspace_bytes(int S, int n_events, int B) {
  using namespace hipac;
  return ci_sizes_ok(S, n_events, B) ? ci_lds_bytes(S) : 0;
}

extern "C" int hipac_eval_ci_counts(uint64_t seed, int64_t first_replicate, int B, int S, int32_t* counts, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(counts, HIPAC_EINVAL, "eval_ci_counts: null argument");
  HIPAC_REQUIRE(ci_sizes_ok(S, 0, B), HIPAC_EINVAL, "eval_ci_counts: S %d, B %d (need 1 <= S <= %d, 1 <= B <= %d)", S, B,
                HIPAC_EVAL_CI_MAX_CASES, HIPAC_EVAL_CI_MAX_REPLICATES);
  HIPAC_REQUIRE(ci_replicates_ok(first_replicate, B), HIPAC_EINVAL, "eval_ci_counts: replicates %lld + %d leave 0 .. 2^32",
                (long long)first_replicate, B);
  hipLaunchKernelGGL(eval_ci_counts_kernel, dim3(B), dim3(kCiThreads), ci_lds_bytes(S), (hipStream_t)stream, S,
                     (uint32_t)first_replicate, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), counts);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_eval_ci_bootstrap(const int32_t* ev_case, const int32_t* ev_hi, const int32_t* ev_own, int n_events,
                                       const int32_t* case_tumours, const int32_t* case_min_own, const int32_t* slide_case,
                                       const int32_t* slide_tie, int S, uint64_t seed, int64_t first_replicate, int B,
                                       const int32_t* rates4, int n_rates, int64_t* tp_at_rate, int64_t* tumours, int64_t* u2,
                                       int32_t* n_pos, int32_t* n_neg, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(ci_sizes_ok(S, n_events, B), HIPAC_EINVAL,
                "eval_ci_bootstrap: S %d, n_events %d, B %d (need 1 <= S <= %d, 0 <= n_events <= %d, 1 <= B <= %d)", S, n_events, B,
                HIPAC_EVAL_CI_MAX_CASES, HIPAC_EVAL_CI_MAX_EVENTS, HIPAC_EVAL_CI_MAX_REPLICATES);
  HIPAC_REQUIRE(case_tumours && case_min_own && slide_case && slide_tie && rates4 && tp_at_rate && tumours && u2 && n_pos && n_neg,
                HIPAC_EINVAL, "eval_ci_bootstrap: null argument");
  HIPAC_REQUIRE(n_events == 0 || (ev_case && ev_hi && ev_own), HIPAC_EINVAL, "eval_ci_bootstrap: null event table");
  HIPAC_REQUIRE((((uintptr_t)ev_case | (uintptr_t)ev_hi | (uintptr_t)ev_own) & 15) == 0, HIPAC_EINVAL,
                "eval_ci_bootstrap: the event arrays must be 16-byte aligned");
  HIPAC_REQUIRE(ci_replicates_ok(first_replicate, B), HIPAC_EINVAL, "eval_ci_bootstrap: replicates %lld + %d leave 0 .. 2^32",
                (long long)first_replicate, B);
  HIPAC_REQUIRE(n_rates >= 1 && n_rates <= HIPAC_EVAL_CI_MAX_RATES, HIPAC_EINVAL, "eval_ci_bootstrap: n_rates %d (1 .. %d)", n_rates,
                HIPAC_EVAL_CI_MAX_RATES);
  CiRates rates = {};
  rates.n = n_rates;
  for (int i = 0; i < n_rates; ++i) {
    HIPAC_REQUIRE(rates4[i] >= 1 && rates4[i] <= (1 << 20), HIPAC_EINVAL, "eval_ci_bootstrap: rates4[%d] = %d (1 .. 2^20)", i, rates4[i]);
    rates.r4[i] = rates4[i];
  }
  hipLaunchKernelGGL(eval_ci_bootstrap_kernel, dim3(B), dim3(kCiThreads), ci_lds_bytes(S), (hipStream_t)stream, ev_case, ev_hi,
                     ev_own, n_events, case_tumours, case_min_own, slide_case, slide_tie, S, (uint32_t)first_replicate,
                     (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), rates, tp_at_rate, tumours, u2, n_pos, n_neg);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

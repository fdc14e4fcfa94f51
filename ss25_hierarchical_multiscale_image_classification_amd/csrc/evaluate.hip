// Patch-level evaluation (include/hipac_evaluate.h has the definitions; tests/eval_patches_cpu.py restates them in numpy):
// the tallies behind `--eval_patches`, integers only.
//
// accumulate.  A workgroup of 256 threads takes kEvRun = 2048 consecutive rows, eight per thread.  A valid row adds one to its
// bin of hist[slide][class][4096] with a global integer atomic: the addresses of a batch spread over 8192 words per slide.
// The confusion counts would not -- all rows of a slide meet on four words -- so a workgroup counts the rows of the run's
// first slide g0 in registers, reduces them over the wave by shuffles and over the waves in LDS, and flushes the four
// sums with one atomic each; rows of another slide (a run that straddles a slide boundary, or rows in no order at all)
// go to their words directly.  Bad rows are counted the same way into n_bad.  Sums of ones: any split of the rows into
// batches, and any schedule, gives the same tables.
//
// bootstrap.  One workgroup per replicate.  The replicate's weighted histogram H[2][4096] lives in registers: thread t owns
// the bins j * 1024 + 4 t .. + 3 of both classes for j = 0..3 (32 VGPRs), so a wave reads 1 KiB of a slide's row with one
// 16-byte load per lane and the 8 loads of a slide are independent.  The draw counts c[G] sit in LDS (ci_draws.h, the
// helper eval_ci.hip draws with); every thread walks the slides in the same order and skips those with c[g] == 0 (about
// a third of them).  Then four exclusive scans of the negatives run at once -- one per 1024-bin segment j, the per-thread
// sums of four bins scanned over the wave by shuffles, the waves' totals exchanged through 16 words of LDS behind one
// barrier -- and the segment totals chain them into the prefix over all 4096 bins.  u2, the class totals and the weighted
// confusion counts are 64-bit workgroup sums.  LDS: 4 G + 384 bytes (at most 16.4 KiB); no global atomics, no floats.
#include "common.h"

#include "../../include/hipac_eval_ci.h"
#include "../../include/hipac_evaluate.h"
#include "ci_draws.h"
#include "wave_reduce.h"

namespace hipac {

constexpr int kEvBins = HIPAC_EVALUATE_BINS;
constexpr int kEvThreads = kCiThreads;                    // 256: the draws helper's workgroup
constexpr int kEvWaves = kEvThreads / 64;
constexpr int kEvRowsPerThread = 8;
constexpr int kEvRun = kEvThreads * kEvRowsPerThread;     // rows of one accumulate workgroup
constexpr int kEvSeg = kEvBins / (4 * kEvThreads);        // 4 segments of 1024 bins: 4 bins per thread and segment
constexpr int kEvScratch = 96;                            // words of LDS behind the counts: 32 scan + 64 reduction
static_assert(HIPAC_EVALUATE_MAX_GROUPS == HIPAC_EVAL_CI_MAX_CASES, "the slides are drawn as eval_ci's cases are");
static_assert(kEvSeg * 4 * kEvThreads == kEvBins && kEvSeg * kEvWaves <= 32, "bin ownership of the replicate kernel");

__global__ __launch_bounds__(kEvThreads) void evaluate_accumulate_kernel(const float* __restrict__ p, const uint8_t* __restrict__ pred,
                                                                          const uint8_t* __restrict__ label,
                                                                          const int32_t* __restrict__ group, int n, int G,
                                                                          uint32_t* __restrict__ hist, uint32_t* __restrict__ conf,
                                                                          uint32_t* __restrict__ n_bad) {
  __shared__ unsigned tally[5];  // the run's first slide: TN, FP, FN, TP; [4] = bad rows
  const long long base = (long long)blockIdx.x * kEvRun;
  if (threadIdx.x < 5) tally[threadIdx.x] = 0;
  __syncthreads();
  const int g_first = group[base];  // base < n: the grid covers exactly ceil(n / kEvRun) runs
  const int g0 = g_first >= 0 && g_first < G ? g_first : -1;
  unsigned loc0 = 0, loc1 = 0, loc2 = 0, loc3 = 0, bad = 0;
#pragma unroll
  for (int i = 0; i < kEvRowsPerThread; ++i) {
    const long long row = base + i * kEvThreads + threadIdx.x;  // consecutive lanes, consecutive rows
    if (row >= n) break;
    const float v = p[row];
    const unsigned y = label[row], yhat = pred[row];
    const int g = group[row];
    if (!(v >= 0.f && v <= 1.f) || y > 1u || yhat > 1u || g < 0 || g >= G) {  // NaN fails both comparisons
      ++bad;
      continue;
    }
    const int bin = min(kEvBins - 1, (int)(v * 4096.0f));
    atomicAdd(&hist[((size_t)g * 2 + y) * kEvBins + bin], 1u);
    const unsigned k = 2 * y + yhat;  // (TN, FP, FN, TP)
    if (g == g0) {
      loc0 += k == 0, loc1 += k == 1, loc2 += k == 2, loc3 += k == 3;
    } else {
      atomicAdd(&conf[(size_t)g * 4 + k], 1u);
    }
  }
  loc0 = wave_sum(loc0), loc1 = wave_sum(loc1), loc2 = wave_sum(loc2), loc3 = wave_sum(loc3), bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0) {
    if (loc0) atomicAdd(&tally[0], loc0);
    if (loc1) atomicAdd(&tally[1], loc1);
    if (loc2) atomicAdd(&tally[2], loc2);
    if (loc3) atomicAdd(&tally[3], loc3);
    if (bad) atomicAdd(&tally[4], bad);
  }
  __syncthreads();
  if (threadIdx.x < 4 && g0 >= 0 && tally[threadIdx.x]) atomicAdd(&conf[(size_t)g0 * 4 + threadIdx.x], tally[threadIdx.x]);
  if (threadIdx.x == 4 && tally[4]) atomicAdd(n_bad, tally[4]);
}

__global__ __launch_bounds__(kEvThreads) void evaluate_bootstrap_kernel(const uint32_t* __restrict__ hist, const uint32_t* __restrict__ conf,
                                                                         int G, uint32_t first, uint32_t k0, uint32_t k1,
                                                                         int64_t* __restrict__ conf_w, int64_t* __restrict__ u2_out,
                                                                         int64_t* __restrict__ n_pos, int64_t* __restrict__ n_neg) {
  extern __shared__ __attribute__((aligned(16))) int32_t ev_lds[];
  int* cnt = ev_lds;                       // [G], padded to a multiple of 4
  int* scan = ev_lds + ((G + 3) & ~3);     // [kEvSeg][kEvWaves] wave totals of the four scans (32 words reserved)
  int* scratch = scan + 32;                // [64] reductions (8-byte aligned: the offsets before it are multiples of 4 words)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;

  ci_draw_counts(cnt, G, first + blockIdx.x, k0, k1);

  // ---- H = sum of the drawn slides' rows, and the weighted confusion counts ----
  uint32_t h[2][kEvSeg][4];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int j = 0; j < kEvSeg; ++j) h[c][j][0] = h[c][j][1] = h[c][j][2] = h[c][j][3] = 0;
  for (int g = 0; g < G; ++g) {
    const uint32_t c = (uint32_t)cnt[g];  // the same word for every lane: a broadcast read, a uniform branch
    if (c == 0) continue;
    const uint4* row = reinterpret_cast<const uint4*>(hist + (size_t)g * 2 * kEvBins) + t;
    uint4 v[2][kEvSeg];
#pragma unroll
    for (int cls = 0; cls < 2; ++cls)
#pragma unroll
      for (int j = 0; j < kEvSeg; ++j) v[cls][j] = row[(cls * kEvBins + j * 4 * kEvThreads) / 4];
#pragma unroll
    for (int cls = 0; cls < 2; ++cls)
#pragma unroll
      for (int j = 0; j < kEvSeg; ++j) {
        h[cls][j][0] += c * v[cls][j].x, h[cls][j][1] += c * v[cls][j].y;
        h[cls][j][2] += c * v[cls][j].z, h[cls][j][3] += c * v[cls][j].w;
      }
  }
  long long cw[4] = {0, 0, 0, 0};
  for (int g = t; g < G; g += kEvThreads) {
    const long long c = cnt[g];
    if (c == 0) continue;
#pragma unroll
    for (int k = 0; k < 4; ++k) cw[k] += c * (long long)conf[(size_t)g * 4 + k];
  }

  // ---- four exclusive scans of the negatives over the threads, one per segment, behind one barrier ----
  uint32_t own[kEvSeg], inc[kEvSeg];
#pragma unroll
  for (int j = 0; j < kEvSeg; ++j) own[j] = inc[j] = h[0][j][0] + h[0][j][1] + h[0][j][2] + h[0][j][3];
#pragma unroll
  for (int j = 0; j < kEvSeg; ++j) inc[j] = wave_scan_incl(inc[j], lane);
  if (lane == 63) {
#pragma unroll
    for (int j = 0; j < kEvSeg; ++j) scan[j * kEvWaves + wave] = (int)inc[j];
  }
  __syncthreads();
  uint32_t carry = 0;  // the negatives of every earlier segment
  long long u2 = 0, pos = 0;
#pragma unroll
  for (int j = 0; j < kEvSeg; ++j) {
    uint32_t off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kEvWaves; ++w) {
      const uint32_t s = (uint32_t)scan[j * kEvWaves + w];
      off += w < wave ? s : 0;
      total += s;
    }
    uint32_t below = carry + off + inc[j] - own[j];  // negatives in the bins before this thread's four of segment j
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t neg = h[0][j][i], ps = h[1][j][i];
      u2 += (long long)ps * (2ll * below + neg);
      pos += ps;
      below += neg;
    }
    carry += total;
  }
  u2 = block_sum<kEvWaves>(u2, scratch);
  pos = block_sum<kEvWaves>(pos, scratch);
#pragma unroll
  for (int k = 0; k < 4; ++k) cw[k] = block_sum<kEvWaves>(cw[k], scratch);
  if (t == 0) {
    u2_out[blockIdx.x] = u2;
    n_pos[blockIdx.x] = pos;
    n_neg[blockIdx.x] = (long long)carry;
#pragma unroll
    for (int k = 0; k < 4; ++k) conf_w[(size_t)blockIdx.x * 4 + k] = cw[k];
  }
}

static size_t ev_lds_bytes(int G) { return (size_t)(((G + 3) & ~3) + kEvScratch) * sizeof(int32_t); }

}  // namespace hipac

extern "C" int hipac_evaluate_abi_version(void) { return HIPAC_EVALUATE_ABI_VERSION; }

extern "C" int hipac_evaluate_accumulate(const float* p, const uint8_t* pred, const uint8_t* label, const int32_t* group, int n, int G,
                                         uint32_t* hist, uint32_t* conf, uint32_t* n_bad, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(n >= 0 && G >= 1 && G <= HIPAC_EVALUATE_MAX_GROUPS, HIPAC_EINVAL, "evaluate_accumulate: n %d, G %d (need n >= 0, 1 <= G <= %d)",
                n, G, HIPAC_EVALUATE_MAX_GROUPS);
  HIPAC_REQUIRE(hist && conf && n_bad && (n == 0 || (p && pred && label && group)), HIPAC_EINVAL, "evaluate_accumulate: null argument");
  HIPAC_REQUIRE(((uintptr_t)hist & 15) == 0, HIPAC_EINVAL, "evaluate_accumulate: hist must be 16-byte aligned");
  if (n == 0) return 0;
  const int runs = (int)(((long long)n + kEvRun - 1) / kEvRun);
  hipLaunchKernelGGL(evaluate_accumulate_kernel, dim3(runs), dim3(kEvThreads), 0, (hipStream_t)stream, p, pred, label, group, n, G, hist,
                     conf, n_bad);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_evaluate_bootstrap(const uint32_t* hist, const uint32_t* conf, int G, uint64_t seed, int64_t first_replicate, int B,
                                        int64_t* conf_w, int64_t* u2, int64_t* n_pos, int64_t* n_neg, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(G >= 1 && G <= HIPAC_EVALUATE_MAX_GROUPS && B >= 1 && B <= HIPAC_EVALUATE_MAX_REPLICATES, HIPAC_EINVAL,
                "evaluate_bootstrap: G %d, B %d (need 1 <= G <= %d, 1 <= B <= %d)", G, B, HIPAC_EVALUATE_MAX_GROUPS,
                HIPAC_EVALUATE_MAX_REPLICATES);
  HIPAC_REQUIRE(hist && conf && conf_w && u2 && n_pos && n_neg, HIPAC_EINVAL, "evaluate_bootstrap: null argument");
  HIPAC_REQUIRE(((uintptr_t)hist & 15) == 0, HIPAC_EINVAL, "evaluate_bootstrap: hist must be 16-byte aligned");
  HIPAC_REQUIRE(first_replicate >= 0 && first_replicate + B <= ((int64_t)1 << 32), HIPAC_EINVAL,
                "evaluate_bootstrap: replicates %lld + %d leave 0 .. 2^32", (long long)first_replicate, B);
  hipLaunchKernelGGL(evaluate_bootstrap_kernel, dim3(B), dim3(kEvThreads), ev_lds_bytes(G), (hipStream_t)stream, hist, conf, G,
                     (uint32_t)first_replicate, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), conf_w, u2, n_pos, n_neg);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

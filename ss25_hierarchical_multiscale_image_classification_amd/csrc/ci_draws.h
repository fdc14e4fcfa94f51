// The draws of a bootstrap replicate (include/hipac_eval_ci.h has the definition; tests/eval_ci_cpu.py restates it in numpy),
// shared by the replicate kernels of eval_ci.hip (cases of the CAMELYON16 evaluation) and evaluate.hip (slides of the patch-level
// evaluation): draw d of replicate r takes word d % 4 of philox4x32_10((d / 4, r, 0, kCiSite), key) and picks (word * S) >> 32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.h"

namespace hipac {

constexpr int kCiThreads = 256;  // threads of a replicate's workgroup
constexpr int kCiSite = 2;       // Philox counter word 3: sites 0 and 1 are the dropout masks

// cnt[s] = how often the S draws of replicate r pick case s (LDS, integer atomics: order-independent); ends with a barrier
__device__ __forceinline__ void ci_draw_counts(int* cnt, int S, uint32_t r, uint32_t k0, uint32_t k1) {
  for (int s = threadIdx.x; s < S; s += kCiThreads) cnt[s] = 0;
  __syncthreads();
  for (int q = threadIdx.x; q * 4 < S; q += kCiThreads) {
    const Philox4 w = philox4x32_10((uint32_t)q, r, 0u, (uint32_t)kCiSite, k0, k1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (q * 4 + i < S) atomicAdd(&cnt[__umulhi(w.w[i], (uint32_t)S)], 1);  // (word * S) >> 32 < S
  }
  __syncthreads();
}

}  // namespace hipac

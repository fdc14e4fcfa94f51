// Device helpers of the MIL head's kernels (mil_train.hip, mil_heads.hip, mil_gated.hip, mil_levels.hip, mil_dropout.hip).
// Every reduction here has one fixed order: the results of the kernels depend on the tiling, never on the run.
#pragma once
#include "common.h"

namespace hipac {

// fixed-order reduction of a 256-thread workgroup (max or sum): shuffle tree inside a wave, the four waves in order through
// red[4] in LDS; every thread gets the result
__device__ __forceinline__ float mil_block_reduce(float v, bool is_max, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) {
    const float t = __shfl_down(v, o, 64);
    v = is_max ? fmaxf(v, t) : v + t;
  }
  __syncthreads();  // red may still be read from a previous call
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < 4; ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
  return r;
}

// butterfly sum over the 64 lanes of a wave; every lane gets the result
__device__ __forceinline__ float mil_wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// u[k][q] = U[k][lane + 64 q], 0 past A: a lane's four hidden units of the K score vectors
template <int K>
__device__ __forceinline__ void mil_load_u(const float* Uw, int A, int lane, float (&u)[K][4]) {
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q) u[k][q] = lane + 64 * q < A ? Uw[k * A + lane + 64 * q] : 0.f;
}

// The four waves' column sums red[4][256 (PLANES + K) + K] of a row sweep, added in wave order and written as one tile's
// (PLANES x [A_pad] | [K][A] | [K]) block of part2
template <int K, int PLANES>
__device__ __forceinline__ void mil_store_part2(const float (*red)[256 * (PLANES + K) + K], int A, int A_pad, int tid,
                                                float* out) {
  for (int e = tid; e < 256 * (PLANES + K) + K; e += 256) {
    const float s = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
    const int blk = e >> 8, j = e & 255;
    if (blk < PLANES) {
      if (j < A_pad) out[blk * A_pad + j] = s;
    } else if (blk < K + PLANES) {
      if (j < A) out[PLANES * A_pad + (blk - PLANES) * A + j] = s;
    } else {
      out[PLANES * A_pad + K * A + j] = s;
    }
  }
}

}  // namespace hipac

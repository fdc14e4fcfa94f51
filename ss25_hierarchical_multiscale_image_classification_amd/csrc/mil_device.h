// Device helpers of the MIL head's K-head kernels (mil_heads.hip, mil_gated.hip, mil_levels.hip): the load of a lane's score
// weights and the store of a row sweep's column sums, the four waves added in wave order.
#pragma once
#include "common.h"

namespace hipac {

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

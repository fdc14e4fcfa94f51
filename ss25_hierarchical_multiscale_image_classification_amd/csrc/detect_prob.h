// The tumour probability of one window from its two-class logits: the one expression both hipac_detect_probs (detect.hip) and
// hipac_tta_reduce (tta.hip) evaluate, so that a reduction over one view equals the plain probabilities bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>

namespace hipac {

// logits: float32[rows][2]; p = 1 / (1 + exp(l_other - l_tumor)) in float32, every operation rounded on its own
__device__ __forceinline__ float tumor_prob(const float* __restrict__ logits, size_t row, int tumor) {
  const float d = logits[2 * row + (1 - tumor)] - logits[2 * row + tumor];
  return 1.0f / (1.0f + expf(d));
}

}  // namespace hipac

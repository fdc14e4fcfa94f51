// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's constants) and the
// dropout mask built on it (include/hipac_mil_dropout.h has the definition; tests/mil_dropout_cpu.py restates it in numpy).
//
// counter = (column / 4, row, sample, site), key = (seed low word, seed high word); output word column % 4 belongs to the
// column, so one call serves the four columns of one 16-byte load.  An element is kept iff its word >= thr.
#pragma once
#include <stdint.h>

namespace hipac {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;  // multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;  // Weyl increments of the key

struct Philox4 {
  uint32_t w[4];
};

__host__ __device__ __forceinline__ uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                          uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = philox_mulhi(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
    const uint32_t hi1 = philox_mulhi(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// What a dropout call needs on the device: thr = floor(p * 2^32) and scale = (float)(1 / (1 - p)), both formed in double
// on the host (0 <= p < 1, so thr fits 32 bits and p = 0 gives thr = 0: every word is kept, scale is exactly 1).
struct DropoutSpec {
  uint32_t k0, k1, thr;
  float scale;
};

static inline DropoutSpec make_dropout_spec(double p, uint64_t seed) {
  DropoutSpec d;
  d.k0 = (uint32_t)(seed & 0xFFFFFFFFull);
  d.k1 = (uint32_t)(seed >> 32);
  d.thr = (uint32_t)(uint64_t)(p * 4294967296.0);  // p >= 0: the conversion truncates = floor
  d.scale = (float)(1.0 / (1.0 - p));
  return d;
}

// the four words of columns 4 * quad .. 4 * quad + 3 of (row, sample, site)
__device__ __forceinline__ Philox4 dropout_words(const DropoutSpec& d, uint32_t quad, uint32_t row, uint32_t sample, uint32_t site) {
  return philox4x32_10(quad, row, sample, site, d.k0, d.k1);
}

// one element: the kept value is fl32(x * scale), a dropped one is +0
__device__ __forceinline__ float dropout_apply(float x, uint32_t word, const DropoutSpec& d) {
  return word >= d.thr ? x * d.scale : 0.f;
}

}  // namespace hipac

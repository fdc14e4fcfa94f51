// The unfused stem's max-pool (single values / pairs) and the uint8 -> fp32 NHWC4 input conversion of the pair modes.
#pragma once
#include <type_traits>
#include "conv_device.h"

namespace hipac {

// 3x3/2 max-pool, pad 1, NHWC, 8 channels (16 B) per thread.  Inputs are
// post-ReLU (>= 0) so the implicit -inf padding never wins; out-of-range taps
// are simply skipped.
template <typename T>
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                           int n) {
  constexpr int HI = 112, WI = 112, HO = 56, WO = 56, C = 64;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)n * HO * WO * (C / 8);
  if (gid >= total) return;
  const int c8 = (int)(gid % (C / 8));
  long long p = gid / (C / 8);
  const int ow = (int)(p % WO);
  p /= WO;
  const int oh = (int)(p % HO);
  const int b = (int)(p / HO);
  using frag = typename Elem<T>::frag;
  float best[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) best[e] = -3.0e38f;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const int ih = oh * 2 - 1 + dy;
    if ((unsigned)ih >= (unsigned)HI) continue;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int iw = ow * 2 - 1 + dx;
      if ((unsigned)iw >= (unsigned)WI) continue;
      const frag v = *reinterpret_cast<const frag*>(in + (((size_t)b * HI + ih) * WI + iw) * C + c8 * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) best[e] = fmaxf(best[e], (float)v[e]);
    }
  }
  frag o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (T)best[e];
  *reinterpret_cast<frag*>(out + (((size_t)b * HO + oh) * WO + ow) * C + c8 * 8) = o;
}

// fp16x3 mode: the same max-pool over the fp32 stem map (exact f32 MFMA), written as (hi, lo) fp16 pairs
// [n,56,56, hi: 64 | lo: 64]
template <typename TO>  // (a template only so that the header can be included from several translation units)
__global__ __launch_bounds__(256) void maxpool3x3s2_split_kernel(const float* __restrict__ in, TO* __restrict__ out,
                                                                 int n) {
  static_assert(std::is_same<TO, _Float16>::value, "pairs are fp16");
  constexpr int HI = 112, WI = 112, HO = 56, WO = 56, C = 64;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)n * HO * WO * (C / 8);
  if (gid >= total) return;
  const int c8 = (int)(gid % (C / 8));
  long long p = gid / (C / 8);
  const int ow = (int)(p % WO);
  p /= WO;
  const int oh = (int)(p % HO);
  const int b = (int)(p / HO);
  float best[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) best[e] = -3.0e38f;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const int ih = oh * 2 - 1 + dy;
    if ((unsigned)ih >= (unsigned)HI) continue;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int iw = ow * 2 - 1 + dx;
      if ((unsigned)iw >= (unsigned)WI) continue;
      const float* src = in + (((size_t)b * HI + ih) * WI + iw) * C + c8 * 8;
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) best[e] = fmaxf(best[e], v0[e]), best[4 + e] = fmaxf(best[4 + e], v1[e]);
    }
  }
  f16x8 oh8, ol8;
  split_pair8(best, oh8, ol8);
  _Float16* dst = out + (((size_t)b * HO + oh) * WO + ow) * (2 * C) + c8 * 8;
  *reinterpret_cast<f16x8*>(dst) = oh8;
  *reinterpret_cast<f16x8*>(dst + C) = ol8;
}

// fp16x3 mode, uint8 input: raw HWC patches -> the zero-padded fp32 NHWC4 tensor [n,230,232,4] through the fp32
// ToTensor / Normalize table (exactly the reference's (v/255 - mean)/std per byte value, src/main.py:815-816)
template <typename TO>
__global__ __launch_bounds__(256) void u8_to_nhwc4_f32_kernel(const unsigned char* __restrict__ x,
                                                              const float* __restrict__ lut, TO* __restrict__ out,
                                                              int n) {
  static_assert(std::is_same<TO, float>::value, "fp32 stem input");
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)n * kPadH * kPadW;
  if (gid >= total) return;
  const int px = (int)(gid % kPadW);
  const long long t = gid / kPadW;
  const int py = (int)(t % kPadH);
  const int b = (int)(t / kPadH);
  const int y = py - 3, xx = px - 3;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if ((unsigned)y < (unsigned)kPatch && (unsigned)xx < (unsigned)kPatch) {
    const unsigned char* src = x + (((size_t)b * kPatch + y) * kPatch + xx) * 3;
    v[0] = lut[src[0]];
    v[1] = lut[256 + src[1]];
    v[2] = lut[512 + src[2]];
  }
  *reinterpret_cast<f32x4*>(out + (size_t)gid * 4) = v;
}

}  // namespace hipac

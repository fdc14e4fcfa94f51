// The small kernels around the ResNet18 trunk: input conversion, the two heads (global average pool, fc, argmax) and
// the test-only tap export, with their launchers.
#include "resnet_handle.h"
#include "wave_reduce.h"

namespace hipac {

// float32 NCHW [n,3,224,224] -> T NHWC4 zero-padded [n,230,232,4]
template <typename T>
__global__ __launch_bounds__(256) void nchw_to_nhwc4_kernel(const float* __restrict__ x, T* __restrict__ out,
                                                            int n) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)n * kPadH * kPadW;
  if (gid >= total) return;
  const int px = (int)(gid % kPadW);
  const long long t = gid / kPadW;
  const int py = (int)(t % kPadH);
  const int b = (int)(t / kPadH);
  const int y = py - 3, xx = px - 3;
  typename Elem<T>::vec4 v;
  v[0] = v[1] = v[2] = v[3] = (T)0.f;
  if ((unsigned)y < (unsigned)kPatch && (unsigned)xx < (unsigned)kPatch) {
    const size_t plane = (size_t)kPatch * kPatch;
    const float* src = x + (size_t)b * 3 * plane + (size_t)y * kPatch + xx;
    v[0] = (T)src[0];
    v[1] = (T)src[plane];
    v[2] = (T)src[2 * plane];
  }
  *reinterpret_cast<typename Elem<T>::vec4*>(out + (size_t)gid * 4) = v;
}

int launch_nchw_to_nhwc4(const float* x, void* out, int n, int precision, hipStream_t s) {
  const long long total = (long long)n * kPadH * kPadW;
  const unsigned grid = (unsigned)((total + 255) / 256);
  if (precision == HIPAC_PREC_BF16)
    hipLaunchKernelGGL((nchw_to_nhwc4_kernel<__bf16>), dim3(grid), dim3(256), 0, s, x, (__bf16*)out, n);
  else if (precision == HIPAC_PREC_FP16)
    hipLaunchKernelGGL((nchw_to_nhwc4_kernel<_Float16>), dim3(grid), dim3(256), 0, s, x, (_Float16*)out, n);
  else  // fp32 and the pair modes: their stem runs on fp32 input
    hipLaunchKernelGGL((nchw_to_nhwc4_kernel<float>), dim3(grid), dim3(256), 0, s, x, (float*)out, n);
  return (int)hipGetLastError();
}

// What both heads do with the pooled features (f0, f1) = channels (2 tid, 2 tid + 1) of image b: store them, optional
// fc -> logits[n,C], optional argmax.  One 256-thread workgroup per image.
__device__ __forceinline__ void head_tail(float f0, float f1, int b, int tid, const float* __restrict__ fc_w,
                                          const float* __restrict__ fc_b, int num_classes, float* __restrict__ feats,
                                          float* __restrict__ logits, long long* __restrict__ labels) {
  __shared__ float red[4][16];
  __shared__ float lg[16];
  if (feats) *reinterpret_cast<float2*>(feats + (size_t)b * 512 + tid * 2) = make_float2(f0, f1);
  if (num_classes <= 0 || (!logits && !labels)) return;
  for (int j = 0; j < num_classes; ++j) {
    const float2 w = *reinterpret_cast<const float2*>(fc_w + (size_t)j * 512 + tid * 2);
    const float v = wave_sum_tree(f0 * w.x + f1 * w.y);
    if ((tid & 63) == 0) red[tid >> 6][j] = v;
  }
  __syncthreads();
  if (tid < num_classes) {
    const float v = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid] + fc_b[tid];
    lg[tid] = v;
    if (logits) logits[(size_t)b * num_classes + tid] = v;
  }
  __syncthreads();
  if (tid == 0 && labels) {
    int best = 0;
    float bv = lg[0];
    for (int j = 1; j < num_classes; ++j)
      if (lg[j] > bv) {  // strict: first maximum wins, as torch.argmax
        bv = lg[j];
        best = j;
      }
    labels[b] = best;
  }
}

// Global average pool over the 7x7 map of the last block (float32 NHWC [n,49,512]) -> feats[n,512], then head_tail.
// Two channels per thread.
__global__ __launch_bounds__(256) void head_kernel(const float* __restrict__ last, const float* __restrict__ fc_w,
                                                   const float* __restrict__ fc_b, int num_classes,
                                                   float* __restrict__ feats, float* __restrict__ logits,
                                                   long long* __restrict__ labels) {
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const float* src = last + (size_t)b * 49 * 512 + tid * 2;
  float s0 = 0.f, s1 = 0.f;
#pragma unroll 7
  for (int p = 0; p < 49; ++p) {
    const float2 v = *reinterpret_cast<const float2*>(src + (size_t)p * 512);
    s0 += v.x;
    s1 += v.y;
  }
  head_tail(s0 / 49.0f, s1 / 49.0f, b, tid, fc_w, fc_b, num_classes, feats, logits, labels);
}

// The same head over the partial sums the last conv's pooled epilogue leaves (halo16.h, POOL): image b = pixels
// [49 b, 49 b + 48] of the flattened 7x7 maps meets at most two 256-pixel tiles mt and both 128-pixel wave halves wm of
// each; part[mt][wm][slot = b - (256 mt) / 49][2][512] = (sum of the pixel values rounded to the grid 2^-10, sum of the
// remainders on the grid 2^-29): both sums are EXACT in fp32 (halo16.h), so the features do not depend on how the image's
// pixels were spread over lanes, waves and tiles -- the same patch gives the same bits at any position of any batch.
// Only the (mt, wm) pairs that overlap the image are read (slots a wave never met are not written).
__global__ __launch_bounds__(256) void head_pool_kernel(const float* __restrict__ part, const float* __restrict__ fc_w,
                                                        const float* __restrict__ fc_b, int num_classes,
                                                        float* __restrict__ feats, float* __restrict__ logits,
                                                        long long* __restrict__ labels) {
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int p0 = 49 * b, p1 = p0 + 48;
  float h0 = 0.f, h1 = 0.f, l0 = 0.f, l1 = 0.f;  // exact sums (grid 2^-10 parts, grid 2^-29 remainders): any order gives these bits
  for (int mt = p0 >> 8; mt <= (p1 >> 8); ++mt)
    for (int wm = 0; wm < 2; ++wm) {
      const int w0 = mt * 256 + wm * 128;
      if (w0 + 127 < p0 || w0 > p1) continue;  // this wave half holds no pixel of the image
      const int slot = b - (mt * 256) / 49;
      const float* src = part + (((size_t)(mt * 2 + wm) * 7 + slot) * 2) * 512 + tid * 2;
      const float2 vh = *reinterpret_cast<const float2*>(src), vl = *reinterpret_cast<const float2*>(src + 512);
      h0 += vh.x, h1 += vh.y;
      l0 += vl.x, l1 += vl.y;
    }
  head_tail((h0 + l0) / 49.0f, (h1 + l1) / 49.0f, b, tid, fc_w, fc_b, num_classes, feats, logits, labels);
}

int launch_head_pool(const float* part, int n, const float* fc_w, const float* fc_b, int num_classes, float* feats,
                     float* logits, int64_t* labels, hipStream_t s) {
  hipLaunchKernelGGL(head_pool_kernel, dim3(n), dim3(256), 0, s, part, fc_w, fc_b, num_classes, feats, logits,
                     (long long*)labels);
  return (int)hipGetLastError();
}

int launch_head(const float* last, int n, const float* fc_w, const float* fc_b, int num_classes, float* feats,
                float* logits, int64_t* labels, hipStream_t s) {
  hipLaunchKernelGGL(head_kernel, dim3(n), dim3(256), 0, s, last, fc_w, fc_b, num_classes, feats, logits,
                     (long long*)labels);
  return (int)hipGetLastError();
}

// NHWC -> NCHW float32, test tap only.  PAIRS = false: src is T[pixel][C]; PAIRS = true (the pair modes): src is
// [pixel][hi: C | lo: C] and the element is hi + lo (exact in fp32).
template <typename T, bool PAIRS>
__global__ __launch_bounds__(256) void tap_export_kernel(const T* __restrict__ src, float* __restrict__ dst, int n,
                                                         int C, int H, int W) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)n * C * H * W;
  if (gid >= total) return;
  const int c = (int)(gid % C);
  long long t = gid / C;
  const int w = (int)(t % W);
  t /= W;
  const int h = (int)(t % H);
  const int b = (int)(t / H);
  float v;
  if constexpr (PAIRS) {
    const T* px = src + (gid / C) * (2 * C);
    v = (float)px[c] + (float)px[C + c];
  } else {
    v = (float)src[gid];
  }
  dst[(((size_t)b * C + c) * H + h) * W + w] = v;
}

int launch_tap_export(const void* src, int is_f32, int precision, int n, int C, int H, int W, float* dst,
                      hipStream_t s) {
  const long long total = (long long)n * C * H * W;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (!is_f32 && pair_mode(precision))
    hipLaunchKernelGGL((tap_export_kernel<_Float16, true>), grid, block, 0, s, (const _Float16*)src, dst, n, C, H, W);
  else if (is_f32 || precision == HIPAC_PREC_FP32)
    hipLaunchKernelGGL((tap_export_kernel<float, false>), grid, block, 0, s, (const float*)src, dst, n, C, H, W);
  else if (precision == HIPAC_PREC_BF16)
    hipLaunchKernelGGL((tap_export_kernel<__bf16, false>), grid, block, 0, s, (const __bf16*)src, dst, n, C, H, W);
  else
    hipLaunchKernelGGL((tap_export_kernel<_Float16, false>), grid, block, 0, s, (const _Float16*)src, dst, n, C, H, W);
  return (int)hipGetLastError();
}

}  // namespace hipac

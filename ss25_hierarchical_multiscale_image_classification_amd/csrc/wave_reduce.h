// Wave and workgroup reductions and scans of the small kernels (evaluation, MIL, validation, preprocessing, stain, tissue,
// PNG, deflate, NT-Xent, the training head).  Device functions only; the one place where their contract is written down.
//
// Wave level: the 64 lanes of a wave, no LDS, no barrier; every lane of the wave must make the call.
//   wave_sum / wave_max / wave_min   xor butterfly, distances 32, 16, ..., 1.  Both partners of a stage form the same value, so
//                                    every lane ends with the result, bit for bit the same.
//   wave_umax                        the same butterfly with max over an unsigned integer type (32 or 64 bits).
//   wave_sum_tree / wave_max_tree    __shfl_down tree, distances 32, 16, ..., 1.  The result is defined in lane 0 only.  Stage
//                                    by stage lane 0 combines the same two partial results as in the butterfly, so it holds the
//                                    same bits; the other lanes do not.  A site keeps the form it was written with.
//   wave_scan_incl                   inclusive prefix sum over the lanes (__shfl_up, distances 1, 2, ..., 32).
// For floats the order is part of the result.  Lane 0 ends with t_1[0], where t_32[l] = v[l] op v[l + 32] and
// t_d[l] = t_2d[l] op t_2d[l + d]: a balanced tree over the lanes, the partner of a stage d lanes up.
//
// Workgroup level: WAVES waves of 64 threads (every user today: 256 threads, WAVES = 4); every thread must make the call and
// every thread gets the result.  Lane 0 of wave w writes its wave's result r_w to scratch[w]; after a barrier every thread
// combines them in wave order, ((r_0 op r_1) op r_2) op r_3; a second barrier ends the call.
//   block_sum / block_min            integers; butterfly inside the wave.
//   block_umax                       unsigned integers, 32 or 64 bits; butterfly inside the wave.
//   block_sum_tree / block_max_tree  tree inside the wave; the fixed-order reduction of the float kernels (sum or max).
//   block_scan_excl                  exclusive prefix sum of one integer per thread in thread order, and the workgroup's total
//                                    (the waves' totals go through the scratch: lane 63 writes).
// Scratch contract, the same for all of them: the caller passes LDS scratch of WAVES values of the reduced type (aligned for
// it); nothing else touches it during the call; it is free again on return, so consecutive calls may share it and the caller
// needs no barrier of its own between them.  Every call is also a workgroup barrier for whatever the caller wrote before it.
//
// Where a kernel exchanges something of its own through LDS -- several values per wave, a layout of partial sums, a carry --
// it calls the wave primitives and keeps that exchange.
//
// Seen and left as they are: the conv and stem kernels (stem.h, halo16.h, halo16x2.h, layer1_c64.h, block16_c64.h), the 16-lane
// scan of tile_place.h, the 32-lane segments of train_kernels.h, the segmented scan of level_planes.hip, the column reductions
// vd_wg_reduce_store (validate.hip) and mil_store_part2 (mil_device.h), and the score loop of mil_heads.hip's mh_score_kernel
// (a call costs its K = 1 instantiation a register).
#pragma once
#include "common.h"

namespace hipac {

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

template <class T>
__device__ __forceinline__ T wave_umax(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

template <class T>
__device__ __forceinline__ T wave_sum_tree(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__device__ __forceinline__ float wave_max_tree(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, 64));
  return v;
}

template <class T>
__device__ __forceinline__ T wave_scan_incl(T v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// the wave results r (lane 0's value counts) through scratch[WAVES], combined in wave order
template <int WAVES, class T, class Op>
__device__ __forceinline__ T block_combine(T r, void* scratch, Op op) {
  T* s = static_cast<T*>(scratch);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = r;
  __syncthreads();
  T t = s[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) t = op(t, s[w]);
  __syncthreads();  // scratch is free again
  return t;
}

template <int WAVES, class T>
__device__ __forceinline__ T block_sum(T v, void* scratch) {
  return block_combine<WAVES>(wave_sum(v), scratch, [](T a, T b) { return a + b; });
}

template <int WAVES>
__device__ __forceinline__ int block_min(int v, void* scratch) {
  return block_combine<WAVES>(wave_min(v), scratch, [](int a, int b) { return min(a, b); });
}

template <int WAVES, class T>
__device__ __forceinline__ T block_umax(T v, void* scratch) {
  return block_combine<WAVES>(wave_umax(v), scratch, [](T a, T b) { return a > b ? a : b; });
}

template <int WAVES, class T>
__device__ __forceinline__ T block_sum_tree(T v, void* scratch) {
  return block_combine<WAVES>(wave_sum_tree(v), scratch, [](T a, T b) { return a + b; });
}

template <int WAVES>
__device__ __forceinline__ float block_max_tree(float v, void* scratch) {
  return block_combine<WAVES>(wave_max_tree(v), scratch, [](float a, float b) { return fmaxf(a, b); });
}

template <int WAVES, class T>
__device__ __forceinline__ T block_scan_excl(T v, void* scratch, T& total) {
  T* s = static_cast<T*>(scratch);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T inc = wave_scan_incl(v, lane);
  if (lane == 63) s[wave] = inc;
  __syncthreads();
  T off = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const T sw = s[w];
    off += w < wave ? sw : 0;
    total += sw;
  }
  __syncthreads();  // scratch is free again
  return off + inc - v;
}

}  // namespace hipac

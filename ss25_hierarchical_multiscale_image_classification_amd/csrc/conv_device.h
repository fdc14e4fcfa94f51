// Device helpers shared by the convolution kernels (gfx950): short vector types, buffer-descriptor LDS-DMA, packing of
// value pairs, the counted vector-memory wait, the developer stamps and the band geometry of the halo kernels.
#pragma once
#include "common.h"

namespace hipac {

typedef __attribute__((ext_vector_type(2))) unsigned short u16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

// Buffer-descriptor LDS-DMA: 16 bytes per lane from base + voffset (VGPR, range-checked against the
// descriptor's size: out of range reads as zeros) + soffset (SGPR, not range-checked) into
// lds_base + lane * 16.  The builtins exist only in the device pass; the host pass needs the kernel
// templates to parse so that their launch stubs are emitted.
#if defined(__HIP_DEVICE_COMPILE__)
using rsrc_t = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ void buffer_load_lds16(rsrc_t rs, void* lds, int voffset, int soffset) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds, 16, voffset, soffset, 0, 0);
}
#else
struct rsrc_t {};
__device__ inline rsrc_t make_rsrc(const void*, int) { return {}; }
__device__ inline void buffer_load_lds16(rsrc_t, void*, int, int) {}
#endif

template <typename T> struct PackPair;  // two exactly representable floats -> one dword of two T (lo, hi)
template <> struct PackPair<_Float16> {
  static __device__ __forceinline__ unsigned pack(float lo, float hi) {
    return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(lo, hi));  // exact inputs: the rounding mode is moot
  }
  static __device__ __forceinline__ unsigned pack_rn(float lo, float hi) {
    // round-to-nearest-even, as every other store of T in this library; one packed conversion
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, f16x2));
  }
};
template <> struct PackPair<__bf16> {
  static __device__ __forceinline__ unsigned pack(float lo, float hi) {
    return __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, hi), __builtin_bit_cast(unsigned, lo), 0x07060302u);
  }
  static __device__ __forceinline__ unsigned pack_rn(float lo, float hi) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
  }
};

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void permlane32_swap(unsigned& a, unsigned& b) {  // a.upper <-> b.lower (32-lane rows)
  const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
  a = r[0];
  b = r[1];
}
#else
__device__ inline void permlane32_swap(unsigned&, unsigned&) {}
#endif

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// fp32 -> (hi, lo) pair of fp16 fragments (the pair layout of precision fp16x3: hi = rn16(v), lo = rn16(v - hi))
__device__ __forceinline__ void split_pair8(const float* v, f16x8& hi, f16x8& lo) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    hi[e] = (_Float16)v[e];
    lo[e] = (_Float16)(v[e] - (float)hi[e]);
  }
}

#ifdef HIPAC_HALO_STAMPS
// developer build: per-phase cycle totals of the halo kernel (s_memtime), summed over workgroups
static __device__ unsigned long long g_halo_stamps[8];
#define HALO_STAMP(var) const unsigned long long var = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_s_waitcnt(0xC07F)
#else
#define HALO_STAMP(var)
#endif

// ---------------------------------------------------------------------------------------
// Halo direct convolution for the 3x3 / stride 1 / pad 1 layers (13 of the 20 convs, 83 % of
// the FLOPs; the kernels are in halo16.h and halo16x2.h).  conv_glds_kernel re-stages the
// activation tile once per filter tap (9x the input through L2 -> LDS, which is what bounds it
// at ~11 TB/s); here a workgroup brings the input rows its BM output pixels need -- a band of
// zero-padded rows, 64 channels deep -- into LDS ONCE per 64-channel chunk and all 9 taps read
// it at shifted pixel offsets.  Only the weight tile (BN x 64 channels per tap) still streams,
// through an LDS-DMA ring one tap ahead of the MFMAs.
//
// Geometry: NHWC activations flattened over (image, row, col) are one pixel array m; tap
// (kh,kw) of output pixel m reads pixel m + (kh-1)*W + (kw-1) unless that falls outside the
// image (x or y edge), where it reads zeros.  So the band a workgroup needs is simply the
// CONTIGUOUS pixel range [m0 - W - 1, mlast + W + 1] (it may run into neighbouring images;
// those pixels are never selected because the edge flags redirect such taps).  In LDS:
// slots 0 and 1 = pixels of zeros, slot q >= 2 = pixel m0 - W - 3 + q, [slot][64 ch] with the
// chunk swizzle of conv_glds.h (c ^ ((q >> 1) & 7)).  Consecutive output pixels sit in consecutive slots,
// so a ds_read_b128 lane group covers all 16 bank groups of the 256-byte bank row; an edge tap
// reads the zero slot of its own parity at its own swizzled chunk, which keeps that property
// (measured before this: 21-29 % of LDS cycles lost to bank conflicts from a single zero slot).
// No per-piece div/mod, no pad rows: BM + 2W + 2 pixels per band.
// ---------------------------------------------------------------------------------------
#ifndef HIPAC_HALO_TAP_UNROLL
#define HIPAC_HALO_TAP_UNROLL 3  // taps per unrolled group: 3 makes kw a constant (9 is slower: 2x, code size)
#endif
#ifndef HIPAC_HALO_GRID
#define HIPAC_HALO_GRID 512  // persistent halo workgroups: 2 per CU x 256 CUs
#endif
constexpr int halo_band_pieces(int W, int BM) { return (BM + 2 * W + 2 + 2 + 7) / 8; }  // 8-pixel (1 KB) pieces

}  // namespace hipac

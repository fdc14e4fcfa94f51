// conv_igemm_kernel ("v1"): implicit-GEMM convolution on MFMA for the ResNet18 trunk (gfx950) -- the stem, every
// layer of the fp32 parity mode and the fp32 training step.
//
// Data layout: activations NHWC in T (bf16 | fp16), weights [Cout][kh][kw][Cin]
// with BatchNorm folded in, fp32 bias per Cout.  The GEMM is
//     D[cout][pixel] = sum_k W[cout][k] * X[pixel][k],   k = (kh, kw, cin)
// with the WEIGHTS as the MFMA "A" operand and the ACTIVATIONS as "B", so that
// in the 32x32 accumulator tile each lane owns one output pixel (lane & 31) and
// runs of 4 consecutive output channels in its registers: the NHWC store is then
// 8 bytes of consecutive channels per lane instead of 2-byte scalars.
//
// Tile: 128 output pixels x BN output channels per 256-thread workgroup
// (4 waves as 2 pixel-halves x 2 channel-halves), K stepped in tiles of one
// filter tap x 64 input channels (one 128-byte pixel run per row), staged through
// LDS with 16-byte pads (row stride 144 B => ds_read_b128 conflict-free) and
// register prefetch of the next K tile behind the MFMAs of the current one.
//
// The 7x7/2 stem reads the pre-padded NHWC4 image: for a fixed kh the 7 taps x 4
// channels of one output pixel are 56 contiguous bytes, so K = 7 tiles of 32
// (28 real + 4 zero-weight) elements and no bounds checks are needed.
#pragma once
#include "conv_device.h"

namespace hipac {

// TKH / TKW / UPS: the parity-class data gradient of a stride-2 convolution (training), see conv_glds_kernel's note: the input is the
// gradient on the coarse grid, the window TKH x TKW taps starting at the output pixel, no padding, output pixel (y, x) stored at
// (2y + PY, 2x + PX) of the fine grid, UPS = 4 | PY << 1 | PX.
template <typename T, int CIN, int COUT, int HI, int WI, int KS, int STRIDE, int BN, bool RELU,
          bool RESID, bool OUTF32, bool STEM, int TKH = 0, int TKW = 0, int UPS = 0>
__global__ __launch_bounds__(256) void conv_igemm_kernel(const T* __restrict__ in,
                                                         const T* __restrict__ wgt,
                                                         const float* __restrict__ bias,
                                                         const T* __restrict__ resid,
                                                         void* __restrict__ outp, int M) {
  using E = Elem<T>;
  using frag = typename E::frag;
  constexpr int KH = UPS ? TKH : KS, KW = UPS ? TKW : KS;
  constexpr int PAD = (STEM || UPS) ? 0 : KS / 2;
  constexpr int HO = STEM ? 112 : (UPS ? HI : (HI + 2 * PAD - KS) / STRIDE + 1);
  constexpr int WO = STEM ? 112 : (UPS ? WI : (WI + 2 * PAD - KS) / STRIDE + 1);
  static_assert(!UPS || (!STEM && STRIDE == 1 && TKH >= 1 && TKW >= 1 && !RESID), "parity-class data gradient");
  constexpr int BK = STEM ? 32 : 64;
  constexpr int KT = STEM ? 7 : KH * KW * (CIN / 64);
  constexpr int KTOT = KT * BK;
  constexpr int EPC = 16 / (int)sizeof(T);  // elements per 16-byte chunk: 8 (bf16/fp16) or 4 (fp32)
  constexpr int LDA = BK + EPC;             // LDS row padded by one chunk, elements
  constexpr int CH = BK / EPC;              // 16-byte chunks per row
  constexpr int BM = 128;
  constexpr int RPP = 256 / CH;       // rows covered per pass of the 256 threads
  constexpr int APT = BM / RPP;       // A pieces per thread
  constexpr int WPT = BN / RPP;       // W pieces per thread
  constexpr int NT = BN / 64;         // 32-wide cout tiles per wave
  constexpr int CC = STEM ? 1 : CIN / 64;
  static_assert(BN % 64 == 0 && COUT % BN == 0, "BN");
  static_assert(WPT >= 1, "WPT");

  __shared__ __attribute__((aligned(16))) T smem[(BM + BN) * LDA];
  T* As = smem;
  T* Ws = smem + BM * LDA;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int r = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;

  // ---- per-thread staging rows -------------------------------------------------
  const int chunk = tid % CH;
  const int row0 = tid / CH;
  int a_base[APT];   // element offset of tap (0,0) for this row (+chunk*8)
  int a_ih0[APT], a_iw0[APT];
  bool a_ok[APT];
#pragma unroll
  for (int i = 0; i < APT; ++i) {
    const int m = m0 + row0 + i * RPP;
    a_ok[i] = m < M;
    const int mm = a_ok[i] ? m : 0;
    const int b = mm / (HO * WO);
    const int rem = mm - b * (HO * WO);
    const int oh = rem / WO;
    const int ow = rem - oh * WO;
    if constexpr (STEM) {
      a_ih0[i] = 0;
      a_iw0[i] = 0;
      a_base[i] = ((b * kPadH + 2 * oh) * kPadW + 2 * ow) * 4 + chunk * EPC;
    } else {
      a_ih0[i] = oh * STRIDE - PAD;
      a_iw0[i] = ow * STRIDE - PAD;
      a_base[i] = ((b * HI + a_ih0[i]) * WI + a_iw0[i]) * CIN + chunk * EPC;
    }
  }
  const T* wsrc = wgt + (size_t)(n0 + row0) * KTOT + chunk * EPC;

  u32x4 areg[APT], wreg[WPT];  // native vectors: HIP's uint4 struct copies lower to memcpy and land in scratch
  // Branch-free staging: out-of-image taps load from offset 0 and are zeroed by
  // a select; the prefetch past the last K tile wraps to tile 0 (loaded, never used).
  auto gload = [&](int kh_, int kw_, int cc_, int t_) {
    static_for<APT>([&](auto I) {
      constexpr int i = decltype(I)::value;
      bool ok = a_ok[i];
      int off;
      if constexpr (STEM) {
        off = a_base[i] + kh_ * (kPadW * 4);
      } else {
        ok = ok && (unsigned)(a_ih0[i] + kh_) < (unsigned)HI && (unsigned)(a_iw0[i] + kw_) < (unsigned)WI;
        off = a_base[i] + (kh_ * WI + kw_) * CIN + cc_ * 64;
      }
      const u32x4 v = *reinterpret_cast<const u32x4*>(in + (ok ? off : 0));
      areg[i] = ok ? v : u32x4{0u, 0u, 0u, 0u};
    });
    static_for<WPT>([&](auto I) {
      constexpr int i = decltype(I)::value;
      wreg[i] = *reinterpret_cast<const u32x4*>(wsrc + (size_t)i * RPP * KTOT + t_ * BK);
    });
  };

  f32x16 acc[2][NT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const T* a_rd = As + (wm * 64 + r) * LDA + 8 * h;
  const T* w_rd = Ws + (wn * (BN / 2) + r) * LDA + 8 * h;

  int kh = 0, kw = 0, cc = 0;
  gload(0, 0, 0, 0);
  for (int t = 0; t < KT; ++t) {
    static_for<APT>([&](auto I) {
      constexpr int i = decltype(I)::value;
      *reinterpret_cast<u32x4*>(As + (row0 + i * RPP) * LDA + chunk * EPC) = areg[i];
    });
    static_for<WPT>([&](auto I) {
      constexpr int i = decltype(I)::value;
      *reinterpret_cast<u32x4*>(Ws + (row0 + i * RPP) * LDA + chunk * EPC) = wreg[i];
    });
    __syncthreads();
    // advance (kh, kw, cc) to tile t+1 and prefetch it behind the MFMAs
    if (++cc == CC) {
      cc = 0;
      if constexpr (STEM) {
        ++kh;
      } else if (++kw == KW) {
        kw = 0;
        ++kh;
      }
    }
    {
      const bool more = t + 1 < KT;
      const int kh_n = more ? kh : 0, kw_n = more ? kw : 0, cc_n = more ? cc : 0, t_n = more ? t + 1 : 0;
      gload(kh_n, kw_n, cc_n, t_n);
    }
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      frag af[2], wf[NT];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const frag*>(a_rd + i * 32 * LDA + kk * 16);
#pragma unroll
      for (int j = 0; j < NT; ++j) wf[j] = *reinterpret_cast<const frag*>(w_rd + j * 32 * LDA + kk * 16);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = E::mfma(wf[j], af[i], acc[i][j]);
    }
    __syncthreads();
  }

  // ---- epilogue: +bias (+residual) (ReLU) -> NHWC store ---------------------------
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + wm * 64 + i * 32 + r;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = n0 + wn * (BN / 2) + j * 32 + 8 * q + 4 * h;
        const float4 bv = *reinterpret_cast<const float4*>(bias + c0);
        float v0 = acc[i][j][4 * q + 0] + bv.x;
        float v1 = acc[i][j][4 * q + 1] + bv.y;
        float v2 = acc[i][j][4 * q + 2] + bv.z;
        float v3 = acc[i][j][4 * q + 3] + bv.w;
        size_t o = (size_t)m * COUT + c0;
        if constexpr (UPS != 0) {  // coarse pixel m = (b, y, x) -> fine position (2y + PY, 2x + PX)
          const int ub = m / (HO * WO), urem = m - ub * (HO * WO), uy = urem / WO, ux = urem - uy * WO;
          o = ((size_t)(ub * 2 * HO + 2 * uy + ((UPS >> 1) & 1)) * (2 * WO) + 2 * ux + (UPS & 1)) * COUT + c0;
        }
        if constexpr (RESID) {
          const typename E::vec4 rv = *reinterpret_cast<const typename E::vec4*>(resid + o);
          v0 += (float)rv[0];
          v1 += (float)rv[1];
          v2 += (float)rv[2];
          v3 += (float)rv[3];
        }
        if constexpr (RELU) {
          v0 = fmaxf(v0, 0.f);
          v1 = fmaxf(v1, 0.f);
          v2 = fmaxf(v2, 0.f);
          v3 = fmaxf(v3, 0.f);
        }
        if constexpr (OUTF32) {
          *reinterpret_cast<float4*>(reinterpret_cast<float*>(outp) + o) = make_float4(v0, v1, v2, v3);
        } else {
          typename E::vec4 ov;
          ov[0] = (T)v0;
          ov[1] = (T)v1;
          ov[2] = (T)v2;
          ov[3] = (T)v3;
          *reinterpret_cast<typename E::vec4*>(reinterpret_cast<T*>(outp) + o) = ov;
        }
      }
    }
  }
}

}  // namespace hipac

// ---------------------------------------------------------------------------------------
// conv_glds_kernel ("v2"): LDS-DMA ring.  Same GEMM, operand roles and epilogue as conv_igemm_kernel
// (conv_v1.h), but the K tiles
// (one filter tap x 64 input channels: 128-byte rows) are brought in by
// global_load_lds_dwordx4 (1 KiB = 8 rows per wave-instruction) into an NSTAGE-deep LDS
// ring that stays NSTAGE-1 tiles ahead of the MFMAs: counted s_waitcnt vmcnt(N), ONE raw
// s_barrier per K tile, no VGPRs spent on staging.  The LDS image is lane-linear (as the
// DMA requires), so the bank-conflict swizzle lives on the SOURCE address and on the read:
// 16-byte chunk c of row R sits at chunk c ^ ((R >> 1) & 7)  (ds_read_b128 conflict-free:
// within a 16-lane group (R & 1, (R >> 1) & 7) is unique).  Out-of-image taps read a
// 128-byte zero page.  Workgroup = (BM/64) x (BN/64) waves, each wave 64 pixels x 64
// channels (2 x 2 MFMA tiles of 32x32, 64 accumulator registers).
// Grid is 1-D and XCD-aware: the channel tiles of one pixel tile get consecutive slots
// on ONE XCD (ids congruent mod 8 share an XCD), so the shared A rows hit that XCD's L2.
//
// PROJ (3x3 / stride 2 layers only): the BasicBlock's 1x1 / stride 2 projection shortcut reads
// exactly the centre tap of this convolution, so it rides along as CC extra K tiles (centre-tap
// activation tile x projection weights) into a second accumulator set and leaves through a
// second epilogue (bias only, no ReLU) into `outp_p`: one launch, one pass over the input.
// ---------------------------------------------------------------------------------------
#pragma once
#include "conv_device.h"

namespace hipac {

template <typename T, int CIN, int COUT, int HI, int WI, int KS, int STRIDE, int BM, int BN, int NSTAGE,
          bool RELU, bool RESID, bool OUTF32, bool PROJ = false, int TKH = 0, int TKW = 0, int UPS = 0>
__global__ __launch_bounds__((BM / 64) * (BN / 64) * 64, 2) void conv_glds_kernel(
    const T* __restrict__ in, const T* __restrict__ wgt, const float* __restrict__ bias,
    const T* __restrict__ resid, void* __restrict__ outp, int M, int n_mtiles, const char* __restrict__ zero_page,
    const T* __restrict__ wgt_p = nullptr, const float* __restrict__ bias_p = nullptr,
    void* __restrict__ outp_p = nullptr) {
  using E = Elem<T>;
  using frag = typename E::frag;
  // UPS != 0 (training: data gradient of a stride-2 conv, one PARITY CLASS of the fine grid per launch): the input is the
  // gradient on the coarse grid, the window is TKH x TKW taps starting AT the output pixel (no padding; taps beyond the
  // bottom / right edge read zeros), the output grid equals the input grid and output pixel (y, x) is stored at fine
  // position (2y + PY, 2x + PX), UPS = 4 | PY << 1 | PX.  See launch_dgrad_s2.
  constexpr int KH = UPS ? TKH : KS, KW = UPS ? TKW : KS;
  constexpr int PAD = UPS ? 0 : KS / 2;
  constexpr int HO = UPS ? HI : (HI + 2 * PAD - KS) / STRIDE + 1;
  constexpr int WO = UPS ? WI : (WI + 2 * PAD - KS) / STRIDE + 1;
  static_assert(!UPS || (STRIDE == 1 && TKH >= 1 && TKW >= 1 && !PROJ && !RESID && !OUTF32), "parity-class data gradient");
  constexpr int CC = CIN / 64;                      // 64-channel chunks of the K loop
  constexpr int KT = KH * KW * CC;
  constexpr int KTOT = KT * 64;
  constexpr int KTP = PROJ ? KT + CC : KT;          // + the projection's K tiles
  static_assert(!PROJ || (KS == 3 && STRIDE == 2 && !RESID && !OUTF32), "projection rides on 3x3/2 only");
  constexpr int MT = 2;                            // 32-pixel sub-tiles per wave
  constexpr int WM = BM / 64, WN = BN / 64, NWAVES = WM * WN;
  constexpr int APW = BM / 8 / NWAVES;  // 1-KiB A pieces per wave per K tile
  constexpr int WPW = BN / 8 / NWAVES;  // 1-KiB W pieces per wave per K tile
  constexpr int PPW = APW + WPW;
  constexpr int STAGE = (BM + BN) * 128;
  constexpr int NTILES_N = COUT / BN;
  static_assert(BM % 64 == 0 && BN % 64 == 0 && COUT % BN == 0 && CIN % 64 == 0, "tile shape");
  static_assert((BM / 8) % NWAVES == 0 && (BN / 8) % NWAVES == 0, "piece split");
  static_assert(NSTAGE >= 2 && NSTAGE * STAGE <= 160 * 1024, "LDS ring");
  static_assert((NSTAGE - 1) * PPW < 64, "vmcnt range");

  extern __shared__ __attribute__((aligned(1024))) unsigned char ring[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % WM, wn = wave / WM;
  const int r = lane & 31, h = lane >> 5;

  // XCD-aware decode of the 1-D grid
  const int bid = blockIdx.x;
  const int xcd = bid & 7, slot = bid >> 3;
  const int mt = (slot / NTILES_N) * 8 + xcd;
  const int nt = slot % NTILES_N;
  if (mt >= n_mtiles) return;  // uniform per block; grid is padded to a multiple of 8 m-tiles
  const int m0 = mt * BM, n0 = nt * BN;

  // ---- DMA source setup: lane -> (row within piece, destination chunk) -----------------
  const int prow = lane >> 3;     // row inside the 8-row piece
  const int dchunk = lane & 7;    // destination 16-byte chunk (lane-linear)
  int a_off[APW];                 // byte offset of tap (0,0), incl. the swizzled source chunk
  unsigned a_mask[APW];           // bit (kh*KW+kw): tap inside the image
#pragma unroll
  for (int i = 0; i < APW; ++i) {
    const int row = (wave + NWAVES * i) * 8 + prow;  // row inside the BM tile
    const int schunk = dchunk ^ ((row >> 1) & 7);
    const int m = m0 + row;
    const bool ok = m < M;
    const int mm = ok ? m : 0;
    const int b = mm / (HO * WO);
    const int rem = mm - b * (HO * WO);
    const int oh = rem / WO, ow = rem - oh * WO;
    const int ih0 = oh * STRIDE - PAD, iw0 = ow * STRIDE - PAD;
    a_off[i] = (((b * HI + ih0) * WI + iw0) * CIN + schunk * 8) * 2;
    unsigned mask = 0;
#pragma unroll
    for (int kh = 0; kh < KH; ++kh)
#pragma unroll
      for (int kw = 0; kw < KW; ++kw)
        if (ok && (unsigned)(ih0 + kh) < (unsigned)HI && (unsigned)(iw0 + kw) < (unsigned)WI)
          mask |= 1u << (kh * KW + kw);
    a_mask[i] = mask;
  }
  int w_off[WPW], wp_off[PROJ ? WPW : 1];
#pragma unroll
  for (int i = 0; i < WPW; ++i) {
    const int row = (wave + NWAVES * i) * 8 + prow;  // row inside the BN tile
    const int schunk = dchunk ^ ((row >> 1) & 7);
    w_off[i] = ((n0 + row) * KTOT + schunk * 8) * 2;
    if constexpr (PROJ) wp_off[i] = ((n0 + row) * (CC * 64) + schunk * 8) * 2;
  }
  const char* in_b = reinterpret_cast<const char*>(in);
  const char* w_b = reinterpret_cast<const char*>(wgt);
  const char* wp_b = reinterpret_cast<const char*>(wgt_p);
  const char* zsrc = zero_page + dchunk * 16;

  using gptr_t = const __attribute__((address_space(1))) void*;
  using lptr_t = __attribute__((address_space(3))) void*;
  // LDS-DMA through buffer descriptors: a tap that leaves the image (or a row beyond M) gets an offset
  // past the descriptor's range and reads as zeros -- no zero-page select, no 64-bit address arithmetic
  const rsrc_t in_rsrc = make_rsrc(in_b, (M / (HO * WO)) * (HI * WI * CIN * 2));
  const rsrc_t w_rsrc = make_rsrc(w_b, COUT * KTOT * 2);
  const rsrc_t wp_rsrc = make_rsrc(PROJ ? wp_b : w_b, COUT * CC * 64 * 2);
  auto issue = [&](int tap, int tapoff_bytes, int kofs_bytes, int stage, bool proj) {
    unsigned char* sbase = ring + stage * STAGE;
    static_for<APW>([&](auto I) {
      constexpr int i = decltype(I)::value;
      const bool ok = (a_mask[i] >> tap) & 1u;
      buffer_load_lds16(in_rsrc, sbase + (wave + NWAVES * i) * 1024, ok ? a_off[i] + tapoff_bytes : (int)0x80000000, 0);
    });
    static_for<WPW>([&](auto I) {
      constexpr int i = decltype(I)::value;
      if (PROJ && proj) buffer_load_lds16(wp_rsrc, sbase + BM * 128 + (wave + NWAVES * i) * 1024, wp_off[i], kofs_bytes);
      else buffer_load_lds16(w_rsrc, sbase + BM * 128 + (wave + NWAVES * i) * 1024, w_off[i], kofs_bytes);
    });
  };

  // ---- fragment read offsets (bytes inside a stage) -------------------------------------
  const int sw = (r >> 1) & 7;
  int rd[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) rd[kk] = r * 128 + (((2 * kk + h) ^ sw) << 4);
  const int a_rd0 = wm * 64 * 128;
  const int w_rd0 = BM * 128 + wn * 64 * 128;

  f32x16 acc[MT][2], accp[PROJ ? MT : 1][PROJ ? 2 : 1];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        acc[i][j][e] = 0.f;
        if constexpr (PROJ) accp[i][j][e] = 0.f;
      }

  // issue-side tile counters (tile index ti = (kh*KS + kw)*CC + cc; then the projection's cc tiles)
  int i_kh = 0, i_kw = 0, i_cc = 0, i_t = 0;
  auto issue_next = [&]() __attribute__((always_inline)) {
    if (PROJ && i_t >= KT) {  // centre tap (1,1), channel chunk i_t - KT, projection weights
      const int pc = i_t - KT;
      issue(4, ((WI + 1) * CIN + pc * 64) * 2, pc * 128, i_t % NSTAGE, true);
    } else {
      const int tap = i_kh * KW + i_kw;
      issue(tap, ((i_kh * WI + i_kw) * CIN + i_cc * 64) * 2, i_t * 128, i_t % NSTAGE, false);
      if (++i_cc == CC) {
        i_cc = 0;
        if (++i_kw == KW) {
          i_kw = 0;
          ++i_kh;
        }
      }
    }
    ++i_t;
  };
#pragma unroll
  for (int p = 0; p < NSTAGE - 1; ++p)
    if (p < KTP) issue_next();

  for (int t = 0; t < KTP; ++t) {
    // tile t must have landed: tiles t+1 .. min(t+NSTAGE-2, KTP-1) may stay in flight
    const int ahead = (KTP - 1 - t) < (NSTAGE - 2) ? (KTP - 1 - t) : (NSTAGE - 2);
    if constexpr (NSTAGE >= 4) {
      if (ahead >= 2) wait_vmcnt<2 * PPW>();
      else if (ahead == 1) wait_vmcnt<PPW>();
      else wait_vmcnt<0>();
    } else if constexpr (NSTAGE == 3) {
      if (ahead >= 1) wait_vmcnt<PPW>();
      else wait_vmcnt<0>();
    } else {
      wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();  // every wave's pieces of tile t are in; stage (t-1)%NSTAGE is free
    if (t + NSTAGE - 1 < KTP) issue_next();
    const unsigned char* st = ring + (t % NSTAGE) * STAGE;
    // fragment reads run one k16 step ahead of the MFMAs that consume them
    frag af[2][MT], wf[2][2];
#pragma unroll
    for (int i = 0; i < MT; ++i) af[0][i] = *reinterpret_cast<const frag*>(st + a_rd0 + i * 4096 + rd[0]);
#pragma unroll
    for (int j = 0; j < 2; ++j) wf[0][j] = *reinterpret_cast<const frag*>(st + w_rd0 + j * 4096 + rd[0]);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      if (kk + 1 < 4) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
          af[(kk + 1) & 1][i] = *reinterpret_cast<const frag*>(st + a_rd0 + i * 4096 + rd[kk + 1]);
#pragma unroll
        for (int j = 0; j < 2; ++j)
          wf[(kk + 1) & 1][j] = *reinterpret_cast<const frag*>(st + w_rd0 + j * 4096 + rd[kk + 1]);
      }
      if (PROJ && t >= KT) {  // uniform: the last CC tiles feed the projection's accumulators
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            accp[PROJ ? i : 0][PROJ ? j : 0] =
                E::mfma(wf[kk & 1][j], af[kk & 1][i], accp[PROJ ? i : 0][PROJ ? j : 0]);
      } else {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = E::mfma(wf[kk & 1][j], af[kk & 1][i], acc[i][j]);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    // the reads of this stage must have retired before any wave passes the next barrier
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }

  // ---- projection epilogue: + bias -> NHWC store (no ReLU, no residual) -------------------
  if constexpr (PROJ) {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int m = m0 + wm * 64 + i * 32 + r;
      if (m >= M) continue;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c0 = n0 + wn * 64 + j * 32 + 8 * q + 4 * h;
          const float4 bv = *reinterpret_cast<const float4*>(bias_p + c0);
          const float pv[4] = {accp[i][j][4 * q + 0] + bv.x, accp[i][j][4 * q + 1] + bv.y, accp[i][j][4 * q + 2] + bv.z,
                               accp[i][j][4 * q + 3] + bv.w};
          typename E::vec4 ov;
          ov[0] = (T)pv[0];
          ov[1] = (T)pv[1];
          ov[2] = (T)pv[2];
          ov[3] = (T)pv[3];
          *reinterpret_cast<typename E::vec4*>(reinterpret_cast<T*>(outp_p) + (size_t)m * COUT + c0) = ov;
        }
    }
  }

  // ---- epilogue: +bias (+residual) (ReLU) -> NHWC store ---------------------------------
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = m0 + wm * 64 + i * 32 + r;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = n0 + wn * 64 + j * 32 + 8 * q + 4 * h;
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

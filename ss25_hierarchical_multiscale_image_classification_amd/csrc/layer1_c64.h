// The register-weight kernels of the 56x56 map: layer1's 3x3 conv and layer2's entry conv with its projection.
#pragma once
#include "conv_device.h"

namespace hipac {

#ifndef HIPAC_C64_PF
#define HIPAC_C64_PF 2  // layer1 kernel: LDS fragment reads run this many k16 steps ahead of their MFMAs
#endif
// order of the 36 (tap, k16) steps of a 3x3 x 64-channel accumulation: (kh, kw, k16 step)
constexpr int c64_step_kh(int st) { return st / 12; }
constexpr int c64_step_kw(int st) { return (st % 12) / 4; }
constexpr int c64_step_kk(int st) { return st % 4; }

// ---------------------------------------------------------------------------------------
// layer1 kernel: 3x3 / stride 1 / 64 -> 64 channels on the 56x56 map (4 of the 20 convs,
// 25 % of the FLOPs, and the largest activations after the stem).
//   * persistent workgroups (grid-stride over work units), 4 waves
//   * a unit = two 8x8 output tiles; each tile's 10x10 input halo (64 ch = 128 B per pixel)
//     is brought into LDS by LDS-DMA: 200 pixels per 128 outputs = 1.56x re-read
//   * the halos are DOUBLE-BUFFERED ACROSS UNITS: the DMA of unit u+1 is issued at the top of
//     unit u and has the whole unit (72 MFMAs + epilogue) to land -- one workgroup barrier per unit
//   * K = 576 is short enough for every lane to keep ITS weight fragments for all 9 taps in
//     registers (36 fragments = 144 VGPRs; wave = one tile x 32 channels), so weights are
//     fetched once per workgroup and LDS serves only activation fragments, with NO barrier
//     inside a unit's 72-MFMA loop
//   * LDS placement of halo pixel (hy,hx): slot hy*10+hx, 16-byte chunk c stored at
//     c ^ (((hx>>1)&1) | ((hy&3)<<1)).  For every tap, a ds_read_b128 lane group (4 runs of 4
//     consecutive x on 4 consecutive rows) then hits 16 distinct 16-byte slots: conflict-free
//   * epilogue per WAVE (no barrier): each 32-pixel x 32-channel sub-tile goes through the
//     wave's private fp32 staging rows and leaves as 16-byte items, 64 contiguous bytes per
//     pixel; the residual items are prefetched into registers one sub-tile ahead
// ---------------------------------------------------------------------------------------
template <typename T, bool RESID, bool RELU = true>
__global__ __launch_bounds__(256, 2) void conv3x3_c64_kernel(const T* __restrict__ in, const T* __restrict__ wgt,
                                                             const float* __restrict__ bias,
                                                             const T* __restrict__ resid, T* __restrict__ out,
                                                             int n_tiles, const char* __restrict__ zero_page) {
  using E = Elem<T>;
  using frag = typename E::frag;
  constexpr int H = 56, W = 56, C = 64, TPI = 49;  // 7 x 7 tiles of 8 x 8 per image
  constexpr int HALO = 10, HPIECES = 13;           // 100 halo pixels -> 13 pieces of 8
  constexpr int H_BYTES = HPIECES * 1024;
  constexpr int U_BYTES = 2 * H_BYTES;             // the two halos of a unit
  constexpr int SROW = 144;                        // staging row: 32 fp32 + 16 B pad
  constexpr int SPX = RESID ? 16 : 32;             // pixels staged at a time (RESID: LDS also holds the residual)
  constexpr int SW_BYTES = SPX * SROW;             // one wave's staging
  constexpr int R_BYTES = RESID ? 4 * 4096 : 0;    // residual of the unit: per wave 2 sub-tiles x 32 px x 64 B
  __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * U_BYTES + R_BYTES + 4 * SW_BYTES + 64 * 4];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wt = wave & 1, wn = wave >> 1;  // tile of the pair, channel half
  const int r = lane & 31, h = lane >> 5;
  unsigned char* const Rl = smem + 2 * U_BYTES + wave * 4096;
  unsigned char* const Sl = smem + 2 * U_BYTES + R_BYTES + wave * SW_BYTES;
  float* const Bl = reinterpret_cast<float*>(smem + 2 * U_BYTES + R_BYTES + 4 * SW_BYTES);  // bias
  if (tid < 64) Bl[tid] = bias[tid];  // visible after the first unit's barrier

  // weights of channels wn*32 + r, all 9 taps x 64 input channels, in registers
  frag wreg[9][4];
  {
    const char* wb = reinterpret_cast<const char*>(wgt) + (size_t)(wn * 32 + r) * (9 * C * 2) + 16 * h;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) wreg[tap][kk] = *reinterpret_cast<const frag*>(wb + tap * 128 + kk * 32);
  }
  // epilogue item k of a sub-tile: pixel e_px + 16k (0..31), channels wn*32 + e_c8*8 .. +7
  const int e_c8 = lane & 3, e_px = lane >> 2;

  using gptr_t = const __attribute__((address_space(1))) void*;
  using lptr_t = __attribute__((address_space(3))) void*;
  const int prow = lane >> 3, dchunk = lane & 7;
  const char* in_b = reinterpret_cast<const char*>(in);

  // LDS-DMA of the two halos of unit u (tiles 2u, 2u+1) into buffer `buf`; 26 pieces over 4 waves.
  // Everything about a piece that does not depend on the tile is computed once: the byte offset of
  // this lane's 16 bytes relative to the tile's first pixel, with 4 edge bits in its low nibble
  // (halo row 0 / row 9 / column 0 / column 9), so a unit costs a handful of VALU per piece.
  // Slots 100..103 of a halo do not exist: they re-fetch pixel 99 (never read).
  constexpr int NPW = (2 * HPIECES + 3) / 4;  // pieces per wave (7; waves 2, 3 have 6)
  int piece_pk[NPW];
#pragma unroll
  for (int k = 0; k < NPW; ++k) {
    const int p = wave + 4 * k;
    const int pp = p >= HPIECES ? p - HPIECES : p;
    int q = pp * 8 + prow;
    q = q < HALO * HALO ? q : HALO * HALO - 1;
    const int hy = q / HALO, hx = q - hy * HALO;
    const int sw = ((hx >> 1) & 1) | ((hy & 3) << 1);
    const int rel = ((hy - 1) * W + (hx - 1)) * (C * 2) + (dchunk ^ sw) * 16;
    piece_pk[k] = rel | (hy == 0 ? 1 : 0) | (hy == HALO - 1 ? 2 : 0) | (hx == 0 ? 4 : 0) | (hx == HALO - 1 ? 8 : 0);
  }
  auto issue_unit = [&](int u, int buf) {
    const char* tbase[2];
    int tmask[2];
#pragma unroll
    for (int tsel = 0; tsel < 2; ++tsel) {  // wave-uniform tile scalars
      const int tile = 2 * u + tsel;
      const int b = tile / TPI, t = tile - b * TPI;
      const int ty = t / 7, tx = t - ty * 7;
      tbase[tsel] = in_b + (((size_t)b * H + ty * 8) * W + tx * 8) * (C * 2);
      // bit 4: the tile lies beyond the batch -> every piece reads zeros
      tmask[tsel] = tile < n_tiles ? ((ty == 0 ? 1 : 0) | (ty == 6 ? 2 : 0) | (tx == 0 ? 4 : 0) | (tx == 6 ? 8 : 0)) : 16;
    }
    static_for<NPW>([&](auto K) {
      constexpr int k = decltype(K)::value;
      const int p = wave + 4 * k;
      if (p < 2 * HPIECES) {
        const int tsel = p >= HPIECES ? 1 : 0;
        const int pp = p - tsel * HPIECES;
        const int tm = tmask[tsel];
        const bool ok = tm != 16 && (piece_pk[k] & tm & 15) == 0;
        const char* src = ok ? tbase[tsel] + (piece_pk[k] & ~15) : zero_page + dchunk * 16;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(smem + buf * U_BYTES + tsel * H_BYTES + pp * 1024),
                                         16, 0, 0);
      }
    });
  };

  // this lane's two output pixels inside its tile: sub-tile i = rows 4i..4i+3; (ly,lx) = (4i + r/8, r%8)
  int lx = r & 7, ly0 = r >> 3;

  const int n_units = (n_tiles + 1) >> 1;
  int u = blockIdx.x;
  // the weight / bias loads above must retire BEFORE the unit loop: otherwise the compiler drains
  // vmcnt -- and with it the prefetched DMA of the next unit -- in front of the first MFMA of
  // every unit (seen in the RESID variant: s_waitcnt vmcnt(0) right after s_setprio 1)
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) asm volatile("" ::"v"(wreg[tap][kk]));  // a use: forces the wait here
  if (u < n_units) issue_unit(u, 0);
#ifdef HIPAC_HALO_STAMPS
  unsigned long long c_sum[5] = {0, 0, 0, 0, 0};
#endif
  bool stored = false;  // wave-uniform: the previous unit's epilogue issued its 4 stores
  for (int it = 0; u < n_units; u += gridDim.x, ++it) {
    const int buf = it & 1;
    HALO_STAMP(c_t0);
    // this unit's halo DMAs are OLDER than the 4 stores of the previous epilogue and vmcnt retires in
    // issue order: leave the stores in flight instead of paying their acknowledgement latency here
    if (stored) wait_vmcnt<4>();
    else wait_vmcnt<0>();
    HALO_STAMP(c_t0b);
    __builtin_amdgcn_s_barrier();  // halos of this unit landed; every wave is past its reads of the other buffer
    HALO_STAMP(c_t1);

    // this wave's tile and the element offset of its epilogue items (pixel e_px + 16k of sub-tile i)
    const bool tile_ok = 2 * u + wt < n_tiles;
    stored = tile_ok;
    const int tile = tile_ok ? 2 * u + wt : n_tiles - 1;  // addresses stay inside the tensors; stores are guarded
    const int tb = tile / TPI, tt = tile - tb * TPI;
    const int ty = tt / 7, tx = tt - ty * 7;
    // pixel (4i + (e_px + 16k) / 8, (e_px + 16k) % 8) of the tile -> NHWC element offset
    auto item_off = [&](int i, int k) -> size_t {
      const int px = e_px + 16 * k;
      const int y = ty * 8 + 4 * i + (px >> 3), x = tx * 8 + (px & 7);
      return (((size_t)tb * H + y) * W + x) * C + wn * 32 + e_c8 * 8;
    };
    // residual of this unit by LDS-DMA: piece j = (sub-tile j/2, item j%2) -- every lane fetches exactly
    // the 16 bytes it adds in the epilogue (item-linear destination, no cross-lane dependency).
    // Issued ahead of the next unit's halos: vmcnt retires in issue order.
    if constexpr (RESID) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        __builtin_amdgcn_global_load_lds((gptr_t)(resid + item_off(j >> 1, j & 1)), (lptr_t)(Rl + j * 1024), 16, 0, 0);
    }
    const bool more = u + (int)gridDim.x < n_units;
    if (more) issue_unit(u + gridDim.x, buf ^ 1);  // lands behind this whole unit

    // keep the 18 tap address bases from being hoisted out of the unit loop (they would
    // cost 18 VGPRs next to 144 of weights): make their inputs opaque per iteration
    asm volatile("" : "+v"(lx), "+v"(ly0));
    const unsigned char* const Hl = smem + buf * U_BYTES + wt * H_BYTES;
    // the bias is the initial accumulator (register group q = channels wn*32 + 8q + 4h .. +3)
    f32x16 acc[2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 bq = *reinterpret_cast<const f32x4*>(Bl + wn * 32 + 8 * q + 4 * h);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][4 * q + e] = bq[e];
    }
    __builtin_amdgcn_s_setprio(1);
    // 36 k16 steps (tap-major); the two activation fragments of step s + PF are requested before the
    // MFMAs of step s, so an LDS read has PF MFMA pairs (PF x 64 cycles) to return
    constexpr int PF = HIPAC_C64_PF;
    frag ring[PF + 1][2];
    // address of fragment (tap, kk, i) = lane base + compile-time slot offset + swizzled chunk, with the
    // chunk term factored per axis: bit 4 = ((hx >> 1) & 1) ^ h depends on kw only, bits 5-6 =
    // (hy & 3) ^ kk on kh only (hy & 3 does not depend on i) -- 2 VALU per k16 step instead of ~5 per read
    int ax[3], by[3];
#pragma unroll
    for (int k3 = 0; k3 < 3; ++k3) {
      ax[k3] = ((((lx + k3) >> 1) & 1) ^ h) << 4;
      by[k3] = ((ly0 + k3) & 3) << 5;
    }
    const unsigned char* const Hb = Hl + ((ly0 * HALO + lx) << 7);
    auto rd_step = [&](auto S) {
      constexpr int st = decltype(S)::value;
      constexpr int kh = c64_step_kh(st), kw = c64_step_kw(st), kk = c64_step_kk(st);
      const unsigned char* const ptr = Hb + (ax[kw] | (by[kh] ^ (kk << 5)));
#pragma unroll
      for (int i = 0; i < 2; ++i)
        ring[st % (PF + 1)][i] = *reinterpret_cast<const frag*>(ptr + (((4 * i + kh) * HALO + kw) << 7));
    };
    static_for<PF>([&](auto S) { rd_step(S); });
    static_for<36>([&](auto S) {
      constexpr int st = decltype(S)::value;
      if constexpr (st + PF < 36) rd_step(std::integral_constant<int, st + PF>{});
#pragma unroll
      for (int i = 0; i < 2; ++i)
        acc[i] = E::mfma(wreg[3 * c64_step_kh(st) + c64_step_kw(st)][c64_step_kk(st)], ring[st % (PF + 1)][i], acc[i]);
      __builtin_amdgcn_sched_barrier(0);  // pin the read-ahead: the scheduler otherwise folds it back to one step
    });
    __builtin_amdgcn_s_setprio(0);
    HALO_STAMP(c_t2);

    // epilogue, per wave: SPX pixels of sub-tile i -> private fp32 rows -> + bias (+ residual) ReLU -> T
    if constexpr (RESID) {
      // this lane's residual pieces have landed once only the next unit's halo DMAs (issued later:
      // 7 per wave for waves 0-1, 6 for waves 2-3) are still outstanding
      if (!more) wait_vmcnt<0>();
      else if (wave < 2) wait_vmcnt<7>();
      else wait_vmcnt<6>();
    }
    static_for<2 * (32 / SPX)>([&](auto PH) {
      constexpr int i = decltype(PH)::value / (32 / SPX), hf = decltype(PH)::value % (32 / SPX);
      if (SPX == 32 || (r >> 4) == hf) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f32x4 v;
          v[0] = acc[i][4 * q + 0];
          v[1] = acc[i][4 * q + 1];
          v[2] = acc[i][4 * q + 2];
          v[3] = acc[i][4 * q + 3];
          *reinterpret_cast<f32x4*>(Sl + (r & (SPX - 1)) * SROW + (8 * q + 4 * h) * 4) = v;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // one wave's LDS operations complete in order
#pragma unroll
      for (int k = 0; k < SPX / 16; ++k) {
        const int px = e_px + 16 * k;            // pixel inside the staged rows
        constexpr int kk = SPX == 32 ? 0 : hf;   // item index inside the sub-tile = k (SPX 32) or hf (SPX 16)
        const int ki = SPX == 32 ? k : kk;
        const f32x4 lo = *reinterpret_cast<const f32x4*>(Sl + px * SROW + e_c8 * 32);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(Sl + px * SROW + e_c8 * 32 + 16);
        float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        if constexpr (RESID) {
          const frag rvv = *reinterpret_cast<const frag*>(Rl + (2 * i + ki) * 1024 + lane * 16);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += (float)rvv[e];
        }
        frag ov;
#pragma unroll
        for (int e = 0; e < 8; ++e) ov[e] = (T)(RELU ? fmaxf(v[e], 0.f) : v[e]);  // (training's convolutions carry no ReLU: BN follows)
        if (tile_ok) *reinterpret_cast<frag*>(out + item_off(i, ki)) = ov;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // staging reads returned before it is overwritten
    });
#ifdef HIPAC_HALO_STAMPS
    HALO_STAMP(c_t3);
    c_sum[0] += c_t0b - c_t0;  // vmcnt drain (DMA of this unit + own stores)
    c_sum[1] += c_t1 - c_t0b;  // barrier
    c_sum[2] += c_t2 - c_t1;   // DMA issue + 72 MFMAs
    c_sum[3] += c_t3 - c_t2;   // epilogue
    c_sum[4] += 1;
#endif
  }
#ifdef HIPAC_HALO_STAMPS
  if (lane == 0) {
    atomicAdd(&g_halo_stamps[4], c_sum[0]);
    atomicAdd(&g_halo_stamps[5], c_sum[1]);
    atomicAdd(&g_halo_stamps[6], c_sum[2]);
    atomicAdd(&g_halo_stamps[7], c_sum[3]);
    atomicAdd(&g_halo_stamps[3], c_sum[4]);
  }
#endif
}

// ---------------------------------------------------------------------------------------
// layer2 entry kernel: 3x3 / stride 2 / 64 -> 128 channels, 56x56 -> 28x28 (+BN+ReLU) AND the
// block's 1x1 / stride 2 projection shortcut (+BN), one launch, one pass over the input.
// Same skeleton as the layer1 kernel: persistent workgroups, every lane keeps ITS weight
// fragments in registers (wave w = output channels 32w .. 32w+31: 36 fragments of the 3x3 conv
// + 4 of the projection = 160 VGPRs), LDS serves only activation fragments, halos double-buffered
// across units by LDS-DMA, one workgroup barrier per unit, per-wave barrier-free epilogues.
//   * unit = one tile of 7 x 4 output pixels (28 of the 32 MFMA columns; 28 tiles per image);
//     all four waves read the same activation fragments (different weights)
//   * its 15 x 9 input halo is stored as [row hy][p] with the EVEN columns first
//     (p = (hx & 1) * 8 + hx / 2, 16 slots per row): a tap (kh, kw) then reads consecutive
//     slots p = (kw & 1) * 8 + x + kw / 2 for consecutive output x -- the stride disappears.
//     16-byte chunk c of slot (hy, p) sits at c ^ (((p >> 1) & 1) | (((hy >> 1) & 3) << 1)):
//     every ds_read_b128 lane group covers all 16 bank groups (simulated: 4.0 LDS cycles per read)
//   * the projection reads exactly the centre tap's fragments: 4 extra MFMAs, no extra LDS reads
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256, 2) void conv3x3s2_c64_kernel(const T* __restrict__ in, const T* __restrict__ wgt,
                                                               const float* __restrict__ bias,
                                                               const T* __restrict__ wgt_p,
                                                               const float* __restrict__ bias_p, T* __restrict__ out,
                                                               T* __restrict__ out_p, int n_tiles,
                                                               const char* __restrict__ zero_page) {
  using E = Elem<T>;
  using frag = typename E::frag;
  constexpr int HI = 56, WI = 56, C = 64, HO = 28, WO = 28, CO = 128;
  constexpr int TW = 7, TH = 4, TPI = (WO / TW) * (HO / TH);  // 4 x 7 = 28 tiles per image
  constexpr int HPIECES = 18;                                // 9 rows x 16 slots = 144 slots
  constexpr int H_BYTES = HPIECES * 1024;
  constexpr int SROW = 144;                                  // staging row: 32 fp32 + 16 B pad
  constexpr int SW_BYTES = 32 * SROW;
  __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * H_BYTES + 4 * SW_BYTES + 2 * CO * 4];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  unsigned char* const Sl = smem + 2 * H_BYTES + wave * SW_BYTES;
  float* const Bl = reinterpret_cast<float*>(smem + 2 * H_BYTES + 4 * SW_BYTES);  // bias[128], bias_p[128]
  if (tid < CO) {
    Bl[tid] = bias[tid];
    Bl[CO + tid] = bias_p[tid];
  }

  // weights of output channel 32*wave + r: 9 taps x 64 input channels, and the projection's 64
  frag wreg[9][4], wpr[4];
  {
    const char* wb = reinterpret_cast<const char*>(wgt) + (size_t)(wave * 32 + r) * (9 * C * 2) + 16 * h;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) wreg[tap][kk] = *reinterpret_cast<const frag*>(wb + tap * 128 + kk * 32);
    const char* pb = reinterpret_cast<const char*>(wgt_p) + (size_t)(wave * 32 + r) * (C * 2) + 16 * h;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) wpr[kk] = *reinterpret_cast<const frag*>(pb + kk * 32);
  }
  const int e_c8 = lane & 3, e_px = lane >> 2;  // epilogue item k: pixel e_px + 16k, channels 32*wave + 8*e_c8 ..

  using gptr_t = const __attribute__((address_space(1))) void*;
  using lptr_t = __attribute__((address_space(3))) void*;
  const int prow = lane >> 3, dchunk = lane & 7;
  const char* in_b = reinterpret_cast<const char*>(in);

  // halo DMA: tile-independent part of every piece computed once (byte offset from the tile's first
  // input pixel, edge bits in the low nibble: bit 0 = halo row 0, bit 1 = halo column 0).
  constexpr int NPW = (HPIECES + 3) / 4;  // pieces per wave (5; waves 2, 3 have 4)
  int piece_pk[NPW];
#pragma unroll
  for (int k = 0; k < NPW; ++k) {
    const int q = (wave + 4 * k) * 8 + prow;  // slot = hy*16 + p
    const int hy = (q >> 4) < 9 ? (q >> 4) : 8;
    int pcol = q & 15;
    pcol = pcol < 15 ? pcol : 14;             // slot 15 of a row does not exist: re-fetch slot 14 (never read)
    const int hx = pcol < 8 ? 2 * pcol : 2 * (pcol - 8) + 1;
    const int key = ((pcol >> 1) & 1) | (((hy >> 1) & 3) << 1);
    const int rel = ((hy - 1) * WI + (hx - 1)) * (C * 2) + (dchunk ^ key) * 16;
    piece_pk[k] = rel | (hy == 0 ? 1 : 0) | (hx == 0 ? 2 : 0);
  }
  auto issue_unit = [&](int tile, int buf) {
    const int b = tile / TPI, t = tile - b * TPI;
    const int ty = t / (WO / TW), tx = t - ty * (WO / TW);
    const char* tbase = in_b + (((size_t)b * HI + ty * (2 * TH)) * WI + tx * (2 * TW)) * (C * 2);
    const int tmask = (ty == 0 ? 1 : 0) | (tx == 0 ? 2 : 0);
    static_for<NPW>([&](auto K) {
      constexpr int k = decltype(K)::value;
      const int pc = wave + 4 * k;
      if (pc < HPIECES) {
        const bool ok = (piece_pk[k] & tmask) == 0;
        const char* src = ok ? tbase + (piece_pk[k] & ~15) : zero_page + dchunk * 16;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(smem + buf * H_BYTES + pc * 1024), 16, 0, 0);
      }
    });
  };

  // this lane's output pixel inside the tile: (y, x) = (r / 8, r % 8); column 7 does not exist and
  // re-reads column 6 (same address: an LDS broadcast), its results are never stored
  int lx = (r & 7) < TW ? (r & 7) : TW - 1, ly = r >> 3;

#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) asm volatile("" ::"v"(wreg[tap][kk]));  // weight loads retire before the loop
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) asm volatile("" ::"v"(wpr[kk]));

  int tile = blockIdx.x;
  if (tile < n_tiles) issue_unit(tile, 0);
  for (int it = 0; tile < n_tiles; tile += gridDim.x, ++it) {
    const int buf = it & 1;
    // the halo DMAs are older than the previous epilogue's 4 stores (vmcnt retires in issue order)
    if (it) wait_vmcnt<4>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();  // this tile's halo landed; every wave is past its reads of the other buffer
    if (tile + (int)gridDim.x < n_tiles) issue_unit(tile + gridDim.x, buf ^ 1);  // lands behind this whole unit

    const int tb = tile / TPI, tt = tile - tb * TPI;
    const int ty = tt / (WO / TW), tx = tt - ty * (WO / TW);
    asm volatile("" : "+v"(lx), "+v"(ly));  // keep the tap address bases from being hoisted (VGPRs)
    const unsigned char* const Hl = smem + buf * H_BYTES;
    f32x16 acc, accp;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = accp[e] = 0.f;
    __builtin_amdgcn_s_setprio(1);
    constexpr int PF = 2;
    frag ring[PF + 1];
    // fragment address = lane base + compile-time slot offset + swizzled chunk, the chunk term factored per
    // axis: bit 4 = ((pcol >> 1) & 1) ^ h depends on kw only, bits 5-6 = ((hy >> 1) & 3) ^ kk on kh only
    int ax[3], by[3];
#pragma unroll
    for (int k3 = 0; k3 < 3; ++k3) {
      const int pcol = (k3 & 1) * 8 + lx + (k3 >> 1);
      ax[k3] = (((pcol >> 1) & 1) ^ h) << 4;
      by[k3] = (((2 * ly + k3) >> 1) & 3) << 5;
    }
    const unsigned char* const Hb = Hl + (((2 * ly) << 4) + lx) * 128;
    auto rd_step = [&](auto S) {
      constexpr int st = decltype(S)::value;
      constexpr int tap = st / 4, kk = st % 4, kh = tap / 3, kw = tap % 3;
      ring[st % (PF + 1)] = *reinterpret_cast<const frag*>(Hb + (ax[kw] | (by[kh] ^ (kk << 5))) +
                                                           (((kh << 4) + (kw & 1) * 8 + (kw >> 1)) << 7));
    };
    static_for<PF>([&](auto S) { rd_step(S); });
    static_for<36>([&](auto S) {
      constexpr int st = decltype(S)::value;
      if constexpr (st + PF < 36) rd_step(std::integral_constant<int, st + PF>{});
      acc = E::mfma(wreg[st / 4][st % 4], ring[st % (PF + 1)], acc);
      if constexpr (st / 4 == 4) accp = E::mfma(wpr[st % 4], ring[st % (PF + 1)], accp);  // centre tap = 1x1/2 input
      __builtin_amdgcn_sched_barrier(0);
    });
    __builtin_amdgcn_s_setprio(0);

    // epilogue, per wave: [32 px][32 ch] fp32 through private staging rows -> 16-byte items
    auto flush = [&](const f32x16& a, const float* bl, bool relu, T* dst) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 v;
        v[0] = a[4 * q + 0];
        v[1] = a[4 * q + 1];
        v[2] = a[4 * q + 2];
        v[3] = a[4 * q + 3];
        *reinterpret_cast<f32x4*>(Sl + r * SROW + (8 * q + 4 * h) * 4) = v;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // one wave's LDS operations complete in order
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int px = e_px + 16 * k;
        const int y = px >> 3, x = px & 7;
        const f32x4 lo = *reinterpret_cast<const f32x4*>(Sl + px * SROW + e_c8 * 32);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(Sl + px * SROW + e_c8 * 32 + 16);
        const f32x4 b_lo = *reinterpret_cast<const f32x4*>(bl + wave * 32 + e_c8 * 8);
        const f32x4 b_hi = *reinterpret_cast<const f32x4*>(bl + wave * 32 + e_c8 * 8 + 4);
        float v[8] = {lo[0] + b_lo[0], lo[1] + b_lo[1], lo[2] + b_lo[2], lo[3] + b_lo[3],
                      hi[0] + b_hi[0], hi[1] + b_hi[1], hi[2] + b_hi[2], hi[3] + b_hi[3]};
        frag ov;
#pragma unroll
        for (int e = 0; e < 8; ++e) ov[e] = (T)(relu ? fmaxf(v[e], 0.f) : v[e]);
        if (x < TW)
          *reinterpret_cast<frag*>(dst + ((((size_t)tb * HO + ty * TH + y) * WO + tx * TW + x) * CO + wave * 32 +
                                         e_c8 * 8)) = ov;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // staging reads returned before it is overwritten
    };
    flush(acc, Bl, true, out);
    flush(accp, Bl + CO, false, out_p);
  }
}

}  // namespace hipac

// The two fused stem kernels (7x7/2 conv + BN + ReLU + 3x3/2 max-pool): the tile kernel and the uint8 strip kernel.
#pragma once
#include <type_traits>
#include "conv_device.h"
#include "halo16x2.h"  // the q8 tensor format of the strip kernel's Q8 form (cvt4_e4m3, kQ8LoScale)

namespace hipac {

// ---------------------------------------------------------------------------------------
// Fused stem: 7x7/2 conv (+BN+ReLU) and the 3x3/2 max-pool in one kernel, so the
// 112x112x64 stem activation (1.6 MB per patch, the largest tensor of the network) never
// reaches HBM.  A workgroup (4 waves) produces an 8x7 tile of POOLED pixels: it needs the
// 17x15 = 255 stem pixels around it (exactly 8 MFMA sub-tiles of 32), which need a 39x36
// pixel patch of the padded NHWC4 input (11 KB).  Workgroups are persistent (grid-stride
// over tiles) and every lane keeps ITS slice of the whole stem weight matrix in registers
// (2 channel tiles x 7 kh x 2 k16 fragments = 112 VGPRs): weights are fetched once per
// workgroup and never re-read, so LDS serves only the activation fragments (1 read per 2
// MFMAs).  The input patch is double-buffered with a register prefetch of the next tile
// behind the MFMAs; the stem tile goes to LDS (bias, ReLU, rounded to T exactly as the
// unfused path stores it) and each thread reduces pooled pixels x 8 channels.
// Stem pixels outside the image (row/col -1) are stored as 0: inputs are post-ReLU (>= 0),
// so they can never win the max.
// ---------------------------------------------------------------------------------------
// U8IN: the input is the raw uint8 HWC patch batch [n,224,224,3]; ToTensor/Normalize is
// applied while the patch is staged (a 3 x 256 table of T values in LDS == the fp32 LUT
// rounded to T, i.e. exactly what hipac_patches_normalize would have written), so the padded
// NHWC4 tensor (427 KB per patch written and read back) never exists.
constexpr int kStemTilesPerImage = 56;

template <typename T, bool U8IN>
__global__ __launch_bounds__(256, 2) void stem_pool_kernel(const void* __restrict__ xin_, const T* __restrict__ wgt,
                                                        const float* __restrict__ bias, T* __restrict__ out,
                                                        int n_tiles, const unsigned short* __restrict__ lut_t,
                                                        long long in_bytes) {
  const T* xin = reinterpret_cast<const T*>(xin_);
  using E = Elem<T>;
  using frag = typename E::frag;
  constexpr int PTH = 8, PTW = 7;                                       // pooled tile
  constexpr int STW = 2 * PTW + 1, STH = 2 * PTH + 1, NPX = STW * STH;  // 15 x 17 = 255 stem pixels
  constexpr int PROWS = 2 * STH + 5, PCOLS = 36;                        // 39 x 36 input pixels (8 B each)
  static_assert(56 / PTW * (56 / PTH) == kStemTilesPerImage, "tile count");
  constexpr int PPR = PCOLS / 2;                                        // 16-byte pieces per patch row
  constexpr int NPIECE = PROWS * PPR;                                   // 702
  constexpr int PF = (NPIECE + 255) / 256;                              // pieces per thread (3)
  constexpr int TILES_X = 56 / PTW, TILES_Y = 56 / PTH, TPI = TILES_X * TILES_Y;  // 8 x 7 = 56 per image
  constexpr int SPX = 144;  // stem-tile pixel stride in LDS: 128 B of channels + 16 B pad (bank spread)
  constexpr int P_BYTES = PROWS * PCOLS * 8, S_BYTES = 256 * SPX;
  constexpr int RAWROW = (PCOLS * 3 + 3 + 3) / 4 * 4, RAWDW = RAWROW / 4;  // raw uint8 window per patch row
  constexpr int RAW_BYTES = U8IN ? PROWS * RAWROW + 3 * 256 * 2 : 0;    // + the T-typed normalise table
  constexpr int NRAW = PROWS * RAWDW, PFR = (NRAW + 255) / 256;          // 1092 dwords, 5 per thread
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * P_BYTES + S_BYTES + RAW_BYTES];
  unsigned char* const Sl = smem + 2 * P_BYTES;
  unsigned char* const Rl = smem + 2 * P_BYTES + S_BYTES;
  unsigned short* const Ll = reinterpret_cast<unsigned short*>(Rl + PROWS * RAWROW);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;

  if constexpr (U8IN) {
    for (int i = threadIdx.x; i < 3 * 256; i += 256) Ll[i] = lut_t[i];
  }
  // this lane's rows of the weight matrix, all of K, in registers for the kernel's lifetime
  frag wreg[2][7][2];
  {
    const char* wb = reinterpret_cast<const char*>(wgt) + r * 448 + 16 * h;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int kh = 0; kh < 7; ++kh)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          wreg[j][kh][kk] = *reinterpret_cast<const frag*>(wb + j * 32 * 448 + kh * 64 + kk * 32);
  }
  float4 bv[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) bv[j][q] = *reinterpret_cast<const float4*>(bias + j * 32 + 8 * q + 4 * h);

  // the two stem pixels of this lane (sub-tiles 2*wave, 2*wave+1); pixel 255 does not exist
  int P[2], a_rd[2], ly[2], lx[2], sidx[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    P[i] = (2 * wave + i) * 32 + r;
    const int Pc = P[i] < NPX ? P[i] : NPX - 1;
    ly[i] = Pc / STW;
    lx[i] = Pc - ly[i] * STW;
    // row-major index in the LDS stem tile; lane 255 of the 17 x 15 tile (a pixel that does not exist)
    // keeps its own dummy row 255 -- it must not share a row with pixel 254
    sidx[i] = P[i] < NPX ? ly[i] * STW + lx[i] : P[i];
    a_rd[i] = ((2 * ly[i]) * PCOLS + 2 * lx[i]) * 8 + 16 * h;
  }

  auto tile_origin = [&](int tile, int& b, int& py0, int& px0) {
    b = tile / TPI;
    const int t = tile - b * TPI;
    const int ty = t / TILES_X;
    py0 = ty * PTH;
    px0 = (t - ty * TILES_X) * PTW;
  };
  u32x4 pre[U8IN ? 1 : PF];
  unsigned praw[U8IN ? PFR : 1];
  auto fetch = [&](int tile) {  // global -> registers: the input patch of `tile`
    int b, py0, px0;
    tile_origin(tile, b, py0, px0);
    const int R0 = 2 * (2 * py0 - 1), C0 = 2 * (2 * px0 - 1);
    if constexpr (U8IN) {
      // raw bytes of image rows R0-3 .. , columns C0-3 .. C0+32, as aligned dwords.  The byte offset of
      // window row `row` is tile_base + row * 672 with ONE 64-bit scalar per tile; its misalignment
      // sh = offset & 3 is the same for every row and image (a row is 672 = 0 mod 4 bytes), so the
      // per-lane part is 32-bit arithmetic only
      const unsigned char* src = reinterpret_cast<const unsigned char*>(xin_);
      const int sh = ((C0 - 3) * 3) & 3;
      const long long tile_base = (((long long)b * kPatch + (R0 - 3)) * kPatch + (C0 - 3)) * 3 - sh;
      const long long lo = -tile_base, hi = in_bytes - 4 - tile_base;  // valid range of the per-lane offset
      const int lo32 = lo > 0 ? (lo < 0x7fffffff ? (int)lo : 0x7fffffff) : 0;
      const int hi32 = hi < 0 ? -1 : (hi < 0x7fffffff ? (int)hi : 0x7fffffff);
      static_for<PFR>([&](auto I) {
        constexpr int k = decltype(I)::value;
        const int i = tid + 256 * k;
        const int row = i / RAWDW, j = i - row * RAWDW;
        const int y = R0 + row - 3;
        const int voff = row * (kPatch * 3) + 4 * j;
        const bool ok = i < NRAW && (unsigned)y < (unsigned)kPatch && voff >= lo32 && voff <= hi32;
        const unsigned v = *reinterpret_cast<const unsigned*>(src + tile_base + (ok ? voff : lo32));
        praw[k] = ok ? v : 0u;
      });
    } else {
      const char* img = reinterpret_cast<const char*>(xin) + (size_t)b * kPadH * kPadW * 8;
      static_for<PF>([&](auto I) {
        constexpr int k = decltype(I)::value;
        const int i = tid + 256 * k;
        const int row = i / PPR, cp = i - row * PPR;
        const int R = R0 + row, C = C0 + 2 * cp;
        const bool ok = i < NPIECE && R >= 0 && C >= 0 && R < kPadH && C + 1 < kPadW;
        const u32x4 v = *reinterpret_cast<const u32x4*>(img + (ok ? ((size_t)R * kPadW + C) * 8 : 0));
        pre[k] = ok ? v : u32x4{0u, 0u, 0u, 0u};
      });
    }
  };
  auto stash = [&](int buf) {  // registers -> LDS (patch buffer, or the raw window when U8IN)
    if constexpr (U8IN) {
      static_for<PFR>([&](auto I) {
        constexpr int k = decltype(I)::value;
        const int i = tid + 256 * k;
        if (i < NRAW) *reinterpret_cast<unsigned*>(Rl + i * 4) = praw[k];
      });
    } else {
      static_for<PF>([&](auto I) {
        constexpr int k = decltype(I)::value;
        const int i = tid + 256 * k;
        if (i < NPIECE) *reinterpret_cast<u32x4*>(smem + buf * P_BYTES + i * 16) = pre[k];
      });
    }
  };
  // U8IN only: raw window -> normalised T NHWC4 patch (pairs of pixels = 16-byte pieces)
  auto convert = [&](int tile, int buf) {
    int b, py0, px0;
    tile_origin(tile, b, py0, px0);
    const int R0 = 2 * (2 * py0 - 1), C0 = 2 * (2 * px0 - 1);
    const int sh = ((C0 - 3) * 3) & 3;  // misalignment of the window's first byte: the same for every row
    for (int i = tid; i < NPIECE; i += 256) {
      const int row = i / PPR, cp = i - row * PPR;
      const int y = R0 + row - 3;
      const unsigned char* rr = Rl + row * RAWROW + sh + 6 * cp;  // byte of channel 0 of the first pixel
      u32x4 v = {0u, 0u, 0u, 0u};
      if ((unsigned)y < (unsigned)kPatch) {
#pragma unroll
        for (int px = 0; px < 2; ++px) {
          const int x = C0 + 2 * cp + px - 3;
          if ((unsigned)x < (unsigned)kPatch) {
            const unsigned c0 = Ll[rr[3 * px + 0]], c1 = Ll[256 + rr[3 * px + 1]], c2 = Ll[512 + rr[3 * px + 2]];
            v[2 * px] = c0 | (c1 << 16);
            v[2 * px + 1] = c2;
          }
        }
      }
      *reinterpret_cast<u32x4*>(smem + buf * P_BYTES + i * 16) = v;
    }
  };

  int tile = blockIdx.x;
  if (tile < n_tiles) {
    fetch(tile);
    stash(0);
    if constexpr (U8IN) {
      __syncthreads();
      convert(tile, 0);
    }
  }
  __syncthreads();
  for (int it = 0; tile < n_tiles; tile += gridDim.x, ++it) {
    const int buf = it & 1;
    const bool more = tile + (int)gridDim.x < n_tiles;
    if (more) fetch(tile + gridDim.x);  // in flight behind the MFMAs
    int b, py0, px0;
    tile_origin(tile, b, py0, px0);
    const int sy0 = 2 * py0 - 1, sx0 = 2 * px0 - 1;
    const unsigned char* Pl = smem + buf * P_BYTES;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
#ifdef HIPAC_ABL_STEM_NO_MFMA
    if (n_tiles < 0)
#endif
#pragma unroll
    for (int kh = 0; kh < 7; ++kh) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        frag af[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const frag*>(Pl + a_rd[i] + kh * (PCOLS * 8) + kk * 32);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = E::mfma(wreg[j][kh][kk], af[i], acc[i][j]);
      }
    }
    // bias + ReLU -> LDS stem tile [pixel][64 ch]; out-of-image stem pixels become 0
#ifdef HIPAC_ABL_STEM_NO_EPI
    if (n_tiles < 0)
#endif
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bool inside = (sy0 + ly[i]) >= 0 && (sx0 + lx[i]) >= 0 && P[i] < NPX;
      const unsigned inside_mask = inside ? 0xffffffffu : 0u;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          typename E::vec4 ov;
          ov[0] = (T)fmaxf(acc[i][j][4 * q + 0] + bv[j][q].x, 0.f);
          ov[1] = (T)fmaxf(acc[i][j][4 * q + 1] + bv[j][q].y, 0.f);
          ov[2] = (T)fmaxf(acc[i][j][4 * q + 2] + bv[j][q].z, 0.f);
          ov[3] = (T)fmaxf(acc[i][j][4 * q + 3] + bv[j][q].w, 0.f);
          // out-of-image stem pixels become +0: one AND per packed dword instead of a select per value
          u32x2 pk = __builtin_bit_cast(u32x2, ov);
          pk[0] &= inside_mask;
          pk[1] &= inside_mask;
          *reinterpret_cast<u32x2*>(Sl + sidx[i] * SPX + (j * 32 + 8 * q + 4 * h) * 2) = pk;
        }
    }
    __syncthreads();  // stem tile complete; every wave is past its reads of patch[buf ^ 1]
    if (more) stash(buf ^ 1);  // patch[buf^1] (raw window) was last read in the previous iteration
    // 3x3/2 max-pool of the tile: pooled pixel x 8 channels per thread item
#ifdef HIPAC_ABL_STEM_NO_POOL
    if (n_tiles < 0)
#endif
    for (int item = tid; item < PTH * PTW * 8; item += 256) {
      const int pp = item >> 3, c8 = item & 7;
      const int py = pp / PTW, px = pp - py * PTW;
      // values are post-ReLU (sign bit clear, or -0.0): their 16-bit patterns order like
      // signed integers, so the max is a packed integer max -- no conversions
      s16x8 best = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
          best = __builtin_elementwise_max(
              best, *reinterpret_cast<const s16x8*>(Sl + ((2 * py + dy) * STW + 2 * px + dx) * SPX + c8 * 16));
      const frag o = __builtin_bit_cast(frag, best);
      *reinterpret_cast<frag*>(out + (((size_t)b * 56 + py0 + py) * 56 + px0 + px) * 64 + c8 * 8) = o;
    }
    __syncthreads();  // pooling reads done (stem tile free) and patch[buf ^ 1] / raw window visible
    if constexpr (U8IN) {
#ifndef HIPAC_ABL_STEM_NO_CONVERT
      if (more) convert(tile + gridDim.x, buf ^ 1);
#endif
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------
// Fused stem, uint8 input, second form ("strip" kernel, stem_pool_strip2_kernel below): the same 7x7/2 conv +
// BN + ReLU + 3x3/2 max-pool on raw uint8 HWC patches, restructured around the MFMA loop:
//   * ToTensor / Normalize are folded into the weights and the bias at pack time: the kernel
//     multiplies the centred byte value v - 128 (an exact integer in bf16 and fp16) by w'' = w / (255 std_c)
//     and a bias table carries sum(w'' (128 - mu''_c)), mu''_c = 255 mean_c, over the taps inside the image and
//     128 sum(w'') over the taps outside (bytes there arrive as 0, i.e. -128, where the reference pads with the
//     normalised 0).  No per-pixel rounding of the input.
//   * K is packed as (channel plane c, row pair rp, column quad cq) = 3 x 4 x 2 fragments of 8
//     = 192 (147 real), 12 k16 steps instead of 14.  In LDS a plane holds, per column, the two rows
//     of a row pair in one dword, so the fragment of stem column sx (input columns 2sx-3+4cq ..+3,
//     rows 2sy-3+2rp, +1) is 16 contiguous bytes at 8 * sx + const: two conflict-free ds_read_b64,
//     no replication of the patch, offsets are immediates.
//   * lane = stem COLUMN, MFMA sub-tile = stem ROW: the 3x3/2 max-pool is a v_max3 over three
//     accumulator sets (rows) of the same lane and two lane shifts; the stem tile never goes to
//     LDS.  A workgroup walks DOWN a strip of 28 pooled columns (half the image width; wave =
//     (channel half, 14-column half)), 4 pooled rows = 8 stem rows per step, and carries the last stem
//     row in registers into the next step, so no stem row is computed twice in y
//     (MFMA efficiency = 28/32 columns x 147/192 of K).
//   * input rows arrive by LDS-DMA (buffer_load ... lds, dword pieces, range-checked) one step
//     ahead; the conversion reads them as aligned dwords and writes 16-byte pieces.
// ---------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void buffer_load_lds4(rsrc_t rs, void* lds, int voffset, int soffset) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds, 4, voffset, soffset, 0, 0);
}
#else
__device__ inline void buffer_load_lds4(rsrc_t, void*, int, int) {}
#endif
constexpr int kStripSteps = 14;  // 56 pooled rows / 4 per step

// ---------------------------------------------------------------------------------------
// Schedule: ONE 8-wave workgroup per CU holds two TEAMS of four waves (team = wave >> 2, i.e. the two
// waves that share a SIMD belong to different teams).  A team works on its own strips with its own LDS;
// its step is cut into two halves that alternate behind ONE workgroup barrier per half:
//     H1(n): the 96-MFMA loop of step n . request the input rows of step n+1 (LDS-DMA)
//     H2(n): epilogue of step n (pooling in registers, store) . conversion of the rows of step n+1
// and team B runs one half behind team A: whenever one wave of a SIMD is in its MFMA loop its partner is
// in the VALU / LDS / store half -- matrix beside vector work, never matrix beside matrix.  Every wave
// converts exactly the raw rows it requested itself (its own counted vmcnt orders them), so no barrier
// is needed inside a half.  The bias is the initial accumulator; ReLU is one packed integer max after
// the x max; the pooled rows leave through per-wave LDS staging as 64 contiguous bytes per pixel.
// ---------------------------------------------------------------------------------------
#ifndef HIPAC_STRIP_PRIO
#define HIPAC_STRIP_PRIO 2  // 0: no s_setprio, 1: around the MFMA loop, 2: on the vector half
#endif
// SPLIT (fp16x3 mode): the byte values are exact in fp16, so only the weights are pairs: `wgt` holds the hi halves
// [64][192] followed by the lo halves [64][192]; hi stays in registers, lo is fetched from LDS per channel plane, and
// every fragment feeds two MFMAs per (row, row pair).  The pooling stays in fp32 (v_max3 in y, two DPP shifts in x,
// ReLU) and the pooled rows leave as (hi, lo) pairs [pixel][hi: 64 | lo: 64], hi then lo through the same staging.
// Q8 (precision fp16q8): the pooled map's q8 tensor [pixel][lo8: 64 | hi8: 64] (halo16x2.h) is written too, from the same staging.
template <typename T, bool SPLIT = false, bool Q8 = false>
__global__ __launch_bounds__(512, 2) void stem_pool_strip2_kernel(const unsigned char* __restrict__ x,
                                                                  const T* __restrict__ wgt,
                                                                  const float* __restrict__ btab, T* __restrict__ out,
                                                                  int n_strips, int in_bytes, unsigned char* __restrict__ out_q = nullptr) {
  using E = Elem<T>;
  using frag = typename E::frag;
  static_assert(!SPLIT || std::is_same<T, _Float16>::value, "split pairs are fp16");
  static_assert(!Q8 || SPLIT, "the q8 tensor belongs to the pair layout");
  constexpr int OPIX = SPLIT ? 128 : 64;              // elements per output pixel
  constexpr int WLO_BYTES = SPLIT ? 2 * 12 * 1024 : 0;  // low weight halves in fragment order: [channel half][k16 step][lane] x 16 B
  constexpr int NRP = 11, PXW = 128;
  constexpr int PLANE = NRP * PXW * 4;
  constexpr int PATCH_BYTES = 3 * PLANE;              // 16 896
  constexpr int RAW_PITCH = 512, RAW_ROWS = 22;        // one 16-byte DMA instruction brings two rows (lanes 0-24, 32-56)
  constexpr int RAW_BYTES = RAW_ROWS * RAW_PITCH;     // 11 616
  constexpr int TEAM_BYTES = PATCH_BYTES + RAW_BYTES;
  constexpr int CARRY_BYTES = 512 * 64;               // per lane 16 floats: the raw last stem row of the previous step
  constexpr int STG_BYTES = 4 * 14 * 64;              // per wave: 4 pooled rows x 14 pixels x 32 channels of T
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * TEAM_BYTES + CARRY_BYTES + 8 * STG_BYTES + 4096 + WLO_BYTES];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int team = wave >> 2, tw = wave & 3;          // team, wave inside the team
  const int jt = tw & 1, st = tw >> 1;                // channel half, 14-column half of the strip
  const int r = lane & 31, h = lane >> 5;
  unsigned char* const Pl = smem + team * TEAM_BYTES;
  unsigned char* const Rl = Pl + PATCH_BYTES;
  unsigned char* const Cl = smem + 2 * TEAM_BYTES + tid * 16;  // chunk k of this lane at + k * 8192 (conflict-free)
  // output staging of this wave (private: no barrier): [pooled row q][pixel k][64 B]; written by the lanes that
  // hold a pooled pixel (8 bytes each), read back as 224 linear 16-byte chunks and stored 64 contiguous
  // bytes per pixel -- per-lane 8-byte stores to 28 different lines cost 2 700 cycles per step
  unsigned char* const Sl = smem + 2 * TEAM_BYTES + CARRY_BYTES + wave * STG_BYTES;
  // Initial accumulators, in LDS (a global load inside the step loop would wait -- vmcnt retires in order -- for the
  // rows just requested): table [row class][column class][64 channels] = folded bias + the border correction.
  // Every byte outside the image arrives as 0 (rows and whole dwords of columns are zero-filled by the DMA's range
  // check: nothing to mask in the conversion) and is fed as 0 - 128, while the reference pads with the normalised 0,
  // i.e. the byte value mu_c = 255 mean_c: the difference depends only on which taps are outside -- stem row
  // 0 / 1 / 111 / other x stem column 0 / 1 / 111 / other -- and is part of the table.
  float* const Bl = reinterpret_cast<float*>(smem + 2 * TEAM_BYTES + CARRY_BYTES + 8 * STG_BYTES);
  for (int i = tid; i < 16 * 64; i += 512) Bl[i] = btab[i];  // visible after the first phase barrier (first read: H1(0))
  int s_off[4];  // element offset of chunk lane + 64 m from the step's first pixel
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int c = lane + 64 * m, pix = c >> 2;
    const int q = (pix * 147) >> 11, k = pix - 14 * q;
    // SPLIT: the staging holds two pooled rows at a time, hi rows then lo rows: staged row q = (half, row & 1)
    s_off[m] = SPLIT ? ((q & 1) * 56 + k) * 128 + (q >> 1) * 64 + (c & 3) * 8 : (q * 56 + k) * 64 + (c & 3) * 8;
  }
  // Q8: staged items c < 112 are the hi halves of (pooled row c / 56, pixel, 8 channels), item c + 112 the lo halves of the same
  int q_off[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int c = lane + 64 * m, pix = c >> 2;
    const int q = pix >= 14 ? 1 : 0, k = pix - 14 * q;
    q_off[m] = (q * 56 + k) * 128 + (c & 3) * 8;
  }

  const float unscale = SPLIT ? btab[16 * 64] : 1.f;  // 2^-S of the split weights' scale (pack_stem_u8)
  frag wreg[12];
  unsigned char* const Wl = smem + 2 * TEAM_BYTES + CARRY_BYTES + 8 * STG_BYTES + 4096 + jt * (12 * 1024) + lane * 16;
  {
    const char* wb = reinterpret_cast<const char*>(wgt) + (size_t)(jt * 32 + r) * (192 * 2) + 16 * h;
    if constexpr (SPLIT) {
      if (team == 0 && st == 0) {  // one wave per channel half parks the lo fragments (visible after the first phase barrier)
#pragma unroll
        for (int s = 0; s < 12; ++s)
          *reinterpret_cast<frag*>(Wl + s * 1024) = *reinterpret_cast<const frag*>(wb + 64 * 192 * 2 + s * 32);
      }
    }
#pragma unroll
    for (int s = 0; s < 12; ++s) wreg[s] = *reinterpret_cast<const frag*>(wb + s * 32);
#pragma unroll
    for (int s = 0; s < 12; ++s) asm volatile("" ::"v"(wreg[s]));
  }
  const rsrc_t in_rsrc = make_rsrc(x, in_bytes);

  // rows owned by this wave: window rows 6 tw .. 6 tw + 5 (row pairs 3 tw .. 3 tw + 2); wave 3 owns rows
  // 18 .. 20 (row 21 does not exist)
  // (wave 3: rows 18 .. 20; its fourth request covers row 20 and the nonexistent row 21 -> zeros)
  auto issue_dma = [&](int strip, int ys) {
    const int b = strip >> 1, side = strip & 1;
    const int base = b * (kPatch * kPatch * 3) + (16 * ys - 3) * (kPatch * 3) + 3 * (112 * side - 5) - 1;  // multiple of 16
    // lane -> (row of the pair, 16-byte chunk); chunks outside the image columns read as zeros: side 0: chunk 0
    // (bytes 0..15 = columns -5..-1), side 1: chunks 22.. (columns 224..)
    const int sub = lane >> 5, ch16 = lane & 31;
    const bool col_ok = ch16 < 25 && (side == 0 ? ch16 >= 1 : ch16 < 22);
    static_for<3>([&](auto K) {
      constexpr int k = decltype(K)::value;
      if (tw < 3 || k < 2) {
        const int row = 6 * tw + 2 * k + sub;
        const int iy = 16 * ys - 3 + row;
        const bool ok = col_ok && (unsigned)iy < (unsigned)kPatch && row < 21;
        buffer_load_lds16(in_rsrc, Rl + (6 * tw + 2 * k) * RAW_PITCH, ok ? base + row * (kPatch * 3) + ch16 * 16 : (int)0x80000000, 0);
      }
    });
  };

  // conversion task of this lane: row pair 3 tw + (lane >> 4) (lanes 48..63 idle; wave 3: lanes 32..63), 8 columns
  const int cRp = 3 * tw + (lane >> 4), cxg = lane & 15;
  const bool ctask = (lane >> 4) < (tw < 3 ? 3 : 2);
  const unsigned char* const craw = Rl + (2 * cRp) * RAW_PITCH + cxg * 24;
  unsigned char* const cdst = Pl + cRp * (PXW * 4) + cxg * 32;
  auto convert = [&](int strip, int ys) {
    (void)strip, (void)ys;
    if (!ctask) return;
    unsigned da[7], db[7];
    {
      const u32x2 a0 = *reinterpret_cast<const u32x2*>(craw), a1 = *reinterpret_cast<const u32x2*>(craw + 8),
                  a2 = *reinterpret_cast<const u32x2*>(craw + 16);
      const u32x2 b0 = *reinterpret_cast<const u32x2*>(craw + RAW_PITCH),
                  b1 = *reinterpret_cast<const u32x2*>(craw + RAW_PITCH + 8),
                  b2 = *reinterpret_cast<const u32x2*>(craw + RAW_PITCH + 16);
      da[0] = a0[0], da[1] = a0[1], da[2] = a1[0], da[3] = a1[1], da[4] = a2[0], da[5] = a2[1];
      db[0] = b0[0], db[1] = b0[1], db[2] = b1[0], db[3] = b1[1], db[4] = b2[0], db[5] = b2[1];
      da[6] = *reinterpret_cast<const unsigned*>(craw + 24);
      db[6] = *reinterpret_cast<const unsigned*>(craw + RAW_PITCH + 24);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      unsigned o[8];
#pragma unroll
      for (int px = 0; px < 8; ++px) {
        const int w = 1 + 3 * px + c;  // byte inside the dword run
        // v - 128: still an exact integer in bf16 / fp16, and the fp32 accumulation no longer carries the DC term
        // 128 sum(w) (bytes outside the image arrive as 0 -> -128: the bias table accounts for them)
        o[px] = PackPair<T>::pack((float)((da[w >> 2] >> (8 * (w & 3))) & 0xffu) - 128.f,
                                  (float)((db[w >> 2] >> (8 * (w & 3))) & 0xffu) - 128.f);
      }
      *reinterpret_cast<u32x4*>(cdst + c * PLANE) = u32x4{o[0], o[1], o[2], o[3]};
      *reinterpret_cast<u32x4*>(cdst + c * PLANE + 16) = u32x4{o[4], o[5], o[6], o[7]};
    }
  };

  const unsigned char* const fbase = Pl + (2 * r + 56 * st) * 4 + 16 * h;
  const int tg = 2 * blockIdx.x + team, tstride = 2 * gridDim.x;   // this team's strips: tg, tg + tstride, ...
  const int my_strips = tg < n_strips ? (n_strips - tg + tstride - 1) / tstride : 0;
  const int n_steps = my_strips * kStripSteps;
  // workgroup-uniform phase count: 2 halves per step + the prologue half, team B one phase behind
  const int max_strips = (n_strips - 2 * (int)blockIdx.x + tstride - 1) / tstride;  // team A's count >= team B's
  const int n_phases = 2 * max_strips * kStripSteps + 2;

#ifdef HIPAC_HALO_STAMPS
  unsigned long long z_sum[6] = {0, 0, 0, 0, 0, 0};
#endif
  f32x16 acc[8];
  const bool first_col_wave = st == 0;  // with side == 0: lane r == 0 is stem column -1
  for (int p = 0; p < n_phases; ++p) {
    const int hs = p - team - 1;            // half index of this team: -1 = prologue, 2n = H1(n), 2n+1 = H2(n)
    HALO_STAMP(z_t0);
    if (hs >= -1 && hs < 2 * n_steps) {
      const int n = hs >> 1;                // step (floor: -1 for the prologue)
      if (hs & 1) {
        // ---------------- H2(n): epilogue of step n, conversion of step n + 1 ----------------
#if HIPAC_STRIP_PRIO == 2
        __builtin_amdgcn_s_setprio(1);  // the vector half goes first: its partner needs one issue slot per 32 cycles
#endif
        const int strip = tg + ((n < 0 ? 0 : n) / kStripSteps) * tstride;
        const int ys = (n < 0 ? 0 : n) % kStripSteps;
#ifdef HIPAC_ABL_STRIP_NO_EPI
#pragma unroll
        for (int i = 0; i < 8; ++i) asm volatile("" ::"v"(acc[i]));
        if (n_strips < 0)
#endif
        if (n >= 0) {
          const int b = strip >> 1, side = strip & 1;
          f32x16 carry;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const f32x4 cv = *reinterpret_cast<const f32x4*>(Cl + k * 8192);
#pragma unroll
            for (int t = 0; t < 4; ++t) carry[4 * k + t] = ys == 0 ? -3.0e38f : cv[t];  // stem row -1 lies outside the image
          }
          const bool writer = (r & 1) == 0 && r <= 26;
          const bool col_m1 = side == 0 && first_col_wave && r == 0;  // this lane holds stem column -1
#ifdef HIPAC_ABL_STRIP_STORE_LOCAL
          T* const dst0 = out + (size_t)blockIdx.x * 16384 + jt * 32 + (b & 0);
#else
          T* const dst0 = out + ((((size_t)b * 56 + 4 * ys) * 56 + 28 * side + 14 * st) * OPIX + jt * 32);
#endif
          typedef __attribute__((ext_vector_type(2))) short s16x2;
          // SPLIT: rows go out two at a time (hi halves in staging rows 0, 1, lo halves in rows 2, 3)
          auto flush_pair = [&](int g) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's staging writes
#pragma unroll
            for (int m = 0; m < 4; ++m)
              if (m < 3 || lane < 32)
                store16_out(dst0 + g * (2 * 56 * 128) + s_off[m], *reinterpret_cast<const u32x4*>(Sl + (lane + 64 * m) * 16));
            if constexpr (Q8) {
              unsigned char* const qdst0 = out_q + ((((size_t)b * 56 + 4 * ys) * 56 + 28 * side + 14 * st) * 128 + jt * 32) + g * (2 * 56 * 128);
#pragma unroll
              for (int m = 0; m < 2; ++m)
                if (m < 1 || lane < 48) {
                  const f16x8 hv = *reinterpret_cast<const f16x8*>(Sl + (lane + 64 * m) * 16);
                  const f16x8 lv = *reinterpret_cast<const f16x8*>(Sl + (lane + 64 * m + 112) * 16);
                  u32x2 h8, l8;
#pragma unroll
                  for (int k = 0; k < 2; ++k) {
                    h8[k] = cvt4_e4m3((float)hv[4 * k], (float)hv[4 * k + 1], (float)hv[4 * k + 2], (float)hv[4 * k + 3]);
                    l8[k] = cvt4_e4m3((float)lv[4 * k] * kQ8LoScale, (float)lv[4 * k + 1] * kQ8LoScale, (float)lv[4 * k + 2] * kQ8LoScale,
                                      (float)lv[4 * k + 3] * kQ8LoScale);
                  }
                  *reinterpret_cast<u32x2*>(qdst0 + q_off[m]) = l8;
                  *reinterpret_cast<u32x2*>(qdst0 + q_off[m] + 64) = h8;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the reads have returned before the rows are overwritten
          };
          // one pooled row at a time: y max (fp32, v_max3), round to T, then the x max of lanes r, r+1, r+2 by two
          // DPP wave shifts and ReLU, both on the 16-bit patterns as SIGNED integers -- among non-negative
          // floats that is the float order, every negative float is below every non-negative one, and the
          // final max with +0 removes whatever negative value is left
          static_for<4>([&](auto Q) {
            constexpr int q = decltype(Q)::value;
            unsigned pk[8];
            unsigned lk_prev = 0;
            (void)lk_prev;
            if constexpr (SPLIT) {
              // fp32 all the way: y max, x max of lanes r, r+1, r+2 (two wave shifts), ReLU; then the (hi, lo) split
#pragma unroll
              for (int d = 0; d < 8; ++d) {
                float pv[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                  const int e = 2 * d + t;
                  const float top = q == 0 ? carry[e] : acc[q == 0 ? 0 : 2 * q - 1][e];
                  const float a0 = col_m1 ? -3.0e38f : fmaxf(fmaxf(top, acc[2 * q][e]), acc[2 * q + 1][e]);
                  const float a1 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, a0), 0x130, 0xf, 0xf, false));
                  const float t1 = fmaxf(a0, a1);
                  const float u2 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, t1), 0x130, 0xf, 0xf, false));
                  pv[t] = fmaxf(fmaxf(t1, u2), 0.f) * unscale;
                }
                const f16x2 h2 = __builtin_convertvector(f32x2{pv[0], pv[1]}, f16x2);
                const f16x2 l2 = __builtin_convertvector(f32x2{pv[0] - (float)h2[0], pv[1] - (float)h2[1]}, f16x2);
                pk[d] = __builtin_bit_cast(unsigned, h2);
                if (writer && (d & 1))  // (d - 1, d) = one 8-byte item of channel quad d / 2
                  *reinterpret_cast<u32x2*>(Sl + ((2 + (q & 1)) * 14 + (r >> 1)) * 64 + (d >> 1) * 16 + h * 8) =
                      u32x2{lk_prev, __builtin_bit_cast(unsigned, l2)};
                lk_prev = __builtin_bit_cast(unsigned, l2);
              }
            } else {
#pragma unroll
            for (int cq = 0; cq < 4; ++cq) {
              float v[4];
#pragma unroll
              for (int t = 0; t < 4; ++t) {
                const int e = 4 * cq + t;
                const float top = q == 0 ? carry[e] : acc[q == 0 ? 0 : 2 * q - 1][e];
                v[t] = fmaxf(fmaxf(top, acc[2 * q][e]), acc[2 * q + 1][e]);
              }
              pk[2 * cq] = PackPair<T>::pack_rn(v[0], v[1]);
              pk[2 * cq + 1] = PackPair<T>::pack_rn(v[2], v[3]);
            }
            }
            if constexpr (!SPLIT)
#pragma unroll
            for (int d = 0; d < 8; ++d) {
              const unsigned a0 = col_m1 ? 0x80008000u : pk[d];  // -0.0: below every value as int16, never wins
              const unsigned a1 = __builtin_amdgcn_update_dpp(0u, a0, 0x130, 0xf, 0xf, false);  // wave_shl:1
              const s16x2 t1 = __builtin_elementwise_max(__builtin_bit_cast(s16x2, a0), __builtin_bit_cast(s16x2, a1));
              const unsigned u2 = __builtin_amdgcn_update_dpp(0u, __builtin_bit_cast(unsigned, t1), 0x130, 0xf, 0xf, false);
              const s16x2 t2 = __builtin_elementwise_max(t1, __builtin_bit_cast(s16x2, u2));
              pk[d] = __builtin_bit_cast(unsigned, __builtin_elementwise_max(t2, s16x2{0, 0}));
            }
            if (writer) {
#pragma unroll
              for (int cq = 0; cq < 4; ++cq)
                *reinterpret_cast<u32x2*>(Sl + ((SPLIT ? (q & 1) : q) * 14 + (r >> 1)) * 64 + cq * 16 + h * 8) = u32x2{pk[2 * cq], pk[2 * cq + 1]};
            }
            if constexpr (SPLIT && q == 1) flush_pair(0);
          });
#pragma unroll
          for (int k = 0; k < 4; ++k)
            *reinterpret_cast<f32x4*>(Cl + k * 8192) = f32x4{acc[7][4 * k], acc[7][4 * k + 1], acc[7][4 * k + 2], acc[7][4 * k + 3]};
          if constexpr (SPLIT) {
            flush_pair(1);
          } else {
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's staging writes (LDS operations of a wave complete in order)
#ifdef HIPAC_ABL_STRIP_NO_STORE
          if (n_strips < 0)
#endif
#pragma unroll
          for (int m = 0; m < 4; ++m)
            if (m < 3 || lane < 32)
              store16_out(dst0 + s_off[m], *reinterpret_cast<const u32x4*>(Sl + (lane + 64 * m) * 16));
          }
        }
        HALO_STAMP(z_te);
#ifdef HIPAC_HALO_STAMPS
        if (n >= 0) z_sum[1] += z_te - z_t0, z_sum[4] += 1;
#endif
        if (n + 1 < n_steps) {
          const int gn = n + 1;
          if (n < 0) {
            issue_dma(tg, 0);  // prologue: nothing was requested yet
            wait_vmcnt<0>();
          } else {
            wait_vmcnt<Q8 ? 16 : SPLIT ? 8 : 4>();  // this wave's raw rows of step n+1 (requested at the end of H1(n)) are older than its 4 (8; Q8: 16) stores
          }
          HALO_STAMP(z_tw);
#ifdef HIPAC_ABL_STRIP_NO_CONVERT
          if (n_strips < 0)
#endif
          convert(tg + (gn / kStripSteps) * tstride, gn % kStripSteps);
#ifdef HIPAC_HALO_STAMPS
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          HALO_STAMP(z_tc);
          if (n >= 0) z_sum[2] += z_tw - z_te, z_sum[3] += z_tc - z_tw;
#endif
          // (the raw rows are consumed -- this wave converts only rows it requested itself -- but those of step n + 2 are
          // NOT requested here: hipcc puts a `s_waitcnt vmcnt(0)` in front of the first LDS read behind an LDS-DMA, and that read
          // is H1's bias read, so H1 began by waiting out the round trip of rows nobody needs before H2.  H1 requests them
          // itself, behind its last LDS read.)
        }
      } else {
        // ---------------- H1(n): MFMA loop of step n, request the rows of step n + 1 ----------------
        f32x16 binit;
        {
          const int strip1 = tg + (n / kStripSteps) * tstride, ys1 = n % kStripSteps, side1 = strip1 & 1;
          // column class of this lane's stem column (0 interior, 1: column 0, 2: column 1, 3: column 111)
          const int cc = (side1 == 0 && st == 0) ? (r == 1 ? 1 : (r == 2 ? 2 : 0)) : ((side1 == 1 && st == 1 && r == 28) ? 3 : 0);
          const float* bl = Bl + cc * 64 + jt * 32 + 4 * h;
          // rows 2..6 never have a special class: their accumulators start as the C operand of their first MFMA
          // (binit, 16 registers) instead of 80 v_mov; rows 0, 1, 7 are set here (from the row-class table when needed)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(bl + 8 * q);
            binit[4 * q + 0] = v.x, binit[4 * q + 1] = v.y, binit[4 * q + 2] = v.z, binit[4 * q + 3] = v.w;
          }
          acc[0] = binit, acc[1] = binit, acc[7] = binit;
          if (ys1 == 0 || ys1 == kStripSteps - 1) {  // uniform: stem rows 0, 1 (first step) / 111 (last step) have taps above / below the image
            static_for<3>([&](auto RC) {
              constexpr int rc = decltype(RC)::value + 1;
              constexpr int i = rc == 1 ? 0 : (rc == 2 ? 1 : 7);
              if ((rc == 3) == (ys1 != 0)) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  const float4 v = *reinterpret_cast<const float4*>(bl + rc * 256 + 8 * q);
                  acc[i][4 * q + 0] = v.x, acc[i][4 * q + 1] = v.y, acc[i][4 * q + 2] = v.z, acc[i][4 * q + 3] = v.w;
                }
              }
            });
          }
        }
#if HIPAC_STRIP_PRIO == 1
        __builtin_amdgcn_s_setprio(1);
#endif
        // Fragment (plane c, row pair j) feeds the up to four MFMAs (i, rp) with i + rp = j, so the loop runs over
        // the 33 fragments, each read ONCE, two fragments ahead of its MFMAs (3-slot register ring, order pinned:
        // left to itself hipcc issues a read right in front of the MFMA that needs it and exposes the LDS latency
        // ~25 times per step).  acc[i] is touched at most once per group of 4 MFMAs: no dependent-MFMA stalls.
#ifdef HIPAC_ABL_STRIP_NO_MFMA
        if (n_strips < 0)
#endif
        {
          frag ring3[3];
          auto rd = [&](auto F) {
            constexpr int f = decltype(F)::value;      // f = c * 11 + j
            const unsigned char* pp = fbase + f * (PXW * 4);
            const u32x2 lo = *reinterpret_cast<const u32x2*>(pp), hi = *reinterpret_cast<const u32x2*>(pp + 8);
            ring3[f % 3] = __builtin_bit_cast(frag, u32x4{lo[0], lo[1], hi[0], hi[1]});
          };
          frag wlo[SPLIT ? 4 : 1];  // SPLIT: the lo weight fragments of the current channel plane
          auto rdw = [&](int c_) {
            if constexpr (SPLIT) {
#pragma unroll
              for (int rp = 0; rp < 4; ++rp) wlo[rp] = *reinterpret_cast<const frag*>(Wl + (c_ * 4 + rp) * 1024);
            }
          };
          rdw(0);
          rd(std::integral_constant<int, 0>{});
          rd(std::integral_constant<int, 1>{});
          static_for<33>([&](auto F) {
            constexpr int f = decltype(F)::value, c = f / NRP, j = f % NRP;
            if constexpr (f + 2 < 33) rd(std::integral_constant<int, f + 2>{});
            static_for<4>([&](auto RP) {
              constexpr int rp = decltype(RP)::value, i = j - rp;
              if constexpr (i >= 0 && i < 8) {
                if constexpr (c == 0 && rp == 0 && i >= 2 && i <= 6) acc[i] = E::mfma(wreg[0], ring3[f % 3], binit);
                else acc[i] = E::mfma(wreg[c * 4 + rp], ring3[f % 3], acc[i]);
              }
            });
            if constexpr (SPLIT) {
              static_for<4>([&](auto RP) {
                constexpr int rp = decltype(RP)::value, i = j - rp;
                if constexpr (i >= 0 && i < 8) acc[i] = E::mfma(wlo[rp], ring3[f % 3], acc[i]);
              });
              if constexpr (j == NRP - 1 && c < 2) rdw(c + 1);  // the next plane's lo fragments, one fragment ahead
            }
            __builtin_amdgcn_sched_barrier(0);
          });
        }
        // the rows of step n + 1, converted in H2(n) behind its epilogue: the round trip hides behind the pooling and the stores.
        // Issued behind the MFMA loop's last LDS read (at the start of H1 the address arithmetic sat in front of the MFMAs, and
        // the compiler's wait in front of the fragment reads); the raw rows' last reader was this wave's own convert in H2(n-1).
#ifdef HIPAC_ABL_STRIP_NO_DMA
        if (n_strips < 0)
#endif
        if (n + 1 < n_steps) issue_dma(tg + ((n + 1) / kStripSteps) * tstride, (n + 1) % kStripSteps);
#if HIPAC_STRIP_PRIO == 1
        __builtin_amdgcn_s_setprio(0);
#endif
#ifdef HIPAC_HALO_STAMPS
#pragma unroll
        for (int i = 0; i < 8; ++i) asm volatile("" ::"v"(acc[i]));
        HALO_STAMP(z_tm);
        z_sum[0] += z_tm - z_t0;
#endif
      }
    }
    HALO_STAMP(z_tb0);
#if HIPAC_STRIP_PRIO == 2
    __builtin_amdgcn_s_setprio(0);
#endif
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // half boundary: patch written <-> patch read, for both teams
#ifdef HIPAC_HALO_STAMPS
    HALO_STAMP(z_tb1);
    z_sum[5] += z_tb1 - z_tb0;
#endif
  }
#ifdef HIPAC_HALO_STAMPS
  if (lane == 0) {
    atomicAdd(&g_halo_stamps[0], z_sum[0]);  // H1: DMA issue + bias + MFMA loop
    atomicAdd(&g_halo_stamps[1], z_sum[1]);  // H2: epilogue
    atomicAdd(&g_halo_stamps[2], z_sum[2]);  // H2: wait for the raw rows
    atomicAdd(&g_halo_stamps[4], z_sum[3]);  // H2: conversion
    atomicAdd(&g_halo_stamps[5], z_sum[5]);  // barrier waits
    atomicAdd(&g_halo_stamps[3], z_sum[4]);  // wave-steps
  }
#endif
}

}  // namespace hipac

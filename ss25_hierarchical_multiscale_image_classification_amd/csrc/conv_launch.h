// Host launchers of the convolution kernels: which kernel a layer shape runs on, its grid and its dynamic LDS.
#pragma once
#include "conv_v1.h"
#include "conv_glds.h"
#include "layer1_c64.h"
#include "halo16.h"
#include "halo16x2.h"

namespace hipac {

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE attribute: set it once per (kernel, device)
constexpr int kMaxDevices = 64;
static inline int ensure_dynamic_lds(const void* kern, int lds, bool* done) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = -1;
  if (dev >= 0 && done[dev]) return 0;
  hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return (int)e;
  if (dev >= 0) done[dev] = true;
  return 0;
}

#ifndef HIPAC_BM_A
#define HIPAC_BM_A 128
#endif
#ifndef HIPAC_NSTAGE_A
#define HIPAC_NSTAGE_A 2
#endif
#ifndef HIPAC_NSTAGE_B
#define HIPAC_NSTAGE_B 2
#endif
#ifndef HIPAC_BM_64
#define HIPAC_BM_64 256
#endif
// Tile shape per layer: COUT = 64 -> 256 pixels x 64 channels (4 waves);
// otherwise 128 x 128 (4 waves, 4-stage ring).
#ifndef HIPAC_BN_A
#define HIPAC_BN_A 128
#endif
template <int BM_, int BN_, int NSTAGE_> struct GldsTile {  // conv_glds_kernel's tile with its workgroup size and LDS ring
  static constexpr int BM = BM_, BN = BN_, NSTAGE = NSTAGE_, THREADS = (BM / 64) * (BN / 64) * 64, LDS = NSTAGE * (BM + BN) * 128;
};
template <int COUT> struct TileCfg : GldsTile<HIPAC_BM_A, (COUT % HIPAC_BN_A == 0 ? HIPAC_BN_A : 128), HIPAC_NSTAGE_A> {};
template <> struct TileCfg<64> : GldsTile<HIPAC_BM_64, 64, HIPAC_NSTAGE_B> {};

// the stride-1 halo16 kernel's weight ring: the deepest (NSW slots) that keeps two workgroups per CU; its dynamic LDS (band,
// ring, bias) is halo16_lds_bytes' (halo16.h)
template <int W, int BM, int BN, int COUT>
struct Halo16Lds {
  static constexpr int NSW = halo16_lds_bytes(W, BM, BN, 3, COUT) <= 80 * 1024 ? 3 : 2;
  static constexpr int LDS = halo16_lds_bytes(W, BM, BN, NSW, COUT);
};

// The grid of the tiled kernels (conv_glds_kernel, the halo kernels) is 1-D and decoded XCD-aware: virtual block v is pixel tile
// (v >> 3) / ctiles * 8 + (v & 7), channel tile (v >> 3) % ctiles.  The pixel-tile count is therefore padded to a multiple of 8 (a
// block whose tile is >= n_mtiles has nothing to do).  cap = 0: one workgroup per virtual block; cap > 0 (the persistent halo
// kernels, HIPAC_HALO_GRID): at most `cap` workgroups that stride over the virtual blocks by the grid size -- both are
// multiples of 8, so a workgroup stays on its XCD and the padded blocks come out whole.
struct TileGrid { int n_mtiles; unsigned blocks; };
static inline TileGrid tile_grid(int M, int BM, int ctiles, int cap) {
  const int n_mtiles = (M + BM - 1) / BM;
  const int mt8 = (n_mtiles + 7) / 8 * 8;
  const int n_vtiles = mt8 * ctiles;
  return {n_mtiles, (unsigned)(cap > 0 && cap < n_vtiles ? cap : n_vtiles)};
}

// launch of a kernel with dynamic LDS on a 1-D grid; returns the hipError_t value
template <auto KERN, typename... Args>
static int launch_dyn_lds(unsigned blocks, int threads, int lds, hipStream_t s, Args... args) {
  static bool attr_done[kMaxDevices] = {};  // per (kernel, device); a benign race at worst repeats the call
  if (int rc_attr = ensure_dynamic_lds((const void*)KERN, lds, attr_done)) return rc_attr;
  hipLaunchKernelGGL(KERN, dim3(blocks), dim3(threads), lds, s, args...);
  return (int)hipGetLastError();
}

template <typename T, int CIN, int COUT, int HI, int WI, int KS, int STRIDE, bool RELU, bool RESID,
          bool OUTF32, bool STEM = false, bool POOL = false>
static int launch_conv(const void* in, const ConvW& w, const void* resid, void* out, int n, hipStream_t s,
                       const char* zero_page = nullptr) {
  constexpr int PAD = STEM ? 0 : KS / 2;
  constexpr int HO = STEM ? 112 : (HI + 2 * PAD - KS) / STRIDE + 1;
  constexpr int WO = STEM ? 112 : (WI + 2 * PAD - KS) / STRIDE + 1;
  const int M = n * HO * WO;
  if constexpr (STEM || sizeof(T) == 4) {
    // the stem, and every layer of the fp32 parity mode (exact f32 MFMA), run on the v1 kernel
    constexpr int BN = 64;
    dim3 grid((M + 127) / 128, COUT / BN);
    hipLaunchKernelGGL((conv_igemm_kernel<T, CIN, COUT, HI, WI, KS, STRIDE, BN, RELU, RESID, OUTF32, STEM>),
                       grid, dim3(256), 0, s, (const T*)in, (const T*)w.w, w.bias, (const T*)resid, out, M);
  } else if constexpr (KS == 3 && STRIDE == 1 && CIN == 64 && COUT == 64 && HI == 56 && !OUTF32) {
    const int n_tiles = n * 49;
    const int n_units = (n_tiles + 1) / 2;
    const int grid = n_units < 512 ? n_units : 512;  // persistent, 2 workgroups per CU
    hipLaunchKernelGGL((conv3x3_c64_kernel<T, RESID, RELU>), dim3(grid), dim3(256), 0, s, (const T*)in, (const T*)w.w,
                       w.bias, (const T*)resid, (T*)out, n_tiles, zero_page);
  } else if constexpr (KS == 3 && STRIDE == 2 && !OUTF32 && !RESID && COUT % 128 == 0 && HI == WI) {
    // the entry convs of layers 2-4 on halo16's stride-2 form: four parity-plane bands per 64-channel chunk
    constexpr int BM = 256, BN = 128, NSW = 2;
    constexpr int LDS = halo16_lds_bytes(WO, BM, BN, NSW, COUT);
    constexpr auto kern = conv3x3_halo16_kernel<T, CIN, COUT, HO, WO, BM, BN, NSW, RELU, false, false, 0, false, true>;
    const TileGrid g = tile_grid(M, BM, COUT / BN, HIPAC_HALO_GRID);
    return launch_dyn_lds<kern>(g.blocks, 256, LDS, s, (const T*)in, (const T*)w.w, w.bias, (const T*)nullptr, out, M, n, g.n_mtiles,
                                zero_page, (const T*)nullptr);
  } else if constexpr (KS == 3 && STRIDE == 1) {
    // layers 2-4: 256-pixel x 128-channel tiles (each wave 128 px x 64 ch: 0.75 LDS reads per MFMA, half the weight DMA per FLOP)
    static_assert(COUT % 128 == 0, "the halo16 kernel takes 128-channel tiles");
    constexpr int BM = 256, BN = 128;
    using L = Halo16Lds<WI, BM, BN, COUT>;
    constexpr auto kern = conv3x3_halo16_kernel<T, CIN, COUT, HI, WI, BM, BN, L::NSW, RELU, RESID, OUTF32, 0, POOL>;
    const TileGrid g = tile_grid(M, BM, COUT / BN, HIPAC_HALO_GRID);
    return launch_dyn_lds<kern>(g.blocks, 256, L::LDS, s, (const T*)in, (const T*)w.w, w.bias, (const T*)resid, out, M, n, g.n_mtiles,
                                zero_page, (const T*)nullptr);
  } else {
    using G = TileCfg<COUT>;
    constexpr auto kern = conv_glds_kernel<T, CIN, COUT, HI, WI, KS, STRIDE, G::BM, G::BN, G::NSTAGE, RELU, RESID, OUTF32>;
    const TileGrid g = tile_grid(M, G::BM, COUT / G::BN, 0);
    return launch_dyn_lds<kern>(g.blocks, G::THREADS, G::LDS, s, (const T*)in, (const T*)w.w, w.bias, (const T*)resid, out, M,
                                g.n_mtiles, zero_page, (const T*)nullptr, (const float*)nullptr, (void*)nullptr);
  }
  return (int)hipGetLastError();
}

// second conv of a down-sampling block with the 1x1 / stride 2 projection folded in as extra K steps (halo kernel, PCIN):
// tmp = relu(conv1(x)) -> out = relu(conv2(tmp) + proj(x) + b2 + bp)
template <typename T, int CO, int HO, int PCIN>
static int launch_conv_projk(const void* tmp, const ConvW& w2, const ConvW& wp, const float* bias_sum, const void* xblk, void* out,
                             int n, hipStream_t s, const char* zero_page) {
  constexpr int BM = 256, BN = 128;
  using L = Halo16Lds<HO, BM, BN, CO>;
  constexpr auto kern = conv3x3_halo16_kernel<T, CO, CO, HO, HO, BM, BN, L::NSW, true, false, false, PCIN>;
  const int M = n * HO * HO;
  const TileGrid g = tile_grid(M, BM, CO / BN, HIPAC_HALO_GRID);
  return launch_dyn_lds<kern>(g.blocks, 256, L::LDS, s, (const T*)tmp, (const T*)w2.w, bias_sum, (const T*)xblk, out, M, n, g.n_mtiles,
                              zero_page, (const T*)wp.w);
}

// Data gradient of a stride-2 convolution (training) WITHOUT the zero-interleaved gradient map: the fine grid falls into four
// parity classes; input position (2y + PY, 2x + PX) only ever meets the taps kh with kh + PY odd ... i.e. kh = 1 for PY = 0 and
// kh in {0, 2} for PY = 1 (same in x): 1, 2, 2 and 4 taps instead of 9 each -- a quarter of the MFMAs of the 3x3 convolution
// over the zero-interleaved map.  `g` = gradient wrt the conv output on the coarse HC x HC grid [n][HC][HC][CG]; `wc` = the class's
// weights [CX][taps][CG] (pack mode 3 of train.hip / train_amp.hip); `dx` = [n][2 HC][2 HC][CX], this class's positions written.
template <typename T, int CG, int CX, int HC, int TKH, int TKW, int PY, int PX>
static int launch_dgrad_s2_class(const void* g, const void* wc, const float* zero_bias, void* dx, int n, hipStream_t s,
                                 const char* zero_page) {
  const int M = n * HC * HC;
  if constexpr (sizeof(T) == 4) {
    // the fp32 training step runs on the v1 kernel (exact f32 MFMA), as launch_conv does
    constexpr int BN = 64;
    dim3 grid((M + 127) / 128, CX / BN);
    hipLaunchKernelGGL((conv_igemm_kernel<T, CG, CX, HC, HC, 1, 1, BN, false, false, false, false, TKH, TKW, 4 | (PY << 1) | PX>), grid,
                       dim3(256), 0, s, (const T*)g, (const T*)wc, zero_bias, (const T*)nullptr, dx, M);
  } else {
    using G = TileCfg<CX>;
    constexpr auto kern =
        conv_glds_kernel<T, CG, CX, HC, HC, 1, 1, G::BM, G::BN, G::NSTAGE, false, false, false, false, TKH, TKW, 4 | (PY << 1) | PX>;
    const TileGrid tg = tile_grid(M, G::BM, CX / G::BN, 0);
    return launch_dyn_lds<kern>(tg.blocks, G::THREADS, G::LDS, s, (const T*)g, (const T*)wc, zero_bias, (const T*)nullptr, dx, M,
                                tg.n_mtiles, zero_page, (const T*)nullptr, (const float*)nullptr, (void*)nullptr);
  }
  return (int)hipGetLastError();
}
// all four classes of a 3x3 / stride 2 conv (KS3 = true) or the one class of a 1x1 / stride 2 conv (the other positions of dx
// must have been zeroed): wc = the four class blocks back to back (1, 2, 2, 4 taps) or the 1x1 matrix [CX][CG]
template <typename T, int CG, int CX, int HC, bool KS3>
static int launch_dgrad_s2(const void* g, const void* wc, const float* zero_bias, void* dx, int n, hipStream_t s, const char* zero_page) {
  const T* w = (const T*)wc;
  constexpr size_t blk = (size_t)CX * CG;
  if constexpr (!KS3) return launch_dgrad_s2_class<T, CG, CX, HC, 1, 1, 0, 0>(g, w, zero_bias, dx, n, s, zero_page);
  if (int rc = launch_dgrad_s2_class<T, CG, CX, HC, 1, 1, 0, 0>(g, w, zero_bias, dx, n, s, zero_page)) return rc;
  if (int rc = launch_dgrad_s2_class<T, CG, CX, HC, 1, 2, 0, 1>(g, w + blk, zero_bias, dx, n, s, zero_page)) return rc;
  if (int rc = launch_dgrad_s2_class<T, CG, CX, HC, 2, 1, 1, 0>(g, w + 3 * blk, zero_bias, dx, n, s, zero_page)) return rc;
  return launch_dgrad_s2_class<T, CG, CX, HC, 2, 2, 1, 1>(g, w + 5 * blk, zero_bias, dx, n, s, zero_page);
}

// 3x3 / stride 2 conv (+BN+ReLU) of a down-sampling BasicBlock with its 1x1 / stride 2 projection
// shortcut (+BN) riding along: x -> (out, out_p).  Layer2 on the register-weight kernel, layer3 on
// conv_glds_kernel<..., PROJ = true>
template <typename T, int CIN, int COUT, int HI>
static int launch_down(const void* in, const ConvW& w, const ConvW& wp, void* out, void* out_p, int n, hipStream_t s,
                       const char* zero_page) {
  if constexpr (CIN == 64 && COUT == 128 && HI == 56) {
    const int n_tiles = n * 28;
    const int grid = n_tiles < 512 ? n_tiles : 512;  // persistent, 2 workgroups per CU
    hipLaunchKernelGGL((conv3x3s2_c64_kernel<T>), dim3(grid), dim3(256), 0, s, (const T*)in, (const T*)w.w, w.bias,
                       (const T*)wp.w, wp.bias, (T*)out, (T*)out_p, n_tiles, zero_page);
  } else {
    using G = TileCfg<COUT>;
    constexpr int HO = HI / 2;
    const int M = n * HO * HO;
    constexpr auto kern = conv_glds_kernel<T, CIN, COUT, HI, HI, 3, 2, G::BM, G::BN, G::NSTAGE, true, false, false, true>;
    const TileGrid g = tile_grid(M, G::BM, COUT / G::BN, 0);
    return launch_dyn_lds<kern>(g.blocks, G::THREADS, G::LDS, s, (const T*)in, (const T*)w.w, w.bias, (const T*)nullptr, out, M,
                                g.n_mtiles, zero_page, (const T*)wp.w, wp.bias, out_p);
  }
  return (int)hipGetLastError();
}

#define HIPAC_TRY(expr)          \
  do {                           \
    int rc__ = (expr);           \
    if (rc__ != 0) {             \
      ::hipac::set_error("kernel launch failed (%d) at %s:%d", rc__, __FILE__, __LINE__); \
      return rc__;               \
    }                            \
  } while (0)

// precision fp16q8 (halo16x2.h): the q8 tensor of the pair tensor at workspace offset o lives at Plan::q8 + o / 2
struct Q8Map {
  char* ws;
  size_t q8;
  void* of(const void* pairs) const { return ws + q8 + (size_t)((const char*)pairs - ws) / 2; }
};
template <int CIN, int COUT, int HW, bool RELU, bool RESID, bool Q8OUT, bool POOL, bool OUTF32 = false, bool S2 = false, int PCIN = 0, bool LO16 = true,
          bool X3 = false>  // HW: the OUTPUT map
static int launch_halo16x2(const void* in, const void* in_q, const ConvW& w, const void* resid, void* out, void* out_q, int n, hipStream_t s,
                           const void* resid_q = nullptr, const void* wgt_p = nullptr, const float* bias = nullptr) {
  constexpr int BM = 256, BN = COUT % 128 == 0 ? 128 : 64;
  constexpr int LDS = halo16x2_lds_bytes(HW, BN, COUT);
  constexpr auto kern = conv3x3_halo16x2_kernel<CIN, COUT, HW, HW, BN, RELU, RESID, Q8OUT, POOL, OUTF32, S2, PCIN, LO16, X3>;
  const int M = n * HW * HW;
  const TileGrid g = tile_grid(M, BM, COUT / BN, HIPAC_HALO_GRID);
  return launch_dyn_lds<kern>(g.blocks, 256, LDS, s, (const _Float16*)in, (const unsigned char*)in_q, (const unsigned char*)w.w,
                              bias ? bias : w.bias, (const _Float16*)resid, out, (unsigned char*)out_q, M, n, g.n_mtiles,
                              (const unsigned char*)resid_q, (const unsigned char*)wgt_p, w.wscale, w.winv);
}
// the two pair modes' convs through one call: MODE 1 = fp16q8 (byte tensors, flags as given), MODE 2 = fp16x3 on the same kernel (pairs
// only: no q8 output, the lo plane always written)
template <int MODE, int CIN, int COUT, int HW, bool RESID, bool Q8OUT, bool POOL, bool OUTF32 = false, bool S2 = false, int PCIN = 0, bool LO16 = true>
static int launch_pairconv(const void* in, const void* in_q, const ConvW& w, const void* resid, void* out, void* out_q, int n, hipStream_t s,
                           const void* resid_q = nullptr, const void* wgt_p = nullptr, const float* bias = nullptr) {
  if constexpr (MODE == 2)
    return launch_halo16x2<CIN, COUT, HW, true, RESID, false, POOL, OUTF32, S2, PCIN, true, true>(in, nullptr, w, resid, out, nullptr, n, s, nullptr, wgt_p, bias);
  else
    return launch_halo16x2<CIN, COUT, HW, true, RESID, Q8OUT, POOL, OUTF32, S2, PCIN, LO16, false>(in, in_q, w, resid, out, out_q, n, s, resid_q, wgt_p, bias);
}

}  // namespace hipac

// Mixed-precision training step of the ResNet18 encoder (opt-in for a-12): what the reference's
// fine-tune loops compute under torch.cuda.amp.autocast() + GradScaler (src/main.py:499-508, :578-587) -- fp16
// operands on v_mfma_f32_32x32x16_f16 with fp32 accumulation, fp16 activations and activation gradients, fp32
// master parameters / gradients / Adam state (the flat buffers of train.hip, unchanged), a loss scale owned by the
// caller (train_native.GradScaler) -- as hand-written HIP:
//
//   forward   weights re-packed fp32 -> fp16 per step; convolutions on the inference kernels behind conv_launch.h (halo
//             kernel for 3x3 / stride 1, LDS-DMA kernel for stride 2 and 1x1, v1 kernel for the stem) with a zero
//             bias and no ReLU; batch statistics from the fp16 map in fp64, two-stage and DETERMINISTIC (per
//             workgroup partials, summed in a fixed order); normalise (+ residual) (+ ReLU) fp16 -> fp16.
//   backward  BN backward (same two-stage reductions), data gradient = the same convolution kernels on flipped /
//             transposed fp16 weights (stride 2: by parity class), weight gradient = wgrad_f16_kernel
//             below: an MFMA GEMM over the pixel axis whose operands (dY and X, both [pixel][channel] in memory) are
//             read TRANSPOSED from LDS by ds_read_b64_tr_b16, split-K partials in fp32 summed in a fixed order (no
//             atomics: a step run twice gives the same bits).
// The gradients that arrive (dfeats) and leave (grads) carry the caller's loss scale.  The host driver of the forward
// and backward, the workspace plan and the launches of the small kernels are shared with train.hip (train_common.h); the
// small kernels themselves (weight packing, batch norm, pools, ReLU masks, the sum of the split-K partials) are templates
// over the element type in train_kernels.h.  This file supplies the fp16 weight-gradient kernel, the gradient unscale /
// finiteness check and the Fp16Step precision struct.
#include "train_common.h"

namespace hipac {

typedef _Float16 h16;
typedef __attribute__((ext_vector_type(4))) short s16x4;

// ---------------------------------------------------------------------------------------------
// weight gradient on the fp16 MFMA:  part[slice][tap][co][ci] = sum over the slice's output pixels m of
//     dY[m][co] * X[pixel(m, tap)][ci]
// One workgroup = one (TC x TC) (co x ci) tile of NTAP filter taps over one slice of the pixel axis; 4 waves = 2 x 2
// wave tiles of (TC/2)^2 per tap.  The dY tile is staged ONCE per 32-pixel sub-chunk and multiplied with the NTAP
// shifted X tiles (one filter row = 3 taps for the 64-channel layers, 7 filter rows for the stem, 1 tap for the wide
// layers, whose 128 x 128 tiles are bound by the operand streams, not by the staging): NTAP MFMAs per dY fragment.  The contraction runs over PIXELS, but both operands lie
// [pixel][channel] in memory: they are staged as they come (16-byte pieces, rows of TC channels) and the MFMA
// fragments -- 8 consecutive pixels of one channel -- are read TRANSPOSED with ds_read_b64_tr_b16 (two per fragment).
// LDS row pitch = 2 TC + 64 bytes: the 4 rows x 2 channel blocks of a 32-lane half then fall on 64 distinct banks.
// The next sub-chunk's global loads are in flight behind the MFMAs; two barriers per sub-chunk.
// STEM: X is the padded NHWC4 input, a "tap" is filter row kh and the "ci" axis of its tile the 32 values (kw, c)
// (TC = 64: only the first 32 columns exist, waves wj = 1 take the odd filter rows instead of a second column half).
// ---------------------------------------------------------------------------------------------
template <int TC, int NTAP, bool STEM>
__global__ __launch_bounds__(256) void wgrad_f16_kernel(const h16* __restrict__ dY, const h16* __restrict__ X,
                                                        float* __restrict__ part, int Cout, int Cin, int KS, int stride, int HO,
                                                        int HI, long long M, int chunk) {
  constexpr int PITCH = 2 * TC + 64;             // bytes per staged pixel row
  constexpr int CH = TC / 8;                     // 16-byte pieces per row
  constexpr int PPT = 32 * CH / 256;             // pieces per thread and tile (1 for TC = 64, 2 for TC = 128)
  constexpr int WT = TC / 2, NF = WT / 32;       // wave tile, 32-wide fragments per wave and operand
  constexpr int TILE = 32 * PITCH;
  constexpr int MYT = STEM ? (NTAP + 1) / 2 : NTAP;  // taps a wave accumulates
  __shared__ __attribute__((aligned(16))) unsigned char smem[(1 + NTAP) * TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int ci_tiles = STEM ? 1 : Cin / TC, co_tiles = Cout / TC;
  int t = blockIdx.x;
  const int cit = t % ci_tiles;
  t /= ci_tiles;
  const int cot = t % co_tiles;
  const int tap0 = (t / co_tiles) * NTAP;
  const int pad = STEM ? 0 : KS / 2;
  const int wi = wave & 1, wj = wave >> 1;  // co half, ci half (STEM: filter-row parity)
  f32x16 acc[MYT][NF][NF];
#pragma unroll
  for (int tp = 0; tp < MYT; ++tp)
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
      for (int j = 0; j < NF; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[tp][i][j][e] = 0.f;
  const long long m_begin = (long long)blockIdx.y * chunk;
  const long long m_end = m_begin + chunk < M ? m_begin + chunk : M;

  u32x4 ra[PPT], rb[NTAP][PPT];
  auto gload = [&](long long m0) {
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      const int piece = tid + 256 * k, spx = piece / CH, sc = piece % CH;
      const long long m = m0 + spx;
      ra[k] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int tp = 0; tp < NTAP; ++tp) rb[tp][k] = u32x4{0u, 0u, 0u, 0u};
      if (m < m_end) {
        ra[k] = *reinterpret_cast<const u32x4*>(dY + m * Cout + cot * TC + 8 * sc);
        const int ox = (int)(m % HO);
        const long long tt = m / HO;
        const int oy = (int)(tt % HO);
        const long long b = tt / HO;
#pragma unroll
        for (int tp = 0; tp < NTAP; ++tp) {
          if constexpr (STEM) {
            if (sc < 4) rb[tp][k] = *reinterpret_cast<const u32x4*>(X + (((b * kPadH + 2 * oy + tap0 + tp) * kPadW) + 2 * ox) * 4 + 8 * sc);
          } else {
            const int tap = tap0 + tp, kh = tap / KS, kw = tap - kh * KS;
            const int iy = oy * stride + kh - pad, ix = ox * stride + kw - pad;
            if ((unsigned)iy < (unsigned)HI && (unsigned)ix < (unsigned)HI)
              rb[tp][k] = *reinterpret_cast<const u32x4*>(X + ((b * HI + iy) * HI + ix) * (long long)Cin + cit * TC + 8 * sc);
          }
        }
      }
    }
  };
  // transposed fragment address of this lane inside a tile: block row q = (lane & 15) >> 2, column quad p = lane & 3
  const int tr_off = ((lane & 15) >> 2) * PITCH + (((lane >> 4) & 1) * 16 + 4 * (lane & 3)) * 2 + 8 * h * PITCH;
  auto frag_tr = [&](const unsigned char* img, int col0, int kk) -> f16x8 {
    const unsigned char* p = img + tr_off + (16 * kk) * PITCH + col0 * 2;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p + 4 * PITCH));
    return __builtin_bit_cast(f16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
  };

  gload(m_begin);
  for (long long m0 = m_begin; m0 < m_end; m0 += 32) {
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      const int piece = tid + 256 * k, spx = piece / CH, sc = piece % CH;
      *reinterpret_cast<u32x4*>(smem + spx * PITCH + 16 * sc) = ra[k];
#pragma unroll
      for (int tp = 0; tp < NTAP; ++tp) *reinterpret_cast<u32x4*>(smem + (1 + tp) * TILE + spx * PITCH + 16 * sc) = rb[tp][k];
    }
    __syncthreads();
    if (m0 + 32 < m_end) gload(m0 + 32);  // in flight behind the MFMAs (and the other workgroups of the CU)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      f16x8 af[NF];
#pragma unroll
      for (int i = 0; i < NF; ++i) af[i] = frag_tr(smem, wi * WT + 32 * i, kk);
#pragma unroll
      for (int tp = 0; tp < MYT; ++tp) {
        const int tile = STEM ? 2 * tp + wj : tp;
        if (STEM && tile >= NTAP) continue;
        f16x8 bf[NF];
#pragma unroll
        for (int j = 0; j < NF; ++j) bf[j] = frag_tr(smem + (1 + tile) * TILE, (STEM ? 0 : wj * WT) + 32 * j, kk);
#pragma unroll
        for (int i = 0; i < NF; ++i)
#pragma unroll
          for (int j = 0; j < NF; ++j) acc[tp][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[tp][i][j], 0, 0, 0);
      }
    }
    __syncthreads();  // every wave has read the tiles: the next sub-chunk may overwrite them
  }
  // D[co][ci]: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 h
  const int row_len = STEM ? 32 : Cin;
  const int ntaps = STEM ? 7 : KS * KS;
#pragma unroll
  for (int tp = 0; tp < MYT; ++tp) {
    const int tap = tap0 + (STEM ? 2 * tp + wj : tp);
    if (STEM && tap >= NTAP) continue;
    float* base = part + ((size_t)blockIdx.y * ntaps + tap) * (size_t)Cout * row_len;
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int col = (STEM ? 0 : cit * TC + wj * WT) + 32 * j + r;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = cot * TC + wi * WT + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
          base[(size_t)row * row_len + col] = acc[tp][i][j][e];
        }
      }
  }
}

// grads *= inv_scale; flag[0] = 1 when an unscaled gradient is inf / nan (GradScaler.unscale_).  Every finite float passes,
// FLT_MAX included: the comparison is against FLT_MAX itself, which only inf and nan fail
__global__ __launch_bounds__(256) void unscale_check_kernel(float* __restrict__ g, long long n, float inv_scale,
                                                            int* __restrict__ flag) {
  bool bad = false;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float v = g[i] * inv_scale;
    g[i] = v;
    bad |= !(fabsf(v) <= 3.402823466e+38f);
  }
  if (bad) atomicOr(flag, 1);
}

// ---------------------------------------------------------------------------------------------
// the fp16 precision of the shared driver (train_common.h)
// ---------------------------------------------------------------------------------------------
constexpr size_t kWgPartBytes = (size_t)160 << 20;

struct Fp16Step {
  using T = h16;
  static constexpr const char* kName = "train_amp";
  static constexpr int kMaxBatch = 2048;  // 32-bit byte offsets
  static constexpr int kPrec = HIPAC_PREC_FP16;
  static constexpr bool kZeroPage = true;
  static size_t wpack_offset(int i) {
    size_t o = 0;
    for (int k = 0; k < i; ++k) o += (packed_w_floats(k) + 127) & ~(size_t)127;  // 256-byte aligned rows of the table
    return o;
  }
  static size_t wgrad_part_bytes(int) { return kWgPartBytes; }  // conv_wgrad bounds its slices by it
  static int conv_wgrad(const TrainCtx& c, int i, int n, const h16* X, const h16* dY, float* grads, int accumulate);
};

// weight gradient of conv i: X = the conv's input map, dY = gradient wrt its output -> grads (PyTorch layout)
int Fp16Step::conv_wgrad(const TrainCtx& c, int i, int n, const h16* X, const h16* dY, float* grads, int accumulate) {
  const ConvDesc& d = kConvs[i];
  float* part = (float*)(c.ws + c.p->wgrad_p);
  const long long M = (long long)n * d.hout * d.hout;
  const bool stem = i == 0;
  const size_t pf = stem ? (size_t)7 * 64 * 32 : conv_w_floats(i);
  const bool big = !stem && d.cout >= 128 && d.cin >= 128;
  const int TC = big ? 128 : 64;
  // taps per workgroup (they share the dY tile): the stem's 7 filter rows; 1 for the 128-channel tiles, 3 (one filter row)
  // for the 64-channel ones -- see DESIGN.md, "Removed alternatives"
  const int ntap_wg = stem ? 7 : (d.ks == 1 || big ? 1 : 3);
  const int tiles = stem ? 1 : (d.ks * d.ks / ntap_wg) * (d.cout / TC) * (d.cin / TC);
  // split the pixel axis so that the launch has ~768 workgroups (3 per CU); slices bounded by the partials buffer
  long long slices = (768 + tiles - 1) / tiles;
  const long long cap = (long long)(kWgPartBytes / (pf * 4));
  if (slices > cap) slices = cap;
  if (slices < 1) slices = 1;
  long long chunk = (M + slices - 1) / slices;
  chunk = (chunk + 31) / 32 * 32;
  if (chunk < 128) chunk = 128;
  slices = (M + chunk - 1) / chunk;
  dim3 grid(tiles, (unsigned)slices);
#define HIPAC_WG(TC_, NT_, ST_)                                                                                          \
  hipLaunchKernelGGL((wgrad_f16_kernel<TC_, NT_, ST_>), grid, dim3(256), 0, c.s, dY, X, part, d.cout, d.cin, d.ks, d.stride, \
                     d.hout, d.hin, M, (int)chunk)
  if (stem) HIPAC_WG(64, 7, true);
  else if (big) HIPAC_WG(128, 1, false);
  else if (ntap_wg == 3) HIPAC_WG(64, 3, false);
  else HIPAC_WG(64, 1, false);
#undef HIPAC_WG
  const long long total = (long long)conv_w_floats(i);
  hipLaunchKernelGGL(wgrad_reduce_kernel<0>, dim3((unsigned)((total + 31) / 32)), dim3(256), 0, c.s, (const float*)part, (int)slices,
                     grads + param_offset(i), d.cout, d.cin, d.ks, stem ? 1 : 0, accumulate);
  return (int)hipGetLastError();
}

}  // namespace hipac

using namespace hipac;

extern "C" {

size_t hipac_train_amp_workspace_bytes(int batch) { return batch > 0 ? make_train_plan<Fp16Step>(batch).total : 0; }

// Test tap, as hipac_train_debug_offset but for the fp16 workspace (maps are fp16 NHWC)
int64_t hipac_train_amp_debug_offset(int batch, int kind, int conv) { return train_debug_offset<Fp16Step>(batch, kind, conv); }

int hipac_train_amp_encoder_forward(const float* params, float* stats, const float* x, int batch, float momentum, float eps,
                                    float* feats, void* workspace, size_t workspace_bytes, void* stream) {
  return train_encoder_forward<Fp16Step>(params, stats, x, batch, momentum, eps, feats, workspace, workspace_bytes,
                                         (hipStream_t)stream);
}

int hipac_train_amp_encoder_backward(const float* params, const float* dfeats, int batch, float* grads, int accumulate,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  return train_encoder_backward<Fp16Step>(params, dfeats, batch, grads, accumulate, workspace, workspace_bytes,
                                          (hipStream_t)stream);
}

// GradScaler.unscale_: grads *= inv_scale in place; found_inf[0] (device int32, zeroed by the caller) is set when a
// gradient is inf / nan (src/main.py:506-508 scaler.step / scaler.update skip the optimizer step then)
int hipac_grads_unscale_check(float* grads, int64_t n, float inv_scale, int32_t* found_inf, void* stream) {
  HIPAC_REQUIRE(grads && found_inf && n > 0, HIPAC_EINVAL, "grads_unscale_check: bad argument");
  hipLaunchKernelGGL(unscale_check_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, grads, (long long)n, inv_scale,
                     (int*)found_inf);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"

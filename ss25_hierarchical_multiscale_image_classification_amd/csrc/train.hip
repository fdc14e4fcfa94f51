// Native training step of the ResNet18 encoder: train-mode forward and
// backward as hand-written HIP, fp32 throughout (the reference's pretrain_simclr runs fp32 without
// autocast, src/models/simclr.py:85-96), convolutions on the exact f32 MFMA (v_mfma_f32_32x32x2_f32).
//
//   forward   conv (implicit GEMM, the v1 kernel, conv_v1.h, on re-packed weights) -> batch statistics
//             (fp64 per-workgroup partial sums added in a fixed order, no atomics) -> normalise (+ residual) (+ ReLU);
//             3x3/2 max-pool with saved arg-max; global average pool.  Pre-BN and post-activation maps of every conv are
//             kept for the backward.
//   backward  BN backward (two passes: d gamma / d beta, then dx), conv weight gradient (MFMA GEMM over the
//             pixel axis, split-K into per-slice partials summed in a fixed order), conv data gradient = the forward
//             kernel on flipped / transposed weights (stride-2 layers: by parity class), max-pool / average-pool
//             backward, ReLU masks fused into the consumers.
//   plus      linear layers (projector, fc) on a strided fp32 MFMA GEMM, weighted cross-entropy, Adam.
//
// The host driver of the forward and backward, the workspace plan and the launches of the small kernels are shared with
// train_amp.hip (train_common.h); the small kernels themselves (weight packing, batch norm, pools, ReLU masks, the sum of
// the split-K partials) are templates over the element type in train_kernels.h.  This file supplies the fp32 weight-gradient
// kernel, the Fp32Step precision struct, and the linear / cross-entropy / Adam kernels.
//
// Activations are NHWC fp32.  Parameters live in ONE flat fp32 buffer in a fixed order (per conv: weight in
// the PyTorch layout [Cout][Cin][kh][kw], then BN gamma, beta); running statistics in a second flat buffer
// (per conv: running_mean, running_var); gradients in a buffer shaped like the parameters.
#include "train_common.h"
#include "wave_reduce.h"

namespace hipac {

// split K of conv i's weight gradient over `slices` chunks of `chunk` pixels so that the launch has ~2048 workgroups
static void wgrad_split(int i, long long M, long long& slices, long long& chunk) {
  const ConvDesc& d = kConvs[i];
  const int tiles = i == 0 ? 7 : d.ks * d.ks * (d.cout / 64) * (d.cin / 64);
  slices = (2048 + tiles - 1) / tiles;
  chunk = (M + slices - 1) / slices;
  chunk = (chunk + 31) / 32 * 32;
  if (chunk < 256) chunk = 256;
  slices = (M + chunk - 1) / chunk;
}

// ---------------------------------------------------------------------------------------------
// weight gradient: dWp[tap][co][ci] += sum_m dY[m][co] * X[pixel(m, tap)][ci]
// One workgroup = one 64 x 64 (co x ci) tile of one filter tap over a contiguous chunk of output pixels
// (split-K over the grid's y dimension); 4 waves = 2 x 2 MFMA tiles of 32 x 32 on v_mfma_f32_32x32x2_f32
// (A = dY[pixel][co], B = X[pixel][ci]: both operands are read along the channel axis, coalesced, no
// transpose); operands staged through LDS 32 pixels at a time; every slice stores its tile into its OWN copy of the packed
// gradient (dWp + slice * per_slice) and wgrad_reduce_kernel (train_kernels.h) adds the slices in a fixed order: no atomics.
// STEM form: X is the padded NHWC4 input, the "ci" axis of a tile is the 32 floats (kw, c) of filter row kh.
// ---------------------------------------------------------------------------------------------
template <bool STEM>
__global__ __launch_bounds__(256) void wgrad_kernel(const float* __restrict__ dY, const float* __restrict__ X,
                                                    float* __restrict__ dWp, int Cout, int Cin, int KS, int stride,
                                                    int HO, int HI, long long M, int chunk) {
  constexpr int LDP = 68;  // LDS row: 64 floats + 4 (keeps float4 stores aligned, spreads banks)
  __shared__ __attribute__((aligned(16))) float As[32 * LDP], Bs[32 * LDP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int ci_tiles = STEM ? 1 : Cin / 64, co_tiles = Cout / 64;
  int t = blockIdx.x;
  const int cit = t % ci_tiles;
  t /= ci_tiles;
  const int cot = t % co_tiles;
  const int tap = t / co_tiles;
  const int kh = STEM ? tap : tap / KS, kw = STEM ? 0 : tap % KS;
  const int pad = STEM ? 0 : KS / 2;
  const int wi = wave & 1, wj = wave >> 1;  // co half, ci half (STEM: ci half is the pixel half instead)
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const long long m_begin = (long long)blockIdx.y * chunk;
  const long long m_end = m_begin + chunk < M ? m_begin + chunk : M;
  const int spx = tid >> 3, sc = tid & 7;  // staging: pixel of the sub-chunk, float4 column (and + 8)
  for (long long m0 = m_begin; m0 < m_end; m0 += 32) {
    const long long m = m0 + spx;
    const bool ok = m < m_end;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, b0 = a0, b1 = a0;
    if (ok) {
      const float* ap = dY + m * Cout + cot * 64 + 4 * sc;
      a0 = *reinterpret_cast<const float4*>(ap);
      a1 = *reinterpret_cast<const float4*>(ap + 32);
      const int ox = (int)(m % HO);
      const long long tt = m / HO;
      const int oy = (int)(tt % HO);
      const long long b = tt / HO;
      if constexpr (STEM) {
        const float* bp = X + (((b * kPadH + 2 * oy + kh) * kPadW) + 2 * ox) * 4 + 4 * sc;  // 32 floats = 8 float4
        b0 = *reinterpret_cast<const float4*>(bp);
      } else {
        const int iy = oy * stride + kh - pad, ix = ox * stride + kw - pad;
        if ((unsigned)iy < (unsigned)HI && (unsigned)ix < (unsigned)HI) {
          const float* bp = X + ((b * HI + iy) * HI + ix) * (long long)Cin + cit * 64 + 4 * sc;
          b0 = *reinterpret_cast<const float4*>(bp);
          b1 = *reinterpret_cast<const float4*>(bp + 32);
        }
      }
    }
    __syncthreads();  // the previous sub-chunk's fragments have been read
    *reinterpret_cast<float4*>(As + spx * LDP + 4 * sc) = a0;
    *reinterpret_cast<float4*>(As + spx * LDP + 32 + 4 * sc) = a1;
    *reinterpret_cast<float4*>(Bs + spx * LDP + 4 * sc) = b0;
    if constexpr (!STEM) *reinterpret_cast<float4*>(Bs + spx * LDP + 32 + 4 * sc) = b1;
    __syncthreads();
    if constexpr (STEM) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {  // this wave's 16 pixels of the sub-chunk
        const int px = wj * 16 + 2 * k + h;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[px * LDP + wi * 32 + r], Bs[px * LDP + r], acc, 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int px = 2 * k + h;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[px * LDP + wi * 32 + r], Bs[px * LDP + wj * 32 + r], acc, 0, 0, 0);
      }
    }
  }
  // D[co][j]: col j = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h
  const int row_len = STEM ? 32 : Cin;
  const size_t per_slice = STEM ? (size_t)7 * 64 * 32 : (size_t)KS * KS * Cout * Cin;
  // STEM: the two waves of a channel half split the PIXELS of a sub-chunk, i.e. both hold a partial sum of the same tile:
  // each gets its own copy (slot 2 * slice + wj)
  const size_t slot = STEM ? (size_t)blockIdx.y * 2 + wj : (size_t)blockIdx.y;
  float* base = dWp + slot * per_slice + ((size_t)tap * Cout + cot * 64 + wi * 32) * row_len +
                (STEM ? 0 : cit * 64 + wj * 32) + r;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int row = (e & 3) + 8 * (e >> 2) + 4 * h;
    base[(size_t)row * row_len] = acc[e];
  }
}

// ---------------------------------------------------------------------------------------------
// strided fp32 GEMM on the f32 MFMA: C[m][n] (+)= sum_k A(m,k) * B(n,k) (+ bias[n]) (ReLU), A(m,k) = a[m*sam + k*sak],
// B(n,k) = b[n*sbn + k*sbk].  64 x 64 tile per workgroup, K stepped by 32 through LDS; every access is
// bounds-checked, so M, N, K are arbitrary (the projector / fc layers are tiny next to the encoder).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gemm_f32_kernel(const float* __restrict__ a, long long sam, long long sak,
                                                       const float* __restrict__ b, long long sbn, long long sbk,
                                                       float* __restrict__ c, long long scm, int M, int N, int K,
                                                       const float* __restrict__ bias, int relu, int accumulate) {
  constexpr int LDP = 33;
  __shared__ float As[64 * LDP], Bs[64 * LDP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int wi = wave & 1, wj = wave >> 1;
  const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  // this thread's 8 + 8 elements of a K tile: rows row0 + 8 j, column kk; the NEXT tile is fetched into registers behind the MFMAs
  const int kk_t = tid & 31, row0 = tid >> 5;
  float ra[8], rb[8];
  auto fetch = [&](int k0) {
    const int k = k0 + kk_t;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int m = m0 + row0 + 8 * j, n = n0 + row0 + 8 * j;
      ra[j] = (m < M && k < K) ? a[m * sam + k * sak] : 0.f;
      rb[j] = (n < N && k < K) ? b[n * sbn + k * sbk] : 0.f;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += 32) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) As[(row0 + 8 * j) * LDP + kk_t] = ra[j], Bs[(row0 + 8 * j) * LDP + kk_t] = rb[j];
    __syncthreads();
    if (k0 + 32 < K) fetch(k0 + 32);
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(wi * 32 + r) * LDP + 2 * kk + h], Bs[(wj * 32 + r) * LDP + 2 * kk + h],
                                                 acc, 0, 0, 0);
  }
  const int n = n0 + wj * 32 + r;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int m = m0 + wi * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
    if (m < M && n < N) {
      float v = acc[e] + (bias ? bias[n] : 0.f);
      if (accumulate) v += c[m * scm + n];
      c[m * scm + n] = relu ? fmaxf(v, 0.f) : v;
    }
  }
}

// column sums of dy[M][N] (bias gradient), masked by (ymask > 0) when given; also writes the masked dy.  A workgroup owns 16
// columns; its 16 row groups (rows m = rg mod 16) run side by side and are added in a fixed order: one thread per column
// walking all M rows was a chain of M dependent loads on two workgroups (377 us for 2048 x 512).
__global__ __launch_bounds__(256) void bias_grad_kernel(const float* __restrict__ dy, const float* __restrict__ ymask,
                                                        float* __restrict__ dym, int M, int N, float* __restrict__ db,
                                                        int accumulate) {
  __shared__ float red[16][17];
  const int c = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int n = blockIdx.x * 16 + c;
  float s = 0.f;
  if (n < N) {
    for (int m = rg; m < M; m += 16) {
      float v = dy[(size_t)m * N + n];
      if (ymask && !(ymask[(size_t)m * N + n] > 0.f)) v = 0.f;
      if (dym) dym[(size_t)m * N + n] = v;
      s += v;
    }
  }
  red[rg][c] = s;
  __syncthreads();
  if (rg == 0 && n < N && db) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][c];
    db[n] = accumulate ? db[n] + t : t;
  }
}

// weighted cross-entropy (mean reduction as torch: sum w[y] * nll / sum w[y]) and its gradient
__global__ __launch_bounds__(256) void ce_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                 const float* __restrict__ cw, int M, int C, float* __restrict__ loss,
                                                 float* __restrict__ dlogits, float* __restrict__ scratch /* [2] */,
                                                 int phase) {
  // phase 0: per-wave (sum w nll, sum w) into scratch[2 ..]; phase 2: their sums in order -> scratch[0], scratch[1];
  // phase 1: gradient (needs scratch[1]) and the loss value
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (phase == 0) {
    float nll = 0.f, w = 0.f;
    if (m < M) {
      const float* l = logits + (size_t)m * C;
      float mx = l[0];
      for (int j = 1; j < C; ++j) mx = fmaxf(mx, l[j]);
      float se = 0.f;
      for (int j = 0; j < C; ++j) se += expf(l[j] - mx);
      const long long yl = labels[m];
      if (yl < 0 || yl >= C) {  // torch raises here; no out-of-bounds read, and the loss comes out NaN
        nll = __builtin_nanf(""), w = 0.f;
      } else {
        const int y = (int)yl;
        w = cw ? cw[y] : 1.f;
        nll = w * (logf(se) + mx - l[y]);
      }
    }
    nll = wave_sum_tree(nll), w = wave_sum_tree(w);
    // every workgroup's four wave sums, then the workgroups in order (phase 2 below): no atomics, a reproducible loss
    if ((threadIdx.x & 63) == 0) scratch[2 + 2 * (blockIdx.x * 4 + (threadIdx.x >> 6))] = nll, scratch[3 + 2 * (blockIdx.x * 4 + (threadIdx.x >> 6))] = w;
  } else if (phase == 2) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      float a = 0.f, b = 0.f;
      const int nw = 4 * ((M + 255) / 256);
      for (int k = 0; k < nw; ++k) a += scratch[2 + 2 * k], b += scratch[3 + 2 * k];
      scratch[0] = a, scratch[1] = b;
    }
  } else if (m < M) {
    const float* l = logits + (size_t)m * C;
    float mx = l[0];
    for (int j = 1; j < C; ++j) mx = fmaxf(mx, l[j]);
    float se = 0.f;
    for (int j = 0; j < C; ++j) se += expf(l[j] - mx);
    const long long yl = labels[m];
    const int y = (yl < 0 || yl >= C) ? -1 : (int)yl;
    const float w = y < 0 ? __builtin_nanf("") : (cw ? cw[y] : 1.f) / scratch[1];
    for (int j = 0; j < C; ++j) dlogits[(size_t)m * C + j] = w * (expf(l[j] - mx) / se - (j == y ? 1.f : 0.f));
    if (m == 0) loss[0] = scratch[0] / scratch[1];
  }
}

// torch.optim.Adam (no weight decay, no amsgrad): in place on p, m, v
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long long n, float lr, float b1, float b2,
                                                   float eps, float bc1, float bc2_sqrt) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float gi = g[i];
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] -= (lr / bc1) * mi / (sqrtf(vi) / bc2_sqrt + eps);
  }
}

// ---------------------------------------------------------------------------------------------
// the fp32 precision of the shared driver (train_common.h)
// ---------------------------------------------------------------------------------------------
struct Fp32Step {
  using T = float;
  static constexpr const char* kName = "train";
  static constexpr int kMaxBatch = 4096;  // 32-bit pixel offsets
  static constexpr int kPrec = HIPAC_PREC_FP32;
  static constexpr bool kZeroPage = false;
  static size_t wpack_offset(int i) {
    size_t o = 0;
    for (int k = 0; k < i; ++k) o += packed_w_floats(k);
    return o;
  }
  // split-K partials of a weight gradient: [slices][packed weights] of the largest conv, summed in slice order afterwards
  static size_t wgrad_part_bytes(int B) {
    size_t maxpart = 0;
    for (int i = 0; i < kNumConvs; ++i) {
      long long sl, ch;
      wgrad_split(i, (long long)B * kConvs[i].hout * kConvs[i].hout, sl, ch);
      const size_t pf = i == 0 ? (size_t)7 * 64 * 32 : conv_w_floats(i);
      if ((size_t)sl * (i == 0 ? 2 : 1) * pf > maxpart) maxpart = (size_t)sl * (i == 0 ? 2 : 1) * pf;
    }
    return maxpart * 4;
  }
  static int conv_wgrad(const TrainCtx& c, int i, int n, const float* X, const float* dY, float* grads, int accumulate);
};

// weight gradient of conv i: X = the conv's input map, dY = gradient wrt its output -> grads (PyTorch layout)
int Fp32Step::conv_wgrad(const TrainCtx& c, int i, int n, const float* X, const float* dY, float* grads, int accumulate) {
  const ConvDesc& d = kConvs[i];
  float* dwp = (float*)(c.ws + c.p->wgrad_p);
  const long long M = (long long)n * d.hout * d.hout;
  const bool stem = i == 0;
  const int tiles = stem ? 7 : d.ks * d.ks * (d.cout / 64) * (d.cin / 64);
  long long slices, chunk;
  wgrad_split(i, M, slices, chunk);  // the workspace plan sized dwp for exactly this split
  if (stem)
    hipLaunchKernelGGL((wgrad_kernel<true>), dim3(tiles, (unsigned)slices), dim3(256), 0, c.s, dY, X, dwp, 64, 3, 7, 2, 112, 224,
                       M, (int)chunk);
  else
    hipLaunchKernelGGL((wgrad_kernel<false>), dim3(tiles, (unsigned)slices), dim3(256), 0, c.s, dY, X, dwp, d.cout, d.cin, d.ks,
                       d.stride, d.hout, d.hin, M, (int)chunk);
  const long long total = (long long)conv_w_floats(i);
  hipLaunchKernelGGL(wgrad_reduce_kernel<0>, dim3((unsigned)((total + 31) / 32)), dim3(256), 0, c.s, (const float*)dwp,
                     (int)(stem ? 2 * slices : slices),
                     grads + param_offset(i), d.cout, d.cin, d.ks, stem ? 1 : 0, accumulate);
  return (int)hipGetLastError();
}

}  // namespace hipac

using namespace hipac;

extern "C" {

int hipac_train_num_convs(void) { return kNumConvs; }

int hipac_train_conv_desc(int i, int* cout, int* cin, int* ks, int* stride, int64_t* param_off, int64_t* stat_off) {
  HIPAC_REQUIRE(i >= 0 && i < kNumConvs, HIPAC_EINVAL, "train_conv_desc: index %d", i);
  if (cout) *cout = kConvs[i].cout;
  if (cin) *cin = kConvs[i].cin;
  if (ks) *ks = kConvs[i].ks;
  if (stride) *stride = kConvs[i].stride;
  if (param_off) *param_off = (int64_t)param_offset(i);
  if (stat_off) *stat_off = (int64_t)stat_offset(i);
  return 0;
}
size_t hipac_train_param_floats(void) { return param_offset(kNumConvs); }
size_t hipac_train_stat_floats(void) { return stat_offset(kNumConvs); }
size_t hipac_train_workspace_bytes(int batch) { return batch > 0 ? make_train_plan<Fp32Step>(batch).total : 0; }

int64_t hipac_train_debug_offset(int batch, int kind, int conv) { return train_debug_offset<Fp32Step>(batch, kind, conv); }

int hipac_train_encoder_forward(const float* params, float* stats, const float* x, int batch, float momentum, float eps,
                                float* feats, void* workspace, size_t workspace_bytes, void* stream) {
  return train_encoder_forward<Fp32Step>(params, stats, x, batch, momentum, eps, feats, workspace, workspace_bytes,
                                         (hipStream_t)stream);
}

int hipac_train_encoder_backward(const float* params, const float* dfeats, int batch, float* grads, int accumulate,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  return train_encoder_backward<Fp32Step>(params, dfeats, batch, grads, accumulate, workspace, workspace_bytes,
                                          (hipStream_t)stream);
}

}  // extern "C"
namespace hipac {
// the strided f32-MFMA GEMM for the other translation units (ntxent.hip): C[m][n] = sum_k A(m,k) B(n,k)
int launch_gemm_f32(const float* a, long long sam, long long sak, const float* b, long long sbn, long long sbk, float* c, long long ldc,
                    int M, int N, int K, hipStream_t s) {
  hipLaunchKernelGGL(gemm_f32_kernel, dim3((M + 63) / 64, (N + 63) / 64), dim3(256), 0, s, a, sam, sak, b, sbn, sbk, c, ldc, M, N, K,
                     (const float*)nullptr, 0, 0);
  return (int)hipGetLastError();
}
}  // namespace hipac
extern "C" {

// y[M][N] = x[M][K] w[N][K]^T + b (ReLU)    -- nn.Linear forward (src/models/simclr.py:20-24 projector, resnet.py:66 fc)
int hipac_linear_forward(const float* x, const float* w, const float* b, float* y, int M, int N, int K, int relu, void* stream) {
  HIPAC_REQUIRE(x && w && y && M > 0 && N > 0 && K > 0, HIPAC_EINVAL, "linear_forward: bad argument");
  hipLaunchKernelGGL(gemm_f32_kernel, dim3((M + 63) / 64, (N + 63) / 64), dim3(256), 0, (hipStream_t)stream, x, (long long)K, 1LL,
                     w, (long long)K, 1LL, y, (long long)N, M, N, K, b, relu, 0);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

// backward of y = relu?(x w^T + b): dy masked by (y > 0) when y is given (dym: scratch [M][N], required then);
// dx[M][K] = dy w (or NULL), dw[N][K] (+)= dy^T x, db[N] (+)= column sums
int hipac_linear_backward(const float* x, const float* w, const float* dy, const float* y, float* dym, float* dx, float* dw,
                          float* db, int M, int N, int K, int accumulate, void* stream) {
  HIPAC_REQUIRE(x && w && dy && dw && M > 0 && N > 0 && K > 0, HIPAC_EINVAL, "linear_backward: bad argument");
  HIPAC_REQUIRE(!y || dym, HIPAC_EINVAL, "linear_backward: a ReLU mask needs the dym scratch");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bias_grad_kernel, dim3((N + 15) / 16), dim3(256), 0, s, dy, y, y ? dym : nullptr, M, N, db, accumulate);
  const float* g = y ? dym : dy;
  if (dx)  // dx[m][k] = sum_n g[m][n] w[n][k]:  A(m, n) = g, B(k, n) = w[n][k]
    hipLaunchKernelGGL(gemm_f32_kernel, dim3((M + 63) / 64, (K + 63) / 64), dim3(256), 0, s, g, (long long)N, 1LL, w, 1LL,
                       (long long)K, dx, (long long)K, M, K, N, (const float*)nullptr, 0, 0);
  // dw[n][k] = sum_m g[m][n] x[m][k]:  A(n, m) = g[m][n], B(k, m) = x[m][k]
  hipLaunchKernelGGL(gemm_f32_kernel, dim3((N + 63) / 64, (K + 63) / 64), dim3(256), 0, s, g, 1LL, (long long)N, x, 1LL,
                     (long long)K, dw, (long long)K, N, K, M, (const float*)nullptr, 0, accumulate);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

// nn.CrossEntropyLoss(weight=class_w) value and gradient (src/main.py:490, :552-566); scratch: float[2 + 8 * ceil(M / 256)]
int hipac_cross_entropy_fwd_bwd(const float* logits, const int64_t* labels, const float* class_w, int M, int C, float* loss,
                                float* dlogits, float* scratch, void* stream) {
  HIPAC_REQUIRE(logits && labels && loss && dlogits && scratch && M > 0 && C > 0 && C <= 64, HIPAC_EINVAL,
                "cross_entropy: bad argument");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ce_kernel, dim3((M + 255) / 256), dim3(256), 0, s, logits, (const long long*)labels, class_w, M, C, loss,
                     dlogits, scratch, 0);
  hipLaunchKernelGGL(ce_kernel, dim3(1), dim3(64), 0, s, logits, (const long long*)labels, class_w, M, C, loss, dlogits, scratch, 2);
  hipLaunchKernelGGL(ce_kernel, dim3((M + 255) / 256), dim3(256), 0, s, logits, (const long long*)labels, class_w, M, C, loss,
                     dlogits, scratch, 1);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

// torch.optim.Adam step t (1-based) on a flat buffer (src/main.py:492, src/models/simclr.py:79)
int hipac_adam_step(float* params, const float* grads, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                    float eps, int step, void* stream) {
  HIPAC_REQUIRE(params && grads && m && v && n > 0 && step >= 1, HIPAC_EINVAL, "adam: bad argument");
  // bias corrections in double, as torch computes them with Python floats (1 - 0.999f in fp32 is 1.3e-5 off at step 1)
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const float bc2 = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, params, grads, m, v, (long long)n, lr,
                     beta1, beta2, eps, bc1, bc2);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"

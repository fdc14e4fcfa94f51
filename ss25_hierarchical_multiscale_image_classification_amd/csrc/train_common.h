// Shared by train.hip (fp32) and train_amp.hip (fp16 mixed precision): the 20 convolutions of the ResNet18 encoder
// in the library's fixed order, the layout of the flat parameter / gradient / running-statistics buffers, the workspace
// plan, the launches of the small kernels (train_kernels.h: one template per kernel over the element type of the maps) and
// the host driver of the train-mode forward and backward.  All of it is written once over a precision struct P that each
// translation unit supplies (no virtual interface) and that holds only what differs between the two:
//   T                          element type of the maps (float / _Float16)
//   kName, kMaxBatch, kPrec    message prefix ("train" / "train_amp"), largest batch, HIPAC_PREC_* of the input conversion
//   kZeroPage                  whether the workspace holds the 256 zero bytes that the fp16 inference kernels read
//   wpack_offset(i)            elements in front of conv i's packed forward weights (fp16: rows of the table 256-byte aligned)
//   wgrad_part_bytes(B)        size of the split-K partials of one weight gradient
//   conv_wgrad                 weight gradient of conv i into the flat gradient buffer (the MFMA kernel of the precision)
#pragma once
#include "conv_launch.h"
#include "train_kernels.h"

namespace hipac {

struct ConvDesc {
  int cout, cin, ks, stride, hin, hout;
};
// 0 stem | per stage: b0.conv1, b0.conv2, [b0.downsample], b1.conv1, b1.conv2
static const ConvDesc kConvs[20] = {
    {64, 3, 7, 2, 224, 112},                                                                          // 0
    {64, 64, 3, 1, 56, 56},   {64, 64, 3, 1, 56, 56},   {64, 64, 3, 1, 56, 56},   {64, 64, 3, 1, 56, 56},    // 1-4
    {128, 64, 3, 2, 56, 28},  {128, 128, 3, 1, 28, 28}, {128, 64, 1, 2, 56, 28},                              // 5-7
    {128, 128, 3, 1, 28, 28}, {128, 128, 3, 1, 28, 28},                                                       // 8-9
    {256, 128, 3, 2, 28, 14}, {256, 256, 3, 1, 14, 14}, {256, 128, 1, 2, 28, 14},                             // 10-12
    {256, 256, 3, 1, 14, 14}, {256, 256, 3, 1, 14, 14},                                                       // 13-14
    {512, 256, 3, 2, 14, 7},  {512, 512, 3, 1, 7, 7},   {512, 256, 1, 2, 14, 7},                              // 15-17
    {512, 512, 3, 1, 7, 7},   {512, 512, 3, 1, 7, 7},                                                         // 18-19
};
constexpr int kNumConvs = 20;

static size_t conv_w_floats(int i) { return (size_t)kConvs[i].cout * kConvs[i].cin * kConvs[i].ks * kConvs[i].ks; }
static size_t param_offset(int i) {  // floats before conv i in the flat parameter buffer
  size_t o = 0;
  for (int k = 0; k < i; ++k) o += conv_w_floats(k) + 2 * (size_t)kConvs[k].cout;
  return o;
}
static size_t stat_offset(int i) {
  size_t o = 0;
  for (int k = 0; k < i; ++k) o += 2 * (size_t)kConvs[k].cout;
  return o;
}
static size_t packed_w_floats(int i) {  // elements of [Cout][K] of the forward kernel (stem: 7 x 32 per row)
  return i == 0 ? (size_t)64 * 224 : conv_w_floats(i);
}


static inline unsigned grid_for(long long n, int cap = 4096) {
  long long g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

constexpr int kRedBlocks = 512;  // workgroups of a BN reduction pass = rows of the partial-sum table

// ---------------------------------------------------------------------------------------------
// workspace of one forward (everything the backward needs) + scratch shared by forward / backward: byte offsets
// ---------------------------------------------------------------------------------------------
struct TrainPlan {
  size_t xin;               // T[B,230,232,4]
  size_t pre[kNumConvs];    // conv output before BN, T
  size_t post[kNumConvs];   // after BN (+ residual) (+ ReLU), T
  size_t pool, pool_idx;    // T[B,56,56,64], uint8 arg-max (0..8, 9 = none)
  size_t mean_rstd;         // per conv: mean[cout], rstd[cout] (floats), packed by stat_offset
  size_t sums;              // double[2 * 512] scratch of the statistics / BN-backward reductions
  size_t red;               // double[kRedBlocks][2 * 512]: per-workgroup partial sums of one reduction pass (no atomics)
  size_t wpack[kNumConvs];  // packed forward weights of conv i, T
  size_t wpack_d;           // packed data-gradient weights (largest conv), T
  size_t wgrad_p;           // float split-K partials of one weight gradient
  size_t zero_bias;         // float[512] zeros
  size_t zero_page;         // 256 zero bytes right behind zero_bias, read by the fp16 inference kernels; 0: none (fp32)
  size_t g[3];              // gradient maps (largest activation each), T
  size_t up;                // gradient through a 1x1 / stride-2 projection, on the fine grid, T
  size_t total;
};

template <class P>
static TrainPlan make_train_plan(int B) {
  constexpr size_t esz = sizeof(typename P::T);
  TrainPlan p{};
  size_t off = 0;
  auto take = [&](size_t bytes) {
    size_t o = off;
    off += align256(bytes);
    return o;
  };
  const size_t b = (size_t)B;
  p.xin = take(b * kPadH * kPadW * 4 * esz);
  size_t maxact = 0, maxw = 0;
  for (int i = 0; i < kNumConvs; ++i) {
    const size_t n = b * kConvs[i].hout * kConvs[i].hout * kConvs[i].cout;
    p.pre[i] = take(n * esz);
    p.post[i] = take(n * esz);
    if (n > maxact) maxact = n;
    if (packed_w_floats(i) > maxw) maxw = packed_w_floats(i);
  }
  p.pool = take(b * 56 * 56 * 64 * esz);
  p.pool_idx = take(b * 56 * 56 * 64);
  p.mean_rstd = take(stat_offset(kNumConvs) * 4);
  p.sums = take(2 * 512 * 8);
  p.red = take((size_t)kRedBlocks * 1024 * 8);
  const size_t wpack = take(P::wpack_offset(kNumConvs) * esz);
  for (int i = 0; i < kNumConvs; ++i) p.wpack[i] = wpack + P::wpack_offset(i) * esz;
  p.wpack_d = take(maxw * esz);
  p.wgrad_p = take(P::wgrad_part_bytes(B));
  p.zero_bias = take(512 * 4);
  if (P::kZeroPage) p.zero_page = take(256);
  for (int k = 0; k < 3; ++k) p.g[k] = take(maxact * esz);
  p.up = take(b * 56 * 56 * 128 * esz);  // largest: layer2 entry (128 ch at 56 x 56)
  p.total = off;
  return p;
}

struct TrainCtx {
  const float* params;  // flat parameter buffer
  float* stats;         // running statistics (may be null: not updated)
  char* ws;
  const TrainPlan* p;
  float eps, momentum;
  hipStream_t s;
};

// ---------------------------------------------------------------------------------------------
// launches of the small kernels (train_kernels.h): V = kVec<T> channels per thread
// ---------------------------------------------------------------------------------------------
// workgroups of a BN reduction pass over [M][C]: a workgroup takes 256 / (C / V) rows per pass
template <typename T>
static int red_blocks(long long M, int C) {
  const int rows_per_pass = 256 / (C / kVec<T>);
  const long long gs = (M + rows_per_pass - 1) / rows_per_pass;
  return (int)(gs > kRedBlocks ? kRedBlocks : gs);  // 2 workgroups per CU
}
// bn_apply_kernel / bn_bwd_apply_kernel load a thread's per-channel constants once: whatever grid_for returns, the grid
// stride is a multiple of 256 * V elements (1024 or 2048), which C must divide -- every C of kConvs (64 ... 512) does
template <typename T>
static bool bn_apply_geometry_ok(int C) { return C % kVec<T> == 0 && (256 * kVec<T>) % C == 0; }

// batch-norm (training statistics) of conv i's output, optional residual and ReLU
template <typename T>
static int bn_forward(const TrainCtx& c, int i, int n, const T* resid, int relu) {
  const ConvDesc& d = kConvs[i];
  if (!bn_apply_geometry_ok<T>(d.cout)) return HIPAC_EINVAL;
  const long long M = (long long)n * d.hout * d.hout;
  const T* x = (const T*)(c.ws + c.p->pre[i]);
  T* y = (T*)(c.ws + c.p->post[i]);
  double* part = (double*)(c.ws + c.p->red);
  double* sums = (double*)(c.ws + c.p->sums);
  float* mean = (float*)(c.ws + c.p->mean_rstd) + stat_offset(i);
  float* rstd = mean + d.cout;
  const float* gamma = c.params + param_offset(i) + conv_w_floats(i);
  const int gs = red_blocks<T>(M, d.cout);
  hipLaunchKernelGGL((bn_reduce_kernel<T, 0>), dim3(gs), dim3(256), 0, c.s, x, (const T*)nullptr, (const T*)nullptr, M, d.cout,
                     (const float*)nullptr, (const float*)nullptr, part);
  float* rm = c.stats ? c.stats + stat_offset(i) : nullptr;
  hipLaunchKernelGGL((bn_sum_parts_kernel<true>), dim3((d.cout + 7) / 8), dim3(256), 0, c.s, (const double*)part, gs, d.cout,
                     sums, M, c.eps, c.momentum, mean, rstd, rm, rm ? rm + d.cout : nullptr);
  const long long nv = M * d.cout / kVec<T>;
  hipLaunchKernelGGL(bn_apply_kernel<T>, dim3(grid_for(nv)), dim3(256), 0, c.s, x, resid, y, nv, d.cout, (const float*)mean,
                     (const float*)rstd, gamma, gamma + d.cout, relu);
  return (int)hipGetLastError();
}

// BN backward of conv i: dy (masked by ymask > 0 if given) -> dx (may alias dy), d gamma / d beta into grads
template <typename T>
static int bn_backward(const TrainCtx& c, int i, int n, const T* dy, const T* ymask, T* dx, float* grads, int accumulate) {
  const ConvDesc& d = kConvs[i];
  if (!bn_apply_geometry_ok<T>(d.cout)) return HIPAC_EINVAL;
  const long long M = (long long)n * d.hout * d.hout;
  const T* x = (const T*)(c.ws + c.p->pre[i]);
  double* part = (double*)(c.ws + c.p->red);
  double* sums = (double*)(c.ws + c.p->sums);
  const float* mean = (const float*)(c.ws + c.p->mean_rstd) + stat_offset(i);
  const float* rstd = mean + d.cout;
  const float* gamma = c.params + param_offset(i) + conv_w_floats(i);
  float* dgamma = grads + param_offset(i) + conv_w_floats(i);
  const int gs = red_blocks<T>(M, d.cout);
  hipLaunchKernelGGL((bn_reduce_kernel<T, 1>), dim3(gs), dim3(256), 0, c.s, dy, x, ymask, M, d.cout, mean, rstd, part);
  hipLaunchKernelGGL((bn_sum_parts_kernel<false>), dim3((d.cout + 7) / 8), dim3(256), 0, c.s, (const double*)part, gs, d.cout,
                     sums, M, 0.f, 0.f, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr);
  const long long nv = M * d.cout / kVec<T>;
  hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, dim3(grid_for(nv)), dim3(256), 0, c.s, dy, x, ymask, dx, nv, M, d.cout, mean, rstd,
                     gamma, (const double*)sums, dgamma, dgamma + d.cout, accumulate);
  return (int)hipGetLastError();
}

// the stem's max-pool and its backward: one thread per V channels of an output position / of a 2 x 2 quad of input positions
template <typename T>
static void maxpool(const T* in, T* out, unsigned char* idx, int n, hipStream_t s) {
  const long long totalv = (long long)n * 56 * 56 * (64 / kVec<T>);
  hipLaunchKernelGGL(maxpool_idx_kernel<T>, dim3((unsigned)((totalv + 255) / 256)), dim3(256), 0, s, in, out, idx, totalv);
}
template <typename T>
static void maxpool_bwd(const T* dout, const unsigned char* idx, T* din, int n, hipStream_t s) {
  const long long totalv = (long long)n * 56 * 56 * (64 / kVec<T>);
  hipLaunchKernelGGL(maxpool_bwd_kernel<T>, dim3((unsigned)((totalv + 255) / 256)), dim3(256), 0, s, dout, idx, din, totalv);
}
template <typename T>
static void avgpool(const T* last, float* feats, int n, hipStream_t s) {
  hipLaunchKernelGGL(avgpool_kernel<T>, dim3(n), dim3(256), 0, s, last, feats, n);
}
template <typename T>
static void avgpool_bwd(const float* dfeats, const T* last, T* dlast, int n, hipStream_t s) {
  const long long total = (long long)n * 49 * 512;
  hipLaunchKernelGGL(avgpool_bwd_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, dfeats, last, dlast, total);
}
template <typename T>
static void add_mask(const T* a, const T* b, const T* y, T* out, long long n_elems, hipStream_t s) {
  const long long nv = n_elems / kVec<T>;
  hipLaunchKernelGGL(add_mask_kernel<T>, dim3(grid_for(nv)), dim3(256), 0, s, a, b, y, out, nv);
}

// ---------------------------------------------------------------------------------------------
// convolutions on the fixed layer geometries: zero bias, no epilogue extras.  fp32 runs every layer on the v1 kernel
// (exact f32 MFMA), fp16 on the inference kernels -- launch_conv / launch_dgrad_s2_class choose by sizeof(T)
// ---------------------------------------------------------------------------------------------
template <typename T, int CIN, int COUT, int HI, int KS, int STRIDE>
static int conv_layer(const T* in, const T* wp, const float* zb, T* out, int n, hipStream_t s, const char* zp) {
  ConvW w{const_cast<T*>(wp), const_cast<float*>(zb)};
  return launch_conv<T, CIN, COUT, HI, HI, KS, STRIDE, false, false, false>(in, w, nullptr, out, n, s, zp);
}
// conv i of the table on input `in`
template <typename T>
static int conv_forward(int i, const T* in, const T* wp, const float* zb, T* out, int n, hipStream_t s, const char* zp) {
  const ConvDesc& d = kConvs[i];
  if (i == 0) {
    ConvW w{const_cast<T*>(wp), const_cast<float*>(zb)};
    return launch_conv<T, 4, 64, 224, 224, 7, 2, false, false, false, true>(in, w, nullptr, out, n, s);
  }
  if (d.ks == 3 && d.stride == 1) {
    switch (d.cout) {
      case 64: return conv_layer<T, 64, 64, 56, 3, 1>(in, wp, zb, out, n, s, zp);
      case 128: return conv_layer<T, 128, 128, 28, 3, 1>(in, wp, zb, out, n, s, zp);
      case 256: return conv_layer<T, 256, 256, 14, 3, 1>(in, wp, zb, out, n, s, zp);
      default: return conv_layer<T, 512, 512, 7, 3, 1>(in, wp, zb, out, n, s, zp);
    }
  }
  if (d.ks == 3) {
    switch (d.cout) {
      case 128: return conv_layer<T, 64, 128, 56, 3, 2>(in, wp, zb, out, n, s, zp);
      case 256: return conv_layer<T, 128, 256, 28, 3, 2>(in, wp, zb, out, n, s, zp);
      default: return conv_layer<T, 256, 512, 14, 3, 2>(in, wp, zb, out, n, s, zp);
    }
  }
  switch (d.cout) {
    case 128: return conv_layer<T, 64, 128, 56, 1, 2>(in, wp, zb, out, n, s, zp);
    case 256: return conv_layer<T, 128, 256, 28, 1, 2>(in, wp, zb, out, n, s, zp);
    default: return conv_layer<T, 256, 512, 14, 1, 2>(in, wp, zb, out, n, s, zp);
  }
}
// data gradient of a 3x3 / stride 1 conv i (Cin = Cout): g (gradient wrt the conv output) -> gradient wrt the conv input, i.e.
// the same convolution on the weights packed in mode 1 (stride-2 convs: conv_dgrad_s2)
template <typename T>
static int conv_dgrad(int i, const T* g, const T* wd, const float* zb, T* out, int n, hipStream_t s, const char* zp) {
  return conv_forward<T>(i, g, wd, zb, out, n, s, zp);
}
// data gradient of a STRIDE-2 conv i by parity classes: g on the coarse grid, weights in mode 3 (3x3) or 1 (1x1; `out` zeroed)
template <typename T>
static int conv_dgrad_s2(int i, const T* g, const T* wd, const float* zb, T* out, int n, hipStream_t s, const char* zp) {
  const ConvDesc& d = kConvs[i];
  if (d.ks == 3) {
    switch (d.cout) {
      case 128: return launch_dgrad_s2<T, 128, 64, 28, true>(g, wd, zb, out, n, s, zp);
      case 256: return launch_dgrad_s2<T, 256, 128, 14, true>(g, wd, zb, out, n, s, zp);
      default: return launch_dgrad_s2<T, 512, 256, 7, true>(g, wd, zb, out, n, s, zp);
    }
  }
  switch (d.cout) {
    case 128: return launch_dgrad_s2<T, 128, 64, 28, false>(g, wd, zb, out, n, s, zp);
    case 256: return launch_dgrad_s2<T, 256, 128, 14, false>(g, wd, zb, out, n, s, zp);
    default: return launch_dgrad_s2<T, 512, 256, 7, false>(g, wd, zb, out, n, s, zp);
  }
}

// conv i's weights, fp32 [co][ci][kh][kw] -> T: mode 0 forward, 1 data gradient (flipped / transposed), 2 stem, 3 data gradient
// of a 3x3 / stride 2 conv by parity class (see pack_w_kernel)
template <class P>
static int pack_weights(const float* w, typename P::T* dst, int i, int mode, hipStream_t s) {
  const ConvDesc& d = kConvs[i];
  const long long total = (long long)conv_w_floats(i);
  if (mode == 2) HIPAC_CHECK_HIP(hipMemsetAsync(dst, 0, packed_w_floats(0) * sizeof(typename P::T), s));
  hipLaunchKernelGGL(pack_w_kernel<typename P::T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w, dst, d.cout, d.cin, d.ks, mode);
  return (int)hipGetLastError();
}

// Test tap: byte offset inside the workspace of a map the forward keeps (kind 0: conv output before BN, 1: after BN
// (+ residual) (+ ReLU), both NHWC T [batch][H][W][Cout]; 2: the pooled stem map [batch][56][56][64]; 3: batch mean[Cout]
// then rstd[Cout] (floats) of conv `conv`; 4: the pool's arg-max bytes [batch][56][56][64], 0..8 = dy * 3 + dx).
// Returns -1 on a bad argument.
template <class P>
static int64_t train_debug_offset(int batch, int kind, int conv) {
  if (batch <= 0 || conv < 0 || conv >= kNumConvs) return -1;
  const TrainPlan p = make_train_plan<P>(batch);
  switch (kind) {
    case 0: return (int64_t)p.pre[conv];
    case 1: return (int64_t)p.post[conv];
    case 2: return (int64_t)p.pool;
    case 3: return (int64_t)(p.mean_rstd + stat_offset(conv) * 4);
    case 4: return (int64_t)p.pool_idx;
    default: return -1;
  }
}

#define TRY(e)                                                                                     \
  do {                                                                                             \
    int rc__ = (e);                                                                                \
    HIPAC_REQUIRE(rc__ == 0, rc__, "%s: launch failed (%d) at line %d", P::kName, rc__, __LINE__); \
  } while (0)

// train-mode forward: stem -> max-pool -> 4 stages of 2 BasicBlocks -> global average pool into feats[batch][512]
template <class P>
static int train_encoder_forward(const float* params, float* stats, const float* x, int batch, float momentum, float eps,
                                 float* feats, void* workspace, size_t workspace_bytes, hipStream_t s) {
  using T = typename P::T;
  HIPAC_REQUIRE(params && x && feats && workspace, HIPAC_EINVAL, "%s_forward: null argument", P::kName);
  HIPAC_REQUIRE(batch > 0 && batch <= P::kMaxBatch, HIPAC_EINVAL, "%s_forward: batch %d (1 .. %d: 32-bit offsets)", P::kName,
                batch, P::kMaxBatch);
  const TrainPlan p = make_train_plan<P>(batch);
  HIPAC_REQUIRE(workspace_bytes >= p.total, HIPAC_EWORKSPACE, "%s_forward: workspace %zu < required %zu", P::kName,
                workspace_bytes, p.total);
  HIPAC_REQUIRE(((uintptr_t)workspace & 255) == 0, HIPAC_EINVAL, "%s_forward: workspace must be 256-byte aligned", P::kName);
  char* ws = (char*)workspace;
  const int n = batch;
  float* zb = (float*)(ws + p.zero_bias);
  const char* zp = p.zero_page ? ws + p.zero_page : nullptr;
  HIPAC_CHECK_HIP(hipMemsetAsync(zb, 0, 512 * 4 + (zp ? 256 : 0), s));  // zero_bias and the zero_page behind it
  auto wpack = [&](int i) { return (T*)(ws + p.wpack[i]); };
  for (int i = 0; i < kNumConvs; ++i) TRY(pack_weights<P>(params + param_offset(i), wpack(i), i, i == 0 ? 2 : 0, s));
  TRY(launch_nchw_to_nhwc4(x, ws + p.xin, n, P::kPrec, s));
  const TrainCtx c{params, stats, ws, &p, eps, momentum, s};
  auto pre = [&](int i) { return (T*)(ws + p.pre[i]); };
  auto post = [&](int i) { return (T*)(ws + p.post[i]); };
  // stem
  TRY(conv_forward<T>(0, (const T*)(ws + p.xin), wpack(0), zb, pre(0), n, s, zp));
  TRY(bn_forward<T>(c, 0, n, nullptr, 1));
  maxpool<T>(post(0), (T*)(ws + p.pool), (unsigned char*)(ws + p.pool_idx), n, s);
  TRY((int)hipGetLastError());
  const T* cur = (const T*)(ws + p.pool);
  int i = 1;
  for (int stage = 0; stage < 4; ++stage) {
    for (int blk = 0; blk < 2; ++blk) {
      const bool down = stage > 0 && blk == 0;
      const int c1 = i, c2 = i + 1, ds = down ? i + 2 : -1;
      TRY(conv_forward<T>(c1, cur, wpack(c1), zb, pre(c1), n, s, zp));
      TRY(bn_forward<T>(c, c1, n, nullptr, 1));
      const T* idt = cur;
      if (down) {
        TRY(conv_forward<T>(ds, cur, wpack(ds), zb, pre(ds), n, s, zp));
        TRY(bn_forward<T>(c, ds, n, nullptr, 0));
        idt = post(ds);
      }
      TRY(conv_forward<T>(c2, post(c1), wpack(c2), zb, pre(c2), n, s, zp));
      TRY(bn_forward<T>(c, c2, n, idt, 1));
      cur = post(c2);
      i += down ? 3 : 2;
    }
  }
  avgpool<T>(cur, feats, n, s);
  TRY((int)hipGetLastError());
  return 0;
}

// backward of the forward above (its workspace holds the maps): dfeats[batch][512] -> every conv / BN gradient into grads
template <class P>
static int train_encoder_backward(const float* params, const float* dfeats, int batch, float* grads, int accumulate,
                                  void* workspace, size_t workspace_bytes, hipStream_t s) {
  using T = typename P::T;
  HIPAC_REQUIRE(params && dfeats && grads && workspace, HIPAC_EINVAL, "%s_backward: null argument", P::kName);
  HIPAC_REQUIRE(batch > 0 && batch <= P::kMaxBatch, HIPAC_EINVAL, "%s_backward: batch %d", P::kName, batch);
  const TrainPlan p = make_train_plan<P>(batch);
  HIPAC_REQUIRE(workspace_bytes >= p.total, HIPAC_EWORKSPACE, "%s_backward: workspace %zu < required %zu", P::kName,
                workspace_bytes, p.total);
  char* ws = (char*)workspace;
  const int n = batch;
  const float* zb = (const float*)(ws + p.zero_bias);
  const char* zp = p.zero_page ? ws + p.zero_page : nullptr;
  T* wd = (T*)(ws + p.wpack_d);
  const TrainCtx c{params, nullptr, ws, &p, 0.f, 0.f, s};
  auto post = [&](int i) { return (T*)(ws + p.post[i]); };
  T* gA = (T*)(ws + p.g[0]);  // gradient wrt the current block's output (after its ReLU mask)
  T* gB = (T*)(ws + p.g[1]);
  T* gC = (T*)(ws + p.g[2]);
  T* up = (T*)(ws + p.up);
  // global average pool + the last block's ReLU
  avgpool_bwd<T>(dfeats, post(19), gA, n, s);
  TRY((int)hipGetLastError());
  // blocks in reverse.  conv indices of block (stage, blk): see kConvs
  static const int kFirst[4][2] = {{1, 3}, {5, 8}, {10, 13}, {15, 18}};
  for (int stage = 3; stage >= 0; --stage) {
    for (int blk = 1; blk >= 0; --blk) {
      const bool down = stage > 0 && blk == 0;
      const int c1 = kFirst[stage][blk], c2 = c1 + 1, ds = down ? c1 + 2 : -1;
      // input of the block = output of the previous block (the pooled map for the very first); that map is
      // also the ReLU mask of the gradient handed to the previous block (nothing to mask after the pool)
      const T* xin_blk;
      const T* prev_post;
      if (stage == 0 && blk == 0) xin_blk = (const T*)(ws + p.pool), prev_post = nullptr;
      else {
        const int pc2 = (blk == 1 ? kFirst[stage][0] : kFirst[stage - 1][1]) + 1;  // conv2 of the previous block
        xin_blk = post(pc2), prev_post = xin_blk;
      }
      const ConvDesc& d1 = kConvs[c1];
      const long long n_in = (long long)n * d1.hin * d1.hin * d1.cin;
      // --- main path: bn2 -> conv2 -> (ReLU) bn1 -> conv1
      TRY(bn_backward<T>(c, c2, n, gA, nullptr, gB, grads, accumulate));  // gB = d pre(c2)
      TRY(P::conv_wgrad(c, c2, n, post(c1), gB, grads, accumulate));
      TRY(pack_weights<P>(params + param_offset(c2), wd, c2, 1, s));
      TRY(conv_dgrad<T>(c2, gB, wd, zb, gC, n, s, zp));                    // gC = d post(c1) (before its ReLU mask)
      TRY(bn_backward<T>(c, c1, n, gC, post(c1), gC, grads, accumulate));  // gC = d pre(c1)
      TRY(P::conv_wgrad(c, c1, n, xin_blk, gC, grads, accumulate));
      if (d1.stride == 2) {
        TRY(pack_weights<P>(params + param_offset(c1), wd, c1, 3, s));
        TRY(conv_dgrad_s2<T>(c1, gC, wd, zb, gB, n, s, zp));               // gB = d block input via the main path
      } else {
        TRY(pack_weights<P>(params + param_offset(c1), wd, c1, 1, s));
        TRY(conv_dgrad<T>(c1, gC, wd, zb, gB, n, s, zp));                  // gB = d block input via the main path
      }
      // --- identity path
      if (down) {
        TRY(bn_backward<T>(c, ds, n, gA, nullptr, gC, grads, accumulate));  // gC = d pre(ds)
        TRY(P::conv_wgrad(c, ds, n, xin_blk, gC, grads, accumulate));
        TRY(pack_weights<P>(params + param_offset(ds), wd, ds, 1, s));
        // 1x1 / stride 2: only the even positions of the fine grid receive a gradient; `up` takes it (gC holds the input)
        HIPAC_CHECK_HIP(hipMemsetAsync(up, 0, (size_t)n * d1.hin * d1.hin * kConvs[ds].cin * sizeof(T), s));
        TRY(conv_dgrad_s2<T>(ds, gC, wd, zb, up, n, s, zp));
        add_mask<T>(gB, up, prev_post, gA, n_in, s);
      } else {
        add_mask<T>(gB, gA, prev_post, gA, n_in, s);
      }
      TRY((int)hipGetLastError());
    }
  }
  // max-pool, stem BN (+ ReLU mask), stem weight gradient
  maxpool_bwd<T>(gA, (const unsigned char*)(ws + p.pool_idx), gB, n, s);
  TRY((int)hipGetLastError());
  TRY(bn_backward<T>(c, 0, n, gB, post(0), gB, grads, accumulate));
  TRY(P::conv_wgrad(c, 0, n, (const T*)(ws + p.xin), gB, grads, accumulate));
  return 0;
}
#undef TRY

}  // namespace hipac

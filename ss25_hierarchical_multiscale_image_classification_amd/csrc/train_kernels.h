// The small kernels around the convolutions of the train-mode ResNet18 step, written once for both precisions
// (train.hip: fp32 maps, train_amp.hip: fp16 maps): weight packing, batch-norm statistics / normalisation / backward,
// ReLU masks, max-pool and average pool with their backwards, and the fixed-order sum of the split-K weight-gradient partials.
// Every map kernel is a template on the element type T of the maps and handles V = 16 / sizeof(T) channels per thread
// (4 floats or 8 halves: one 16-byte access); the arithmetic is fp32 / fp64 whatever T is.  No atomics anywhere: every
// reduction adds per-workgroup partial sums in a fixed order, so a step run twice gives the same bits.
#pragma once
#include "common.h"

namespace hipac {

template <typename T> constexpr int kVec = 16 / (int)sizeof(T);          // channels per thread
template <typename T> constexpr int kVecLog2 = kVec<T> == 8 ? 3 : 2;  // C >> kVecLog2<T>: threads per row of C channels
template <typename T, int N> using vec_t = T __attribute__((ext_vector_type(N)));

// 16-byte load / store of V elements to and from float[V]
template <typename T>
__device__ __forceinline__ void ldv(const T* p, float (&v)[kVec<T>]) {
  const vec_t<T, kVec<T>> t = *reinterpret_cast<const vec_t<T, kVec<T>>*>(p);
#pragma unroll
  for (int e = 0; e < kVec<T>; ++e) v[e] = (float)t[e];
}
template <typename T>
__device__ __forceinline__ void stv(T* p, const float (&v)[kVec<T>]) {
  vec_t<T, kVec<T>> t;
#pragma unroll
  for (int e = 0; e < kVec<T>; ++e) t[e] = (T)v[e];
  *reinterpret_cast<vec_t<T, kVec<T>>*>(p) = t;
}
// V arg-max bytes of the pool as V / 4 dwords (channel 4 j + k of the group = byte k of dword j)
template <int V>
__device__ __forceinline__ void ld_codes(const unsigned char* p, unsigned (&w)[V / 4]) {
  if constexpr (V == 8) {
    const u32x2 t = *reinterpret_cast<const u32x2*>(p);
    w[0] = t[0], w[1] = t[1];
  } else w[0] = *reinterpret_cast<const unsigned*>(p);
}
template <int V>
__device__ __forceinline__ void st_codes(unsigned char* p, const unsigned (&w)[V / 4]) {
  if constexpr (V == 8) *reinterpret_cast<u32x2*>(p) = u32x2{w[0], w[1]};
  else *reinterpret_cast<unsigned*>(p) = w[0];
}

// conv weights, fp32 [co][ci][kh][kw] -> T:
// mode 0: forward pack  dst[co][(kh*ks+kw)*cin + ci]
// mode 1: data-gradient dst[ci][((ks-1-kh)*ks + ks-1-kw)*cout + co]
// mode 2: stem          dst[co][kh*32 + kw*4 + ci] (row of 224, rest zero: the caller clears dst)
// mode 3: data gradient of a 3x3 / stride 2 conv, four parity-class blocks (see below)
template <typename T>
__global__ __launch_bounds__(256) void pack_w_kernel(const float* __restrict__ w, T* __restrict__ dst, int cout, int cin, int ks,
                                                     int mode) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)cout * cin * ks * ks) return;
  const int kw = (int)(gid % ks);
  long long t = gid / ks;
  const int kh = (int)(t % ks);
  t /= ks;
  const int ci = (int)(t % cin), co = (int)(t / cin);
  const T v = (T)w[gid];
  if (mode == 0) dst[(size_t)co * ks * ks * cin + (size_t)(kh * ks + kw) * cin + ci] = v;
  else if (mode == 1) dst[(size_t)ci * ks * ks * cout + (size_t)((ks - 1 - kh) * ks + ks - 1 - kw) * cout + co] = v;
  else if (mode == 3) {
    // data gradient of a 3x3 / stride 2 conv by parity class (launch_dgrad_s2, conv_launch.h): class (py, px) = (kh != 1, kw != 1),
    // its taps (a, b) = ((2 - kh) / 2, (2 - kw) / 2) -- tap a = 0 is the coarse row of the output position itself (kh = 2), a = 1 the
    // row below (kh = 0); blocks of 1, 2, 2, 4 taps back to back, each [ci][tap][co]
    const int py = kh != 1, px = kw != 1, a = py ? (2 - kh) / 2 : 0, b = px ? (2 - kw) / 2 : 0;
    const int ntap = (py ? 2 : 1) * (px ? 2 : 1), tap = a * (px ? 2 : 1) + b;
    const size_t blk = (size_t)cin * cout, off = (py ? 3 : 0) * blk + (px ? (py ? 2 : 1) : 0) * blk;
    dst[off + (size_t)ci * ntap * cout + (size_t)tap * cout + co] = v;
  } else dst[(size_t)co * 224 + kh * 32 + kw * 4 + ci] = v;
}

// Two per-channel sums over the M rows of [M][C] maps (C % V == 0, C / V <= 256), V channels per thread, fp64, NO atomics:
// workgroup b leaves its partial sums in part[b][0..C) and part[b][512..512+C).  MODE 0: (sum x, sum x^2).  MODE 1 (BN
// backward): (sum dy, sum dy * xhat) with dy masked by (ymask > 0) when given.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void bn_reduce_kernel(const T* __restrict__ a, const T* __restrict__ x,
                                                        const T* __restrict__ ymask, long long M, int C,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        double* __restrict__ part) {
  constexpr int V = kVec<T>;
  const int cv = C >> kVecLog2<T>, rows_per_pass = 256 / cv, tid = threadIdx.x, g = tid % cv, rsub = tid / cv;
  double s[V], q[V];
#pragma unroll
  for (int k = 0; k < V; ++k) s[k] = q[k] = 0.0;
  if (rsub < rows_per_pass) {
    float mu[V], rs[V];
    if (MODE == 1) {
#pragma unroll
      for (int k = 0; k < V; ++k) mu[k] = mean[V * g + k], rs[k] = rstd[V * g + k];
    }
    const long long step = (long long)gridDim.x * rows_per_pass;
    long long r = (long long)blockIdx.x * rows_per_pass + rsub;
    if (MODE == 0) {
      // four rows in flight per thread (the pass is a chain of dependent 16-byte loads otherwise), added in row order
      for (; r + 3 * step < M; r += 4 * step) {
        float v0[V], v1[V], v2[V], v3[V];
        ldv(a + r * C + V * g, v0), ldv(a + (r + step) * C + V * g, v1), ldv(a + (r + 2 * step) * C + V * g, v2), ldv(a + (r + 3 * step) * C + V * g, v3);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          s[k] += v0[k], q[k] += (double)v0[k] * v0[k];
          s[k] += v1[k], q[k] += (double)v1[k] * v1[k];
          s[k] += v2[k], q[k] += (double)v2[k] * v2[k];
          s[k] += v3[k], q[k] += (double)v3[k] * v3[k];
        }
      }
    }
    if (MODE == 1) {
      // two rows (four to six loads) in flight per thread, added in row order
      for (; r + step < M; r += 2 * step) {
        float va[V], vb[V], xa[V], xb[V];
        ldv(a + r * C + V * g, va), ldv(a + (r + step) * C + V * g, vb);
        ldv(x + r * C + V * g, xa), ldv(x + (r + step) * C + V * g, xb);
        if (ymask) {
          float ma[V], mb[V];
          ldv(ymask + r * C + V * g, ma), ldv(ymask + (r + step) * C + V * g, mb);
#pragma unroll
          for (int k = 0; k < V; ++k) va[k] = ma[k] > 0.f ? va[k] : 0.f, vb[k] = mb[k] > 0.f ? vb[k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
          s[k] += va[k], q[k] += (double)va[k] * ((xa[k] - mu[k]) * rs[k]);
          s[k] += vb[k], q[k] += (double)vb[k] * ((xb[k] - mu[k]) * rs[k]);
        }
      }
    }
    for (; r < M; r += step) {
      float v[V];
      ldv(a + r * C + V * g, v);
      if (MODE == 0) {
#pragma unroll
        for (int k = 0; k < V; ++k) s[k] += v[k], q[k] += (double)v[k] * v[k];
      } else {
        float xv[V];
        ldv(x + r * C + V * g, xv);
        if (ymask) {
          float m[V];
          ldv(ymask + r * C + V * g, m);
#pragma unroll
          for (int k = 0; k < V; ++k) v[k] = m[k] > 0.f ? v[k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < V; ++k) s[k] += v[k], q[k] += (double)v[k] * ((xv[k] - mu[k]) * rs[k]);
      }
    }
  }
  __shared__ double red[2][256][V];
#pragma unroll
  for (int k = 0; k < V; ++k) red[0][tid][k] = s[k], red[1][tid][k] = q[k];
  __syncthreads();
  if (tid < cv) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      double sa = 0, sb = 0;
      for (int rr = 0; rr < rows_per_pass; ++rr) sa += red[0][rr * cv + tid][k], sb += red[1][rr * cv + tid][k];
      part[(size_t)blockIdx.x * 1024 + V * tid + k] = sa;
      part[(size_t)blockIdx.x * 1024 + 512 + V * tid + k] = sb;
    }
  }
}

// partial sums -> sums[c], sums[512 + c] in a FIXED order (lane l of the channel's 32 adds blocks l, l + 32, ... in turn,
// then a shuffle tree): 8 channels per workgroup; FINAL (the forward): also mean / rstd (biased variance, as the normalisation
// uses) and the running statistics (momentum, unbiased variance)
template <bool FINAL>
__global__ __launch_bounds__(256) void bn_sum_parts_kernel(const double* __restrict__ part, int nblocks, int C,
                                                           double* __restrict__ sums, long long M, float eps, float momentum,
                                                           float* __restrict__ mean, float* __restrict__ rstd,
                                                           float* __restrict__ run_mean, float* __restrict__ run_var) {
  const int c = blockIdx.x * 8 + (threadIdx.x >> 5), l = threadIdx.x & 31;
  double a = 0, b = 0;
  if (c < C)
    for (int k = l; k < nblocks; k += 32) a += part[(size_t)k * 1024 + c], b += part[(size_t)k * 1024 + 512 + c];
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) a += __shfl_down(a, o, 32), b += __shfl_down(b, o, 32);
  if (c >= C || l != 0) return;
  sums[c] = a, sums[512 + c] = b;
  if (FINAL) {
    const double mu = a / (double)M;
    double var = b / (double)M - mu * mu;
    if (var < 0) var = 0;
    mean[c] = (float)mu;
    rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (run_mean) {
      const double unb = M > 1 ? var * (double)M / (double)(M - 1) : var;
      run_mean[c] = (float)((1.0 - momentum) * run_mean[c] + momentum * mu);
      run_var[c] = (float)((1.0 - momentum) * run_var[c] + momentum * unb);
    }
  }
}

// y = (x - mean) * rstd * gamma + beta (+ resid) (ReLU).  The grid stride (gridDim.x * 256 * V elements) must be a multiple
// of C (bn_apply_geometry_ok, train_common.h): a thread then meets the same V channels in every iteration and loads their
// constants once.
template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ x, const T* __restrict__ resid, T* __restrict__ y,
                                                       long long nv, int C, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, int relu) {
  constexpr int V = kVec<T>;
  const int c = (threadIdx.x * V) % C;
  float mu[V], sc[V], be[V];
#pragma unroll
  for (int k = 0; k < V; ++k) mu[k] = mean[c + k], sc[k] = rstd[c + k], be[k] = beta[c + k];
  float ga[V];
#pragma unroll
  for (int k = 0; k < V; ++k) ga[k] = gamma[c + k];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
    float v[V], o[V];
    ldv(x + i * V, v);
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = (v[k] - mu[k]) * sc[k] * ga[k] + be[k];
    if (resid) {
      float r[V];
      ldv(resid + i * V, r);
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] += r[k];
    }
    if (relu) {
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = fmaxf(o[k], 0.f);
    }
    stv(y + i * V, o);
  }
}

// BN backward, pass 2: dx = gamma * rstd * (dy - sum_dy / M - xhat * sum_dy_xhat / M); d gamma, d beta (fp32 gradients).
// The per-channel constants are hoisted as in bn_apply_kernel.
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                           const T* __restrict__ ymask, T* __restrict__ dx, long long nv,
                                                           long long M, int C, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                           const double* __restrict__ sums, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, int accumulate) {
  constexpr int V = kVec<T>;
  if (blockIdx.x == 0) {
    for (int c = threadIdx.x; c < C; c += 256) {
      const float dg = (float)sums[512 + c], db = (float)sums[c];
      dgamma[c] = accumulate ? dgamma[c] + dg : dg;
      dbeta[c] = accumulate ? dbeta[c] + db : db;
    }
  }
  const double invM = 1.0 / (double)M;
  const int c = (threadIdx.x * V) % C;
  float mu[V], rs[V], gr[V], sb[V], sg[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    mu[k] = mean[c + k], rs[k] = rstd[c + k], gr[k] = gamma[c + k] * rstd[c + k];
    sb[k] = (float)(sums[c + k] * invM), sg[k] = (float)(sums[512 + c + k] * invM);
  }
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
    float d[V], v[V], o[V];
    ldv(dy + i * V, d);
    ldv(x + i * V, v);
    if (ymask) {
      float m[V];
      ldv(ymask + i * V, m);
#pragma unroll
      for (int k = 0; k < V; ++k) d[k] = m[k] > 0.f ? d[k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = gr[k] * (d[k] - sb[k] - (v[k] - mu[k]) * rs[k] * sg[k]);
    stv(dx + i * V, o);
  }
}

// out = (a + b) masked by (y > 0); b / y optional
template <typename T>
__global__ __launch_bounds__(256) void add_mask_kernel(const T* __restrict__ a, const T* __restrict__ b, const T* __restrict__ y,
                                                       T* __restrict__ out, long long nv) {
  constexpr int V = kVec<T>;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
    float v[V];
    ldv(a + i * V, v);
    if (b) {
      float w[V];
      ldv(b + i * V, w);
#pragma unroll
      for (int k = 0; k < V; ++k) v[k] += w[k];
    }
    if (y) {
      float m[V];
      ldv(y + i * V, m);
#pragma unroll
      for (int k = 0; k < V; ++k) v[k] = m[k] > 0.f ? v[k] : 0.f;
    }
    stv(out + i * V, v);
  }
}

// 3x3/2 max-pool, pad 1, of [B,112,112,64] with the arg-max kept (first maximum in (dy, dx) scan order, as torch; code
// dy * 3 + dx, 9 = none); V channels of one output position per thread, totalv = B * 56 * 56 * (64 / V)
template <typename T>
__global__ __launch_bounds__(256) void maxpool_idx_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                          unsigned char* __restrict__ idx, long long totalv) {
  constexpr int HI = 112, HO = 56, C = 64, V = kVec<T>;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= totalv) return;
  const int cv = (int)(gid % (C / V));
  long long p = gid / (C / V);
  const int ow = (int)(p % HO);
  p /= HO;
  const int oh = (int)(p % HO);
  const long long b = p / HO;
  float best[V];
  int bi[V];
#pragma unroll
  for (int k = 0; k < V; ++k) best[k] = -INFINITY, bi[k] = 9;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const int ih = oh * 2 - 1 + dy;
    if ((unsigned)ih >= (unsigned)HI) continue;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int iw = ow * 2 - 1 + dx;
      if ((unsigned)iw >= (unsigned)HI) continue;
      float v[V];
      ldv(in + ((b * HI + ih) * HI + iw) * C + V * cv, v);
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (v[k] > best[k] || bi[k] == 9) best[k] = v[k], bi[k] = dy * 3 + dx;
    }
  }
  stv(out + gid * V, best);
  unsigned w[V / 4];
#pragma unroll
  for (int k = 0; k < V / 4; ++k) w[k] = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int j = 0; j < V / 4; ++j) w[j] |= (unsigned)bi[4 * j + k] << (8 * k);
  st_codes<V>(idx + gid * V, w);
}

// max-pool backward (gather form): every input position sums the gradients of the <= 4 windows that chose it.  A thread owns a
// 2 x 2 quad of input positions (2y .. 2y+1, 2x .. 2x+1) x V channels: the quad only ever belongs to the four windows
// (y .. y+1) x (x .. x+1) -- row 2y to window row y alone (dy = 1), row 2y+1 to window rows y (dy = 2) and y+1 (dy = 0) -- so four
// window loads serve four outputs.  totalv = B * 56 * 56 * (64 / V)
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ dout, const unsigned char* __restrict__ idx,
                                                          T* __restrict__ din, long long totalv) {
  constexpr int HI = 112, HO = 56, C = 64, V = kVec<T>;
  // An (odd, odd) input position adds up to four window gradients, and the order of a float sum is part of the result.  The
  // fp16 step has always walked the windows upwards; the fp32 step's earlier one-thread-per-position kernel met them in
  // descending window row, then descending window column.  This constant exists only to keep the fp32 bits.
  constexpr bool kDescending = std::is_same<T, float>::value;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;  // (b, y, x, cv) over the 56 x 56 quads
  if (gid >= totalv) return;
  const int cv = (int)(gid % (C / V));
  long long p = gid / (C / V);
  const int x = (int)(p % HO);
  p /= HO;
  const int y = (int)(p % HO);
  const long long b = p / HO;
  float acc[2][2][V];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < V; ++k) acc[i][j][k] = 0.f;
#pragma unroll
  for (int sy = 0; sy < 2; ++sy) {
    const int wy = kDescending ? 1 - sy : sy, oh = y + wy;
    if (oh >= HO) continue;
#pragma unroll
    for (int sx = 0; sx < 2; ++sx) {
      const int wx = kDescending ? 1 - sx : sx, ow = x + wx;
      if (ow >= HO) continue;
      const long long o = ((b * HO + oh) * HO + ow) * C + V * cv;
      unsigned ib[V / 4];
      ld_codes<V>(idx + o, ib);
      float g[V];
      ldv(dout + o, g);
      // window (oh, ow) covers input rows 2 oh - 1 + dy: quad row i = 0 (input row 2y) is dy = 1 of wy = 0; quad row i = 1
      // (input row 2y + 1) is dy = 2 of wy = 0 and dy = 0 of wy = 1 -- the same in x
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int dy = wy == 0 ? 1 + i : (i == 1 ? 0 : -1);
        if (dy < 0) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int dx = wx == 0 ? 1 + j : (j == 1 ? 0 : -1);
          if (dx < 0) continue;
          const int code = dy * 3 + dx;
#pragma unroll
          for (int k = 0; k < V; ++k)
            if ((int)((ib[k >> 2] >> (8 * (k & 3))) & 0xffu) == code) acc[i][j][k] += g[k];
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
      stv(din + (((b * HI + 2 * y + i) * HI + 2 * x + j) * C + V * cv), acc[i][j]);
}

// feats[b][c] = mean over the 49 pixels of last[b][49][512]; one workgroup per image, two channels per thread
template <typename T>
__global__ __launch_bounds__(256) void avgpool_kernel(const T* __restrict__ last, float* __restrict__ feats, int n) {
  const int b = blockIdx.x, t = threadIdx.x;
  float s0 = 0.f, s1 = 0.f;
  for (int p = 0; p < 49; ++p) {
    const vec_t<T, 2> v = *reinterpret_cast<const vec_t<T, 2>*>(last + ((size_t)b * 49 + p) * 512 + 2 * t);
    s0 += (float)v[0], s1 += (float)v[1];
  }
  *reinterpret_cast<float2*>(feats + (size_t)b * 512 + 2 * t) = make_float2(s0 / 49.0f, s1 / 49.0f);
}

// d last[b][p][c] = dfeats[b][c] / 49 where last > 0 (the final ReLU)
template <typename T>
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const float* __restrict__ dfeats, const T* __restrict__ last,
                                                          T* __restrict__ dlast, long long total) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int c = (int)(gid % 512);
  const long long b = gid / (49 * 512);
  dlast[gid] = (float)last[gid] > 0.f ? (T)(dfeats[b * 512 + c] * (1.0f / 49.0f)) : (T)0.f;
}

// split-K partials of a weight gradient (generic: part[slice][tap][co][ci]; stem: part[slice][kh][co][kw*4 + ci], 32 per row)
// -> the PyTorch-layout gradient (accumulate or overwrite).  32 weights per workgroup x 8 slice groups: group g adds slices
// g, g + 8, ... in turn, then the 8 group sums are added in order -- a fixed order, hence reproducible
template <int UNUSED = 0>  // (a template: the header is part of two translation units)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, int slices, float* __restrict__ dw,
                                                           int cout, int cin, int ks, int stem, int accumulate) {
  __shared__ float red[8][32];
  const int e = threadIdx.x & 31, g = threadIdx.x >> 5;
  const long long gid = (long long)blockIdx.x * 32 + e;
  const long long total = (long long)cout * cin * ks * ks;
  float s = 0.f;
  if (gid < total) {
    const int kw = (int)(gid % ks);
    long long t = gid / ks;
    const int kh = (int)(t % ks);
    t /= ks;
    const int ci = (int)(t % cin), co = (int)(t / cin);
    const size_t per_slice = stem ? (size_t)7 * cout * 32 : (size_t)total;
    const size_t o = stem ? ((size_t)kh * cout + co) * 32 + kw * 4 + ci : ((size_t)(kh * ks + kw) * cout + co) * cin + ci;
    for (int k = g; k < slices; k += 8) s += part[(size_t)k * per_slice + o];
  }
  red[g][e] = s;
  __syncthreads();
  if (g == 0 && gid < total) {
    float v = red[0][e];
#pragma unroll
    for (int k = 1; k < 8; ++k) v += red[k][e];
    dw[gid] = accumulate ? dw[gid] + v : v;
  }
}

}  // namespace hipac

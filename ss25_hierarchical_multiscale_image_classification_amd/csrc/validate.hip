// The feature sanity check (include/hipac_validate.h): the sweeps over the [N][F] feature matrix behind a two-component
// PCA and a class-weighted logistic-regression probe fitted with Newton's method, fp32.
//
//   colsum    out[f]  = sum_i w_i x_i[f]
//   gram      G[a][b] = sum_i w_i (x_i[a] - c[a]) (x_i[b] - c[b])        v_mfma_f32_32x32x2_f32
//   sweep     m_i = x_i . w + b; loss, r_i, d_i; sum r_i x_i, sum d_i x_i, sum r_i, sum d_i   one read of X
//   project   Z[i][k] = (x_i - c) . W[k]; per-class sums and counts
//
// The three row sweeps share one shape: a wave owns a row at a time and keeps it in registers (lane l holds the float4
// columns l, l + 64, ..: NV = 1, 2, 4 or 8 of them), so the dot product, the factors made from it and the weighted
// column sums all come from one read; 8 / NV rows are in flight per wave.  A workgroup adds its four waves' sums in wave
// order and writes one slab row; mil_train.hip's slab reduction adds the slab rows in a fixed order.  The Gram kernel
// works on 128 x 128 blocks on or above the diagonal, one slice of rows per workgroup, and its own reduction mirrors
// the upper triangle.  No float atomics anywhere: every result is a function of the arguments alone.
#include "common.h"

#include "../../include/hipac_validate.h"
#include "mil_train_internal.h"
#include "wave_reduce.h"

namespace hipac {

constexpr int kVdMaxF = 2048, kVdMaxN = 1 << 24, kVdMaxK = HIPAC_VALIDATE_MAX_COMPONENTS;
constexpr int kVdSweepSlices = 1024;                // most workgroups of a row sweep: 4 per CU
constexpr int kVdGramGranule = 128;                 // a slice is a multiple of this many rows: the two-level sum's inner length
constexpr int kVdGramTarget = 768;                  // workgroups the Gram grid aims at: 3 per CU
constexpr size_t kVdGramSlabCap = (size_t)128 << 20;  // bytes of Gram slabs at most (8 slices at F = 2048)
constexpr int kVdProjStride = 16;                   // floats of one projection slab row: [2][4] class sums | 2 counts | pad

static bool vd_sizes_ok(int n, int F) { return F >= 4 && F <= kVdMaxF && F % 4 == 0 && n >= 1 && n <= kVdMaxN; }

static void vd_sweep_slices(int n, int* chunk, int* slices) {
  int s = (n + 255) / 256;
  if (s > kVdSweepSlices) s = kVdSweepSlices;
  *chunk = (n + s - 1) / s;
  *slices = (n + *chunk - 1) / *chunk;
}

static int vd_gram_blocks(int F) {
  const int T = (F + 127) / 128;
  return T * (T + 1) / 2;
}

static void vd_gram_slices(int n, int F, int* chunk, int* slices) {
  const int nblk = vd_gram_blocks(F);
  long long s = (kVdGramTarget + nblk - 1) / nblk;
  const long long cap = (long long)(kVdGramSlabCap / ((size_t)F * F * 4));
  const long long by_n = (n + kVdGramGranule - 1) / kVdGramGranule;
  if (s > cap) s = cap;
  if (s > by_n) s = by_n;
  if (s < 1) s = 1;
  long long c = (n + s - 1) / s;
  c = (c + kVdGramGranule - 1) / kVdGramGranule * kVdGramGranule;
  *chunk = (int)c;
  *slices = (int)((n + c - 1) / c);
}

__device__ __forceinline__ float vd_dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// the four waves' column sums v (lane l: float4 columns l + 64 j) added in wave order -> dst[F]
template <int NV>
__device__ __forceinline__ void vd_wg_reduce_store(const float4 (&v)[NV], float4* red, float* dst, int F4) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __syncthreads();  // red may still be read from the previous call
#pragma unroll
  for (int j = 0; j < NV; ++j) red[wave * (NV * 64) + j * 64 + lane] = v[j];
  __syncthreads();
  for (int c4 = tid; c4 < NV * 64; c4 += 256)
    if (c4 < F4) {
      float4 a = red[c4];
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        const float4 t = red[k * (NV * 64) + c4];
        a.x += t.x, a.y += t.y, a.z += t.z, a.w += t.w;
      }
      reinterpret_cast<float4*>(dst)[c4] = a;
    }
}

template <int NV>
__device__ __forceinline__ void vd_load_vec(const float* p, int F4, float4 (&v)[NV]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c4 = lane + 64 * j;
    v[j] = (p && c4 < F4) ? reinterpret_cast<const float4*>(p)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// R rows m0 .. m0 + R - 1 of the batch (those below m_end) into registers; src[q] = the matrix row, -1 past the end
template <int NV, int R>
__device__ __forceinline__ void vd_load_rows(const float* __restrict__ X, const int32_t* __restrict__ rows, int F, int m0, int m_end,
                                             float4 (&x)[R][NV], int (&src)[R]) {
  const int lane = threadIdx.x & 63, F4 = F >> 2;
#pragma unroll
  for (int q = 0; q < R; ++q) {
    const int m = m0 + q;
    src[q] = m < m_end ? (rows ? rows[m] : m) : -1;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int c4 = lane + 64 * j;
      x[q][j] = (src[q] >= 0 && c4 < F4) ? reinterpret_cast<const float4*>(X + (size_t)src[q] * F)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
}

// slab[slice][F] = sum over the slice's rows of w_i x_i
template <int NV>
__global__ __launch_bounds__(256) void vd_colsum_kernel(const float* __restrict__ X, const int32_t* __restrict__ rows, int n, int F,
                                                        int chunk, const float* __restrict__ w, float* __restrict__ slab) {
  constexpr int R = 8 / NV;
  __shared__ float4 red[4 * NV * 64];
  const int wave = threadIdx.x >> 6;
  const int m_begin = blockIdx.x * chunk, m_end = m_begin + chunk < n ? m_begin + chunk : n;
  float4 acc[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int m0 = m_begin + wave * R; m0 < m_end; m0 += 4 * R) {
    float4 x[R][NV];
    int src[R];
    vd_load_rows<NV, R>(X, rows, F, m0, m_end, x, src);
#pragma unroll
    for (int q = 0; q < R; ++q)
      if (src[q] >= 0) {
        const float wi = w ? w[m0 + q] : 1.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j].x += wi * x[q][j].x, acc[j].y += wi * x[q][j].y, acc[j].z += wi * x[q][j].z, acc[j].w += wi * x[q][j].w;
      }
  }
  vd_wg_reduce_store<NV>(acc, red, slab + (size_t)blockIdx.x * F, F >> 2);
}

// slab[slice][2 F + 4] = sum r_i x_i [F] | sum d_i x_i [F] | sum r_i | sum d_i | sum l_i | 0 over the slice's rows
template <int NV>
__global__ __launch_bounds__(256) void vd_sweep_kernel(const float* __restrict__ X, const int32_t* __restrict__ rows, int n, int F,
                                                       int chunk, const float* __restrict__ coef, const float* __restrict__ intercept,
                                                       const int64_t* __restrict__ labels, const float* __restrict__ class_w,
                                                       float* __restrict__ d_out, float* __restrict__ m_out, float* __restrict__ slab) {
  constexpr int R = 8 / NV;
  __shared__ float4 red[4 * NV * 64];
  __shared__ double sc[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m_begin = blockIdx.x * chunk, m_end = m_begin + chunk < n ? m_begin + chunk : n;
  float4 wv[NV], gr[NV], gd[NV];
  vd_load_vec<NV>(coef, F >> 2, wv);
  const float b = intercept[0], s0 = class_w[0], s1 = class_w[1];
#pragma unroll
  for (int j = 0; j < NV; ++j) gr[j] = gd[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  double sr = 0., sd = 0., sl = 0.;  // three adds per row: double keeps the scalar sums at the rounding of their terms
  for (int m0 = m_begin + wave * R; m0 < m_end; m0 += 4 * R) {
    float4 x[R][NV];
    int src[R];
    vd_load_rows<NV, R>(X, rows, F, m0, m_end, x, src);
#pragma unroll
    for (int q = 0; q < R; ++q) {
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < NV; ++j) dot += vd_dot4(x[q][j], wv[j]);
      dot = wave_sum(dot);
      if (src[q] >= 0) {  // wave-uniform
        const float m = dot + b;
        const bool y = labels[src[q]] != 0;
        const float s = y ? s1 : s0;
        const float e = expf(-fabsf(m)), inv = 1.f / (1.f + e);
        const float p = m >= 0.f ? inv : e * inv;
        const float r = s * (p - (y ? 1.f : 0.f));
        const float d = s * (e * inv * inv);  // p (1 - p) = e / (1 + e)^2
        sl += (double)(s * (fmaxf(m, 0.f) + log1pf(e) - (y ? m : 0.f)));
        sr += r;
        sd += d;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          gr[j].x += r * x[q][j].x, gr[j].y += r * x[q][j].y, gr[j].z += r * x[q][j].z, gr[j].w += r * x[q][j].w;
          gd[j].x += d * x[q][j].x, gd[j].y += d * x[q][j].y, gd[j].z += d * x[q][j].z, gd[j].w += d * x[q][j].w;
        }
        if (lane == 0) {
          d_out[m0 + q] = d;
          if (m_out) m_out[m0 + q] = m;
        }
      }
    }
  }
  float* out = slab + (size_t)blockIdx.x * (2 * F + 4);
  vd_wg_reduce_store<NV>(gr, red, out, F >> 2);
  vd_wg_reduce_store<NV>(gd, red, out + F, F >> 2);
  if (lane == 0) sc[wave][0] = sr, sc[wave][1] = sd, sc[wave][2] = sl;
  __syncthreads();
  if (threadIdx.x < 4) out[2 * F + threadIdx.x] = threadIdx.x < 3 ? (float)(((sc[0][threadIdx.x] + sc[1][threadIdx.x]) + sc[2][threadIdx.x]) + sc[3][threadIdx.x]) : 0.f;
}

// Z[i][k] = (x_i - c) . W[k]; slab[slice][16] = class sums [2][4] | counts [2] | 0 ..
template <int NV>
__global__ __launch_bounds__(256) void vd_project_kernel(const float* __restrict__ X, const int32_t* __restrict__ rows, int n, int F,
                                                         int chunk, const float* __restrict__ c, const float* __restrict__ W, int K,
                                                         const int64_t* __restrict__ labels, float* __restrict__ Z,
                                                         float* __restrict__ slab) {
  __shared__ float sc[4][kVdProjStride];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m_begin = blockIdx.x * chunk, m_end = m_begin + chunk < n ? m_begin + chunk : n;
  float4 cv[NV], wk[kVdMaxK][NV];
  vd_load_vec<NV>(c, F >> 2, cv);
#pragma unroll
  for (int k = 0; k < kVdMaxK; ++k) vd_load_vec<NV>(k < K ? W + (size_t)k * F : nullptr, F >> 2, wk[k]);
  float cs[2][kVdMaxK] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, cnt[2] = {0.f, 0.f};
  for (int m0 = m_begin + wave; m0 < m_end; m0 += 4) {
    float4 x[1][NV];
    int src[1];
    vd_load_rows<NV, 1>(X, rows, F, m0, m_end, x, src);
    // columns past F: x and c are both zero there
#pragma unroll
    for (int j = 0; j < NV; ++j) x[0][j].x -= cv[j].x, x[0][j].y -= cv[j].y, x[0][j].z -= cv[j].z, x[0][j].w -= cv[j].w;
    float z[kVdMaxK];
#pragma unroll
    for (int k = 0; k < kVdMaxK; ++k) {
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < NV; ++j) dot += vd_dot4(x[0][j], wk[k][j]);
      z[k] = wave_sum(dot);
    }
    const int y = labels ? (labels[src[0]] != 0 ? 1 : 0) : 0;
    cnt[y] += 1.f;
#pragma unroll
    for (int k = 0; k < kVdMaxK; ++k) {
      if (y) cs[1][k] += z[k];
      else cs[0][k] += z[k];
      if (lane == 0 && k < K) Z[(size_t)m0 * K + k] = z[k];
    }
  }
  if (lane < kVdProjStride) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < kVdMaxK; ++k) {
      if (lane == k) v = cs[0][k];
      if (lane == kVdMaxK + k) v = cs[1][k];
    }
    if (lane == 2 * kVdMaxK) v = cnt[0];
    if (lane == 2 * kVdMaxK + 1) v = cnt[1];
    sc[wave][lane] = v;
  }
  __syncthreads();
  if (threadIdx.x < kVdProjStride)
    slab[(size_t)blockIdx.x * kVdProjStride + threadIdx.x] = ((sc[0][threadIdx.x] + sc[1][threadIdx.x]) + sc[2][threadIdx.x]) + sc[3][threadIdx.x];
}

constexpr int kVdGramLd = 132;  // LDS row of a Gram panel: 128 floats + 4 keeps float4 stores aligned and spreads banks

// 32 staged rows into a wave's 2 x 2 tiles: acc[2 ti + tj] += A[ti]^T B[tj].  A wave's quarter is wholly on or above the
// diagonal (LOWER: all four tiles), straddles it (the lower-left tile acc[2] is skipped), or lies below it (not called).
template <bool LOWER>
__device__ __forceinline__ void vd_gram_mma(const float* __restrict__ a, const float* __restrict__ b, int h, f32x16 (&acc)[4]) {
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int px = (2 * k + h) * kVdGramLd;
    const float a0 = a[px], a1 = a[px + 32], b0 = b[px], b1 = b[px + 32];
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[1], 0, 0, 0);
    if constexpr (LOWER) acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[2], 0, 0, 0);
    acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[3], 0, 0, 0);
  }
}

// Gram partials: slab[slice][a][b] = sum over the slice's rows of w_i (x_i[a] - c[a]) (x_i[b] - c[b]) for one 128 x 128
// block (bi, bj), bi <= bj, of G.  The reduction axis (rows) is the MFMA's k, as in mil_train.hip's mt_dv_kernel: 32
// rows at a time are staged into LDS as [row][column] -- the A panel (columns of block bi) as w_i (x - c), the B panel
// (columns of block bj) as x - c -- and read with the row as k.  A wave owns a 64 x 64 quarter = 2 x 2 tiles of 32 x 32
// and skips the tiles below the diagonal (a diagonal block does 10 of its 16 tiles, and loads its panel once).  The
// next 32 rows are fetched into registers while the MFMAs of the current ones run.  Two levels of summation as in
// mt_dv_kernel: 128 rows into acc, acc into tot.
__global__ __launch_bounds__(256) void vd_gram_kernel(const float* __restrict__ X, const int32_t* __restrict__ rows, int n, int F,
                                                      int chunk, const float* __restrict__ w, const float* __restrict__ c, int T,
                                                      float* __restrict__ slab) {
  constexpr int LD = kVdGramLd;
  __shared__ __attribute__((aligned(16))) float As[32 * LD], Bs[32 * LD], Cs[2 * 128];  // Cs: the centre of both panels
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: the tile switches below are branches, not lane masks
  const int r = lane & 31, h = lane >> 5;
  const int wi = wave >> 1, wj = wave & 1;
  int bi = 0, rem = blockIdx.x;  // blockIdx.x counts the blocks on or above the diagonal row by row
  while (rem >= T - bi) rem -= T - bi, ++bi;
  const int bj = bi + rem;
  const bool diag = bi == bj;
  bool act[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) act[t] = bi * 4 + wi * 2 + (t >> 1) <= bj * 4 + wj * 2 + (t & 1);
  const int m_begin = blockIdx.y * chunk;
  const int m_end = m_begin + chunk < n ? m_begin + chunk : n;
  const int spx = tid >> 3, sc = tid & 7;  // staging: row of the 32, float4 columns sc + 8 q
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  bool ina[4], inb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) ina[q] = bi * 128 + 4 * (sc + 8 * q) < F, inb[q] = bj * 128 + 4 * (sc + 8 * q) < F;
  {
    const int f = (tid < 128 ? bi * 128 : bj * 128 - 128) + tid;
    Cs[tid] = (c && f < F) ? c[f] : 0.f;  // read after the loop's first barrier
  }
  f32x16 acc[4], tot[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f, tot[t][e] = 0.f;

  float4 xa[4], xb[4];
  float wgt = 1.f;
  bool valid = false;
  // the raw rows m0 .. m0 + 31 of both panels into registers
#define VD_GRAM_FETCH(M0)                                                                                      \
  {                                                                                                            \
    const int m = (M0) + spx;                                                                                  \
    valid = m < m_end;                                                                                         \
    wgt = 1.f;                                                                                                 \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) xa[q] = xb[q] = zero4;                                       \
    if (valid) {                                                                                               \
      const float* row = X + (size_t)(rows ? rows[m] : m) * F;                                                 \
      if (w) wgt = w[m];                                                                                       \
      _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                          \
        if (ina[q]) xa[q] = *reinterpret_cast<const float4*>(row + bi * 128 + 4 * (sc + 8 * q));               \
        if (!diag && inb[q]) xb[q] = *reinterpret_cast<const float4*>(row + bj * 128 + 4 * (sc + 8 * q));      \
      }                                                                                                        \
    }                                                                                                          \
  }
  VD_GRAM_FETCH(m_begin)
  int sub = 0;
  for (int m0 = m_begin; m0 < m_end; m0 += 32) {
    __syncthreads();  // the previous 32 rows' fragments have been read
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // rows past the slice and columns past F are staged as zeros (not as -c)
      float4 a = zero4, b = zero4;
      const float4 ca = *reinterpret_cast<const float4*>(Cs + 4 * (sc + 8 * q)), cb = *reinterpret_cast<const float4*>(Cs + 128 + 4 * (sc + 8 * q));
      if (valid && ina[q]) {
        a = make_float4(xa[q].x - ca.x, xa[q].y - ca.y, xa[q].z - ca.z, xa[q].w - ca.w);
        if (diag) b = a;
        a.x *= wgt, a.y *= wgt, a.z *= wgt, a.w *= wgt;
      }
      if (!diag && valid && inb[q]) b = make_float4(xb[q].x - cb.x, xb[q].y - cb.y, xb[q].z - cb.z, xb[q].w - cb.w);
      *reinterpret_cast<float4*>(As + spx * LD + 4 * (sc + 8 * q)) = a;
      *reinterpret_cast<float4*>(Bs + spx * LD + 4 * (sc + 8 * q)) = b;
    }
    __syncthreads();
    if (m0 + 32 < m_end) VD_GRAM_FETCH(m0 + 32)
    // one scalar branch per 32 rows, straight-line MFMAs inside
    if (act[2]) vd_gram_mma<true>(As + (wi * 2) * 32 + r, Bs + (wj * 2) * 32 + r, h, acc);
    else if (act[0]) vd_gram_mma<false>(As + (wi * 2) * 32 + r, Bs + (wj * 2) * 32 + r, h, acc);
    if (++sub == 4 || m0 + 32 >= m_end) {
      sub = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        tot[t] += acc[t];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
      }
    }
  }
#undef VD_GRAM_FETCH
  // D[a][b]: column b = lane & 31, row a = (reg & 3) + 8 (reg >> 2) + 4 h
  float* base = slab + (size_t)blockIdx.y * F * F;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (act[t]) {
      const int gb = bj * 128 + (wj * 2 + (t & 1)) * 32 + r;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int ga = bi * 128 + (wi * 2 + (t >> 1)) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (ga < F && gb < F) base[(size_t)ga * F + gb] = tot[t][e];
      }
    }
}

// G[a][b] = G[b][a] = sum over slices of slab[k][a][b] for a <= b.  One workgroup per 32 x 32 tile on or above the diagonal
// (the tiles vd_gram_kernel writes); a thread owns one float4 of the tile and adds the slices in four interleaved chains
// (slices k, k + 4, ..), then (s0 + s1) + (s2 + s3): a fixed order.  The tile goes through LDS so that the mirrored tile
// is written along its rows too; a diagonal tile takes its lower half from its upper half.
__global__ __launch_bounds__(256) void vd_gram_reduce_kernel(const float* __restrict__ slab, int slices, int F, int Tt,
                                                             float* __restrict__ G) {
  __shared__ float tile[32][33];
  const int tid = threadIdx.x, row = tid >> 3, c4 = tid & 7;
  int ti = 0, rem = blockIdx.x;  // blockIdx.x counts the tiles on or above the diagonal row by row
  while (rem >= Tt - ti) rem -= Tt - ti, ++ti;
  const int tj = ti + rem;
  const size_t count = (size_t)F * F;
  const int a = ti * 32 + row, b = tj * 32 + 4 * c4;
  const bool in = a < F && b < F;  // F is a multiple of 4: a float4 is inside or outside as a whole
  float4 s[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) s[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (in) {
    const float* p = slab + (size_t)a * F + b;
    int k = 0;
    for (; k + 4 <= slices; k += 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(p + (size_t)(k + j) * count);
        s[j].x += v.x, s[j].y += v.y, s[j].z += v.z, s[j].w += v.w;
      }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (k + j < slices) {
        const float4 v = *reinterpret_cast<const float4*>(p + (size_t)(k + j) * count);
        s[j].x += v.x, s[j].y += v.y, s[j].z += v.z, s[j].w += v.w;
      }
  }
  const float4 v = make_float4((s[0].x + s[1].x) + (s[2].x + s[3].x), (s[0].y + s[1].y) + (s[2].y + s[3].y),
                               (s[0].z + s[1].z) + (s[2].z + s[3].z), (s[0].w + s[1].w) + (s[2].w + s[3].w));
  tile[row][4 * c4] = v.x, tile[row][4 * c4 + 1] = v.y, tile[row][4 * c4 + 2] = v.z, tile[row][4 * c4 + 3] = v.w;
  __syncthreads();
  // element (x, y) of the symmetric tile: from the upper half
  auto sym = [&](int x, int y) { return x <= y ? tile[x][y] : tile[y][x]; };
  if (ti == tj) {
    if (in)
      *reinterpret_cast<float4*>(G + (size_t)a * F + b) =
          make_float4(sym(row, 4 * c4), sym(row, 4 * c4 + 1), sym(row, 4 * c4 + 2), sym(row, 4 * c4 + 3));
    return;
  }
  if (in) *reinterpret_cast<float4*>(G + (size_t)a * F + b) = v;
  const int ma = tj * 32 + row, mb = ti * 32 + 4 * c4;  // the mirrored tile: G[ma][mb + j] = tile[4 c4 + j][row]
  if (ma < F && mb < F)
    *reinterpret_cast<float4*>(G + (size_t)ma * F + mb) =
        make_float4(tile[4 * c4][row], tile[4 * c4 + 1][row], tile[4 * c4 + 2][row], tile[4 * c4 + 3][row]);
}

static int vd_nv(int F) { return F <= 256 ? 1 : F <= 512 ? 2 : F <= 1024 ? 4 : 8; }

#define VD_FOR_NV(F, CALL) \
  switch (vd_nv(F)) {      \
    case 1: CALL(1); break; \
    case 2: CALL(2); break; \
    case 4: CALL(4); break; \
    default: CALL(8); break; \
  }

}  // namespace hipac

using namespace hipac;

extern "C" {

int hipac_validate_abi_version(void) { return HIPAC_VALIDATE_ABI_VERSION; }

size_t hipac_validate_colsum_workspace_bytes(int n, int F) {
  if (!vd_sizes_ok(n, F)) return 0;
  int chunk, slices;
  vd_sweep_slices(n, &chunk, &slices);
  return align256((size_t)slices * F * 4);
}

int hipac_validate_gram_slices(int n, int F) {
  if (!vd_sizes_ok(n, F)) return 0;
  int chunk, slices;
  vd_gram_slices(n, F, &chunk, &slices);
  return slices;
}

size_t hipac_validate_gram_workspace_bytes(int n, int F) {
  if (!vd_sizes_ok(n, F)) return 0;
  int chunk, slices;
  vd_gram_slices(n, F, &chunk, &slices);
  return align256((size_t)slices * F * F * 4);
}

size_t hipac_validate_logistic_workspace_bytes(int n, int F) {
  if (!vd_sizes_ok(n, F)) return 0;
  int chunk, slices;
  vd_sweep_slices(n, &chunk, &slices);
  return align256((size_t)slices * (2 * F + 4) * 4);
}

size_t hipac_validate_project_workspace_bytes(int n, int F, int K) {
  if (!vd_sizes_ok(n, F) || K < 1 || K > kVdMaxK) return 0;
  int chunk, slices;
  vd_sweep_slices(n, &chunk, &slices);
  return align256((size_t)slices * kVdProjStride * 4);
}

#define VD_COMMON_CHECKS(name, need)                                                                                          \
  HIPAC_REQUIRE(vd_sizes_ok(n, F), HIPAC_EINVAL, name ": n %d, F %d (1 <= n <= 2^24, F a multiple of 4 in 4..2048)", n, F);    \
  HIPAC_REQUIRE(n_feat_rows > 0 && (rows || n <= n_feat_rows), HIPAC_EINVAL, name ": n_feat_rows %d for n %d rows", n_feat_rows, \
                n);                                                                                                           \
  HIPAC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)workspace & 15) == 0, HIPAC_EINVAL,                                   \
                name ": X / workspace must be 16-byte aligned");                                                              \
  HIPAC_REQUIRE(workspace_bytes >= (need), HIPAC_EWORKSPACE, name ": workspace %zu bytes, %zu needed", workspace_bytes, (size_t)(need))

int hipac_validate_colsum(const float* X, int n_feat_rows, const int32_t* rows, int n, int F, const float* w, float* out,
                          void* workspace, size_t workspace_bytes, void* stream) {
  HIPAC_REQUIRE(X && out && workspace, HIPAC_EINVAL, "validate_colsum: null argument");
  VD_COMMON_CHECKS("validate_colsum", hipac_validate_colsum_workspace_bytes(n, F));
  int chunk, slices;
  vd_sweep_slices(n, &chunk, &slices);
  hipStream_t s = (hipStream_t)stream;
  float* slab = (float*)workspace;
#define VD_COLSUM(NV) hipLaunchKernelGGL(vd_colsum_kernel<NV>, dim3(slices), dim3(256), 0, s, X, rows, n, F, chunk, w, slab)
  VD_FOR_NV(F, VD_COLSUM)
#undef VD_COLSUM
  mil_train_launch_slab_reduce(slab, slices, (size_t)F, 0, F, out, 0, s);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int hipac_validate_gram(const float* X, int n_feat_rows, const int32_t* rows, int n, int F, const float* w, const float* c,
                        float* G, void* workspace, size_t workspace_bytes, void* stream) {
  HIPAC_REQUIRE(X && G && workspace, HIPAC_EINVAL, "validate_gram: null argument");
  VD_COMMON_CHECKS("validate_gram", hipac_validate_gram_workspace_bytes(n, F));
  HIPAC_REQUIRE(((uintptr_t)c & 15) == 0, HIPAC_EINVAL, "validate_gram: c must be 16-byte aligned");
  int chunk, slices;
  vd_gram_slices(n, F, &chunk, &slices);
  hipStream_t s = (hipStream_t)stream;
  float* slab = (float*)workspace;
  const int T = (F + 127) / 128;
  hipLaunchKernelGGL(vd_gram_kernel, dim3(vd_gram_blocks(F), slices), dim3(256), 0, s, X, rows, n, F, chunk, w, c, T, slab);
  const int Tt = (F + 31) / 32;
  hipLaunchKernelGGL(vd_gram_reduce_kernel, dim3(Tt * (Tt + 1) / 2), dim3(256), 0, s, (const float*)slab, slices, F, Tt, G);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int hipac_validate_logistic_sweep(const float* X, int n_feat_rows, const int32_t* rows, int n, int F, const float* coef,
                                  const float* intercept, const int64_t* labels, const float* class_w, float* sums, float* d,
                                  float* margins, void* workspace, size_t workspace_bytes, void* stream) {
  HIPAC_REQUIRE(X && coef && intercept && labels && class_w && sums && d && workspace, HIPAC_EINVAL,
                "validate_logistic_sweep: null argument");
  VD_COMMON_CHECKS("validate_logistic_sweep", hipac_validate_logistic_workspace_bytes(n, F));
  HIPAC_REQUIRE(((uintptr_t)coef & 15) == 0, HIPAC_EINVAL, "validate_logistic_sweep: coef must be 16-byte aligned");
  int chunk, slices;
  vd_sweep_slices(n, &chunk, &slices);
  hipStream_t s = (hipStream_t)stream;
  float* slab = (float*)workspace;
#define VD_SWEEP(NV)                                                                                                        \
  hipLaunchKernelGGL(vd_sweep_kernel<NV>, dim3(slices), dim3(256), 0, s, X, rows, n, F, chunk, coef, intercept, labels, class_w, d, \
                     margins, slab)
  VD_FOR_NV(F, VD_SWEEP)
#undef VD_SWEEP
  mil_train_launch_slab_reduce(slab, slices, (size_t)(2 * F + 4), 0, 2 * F + 3, sums, 0, s);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int hipac_validate_project(const float* X, int n_feat_rows, const int32_t* rows, int n, int F, const float* c, const float* W,
                           int K, const int64_t* labels, float* Z, float* class_sums, float* class_counts, void* workspace,
                           size_t workspace_bytes, void* stream) {
  HIPAC_REQUIRE(X && W && Z && workspace, HIPAC_EINVAL, "validate_project: null argument");
  HIPAC_REQUIRE(K >= 1 && K <= kVdMaxK, HIPAC_EINVAL, "validate_project: K %d (1..%d)", K, kVdMaxK);
  HIPAC_REQUIRE(!labels || (class_sums && class_counts), HIPAC_EINVAL, "validate_project: null class_sums / class_counts with labels");
  VD_COMMON_CHECKS("validate_project", hipac_validate_project_workspace_bytes(n, F, K));
  HIPAC_REQUIRE(((uintptr_t)c & 15) == 0 && ((uintptr_t)W & 15) == 0, HIPAC_EINVAL, "validate_project: c / W must be 16-byte aligned");
  int chunk, slices;
  vd_sweep_slices(n, &chunk, &slices);
  hipStream_t s = (hipStream_t)stream;
  float* slab = (float*)workspace;
#define VD_PROJECT(NV) \
  hipLaunchKernelGGL(vd_project_kernel<NV>, dim3(slices), dim3(256), 0, s, X, rows, n, F, chunk, c, W, K, labels, Z, slab)
  VD_FOR_NV(F, VD_PROJECT)
#undef VD_PROJECT
  if (labels) {
    // class sums [2][K] out of the slab's [2][4], then the two counts
    mil_train_launch_slab_reduce(slab, slices, (size_t)kVdProjStride, 0, K, class_sums, 0, s);
    mil_train_launch_slab_reduce(slab, slices, (size_t)kVdProjStride, kVdMaxK, K, class_sums + K, 0, s);
    mil_train_launch_slab_reduce(slab, slices, (size_t)kVdProjStride, 2 * kVdMaxK, 2, class_counts, 0, s);
  }
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"

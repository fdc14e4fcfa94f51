// Gated attention pooling for the MIL head (include/hipac_mil_gated.h; Ilse et al. 2018, eq. 9): a learned sigmoid gate
// over the hidden units of the attention, K heads, inference and the training step, fp32.
//
//   T = tanh(X V^T + b_V) [n][A]   G = sigmoid(X G_w^T + b_G) [n][A]   S = (T o G) U^T + b_U [n][K]
//   a[:, k] = softmax of S[:, k] inside each bag   M[b][k] = sum_i a[i][k] x_i   logits = classifier(M[b][0] | .. | M[b][K-1])
//   backward (g[b][k] = dL/dM[b][k]):  ds[i][k] = a[i][k] (x_i . g[b][k] - M[b][k] . g[b][k]),  e_i = sum_k ds[i][k] U[k],
//   dT_i = e_i o G_i o (1 - T_i^2) in place over T,  dG_i = e_i o T_i o G_i o (1 - G_i) in place over G,
//   dV = dT^T X, db_V = sum dT_i, dG_w = dG^T X, db_G = sum dG_i, dU[k] = sum ds[i][k] (T_i o G_i), db_U[k] = sum ds[i][k].
//
// The gate doubles the two MFMA products but not the sweeps over X: mg_h_kernel stages every X tile into LDS once and feeds
// it to both X V^T and X G_w^T, mg_dv_kernel stages every X tile once for both dT^T X and dG^T X.  A step sweeps X four
// times whatever K is (hidden layer, pooling, row sweep, weight gradients), as the ungated steps do.  T o G is not kept:
// the score kernel and the row sweep form it at the read (two planes of [n][A_pad] floats, not three).
// Pad columns A .. A_pad-1 of BOTH planes are written 0 (not sigmoid(0) = 0.5), so T o G, dT and dG are exactly 0 there.
//
// The tiling and the segment scheme are mil_train.hip's: 64 rows per tile whatever the bag boundaries, segment (tile t,
// bag b) = id t + b, partial slabs added in a fixed order; no float atomics.  What does not depend on the gate comes
// through mil_train_internal.h (row -> bag map, mil_heads.hip's pooling partials, pool combine, M . g, slab sums, and the
// host side: the workspace plan with two hidden planes, the argument checks, the classifier chain) and mil_device.h (the
// score weights' load and the part2 write-out, shared with mil_heads.hip's kernels); the per-head softmax
// has the form of mil_heads.hip's kernel but divides by the sum (see mg_softmax_kernel).  Here: the kernels whose
// arithmetic has the gate in it, the forward up to the pooled vectors and the two entry points.
#include "common.h"

#include "../../include/hipac_mil_gated.h"
#include "mil_device.h"
#include "mil_train_internal.h"
#include "wave_reduce.h"

namespace hipac {

constexpr int kMgTile = 64;  // rows per tile: mil_train.hip's kMtTile (mil_train_launch_pool_combine assumes it)
constexpr int kMgMaxHeads = 8;

static bool mil_gated_dims_ok(const hipac_mil_gated_params_t* p, int heads, int n, int n_bags) {
  return p && heads >= 1 && heads <= kMgMaxHeads && mil_train_sizes_ok(&p->base, n, n_bags);
}

// T[m][j] = tanh(x_m . V[j] + b_V[j]) and G[m][j] = sigmoid(x_m . G_w[j] + b_G[j]) on v_mfma_f32_32x32x2_f32, in the form of
// mt_h_kernel: 64 rows x 64 hidden units per workgroup (4 waves = 2 x 2 tiles of 32 x 32), K stepped by 32 through LDS, the
// next K tile fetched behind the MFMAs.  The X tile is staged once and every A fragment read from LDS feeds the V and the G
// MFMA.  Columns A .. A_pad-1 of both planes are written 0.
__global__ __launch_bounds__(256) void mg_h_kernel(const float* __restrict__ feats, const int32_t* __restrict__ rows, int n, int F,
                                                   const float* __restrict__ Vw, const float* __restrict__ Vb,
                                                   const float* __restrict__ Gw, const float* __restrict__ Gb, int A, int A_pad,
                                                   float* __restrict__ T, float* __restrict__ G) {
  constexpr int LDP = 33;
  __shared__ float As[64 * LDP], Bv[64 * LDP], Bg[64 * LDP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int wi = wave & 1, wj = wave >> 1;
  const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
  f32x16 accV, accG;
#pragma unroll
  for (int e = 0; e < 16; ++e) accV[e] = 0.f, accG[e] = 0.f;
  const int kk_t = tid & 31, row0 = tid >> 5;
  const float* xa[8];
  size_t wo[8];
  bool wok[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int m = m0 + row0 + 8 * j, c = n0 + row0 + 8 * j;
    xa[j] = m < n ? feats + (size_t)(rows ? rows[m] : m) * F : nullptr;
    wok[j] = c < A;
    wo[j] = wok[j] ? (size_t)c * F : 0;
  }
  float ra[8], rv[8], rg[8];
  auto fetch = [&](int k0) {
    const int k = k0 + kk_t;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ra[j] = (xa[j] && k < F) ? xa[j][k] : 0.f;
      rv[j] = (wok[j] && k < F) ? Vw[wo[j] + k] : 0.f;
      rg[j] = (wok[j] && k < F) ? Gw[wo[j] + k] : 0.f;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < F; k0 += 32) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int at = (row0 + 8 * j) * LDP + kk_t;
      As[at] = ra[j], Bv[at] = rv[j], Bg[at] = rg[j];
    }
    __syncthreads();
    if (k0 + 32 < F) fetch(k0 + 32);
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const float a = As[(wi * 32 + r) * LDP + 2 * kk + h];
      accV = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bv[(wj * 32 + r) * LDP + 2 * kk + h], accV, 0, 0, 0);
      accG = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bg[(wj * 32 + r) * LDP + 2 * kk + h], accG, 0, 0, 0);
    }
  }
  // D[m][c]: column c = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h
  const int c = n0 + wj * 32 + r;
  if (c >= A_pad) return;
  const bool real = c < A;
  const float bv = real ? Vb[c] : 0.f, bg = real ? Gb[c] : 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int m = m0 + wi * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
    if (m < n) {
      T[(size_t)m * A_pad + c] = real ? tanhf(accV[e] + bv) : 0.f;
      G[(size_t)m * A_pad + c] = real ? 1.f / (1.f + expf(-(accG[e] + bg))) : 0.f;
    }
  }
}

// S[i][k] = U[k] . (T_i o G_i) + b_U[k]: mh_score_kernel's form (one wave per row, 16 rows per workgroup, the row read once for
// the K heads) with the gate applied at the read
template <int K>
__global__ __launch_bounds__(256) void mg_score_kernel(const float* __restrict__ T, const float* __restrict__ G, int n, int A,
                                                       int A_pad, const float* __restrict__ Uw, const float* __restrict__ Ub,
                                                       float* __restrict__ scores) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float u[K][4];
  mil_load_u<K>(Uw, A, lane, u);
  for (int rr = wave; rr < 16; rr += 4) {
    const int i = blockIdx.x * 16 + rr;
    if (i >= n) break;
    float h[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const size_t at = (size_t)i * A_pad + lane + 64 * q;
      h[q] = lane + 64 * q < A ? T[at] * G[at] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float v = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) v = fmaf(u[k][q], h[q], v);
      v = wave_sum(v);
      if (lane == 0) scores[(size_t)i * K + k] = v + Ub[k];
    }
  }
}

// softmax of column k of the scores inside bag b: one workgroup per (bag, head) (mh_softmax_kernel's form).  The weight is
// exp(s - m) / z, one correctly rounded division, not a product with a rounded 1 / z: the reciprocal costs a rounding that left
// a weight of a two-row bag more than an ulp from its value (3.3e-8 against 4e-9 on the test's bags)
__global__ __launch_bounds__(256) void mg_softmax_kernel(const float* __restrict__ scores, const int32_t* __restrict__ offs, int K,
                                                         float* __restrict__ attn) {
  __shared__ float red[4];
  const int b = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  const int o0 = offs[b], o1 = offs[b + 1];
  float mx = -INFINITY;
  for (int i = o0 + tid; i < o1; i += 256) mx = fmaxf(mx, scores[(size_t)i * K + k]);
  const float m = block_max_tree<4>(mx, red);
  float z = 0.f;
  for (int i = o0 + tid; i < o1; i += 256) z += expf(scores[(size_t)i * K + k] - m);
  const float zs = block_sum_tree<4>(z, red);
  for (int i = o0 + tid; i < o1; i += 256) attn[(size_t)i * K + k] = expf(scores[(size_t)i * K + k] - m) / zs;
}

// one sweep over the rows of a tile: mh_ds_kernel's sweep with the gated epilogue.  A wave takes rows wave, wave + 4, ...;
// it reads x_i once and forms the K products x_i . g[b][k], then ds[i][k] = a[i][k] (x_i . g[b][k] - cdot[b][k]) and
// e_i = sum_k ds[i][k] U[k]; T_i becomes dT_i = e_i G_i (1 - T_i^2) and G_i becomes dG_i = e_i T_i G_i (1 - G_i), in place;
// the tile's column sums go to part2[tile] = (sum dT_i [A_pad] | sum dG_i [A_pad] | sum ds[i][k] T_i G_i [K][A] | sum ds[i][k] [K])
template <int K>
__global__ __launch_bounds__(256) void mg_ds_kernel(const float* __restrict__ feats, const int32_t* __restrict__ rows,
                                                    const int32_t* __restrict__ bag_of, const float* __restrict__ attn,
                                                    const float* __restrict__ g, const float* __restrict__ cdot,
                                                    const float* __restrict__ Uw, float* __restrict__ T, float* __restrict__ G, int n,
                                                    int F, int A, int A_pad, float* __restrict__ part2) {
  constexpr int RED = 256 * (K + 2) + K;
  __shared__ float red[4][RED];
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float accT[4] = {0.f, 0.f, 0.f, 0.f}, accG[4] = {0.f, 0.f, 0.f, 0.f}, accU[K][4], accB[K], u[K][4];
  mil_load_u<K>(Uw, A, lane, u);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    accB[k] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) accU[k][q] = 0.f;
  }
  const int F4 = F / 4;
  for (int rr = wave; rr < kMgTile; rr += 4) {
    const int i = tile * kMgTile + rr;
    if (i >= n) break;
    const int b = bag_of[i];
    const f32x4* x = reinterpret_cast<const f32x4*>(feats + (size_t)(rows ? rows[i] : i) * F);
    const f32x4* gb = reinterpret_cast<const f32x4*>(g + (size_t)b * K * F);
    // the K dot products: the same loop as in mil_heads.hip's mh_ds_kernel (as a function of mil_device.h it moved mh_ds_kernel's
    // register counts, so it is written out in both)
    float t[K], ds[K];
#pragma unroll
    for (int k = 0; k < K; ++k) t[k] = 0.f;
    for (int c = lane; c < F4; c += 64) {
      const f32x4 xv = x[c];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const f32x4 gv = gb[k * F4 + c];
        t[k] = fmaf(xv[0], gv[0], t[k]), t[k] = fmaf(xv[1], gv[1], t[k]), t[k] = fmaf(xv[2], gv[2], t[k]);
        t[k] = fmaf(xv[3], gv[3], t[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      ds[k] = attn[(size_t)i * K + k] * (wave_sum(t[k]) - cdot[b * K + k]);
      accB[k] += ds[k];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = lane + 64 * q;
      if (j < A_pad) {
        float* tp = T + (size_t)i * A_pad + j;
        float* gp = G + (size_t)i * A_pad + j;
        const float tv = j < A ? *tp : 0.f, gv = j < A ? *gp : 0.f;
        float e = ds[0] * u[0][q];
#pragma unroll
        for (int k = 1; k < K; ++k) e = fmaf(ds[k], u[k][q], e);
        const float dt = e * gv * (1.f - tv * tv);
        const float dg = e * tv * gv * (1.f - gv);
        *tp = dt, *gp = dg;
        accT[q] += dt, accG[q] += dg;
        const float hg = tv * gv;
#pragma unroll
        for (int k = 0; k < K; ++k) accU[k][q] = fmaf(ds[k], hg, accU[k][q]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    red[wave][64 * q + lane] = accT[q], red[wave][256 + 64 * q + lane] = accG[q];
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave][256 * (k + 2) + 64 * q + lane] = accU[k][q];
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave][256 * (K + 2) + k] = accB[k];
  }
  __syncthreads();
  mil_store_part2<K, 2>(red, A, A_pad, tid, part2 + (size_t)tile * (2 * (size_t)A_pad + (size_t)K * A + K));
}

// dV and dG_w partials in one sweep of X, in the form of mt_dv_kernel: slab[slice][0][a][f] = sum over the slice's rows of
// dT[m][a] X[rows[m]][f], slab[slice][1][a][f] the same with dG, on v_mfma_f32_32x32x2_f32.  One workgroup = 64 feature columns
// x up to 64 TP hidden units of BOTH products x one slice of rows; the rows are the MFMA's k.  X is staged 32 rows at a time
// into LDS once, and every X fragment read from LDS feeds the dT and the dG MFMAs.  TP = row tiles of 32 hidden units per wave
// and product.  Up to A_pad = 192 (TP <= 3) one workgroup column holds all hidden units and the kernel reads every feature
// element once.  A_pad = 224 / 256 would take TP = 4 -- 8 accumulator tiles and their 8 second-level sums per wave, 512
// registers and a spill -- so there the hidden units are split over two workgroup columns (blockIdx.z) of TP = 2 and X is read
// twice by this kernel, at that size only.
template <int TP>
__global__ __launch_bounds__(256) void mg_dv_kernel(const float* __restrict__ dT, const float* __restrict__ dG,
                                                    const float* __restrict__ feats, const int32_t* __restrict__ rows, int n, int F,
                                                    int A, int A_pad, int chunk, float* __restrict__ slab) {
  constexpr int LDB = 68;                // 64 floats + 4: keeps float4 stores aligned, spreads banks
  constexpr int LDA_MAX = TP * 64 + 4;  // A_pad <= 64 TP
  __shared__ __attribute__((aligned(16))) float At[32 * LDA_MAX], Ag[32 * LDA_MAX], Bs[32 * LDB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int cj = wave & 1, a0 = wave >> 1;  // column half; row tiles a0, a0 + 2, .. of this workgroup's hidden units
  const int tbase = blockIdx.z * 2 * TP;    // this workgroup's first row tile; it holds nAt <= 2 TP of them
  const int nAt = A_pad / 32 - tbase < 2 * TP ? A_pad / 32 - tbase : 2 * TP, A4 = nAt * 8;
  const int LDA = nAt * 32 + 4;
  const int f0 = blockIdx.x * 64;
  const int m_begin = blockIdx.y * chunk;
  const int m_end = m_begin + chunk < n ? m_begin + chunk : n;
  // two levels of summation, as in mt_dv_kernel: the MFMA adds 128 rows into acc one after another, then acc is added to tot
  f32x16 accT[TP], accG[TP], totT[TP], totG[TP];
#pragma unroll
  for (int t = 0; t < TP; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) accT[t][e] = 0.f, accG[t][e] = 0.f, totT[t][e] = 0.f, totG[t][e] = 0.f;
  int sub = 0;
  const int spx = tid >> 3, sc = tid & 7;  // staging of X: row of the sub-chunk, float4 column (and + 8)
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int m0 = m_begin; m0 < m_end; m0 += 32) {
    float4 b0 = zero4, b1 = zero4;
    if (m0 + spx < m_end) {
      const int m = m0 + spx;
      const float* bp = feats + (size_t)(rows ? rows[m] : m) * F + f0 + 4 * sc;
      if (f0 + 4 * sc < F) b0 = *reinterpret_cast<const float4*>(bp);
      if (f0 + 32 + 4 * sc < F) b1 = *reinterpret_cast<const float4*>(bp + 32);
    }
    float4 at[2 * TP], ag[2 * TP];
#pragma unroll
    for (int it = 0; it < 2 * TP; ++it) {
      at[it] = zero4, ag[it] = zero4;
      if (it < nAt) {
        const int idx = tid + 256 * it, row = idx / A4, c4 = idx - row * A4;
        if (m0 + row < m_end) {
          at[it] = *reinterpret_cast<const float4*>(dT + (size_t)(m0 + row) * A_pad + tbase * 32 + 4 * c4);
          ag[it] = *reinterpret_cast<const float4*>(dG + (size_t)(m0 + row) * A_pad + tbase * 32 + 4 * c4);
        }
      }
    }
    __syncthreads();  // the previous sub-chunk's fragments have been read
    *reinterpret_cast<float4*>(Bs + spx * LDB + 4 * sc) = b0;
    *reinterpret_cast<float4*>(Bs + spx * LDB + 32 + 4 * sc) = b1;
#pragma unroll
    for (int it = 0; it < 2 * TP; ++it)
      if (it < nAt) {
        const int idx = tid + 256 * it, row = idx / A4, c4 = idx - row * A4;
        *reinterpret_cast<float4*>(At + row * LDA + 4 * c4) = at[it];
        *reinterpret_cast<float4*>(Ag + row * LDA + 4 * c4) = ag[it];
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int px = 2 * k + h;
      const float bv = Bs[px * LDB + cj * 32 + r];
#pragma unroll
      for (int t = 0; t < TP; ++t)
        if (a0 + 2 * t < nAt) {
          accT[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(At[px * LDA + (a0 + 2 * t) * 32 + r], bv, accT[t], 0, 0, 0);
          accG[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ag[px * LDA + (a0 + 2 * t) * 32 + r], bv, accG[t], 0, 0, 0);
        }
    }
    if (++sub == 4 || m0 + 32 >= m_end) {
      sub = 0;
#pragma unroll
      for (int t = 0; t < TP; ++t) {
        totT[t] += accT[t], totG[t] += accG[t];
#pragma unroll
        for (int e = 0; e < 16; ++e) accT[t][e] = 0.f, accG[t][e] = 0.f;
      }
    }
  }
  // D[a][f]: column f = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h
  const int f = f0 + cj * 32 + r;
  float* baseT = slab + (size_t)blockIdx.y * 2 * A * F;
  float* baseG = baseT + (size_t)A * F;
#pragma unroll
  for (int t = 0; t < TP; ++t)
    if (a0 + 2 * t < nAt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int a = (tbase + a0 + 2 * t) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (a < A && f < F) baseT[(size_t)a * F + f] = totT[t][e], baseG[(size_t)a * F + f] = totG[t][e];
      }
    }
}

// the forward up to the pooled vectors, shared by inference and the step: bag_of, T, G, a [n][K], pooled [n_bags][K F]
static void mil_gated_pool(const hipac_mil_gated_params_t* gp, int K, const float* feats, const int32_t* rows,
                           const int32_t* bag_offsets, int n, int n_bags, const MilHeadPlan& q, char* ws, float* a, float* pooled,
                           hipStream_t s) {
  const hipac_mil_params_t* p = &gp->base;
  const int F = p->feature_dim, A = p->attn_dim;
  int32_t* bag_of = (int32_t*)(ws + q.bag_of);
  float* T = (float*)(ws + q.H);
  float* G = (float*)(ws + q.G);
  float* scores = (float*)(ws + q.scores);
  float* part = (float*)(ws + q.part);
  mil_train_launch_bag_of(bag_offsets, n_bags, n, bag_of, s);
  hipLaunchKernelGGL(mg_h_kernel, dim3(q.ntiles, (A + 63) / 64), dim3(256), 0, s, feats, rows, n, F, p->attn_V_w, p->attn_V_b,
                     gp->attn_G_w, gp->attn_G_b, A, q.A_pad, T, G);
  mil_for_count<kMgMaxHeads>(K, [&](auto kk) {
    hipLaunchKernelGGL(mg_score_kernel<decltype(kk)::value>, dim3((n + 15) / 16), dim3(256), 0, s, (const float*)T, (const float*)G, n,
                       A, q.A_pad, p->attn_U_w, p->attn_U_b, scores);
  });
  hipLaunchKernelGGL(mg_softmax_kernel, dim3(n_bags, K), dim3(256), 0, s, (const float*)scores, bag_offsets, K, a);
  mil_heads_launch_pool(feats, rows, bag_of, a, n, F, K, q.ntiles, part, s);
  mil_train_launch_pool_combine(part, bag_offsets, n_bags, K * F, pooled, s);
}

static void mil_gated_launch_dv(const float* dT, const float* dG, const float* feats, const int32_t* rows, int n, int F, int A,
                                int A_pad, int chunk, int slices, float* slab, hipStream_t s) {
#define MG_DV(TPW, COLS)                                                                                                       \
  hipLaunchKernelGGL(mg_dv_kernel<TPW>, dim3((F + 63) / 64, slices, COLS), dim3(256), 0, s, dT, dG, feats, rows, n, F, A, A_pad, \
                     chunk, slab)
  switch ((A_pad / 32 + 1) / 2) {  // row tiles per wave and product
    case 1: MG_DV(1, 1); break;
    case 2: MG_DV(2, 1); break;
    case 3: MG_DV(3, 1); break;
    default: MG_DV(2, 2); break;  // A_pad = 224, 256: two workgroup columns of 128 hidden units (and 96 or 128)
  }
#undef MG_DV
}

}  // namespace hipac

using namespace hipac;

extern "C" {

int hipac_mil_gated_abi_version(void) { return HIPAC_MIL_GATED_ABI_VERSION; }

size_t hipac_mil_gated_forward_workspace_bytes(const hipac_mil_gated_params_t* params, int heads, int n, int n_bags) {
  return mil_gated_dims_ok(params, heads, n, n_bags) ? make_mil_head_plan(&params->base, heads, n, n_bags, 2, heads, false).total : 0;
}

size_t hipac_mil_gated_train_workspace_bytes(const hipac_mil_gated_params_t* params, int heads, int n, int n_bags) {
  return mil_gated_dims_ok(params, heads, n, n_bags) ? make_mil_head_plan(&params->base, heads, n, n_bags, 2, heads, true).total : 0;
}

int hipac_mil_gated_forward(const hipac_mil_gated_params_t* gp, int heads, const float* feats, const int32_t* bag_offsets, int n,
                            int n_bags, float* logits, float* attn, float* pooled, void* workspace, size_t workspace_bytes,
                            void* stream) {
  const hipac_mil_params_t* p = gp ? &gp->base : nullptr;
  const int rc = mil_check_forward_args("mil_gated_forward", gp && feats && bag_offsets && logits && workspace, "heads", heads,
                                        kMgMaxHeads, p, gp && gp->attn_G_w && gp->attn_G_b, n, n_bags, feats, workspace);
  if (rc) return rc;
  const MilHeadPlan q = make_mil_head_plan(p, heads, n, n_bags, 2, heads, false);
  HIPAC_REQUIRE(workspace_bytes >= q.total, HIPAC_EWORKSPACE, "mil_gated_forward: workspace %zu bytes, %zu needed", workspace_bytes,
                q.total);
  char* ws = (char*)workspace;
  float* a = attn ? attn : (float*)(ws + q.attn);
  float* pl = pooled ? pooled : (float*)(ws + q.pooled);
  mil_gated_pool(gp, heads, feats, nullptr, bag_offsets, n, n_bags, q, ws, a, pl, (hipStream_t)stream);
  HIPAC_CHECK_HIP(hipGetLastError());
  return mil_classifier_forward(p, pl, heads * p->feature_dim, n_bags, (float*)(ws + q.hid), logits, stream);
}

int hipac_mil_gated_train_fwd_bwd(const hipac_mil_gated_params_t* gp, int heads, const float* feats, int n_feat_rows,
                                  const int32_t* rows, const int32_t* bag_offsets, int n, int n_bags, const int64_t* labels,
                                  const float* class_w, const hipac_mil_gated_params_t* ggrads, float* loss, float* logits,
                                  float* attn, void* workspace, size_t workspace_bytes, int accumulate, void* stream) {
  const bool ptrs = gp && feats && bag_offsets && labels && ggrads && loss && logits && workspace;
  const hipac_mil_params_t* p = ptrs ? &gp->base : nullptr;
  const hipac_mil_params_t* grads = ptrs ? &ggrads->base : nullptr;
  int rc = mil_check_train_args("mil_gated_train_fwd_bwd", ptrs, "heads", heads, kMgMaxHeads, p, grads, true,
                                ptrs && gp->attn_G_w && gp->attn_G_b && ggrads->attn_G_w && ggrads->attn_G_b, n, n_bags, n_feat_rows,
                                rows != nullptr, feats, workspace);
  if (rc) return rc;
  const MilHeadPlan q = make_mil_head_plan(p, heads, n, n_bags, 2, heads, true);
  HIPAC_REQUIRE(workspace_bytes >= q.total, HIPAC_EWORKSPACE, "mil_gated_train_fwd_bwd: workspace %zu bytes, %zu needed",
                workspace_bytes, q.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int F = p->feature_dim, A = p->attn_dim, B = n_bags, K = heads;
  float* pooled = (float*)(ws + q.pooled);
  float* g = (float*)(ws + q.g);
  float* a = attn ? attn : (float*)(ws + q.attn);
  float* T = (float*)(ws + q.H);
  float* G = (float*)(ws + q.G);
  float* cdot = (float*)(ws + q.cdot);
  float* part2 = (float*)(ws + q.part2);
  float* slab = (float*)(ws + q.slab);

  mil_gated_pool(gp, K, feats, rows, bag_offsets, n, B, q, ws, a, pooled, s);
  HIPAC_CHECK_HIP(hipGetLastError());
  // classifier.0 over the K F pooled columns + ReLU, classifier.2, cross-entropy, and their backward
  rc = mil_classifier_fwd_bwd(p, grads, K * F, B, labels, class_w, loss, logits, q, ws, true, accumulate, stream, nullptr, nullptr);
  if (rc) return rc;
  // pooled and g are [B K][F]: cdot[b][k] = M[b][k] . g[b][k]
  mil_train_launch_cdot(pooled, g, F, B * K, cdot, s);
  mil_for_count<kMgMaxHeads>(K, [&](auto kk) {
    hipLaunchKernelGGL(mg_ds_kernel<decltype(kk)::value>, dim3(q.ntiles), dim3(256), 0, s, feats, rows, (const int32_t*)(ws + q.bag_of),
                       (const float*)a, (const float*)g, (const float*)cdot, p->attn_U_w, T, G, n, F, A, q.A_pad, part2);
  });
  // two hidden planes in part2 and two products per slice in slab: the end of the step is not mil_head_launch_grads'
  const size_t Ap = (size_t)q.A_pad;
  mil_train_launch_slab_reduce(part2, q.ntiles, q.P2, 0, A, (float*)grads->attn_V_b, accumulate, s);
  mil_train_launch_slab_reduce(part2, q.ntiles, q.P2, Ap, A, (float*)ggrads->attn_G_b, accumulate, s);
  mil_train_launch_slab_reduce(part2, q.ntiles, q.P2, 2 * Ap, (long long)K * A, (float*)grads->attn_U_w, accumulate, s);
  mil_train_launch_slab_reduce(part2, q.ntiles, q.P2, 2 * Ap + (size_t)K * A, K, (float*)grads->attn_U_b, accumulate, s);
  mil_gated_launch_dv(T, G, feats, rows, n, F, A, q.A_pad, q.chunk, q.slices, slab, s);
  const long long total = (long long)A * F;
  mil_train_launch_slab_reduce(slab, q.slices, 2 * (size_t)total, 0, total, (float*)grads->attn_V_w, accumulate, s);
  mil_train_launch_slab_reduce(slab, q.slices, 2 * (size_t)total, (size_t)total, total, (float*)ggrads->attn_G_w, accumulate, s);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"

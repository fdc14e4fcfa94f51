// MIL training step (include/hipac_mil_train.h): forward + backward of MILClassifier (src/models/mil_classifier.py:5-45)
// over a batch of ragged bags, fp32.  Feature rows are read in place through an int32 row index.
//
// Rows are tiled 64 at a time across the grid, whatever the bag boundaries.  A "segment" is the run of rows that
// one tile holds of one bag; because both the tile index and the bag index only grow along the rows, segment
// (tile t, bag b) has the id t + b, the segments of bag b are the ids tile(first row) + b .. tile(last row) + b, and
// there are at most ntiles + n_bags of them.  Per-bag sums (the pooled vector) are written per segment and added
// per bag in a fixed order; sums over all rows (dV, db_V, dU, db_U) are written per row slice and added in a fixed
// order.  No float atomics: the result depends on the tiling, never on the run.
//
// attention pooling, forward:  H = tanh(X V^T + b_V) (f32 MFMA, kept: A floats per row), s = H U + b_U,
//                              a = softmax of s inside each bag, pooled_b = sum a_i x_i
//            backward (g_b = dL/dpooled_b):  ds_i = a_i (x_i . g_b - pooled_b . g_b),  dH_i = ds_i U (1 - H_i^2) (in place
//                              over H),  dV = dH^T X (f32 MFMA, reduction over rows), db_V = sum dH_i, dU = sum ds_i H_i,
//                              db_U = sum ds_i.  Two sweeps over X: the row dot products, then dV (DESIGN.md 3.3b has the
//                              measurement against the form that keeps P = X W1^T from the forward and sweeps once).
//                              pooled_b . g_b is taken as sum_j a_j (x_j . g_b) / sum_j a_j from the kept row dot products
//                              (mt_rowdot_kernel, mt_bag_cdot_kernel), so that sum_i ds_i of a bag rounds to 0.
// mean / max pooling have no parameter in front of the classifier: the features are data, not parameters, so their
// backward ends at dL/dpooled.
// The classifier, the cross-entropy and Adam are hipac.h's hipac_linear_* / hipac_cross_entropy_fwd_bwd / hipac_adam_step.
// This file also defines what mil_train_internal.h declares for the K-head steps (mil_heads.hip, mil_gated.hip,
// mil_levels.hip): their workspace plan, argument checks, classifier chain and the launches that do not depend on K.
#include "common.h"

#include "../../include/hipac_mil_train.h"
#include "mil_train_internal.h"
#include "wave_reduce.h"

namespace hipac {

constexpr int kMtTile = 64;         // rows per tile (pooling, ds sweep)
constexpr int kMtMaxRows = 1 << 24;  // n * A_pad stays far inside size_t and the tile counts inside int

static bool mil_train_dims_ok(const hipac_mil_params_t* p, int pooling, int n, int n_bags) {
  if (!p || pooling < HIPAC_MIL_ATTENTION || pooling > HIPAC_MIL_MAX) return false;
  if (n <= 0 || n_bags <= 0 || n_bags > n || n > kMtMaxRows) return false;
  if (p->feature_dim < 4 || p->feature_dim % 4 != 0 || p->feature_dim > 2048) return false;
  if (p->hidden_dim < 1 || p->hidden_dim > 256 || p->num_classes < 1 || p->num_classes > 16) return false;
  if (pooling == HIPAC_MIL_ATTENTION && (p->attn_dim < 1 || p->attn_dim > 256)) return false;
  return true;
}

// the single-head step's layout of MilHeadPlan's buffers (no G; P2 = sum dH_i [A_pad] | sum ds_i H_i [A_pad] | sum ds_i)
static MilHeadPlan make_mil_train_plan(const hipac_mil_params_t* p, int pooling, int n, int n_bags) {
  MilHeadPlan q{};
  const size_t F = p->feature_dim, Hd = p->hidden_dim, Cn = p->num_classes, B = n_bags;
  const bool att = pooling == HIPAC_MIL_ATTENTION;
  q.A_pad = att ? (p->attn_dim + 31) / 32 * 32 : 0;
  q.ntiles = (n + kMtTile - 1) / kMtTile;
  q.nseg = q.ntiles + n_bags;
  mil_train_dv_slices(n, p->feature_dim, &q.chunk, &q.slices);
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align256(bytes);
    return at;
  };
  q.bag_of = take((size_t)n * 4);
  q.pooled = take(B * F * 4);
  q.hid = take(B * Hd * 4);
  q.dhid = take(B * Hd * 4);
  q.dym = take(B * Hd * 4);
  q.dlogits = take(B * Cn * 4);
  q.g = take(B * F * 4);
  q.ce = take((2 + 8 * ((B + 255) / 256)) * 4);
  q.cdot = take(B * 8);  // doubles here (mt_bag_cdot_kernel)
  q.part = take((size_t)q.nseg * F * 4);
  if (att) {
    q.scores = take((size_t)n * 4);
    q.attn = take((size_t)n * 4);
    q.H = take((size_t)n * q.A_pad * 4);
    q.P2 = 2 * (size_t)q.A_pad + 1;
    q.part2 = take((size_t)q.ntiles * q.P2 * 4);
    q.slab = take((size_t)q.slices * p->attn_dim * F * 4);
  }
  q.total = o;
  return q;
}

// bag_of[i] = the bag that holds batch row i (binary search in the offsets)
__global__ __launch_bounds__(256) void mt_bag_of_kernel(const int32_t* __restrict__ offs, int n_bags, int n,
                                                        int32_t* __restrict__ bag_of) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = n_bags - 1;  // offs[lo] <= i < offs[hi + 1]
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offs[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  bag_of[i] = lo;
}

// H[m][j] = tanh(sum_k X[rows[m]][k] V[j][k] + b_V[j]) on v_mfma_f32_32x32x2_f32: 64 rows x 64 hidden units per workgroup
// (4 waves = 2 x 2 tiles of 32 x 32), K stepped by 32 through LDS, the next K tile fetched behind the MFMAs
// (the form of train.hip's gemm_f32_kernel, with the row index on the A operand).  Columns A .. A_pad-1 are written 0.
__global__ __launch_bounds__(256) void mt_h_kernel(const float* __restrict__ feats, const int32_t* __restrict__ rows, int n, int F,
                                                   const float* __restrict__ Vw, const float* __restrict__ Vb, int A, int A_pad,
                                                   float* __restrict__ H) {
  constexpr int LDP = 33;
  __shared__ float As[64 * LDP], Bs[64 * LDP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int wi = wave & 1, wj = wave >> 1;
  const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const int kk_t = tid & 31, row0 = tid >> 5;
  const float* xa[8];
  const float* vb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int m = m0 + row0 + 8 * j, c = n0 + row0 + 8 * j;
    xa[j] = m < n ? feats + (size_t)(rows ? rows[m] : m) * F : nullptr;
    vb[j] = c < A ? Vw + (size_t)c * F : nullptr;
  }
  float ra[8], rb[8];
  auto fetch = [&](int k0) {
    const int k = k0 + kk_t;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ra[j] = (xa[j] && k < F) ? xa[j][k] : 0.f;
      rb[j] = (vb[j] && k < F) ? vb[j][k] : 0.f;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < F; k0 += 32) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) As[(row0 + 8 * j) * LDP + kk_t] = ra[j], Bs[(row0 + 8 * j) * LDP + kk_t] = rb[j];
    __syncthreads();
    if (k0 + 32 < F) fetch(k0 + 32);
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(wi * 32 + r) * LDP + 2 * kk + h], Bs[(wj * 32 + r) * LDP + 2 * kk + h],
                                                 acc, 0, 0, 0);
  }
  // D[m][c]: column c = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h
  const int c = n0 + wj * 32 + r;
  if (c >= A_pad) return;
  const float bias = c < A ? Vb[c] : 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int m = m0 + wi * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
    if (m < n) H[(size_t)m * A_pad + c] = c < A ? tanhf(acc[e] + bias) : 0.f;
  }
}

// s_i = U . H_i + b_U: one wave per row, 16 rows per workgroup
__global__ __launch_bounds__(256) void mt_score_kernel(const float* __restrict__ H, int n, int A, int A_pad,
                                                       const float* __restrict__ Uw, const float* __restrict__ Ub,
                                                       float* __restrict__ scores) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int rr = wave; rr < 16; rr += 4) {
    const int i = blockIdx.x * 16 + rr;
    if (i >= n) break;
    float v = 0.f;
    for (int j = lane; j < A; j += 64) v = fmaf(Uw[j], H[(size_t)i * A_pad + j], v);
    v = wave_sum(v);
    if (lane == 0) scores[i] = v + Ub[0];
  }
}

// softmax of the scores inside each bag.  4 bytes per row: the one per-bag pass of the step; everything that touches
// a feature row is tiled over the grid
__global__ __launch_bounds__(256) void mt_softmax_kernel(const float* __restrict__ scores, const int32_t* __restrict__ offs,
                                                         float* __restrict__ attn) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int o0 = offs[b], o1 = offs[b + 1];
  float mx = -INFINITY;
  for (int i = o0 + tid; i < o1; i += 256) mx = fmaxf(mx, scores[i]);
  const float m = block_max_tree<4>(mx, red);
  float z = 0.f;
  for (int i = o0 + tid; i < o1; i += 256) z += expf(scores[i] - m);
  const float inv = 1.f / block_sum_tree<4>(z, red);
  for (int i = o0 + tid; i < o1; i += 256) attn[i] = expf(scores[i] - m) * inv;
}

// pooling partials: tile t of 64 rows -> part[t + b][F] for every bag b it holds (sum of w_i x_i, sum of x_i, or max)
__global__ __launch_bounds__(256) void mt_pool_kernel(const float* __restrict__ feats, const int32_t* __restrict__ rows,
                                                      const int32_t* __restrict__ bag_of, const float* __restrict__ w, int n,
                                                      int F, int pooling, float* __restrict__ part) {
  __shared__ int sb[kMtTile];
  __shared__ int sro[kMtTile];
  __shared__ float sw[kMtTile];
  const int tile = blockIdx.x, tid = threadIdx.x;
  const int r0 = tile * kMtTile;
  const int cnt = n - r0 < kMtTile ? n - r0 : kMtTile;
  if (tid < cnt) {
    sb[tid] = bag_of[r0 + tid];
    sro[tid] = rows ? rows[r0 + tid] : r0 + tid;
    sw[tid] = w ? w[r0 + tid] : 1.f;
  }
  __syncthreads();
  const int F4 = F / 4;
  const f32x4* x4 = reinterpret_cast<const f32x4*>(feats);
  f32x4* p4 = reinterpret_cast<f32x4*>(part);
  const float init = pooling == HIPAC_MIL_MAX ? -INFINITY : 0.f;
  for (int c = tid; c < F4; c += 256) {
    f32x4 acc = {init, init, init, init};
    int cur = sb[0];
    for (int i = 0; i < cnt; ++i) {
      const int b = sb[i];
      if (b != cur) {
        p4[(size_t)(tile + cur) * F4 + c] = acc;
        acc = f32x4{init, init, init, init};
        cur = b;
      }
      const f32x4 x = x4[(size_t)sro[i] * F4 + c];
      if (pooling == HIPAC_MIL_MAX) {
        acc[0] = fmaxf(acc[0], x[0]), acc[1] = fmaxf(acc[1], x[1]), acc[2] = fmaxf(acc[2], x[2]), acc[3] = fmaxf(acc[3], x[3]);
      } else if (pooling == HIPAC_MIL_MEAN) {
        acc += x;
      } else {
        const float a = sw[i];
        acc[0] = fmaf(a, x[0], acc[0]), acc[1] = fmaf(a, x[1], acc[1]), acc[2] = fmaf(a, x[2], acc[2]), acc[3] = fmaf(a, x[3], acc[3]);
      }
    }
    p4[(size_t)(tile + cur) * F4 + c] = acc;
  }
}

// pooled[b][f] = the segments of bag b combined: 32 columns x 8 groups per workgroup, group g takes segments g, g + 8, ...
// in turn, then the 8 group results are combined in order
__global__ __launch_bounds__(256) void mt_pool_combine_kernel(const float* __restrict__ part, const int32_t* __restrict__ offs, int F,
                                                              int pooling, float* __restrict__ pooled) {
  __shared__ float red[8][32];
  const int b = blockIdx.x, e = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int f = blockIdx.y * 32 + e;
  const int o0 = offs[b], o1 = offs[b + 1];
  const int s0 = o0 / kMtTile + b, s1 = (o1 - 1) / kMtTile + b;
  const bool is_max = pooling == HIPAC_MIL_MAX;
  float v = is_max ? -INFINITY : 0.f;
  if (f < F)
    for (int k = s0 + g; k <= s1; k += 8) {
      const float t = part[(size_t)k * F + f];
      v = is_max ? fmaxf(v, t) : v + t;
    }
  red[g][e] = v;
  __syncthreads();
  if (g == 0 && f < F) {
    float t = red[0][e];
#pragma unroll
    for (int k = 1; k < 8; ++k) t = is_max ? fmaxf(t, red[k][e]) : t + red[k][e];
    if (pooling == HIPAC_MIL_MEAN) t = t / (float)(o1 - o0);
    pooled[(size_t)b * F + f] = t;
  }
}

// cdot[b] = pooled_b . g_b = sum_j a_j (x_j . g_b), the softmax backward's second term, as the K-head steps take it
// (mil_train_launch_cdot): known before any row is read.  The products are added in the order in which their ds kernels add
// x_i . g_b: lane c takes the float4s c, c + 64, ..., then the butterfly.  The two terms of ds_i = a_i (x_i . g_b - cdot_b)
// then round alike, and in a bag of one row, where a_i is 1 and pooled_b is x_i bit for bit, they are equal bit for bit:
// ds_i is exactly 0 there, as in exact arithmetic, and not a rounding residue that reaches every attention gradient.
__global__ __launch_bounds__(256) void mt_cdot_kernel(const float* __restrict__ pooled, const float* __restrict__ g, int F, int B,
                                                      float* __restrict__ cdot) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const f32x4* pb = reinterpret_cast<const f32x4*>(pooled + (size_t)b * F);
  const f32x4* gb = reinterpret_cast<const f32x4*>(g + (size_t)b * F);
  float v = 0.f;
  for (int c = lane; c < F / 4; c += 64) {
    const f32x4 pv = pb[c], gv = gb[c];
    v = fmaf(pv[0], gv[0], v), v = fmaf(pv[1], gv[1], v), v = fmaf(pv[2], gv[2], v), v = fmaf(pv[3], gv[3], v);
  }
  v = wave_sum(v);
  if (lane == 0) cdot[b] = v;
}

// The single-head step forms the softmax backward from ONE evaluation of the row dot products, as its closed form has it:
// ds_i = a_i (t_i - c_b), t_i = x_i . g_b, c_b = sum_j a_j t_j / sum_j a_j (= pooled_b . g_b, sum_j a_j being 1 in exact
// arithmetic).  sum_i ds_i of a bag is then 0 up to the rounding of its own terms, whatever the rounding of the t_i, and ds_i
// of a one-row bag is exactly 0.  With c_b taken from pooled_b . g_b, a second evaluation, the sum kept a rounding of the dot
// products, which is what db_U = sum ds_i and, for small A, db_V = U sum ds_i (1 - H_i^2) consist of.

// t_i = x_i . g_b for the rows of a tile; a wave takes rows wave, wave + 4, ...  The first of the backward's two sweeps over X.
__global__ __launch_bounds__(256) void mt_rowdot_kernel(const float* __restrict__ feats, const int32_t* __restrict__ rows,
                                                        const int32_t* __restrict__ bag_of, const float* __restrict__ g, int n, int F,
                                                        float* __restrict__ rowdot) {
  const int tile = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int F4 = F / 4;
  for (int rr = wave; rr < kMtTile; rr += 4) {
    const int i = tile * kMtTile + rr;
    if (i >= n) break;
    const f32x4* x = reinterpret_cast<const f32x4*>(feats + (size_t)(rows ? rows[i] : i) * F);
    const f32x4* gb = reinterpret_cast<const f32x4*>(g + (size_t)bag_of[i] * F);
    float t = 0.f;
    for (int c = lane; c < F4; c += 64) {
      const f32x4 xv = x[c], gv = gb[c];
      t = fmaf(xv[0], gv[0], t), t = fmaf(xv[1], gv[1], t), t = fmaf(xv[2], gv[2], t), t = fmaf(xv[3], gv[3], t);
    }
    t = wave_sum(t);
    if (lane == 0) rowdot[i] = t;
  }
}

// c_b = sum_j a_j t_j / sum_j a_j in double, one workgroup per bag: 4 bytes per row twice, like the softmax.  Fixed order:
// shuffle tree inside a wave, the four waves in order.
__global__ __launch_bounds__(256) void mt_bag_cdot_kernel(const float* __restrict__ rowdot, const float* __restrict__ attn,
                                                          const int32_t* __restrict__ offs, double* __restrict__ cdot) {
  __shared__ double red[2][4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int o0 = offs[b], o1 = offs[b + 1];
  double num = 0.0, den = 0.0;
  for (int i = o0 + tid; i < o1; i += 256) {
    const double a = attn[i];
    num += a * (double)rowdot[i];
    den += a;
  }
  num = wave_sum_tree(num), den = wave_sum_tree(den);
  if (lane == 0) red[0][wave] = num, red[1][wave] = den;
  __syncthreads();
  if (tid == 0)
    cdot[b] = (((red[0][0] + red[0][1]) + red[0][2]) + red[0][3]) / (((red[1][0] + red[1][1]) + red[1][2]) + red[1][3]);
}

// one sweep over the H rows of a tile: ds_i = a_i (t_i - c_b), the difference taken in double; H_i becomes dH_i = ds_i U (1 - H_i^2)
// in place; the tile's column sums part2[tile] = (sum dH_i [A_pad] | sum ds_i H_i [A_pad] | sum ds_i), added in double and
// rounded once.  A wave takes rows wave, wave + 4, ...
__global__ __launch_bounds__(256) void mt_ds_kernel(const float* __restrict__ rowdot, const int32_t* __restrict__ bag_of,
                                                    const float* __restrict__ attn, const double* __restrict__ cdot,
                                                    const float* __restrict__ Uw, float* __restrict__ H, int n, int A, int A_pad,
                                                    float* __restrict__ part2) {
  __shared__ double red[4][513];
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double accV[4] = {0.0, 0.0, 0.0, 0.0}, accU[4] = {0.0, 0.0, 0.0, 0.0}, accB = 0.0;
  float u[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) u[q] = lane + 64 * q < A ? Uw[lane + 64 * q] : 0.f;
  for (int rr = wave; rr < kMtTile; rr += 4) {
    const int i = tile * kMtTile + rr;
    if (i >= n) break;
    const float ds = attn[i] * (float)((double)rowdot[i] - cdot[bag_of[i]]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = lane + 64 * q;
      if (j < A_pad) {
        float* hp = H + (size_t)i * A_pad + j;
        const float hv = j < A ? *hp : 0.f;
        const float dh = ds * u[q] * (1.f - hv * hv);
        *hp = dh;
        accV[q] += (double)dh;
        accU[q] += (double)ds * (double)hv;
      }
    }
    accB += (double)ds;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) red[wave][64 * q + lane] = accV[q], red[wave][256 + 64 * q + lane] = accU[q];
  if (lane == 0) red[wave][512] = accB;
  __syncthreads();
  float* out = part2 + (size_t)tile * (2 * A_pad + 1);
  for (int k = tid; k < 513; k += 256) {
    const float s = (float)(((red[0][k] + red[1][k]) + red[2][k]) + red[3][k]);
    if (k < 256) {
      if (k < A_pad) out[k] = s;
    } else if (k < 512) {
      if (k - 256 < A_pad) out[A_pad + k - 256] = s;
    } else {
      out[2 * A_pad] = s;
    }
  }
}

// dst[e] (+)= sum over slices of part[k * per_slice + off + e], e < count.  32 elements x 8 slice groups per workgroup: group g
// adds slices g, g + 8, ... in turn, then the 8 group sums are added in order -- a fixed order, hence reproducible
__global__ __launch_bounds__(256) void mt_slab_reduce_kernel(const float* __restrict__ part, int slices, size_t per_slice, size_t off,
                                                             long long count, float* __restrict__ dst, int accumulate) {
  __shared__ float red[8][32];
  const int e = threadIdx.x & 31, g = threadIdx.x >> 5;
  const long long gid = (long long)blockIdx.x * 32 + e;
  float s = 0.f;
  if (gid < count)
    for (int k = g; k < slices; k += 8) s += part[(size_t)k * per_slice + off + gid];
  red[g][e] = s;
  __syncthreads();
  if (g == 0 && gid < count) {
    float v = red[0][e];
#pragma unroll
    for (int k = 1; k < 8; ++k) v += red[k][e];
    dst[gid] = accumulate ? dst[gid] + v : v;
  }
}

// dV partials: slab[slice][a][f] = sum over the slice's rows of dH[m][a] X[rows[m]][f] on v_mfma_f32_32x32x2_f32.
// One workgroup = 64 feature columns x ALL hidden units (A_pad / 32 <= 8 row tiles x 2 column tiles, up to 4 per wave)
// x one slice of rows, so this kernel reads every feature element exactly once; the reduction axis (rows) is the MFMA's k:
// both operands are staged 32 rows at a time into LDS as [row][channel] and read with the row as k, as train.hip's
// wgrad_kernel does (A = dH[row][a], B = X[row][f]: coalesced along the channel axis, no transpose).
__global__ __launch_bounds__(256) void mt_dv_kernel(const float* __restrict__ dH, const float* __restrict__ feats,
                                                    const int32_t* __restrict__ rows, int n, int F, int A, int A_pad, int chunk,
                                                    float* __restrict__ slab) {
  constexpr int LDB = 68;  // 64 floats + 4: keeps float4 stores aligned, spreads banks
  __shared__ __attribute__((aligned(16))) float As[32 * 260], Bs[32 * LDB];
  const int LDA = A_pad + 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int cj = wave & 1, a0 = wave >> 1;  // column half; row tiles a0, a0 + 2, a0 + 4, a0 + 6
  const int nAt = A_pad / 32, A4 = A_pad / 4;
  const int f0 = blockIdx.x * 64;
  const int m_begin = blockIdx.y * chunk;
  const int m_end = m_begin + chunk < n ? m_begin + chunk : n;
  // two levels of summation: the MFMA adds 128 rows into acc one after another, then acc is added to tot -- a chain of
  // chunk / 128 + 128 additions per element instead of chunk
  f32x16 acc[4], tot[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f, tot[t][e] = 0.f;
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
    float4 av[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      av[it] = zero4;
      if (it < nAt) {
        const int idx = tid + 256 * it, row = idx / A4, c4 = idx - row * A4;
        if (m0 + row < m_end) av[it] = *reinterpret_cast<const float4*>(dH + (size_t)(m0 + row) * A_pad + 4 * c4);
      }
    }
    __syncthreads();  // the previous sub-chunk's fragments have been read
    *reinterpret_cast<float4*>(Bs + spx * LDB + 4 * sc) = b0;
    *reinterpret_cast<float4*>(Bs + spx * LDB + 32 + 4 * sc) = b1;
#pragma unroll
    for (int it = 0; it < 8; ++it)
      if (it < nAt) {
        const int idx = tid + 256 * it, row = idx / A4, c4 = idx - row * A4;
        *reinterpret_cast<float4*>(As + row * LDA + 4 * c4) = av[it];
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int px = 2 * k + h;
      const float bv = Bs[px * LDB + cj * 32 + r];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (a0 + 2 * t < nAt) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(As[px * LDA + (a0 + 2 * t) * 32 + r], bv, acc[t], 0, 0, 0);
    }
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
  // D[a][f]: column f = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h
  const int f = f0 + cj * 32 + r;
  float* base = slab + (size_t)blockIdx.y * A * F;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (a0 + 2 * t < nAt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int a = (a0 + 2 * t) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (a < A && f < F) base[(size_t)a * F + f] = tot[t][e];
      }
    }
}

__global__ __launch_bounds__(256) void mt_l2_add_kernel(float* __restrict__ g, const float* __restrict__ p, long long n, float wd) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) g[i] += wd * p[i];
}

}  // namespace hipac

namespace hipac {

// mil_train_internal.h: what the K-head steps share with this one on the host
MilHeadPlan make_mil_head_plan(const hipac_mil_params_t* p, int K, int n, int n_bags, int planes, int attn_cols, bool train) {
  MilHeadPlan q{};
  const size_t F = p->feature_dim, A = p->attn_dim, Hd = p->hidden_dim, Cn = p->num_classes, B = n_bags, Kh = K;
  q.A_pad = (p->attn_dim + 31) / 32 * 32;
  q.ntiles = (n + kMtTile - 1) / kMtTile;
  q.nseg = q.ntiles + n_bags;
  q.P2 = (size_t)planes * q.A_pad + Kh * A + Kh;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align256(bytes);
    return at;
  };
  q.bag_of = take((size_t)n * 4);
  q.pooled = take(B * Kh * F * 4);
  q.hid = take(B * Hd * 4);
  q.part = take((size_t)q.nseg * Kh * F * 4);
  q.scores = take((size_t)n * attn_cols * 4);
  q.attn = take((size_t)n * attn_cols * 4);
  q.H = take((size_t)n * q.A_pad * 4);
  if (planes == 2) q.G = take((size_t)n * q.A_pad * 4);
  if (train) {
    mil_train_dv_slices(n, p->feature_dim, &q.chunk, &q.slices);
    q.dhid = take(B * Hd * 4);
    q.dym = take(B * Hd * 4);
    q.dlogits = take(B * Cn * 4);
    q.g = take(B * Kh * F * 4);
    q.ce = take((2 + 8 * ((B + 255) / 256)) * 4);
    q.cdot = take(B * Kh * 4);
    q.part2 = take((size_t)q.ntiles * q.P2 * 4);
    q.slab = take((size_t)q.slices * planes * A * F * 4);
  }
  q.total = o;
  return q;
}

int mil_check_forward_args(const char* who, bool ptrs, const char* count_name, int count, int max_count, const hipac_mil_params_t* p,
                           bool gate, int n, int n_bags, const void* feats, const void* workspace) {
  HIPAC_REQUIRE(ptrs, HIPAC_EINVAL, "%s: null argument", who);
  HIPAC_REQUIRE(count >= 1 && count <= max_count, HIPAC_EINVAL, "%s: %s %d (1..%d)", who, count_name, count, max_count);
  HIPAC_REQUIRE(mil_train_sizes_ok(p, n, n_bags), HIPAC_EINVAL,
                "%s: n %d, n_bags %d, feature_dim %d, attn_dim %d, hidden_dim %d, num_classes %d", who, n, n_bags, p->feature_dim,
                p->attn_dim, p->hidden_dim, p->num_classes);
  HIPAC_REQUIRE(p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b, HIPAC_EINVAL, "%s: classifier weights missing", who);
  HIPAC_REQUIRE(p->attn_V_w && p->attn_V_b && p->attn_U_w && p->attn_U_b && gate, HIPAC_EINVAL, "%s: attention weights missing", who);
  HIPAC_REQUIRE(((uintptr_t)feats & 15) == 0 && ((uintptr_t)workspace & 15) == 0, HIPAC_EINVAL,
                "%s: feats / workspace must be 16-byte aligned", who);
  return 0;
}

int mil_check_train_args(const char* who, bool ptrs, const char* count_name, int count, int max_count, const hipac_mil_params_t* p,
                         const hipac_mil_params_t* grads, bool attention, bool gate, int n, int n_bags, int n_feat_rows, bool has_rows,
                         const void* feats, const void* workspace) {
  HIPAC_REQUIRE(ptrs, HIPAC_EINVAL, "%s: null argument", who);
  if (count_name)
    HIPAC_REQUIRE(count >= 1 && count <= max_count, HIPAC_EINVAL, "%s: %s %d (1..%d)", who, count_name, count, max_count);
  HIPAC_REQUIRE(mil_train_dims_ok(p, attention ? HIPAC_MIL_ATTENTION : HIPAC_MIL_MEAN, n, n_bags), HIPAC_EINVAL,
                "%s: n %d, n_bags %d, feature_dim %d, attn_dim %d, hidden_dim %d, num_classes %d", who, n, n_bags, p->feature_dim,
                p->attn_dim, p->hidden_dim, p->num_classes);
  HIPAC_REQUIRE(n_feat_rows > 0 && (has_rows || n <= n_feat_rows), HIPAC_EINVAL, "%s: n_feat_rows %d for n %d rows", who, n_feat_rows, n);
  HIPAC_REQUIRE(p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b && grads->fc1_w && grads->fc1_b && grads->fc2_w && grads->fc2_b,
                HIPAC_EINVAL, "%s: classifier weights or their gradient buffers missing", who);
  if (attention)
    HIPAC_REQUIRE(p->attn_V_w && p->attn_V_b && p->attn_U_w && p->attn_U_b && grads->attn_V_w && grads->attn_V_b &&
                      grads->attn_U_w && grads->attn_U_b && gate,
                  HIPAC_EINVAL, "%s: attention weights or their gradient buffers missing", who);
  HIPAC_REQUIRE(((uintptr_t)feats & 15) == 0 && ((uintptr_t)workspace & 15) == 0, HIPAC_EINVAL,
                "%s: feats / workspace must be 16-byte aligned", who);
  return 0;
}

int mil_classifier_forward(const hipac_mil_params_t* p, const float* pooled, int cols, int B, float* hid, float* logits, void* stream) {
  const int rc = hipac_linear_forward(pooled, p->fc1_w, p->fc1_b, hid, B, p->hidden_dim, cols, 1, stream);
  if (rc) return rc;
  return hipac_linear_forward(hid, p->fc2_w, p->fc2_b, logits, B, p->num_classes, p->hidden_dim, 0, stream);
}

int mil_classifier_fwd_bwd(const hipac_mil_params_t* p, const hipac_mil_params_t* grads, int cols, int B, const int64_t* labels,
                           const float* class_w, float* loss, float* logits, const MilHeadPlan& q, char* ws, bool want_g, int accumulate,
                           void* stream, MilHiddenHook hook, void* hook_ctx) {
  const int Hd = p->hidden_dim, Cn = p->num_classes;
  hipStream_t s = (hipStream_t)stream;
  float* pooled = (float*)(ws + q.pooled);
  float* hid = (float*)(ws + q.hid);
  float* dhid = (float*)(ws + q.dhid);
  float* dlogits = (float*)(ws + q.dlogits);
  int rc = hipac_linear_forward(pooled, p->fc1_w, p->fc1_b, hid, B, Hd, cols, 1, stream);
  if (rc) return rc;
  if (hook && (rc = hook(hid, B, Hd, hook_ctx, s))) return rc;
  rc = hipac_linear_forward(hid, p->fc2_w, p->fc2_b, logits, B, Cn, Hd, 0, stream);
  if (rc) return rc;
  rc = hipac_cross_entropy_fwd_bwd(logits, labels, class_w, B, Cn, loss, dlogits, (float*)(ws + q.ce), stream);
  if (rc) return rc;
  rc = hipac_linear_backward(hid, p->fc2_w, dlogits, nullptr, nullptr, dhid, (float*)grads->fc2_w, (float*)grads->fc2_b, B, Cn, Hd,
                             accumulate, stream);
  if (rc) return rc;
  if (hook && (rc = hook(dhid, B, Hd, hook_ctx, s))) return rc;
  return hipac_linear_backward(pooled, p->fc1_w, dhid, hid, (float*)(ws + q.dym), want_g ? (float*)(ws + q.g) : nullptr,
                               (float*)grads->fc1_w, (float*)grads->fc1_b, B, Hd, cols, accumulate, stream);
}

void mil_head_launch_grads(const hipac_mil_params_t* grads, int K, const float* feats, const int32_t* rows, int n, int F, int A,
                           const MilHeadPlan& q, char* ws, int accumulate, hipStream_t s) {
  const float* part2 = (const float*)(ws + q.part2);
  float* slab = (float*)(ws + q.slab);
  const size_t Ap = (size_t)q.A_pad;
  mil_train_launch_slab_reduce(part2, q.ntiles, q.P2, 0, A, (float*)grads->attn_V_b, accumulate, s);
  mil_train_launch_slab_reduce(part2, q.ntiles, q.P2, Ap, (long long)K * A, (float*)grads->attn_U_w, accumulate, s);
  mil_train_launch_slab_reduce(part2, q.ntiles, q.P2, Ap + (size_t)K * A, K, (float*)grads->attn_U_b, accumulate, s);
  mil_train_launch_dv((const float*)(ws + q.H), feats, rows, n, F, A, q.A_pad, q.chunk, q.slices, slab, s);
  const long long total = (long long)A * F;
  mil_train_launch_slab_reduce(slab, q.slices, (size_t)total, 0, total, (float*)grads->attn_V_w, accumulate, s);
}

// The step itself.  `hook` (mil_train_internal.h) is called on hid after classifier.0 + ReLU and on dhid after
// classifier.2's backward; hipac_mil_train_fwd_bwd passes none.
int mil_train_run(const hipac_mil_params_t* p, int pooling, const float* feats, int n_feat_rows, const int32_t* rows,
                  const int32_t* bag_offsets, int n, int n_bags, const int64_t* labels, const float* class_w,
                  const hipac_mil_params_t* grads, float* loss, float* logits, float* attn, void* workspace, size_t workspace_bytes,
                  int accumulate, void* stream, MilHiddenHook hook, void* hook_ctx) {
  HIPAC_REQUIRE(p && feats && bag_offsets && labels && grads && loss && logits && workspace, HIPAC_EINVAL,
                "mil_train_fwd_bwd: null argument");
  HIPAC_REQUIRE(pooling >= HIPAC_MIL_ATTENTION && pooling <= HIPAC_MIL_MAX, HIPAC_EINVAL, "mil_train_fwd_bwd: pooling %d", pooling);
  const bool att = pooling == HIPAC_MIL_ATTENTION;
  int rc = mil_check_train_args("mil_train_fwd_bwd", true, nullptr, 0, 0, p, grads, att, true, n, n_bags, n_feat_rows, rows != nullptr,
                                feats, workspace);
  if (rc) return rc;
  const MilHeadPlan q = make_mil_train_plan(p, pooling, n, n_bags);
  HIPAC_REQUIRE(workspace_bytes >= q.total, HIPAC_EWORKSPACE, "mil_train_fwd_bwd: workspace %zu bytes, %zu needed", workspace_bytes,
                q.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int F = p->feature_dim, A = p->attn_dim, B = n_bags;
  int32_t* bag_of = (int32_t*)(ws + q.bag_of);
  float* pooled = (float*)(ws + q.pooled);
  float* g = (float*)(ws + q.g);
  float* part = (float*)(ws + q.part);
  float* a = att ? (attn ? attn : (float*)(ws + q.attn)) : nullptr;
  float* H = (float*)(ws + q.H);

  hipLaunchKernelGGL(mt_bag_of_kernel, dim3((n + 255) / 256), dim3(256), 0, s, bag_offsets, B, n, bag_of);
  if (att) {
    hipLaunchKernelGGL(mt_h_kernel, dim3(q.ntiles, (A + 63) / 64), dim3(256), 0, s, feats, rows, n, F, p->attn_V_w, p->attn_V_b, A,
                       q.A_pad, H);
    hipLaunchKernelGGL(mt_score_kernel, dim3((n + 15) / 16), dim3(256), 0, s, (const float*)H, n, A, q.A_pad, p->attn_U_w,
                       p->attn_U_b, (float*)(ws + q.scores));
    hipLaunchKernelGGL(mt_softmax_kernel, dim3(B), dim3(256), 0, s, (const float*)(ws + q.scores), bag_offsets, a);
  }
  hipLaunchKernelGGL(mt_pool_kernel, dim3(q.ntiles), dim3(256), 0, s, feats, rows, (const int32_t*)bag_of, (const float*)a, n, F,
                     pooling, part);
  hipLaunchKernelGGL(mt_pool_combine_kernel, dim3(B, (F + 31) / 32), dim3(256), 0, s, (const float*)part, bag_offsets, F, pooling,
                     pooled);
  HIPAC_CHECK_HIP(hipGetLastError());
  rc = mil_classifier_fwd_bwd(p, grads, F, B, labels, class_w, loss, logits, q, ws, att, accumulate, stream, hook, hook_ctx);
  if (rc) return rc;
  if (att) {
    double* cdot = (double*)(ws + q.cdot);
    float* rowdot = (float*)(ws + q.scores);  // the scores are spent once the softmax has run
    float* part2 = (float*)(ws + q.part2);
    float* slab = (float*)(ws + q.slab);
    hipLaunchKernelGGL(mt_rowdot_kernel, dim3(q.ntiles), dim3(256), 0, s, feats, rows, (const int32_t*)bag_of, (const float*)g, n, F,
                       rowdot);
    hipLaunchKernelGGL(mt_bag_cdot_kernel, dim3(B), dim3(256), 0, s, (const float*)rowdot, (const float*)a, bag_offsets, cdot);
    hipLaunchKernelGGL(mt_ds_kernel, dim3(q.ntiles), dim3(256), 0, s, (const float*)rowdot, (const int32_t*)bag_of, (const float*)a,
                       (const double*)cdot, p->attn_U_w, H, n, A, q.A_pad, part2);
    mil_train_launch_slab_reduce(part2, q.ntiles, q.P2, 0, A, (float*)grads->attn_V_b, accumulate, s);
    mil_train_launch_slab_reduce(part2, q.ntiles, q.P2, (size_t)q.A_pad, A, (float*)grads->attn_U_w, accumulate, s);
    mil_train_launch_slab_reduce(part2, q.ntiles, q.P2, 2 * (size_t)q.A_pad, 1, (float*)grads->attn_U_b, accumulate, s);
    mil_train_launch_dv(H, feats, rows, n, F, A, q.A_pad, q.chunk, q.slices, slab, s);
    const long long total = (long long)A * F;
    mil_train_launch_slab_reduce(slab, q.slices, (size_t)total, 0, total, (float*)grads->attn_V_w, accumulate, s);
    HIPAC_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

// mil_train_internal.h: the launches of the kernels above that do not depend on the number of attention heads.  The same
// launch shapes as in mil_train_run.
bool mil_train_sizes_ok(const hipac_mil_params_t* p, int n, int n_bags) { return mil_train_dims_ok(p, HIPAC_MIL_ATTENTION, n, n_bags); }

// dV: one workgroup = 64 feature columns x all of A x one slice of rows; about 512 workgroups in all
void mil_train_dv_slices(int n, int F, int* chunk, int* slices) {
  const int fchunks = (F + 63) / 64;
  const int target = 512 / fchunks > 0 ? 512 / fchunks : 1;
  *chunk = ((n + target - 1) / target + 31) / 32 * 32;
  *slices = (n + *chunk - 1) / *chunk;
}

void mil_train_launch_bag_of(const int32_t* offs, int n_bags, int n, int32_t* bag_of, hipStream_t s) {
  hipLaunchKernelGGL(mt_bag_of_kernel, dim3((n + 255) / 256), dim3(256), 0, s, offs, n_bags, n, bag_of);
}

void mil_train_launch_h(const float* feats, const int32_t* rows, int n, int F, const float* Vw, const float* Vb, int A, int A_pad,
                        float* H, hipStream_t s) {
  hipLaunchKernelGGL(mt_h_kernel, dim3((n + kMtTile - 1) / kMtTile, (A + 63) / 64), dim3(256), 0, s, feats, rows, n, F, Vw, Vb, A,
                     A_pad, H);
}

void mil_train_launch_pool_combine(const float* part, const int32_t* offs, int n_bags, int F, float* pooled, hipStream_t s) {
  hipLaunchKernelGGL(mt_pool_combine_kernel, dim3(n_bags, (F + 31) / 32), dim3(256), 0, s, part, offs, F, (int)HIPAC_MIL_ATTENTION,
                     pooled);
}

void mil_train_launch_cdot(const float* pooled, const float* g, int F, int B, float* cdot, hipStream_t s) {
  hipLaunchKernelGGL(mt_cdot_kernel, dim3((B + 3) / 4), dim3(256), 0, s, pooled, g, F, B, cdot);
}

void mil_train_launch_slab_reduce(const float* part, int slices, size_t per_slice, size_t off, long long count, float* dst,
                                  int accumulate, hipStream_t s) {
  hipLaunchKernelGGL(mt_slab_reduce_kernel, dim3((unsigned)((count + 31) / 32)), dim3(256), 0, s, part, slices, per_slice, off, count,
                     dst, accumulate);
}

void mil_train_launch_dv(const float* dH, const float* feats, const int32_t* rows, int n, int F, int A, int A_pad, int chunk,
                         int slices, float* slab, hipStream_t s) {
  hipLaunchKernelGGL(mt_dv_kernel, dim3((F + 63) / 64, slices), dim3(256), 0, s, dH, feats, rows, n, F, A, A_pad, chunk, slab);
}

}  // namespace hipac

using namespace hipac;

extern "C" {

int hipac_mil_train_abi_version(void) { return HIPAC_MIL_TRAIN_ABI_VERSION; }

size_t hipac_mil_train_workspace_bytes(const hipac_mil_params_t* params, int pooling, int n, int n_bags) {
  return mil_train_dims_ok(params, pooling, n, n_bags) ? make_mil_train_plan(params, pooling, n, n_bags).total : 0;
}

int hipac_mil_train_fwd_bwd(const hipac_mil_params_t* p, int pooling, const float* feats, int n_feat_rows, const int32_t* rows,
                            const int32_t* bag_offsets, int n, int n_bags, const int64_t* labels, const float* class_w,
                            const hipac_mil_params_t* grads, float* loss, float* logits, float* attn, void* workspace,
                            size_t workspace_bytes, int accumulate, void* stream) {
  return mil_train_run(p, pooling, feats, n_feat_rows, rows, bag_offsets, n, n_bags, labels, class_w, grads, loss, logits, attn,
                       workspace, workspace_bytes, accumulate, stream, nullptr, nullptr);
}

int hipac_mil_train_l2_add(float* grads, const float* params, int64_t n, float wd, void* stream) {
  HIPAC_REQUIRE(grads && params && n > 0, HIPAC_EINVAL, "mil_train_l2_add: bad argument");
  long long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(mt_l2_add_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, grads, params, (long long)n, wd);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"

// Multi-head attention pooling for the MIL head (include/hipac_mil_heads.h): K attention branches over one shared
// hidden layer, inference and the training step, fp32.
//
//   H = tanh(X V^T + b_V) [n][A]   S = H U^T + b_U [n][K]   a[:, k] = softmax of S[:, k] inside each bag
//   M[b][k] = sum_i a[i][k] x_i    pooled_b = (M[b][0] | .. | M[b][K-1])    logits = classifier(pooled)
//   backward (g[b][k] = dL/dM[b][k]):  ds[i][k] = a[i][k] (x_i . g[b][k] - M[b][k] . g[b][k]),
//   dH_i = (sum_k ds[i][k] U[k]) (1 - H_i^2) in place over H, dV = dH^T X, db_V = sum dH_i, dU[k] = sum ds[i][k] H_i,
//   db_U[k] = sum ds[i][k].
//
// X V^T and dV = dH^T X do not depend on K: they are mil_train.hip's kernels, launched through mil_train_internal.h, and
// so are the row -> bag map, the per-bag combination of the pooling segments (over K F columns instead of F), the
// M . g products (over B K rows instead of B) and the fixed-order slab sums.  What depends on K is here, and every
// kernel here that touches a feature row reads it ONCE for all K heads: the pooling keeps K f32x4 accumulators per lane
// (32 VGPRs at K = 8), the backward's row sweep K dot products.  A step therefore sweeps X four times whatever K is
// (X V^T, pooling, row dots, dV), as the single-head step does.  The tiling and the segment scheme are mil_train.hip's:
// 64 rows per tile whatever the bag boundaries, segment (tile t, bag b) = id t + b; no float atomics.
#include "common.h"

#include "../../include/hipac_mil_heads.h"
#include "mil_train_internal.h"

namespace hipac {

constexpr int kMhTile = 64;  // rows per tile: mil_train.hip's kMtTile (mil_train_launch_pool_combine assumes it)
constexpr int kMhMaxHeads = HIPAC_MIL_MAX_HEADS;

struct MilHeadsPlan {
  int A_pad, ntiles, nseg, chunk, slices;
  size_t P2;  // floats of one tile's column sums: sum dH_i [A_pad] | sum ds[i][k] H_i [K][A] | sum ds[i][k] [K]
  size_t bag_of, pooled, hid, dhid, dym, dlogits, g, ce, cdot, part, scores, attn, H, part2, slab, total;
};

static bool mil_heads_dims_ok(const hipac_mil_params_t* p, int heads, int n, int n_bags) {
  return heads >= 1 && heads <= kMhMaxHeads && mil_train_sizes_ok(p, n, n_bags);
}

static MilHeadsPlan make_mil_heads_plan(const hipac_mil_params_t* p, int heads, int n, int n_bags, bool train) {
  MilHeadsPlan q{};
  const size_t F = p->feature_dim, A = p->attn_dim, Hd = p->hidden_dim, Cn = p->num_classes, B = n_bags, K = heads;
  q.A_pad = (p->attn_dim + 31) / 32 * 32;
  q.ntiles = (n + kMhTile - 1) / kMhTile;
  q.nseg = q.ntiles + n_bags;
  q.P2 = (size_t)q.A_pad + K * A + K;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align256(bytes);
    return at;
  };
  q.bag_of = take((size_t)n * 4);
  q.pooled = take(B * K * F * 4);
  q.hid = take(B * Hd * 4);
  q.part = take((size_t)q.nseg * K * F * 4);
  q.scores = take((size_t)n * K * 4);
  q.attn = take((size_t)n * K * 4);
  q.H = take((size_t)n * q.A_pad * 4);
  if (train) {
    mil_train_dv_slices(n, p->feature_dim, &q.chunk, &q.slices);
    q.dhid = take(B * Hd * 4);
    q.dym = take(B * Hd * 4);
    q.dlogits = take(B * Cn * 4);
    q.g = take(B * K * F * 4);
    q.ce = take((2 + 8 * ((B + 255) / 256)) * 4);
    q.cdot = take(B * K * 4);
    q.part2 = take((size_t)q.ntiles * q.P2 * 4);
    q.slab = take((size_t)q.slices * A * F * 4);
  }
  q.total = o;
  return q;
}

// S[i][k] = U[k] . H_i + b_U[k]: one wave per row, 16 rows per workgroup; the row of H is read once for the K heads
template <int K>
__global__ __launch_bounds__(256) void mh_score_kernel(const float* __restrict__ H, int n, int A, int A_pad,
                                                       const float* __restrict__ Uw, const float* __restrict__ Ub,
                                                       float* __restrict__ scores) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float u[K][4];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q) u[k][q] = lane + 64 * q < A ? Uw[k * A + lane + 64 * q] : 0.f;
  for (int rr = wave; rr < 16; rr += 4) {
    const int i = blockIdx.x * 16 + rr;
    if (i >= n) break;
    float h[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) h[q] = lane + 64 * q < A ? H[(size_t)i * A_pad + lane + 64 * q] : 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float v = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) v = fmaf(u[k][q], h[q], v);
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0) scores[(size_t)i * K + k] = v + Ub[k];
    }
  }
}

__device__ __forceinline__ float mh_block_reduce(float v, bool is_max, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) {
    const float t = __shfl_down(v, o, 64);
    v = is_max ? fmaxf(v, t) : v + t;
  }
  __syncthreads();  // red may still be read from a previous call
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < 4; ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
  return r;
}

// softmax of column k of the scores inside bag b: one workgroup per (bag, head).  4 K bytes per row
__global__ __launch_bounds__(256) void mh_softmax_kernel(const float* __restrict__ scores, const int32_t* __restrict__ offs, int K,
                                                         float* __restrict__ attn) {
  __shared__ float red[4];
  const int b = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  const int o0 = offs[b], o1 = offs[b + 1];
  float mx = -INFINITY;
  for (int i = o0 + tid; i < o1; i += 256) mx = fmaxf(mx, scores[(size_t)i * K + k]);
  const float m = mh_block_reduce(mx, true, red);
  float z = 0.f;
  for (int i = o0 + tid; i < o1; i += 256) z += expf(scores[(size_t)i * K + k] - m);
  const float inv = 1.f / mh_block_reduce(z, false, red);
  for (int i = o0 + tid; i < o1; i += 256) attn[(size_t)i * K + k] = expf(scores[(size_t)i * K + k] - m) * inv;
}

// pooling partials: tile t of 64 rows -> part[t + b][K][F] for every bag b it holds.  A lane owns four feature columns and
// keeps one f32x4 accumulator per head, so a row's columns are loaded once and used K times
template <int K>
__global__ __launch_bounds__(256) void mh_pool_kernel(const float* __restrict__ feats, const int32_t* __restrict__ rows,
                                                      const int32_t* __restrict__ bag_of, const float* __restrict__ w, int n, int F,
                                                      float* __restrict__ part) {
  __shared__ int sb[kMhTile];
  __shared__ int sro[kMhTile];
  __shared__ float sw[kMhTile * K];
  const int tile = blockIdx.x, tid = threadIdx.x;
  const int r0 = tile * kMhTile;
  const int cnt = n - r0 < kMhTile ? n - r0 : kMhTile;
  if (tid < cnt) {
    sb[tid] = bag_of[r0 + tid];
    sro[tid] = rows ? rows[r0 + tid] : r0 + tid;
  }
  for (int e = tid; e < cnt * K; e += 256) sw[e] = w[(size_t)r0 * K + e];
  __syncthreads();
  const int F4 = F / 4;
  const f32x4* x4 = reinterpret_cast<const f32x4*>(feats);
  f32x4* p4 = reinterpret_cast<f32x4*>(part);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int c = tid; c < F4; c += 256) {
    f32x4 acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = zero;
    int cur = sb[0];
    for (int i = 0; i < cnt; ++i) {
      const int b = sb[i];
      if (b != cur) {
#pragma unroll
        for (int k = 0; k < K; ++k) p4[((size_t)(tile + cur) * K + k) * F4 + c] = acc[k], acc[k] = zero;
        cur = b;
      }
      const f32x4 x = x4[(size_t)sro[i] * F4 + c];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float a = sw[i * K + k];
        acc[k][0] = fmaf(a, x[0], acc[k][0]), acc[k][1] = fmaf(a, x[1], acc[k][1]);
        acc[k][2] = fmaf(a, x[2], acc[k][2]), acc[k][3] = fmaf(a, x[3], acc[k][3]);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) p4[((size_t)(tile + cur) * K + k) * F4 + c] = acc[k];
  }
}

// one sweep over the rows of a tile.  A wave takes rows wave, wave + 4, ...; it reads x_i once and forms the K products
// x_i . g[b][k] (g is n_bags K F floats, cache resident), then ds[i][k] = a[i][k] (x_i . g[b][k] - cdot[b][k]); H_i becomes
// dH_i = (sum_k ds[i][k] U[k]) (1 - H_i^2) in place; the tile's column sums go to
// part2[tile] = (sum dH_i [A_pad] | sum ds[i][k] H_i [K][A] | sum ds[i][k] [K])
template <int K>
__global__ __launch_bounds__(256) void mh_ds_kernel(const float* __restrict__ feats, const int32_t* __restrict__ rows,
                                                    const int32_t* __restrict__ bag_of, const float* __restrict__ attn,
                                                    const float* __restrict__ g, const float* __restrict__ cdot,
                                                    const float* __restrict__ Uw, float* __restrict__ H, int n, int F, int A,
                                                    int A_pad, float* __restrict__ part2) {
  constexpr int RED = 256 * (K + 1) + K;
  __shared__ float red[4][RED];
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float accV[4] = {0.f, 0.f, 0.f, 0.f}, accU[K][4], accB[K], u[K][4];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    accB[k] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) accU[k][q] = 0.f, u[k][q] = lane + 64 * q < A ? Uw[k * A + lane + 64 * q] : 0.f;
  }
  const int F4 = F / 4;
  for (int rr = wave; rr < kMhTile; rr += 4) {
    const int i = tile * kMhTile + rr;
    if (i >= n) break;
    const int b = bag_of[i];
    const f32x4* x = reinterpret_cast<const f32x4*>(feats + (size_t)(rows ? rows[i] : i) * F);
    const f32x4* gb = reinterpret_cast<const f32x4*>(g + (size_t)b * K * F);
    float t[K];
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
    float ds[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float v = t[k];
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      ds[k] = attn[(size_t)i * K + k] * (v - cdot[b * K + k]);
      accB[k] += ds[k];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = lane + 64 * q;
      if (j < A_pad) {
        float* hp = H + (size_t)i * A_pad + j;
        const float hv = j < A ? *hp : 0.f;
        float s = ds[0] * u[0][q];
#pragma unroll
        for (int k = 1; k < K; ++k) s = fmaf(ds[k], u[k][q], s);
        const float dh = s * (1.f - hv * hv);
        *hp = dh;
        accV[q] += dh;
#pragma unroll
        for (int k = 0; k < K; ++k) accU[k][q] = fmaf(ds[k], hv, accU[k][q]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    red[wave][64 * q + lane] = accV[q];
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave][256 * (k + 1) + 64 * q + lane] = accU[k][q];
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave][256 * (K + 1) + k] = accB[k];
  }
  __syncthreads();
  float* out = part2 + (size_t)tile * ((size_t)A_pad + (size_t)K * A + K);
  for (int e = tid; e < RED; e += 256) {
    const float s = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
    const int blk = e >> 8, j = e & 255;
    if (blk == 0) {
      if (j < A_pad) out[j] = s;
    } else if (blk <= K) {
      if (j < A) out[A_pad + (blk - 1) * A + j] = s;
    } else {
      out[A_pad + K * A + j] = s;
    }
  }
}

#define MH_FOR_HEADS(heads, CALL) \
  switch (heads) {                \
    case 1: CALL(1); break;       \
    case 2: CALL(2); break;       \
    case 3: CALL(3); break;       \
    case 4: CALL(4); break;       \
    case 5: CALL(5); break;       \
    case 6: CALL(6); break;       \
    case 7: CALL(7); break;       \
    default: CALL(8); break;      \
  }

// the forward up to the pooled vectors, shared by inference and the step: bag_of, H, a [n][K], pooled [n_bags][K F]
static void mil_heads_pool(const hipac_mil_params_t* p, int K, const float* feats, const int32_t* rows, const int32_t* bag_offsets,
                           int n, int n_bags, const MilHeadsPlan& q, char* ws, float* a, float* pooled, hipStream_t s) {
  const int F = p->feature_dim, A = p->attn_dim;
  int32_t* bag_of = (int32_t*)(ws + q.bag_of);
  float* H = (float*)(ws + q.H);
  float* scores = (float*)(ws + q.scores);
  float* part = (float*)(ws + q.part);
  mil_train_launch_bag_of(bag_offsets, n_bags, n, bag_of, s);
  mil_train_launch_h(feats, rows, n, F, p->attn_V_w, p->attn_V_b, A, q.A_pad, H, s);
#define MH_SCORE(KK) \
  hipLaunchKernelGGL(mh_score_kernel<KK>, dim3((n + 15) / 16), dim3(256), 0, s, (const float*)H, n, A, q.A_pad, p->attn_U_w, p->attn_U_b, scores)
  MH_FOR_HEADS(K, MH_SCORE)
#undef MH_SCORE
  hipLaunchKernelGGL(mh_softmax_kernel, dim3(n_bags, K), dim3(256), 0, s, (const float*)scores, bag_offsets, K, a);
#define MH_POOL(KK) \
  hipLaunchKernelGGL(mh_pool_kernel<KK>, dim3(q.ntiles), dim3(256), 0, s, feats, rows, (const int32_t*)bag_of, (const float*)a, n, F, part)
  MH_FOR_HEADS(K, MH_POOL)
#undef MH_POOL
  mil_train_launch_pool_combine(part, bag_offsets, n_bags, K * F, pooled, s);
}

void mil_heads_launch_pool(const float* feats, const int32_t* rows, const int32_t* bag_of, const float* a, int n, int F, int K,
                           int ntiles, float* part, hipStream_t s) {
#define MH_POOL(KK) hipLaunchKernelGGL(mh_pool_kernel<KK>, dim3(ntiles), dim3(256), 0, s, feats, rows, bag_of, a, n, F, part)
  MH_FOR_HEADS(K, MH_POOL)
#undef MH_POOL
}

}  // namespace hipac

using namespace hipac;

extern "C" {

int hipac_mil_heads_abi_version(void) { return HIPAC_MIL_HEADS_ABI_VERSION; }

size_t hipac_mil_heads_forward_workspace_bytes(const hipac_mil_params_t* params, int heads, int n, int n_bags) {
  return mil_heads_dims_ok(params, heads, n, n_bags) ? make_mil_heads_plan(params, heads, n, n_bags, false).total : 0;
}

size_t hipac_mil_heads_train_workspace_bytes(const hipac_mil_params_t* params, int heads, int n, int n_bags) {
  return mil_heads_dims_ok(params, heads, n, n_bags) ? make_mil_heads_plan(params, heads, n, n_bags, true).total : 0;
}

int hipac_mil_heads_forward(const hipac_mil_params_t* p, int heads, const float* feats, const int32_t* bag_offsets, int n,
                            int n_bags, float* logits, float* attn, float* pooled, void* workspace, size_t workspace_bytes,
                            void* stream) {
  HIPAC_REQUIRE(p && feats && bag_offsets && logits && workspace, HIPAC_EINVAL, "mil_heads_forward: null argument");
  HIPAC_REQUIRE(heads >= 1 && heads <= kMhMaxHeads, HIPAC_EINVAL, "mil_heads_forward: heads %d (1..%d)", heads, kMhMaxHeads);
  HIPAC_REQUIRE(mil_heads_dims_ok(p, heads, n, n_bags), HIPAC_EINVAL,
                "mil_heads_forward: n %d, n_bags %d, feature_dim %d, attn_dim %d, hidden_dim %d, num_classes %d", n, n_bags,
                p->feature_dim, p->attn_dim, p->hidden_dim, p->num_classes);
  HIPAC_REQUIRE(p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b, HIPAC_EINVAL, "mil_heads_forward: classifier weights missing");
  HIPAC_REQUIRE(p->attn_V_w && p->attn_V_b && p->attn_U_w && p->attn_U_b, HIPAC_EINVAL, "mil_heads_forward: attention weights missing");
  HIPAC_REQUIRE(((uintptr_t)feats & 15) == 0 && ((uintptr_t)workspace & 15) == 0, HIPAC_EINVAL,
                "mil_heads_forward: feats / workspace must be 16-byte aligned");
  const MilHeadsPlan q = make_mil_heads_plan(p, heads, n, n_bags, false);
  HIPAC_REQUIRE(workspace_bytes >= q.total, HIPAC_EWORKSPACE, "mil_heads_forward: workspace %zu bytes, %zu needed", workspace_bytes,
                q.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* a = attn ? attn : (float*)(ws + q.attn);
  float* pl = pooled ? pooled : (float*)(ws + q.pooled);
  float* hid = (float*)(ws + q.hid);
  mil_heads_pool(p, heads, feats, nullptr, bag_offsets, n, n_bags, q, ws, a, pl, s);
  HIPAC_CHECK_HIP(hipGetLastError());
  int rc = hipac_linear_forward(pl, p->fc1_w, p->fc1_b, hid, n_bags, p->hidden_dim, heads * p->feature_dim, 1, stream);
  if (rc) return rc;
  return hipac_linear_forward(hid, p->fc2_w, p->fc2_b, logits, n_bags, p->num_classes, p->hidden_dim, 0, stream);
}

int hipac_mil_heads_train_fwd_bwd(const hipac_mil_params_t* p, int heads, const float* feats, int n_feat_rows, const int32_t* rows,
                                  const int32_t* bag_offsets, int n, int n_bags, const int64_t* labels, const float* class_w,
                                  const hipac_mil_params_t* grads, float* loss, float* logits, float* attn, void* workspace,
                                  size_t workspace_bytes, int accumulate, void* stream) {
  HIPAC_REQUIRE(p && feats && bag_offsets && labels && grads && loss && logits && workspace, HIPAC_EINVAL,
                "mil_heads_train_fwd_bwd: null argument");
  HIPAC_REQUIRE(heads >= 1 && heads <= kMhMaxHeads, HIPAC_EINVAL, "mil_heads_train_fwd_bwd: heads %d (1..%d)", heads, kMhMaxHeads);
  HIPAC_REQUIRE(mil_heads_dims_ok(p, heads, n, n_bags), HIPAC_EINVAL,
                "mil_heads_train_fwd_bwd: n %d, n_bags %d, feature_dim %d, attn_dim %d, hidden_dim %d, num_classes %d", n, n_bags,
                p->feature_dim, p->attn_dim, p->hidden_dim, p->num_classes);
  HIPAC_REQUIRE(n_feat_rows > 0 && (rows || n <= n_feat_rows), HIPAC_EINVAL, "mil_heads_train_fwd_bwd: n_feat_rows %d for n %d rows",
                n_feat_rows, n);
  HIPAC_REQUIRE(p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b && grads->fc1_w && grads->fc1_b && grads->fc2_w && grads->fc2_b,
                HIPAC_EINVAL, "mil_heads_train_fwd_bwd: classifier weights or their gradient buffers missing");
  HIPAC_REQUIRE(p->attn_V_w && p->attn_V_b && p->attn_U_w && p->attn_U_b && grads->attn_V_w && grads->attn_V_b && grads->attn_U_w &&
                    grads->attn_U_b,
                HIPAC_EINVAL, "mil_heads_train_fwd_bwd: attention weights or their gradient buffers missing");
  HIPAC_REQUIRE(((uintptr_t)feats & 15) == 0 && ((uintptr_t)workspace & 15) == 0, HIPAC_EINVAL,
                "mil_heads_train_fwd_bwd: feats / workspace must be 16-byte aligned");
  const MilHeadsPlan q = make_mil_heads_plan(p, heads, n, n_bags, true);
  HIPAC_REQUIRE(workspace_bytes >= q.total, HIPAC_EWORKSPACE, "mil_heads_train_fwd_bwd: workspace %zu bytes, %zu needed",
                workspace_bytes, q.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int F = p->feature_dim, A = p->attn_dim, Hd = p->hidden_dim, Cn = p->num_classes, B = n_bags, K = heads;
  float* pooled = (float*)(ws + q.pooled);
  float* hid = (float*)(ws + q.hid);
  float* dhid = (float*)(ws + q.dhid);
  float* dym = (float*)(ws + q.dym);
  float* dlogits = (float*)(ws + q.dlogits);
  float* g = (float*)(ws + q.g);
  float* a = attn ? attn : (float*)(ws + q.attn);
  float* H = (float*)(ws + q.H);
  float* cdot = (float*)(ws + q.cdot);
  float* part2 = (float*)(ws + q.part2);
  float* slab = (float*)(ws + q.slab);

  mil_heads_pool(p, K, feats, rows, bag_offsets, n, B, q, ws, a, pooled, s);
  HIPAC_CHECK_HIP(hipGetLastError());
  // classifier.0 over the K F pooled columns + ReLU, classifier.2, cross-entropy, and their backward: hipac.h's entry points
  int rc = hipac_linear_forward(pooled, p->fc1_w, p->fc1_b, hid, B, Hd, K * F, 1, stream);
  if (rc) return rc;
  rc = hipac_linear_forward(hid, p->fc2_w, p->fc2_b, logits, B, Cn, Hd, 0, stream);
  if (rc) return rc;
  rc = hipac_cross_entropy_fwd_bwd(logits, labels, class_w, B, Cn, loss, dlogits, (float*)(ws + q.ce), stream);
  if (rc) return rc;
  rc = hipac_linear_backward(hid, p->fc2_w, dlogits, nullptr, nullptr, dhid, (float*)grads->fc2_w, (float*)grads->fc2_b, B, Cn, Hd,
                             accumulate, stream);
  if (rc) return rc;
  rc = hipac_linear_backward(pooled, p->fc1_w, dhid, hid, dym, g, (float*)grads->fc1_w, (float*)grads->fc1_b, B, Hd, K * F,
                             accumulate, stream);
  if (rc) return rc;
  // pooled and g are [B K][F]: cdot[b][k] = M[b][k] . g[b][k]
  mil_train_launch_cdot(pooled, g, F, B * K, cdot, s);
#define MH_DS(KK)                                                                                                               \
  hipLaunchKernelGGL(mh_ds_kernel<KK>, dim3(q.ntiles), dim3(256), 0, s, feats, rows, (const int32_t*)(ws + q.bag_of), (const float*)a, \
                     (const float*)g, (const float*)cdot, p->attn_U_w, H, n, F, A, q.A_pad, part2)
  MH_FOR_HEADS(K, MH_DS)
#undef MH_DS
  mil_train_launch_slab_reduce(part2, q.ntiles, q.P2, 0, A, (float*)grads->attn_V_b, accumulate, s);
  mil_train_launch_slab_reduce(part2, q.ntiles, q.P2, (size_t)q.A_pad, (long long)K * A, (float*)grads->attn_U_w, accumulate, s);
  mil_train_launch_slab_reduce(part2, q.ntiles, q.P2, (size_t)q.A_pad + (size_t)K * A, K, (float*)grads->attn_U_b, accumulate, s);
  mil_train_launch_dv(H, feats, rows, n, F, A, q.A_pad, q.chunk, q.slices, slab, s);
  const long long total = (long long)A * F;
  mil_train_launch_slab_reduce(slab, q.slices, (size_t)total, 0, total, (float*)grads->attn_V_w, accumulate, s);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"

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
// M . g products (over B K rows instead of B) and the fixed-order slab sums.  The workspace plan, the argument checks and
// the classifier chain are mil_train_internal.h's too, the reductions inside the kernels wave_reduce.h's.  What depends on K
// is here: the four kernels, the forward up to the pooled vectors and the two entry points.  Every
// kernel here that touches a feature row reads it ONCE for all K heads: the pooling keeps K f32x4 accumulators per lane
// (32 VGPRs at K = 8), the backward's row sweep K dot products.  A step therefore sweeps X four times whatever K is
// (X V^T, pooling, row dots, dV), as the single-head step does.  The tiling and the segment scheme are mil_train.hip's:
// 64 rows per tile whatever the bag boundaries, segment (tile t, bag b) = id t + b; no float atomics.
#include "common.h"

#include "../../include/hipac_mil_heads.h"
#include "mil_device.h"
#include "mil_train_internal.h"
#include "wave_reduce.h"

namespace hipac {

constexpr int kMhTile = 64;  // rows per tile: mil_train.hip's kMtTile (mil_train_launch_pool_combine assumes it)
constexpr int kMhMaxHeads = HIPAC_MIL_MAX_HEADS;

static bool mil_heads_dims_ok(const hipac_mil_params_t* p, int heads, int n, int n_bags) {
  return heads >= 1 && heads <= kMhMaxHeads && mil_train_sizes_ok(p, n, n_bags);
}

// S[i][k] = U[k] . H_i + b_U[k]: one wave per row, 16 rows per workgroup; the row of H is read once for the K heads
template <int K>
__global__ __launch_bounds__(256) void mh_score_kernel(const float* __restrict__ H, int n, int A, int A_pad,
                                                       const float* __restrict__ Uw, const float* __restrict__ Ub,
                                                       float* __restrict__ scores) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float u[K][4];
  mil_load_u<K>(Uw, A, lane, u);
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
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);  // not wave_sum: it costs K = 1 a register here (21 -> 22)
      if (lane == 0) scores[(size_t)i * K + k] = v + Ub[k];
    }
  }
}

// softmax of column k of the scores inside bag b: one workgroup per (bag, head).  4 K bytes per row
__global__ __launch_bounds__(256) void mh_softmax_kernel(const float* __restrict__ scores, const int32_t* __restrict__ offs, int K,
                                                         float* __restrict__ attn) {
  __shared__ float red[4];
  const int b = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  const int o0 = offs[b], o1 = offs[b + 1];
  float mx = -INFINITY;
  for (int i = o0 + tid; i < o1; i += 256) mx = fmaxf(mx, scores[(size_t)i * K + k]);
  const float m = block_max_tree<4>(mx, red);
  float z = 0.f;
  for (int i = o0 + tid; i < o1; i += 256) z += expf(scores[(size_t)i * K + k] - m);
  const float inv = 1.f / block_sum_tree<4>(z, red);
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
  mil_load_u<K>(Uw, A, lane, u);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    accB[k] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) accU[k][q] = 0.f;
  }
  const int F4 = F / 4;
  for (int rr = wave; rr < kMhTile; rr += 4) {
    const int i = tile * kMhTile + rr;
    if (i >= n) break;
    const int b = bag_of[i];
    const f32x4* x = reinterpret_cast<const f32x4*>(feats + (size_t)(rows ? rows[i] : i) * F);
    const f32x4* gb = reinterpret_cast<const f32x4*>(g + (size_t)b * K * F);
    // the K dot products: the same loop as in mil_gated.hip's mg_ds_kernel (as a function of mil_device.h it moved mh_ds_kernel's
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
  mil_store_part2<K, 1>(red, A, A_pad, tid, part2 + (size_t)tile * ((size_t)A_pad + (size_t)K * A + K));
}

void mil_heads_launch_pool(const float* feats, const int32_t* rows, const int32_t* bag_of, const float* a, int n, int F, int K,
                           int ntiles, float* part, hipStream_t s) {
  mil_for_count<kMhMaxHeads>(K, [&](auto kk) {
    hipLaunchKernelGGL(mh_pool_kernel<decltype(kk)::value>, dim3(ntiles), dim3(256), 0, s, feats, rows, bag_of, a, n, F, part);
  });
}

// the forward up to the pooled vectors, shared by inference and the step: bag_of, H, a [n][K], pooled [n_bags][K F]
static void mil_heads_pool(const hipac_mil_params_t* p, int K, const float* feats, const int32_t* rows, const int32_t* bag_offsets,
                           int n, int n_bags, const MilHeadPlan& q, char* ws, float* a, float* pooled, hipStream_t s) {
  const int F = p->feature_dim, A = p->attn_dim;
  int32_t* bag_of = (int32_t*)(ws + q.bag_of);
  float* H = (float*)(ws + q.H);
  float* scores = (float*)(ws + q.scores);
  float* part = (float*)(ws + q.part);
  mil_train_launch_bag_of(bag_offsets, n_bags, n, bag_of, s);
  mil_train_launch_h(feats, rows, n, F, p->attn_V_w, p->attn_V_b, A, q.A_pad, H, s);
  mil_for_count<kMhMaxHeads>(K, [&](auto kk) {
    hipLaunchKernelGGL(mh_score_kernel<decltype(kk)::value>, dim3((n + 15) / 16), dim3(256), 0, s, (const float*)H, n, A, q.A_pad,
                       p->attn_U_w, p->attn_U_b, scores);
  });
  hipLaunchKernelGGL(mh_softmax_kernel, dim3(n_bags, K), dim3(256), 0, s, (const float*)scores, bag_offsets, K, a);
  mil_heads_launch_pool(feats, rows, bag_of, a, n, F, K, q.ntiles, part, s);
  mil_train_launch_pool_combine(part, bag_offsets, n_bags, K * F, pooled, s);
}

}  // namespace hipac

using namespace hipac;

extern "C" {

int hipac_mil_heads_abi_version(void) { return HIPAC_MIL_HEADS_ABI_VERSION; }

size_t hipac_mil_heads_forward_workspace_bytes(const hipac_mil_params_t* params, int heads, int n, int n_bags) {
  return mil_heads_dims_ok(params, heads, n, n_bags) ? make_mil_head_plan(params, heads, n, n_bags, 1, heads, false).total : 0;
}

size_t hipac_mil_heads_train_workspace_bytes(const hipac_mil_params_t* params, int heads, int n, int n_bags) {
  return mil_heads_dims_ok(params, heads, n, n_bags) ? make_mil_head_plan(params, heads, n, n_bags, 1, heads, true).total : 0;
}

int hipac_mil_heads_forward(const hipac_mil_params_t* p, int heads, const float* feats, const int32_t* bag_offsets, int n,
                            int n_bags, float* logits, float* attn, float* pooled, void* workspace, size_t workspace_bytes,
                            void* stream) {
  const int rc = mil_check_forward_args("mil_heads_forward", p && feats && bag_offsets && logits && workspace, "heads", heads,
                                        kMhMaxHeads, p, true, n, n_bags, feats, workspace);
  if (rc) return rc;
  const MilHeadPlan q = make_mil_head_plan(p, heads, n, n_bags, 1, heads, false);
  HIPAC_REQUIRE(workspace_bytes >= q.total, HIPAC_EWORKSPACE, "mil_heads_forward: workspace %zu bytes, %zu needed", workspace_bytes,
                q.total);
  char* ws = (char*)workspace;
  float* a = attn ? attn : (float*)(ws + q.attn);
  float* pl = pooled ? pooled : (float*)(ws + q.pooled);
  mil_heads_pool(p, heads, feats, nullptr, bag_offsets, n, n_bags, q, ws, a, pl, (hipStream_t)stream);
  HIPAC_CHECK_HIP(hipGetLastError());
  return mil_classifier_forward(p, pl, heads * p->feature_dim, n_bags, (float*)(ws + q.hid), logits, stream);
}

int hipac_mil_heads_train_fwd_bwd(const hipac_mil_params_t* p, int heads, const float* feats, int n_feat_rows, const int32_t* rows,
                                  const int32_t* bag_offsets, int n, int n_bags, const int64_t* labels, const float* class_w,
                                  const hipac_mil_params_t* grads, float* loss, float* logits, float* attn, void* workspace,
                                  size_t workspace_bytes, int accumulate, void* stream) {
  int rc = mil_check_train_args("mil_heads_train_fwd_bwd", p && feats && bag_offsets && labels && grads && loss && logits && workspace,
                                "heads", heads, kMhMaxHeads, p, grads, true, true, n, n_bags, n_feat_rows, rows != nullptr, feats,
                                workspace);
  if (rc) return rc;
  const MilHeadPlan q = make_mil_head_plan(p, heads, n, n_bags, 1, heads, true);
  HIPAC_REQUIRE(workspace_bytes >= q.total, HIPAC_EWORKSPACE, "mil_heads_train_fwd_bwd: workspace %zu bytes, %zu needed",
                workspace_bytes, q.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int F = p->feature_dim, A = p->attn_dim, B = n_bags, K = heads;
  float* pooled = (float*)(ws + q.pooled);
  float* g = (float*)(ws + q.g);
  float* a = attn ? attn : (float*)(ws + q.attn);
  float* cdot = (float*)(ws + q.cdot);

  mil_heads_pool(p, K, feats, rows, bag_offsets, n, B, q, ws, a, pooled, s);
  HIPAC_CHECK_HIP(hipGetLastError());
  // classifier.0 over the K F pooled columns + ReLU, classifier.2, cross-entropy, and their backward
  rc = mil_classifier_fwd_bwd(p, grads, K * F, B, labels, class_w, loss, logits, q, ws, true, accumulate, stream, nullptr, nullptr);
  if (rc) return rc;
  // pooled and g are [B K][F]: cdot[b][k] = M[b][k] . g[b][k]
  mil_train_launch_cdot(pooled, g, F, B * K, cdot, s);
  mil_for_count<kMhMaxHeads>(K, [&](auto kk) {
    hipLaunchKernelGGL(mh_ds_kernel<decltype(kk)::value>, dim3(q.ntiles), dim3(256), 0, s, feats, rows, (const int32_t*)(ws + q.bag_of),
                       (const float*)a, (const float*)g, (const float*)cdot, p->attn_U_w, (float*)(ws + q.H), n, F, A, q.A_pad,
                       (float*)(ws + q.part2));
  });
  mil_head_launch_grads(grads, K, feats, rows, n, F, A, q, ws, accumulate, s);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"

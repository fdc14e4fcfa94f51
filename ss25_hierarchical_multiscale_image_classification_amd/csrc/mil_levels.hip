// Multiscale attention pooling for the MIL head (include/hipac_mil_levels.h): a bag holds rows of L pyramid levels, every
// level has its own attention branch over the shared hidden layer and its own softmax inside the bag, fp32.
//
//   H = tanh(X V^T + b_V) [n][A]   s_i = U[lev(i)] . H_i + b_U[lev(i)]   a_i = softmax of s over the rows of the same (bag, level)
//   M[b][k] = sum_{lev(i) = k} a_i x_i    pooled_b = (M[b][0] | .. | M[b][L-1])    logits = classifier(pooled)
//   backward (g[b][k] = dL/dM[b][k]):  ds_i = a_i (x_i . g[b][lev(i)] - M[b][lev(i)] . g[b][lev(i)]),
//   dH_i = ds_i U[lev(i)] (1 - H_i^2) in place over H, dV = dH^T X, db_V = sum dH_i, dU[k] = sum_{lev(i) = k} ds_i H_i,
//   db_U[k] = sum_{lev(i) = k} ds_i.
//
// Algebraically the L-head model of mil_heads.hip with the scores of a row at minus infinity in the heads of the other levels;
// but a row belongs to ONE level, so its score, its pooling FMA, its row dot product and its ds U product are formed once here
// where a masked L-head step forms them L times to produce zeros.  X V^T, dV = dH^T X, the row -> bag map, the per-bag
// combination of the pooling segments (over L F columns), the M . g products (over B L rows) and the fixed-order slab sums are
// mil_train.hip's, launched through mil_train_internal.h as mil_heads.hip launches them; the workspace plan (with scores and
// attn one column wide), the argument checks, the classifier chain and the end of the step (db_V | dU | db_U | dV) are that
// header's as well, the reductions inside the kernels wave_reduce.h's.  Here: the ml_ kernels, the forward up to the pooled
// vectors and the two entry points.  The tiling and the segment scheme are
// mil_train.hip's: 64 rows per tile whatever the bag boundaries, segment (tile t, bag b) = id t + b; no float atomics.
// The level of a row is uniform over the wave (pooling: over the workgroup) that handles it, so the per-level accumulators are
// picked by a uniform switch over registers, never by a dynamic index.  A level_of value >= L is a row of no level: it is
// skipped before anything is indexed with it.
#include "common.h"

#include "../../include/hipac_mil_levels.h"
#include "mil_device.h"
#include "mil_train_internal.h"
#include "wave_reduce.h"

namespace hipac {

constexpr int kMlTile = 64;  // rows per tile: mil_train.hip's kMtTile (mil_train_launch_pool_combine assumes it)
constexpr int kMlMaxLevels = HIPAC_MIL_MAX_LEVELS;

static bool mil_levels_dims_ok(const hipac_mil_params_t* p, int levels, int n, int n_bags) {
  return levels >= 1 && levels <= kMlMaxLevels && mil_train_sizes_ok(p, n, n_bags);
}

// s_i = U[lev(i)] . H_i + b_U[lev(i)]: one wave per row, 16 rows per workgroup, one dot product per row.  U is L A floats and
// stays in the cache; a row of no level gets the score 0, which nothing reads
__global__ __launch_bounds__(256) void ml_score_kernel(const float* __restrict__ H, const uint8_t* __restrict__ level_of, int n, int A,
                                                       int A_pad, int L, const float* __restrict__ Uw, const float* __restrict__ Ub,
                                                       float* __restrict__ scores) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int rr = wave; rr < 16; rr += 4) {
    const int i = blockIdx.x * 16 + rr;
    if (i >= n) break;
    const int lev = level_of[i];
    if (lev >= L) {
      if (lane == 0) scores[i] = 0.f;
      continue;
    }
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = lane + 64 * q;
      if (j < A) v = fmaf(Uw[lev * A + j], H[(size_t)i * A_pad + j], v);
    }
    v = wave_sum(v);
    if (lane == 0) scores[i] = v + Ub[lev];
  }
}

// softmax over the rows of level k inside bag b: one workgroup per (bag, level), the rows taken in row order.  An empty
// (bag, level) has z = 0 (a level with a row has z >= 1: its largest score adds exp(0)) and writes nothing.  The workgroups of
// level 0 also write the 0 of the rows of no level
__global__ __launch_bounds__(256) void ml_softmax_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ level_of,
                                                         const int32_t* __restrict__ offs, int L, float* __restrict__ attn) {
  __shared__ float red[4];
  const int b = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  const int o0 = offs[b], o1 = offs[b + 1];
  float mx = -INFINITY;
  for (int i = o0 + tid; i < o1; i += 256) {
    const int lev = level_of[i];
    if (lev == k) mx = fmaxf(mx, scores[i]);
    if (k == 0 && lev >= L) attn[i] = 0.f;
  }
  const float m = block_max_tree<4>(mx, red);
  float z = 0.f;
  for (int i = o0 + tid; i < o1; i += 256)
    if (level_of[i] == k) z += expf(scores[i] - m);
  z = block_sum_tree<4>(z, red);
  if (!(z > 0.f)) return;  // the same z in every thread
  const float inv = 1.f / z;
  for (int i = o0 + tid; i < o1; i += 256)
    if (level_of[i] == k) attn[i] = expf(scores[i] - m) * inv;
}

template <int L, int K>
__device__ __forceinline__ void ml_pool_fma(f32x4 (&acc)[L], float a, const f32x4& x) {
  if constexpr (K < L) {
    acc[K][0] = fmaf(a, x[0], acc[K][0]), acc[K][1] = fmaf(a, x[1], acc[K][1]);
    acc[K][2] = fmaf(a, x[2], acc[K][2]), acc[K][3] = fmaf(a, x[3], acc[K][3]);
  }
}

// pooling partials: tile t of 64 rows -> part[t + b][L][F] for every bag b it holds.  A lane owns four feature columns and
// keeps one f32x4 accumulator per level; a row does one FMA per column, into the accumulator of its level (the level is the
// same in the whole workgroup: a uniform switch).  Every level of a segment is written, zeros where it has no row
template <int L>
__global__ __launch_bounds__(256) void ml_pool_kernel(const float* __restrict__ feats, const int32_t* __restrict__ rows,
                                                      const int32_t* __restrict__ bag_of, const uint8_t* __restrict__ level_of,
                                                      const float* __restrict__ w, int n, int F, float* __restrict__ part) {
  __shared__ int sb[kMlTile];
  __shared__ int sro[kMlTile];
  __shared__ int slev[kMlTile];
  __shared__ float sw[kMlTile];
  const int tile = blockIdx.x, tid = threadIdx.x;
  const int r0 = tile * kMlTile;
  const int cnt = n - r0 < kMlTile ? n - r0 : kMlTile;
  if (tid < cnt) {
    sb[tid] = bag_of[r0 + tid];
    sro[tid] = rows ? rows[r0 + tid] : r0 + tid;
    slev[tid] = level_of[r0 + tid];
    sw[tid] = w[r0 + tid];
  }
  __syncthreads();
  const int F4 = F / 4;
  const f32x4* x4 = reinterpret_cast<const f32x4*>(feats);
  f32x4* p4 = reinterpret_cast<f32x4*>(part);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int c = tid; c < F4; c += 256) {
    f32x4 acc[L];
#pragma unroll
    for (int k = 0; k < L; ++k) acc[k] = zero;
    int cur = sb[0];
    for (int i = 0; i < cnt; ++i) {
      const int b = sb[i];
      if (b != cur) {
#pragma unroll
        for (int k = 0; k < L; ++k) p4[((size_t)(tile + cur) * L + k) * F4 + c] = acc[k], acc[k] = zero;
        cur = b;
      }
      const int lev = slev[i];
      if (lev >= L) continue;  // a row of no level: not even loaded
      const f32x4 x = x4[(size_t)sro[i] * F4 + c];
      const float a = sw[i];
      switch (lev) {
        case 0: ml_pool_fma<L, 0>(acc, a, x); break;
        case 1: ml_pool_fma<L, 1>(acc, a, x); break;
        case 2: ml_pool_fma<L, 2>(acc, a, x); break;
        default: ml_pool_fma<L, 3>(acc, a, x); break;
      }
    }
#pragma unroll
    for (int k = 0; k < L; ++k) p4[((size_t)(tile + cur) * L + k) * F4 + c] = acc[k];
  }
}

// the row of level K: H_i becomes dH_i = ds U[K] (1 - H_i^2) in place, sum dH_i and sum ds H_i (into level K's block) grow
template <int L, int K>
__device__ __forceinline__ void ml_ds_row(float ds, const float (&u)[L][4], float (&accU)[L][4], float (&accB)[L], float (&accV)[4],
                                          float* __restrict__ hrow, int lane, int A, int A_pad) {
  if constexpr (K < L) {
    accB[K] += ds;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = lane + 64 * q;
      if (j < A_pad) {
        const float hv = j < A ? hrow[j] : 0.f;
        const float dh = ds * u[K][q] * (1.f - hv * hv);
        hrow[j] = dh;
        accV[q] += dh;
        accU[K][q] = fmaf(ds, hv, accU[K][q]);
      }
    }
  }
}

// one sweep over the rows of a tile.  A wave takes rows wave, wave + 4, ...; it reads x_i once and forms the ONE product
// x_i . g[b][lev(i)] (g is n_bags L F floats, cache resident), then ds_i = a_i (x_i . g[b][lev(i)] - cdot[b][lev(i)]); H_i
// becomes dH_i = ds_i U[lev(i)] (1 - H_i^2) in place (zeros for a row of no level, whose x_i is not read); the tile's column
// sums go to part2[tile] = (sum dH_i [A_pad] | sum ds_i H_i routed into [L][A] | sum ds_i routed into [L])
template <int L>
__global__ __launch_bounds__(256) void ml_ds_kernel(const float* __restrict__ feats, const int32_t* __restrict__ rows,
                                                    const int32_t* __restrict__ bag_of, const uint8_t* __restrict__ level_of,
                                                    const float* __restrict__ attn, const float* __restrict__ g,
                                                    const float* __restrict__ cdot, const float* __restrict__ Uw, float* __restrict__ H,
                                                    int n, int F, int A, int A_pad, float* __restrict__ part2) {
  constexpr int RED = 256 * (L + 1) + L;
  __shared__ float red[4][RED];
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float accV[4] = {0.f, 0.f, 0.f, 0.f}, accU[L][4], accB[L], u[L][4];
#pragma unroll
  for (int k = 0; k < L; ++k) {
    accB[k] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) accU[k][q] = 0.f, u[k][q] = lane + 64 * q < A ? Uw[k * A + lane + 64 * q] : 0.f;
  }
  const int F4 = F / 4;
  for (int rr = wave; rr < kMlTile; rr += 4) {
    const int i = tile * kMlTile + rr;
    if (i >= n) break;
    const int lev = level_of[i];
    float* hrow = H + (size_t)i * A_pad;
    if (lev >= L) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (lane + 64 * q < A_pad) hrow[lane + 64 * q] = 0.f;
      continue;
    }
    const int b = bag_of[i];
    const f32x4* x = reinterpret_cast<const f32x4*>(feats + (size_t)(rows ? rows[i] : i) * F);
    const f32x4* gb = reinterpret_cast<const f32x4*>(g + ((size_t)b * L + lev) * F);
    float t = 0.f;
    for (int c = lane; c < F4; c += 64) {
      const f32x4 xv = x[c], gv = gb[c];
      t = fmaf(xv[0], gv[0], t), t = fmaf(xv[1], gv[1], t), t = fmaf(xv[2], gv[2], t), t = fmaf(xv[3], gv[3], t);
    }
    const float ds = attn[i] * (wave_sum(t) - cdot[b * L + lev]);
    switch (lev) {
      case 0: ml_ds_row<L, 0>(ds, u, accU, accB, accV, hrow, lane, A, A_pad); break;
      case 1: ml_ds_row<L, 1>(ds, u, accU, accB, accV, hrow, lane, A, A_pad); break;
      case 2: ml_ds_row<L, 2>(ds, u, accU, accB, accV, hrow, lane, A, A_pad); break;
      default: ml_ds_row<L, 3>(ds, u, accU, accB, accV, hrow, lane, A, A_pad); break;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    red[wave][64 * q + lane] = accV[q];
#pragma unroll
    for (int k = 0; k < L; ++k) red[wave][256 * (k + 1) + 64 * q + lane] = accU[k][q];
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < L; ++k) red[wave][256 * (L + 1) + k] = accB[k];
  }
  __syncthreads();
  mil_store_part2<L, 1>(red, A, A_pad, tid, part2 + (size_t)tile * ((size_t)A_pad + (size_t)L * A + L));
}

// the forward up to the pooled vectors, shared by inference and the step: bag_of, H, a [n], pooled [n_bags][L F]
static void mil_levels_pool(const hipac_mil_params_t* p, int L, const float* feats, const int32_t* rows, const uint8_t* level_of,
                            const int32_t* bag_offsets, int n, int n_bags, const MilHeadPlan& q, char* ws, float* a, float* pooled,
                            hipStream_t s) {
  const int F = p->feature_dim, A = p->attn_dim;
  int32_t* bag_of = (int32_t*)(ws + q.bag_of);
  float* H = (float*)(ws + q.H);
  float* scores = (float*)(ws + q.scores);
  float* part = (float*)(ws + q.part);
  mil_train_launch_bag_of(bag_offsets, n_bags, n, bag_of, s);
  mil_train_launch_h(feats, rows, n, F, p->attn_V_w, p->attn_V_b, A, q.A_pad, H, s);
  hipLaunchKernelGGL(ml_score_kernel, dim3((n + 15) / 16), dim3(256), 0, s, (const float*)H, level_of, n, A, q.A_pad, L, p->attn_U_w,
                     p->attn_U_b, scores);
  hipLaunchKernelGGL(ml_softmax_kernel, dim3(n_bags, L), dim3(256), 0, s, (const float*)scores, level_of, bag_offsets, L, a);
  mil_for_count<kMlMaxLevels>(L, [&](auto ll) {
    hipLaunchKernelGGL(ml_pool_kernel<decltype(ll)::value>, dim3(q.ntiles), dim3(256), 0, s, feats, rows, (const int32_t*)bag_of,
                       level_of, (const float*)a, n, F, part);
  });
  mil_train_launch_pool_combine(part, bag_offsets, n_bags, L * F, pooled, s);
}

}  // namespace hipac

using namespace hipac;

extern "C" {

int hipac_mil_levels_abi_version(void) { return HIPAC_MIL_LEVELS_ABI_VERSION; }

size_t hipac_mil_levels_forward_workspace_bytes(const hipac_mil_params_t* params, int levels, int n, int n_bags) {
  return mil_levels_dims_ok(params, levels, n, n_bags) ? make_mil_head_plan(params, levels, n, n_bags, 1, 1, false).total : 0;
}

size_t hipac_mil_levels_train_workspace_bytes(const hipac_mil_params_t* params, int levels, int n, int n_bags) {
  return mil_levels_dims_ok(params, levels, n, n_bags) ? make_mil_head_plan(params, levels, n, n_bags, 1, 1, true).total : 0;
}

int hipac_mil_levels_forward(const hipac_mil_params_t* p, int levels, const float* feats, const uint8_t* level_of,
                             const int32_t* bag_offsets, int n, int n_bags, float* logits, float* attn, float* pooled, void* workspace,
                             size_t workspace_bytes, void* stream) {
  const int rc = mil_check_forward_args("mil_levels_forward", p && feats && level_of && bag_offsets && logits && workspace, "levels",
                                        levels, kMlMaxLevels, p, true, n, n_bags, feats, workspace);
  if (rc) return rc;
  const MilHeadPlan q = make_mil_head_plan(p, levels, n, n_bags, 1, 1, false);
  HIPAC_REQUIRE(workspace_bytes >= q.total, HIPAC_EWORKSPACE, "mil_levels_forward: workspace %zu bytes, %zu needed", workspace_bytes,
                q.total);
  char* ws = (char*)workspace;
  float* a = attn ? attn : (float*)(ws + q.attn);
  float* pl = pooled ? pooled : (float*)(ws + q.pooled);
  mil_levels_pool(p, levels, feats, nullptr, level_of, bag_offsets, n, n_bags, q, ws, a, pl, (hipStream_t)stream);
  HIPAC_CHECK_HIP(hipGetLastError());
  return mil_classifier_forward(p, pl, levels * p->feature_dim, n_bags, (float*)(ws + q.hid), logits, stream);
}

int hipac_mil_levels_train_fwd_bwd(const hipac_mil_params_t* p, int levels, const float* feats, int n_feat_rows, const int32_t* rows,
                                   const uint8_t* level_of, const int32_t* bag_offsets, int n, int n_bags, const int64_t* labels,
                                   const float* class_w, const hipac_mil_params_t* grads, float* loss, float* logits, float* attn,
                                   void* workspace, size_t workspace_bytes, int accumulate, void* stream) {
  int rc = mil_check_train_args("mil_levels_train_fwd_bwd",
                                p && feats && level_of && bag_offsets && labels && grads && loss && logits && workspace, "levels", levels,
                                kMlMaxLevels, p, grads, true, true, n, n_bags, n_feat_rows, rows != nullptr, feats, workspace);
  if (rc) return rc;
  const MilHeadPlan q = make_mil_head_plan(p, levels, n, n_bags, 1, 1, true);
  HIPAC_REQUIRE(workspace_bytes >= q.total, HIPAC_EWORKSPACE, "mil_levels_train_fwd_bwd: workspace %zu bytes, %zu needed",
                workspace_bytes, q.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int F = p->feature_dim, A = p->attn_dim, B = n_bags, L = levels;
  float* pooled = (float*)(ws + q.pooled);
  float* g = (float*)(ws + q.g);
  float* a = attn ? attn : (float*)(ws + q.attn);
  float* cdot = (float*)(ws + q.cdot);

  mil_levels_pool(p, L, feats, rows, level_of, bag_offsets, n, B, q, ws, a, pooled, s);
  HIPAC_CHECK_HIP(hipGetLastError());
  // classifier.0 over the L F pooled columns + ReLU, classifier.2, cross-entropy, and their backward
  rc = mil_classifier_fwd_bwd(p, grads, L * F, B, labels, class_w, loss, logits, q, ws, true, accumulate, stream, nullptr, nullptr);
  if (rc) return rc;
  // pooled and g are [B L][F]: cdot[b][k] = M[b][k] . g[b][k]
  mil_train_launch_cdot(pooled, g, F, B * L, cdot, s);
  mil_for_count<kMlMaxLevels>(L, [&](auto ll) {
    hipLaunchKernelGGL(ml_ds_kernel<decltype(ll)::value>, dim3(q.ntiles), dim3(256), 0, s, feats, rows, (const int32_t*)(ws + q.bag_of),
                       level_of, (const float*)a, (const float*)g, (const float*)cdot, p->attn_U_w, (float*)(ws + q.H), n, F, A, q.A_pad,
                       (float*)(ws + q.part2));
  });
  mil_head_launch_grads(grads, L, feats, rows, n, F, A, q, ws, accumulate, s);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"

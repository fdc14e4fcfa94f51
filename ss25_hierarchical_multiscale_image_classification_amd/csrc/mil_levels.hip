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
// mil_train.hip's, launched through mil_train_internal.h as mil_heads.hip launches them.  The tiling and the segment scheme are
// mil_train.hip's: 64 rows per tile whatever the bag boundaries, segment (tile t, bag b) = id t + b; no float atomics.
// The level of a row is uniform over the wave (pooling: over the workgroup) that handles it, so the per-level accumulators are
// picked by a uniform switch over registers, never by a dynamic index.  A level_of value >= L is a row of no level: it is
// skipped before anything is indexed with it.
#include "common.h"

#include "../../include/hipac_mil_levels.h"
#include "mil_train_internal.h"

namespace hipac {

constexpr int kMlTile = 64;  // rows per tile: mil_train.hip's kMtTile (mil_train_launch_pool_combine assumes it)
constexpr int kMlMaxLevels = HIPAC_MIL_MAX_LEVELS;

struct MilLevelsPlan {
  int A_pad, ntiles, nseg, chunk, slices;
  size_t P2;  // floats of one tile's column sums: sum dH_i [A_pad] | sum ds_i H_i routed into [L][A] | sum ds_i routed into [L]
  size_t bag_of, pooled, hid, dhid, dym, dlogits, g, ce, cdot, part, scores, attn, H, part2, slab, total;
};

static bool mil_levels_dims_ok(const hipac_mil_params_t* p, int levels, int n, int n_bags) {
  return levels >= 1 && levels <= kMlMaxLevels && mil_train_sizes_ok(p, n, n_bags);
}

static MilLevelsPlan make_mil_levels_plan(const hipac_mil_params_t* p, int levels, int n, int n_bags, bool train) {
  MilLevelsPlan q{};
  const size_t F = p->feature_dim, A = p->attn_dim, Hd = p->hidden_dim, Cn = p->num_classes, B = n_bags, L = levels;
  q.A_pad = (p->attn_dim + 31) / 32 * 32;
  q.ntiles = (n + kMlTile - 1) / kMlTile;
  q.nseg = q.ntiles + n_bags;
  q.P2 = (size_t)q.A_pad + L * A + L;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align256(bytes);
    return at;
  };
  q.bag_of = take((size_t)n * 4);
  q.pooled = take(B * L * F * 4);
  q.hid = take(B * Hd * 4);
  q.part = take((size_t)q.nseg * L * F * 4);
  q.scores = take((size_t)n * 4);
  q.attn = take((size_t)n * 4);
  q.H = take((size_t)n * q.A_pad * 4);
  if (train) {
    mil_train_dv_slices(n, p->feature_dim, &q.chunk, &q.slices);
    q.dhid = take(B * Hd * 4);
    q.dym = take(B * Hd * 4);
    q.dlogits = take(B * Cn * 4);
    q.g = take(B * L * F * 4);
    q.ce = take((2 + 8 * ((B + 255) / 256)) * 4);
    q.cdot = take(B * L * 4);
    q.part2 = take((size_t)q.ntiles * q.P2 * 4);
    q.slab = take((size_t)q.slices * A * F * 4);
  }
  q.total = o;
  return q;
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
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) scores[i] = v + Ub[lev];
  }
}

__device__ __forceinline__ float ml_block_reduce(float v, bool is_max, float* red) {
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
  const float m = ml_block_reduce(mx, true, red);
  float z = 0.f;
  for (int i = o0 + tid; i < o1; i += 256)
    if (level_of[i] == k) z += expf(scores[i] - m);
  z = ml_block_reduce(z, false, red);
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
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    const float ds = attn[i] * (t - cdot[b * L + lev]);
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
  float* out = part2 + (size_t)tile * ((size_t)A_pad + (size_t)L * A + L);
  for (int e = tid; e < RED; e += 256) {
    const float s = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
    const int blk = e >> 8, j = e & 255;
    if (blk == 0) {
      if (j < A_pad) out[j] = s;
    } else if (blk <= L) {
      if (j < A) out[A_pad + (blk - 1) * A + j] = s;
    } else {
      out[A_pad + L * A + j] = s;
    }
  }
}

#define ML_FOR_LEVELS(levels, CALL) \
  switch (levels) {                 \
    case 1: CALL(1); break;         \
    case 2: CALL(2); break;         \
    case 3: CALL(3); break;         \
    default: CALL(4); break;        \
  }

// the forward up to the pooled vectors, shared by inference and the step: bag_of, H, a [n], pooled [n_bags][L F]
static void mil_levels_pool(const hipac_mil_params_t* p, int L, const float* feats, const int32_t* rows, const uint8_t* level_of,
                            const int32_t* bag_offsets, int n, int n_bags, const MilLevelsPlan& q, char* ws, float* a, float* pooled,
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
#define ML_POOL(LL)                                                                                                                 \
  hipLaunchKernelGGL(ml_pool_kernel<LL>, dim3(q.ntiles), dim3(256), 0, s, feats, rows, (const int32_t*)bag_of, level_of, (const float*)a, \
                     n, F, part)
  ML_FOR_LEVELS(L, ML_POOL)
#undef ML_POOL
  mil_train_launch_pool_combine(part, bag_offsets, n_bags, L * F, pooled, s);
}

}  // namespace hipac

using namespace hipac;

extern "C" {

int hipac_mil_levels_abi_version(void) { return HIPAC_MIL_LEVELS_ABI_VERSION; }

size_t hipac_mil_levels_forward_workspace_bytes(const hipac_mil_params_t* params, int levels, int n, int n_bags) {
  return mil_levels_dims_ok(params, levels, n, n_bags) ? make_mil_levels_plan(params, levels, n, n_bags, false).total : 0;
}

size_t hipac_mil_levels_train_workspace_bytes(const hipac_mil_params_t* params, int levels, int n, int n_bags) {
  return mil_levels_dims_ok(params, levels, n, n_bags) ? make_mil_levels_plan(params, levels, n, n_bags, true).total : 0;
}

int hipac_mil_levels_forward(const hipac_mil_params_t* p, int levels, const float* feats, const uint8_t* level_of,
                             const int32_t* bag_offsets, int n, int n_bags, float* logits, float* attn, float* pooled, void* workspace,
                             size_t workspace_bytes, void* stream) {
  HIPAC_REQUIRE(p && feats && level_of && bag_offsets && logits && workspace, HIPAC_EINVAL, "mil_levels_forward: null argument");
  HIPAC_REQUIRE(levels >= 1 && levels <= kMlMaxLevels, HIPAC_EINVAL, "mil_levels_forward: levels %d (1..%d)", levels, kMlMaxLevels);
  HIPAC_REQUIRE(mil_levels_dims_ok(p, levels, n, n_bags), HIPAC_EINVAL,
                "mil_levels_forward: n %d, n_bags %d, feature_dim %d, attn_dim %d, hidden_dim %d, num_classes %d", n, n_bags,
                p->feature_dim, p->attn_dim, p->hidden_dim, p->num_classes);
  HIPAC_REQUIRE(p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b, HIPAC_EINVAL, "mil_levels_forward: classifier weights missing");
  HIPAC_REQUIRE(p->attn_V_w && p->attn_V_b && p->attn_U_w && p->attn_U_b, HIPAC_EINVAL, "mil_levels_forward: attention weights missing");
  HIPAC_REQUIRE(((uintptr_t)feats & 15) == 0 && ((uintptr_t)workspace & 15) == 0, HIPAC_EINVAL,
                "mil_levels_forward: feats / workspace must be 16-byte aligned");
  const MilLevelsPlan q = make_mil_levels_plan(p, levels, n, n_bags, false);
  HIPAC_REQUIRE(workspace_bytes >= q.total, HIPAC_EWORKSPACE, "mil_levels_forward: workspace %zu bytes, %zu needed", workspace_bytes,
                q.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* a = attn ? attn : (float*)(ws + q.attn);
  float* pl = pooled ? pooled : (float*)(ws + q.pooled);
  float* hid = (float*)(ws + q.hid);
  mil_levels_pool(p, levels, feats, nullptr, level_of, bag_offsets, n, n_bags, q, ws, a, pl, s);
  HIPAC_CHECK_HIP(hipGetLastError());
  int rc = hipac_linear_forward(pl, p->fc1_w, p->fc1_b, hid, n_bags, p->hidden_dim, levels * p->feature_dim, 1, stream);
  if (rc) return rc;
  return hipac_linear_forward(hid, p->fc2_w, p->fc2_b, logits, n_bags, p->num_classes, p->hidden_dim, 0, stream);
}

int hipac_mil_levels_train_fwd_bwd(const hipac_mil_params_t* p, int levels, const float* feats, int n_feat_rows, const int32_t* rows,
                                   const uint8_t* level_of, const int32_t* bag_offsets, int n, int n_bags, const int64_t* labels,
                                   const float* class_w, const hipac_mil_params_t* grads, float* loss, float* logits, float* attn,
                                   void* workspace, size_t workspace_bytes, int accumulate, void* stream) {
  HIPAC_REQUIRE(p && feats && level_of && bag_offsets && labels && grads && loss && logits && workspace, HIPAC_EINVAL,
                "mil_levels_train_fwd_bwd: null argument");
  HIPAC_REQUIRE(levels >= 1 && levels <= kMlMaxLevels, HIPAC_EINVAL, "mil_levels_train_fwd_bwd: levels %d (1..%d)", levels,
                kMlMaxLevels);
  HIPAC_REQUIRE(mil_levels_dims_ok(p, levels, n, n_bags), HIPAC_EINVAL,
                "mil_levels_train_fwd_bwd: n %d, n_bags %d, feature_dim %d, attn_dim %d, hidden_dim %d, num_classes %d", n, n_bags,
                p->feature_dim, p->attn_dim, p->hidden_dim, p->num_classes);
  HIPAC_REQUIRE(n_feat_rows > 0 && (rows || n <= n_feat_rows), HIPAC_EINVAL, "mil_levels_train_fwd_bwd: n_feat_rows %d for n %d rows",
                n_feat_rows, n);
  HIPAC_REQUIRE(p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b && grads->fc1_w && grads->fc1_b && grads->fc2_w && grads->fc2_b,
                HIPAC_EINVAL, "mil_levels_train_fwd_bwd: classifier weights or their gradient buffers missing");
  HIPAC_REQUIRE(p->attn_V_w && p->attn_V_b && p->attn_U_w && p->attn_U_b && grads->attn_V_w && grads->attn_V_b && grads->attn_U_w &&
                    grads->attn_U_b,
                HIPAC_EINVAL, "mil_levels_train_fwd_bwd: attention weights or their gradient buffers missing");
  HIPAC_REQUIRE(((uintptr_t)feats & 15) == 0 && ((uintptr_t)workspace & 15) == 0, HIPAC_EINVAL,
                "mil_levels_train_fwd_bwd: feats / workspace must be 16-byte aligned");
  const MilLevelsPlan q = make_mil_levels_plan(p, levels, n, n_bags, true);
  HIPAC_REQUIRE(workspace_bytes >= q.total, HIPAC_EWORKSPACE, "mil_levels_train_fwd_bwd: workspace %zu bytes, %zu needed",
                workspace_bytes, q.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int F = p->feature_dim, A = p->attn_dim, Hd = p->hidden_dim, Cn = p->num_classes, B = n_bags, L = levels;
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

  mil_levels_pool(p, L, feats, rows, level_of, bag_offsets, n, B, q, ws, a, pooled, s);
  HIPAC_CHECK_HIP(hipGetLastError());
  // classifier.0 over the L F pooled columns + ReLU, classifier.2, cross-entropy, and their backward: hipac.h's entry points
  int rc = hipac_linear_forward(pooled, p->fc1_w, p->fc1_b, hid, B, Hd, L * F, 1, stream);
  if (rc) return rc;
  rc = hipac_linear_forward(hid, p->fc2_w, p->fc2_b, logits, B, Cn, Hd, 0, stream);
  if (rc) return rc;
  rc = hipac_cross_entropy_fwd_bwd(logits, labels, class_w, B, Cn, loss, dlogits, (float*)(ws + q.ce), stream);
  if (rc) return rc;
  rc = hipac_linear_backward(hid, p->fc2_w, dlogits, nullptr, nullptr, dhid, (float*)grads->fc2_w, (float*)grads->fc2_b, B, Cn, Hd,
                             accumulate, stream);
  if (rc) return rc;
  rc = hipac_linear_backward(pooled, p->fc1_w, dhid, hid, dym, g, (float*)grads->fc1_w, (float*)grads->fc1_b, B, Hd, L * F, accumulate,
                             stream);
  if (rc) return rc;
  // pooled and g are [B L][F]: cdot[b][k] = M[b][k] . g[b][k]
  mil_train_launch_cdot(pooled, g, F, B * L, cdot, s);
#define ML_DS(LL)                                                                                                                \
  hipLaunchKernelGGL(ml_ds_kernel<LL>, dim3(q.ntiles), dim3(256), 0, s, feats, rows, (const int32_t*)(ws + q.bag_of), level_of,        \
                     (const float*)a, (const float*)g, (const float*)cdot, p->attn_U_w, H, n, F, A, q.A_pad, part2)
  ML_FOR_LEVELS(L, ML_DS)
#undef ML_DS
  mil_train_launch_slab_reduce(part2, q.ntiles, q.P2, 0, A, (float*)grads->attn_V_b, accumulate, s);
  mil_train_launch_slab_reduce(part2, q.ntiles, q.P2, (size_t)q.A_pad, (long long)L * A, (float*)grads->attn_U_w, accumulate, s);
  mil_train_launch_slab_reduce(part2, q.ntiles, q.P2, (size_t)q.A_pad + (size_t)L * A, L, (float*)grads->attn_U_b, accumulate, s);
  mil_train_launch_dv(H, feats, rows, n, F, A, q.A_pad, q.chunk, q.slices, slab, s);
  const long long total = (long long)A * F;
  mil_train_launch_slab_reduce(slab, q.slices, (size_t)total, 0, total, (float*)grads->attn_V_w, accumulate, s);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"

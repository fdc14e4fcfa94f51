// Lesion detection stage (include/hipac_detect.h): window logits -> tumour probabilities -> per-level cell maps -> fused map ->
// Gaussian smoothing -> non-maximum suppression.  Everything stays in HBM; the caller copies the short detection list back.
//
// Reproducibility is the design constraint: no floating-point atomics, every sum in a fixed order, and the
// build compiles without contraction (-ffp-contract=off, build.py), so a multiply followed by an add rounds twice as numpy does.
//
//   level map   a gather, not a scatter: every window's row index is stored at its cell origin (one writer per origin, plain
//               stores), then a cell walks its K x K candidate origins in raster order and adds in that order.
//   smoothing   two passes of 2R + 1 taps, rows then columns, zeros outside; the taps travel in the kernel arguments.
//   NMS         rounds instead of dependent arg-max launches.  state[c] is LIVE, DEAD or SELECTED.  A live cell is selected when
//               every cell of its radius-r neighbourhood that beats it under (value descending, raster index ascending) is DEAD;
//               it then marks its neighbourhood DEAD.  One kernel per round, and the flags may be read while the same round
//               writes them: SELECTED is only ever written to a cell of the greedy set G and DEAD only to a cell G clears
//               (take the first write that breaks this: a cell outside G that selects itself was cleared by a g in G that beats
//               it, and must have read g as DEAD, which no earlier write can have stored; a cell of G that marks a neighbour
//               marks a cell G clears), so a stale read can only delay a selection to a later round.  A round always selects
//               the largest live cell, so the rounds end; a smooth hill needs about (its radius) / (r + 1) of them.  The host
//               enqueues kNmsRounds rounds -- each returns at once when the previous one selected nothing -- and then one
//               single-block kernel that loops until nothing is selected: it does the rest on flat plateaus, where the
//               tie rule turns the selection into a wave front, and returns at once otherwise.  The selected cells'
//               keys (~value bits, raster index) are sorted ascending by a bitonic network over the padded grid.
#include "common.h"

#include <math.h>

#include "../../include/hipac_detect.h"
#include "detect_prob.h"

namespace hipac {

constexpr int kNmsRounds = 32;  // grid-wide rounds before the single-block finisher
constexpr int kNmsLive = 0, kNmsDead = 1, kNmsSelected = 2;
constexpr uint64_t kNmsNoKey = ~(uint64_t)0;

struct GaussTaps {
  float w[2 * HIPAC_DETECT_MAX_TAPS_R + 1];
};

__global__ __launch_bounds__(256) void detect_probs_kernel(const float* __restrict__ logits, int n, int tumor, float* __restrict__ p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  p[i] = tumor_prob(logits, (size_t)i, tumor);
}

__global__ __launch_bounds__(256) void detect_fill_kernel(int32_t* __restrict__ a, int n, int32_t v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) a[i] = v;
}

__global__ __launch_bounds__(256) void detect_origin_kernel(const int32_t* __restrict__ meta, int n, int level, int stride, int gw,
                                                            int gh, int32_t* __restrict__ origin) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || meta[4 * i] != level) return;
  const int x = meta[4 * i + 1], y = meta[4 * i + 2];
  if (x < 0 || y < 0) return;
  const int cx = x / stride, cy = y / stride;
  if (cx < gw && cy < gh) origin[cy * gw + cx] = i;
}

__global__ __launch_bounds__(256) void detect_gather_kernel(const float* __restrict__ p, const int32_t* __restrict__ origin, int K,
                                                            int gw, int gh, float* __restrict__ map, int32_t* __restrict__ count) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= gw * gh) return;
  const int j = c / gw, i = c - j * gw;
  const int y0 = j - K + 1 > 0 ? j - K + 1 : 0, x0 = i - K + 1 > 0 ? i - K + 1 : 0;
  float sum = 0.0f;
  int cnt = 0;
  for (int oy = y0; oy <= j; ++oy) {
    for (int ox = x0; ox <= i; ++ox) {
      const int w = origin[oy * gw + ox];
      if (w >= 0) {
        sum = sum + p[w];
        ++cnt;
      }
    }
  }
  map[c] = cnt ? sum / (float)cnt : 0.0f;
  count[c] = cnt;
}

__global__ __launch_bounds__(256) void detect_fuse_kernel(const float* __restrict__ maps, const int32_t* __restrict__ counts,
                                                          int n_levels, int N, int mode, float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  float acc = 0.0f;
  int have = 0;
  for (int l = 0; l < n_levels; ++l) {
    if (counts[(size_t)l * N + c] <= 0) continue;
    const float v = maps[(size_t)l * N + c];
    if (mode == HIPAC_DETECT_FUSE_MAX) {
      acc = (have == 0 || v > acc) ? v : acc;
    } else {
      acc = acc + v;
    }
    ++have;
  }
  out[c] = have == 0 ? 0.0f : (mode == HIPAC_DETECT_FUSE_MAX ? acc : acc / (float)have);
}

// one pass of the separable filter along x (step = 1, len = gw) or y (step = gw, len = gh)
__global__ __launch_bounds__(256) void detect_smooth_kernel(const float* __restrict__ in, int gw, int gh, int along_y, GaussTaps taps,
                                                            int R, float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= gw * gh) return;
  const int y = c / gw, x = c - y * gw;
  const int pos = along_y ? y : x, len = along_y ? gh : gw, step = along_y ? gw : 1;
  float acc = 0.0f;
  for (int k = -R; k <= R; ++k) {
    const int q = pos + k;
    const float v = (q >= 0 && q < len) ? in[c + k * step] : 0.0f;
    const float prod = taps.w[k + R] * v;
    acc = acc + prod;
  }
  out[c] = acc;
}

// ---- NMS ------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int st_load(const int* s, int i) { return __hip_atomic_load(s + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_store(int* s, int i, int v) { __hip_atomic_store(s + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ascending key = (value descending, raster index ascending): the float's bits made monotone, inverted, above the index
__device__ __forceinline__ uint64_t nms_key(float v, int c) {
  const uint32_t b = __float_as_uint(v + 0.0f);  // -0 and +0 compare equal: one key for both
  const uint32_t mono = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((uint64_t)(~mono) << 32) | (uint32_t)c;
}

__device__ __forceinline__ float nms_key_value(uint64_t key) {
  const uint32_t mono = ~(uint32_t)(key >> 32);
  return __uint_as_float((mono & 0x80000000u) ? (mono & 0x7fffffffu) : ~mono);
}

__global__ __launch_bounds__(256) void nms_init_kernel(const float* __restrict__ map, unsigned N, unsigned Npad, float threshold,
                                                       int* __restrict__ state, uint64_t* __restrict__ keys, int* __restrict__ progress) {
  const unsigned c = blockIdx.x * 256u + threadIdx.x;
  if (c < (unsigned)kNmsRounds) progress[c] = 0;
  if (c >= Npad) return;
  keys[c] = kNmsNoKey;
  if (c < N) state[c] = map[c] >= threshold ? kNmsLive : kNmsDead;  // NaN compares false: never a detection
}

// one cell of one round; true when the cell selected itself
__device__ __forceinline__ bool nms_try(const float* __restrict__ map, int gw, int gh, int r, int c, int* state, uint64_t* keys) {
  if (st_load(state, c) != kNmsLive) return false;
  const float v = map[c];
  const int j = c / gw, i = c - j * gw;
  const int y0 = j - r > 0 ? j - r : 0, y1 = j + r < gh - 1 ? j + r : gh - 1;
  const int x0 = i - r > 0 ? i - r : 0, x1 = i + r < gw - 1 ? i + r : gw - 1;
  const int r2 = r * r;
  for (int y = y0; y <= y1; ++y) {
    for (int x = x0; x <= x1; ++x) {
      const int n = y * gw + x;
      if ((x - i) * (x - i) + (y - j) * (y - j) > r2 || n == c) continue;
      if (st_load(state, n) == kNmsDead) continue;
      const float vn = map[n];
      if (vn > v || (vn == v && n < c)) return false;  // a live (or selected) cell of the neighbourhood beats this one
    }
  }
  st_store(state, c, kNmsSelected);
  for (int y = y0; y <= y1; ++y) {
    for (int x = x0; x <= x1; ++x) {
      const int n = y * gw + x;
      if ((x - i) * (x - i) + (y - j) * (y - j) <= r2 && n != c) st_store(state, n, kNmsDead);
    }
  }
  keys[c] = nms_key(v, c);
  return true;
}

__global__ __launch_bounds__(256) void nms_round_kernel(const float* __restrict__ map, int gw, int gh, int r, int round, int* state,
                                                        uint64_t* keys, int* progress) {
  if (round > 0 && progress[round - 1] == 0) return;  // the previous round selected nothing: nothing is left
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= gw * gh) return;
  if (nms_try(map, gw, gh, r, c, state, keys)) st_store(progress, round, 1);
}

// whatever kNmsRounds rounds left (plateaus): one block, so that a barrier separates the rounds
__global__ __launch_bounds__(1024) void nms_finish_kernel(const float* __restrict__ map, int gw, int gh, int r, int* state, uint64_t* keys,
                                                          const int* progress) {
  if (progress[kNmsRounds - 1] == 0) return;
  __shared__ int any;
  const int N = gw * gh;
  for (;;) {
    if (threadIdx.x == 0) any = 0;
    __syncthreads();
    bool sel = false;
    for (int c = threadIdx.x; c < N; c += 1024) sel |= nms_try(map, gw, gh, r, c, state, keys);
    if (sel) any = 1;
    __threadfence();
    __syncthreads();
    const bool more = any != 0;
    __syncthreads();
    if (!more) return;
  }
}

// compare-exchange step (k, j) of the bitonic network over n = 2^m keys, ascending
__global__ __launch_bounds__(256) void nms_bitonic_kernel(uint64_t* __restrict__ a, unsigned n, unsigned k, unsigned j) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const unsigned l = i ^ j;
  if (i >= n || l <= i) return;
  const uint64_t x = a[i], y = a[l];
  const bool up = (i & k) == 0;
  if ((x > y) == up) {
    a[i] = y;
    a[l] = x;
  }
}

// M = min(max_detections, padded grid) threads
__global__ __launch_bounds__(256) void nms_emit_kernel(const uint64_t* __restrict__ keys, int M, int gw, float* __restrict__ p,
                                                       int32_t* __restrict__ ij, int32_t* __restrict__ count) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= M) return;
  const uint64_t key = keys[k];
  if (key == kNmsNoKey) {
    if (k == 0) *count = 0;
    return;
  }
  const int c = (int)(uint32_t)key;
  p[k] = nms_key_value(key);
  ij[2 * k] = c % gw;
  ij[2 * k + 1] = c / gw;
  if (k + 1 == M || keys[k + 1] == kNmsNoKey) *count = k + 1;
}

static bool grid_ok(int gw, int gh) { return gw >= 1 && gh >= 1 && (int64_t)gw * gh < ((int64_t)1 << 31); }

static size_t pow2_at_least(size_t n) {
  size_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

static inline dim3 blocks_for(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace hipac

extern "C" int hipac_detect_abi_version(void) { return HIPAC_DETECT_ABI_VERSION; }

extern "C" int hipac_detect_probs(const float* logits, int n, int tumor_class, float* p, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(n >= 0, HIPAC_EINVAL, "detect_probs: n %d", n);
  HIPAC_REQUIRE(tumor_class == 0 || tumor_class == 1, HIPAC_EINVAL, "detect_probs: tumor_class %d (two classes: 0 or 1)", tumor_class);
  if (n == 0) return 0;
  HIPAC_REQUIRE(logits && p, HIPAC_EINVAL, "detect_probs: null argument");
  hipLaunchKernelGGL(detect_probs_kernel, blocks_for(n), dim3(256), 0, (hipStream_t)stream, logits, n, tumor_class, p);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_detect_level_map(const float* p, const int32_t* meta, int n, int level, int stride, int K, int gw, int gh,
                                      int32_t* origin, float* map, int32_t* count, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(origin && map && count, HIPAC_EINVAL, "detect_level_map: null argument");
  HIPAC_REQUIRE(n >= 0, HIPAC_EINVAL, "detect_level_map: n %d", n);
  HIPAC_REQUIRE(n == 0 || (p && meta), HIPAC_EINVAL, "detect_level_map: null argument");
  HIPAC_REQUIRE(K >= 1 && K <= HIPAC_DETECT_MAX_K, HIPAC_EINVAL, "detect_level_map: K %d outside 1..%d", K, HIPAC_DETECT_MAX_K);
  HIPAC_REQUIRE(stride >= 1, HIPAC_EINVAL, "detect_level_map: stride %d", stride);
  HIPAC_REQUIRE(grid_ok(gw, gh), HIPAC_EINVAL, "detect_level_map: grid %d x %d (need gw, gh >= 1 and gw * gh < 2^31)", gw, gh);
  hipStream_t s = (hipStream_t)stream;
  const int N = gw * gh;
  hipLaunchKernelGGL(detect_fill_kernel, blocks_for(N), dim3(256), 0, s, origin, N, -1);
  if (n) hipLaunchKernelGGL(detect_origin_kernel, blocks_for(n), dim3(256), 0, s, meta, n, level, stride, gw, gh, origin);
  hipLaunchKernelGGL(detect_gather_kernel, blocks_for(N), dim3(256), 0, s, p, (const int32_t*)origin, K, gw, gh, map, count);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_detect_fuse(const float* maps, const int32_t* counts, int n_levels, int gw, int gh, int mode, float* out,
                                 void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(maps && counts && out, HIPAC_EINVAL, "detect_fuse: null argument");
  HIPAC_REQUIRE(n_levels >= 1 && n_levels <= HIPAC_DETECT_MAX_LEVELS, HIPAC_EINVAL, "detect_fuse: n_levels %d outside 1..%d", n_levels,
                HIPAC_DETECT_MAX_LEVELS);
  HIPAC_REQUIRE(mode == HIPAC_DETECT_FUSE_MEAN || mode == HIPAC_DETECT_FUSE_MAX, HIPAC_EINVAL, "detect_fuse: mode %d", mode);
  HIPAC_REQUIRE(grid_ok(gw, gh), HIPAC_EINVAL, "detect_fuse: grid %d x %d (need gw, gh >= 1 and gw * gh < 2^31)", gw, gh);
  const int N = gw * gh;
  hipLaunchKernelGGL(detect_fuse_kernel, blocks_for(N), dim3(256), 0, (hipStream_t)stream, maps, counts, n_levels, N, mode, out);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_detect_smooth(const float* in, int gw, int gh, const float* taps, int radius, float* tmp, float* out,
                                   void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(in && taps && tmp && out, HIPAC_EINVAL, "detect_smooth: null argument");
  HIPAC_REQUIRE(radius >= 0 && radius <= HIPAC_DETECT_MAX_TAPS_R, HIPAC_EINVAL, "detect_smooth: radius %d outside 0..%d", radius,
                HIPAC_DETECT_MAX_TAPS_R);
  HIPAC_REQUIRE(grid_ok(gw, gh), HIPAC_EINVAL, "detect_smooth: grid %d x %d (need gw, gh >= 1 and gw * gh < 2^31)", gw, gh);
  HIPAC_REQUIRE(in != tmp && in != out && tmp != out, HIPAC_EINVAL, "detect_smooth: in, tmp and out must be distinct buffers");
  GaussTaps t = {};
  for (int k = 0; k < 2 * radius + 1; ++k) t.w[k] = taps[k];
  hipStream_t s = (hipStream_t)stream;
  const int N = gw * gh;
  hipLaunchKernelGGL(detect_smooth_kernel, blocks_for(N), dim3(256), 0, s, in, gw, gh, 0, t, radius, tmp);
  hipLaunchKernelGGL(detect_smooth_kernel, blocks_for(N), dim3(256), 0, s, (const float*)tmp, gw, gh, 1, t, radius, out);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" size_t hipac_detect_nms_workspace_bytes(int gw, int gh) {
  using namespace hipac;
  if (!grid_ok(gw, gh)) return 0;
  const size_t N = (size_t)gw * gh;
  // cell states, the keys of the padded grid, the per-round progress flags
  return align256(N * sizeof(int)) + align256(pow2_at_least(N) * sizeof(uint64_t)) + align256(kNmsRounds * sizeof(int));
}

extern "C" int hipac_detect_nms(const float* map, int gw, int gh, int radius, float threshold, int max_detections, float* p,
                                int32_t* ij, int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(map && p && ij && count && workspace, HIPAC_EINVAL, "detect_nms: null argument");
  HIPAC_REQUIRE(grid_ok(gw, gh), HIPAC_EINVAL, "detect_nms: grid %d x %d (need gw, gh >= 1 and gw * gh < 2^31)", gw, gh);
  HIPAC_REQUIRE(radius >= 0 && radius <= HIPAC_DETECT_MAX_NMS_R, HIPAC_EINVAL, "detect_nms: radius %d outside 0..%d", radius,
                HIPAC_DETECT_MAX_NMS_R);
  HIPAC_REQUIRE(max_detections >= 1, HIPAC_EINVAL, "detect_nms: max_detections %d", max_detections);
  const size_t need = hipac_detect_nms_workspace_bytes(gw, gh);
  HIPAC_REQUIRE(workspace_bytes >= need, HIPAC_EWORKSPACE, "detect_nms: workspace %zu < %zu", workspace_bytes, need);
  const int N = gw * gh;
  const size_t Npad = pow2_at_least((size_t)N);
  int* state = (int*)workspace;
  uint64_t* keys = (uint64_t*)((char*)state + align256((size_t)N * sizeof(int)));
  int* progress = (int*)((char*)keys + align256(Npad * sizeof(uint64_t)));
  hipStream_t s = (hipStream_t)stream;
  const size_t init_n = Npad > (size_t)kNmsRounds ? Npad : (size_t)kNmsRounds;
  hipLaunchKernelGGL(nms_init_kernel, blocks_for(init_n), dim3(256), 0, s, map, (unsigned)N, (unsigned)Npad, threshold, state, keys, progress);
  for (int round = 0; round < kNmsRounds; ++round)
    hipLaunchKernelGGL(nms_round_kernel, blocks_for(N), dim3(256), 0, s, map, gw, gh, radius, round, state, keys, progress);
  hipLaunchKernelGGL(nms_finish_kernel, dim3(1), dim3(1024), 0, s, map, gw, gh, radius, state, keys, (const int*)progress);
  for (size_t k = 2; k <= Npad; k <<= 1)
    for (size_t j = k >> 1; j > 0; j >>= 1)
      hipLaunchKernelGGL(nms_bitonic_kernel, blocks_for(Npad), dim3(256), 0, s, keys, (unsigned)Npad, (unsigned)k, (unsigned)j);
  const int M = (size_t)max_detections < Npad ? max_detections : (int)Npad;
  hipLaunchKernelGGL(nms_emit_kernel, blocks_for(M), dim3(256), 0, s, (const uint64_t*)keys, M, gw, p, ij, count);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

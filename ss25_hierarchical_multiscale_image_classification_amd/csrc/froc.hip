// CAMELYON16 FROC evaluation stage (include/hipac_eval.h; reference: src/utils/evaluation_FROC.py).
//
// hipac_eval_mask: computeEvaluationMask of one mask level, bit for bit:
//   1. thresholded exact EDT.  scipy compares sqrt((double)d2) < T with d2 the exact squared distance to the nearest
//      byte == 255.  For integer d2 that test is d2 < K, K = the least integer with sqrt((double)K) >= T (sqrt is monotone),
//      computed once on the host.  Only distances below sqrt(K) matter, so both separable passes are bounded stencils of
//      radius R = the largest g with g^2 < K: the column pass stores the vertical distance to the nearest seed (R + 1 =
//      "farther"), the row pass looks for a column offset dc with dc^2 + g^2 < K.  Exact for every T, not an approximation.
//      No seed at all: scipy measures to a virtual zero at (row -1, column 0), d2 = (r + 1)^2 + c^2.
//   2. binary_fill_holes: union-find over the background with 4-connectivity, roots touching the border flagged, every
//      background pixel of an unflagged root set.
//   3. label(connectivity = 2): union-find over the foreground with 8-connectivity.  Links go toward the smaller linear index
//      (atomicMin), so every root is its component's first raster pixel whatever the schedule; an exclusive prefix sum over
//      the root flags (fixed chunks, one block scan) numbers the roots 1..n in raster order, as scipy / scikit-image do.
// The output buffer `labels` doubles as the column-pass distances and as both union-find forests.
//
// hipac_eval_region_moments: int64 (n, sum r, sum c, sum r^2, sum c^2, sum rc) per label, pre-reduced per row run inside a
// 16-pixel segment and added with integer atomics (order-independent: bitwise reproducible).
#include "common.h"

#include <math.h>

#include "../../include/hipac_eval.h"
#include "wave_reduce.h"

namespace hipac {

constexpr int kEvalChunk = 1024;  // pixels per block of the numbering scan (256 threads x 4 consecutive pixels)
constexpr int kMomentSeg = 16;    // pixels per thread of the moments kernel

__device__ __forceinline__ int uf_load(const int* L, int i) {
  return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int uf_find(const int* L, int x) {
  int y = uf_load(L, x);
  while (y != x) {
    x = y;
    y = uf_load(L, x);
  }
  return x;
}

// join the trees of a and b; every parent link points to a smaller index, so the root is the minimum of the component
__device__ __forceinline__ void uf_unite(int* L, int a, int b) {
  for (;;) {
    a = uf_find(L, a);
    b = uf_find(L, b);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(L + b, a);
    if (old == b) return;
    b = old;
  }
}

// pass 1: G[p] = distance to the nearest seed (mask == 255) in p's column if <= R, else R + 1; any = 1 if a seed exists
__global__ __launch_bounds__(256) void eval_column_kernel(const uint8_t* __restrict__ mask, int W, int H, int64_t pitch, int R,
                                                          int* __restrict__ G, int* __restrict__ any) {
  const int N = W * H;
  const int p = blockIdx.x * 256 + threadIdx.x;
  bool seed = false;
  if (p < N) {
    const int r = p / W, c = p - r * W;
    seed = mask[(int64_t)r * pitch + c] == 255;
    int g = seed ? 0 : R + 1;
    for (int d = 1; d <= R && g > R; ++d) {
      if ((r >= d && mask[(int64_t)(r - d) * pitch + c] == 255) || (r + d < H && mask[(int64_t)(r + d) * pitch + c] == 255)) g = d;
    }
    G[p] = g;
  }
  if (__ballot(seed) && (threadIdx.x & 63) == 0) __hip_atomic_store(any, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// pass 2: bin[p] = (squared distance < K)
__global__ __launch_bounds__(256) void eval_row_kernel(const int* __restrict__ G, int W, int H, int R, int K,
                                                       const int* __restrict__ any, uint8_t* __restrict__ bin) {
  const int N = W * H;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= N) return;
  const int r = p / W, c = p - r * W;
  bool in = false;
  if (*any == 0) {
    const int64_t d2 = (int64_t)(r + 1) * (r + 1) + (int64_t)c * c;
    in = d2 < K;
  } else {
    const int* row = G + (int64_t)r * W;
    for (int dc = 0; dc <= R && !in; ++dc) {
      const int rest = K - dc * dc;  // need g^2 < rest
      if (c >= dc) {
        const int g = row[c - dc];
        in = g <= R && g * g < rest;
      }
      if (!in && dc && c + dc < W) {
        const int g = row[c + dc];
        in = g <= R && g * g < rest;
      }
    }
  }
  bin[p] = in ? 1 : 0;
}

__global__ __launch_bounds__(256) void eval_iota_kernel(int* __restrict__ L, int N) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < N) L[p] = p;
}

// background (bin == 0), 4-connected: link to the left and upper neighbours
__global__ __launch_bounds__(256) void eval_bg_merge_kernel(const uint8_t* __restrict__ bin, int W, int H, int* L) {
  const int N = W * H;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= N || bin[p]) return;
  const int r = p / W, c = p - r * W;
  if (c > 0 && !bin[p - 1]) uf_unite(L, p, p - 1);
  if (r > 0 && !bin[p - W]) uf_unite(L, p, p - W);
}

// background: path to the root; a background pixel on the border flags its root (every writer stores the same 1)
__global__ __launch_bounds__(256) void eval_bg_compress_kernel(const uint8_t* __restrict__ bin, int W, int H, int* L,
                                                               uint8_t* __restrict__ border) {
  const int N = W * H;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= N || bin[p]) return;
  const int root = uf_find(L, p);
  L[p] = root;
  const int r = p / W, c = p - r * W;
  if (r == 0 || c == 0 || r == H - 1 || c == W - 1) border[root] = 1;
}

// filled = binary | (background whose root does not reach the border); L[p] = p again for the foreground forest
// (each thread reads only its own L[p] and the flags)
__global__ __launch_bounds__(256) void eval_fill_kernel(uint8_t* __restrict__ bin, int N, int* __restrict__ L,
                                                        const uint8_t* __restrict__ border) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= N) return;
  if (!bin[p] && !border[L[p]]) bin[p] = 1;
  L[p] = p;
}

// foreground, 8-connected: link to the left, upper-left, upper and upper-right neighbours
__global__ __launch_bounds__(256) void eval_fg_merge_kernel(const uint8_t* __restrict__ bin, int W, int H, int* L) {
  const int N = W * H;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= N || !bin[p]) return;
  const int r = p / W, c = p - r * W;
  if (c > 0 && bin[p - 1]) uf_unite(L, p, p - 1);
  if (r > 0) {
    if (c > 0 && bin[p - W - 1]) uf_unite(L, p, p - W - 1);
    if (bin[p - W]) uf_unite(L, p, p - W);
    if (c + 1 < W && bin[p - W + 1]) uf_unite(L, p, p - W + 1);
  }
}

__global__ __launch_bounds__(256) void eval_fg_compress_kernel(const uint8_t* __restrict__ bin, int N, int* L) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= N || !bin[p]) return;
  L[p] = uf_find(L, p);
}

__device__ __forceinline__ bool is_root(const uint8_t* bin, const int* L, int p) { return bin[p] && L[p] == p; }

// roots per chunk of kEvalChunk pixels
__global__ __launch_bounds__(256) void eval_count_kernel(const uint8_t* __restrict__ bin, int N, const int* __restrict__ L,
                                                         int* __restrict__ cnt) {
  __shared__ int wsum[4];
  const int p0 = blockIdx.x * kEvalChunk + threadIdx.x * 4;
  int k = 0;
  for (int i = 0; i < 4; ++i)
    if (p0 + i < N && is_root(bin, L, p0 + i)) ++k;
  int total;
  block_scan_excl<4>(k, wsum, total);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// one block: cnt[0..n) -> exclusive prefix sums in place, *n_labels = total
__global__ __launch_bounds__(1024) void eval_scan_kernel(int* cnt, int n, int32_t* __restrict__ n_labels) {
  __shared__ int part[1024];
  const int per = (n + 1023) / 1024;
  const int b = threadIdx.x * per, e = min(n, b + per);
  int s = 0;
  for (int i = b; i < e; ++i) s += cnt[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan
    const int y = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += y;
    __syncthreads();
  }
  int run = part[threadIdx.x] - s;
  for (int i = b; i < e; ++i) {
    const int v = cnt[i];
    cnt[i] = run;
    run += v;
  }
  if (threadIdx.x == 1023) *n_labels = part[1023];
}

// a root gets -(its number), numbers 1..n in raster order
__global__ __launch_bounds__(256) void eval_number_kernel(const uint8_t* __restrict__ bin, int N, int* L,
                                                          const int* __restrict__ cnt) {
  __shared__ int wsum[4];
  const int p0 = blockIdx.x * kEvalChunk + threadIdx.x * 4;
  bool f[4];
  int k = 0;
  for (int i = 0; i < 4; ++i) {
    f[i] = p0 + i < N && is_root(bin, L, p0 + i);
    k += f[i];
  }
  int total;
  const int before = block_scan_excl<4>(k, wsum, total);  // its barriers: every root test of the block read L before any root is overwritten
  int next = cnt[blockIdx.x] + before + 1;
  for (int i = 0; i < 4; ++i)
    if (f[i]) L[p0 + i] = -(next++);
}

// non-root foreground takes its root's negated number; background 0 (roots are only read here)
__global__ __launch_bounds__(256) void eval_resolve_kernel(const uint8_t* __restrict__ bin, int N, int* L) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= N) return;
  if (!bin[p]) {
    L[p] = 0;
    return;
  }
  const int v = L[p];
  if (v >= 0) L[p] = L[v];
}

__global__ __launch_bounds__(256) void eval_negate_kernel(int* L, int N) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < N) L[p] = -L[p];
}

__device__ __forceinline__ void moments_flush(unsigned long long* M, int n_labels, int lab, int64_t r, int64_t k, int64_t sc,
                                              int64_t scc) {
  if (lab < 1 || lab > n_labels || k == 0) return;
  unsigned long long* m = M + (size_t)(lab - 1) * 6;
  atomicAdd(m + 0, (unsigned long long)k);
  atomicAdd(m + 1, (unsigned long long)(r * k));
  atomicAdd(m + 2, (unsigned long long)sc);
  atomicAdd(m + 3, (unsigned long long)(r * r * k));
  atomicAdd(m + 4, (unsigned long long)scc);
  atomicAdd(m + 5, (unsigned long long)(r * sc));
}

// one thread per kMomentSeg-pixel row segment; a run of one label is summed locally and added once
__global__ __launch_bounds__(256) void eval_moments_kernel(const int32_t* __restrict__ labels, int W, int H, int n_labels,
                                                           unsigned long long* M) {
  const int segs = (W + kMomentSeg - 1) / kMomentSeg;
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= (int64_t)segs * H) return;
  const int r = (int)(s / segs), c0 = (int)(s - (int64_t)r * segs) * kMomentSeg, c1 = min(W, c0 + kMomentSeg);
  const int32_t* row = labels + (int64_t)r * W;
  int lab = 0;
  int64_t k = 0, sc = 0, scc = 0;
  for (int c = c0; c < c1; ++c) {
    const int v = row[c];
    if (v != lab) {
      moments_flush(M, n_labels, lab, r, k, sc, scc);
      lab = v, k = 0, sc = 0, scc = 0;
    }
    ++k, sc += c, scc += (int64_t)c * c;
  }
  moments_flush(M, n_labels, lab, r, k, sc, scc);
}

__global__ __launch_bounds__(256) void eval_lookup_kernel(const int32_t* __restrict__ labels, int W, int H, int level,
                                                          const int64_t* __restrict__ xy, int n, int32_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t d = (int64_t)1 << level;
  const int64_t x = xy[2 * i] / d, y = xy[2 * i + 1] / d;  // C++ division truncates toward zero, as int(v / 2**level)
  out[i] = (x >= 0 && x < W && y >= 0 && y < H) ? labels[y * W + x] : 0;
}

static bool eval_size_ok(int W, int H) { return W >= 1 && H >= 1 && (int64_t)W * H < ((int64_t)1 << 31); }

}  // namespace hipac

extern "C" int hipac_eval_abi_version(void) { return HIPAC_EVAL_ABI_VERSION; }

extern "C" size_t hipac_eval_workspace_bytes(int W, int H) {
  using namespace hipac;
  if (!eval_size_ok(W, H)) return 0;
  const size_t N = (size_t)W * H, chunks = (N + kEvalChunk - 1) / kEvalChunk;
  // binary / filled mask, border flags of the background roots, roots per chunk, the any-seed flag
  return align256(N) + align256(N) + align256(chunks * sizeof(int)) + 256;
}

extern "C" int hipac_eval_mask(const uint8_t* mask, int W, int H, int64_t pitch, double threshold, int32_t* labels,
                               int32_t* n_labels, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(mask && labels && n_labels && workspace, HIPAC_EINVAL, "eval_mask: null argument");
  HIPAC_REQUIRE(eval_size_ok(W, H), HIPAC_EINVAL, "eval_mask: sizes %d x %d (need W, H >= 1 and W * H < 2^31)", W, H);
  HIPAC_REQUIRE(pitch >= W, HIPAC_EINVAL, "eval_mask: pitch %lld < W %d", (long long)pitch, W);
  HIPAC_REQUIRE(threshold > 0.0 && threshold < 46340.0, HIPAC_EINVAL, "eval_mask: threshold %g outside (0, 46340)", threshold);
  const size_t need = hipac_eval_workspace_bytes(W, H);
  HIPAC_REQUIRE(workspace_bytes >= need, HIPAC_EWORKSPACE, "eval_mask: workspace %zu < %zu", workspace_bytes, need);
  // K = least integer with sqrt((double)K) >= threshold; R = largest g with g * g < K
  int K = (int)floor(threshold * threshold);
  K = K > 2 ? K - 2 : 0;
  while (sqrt((double)K) < threshold) ++K;
  int R = 0;
  while ((R + 1) * (R + 1) < K) ++R;
  const int N = W * H;
  const int chunks = (N + kEvalChunk - 1) / kEvalChunk;
  uint8_t* bin = (uint8_t*)workspace;
  uint8_t* border = bin + align256(N);
  int* cnt = (int*)(border + align256(N));
  int* any = (int*)((char*)cnt + align256((size_t)chunks * sizeof(int)));
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((N + 255) / 256), block(256);
  HIPAC_CHECK_HIP(hipMemsetAsync(any, 0, sizeof(int), s));
  HIPAC_CHECK_HIP(hipMemsetAsync(border, 0, N, s));
  hipLaunchKernelGGL(eval_column_kernel, grid, block, 0, s, mask, W, H, pitch, R, labels, any);
  hipLaunchKernelGGL(eval_row_kernel, grid, block, 0, s, (const int*)labels, W, H, R, K, (const int*)any, bin);
  hipLaunchKernelGGL(eval_iota_kernel, grid, block, 0, s, labels, N);
  hipLaunchKernelGGL(eval_bg_merge_kernel, grid, block, 0, s, (const uint8_t*)bin, W, H, labels);
  hipLaunchKernelGGL(eval_bg_compress_kernel, grid, block, 0, s, (const uint8_t*)bin, W, H, labels, border);
  hipLaunchKernelGGL(eval_fill_kernel, grid, block, 0, s, bin, N, labels, (const uint8_t*)border);
  hipLaunchKernelGGL(eval_fg_merge_kernel, grid, block, 0, s, (const uint8_t*)bin, W, H, labels);
  hipLaunchKernelGGL(eval_fg_compress_kernel, grid, block, 0, s, (const uint8_t*)bin, N, labels);
  hipLaunchKernelGGL(eval_count_kernel, dim3(chunks), block, 0, s, (const uint8_t*)bin, N, (const int*)labels, cnt);
  hipLaunchKernelGGL(eval_scan_kernel, dim3(1), dim3(1024), 0, s, cnt, chunks, n_labels);
  hipLaunchKernelGGL(eval_number_kernel, dim3(chunks), block, 0, s, (const uint8_t*)bin, N, labels, (const int*)cnt);
  hipLaunchKernelGGL(eval_resolve_kernel, grid, block, 0, s, (const uint8_t*)bin, N, labels);
  hipLaunchKernelGGL(eval_negate_kernel, grid, block, 0, s, labels, N);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_eval_region_moments(const int32_t* labels, int W, int H, int n_labels, int64_t* moments, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(labels && moments, HIPAC_EINVAL, "eval_region_moments: null argument");
  HIPAC_REQUIRE(eval_size_ok(W, H) && W <= 65536 && H <= 65536, HIPAC_EINVAL, "eval_region_moments: sizes %d x %d", W, H);
  HIPAC_REQUIRE(n_labels >= 0 && n_labels <= W * H, HIPAC_EINVAL, "eval_region_moments: n_labels %d", n_labels);
  if (n_labels == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  HIPAC_CHECK_HIP(hipMemsetAsync(moments, 0, (size_t)n_labels * 6 * sizeof(int64_t), s));
  const int64_t segs = (int64_t)((W + kMomentSeg - 1) / kMomentSeg) * H;
  hipLaunchKernelGGL(eval_moments_kernel, dim3((unsigned)((segs + 255) / 256)), dim3(256), 0, s, labels, W, H, n_labels,
                     (unsigned long long*)moments);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_eval_lookup(const int32_t* labels, int W, int H, int level, const int64_t* xy, int n, int32_t* out,
                                 void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(eval_size_ok(W, H), HIPAC_EINVAL, "eval_lookup: sizes %d x %d", W, H);
  HIPAC_REQUIRE(level >= 0 && level <= 30, HIPAC_EINVAL, "eval_lookup: level %d", level);
  HIPAC_REQUIRE(n >= 0, HIPAC_EINVAL, "eval_lookup: n %d", n);
  if (n == 0) return 0;
  HIPAC_REQUIRE(labels && xy && out, HIPAC_EINVAL, "eval_lookup: null argument");
  hipLaunchKernelGGL(eval_lookup_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, labels, W, H, level, xy, n,
                     out);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

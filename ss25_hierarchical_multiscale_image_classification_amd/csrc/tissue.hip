// Otsu tissue mask (include/hipac_tissue.h): level image -> thumbnail, saturation, histogram -> Otsu threshold -> cleaned mask ->
// summed-area table -> one keep flag per window.  Everything stays in HBM, and the threshold is read from device memory by the mask
// kernels, so the host never waits between the stages.
//
// Integers throughout, so the order of the work cannot show in the result; the one floating-point place is
// the Otsu score, IEEE double without contraction (-ffp-contract=off, build.py).  The only atomics are integer adds.
//
//   thumbnail   the one kernel that reads real data (the whole level, once).  A thread owns max(16, f) level pixels of f rows: 16
//               pixels are 48 bytes = three aligned 16-byte loads, and neighbouring threads read neighbouring 48-byte pieces, so a
//               wave reads 3 KB of a row contiguously.  It finishes 16 / f (at least one) mask pixels on its own: no exchange
//               between threads except the histogram, counted in LDS and added to global memory once per non-empty bin.
//   otsu        one workgroup: inclusive scans of h and i h over the 256 bins, the score per bin, arg-max with the lowest index.
//   mask        separable passes of one kernel (min or max over 2 R + 1 pixels of a row or a column, 0 outside); the first pass
//               thresholds the saturation as it reads it.
//   integral    one wave per row (shuffle scan, 64 pixels a step), then one thread per column walking down.
//   keep        one thread per window, four table reads.
#include "common.h"

#include "../../include/hipac_tissue.h"
#include "wave_reduce.h"

namespace hipac {

static inline dim3 tissue_blocks(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

static bool tissue_size_ok(int mw, int mh) { return mw >= 1 && mh >= 1 && (long long)mw * mh < HIPAC_TISSUE_MAX_PIXELS; }

template <int F>
__global__ __launch_bounds__(256) void tissue_thumb_kernel(const uint8_t* __restrict__ img, int W, int H, size_t pitch, int mw, int mh,
                                                           int ncx, uint8_t* __restrict__ thumb, uint8_t* __restrict__ sat,
                                                           uint32_t* __restrict__ hist) {
  constexpr int CW = F > 16 ? F : 16;          // level pixels of a row one thread owns
  constexpr int NSUB = CW / 16, NPX = CW / F;  // 48-byte pieces per row; mask pixels it finishes
  __shared__ uint32_t lh[256];
  lh[threadIdx.x] = 0;
  __syncthreads();
  const unsigned g = blockIdx.x * 256u + threadIdx.x;
  if (g < (unsigned)ncx * (unsigned)mh) {
    const int j = (int)(g / (unsigned)ncx), cx = (int)(g - (unsigned)j * (unsigned)ncx);
    const int x0 = cx * CW, y0 = j * F;
    const int ny = H - y0 < F ? H - y0 : F;
    uint32_t acc[NPX][3] = {};
    for (int r = 0; r < ny; ++r) {
      const uint8_t* row = img + (size_t)(y0 + r) * pitch + (size_t)x0 * 3;
#pragma unroll
      for (int s = 0; s < NSUB; ++s) {
        const int valid = W - (x0 + 16 * s);  // pixels of this piece inside the level: the rest is row padding, never a pixel
        if (valid > 0) {
          const u32x4* p = reinterpret_cast<const u32x4*>(row + 48 * s);
          const u32x4 v0 = p[0], v1 = p[1], v2 = p[2];
          const uint32_t w[12] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3], v2[0], v2[1], v2[2], v2[3]};
#pragma unroll
          for (int b = 0; b < 48; ++b) {
            const int px = b / 3;
            const uint32_t byte = (w[b >> 2] >> (8 * (b & 3))) & 0xffu;
            acc[(16 * s + px) / F][b % 3] += px < valid ? byte : 0u;
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < NPX; ++q) {
      const int i = cx * NPX + q;
      if (i < mw) {
        const int nx = W - i * F < F ? W - i * F : F;
        const uint32_t n = (uint32_t)(nx * ny);
        uint32_t c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = (2u * acc[q][k] + n) / (2u * n);
        const uint32_t mx = max(c[0], max(c[1], c[2])), mn = min(c[0], min(c[1], c[2]));
        const uint32_t sv = mx == 0 ? 0u : (2u * 255u * (mx - mn) + mx) / (2u * mx);
        const size_t o = (size_t)j * mw + i;
        thumb[3 * o] = (uint8_t)c[0], thumb[3 * o + 1] = (uint8_t)c[1], thumb[3 * o + 2] = (uint8_t)c[2];
        sat[o] = (uint8_t)sv;
        atomicAdd(&lh[sv], 1u);
      }
    }
  }
  __syncthreads();
  const uint32_t v = lh[threadIdx.x];
  if (v) atomicAdd(&hist[threadIdx.x], v);
}

__global__ __launch_bounds__(256) void tissue_otsu_kernel(const uint32_t* __restrict__ hist, int floor, int32_t* __restrict__ thr) {
  __shared__ long long w[256], m[256];
  __shared__ double bv[256];
  __shared__ int bt[256];
  const int t = threadIdx.x;
  w[t] = (long long)hist[t];
  m[t] = (long long)t * (long long)hist[t];
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const long long aw = t >= o ? w[t - o] : 0, am = t >= o ? m[t - o] : 0;
    __syncthreads();
    w[t] += aw, m[t] += am;
    __syncthreads();
  }
  const long long N = w[255], M = m[255], w0 = w[t], m0 = m[t];
  double v = -1.0;  // not a candidate
  if (t < 255 && w0 > 0 && w0 < N) {
    const double d = (double)(M * w0 - N * m0);
    const double dd = d * d;
    v = dd / (double)(w0 * (N - w0));
  }
  bv[t] = v, bt[t] = t;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      const double v2 = bv[t + o];
      const int t2 = bt[t + o];
      if (v2 > bv[t] || (v2 == bv[t] && t2 < bt[t])) bv[t] = v2, bt[t] = t2;
    }
    __syncthreads();
  }
  if (t == 0) {
    const int best = bv[0] < 0.0 ? 255 : bt[0];
    thr[0] = best;
    thr[1] = best > floor ? best : floor;
  }
}

// one separable pass along x (along_y = 0) or y: min or max over 2 R + 1 pixels, 0 outside.  thr != nullptr: `in` is the saturation
// and a pixel is sat > thr[1]
__global__ __launch_bounds__(256) void tissue_morph_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ thr, int mw, int mh,
                                                           int along_y, int R, int is_max, uint8_t* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= mw * mh) return;
  const int y = c / mw, x = c - y * mw;
  const int pos = along_y ? y : x, len = along_y ? mh : mw, step = along_y ? mw : 1;
  const int t = thr ? thr[1] : 0;
  int acc = is_max ? 0 : 1;
  for (int k = -R; k <= R; ++k) {
    const int q = pos + k;
    int v = 0;
    if (q >= 0 && q < len) {
      const int u = in[c + k * step];
      v = thr ? (u > t ? 1 : 0) : u;
    }
    acc = is_max ? (v > acc ? v : acc) : (v < acc ? v : acc);
  }
  out[c] = (uint8_t)acc;
}

// block 0 zeroes the table's first row; block j + 1 scans mask row j into table row j + 1 (one wave, 64 pixels a step)
__global__ __launch_bounds__(64) void tissue_rowscan_kernel(const uint8_t* __restrict__ mask, int mw, int32_t* __restrict__ table) {
  const int lane = threadIdx.x, tw = mw + 1;
  if (blockIdx.x == 0) {
    for (int i = lane; i < tw; i += 64) table[i] = 0;
    return;
  }
  const int j = blockIdx.x - 1;
  int32_t* out = table + (size_t)(j + 1) * tw;
  if (lane == 0) out[0] = 0;
  int carry = 0;
  for (int i0 = 0; i0 < mw; i0 += 64) {
    const int i = i0 + lane;
    const int v = wave_scan_incl(i < mw ? (int)mask[(size_t)j * mw + i] : 0, lane) + carry;
    if (i < mw) out[i + 1] = v;
    carry = __shfl(v, 63, 64);
  }
}

__global__ __launch_bounds__(256) void tissue_colscan_kernel(int mw, int mh, int32_t* __restrict__ table) {
  const int i = blockIdx.x * 256 + threadIdx.x + 1;
  if (i > mw) return;
  const int tw = mw + 1;
  int acc = 0;
#pragma unroll 8
  for (int j = 1; j <= mh; ++j) {
    acc += table[(size_t)j * tw + i];
    table[(size_t)j * tw + i] = acc;
  }
}

__global__ __launch_bounds__(256) void tissue_keep_kernel(const int32_t* __restrict__ table, int mw, int mh, const int32_t* __restrict__ xy,
                                                          int n, int level, int min_permille, uint8_t* __restrict__ keep,
                                                          int32_t* __restrict__ count) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const long long X = (long long)xy[2 * k] * (1 << level), Y = (long long)xy[2 * k + 1] * (1 << level);
  const long long x0 = X >> 5, x1 = (X + HIPAC_TISSUE_WINDOW + HIPAC_TISSUE_CELL - 1) >> 5;
  const long long y0 = Y >> 5, y1 = (Y + HIPAC_TISSUE_WINDOW + HIPAC_TISSUE_CELL - 1) >> 5;
  const long long n_rect = (x1 - x0) * (y1 - y0);
  auto clampi = [](long long v, int hi) { return (int)(v < 0 ? 0 : (v > hi ? hi : v)); };
  const int cx0 = clampi(x0, mw), cx1 = clampi(x1, mw), cy0 = clampi(y0, mh), cy1 = clampi(y1, mh);
  const size_t tw = (size_t)mw + 1;
  const int c = table[cy1 * tw + cx1] - table[cy0 * tw + cx1] - table[cy1 * tw + cx0] + table[cy0 * tw + cx0];
  count[k] = c;
  keep[k] = (c >= 1 && 1000ll * c >= (long long)min_permille * n_rect) ? 1 : 0;
}

template <int F>
static void launch_thumb(const uint8_t* img, int W, int H, size_t pitch, int mw, int mh, uint8_t* thumb, uint8_t* sat, uint32_t* hist,
                         hipStream_t s) {
  constexpr int CW = F > 16 ? F : 16;
  const int ncx = (W + CW - 1) / CW;
  hipLaunchKernelGGL(tissue_thumb_kernel<F>, tissue_blocks((size_t)ncx * mh), dim3(256), 0, s, img, W, H, pitch, mw, mh, ncx, thumb, sat,
                     hist);
}

}  // namespace hipac

extern "C" int hipac_tissue_abi_version(void) { return HIPAC_TISSUE_ABI_VERSION; }

extern "C" int hipac_tissue_thumbnail(const uint8_t* img, int width, int height, size_t pitch, int f, uint8_t* thumb, uint8_t* sat,
                                      uint32_t* hist, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(img && thumb && sat && hist, HIPAC_EINVAL, "tissue_thumbnail: null argument");
  HIPAC_REQUIRE(f == 4 || f == 8 || f == 16 || f == 32, HIPAC_EINVAL, "tissue_thumbnail: f %d (need 4, 8, 16 or 32 = 32 >> level)", f);
  HIPAC_REQUIRE(width >= 1 && height >= 1, HIPAC_EINVAL, "tissue_thumbnail: level %d x %d", width, height);
  const int mw = (int)(((long long)width + f - 1) / f), mh = (int)(((long long)height + f - 1) / f);
  HIPAC_REQUIRE(tissue_size_ok(mw, mh), HIPAC_EINVAL, "tissue_thumbnail: mask %d x %d (need mw * mh < 2^24)", mw, mh);
  const size_t row_bytes = (size_t)((width + 15) / 16) * 48;
  HIPAC_REQUIRE(pitch % 48 == 0 && pitch >= row_bytes, HIPAC_EINVAL,
                "tissue_thumbnail: pitch %zu (need a multiple of 48 bytes, at least %zu for %d pixels)", pitch, row_bytes, width);
  HIPAC_REQUIRE(((uintptr_t)img & 15) == 0, HIPAC_EINVAL, "tissue_thumbnail: image not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  HIPAC_CHECK_HIP(hipMemsetAsync(hist, 0, 256 * sizeof(uint32_t), s));
  if (f == 4) launch_thumb<4>(img, width, height, pitch, mw, mh, thumb, sat, hist, s);
  else if (f == 8) launch_thumb<8>(img, width, height, pitch, mw, mh, thumb, sat, hist, s);
  else if (f == 16) launch_thumb<16>(img, width, height, pitch, mw, mh, thumb, sat, hist, s);
  else launch_thumb<32>(img, width, height, pitch, mw, mh, thumb, sat, hist, s);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_tissue_otsu(const uint32_t* hist, int floor, int32_t* thresholds, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(hist && thresholds, HIPAC_EINVAL, "tissue_otsu: null argument");
  HIPAC_REQUIRE(floor >= 0 && floor <= 255, HIPAC_EINVAL, "tissue_otsu: floor %d outside 0..255", floor);
  hipLaunchKernelGGL(tissue_otsu_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, hist, floor, thresholds);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_tissue_mask(const uint8_t* sat, int mw, int mh, const int32_t* thresholds, int opening, int dilate, uint8_t* tmp,
                                 uint8_t* mask, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(sat && thresholds && tmp && mask, HIPAC_EINVAL, "tissue_mask: null argument");
  HIPAC_REQUIRE(tissue_size_ok(mw, mh), HIPAC_EINVAL, "tissue_mask: mask %d x %d (need mw, mh >= 1 and mw * mh < 2^24)", mw, mh);
  HIPAC_REQUIRE(dilate >= 0 && dilate <= HIPAC_TISSUE_MAX_DILATE, HIPAC_EINVAL, "tissue_mask: dilate %d outside 0..%d", dilate,
                HIPAC_TISSUE_MAX_DILATE);
  HIPAC_REQUIRE(sat != tmp && sat != mask && tmp != mask, HIPAC_EINVAL, "tissue_mask: sat, tmp and mask must be distinct buffers");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid = tissue_blocks((size_t)mw * mh);
  const uint8_t* ctmp = tmp;
  const uint8_t* cmask = mask;
  const int32_t* none = nullptr;
  if (opening) {
    // erosion 3 x 3, then the opening's dilation and the final one as a single (2 (D + 1) + 1)^2 square: two dilations by squares,
    // clipped to the mask, compose exactly (clamp the intermediate pixel into the rectangle: it stays within reach of both ends)
    hipLaunchKernelGGL(tissue_morph_kernel, grid, dim3(256), 0, s, sat, thresholds, mw, mh, 0, 1, 0, tmp);
    hipLaunchKernelGGL(tissue_morph_kernel, grid, dim3(256), 0, s, ctmp, none, mw, mh, 1, 1, 0, mask);
    hipLaunchKernelGGL(tissue_morph_kernel, grid, dim3(256), 0, s, cmask, none, mw, mh, 0, dilate + 1, 1, tmp);
    hipLaunchKernelGGL(tissue_morph_kernel, grid, dim3(256), 0, s, ctmp, none, mw, mh, 1, dilate + 1, 1, mask);
  } else {
    hipLaunchKernelGGL(tissue_morph_kernel, grid, dim3(256), 0, s, sat, thresholds, mw, mh, 0, dilate, 1, tmp);
    hipLaunchKernelGGL(tissue_morph_kernel, grid, dim3(256), 0, s, ctmp, none, mw, mh, 1, dilate, 1, mask);
  }
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_tissue_integral(const uint8_t* mask, int mw, int mh, int32_t* table, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(mask && table, HIPAC_EINVAL, "tissue_integral: null argument");
  HIPAC_REQUIRE(tissue_size_ok(mw, mh), HIPAC_EINVAL, "tissue_integral: mask %d x %d (need mw, mh >= 1 and mw * mh < 2^24)", mw, mh);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(tissue_rowscan_kernel, dim3((unsigned)mh + 1), dim3(64), 0, s, mask, mw, table);
  hipLaunchKernelGGL(tissue_colscan_kernel, tissue_blocks((size_t)mw), dim3(256), 0, s, mw, mh, table);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_tissue_window_keep(const int32_t* table, int mw, int mh, const int32_t* xy, int n, int level, int min_permille,
                                        uint8_t* keep, int32_t* count, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(n >= 0, HIPAC_EINVAL, "tissue_window_keep: n %d", n);
  HIPAC_REQUIRE(table && (n == 0 || (xy && keep && count)), HIPAC_EINVAL, "tissue_window_keep: null argument");
  HIPAC_REQUIRE(tissue_size_ok(mw, mh), HIPAC_EINVAL, "tissue_window_keep: mask %d x %d (need mw, mh >= 1 and mw * mh < 2^24)", mw, mh);
  HIPAC_REQUIRE(level >= 0 && level <= 3, HIPAC_EINVAL, "tissue_window_keep: level %d outside 0..3", level);
  HIPAC_REQUIRE(min_permille >= 0 && min_permille <= 1000, HIPAC_EINVAL, "tissue_window_keep: min_permille %d outside 0..1000",
                min_permille);
  if (n == 0) return 0;
  hipLaunchKernelGGL(tissue_keep_kernel, tissue_blocks((size_t)n), dim3(256), 0, (hipStream_t)stream, table, mw, mh, xy, n, level,
                     min_permille, keep, count);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

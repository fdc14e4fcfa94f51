// Macenko stain normalisation (include/hipac_stain.h): moments -> basis -> angle histogram -> stain vectors -> concentration
// histograms -> 3 x 3 map -> every pixel of every level.  Everything stays in HBM: the status and the map are read from device
// memory by the apply kernel, so the host never waits for the fit.
//
// Optical densities are integers (the literal table below, units of 2^-12), sums and histograms are integers with integer atomics
// only, and the small matrices are IEEE double, one rounding per operation (-ffp-contract=off, build.py), written in the order of
// tests/stain_cpu.py: every output is bit for bit the restatement's.
//
//   moments, angle_hist, conc_hist   one walk over the level each (stain_visit): a thread owns 16 pixels = 48 bytes = three aligned
//               16-byte loads, as in tissue_thumb_kernel; a fixed grid strides over the level.  Moments: 64-bit sums per thread, wave
//               shuffle, LDS across the waves, ten atomics per workgroup.  Histograms: counted in LDS, non-empty bins added once.
//   basis, vectors, matrix   one workgroup; the rank searches use all 256 threads (16 bins each), the doubles are thread 0's.
//   apply       the HBM-bound hot path.  A workgroup builds inv[] (22714 bytes, a binary search per entry) and od[] as double in
//               LDS once and then strides over the image; per 48-byte piece: three 16-byte loads, 16 x 3 table look-ups, 16 x 3
//               three-term double products, three 16-byte stores (byte stores for the piece that holds the row's last pixels).
#include "common.h"

#include "../../include/hipac_stain.h"
#include "stain_od.h"
#include "wave_reduce.h"

namespace hipac {

static const int32_t kStainOdHost[256] = {HIPAC_STAIN_OD_LIST};
__constant__ int32_t kStainOd[256] = {HIPAC_STAIN_OD_LIST};

constexpr int kNB = HIPAC_STAIN_ANGLE_BINS, kNBC = HIPAC_STAIN_CONC_BINS, kOdMax = HIPAC_STAIN_OD_MAX;
constexpr unsigned kStainReduceBlocks = 2048, kStainApplyBlocks = 1536;  // 256 CUs x 8 / x 6 workgroups (25 KB of LDS each)

struct StainImage {
  const uint8_t* img;
  int W, H;
  size_t pitch;
  const uint8_t* mask;  // nullptr: no mask
  int mw, fshift, bq;
};

// fn(o0, o1, o2) for every tissue pixel of the pieces this thread owns; od: int32[256] in LDS
template <class F>
__device__ __forceinline__ void stain_visit(const StainImage& g, const int32_t* od, F&& fn) {
  const unsigned ncx = (unsigned)(g.W + 15) >> 4;
  const unsigned long long total = (unsigned long long)ncx * (unsigned)g.H;  // <= W * H < 2^32
  for (unsigned long long p = blockIdx.x * 256ull + threadIdx.x; p < total; p += gridDim.x * 256ull) {
    const unsigned y = (unsigned)p / ncx, cx = (unsigned)p - y * ncx;
    const int x0 = (int)cx * 16;
    const int valid = g.W - x0;  // pixels of this piece inside the level: the rest is row padding, never a pixel
    const u32x4* src = reinterpret_cast<const u32x4*>(g.img + (size_t)y * g.pitch + (size_t)x0 * 3);
    const u32x4 v0 = src[0], v1 = src[1], v2 = src[2];
    const uint32_t w[12] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3], v2[0], v2[1], v2[2], v2[3]};
    const uint8_t* mrow = g.mask ? g.mask + (size_t)(y >> g.fshift) * g.mw : nullptr;
#pragma unroll
    for (int px = 0; px < 16; ++px) {
      if (px < valid) {
        int o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int b = 3 * px + c;
          o[c] = od[(w[b >> 2] >> (8 * (b & 3))) & 0xffu];
        }
        bool t = min(o[0], min(o[1], o[2])) >= g.bq;
        if (t && mrow) t = mrow[(x0 + px) >> g.fshift] != 0;
        if (t) fn(o[0], o[1], o[2]);
      }
    }
  }
}

__device__ __forceinline__ void stain_load_od(int32_t* od) {
  od[threadIdx.x] = kStainOd[threadIdx.x];
  __syncthreads();
}

__global__ __launch_bounds__(256) void stain_moments_kernel(StainImage g, unsigned long long* __restrict__ mom) {
  __shared__ int32_t od[256];
  __shared__ long long part[4][10];
  stain_load_od(od);
  long long acc[10] = {};
  stain_visit(g, od, [&](int o0, int o1, int o2) {
    const long long a = o0, b = o1, c = o2;
    acc[0] += 1, acc[1] += a, acc[2] += b, acc[3] += c;
    acc[4] += a * a, acc[5] += a * b, acc[6] += a * c, acc[7] += b * b, acc[8] += b * c, acc[9] += c * c;
  });
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const long long v = wave_sum_tree(acc[i]);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < 10) {
    const long long v = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
    if (v) atomicAdd(&mom[threadIdx.x], (unsigned long long)v);
  }
}

__device__ __forceinline__ double stain_dot(double o0, double o1, double o2, const double* v) { return (o0 * v[0] + o1 * v[1]) + o2 * v[2]; }

__global__ __launch_bounds__(256) void stain_angle_kernel(StainImage g, const double* __restrict__ basis, uint32_t* __restrict__ hist) {
  __shared__ int32_t od[256];
  __shared__ uint32_t lh[kNB];
  for (int i = threadIdx.x; i < kNB; i += 256) lh[i] = 0;
  stain_load_od(od);
  double v1[3], v2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) v1[c] = basis[c], v2[c] = basis[3 + c];
  stain_visit(g, od, [&](int o0, int o1, int o2) {
    const double a = (double)o0, b = (double)o1, c = (double)o2;
    const double x = stain_dot(a, b, c, v1), y = stain_dot(a, b, c, v2);
    int bin;
    if (x > 0.0) {
      const double d = y / (x + fabs(y));
      bin = (int)((d + 1.0) * (double)(kNB / 2));
      bin = bin > kNB - 1 ? kNB - 1 : bin;
    } else {
      bin = y < 0.0 ? 0 : kNB - 1;
    }
    atomicAdd(&lh[bin], 1u);
  });
  __syncthreads();
  for (int i = threadIdx.x; i < kNB; i += 256) {
    const uint32_t v = lh[i];
    if (v) atomicAdd(&hist[i], v);
  }
}

__device__ __forceinline__ int stain_conc_bin(double C) {
  const double t = C * 0.125;
  return t < 0.0 ? 0 : (t >= (double)kNBC ? kNBC - 1 : (int)t);
}

__global__ __launch_bounds__(256) void stain_conc_kernel(StainImage g, const double* __restrict__ he_p, uint32_t* __restrict__ chist) {
  __shared__ int32_t od[256];
  __shared__ uint32_t lh[2 * kNBC];
  for (int i = threadIdx.x; i < 2 * kNBC; i += 256) lh[i] = 0;
  stain_load_od(od);
  double p0[3], p1[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) p0[c] = he_p[6 + c], p1[c] = he_p[9 + c];
  stain_visit(g, od, [&](int o0, int o1, int o2) {
    const double a = (double)o0, b = (double)o1, c = (double)o2;
    atomicAdd(&lh[stain_conc_bin(stain_dot(a, b, c, p0))], 1u);
    atomicAdd(&lh[kNBC + stain_conc_bin(stain_dot(a, b, c, p1))], 1u);
  });
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * kNBC; i += 256) {
    const uint32_t v = lh[i];
    if (v) atomicAdd(&chist[i], v);
  }
}

// ---- the small stages ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(64) void stain_basis_kernel(const long long* __restrict__ mom, double* __restrict__ basis, int32_t* __restrict__ status) {
  if (threadIdx.x != 0) return;
  double out[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int st = 0;
  if (mom[0] >= 2) {
    const double n = (double)mom[0];
    double mean[3], A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int c = 0; c < 3; ++c) mean[c] = (double)mom[1 + c] / n;
    const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {0, 1, 2, 1, 2, 2};
    for (int i = 0; i < 6; ++i) {
      const double v = ((double)mom[4 + i] - (double)mom[1 + pa[i]] * mean[pb[i]]) / (n - 1.0);
      A[pa[i]][pb[i]] = v, A[pb[i]][pa[i]] = v;
    }
    const int jp[3] = {0, 0, 1}, jq[3] = {1, 2, 2};
    for (int sweep = 0; sweep < HIPAC_STAIN_JACOBI_SWEEPS; ++sweep) {
      for (int r = 0; r < 3; ++r) {
        const int p = jp[r], q = jq[r];
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq, A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk, A[q][k] = s * apk + c * aqk;
        }
        A[p][q] = 0.0, A[q][p] = 0.0;
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq, V[k][q] = s * vkp + c * vkq;
        }
      }
    }
    const double w[3] = {A[0][0], A[1][1], A[2][2]};
    int i1 = 0;
    for (int i = 1; i < 3; ++i)
      if (w[i] > w[i1]) i1 = i;
    int i2 = -1;
    for (int i = 0; i < 3; ++i)
      if (i != i1 && (i2 < 0 || w[i] > w[i2])) i2 = i;
    if (w[i2] > 0.0) {
      st = 1;
      const int idx[2] = {i1, i2};
      for (int r = 0; r < 2; ++r) {
        double v[3] = {V[0][idx[r]], V[1][idx[r]], V[2][idx[r]]};
        if ((v[0] + v[1]) + v[2] < 0.0) v[0] = -v[0], v[1] = -v[1], v[2] = -v[2];
        out[3 * r] = v[0], out[3 * r + 1] = v[1], out[3 * r + 2] = v[2];
      }
    }
  }
  for (int i = 0; i < 6; ++i) basis[i] = out[i];
  status[0] = st;
}

// All 256 threads: n = sum h over `bins` = 16 * 256 bins, k = max(1, ceil(permille n / 1000)), res[0] / res[1] = the first bins whose
// cumulative counts reach k / n - k + 1 (`bins` when there is none: n = 0).  cum: LDS [257], res: LDS [2].  Returns n.
__device__ long long stain_rank_bins(const uint32_t* __restrict__ h, int permille, long long* cum, int* res) {
  const int t = threadIdx.x;
  uint32_t mine[16];
  long long s = 0;
  for (int i = 0; i < 16; ++i) mine[i] = h[16 * t + i], s += mine[i];
  __syncthreads();  // cum and res may still be read from an earlier call
  cum[t + 1] = s;
  if (t == 0) cum[0] = 0, res[0] = 16 * 256, res[1] = 16 * 256;
  __syncthreads();
  if (t == 0)
    for (int i = 1; i <= 256; ++i) cum[i] += cum[i - 1];
  __syncthreads();
  const long long n = cum[256];
  const long long k0 = ((long long)permille * n + 999) / 1000, k = k0 < 1 ? 1 : k0;
  const long long want[2] = {k, n - k + 1};
  for (int j = 0; j < 2; ++j) {
    if (cum[t] < want[j] && want[j] <= cum[t + 1]) {
      long long c = cum[t];
      for (int i = 0; i < 16; ++i) {
        c += mine[i];
        if (c >= want[j]) {
          res[j] = 16 * t + i;
          break;
        }
      }
    }
  }
  __syncthreads();
  return n;
}

__device__ void stain_direction(int b, const double* basis, double* out) {
  const double d = (double)(2 * b + 1) / (double)kNB - 1.0;
  double cx = 1.0 - fabs(d), cy = d;
  const double r = sqrt(cx * cx + cy * cy);
  cx = cx / r, cy = cy / r;
  for (int c = 0; c < 3; ++c) out[c] = basis[c] * cx + basis[3 + c] * cy;
}

__global__ __launch_bounds__(256) void stain_vectors_kernel(const uint32_t* __restrict__ hist, const double* __restrict__ basis,
                                                            const int32_t* __restrict__ basis_status, int permille, double* __restrict__ he_p,
                                                            int32_t* __restrict__ status) {
  __shared__ long long cum[257];
  __shared__ int res[2];
  const long long n = stain_rank_bins(hist, permille, cum, res);
  if (threadIdx.x != 0) return;
  double out[12] = {};
  int st = 0;
  if (basis_status[0] != 0 && n >= 1) {
    double lo[3], hi[3];
    stain_direction(res[0], basis, lo);
    stain_direction(res[1], basis, hi);
    const bool lo_is_h = lo[0] > hi[0];
    const double* h = lo_is_h ? lo : hi;
    const double* e = lo_is_h ? hi : lo;
    const double a = stain_dot(h[0], h[1], h[2], h), b = stain_dot(h[0], h[1], h[2], e), d = stain_dot(e[0], e[1], e[2], e);
    const double det = a * d - b * b;
    if (det > 0.0) {
      st = 1;
      for (int c = 0; c < 3; ++c) {
        out[2 * c] = h[c], out[2 * c + 1] = e[c];
        out[6 + c] = (d * h[c] - b * e[c]) / det;
        out[9 + c] = (a * e[c] - b * h[c]) / det;
      }
    }
  }
  for (int i = 0; i < 12; ++i) he_p[i] = out[i];
  status[0] = st;
}

struct StainTarget {
  double he[6], maxc[2];
};

__global__ __launch_bounds__(256) void stain_matrix_kernel(const uint32_t* __restrict__ chist, const double* __restrict__ he_p,
                                                           const int32_t* __restrict__ vec_status, StainTarget tg, double* __restrict__ m_maxc,
                                                           int32_t* __restrict__ status) {
  __shared__ long long cum[257];
  __shared__ int res[2];
  long long n[2];
  int b[2];
  for (int s = 0; s < 2; ++s) {
    n[s] = stain_rank_bins(chist + s * kNBC, 10, cum, res);
    b[s] = res[1];
  }
  if (threadIdx.x != 0) return;
  double out[11] = {};
  int st = 0;
  if (vec_status[0] != 0 && n[0] >= 1 && n[1] >= 1) {
    st = 1;
    double g[2];
    for (int s = 0; s < 2; ++s) {
      out[9 + s] = (double)(2 * b[s] + 1) / 1024.0;
      g[s] = tg.maxc[s] / out[9 + s];
    }
    for (int c = 0; c < 3; ++c)
      for (int j = 0; j < 3; ++j) out[3 * c + j] = tg.he[2 * c] * (g[0] * he_p[6 + j]) + tg.he[2 * c + 1] * (g[1] * he_p[9 + j]);
  }
  for (int i = 0; i < 11; ++i) m_maxc[i] = out[i];
  status[0] = st;
}

// ---- apply ----------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void stain_apply_kernel(const uint8_t* src, uint8_t* dst, int W, int H, size_t pitch,
                                                          const double* __restrict__ m, const int32_t* __restrict__ status) {
  __shared__ int32_t od[256];
  __shared__ double odf[256];
  __shared__ uint8_t inv[(kOdMax + 1 + 15) / 16 * 16];
  const bool on = status[0] != 0;
  if (!on && src == dst) return;
  double M[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) M[i] = m[i];
  if (on) {
    od[threadIdx.x] = kStainOd[threadIdx.x];
    odf[threadIdx.x] = (double)kStainOd[threadIdx.x];
    __syncthreads();
    for (int q = threadIdx.x; q <= kOdMax; q += 256) {
      int lo = 0, hi = 255;  // the smallest v with od[v] <= q (od decreases; od[255] = 0 <= q)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (od[mid] <= q) hi = mid;
        else lo = mid + 1;
      }
      // od[lo - 1] > q >= od[lo]: the nearer of the two, ties to the larger v
      inv[q] = (uint8_t)((lo > 0 && od[lo - 1] - q < q - od[lo]) ? lo - 1 : lo);
    }
    __syncthreads();
  }
  const unsigned ncx = (unsigned)(W + 15) >> 4;
  const unsigned long long total = (unsigned long long)ncx * (unsigned)H;
  for (unsigned long long p = blockIdx.x * 256ull + threadIdx.x; p < total; p += gridDim.x * 256ull) {
    const unsigned y = (unsigned)p / ncx, cx = (unsigned)p - y * ncx;
    const size_t off = (size_t)y * pitch + (size_t)cx * 48;
    const int valid = W - (int)cx * 16;
    const u32x4* s4 = reinterpret_cast<const u32x4*>(src + off);
    const u32x4 v0 = s4[0], v1 = s4[1], v2 = s4[2];
    uint32_t w[12] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3], v2[0], v2[1], v2[2], v2[3]};
    if (on) {
      uint32_t r[12] = {};
#pragma unroll
      for (int px = 0; px < 16; ++px) {
        double o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int b = 3 * px + c;
          o[c] = odf[(w[b >> 2] >> (8 * (b & 3))) & 0xffu];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int b = 3 * px + c;
          double v = rint((M[3 * c] * o[0] + M[3 * c + 1] * o[1]) + M[3 * c + 2] * o[2]);
          v = v < 0.0 ? 0.0 : (v > (double)kOdMax ? (double)kOdMax : v);
          r[b >> 2] |= (uint32_t)inv[(int)v] << (8 * (b & 3));
        }
      }
#pragma unroll
      for (int i = 0; i < 12; ++i) w[i] = r[i];
    }
    if (valid >= 16) {
      u32x4* d4 = reinterpret_cast<u32x4*>(dst + off);
      d4[0] = u32x4{w[0], w[1], w[2], w[3]};
      d4[1] = u32x4{w[4], w[5], w[6], w[7]};
      d4[2] = u32x4{w[8], w[9], w[10], w[11]};
    } else {
      // the piece with the row's last pixels: bytes behind pixel `width` are not written
      for (int b = 0; b < 3 * valid; ++b) dst[off + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
    }
  }
}

static inline dim3 stain_grid(int width, int height, unsigned cap) {
  const unsigned long long pieces = (unsigned long long)((width + 15) / 16) * (unsigned long long)height;
  const unsigned long long blocks = (pieces + 255) / 256;
  return dim3((unsigned)(blocks < cap ? blocks : cap));
}

// the image conventions of hipac_stain.h; 0 or HIPAC_EINVAL with the message set
static int stain_check_image(const char* who, const void* img, int width, int height, size_t pitch) {
  HIPAC_REQUIRE(width >= 1 && height >= 1, HIPAC_EINVAL, "%s: image %d x %d", who, width, height);
  HIPAC_REQUIRE((unsigned long long)width * (unsigned long long)height < (1ull << 32), HIPAC_EINVAL,
                "%s: image %d x %d (need width * height < 2^32)", who, width, height);
  const size_t row_bytes = (size_t)((width + 15) / 16) * 48;
  HIPAC_REQUIRE(pitch % 48 == 0 && pitch >= row_bytes, HIPAC_EINVAL, "%s: pitch %zu (need a multiple of 48 bytes, at least %zu for %d pixels)",
                who, pitch, row_bytes, width);
  HIPAC_REQUIRE(((uintptr_t)img & 15) == 0, HIPAC_EINVAL, "%s: image not 16-byte aligned", who);
  return 0;
}

static int stain_make_image(const char* who, const uint8_t* img, int width, int height, size_t pitch, const uint8_t* mask, int mw, int mh,
                            int f, int beta_q, StainImage* out) {
  if (int rc = stain_check_image(who, img, width, height, pitch)) return rc;
  HIPAC_REQUIRE(beta_q >= 0 && beta_q <= kOdMax, HIPAC_EINVAL, "%s: beta_q %d outside 0..%d", who, beta_q, kOdMax);
  int fshift = 0;
  if (mask) {
    HIPAC_REQUIRE(f == 4 || f == 8 || f == 16 || f == 32, HIPAC_EINVAL, "%s: f %d (need 4, 8, 16 or 32 level pixels per mask pixel)", who, f);
    const int want_w = (int)(((long long)width + f - 1) / f), want_h = (int)(((long long)height + f - 1) / f);
    HIPAC_REQUIRE(mw == want_w && mh == want_h, HIPAC_EINVAL, "%s: mask %d x %d (a %d x %d level at f %d has %d x %d)", who, mw, mh, width,
                  height, f, want_w, want_h);
    fshift = f == 4 ? 2 : (f == 8 ? 3 : (f == 16 ? 4 : 5));
  }
  *out = StainImage{img, width, height, pitch, mask, mw, fshift, beta_q};
  return 0;
}

}  // namespace hipac

extern "C" int hipac_stain_abi_version(void) { return HIPAC_STAIN_ABI_VERSION; }

extern "C" int hipac_stain_od_table(int32_t* od) {
  using namespace hipac;
  HIPAC_REQUIRE(od, HIPAC_EINVAL, "stain_od_table: null argument");
  for (int i = 0; i < 256; ++i) od[i] = kStainOdHost[i];
  return 0;
}

extern "C" int hipac_stain_moments(const uint8_t* img, int width, int height, size_t pitch, const uint8_t* mask, int mw, int mh, int f,
                                   int beta_q, int64_t* moments, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(img && moments, HIPAC_EINVAL, "stain_moments: null argument");
  StainImage g;
  if (int rc = stain_make_image("stain_moments", img, width, height, pitch, mask, mw, mh, f, beta_q, &g)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIPAC_CHECK_HIP(hipMemsetAsync(moments, 0, 10 * sizeof(int64_t), s));
  hipLaunchKernelGGL(stain_moments_kernel, stain_grid(width, height, kStainReduceBlocks), dim3(256), 0, s, g,
                     reinterpret_cast<unsigned long long*>(moments));
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_stain_basis(const int64_t* moments, double* basis, int32_t* status, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(moments && basis && status, HIPAC_EINVAL, "stain_basis: null argument");
  hipLaunchKernelGGL(stain_basis_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<const long long*>(moments), basis,
                     status);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_stain_angle_hist(const uint8_t* img, int width, int height, size_t pitch, const uint8_t* mask, int mw, int mh, int f,
                                      int beta_q, const double* basis, uint32_t* hist, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(img && basis && hist, HIPAC_EINVAL, "stain_angle_hist: null argument");
  StainImage g;
  if (int rc = stain_make_image("stain_angle_hist", img, width, height, pitch, mask, mw, mh, f, beta_q, &g)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIPAC_CHECK_HIP(hipMemsetAsync(hist, 0, kNB * sizeof(uint32_t), s));
  hipLaunchKernelGGL(stain_angle_kernel, stain_grid(width, height, kStainReduceBlocks), dim3(256), 0, s, g, basis, hist);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_stain_vectors(const uint32_t* hist, const double* basis, const int32_t* basis_status, int alpha_permille, double* he_p,
                                   int32_t* status, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(hist && basis && basis_status && he_p && status, HIPAC_EINVAL, "stain_vectors: null argument");
  HIPAC_REQUIRE(alpha_permille >= 1 && alpha_permille <= HIPAC_STAIN_MAX_ALPHA, HIPAC_EINVAL, "stain_vectors: alpha_permille %d outside 1..%d",
                alpha_permille, HIPAC_STAIN_MAX_ALPHA);
  hipLaunchKernelGGL(stain_vectors_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, hist, basis, basis_status, alpha_permille, he_p,
                     status);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_stain_conc_hist(const uint8_t* img, int width, int height, size_t pitch, const uint8_t* mask, int mw, int mh, int f,
                                     int beta_q, const double* he_p, uint32_t* chist, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(img && he_p && chist, HIPAC_EINVAL, "stain_conc_hist: null argument");
  StainImage g;
  if (int rc = stain_make_image("stain_conc_hist", img, width, height, pitch, mask, mw, mh, f, beta_q, &g)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIPAC_CHECK_HIP(hipMemsetAsync(chist, 0, 2 * kNBC * sizeof(uint32_t), s));
  hipLaunchKernelGGL(stain_conc_kernel, stain_grid(width, height, kStainReduceBlocks), dim3(256), 0, s, g, he_p, chist);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_stain_matrix(const uint32_t* chist, const double* he_p, const int32_t* vec_status, const double* target, double* m_maxc,
                                  int32_t* status, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(chist && he_p && vec_status && target && m_maxc && status, HIPAC_EINVAL, "stain_matrix: null argument");
  StainTarget tg;
  for (int i = 0; i < 6; ++i) tg.he[i] = target[i];
  tg.maxc[0] = target[6], tg.maxc[1] = target[7];
  for (int i = 0; i < 8; ++i)
    HIPAC_REQUIRE(target[i] - target[i] == 0.0, HIPAC_EINVAL, "stain_matrix: target[%d] is not finite", i);
  HIPAC_REQUIRE(tg.maxc[0] > 0.0 && tg.maxc[1] > 0.0, HIPAC_EINVAL, "stain_matrix: target maxC %g, %g (need both > 0)", tg.maxc[0], tg.maxc[1]);
  hipLaunchKernelGGL(stain_matrix_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, chist, he_p, vec_status, tg, m_maxc, status);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_stain_apply(const uint8_t* src, uint8_t* dst, int width, int height, size_t pitch, const double* m, const int32_t* status,
                                 void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(src && dst && m && status, HIPAC_EINVAL, "stain_apply: null argument");
  if (int rc = stain_check_image("stain_apply", src, width, height, pitch)) return rc;
  HIPAC_REQUIRE(((uintptr_t)dst & 15) == 0, HIPAC_EINVAL, "stain_apply: destination not 16-byte aligned");
  const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst, bytes = (uintptr_t)height * pitch;
  HIPAC_REQUIRE(a == b || a + bytes <= b || b + bytes <= a, HIPAC_EINVAL,
                "stain_apply: src and dst overlap partly (need dst == src or disjoint images)");
  hipLaunchKernelGGL(stain_apply_kernel, stain_grid(width, height, kStainApplyBlocks), dim3(256), 0, (hipStream_t)stream, src, dst, width,
                     height, pitch, m, status);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

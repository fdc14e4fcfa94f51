// The per-pixel arithmetic of the HED stain augmentation (include/hipac_augment_hed.h), shared by the colour kernel's load of a
// view into LDS and by the stand-alone stage (augment.hip).  Optical densities come from the literal table of stain_od.h; the
// map is IEEE double with one rounding per operation in the order of tests/augment_hed_cpu.py (-ffp-contract=off, build.py).
//
// The inverse.  stain_apply_kernel keeps inv[] (22.7 KB, one byte per optical density) in LDS; next to a whole view (147 KB)
// there is no room for it.  The table is strictly decreasing with steps of at least 16, so the midpoints between neighbouring
// entries, where inv[] changes, are at least 16 apart: over a bucket of 16 consecutive optical densities inv[] changes at most once,
// and then by one.  kHedBuckets uint16 entries (2.8 KB) hold, per bucket k, v0 = inv[16 k] and the first offset s in 1 .. 15 at which
// inv[16 k + s] = v0 - 1 (16: nowhere): inv[t] = v0 - ((t & 15) >= s), one LDS read and four integer operations, exactly
// stain_apply_kernel's rule (nearest entry, ties to the larger v).  Every workgroup builds the buckets in its prologue from the
// literal table (a binary search per bucket).
#pragma once

#include "common.h"
#include "stain_od.h"

namespace hipac {

constexpr int kHedPayload = 12;  // doubles per view: A[3][3] row-major, then bq[3]
constexpr int kHedOdMax = 22713;
constexpr int kHedBuckets = (kHedOdMax >> 4) + 1;  // 1420
constexpr int kHedTableBytes = 256 * (int)sizeof(double) + (kHedBuckets + 3) / 4 * 4 * (int)sizeof(uint16_t);  // od[] as double, the buckets

// odf[256] and inv16[kHedBuckets] in LDS from od[256] (constant memory), by all `threads` threads of the workgroup; ends in a barrier
__device__ __forceinline__ void hed_build_tables(const int32_t* od, double* odf, uint16_t* inv16, int tid, int threads) {
  for (int v = tid; v < 256; v += threads) odf[v] = (double)od[v];
  for (int k = tid; k < kHedBuckets; k += threads) {
    const int t0 = 16 * k;
    int lo = 0, hi = 255;  // the smallest v with od[v] <= t0 (od decreases; od[255] = 0 <= t0)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (od[mid] <= t0) hi = mid;
      else lo = mid + 1;
    }
    // od[lo - 1] > t0 >= od[lo]: the nearer of the two, ties to the larger v
    const int v0 = (lo > 0 && od[lo - 1] - t0 < t0 - od[lo]) ? lo - 1 : lo;
    // inv[] leaves v0 behind the midpoint of od[v0 - 1] and od[v0] (the midpoint itself is a tie: v0)
    int s = 16;
    if (v0 > 0) {
      const int first = (od[v0 - 1] + od[v0]) / 2 + 1 - t0;  // >= 1, since inv[t0] = v0
      s = first < 16 ? first : 16;
    }
    inv16[k] = (uint16_t)(v0 | (s << 8));
  }
  __syncthreads();
}

// 0 <= t <= od[0]
__device__ __forceinline__ int hed_inverse(const uint16_t* inv16, int t) {
  const int e = inv16[t >> 4];
  return (e & 255) - ((t & 15) >= (e >> 8) ? 1 : 0);
}

// one pixel: m = the view's payload in registers, odf = od[] as double in LDS
__device__ __forceinline__ void hed_pixel(const double* odf, const uint16_t* inv16, const double* m, int& r, int& g, int& b) {
  const double o0 = odf[r], o1 = odf[g], o2 = odf[b];
  int out[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double t = rint(((m[3 * c] * o0 + m[3 * c + 1] * o1) + m[3 * c + 2] * o2) + m[9 + c]);
    t = fmin(fmax(t, 0.0), (double)kHedOdMax);  // fmax drops a NaN: it counts as 0, and the index stays inside the table
    out[c] = hed_inverse(inv16, (int)t);
  }
  r = out[0], g = out[1], b = out[2];
}

// four pixels = 12 bytes = three dwords, the unit in which both kernels walk a view (150 528 bytes = 12 544 such groups)
__device__ __forceinline__ void hed_group(const double* odf, const uint16_t* inv16, const double* m, unsigned& w0, unsigned& w1, unsigned& w2) {
  const unsigned w[3] = {w0, w1, w2};
  unsigned res[3] = {0u, 0u, 0u};
#pragma unroll
  for (int px = 0; px < 4; ++px) {
    int v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int byte = 3 * px + c;
      v[c] = (int)((w[byte >> 2] >> (8 * (byte & 3))) & 0xffu);
    }
    hed_pixel(odf, inv16, m, v[0], v[1], v[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int byte = 3 * px + c;
      res[byte >> 2] |= (unsigned)v[c] << (8 * (byte & 3));
    }
  }
  w0 = res[0], w1 = res[1], w2 = res[2];
}

}  // namespace hipac

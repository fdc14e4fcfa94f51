// Test-time augmentation of the detector (include/hipac_tta.h): the eight dihedral views of uint8[n][224][224][3] patches and
// the reduction of the per-view logits.
//
// The unit of every global access is a QUAD: 4 whole RGB pixels = 12 bytes = one global_load/store_dwordx3 per lane.  A row is 56
// quads and no pixel straddles two lanes, so a view never needs a neighbour lane's bytes (no cross-lane operation anywhere), and
// consecutive lanes touch consecutive quads: every wave-wide load or store covers contiguous runs of whole (tile) rows.
//
//   r even   no transposition: out row i is in row i or 223 - i, with the quads (and the pixels inside a quad) in the same or the
//            reverse order.  Registers only; a workgroup moves 1792 consecutive output quads = 32 rows = 21 504 contiguous bytes,
//            read from 32 whole rows as well.
//   r odd    rows become columns: 112 x 112 pixel tiles (2 x 2 per patch; 112 divides 224, there is no edge tile) through LDS.
//            A 32-lane half of a wave owns one tile row: lanes 0..27 one quad each (336 contiguous bytes), lanes 28..31 idle --
//            so no half ever spans two rows, in the load phase or in the store phase.
//
// LDS layout of the transposing kernel: one dword per pixel, tile[R(a)][C(c)] with a pitch of 113 dwords, where source row a and
// source column c are stored de-interleaved by their position in a quad: R(a) = (a % 4) * 28 + a / 4, C(c) = (c % 4) * 28 + c / 4.
// Bank = (byte address / 4) % 32 for ds_write_b32 and ds_read_b32, conflicts counted per 32-lane half:
//   write  instruction k of a half stores pixel k of the lanes' quads: row R(a) fixed, columns k * 28 + t for lanes t = 0..27:
//          28 consecutive dwords, 28 distinct banks.
//   read   instruction k of a half fetches, for one fixed column C(c), the rows k * 28 + t (or, when the view reverses the source
//          rows, (3 - k) * 28 + 27 - t): a stride of +-113 dwords = +-17 banks, and 17 is odd, so the 28 lanes hit 28 distinct banks.
// Both phases are conflict-free; without the de-interleaving a lane's pixel k would sit at 4 t + k, a bank stride of 4 (or 4 * 113),
// which is an 8-bank, 4-way conflict on one of the two sides whatever the pitch.
#include "common.h"

#include "../../include/hipac_tta.h"
#include "detect_prob.h"

namespace hipac {

constexpr int kSide = HIPAC_TTA_SIDE;
constexpr int kRowBytes = kSide * 3;                        // 672
constexpr size_t kPatchBytes = (size_t)kSide * kRowBytes;   // 150 528
constexpr int kRowQuads = kSide / 4;                        // 56
constexpr int kFlipParts = 7, kFlipQuads = 7;               // even views: 7 workgroups per patch, 7 quads per thread (7 * 7 * 256 = 224 * 56)
constexpr int kTile = 112, kTileQuads = kTile / 4, kPitch = kTile + 1;
constexpr int kTilePasses = kTile / 8;                      // 4 waves x 2 halves = 8 tile rows per pass
constexpr int kMaxPatches = 1 << 28;                        // 7 n workgroups stay below 2^31
static_assert(kFlipParts * kFlipQuads * 256 == kSide * kRowQuads && 2 * kTile == kSide && kTile % 8 == 0 && (kPitch & 1), "tiling");

struct Quad {
  uint32_t d[3];  // 4 pixels, 3 bytes each, as they lie in memory (little endian)
};

__device__ __forceinline__ Quad load_quad(const uint8_t* p) { return *reinterpret_cast<const Quad*>(p); }
__device__ __forceinline__ void store_quad(uint8_t* p, const Quad& q) { *reinterpret_cast<Quad*>(p) = q; }

// px[k] = 0x00BBGGRR of pixel k
__device__ __forceinline__ void unpack_quad(const Quad& q, uint32_t (&px)[4]) {
  px[0] = q.d[0] & 0xffffffu;
  px[1] = (q.d[0] >> 24) | ((q.d[1] & 0xffffu) << 8);
  px[2] = (q.d[1] >> 16) | ((q.d[2] & 0xffu) << 16);
  px[3] = q.d[2] >> 8;
}

__device__ __forceinline__ Quad pack_quad(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) {
  Quad q;
  q.d[0] = p0 | (p1 << 24);
  q.d[1] = (p1 >> 8) | (p2 << 16);
  q.d[2] = (p2 >> 16) | (p3 << 8);
  return q;
}

// r = 0, 2.  grid: 7 workgroups per patch
template <bool kRowRev, bool kColRev>
__global__ __launch_bounds__(256) void tta_flip_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
  const size_t patch = blockIdx.x / kFlipParts;
  const int first = (int)(blockIdx.x % kFlipParts) * (kFlipQuads * 256) + (int)threadIdx.x;
  const uint8_t* src = in + patch * kPatchBytes;
  uint8_t* dst = out + patch * kPatchBytes;
  Quad q[kFlipQuads];
#pragma unroll
  for (int k = 0; k < kFlipQuads; ++k) {
    const int piece = first + k * 256, i = piece / kRowQuads, t = piece - i * kRowQuads;
    const int a = kRowRev ? kSide - 1 - i : i, ts = kColRev ? kRowQuads - 1 - t : t;
    q[k] = load_quad(src + a * kRowBytes + ts * 12);
  }
#pragma unroll
  for (int k = 0; k < kFlipQuads; ++k) {
    Quad o = q[k];
    if (kColRev) {
      uint32_t px[4];
      unpack_quad(q[k], px);
      o = pack_quad(px[3], px[2], px[1], px[0]);
    }
    store_quad(dst + (size_t)(first + k * 256) * 12, o);
  }
}

// r = 1, 3: out[i][j] = x[a][c], a = kRowRev ? 223 - j : j, c = kColRev ? 223 - i : i.  grid: 4 workgroups (tiles) per patch
template <bool kRowRev, bool kColRev>
__global__ __launch_bounds__(256) void tta_transpose_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
  __shared__ uint32_t tile[kTile * kPitch];  // 50 624 bytes: three workgroups per CU
  const size_t patch = blockIdx.x >> 2;
  const int i0 = (int)((blockIdx.x >> 1) & 1) * kTile, j0 = (int)(blockIdx.x & 1) * kTile;  // the output tile
  const int a0 = kRowRev ? kSide - kTile - j0 : j0, c0 = kColRev ? kSide - kTile - i0 : i0;   // the source tile
  const int t = threadIdx.x & 31, row = threadIdx.x >> 5;  // row 0..7 of a pass: (wave, half)
  const bool active = t < kTileQuads;  // four lanes of every half idle; the barrier below stays in uniform control flow
  const uint8_t* src = in + patch * kPatchBytes + (size_t)a0 * kRowBytes + (c0 + 4 * t) * 3;
  Quad q[kTilePasses];
#pragma unroll
  for (int pass = 0; pass < kTilePasses; ++pass)  // all fourteen loads in flight before the first LDS store
    if (active) q[pass] = load_quad(src + (pass * 8 + row) * kRowBytes);
  if (active) {
#pragma unroll
    for (int pass = 0; pass < kTilePasses; ++pass) {
      const int la = pass * 8 + row;
      uint32_t px[4];
      unpack_quad(q[pass], px);
      uint32_t* w = tile + ((la & 3) * kTileQuads + (la >> 2)) * kPitch + t;
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k * kTileQuads] = px[k];
    }
  }
  __syncthreads();
  if (!active) return;
  uint8_t* dst = out + patch * kPatchBytes + (size_t)i0 * kRowBytes + (j0 + 4 * t) * 3;
#pragma unroll
  for (int pass = 0; pass < kTilePasses; ++pass) {
    const int li = pass * 8 + row, lc = kColRev ? kTile - 1 - li : li;
    const uint32_t* r = tile + (lc & 3) * kTileQuads + (lc >> 2);
    uint32_t px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // source row la = 4 t + k, or 111 - (4 t + k) = 4 (27 - t) + (3 - k)
      const int R = kRowRev ? (3 - k) * kTileQuads + (kTileQuads - 1 - t) : k * kTileQuads + t;
      px[k] = r[R * kPitch];
    }
    store_quad(dst + li * kRowBytes, pack_quad(px[0], px[1], px[2], px[3]));
  }
}

__global__ __launch_bounds__(256) void tta_reduce_kernel(const float* __restrict__ logits, int views, int n, int tumor,
                                                         float* __restrict__ p, float* __restrict__ range) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float sum = tumor_prob(logits, (size_t)i, tumor);
  float lo = sum, hi = sum;
  bool nan = sum != sum;
  for (int v = 1; v < views; ++v) {
    const float pv = tumor_prob(logits, (size_t)v * n + i, tumor);
    sum = sum + pv;
    lo = pv < lo ? pv : lo;
    hi = pv > hi ? pv : hi;
    nan |= pv != pv;
  }
  p[i] = sum / (float)views;
  if (range) range[i] = nan ? sum : hi - lo;  // a NaN view makes `sum` NaN
}

}  // namespace hipac

extern "C" int hipac_tta_abi_version(void) { return HIPAC_TTA_ABI_VERSION; }

extern "C" int hipac_tta_view(const uint8_t* in, int n, int view, uint8_t* out, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(in && out, HIPAC_EINVAL, "tta_view: null argument");
  HIPAC_REQUIRE(n >= 0 && n < kMaxPatches, HIPAC_EINVAL, "tta_view: n %d outside 0..2^28 - 1", n);
  HIPAC_REQUIRE(view >= 0 && view < HIPAC_TTA_VIEWS, HIPAC_EINVAL, "tta_view: view %d outside 0..%d", view, HIPAC_TTA_VIEWS - 1);
  HIPAC_REQUIRE(((uintptr_t)in | (uintptr_t)out) % 4 == 0, HIPAC_EINVAL, "tta_view: in and out must be 4-byte aligned");
  const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out, bytes = (uintptr_t)n * kPatchBytes;
  HIPAC_REQUIRE(a + bytes <= b || b + bytes <= a, HIPAC_EINVAL,
                "tta_view: the byte ranges of in and out intersect (the view is not made in place)");
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int r = view & 3, f = view >> 2;
  if ((r & 1) == 0) {
    const bool row_rev = r == 2, col_rev = (r == 2) != (f == 1);
    const dim3 grid((unsigned)n * kFlipParts);
    if (row_rev && col_rev) hipLaunchKernelGGL((tta_flip_kernel<true, true>), grid, dim3(256), 0, s, in, out);
    else if (row_rev) hipLaunchKernelGGL((tta_flip_kernel<true, false>), grid, dim3(256), 0, s, in, out);
    else if (col_rev) hipLaunchKernelGGL((tta_flip_kernel<false, true>), grid, dim3(256), 0, s, in, out);
    else hipLaunchKernelGGL((tta_flip_kernel<false, false>), grid, dim3(256), 0, s, in, out);
  } else {
    const bool row_rev = r == 3, col_rev = (r == 1) != (f == 1);
    const dim3 grid((unsigned)n * 4);
    if (row_rev && col_rev) hipLaunchKernelGGL((tta_transpose_kernel<true, true>), grid, dim3(256), 0, s, in, out);
    else if (row_rev) hipLaunchKernelGGL((tta_transpose_kernel<true, false>), grid, dim3(256), 0, s, in, out);
    else if (col_rev) hipLaunchKernelGGL((tta_transpose_kernel<false, true>), grid, dim3(256), 0, s, in, out);
    else hipLaunchKernelGGL((tta_transpose_kernel<false, false>), grid, dim3(256), 0, s, in, out);
  }
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int hipac_tta_reduce(const float* logits, int views, int n, int tumor_class, float* p, float* range, void* stream) {
  using namespace hipac;
  HIPAC_REQUIRE(views >= 1 && views <= HIPAC_TTA_VIEWS, HIPAC_EINVAL, "tta_reduce: views %d outside 1..%d", views, HIPAC_TTA_VIEWS);
  HIPAC_REQUIRE(n >= 0, HIPAC_EINVAL, "tta_reduce: n %d", n);
  HIPAC_REQUIRE(tumor_class == 0 || tumor_class == 1, HIPAC_EINVAL, "tta_reduce: tumor_class %d (two classes: 0 or 1)", tumor_class);
  if (n == 0) return 0;
  HIPAC_REQUIRE(logits && p, HIPAC_EINVAL, "tta_reduce: null argument");
  hipLaunchKernelGGL(tta_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits, views, n,
                     tumor_class, p, range);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

// TIFF LZW tiles decoded on the device (include/hipac_lzw.h; the definition is tiff_pyramid.lzw_decode).
//
//   lzw_decode_kernel   one tile = one stream = one wavefront (a workgroup of 64).  The code parse is serial and wave-uniform: the
//               compressed bytes are fetched 256 at a time, one big-endian dword per lane, and a code is cut out of a 64-bit
//               window refilled through v_readlane.  A table entry is (offset of one earlier occurrence of the string in this
//               tile's own output, length - 1) in one dword, so emitting a code is a copy inside the tile's scratch that the 64
//               lanes do together; the entry a code adds is "previous string + first byte of this one", which is exactly the
//               bytes at the previous string's position, one longer.  A Clear resets the entry count and nothing else.  The
//               table is 4096 dwords = 16 KiB of LDS: ten tiles are resident per CU.
//               A copy reads bytes the wave stored earlier: before a copy whose source reaches past the last fence the wave
//               waits for its stores (vmcnt(0); the CU's L1 is write-through and the wave's own).
//   lzw_place_kernel    undoes the predictor and places the tile into its level, clipped (tile_place.h, shared with deflate.hip).
//
// Safety: every offset is checked or clamped before use -- a tile descriptor against the file and its level, a code against
// the entry count, an entry against the bytes already written, every copy against the tile size, every fetch against the
// stream's end.  A wrong stream ends as status 1, never as an access outside the scratch, the table or the file.
#include "common.h"

#include <cstring>

#include "../../include/hipac_lzw.h"
#include "tile_place.h"

namespace hipac {

struct LzwLevels {
  hipac_lzw_level l[HIPAC_LZW_MAX_LEVELS];
  int n;
};

constexpr int kLzwEntries = 4096, kLzwOffBits = 20;
static_assert(HIPAC_LZW_MAX_TILE_BYTES == 1 << kLzwOffBits, "an entry keeps the offset in 20 bits and length - 1 in 12");

__device__ __forceinline__ uint32_t lzw_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// big-endian dword `d0 + lane` of the stream [p, p + len): bytes behind the end read as 0 and are not fetched
__device__ __forceinline__ uint32_t lzw_fetch(const uint8_t* p, long long len, long long d0, int lane) {
  const long long b = 4 * (d0 + lane);
  uint32_t w = 0;
  if (b + 4 <= len) {
    __builtin_memcpy(&w, p + b, 4);
    return __builtin_bswap32(w);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (b + k < len) w |= (uint32_t)p[b + k] << (24 - 8 * k);
  return w;
}

__global__ __launch_bounds__(64) void lzw_decode_kernel(const uint8_t* __restrict__ file, long long file_bytes, LzwLevels lv,
                                                        const long long* __restrict__ tile_off, const long long* __restrict__ tile_len,
                                                        const int* __restrict__ tile_xyl, uint8_t* scratch, long long stride,
                                                        uint8_t* __restrict__ status) {
  __shared__ uint32_t tab[kLzwEntries];
  const int t = blockIdx.x, lane = threadIdx.x;
  const long long off = tile_off[t], len = tile_len[t];
  const int x = tile_xyl[3 * t], y = tile_xyl[3 * t + 1], li = tile_xyl[3 * t + 2];
  int st = HIPAC_LZW_OK;
  if (len == 0) st = HIPAC_LZW_MISSING;
  if (len < 0 || off < 0 || off > file_bytes || len > file_bytes - off || li < 0 || li >= lv.n) st = HIPAC_LZW_BAD_TILE;
  uint32_t n_out = 0;
  if (st == HIPAC_LZW_OK) {
    const hipac_lzw_level& L = lv.l[li];
    if (x < 0 || y < 0 || x >= L.W || y >= L.H || x % L.tile_w || y % L.tile_h) st = HIPAC_LZW_BAD_TILE;
    n_out = (uint32_t)L.tile_w * (uint32_t)L.tile_h * (uint32_t)L.samples;  // <= stride: checked on the host
  }
  if (st != HIPAC_LZW_OK) {
    if (lane == 0) status[t] = (uint8_t)st;
    return;
  }
  const uint8_t* src = file + off;
  uint8_t* out = scratch + (long long)t * stride;

  bool bad = len >= 2 && src[0] == 0 && (src[1] & 1);  // the old LSB-first variant (libtiff's test)
  long long bits_left = 8 * len, next_dword = 0;
  unsigned long long acc = 0;  // the low `nb` bits are the next bits of the stream
  uint32_t chunk = 0, nb = 0, width = 9, next = 258, opos = 0, fenced = 0, prev_pos = 0, prev_len = 0;
  bool have_prev = false, first = true;
  while (!bad && opos < n_out && bits_left >= (long long)width) {
    if (nb < width) {  // at most 11 bits are left: 32 more fit
      if ((next_dword & 63) == 0) chunk = lzw_fetch(src, len, next_dword, lane);
      const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)chunk, (int)lzw_uniform((uint32_t)next_dword & 63u));
      acc = (acc << 32) | w;
      nb += 32;
      ++next_dword;
    }
    nb -= width;
    bits_left -= width;
    const uint32_t code = (uint32_t)(acc >> nb) & ((1u << width) - 1u);  // < 4096
    if (code == 257) {
      bad = first;
      break;
    }
    first = false;
    if (code == 256) {
      next = 258, width = 9, have_prev = false;
      continue;
    }
    uint32_t from, n;  // the string: n bytes at out + from, or the literal `code`
    if (code < 256) {
      from = 0, n = 1;
    } else if (!have_prev) {
      bad = true;  // the code after a Clear, or the first one, is no literal
      break;
    } else if (code < next) {
      const uint32_t e = lzw_uniform(tab[code]);
      from = e & ((1u << kLzwOffBits) - 1u), n = (e >> kLzwOffBits) + 1;
    } else if (code == next && next < kLzwEntries) {
      from = prev_pos, n = prev_len + 1;  // KwKwK: the previous string and its first byte again
    } else {
      bad = true;  // larger than the next free entry
      break;
    }
    if (have_prev && next < kLzwEntries) {
      if (prev_len >= (uint32_t)kLzwEntries) {
        bad = true;  // cannot happen (an entry is at most one longer than the entry count): kept as a bound on the length field
        break;
      }
      tab[next] = prev_pos | (prev_len << kLzwOffBits);  // every lane stores the same dword: previous string + one byte
      ++next;
      if (next + 1 >= (1u << width) && width < 12) ++width;
    }
    const uint32_t m = min(n, n_out - opos);
    if (code < 256) {
      if (lane == 0) out[opos] = (uint8_t)code;
    } else {
      // from < opos and from + n <= opos + 1 for every entry the parse above makes; checked all the same
      if (from >= opos || from + n > opos + 1) {
        bad = true;
        break;
      }
      if (from + n > fenced) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): a one-wave workgroup's fence is no wait by itself
        fenced = opos;
      }
      for (uint32_t i = lane; i < m; i += 64) {
        uint32_t s = from + i;
        if (s >= opos) s = from;  // the last byte of KwKwK is the first byte
        out[opos + i] = out[s];
      }
    }
    prev_pos = opos, prev_len = n, have_prev = true;
    opos += m;
  }
  if (!bad)
    for (uint32_t i = opos + lane; i < n_out; i += 64) out[i] = 0;  // a stream that ends early leaves zeros
  if (lane == 0) status[t] = bad ? HIPAC_LZW_REFUSED : HIPAC_LZW_OK;
}

static_assert(HIPAC_LZW_OK == 0 && HIPAC_LZW_REFUSED == 1, "tile_place.h takes these two values");

__global__ __launch_bounds__(256) void lzw_place_kernel(LzwLevels lv, const int* __restrict__ tile_xyl, const uint8_t* __restrict__ status,
                                                        const uint8_t* __restrict__ scratch, long long stride) {
  tile_place(lv, tile_xyl, status, scratch, stride);
}

static size_t lzw_tile_stride(int tile_w, int tile_h, int samples) { return align256((size_t)tile_w * tile_h * samples); }

static bool lzw_tile_ok(int tile_w, int tile_h, int samples) {
  return tile_w >= 1 && tile_h >= 1 && (samples == 1 || samples == 3 || samples == 4) &&
         (long long)tile_w * tile_h * samples <= HIPAC_LZW_MAX_TILE_BYTES;
}

}  // namespace hipac

using namespace hipac;

extern "C" int hipac_lzw_abi_version(void) { return HIPAC_LZW_ABI_VERSION; }

extern "C" size_t hipac_lzw_workspace_bytes(int tile_w, int tile_h, int samples, int n_tiles) {
  if (!lzw_tile_ok(tile_w, tile_h, samples) || n_tiles < 1 || n_tiles > HIPAC_LZW_MAX_TILES) return 0;
  return (size_t)n_tiles * lzw_tile_stride(tile_w, tile_h, samples);
}

extern "C" int hipac_lzw_decode_tiles(const uint8_t* file_dev, int64_t file_bytes, const hipac_lzw_level* levels, int n_levels,
                                      const int64_t* tile_off, const int64_t* tile_len, const int32_t* tile_xyl, int n_tiles,
                                      void* workspace, size_t workspace_bytes, uint8_t* status_dev, void* stream) {
  HIPAC_REQUIRE(file_dev && levels && tile_off && tile_len && tile_xyl && workspace && status_dev, HIPAC_EINVAL,
                "lzw_decode_tiles: null argument");
  HIPAC_REQUIRE(file_bytes >= 0, HIPAC_EINVAL, "lzw_decode_tiles: file_bytes %lld", (long long)file_bytes);
  HIPAC_REQUIRE(n_tiles >= 1 && n_tiles <= HIPAC_LZW_MAX_TILES, HIPAC_EINVAL, "lzw_decode_tiles: n_tiles %d outside 1..%d", n_tiles,
                HIPAC_LZW_MAX_TILES);
  HIPAC_REQUIRE(n_levels >= 1 && n_levels <= HIPAC_LZW_MAX_LEVELS, HIPAC_EINVAL, "lzw_decode_tiles: n_levels %d outside 1..%d", n_levels,
                HIPAC_LZW_MAX_LEVELS);
  LzwLevels lv;
  std::memset(&lv, 0, sizeof(lv));
  lv.n = n_levels;
  size_t stride = 0;
  int max_th = 0;
  for (int l = 0; l < n_levels; ++l) {
    const hipac_lzw_level& L = levels[l];
    HIPAC_REQUIRE(L.pixels && L.W >= 1 && L.H >= 1 && L.pitch_bytes >= (int64_t)L.W * 3, HIPAC_EINVAL,
                  "lzw_decode_tiles: bad geometry of level %d", l);
    HIPAC_REQUIRE(lzw_tile_ok(L.tile_w, L.tile_h, L.samples), HIPAC_EINVAL,
                  "lzw_decode_tiles: level %d: tile %d x %d x %d samples (need samples 1, 3 or 4 and at most %d bytes)", l, L.tile_w,
                  L.tile_h, L.samples, HIPAC_LZW_MAX_TILE_BYTES);
    HIPAC_REQUIRE(L.predictor == 1 || L.predictor == 2, HIPAC_EINVAL, "lzw_decode_tiles: level %d: predictor %d (need 1 or 2)", l,
                  L.predictor);
    lv.l[l] = L;
    const size_t s = lzw_tile_stride(L.tile_w, L.tile_h, L.samples);
    stride = s > stride ? s : stride;
    max_th = L.tile_h > max_th ? L.tile_h : max_th;
  }
  HIPAC_REQUIRE(((uintptr_t)workspace & 255) == 0, HIPAC_EINVAL, "lzw_decode_tiles: workspace not 256-byte aligned");
  HIPAC_REQUIRE(workspace_bytes >= (size_t)n_tiles * stride, HIPAC_EWORKSPACE,
                "lzw_decode_tiles: workspace %zu bytes, %zu needed (hipac_lzw_workspace_bytes of the largest tile)", workspace_bytes,
                (size_t)n_tiles * stride);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lzw_decode_kernel, dim3((unsigned)n_tiles), dim3(64), 0, s, file_dev, (long long)file_bytes, lv,
                     (const long long*)tile_off, (const long long*)tile_len, (const int*)tile_xyl, (uint8_t*)workspace, (long long)stride,
                     status_dev);
  hipLaunchKernelGGL(lzw_place_kernel, dim3((unsigned)((max_th + 15) / 16), (unsigned)n_tiles), dim3(256), 0, s, lv, (const int*)tile_xyl,
                     (const uint8_t*)status_dev, (const uint8_t*)workspace, (long long)stride);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

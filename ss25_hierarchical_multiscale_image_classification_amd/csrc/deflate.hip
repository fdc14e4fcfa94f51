// TIFF deflate tiles decoded on the device (include/hipac_deflate.h; the definition is tiff_pyramid.inflate, which agrees with zlib).
//
//   deflate_decode_kernel   one tile = one zlib stream = one wavefront (a workgroup of 64).  The symbol parse is serial and
//               wave-uniform: the compressed bytes are fetched 256 at a time, one little-endian dword per lane, and fed through
//               v_readlane into a 64-bit window whose low bits are the next bits of the stream.
//               A Huffman code is kept in canonical form (RFC 1951 3.2.2): lane L of the wave holds, for the codes of length L,
//               the first code, their number and where their symbols start in a table of symbols sorted by (length, symbol) in
//               LDS.  To decode, every lane 1..15 cuts its own L bits out of the window (MSB first), tests "first <= code <
//               first + count", and one ballot gives the length: the lowest lane that hit.  A bit pattern no code owns hits in no
//               lane.  The tables are built by the lanes together: lane L counts and then places the symbols of length L.  LDS
//               per tile is 1.1 KiB (code lengths, three symbol tables, 16 counts), so the register file and not the LDS bounds
//               the tiles per CU.
//               The 32 KiB window is the tile's own output in scratch.  A match is copied by the 64 lanes together;
//               out[i] = out[i - d] with d < length repeats the last d bytes, so lane i reads out[from + i % d], all of it
//               written before the match began.  A copy reads bytes the wave stored earlier: before a copy whose source
//               reaches past the last fence the wave waits for its stores (vmcnt(0); the CU's L1 is write-through and the
//               wave's own).  Adler-32 is two sums over the finished tile, taken a dword per lane and reduced with shuffles.
//   deflate_place_kernel    undoes the predictor and places the tile into its level, clipped (tile_place.h, shared with lzw.hip).
//
// Safety: every offset is checked before use -- a tile descriptor against the file and its level, every bit taken against the
// stream's end (bytes behind it are not fetched and read as 0), every index into a table of code lengths or symbols against
// the table, every distance against the bytes written, every copy against the tile size.  A wrong stream ends as status 1,
// never as an access outside the scratch, the tables or the file.
#include "common.h"

#include <cstring>

#include "../../include/hipac_deflate.h"
#include "tile_place.h"
#include "wave_reduce.h"

namespace hipac {

struct DeflateLevels {
  hipac_deflate_level l[HIPAC_DEFLATE_MAX_LEVELS];
  int n;
};

constexpr int kLitLenSyms = 288, kDistSyms = 32, kCodeLenSyms = 19;  // table sizes; a dynamic block has at most 286 and 30
enum { kCodes = 0, kLens = 1, kDists = 2 };

__device__ const uint16_t kLenBase[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                          31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__device__ const uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__device__ const uint16_t kDistBase[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                           193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__device__ const uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__device__ const uint8_t kCodeLenOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ uint32_t dfl_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// The bits of the stream [p, p + len), LSB first.  All members but `chunk` hold the same value in every lane.
struct DeflateBits {
  const uint8_t* p;
  long long len, used, next_dword, chunk_base;  // bits taken; the next dword to feed; the first of the 64 dwords in `chunk`
  unsigned long long acc;                       // the low `nb` bits are the next bits of the stream
  uint32_t nb, chunk;

  // little-endian dword `d` of the stream: bytes behind the end read as 0 and are not fetched
  __device__ __forceinline__ uint32_t fetch(long long d) const {
    const long long b = 4 * d;
    uint32_t w = 0;
    if (b + 4 <= len) {
      __builtin_memcpy(&w, p + b, 4);
      return w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (b + k < len) w |= (uint32_t)p[b + k] << (8 * k);
    return w;
  }
  __device__ __forceinline__ uint32_t next(int lane) {
    const long long base = next_dword & ~63ll;
    if (base != chunk_base) {
      chunk = fetch(base + lane);
      chunk_base = base;
    }
    const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)chunk, (int)dfl_uniform((uint32_t)next_dword & 63u));
    ++next_dword;
    return w;
  }
  __device__ __forceinline__ void seek(long long byte, int lane) {  // byte <= len
    next_dword = byte >> 2;
    const uint32_t sh = 8u * (uint32_t)(byte & 3);
    acc = next(lane) >> sh;
    nb = 32 - sh;
    used = 8 * byte;
  }
  __device__ __forceinline__ void refill(int lane) {  // at least 32 bits afterwards
    if (nb <= 32) {
      acc |= (unsigned long long)next(lane) << nb;
      nb += 32;
    }
  }
  __device__ __forceinline__ bool have(uint32_t k) const { return used + (long long)k <= 8 * len; }
  __device__ __forceinline__ uint32_t peek(uint32_t k) const { return (uint32_t)acc & ((1u << k) - 1u); }  // k <= 16
  __device__ __forceinline__ void drop(uint32_t k) { acc >>= k, nb -= k, used += k; }
};

// What lane L keeps of a canonical code: the codes of length L are first .. first + count - 1, their symbols start at `offset`.
struct DeflateCode {
  uint32_t first, count, offset;
};

// `n` code lengths (LDS, each 0 .. 15) -> the code, its symbols sorted into `syms` (LDS, room for n).  False for the sets zlib
// rejects: over-subscribed, or incomplete other than a single one-bit literal/length or distance code or an empty distance set.
__device__ __forceinline__ bool deflate_build(const uint8_t* lens, uint32_t n, uint16_t* syms, uint32_t* cnt, int kind, int lane,
                                              DeflateCode& h) {
  __syncthreads();  // `lens` was written by other lanes, `syms` and `cnt` may still be read
  const bool mine = lane >= 1 && lane < 16;
  uint32_t c = 0;
  if (mine)
    for (uint32_t i = 0; i < n; ++i) c += lens[i] == (uint32_t)lane;
  if (lane < 16) cnt[lane] = c;
  __syncthreads();
  int left = 1;
  uint32_t first = 0, off = 0, longest = 0;
  h = DeflateCode{0, 0, 0};
  for (uint32_t l = 1; l < 16; ++l) {
    const uint32_t k = cnt[l];                   // <= n <= 288
    left = left < 0 ? -1 : 2 * left - (int)k;    // over-subscribed once negative
    if (l == (uint32_t)lane) h = DeflateCode{first, k, off};
    first = (first + k) << 1;
    off += k;
    if (k) longest = l;
  }
  if (mine) {
    uint32_t at = h.offset;  // offset + count <= n: the counts of all lengths sum to at most n
    for (uint32_t i = 0; i < n; ++i)
      if (lens[i] == (uint32_t)lane && at < n) syms[at++] = (uint16_t)i;
  }
  __syncthreads();
  if (left < 0) return false;
  return !(left > 0 && (kind == kCodes || longest > 1 || (longest == 0 && kind != kDists)));
}

// The symbol whose code starts the 15 bits `ahead` (LSB = the next bit of the stream), its length in `l`; -1 for a bit pattern
// no code owns.  `n`: the entries of `syms`.
__device__ __forceinline__ int deflate_symbol(const DeflateCode& h, const uint16_t* syms, uint32_t n, uint32_t ahead, int lane, uint32_t& l) {
  const bool mine = lane >= 1 && lane < 16;
  const uint32_t code = mine ? __builtin_bitreverse32(ahead) >> (32 - lane) : 0u;  // the first `lane` bits, MSB first
  const bool hit = mine && code - h.first < h.count && code >= h.first;
  const unsigned long long m = __ballot(hit);
  if (m == 0) return -1;
  l = (uint32_t)__ffsll((long long)m) - 1u;  // 1 .. 15: the shortest length that hits is the code (3.2.2)
  const uint32_t at = (uint32_t)__builtin_amdgcn_readlane((int)(h.offset + code - h.first), (int)dfl_uniform(l));
  if (at >= n) return -1;
  return (int)dfl_uniform(syms[at]);
}

__device__ __forceinline__ void deflate_wait_for_stores() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): a one-wave workgroup's fence is no wait by itself
}

__global__ __launch_bounds__(64) void deflate_decode_kernel(const uint8_t* __restrict__ file, long long file_bytes, DeflateLevels lv,
                                                            const long long* __restrict__ tile_off, const long long* __restrict__ tile_len,
                                                            const int* __restrict__ tile_xyl, uint8_t* scratch, long long stride,
                                                            uint8_t* __restrict__ status) {
  __shared__ uint8_t lens[kLitLenSyms + kDistSyms];  // a block's code lengths: literal/length, then distance
  __shared__ uint8_t cl_lens[kCodeLenSyms];
  __shared__ uint16_t ll_syms[kLitLenSyms], d_syms[kDistSyms], cl_syms[kCodeLenSyms];
  __shared__ uint32_t cnt[16];
  const int t = blockIdx.x, lane = threadIdx.x;
  const long long off = tile_off[t], len = tile_len[t];
  const int x = tile_xyl[3 * t], y = tile_xyl[3 * t + 1], li = tile_xyl[3 * t + 2];
  int st = HIPAC_DEFLATE_OK;
  if (len == 0) st = HIPAC_DEFLATE_MISSING;
  if (len < 0 || off < 0 || off > file_bytes || len > file_bytes - off || li < 0 || li >= lv.n) st = HIPAC_DEFLATE_BAD_TILE;
  uint32_t n_out = 0;
  if (st == HIPAC_DEFLATE_OK) {
    const hipac_deflate_level& L = lv.l[li];
    if (x < 0 || y < 0 || x >= L.W || y >= L.H || x % L.tile_w || y % L.tile_h) st = HIPAC_DEFLATE_BAD_TILE;
    n_out = (uint32_t)L.tile_w * (uint32_t)L.tile_h * (uint32_t)L.samples;  // <= stride: checked on the host
  }
  if (st != HIPAC_DEFLATE_OK) {
    if (lane == 0) status[t] = (uint8_t)st;
    return;
  }
  const uint8_t* src = file + off;
  uint8_t* out = scratch + (long long)t * stride;

  bool bad = len < 2;
  if (!bad) {
    const uint32_t cmf = src[0], flg = src[1];
    bad = (cmf * 256 + flg) % 31 != 0 || (cmf & 15) != 8 || (cmf >> 4) > 7 || (flg & 32);
  }
  DeflateBits br{src, len, 0, 0, -1, 0, 0, 0};
  if (!bad) br.seek(2, lane);
  uint32_t opos = 0, fenced = 0, final_block = 0;
  DeflateCode hl{0, 0, 0}, hd{0, 0, 0}, hc{0, 0, 0};
  while (!bad && !final_block) {
    br.refill(lane);
    if (!br.have(3)) {
      bad = true;
      break;
    }
    final_block = br.peek(1);
    const uint32_t type = br.peek(3) >> 1;
    br.drop(3);
    if (type == 3) {
      bad = true;
      break;
    }
    if (type == 0) {  // stored: to the byte boundary, LEN, ~LEN, LEN bytes
      br.drop((uint32_t)(-br.used) & 7u);
      br.refill(lane);
      if (!br.have(32)) {
        bad = true;
        break;
      }
      const uint32_t n = br.peek(16), inv = (uint32_t)(br.acc >> 16) & 0xFFFFu;
      br.drop(32);
      const long long at = br.used >> 3;
      if (n != (inv ^ 0xFFFFu) || at + n > len || n > n_out - opos) {
        bad = true;
        break;
      }
      for (uint32_t i = lane; i < n; i += 64) out[opos + i] = src[at + i];
      opos += n;
      br.seek(at + n, lane);
      continue;
    }
    uint32_t n_ll = kLitLenSyms, n_d = kDistSyms;
    if (type == 1) {
      for (uint32_t i = lane; i < (uint32_t)(kLitLenSyms + kDistSyms); i += 64)
        lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
    } else {
      if (!br.have(14)) {
        bad = true;
        break;
      }
      n_ll = br.peek(5) + 257, n_d = (br.peek(10) >> 5) + 1;
      const uint32_t n_cl = (br.peek(14) >> 10) + 4;  // <= 19
      br.drop(14);
      if (n_ll > 286 || n_d > 30) {
        bad = true;
        break;
      }
      __syncthreads();
      if (lane < kCodeLenSyms) cl_lens[lane] = 0;
      __syncthreads();
      for (uint32_t i = 0; i < n_cl && !bad; ++i) {
        br.refill(lane);
        if (!br.have(3)) bad = true;
        else if (lane == 0) cl_lens[kCodeLenOrder[i]] = (uint8_t)br.peek(3);
        br.drop(3);
      }
      if (bad || !deflate_build(cl_lens, kCodeLenSyms, cl_syms, cnt, kCodes, lane, hc)) {
        bad = true;
        break;
      }
      const uint32_t total = n_ll + n_d;  // <= 316
      uint32_t got = 0, prev = 0;
      while (got < total) {
        br.refill(lane);
        uint32_t l = 0;
        const int sym = deflate_symbol(hc, cl_syms, kCodeLenSyms, br.peek(15), lane, l);
        if (sym < 0 || sym > 18 || !br.have(l)) {
          bad = true;
          break;
        }
        br.drop(l);  // <= 7 of at least 32 bits: the extra bits are there
        uint32_t value = 0, rep = 1;
        if (sym < 16) {
          value = (uint32_t)sym;
        } else {
          const uint32_t eb = sym == 16 ? 2 : sym == 17 ? 3 : 7;
          if (!br.have(eb) || (sym == 16 && got == 0)) {
            bad = true;
            break;
          }
          rep = (sym == 18 ? 11 : 3) + br.peek(eb);
          br.drop(eb);
          value = sym == 16 ? prev : 0;
        }
        if (rep > total - got) {
          bad = true;
          break;
        }
        for (uint32_t i = lane; i < rep; i += 64) lens[got + i] = (uint8_t)value;  // got + rep <= total <= 316
        got += rep, prev = value;
      }
      if (bad) break;
      __syncthreads();
      if (lens[256] == 0) {  // no end-of-block code
        bad = true;
        break;
      }
    }
    if (!deflate_build(lens, n_ll, ll_syms, cnt, kLens, lane, hl) || !deflate_build(lens + n_ll, n_d, d_syms, cnt, kDists, lane, hd)) {
      bad = true;
      break;
    }
    for (;;) {
      br.refill(lane);
      uint32_t l = 0;
      int sym = deflate_symbol(hl, ll_syms, n_ll, br.peek(15), lane, l);
      if (sym < 0 || !br.have(l)) {
        bad = true;
        break;
      }
      br.drop(l);
      if (sym < 256) {
        if (opos >= n_out) {
          bad = true;
          break;
        }
        if (lane == 0) out[opos] = (uint8_t)sym;
        ++opos;
        continue;
      }
      if (sym == 256) break;
      sym -= 257;
      if (sym >= 29) {  // length symbols 286 and 287
        bad = true;
        break;
      }
      uint32_t eb = kLenExtra[sym];  // <= 5 of the at least 17 bits left
      if (!br.have(eb)) {
        bad = true;
        break;
      }
      const uint32_t n = kLenBase[sym] + br.peek(eb);
      br.drop(eb);
      br.refill(lane);
      const int ds = deflate_symbol(hd, d_syms, n_d, br.peek(15), lane, l);
      if (ds < 0 || ds >= 30 || !br.have(l)) {  // distance symbols 30 and 31
        bad = true;
        break;
      }
      br.drop(l);
      eb = kDistExtra[ds];  // <= 13 of the at least 17 bits left
      if (!br.have(eb)) {
        bad = true;
        break;
      }
      const uint32_t d = kDistBase[ds] + br.peek(eb);  // 1 .. 32768
      br.drop(eb);
      if (d > opos || n > n_out - opos) {
        bad = true;
        break;
      }
      const uint32_t from = opos - d;
      if (from + min(n, d) > fenced) {
        deflate_wait_for_stores();
        fenced = opos;
      }
      for (uint32_t i = lane; i < n; i += 64) out[opos + i] = out[from + (d >= n ? i : i % d)];  // from + i % d < opos
      opos += n;
    }
  }
  if (!bad) {  // to the byte boundary, then the Adler-32 of the n_out bytes, big-endian
    br.drop((uint32_t)(-br.used) & 7u);
    br.refill(lane);
    bad = !br.have(32) || opos != n_out;
  }
  if (!bad) {
    const uint32_t want = __builtin_bswap32((uint32_t)br.acc);
    deflate_wait_for_stores();
    unsigned long long s1 = 0, s2 = 0;  // sum of b[i] and of (n_out - i) b[i]: below 2^48 for 2^20 bytes
    for (uint32_t i = 4 * lane; i < n_out; i += 256) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(out + i);  // the scratch of a tile is a multiple of 256 bytes
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k)
        if (i + k < n_out) {
          const uint32_t b = (w >> (8 * k)) & 255u;
          s1 += b, s2 += (unsigned long long)(n_out - i - k) * b;
        }
    }
    s1 = wave_sum(s1), s2 = wave_sum(s2);
    const uint32_t a = (uint32_t)((s1 + 1) % 65521u), b = (uint32_t)((s2 + n_out) % 65521u);
    bad = want != (b << 16 | a);
  }
  if (lane == 0) status[t] = bad ? HIPAC_DEFLATE_REFUSED : HIPAC_DEFLATE_OK;
}

static_assert(HIPAC_DEFLATE_OK == 0 && HIPAC_DEFLATE_REFUSED == 1, "tile_place.h takes these two values");

__global__ __launch_bounds__(256) void deflate_place_kernel(DeflateLevels lv, const int* __restrict__ tile_xyl,
                                                            const uint8_t* __restrict__ status, const uint8_t* __restrict__ scratch,
                                                            long long stride) {
  tile_place(lv, tile_xyl, status, scratch, stride);
}

static size_t deflate_tile_stride(int tile_w, int tile_h, int samples) { return align256((size_t)tile_w * tile_h * samples); }

static bool deflate_tile_ok(int tile_w, int tile_h, int samples) {
  return tile_w >= 1 && tile_h >= 1 && (samples == 1 || samples == 3 || samples == 4) &&
         (long long)tile_w * tile_h * samples <= HIPAC_DEFLATE_MAX_TILE_BYTES;
}

}  // namespace hipac

using namespace hipac;

extern "C" int hipac_deflate_abi_version(void) { return HIPAC_DEFLATE_ABI_VERSION; }

extern "C" size_t hipac_deflate_workspace_bytes(int tile_w, int tile_h, int samples, int n_tiles) {
  if (!deflate_tile_ok(tile_w, tile_h, samples) || n_tiles < 1 || n_tiles > HIPAC_DEFLATE_MAX_TILES) return 0;
  return (size_t)n_tiles * deflate_tile_stride(tile_w, tile_h, samples);
}

extern "C" int hipac_deflate_decode_tiles(const uint8_t* file_dev, int64_t file_bytes, const hipac_deflate_level* levels, int n_levels,
                                          const int64_t* tile_off, const int64_t* tile_len, const int32_t* tile_xyl, int n_tiles,
                                          void* workspace, size_t workspace_bytes, uint8_t* status_dev, void* stream) {
  HIPAC_REQUIRE(file_dev && levels && tile_off && tile_len && tile_xyl && workspace && status_dev, HIPAC_EINVAL,
                "deflate_decode_tiles: null argument");
  HIPAC_REQUIRE(file_bytes >= 0, HIPAC_EINVAL, "deflate_decode_tiles: file_bytes %lld", (long long)file_bytes);
  HIPAC_REQUIRE(n_tiles >= 1 && n_tiles <= HIPAC_DEFLATE_MAX_TILES, HIPAC_EINVAL, "deflate_decode_tiles: n_tiles %d outside 1..%d",
                n_tiles, HIPAC_DEFLATE_MAX_TILES);
  HIPAC_REQUIRE(n_levels >= 1 && n_levels <= HIPAC_DEFLATE_MAX_LEVELS, HIPAC_EINVAL, "deflate_decode_tiles: n_levels %d outside 1..%d",
                n_levels, HIPAC_DEFLATE_MAX_LEVELS);
  DeflateLevels lv;
  std::memset(&lv, 0, sizeof(lv));
  lv.n = n_levels;
  size_t stride = 0;
  int max_th = 0;
  for (int l = 0; l < n_levels; ++l) {
    const hipac_deflate_level& L = levels[l];
    HIPAC_REQUIRE(L.pixels && L.W >= 1 && L.H >= 1 && L.pitch_bytes >= (int64_t)L.W * 3, HIPAC_EINVAL,
                  "deflate_decode_tiles: bad geometry of level %d", l);
    HIPAC_REQUIRE(deflate_tile_ok(L.tile_w, L.tile_h, L.samples), HIPAC_EINVAL,
                  "deflate_decode_tiles: level %d: tile %d x %d x %d samples (need samples 1, 3 or 4 and at most %d bytes)", l, L.tile_w,
                  L.tile_h, L.samples, HIPAC_DEFLATE_MAX_TILE_BYTES);
    HIPAC_REQUIRE(L.predictor == 1 || L.predictor == 2, HIPAC_EINVAL, "deflate_decode_tiles: level %d: predictor %d (need 1 or 2)", l,
                  L.predictor);
    lv.l[l] = L;
    const size_t s = deflate_tile_stride(L.tile_w, L.tile_h, L.samples);
    stride = s > stride ? s : stride;
    max_th = L.tile_h > max_th ? L.tile_h : max_th;
  }
  HIPAC_REQUIRE(((uintptr_t)workspace & 255) == 0, HIPAC_EINVAL, "deflate_decode_tiles: workspace not 256-byte aligned");
  HIPAC_REQUIRE(workspace_bytes >= (size_t)n_tiles * stride, HIPAC_EWORKSPACE,
                "deflate_decode_tiles: workspace %zu bytes, %zu needed (hipac_deflate_workspace_bytes of the largest tile)",
                workspace_bytes, (size_t)n_tiles * stride);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(deflate_decode_kernel, dim3((unsigned)n_tiles), dim3(64), 0, s, file_dev, (long long)file_bytes, lv,
                     (const long long*)tile_off, (const long long*)tile_len, (const int*)tile_xyl, (uint8_t*)workspace,
                     (long long)stride, status_dev);
  hipLaunchKernelGGL(deflate_place_kernel, dim3((unsigned)((max_th + 15) / 16), (unsigned)n_tiles), dim3(256), 0, s, lv,
                     (const int*)tile_xyl, (const uint8_t*)status_dev, (const uint8_t*)workspace, (long long)stride);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

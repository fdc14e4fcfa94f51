// PNG patch files encoded on the device (include/hipac_png.h states the format; tests/png_encode_cpu.py restates it byte for byte).
//
//   png_band_kernel     one band (whole filtered rows, at most HIPAC_PNG_BAND_BYTES) = one workgroup of 256; the bands of all
//               windows of a call share one grid.  Everything a band needs lives in LDS (54 KiB: the filtered bytes, the output
//               bytes, the code tables):
//                 1. filter    a wave per row: five cost sums per lane, one shuffle reduction, the chosen row into LDS;
//                 2. runs      thread t owns the bytes [t C, (t + 1) C) of the band; where the run covering its first byte began
//                              and where the run covering its last byte ends come from two scans over the 256 chunks, so every
//                              thread derives its own tokens (literal / distance-1 match) without a token array;
//                 3. counts    integer LDS atomics into the literal/length histogram;
//                 4. codes     rank sort by (count, symbol) across the threads, the two-queue merge on one thread (285 steps),
//                              leaf depths across the threads; counts halved and rebuilt while a code is too long; the same
//                              for the code-length code; the three exact bit counts pick the block type;
//                 5. emit      a scan of the chunks' bit lengths, then every token OR-ed into zeroed LDS dwords;
//                 6. sums      the Adler-32 partial of the band, and the chunk's CRC-32 from 256 slices combined pairwise with
//                              the x^n mod P operator (zlib's crc32_combine).
//               The band's bytes and (size, CRC, Adler partial) go to its workspace slot with dword stores.
//   png_gather_kernel   one window = one workgroup: thread 0 lays the chunks out (a running sum over at most 448 bands) and
//               combines the Adler partials, then all threads copy the bands behind their chunk headers and thread 0 writes the
//               signature, IHDR, the Adler chunk, IEND and the file's size.
//
// Remainder rule of a run (header comment): m = n - 1 bytes behind the first literal, m / 258 full matches, then one match of
// r = m % 258 when r >= 3, else r literals.
//
// Integer arithmetic only; plain C++ and vector stores.  Safety: every source pixel is tested against W and H before its
// address is formed; every LDS table index is clamped or tested against its table; a band's bytes are bounded by its slot
// (kOutBytes and the slot stride, both checked before the copy); the gather tests the file's total against out_stride before it
// writes a byte.  Every loop runs to a bound fixed before it starts.
#include "common.h"

#include "../../include/hipac_png.h"
#include "wave_reduce.h"

namespace hipac {

constexpr int kPngThreads = 256;
constexpr int kBand = HIPAC_PNG_BAND_BYTES;
constexpr int kOutBytes = kBand + 16;  // zlib header 2 + stored header 5 + empty stored block 5, rounded up to dwords
constexpr int kOutDwords = kOutBytes / 4;
constexpr int kMaxBands = 512;  // per window: 448 at P = 1792
constexpr int kSyms = 288;      // literal/length table size (286 used by dynamic blocks, 288 by the fixed code)
constexpr int kClTokens = 320;  // run-length tokens of at most 287 code lengths
constexpr uint32_t kCrcPoly = 0xEDB88320u;
static_assert(kBand <= 65535 && kBand % 4 == 0, "a stored band is one stored block");
static_assert((HIPAC_PNG_MAX_P + (kBand / (1 + 3 * HIPAC_PNG_MAX_P)) - 1) / (kBand / (1 + 3 * HIPAC_PNG_MAX_P)) <= kMaxBands, "bands per window");
static_assert(1 + 3 * HIPAC_PNG_MAX_P <= kBand, "a band holds at least one row");

constexpr uint32_t crc_mult_c(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int k = 0; k < 32; ++k) {
    if (a & (1u << (31 - k))) p ^= b;
    b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
struct CrcTables {
  uint32_t byte[256];
  uint32_t x2n[32];  // x^(2^n) mod P
  constexpr CrcTables() : byte(), x2n() {
    for (uint32_t n = 0; n < 256; ++n) {
      uint32_t c = n;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
      byte[n] = c;
    }
    uint32_t p = 1u << 30;
    x2n[0] = p;
    for (int n = 1; n < 32; ++n) x2n[n] = p = crc_mult_c(p, p);
  }
};
__device__ const CrcTables kCrc{};
constexpr uint32_t kCrcIdat = 0x35AF061Eu;  // CRC-32 of "IDAT"

__device__ const uint16_t kPngLenBase[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                             31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__device__ const uint8_t kPngLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__device__ const uint8_t kPngClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ uint32_t crc_mult(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll 4
  for (int k = 0; k < 32; ++k) {
    if (a & (1u << (31 - k))) p ^= b;
    b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
// crc32_combine: the CRC of A B from the CRCs of A and B and the length of B
__device__ uint32_t crc_combine(uint32_t crc1, uint32_t crc2, uint32_t len2) {
  uint32_t p = 1u << 31;
  for (int k = 0; k < 29; ++k)  // x^(8 len2): bit k of len2 is x^(2^(k + 3)); len2 < 2^29
    if (len2 >> k & 1) p = crc_mult(kCrc.x2n[(k + 3) & 31], p);
  return crc_mult(p, crc1) ^ crc2;
}

// length 3 .. 258 -> length code 0 .. 28 (the largest whose base is not above it)
__device__ __forceinline__ int png_len_code(int len) {
  int c = 0;
#pragma unroll
  for (int k = 1; k < 29; ++k) c += (int)kPngLenBase[k] <= len;
  return c;
}

struct PngBandMeta {
  uint32_t nbytes, crc, adler_a, adler_b;
};

struct PngLds {
  uint32_t f[kBand / 4];       // the filtered band, as bytes
  uint32_t out[kOutDwords];    // the band's output bytes, zeroed, OR-ed into
  uint32_t cnt[kSyms];         // literal/length counts
  uint32_t work[kSyms];        // the counts the tree is built from (halved by the limiter)
  uint32_t w[kSyms];           // weights of the internal nodes, in the order they were made
  uint16_t sorted[kSyms];      // used symbols by (count, symbol)
  uint16_t lpar[kSyms], npar[kSyms], depth[kSyms];  // parent of a sorted leaf / of an internal node; depth of an internal node
  uint16_t code[kSyms];        // bit-reversed canonical codes
  uint16_t clt[kClTokens];     // code-length tokens: symbol | extra << 5
  uint8_t len[kSyms];          // literal/length code lengths
  uint8_t fixlen[kSyms];
  uint32_t clcnt[19];
  uint16_t clcode[19];
  uint8_t cllen[19];
  uint32_t nextcode[16];
  int scan_a[kPngThreads], scan_b[kPngThreads];
  uint32_t crc[kPngThreads], crclen[kPngThreads];
  uint32_t n_used, maxlen, extra_total, n_match, adler_a, adler_b;
  int hlit, hclen, n_clt, kind, hdr_bits, nbytes;
};

// Code lengths of `cnt[0 .. nsym)` into `len`, at most `limit` bits (see the header for the construction).  All threads call.
__device__ void png_huffman(PngLds& s, const uint32_t* cnt, int nsym, uint32_t limit, uint8_t* len) {
  const int tid = threadIdx.x;
  for (int i = tid; i < nsym; i += kPngThreads) s.work[i] = cnt[i];
  for (int round = 0; round < 20; ++round) {  // counts are below 2^17: after 17 halvings every count is 1 and the tree is balanced
    if (tid == 0) s.n_used = 0, s.maxlen = 0;
    __syncthreads();
    for (int i = tid; i < nsym; i += kPngThreads) {
      const uint32_t c = s.work[i];
      len[i] = 0;
      if (c) {
        int rank = 0;
        for (int j = 0; j < nsym; ++j) {
          const uint32_t cj = s.work[j];
          rank += (cj != 0) & ((cj < c) | ((cj == c) & (j < i)));
        }
        s.sorted[rank] = (uint16_t)i;  // rank < number of used symbols <= nsym
        atomicAdd(&s.n_used, 1u);
      }
    }
    __syncthreads();
    const int n = (int)s.n_used;
    if (tid == 0 && n >= 2) {
      int i = 0, j = 0;
      for (int m = 0; m < n - 1; ++m) {
        uint32_t total = 0;
        for (int rep = 0; rep < 2; ++rep) {
          const bool leaf = i < n && (j >= m || s.work[s.sorted[i]] <= s.w[j]);
          if (leaf) {
            total += s.work[s.sorted[i]];
            s.lpar[i++] = (uint16_t)m;
          } else {
            total += s.w[j];
            s.npar[j++] = (uint16_t)m;
          }
        }
        s.w[m] = total;
      }
      s.depth[n - 2] = 0;
      for (int k = n - 3; k >= 0; --k) s.depth[k] = (uint16_t)(s.depth[min((int)s.npar[k], n - 2)] + 1);
    }
    __syncthreads();
    if (n >= 2) {
      for (int k = tid; k < n; k += kPngThreads) {
        const uint32_t l = (uint32_t)s.depth[min((int)s.lpar[k], n - 2)] + 1;
        len[min((int)s.sorted[k], nsym - 1)] = (uint8_t)min(l, 255u);
        atomicMax(&s.maxlen, l);
      }
    } else if (n == 1 && tid == 0) {
      len[min((int)s.sorted[0], nsym - 1)] = 1;
    }
    __syncthreads();
    const bool done = s.maxlen <= limit;
    if (!done)
      for (int i = tid; i < nsym; i += kPngThreads) s.work[i] = (s.work[i] + 1) >> 1;
    __syncthreads();
    if (done) break;
  }
}

// Bit-reversed canonical codes of `len[0 .. nsym)` (lengths at most 15).  All threads call.
__device__ void png_codes(PngLds& s, const uint8_t* len, int nsym, uint16_t* code) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    uint32_t bl[16];
    for (int b = 0; b < 16; ++b) bl[b] = 0;
    for (int i = 0; i < nsym; ++i) bl[len[i] & 15] += 1;
    bl[0] = 0;
    uint32_t c = 0;
    s.nextcode[0] = 0;
    for (int b = 1; b < 16; ++b) s.nextcode[b] = c = (c + bl[b - 1]) << 1;
  }
  __syncthreads();
  for (int i = tid; i < nsym; i += kPngThreads) {
    const uint32_t l = len[i] & 15;
    uint32_t before = 0;
    for (int j = 0; j < i; ++j) before += (uint32_t)(len[j] & 15) == l;
    code[i] = l ? (uint16_t)(__brev(s.nextcode[l] + before) >> (32 - l)) : (uint16_t)0;
  }
  __syncthreads();
}

__device__ __forceinline__ void png_put(uint32_t* out, uint32_t bit, uint32_t value, uint32_t nbits) {
  if (nbits == 0) return;
  const uint32_t d = bit >> 5, sh = bit & 31;
  if (d < (uint32_t)kOutDwords) atomicOr(&out[d], value << sh);
  if (sh + nbits > 32 && d + 1 < (uint32_t)kOutDwords) atomicOr(&out[d + 1], value >> (32 - sh));
}

// The tokens of the bytes [lo, hi) of the band f[0 .. L): f(kind, value) with kind 0 = literal `value`, 1 = match of length
// `value`.  `start_in`: where the run covering byte lo began (used when lo does not begin a run); `next_start`: the first run
// start at or behind hi (L if none).
template <class F>
__device__ __forceinline__ void png_walk(const uint8_t* f, int lo, int hi, int start_in, int next_start, F&& emit) {
  int s = start_in, e = lo;  // the run [s, e) covering the byte before i
  for (int i = lo; i < hi; ++i) {
    if (i >= e) {
      if (i == 0 || f[i] != f[i - 1]) s = i;
      int q = i + 1;
      for (; q < hi; ++q)
        if (f[q] != f[i]) break;
      e = q < hi ? q : next_start;
    }
    const int n = e - s, k = i - s, v = f[i];
    if (n < 4 || k == 0) {
      emit(0, v);
      continue;
    }
    const int m = n - 1, j = k - 1, full = m / 258 * 258, r = m - full;
    if (j < full) {
      if (j % 258 == 0) emit(1, 258);
    } else if (r >= 3) {
      if (j == full) emit(1, r);
    } else {
      emit(0, v);
    }
  }
}

__device__ __forceinline__ uint32_t png_pixel(const uint8_t* __restrict__ level, int W, int H, long long pitch, long long X,
                                              long long Y, int ch) {
  if (X < 0 || X >= W || Y < 0 || Y >= H) return 255u;
  return level[Y * pitch + X * 3 + ch];
}

__device__ __forceinline__ uint32_t png_cost(uint32_t v) { return v < 256u - v ? v : 256u - v; }

// the five filtered values of byte i of window row r
__device__ __forceinline__ void png_filter5(const uint8_t* __restrict__ level, int W, int H, long long pitch, long long x0,
                                            long long y0, int r, int i, uint32_t out[5]) {
  const int col = i / 3, ch = i - 3 * col;
  const uint32_t x = png_pixel(level, W, H, pitch, x0 + col, y0 + r, ch);
  const uint32_t a = col > 0 ? png_pixel(level, W, H, pitch, x0 + col - 1, y0 + r, ch) : 0u;
  const uint32_t b = r > 0 ? png_pixel(level, W, H, pitch, x0 + col, y0 + r - 1, ch) : 0u;
  const uint32_t c = (r > 0 && col > 0) ? png_pixel(level, W, H, pitch, x0 + col - 1, y0 + r - 1, ch) : 0u;
  const int p = (int)a + (int)b - (int)c;
  const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
  const uint32_t paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  out[0] = x;
  out[1] = (x - a) & 255u;
  out[2] = (x - b) & 255u;
  out[3] = (x - ((a + b) >> 1)) & 255u;
  out[4] = (x - paeth) & 255u;
}

__global__ __launch_bounds__(kPngThreads) void png_band_kernel(const uint8_t* __restrict__ level, int W, int H, long long pitch,
                                                               const int* __restrict__ xy, int n_windows, int P, int band_rows,
                                                               int n_bands, uint8_t* __restrict__ slots, long long slot_stride,
                                                               PngBandMeta* __restrict__ meta) {
  __shared__ PngLds s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long gband = blockIdx.x;
  const int win = (int)(gband / n_bands), band = (int)(gband - (long long)win * n_bands);
  if (win >= n_windows) return;
  const long long x0 = xy[2 * win], y0 = xy[2 * win + 1];
  const int row_bytes = 1 + 3 * P, r0 = band * band_rows, r1 = min(P, r0 + band_rows);
  const int L = (r1 - r0) * row_bytes;
  if (r0 >= r1 || L > kBand) return;  // never: the host derives band_rows and n_bands from P
  const bool first = band == 0, last = band == n_bands - 1;
  uint8_t* const f = reinterpret_cast<uint8_t*>(s.f);
  uint8_t* const outb = reinterpret_cast<uint8_t*>(s.out);

  // ---- 0. clear
  for (int i = tid; i < kOutDwords; i += kPngThreads) s.out[i] = 0;
  for (int i = tid; i < kSyms; i += kPngThreads) {
    s.cnt[i] = 0;
    s.fixlen[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
  }
  if (tid < 19) s.clcnt[tid] = 0;
  if (tid == 0) s.extra_total = s.n_match = s.adler_a = s.adler_b = 0;

  // ---- 1. filter: a wave per row
  for (int r = r0 + wave; r < r1; r += kPngThreads / 64) {
    uint32_t cost[5] = {0, 0, 0, 0, 0};
    for (int i = lane; i < 3 * P; i += 64) {
      uint32_t v[5];
      png_filter5(level, W, H, pitch, x0, y0, r, i, v);
#pragma unroll
      for (int t = 0; t < 5; ++t) cost[t] += png_cost(v[t]);
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) cost[t] = wave_sum(cost[t]);
    int best = 0;
#pragma unroll
    for (int t = 1; t < 5; ++t)
      if (cost[t] < cost[best]) best = t;  // ties: the lowest type
    uint8_t* const row = f + (r - r0) * row_bytes;
    if (lane == 0) row[0] = (uint8_t)best;
    for (int i = lane; i < 3 * P; i += 64) {
      uint32_t v[5];
      png_filter5(level, W, H, pitch, x0, y0, r, i, v);
      row[1 + i] = (uint8_t)v[best];
    }
  }
  __syncthreads();

  // ---- 2. runs: where the run covering a chunk's first byte began, where the first run behind the chunk begins
  const int C = (L + kPngThreads - 1) / kPngThreads;
  const int lo = min(L, tid * C), hi = min(L, lo + C);
  {
    int last_start = -1, first_start = L;
    for (int i = lo; i < hi; ++i)
      if (i == 0 || f[i] != f[i - 1]) {
        last_start = i;
        first_start = min(first_start, i);
      }
    s.scan_a[tid] = last_start;
    s.scan_b[tid] = first_start;
  }
  __syncthreads();
  int start_in = 0, next_start = L;
  for (int t = 0; t < kPngThreads; ++t) {
    if (t < tid) start_in = max(start_in, s.scan_a[t]);
    if (t > tid) next_start = min(next_start, s.scan_b[t]);
  }
  __syncthreads();

  // ---- 3. counts, and the Adler partial on the way
  {
    uint32_t extra = 0, matches = 0;
    png_walk(f, lo, hi, start_in, next_start, [&](int kind, int v) {
      if (kind == 0) {
        atomicAdd(&s.cnt[v & 255], 1u);
      } else {
        const int c = png_len_code(v);
        atomicAdd(&s.cnt[257 + c], 1u);
        extra += kPngLenExtra[c];
        matches += 1;
      }
    });
    unsigned long long a = 0, b = 0;
    for (int i = lo; i < hi; ++i) {
      a += f[i];
      b += (unsigned long long)(L - i) * f[i];
    }
    if (extra) atomicAdd(&s.extra_total, extra);
    if (matches) atomicAdd(&s.n_match, matches);
    atomicAdd(&s.adler_a, (uint32_t)(a % 65521u));
    atomicAdd(&s.adler_b, (uint32_t)(b % 65521u));
    if (tid == 0) s.cnt[256] = 1;
  }
  __syncthreads();

  // ---- 4. codes and the three bit counts
  png_huffman(s, s.cnt, 286, 15, s.len);
  if (tid == 0) {
    int hlit = 257;
    for (int i = 257; i < 286; ++i)
      if (s.len[i]) hlit = i + 1;
    s.hlit = hlit;
    // run-length tokens of len[0 .. hlit) followed by the one distance length, 1
    int nt = 0, i = 0;
    const int total = hlit + 1;
    auto at = [&](int k) -> int { return k < hlit ? (int)s.len[k] : 1; };
    for (int guard = 0; guard < 288 && i < total; ++guard) {
      const int v = at(i);
      int e = i + 1;
      for (; e < total; ++e)
        if (at(e) != v) break;
      int run = e - i;
      bool sent = false;
      for (int g2 = 0; g2 < 288 && run > 0; ++g2) {
        int t, sym, ev;
        if (v == 0 && run >= 11) {
          t = min(run, 138), sym = 18, ev = t - 11;
        } else if (v == 0 && run >= 3) {
          t = run, sym = 17, ev = t - 3;
        } else if (v != 0 && sent && run >= 3) {
          t = min(run, 6), sym = 16, ev = t - 3;
        } else {
          t = 1, sym = v, ev = 0, sent = true;
        }
        if (nt < kClTokens) s.clt[nt++] = (uint16_t)(sym | ev << 5);
        s.clcnt[sym] += 1;  // sym <= 18
        run -= t;
      }
      i = e;
    }
    s.n_clt = nt;
  }
  __syncthreads();
  png_huffman(s, s.clcnt, 19, 7, s.cllen);
  png_codes(s, s.cllen, 19, s.clcode);
  if (tid == 0) {
    int hclen = 19;
    for (int k = 18; k >= 4; --k) {
      if (s.cllen[kPngClOrder[k]] != 0) break;
      hclen = k;
    }
    s.hclen = hclen;
    uint32_t lit_fixed = 0, lit_dyn = 0, cl_bits = 0;
    for (int i = 0; i < 286; ++i) {
      lit_fixed += s.cnt[i] * s.fixlen[i];
      lit_dyn += s.cnt[i] * s.len[i];
    }
    for (int k = 0; k < s.n_clt; ++k) {
      const int sym = s.clt[k] & 31;
      cl_bits += s.cllen[min(sym, 18)] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
    }
    const uint32_t stored_bits = 40u + 8u * (uint32_t)L;
    const uint32_t fixed_bits = 3 + lit_fixed + s.extra_total + 5 * s.n_match;
    const uint32_t dyn_hdr = 3 + 14 + 3 * (uint32_t)hclen + cl_bits;
    const uint32_t dyn_bits = dyn_hdr + lit_dyn + s.extra_total + s.n_match;
    int kind = 0;
    uint32_t best = stored_bits;
    if (fixed_bits < best) kind = 1, best = fixed_bits;
    if (dyn_bits < best) kind = 2, best = dyn_bits;
    s.kind = kind;
    s.hdr_bits = kind == 2 ? (int)dyn_hdr : 3;
  }
  __syncthreads();
  const int kind = s.kind;
  const uint32_t base_bits = first ? 16u : 0u;
  if (first && tid == 0) s.out[0] = 0x0178u;  // 78 01
  __syncthreads();

  // ---- 5. emit
  if (kind == 0) {
    const int at = (int)(base_bits >> 3);
    if (tid == 0) {
      outb[at] = last ? 1 : 0;
      outb[at + 1] = (uint8_t)(L & 255);
      outb[at + 2] = (uint8_t)(L >> 8);
      outb[at + 3] = (uint8_t)(~L & 255);
      outb[at + 4] = (uint8_t)((~L >> 8) & 255);
    }
    for (int i = tid; i < L; i += kPngThreads) outb[at + 5 + i] = f[i];  // at + 5 + L <= kBand + 7 < kOutBytes
    if (tid == 0) {
      int nb = at + 5 + L;
      if (!last) {
        outb[nb + 3] = 255;
        outb[nb + 4] = 255;
        nb += 5;
      }
      s.nbytes = nb;
    }
  } else {
    const uint8_t* const lens = kind == 2 ? s.len : s.fixlen;
    const uint32_t dist_bits = kind == 2 ? 1u : 5u;
    png_codes(s, lens, kind == 2 ? 286 : 288, s.code);
    uint32_t my_bits = 0;
    png_walk(f, lo, hi, start_in, next_start, [&](int k, int v) {
      if (k == 0) {
        my_bits += lens[v & 255];
      } else {
        const int c = png_len_code(v);
        my_bits += lens[257 + c] + kPngLenExtra[c] + dist_bits;
      }
    });
    s.scan_a[tid] = (int)my_bits;
    __syncthreads();
    uint32_t bit = base_bits + (uint32_t)s.hdr_bits, all_bits = 0;
    for (int t = 0; t < kPngThreads; ++t) {
      const uint32_t v = (uint32_t)s.scan_a[t];
      if (t < tid) bit += v;
      all_bits += v;
    }
    if (tid == 0) {
      uint32_t hb = base_bits;
      png_put(s.out, hb, (last ? 1u : 0u) | (uint32_t)kind << 1, 3);
      hb += 3;
      if (kind == 2) {
        png_put(s.out, hb, (uint32_t)(s.hlit - 257) | 0u << 5 | (uint32_t)(s.hclen - 4) << 10, 14);
        hb += 14;
        for (int k = 0; k < s.hclen; ++k, hb += 3) png_put(s.out, hb, s.cllen[kPngClOrder[k]], 3);
        for (int k = 0; k < s.n_clt; ++k) {
          const int sym = min(s.clt[k] & 31, 18), ev = s.clt[k] >> 5;
          const uint32_t l = s.cllen[sym], eb = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
          png_put(s.out, hb, (uint32_t)s.clcode[sym] | (uint32_t)ev << l, l + eb);
          hb += l + eb;
        }
      }
      // end of block behind the last token, then the byte alignment
      const uint32_t eob = base_bits + (uint32_t)s.hdr_bits + all_bits;
      png_put(s.out, eob, s.code[256], lens[256]);
      uint32_t end = eob + lens[256];
      if (!last) end += 3;
      int nb = (int)((end + 7) >> 3);
      if (!last) {
        png_put(s.out, (uint32_t)(nb + 2) * 8u, 0xFFFFu, 16);  // 00 00 FF FF; OR-ed like the tokens, whose dword it may share
        nb += 4;
      }
      s.nbytes = nb;
    }
    png_walk(f, lo, hi, start_in, next_start, [&](int k, int v) {
      if (k == 0) {
        const uint32_t l = lens[v & 255];
        png_put(s.out, bit, s.code[v & 255], l);
        bit += l;
      } else {
        const int c = png_len_code(v);
        const uint32_t l = lens[257 + c], eb = kPngLenExtra[c];
        png_put(s.out, bit, (uint32_t)s.code[257 + c] | (uint32_t)(v - kPngLenBase[c]) << l, l + eb + dist_bits);
        bit += l + eb + dist_bits;
      }
    });
  }
  __syncthreads();

  // ---- 6. CRC of "IDAT" + bytes, and the results
  const int nbytes = min(s.nbytes, kOutBytes);
  {
    const int S = (nbytes + kPngThreads - 1) / kPngThreads;
    const int c0 = min(nbytes, tid * S), c1 = min(nbytes, c0 + S);
    uint32_t c = 0xFFFFFFFFu;
    for (int i = c0; i < c1; ++i) c = kCrc.byte[(c ^ outb[i]) & 255] ^ (c >> 8);
    s.crc[tid] = c1 > c0 ? ~c : 0u;
    s.crclen[tid] = (uint32_t)(c1 - c0);
  }
  __syncthreads();
  for (int stride = 1; stride < kPngThreads; stride *= 2) {
    if (tid % (2 * stride) == 0) {
      s.crc[tid] = crc_combine(s.crc[tid], s.crc[tid + stride], s.crclen[tid + stride]);
      s.crclen[tid] += s.crclen[tid + stride];
    }
    __syncthreads();
  }
  uint8_t* const slot = slots + gband * slot_stride;
  if ((long long)nbytes <= slot_stride) {
    uint32_t* const dst = reinterpret_cast<uint32_t*>(slot);  // slots are 256-byte aligned, the stride a multiple of 256
    for (int i = tid; i < (nbytes + 3) / 4; i += kPngThreads) dst[i] = s.out[i];
  }
  if (tid == 0) {
    PngBandMeta m;
    m.nbytes = (long long)nbytes <= slot_stride ? (uint32_t)nbytes : 0u;
    m.crc = crc_combine(kCrcIdat, s.crc[0], (uint32_t)nbytes);
    m.adler_a = (1u + s.adler_a) % 65521u;
    m.adler_b = ((uint32_t)L + s.adler_b) % 65521u;
    meta[gband] = m;
  }
}

__device__ __forceinline__ void png_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}
__device__ uint32_t png_crc_bytes(const uint8_t* p, int n) {
  uint32_t c = 0xFFFFFFFFu;
  for (int i = 0; i < n; ++i) c = kCrc.byte[(c ^ p[i]) & 255] ^ (c >> 8);
  return ~c;
}

__global__ __launch_bounds__(kPngThreads) void png_gather_kernel(const uint8_t* __restrict__ slots, long long slot_stride,
                                                                 const PngBandMeta* __restrict__ meta, int n_windows, int P,
                                                                 int band_rows, int n_bands, uint8_t* __restrict__ out,
                                                                 long long out_stride, long long* __restrict__ sizes) {
  __shared__ long long s_off[kMaxBands];
  __shared__ uint32_t s_len[kMaxBands];
  __shared__ long long s_total;
  __shared__ uint32_t s_adler;
  const int tid = threadIdx.x, win = blockIdx.x;
  if (win >= n_windows || n_bands > kMaxBands) return;
  const PngBandMeta* const wm = meta + (long long)win * n_bands;
  if (tid == 0) {
    long long off = 8 + 25;
    uint32_t a = 1, b = 0;
    const uint32_t row_bytes = 1u + 3u * (uint32_t)P;
    for (int k = 0; k < n_bands; ++k) {
      const PngBandMeta m = wm[k];
      s_off[k] = off;
      s_len[k] = m.nbytes;
      off += 12 + (long long)m.nbytes;
      const uint32_t rows = (uint32_t)(min(P, (k + 1) * band_rows) - k * band_rows);
      const unsigned long long len2 = (unsigned long long)rows * row_bytes;
      const uint32_t a1 = a;
      a = (a1 + m.adler_a + 65520u) % 65521u;
      b = (uint32_t)((b + m.adler_b + len2 % 65521u * ((a1 + 65520u) % 65521u)) % 65521u);
    }
    s_adler = b << 16 | a;
    s_total = off + 16 + 12;
  }
  __syncthreads();
  const long long total = s_total;
  uint8_t* const file = out + (long long)win * out_stride;
  if (total > out_stride) {  // never: out_stride >= hipac_png_file_bound(P)
    if (tid == 0) sizes[win] = 0;
    return;
  }
  for (int k = 0; k < n_bands; ++k) {
    const uint8_t* const src = slots + ((long long)win * n_bands + k) * slot_stride;
    uint8_t* const dst = file + s_off[k] + 8;
    const int len = (int)min((long long)s_len[k], slot_stride);
    for (int i = tid; i < len; i += kPngThreads) dst[i] = src[i];
    if (tid == 0) {
      png_be32(file + s_off[k], (uint32_t)len);
      file[s_off[k] + 4] = 'I', file[s_off[k] + 5] = 'D', file[s_off[k] + 6] = 'A', file[s_off[k] + 7] = 'T';
      png_be32(dst + len, wm[k].crc);
    }
  }
  if (tid == 0) {
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    for (int i = 0; i < 8; ++i) file[i] = sig[i];
    uint8_t ih[17] = {'I', 'H', 'D', 'R', 0, 0, 0, 0, 0, 0, 0, 0, 8, 2, 0, 0, 0};
    png_be32(ih + 4, (uint32_t)P);
    png_be32(ih + 8, (uint32_t)P);
    png_be32(file + 8, 13);
    for (int i = 0; i < 17; ++i) file[12 + i] = ih[i];
    png_be32(file + 29, png_crc_bytes(ih, 17));
    uint8_t* t = file + total - 28;
    uint8_t ad[8] = {'I', 'D', 'A', 'T', 0, 0, 0, 0};
    png_be32(ad + 4, s_adler);
    png_be32(t, 4);
    for (int i = 0; i < 8; ++i) t[4 + i] = ad[i];
    png_be32(t + 12, png_crc_bytes(ad, 8));
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    for (int i = 0; i < 12; ++i) t[16 + i] = iend[i];
    sizes[win] = total;
  }
}

static bool png_size_ok(int P) { return P >= 1 && P <= HIPAC_PNG_MAX_P; }
static int png_band_rows(int P) {
  const int r = kBand / (1 + 3 * P);
  return r < 1 ? 1 : r;
}
static int png_n_bands(int P) { return (P + png_band_rows(P) - 1) / png_band_rows(P); }
static size_t png_slot_stride(int P) { return align256((size_t)png_band_rows(P) * (1 + 3 * P) + 16); }

}  // namespace hipac

using namespace hipac;

extern "C" int hipac_png_abi_version(void) { return HIPAC_PNG_ABI_VERSION; }

extern "C" size_t hipac_png_file_bound(int P) {
  if (!png_size_ok(P)) return 0;
  const size_t nb = (size_t)png_n_bands(P);
  return 8 + 25 + 12 * nb + 2 + (size_t)P * (1 + 3 * (size_t)P) + 5 * nb + 5 * (nb - 1) + 16 + 12;
}

extern "C" size_t hipac_png_workspace_bytes(int P, int n) {
  if (!png_size_ok(P) || n < 1 || n > HIPAC_PNG_MAX_WINDOWS) return 0;
  const size_t bands = (size_t)n * png_n_bands(P);
  return bands * png_slot_stride(P) + align256(bands * sizeof(PngBandMeta));
}

extern "C" int hipac_png_encode_windows(const uint8_t* level, int W, int H, int64_t pitch_bytes, const int32_t* xy, int n, int P,
                                        uint8_t* out, int64_t out_stride, int64_t* sizes_dev, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  HIPAC_REQUIRE(level && xy && out && sizes_dev && workspace, HIPAC_EINVAL, "png_encode_windows: null argument");
  HIPAC_REQUIRE(W >= 1 && H >= 1 && pitch_bytes >= (int64_t)W * 3, HIPAC_EINVAL,
                "png_encode_windows: bad geometry %d x %d, pitch %lld", W, H, (long long)pitch_bytes);
  HIPAC_REQUIRE(n >= 1 && n <= HIPAC_PNG_MAX_WINDOWS, HIPAC_EINVAL, "png_encode_windows: n %d outside 1..%d", n,
                HIPAC_PNG_MAX_WINDOWS);
  HIPAC_REQUIRE(png_size_ok(P), HIPAC_EINVAL, "png_encode_windows: P %d outside 1..%d", P, HIPAC_PNG_MAX_P);
  HIPAC_REQUIRE(((uintptr_t)workspace & 255) == 0, HIPAC_EINVAL, "png_encode_windows: workspace not 256-byte aligned");
  HIPAC_REQUIRE(((uintptr_t)sizes_dev & 7) == 0 && ((uintptr_t)xy & 3) == 0, HIPAC_EINVAL,
                "png_encode_windows: xy or sizes_dev not aligned to its element");
  const size_t need = hipac_png_workspace_bytes(P, n);
  HIPAC_REQUIRE(workspace_bytes >= need, HIPAC_EWORKSPACE, "png_encode_windows: workspace %zu bytes, %zu needed", workspace_bytes,
                need);
  HIPAC_REQUIRE(out_stride >= (int64_t)hipac_png_file_bound(P), HIPAC_EINVAL,
                "png_encode_windows: out_stride %lld below hipac_png_file_bound(%d) = %zu", (long long)out_stride, P,
                hipac_png_file_bound(P));
  const int rows = png_band_rows(P), nb = png_n_bands(P);
  const size_t stride = png_slot_stride(P), bands = (size_t)n * nb;
  uint8_t* const slots = (uint8_t*)workspace;
  PngBandMeta* const meta = (PngBandMeta*)(slots + bands * stride);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(png_band_kernel, dim3((unsigned)bands), dim3(kPngThreads), 0, s, level, W, H, (long long)pitch_bytes,
                     (const int*)xy, n, P, rows, nb, slots, (long long)stride, meta);
  hipLaunchKernelGGL(png_gather_kernel, dim3((unsigned)n), dim3(kPngThreads), 0, s, (const uint8_t*)slots, (long long)stride,
                     (const PngBandMeta*)meta, n, P, rows, nb, out, (long long)out_stride, (long long*)sizes_dev);
  HIPAC_CHECK_HIP(hipGetLastError());
  return 0;
}

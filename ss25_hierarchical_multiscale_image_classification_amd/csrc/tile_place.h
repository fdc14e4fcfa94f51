// The last step of the TIFF tile decoders that leave a tile's samples in scratch (lzw.hip, deflate.hip): undo the predictor and
// place the tile into its level, clipped.  16 lanes per tile row: a lane owns a run of whole 4-pixel groups, sums it, the 16 sums
// are scanned with shuffles, and the run is written as 12-byte groups (three dword stores where the address allows, bytes at the
// clipped edge).  `Level` has the fields of hipac_lzw_level; `Levels` is { Level l[]; int n; }.  Status 0 = decoded, 1 = refused
// (the tile's pixels are written as 0); tiles of any other status are skipped.
#pragma once
#include "common.h"

namespace hipac {

// four pixels of `S` samples at byte offset `o` of a decoded tile, as bytes v[px][s]; pixels at or behind `avail` read as 0
template <int S>
__device__ __forceinline__ void tile_load4(const uint8_t* tile, uint32_t o, int avail, uint8_t (&v)[4][4]) {
  if (avail >= 4 && (o & 3u) == 0) {
    uint32_t w[S];
#pragma unroll
    for (int k = 0; k < S; ++k) w[k] = *reinterpret_cast<const uint32_t*>(tile + o + 4 * k);
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int b = p * S + s;
        v[p][s] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
      }
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int s = 0; s < S; ++s) v[p][s] = p < avail ? tile[o + p * S + s] : (uint8_t)0;
  }
}

template <int S, class Level>
__device__ __forceinline__ void tile_place_rows(const Level& L, int x0, int y0, const uint8_t* tile, bool zero) {
  const int g = threadIdx.x & 15, r = (int)blockIdx.x * 16 + ((int)threadIdx.x >> 4);
  const bool row_ok = r < L.tile_h && y0 + r < L.H;  // lanes of rows outside still take part in the shuffles
  const int seg = ((L.tile_w + 15) / 16 + 3) & ~3;  // pixels per lane: whole groups of four
  const int p0 = g * seg, p1 = min(p0 + seg, L.tile_w);
  const uint32_t row = (uint32_t)r * (uint32_t)L.tile_w * S;
  uint32_t run[S];
#pragma unroll
  for (int s = 0; s < S; ++s) run[s] = 0;
  if (L.predictor == 2 && !zero) {
    if (row_ok)
      for (int p = p0; p < p1; p += 4) {
        uint8_t v[4][4];
        tile_load4<S>(tile, row + (uint32_t)p * S, p1 - p, v);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int s = 0; s < S; ++s) run[s] += v[q][s];
      }
#pragma unroll
    for (int s = 0; s < S; ++s) {  // inclusive scan over the 16 lanes of the row, then exclusive
      uint32_t inc = run[s];
#pragma unroll
      for (int d = 1; d < 16; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 16);
        if (g >= d) inc += up;
      }
      run[s] = inc - run[s];
    }
  }
  if (!row_ok) return;
  const int clip = min(L.tile_w, L.W - x0);  // pixels of this tile inside the level
  uint8_t* drow = L.pixels + (long long)(y0 + r) * L.pitch_bytes + (long long)x0 * 3;
  for (int p = p0; p < p1 && p < clip; p += 4) {
    uint8_t v[4][4] = {};
    if (!zero) tile_load4<S>(tile, row + (uint32_t)p * S, p1 - p, v);
    uint8_t o[12];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (L.predictor == 2) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
          run[s] += v[q][s];
          v[q][s] = (uint8_t)run[s];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) o[3 * q + c] = v[q][S == 1 ? 0 : c];
    }
    uint8_t* d = drow + (long long)p * 3;
    if (p + 4 <= clip && ((uintptr_t)d & 3) == 0) {
      uint32_t w[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) w[k] = o[4 * k] | (uint32_t)o[4 * k + 1] << 8 | (uint32_t)o[4 * k + 2] << 16 | (uint32_t)o[4 * k + 3] << 24;
#pragma unroll
      for (int k = 0; k < 3; ++k) reinterpret_cast<uint32_t*>(d)[k] = w[k];
    } else {
#pragma unroll
      for (int b = 0; b < 12; ++b)
        if (p + b / 3 < clip) d[b] = o[b];
    }
  }
}

// grid (ceil(largest tile_h / 16), n_tiles), 256 threads = 16 rows x 16 lanes.  The decode kernel has checked (x, y, level) of
// every tile whose status is 0 or 1.
template <class Levels>
__device__ __forceinline__ void tile_place(const Levels& lv, const int* __restrict__ tile_xyl, const uint8_t* __restrict__ status,
                                           const uint8_t* __restrict__ scratch, long long stride) {
  const int t = blockIdx.y;
  const int st = status[t];
  if (st != 0 && st != 1) return;
  const int x0 = tile_xyl[3 * t], y0 = tile_xyl[3 * t + 1], li = tile_xyl[3 * t + 2];
  if (li < 0 || li >= lv.n) return;
  const auto& L = lv.l[li];
  if ((int)blockIdx.x * 16 >= L.tile_h) return;
  const uint8_t* tile = scratch + (long long)t * stride;
  const bool zero = st == 1;
  if (L.samples == 1) tile_place_rows<1>(L, x0, y0, tile, zero);
  else if (L.samples == 3) tile_place_rows<3>(L, x0, y0, tile, zero);
  else tile_place_rows<4>(L, x0, y0, tile, zero);
}

}  // namespace hipac

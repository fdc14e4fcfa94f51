/*
 * hipac_lzw.h -- C ABI of the TIFF LZW tile decoder of libhipac_hip.so (gfx950): tiles of a tiled pyramidal TIFF with
 * compression 5 decoded in HBM, straight into a level image -- the LZW counterpart of hipac_jpeg_decode_tiles (include/hipac.h).
 * The file's bytes go to the device once; nothing is parsed on the host.
 *
 * These entry points live in the same shared library as include/hipac.h but carry their own version number, so adding them
 * leaves hipac.h's ABI untouched.
 *
 * Conventions: those of include/hipac.h.  Plain pointers and sizes; every data pointer is DEVICE memory unless its comment says
 * HOST; all work is enqueued asynchronously on `stream` (hipStream_t as void*, NULL = default stream); nothing synchronises the
 * device; the caller owns every buffer; 0 on success, otherwise a hipError_t value or a HIPAC_E* code, with the message in the
 * thread-local last-error string of hipac.h.  Every argument check answers before the first launch.
 *
 * The stream format is TIFF 6.0 LZW as tiff_pyramid.lzw_decode states it, which is the definition: MSB-first codes of 9 to 12
 * bits, 256 = Clear, 257 = EOI, the width grows one code early (table sizes 511, 1023, 2047), the code after a Clear is a literal
 * (further Clears are skipped, EOI ends the stream), a code equal to the next free entry is the previous string plus its own first
 * byte, a table filled to 4095 without a Clear stays at 12 bits and takes no entries.  Decoding stops at EOI, after
 * tile_w * tile_h * samples bytes, or when fewer bits than one code are left; bytes not written are 0.  Predictor 2 (horizontal
 * differencing, 8-bit samples) is undone per row and sample as a running sum mod 256 over the whole tile width.
 *
 * Integer arithmetic only and no atomics: two runs give the same bytes.  Every table index, every source and destination offset
 * and every read of the compressed bytes is range-checked inside the kernels: no stream, and no tile descriptor, makes them touch
 * memory outside the tile's scratch, the level images as `levels` describes them, or [file_dev, file_dev + file_bytes).
 */
#ifndef HIPAC_LZW_H_
#define HIPAC_LZW_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_LZW_ABI_VERSION 1

#define HIPAC_LZW_MAX_TILE_BYTES 1048576 /* tile_w * tile_h * samples: a table entry keeps a 20-bit offset into the tile */
#define HIPAC_LZW_MAX_TILES 65535        /* per call */
#define HIPAC_LZW_MAX_LEVELS 16          /* the level table travels as a kernel argument */

/* status_dev values */
#define HIPAC_LZW_OK 0       /* decoded and placed */
#define HIPAC_LZW_REFUSED 1  /* malformed stream (see above, or the old LSB-first variant): the tile's pixels are written as 0 */
#define HIPAC_LZW_MISSING 2  /* byte count 0: the level keeps what it holds */
#define HIPAC_LZW_BAD_TILE 3 /* the byte range leaves the file, or (x, y, level) is no tile of `levels`: nothing is written */

/* Where the tiles of a level go: DEVICE uint8[H][pitch_bytes] of RGB pixels, W of them per row (pitch_bytes >= 3 W; tiles are
 * clipped to W x H); the level's tile size; samples per pixel 1 (replicated to R, G and B), 3, or 4 (alpha dropped); predictor
 * 1 or 2. */
typedef struct {
  uint8_t* pixels;
  int64_t pitch_bytes;
  int32_t W, H, tile_w, tile_h, samples, predictor;
} hipac_lzw_level;

int hipac_lzw_abi_version(void);

/* Scratch for n_tiles tiles of at most tile_w x tile_h x samples.  0 for sizes the decoder refuses: a side < 1, samples other
 * than 1, 3, 4, more than HIPAC_LZW_MAX_TILE_BYTES per tile, n_tiles outside 1 .. HIPAC_LZW_MAX_TILES. */
size_t hipac_lzw_workspace_bytes(int tile_w, int tile_h, int samples, int n_tiles);

/*   file_dev, file_bytes : the file's bytes; not one byte behind them is read
 *   levels               : HOST hipac_lzw_level[n_levels], n_levels <= HIPAC_LZW_MAX_LEVELS
 *   tile_off, tile_len   : int64[n_tiles] TileOffsets / TileByteCounts (len 0 = missing tile)
 *   tile_xyl             : int32[n_tiles][3]: (x, y) of the tile's top-left pixel (multiples of the tile size, inside the
 *                          level) and its index into `levels`; tiles of all levels share one call
 *   workspace            : hipac_lzw_workspace_bytes(largest tile_w, largest tile_h, largest samples, n_tiles) bytes, 256-byte
 *                          aligned
 *   status_dev           : uint8[n_tiles], one HIPAC_LZW_* value per tile; read it after the stream has been waited for */
int hipac_lzw_decode_tiles(const uint8_t* file_dev, int64_t file_bytes, const hipac_lzw_level* levels, int n_levels,
                           const int64_t* tile_off, const int64_t* tile_len, const int32_t* tile_xyl, int n_tiles, void* workspace,
                           size_t workspace_bytes, uint8_t* status_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_LZW_H_ */

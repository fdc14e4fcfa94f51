/*
 * hipac_deflate.h -- C ABI of the TIFF deflate tile decoder of libhipac_hip.so (gfx950): tiles of a tiled pyramidal TIFF with
 * compression 8 (or 32946) inflated in HBM, straight into a level image -- the deflate counterpart of hipac_lzw_decode_tiles
 * (include/hipac_lzw.h).  The file's bytes go to the device once; nothing is parsed on the host.
 *
 * These entry points live in the same shared library as include/hipac.h but carry their own version number, so adding them
 * leaves hipac.h's and hipac_lzw.h's ABI untouched.
 *
 * Conventions: those of include/hipac.h.  Plain pointers and sizes; every data pointer is DEVICE memory unless its comment says
 * HOST; all work is enqueued asynchronously on `stream` (hipStream_t as void*, NULL = default stream); nothing synchronises the
 * device; the caller owns every buffer; 0 on success, otherwise a hipError_t value or a HIPAC_E* code, with the message in the
 * thread-local last-error string of hipac.h.  Every argument check answers before the first launch.
 *
 * The stream format is a zlib stream (RFC 1950 around RFC 1951) as tiff_pyramid.inflate states it, which is the definition and
 * agrees with zlib: a tile is decoded (status OK) when the header is valid (CM = 8, CINFO <= 7, (CMF * 256 + FLG) % 31 == 0,
 * FDICT = 0), every block is well-formed, exactly tile_w * tile_h * samples bytes come out and the big-endian Adler-32 behind the
 * last block matches; bytes behind the checksum are ignored.  Everything else is REFUSED: block type 3, a stored block whose LEN
 * and ~NLEN disagree, more than 286 literal/length or 30 distance code lengths, an over-subscribed set of code lengths or an
 * incomplete one (but a single one-bit literal/length or distance code, and a distance set without codes, are taken), a repeat
 * without a previous length or past HLIT + HDIST, no end-of-block code, a bit pattern no code owns, length symbols 286 / 287,
 * distance symbols 30 / 31, a distance beyond the bytes written so far, input that ends mid-stream, output beyond the tile or
 * short of it, a checksum mismatch.  Predictor 2 (horizontal differencing, 8-bit samples) is undone per row and sample as a
 * running sum mod 256 over the whole tile width.
 *
 * Integer arithmetic only and no atomics: two runs give the same bytes.  Every read of the compressed bytes, every index into a
 * Huffman table, every back-reference and every destination offset is range-checked inside the kernels: no stream, and no tile
 * descriptor, makes them touch memory outside the tile's scratch, the level images as `levels` describes them, or
 * [file_dev, file_dev + file_bytes).
 */
#ifndef HIPAC_DEFLATE_H_
#define HIPAC_DEFLATE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_DEFLATE_ABI_VERSION 1

#define HIPAC_DEFLATE_MAX_TILE_BYTES 1048576 /* tile_w * tile_h * samples (512 x 512 x 4): offsets into a tile stay below 2^20 */
#define HIPAC_DEFLATE_MAX_TILES 65535        /* per call */
#define HIPAC_DEFLATE_MAX_LEVELS 16          /* the level table travels as a kernel argument */

/* status_dev values */
#define HIPAC_DEFLATE_OK 0       /* decoded and placed */
#define HIPAC_DEFLATE_REFUSED 1  /* not a stream the definition accepts (see above): the tile's pixels are written as 0 */
#define HIPAC_DEFLATE_MISSING 2  /* byte count 0: the level keeps what it holds */
#define HIPAC_DEFLATE_BAD_TILE 3 /* the byte range leaves the file, or (x, y, level) is no tile of `levels`: nothing is written */

/* Where the tiles of a level go: DEVICE uint8[H][pitch_bytes] of RGB pixels, W of them per row (pitch_bytes >= 3 W; tiles are
 * clipped to W x H); the level's tile size; samples per pixel 1 (replicated to R, G and B), 3, or 4 (alpha dropped); predictor
 * 1 or 2.  The fields of hipac_lzw_level. */
typedef struct {
  uint8_t* pixels;
  int64_t pitch_bytes;
  int32_t W, H, tile_w, tile_h, samples, predictor;
} hipac_deflate_level;

int hipac_deflate_abi_version(void);

/* Scratch for n_tiles tiles of at most tile_w x tile_h x samples.  0 for sizes the decoder refuses: a side < 1, samples other
 * than 1, 3, 4, more than HIPAC_DEFLATE_MAX_TILE_BYTES per tile, n_tiles outside 1 .. HIPAC_DEFLATE_MAX_TILES. */
size_t hipac_deflate_workspace_bytes(int tile_w, int tile_h, int samples, int n_tiles);

/*   file_dev, file_bytes : the file's bytes; not one byte behind them is read
 *   levels               : HOST hipac_deflate_level[n_levels], n_levels <= HIPAC_DEFLATE_MAX_LEVELS
 *   tile_off, tile_len   : int64[n_tiles] TileOffsets / TileByteCounts (len 0 = missing tile)
 *   tile_xyl             : int32[n_tiles][3]: (x, y) of the tile's top-left pixel (multiples of the tile size, inside the
 *                          level) and its index into `levels`; tiles of all levels share one call
 *   workspace            : hipac_deflate_workspace_bytes(largest tile_w, largest tile_h, largest samples, n_tiles) bytes,
 *                          256-byte aligned
 *   status_dev           : uint8[n_tiles], one HIPAC_DEFLATE_* value per tile; read it after the stream has been waited for */
int hipac_deflate_decode_tiles(const uint8_t* file_dev, int64_t file_bytes, const hipac_deflate_level* levels, int n_levels,
                               const int64_t* tile_off, const int64_t* tile_len, const int32_t* tile_xyl, int n_tiles,
                               void* workspace, size_t workspace_bytes, uint8_t* status_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_DEFLATE_H_ */

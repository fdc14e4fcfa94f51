/*
 * hipac_png.h -- C ABI of the PNG patch encoder of libhipac_hip.so (gfx950): windows of a resident RGB level image become
 * complete PNG files in HBM -- row filter, deflate and both checksums run on the device, only compressed bytes go to the host.
 * It is the encoder counterpart of hipac_deflate_decode_tiles (include/hipac_deflate.h).
 *
 * These entry points live in the same shared library as include/hipac.h but carry their own version number, so adding them
 * leaves every other header's ABI untouched.
 *
 * Conventions: those of include/hipac.h.  Plain pointers and sizes; every data pointer is DEVICE memory; all work is enqueued
 * asynchronously on `stream` (hipStream_t as void*, NULL = default stream); nothing synchronises the device; the caller owns
 * every buffer; 0 on success, otherwise a hipError_t value or a HIPAC_E* code, with the message in the thread-local last-error
 * string of hipac.h.  Every argument check answers before the first launch.
 *
 * The format (tests/png_encode_cpu.py restates it byte for byte and is what the device is compared with):
 *
 *   file     PNG signature; IHDR (P x P, bit depth 8, colour type 2, no interlace); one IDAT chunk per band; one IDAT chunk
 *            holding the four Adler-32 bytes; IEND.
 *   pixels   the P x P window whose top-left corner is (x, y) in the level image, clipped to W x H; every byte outside the
 *            level image is 255.
 *   filter   per row the type of None, Sub, Up, Average, Paeth (3 bytes per pixel) whose filtered row has the smallest sum of
 *            min(v, 256 - v); ties go to the lowest type; the row above the first is zeros.  The filter reads raw pixels, so it
 *            crosses band borders.
 *   bands    the filtered stream (P rows of 1 + 3 P bytes) is cut into bands of whole rows, each as many rows as fit into
 *            HIPAC_PNG_BAND_BYTES and at least one.  Every band is compressed on its own.
 *   tokens   a maximal run of n >= 4 equal bytes inside a band is one literal followed by distance-1 matches over the other
 *            m = n - 1 bytes: m / 258 matches of length 258, then, with r = m % 258, one match of length r when r >= 3, or r
 *            literals when r is 1 or 2.  Everything else is literals.
 *   block    a band is ONE deflate block, of the type with the smallest exact bit count among stored (40 + 8 L bits for a band
 *            of L bytes: the band starts byte-aligned), fixed Huffman and dynamic Huffman; ties go to the simpler type.
 *   codes    dynamic blocks: symbols with a non-zero count are sorted by (count, symbol) and merged with the two-queue method;
 *            of a leaf and an internal node of equal weight the leaf goes first, internal nodes go in the order they were made.
 *            If a code is longer than the limit (15 for literal/length codes, 7 for the code-length code) every non-zero count
 *            c becomes (c + 1) / 2 and the tree is built again.  A single used symbol gets length 1.  Codes are canonical
 *            (RFC 1951 3.2.2).  HDIST = 0: distance code 0 with length 1.  The code lengths (HLIT + 257 of them, then the one
 *            distance length) are run-length coded greedily: a run of zeros takes 18 (up to 138) while 11 or more remain, then
 *            17 for 3..10, else single zeros; a run of a non-zero length sends the length once, then 16 (up to 6) while 3 or
 *            more remain, else the length again.  HLIT and HCLEN are trimmed as far as RFC 1951 allows.
 *   align    every band but the last is followed by an empty stored block (3 header bits, padding, 00 00 FF FF); the last
 *            band's block carries BFINAL and is padded to a byte.
 *   zlib     78 01 in front of the first band (inside its IDAT chunk); the Adler-32 of the whole filtered stream behind the
 *            last, combined from per-band sums.
 *
 * Integer arithmetic only; the bit stream is OR-ed into zeroed LDS dwords, so the bytes are a pure function of the pixels: two
 * runs, and two different batch compositions, give the same files.  Every source read is range-checked against W, H and
 * pitch_bytes, every table index against its table, every scratch and output offset against the workspace and out_stride: no
 * window descriptor makes the kernels touch memory outside the level image, the workspace, `out` and `sizes_dev` as the
 * arguments describe them.
 */
#ifndef HIPAC_PNG_H_
#define HIPAC_PNG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_PNG_ABI_VERSION 1

#define HIPAC_PNG_BAND_BYTES 24576 /* filtered bytes per band (<= 65535: a stored band is one stored block); whole rows */
#define HIPAC_PNG_MAX_P 1792       /* window side: 1 .. HIPAC_PNG_MAX_P (the level-0 window) */
#define HIPAC_PNG_MAX_WINDOWS 4096 /* per call */

int hipac_png_abi_version(void);

/* Exact upper bound of one file's size: every band stored, plus every chunk and wrapper byte.  0 for P outside
 * 1 .. HIPAC_PNG_MAX_P. */
size_t hipac_png_file_bound(int P);

/* Scratch for n windows of side P.  0 for refused sizes: P outside 1 .. HIPAC_PNG_MAX_P, n outside 1 .. HIPAC_PNG_MAX_WINDOWS. */
size_t hipac_png_workspace_bytes(int P, int n);

/*   level, W, H, pitch_bytes : uint8[H][pitch_bytes] of RGB pixels, W of them per row (pitch_bytes >= 3 W)
 *   xy                       : int32[n][2], the top-left corner of every window; any value is taken -- a window partly or
 *                              entirely outside the level is padded with white, not refused
 *   P                        : window side
 *   out, out_stride          : file i starts at out + i * out_stride; out_stride >= hipac_png_file_bound(P); bytes behind a
 *                              file's size are not written
 *   sizes_dev                : int64[n], the size of every file; read it after the stream has been waited for
 *   workspace                : hipac_png_workspace_bytes(P, n) bytes, 256-byte aligned */
int hipac_png_encode_windows(const uint8_t* level, int W, int H, int64_t pitch_bytes, const int32_t* xy, int n, int P, uint8_t* out,
                             int64_t out_stride, int64_t* sizes_dev, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_PNG_H_ */

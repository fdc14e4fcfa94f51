/*
 * hipac_stain.h -- C ABI of the Macenko stain normalisation of libhipac_hip.so (gfx950): the opt-in stage of
 * `--stain_norm macenko`.  The stain vectors of a slide are fitted on its coarsest resident level (three reductions over the
 * level and a handful of 3 x 3 double-precision operations, all on the device), and every level is then mapped pixel by pixel
 * to the target stain appearance: od' = M od in optical-density space.  The reference has no such stage; this is the project's
 * addition and is off in parity runs.
 *
 * These entry points live in the same shared library as include/hipac.h but carry their own version number, so adding them
 * leaves hipac.h's ABI untouched.
 *
 * Conventions: those of include/hipac.h.  Plain pointers and sizes; every data pointer is DEVICE memory unless its comment says
 * HOST; all work is enqueued asynchronously on `stream` (hipStream_t as void*, NULL = default stream); nothing synchronises the
 * device; the caller owns every buffer; 0 on success, otherwise a hipError_t value or a HIPAC_E* code, with the message in the
 * thread-local last-error string of hipac.h.  Every argument check answers before the first launch.
 *
 * Arithmetic.  Optical densities are integers in units of 2^-12: od[v] = rint(2^12 ln(256 / (v + 1))), a literal table of the
 * library (od[0] = 22713, od[255] = 0, strictly decreasing).  Sums and histograms are integers and the only atomics are integer
 * adds, which commute.  The small matrices are IEEE double with one rounding per operation in a fixed order (the library is
 * compiled without floating-point contraction; only + - * / sqrt and rint are used).  Every output is bitwise identical from run
 * to run and equal to the numpy restatement tests/stain_cpu.py, which is the definition of every formula below.
 *
 * Images: uint8[height][pitch bytes] of RGB pixels, `width` of them per row; 16-byte aligned, pitch a multiple of 48 bytes and
 * at least 3 * 16 * ceil(width / 16); width, height >= 1 and width * height < 2^32, which keeps every sum inside int64.  Bytes of
 * a row behind pixel `width` are never read as pixels and never written.
 *
 * Tissue pixels: a pixel counts iff min_c od[pixel_c] >= beta_q (0 <= beta_q <= od[0]; rint(beta 2^12)) and, when `mask` is not
 * NULL, mask[y / f][x / f] != 0.  mask: uint8[mh][mw] as hipac_tissue_mask makes it, f = 4, 8, 16 or 32 level pixels per mask
 * pixel, mw = ceil(width / f), mh = ceil(height / f).  With mask == NULL, mw, mh and f are ignored.
 *
 * A stage whose input status is 0 writes zeros and status 0; hipac_stain_apply then copies the pixels.
 */
#ifndef HIPAC_STAIN_H_
#define HIPAC_STAIN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPAC_STAIN_ABI_VERSION 1

#define HIPAC_STAIN_Q 12              /* optical densities are integers in units of 2^-12 */
#define HIPAC_STAIN_OD_MAX 22713      /* od[0] */
#define HIPAC_STAIN_ANGLE_BINS 4096   /* NB */
#define HIPAC_STAIN_CONC_BINS 4096    /* NBC, over [0, 8) OD */
#define HIPAC_STAIN_JACOBI_SWEEPS 10
#define HIPAC_STAIN_MAX_ALPHA 499     /* alpha_permille is 1 .. 499 */

int hipac_stain_abi_version(void);

/* Copies the optical-density table out.  od: HOST int32[256].  Touches no device. */
int hipac_stain_od_table(int32_t* od);

/* moments: int64[10] = n, S_0 S_1 S_2, S_00 S_01 S_02 S_11 S_12 S_22 over the tissue pixels' integer ODs; zeroed by this call.
 * Reduced per workgroup, then one integer atomic per value. */
int hipac_stain_moments(const uint8_t* img, int width, int height, size_t pitch, const uint8_t* mask, int mw, int mh, int f,
                        int beta_q, int64_t* moments, void* stream);

/* The plane of the stains.  One thread.  cov[a][b] = (S_ab - S_a (S_b / n)) / (n - 1) for a <= b, mirrored; cyclic Jacobi with the
 * pairs (0, 1), (0, 2), (1, 2), HIPAC_STAIN_JACOBI_SWEEPS sweeps, a rotation skipped only when its off-diagonal is exactly 0.
 * basis: double[2][3] = the eigenvectors of the two largest eigenvalues (ties to the lowest index), each flipped so that its
 * component sum is not negative.  status: int32[1] = 0 (and basis 0) if n < 2 or the second eigenvalue is not positive, else 1. */
int hipac_stain_basis(const int64_t* moments, double* basis, int32_t* status, void* stream);

/* hist: uint32[HIPAC_STAIN_ANGLE_BINS], zeroed by this call.  Per tissue pixel x = (o0 v1[0] + o1 v1[1]) + o2 v1[2], y likewise
 * with v2, d = y / (x + |y|), bin = min(NB - 1, floor((d + 1) NB / 2)); x <= 0: bin 0 if y < 0, else NB - 1.  Counted per
 * workgroup in LDS, then added with integer atomics. */
int hipac_stain_angle_hist(const uint8_t* img, int width, int height, size_t pitch, const uint8_t* mask, int mw, int mh, int f,
                           int beta_q, const double* basis, uint32_t* hist, void* stream);

/* The stain vectors.  n = sum hist, k = max(1, ceil(alpha_permille n / 1000)); b_lo / b_hi = the first bins whose cumulative
 * counts reach k / n - k + 1; bin centre d = (2 b + 1) / NB - 1, direction (1 - |d|, d) normalised, vector v1 cx + v2 cy; the
 * vector with the larger red component is haematoxylin.
 * he_p: double[12] = HE[3][2] (columns H, E), then P[2][3] = (HE^T HE)^-1 HE^T by the closed-form 2 x 2 inverse.
 * status: int32[1] = 0 (and he_p 0) if basis_status[0] is 0, n is 0 or the determinant is not positive, else 1.
 * 1 <= alpha_permille <= HIPAC_STAIN_MAX_ALPHA. */
int hipac_stain_vectors(const uint32_t* hist, const double* basis, const int32_t* basis_status, int alpha_permille, double* he_p,
                        int32_t* status, void* stream);

/* chist: uint32[2][HIPAC_STAIN_CONC_BINS], zeroed by this call.  Per tissue pixel and stain s, C = (o0 P[s][0] + o1 P[s][1]) +
 * o2 P[s][2], bin = clamp(floor(C / 8), 0, NBC - 1) (C is in units of 2^-12: NBC / (8 2^12) = 1 / 8). */
int hipac_stain_conc_hist(const uint8_t* img, int width, int height, size_t pitch, const uint8_t* mask, int mw, int mh, int f,
                          int beta_q, const double* he_p, uint32_t* chist, void* stream);

/* The pixel map.  maxC_s = (2 b + 1) / 1024 with b the 99th-percentile bin of chist[s] (the rank rule above at 10 permille);
 * g_s = maxCref_s / maxC_s; M[c][j] = HEref[c][0] (g_0 P[0][j]) + HEref[c][1] (g_1 P[1][j]).
 * target: HOST double[8] = HEref[3][2], then maxCref[2], all finite, maxCref > 0.
 * m_maxc: double[11] = M[3][3], then maxC[2].  status: int32[1] = vec_status[0] (0: m_maxc is 0). */
int hipac_stain_matrix(const uint32_t* chist, const double* he_p, const int32_t* vec_status, const double* target, double* m_maxc,
                       int32_t* status, void* stream);

/* Applies the map to an image.  Per pixel and channel c: od'_c = (M[c][0] o0 + M[c][1] o1) + M[c][2] o2 with o = od[pixel],
 * q = clamp(rint(od'_c), 0, od[0]), out_c = inv[q], inv[q] = the v whose od[v] is nearest to q, ties to the larger v.
 * m: double[9] and status: int32[1] are read from DEVICE memory (the host never waits for the fit); status 0 copies the pixels.
 * dst == src (in place) or dst disjoint from src, both with the same pitch; a partial overlap is refused.  16-byte loads and
 * stores, both tables in LDS. */
int hipac_stain_apply(const uint8_t* src, uint8_t* dst, int width, int height, size_t pitch, const double* m, const int32_t* status,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPAC_STAIN_H_ */

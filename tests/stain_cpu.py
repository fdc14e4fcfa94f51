"""numpy restatement of the Macenko stain normalisation (include/hipac_stain.h), one function per stage, and
the textbook float64 algorithm it is measured against.  Not a test: tests/test_stain_host.py checks the restatement against the
textbook, tests/test_gpu_stain.py compares the device with it bit for bit.

Optical densities are integers in units of 2^-12 (the table ``OD``); the sums and histograms are integers; the small matrices are
IEEE double with one rounding per operation, written out operation by operation (Python floats), so that the device, compiled
without floating-point contraction, reproduces every bit."""
import math

import numpy as np

Q = 12
NB = 4096    # angle bins
NBC = 4096   # concentration bins over [0, 8) OD
SWEEPS = 10  # cyclic Jacobi sweeps
HE_REF = ((0.5626, 0.2159), (0.7201, 0.8012), (0.4062, 0.5581))
MAXC_REF = (1.9705, 1.0308)

OD = np.rint(4096.0 * np.log(256.0 / (np.arange(256) + 1.0))).astype(np.int32)  # the library carries it as a literal table
OD_MAX = int(OD[0])


def inverse_table(od=OD):
    """uint8[od[0] + 1]: inv[q] = the v whose od[v] is nearest to q, ties to the larger v.  Integers only."""
    od = np.asarray(od).astype(np.int64)
    q = np.arange(int(od[0]) + 1, dtype=np.int64)
    dist = np.abs(od[None, :] - q[:, None])                       # [q, v]
    return (255 - np.argmin(dist[:, ::-1], axis=1)).astype(np.uint8)  # argmin takes the first minimum: the largest v


INV = inverse_table()


def beta_q(beta):
    return int(np.rint(float(beta) * 4096.0))


def alpha_permille(alpha_percent):
    return int(np.rint(float(alpha_percent) * 10.0))


def pixel_od(level, width):
    """int32[H, width, 3] optical densities of the pixels of ``level`` uint8[H, Wpad >= width, 3]."""
    return OD[np.asarray(level)[:, :width]]


def tissue_pixels(level, width, bq, mask=None, f=None):
    """bool[H, width]: min_c od >= bq, and the mask pixel (f level pixels per mask pixel) set when a mask is given."""
    o = pixel_od(level, width)
    t = o.min(axis=2) >= int(bq)
    if mask is not None:
        H = o.shape[0]
        m = np.asarray(mask).astype(bool)
        assert m.shape == (-(-H // f), -(-width // f))
        t &= m[np.arange(H)[:, None] // f, np.arange(width)[None, :] // f]
    return t


def tissue_od(level, width, bq, mask=None, f=None):
    """int64[n, 3]: the ODs of the tissue pixels in row-major order."""
    return pixel_od(level, width)[tissue_pixels(level, width, bq, mask, f)].astype(np.int64)


PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def moments(o):
    """int64[10]: n, S_0..S_2, S_00 S_01 S_02 S_11 S_12 S_22 of int64[n, 3] ODs."""
    o = np.asarray(o, np.int64).reshape(-1, 3)
    return np.array([o.shape[0], *o.sum(axis=0), *[(o[:, a] * o[:, b]).sum() for a, b in PAIRS]], np.int64)


def jacobi(A):
    """(eigenvalues [3], V [3][3], eigenvectors in columns) of a symmetric 3 x 3 list of floats: cyclic Jacobi, pairs (0, 1), (0, 2),
    (1, 2), SWEEPS sweeps; a rotation is skipped only when its off-diagonal element is exactly 0."""
    A = [[float(x) for x in row] for row in A]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = A[p][q]
            if apq == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            at = abs(theta)
            t = 1.0 / (at + math.sqrt(theta * theta + 1.0))
            if theta < 0.0:
                t = -t
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            for k in range(3):
                akp, akq = A[k][p], A[k][q]
                A[k][p] = c * akp - s * akq
                A[k][q] = s * akp + c * akq
            for k in range(3):
                apk, aqk = A[p][k], A[q][k]
                A[p][k] = c * apk - s * aqk
                A[q][k] = s * apk + c * aqk
            A[p][q] = A[q][p] = 0.0
            for k in range(3):
                vkp, vkq = V[k][p], V[k][q]
                V[k][p] = c * vkp - s * vkq
                V[k][q] = s * vkp + c * vkq
    return [A[0][0], A[1][1], A[2][2]], V


def covariance(mom):
    """Upper triangle mirrored: cov[a][b] = (S_ab - S_a * (S_b / n)) / (n - 1), a <= b, every operand converted to double first."""
    m = [int(x) for x in mom]
    n = float(m[0])
    mean = [float(m[1 + c]) / n for c in range(3)]
    cov = [[0.0] * 3 for _ in range(3)]
    for i, (a, b) in enumerate(PAIRS):
        cov[a][b] = cov[b][a] = (float(m[4 + i]) - float(m[1 + a]) * mean[b]) / (n - 1.0)
    return cov


def basis(mom):
    """(basis float64[2, 3] = v1, v2; status).  status 0 (basis all zero) if n < 2 or the second eigenvalue is not positive."""
    out = np.zeros((2, 3), np.float64)
    if int(mom[0]) < 2:
        return out, 0
    w, V = jacobi(covariance(mom))
    i1 = 0
    for i in (1, 2):
        if w[i] > w[i1]:
            i1 = i
    i2 = -1
    for i in range(3):
        if i != i1 and (i2 < 0 or w[i] > w[i2]):
            i2 = i
    if not w[i2] > 0.0:
        return out, 0
    for r, i in enumerate((i1, i2)):
        v = [V[0][i], V[1][i], V[2][i]]
        if (v[0] + v[1]) + v[2] < 0.0:
            v = [-x for x in v]
        out[r] = v
    return out, 1


def project(o, v):
    o = np.asarray(o, np.int64).reshape(-1, 3).astype(np.float64)
    return (o[:, 0] * v[0] + o[:, 1] * v[1]) + o[:, 2] * v[2]


def angle_bins(o, bas):
    """The angle bin of every row of ``o``: d = y / (x + |y|), bin = min(NB - 1, floor((d + 1) * NB / 2)); x <= 0: 0 or NB - 1 by the
    sign of y."""
    x, y = project(o, bas[0]), project(o, bas[1])
    ok = x > 0.0
    den = np.where(ok, x + np.abs(y), 1.0)
    d = y / den
    b = np.minimum(NB - 1, ((d + 1.0) * (NB / 2.0)).astype(np.int64))
    return np.where(ok, b, np.where(y < 0.0, 0, NB - 1))


def angle_histogram(o, bas):
    return np.bincount(angle_bins(o, bas), minlength=NB).astype(np.uint32)


def rank_bins(hist, permille):
    """(n, b_lo, b_hi): k = max(1, ceil(permille * n / 1000)); the first bins whose cumulative counts reach k and n - k + 1."""
    cum = np.cumsum(np.asarray(hist).astype(np.int64))
    n = int(cum[-1])
    k = max(1, (int(permille) * n + 999) // 1000)
    return n, int(np.searchsorted(cum, k, side="left")), int(np.searchsorted(cum, n - k + 1, side="left"))


def _direction(b, bas):
    d = float(2 * b + 1) / float(NB) - 1.0
    cx, cy = 1.0 - abs(d), d
    r = math.sqrt(cx * cx + cy * cy)
    cx, cy = cx / r, cy / r
    return [float(bas[0][c]) * cx + float(bas[1][c]) * cy for c in range(3)]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def vectors(hist, bas, basis_status, permille):
    """(HE float64[3, 2], P float64[2, 3], status): the stain vectors of the angle histogram and the pseudo-inverse of HE."""
    HE, P = np.zeros((3, 2), np.float64), np.zeros((2, 3), np.float64)
    if not basis_status:
        return HE, P, 0
    n, b_lo, b_hi = rank_bins(hist, permille)
    if n < 1:
        return HE, P, 0
    lo, hi = _direction(b_lo, bas), _direction(b_hi, bas)
    h, e = (lo, hi) if lo[0] > hi[0] else (hi, lo)
    a, b, d = _dot(h, h), _dot(h, e), _dot(e, e)
    det = a * d - b * b
    if not det > 0.0:
        return HE, P, 0
    for c in range(3):
        HE[c] = (h[c], e[c])
        P[0, c] = (d * h[c] - b * e[c]) / det
        P[1, c] = (a * e[c] - b * h[c]) / det
    return HE, P, 1


def concentration_bins(o, P):
    """int64[2, n]: bin = clamp(floor(C / 8), 0, NBC - 1) of C = P od (C in units of 2^-12, NBC / (8 * 2^12) = 1 / 8)."""
    out = []
    for s in range(2):
        t = project(o, P[s]) * 0.125
        out.append(np.where(t < 0.0, 0, np.where(t >= float(NBC), NBC - 1, np.minimum(t, float(NBC)).astype(np.int64))))
    return np.stack(out)


def concentration_histograms(o, P):
    b = concentration_bins(o, P)
    return np.stack([np.bincount(b[s], minlength=NBC) for s in range(2)]).astype(np.uint32)


def matrix(chist, P, vec_status, he_ref=HE_REF, maxc_ref=MAXC_REF):
    """(M float64[3, 3], maxC float64[2], status): maxC_s = the centre of the 99th-percentile bin (rank rule at 10 permille),
    M[c][j] = he_ref[c][0] * (g_0 * P[0][j]) + he_ref[c][1] * (g_1 * P[1][j]), g_s = maxc_ref[s] / maxC_s."""
    M, maxc = np.zeros((3, 3), np.float64), np.zeros(2, np.float64)
    if not vec_status:
        return M, maxc, 0
    g = []
    for s in range(2):
        n, _, b = rank_bins(chist[s], 10)
        if n < 1:
            return np.zeros((3, 3), np.float64), np.zeros(2, np.float64), 0
        maxc[s] = float(2 * b + 1) / 1024.0
        g.append(float(maxc_ref[s]) / float(maxc[s]))
    for c in range(3):
        for j in range(3):
            M[c, j] = float(he_ref[c][0]) * (g[0] * float(P[0, j])) + float(he_ref[c][1]) * (g[1] * float(P[1, j]))
    return M, maxc, 1


def apply(level, width, M, status):
    """The normalised copy of ``level``: per pixel od' = M od, q = clamp(rint(od'), 0, od[0]), out = inv[q]; columns at and behind
    ``width`` and everything when ``status`` is 0 are copied."""
    out = np.array(level, copy=True)
    if not status:
        return out
    o = pixel_od(level, width).astype(np.float64)
    for c in range(3):
        v = (M[c][0] * o[..., 0] + M[c][1] * o[..., 1]) + M[c][2] * o[..., 2]
        q = np.clip(np.rint(v), 0.0, float(OD_MAX)).astype(np.int64)
        out[:, :width, c] = INV[q]
    return out


def fit(level, width, alpha=1.0, beta=0.15, mask=None, f=None, he_ref=HE_REF, maxc_ref=MAXC_REF):
    """Every stage on one level: dict with moments, basis, basis_status, angle_hist, HE, P, vec_status, conc_hist, M, maxC, status."""
    o = tissue_od(level, width, beta_q(beta), mask, f)
    mom = moments(o)
    bas, bs = basis(mom)
    ah = angle_histogram(o, bas)
    HE, P, vs = vectors(ah, bas, bs, alpha_permille(alpha))
    ch = concentration_histograms(o, P)
    M, maxc, st = matrix(ch, P, vs, he_ref, maxc_ref)
    return {"moments": mom, "basis": bas, "basis_status": bs, "angle_hist": ah, "HE": HE, "P": P, "vec_status": vs, "conc_hist": ch,
            "M": M, "maxC": maxc, "status": st, "n": int(mom[0])}


def normalize(level, width, **kw):
    r = fit(level, width, **kw)
    return apply(level, width, r["M"], r["status"]), r


# ---- the textbook ------------------------------------------------------------------------------------------------------


def textbook_fit(img, alpha=1.0, beta=0.15):
    """Macenko et al. 2009 in float64 as it is usually written: OD = -ln((I + 1) / 256), np.cov, eigh, arctan2, np.percentile,
    lstsq.  img: uint8[H, W, 3].  Returns (HE float64[3, 2], maxC float64[2], C float64[2, H * W])."""
    od = -np.log((np.asarray(img).reshape(-1, 3).astype(np.float64) + 1.0) / 256.0)
    odhat = od[~np.any(od < beta, axis=1)]
    _, eigvecs = np.linalg.eigh(np.cov(odhat.T))
    that = odhat @ eigvecs[:, 1:3]
    phi = np.arctan2(that[:, 1], that[:, 0])
    vmin = eigvecs[:, 1:3] @ np.array([np.cos(np.percentile(phi, alpha)), np.sin(np.percentile(phi, alpha))])
    vmax = eigvecs[:, 1:3] @ np.array([np.cos(np.percentile(phi, 100 - alpha)), np.sin(np.percentile(phi, 100 - alpha))])
    # the sign of an eigenvector is arbitrary: make both stain vectors point into the positive octant
    vmin, vmax = (v if v.sum() >= 0 else -v for v in (vmin, vmax))
    HE = np.array((vmin, vmax)).T if vmin[0] > vmax[0] else np.array((vmax, vmin)).T
    C = np.linalg.lstsq(HE, od.T, rcond=None)[0]
    Chat = np.linalg.lstsq(HE, odhat.T, rcond=None)[0]
    return HE, np.array([np.percentile(Chat[0], 99), np.percentile(Chat[1], 99)]), C


def textbook_normalize(img, alpha=1.0, beta=0.15, he_ref=HE_REF, maxc_ref=MAXC_REF):
    """(normalised uint8 image, HE, maxC).  Pixel value v stands for the intensity v + 1 of 256, as in the OD above."""
    HE, maxc, C = textbook_fit(img, alpha, beta)
    C2 = C * (np.asarray(maxc_ref) / maxc)[:, None]
    inorm = 256.0 * np.exp(-(np.asarray(he_ref) @ C2)) - 1.0
    out = np.clip(np.rint(inorm), 0, 255).astype(np.uint8).T.reshape(np.asarray(img).shape)
    return out, HE, maxc

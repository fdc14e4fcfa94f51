"""numpy restatement of the Otsu tissue mask (include/hipac_tissue.h), one function per stage.  Not a test:
tests/test_tissue_host.py checks it against scipy and exact rational arithmetic, tests/test_gpu_tissue.py compares the device
with it bit for bit.  Integers throughout; the Otsu score is the one float64 place, one rounding per operation."""
from fractions import Fraction

import numpy as np

CELL, WINDOW = 32, 1792


def mask_size(width, height, f):
    return -(-width // f), -(-height // f)


def thumbnail(level, width, f):
    """uint8[mh, mw, 3]: the per-channel mean of every f x f box of ``level`` uint8[H, Wpad >= width, 3], clipped to ``width`` x H,
    rounded half up.  Columns at and behind ``width`` are never read."""
    img = np.asarray(level)[:, :width].astype(np.int64)
    H = img.shape[0]
    mw, mh = mask_size(width, H, f)
    pad = np.zeros((mh * f, mw * f, 3), np.int64)
    pad[:H, :width] = img
    s = pad.reshape(mh, f, mw, f, 3).sum(axis=(1, 3))
    nx = np.minimum(f, width - np.arange(mw) * f)
    ny = np.minimum(f, H - np.arange(mh) * f)
    n = (ny[:, None] * nx[None, :])[:, :, None]
    return ((2 * s + n) // (2 * n)).astype(np.uint8)


def saturation(thumb):
    """uint8[mh, mw]: 0 where the largest channel is 0, else (2 * 255 * (mx - mn) + mx) // (2 * mx)."""
    t = np.asarray(thumb).astype(np.int64)
    mx, mn = t.max(axis=2), t.min(axis=2)
    safe = np.maximum(mx, 1)
    return np.where(mx == 0, 0, (2 * 255 * (mx - mn) + mx) // (2 * safe)).astype(np.uint8)


def histogram(sat):
    return np.bincount(np.asarray(sat, np.uint8).ravel(), minlength=256).astype(np.uint32)


def otsu_scores(hist):
    """(candidate bool[255], v float64[255]) for t = 0 .. 254: v = (d * d) / float64(w0 * (N - w0)), d = float64(M * w0 - N * m0)."""
    h = np.asarray(hist).astype(np.int64)
    w0 = np.cumsum(h)[:255]
    m0 = np.cumsum(h * np.arange(256, dtype=np.int64))[:255]
    N, M = int(h.sum()), int((h * np.arange(256, dtype=np.int64)).sum())
    cand = (w0 > 0) & (w0 < N)
    d = (M * w0 - N * m0).astype(np.float64)
    den = np.where(cand, w0 * (N - w0), 1).astype(np.float64)
    dd = d * d
    return cand, dd / den


def otsu(hist):
    """The candidate with the largest score, ties to the lowest t; 255 without a candidate."""
    cand, v = otsu_scores(hist)
    if not cand.any():
        return 255
    return int(np.argmax(np.where(cand, v, -1.0)))  # argmax returns the first of equal values


def otsu_exact(hist):
    """The same arg-max in exact rational arithmetic, and whether the largest score is reached by one t only."""
    h = [int(x) for x in np.asarray(hist)]
    N, M = sum(h), sum(i * x for i, x in enumerate(h))
    best, best_t, unique = None, 255, True
    w0 = m0 = 0
    for t in range(255):
        w0 += h[t]
        m0 += t * h[t]
        if not 0 < w0 < N:
            continue
        v = Fraction((M * w0 - N * m0) ** 2, w0 * (N - w0))
        if best is None or v > best:
            best, best_t, unique = v, t, True
        elif v == best:
            unique = False
    return best_t, unique


def thresholds(hist, floor=16):
    t = otsu(hist)
    return t, max(t, int(floor))


def raw_mask(sat, t_eff):
    return (np.asarray(sat).astype(np.int64) > int(t_eff)).astype(np.uint8)


def _square(mask, radius, op, outside):
    m = np.asarray(mask).astype(np.uint8)
    mh, mw = m.shape
    p = np.full((mh + 2 * radius, mw + 2 * radius), outside, np.uint8)
    p[radius:radius + mh, radius:radius + mw] = m
    out = p[radius:radius + mh, radius:radius + mw].copy()
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            out = op(out, p[dy:dy + mh, dx:dx + mw])
    return out


def erode(mask, radius=1):
    """Erosion with a (2 radius + 1)^2 square; everything outside the mask is background."""
    return _square(mask, radius, np.minimum, 0)


def dilate(mask, radius=1):
    return _square(mask, radius, np.maximum, 0)


def clean(raw, dilate_radius=1, opening=True):
    m = np.asarray(raw).astype(np.uint8)
    if opening:
        m = dilate(erode(m, 1), 1)
    return dilate(m, int(dilate_radius))


def integral(mask):
    m = np.asarray(mask).astype(np.int64)
    t = np.zeros((m.shape[0] + 1, m.shape[1] + 1), np.int64)
    for j in range(m.shape[0]):
        run = 0
        for i in range(m.shape[1]):
            run += m[j, i]
            t[j + 1, i + 1] = t[j, i + 1] + run
    return t.astype(np.int32)


def integral_fast(mask):
    """The same table by two cumulative sums (test_tissue_host.py checks the loop above against it)."""
    m = np.asarray(mask).astype(np.int64)
    t = np.zeros((m.shape[0] + 1, m.shape[1] + 1), np.int32)
    t[1:, 1:] = m.cumsum(0).cumsum(1)
    return t


def window_rect(x, y, level):
    """(x0, x1, y0, y1): the mask rectangle [x0, x1) x [y0, y1) of a window of ``level`` at (x, y), unclipped."""
    X, Y = int(x) * (1 << level), int(y) * (1 << level)
    return X >> 5, (X + WINDOW + CELL - 1) >> 5, Y >> 5, (Y + WINDOW + CELL - 1) >> 5


def window_keep(table, xy, level, min_permille):
    """(keep uint8[n], count int32[n])."""
    table = np.asarray(table).astype(np.int64)
    mh, mw = table.shape[0] - 1, table.shape[1] - 1
    xy = np.asarray(xy).astype(np.int64).reshape(-1, 2)
    X, Y = xy[:, 0] * (1 << level), xy[:, 1] * (1 << level)
    x0, x1, y0, y1 = X >> 5, (X + WINDOW + CELL - 1) >> 5, Y >> 5, (Y + WINDOW + CELL - 1) >> 5
    n_rect = (x1 - x0) * (y1 - y0)
    cx0, cx1, cy0, cy1 = np.clip(x0, 0, mw), np.clip(x1, 0, mw), np.clip(y0, 0, mh), np.clip(y1, 0, mh)
    c = table[cy1, cx1] - table[cy0, cx1] - table[cy1, cx0] + table[cy0, cx0]
    keep = (c >= 1) & (1000 * c >= int(min_permille) * n_rect)
    return keep.astype(np.uint8), c.astype(np.int32)


def tissue_mask(level, width, f, floor=16, dilate_radius=1, opening=True):
    """Every stage of one slide: dict with thumb, sat, hist, thresholds (t, t_eff), mask, table."""
    thumb = thumbnail(level, width, f)
    sat = saturation(thumb)
    hist = histogram(sat)
    t, te = thresholds(hist, floor)
    mask = clean(raw_mask(sat, te), dilate_radius, opening)
    return {"thumb": thumb, "sat": sat, "hist": hist, "thresholds": (t, te), "mask": mask, "table": integral_fast(mask)}

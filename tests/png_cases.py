"""Cases shared by the CPU and GPU tests of the PNG patch encoder (include/hipac_png.h): one small mosaic level image and the
windows cut from it.  ``CALLS`` maps a window side P to the windows of one call; ``level()`` is built once and never changed."""
import functools

import numpy as np

W, H = 701, 523  # odd on purpose; the GPU tests give it a pitch above 3 W
TISSUE, NOISE, RUNS, WHITE, GEO = (0, 0), (300, 0), (600, 0), (0, 300), (300, 300)  # top-left corners of the regions


def smooth_tissue(h, w, seed, white_share=0.0):
    """A smooth H&E-like image: low-frequency colour fields, fine grain, and a white border region of the given share."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.zeros((h, w))
    for _ in range(6):
        kx, ky, ph = rng.uniform(-0.06, 0.06), rng.uniform(-0.06, 0.06), rng.uniform(0, 6.28)
        f += np.sin(kx * xx + ky * yy + ph)
    f = (f - f.min()) / (f.max() - f.min())
    base = np.stack([205 - 70 * f, 150 - 90 * f, 200 - 50 * f], -1)
    img = np.clip(base + rng.normal(0, 2.0, (h, w, 3)), 0, 255).round().astype(np.uint8)
    if white_share > 0:
        edge = xx + 0.3 * yy + 12 * np.sin(yy / 17.0)
        img[edge > np.quantile(edge, 1 - white_share)] = 255
    return img


def tissue_region(n, seed):
    """smooth_tissue with strips that favour each row filter: vertical stripes (Up), a copy shifted by one pixel and row
    (Paeth / Average), near-black ink with sparse specks (None); the smooth field itself takes Sub, Average and Paeth."""
    rng = np.random.default_rng(seed + 1)
    img = smooth_tissue(n, n, seed, white_share=0.25)
    cols = rng.integers(60, 230, (1, n, 3))
    img[40:52] = np.clip(cols + rng.integers(-1, 2, (12, n, 3)), 0, 255)
    img[90:100] = (rng.random((10, n, 3)) < 0.2).astype(np.uint8)
    ramp = (np.arange(n)[None, :, None] * 3 + np.arange(12)[:, None, None] * 5 + np.array([0, 40, 90])[None, None]) % 200
    img[140:152] = ramp
    return img


def runs_block():
    """86 x 86 (a row is 259 bytes): noise row N, N with its first j bytes raised by one (Up: a tail of 258 - j zeros), a zero
    row (None: 259 zeros) and a row of ones (Sub: ends the run).  The tails of 0, 1, 2, 3 zeros give runs of 259 .. 262 bytes
    across the filter byte: the remainders 0, 1, 2, 3 of the token rule, each behind one full-length match."""
    rng = np.random.default_rng(86)
    blk = rng.integers(0, 256, (86, 258), dtype=np.uint8)
    r = 1
    for tail in (0, 1, 2, 3, 0, 3):
        blk[r + 1] = blk[r]
        blk[r + 1, :258 - tail] += 1
        blk[r + 2] = 0
        blk[r + 3] = 1
        r += 5
    return blk.reshape(86, 86, 3)


def geometric_block(h, w):
    """Byte values 0, -1, 1, -2, 2, ... (18 of them, mod 256; the commonest nearest to zero, so that the row filter None keeps the
    distribution) whose counts grow by 1.7 per value: an unlimited Huffman tree over them is a chain deeper than 15.  The
    P = 86 window at (1, 1) of the block holds the counts exactly, and its commonest value never runs to four in a row."""
    signed = lambda j: j // 2 if j % 2 == 0 else 256 - (j + 1) // 2
    rng = np.random.default_rng(5)
    n = 86 * 86 * 3
    counts = [int(np.ceil(1.7 ** k)) for k in range(18)]
    counts[17] += n - sum(counts)
    rare = np.concatenate([np.full(c, signed(17 - k), np.uint8) for k, c in enumerate(counts[:17])])
    exact = np.zeros(n, np.uint8)
    free = np.flatnonzero(np.arange(n) % 3 != 0)  # the commonest value only here: runs of at most two
    top = rng.permutation(free)[:counts[17]]
    exact[top] = signed(0)
    rest = np.setdiff1d(np.arange(n), top)
    exact[rest] = rng.permutation(rare)
    reps = (h * w * 3 + n - 1) // n
    out = np.concatenate([rng.permutation(exact) for _ in range(reps)])[:h * w * 3].reshape(h, w, 3)
    out[1:87, 1:87] = exact.reshape(86, 86, 3)
    return out


@functools.lru_cache(maxsize=None)
def level():
    rng = np.random.default_rng(3)
    img = np.empty((H, W, 3), np.uint8)
    img[:] = ((np.arange(W)[None, :, None] // 3 + np.arange(H)[:, None, None] // 2) % 256).astype(np.uint8)
    img[0:300, 0:300] = tissue_region(300, 11)
    img[0:300, 300:600] = rng.integers(0, 256, (300, 300, 3), dtype=np.uint8)
    img[0:86, 600:686] = runs_block()
    img[300:, 0:300] = 255
    img[300:, 300:560] = geometric_block(H - 300, 260)
    img.setflags(write=False)
    return img


# name -> (x, y); the windows of every call.  P = 86: every kind in one call
CALLS = {
    1: {"inside": (5, 5), "white": (10, 400), "outside": (W, 3), "corner": (W - 1, H - 1)},
    5: {"tissue": (33, 21), "noise": (401, 77), "right": (W - 2, 100), "below": (100, H - 3), "outside": (-5, -5), "white": (7, 333)},
    86: {"tissue_odd_x": (17, 23), "noise": (333, 41), "runs": (600, 0), "white": (101, 380), "geometric": (301, 301),
         "right": (650, 11), "below": (51, 480), "outside": (5000, 5000), "above_left": (-40, -31), "far_left": (-86, 0)},
    224: {"tissue": (1, 3), "noise": (303, 9), "white": (3, 299), "geometric": (305, 299), "right_below": (601, 401),
          "outside": (-224, 40)},
}

ALL_WINDOWS = [(P, name) for P, wins in CALLS.items() for name in wins]


def size_cases():
    """(name, uint8[P, P, 3]) of the size check: smooth P = 224 and P = 448 windows with and without a white border."""
    return [("224_w0", smooth_tissue(224, 224, 21)), ("224_w40", smooth_tissue(224, 224, 22, 0.4)),
            ("448_w0", smooth_tissue(448, 448, 23)), ("448_w20", smooth_tissue(448, 448, 24, 0.2))]

"""Evaluation-mask inputs shared by tests/test_froc_reference.py (CPU) and tests/test_gpu_froc_topology.py: topologies
that make the union-finds of csrc/froc.hip walk long chains, number many roots or meet the numbering scan's chunk
boundaries, at thresholds where fine structure survives (K = 1: binary == (mask == 255)).  No GPU import here.

Every case is (name, mask uint8[H, W], resolution, level); `res_for_threshold` sets the distance threshold directly, as
in tests/golden/make_golden_froc.py.  The structural property each case is built for is asserted in
tests/test_froc_reference.py, so a generator that drifts cannot quietly stop testing it."""
import math

import numpy as np

LEVEL = 5
CHUNK = 1024  # pixels per block of the numbering scan (kEvalChunk in csrc/froc.hip)


def eval_threshold(resolution, level=LEVEL):
    return 75 / (resolution * pow(2, level) * 2)


def res_for_threshold(t, level=LEVEL):
    """The resolution whose evaluation threshold at `level` is t, or the least double above t where the division does
    not round-trip (exact for 0.5, 1.0 and 5.0)."""
    res = 75 / (t * pow(2, level) * 2)
    while eval_threshold(res, level) < t:
        res = math.nextafter(res, 0.0)
    return res


def blob_mask(H, W, seed, n=60):
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), np.uint8)
    for _ in range(n):
        r, c = int(rng.integers(0, H)), int(rng.integers(0, W))
        a, b = int(rng.integers(2, max(3, H // 12))), int(rng.integers(2, max(3, W // 12)))
        r0, r1, c0, c1 = max(0, r - a), min(H, r + a + 1), max(0, c - b), min(W, c + b + 1)
        rr, cc = np.ogrid[r0:r1, c0:c1]
        e = ((rr - r) / a) ** 2 + ((cc - c) / b) ** 2
        sub = m[r0:r1, c0:c1]
        sub[e <= 1] = 255
        if rng.random() < 0.4:
            sub[e <= 0.3] = 0  # a hole
    m[rng.random((H, W)) < 2e-4] = 255
    return m


def random_draws():
    """The ten small draws of test_gpu_froc.py::test_random_masks_match_live_scipy: (mask, resolution, level)."""
    rng = np.random.default_rng(1)
    out = []
    for i in range(10):
        H, W = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        level = int(rng.integers(0, 8))
        out.append((blob_mask(H, W, 100 + i, n=int(rng.integers(0, 30))), 0.243, level))
    return out


def exact_moments(labels, n=None):
    """int64[n, 6] = (count, sum r, sum c, sum r^2, sum c^2, sum r c) of labels 1..n (n = the largest label unless
    given); values outside 1..n are ignored."""
    labels = np.asarray(labels)
    n = int(labels.max(initial=0)) if n is None else n
    r, c = (v.astype(np.int64) for v in np.nonzero((labels >= 1) & (labels <= n)))
    lab = labels[r, c].astype(np.int64) - 1
    out = np.zeros((n, 6), np.int64)
    for k, v in enumerate((np.ones_like(r), r, c, r * r, c * c, r * c)):
        np.add.at(out[:, k], lab, v)
    return out


# ---- chain-like cases ------------------------------------------------------------------------------------------------

def spiral_arm(H=67, W=71, margin=3, pitch=2):
    """A one-pixel arm winding inwards from (margin, margin); the corridor between its turns is one pixel wide and opens
    to the margin under the arm's first pixel."""
    m = np.zeros((H, W), np.uint8)
    lo_r, hi_r, lo_c, hi_c = margin, H - 1 - margin, margin, W - 1 - margin
    r, c, d = margin, margin, 0
    m[r, c] = 255
    while True:
        if d == 0 and hi_c > c:
            m[r, c:hi_c + 1] = 255
            c, lo_r = hi_c, lo_r + pitch
        elif d == 1 and hi_r > r:
            m[r:hi_r + 1, c] = 255
            r, hi_c = hi_r, hi_c - pitch
        elif d == 2 and lo_c < c:
            m[r, lo_c:c + 1] = 255
            c, hi_r = lo_c, hi_r - pitch
        elif d == 3 and lo_r < r:
            m[lo_r:r + 1, c] = 255
            r, lo_c = lo_r, lo_c + pitch
        else:
            return m
        d = (d + 1) % 4


def rings(gaps, S=63, count=10, step=3):
    """`count` concentric one-pixel square rings `step` apart, the outermost one pixel in from the border; with `gaps`
    each ring misses one pixel, in its top side for even rings and in its bottom side for odd ones."""
    m = np.zeros((S, S), np.uint8)
    mid = S // 2
    for i in range(count):
        lo, hi = 1 + step * i, S - 2 - step * i
        assert lo < mid < hi
        m[lo, lo:hi + 1] = m[hi, lo:hi + 1] = 255
        m[lo:hi + 1, lo] = m[lo:hi + 1, hi] = 255
        if gaps:
            m[lo if i % 2 == 0 else hi, mid] = 0
    return m


def two_combs(H=61, W=63, gap=31):
    """Two interleaved combs: the first is the frame (its rail the left column, teeth pointing right), open in one pixel
    of the top border; the second hangs inside it from a rail near the right side, teeth pointing left.  The background
    between the teeth is a one-pixel serpentine whose only way out is the opening."""
    m = np.zeros((H, W), np.uint8)
    m[:, 0] = m[:, W - 1] = m[0, :] = m[H - 1, :] = 255
    m[0, gap] = 0
    for r in range(4, H - 3, 4):
        m[r, 0:W - 4] = 255  # the first comb's teeth end one pixel short of the second's rail
    rows = list(range(2, H - 2, 4))
    for r in rows:
        m[r, 2:W - 2] = 255  # the second comb's teeth end one pixel short of the first's rail
    m[rows[0]:rows[-1] + 1, W - 3] = 255
    return m


def lines(H=60, W=100):
    m = np.zeros((H, W), np.uint8)
    m[::2, :] = 255
    return m


def checker(H=33, W=35):
    rr, cc = np.mgrid[:H, :W]
    return np.where((rr + cc) % 2 == 0, 255, 0).astype(np.uint8)


def diagonals(S=33):
    m = np.zeros((S, S), np.uint8)
    i = np.arange(S)
    m[i, i] = m[i, S - 1 - i] = 255
    return m


def raster_order(H=30, W=60):
    """Five components whose first raster pixels come in another order than their bounding boxes: the U's is the tip of
    its right arm in row 0."""
    m = np.zeros((H, W), np.uint8)
    m[2:21, 35] = 255  # the U: left arm from row 2, bottom, right arm from row 0
    m[20, 35:51] = 255
    m[0:21, 50] = 255
    m[1:6, 0:4] = 255  # a blob starting at row 1, far left
    m[4:9, 40:45] = 255  # a blob inside the U
    m[H - 1, 0] = 255
    m[H - 1, W - 1] = 255  # pixel N - 1
    return m


def corner_square(sealed, H=40, W=50, S=9):
    """A hollow square in the image's corner.  Not sealed: one pixel of its wall on the top border is missing, the
    cavity's only way out.  Sealed: no gap, and one foreground pixel inside the cavity."""
    m = np.zeros((H, W), np.uint8)
    m[0:S, 0:S] = 255
    m[1:S - 1, 1:S - 1] = 0
    if sealed:
        m[S // 2, S // 2] = 255
    else:
        m[0, S // 2] = 0
    return m


NEAR_255_SEEDS = ((0, 0), (5, 17), (20, 3), (20, 30), (36, 40))


def near_255(H=37, W=41):
    rng = np.random.default_rng(255)
    m = np.where(rng.random((H, W)) < 0.5, 254, 1).astype(np.uint8)
    for r, c in NEAR_255_SEEDS:
        m[r, c] = 255
    return m


PYTHAGORAS_SEEDS = ((12, 12), (28, 30), (0, 44), (39, 0))


def pythagoras(H=40, W=45):
    m = np.zeros((H, W), np.uint8)
    for r, c in PYTHAGORAS_SEEDS:
        m[r, c] = 255
    return m


def lattice(H, W, r0=0, c0=0):
    m = np.zeros((H, W), np.uint8)
    m[r0::2, c0::2] = 255
    return m


# roots_on_chunks: 40 x 1025 lattices whose first rows put a root on the last pixel of the numbering scan's first chunk,
# on the first pixel of its second chunk, and on that chunk's second pixel: name suffix -> (row offset, column offset)
CHUNK_ROOTS = {1023: (0, 1), 1024: (0, 0), 1025: (1, 0)}


def cases():
    """[(name, mask, resolution, level)]; the name ends in '@T'."""
    both = [("spiral_arm", spiral_arm()), ("open_rings", rings(True)), ("closed_rings", rings(False)),
            ("two_combs", two_combs()), ("lines", lines()), ("checker", checker()), ("diagonals", diagonals()),
            ("raster_order", raster_order()), ("border_leak", corner_square(False)),
            ("sealed_with_island", corner_square(True)), ("near_255", near_255()), ("root_at_zero", lattice(35, 37))]
    both += [(f"roots_on_chunks_{p}", lattice(40, CHUNK + 1, r0, c0)) for p, (r0, c0) in CHUNK_ROOTS.items()]
    out = [(f"{name}@{t}", m, res_for_threshold(t), LEVEL) for name, m in both for t in (0.5, 1.0)]
    out.append(("open_rings@1.3", rings(True), res_for_threshold(1.3), LEVEL))
    out.append(("pythagoras@5.0", pythagoras(), res_for_threshold(5.0), LEVEL))
    out.append(("pythagoras_next@5.0+", pythagoras(), res_for_threshold(math.nextafter(5.0, 6.0)), LEVEL))
    return out


# ---- closed-form large cases -----------------------------------------------------------------------------------------

LARGE_LATTICES = ((1024, 1024), (1025, 1024))  # (H, W): 1024 numbering chunks (one per scan thread) and 1025 (two)


def lattice_expected(H, W):
    """Labels and moments of `lattice(H, W)` at a threshold of at most 1, written down directly: every seed is its own
    component, (2i, 2j) has label i * ceil(W / 2) + j + 1 and the moments (1, r, c, r^2, c^2, r c)."""
    per_row = (W + 1) // 2
    labels = np.zeros((H, W), np.int32)
    i, j = np.mgrid[:(H + 1) // 2, :per_row]
    labels[::2, ::2] = i * per_row + j + 1
    r, c = (2 * i).ravel().astype(np.int64), (2 * j).ravel().astype(np.int64)
    return labels, np.stack([np.ones_like(r), r, c, r * r, c * c, r * c], axis=1)

"""numpy restatement of the HED stain augmentation (include/hipac_augment_hed.h): the map builder, the per-pixel rule, and the
textbook float64 formula the rule is measured against.  Not a test: tests/test_augment_hed_host.py compares the package's host
code with it, tests/test_gpu_augment_hed.py the device, bit for bit.  Written from the header, not from augment_hed.py: Python
floats one operation at a time for the map, plain table look-ups for the pixels.

    od' = od Rinv diag(alpha) R + beta R        (row vectors; R = rows H, E, D)
"""
import numpy as np

from stain_cpu import INV, OD, OD_MAX

R = ((0.65, 0.70, 0.29), (0.07, 0.99, 0.11), (0.27, 0.57, 0.78))
RINV = ((1.8779827368521353, -1.0076786862855645, -0.5561158181996246),
        (-0.06590806222356332, 1.1347303724996625, -0.1355217986283712),
        (-0.6019073634392891, -0.4804141884970579, 1.5735880719641926))
STREAM_KEY = 11
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def rng(seed, rank=0):
    return np.random.default_rng([seed, rank, STREAM_KEY])


def draws(n, sigma, gen):
    """[(alpha[3], beta[3])] of n views: per view three U(1 - sigma, 1 + sigma), then three U(-sigma, sigma), one call each."""
    out = []
    for _ in range(n):
        alpha = [float(gen.uniform(1.0 - sigma, 1.0 + sigma)) for _ in range(3)]
        beta = [float(gen.uniform(-sigma, sigma)) for _ in range(3)]
        out.append((alpha, beta))
    return out


def payload(alpha, beta):
    """One view's double[12] = A row-major, then bq, as a list of Python floats (one rounding per operation)."""
    T = [[RINV[i][j] * alpha[j] for j in range(3)] for i in range(3)]
    A = [[(T[k][0] * R[0][c] + T[k][1] * R[1][c]) + T[k][2] * R[2][c] for k in range(3)] for c in range(3)]
    bq = [4096.0 * ((beta[0] * R[0][c] + beta[1] * R[1][c]) + beta[2] * R[2][c]) for c in range(3)]
    return [A[c][k] for c in range(3) for k in range(3)] + bq


def maps(n, sigma, gen):
    """float64 [n, 12]."""
    return np.array([payload(a, b) for a, b in draws(n, sigma, gen)], np.float64).reshape(n, 12)


def apply_one(image, m):
    """uint8 [..., 3] under one payload m[12]; also returns the unclamped t (float64 [..., 3]) for the clamp assertions."""
    o = OD[np.asarray(image)].astype(np.float64)
    out = np.empty_like(np.asarray(image))
    raw = np.empty(o.shape, np.float64)
    for c in range(3):
        t = np.rint(((float(m[3 * c]) * o[..., 0] + float(m[3 * c + 1]) * o[..., 1]) + float(m[3 * c + 2]) * o[..., 2]) + float(m[9 + c]))
        raw[..., c] = t
        out[..., c] = INV[np.clip(t, 0.0, float(OD_MAX)).astype(np.int64)]
    return out, raw


def apply(images, ms):
    """uint8 [n, ..., 3] under float64 [n, 12]."""
    return np.stack([apply_one(im, m)[0] for im, m in zip(images, ms)])


def textbook(image, m):
    """The float64 formula: od = ln(256 / (v + 1)), od' = od A^T + b, v' = clip(rint(256 exp(-od') - 1), 0, 255)."""
    od = np.log(256.0 / (np.asarray(image).astype(np.float64) + 1.0))
    A = np.asarray(m[:9], np.float64).reshape(3, 3)
    b = np.asarray(m[9:], np.float64) / 4096.0
    return np.clip(np.rint(256.0 * np.exp(-(od @ A.T + b)) - 1.0), 0, 255).astype(np.uint8)


# ---- the cases of the distance to the textbook (tests/tools/measure_augment_hed.py records, tests/test_augment_hed_host.py gates) ----

SIGMAS = (0.05, 0.2, 0.5)
N_MAPS = 64
N_COLOURS = 4096


def random_colours(seed=1):
    return np.random.default_rng(seed).integers(0, 256, (N_COLOURS, 3), dtype=np.uint8)


def he_colours(seed=2):
    """Colours of pixels that hold haematoxylin and eosin only: concentrations U(0, 1.5) each."""
    c = np.random.default_rng(seed).uniform(0.0, 1.5, (N_COLOURS, 2))
    od = c[:, :1] * np.array(R[0]) + c[:, 1:] * np.array(R[1])
    return np.clip(np.rint(256.0 * np.exp(-od) - 1.0), 0, 255).astype(np.uint8)


def distances():
    """{sigma: {"max_level_diff", "share_differing"}} of the restatement against the textbook over both colour sets, N_MAPS maps
    per sigma from rng(5)."""
    out = {}
    for sigma in SIGMAS:
        ms = maps(N_MAPS, sigma, rng(5))
        worst, differ, total = 0, 0, 0
        for colours in (random_colours(), he_colours()):
            for m in ms:
                d = np.abs(apply_one(colours, m)[0].astype(np.int64) - textbook(colours, m).astype(np.int64))
                worst, differ, total = max(worst, int(d.max())), differ + int((d != 0).sum()), total + d.size
        out[str(sigma)] = {"max_level_diff": worst, "share_differing": differ / total}
    return out

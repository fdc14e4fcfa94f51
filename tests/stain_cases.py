"""Inputs shared by tests/test_stain_host.py, tests/test_gpu_stain.py and tests/tools/measure_stain.py (not a test)."""
import numpy as np

# unit stain vectors of the seeded two-stain images (columns: haematoxylin, eosin)
TRUE_HE = np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11]]).T
TRUE_HE = TRUE_HE / np.linalg.norm(TRUE_HE, axis=0)
SEEDS = (1, 2, 3)                # the images the distances are recorded on
CHECK_SEEDS = (11, 12, 13)       # other seeds of the same recipe: the host test runs on these
SHAPE = (400, 500)               # 200 000 pixels


def two_stain_image(seed, shape=SHAPE, white=0.3):
    """uint8[H, W, 3]: gamma-distributed concentrations of the two stains TRUE_HE, Gaussian pixel noise, a ``white`` share of
    near-white background pixels."""
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    c = np.stack([rng.gamma(2.0, 0.35, n), rng.gamma(2.0, 0.25, n)])
    img = 256.0 * np.exp(-(TRUE_HE @ c)) - 1.0 + rng.normal(0.0, 1.5, (3, n))
    img[:, rng.random(n) < white] = rng.integers(235, 256, (3, 1))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8).T.reshape(shape[0], shape[1], 3).copy()


def angles_deg(a, b):
    """Angle in degrees between the matching columns of two 3 x 2 matrices."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    cos = np.abs((a * b).sum(0)) / (np.linalg.norm(a, axis=0) * np.linalg.norm(b, axis=0))
    return np.degrees(np.arccos(np.clip(cos, 0.0, 1.0)))


def distances(img, alpha=1.0, beta=0.15):
    """The four distances between the restatement and the textbook on one image, plus both angles to the known vectors."""
    import stain_cpu

    out, r = stain_cpu.normalize(img, img.shape[1], alpha=alpha, beta=beta)
    want, he, maxc = stain_cpu.textbook_normalize(img, alpha, beta)
    diff = np.abs(out.astype(np.int64) - want.astype(np.int64)).max(axis=2)
    return {"status": int(r["status"]), "angle_deg": float(angles_deg(r["HE"], he).max()), "dmaxc": float(np.abs(r["maxC"] - maxc).max()),
            "max_pixel_diff": int(diff.max()), "share_differing": float((diff > 0).mean()),
            "angle_to_truth_deg": angles_deg(r["HE"], TRUE_HE).tolist(), "textbook_angle_to_truth_deg": angles_deg(he, TRUE_HE).tolist(),
            "angle_vs_textbook_deg": angles_deg(r["HE"], he).tolist()}


def degenerate_images():
    """[(name, uint8[H, W, 3])]: inputs on which no two stains can be found (status 0, pixels unchanged)."""
    white = np.full((12, 20, 3), 255, np.uint8)
    constant = np.full((12, 20, 3), (90, 60, 120), np.uint8)
    single = white.copy()
    single[5, 7] = (90, 60, 120)
    # one stain: the optical density of the red channel varies, the other two are constant -- the covariance has rank one exactly
    one = np.full((12, 20, 3), (0, 100, 140), np.uint8)
    one[..., 0] = (np.arange(240).reshape(12, 20) * 37) % 200
    return [("all white", white), ("constant", constant), ("single tissue pixel", single), ("one stain", one)]


def padded(img, rng=None, fill=None):
    """uint8[H, ceil16(W), 3] with the row padding filled with non-zero bytes (dark ones: they would count as tissue if read)."""
    h, w, _ = img.shape
    wp = (w + 15) // 16 * 16
    a = np.empty((h, wp, 3), np.uint8)
    a[:, :w] = img
    if wp > w:
        a[:, w:] = rng.integers(1, 200, (h, wp - w, 3)) if rng is not None else (fill if fill is not None else 77)
    return a


def stained_level(w, h, seed):
    """A padded two-stain level of any size (with a white share), for the device tests."""
    return padded(two_stain_image(seed, (h, w)), np.random.default_rng(seed + 1000))


def random_mask(w, h, f, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((-(-h // f), -(-w // f))) < 0.6).astype(np.uint8)

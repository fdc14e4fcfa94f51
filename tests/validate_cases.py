"""Seeded inputs of the --validate tests (tests/test_gpu_validate.py, tests/test_validate_host.py,
tests/tools/measure_validate_fp32.py): two overlapping Gaussian clusters plus two injected high-variance directions.

A row is  1 + 0.5 g + 1.5 (y - 0.5) u0 + 4 t1 v1 + 2.5 t2 v2  with g ~ N(0, I), t1, t2 ~ N(0, 1), y ~ Bernoulli(0.4) and
u0, v1, v2 orthonormal.  The covariance therefore has the eigenvalues 16.25 (v1), 6.5 (v2), 0.25 + 2.25 * 0.24 = 0.79 (u0)
and 0.25 for the rest: where n is well above F the leading three sample eigenvalues differ pairwise by far more than the
factor 1.5 that ``assert_separated`` asks for, so the two leading components are well defined.  The clusters are 1.5 apart
at a noise of 0.5, three standard deviations: a linear probe cannot reach accuracy 1 (Bayes error 6.7 %).
"""
import numpy as np

# (n, F) of the kernel tests.  Gram slices (128-row granules, see hipac_validate_gram_slices): (1031, 512) spans 9 slices with
# a ragged last one of 7 rows; (300, 2048) spans 3 slices with a ragged last one of 44 rows; the others are one slice.
SHAPES = [(1, 4), (63, 36), (64, 64), (65, 100), (1031, 512), (300, 2048)]
E2E = [(777, 128, 11), (4001, 512, 17)]  # (n, F, seed) of the end-to-end cases
SPLIT_SEED = 5


def make_features(n, F, seed):
    """-> (features float32 [n, F], labels int64 [n]); for n >= 4 both classes have at least two rows."""
    rng = np.random.Generator(np.random.PCG64([seed, n, F]))
    y = (rng.random(n) < 0.4).astype(np.int64)
    if n >= 4:
        y[:2], y[2:4] = 0, 1
    q, _ = np.linalg.qr(rng.standard_normal((F, 3)))
    u0, v1, v2 = q[:, 0], q[:, 1], q[:, 2]
    x = 1.0 + 0.5 * rng.standard_normal((n, F))
    x += 1.5 * (y - 0.5)[:, None] * u0
    x += 4.0 * rng.standard_normal(n)[:, None] * v1 + 2.5 * rng.standard_normal(n)[:, None] * v2
    return np.ascontiguousarray(x, dtype=np.float32), y


def make_rows(n, seed):
    """A permuted subset with repeats: n draws from 0..n-1 with replacement, unsorted (int32)."""
    rng = np.random.Generator(np.random.PCG64([seed, n, 1]))
    return rng.integers(0, n, size=n).astype(np.int32)


def make_weights(n, seed):
    """Random weights in [0, 2) with exact zeros at every fifth position (float32)."""
    rng = np.random.Generator(np.random.PCG64([seed, n, 2]))
    w = (2.0 * rng.random(n)).astype(np.float32)
    w[3::5] = 0.0
    return w


def make_coef(F, seed, scale=1.0):
    """(coef float32 [F], intercept float32 [1]) whose margins on ``make_features`` rows have a spread of about 2 * scale."""
    rng = np.random.Generator(np.random.PCG64([seed, F, 3]))
    w = rng.standard_normal(F)
    w *= scale / (np.linalg.norm(w) * 0.5)  # x has a noise of 0.5 per column; the injected directions add to it
    return w.astype(np.float32), np.array([0.25 * scale], np.float32)


CLASS_W = np.array([0.7, 1.9], np.float32)


def mean32(x, rows=None):
    """The centre the tests hand to every implementation alike: the float32 rounding of the float64 mean.
    For the single row of (1, 4) the centre IS the row, so x - c is exactly 0 in every precision: the Gram matrix about the mean,
    Z and the class sums of that shape are exactly 0, their recorded float32 distance is 0 and their gate is 0.  That holds
    only while the shape has one row and the centre is formed this way; change either and those gates become ordinary ones."""
    xr = x if rows is None else x[rows]
    return xr.astype(np.float64).mean(axis=0).astype(np.float32)


def rel(a, b):
    """max|a - b| / max|b|; 0 when both are zero everywhere, inf when only b is."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    num, den = float(np.max(np.abs(a - b))) if a.size else 0.0, float(np.max(np.abs(b))) if b.size else 0.0
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return num / den


def leading_eigenvalues(x, k=4):
    xc = x.astype(np.float64) - x.astype(np.float64).mean(axis=0)
    return np.linalg.eigvalsh(xc.T @ xc / max(x.shape[0] - 1, 1))[::-1][:k]


def assert_separated(x, factor=1.5):
    """The first three eigenvalues of the float64 covariance differ pairwise by at least ``factor``: without that the two
    leading components are not well defined and comparing them means nothing."""
    ev = leading_eigenvalues(x, 3)
    assert ev[0] >= factor * ev[1] and ev[1] >= factor * ev[2] and ev[2] > 0, ev
    return ev


# ---- the cases of the kernel tests, shared by the GPU tests and tests/tools/measure_validate_fp32.py -------------------


def group_key(F):
    return str(F)


def gram_cases():
    """(case id, n, F, rows?, weights?, centre?) -- every shape crossed with the three switches."""
    return [(f"{n}x{F}-{'rows' if r else 'ident'}-{'w' if w else 'unw'}-{'mean' if c else 'origin'}", n, F, r, w, c)
            for n, F in SHAPES for r in (False, True) for w in (False, True) for c in (False, True)]


def gram_inputs(n, F, use_rows, use_w, use_c):
    """-> (x [n, F], labels [n], rows or None, w or None, c or None)."""
    x, y = make_features(n, F, 1)
    rows = make_rows(n, 2) if use_rows else None
    w = make_weights(n, 3) if use_w else None
    c = mean32(x, rows) if use_c else None
    return x, y, rows, w, c


def sweep_cases():
    """(case id, n, F, rows?, kind): kind 'plain' on every shape; 'margin80' has the coefficients scaled until the
    margins pass +-80; 'one_class' has every label 0."""
    out = [(f"{n}x{F}-{'rows' if r else 'ident'}", n, F, r, "plain") for n, F in SHAPES for r in (False, True)]
    return out + [("1031x512-margin80", 1031, 512, False, "margin80"), ("65x100-one_class", 65, 100, True, "one_class")]


def sweep_inputs(n, F, use_rows, kind):
    """-> (x, labels, rows or None, coef [F], intercept [1], class_w [2])."""
    x, y = make_features(n, F, 1)
    if kind == "one_class":
        y = np.zeros_like(y)
    coef, icpt = make_coef(F, 4, scale=30.0 if kind == "margin80" else 1.0)
    return x, y, (make_rows(n, 2) if use_rows else None), coef, icpt, CLASS_W


PROJECT_K = {4: 1, 36: 2, 64: 3, 100: 4, 512: 2, 2048: 4}


def project_cases():
    """(case id, n, F, rows?, labels?): with labels the centre is the mean, without it the origin."""
    return [(f"{n}x{F}-{'rows' if r else 'ident'}-{'labels' if lab else 'nolabels'}", n, F, r, lab)
            for n, F in SHAPES for r in (False, True) for lab in (True, False)]


def project_inputs(n, F, use_rows, use_labels):
    """-> (x, labels or None, rows or None, W [K, F] orthonormal rows, c or None)."""
    x, y = make_features(n, F, 1)
    rows = make_rows(n, 2) if use_rows else None
    rng = np.random.Generator(np.random.PCG64([5, F, 4]))
    q, _ = np.linalg.qr(rng.standard_normal((F, PROJECT_K[F])))
    return x, (y if use_labels else None), rows, np.ascontiguousarray(q.T, dtype=np.float32), (mean32(x, rows) if use_labels else None)

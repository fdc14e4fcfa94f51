"""Shapes and seeded inputs of the k-NN tests, shared by tests/tools/measure_knn_fp32.py (numpy, CPU) and
tests/test_gpu_knn.py (device) so that both see the same numbers."""
import numpy as np

# (F, n_q, n_b, K).  Why these: one pair; one short of a 32-row MFMA tile and of a 64-row half; exactly the tile edges; one
# past them; several bank tiles; several query tiles and bank tiles with the largest K of the 128-query kernel; n_b = K and
# n_b just above it on the 32-query kernel (K > 128); the largest F (64 staged chunks) with three queries.  F = 72 is two
# staged chunks and a quarter, F = 4 half of one MFMA step.  (4, 33, 65, 5) gives the F = 4 group more than one pair: a gate
# measured on a single similarity can fall below the half ulp that any float32 result may be off by.
FLOAT64_SHAPES = [(4, 1, 1, 1), (4, 33, 65, 5), (72, 31, 63, 5), (72, 32, 64, 20), (512, 33, 65, 20), (512, 65, 1000, 20),
                  (512, 257, 5000, 64), (128, 40, 256, 256), (128, 40, 300, 256), (2048, 3, 130, 7)]
# the bank is cut into column groups (hipac_knn_bank_splits >= 2); the second has K = 250 in groups of 256 rows
SPLIT_SHAPES = [(64, 5, 20000, 20), (64, 3, 2560, 250)]


def group_key(F):
    return f"F{F}"


def shape_id(shape):
    return "x".join(str(v) for v in shape)


def float64_inputs(F, n_q, n_b, K):
    """-> (x float32 [n_q + n_b + 3, F] = 0.7 randn, q_rows int32 [n_q], b_rows int32 [n_b]): disjoint, both permuted."""
    rng = np.random.Generator(np.random.PCG64(1000 * F + 7 * n_q + n_b + K))
    n = n_q + n_b + 3
    x = (0.7 * rng.standard_normal((n, F))).astype(np.float32)
    perm = rng.permutation(n).astype(np.int32)
    return x, perm[:n_q].copy(), perm[n_q:n_q + n_b].copy()


def tie_inputs():
    """F = 8, integer features in -2..2 (every dot product exact); 33 queries and 300 bank positions drawn with repeats from
    200 rows, a third of the bank positions copies of earlier ones; both lists permuted."""
    rng = np.random.Generator(np.random.PCG64(4242))
    x = rng.integers(-2, 3, size=(200, 8)).astype(np.float32)
    b = rng.integers(0, 200, size=200)
    b_rows = rng.permutation(np.concatenate([b, rng.choice(b, size=100)])).astype(np.int32)
    q_rows = rng.integers(0, 200, size=33).astype(np.int32)
    return x, q_rows, b_rows


def e2e_inputs():
    """400 x 64 two-cluster features: mean +-1.5 times a fixed sign pattern, unit noise, 25 % positives; labels int64."""
    rng = np.random.Generator(np.random.PCG64(99))
    y = np.zeros(400, np.int64)
    y[rng.permutation(400)[:100]] = 1
    pattern = np.where(np.arange(64) % 3 == 0, -1.0, 1.0)
    x = ((2 * y[:, None] - 1) * 1.5 * pattern[None, :] + rng.standard_normal((400, 64))).astype(np.float32)
    return x, y

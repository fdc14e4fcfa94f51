"""numpy restatement of include/hipac_tta.h: the eight views of square patches in both the rot90 form and the index form (asserted
equal on every call), the table of inverses, and the float32 reduction of given per-view probabilities."""
import numpy as np

VIEWS = 8
INVERSE = (0, 3, 2, 1, 4, 5, 6, 7)


def view_rot90(x, v):
    """x: [n, S, S, C]; view v = r + 4 f: mirror the columns if f, then r quarter turns counter-clockwise."""
    r, f = v & 3, v >> 2
    return np.ascontiguousarray(np.rot90(x[:, :, ::-1] if f else x, r, axes=(1, 2)))


def view_index(x, v):
    """The same view from the header's formulas: out[i][j] = z[a][b], z[a][b] = x[a][S - 1 - b] if f else x[a][b]."""
    r, f = v & 3, v >> 2
    S = x.shape[1]
    i, j = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    a, b = ((i, j), (j, S - 1 - i), (S - 1 - i, S - 1 - j), (S - 1 - j, i))[r]
    if f:
        b = S - 1 - b
    return np.ascontiguousarray(x[:, a, b])


def view(x, v):
    x = np.asarray(x)
    assert x.ndim == 4 and x.shape[1] == x.shape[2] and 0 <= v < VIEWS
    out = view_rot90(x, v)
    assert np.array_equal(out, view_index(x, v))
    return out


def reduce(pv):
    """pv: float32[V, n] per-view probabilities.  (mean, range): the sum added in ascending view order in float32 from the
    first term and divided once by float32(V); the largest minus the smallest view.  A window with a NaN view has NaN in both."""
    pv = np.asarray(pv)
    assert pv.dtype == np.float32 and pv.ndim == 2 and pv.shape[0] >= 1
    total = pv[0].copy()
    lo, hi = pv[0].copy(), pv[0].copy()
    with np.errstate(invalid="ignore"):
        for v in range(1, pv.shape[0]):
            total = (total + pv[v]).astype(np.float32)
            lo = np.where(pv[v] < lo, pv[v], lo)
            hi = np.where(pv[v] > hi, pv[v], hi)
        mean = (total / np.float32(pv.shape[0])).astype(np.float32)
        rng = (hi - lo).astype(np.float32)
    rng[np.isnan(pv).any(0)] = np.float32(np.nan)
    return mean, rng

"""The weighted k-NN probe of include/hipac_knn.h restated in numpy: what tests/test_gpu_knn.py compares the device with.

``similarities`` has two forms: float64 (the reference) and float32 via numpy's float32 matmul (the yardstick whose own
distance from float64 sets the gates, tests/tools/measure_knn_fp32.py).  ``topk`` is the ordering rule alone: descending
similarity, equal similarities by ascending position, NaN after -inf.
"""
import numpy as np


def take(x, rows):
    return x if rows is None else x[np.asarray(rows)]


def inv_norms(x, rows=None, dtype=np.float64):
    """1 / max(|x_i|, 1e-12); with dtype float32 every step is float32."""
    v = take(x, rows).astype(dtype)
    n = np.sqrt((v * v).sum(axis=1, dtype=dtype)).astype(dtype)
    return (dtype(1) / np.maximum(n, dtype(1e-12))).astype(dtype)


def similarities(x, q_rows=None, b_rows=None, q_scale=None, b_scale=None, dtype=np.float64):
    """sim[i][j] = ((x_q[i] . x_b[j]) * q_scale[i]) * b_scale[j] in ``dtype`` (None = no scale)."""
    q, b = take(x, q_rows).astype(dtype), take(x, b_rows).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        s = q @ b.T
        if q_scale is not None:
            s = (s * np.asarray(q_scale, dtype)[:, None]).astype(dtype)
        if b_scale is not None:
            s = (s * np.asarray(b_scale, dtype)[None, :]).astype(dtype)
    return s


def topk(sim, k):
    """-> (values [n_q, k], positions int32 [n_q, k]) by the rule: larger first, equal by lower position, NaN last."""
    sim = np.asarray(sim)
    n_q, n_b = sim.shape
    vals, idx = np.empty((n_q, k), sim.dtype), np.empty((n_q, k), np.int32)
    pos = np.arange(n_b)
    for i in range(n_q):
        row = sim[i]
        nan = np.isnan(row)
        neg = np.where(nan, 0, -(row + 0))  # -0 and +0 are equal; lexsort's last key is the primary one
        order = np.lexsort((pos, neg, nan))[:k]
        vals[i], idx[i] = row[order], order
    return vals, idx


def vote(sim, idx, bank_labels, temperature, class_w):
    """-> (scores float64 [n_q, 2], pred int32 [n_q]); one rounding per operation, neighbours added in list order."""
    sim, idx = np.asarray(sim), np.asarray(idx)
    lab = np.asarray(bank_labels)
    inv_T = 1.0 / float(temperature)
    scores, pred = np.empty((sim.shape[0], 2), np.float64), np.zeros(sim.shape[0], np.int32)
    for i in range(sim.shape[0]):
        s0 = np.float64(sim[i, 0])
        a = [np.float64(0), np.float64(0)]
        with np.errstate(invalid="ignore", over="ignore"):
            for t in range(sim.shape[1]):
                w = np.exp((np.float64(sim[i, t]) - s0) * inv_T)
                c = 1 if lab[idx[i, t]] != 0 else 0
                a[c] = a[c] + w
        sc = [np.float64(class_w[0]) * a[0], np.float64(class_w[1]) * a[1]]
        if np.isnan(s0):
            sc = [np.nan, np.nan]
        scores[i] = sc
        pred[i] = 1 if sc[1] > sc[0] else 0
    return scores, pred


def classify(x, y, train, test, k, temperature, class_w):
    """The whole probe in float64: cosine similarities, lists, vote.  -> sim, idx, scores, pred."""
    qs, bs = inv_norms(x, test), inv_norms(x, train)
    sim, idx = topk(similarities(x, test, train, qs, bs), k)
    scores, pred = vote(sim, idx, np.asarray(y)[np.asarray(train)], temperature, class_w)
    return {"sim": sim, "idx": idx, "scores": scores, "pred": pred}

"""The patch-level evaluation of include/hipac_evaluate.h restated in plain numpy / Python integers, the float definitions
``evaluate.metrics_from_confusion`` / ``evaluate.curves`` are checked against, and the row sets the tests run on; shared by
tests/test_evaluate_host.py, tests/test_gpu_eval_patches.py and tools/evalpatchbench.py.

* ``accumulate``: the three running tables from rows, one row at a time.
* ``integers`` / ``integers_all``: a replicate's integers from the draw counts of tests/eval_ci_cpu.py (``draws``), through the
  dense weighted histogram the kernel never materialises.
* ``metrics`` / ``roc_ap``: the reference's src/utils/metrics.py formulas on 0 / 1 arrays, and ROC / AUC / average precision
  from per-row bins by sorting and pair counting -- routes that share nothing with the package's histogram arithmetic.
* ``row_cases``: the row sets of the GPU tests, made once per process.
"""
import functools

import numpy as np

from eval_ci_cpu import draws  # noqa: F401 -- the draws are eval_ci's, by definition

BINS = 4096
SEED = 0x9E3779B97F4A7C15  # both key words in use


def bin_of(p32):
    """The header's bin of float32 probabilities: min(4095, (int)(p * 4096.0f))."""
    p32 = np.asarray(p32, np.float32)
    return np.minimum(BINS - 1, (p32 * np.float32(4096.0)).astype(np.int64))


def bin_of_f64(p64):
    """The same formula in float64 (what a float64 softmax would be binned to)."""
    return np.minimum(BINS - 1, np.floor(np.asarray(p64, np.float64) * 4096.0).astype(np.int64))


def empty_tables(G):
    return {"hist": np.zeros((G, 2, BINS), np.int64), "conf": np.zeros((G, 4), np.int64), "n_bad": 0}


def accumulate(tables, p, pred, label, group):
    """Add rows to ``tables`` in place, by the header's rules; returns ``tables``."""
    G = tables["hist"].shape[0]
    p = np.asarray(p, np.float32)
    for v, yhat, y, g in zip(p.tolist(), np.asarray(pred).tolist(), np.asarray(label).tolist(), np.asarray(group).tolist()):
        if v != v or v < 0.0 or v > 1.0 or y > 1 or yhat > 1 or g < 0 or g >= G:
            tables["n_bad"] += 1
            continue
        tables["hist"][g, y, int(bin_of(np.float32(v)))] += 1
        tables["conf"][g, 2 * y + yhat] += 1  # (TN, FP, FN, TP)
    return tables


def integers(hist, conf, counts):
    """One replicate's integers (conf_w[4], u2, n_pos, n_neg) as Python integers."""
    c = np.asarray(counts, np.int64)
    H = np.einsum("g,gtb->tb", c, np.asarray(hist))  # [2, 4096], int64
    conf_w = [int(v) for v in (c[:, None] * np.asarray(conf, np.int64)).sum(0)]
    below = np.concatenate([[0], np.cumsum(H[0])[:-1]])  # negatives in the bins before b
    u2 = sum(int(v) for v in H[1] * (2 * below + H[0]))  # each term fits int64 under the contract; the sum is exact
    return conf_w, u2, int(H[1].sum()), int(H[0].sum())


def integers_all(hist, conf, counts):
    """The dict of arrays ``evaluate.bootstrap_integers`` returns, for counts int[B, G]."""
    rows = [integers(hist, conf, c) for c in counts]
    return {"conf_w": np.asarray([r[0] for r in rows], np.int64).reshape(len(rows), 4), "u2": np.asarray([r[1] for r in rows], np.int64),
            "n_pos": np.asarray([r[2] for r in rows], np.int64), "n_neg": np.asarray([r[3] for r in rows], np.int64)}


# ---- the float definitions ----------------------------------------------------------------------------------------------


def metrics(y_true, y_pred):
    """src/utils/metrics.py on 0 / 1 arrays (accuracy None for no rows), plus specificity and balanced accuracy."""
    y_true, y_pred = np.asarray(y_true, np.int64), np.asarray(y_pred, np.int64)
    tp = int(((y_true == 1) & (y_pred == 1)).sum())
    tn = int(((y_true == 0) & (y_pred == 0)).sum())
    fp = int(((y_true == 0) & (y_pred == 1)).sum())
    fn = int(((y_true == 1) & (y_pred == 0)).sum())
    prec = tp / (tp + fp) if (tp + fp) > 0 else 0.0
    rec = tp / (tp + fn) if (tp + fn) > 0 else 0.0
    spec = tn / (tn + fp) if (tn + fp) > 0 else 0.0
    return {"accuracy": float((y_true == y_pred).mean()) if y_true.size else None, "precision": prec, "recall": rec,
            "f1_score": 2 * (prec * rec) / (prec + rec) if (prec + rec) > 0 else 0.0, "specificity": spec,
            "balanced_accuracy": (rec + spec) / 2}


def auc_pairs(label, score):
    """The Mann-Whitney AUC by counting pairs (ties half), in exact integers up to the last division; None for one class."""
    label, score = np.asarray(label).astype(bool), np.asarray(score)
    pos, neg = np.sort(score[label]), np.sort(score[~label])
    if not pos.size or not neg.size:
        return None
    below = np.searchsorted(neg, pos, side="left")
    tied = np.searchsorted(neg, pos, side="right") - below
    return int((2 * below + tied).sum()), int(pos.size), int(neg.size)


def roc_ap(label, bins):
    """(thresholds, fpr, tpr, average precision) from per-row bins: the distinct bins in descending order after (0, 0)."""
    label, bins = np.asarray(label).astype(bool), np.asarray(bins, np.int64)
    P, N = int(label.sum()), int((~label).sum())
    thr, fpr, tpr, ap, prev_tp = [None], [0.0 if N else None], [0.0 if P else None], 0.0, 0
    for b in sorted(set(bins.tolist()), reverse=True):
        tp, fp = int((label & (bins >= b)).sum()), int((~label & (bins >= b)).sum())
        thr.append(b / BINS)
        fpr.append(fp / N if N else None)
        tpr.append(tp / P if P else None)
        if P:
            ap += ((tp - prev_tp) / P) * (tp / (tp + fp))
        prev_tp = tp
    return thr, fpr, tpr, (ap if P else None)


# ---- the row sets -------------------------------------------------------------------------------------------------------


def edge_scores():
    """float32 scores on and just below bin edges, with 0 and 1."""
    k = np.array([1, 2, 7, 1024, 2048, 4095], np.float32) / np.float32(4096.0)
    return np.concatenate([[0.0, 1.0], k, np.nextafter(k, np.float32(0.0)), [np.nextafter(np.float32(1.0), np.float32(0.0))]]).astype(np.float32)


def make_rows(seed, n, G, kind="mixed"):
    """n rows of ``G`` slides arriving slide by slide: p float32, pred, label uint8, group int32.  ``mixed``: random scores
    with every edge score in, slide 1 (when G > 2) left without rows, a few bad rows (NaN, label 2, group = G, group -1);
    ``equal``: all scores 0.5; ``one_class``: no tumour row."""
    rng = np.random.default_rng(seed)
    slides = [g for g in range(G) if not (G > 2 and g == 1)]
    group = np.sort(rng.choice(slides, n)).astype(np.int32) if n else np.zeros(0, np.int32)
    label = (rng.random(n) < 0.4).astype(np.uint8)
    p = np.clip(0.5 + 0.25 * rng.standard_normal(n) + 0.2 * (label.astype(np.float64) - 0.5), 0.0, 1.0).astype(np.float32)
    if kind == "equal":
        p[:] = 0.5
    if kind == "one_class":
        label[:] = 0
    pred = (p > 0.5).astype(np.uint8)
    if kind == "mixed" and n:
        e = edge_scores()
        at = rng.permutation(n)[:min(n, e.size)]
        p[at] = e[:at.size]
        pred[at] = (p[at] > 0.5).astype(np.uint8)
        if n >= 255:
            bad = rng.permutation(n)[:5]
            p[bad[0]] = np.nan
            label[bad[1]] = 2
            group[bad[2]] = G
            group[bad[3]] = -1
            pred[bad[4]] = 3
    return p, pred, label, group


@functools.lru_cache(maxsize=None)
def row_cases():
    """name -> (G, rows): G in {1, 3, 37} x n in {0, 1, 255, 257, 5000}, plus all-equal scores and a one-class set."""
    out = {}
    for G in (1, 3, 37):
        for n in (0, 1, 255, 257, 5000):
            out[f"G{G}_n{n}"] = (G, make_rows(1000 * G + n, n, G))
    out["G3_equal"] = (3, make_rows(7, 300, 3, "equal"))
    out["G3_one_class"] = (3, make_rows(8, 300, 3, "one_class"))
    return out


@functools.lru_cache(maxsize=None)
def reference_tables(name):
    """The restatement's tables of a row case (made once, left unchanged by the tests)."""
    G, rows = row_cases()[name]
    return accumulate(empty_tables(G), *rows)


def sparse_tables(G=4096, seed=3):
    """hist / conf of G slides with a handful of occupied bins each (some slides empty): what G = 4096 needs to stay small."""
    rng = np.random.default_rng(seed)
    t = {"hist": np.zeros((G, 2, BINS), np.int32), "conf": np.zeros((G, 4), np.int64), "n_bad": 0}
    for g in range(G):
        for _ in range(int(rng.integers(0, 4))):
            y, b, k = int(rng.integers(0, 2)), int(rng.integers(0, BINS)), int(rng.integers(1, 50))
            t["hist"][g, y, b] += k
            hit = int(rng.integers(0, k + 1))  # k rows of class y, `hit` of them called tumour
            t["conf"][g, 2 * y + 1] += hit
            t["conf"][g, 2 * y] += k - hit
    return t

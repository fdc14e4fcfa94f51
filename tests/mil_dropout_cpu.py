"""The dropout mask of include/hipac_mil_dropout.h restated in numpy, and the yardsticks built on it, shared by
tests/test_mil_dropout_host.py, tests/test_gpu_mil_dropout.py and tests/tools/measure_mil_dropout_fp32.py.

* ``philox`` / ``keep_mask`` / ``masked_rows``: Philox4x32-10, counter (column // 4, row, sample, site), key = the two
  words of the seed; kept iff word >= floor(p * 2^32); a kept value is fl32(x * fl32(1 / (1 - p))).  Written apart from
  the package's ``mil_dropout.host_mask`` so that the two can be held against each other.
* ``train_reference`` / ``mc_reference``: ``mil.MILClassifier`` in ``train()`` mode under torch autograd on the CPU, one
  bag per forward, with these masks applied explicitly -- float64 for the tests, float32 for the measurement of the gates.
* ``mc_statistics``: the five statistics of hipac_mil_mc_forward from per-sample logits, in float64, with the device's
  order of operations (samples in order, classes in order, two passes for the variance).
"""
import math

import numpy as np
import torch
import torch.nn as nn

import mil_train_cases as base

DIMS = [(128, 64, 32, 3), (512, 128, 128, 2)]  # (F, A, hidden, C), from tests/mil_train_cases.py
SIZES = [1, 63, 64, 65, 130]  # a bag of one row; bags ending on, before and after a 64-row edge; one bag over three tiles
POOLINGS = base.POOLINGS
PS = [0.1, 0.5]
TS = [1, 2, 7]
SEED = 0x9E3779B97F4A7C15  # both key words in use

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 -> the four output words (uint32 arrays of the counters' broadcast shape)."""
    x0, x1, x2, x3 = [np.array(v, dtype=np.uint64) & LO for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0), int(k1)
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) % 2 ** 32, (k1 + W1) % 2 ** 32
        prod0, prod1 = x0 * np.uint64(M0), x2 * np.uint64(M1)
        hi0, lo0, hi1, lo1 = prod0 >> np.uint64(32), prod0 & LO, prod1 >> np.uint64(32), prod1 & LO
        x0, x1, x2, x3 = hi1 ^ x1 ^ np.uint64(k0), lo1, hi0 ^ x3 ^ np.uint64(k1), lo0
    return x0.astype(np.uint32), x1.astype(np.uint32), x2.astype(np.uint32), x3.astype(np.uint32)


def words(seed, sample, site, n_rows, n_cols, row0=0):
    """uint32[n_rows, n_cols]: the word of every element."""
    cols = np.arange(n_cols)
    rows = np.arange(row0, row0 + n_rows)
    w = philox((cols // 4)[None, :], rows[:, None], sample, site, seed % 2 ** 32, seed // 2 ** 32 % 2 ** 32)
    return np.choose((cols % 4)[None, :], w)


def thr_of(p):
    assert 0.0 <= p < 1.0
    return int(math.floor(p * 2.0 ** 32))


def scale_of(p):
    return np.float32(1.0 / (1.0 - p))


def keep_mask(p, seed, sample, site, n_rows, n_cols, row0=0):
    return words(seed, sample, site, n_rows, n_cols, row0) >= np.uint32(thr_of(p))


def masked_rows(x, p, seed, sample, row0=0):
    """float32[n, F] -> the site-0 masked rows in float32: fl32(x * scale) where kept, 0 elsewhere."""
    x = np.asarray(x, np.float32)
    keep = keep_mask(p, seed, sample, 0, x.shape[0], x.shape[1], row0)
    return np.where(keep, x * scale_of(p), np.float32(0)).astype(np.float32)


# ----------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------
def make_inputs(dims, permuted, seed=0):
    return base.make_inputs(dims, permuted, sizes=SIZES, seed=seed)


def make_model(dims, pooling):
    return base.make_model(dims, pooling)


def group_key(dims, pooling):
    return ",".join(map(str, dims)) + "," + pooling


def case_list():
    """(id, dims, pooling, p): every dims x pooling x p; the training cases also take class weights and a permuted row
    index."""
    return [(f"{pooling}-F{dims[0]}-p{p}", dims, pooling, p) for dims in DIMS for pooling in POOLINGS for p in PS]


# ----------------------------------------------------------------------------
# yardsticks
# ----------------------------------------------------------------------------
def forward_masked(m, xm, offsets, p, seed, sample):
    """The twin ``m`` over already-masked rows ``xm`` (tensor of m's dtype), the hidden mask applied explicitly
    -> logits [B, C], [attention per bag] (None entries for mean / max)."""
    hidden = m.classifier[0].out_features
    B = len(offsets) - 1
    keep = torch.from_numpy(keep_mask(p, seed, sample, 1, B, hidden))
    s = torch.tensor(float(scale_of(p)), dtype=xm.dtype)
    logits, attn = [], []
    for b, (a, e) in enumerate(zip(offsets[:-1], offsets[1:])):
        pooled, w = m._aggregate(xm[a:e])
        hid = torch.relu(m.classifier[0](pooled))
        hid = torch.where(keep[b], hid * s, torch.zeros((), dtype=xm.dtype))
        logits.append(m.classifier[2](hid))
        attn.append(None if w is None else w[:, 0])
    return torch.stack(logits), attn


def train_reference(model_f32, pooling, feats, rows, offsets, labels, cw, p, seed, step, dtype):
    """loss, logits and gradients of the step under the masks of (seed, sample = step), in ``dtype`` on the CPU."""
    m = base.make_twin(model_f32, dtype)
    x = feats if rows is None else feats[rows.long()]
    xm = torch.from_numpy(masked_rows(x.numpy(), p, seed, step)).to(dtype)
    logits, _ = forward_masked(m, xm, offsets, p, seed, step)
    loss = nn.CrossEntropyLoss(weight=None if cw is None else cw.to(dtype))(logits, labels)
    loss.backward()
    return loss.detach(), logits.detach(), {k: q.grad.detach().clone() for k, q in m.named_parameters()}


def mc_reference(model_f32, pooling, feats, offsets, p, seed, first_sample, n_samples, dtype):
    """-> logits [T, B, C], attention [T, n] (None for mean / max), in ``dtype`` on the CPU."""
    m = base.make_twin(model_f32, dtype)
    zs, ws = [], []
    with torch.no_grad():
        for t in range(first_sample, first_sample + n_samples):
            xm = torch.from_numpy(masked_rows(feats.numpy(), p, seed, t)).to(dtype)
            z, w = forward_masked(m, xm, offsets, p, seed, t)
            zs.append(z)
            ws.append(None if w[0] is None else torch.cat(w))
    return torch.stack(zs), (None if ws[0] is None else torch.stack(ws))


def mc_statistics(logits):
    """float [T, B, C] -> dict of float64 arrays: mean_prob, var_prob [B, C]; entropy, expected_entropy, mutual_info [B]."""
    z = np.asarray(logits, np.float64)
    T, B, C = z.shape
    out = {"mean_prob": np.zeros((B, C)), "var_prob": np.zeros((B, C)), "entropy": np.zeros(B), "expected_entropy": np.zeros(B),
           "mutual_info": np.zeros(B)}

    def probs(t, b):
        mx = max(float(v) for v in z[t, b])
        e = [math.exp(float(v) - mx) for v in z[t, b]]
        s = 0.0
        for v in e:
            s += v
        return [v / s for v in e]

    for b in range(B):
        mean, eh = [0.0] * C, 0.0
        for t in range(T):
            pr, h = probs(t, b), 0.0
            for c in range(C):
                mean[c] += pr[c]
                if pr[c] > 0.0:
                    h += pr[c] * math.log(pr[c])
            eh += -h
        mean = [v / T for v in mean]
        eh = eh / T
        var = [0.0] * C
        if T > 1:
            for t in range(T):
                pr = probs(t, b)
                for c in range(C):
                    d = pr[c] - mean[c]
                    var[c] += d * d
            var = [v / (T - 1) for v in var]
        h = 0.0
        for c in range(C):
            if mean[c] > 0.0:
                h += mean[c] * math.log(mean[c])
        out["mean_prob"][b], out["var_prob"][b] = mean, var
        out["entropy"][b], out["expected_entropy"][b], out["mutual_info"][b] = -h, eh, max(-h - eh, 0.0)
    return out


rel = base.rel

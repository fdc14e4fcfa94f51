"""CPU references of the training head's four primitives (csrc/train.hip: linear forward / backward, weighted
cross-entropy, Adam; csrc/ntxent.hip: NT-Xent), for tests/test_oracle_head.py and tests/test_gpu_head.py.

Two families, neither of which calls the native code:

  * float64 references (numpy, NT-Xent: oracle/ntxent_ref.py under torch autograd in float64), written from the formulas in
    the kernels' header comments and the reference's src/models/simclr.py:31-54.  Sums are numpy's / torch's own.
  * float32 stand-ins (class StandIn): the same formulas in plain torch float32 ops, summation order torch's.  They serve
    two ends: their distance from the float64 reference on the test's own inputs is what the gates of the GPU test are
    made of (tests/tools/measure_head_fp32.py), and with ``fault=`` they apply exactly ONE of the faults of FAULTS, the
    mistakes a change to the kernels could make, to show that the cases and metrics of tests/head_cases.py notice each.

Scalars of the C ABI are floats: lr, the betas, eps and the temperature enter every reference as the float32 value the
native call receives, widened to double (beta2 = 0.999 is 0.99900001287 there, and 1 - beta2 is 1.3e-5 from 0.001).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ntxent_ref  # noqa: E402

FAULTS = {
    "linear": ("k_tail", "mask_ge", "acc_overwrite", "db_rows16"),
    "ce": ("mean_over_m", "group_tail", "no_max_shift"),
    "adam": ("no_stride", "eps_in_sqrt", "bc_prev_step"),
    "ntxent": ("diag_in_lse", "pair_no_wrap", "lse_tail", "no_projection"),
}
ADAM_GRID_ELEMS = 4096 * 256  # adam_kernel: the grid is capped at 4096 workgroups of 256 threads


def f64(a):
    return np.asarray(a, dtype=np.float64)


def f32s(v):
    """A float scalar as the C ABI passes it on: rounded to float32, widened to double."""
    return float(np.float32(v))


# ---------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------
def linear_forward(x, w, b, relu):
    """y[M][N] = x[M][K] w[N][K]^T + b (ReLU)."""
    y = f64(x) @ f64(w).T
    if b is not None:
        y = y + f64(b)
    return np.maximum(y, 0.0) if relu else y


def linear_forward_sums(x, w, b):
    """Per element of y: the sum of |products| plus |bias| (the S of the error bound), and the reduction length."""
    s = np.abs(f64(x)) @ np.abs(f64(w)).T
    if b is not None:
        s = s + np.abs(f64(b))
    return s, np.shape(x)[1]


def relu_mask(y):
    """The units a ReLU lets the gradient through: y > 0 (false at +0, -0, negatives and NaN)."""
    with np.errstate(invalid="ignore"):
        return np.asarray(y) > 0


def linear_backward(x, w, dy, y=None, dw_prev=None, db_prev=None):
    """Backward of y = relu?(x w^T + b): (dx[M][K], dw[N][K], db[N], masked dy[M][N]).  ``y`` (the layer's output) switches
    the ReLU mask on; ``dw_prev`` / ``db_prev`` are what an accumulating call adds to."""
    dym = f64(dy) if y is None else np.where(relu_mask(y), f64(dy), 0.0)
    dx = dym @ f64(w)
    dw = dym.T @ f64(x)
    db = dym.sum(axis=0)
    if dw_prev is not None:
        dw = dw + f64(dw_prev)
    if db_prev is not None:
        db = db + f64(db_prev)
    return dx, dw, db, dym


def linear_backward_sums(x, w, dy, y=None, dw_prev=None, db_prev=None):
    """The S of dx, dw and db (sum of |products|, plus |previous value| where one is added)."""
    a = np.abs(f64(dy)) if y is None else np.where(relu_mask(y), np.abs(f64(dy)), 0.0)
    sdx = a @ np.abs(f64(w))
    sdw = a.T @ np.abs(f64(x))
    sdb = a.sum(axis=0)
    if dw_prev is not None:
        sdw = sdw + np.abs(f64(dw_prev))
    if db_prev is not None:
        sdb = sdb + np.abs(f64(db_prev))
    return sdx, sdw, sdb


def cross_entropy(logits, labels, class_w=None):
    """nn.CrossEntropyLoss(weight=class_w), mean reduction sum w[y] nll / sum w[y]: (loss, dlogits[M][C])."""
    l = f64(logits)
    labels = np.asarray(labels, dtype=np.int64)
    rows = np.arange(l.shape[0])
    mx = l.max(axis=1, keepdims=True)
    e = np.exp(l - mx)
    se = e.sum(axis=1)
    nll = np.log(se) + mx[:, 0] - l[rows, labels]
    w = np.ones(l.shape[0]) if class_w is None else f64(class_w)[labels]
    with np.errstate(invalid="ignore", divide="ignore"):
        sw = w.sum()
        loss = (w * nll).sum() / sw
        d = e / se[:, None]
        d[rows, labels] -= 1.0
        return float(loss), d * (w / sw)[:, None]


def adam_steps(p, grads, m, v, step, lr, beta1, beta2, eps):
    """torch.optim.Adam (no weight decay, no amsgrad): steps ``step``, ``step + 1``, ... (1-based), one per entry of
    ``grads``, from the state (m, v).  Bias corrections in double.  Returns (p, m, v) in float64."""
    p, m, v = f64(p).copy(), f64(m).copy(), f64(v).copy()
    lr, b1, b2, eps = f32s(lr), f32s(beta1), f32s(beta2), f32s(eps)
    for k, g in enumerate(grads):
        g = f64(g)
        t = step + k
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        p = p - lr * (m / bc1) / (np.sqrt(v / bc2) + eps)
    return p, m, v


def ntxent(z, temperature):
    """NT-Xent of z = cat(z_i, z_j) [2N][D] as the reference computes it (oracle/ntxent_ref.py), float64 autograd:
    (loss, dz[2N][D])."""
    zt = torch.from_numpy(f64(z).copy()).requires_grad_(True)
    n = zt.shape[0] // 2
    loss = ntxent_ref.nt_xent_loss_ref(zt[:n], zt[n:], f32s(temperature))
    loss.backward()
    return float(loss.detach()), zt.grad.numpy()


# ---------------------------------------------------------------------------------------------
# float32 stand-ins, one injected fault at a time
# ---------------------------------------------------------------------------------------------
def _t(a, dtype):
    return torch.from_numpy(np.array(a)).to(dtype)  # a copy: the cases' arrays are read-only


class StandIn:
    """The head's primitives in plain torch ops of ``dtype`` (float32: the stand-in; float64: the closed forms, held to
    autograd by tests/test_oracle_head.py).  Inputs and outputs are numpy arrays, as the native runner's."""

    def __init__(self, fault=None, dtype=torch.float32):
        assert fault is None or any(fault in v for v in FAULTS.values()), fault
        self.fault, self.dtype = fault, dtype

    def _np(self, t):
        return t.numpy()

    # a [M][L] times bt [L][N]
    def _mm(self, a, bt):
        L = a.shape[1]
        if self.fault == "k_tail" and L % 32:
            a, bt = a[:, : 32 * (L // 32)], bt[: 32 * (L // 32)]
        return a @ bt

    def linear_forward(self, x, w, b, relu):
        x, w = _t(x, self.dtype), _t(w, self.dtype)
        y = self._mm(x, w.T)
        if b is not None:
            y = y + _t(b, self.dtype)
        return self._np(torch.relu(y) if relu else y)

    def linear_backward(self, x, w, dy, y, dw0, db0, accumulate, want_dx):
        """-> (dym or None, dx or None, dw, db); dw0 / db0 are the buffers' contents before the call."""
        x, w, g = _t(x, self.dtype), _t(w, self.dtype), _t(dy, self.dtype)
        dym = None
        if y is not None:
            yt = _t(y, self.dtype)
            keep = yt >= 0 if self.fault == "mask_ge" else yt > 0
            g = dym = torch.where(keep, g, torch.zeros_like(g))
        M = g.shape[0]
        db = (g[: 16 * (M // 16)] if self.fault == "db_rows16" else g).sum(dim=0)
        dx = self._mm(g, w) if want_dx else None
        dw = self._mm(g.T, x)
        if accumulate:
            db = _t(db0, self.dtype) + db
            if self.fault != "acc_overwrite":
                dw = _t(dw0, self.dtype) + dw
        return (None if dym is None else self._np(dym), None if dx is None else self._np(dx), self._np(dw), self._np(db))

    def cross_entropy(self, logits, labels, class_w):
        l = _t(logits, self.dtype)
        y = torch.from_numpy(np.asarray(labels, dtype=np.int64))
        M = l.shape[0]
        rows = torch.arange(M)
        if self.fault == "no_max_shift":
            e = torch.exp(l)
            se = e.sum(dim=1)
            nll = torch.log(se) - l[rows, y]
        else:
            mx = l.max(dim=1).values
            e = torch.exp(l - mx[:, None])
            se = e.sum(dim=1)
            nll = torch.log(se) + mx - l[rows, y]
        w = torch.ones(M, dtype=self.dtype) if class_w is None else _t(class_w, self.dtype)[y]
        top = 256 * (M // 256) if self.fault == "group_tail" else M
        num = (w * nll)[:top].sum()
        den = torch.tensor(float(M), dtype=self.dtype) if self.fault == "mean_over_m" else w[:top].sum()
        d = e / se[:, None]
        d[rows, y] -= 1.0
        return float(num / den), self._np(d * (w / den)[:, None])

    def adam_steps(self, p, grads, m, v, step, lr, beta1, beta2, eps):
        p, m, v = _t(p, self.dtype).clone(), _t(m, self.dtype).clone(), _t(v, self.dtype).clone()
        lr, b1, b2, eps = f32s(lr), f32s(beta1), f32s(beta2), f32s(eps)
        n = p.numel()
        top = min(n, ADAM_GRID_ELEMS) if self.fault == "no_stride" else n
        for k, g in enumerate(grads):
            g = _t(g, self.dtype)[:top]
            t = step + k
            tc = t - 1 if (self.fault == "bc_prev_step" and t >= 2) else t
            bc1, bc2 = 1.0 - b1 ** tc, 1.0 - b2 ** tc
            mi = b1 * m[:top] + (1.0 - b1) * g
            vi = b2 * v[:top] + (1.0 - b2) * g * g
            if self.fault == "eps_in_sqrt":
                den = torch.sqrt(vi / bc2 + eps)
            else:
                den = torch.sqrt(vi) / (bc2 ** 0.5) + eps
            m[:top], v[:top] = mi, vi
            p[:top] = p[:top] - (lr / bc1) * mi / den
        return self._np(p), self._np(m), self._np(v)

    def ntxent(self, z, temperature, want_grad=True):
        """The closed form of csrc/ntxent.hip's header comment."""
        z = _t(z, self.dtype)
        rows, n, t = z.shape[0], z.shape[0] // 2, f32s(temperature)
        inv = 1.0 / z.norm(dim=1).clamp_min(1e-12)
        zn = z * inv[:, None]
        S = (zn @ zn.T) / t
        i = torch.arange(rows)
        pair = (i + n).clamp_max(rows - 1) if self.fault == "pair_no_wrap" else (i + n) % rows
        eye = torch.eye(rows, dtype=torch.bool)
        Sm = S if self.fault == "diag_in_lse" else S.masked_fill(eye, float("-inf"))
        if self.fault == "lse_tail" and rows % 256:
            Sm = Sm[:, : 256 * (rows // 256)]
        lse = torch.logsumexp(Sm, dim=1) if Sm.shape[1] else torch.full((rows,), float("-inf"), dtype=self.dtype)
        Soff = S.masked_fill(eye, float("-inf"))
        loss = float((lse - Soff[i, pair]).mean())
        if not want_grad:
            return loss, None
        C = torch.exp(Soff - lse[:, None]) + torch.exp(Soff - lse[None, :])
        C[i, pair] -= 2.0
        C = C.masked_fill(eye, 0.0)
        g = (C @ zn) / (rows * t)
        if self.fault == "no_projection":
            dz = g * inv[:, None]
        else:
            dz = (g - zn * (zn * g).sum(dim=1, keepdim=True)) * inv[:, None]
        return loss, self._np(dz)

"""Cases, metrics and gates of the training head's primitives, shared by tests/test_oracle_head.py (CPU: the float32
stand-in of tests/head_cpu.py, with and without an injected fault) and tests/test_gpu_head.py (the native C ABI).

Every case is seeded, made on the CPU and stored as float32.  The shapes are the smallest that reach each boundary of
the kernels (csrc/train.hip, csrc/ntxent.hip): the 64 x 64 x 32 tiles of gemm_f32_kernel (all three stride forms, so
every listed size is also a reduction length in the backward), the 16 x 16 blocks of bias_grad_kernel, the 256-row
groups of ce_kernel and its scratch of 2 + 8 * ceil(M / 256) floats, the 4096 x 256 grid cap of adam_kernel, the
256-column walk of ntx_lse_kernel.

An implementation under test is an object with

    linear_forward(x, w, b, relu) -> y
    linear_backward(x, w, dy, y, dw0, db0, accumulate, want_dx) -> (dym | None, dx | None, dw, db)
    cross_entropy(logits, labels, class_w) -> (loss, dlogits)
    adam_steps(p, grads, m, v, step, lr, beta1, beta2, eps) -> (p, m, v)
    ntxent(z, temperature, want_grad=True) -> (loss, dz | None)

on numpy arrays (head_cpu.StandIn; the native runner of tests/test_gpu_head.py).

Gates.  Linear outputs: element-wise and derived, |got - ref64| <= (L + 3) * 2^-24 * S, L the reduction length, S the
float64 sum of |products| of that element plus |bias| and |previous value| where they enter -- the standard bound of a
length-L float32 sum in any order, fused or not; an element with S = 0 must be exact; the ReLU-masked dy must be
bitwise right.  ``linear_ratios`` returns |got - ref64| / bound, worst element per tensor; 1 is the gate.
Cross-entropy, Adam, NT-Xent: each tensor at FACTOR = 10 x the distance the float32 stand-in keeps from the float64
reference on exactly these inputs, metric max|a - b| / max|b| (Adam's p: applied to the move p_new - p_old), the largest
figure over the cases of a group = (primitive, tensor, input kind); tests/tools/measure_head_fp32.py records them in
tests/golden/head_fp32_distances.json.  A gate of exactly 0 asks for exact zeros.
"""
from __future__ import annotations

import functools
import itertools
import json
import math
import os

import numpy as np
import torch

import head_cpu as H

U = 2.0 ** -24
FACTOR = 10.0
FLT_MIN = np.float32(1.17549435e-38)
JSON_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_fp32_distances.json")
HOW = "python tests/tools/measure_head_fp32.py"


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * m for k, m in zip(key, (1, 1009, 1000003, 7919, 104729))) + 12345)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).numpy()


# ---------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------
def rel(got, ref):
    """max|got - ref| / max|ref|.  NaNs must sit at the same places (else inf); an all-zero reference asks for zeros."""
    got, ref = H.f64(got), H.f64(ref)
    if got.shape != ref.shape:
        return math.inf
    ng, nr = np.isnan(got), np.isnan(ref)
    if (ng != nr).any():
        return math.inf
    if nr.all():
        return 0.0
    d = float(np.abs(got[~nr] - ref[~nr]).max())
    s = float(np.abs(ref[~nr]).max())
    if d == 0.0:
        return 0.0
    return d / s if s > 0.0 else math.inf


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def bound_ratio(got, ref, S, L):
    """Worst |got - ref| / ((L + 3) 2^-24 S) over the elements; an element with S = 0 must be exact."""
    got = H.f64(got)
    if got.shape != ref.shape:
        return math.inf
    d = np.abs(got - ref)
    if np.isnan(d).any():
        return math.inf
    b = (L + 3) * U * S
    r = np.where(b > 0, d / np.where(b > 0, b, 1.0), np.where(d == 0, 0.0, math.inf))
    return float(r.max())


# ---------------------------------------------------------------------------------------------
# linear
# ---------------------------------------------------------------------------------------------
LINEAR_SHAPES = [(1, 1, 1), (1, 2, 31), (63, 65, 32), (64, 64, 33), (65, 63, 64), (129, 1, 95), (2, 130, 1), (15, 17, 70),
                 (16, 128, 512)]
MASK_SHAPE = (15, 17, 70)
# (row, column) -> value of y in the special mask case; the second entry says whether the unit lets the gradient through
MASK_PLACES = {(0, 0): (np.float32(0.0), False), (3, 16): (np.float32(-0.0), False), (7, 5): (FLT_MIN, True),
               (14, 16): (-FLT_MIN, False), (14, 0): (np.float32("nan"), False)}


@functools.lru_cache(maxsize=None)
def linear_inputs(shape):
    M, N, K = shape
    g = _gen(1, M, N, K)
    d = {"x": _randn(g, M, K), "w": _randn(g, N, K) * np.float32(0.3), "b": _randn(g, N) * np.float32(0.5),
         "dy": _randn(g, M, N), "dw0": _randn(g, N, K), "db0": _randn(g, N)}
    # the mask input of the backward: the layer's own ReLU output (about half of it exact zeros)
    d["y"] = H.linear_forward(d["x"], d["w"], d["b"], True).astype(np.float32)
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def mask_special_y():
    M, N, _ = MASK_SHAPE
    y = _randn(_gen(2, M, N), M, N)
    for (r, c), (val, _) in MASK_PLACES.items():
        y[r, c] = val
    y.setflags(write=False)
    return y


def linear_runs():
    """(tag, mask, accumulate, want_dx) of every backward run of a shape."""
    return [(f"bwd-mask{int(mk)}-acc{acc}-dx{int(dx)}", mk, acc, dx)
            for mk, acc, dx in itertools.product((False, True), (0, 1), (True, False))]


def _backward_ratios(impl, d, y, acc, want_dx, tag, out):
    M, N = d["dy"].shape
    K = d["x"].shape[1]
    prev = (d["dw0"], d["db0"]) if acc else (None, None)
    dx, dw, db, dym = H.linear_backward(d["x"], d["w"], d["dy"], y, *prev)
    sdx, sdw, sdb = H.linear_backward_sums(d["x"], d["w"], d["dy"], y, *prev)
    gdym, gdx, gdw, gdb = impl.linear_backward(d["x"], d["w"], d["dy"], y, d["dw0"], d["db0"], acc, want_dx)
    if y is not None:
        out[f"{tag}/dym_bits"] = 0.0 if (gdym is not None and same_bits(gdym, dym.astype(np.float32))) else math.inf
    if want_dx:
        out[f"{tag}/dx"] = bound_ratio(gdx, dx, sdx, N) if gdx is not None else math.inf
    out[f"{tag}/dw"] = bound_ratio(gdw, dw, sdw, M)
    out[f"{tag}/db"] = bound_ratio(gdb, db, sdb, M)
    return gdym


def linear_ratios(impl, shape):
    """{run/tensor: worst |got - ref64| / bound}; every entry must be <= 1 (bitwise checks give 0 or inf)."""
    d = linear_inputs(shape)
    K = shape[2]
    out = {}
    s, _ = H.linear_forward_sums(d["x"], d["w"], d["b"])
    for relu in (False, True):
        got = impl.linear_forward(d["x"], d["w"], d["b"], relu)
        out[f"fwd-relu{int(relu)}/y"] = bound_ratio(got, H.linear_forward(d["x"], d["w"], d["b"], relu), s, K)
    for tag, mk, acc, want_dx in linear_runs():
        _backward_ratios(impl, d, d["y"] if mk else None, acc, want_dx, tag, out)
    if shape == MASK_SHAPE:  # y holds +0, -0, FLT_MIN, -FLT_MIN and NaN at known places
        y = mask_special_y()
        for acc in (0, 1):
            gdym = _backward_ratios(impl, d, y, acc, True, f"special-acc{acc}", out)
            ok = gdym is not None
            for (r, c), (_, kept) in MASK_PLACES.items():
                want = d["dy"][r, c] if kept else np.float32(0.0)
                ok = ok and same_bits(gdym[r, c], want)
            out[f"special-acc{acc}/dym_places"] = 0.0 if ok else math.inf
    return out


# ---------------------------------------------------------------------------------------------
# cross-entropy
# ---------------------------------------------------------------------------------------------
CE_SHAPES = [(1, 1), (1, 2), (255, 3), (256, 2), (257, 64), (513, 5)]
CE_WEIGHTS = ("none", "random", "zero")
CE_LOGITS = ("randn", "spread1e4", "equal_block")
BAD_LABEL_SHAPE = (257, 3)
BAD_LABELS = {0: -1, 128: 3, 256: 2 ** 40}


def ce_case_list():
    return [(f"ce-{M}x{C}-w_{wk}-{lk}", (M, C), wk, lk) for (M, C) in CE_SHAPES for wk in CE_WEIGHTS for lk in CE_LOGITS]


@functools.lru_cache(maxsize=None)
def ce_inputs(shape, wk, lk):
    M, C = shape
    g = _gen(3, M, C, CE_WEIGHTS.index(wk), CE_LOGITS.index(lk))
    logits = _randn(g, M, C)
    if lk == "spread1e4":
        logits = logits * np.float32(1e4)
    elif lk == "equal_block":  # a block of rows with all logits equal
        logits[M // 3: M // 3 + max(1, M // 4)] = np.float32(1.5)
    labels = torch.randint(0, C, (M,), generator=g).numpy().astype(np.int64)
    cw = None
    if wk != "none":
        cw = (0.5 + 3.5 * torch.rand(C, generator=g)).numpy()
        if wk == "zero":
            cw[labels[0]] = 0.0  # a class of weight 0 that does occur
    return logits, labels, cw


def ce_figures(impl, case):
    cid, shape, wk, lk = case
    logits, labels, cw = ce_inputs(shape, wk, lk)
    loss, dl = H.cross_entropy(logits, labels, cw)
    gloss, gdl = impl.cross_entropy(logits, labels, cw)
    return {f"ce.loss.{lk}": rel(gloss, loss), f"ce.dlogits.{lk}": rel(gdl, dl)}


@functools.lru_cache(maxsize=None)
def ce_bad_label_inputs():
    """(logits, labels with BAD_LABELS in place, class weights, rows that keep a valid label)."""
    M, C = BAD_LABEL_SHAPE
    g = _gen(4, M, C)
    logits = _randn(g, M, C)
    labels = torch.randint(0, C, (M,), generator=g).numpy().astype(np.int64)
    cw = (0.5 + 3.5 * torch.rand(C, generator=g)).numpy()
    for r, v in BAD_LABELS.items():
        labels[r] = v
    good = np.array([r for r in range(M) if r not in BAD_LABELS])
    return logits, labels, cw, good


# ---------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------
ADAM_N = (1, 255, 257, H.ADAM_GRID_ELEMS + 1)
ADAM_KINDS = {"randn": 1.0, "x1e4": 1e4, "x1e-12": 1e-12, "zeros": 1.0}
# mode -> (first step, number of steps, beta1, beta2, eps, state)
ADAM_MODES = {"A-default": (1, 3, 0.9, 0.999, 1e-8, "zero"), "A-betas": (1, 3, 0.5, 0.9, 1e-6, "zero"),
              "B-t1000": (1000, 1, 0.9, 0.999, 1e-8, "random")}
ADAM_LR = 1e-3


def adam_zero_places(n):
    return sorted({0, n // 2, n - 1})


def adam_case_list():
    cases = [(f"adam-n{n}-{kind}-{mode}", n, kind, mode) for n in ADAM_N for kind in ADAM_KINDS for mode in ADAM_MODES]
    return cases + [("adam-n257-small_p-A-default", 257, "small_p", "A-default")]  # |p| <= 1e-3: p's rounding does not hide the step


def adam_inputs(n, kind, mode):
    """(p, [g ...], m, v, first step, beta1, beta2, eps)"""
    step, steps, b1, b2, eps, state = ADAM_MODES[mode]
    g = _gen(5, n, list(ADAM_KINDS).index(kind) if kind in ADAM_KINDS else 9, list(ADAM_MODES).index(mode))
    scale = np.float32(ADAM_KINDS.get(kind, 1.0))
    p = _randn(g, n)
    if kind == "small_p":
        p = (2e-3 * torch.rand(n, generator=g) - 1e-3).numpy().astype(np.float32)
    elif kind == "x1e-12":  # the step is lr * g / eps ~ 1e-7 here: half an ulp of a p of 1, so p is ~ 1e-6
        p = p * np.float32(1e-6)
    grads = [_randn(g, n) * scale for _ in range(steps)]
    if kind == "zeros":
        for gr in grads:
            gr[adam_zero_places(n)] = 0.0
    if state == "zero":
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m = _randn(g, n) * np.float32(0.5) * scale
        v = torch.rand(n, generator=g).numpy() * scale * scale
    return p, grads, m, v, step, b1, b2, eps


def adam_figures(impl, case):
    cid, n, kind, mode = case
    p, grads, m, v, step, b1, b2, eps = adam_inputs(n, kind, mode)
    rp, rm, rv = H.adam_steps(p, grads, m, v, step, ADAM_LR, b1, b2, eps)
    gp, gm, gv = impl.adam_steps(p, grads, m, v, step, ADAM_LR, b1, b2, eps)
    figs = {f"adam.move.{kind}": rel(H.f64(gp) - H.f64(p), rp - H.f64(p)), f"adam.m.{kind}": rel(gm, rm),
            f"adam.v.{kind}": rel(gv, rv)}
    if kind == "zeros" and ADAM_MODES[mode][5] == "zero":  # zero gradient on zero state: p, m, v keep their bits
        z = adam_zero_places(n)
        same = same_bits(np.asarray(gp)[z], p[z]) and same_bits(np.asarray(gm)[z], m[z]) and same_bits(np.asarray(gv)[z], v[z])
        figs["adam.zero_places.zeros"] = 0.0 if same else math.inf
    return figs


# ---------------------------------------------------------------------------------------------
# NT-Xent
# ---------------------------------------------------------------------------------------------
NTX_SHAPES = [(1, 1, 0.5), (2, 63, 0.07), (3, 65, 0.05), (128, 32, 0.1), (129, 32, 0.1), (37, 300, 0.07)]
NTX_VARIANT_SHAPES = [(3, 65, 0.05), (129, 32, 0.1)]
NTX_VARIANTS = ("x1e-3", "x1e3", "zj_eq_zi", "identical", "zero_row")
NTX_ZERO_ROW = 1


def ntxent_case_list():
    cases = [(f"ntxent-n{n}-d{d}-t{t}-plain", (n, d, t), "plain") for (n, d, t) in NTX_SHAPES]
    return cases + [(f"ntxent-n{n}-d{d}-t{t}-{k}", (n, d, t), k) for (n, d, t) in NTX_VARIANT_SHAPES for k in NTX_VARIANTS]


@functools.lru_cache(maxsize=None)
def ntxent_inputs(shape, kind):
    n, d, t = shape
    g = _gen(6, n, d)
    zi = _randn(g, n, d) * np.float32(1.7)
    # weakly correlated views: with strongly correlated ones the small, cold cases (n = 3 at t = 0.05) have a loss of 1e-6
    # left over from terms of 10, and float32 itself is 1e-2 off there
    zj = zi * np.float32(0.1) + _randn(g, n, d)
    if kind == "x1e-3":
        zi, zj = zi * np.float32(1e-3), zj * np.float32(1e-3)
    elif kind == "x1e3":
        zi, zj = zi * np.float32(1e3), zj * np.float32(1e3)
    elif kind == "zj_eq_zi":
        zj = zi.copy()
    elif kind == "identical":  # two samples identical, in both views
        zi[1], zj[1] = zi[0], zj[0]
    z = np.concatenate([zi, zj]).astype(np.float32)
    if kind == "zero_row":  # takes the max(|z|, 1e-12) clamp; its gradient is about g * 1e12, and finite
        z[NTX_ZERO_ROW] = 0.0
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def ntxent_reference(shape, kind):
    return H.ntxent(ntxent_inputs(shape, kind), shape[2])


def ntxent_figures(impl, case, got=None):
    cid, shape, kind = case
    z = ntxent_inputs(shape, kind)
    loss, dz = ntxent_reference(shape, kind)
    gloss, gdz = got if got is not None else impl.ntxent(z, shape[2], True)
    figs = {f"ntxent.loss.{kind}": rel(gloss, loss)}
    if kind == "zero_row":  # that row against its own maximum, the others among themselves: 1e12 would swamp the max-norm
        others = np.arange(z.shape[0]) != NTX_ZERO_ROW
        figs["ntxent.dz_zero_row.zero_row"] = rel(np.asarray(gdz)[NTX_ZERO_ROW], dz[NTX_ZERO_ROW])
        figs["ntxent.dz_rest.zero_row"] = rel(np.asarray(gdz)[others], dz[others])
    else:
        figs[f"ntxent.dz.{kind}"] = rel(gdz, dz)
    return figs


# ---------------------------------------------------------------------------------------------
# gates
# ---------------------------------------------------------------------------------------------
FIGURES = {"ce": (ce_case_list, ce_figures), "adam": (adam_case_list, adam_figures), "ntxent": (ntxent_case_list, ntxent_figures)}


def measure(log=None):
    """The float32 stand-in's distances from the float64 references on every case, and the largest per group."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # one summation order whatever the machine's core count
    try:
        impl = H.StandIn()
        out = {"factor": FACTOR, "how": HOW, "cases": {}, "per_group": {}}
        for prim, (case_list, figures) in FIGURES.items():
            for case in case_list():
                figs = figures(impl, case)
                out["cases"][case[0]] = figs
                for k, v in figs.items():
                    out["per_group"][k] = max(out["per_group"].get(k, 0.0), v)
                if log:
                    log(case[0] + ": " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
        return out
    finally:
        torch.set_num_threads(threads)


@functools.lru_cache(maxsize=None)
def recorded():
    with open(JSON_PATH) as f:
        return json.load(f)


def gate(key):
    return FACTOR * recorded()["per_group"][key]


def over_gate(tag, figs, log=print):
    """Prints every figure next to its gate; returns the (key, figure, gate) that exceed theirs."""
    bad = []
    for k, v in figs.items():
        g = gate(k)
        log(f"[head] {tag}: {k} {v:.2e} / gate {g:.2e}")
        if not v <= g:
            bad.append((k, v, g))
    return bad

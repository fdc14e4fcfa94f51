"""Oracle: the inference trunk of the C ABI (csrc/trunk.h, precisions bf16 / fp16 / fp32) restated BLOCK BY BLOCK in torch
float64 on the CPU, from given maps.

TEST INFRASTRUCTURE (see oracle/__init__.py).  tests/test_gpu_resnet*.py compare the device with the fp32 oracle end to
end, one number per tensor, at 2.5e-2 / 3e-2 (bf16) because 16-bit rounding accumulates through 20 layers.  Here every
stage is recomputed FROM THE DEVICE'S OWN INPUT MAP (``PackedResNet18.tap``), with the device's folded and quantised
weights, so that one rounding lies between the given input and the checked output and the bound can be derived per
element; no element is left out.  Pinned on torch itself by tests/test_oracle_infer_replay.py, run against the device by
tests/test_gpu_infer_replay.py.

``storage`` is None, torch.bfloat16, torch.float16 or torch.float32: the element type T of the device's maps and
weights.  "rnd" is RNE to T through torch (``.to(storage)``; nothing for None).  e = 2^-24.

fp16x3 and fp16q8 are not replayed here but in oracle/pair_replay.py.  Their block error is not one rounding of a stored value
(the lo x lo product is dropped; fp16q8 runs e4m3 cross products with fixed scales) and they run other kernels (halo16x2.h), so
that module works differently: CONV BY CONV instead of block by block (their inner maps can be fetched), from the RAW stored
planes (fp16 pairs, e4m3 bytes) with the weights restated from the state dict, and against a gate of 10 x the measured distance
of a float32 stand-in instead of a derived worst case -- (K + 2) e S is wider than every fault in their 2^-11 machinery.

Rounding sites of the inference driver, read off csrc/resnet_pack.hip, trunk.h, resnet_forward.hip and the kernels'
epilogues (everything else is fp32 arithmetic on the device and float64 here):
  weights   pack_conv               scale = gamma / sqrt((double)var + (double)eps) in double (eps crosses the ABI as a float);
                                    w' = (float)((double)w * scale), then RNE to T (nothing more for fp32);
                                    bias = (float)(beta - mean * scale)
            pack_net                folded-projection blocks (bf16 / fp16, HIPAC_PROJK=1): bias_c2p = (float)b2 + (float)bp,
                                    added in float
            pack_stem_u8            rw = rnd((float)(w * scale / (255 std_c))); table[row class][column class][o] =
                                    (float)(b0 + sum over the 147 taps of (tap inside the image ? rw (128 - 255 mean_c) : 128 rw)),
                                    summed in double; class 0 interior, 1: stem row / column 0 (taps 0-2 outside), 2: row /
                                    column 1 (tap 0), 3: row / column 111 (taps 5, 6)
            pack_net (lut_t)        rnd of the fp32 table (v / 255 - mean_c) / std_c, evaluated in fp32 in that order
  stem      strip kernel            (uint8 input, default) fp32 sum of rw (v - 128), bytes outside the image counted as 0, on
                                    top of the table entry of the pixel's classes = b0 + sum over the taps inside of
                                    rw (v - 255 mean_c); no rounding of the input; max over rows in fp32, ONE rounding to T,
                                    max over columns and ReLU on T values
            tile kernel             input rnd(lut[v]) (uint8, HIPAC_STEM_STRIP=0) or rnd(x) (launch_nchw_to_nhwc4); fp32 sum +
                                    bias, ReLU, ONE rounding to T into LDS; the pool takes maxima of T values
            unfused                 (HIPAC_FUSE_STEM=0, always in fp32 mode) the same stem conv, its map stored as T (tap 0),
                                    maxpool3x3s2_kernel: exact
            A maximum of T values is a T value and rounding is monotone, so every form has exactly one rounding between
            the input and the pooled map.
  block     conv1                   + bias, ReLU -> the INNER map, rounded to T.  layer1's fused block (block16_c64.h) keeps
                                    it in LDS, the other blocks in tmp_e / tmp_l; it has no tap either way
            conv2                   + bias + shortcut, ReLU -> the output, rounded to T.  Shortcut: the block input
                                    (exact); or the 1x1 / 2 projection summed IN conv2's accumulator with bias_c2p (layers
                                    2-4 of bf16 / fp16 by default: no rounding of its own); or a projection MAP rounded to T
                                    (HIPAC_PROJK=0: launch_down in layers 2-3, its own launch in layer 4; always in fp32 mode)
            last block              the output is the fp32 accumulator (OUTF32): no rounding to T
  head      halo16.h POOL           (bf16 / fp16, default) every value of the last map is split v = hi + lo + r, hi on the
                                    grid 2^-10, lo on the grid 2^-29, |r| <= 2^-30 DROPPED; the sums of hi and of lo are
                                    exact in fp32 while sum(hi) < 2^14 and v < 2^12; features = (sum hi + sum lo) / 49
                                    (head_pool_kernel).  The tap of the last map re-runs the last conv with its fp32-map
                                    epilogue: the same accumulators
            head_kernel             (fp32 mode, HIPAC_POOL_HEAD=0) fp32 sum of the 49 values in order, / 49
            head_tail               fc: an fp32 sum of 512 products plus the bias, fp32 weights
Maps are NCHW float64 tensors whatever the device's layout is.

THE BLOCK CHECK.  The inner map has no tap, and the device's fp32 sum may round an inner element to the neighbour of what
float64 rounds it to.  So the bound is an interval, derived and not tuned:
    a   = conv(X, W1) + b1                    S1 = conv(|X|, |W1|) + |b1|          A = (K1 + 1) e S1
    t_lo, t_ref, t_hi = rnd(relu(a - A)), rnd(relu(a)), rnd(relu(a + A))           D1 = t_hi - t_lo  (>= 0, almost everywhere 0)
    o   = conv(t_ref, W2) + b2 + shortcut(X)
    B   = conv(D1, |W2|) + (K2 + 2) e (conv(t_hi, |W2|) + |b2| + |shortcut terms|)   [+ P_hi - P_lo for a rounded projection map]
    pass:  rnd(relu(o - B)) <= dev_out <= rnd(relu(o + B))                         for every element
K1 = 9 cin, K2 = 9 cout (+ cin when the projection rides in the accumulator: its products then count in the magnitude
sum).  The device's inner element lies in [t_lo, t_hi] (its fp32 sum is within A of a, rounding and ReLU are monotone), so
its conv2 sum is within conv(D1, |W2|) of the replay's, and its fp32 accumulation within (K + 2) e of the magnitude sum.
A rounded projection map is treated like the inner map: p = conv1x1(X, Wp) + bp, P = rnd(p -+ (cin + 1) e Sp).

Every stage returns a dict:
    ratio   ASSERTED <= 1.  |dev - middle| / half-width of the stage's interval, worst element; an element outside an
            interval of width 0 gives inf.  For the stages with a symmetric bound this is |dev - ref| / bound.
    fig     reported.  |dev - ref| / bound.  Block: the bound is half the interval's width, clamped below by one rounding of
            relu(o) -- 0.5 on average for a correctly rounded 16-bit map, ~1 for the neighbouring value.
    sqrtk   reported, not asserted.  K e S is the worst case of an fp32 sum in any order; at K = 4608 it is about one
            average product.  The finer figure: the part of |dev - ref| that neither the rounding cell of the device's
            value (half a unit in its last place) nor the D terms explain, in units of sqrt(K) e S.
    n_out   elements outside the interval;  worst = index of the worst element.
    msq     blocks only, ASSERTED <= ``msq_gate(msq_n)``.  The interval is a worst case, and a worst case cannot see an error
            of the size of the rounding noise itself: an inner map left UNROUNDED moves an output by about a third of a unit
            in its last place, a block output rounded TOWARDS ZERO by half a unit, and where K1 e S1 reaches the spacing of T
            (fp16 from layer1 on, bf16 in layers 3-4) nearly every inner element may round either way, so that the interval
            is units wide.  Such errors show in the mean square: over the msq_n elements the ReLU cannot clip (lo > 0),
                msq = mean( (dev - relu(o))^2 / (h^2 / 3 + unit^2) ),
            h = half a unit in the last place of dev (a correct rounding's error is uniform over its cell: variance h^2 / 3)
            and unit = sqrt(K) e S + the inner map's typical error carried through conv2 in quadrature -- per inner element
            q = sqrt(K1) e S1 where T is finer than q, and a whole unit of T with probability q / unit where it is coarser
            (``_noise_var``).  unit is an upper estimate of the typical error (e for e / sqrt(3), S for the partial sums), so a
            correct device stays below 1; the gate adds six standard deviations of the mean.  Measured on the float32
            stand-in: 0.83 - 0.92 (bf16), 0.46 - 0.75 (fp16); with an unrounded inner map 2.8 - 4.4 (bf16), 1.16 - 1.48 (fp16,
            layers 1 - 2; from layer3 on the fault is no larger than the modelled noise of fp16: 0.97, 0.62), rounded towards
            zero 1.8 - 3.6.

The convolutions of MAGNITUDES (S, D) are evaluated in float32 and scaled by 1 + 2^-10 (``_mag``): their own error is below
2^-11 of the result, so they stay upper bounds.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

from .resnet18_ref import BN_EPS
from .train_replay import EPS32, pool_windows
from .transform_ref import IMAGENET_MEAN, IMAGENET_STD

BLOCKS = tuple(f"layer{s}.{b}" for s in (1, 2, 3, 4) for b in (0, 1))
STORAGE = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
_U = {None: 0.0, torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
_HALF_SUB = {None: 0.0, torch.float32: 2.0 ** -150, torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134}
_PREC_EMIN = {torch.float32: (24, -126), torch.float16: (11, -14), torch.bfloat16: (8, -126)}
STEM_FORMS = ("u8_strip", "u8_table", "nchw_f32")


def rnd(t: torch.Tensor, storage) -> torch.Tensor:
    return t if storage is None else t.to(storage).to(torch.float64)


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.float64)


def rounding_bound(ref: torch.Tensor, storage) -> torch.Tensor:
    """The error of ONE rounding of ``ref`` to storage: u |ref|, and half the spacing of the subnormals below that."""
    return (_U[storage] * ref.abs()).clamp_min(_HALF_SUB[storage])


def _cell_half(dev: torch.Tensor, storage) -> torch.Tensor:
    """Half a unit in the last place of the T value ``dev``: what a correct rounding to ``dev`` can hide."""
    if storage is None:
        return torch.zeros_like(dev)
    p, emin = _PREC_EMIN[storage]
    _, ex = torch.frexp(dev.abs())
    e = torch.where(dev == 0, torch.full_like(ex, emin), (ex - 1).clamp_min(emin))
    return torch.ldexp(torch.ones_like(dev), e - p)


def _conv(x, w, stride=1):
    return F.conv2d(x, w, None, stride=stride, padding=w.shape[-1] // 2)


def _mag(x, w, stride=1, padding=None):
    """A convolution of magnitudes, for a bound: in float32 (many times faster than float64 on the CPU; its own error is below
    K e < 2^-11 of the result) and scaled by 1 + 2^-10, so that it stays an upper bound of the exact sum."""
    pad = w.shape[-1] // 2 if padding is None else padding
    return F.conv2d(x.to(torch.float32), w.to(torch.float32), None, stride=stride, padding=pad).to(torch.float64) * (1.0 + 2.0 ** -10)


def _bv(b):
    return b.view(1, -1, 1, 1)


# ---------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------
def strip_table(rw: torch.Tensor, b0: torch.Tensor) -> torch.Tensor:
    """The strip stem's bias table [4][4][64] in float64, exactly as pack_stem_u8 builds it from the rounded weights ``rw``
    [64,3,7,7] and the folded bias ``b0``: a tap inside the image adds rw (128 - 255 mean_c), a tap outside 128 rw."""
    k = torch.arange(7)
    out = torch.stack([k < 0, k <= 2, k == 0, k >= 5])  # [class][tap]: the tap falls outside the image
    inside = (~out).view(4, 1, 7, 1) & (~out).view(1, 4, 1, 7)  # [row class][column class][kh][kw]
    mu = 255.0 * torch.tensor(IMAGENET_MEAN, dtype=torch.float64)
    coef = 128.0 - inside.to(torch.float64).view(4, 4, 1, 7, 7) * mu.view(1, 1, 3, 1, 1)
    return b0.view(1, 1, -1) + torch.einsum("ochw,rschw->rso", rw, coef)


def fold(sd: Dict[str, torch.Tensor], storage, eps: float = BN_EPS) -> dict:
    """The device's weights as float64 tensors: {"stem": {w, b}, "stem_u8": {rw, tab}, "layerS.B": {w1, b1, w2, b2[, wp, bp,
    bias_c2p]}, "fc": {w, b}} -- weights quantised to ``storage``, biases and the table float32 values (all unrounded
    float64 for storage None)."""
    e = eps if storage is None else float(torch.tensor(eps, dtype=torch.float32))
    f32 = (lambda t: t) if storage is None else _f32
    q = (lambda t: t) if storage is None else (lambda t: t.to(torch.float32).to(storage).to(torch.float64))

    def cb(conv, bn):
        scale = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + e)
        return sd[conv + ".weight"].double() * scale.view(-1, 1, 1, 1), sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * scale

    out: dict = {}
    w, b = cb("conv1", "bn1")
    out["stem"] = dict(w=q(w), b=f32(b))
    std = torch.tensor(IMAGENET_STD, dtype=torch.float64).view(1, 3, 1, 1)
    rw = q(w / (255.0 * std))
    out["stem_u8"] = dict(rw=rw, tab=f32(strip_table(rw, b)))
    for name in BLOCKS:
        w1, b1 = cb(name + ".conv1", name + ".bn1")
        w2, b2 = cb(name + ".conv2", name + ".bn2")
        blk = dict(w1=q(w1), b1=f32(b1), w2=q(w2), b2=f32(b2))
        if (name + ".downsample.0.weight") in sd:
            wp, bp = cb(name + ".downsample.0", name + ".downsample.1")
            blk.update(wp=q(wp), bp=f32(bp), bias_c2p=f32(f32(b2) + f32(bp)))
        out[name] = blk
    if "fc.weight" in sd:
        out["fc"] = dict(w=sd["fc.weight"].double(), b=sd["fc.bias"].double())
    return out


def normalize_lut(storage) -> torch.Tensor:
    """[3,256] float64: the device's table of ToTensor + Normalize, evaluated in fp32 in torchvision's order and rounded to
    storage (pack_net); exact in float64 for storage None."""
    wd = torch.float64 if storage is None else torch.float32
    v = torch.arange(256, dtype=wd) / torch.tensor(255.0, dtype=wd)
    lut = (v.view(1, -1) - torch.tensor(IMAGENET_MEAN, dtype=wd).view(3, 1)) / torch.tensor(IMAGENET_STD, dtype=wd).view(3, 1)
    return rnd(lut.to(torch.float64), storage)


# ---------------------------------------------------------------------------------------------------------------------
# stages
# ---------------------------------------------------------------------------------------------------------------------
def replay_stem(form: str, inp: torch.Tensor, Fd: dict, storage):
    """The stem conv + bias BEFORE ReLU and rounding, in float64, for every stem form -> (a [B,64,112,112], S = the sum of
    the magnitudes the device adds, K = 147).  ``inp``: uint8 [B,224,224,3] for "u8_strip" / "u8_table", float [B,3,224,224]
    for "nchw_f32"."""
    if form == "u8_strip":
        rw, tab = Fd["stem_u8"]["rw"], Fd["stem_u8"]["tab"]
        c = F.pad(inp.permute(0, 3, 1, 2).to(torch.float64) - 128.0, (3, 3, 3, 3), value=-128.0)  # bytes outside arrive as 0
        cls = torch.zeros(112, dtype=torch.long)
        cls[0], cls[1], cls[111] = 1, 2, 3
        t = tab[cls][:, cls].permute(2, 0, 1).unsqueeze(0)  # [1,64,112,112]: the entry of (row class, column class)
        return F.conv2d(c, rw, None, stride=2) + t, _mag(c.abs(), rw.abs(), 2, 0) + t.abs(), 147
    if form == "u8_table":
        lut = normalize_lut(storage)
        v = inp.permute(0, 3, 1, 2).long()
        x = torch.stack([lut[ch][v[:, ch]] for ch in range(3)], dim=1)
    elif form == "nchw_f32":
        x = rnd(inp.to(torch.float64), storage)
    else:
        raise ValueError(form)
    w, b = Fd["stem"]["w"], Fd["stem"]["b"]
    return _conv(x, w, 2) + _bv(b), _mag(x.abs(), w.abs(), 2) + _bv(b.abs()), 147


def _max_pool(t: torch.Tensor) -> torch.Tensor:
    return pool_windows(t).max(dim=2).values


def msq_gate(n: int) -> float:
    """1 + 6 standard deviations of a mean of n terms x^2 / var(x) (relative deviation sqrt(2) each, the Gaussian's; a uniform
    rounding error has 0.9)."""
    return 1.0 + 6.0 * math.sqrt(2.0 / max(n, 1))


def _stage(dev, ref, lo, hi, fig_bound, unit, storage, stat_mask=None) -> dict:
    """One stage's figures (module docstring) from the interval [lo, hi] every element of ``dev`` must lie in."""
    dev = dev.to(torch.float64)
    half, mid = (hi - lo) / 2, (hi + lo) / 2
    outside = (dev < lo) | (dev > hi)
    d = (dev - mid).abs()
    r = torch.where(half > 0, d / half.clamp_min(1e-300), torch.where(outside, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    n_out = int(outside.sum())
    ratio = float(r.max())
    ratio = max(ratio, math.nextafter(1.0, 2.0)) if n_out else min(ratio, 1.0)
    err = (dev - ref).abs()
    fig = torch.where(fig_bound > 0, err / fig_bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    unexplained = (err - _cell_half(dev, storage)).clamp_min(0)
    sq = torch.where(unit > 0, unexplained / unit.clamp_min(1e-300), torch.where(unexplained > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = tuple(int(i) for i in torch.unravel_index(torch.argmax(torch.where(outside, r + 1e300, r)), r.shape))
    out = dict(ratio=ratio, fig=float(fig.max()), sqrtk=float(sq.max()), n_out=n_out, worst=worst)
    if stat_mask is not None:
        var = _cell_half(dev, storage) ** 2 / 3 + unit ** 2  # a rounding error uniform over its cell + the typical fp32 sum error
        m = stat_mask & (var > 0)
        out["msq_n"] = int(m.sum())
        out["msq"] = float((err[m] ** 2 / var[m]).mean()) if out["msq_n"] else 0.0
    return out


def check_stem(form: str, inp, Fd: dict, storage, pool_dev, stem_dev=None) -> Dict[str, dict]:
    """The stem against its float64 replay, u |ref| + (K + 2) e S per element.  With the stem map ``stem_dev`` (unfused forms):
    {"stem": that bound, "pool": the pooled map against the window maxima of the GIVEN stem map, ratio 0 if bit-equal, else
    1 + the number of differing elements}.  Without (fused): {"stem_pool": the pooled map against the window maxima of the
    replayed map; |max a_i - max b_i| <= max |a_i - b_i|, so the bound is the largest bound of the window}."""
    a, S, K = replay_stem(form, inp, Fd, storage)
    ref = a.clamp_min(0)
    bound = rounding_bound(ref, storage) + (K + 2) * EPS32 * S
    if stem_dev is not None:
        stem_dev, pool_dev = stem_dev.to(torch.float64), pool_dev.to(torch.float64)
        n = int((pool_dev != _max_pool(stem_dev)).sum())
        return {"stem": _stage(stem_dev, ref, ref - bound, ref + bound, bound, math.sqrt(K) * EPS32 * S, storage),
                "pool": dict(ratio=0.0 if n == 0 else 1.0 + n, fig=float(n), sqrtk=0.0, n_out=n, worst=())}
    pref = _max_pool(ref)
    pbound = pool_windows(bound).nan_to_num(neginf=0.0).max(dim=2).values
    pS = pool_windows(S).nan_to_num(neginf=0.0).max(dim=2).values
    return {"stem_pool": _stage(pool_dev, pref, pref - pbound, pref + pbound, pbound, math.sqrt(K) * EPS32 * pS, storage)}


def block_kind(name: str, storage, projk: bool = True) -> str:
    """The shortcut of block ``name``: "identity", "projk" (projection in conv2's accumulator) or "proj_map" (rounded map)."""
    if not name.endswith(".0") or name == "layer1.0":
        return "identity"
    return "projk" if projk and storage in (torch.bfloat16, torch.float16) else "proj_map"


def _noise_var(q, ref, storage):
    """The variance an fp32 sum's typical error ``q`` leaves in a value stored as T: q^2 where the format is finer than q; where
    it is coarser the stored value moves by a whole unit in the last place with probability q / unit."""
    return q * torch.maximum(q, 2 * _cell_half(ref, storage))


def _inner(X, w, stride, storage):
    a = _conv(X, w["w1"], stride) + _bv(w["b1"])
    S1 = _mag(X.abs(), w["w1"].abs(), stride) + _bv(w["b1"].abs())
    K1 = 9 * w["w1"].shape[1]
    A = (K1 + 1) * EPS32 * S1
    t_lo, t_ref, t_hi = rnd((a - A).clamp_min(0), storage), rnd(a.clamp_min(0), storage), rnd((a + A).clamp_min(0), storage)
    var = _noise_var(math.sqrt(K1) * EPS32 * S1, t_ref, storage) * (t_hi > 0)
    return t_lo, t_ref, t_hi, var


def check_block(X, dev_out, w: dict, kind: str, storage, last: bool = False) -> dict:
    """One BasicBlock from its given input map ``X`` [B,cin,H,H]: the interval check of the module docstring on ``dev_out``.
    ``w``: the block's entry of ``fold``; ``last``: the network's last block, whose output is the fp32 accumulator."""
    X = X.to(torch.float64)
    stride = 1 if kind == "identity" else 2
    cin, cout = w["w1"].shape[1], w["w1"].shape[0]
    t_lo, t_ref, t_hi, var = _inner(X, w, stride, storage)
    W2a = w["w2"].abs()
    o, S2, D = _conv(t_ref, w["w2"]), _mag(t_hi, W2a), _mag(t_hi - t_lo, W2a)
    var = _mag(var, W2a * W2a)  # the inner map's typical error, carried through conv2 in quadrature
    K = 9 * cout
    if kind == "identity":
        o, S2 = o + _bv(w["b2"]) + X, S2 + _bv(w["b2"].abs()) + X.abs()
    elif kind == "projk":
        o, S2 = o + _conv(X, w["wp"], 2) + _bv(w["bias_c2p"]), S2 + _mag(X.abs(), w["wp"].abs(), 2) + _bv(w["bias_c2p"].abs())
        K += cin
    elif kind == "proj_map":
        p, Sp = _conv(X, w["wp"], 2) + _bv(w["bp"]), _mag(X.abs(), w["wp"].abs(), 2) + _bv(w["bp"].abs())
        Ap = (cin + 1) * EPS32 * Sp
        P_lo, P_ref, P_hi = rnd(p - Ap, storage), rnd(p, storage), rnd(p + Ap, storage)
        o, S2, D = o + _bv(w["b2"]) + P_ref, S2 + _bv(w["b2"].abs()) + torch.maximum(P_lo.abs(), P_hi.abs()), D + (P_hi - P_lo)
        var = var + _noise_var(math.sqrt(cin) * EPS32 * Sp, P_ref, storage)
    else:
        raise ValueError(kind)
    B = D + (K + 2) * EPS32 * S2
    st_out = None if last else storage
    lo, hi, ref = rnd((o - B).clamp_min(0), st_out), rnd((o + B).clamp_min(0), st_out), o.clamp_min(0)
    fig_bound = torch.maximum((hi - lo) / 2, rounding_bound(ref, st_out))
    return _stage(dev_out, ref, lo, hi, fig_bound, math.sqrt(K) * EPS32 * S2 + torch.sqrt(var), st_out, stat_mask=lo > 0)


def check_head(tap9, feats, logits, fc: Optional[dict], pool_head: bool) -> Dict[str, dict]:
    """The features against the float64 mean of the GIVEN last map ``tap9`` [B,512,7,7]: 2^-30 + 3 e |mean| for the split-sum
    head (``pool_head``; its exactness precondition is asserted, not assumed), 50 e mean|v| for head_kernel.  The logits
    against the fc of the GIVEN features: 514 e (sum |f w| + |b|)."""
    v, f = tap9.to(torch.float64), feats.to(torch.float64)
    mean, mabs = v.mean(dim=(2, 3)), v.abs().mean(dim=(2, 3))
    if pool_head:
        hi_sum = (torch.round(v * 1024.0) / 1024.0).sum(dim=(2, 3))
        assert float(hi_sum.max()) < 2.0 ** 14 and float(v.max()) < 2.0 ** 12 and float(v.min()) >= 0.0, \
            "the split sums of halo16.h (POOL) are exact only while sum(hi) < 2^14: the last map leaves that range"
        bound = 2.0 ** -30 + 3 * EPS32 * mean.abs()
    else:
        bound = 50 * EPS32 * mabs
    out = {"feats": _stage(f, mean, mean - bound, mean + bound, bound, 7 * EPS32 * mabs + (2.0 ** -30 if pool_head else 0.0), None)}
    if logits is not None:
        ref = f @ fc["w"].t() + fc["b"]
        S = f.abs() @ fc["w"].abs().t() + fc["b"].abs()
        bound = 514 * EPS32 * S
        out["logits"] = _stage(logits.to(torch.float64), ref, ref - bound, ref + bound, bound, math.sqrt(512) * EPS32 * S, None)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# drivers
# ---------------------------------------------------------------------------------------------------------------------
def check_forward(dev: dict, Fd: dict, storage, stem: str = "u8_strip", projk: bool = True, pool_head: bool = True) -> Dict[str, dict]:
    """Every stage of one forward from the device's own maps.  ``dev``: "input" (``replay_stem``'s ``inp``), "pool"
    [B,64,56,56], optional "stem" [B,64,112,112] (the unfused forms), "blocks" (the eight block outputs), "feats" [B,512],
    optional "logits".  ``stem`` / ``projk`` / ``pool_head``: the forms the device ran (fp32 mode has neither a folded
    projection nor the split-sum head).  -> {stage: figures}."""
    if storage == torch.float32:
        projk = pool_head = False
    out = dict(check_stem(stem, dev["input"], Fd, storage, dev["pool"], dev.get("stem")))
    X = dev["pool"]
    for i, name in enumerate(BLOCKS):
        out[name] = check_block(X, dev["blocks"][i], Fd[name], block_kind(name, storage, projk), storage, last=i == 7)
        X = dev["blocks"][i]
    out.update(check_head(dev["blocks"][7], dev["feats"], dev.get("logits"), Fd.get("fc"), pool_head))
    return out


def slice_image(dev: dict, i: int) -> dict:
    return {k: ([t[i:i + 1] for t in v] if isinstance(v, (list, tuple)) else v[i:i + 1]) for k, v in dev.items() if v is not None}


def check_images(dev: dict, images: Sequence[int], Fd: dict, storage, **forms) -> Dict[str, dict]:
    """``check_forward`` image by image (the replay is per image; this bounds its memory) over ``images`` of the batch ``dev``
    holds; per stage the worst image's figures (n_out summed), its "worst" index led by the image's number."""
    merged: Dict[str, dict] = {}
    for i in images:
        for stage, r in check_forward(slice_image(dev, i), Fd, storage, **forms).items():
            r = dict(r, worst=(i,) + tuple(r["worst"][1:]))
            m = merged.get(stage)
            if m is None:
                merged[stage] = r
                continue
            n_out = m["n_out"] + r["n_out"]
            best = r if r["ratio"] > m["ratio"] else m
            merged[stage] = dict(ratio=best["ratio"], fig=max(m["fig"], r["fig"]), sqrtk=max(m["sqrtk"], r["sqrtk"]), n_out=n_out, worst=best["worst"])
            if "msq" in r:
                n = m["msq_n"] + r["msq_n"]
                merged[stage].update(msq_n=n, msq=(m["msq"] * m["msq_n"] + r["msq"] * r["msq_n"]) / max(n, 1))
    return merged


def replay_forward(inp, Fd: dict, storage, stem: str = "u8_strip", projk: bool = True) -> dict:
    """The whole forward CHAINED from the input in float64 with the roundings of the module docstring (none for storage None):
    {"stem", "pool", "blocks": [8], "feats", "logits"}.  The projection is summed unrounded (``projk``) or as a rounded map."""
    a, _, _ = replay_stem(stem, inp, Fd, storage)
    maps = {"stem": rnd(a.clamp_min(0), storage)}
    X = maps["pool"] = _max_pool(maps["stem"])
    maps["blocks"] = []
    for i, name in enumerate(BLOCKS):
        w, kind = Fd[name], block_kind(name, storage, projk)
        t = rnd((_conv(X, w["w1"], 1 if kind == "identity" else 2) + _bv(w["b1"])).clamp_min(0), storage)
        o = _conv(t, w["w2"])
        if kind == "identity":
            o = o + _bv(w["b2"]) + X
        elif kind == "projk":
            o = o + _conv(X, w["wp"], 2) + _bv(w["bias_c2p"])
        else:
            o = o + _bv(w["b2"]) + rnd(_conv(X, w["wp"], 2) + _bv(w["bp"]), storage)
        X = rnd(o.clamp_min(0), None if i == 7 else storage)
        maps["blocks"].append(X)
    maps["feats"] = X.mean(dim=(2, 3))
    if "fc" in Fd:
        maps["logits"] = maps["feats"] @ Fd["fc"]["w"].t() + Fd["fc"]["b"]
    return maps


def summary(results: Dict[str, dict]) -> str:
    """One line per stage for the tests' output."""
    return "\n".join(f"  {s:10s} ratio {r['ratio']:.3f}  fig {r['fig']:.3g}  sqrtK {r['sqrtk']:.3g}  outside {r['n_out']}  worst {r['worst']}"
                     + (f"  msq {r['msq']:.3f} (gate {msq_gate(r['msq_n']):.3f})" if "msq" in r else "") for s, r in results.items())


def failures(results: Dict[str, dict]) -> List[str]:
    bad = [f"{s}: {r['n_out']} elements outside, worst ratio {r['ratio']:.3g} at (image, channel, row, column) = {r['worst']}"
           for s, r in results.items() if not r["ratio"] <= 1.0]
    return bad + [f"{s}: mean square error {r['msq']:.3f} of the model's over {r['msq_n']} elements, gate {msq_gate(r['msq_n']):.3f}"
                  for s, r in results.items() if "msq" in r and not r["msq"] <= msq_gate(r["msq_n"])]

"""Oracle: the native train-mode encoder step (csrc/train_common.h) restated STAGE BY STAGE in torch on the CPU.

TEST INFRASTRUCTURE (see oracle/__init__.py).  Unlike oracle/train_ref.py -- one independent autograd graph of the
whole step -- this module replays the driver one kernel at a time FROM GIVEN MAPS (the device's own, read through
``NativeEncoder.tap``), in float64, and rounds to the type of the maps exactly where the device stores one.  A forward
stage then has one rounding between its input and its output, so its error bound can be derived
(``check_forward_stages``); the backward needs no ReLU pattern handed over, because the masks ARE the given maps
(``replay_backward``).  Pinned on torch itself by tests/test_oracle_train_replay.py.

``storage`` is None, torch.float32 or torch.float16: the element type T of the device's maps.  "Round to storage"
is ``.to(storage).to(float64)`` (nothing for None).

Rounding sites of the driver, read off csrc/train_kernels.h and the conv kernels (everything else is fp32 / fp64
arithmetic on the device and float64 here):
  forward   launch_nchw_to_nhwc4          x -> T                      (the stem's input)
            pack_w_kernel                 (T)w[gid]                   every conv weight, modes 0 / 2
            conv kernels                  one rounding of the fp32 accumulator -> pre[i]
            bn_sum_parts_kernel<true>     mean, rstd -> float32       (biased variance; float64 sums)
            bn_apply_kernel               stv(y)                      -> post[i]
            maxpool_idx_kernel            stv(out)                    exact: a maximum of T values is a T value
            avgpool_kernel                feats are float32, not T
  backward  avgpool_bwd_kernel            (T)(dfeats * (1.0f / 49.0f))  the product is an fp32 product
            bn_bwd_apply_kernel           stv(dx); d gamma, d beta = (float) of the float64 sums
            pack_w_kernel                 (T)w[gid]                   modes 1 / 3 (data-gradient weights)
            conv kernels (data gradient)  one rounding of the fp32 accumulator, per parity class for stride 2
            add_mask_kernel               stv(out) of (a + b) masked
            maxpool_bwd_kernel            stv(din) of the sum of <= 4 window gradients
            wgrad kernels / wgrad_reduce  fp32 partials and sums: NOT rounded to T
Conv order, geometry and names: ``CONVS`` below = ``train_native.conv_table()`` (checked by the test on a machine
that can load the library).  Maps are NCHW float64 tensors whatever the device's layout is.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from .resnet18_ref import BN_EPS, STAGES

BN_MOMENTUM = 0.1
EPS32 = 2.0 ** -24


def _table() -> List[dict]:
    t = [dict(conv="conv1", bn="bn1", cout=64, cin=3, ks=7, stride=2, hin=224, hout=112)]
    h, cin = 56, 64
    for s, (name, c, stride) in enumerate(STAGES):
        ho = h // stride
        t.append(dict(conv=f"{name}.0.conv1", bn=f"{name}.0.bn1", cout=c, cin=cin, ks=3, stride=stride, hin=h, hout=ho))
        t.append(dict(conv=f"{name}.0.conv2", bn=f"{name}.0.bn2", cout=c, cin=c, ks=3, stride=1, hin=ho, hout=ho))
        if s > 0:
            t.append(dict(conv=f"{name}.0.downsample.0", bn=f"{name}.0.downsample.1", cout=c, cin=cin, ks=1, stride=stride, hin=h, hout=ho))
        t.append(dict(conv=f"{name}.1.conv1", bn=f"{name}.1.bn1", cout=c, cin=c, ks=3, stride=1, hin=ho, hout=ho))
        t.append(dict(conv=f"{name}.1.conv2", bn=f"{name}.1.bn2", cout=c, cin=c, ks=3, stride=1, hin=ho, hout=ho))
        h, cin = ho, c
    return t


CONVS = _table()
# blocks in forward order: (conv1, conv2, projection or -1, conv2 of the previous block or -1 for the pooled map)
BLOCKS = ((1, 2, -1, -1), (3, 4, -1, 2), (5, 6, 7, 4), (8, 9, -1, 6), (10, 11, 12, 9), (13, 14, -1, 11), (15, 16, 17, 14),
          (18, 19, -1, 16))


def unit_roundoff(storage) -> float:
    return {None: 0.0, torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11}[storage]


def rounding_bound(ref: torch.Tensor, storage) -> torch.Tensor:
    """The error of ONE rounding of ``ref`` to storage: u |ref| where the format is normal, and half the spacing of its
    subnormals (2^-25 for float16, 2^-150 for float32) below that -- there the spacing no longer shrinks with |ref|, and
    u |ref| alone is not a bound that a correctly rounded float16 map can meet (a ReLU output of 3e-5 is stored with an
    error of up to 3e-8, a thousandth of its value)."""
    half_sub = {None: 0.0, torch.float32: 2.0 ** -150, torch.float16: 2.0 ** -25}[storage]
    return (unit_roundoff(storage) * ref.abs()).clamp_min(half_sub)


def _rnd(t: torch.Tensor, storage) -> torch.Tensor:
    return t if storage is None else t.to(storage).to(t.dtype)


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(t.dtype)


def _conv(x, w, e):
    return F.conv2d(x, w, None, stride=e["stride"], padding=e["ks"] // 2)


def _weights(params, storage, dtype=torch.float64):
    return [_rnd(params[e["conv"] + ".weight"].detach().to(torch.float64), storage).to(dtype) for e in CONVS]


def _bn_params(params, i, dtype=torch.float64):
    e = CONVS[i]
    return params[e["bn"] + ".weight"].detach().to(dtype).view(1, -1, 1, 1), params[e["bn"] + ".bias"].detach().to(dtype).view(1, -1, 1, 1)


def batch_stats(pre: torch.Tensor):
    """float64 (mean, biased variance) per channel of a [B,C,H,W] map."""
    mean = pre.mean(dim=(0, 2, 3))
    var = ((pre - mean.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
    return mean, var


def _eps(storage) -> float:
    return BN_EPS if storage is None else float(torch.tensor(BN_EPS, dtype=torch.float32))  # the C ABI takes a float


def _bn_apply(pre, mean, rstd, gamma, beta, resid, relu):
    y = (pre - mean.view(1, -1, 1, 1)) * rstd.view(1, -1, 1, 1) * gamma + beta
    if resid is not None:
        y = y + resid
    return y.clamp_min(0) if relu else y


def pool_windows(post0: torch.Tensor) -> torch.Tensor:
    """[B,C,112,112] -> [B,C,9,56,56]: the 3x3 / stride 2 / pad 1 windows in (dy, dx) scan order, -inf outside."""
    B, C_, H, W = post0.shape
    p = F.pad(post0, (1, 1, 1, 1), value=float("-inf"))
    return F.unfold(p, kernel_size=3, stride=2).view(B, C_, 9, H // 2, W // 2)


def pool_first_max(post0: torch.Tensor):
    """(pooled map, uint8 code dy * 3 + dx of the FIRST maximum of every window in scan order)."""
    win = pool_windows(post0)
    mx = win.max(dim=2).values
    pos = torch.arange(9).view(1, 1, 9, 1, 1)
    code = torch.where(win == mx.unsqueeze(2), pos, torch.full_like(pos, 9)).min(dim=2).values
    return mx, code.to(torch.uint8)


def _resid_and_relu(i: int):
    """(index of the conv whose post map / -1 for the block input is added before the ReLU, or None; relu) of BN i."""
    for c1, c2, ds, prev in BLOCKS:
        if i == c1:
            return None, True
        if i == c2:
            return ("ds", ds) if ds >= 0 else ("in", prev), True
        if i == ds:
            return None, False
    return None, True  # the stem


def _block_input(maps, prev):
    return maps["pool"] if prev < 0 else maps[("post", prev)]


def emulate_forward(x: torch.Tensor, params: Dict[str, torch.Tensor], storage, running: Optional[Dict[str, torch.Tensor]] = None) -> dict:
    """The train-mode forward of train_encoder_forward with the device's roundings.  Returns float64 NCHW maps keyed like
    the device taps: ("pre", i), ("post", i), "pool", "pool_idx" (uint8), ("stats", i) = (mean, rstd) -- float32 values
    (float64 for storage None) -- plus "x" (the rounded input), "feats" [B,512] and, when ``running`` (torchvision-named running statistics) is given,
    ("running", i) = (running_mean, running_var) after the step."""
    w = _weights(params, storage)
    xin = _rnd(x.detach().to(torch.float64), storage)
    maps: dict = {"x": xin}

    def conv_bn(i, inp, resid, relu):
        pre = _rnd(_conv(inp, w[i], CONVS[i]), storage)
        mean, var = batch_stats(pre)
        rstd = 1.0 / torch.sqrt(var + _eps(storage))
        if running is not None:
            maps[("running", i)] = _running_update(running, i, mean, var, pre, storage)
        if storage is not None:
            mean, rstd = _f32(mean), _f32(rstd)
        gamma, beta = _bn_params(params, i)
        maps[("pre", i)], maps[("stats", i)] = pre, (mean, rstd)
        maps[("post", i)] = _rnd(_bn_apply(pre, mean, rstd, gamma, beta, resid, relu), storage)
        return maps[("post", i)]

    y = conv_bn(0, xin, None, True)
    maps["pool"], maps["pool_idx"] = pool_first_max(y)
    cur = maps["pool"]
    for c1, c2, ds, _ in BLOCKS:
        t = conv_bn(c1, cur, None, True)
        idt = conv_bn(ds, cur, None, False) if ds >= 0 else cur
        cur = conv_bn(c2, t, idt, True)
    f = cur.mean(dim=(2, 3))
    maps["feats"] = f if storage is None else _f32(f)
    return maps


def _running_update(running, i, mean, var, pre, storage):
    e = CONVS[i]
    M = pre.numel() // pre.shape[1]
    unb = var * M / (M - 1) if M > 1 else var
    rm = running[e["bn"] + ".running_mean"].detach().to(torch.float64)
    rv = running[e["bn"] + ".running_var"].detach().to(torch.float64)
    mom = BN_MOMENTUM if storage is None else float(torch.tensor(BN_MOMENTUM, dtype=torch.float32))  # the C ABI takes a float
    return (1.0 - mom) * rm + mom * mean, (1.0 - mom) * rv + mom * unb


def _ratio(err: torch.Tensor, bound: torch.Tensor) -> float:
    """worst |err| / bound; an element with bound 0 must have error 0."""
    err, bound = err.abs(), bound.abs()
    zero = bound == 0
    if bool((err[zero] > 0).any()):
        return float("inf")
    r = err[~zero] / bound[~zero]
    return float(r.max()) if r.numel() else 0.0


def check_forward_stages(maps: dict, x: torch.Tensor, params: Dict[str, torch.Tensor], storage,
                         running: Optional[Dict[str, torch.Tensor]] = None) -> Dict[object, float]:
    """Every forward stage recomputed in float64 from the stage's GIVEN input maps; returns the worst
    |given - ref| / bound per stage, no element left out (e = 2^-24; u |ref| = ``rounding_bound``: the unit roundoff of the
    maps times |ref|, with the format's subnormal floor):
      ("conv", i)     u |ref| + K e S, K = cin ks^2, S = the same convolution of |x| and |w| (the worst case of an fp32
                      sum of K products in any order)
      ("stats", i)    mean: 2^-23 |ref| + 1e-12 rms(x); rstd: 2^-23 |ref| -- from the given pre[i]
      ("running", i)  2^-23 of the updated value (momentum 0.1, unbiased variance); only when ``running`` (the statistics
                      BEFORE the step) is given and the maps hold ("running", i)
      ("bn", i)       u |ref| + 8 e (|xhat gamma| + |beta| + |resid|), from the given pre, mean / rstd and residual map
      "pool"          the given pooled map against the window maxima of the given post[0]: 0 if bit-equal, else 1 + the
                      number of differing elements;  "pool_idx" likewise against the first maximum in scan order
      "feats"         50 e mean|v| against the float64 mean of the given last map"""
    out: Dict[object, float] = {}
    w = _weights(params, storage)
    xin = _rnd(x.detach().to(torch.float64), storage)

    def src(i):
        if i == 0:
            return xin
        for c1, c2, ds, prev in BLOCKS:
            if i == c1 or i == ds:
                return _block_input(maps, prev).to(torch.float64)
            if i == c2:
                return maps[("post", c1)].to(torch.float64)
        raise KeyError(i)

    for i, e in enumerate(CONVS):
        inp, pre = src(i), maps[("pre", i)].to(torch.float64)
        ref = _conv(inp, w[i], e)
        S = _conv(inp.abs(), w[i].abs(), e)
        K = e["cin"] * e["ks"] ** 2
        out[("conv", i)] = _ratio(pre - ref, rounding_bound(ref, storage) + K * EPS32 * S)
        # statistics of the given pre map
        mean, var = batch_stats(pre)
        rstd = 1.0 / torch.sqrt(var + _eps(storage))
        g_mean, g_rstd = (t.to(torch.float64) for t in maps[("stats", i)])
        rms = torch.sqrt((pre ** 2).mean(dim=(0, 2, 3)))
        out[("stats", i)] = max(_ratio(g_mean - mean, 2.0 ** -23 * mean.abs() + 1e-12 * rms), _ratio(g_rstd - rstd, 2.0 ** -23 * rstd.abs()))
        if running is not None and ("running", i) in maps:
            rm, rv = _running_update(running, i, mean, var, pre, storage)
            g_rm, g_rv = (t.to(torch.float64) for t in maps[("running", i)])
            out[("running", i)] = max(_ratio(g_rm - rm, 2.0 ** -23 * rm.abs()), _ratio(g_rv - rv, 2.0 ** -23 * rv.abs()))
        # normalisation from the given statistics
        gamma, beta = _bn_params(params, i)
        rs, relu = _resid_and_relu(i)
        resid = None if rs is None else (maps[("post", rs[1])] if rs[0] == "ds" else _block_input(maps, rs[1])).to(torch.float64)
        ref = _bn_apply(pre, g_mean, g_rstd, gamma, beta, resid, relu)
        xg = ((pre - g_mean.view(1, -1, 1, 1)) * g_rstd.view(1, -1, 1, 1) * gamma).abs()
        bound = rounding_bound(ref, storage) + 8 * EPS32 * (xg + beta.abs() + (0 if resid is None else resid.abs()))
        out[("bn", i)] = _ratio(maps[("post", i)].to(torch.float64) - ref, bound)
    mx, code = pool_first_max(maps[("post", 0)].to(torch.float64))
    n = int((maps["pool"].to(torch.float64) != mx).sum())
    out["pool"] = 0.0 if n == 0 else 1.0 + n
    n = int((maps["pool_idx"] != code).sum())
    out["pool_idx"] = 0.0 if n == 0 else 1.0 + n
    last = maps[("post", 19)].to(torch.float64)
    out["feats"] = _ratio(maps["feats"].to(torch.float64) - last.mean(dim=(2, 3)), 50 * EPS32 * last.abs().mean(dim=(2, 3)))
    return out


def replay_backward(maps: dict, params: Dict[str, torch.Tensor], dfeats: torch.Tensor, storage, accum_dtype=torch.float64,
                    grad_maps: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """train_encoder_backward stage by stage on the given forward maps: dfeats [B,512] -> gradients under torchvision
    names (``accum_dtype`` tensors), like ``NativeEncoder.state_dict(grads=True)``.  ``maps["x"]`` is the step's input
    (rounded to storage here, as the device's NHWC4 copy is).  ``accum_dtype=torch.float32`` runs the same stages
    with float32 convolutions and sums.  ``grad_maps`` (optional dict) receives every rounded gradient map under a
    readable key."""
    A = accum_dtype
    grads: Dict[str, torch.Tensor] = {}
    w = _weights(params, storage, A)

    def m(key):
        return maps[key].to(A)

    def rnd(t):
        return _rnd(t, storage)

    def keep(key, t):
        if grad_maps is not None:
            grad_maps[key] = t
        return t

    def bn_bwd(i, dy, mask):
        e = CONVS[i]
        pre = m(("pre", i))
        mean, rstd = (t.to(A).view(1, -1, 1, 1) for t in maps[("stats", i)])
        gamma, _ = _bn_params(params, i, A)
        if mask is not None:
            dy = torch.where(mask > 0, dy, torch.zeros_like(dy))
        xhat = (pre - mean) * rstd
        M = pre.numel() // pre.shape[1]
        s, q = dy.sum(dim=(0, 2, 3)), (dy * xhat).sum(dim=(0, 2, 3))
        grads[e["bn"] + ".weight"], grads[e["bn"] + ".bias"] = q, s
        dx = gamma * rstd * (dy - s.view(1, -1, 1, 1) / M - xhat * q.view(1, -1, 1, 1) / M)
        return keep(f"bn{i}.dx", rnd(dx))

    def wgrad(i, inp, dy):
        e = CONVS[i]
        grads[e["conv"] + ".weight"] = torch.nn.grad.conv2d_weight(inp, w[i].shape, dy, stride=e["stride"], padding=e["ks"] // 2)

    def dgrad(i, dy):
        e = CONVS[i]
        B = dy.shape[0]
        dx = torch.nn.grad.conv2d_input((B, e["cin"], e["hin"], e["hin"]), w[i], dy, stride=e["stride"], padding=e["ks"] // 2)
        return keep(f"conv{i}.dx", rnd(dx))

    last = m(("post", 19))
    if storage is None:
        g = dfeats.detach().to(A) / 49.0
    else:  # the device multiplies in fp32 by the fp32 constant 1 / 49, then rounds to the map type
        g = (dfeats.detach().to(torch.float32) * torch.tensor(1.0 / 49.0, dtype=torch.float32)).to(A)
    gA = keep("avgpool.dx", rnd(torch.where(last > 0, g.view(g.shape[0], -1, 1, 1).expand_as(last), torch.zeros_like(last))))
    for c1, c2, ds, prev in reversed(BLOCKS):
        xin_blk = m("pool") if prev < 0 else m(("post", prev))
        gB = bn_bwd(c2, gA, None)
        wgrad(c2, m(("post", c1)), gB)
        gC = dgrad(c2, gB)
        gC = bn_bwd(c1, gC, m(("post", c1)))
        wgrad(c1, xin_blk, gC)
        gB = dgrad(c1, gC)
        if ds >= 0:
            gC = bn_bwd(ds, gA, None)
            wgrad(ds, xin_blk, gC)
            side = dgrad(ds, gC)
        else:
            side = gA
        tot = gB + side
        if prev >= 0:
            tot = torch.where(xin_blk > 0, tot, torch.zeros_like(tot))
        gA = keep(f"block{c1}.dx", rnd(tot))
    # max-pool backward by the arg-max bytes: window (oh, ow) sends its gradient to input (2 oh - 1 + dy, 2 ow - 1 + dx)
    idx = maps["pool_idx"].long()
    B, C_, HO, WO = gA.shape
    oy, ox = torch.arange(HO).view(1, 1, HO, 1), torch.arange(WO).view(1, 1, 1, WO)
    flat = ((2 * oy - 1 + idx // 3) * 112 + (2 * ox - 1 + idx % 3)).view(B, C_, -1)
    din = torch.zeros((B, C_, 112 * 112), dtype=A)
    din.scatter_add_(2, flat, gA.reshape(B, C_, -1))
    gB = keep("maxpool.dx", rnd(din.view(B, C_, 112, 112)))
    gB = bn_bwd(0, gB, m(("post", 0)))
    wgrad(0, _rnd(maps["x"].detach().to(torch.float64), storage).to(A), gB)
    return grads


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    """max|a - b| / max|b| in float64."""
    a, b = a.detach().to(torch.float64), b.detach().to(torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
